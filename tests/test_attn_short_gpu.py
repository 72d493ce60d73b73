"""The short-context decode-attention kernel (k_attn_decode_short: all chunks
of a q head in one workgroup, split-KV combine through LDS) against the
grouped kernel it replaces at nchunk 4 and 8, and against the float64
reference (-m gpu).

The kernel's arithmetic is the grouped kernel's operation for operation, so
the two outputs must be BIT-identical at the same (n, nchunk, window); the
grouped path is reached in the same process with CAKE_ATTN_SHORT=0, which
the library reads on every launch.  attn_decode_path() proves which kernel a
launch takes.

Routing: the short kernel is the default at nchunk 4.  At nchunk 8 it measured
no faster than the grouped kernel (profiles/short_attn_NOTES.md), so the
product keeps the grouped kernel there and the short one runs only under
CAKE_ATTN_SHORT=2; its nchunk-8 cases are tested under that setting."""
import numpy as np
import pytest

import cake_amd
from tests import attn_cases as ac
from tests.attn_ref import attn_ref

pytestmark = pytest.mark.gpu

CONFIGS = [(4, 1), (8, 1), (8, 2)]
NCHUNKS = (4, 8)
NS = (1, 2, 63, 64, 65, 128, 129, 255, 256, 257, 300, 511, 512, 600)
WINDOWS = ac.DEC_WINDOWS
MAX_SEQ = 640
HD = 128


def _cases():
    """Pruned like attn_cases._decode_cases: every n with every nchunk for
    every config, the window cycling with config- and nchunk-dependent
    offsets in two passes, so every (n, nchunk) and every (window, nchunk)
    pair appears for every config."""
    out = []
    for g, cfg in enumerate(CONFIGS):
        for k, nc in enumerate(NCHUNKS):
            seen = set()
            trip = [(n, nc, WINDOWS[(i + 2 * g + k) % 6])
                    for i, n in enumerate(NS)]
            trip += [(NS[(2 * i + g) % len(NS)], nc,
                      WINDOWS[(i + g + k + 3) % 6]) for i in range(7)]
            # several tiles per chunk, full context
            trip += [(300, nc, 0), (600, nc, 0), (257, nc, 0)]
            for t in trip:
                if t not in seen:
                    seen.add(t)
                    out.append(cfg + t)
    return out


CASES = _cases()


def _short_on(monkeypatch, nchunk):
    """The setting under which the short kernel takes this chunk count: the
    default at 4, CAKE_ATTN_SHORT=2 at 8."""
    if nchunk == 4:
        monkeypatch.delenv("CAKE_ATTN_SHORT", raising=False)
    else:
        monkeypatch.setenv("CAKE_ATTN_SHORT", "2")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _within(fam, got, ref, A, fails):
    ratio = np.abs(got - ref) / (ac.TOL_F32P * A + ac.ABS_EPS)
    worst = np.inf if np.isnan(got).any() else float(np.max(ratio))
    if not worst <= 1.0:
        fails.append(f"{fam}: err/(tol*A) = {worst:.3f}")


@pytest.mark.parametrize("case", CASES, ids=lambda x: "-".join(map(str, x)))
def test_short_vs_grouped(case, monkeypatch):
    nh, nkv, n, nchunk, window = case
    pos = n - 1
    lo = n - window if (window and n > window) else 0
    fails = []
    for fam in ac.FAMILIES:
        q, kc, vc = ac.make_inputs(fam, nh, nkv, HD, MAX_SEQ, 1, pos, window,
                                   decode=True)
        ref, A = attn_ref(q, kc, vc, pos, window)
        _short_on(monkeypatch, nchunk)
        assert cake_amd.attn_decode_path(nh, nkv, HD, nchunk) == 2
        new = []
        for fill in (0, ac.STALE):
            k, v, _ = ac.set_stale(kc, vc, lo, n, fill)
            new.append(cake_amd.op_attn_decode(q[0], k, v, pos, window,
                                               nchunk, repeats=3))
        monkeypatch.setenv("CAKE_ATTN_SHORT", "0")
        assert cake_amd.attn_decode_path(nh, nkv, HD, nchunk) == 1
        k0, v0, _ = ac.set_stale(kc, vc, lo, n, 0)
        old = cake_amd.op_attn_decode(q[0], k0, v0, pos, window, nchunk,
                                      repeats=1)
        if not np.array_equal(_bits(new[0][0]), _bits(old[0])):
            fails.append(f"{fam}: short != grouped in "
                         f"{(_bits(new[0][0]) != _bits(old[0])).sum()} elements")
        if not np.array_equal(_bits(new[0]), _bits(new[1])):
            fails.append(f"{fam}: output depends on stale slots outside "
                         f"[{lo},{n})")
        for r in (1, 2):
            if not np.array_equal(_bits(new[0][0]), _bits(new[0][r])):
                fails.append(f"{fam}: repeat {r} differs from repeat 0")
        _within(fam, new[0][0:1], ref, A, fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("nh,nkv", CONFIGS)
def test_alternating_short_and_grouped(nh, nkv, monkeypatch):
    """Short (nchunk 4, 8) and grouped (nchunk 16) launches interleaved on one
    set of buffers: every launch is right, and only the grouped launches
    move the arrival counters (each adds nchunk to each of its grid_y
    counters)."""
    monkeypatch.setenv("CAKE_ATTN_SHORT", "2")
    n, window = 300, 0
    gy = cake_amd.attn_dispatch(1, nh, nkv, HD)["decode_grid_y"]
    seq = [4, 16, 4, 16, 8, 16, 8]
    assert [cake_amd.attn_decode_path(nh, nkv, HD, c) for c in seq] == \
        [2, 1, 2, 1, 2, 1, 2]
    fails = []
    for fam in ac.FAMILIES:
        q, kc, vc = ac.make_inputs(fam, nh, nkv, HD, MAX_SEQ, 1, n - 1,
                                   window, decode=True)
        ref, A = attn_ref(q, kc, vc, n - 1, window)
        k, v, _ = ac.set_stale(kc, vc, 0, n, ac.STALE)
        out, cnt = cake_amd.op_attn_decode_seq(q[0], k, v, n - 1, seq, window)
        for i in range(len(seq)):
            _within(f"{fam}/launch{i}", out[i:i + 1], ref, A, fails)
        for a, b in ((0, 2), (1, 3), (1, 5), (4, 6)):
            if not np.array_equal(_bits(out[a]), _bits(out[b])):
                fails.append(f"{fam}: launches {a} and {b} differ")
        want = np.zeros(nh, dtype=np.uint32)
        want[:gy] = 16 * seq.count(16)
        if not np.array_equal(cnt, want):
            fails.append(f"{fam}: counters {cnt.tolist()} != {want.tolist()}")
        out, cnt = cake_amd.op_attn_decode_seq(q[0], k, v, n - 1, [4, 8, 4],
                                               window)
        if cnt.any():
            fails.append(f"{fam}: short launches moved the counters: "
                         f"{cnt.tolist()}")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("nh,nkv", CONFIGS)
def test_routing(nh, nkv, monkeypatch):
    """knob unset: short at nchunk 4 only; 0: grouped everywhere; 2: short at
    4 and 8; other chunk counts and G % 4 != 0 never take the short kernel."""
    path = lambda c: cake_amd.attn_decode_path(nh, nkv, HD, c)
    monkeypatch.delenv("CAKE_ATTN_SHORT", raising=False)
    assert [path(c) for c in (1, 2, 4, 8, 12, 16)] == [1, 1, 2, 1, 1, 1]
    monkeypatch.setenv("CAKE_ATTN_SHORT", "0")
    assert [path(c) for c in (4, 8)] == [1, 1]
    monkeypatch.setenv("CAKE_ATTN_SHORT", "2")
    assert [path(c) for c in (1, 2, 4, 8, 12, 16)] == [1, 1, 2, 2, 1, 1]
    assert cake_amd.attn_decode_path(2, 1, HD, 4) == 1
    assert cake_amd.attn_decode_path(6, 2, HD, 4) == 0
