"""Op-level GPU parity (-m gpu) of the grouped MFMA decode-attention kernel
(k_attn_decode_mq, kernels_attn_mq.hip; CAKE_ATTN_MQ=1) against the float64
reference of tests/attn_ref.py, on the inputs, families and bound of
tests/attn_cases.py: |got - ref| <= TOL_F32P * A + ABS_EPS element-wise.  The
bound's derivation holds here because P enters the P.V MFMAs as bf16 hi + bf16
lo, below 2^-16 relative, and the scores accumulate bf16 products in f32."""
import numpy as np
import pytest

import cake_amd
from tests import attn_cases as ac
from tests.attn_ref import attn_ref

pytestmark = pytest.mark.gpu

# G = 3, 5, 6 (two kv heads), 7, 7 and 4 at hd 64, 16 (no padding rows), 1
GEOMS = [(3, 1, 128), (5, 1, 128), (6, 2, 128), (7, 1, 128), (14, 2, 64),
         (8, 2, 64), (16, 1, 128), (1, 1, 64)]
NS = (1, 2, 31, 32, 33, 64, 65, 129, 300, 2100)
NCHUNKS = (1, 4, 8, 24, 64)
WINDOWS = (0, 1, 33, 64, 96)
# pruned cross: every n, nchunk and window appears (three cyclic picks per
# geometry), then the corners: more chunks than positions, several 128-position
# steps per wave with and without split, a windowed span cut into 64 chunks
CASES = [g + (NS[(3 * gi + i) % 10], NCHUNKS[(gi + i) % 5],
              WINDOWS[(2 * gi + i) % 5])
         for gi, g in enumerate(GEOMS) for i in range(3)] + [
    (7, 1, 128, 1, 64, 0), (14, 2, 64, 2, 64, 0), (7, 1, 128, 2100, 1, 0),
    (14, 2, 64, 2100, 4, 0), (6, 2, 128, 2100, 64, 96), (3, 1, 128, 300, 4, 0)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _bound_fails(tag, got, ref, A):
    ratio = np.abs(got - ref) / (ac.TOL_F32P * A + ac.ABS_EPS)
    worst = np.inf if np.isnan(ratio).any() else float(ratio.max())
    return [] if worst <= 1.0 else [f"{tag}: err/(tol*A) = {worst:.3f}"]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_decode_mq(case, monkeypatch):
    nh, nkv, hd, n, nchunk, window = case
    monkeypatch.setenv("CAKE_ATTN_MQ", "1")
    assert cake_amd.attn_decode_path(nh, nkv, hd, nchunk) == 4
    assert cake_amd.attn_decode_group(nh, nkv, hd) == nh // nkv
    pos, max_seq = n - 1, ac.decode_max_seq(n)
    lo = n - window if (window and n > window) else 0
    fails = []
    for fam in ac.FAMILIES:
        q, kc, vc = ac.make_inputs(fam, nh, nkv, hd, max_seq, 1, pos, window,
                                   decode=True)
        ref, A = attn_ref(q, kc, vc, pos, window)
        outs = []
        for fill in (0, ac.STALE):
            k, v, _ = ac.set_stale(kc, vc, lo, n, fill)
            outs.append(cake_amd.op_attn_decode(q[0], k, v, pos, window,
                                                nchunk, repeats=3))
        if not np.array_equal(_bits(outs[0]), _bits(outs[1])):
            fails.append(f"{fam}: output depends on slots outside [{lo},{n})")
        for r in (1, 2):
            if not np.array_equal(_bits(outs[0][0]), _bits(outs[0][r])):
                fails.append(f"{fam}: repeat {r} differs from repeat 0")
        fails += _bound_fails(fam, outs[0][0:1], ref, A)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("geom", [(7, 1, 128), (14, 2, 64)],
                         ids=lambda g: "-".join(map(str, g)))
def test_decode_mq_changing_nchunk(geom, monkeypatch):
    """The kernel's counter contract: the election is modulo nchunk and the
    elected block stores 0 to its word, so launches with changing chunk counts
    share one zeroing: every launch is right and every word ends at zero."""
    nh, nkv, hd = geom
    monkeypatch.setenv("CAKE_ATTN_MQ", "1")
    n, seq = 300, [4, 8, 24, 8, 64, 1, 4]
    q, kc, vc = ac.make_inputs("peaky", nh, nkv, hd, 320, 1, n - 1, 0,
                               decode=True)
    ref, A = attn_ref(q, kc, vc, n - 1, 0)
    out, cnt = cake_amd.op_attn_decode_seq(q[0], kc, vc, n - 1, seq, 0)
    fails = []
    for i, c in enumerate(seq):
        fails += _bound_fails(f"launch {i} (nchunk {c})", out[i:i + 1], ref, A)
    assert not fails, "\n".join(fails)
    assert np.array_equal(_bits(out[0]), _bits(out[6]))
    assert not np.asarray(cnt).any(), cnt
