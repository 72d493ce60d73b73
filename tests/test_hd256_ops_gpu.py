"""Op-level GPU parity at head_dim 256 (-m gpu): the decode kernel
k_attn_decode_256<GB>, the MFMA-256 and the plain prefill kernels, and the
hd-generic stores and linear kernels at Falcon3's shapes, against the float64
references of tests/attn_ref.py and tests/linear_ref.py.

Bounds, input families and the stale-slot rule are those of
test_attn_ops_gpu.py: |got - ref| <= tol * A + 2^-40 element-wise with
A = P.|V|; tol = 2^-7 where P stays f32 (decode, plain prefill), 2^-6 where it
is rounded to bf16 (MFMA prefill).  tests/test_hd256_ref.py proves on the CPU
that these very inputs have teeth.  Every decode case runs on the grouped
route (CAKE_ATTN256_GB=4: GB = the largest of 4, 3, 2, 1 dividing G) and on
the default one, GB 1 (the grouped route measured slower and is opt-in).

Run with -s for launch counts and the worst err / (tol * A) per kernel."""
import collections
import contextlib
import os

import numpy as np
import pytest

import cake_amd
from tests import attn_cases as ac
from tests import hd256_cases as hc
from tests import linear_cases as lc
from tests import test_attn_ops_gpu as ta
from tests import test_linear_ops_gpu as tl
from tests.attn_ref import attn_ref, kv_store_ref

pytestmark = pytest.mark.gpu

LAUNCHES = collections.Counter()
WORST = collections.defaultdict(float)
_bits = ta._bits


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nhd-256 op tests: kernel launches and worst err/(tol*A)")
    for k in sorted(LAUNCHES):
        print(f"  {k:34s} launches {LAUNCHES[k]:5d}  worst {WORST[k]:.3f}")


@contextlib.contextmanager
def _gb_cap(cap):
    """CAKE_ATTN256_GB for the calls inside (the library reads it per
    launch); None = unset."""
    old = os.environ.pop("CAKE_ATTN256_GB", None)
    if cap is not None:
        os.environ["CAKE_ATTN256_GB"] = str(cap)
    try:
        yield
    finally:
        os.environ.pop("CAKE_ATTN256_GB", None)
        if old is not None:
            os.environ["CAKE_ATTN256_GB"] = old


def _check(kernel, fam, got, ref, A, tol, fails):
    ratio = np.abs(got - ref) / (tol * A + ac.ABS_EPS)
    worst = np.inf if np.isnan(got).any() else float(np.max(ratio))
    WORST[kernel] = max(WORST[kernel], worst)
    if not worst <= 1.0:
        i = np.unravel_index(np.nanargmax(ratio), ratio.shape)
        fails.append(f"{kernel} {fam}: err/(tol*A) = {worst:.3f} at {i} "
                     f"(got {got[i]:.6g}, ref {ref[i]:.6g})")


# ---- decode ------------------------------------------------------------------
@pytest.mark.parametrize("case", hc.DEC_CASES,
                         ids=lambda x: "-".join(map(str, x)))
def test_decode_256(case):
    nh, nkv, hd, n, nchunk, window = case
    with _gb_cap(4):
        gb = cake_amd.attn_decode_group(nh, nkv, hd)
        assert gb == hc.GROUP_OF_G[nh // nkv]
        assert cake_amd.attn_decode_path(nh, nkv, hd, nchunk) == 3
        gy = cake_amd.attn_dispatch(1, nh, nkv, hd)["decode_grid_y"]
        assert gy == nh // gb and nchunk * nh <= 512
    pos, max_seq = n - 1, ac.decode_max_seq(n)
    lo = n - window if (window and n > window) else 0
    tail = " direct" if nchunk == 1 else " combine"
    fails = []
    for fam in ac.FAMILIES:
        q, kc, vc = ac.make_inputs(fam, nh, nkv, hd, max_seq, 1, pos, window,
                                   decode=True)
        ref, A = attn_ref(q, kc, vc, pos, window)
        outs = []
        with _gb_cap(4):
            for fill in (0, ac.STALE):
                k, v, _ = ac.set_stale(kc, vc, lo, n, fill)
                outs.append(cake_amd.op_attn_decode(q[0], k, v, pos, window,
                                                    nchunk, repeats=3))
                LAUNCHES[f"decode 256 GB{gb}{tail}"] += 3
        if not np.array_equal(_bits(outs[0]), _bits(outs[1])):
            fails.append(f"{fam}: output depends on stale slots outside "
                         f"[{lo},{n})")
        for r in (1, 2):
            if not np.array_equal(_bits(outs[0][0]), _bits(outs[0][r])):
                fails.append(f"{fam}: repeat {r} differs from repeat 0 on "
                             "counters zeroed once")
        for r in range(3):
            _check(f"decode 256 GB{gb}{tail}", f"{fam}/repeat{r}",
                   outs[0][r:r + 1], ref, A, ac.TOL_F32P, fails)
        # the per-head route of the same kernel (the default), same bound
        with _gb_cap(None):
            assert cake_amd.attn_decode_group(nh, nkv, hd) == 1
            k, v, _ = ac.set_stale(kc, vc, lo, n, ac.STALE)
            one = cake_amd.op_attn_decode(q[0], k, v, pos, window, nchunk)
            LAUNCHES[f"decode 256 GB1 default{tail}"] += 1
        _check(f"decode 256 GB1 default{tail}", fam, one, ref, A, ac.TOL_F32P,
               fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("geom", [(3, 1), (8, 4), (5, 1)],
                         ids=lambda g: f"nh{g[0]}kv{g[1]}")
@pytest.mark.parametrize("cap", [None, 4], ids=["per-head", "grouped"])
@pytest.mark.parametrize("seq", hc.DEC_SEQS, ids=lambda s: "-".join(map(str, s)))
def test_decode_256_changing_nchunk(geom, seq, cap):
    """Launches with changing chunk counts share one set of counters: every
    launch is right, and the elected blocks leave every word at zero."""
    nh, nkv = geom
    n, window = 300, 0
    q, kc, vc = ac.make_inputs("peaky", nh, nkv, hc.HD, 320, 1, n - 1, window,
                               decode=True)
    ref, A = attn_ref(q, kc, vc, n - 1, window)
    with _gb_cap(cap):
        out, cnt = cake_amd.op_attn_decode_seq(q[0], kc, vc, n - 1, list(seq),
                                               window)
    LAUNCHES["decode 256 seq"] += len(seq)
    fails = []
    for i in range(len(seq)):
        _check("decode 256 seq", f"launch {i} (nchunk {seq[i]})",
               out[i:i + 1], ref, A, ac.TOL_F32P, fails)
    assert not fails, "\n".join(fails)
    assert not np.asarray(cnt).any(), cnt


# ---- prefill -----------------------------------------------------------------
@pytest.mark.parametrize("case", hc.PF_CASES,
                         ids=lambda x: "-".join(map(str, x)))
def test_prefill_256(case):
    nh, nkv, S, pos0, window, max_seq = case
    fails = []
    for fam in ac.FAMILIES:
        q, kc, vc = ac.make_inputs(fam, nh, nkv, hc.HD, max_seq, S, pos0,
                                   window)
        ref, A = attn_ref(q, kc, vc, pos0, window)
        for name, variant, tol in (
                ("prefill mfma 256", hc.PF_MFMA, ac.TOL_MFMA),
                ("prefill plain 256", hc.PF_PLAIN, ac.TOL_F32P)):
            outs = []
            for fill in (0, ac.STALE):
                k, v, vt = ac.set_stale(kc, vc, 0, pos0 + S, fill)
                outs.append(cake_amd.op_attn_prefill(q, k, v, vt, pos0, window,
                                                     variant))
                LAUNCHES[name] += 1
            if not np.array_equal(_bits(outs[0]), _bits(outs[1])):
                fails.append(f"{name} {fam}: output depends on stale slots "
                             f">= {pos0 + S}")
            _check(name, fam, outs[0], ref, A, tol, fails)
    assert not fails, "\n".join(fails)


def test_prefill_256_default_variant_is_the_engines():
    nh, nkv, S, pos0, window, max_seq = hc.PF_CASES[0]
    d = cake_amd.attn_dispatch(S, nh, nkv, hc.HD)
    assert (d["pfv"], d["nw"], d["split"], d["deep"]) == hc.PF_MFMA
    q, kc, vc = ac.make_inputs("peaky", nh, nkv, hc.HD, max_seq, S, pos0,
                               window)
    vt = np.ascontiguousarray(vc.transpose(0, 2, 1))
    a = cake_amd.op_attn_prefill(q, kc, vc, vt, pos0, window)
    b = cake_amd.op_attn_prefill(q, kc, vc, vt, pos0, window, hc.PF_MFMA)
    assert np.array_equal(_bits(a), _bits(b))
    # the hd-128 variants are not dispatchable here
    with pytest.raises(cake_amd.CakeHipError, match="not dispatchable"):
        cake_amd.op_attn_prefill(q, kc, vc, vt, pos0, window, (2, 8, 0, 0))


# ---- rope + KV store -----------------------------------------------------------
def _run_store(nh, nkv, hd, S, pos0, norm, decode):
    max_seq, eps = hc.STORE_MAX_SEQ, 1e-6
    qkv, cos, sin, kc, vc, vtc, qn, kn = ta._store_inputs(
        nh, nkv, hd, max_seq, S, norm, nh * 1000 + S * 10 + pos0 + norm)
    gq, gk, gv, gvt = cake_amd.op_kv_store(
        qkv, cos, sin, kc, vc, vtc, pos0, nh, nkv, qn, kn, eps, decode)
    kernel = "rope_store 256 " + ("decode" if decode else "prefill")
    LAUNCHES[kernel] += 1
    rq, rk, rv, rvt, qtol, ktol = kv_store_ref(
        qkv, cos, sin, pos0, nh, nkv, kc, vc, vtc, qn, kn, eps)
    rows = slice(pos0, pos0 + S)
    WORST[kernel] = max(WORST[kernel], np.max(np.abs(gq - rq) / qtol),
                        np.max(np.abs(gk - rk)[:, rows] / ktol[:, rows]))
    assert (np.abs(gq - rq) <= qtol).all()
    assert (np.abs(gk[:, rows] - rk[:, rows]) <= ktol[:, rows]).all()
    assert np.array_equal(_bits(gv[:, rows]), _bits(rv[:, rows]))
    assert np.array_equal(_bits(gvt[:, :, rows]),
                          _bits(gv[:, rows].transpose(0, 2, 1)))
    out = np.ones(max_seq, dtype=bool)
    out[rows] = False
    assert np.array_equal(_bits(gk[:, out]), _bits(kc[:, out]))
    assert np.array_equal(_bits(gv[:, out]), _bits(vc[:, out]))
    assert np.array_equal(_bits(gvt[:, :, out]), _bits(vtc[:, :, out]))


@pytest.mark.parametrize("norm", [False, True], ids=["plain", "qknorm"])
@pytest.mark.parametrize("S,pos0", hc.STORE_PREFILL)
@pytest.mark.parametrize("geom", hc.STORE_GEOM,
                         ids=lambda g: "-".join(map(str, g)))
def test_kv_store_prefill_256(geom, S, pos0, norm):
    _run_store(*geom, S, pos0, norm, decode=False)


@pytest.mark.parametrize("norm", [False, True], ids=["plain", "qknorm"])
@pytest.mark.parametrize("pos", hc.STORE_DECODE_POS)
@pytest.mark.parametrize("geom", hc.STORE_GEOM,
                         ids=lambda g: "-".join(map(str, g)))
def test_kv_store_decode_256(geom, pos, norm):
    _run_store(*geom, 1, pos, norm, decode=True)


# ---- linear kernels at Falcon3's shapes -------------------------------------
@pytest.mark.parametrize("case", hc.rope_cases(),
                         ids=lambda c: "-".join(map(str, c)))
def test_qkv_rope_256(case):
    tl.test_qkv_rope(case)      # same inputs, references and bounds


@pytest.mark.parametrize("K", hc.NEW_GEMV_K)
def test_gemv_bf16_new_k(K):
    tl._run_gemv("bf16", K, 4, lc.gemv_n(4), lc.gemv_norm_modes("bf16", K))


def test_gateup_bf16_new_k():
    # gate-up's K is the hidden size (<= 16384 by contract): 9216 runs, 23040
    # is only ever a down-projection K
    tl._run_gateup(False, hc.NEW_GEMV_K[0], 4, lc.gateup_i(False, 4))
