"""Op-level GPU parity of the attention kernels and the rope + KV-store step
against the float64 references in tests/attn_ref.py (-m gpu).

Every attention assertion is element-wise, |got - ref| <= tol * A + 2^-40 with
A = P.|V| (never normalized by a max), tol derived in tests/attn_cases.py.
Each case runs four input families (peaky / ramp_up / ramp_down / flat; the
CPU teeth tests prove that on these very inputs a wrong mask edge, a dropped
key or a wrong kv-head exceeds 2 * tol) and each family twice: with every
cache slot outside the visible range zeroed and with those slots at +-2^60.
The two outputs must be bit-identical — the product only guarantees zeros
beyond the live context after a reset.

Run with -s to get the per-kernel launch counts and the worst observed
err / (tol * A) (the table in DESIGN.md)."""
import collections

import numpy as np
import pytest

import cake_amd
from tests import attn_cases as ac
from tests.attn_ref import attn_ref, kv_store_ref
from tests.helpers import quantize_bf16

pytestmark = pytest.mark.gpu

LAUNCHES = collections.Counter()
WORST = collections.defaultdict(float)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nattention op tests: kernel launches and worst err/(tol*A)")
    for k in sorted(LAUNCHES):
        print(f"  {k:34s} launches {LAUNCHES[k]:5d}  worst {WORST[k]:.3f}")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _check(kernel, fam, got, ref, A, tol, fails):
    ratio = np.abs(got - ref) / (tol * A + ac.ABS_EPS)
    worst = float(np.nanmax(ratio)) if not np.isnan(ratio).all() else np.inf
    if np.isnan(got).any():
        worst = np.inf
    WORST[kernel] = max(WORST[kernel], worst)
    if not worst <= 1.0:
        i = np.unravel_index(np.nanargmax(ratio), ratio.shape)
        fails.append(f"{fam}: err/(tol*A) = {worst:.3f} at {i} "
                     f"(got {got[i]:.6g}, ref {ref[i]:.6g})")


def _pf_name(v):
    pfv, nw, split, deep = v
    if pfv == 0:
        return "prefill generic"
    if pfv == 1:
        return "prefill mfma v1"
    return f"prefill mfma2 NW{nw} " + (
        "split+combine" if split else f"DEEP{deep}" if deep else "plain")


def _run_prefill(variant, nh, nkv, hd, S, pos0, window, max_seq, tol):
    kernel = _pf_name(variant)
    fails = []
    for fam in ac.FAMILIES:
        q, kc, vc = ac.make_inputs(fam, nh, nkv, hd, max_seq, S, pos0, window)
        ref, A = attn_ref(q, kc, vc, pos0, window)
        outs = []
        for fill in (0, ac.STALE):
            k, v, vt = ac.set_stale(kc, vc, 0, pos0 + S, fill)
            outs.append(cake_amd.op_attn_prefill(q, k, v, vt, pos0, window,
                                                 variant))
            LAUNCHES[kernel] += 1
        if not np.array_equal(_bits(outs[0]), _bits(outs[1])):
            fails.append(f"{fam}: output depends on stale slots >= "
                         f"{pos0 + S} ({(_bits(outs[0]) != _bits(outs[1])).sum()}"
                         " elements differ)")
        _check(kernel, fam, outs[0], ref, A, tol, fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize(
    "variant,case", ac.PF_MFMA_CASES,
    ids=lambda x: "-".join(map(str, x)))
def test_prefill_mfma(variant, case):
    nh, nkv, S, pos0, window, max_seq = case
    _run_prefill(variant, nh, nkv, 128, S, pos0, window, max_seq,
                 ac.TOL_MFMA)


@pytest.mark.parametrize("case", ac.PF_GENERIC_CASES,
                         ids=lambda x: "-".join(map(str, x)))
def test_prefill_generic(case):
    hd, nh, nkv, S, pos0, window = case
    _run_prefill((0, 0, 0, 0), nh, nkv, hd, S, pos0, window, 128,
                 ac.TOL_F32P)


def _run_decode(case):
    nh, nkv, hd, n, nchunk, window = case
    gy = cake_amd.attn_dispatch(1, nh, nkv, hd)["decode_grid_y"]
    if gy:
        G = nh // nkv
        kernel = f"decode grouped GB{min(G, 4)}" + (
            " subg2" if G == 8 else "") + (
            " direct" if nchunk == 1 else
            " combine<=32" if nchunk <= 32 else " combine>32")
        assert nchunk * gy <= 512     # the engine's co-residency envelope
    else:
        kernel = f"decode per-head hd{hd}"
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
            LAUNCHES[kernel] += 3
        if not np.array_equal(_bits(outs[0]), _bits(outs[1])):
            fails.append(f"{fam}: output depends on stale slots outside "
                         f"[{lo},{n})")
        for r in (1, 2):
            if not np.array_equal(_bits(outs[0][0]), _bits(outs[0][r])):
                fails.append(f"{fam}: repeat {r} differs from repeat 0 "
                             "(arrival counters not re-zeroed)")
        for r in range(3):
            _check(kernel, f"{fam}/repeat{r}", outs[0][r:r + 1], ref, A,
                   ac.TOL_F32P, fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("case", ac.DEC_G_CASES,
                         ids=lambda x: "-".join(map(str, x)))
def test_decode_grouped(case):
    assert cake_amd.attn_dispatch(1, *case[:3])["decode_grid_y"] > 0
    _run_decode(case)


@pytest.mark.parametrize("case", ac.DEC_F_CASES,
                         ids=lambda x: "-".join(map(str, x)))
def test_decode_per_head(case):
    assert cake_amd.attn_dispatch(1, *case[:3])["decode_grid_y"] == 0
    _run_decode(case)


# ---- rope + KV store --------------------------------------------------------
def _store_inputs(nh, nkv, hd, max_seq, S, norm, seed):
    rng = np.random.default_rng(seed)
    qkv = quantize_bf16(
        (2.0 * rng.standard_normal((S, (nh + 2 * nkv) * hd))
         ).astype(np.float32))
    inv = 1.0 / np.power(10000.0, np.arange(0, hd, 2) / hd)
    ang = (np.arange(max_seq)[:, None] * inv[None, :]).astype(np.float32)
    cos, sin = np.cos(ang), np.sin(ang)
    # sentinel images: ordinary values with +-2^60 mixed in; vtc is NOT the
    # transpose of vc, so a write to a wrong column cannot hide
    def sentinel():
        a = rng.standard_normal((nkv, max_seq, hd))
        a = np.where(rng.random(a.shape) < 0.25,
                     rng.choice([-ac.STALE, ac.STALE], size=a.shape), a)
        return quantize_bf16(a.astype(np.float32))
    kc, vc = sentinel(), sentinel()
    vtc = np.ascontiguousarray(sentinel().transpose(0, 2, 1))
    qn = kn = None
    if norm:
        qn = quantize_bf16((1 + 0.1 * rng.standard_normal(hd)
                            ).astype(np.float32))
        kn = quantize_bf16((1 + 0.1 * rng.standard_normal(hd)
                            ).astype(np.float32))
    return qkv, cos, sin, kc, vc, vtc, qn, kn


def _run_store(hd, S, pos0, norm, decode):
    nh, nkv, max_seq, eps = 4, 2, 96, 1e-6
    qkv, cos, sin, kc, vc, vtc, qn, kn = _store_inputs(
        nh, nkv, hd, max_seq, S, norm, hd * 1000 + S * 10 + pos0 + norm)
    gq, gk, gv, gvt = cake_amd.op_kv_store(
        qkv, cos, sin, kc, vc, vtc, pos0, nh, nkv, qn, kn, eps, decode)
    kernel = "rope_store " + ("decode" if decode else "prefill")
    LAUNCHES[kernel] += 1
    rq, rk, rv, rvt, qtol, ktol = kv_store_ref(
        qkv, cos, sin, pos0, nh, nkv, kc, vc, vtc, qn, kn, eps)
    rows = slice(pos0, pos0 + S)
    # (for the store the "worst" column is err / bound of q and K)
    WORST[kernel] = max(WORST[kernel], np.max(np.abs(gq - rq) / qtol),
                        np.max(np.abs(gk - rk)[:, rows] / ktol[:, rows]))
    assert (np.abs(gq - rq) <= qtol).all(), \
        f"q: worst {np.max(np.abs(gq - rq) / qtol):.3f} of the bound"
    assert (np.abs(gk[:, rows] - rk[:, rows]) <= ktol[:, rows]).all(), \
        f"K: worst {np.max(np.abs(gk - rk)[:, rows] / ktol[:, rows]):.3f}"
    # V is a copy: exact, and the transposed image holds the same bits
    assert np.array_equal(_bits(gv[:, rows]), _bits(rv[:, rows]))
    assert np.array_equal(_bits(gvt[:, :, rows]),
                          _bits(gv[:, rows].transpose(0, 2, 1)))
    # every other slot keeps its sentinel
    out = np.ones(max_seq, dtype=bool)
    out[rows] = False
    assert np.array_equal(_bits(gk[:, out]), _bits(kc[:, out]))
    assert np.array_equal(_bits(gv[:, out]), _bits(vc[:, out]))
    assert np.array_equal(_bits(gvt[:, :, out]), _bits(vtc[:, :, out]))


@pytest.mark.parametrize("norm", [False, True], ids=["plain", "qknorm"])
@pytest.mark.parametrize("pos0", [0, 45])
@pytest.mark.parametrize("S", [1, 5, 33])
@pytest.mark.parametrize("hd", [8, 64, 128])
def test_kv_store_prefill(hd, S, pos0, norm):
    _run_store(hd, S, pos0, norm, decode=False)


@pytest.mark.parametrize("norm", [False, True], ids=["plain", "qknorm"])
@pytest.mark.parametrize("pos", [0, 45, 95])       # 95 == max_seq - 1
@pytest.mark.parametrize("hd", [8, 64, 128])
def test_kv_store_decode(hd, pos, norm):
    _run_store(hd, 1, pos, norm, decode=True)


def test_store_then_attention_chain():
    """store -> attention through the op entries equals the reference end to
    end; the decode kernels (store at pos S, attention at pos S) and a
    prefill of S + 1 rows agree on the last row."""
    nh, nkv, hd, max_seq, S, eps = 4, 2, 128, 64, 33, 1e-6
    qkv, cos, sin, _, _, _, qn, kn = _store_inputs(nh, nkv, hd, max_seq,
                                                   S + 1, True, 77)
    zk = np.zeros((nkv, max_seq, hd), np.float32)
    zt = np.zeros((nkv, hd, max_seq), np.float32)
    # reference: store in float64, round to the cache's bf16, attend
    rq, rk, rv, _, _, _ = kv_store_ref(qkv, cos, sin, 0, nh, nkv, zk, zk, zt,
                                       qn, kn, eps)
    f = lambda a: quantize_bf16(a.astype(np.float32))
    ref, A = attn_ref(f(rq), f(rk), f(rv), 0, 0)
    # GPU: S + 1 rows in one prefill store, then prefill attention
    gq, gk, gv, gvt = cake_amd.op_kv_store(qkv, cos, sin, zk, zk, zt, 0, nh,
                                           nkv, qn, kn, eps)
    pf = cake_amd.op_attn_prefill(gq, gk, gv, gvt, 0)
    assert (np.abs(pf - ref) <= ac.TOL_MFMA * A + ac.ABS_EPS).all()
    # GPU: S rows by the prefill store, row S by the decode store
    _, k1, v1, vt1 = cake_amd.op_kv_store(qkv[:S], cos, sin, zk, zk, zt, 0,
                                          nh, nkv, qn, kn, eps)
    q2, k2, v2, vt2 = cake_amd.op_kv_store(qkv[S:], cos, sin, k1, v1, vt1, S,
                                           nh, nkv, qn, kn, eps, decode=True)
    for a, b in ((k2, gk), (v2, gv), (vt2, gvt), (q2[0], gq[S])):
        assert np.array_equal(_bits(a), _bits(b))
    dec = cake_amd.op_attn_decode(q2[0], k2, v2, S, nchunk=4)[0]
    assert (np.abs(dec - ref[S]) <= ac.TOL_F32P * A[S] + ac.ABS_EPS).all()
    assert (np.abs(dec - pf[S]) <= ac.TOL_MFMA * A[S] + ac.ABS_EPS).all()
