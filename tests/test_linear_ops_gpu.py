"""Op-level GPU parity of the linear-layer kernels (GEMV, fp8 GEMV, split-K,
gate-up, fused qkv-rope, the four hand-written GEMMs and hipBLASLt, fp8
dequant) against the float64 references in tests/linear_ref.py (-m gpu).

Exact-family inputs must come back bit for bit (RNE-to-bf16 of the exact
sum, or the f32 sum itself); random inputs element-wise inside
|got - ref| <= tol * A + 2^-40, tol and A derived in tests/linear_cases.py
and never normalised by a max.  Every output buffer carries guard elements
that must keep their sentinel.  tests/test_linear_ref.py proves, for every
call made here and on its very inputs, that a dropped or doubled tail, a
neighbouring row, a wrong scale block, a transposed tile ... exceeds twice
what is tolerated here in at least one of the input families of that call.

The module stops launching after the first device error and after
MODULE_LIMIT_S seconds.  Run with -s for the per-family launch counts and
the worst observed err / bound and the wall time per test function (the
table in DESIGN.md)."""
import collections
import functools
import time

import numpy as np
import pytest

import cake_amd
from tests import linear_cases as lc
from tests import linear_ref as lr

pytestmark = pytest.mark.gpu

LAUNCHES = collections.Counter()
WORST = collections.defaultdict(float)
WALL = collections.defaultdict(float)
SKIPPED_LIB = []
MODULE_LIMIT_S = 600.0
_state = dict(t0=None, dead=None)


@pytest.fixture(scope="module", autouse=True)
def _report():
    _state["t0"] = time.monotonic()
    yield
    wall = time.monotonic() - _state["t0"]
    print("\nlinear op tests: kernel launches and worst err/bound "
          f"(module wall {wall:.1f} s)")
    for k in sorted(set(LAUNCHES) | set(WORST)):
        print(f"  {k:36s} launches {LAUNCHES[k]:5d}  worst {WORST[k]:.3f}")
    for k in sorted(WALL):
        print(f"  wall {k:36s} {WALL[k]:6.2f} s")
    print(f"  library rejected {len(SKIPPED_LIB)} shapes: {SKIPPED_LIB}")


@pytest.fixture(autouse=True)
def _gate(request):
    """One time limit for the module, and nothing runs after a device error."""
    if _state["dead"]:
        pytest.fail(f"not run: earlier device error ({_state['dead']})")
    if time.monotonic() - _state["t0"] > MODULE_LIMIT_S:
        pytest.fail(f"not run: module time limit {MODULE_LIMIT_S} s passed")
    t = time.monotonic()
    yield
    WALL[request.node.originalname] += time.monotonic() - t


def _call(fn, *a, **kw):
    """Every GPU call goes through here, so a device error stops the rest."""
    try:
        return fn(*a, **kw)
    except cake_amd.CakeHipError as e:
        if "hip error" in str(e):
            _state["dead"] = str(e)
        raise


def _guards(fam, tag, g, fails):
    if not np.array_equal(lr.f32_bits(g),
                          lr.f32_bits(np.full_like(g, cake_amd.OP_SENTINEL))):
        fails.append(f"{tag}: a guard element past the output was written")


def _judge(fam, tag, exact, got, ref, bound, f32_out, fails):
    """Bit equality for exact inputs, the element-wise bound otherwise."""
    got = np.asarray(got, dtype=np.float32)
    if exact:
        bad = lc.got_bits(got, f32_out) != lc.out_bits(ref, f32_out)
        WORST[fam] = max(WORST[fam], np.inf if bad.any() else 0.0)
        if bad.any():
            i = np.unravel_index(np.argmax(bad), bad.shape)
            fails.append(f"{tag}: {bad.sum()} of {bad.size} elements differ "
                         f"from the exact result, first at {i}: got "
                         f"{got[i]!r}, exact sum {ref[i]!r}")
        return
    ratio = np.abs(got.astype(np.float64) - ref) / bound
    worst = np.inf if np.isnan(got).any() else float(np.max(ratio))
    WORST[fam] = max(WORST[fam], worst)
    if not worst <= 1.0:
        i = np.unravel_index(np.nanargmax(ratio), ratio.shape)
        fails.append(f"{tag}: err/bound = {worst:.3f} at {i} (got {got[i]:.7g}"
                     f", ref {ref[i]:.7g})")


def _fam_name(kind, K, fp8=False):
    d = cake_amd.linear_dispatch(kind, 128, K, fp8=fp8)
    return f"{d['family']} KB{d['kb']}" if d["kb"] else d["family"]


# ---- GEMV -------------------------------------------------------------------
def _run_gemv(kind, K, rows, N, norm_modes):
    fam_k = _fam_name("plain", K, kind == "fp8") + f" rows{rows}"
    fails = []
    for epi in (0, 1, 2):
        for norm in norm_modes:
            for fam in lc.gemv_families(norm is not None):
                d = lc.gemv_inputs(fam, kind, N, K, epi, norm is not None)
                ref, A = lc.gemv_expect(d, epi, norm)
                kw = dict(kind=kind, sc=d["sc"], epi=epi, res=d["res"],
                          rows=rows, alias=epi == 1, eps=lc.EPS)
                if norm == "fused":
                    kw["nw"] = d["nw"]
                elif norm == "chain":
                    kw.update(nw=d["nw"], chain=2, scale_in=np.float32(
                        lr.norm_scale(d["x"][0], lc.EPS)))
                out, g, _ = _call(cake_amd.op_gemv, d["x"], d["w"], **kw)
                LAUNCHES[fam_k] += 1
                tag = f"epi{epi}/{norm}/{fam}"
                _guards(fam_k, tag, g, fails)
                _judge(fam_k, tag, d["exact"], out[0], ref,
                       lc.gemv_tol(epi) * A + lc.ABS_EPS, epi == 2, fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("rows", lc.GEMV_ROWS)
@pytest.mark.parametrize("K", lc.GEMV_K)
def test_gemv_bf16(K, rows):
    _run_gemv("bf16", K, rows, lc.gemv_n(rows),
              lc.gemv_norm_modes("bf16", K))


@pytest.mark.parametrize("rows", lc.FP8_ROWS)
@pytest.mark.parametrize("K", lc.FP8_K)
def test_gemv_fp8(K, rows):
    _run_gemv("fp8", K, rows, lc.FP8_N, lc.gemv_norm_modes("fp8", K))


# ---- arrival counters: split-K and the fp8 norm-chain producer --------------
@pytest.mark.parametrize("start", [0, lc.SPLITK_PREWRAP],
                         ids=["zero", "prewrap"])
@pytest.mark.parametrize("K", lc.SPLITK_K)
def test_gemv_splitk_counters(K, start):
    """Three launches on counters set once; from 2^32 - 2 the u32 wraps
    between the first and the second.  Every repeat meets its own reference
    (different x and residual rows, out aliased onto the residual)."""
    N, fam_k = lc.SPLITK_N, _fam_name("splitk", K)
    fails = []
    for fam in lc.FAMILIES[:3]:
        d = lc.gemv_inputs(fam, "splitk", N, K, 1, False, lc.REPEATS)
        out, g, _ = _call(cake_amd.op_gemv, d["x"], d["w"], kind="splitk",
                          epi=1, res=d["res"], alias=True, cnt_init=start)
        LAUNCHES[fam_k] += 3
        _guards(fam_k, fam, g, fails)
        for i in range(3):
            ref, A = lc.gemv_expect(d, 1, None, i)
            _judge(fam_k, f"{fam}/repeat{i}", d["exact"], out[i], ref,
                   lc.TOL_BF16 * A + lc.ABS_EPS, False, fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("start", ["zero", "prewrap"])
@pytest.mark.parametrize("rows", lc.FP8_ROWS)
@pytest.mark.parametrize("K", lc.PRODUCE_K)
def test_normchain_produce_counters(K, rows, start):
    """N = 640: 160 (rows 4) or 80 (rows 8) blocks, 20 or 10 per shard, which
    do not divide 2^32.  "prewrap" starts every word phase-aligned one launch
    below 2^32: a monotonic counter would wrap inside the second launch and
    elect no block there (tests/test_linear_ref.py shows that on the host
    model).  The kernel re-zeroes the word at each election, so on it this
    start exercises a non-zero aligned start only; the counters then stay
    below shard_total for good.  Every repeat's scale_out must be
    rsqrt(mean q^2 + eps) of ITS OWN quantized outputs."""
    N = lc.PRODUCE_N
    nblk = N // rows
    assert all(st & (st - 1) for st in lc.chain_shard_totals(nblk))
    cnt = lc.chain_cnt_zero() if start == "zero" else \
        lc.chain_cnt_prewrap(nblk)
    fam_k = _fam_name("plain", K, True) + f" rows{rows} produce"
    fails = []
    for fam in ("exact_sparse", "exact_dense", "random"):
        d = lc.gemv_inputs(fam, "fp8", N, K, 1, False, lc.REPEATS)
        out, g, so = _call(cake_amd.op_gemv, d["x"], d["w"], kind="fp8",
                           sc=d["sc"], epi=1, res=d["res"], rows=rows,
                           alias=True, chain=1, cnt_init=cnt, eps=lc.EPS)
        LAUNCHES[fam_k] += 3
        _guards(fam_k, fam, g, fails)
        for i in range(3):
            ref, A = lc.gemv_expect(d, 1, None, i)
            _judge(fam_k, f"{fam}/repeat{i}", d["exact"], out[i], ref,
                   lc.TOL_BF16 * A + lc.ABS_EPS, False, fails)
            # exact family: q is the reference's own; random: the kernel's
            q = lr.bf16(ref) if d["exact"] else out[i].astype(np.float64)
            want = lr.sumsq_scale(q, lc.EPS)
            rel = abs(float(so[i]) - want) / want
            WORST[fam_k + " scale/2^-20"] = max(
                WORST[fam_k + " scale/2^-20"], rel * 2.0 ** 20)
            if not rel <= 2.0 ** -20:
                fails.append(f"{fam}/repeat{i}: scale_out {so[i]!r} vs "
                             f"{want!r} (rel {rel:.3e}; sentinel = no block "
                             "was elected)")
                continue
            if fam != "random" or K != 256:
                continue
            # the consumer of THIS scale: x = the producer's output row, f32
            # logits out, reference on the float64 scale.  The norm row is
            # moved off every rounding tie by 2^-19 (the scale's 2^-20 plus
            # the kernel's f32 roundings).
            rng = lc._rng("chain consumer", rows, start, i)
            xq = out[i].astype(np.float32)
            nw = lc._q(1 + 0.2 * rng.standard_normal(N))
            for _ in range(64):
                near = lr.tie_margin(xq.astype(np.float64) * want *
                                     nw) < 2.0 ** -19
                if not near.any():
                    break
                nw.view(np.uint32)[near] += np.uint32(0x10000)
            assert not near.any()
            w8, sc = lc.random_w8(128, N, rng)
            got = _call(cake_amd.op_gemv, xq, w8, kind="fp8", sc=sc, epi=2,
                        nw=nw, chain=2, scale_in=so[i])[0][0]
            LAUNCHES[fam_k.replace("produce", "consume")] += 1
            cref, cA = lr.gemv_ref(lr.dequant(w8, sc), xq, None, nw, 0.0,
                                   want, None, True)
            _judge(fam_k.replace("produce", "consume"),
                   f"{fam}/repeat{i}/consumer", False, got, cref,
                   lc.TOL_F32 * cA + lc.ABS_EPS, True, fails)
    assert not fails, "\n".join(fails)


# ---- gate-up ----------------------------------------------------------------
def _run_gateup(fp8, K, rows, I):
    fam_k = _fam_name("gateup", K, fp8) + f" rows{rows}"
    fails = []
    for norm in (None, "fused") + (("chain",) if fp8 else ()):
        for fam in lc.gemv_families(norm is not None):
            d = lc.gateup_inputs(fam, fp8, I, K, norm is not None)
            scale = None
            kw = dict(sc=d["sc"], eps=lc.EPS, rows=0 if fp8 else rows)
            if norm:
                kw["nw"] = d["nw"]
            if norm == "chain":
                kw["scale_in"] = np.float32(lr.norm_scale(d["x"], lc.EPS))
                scale = float(kw["scale_in"])
            val, g, u, Ag, Au = lr.gateup_ref(
                d["W64"], d["x"], I, d["nw"], lc.EPS, scale, None, fp8)
            out, gd = _call(cake_amd.op_gemv_gateup, d["x"], d["w"], I, **kw)
            LAUNCHES[fam_k] += 1
            tag = f"{norm}/{fam}"
            _guards(fam_k, tag, gd, fails)
            _judge(fam_k, tag, False, out, val,
                   lc.gateup_bound(val, g, u, Ag, Au), False, fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("rows", [4, 8])
@pytest.mark.parametrize("K", lc.GATEUP_K)
def test_gateup_bf16(K, rows):
    _run_gateup(False, K, rows, lc.gateup_i(False, rows))


@pytest.mark.parametrize("K", lc.GATEUP_FP8_K)
def test_gateup_fp8(K):
    _run_gateup(True, K, 4, lc.gateup_i(True, 4))


# ---- bit-exact invariants the kernel comments claim -------------------------
def _pow2_x(K, rng):
    """x in {+-2^j}: the sum of squares is exact in f32 in any order, so the
    fused kernels and k_rmsnorm compute the very same scale."""
    return (rng.choice([-1.0, 1.0], size=K) * 2.0 ** rng.integers(
        -2, 3, size=K)).astype(np.float32)


@pytest.mark.parametrize("K", [72, 2056, 4104, 8200, 16384])
def test_fused_norm_equals_rmsnorm_then_gemv_bf16(K):
    rng = lc._rng("inv", K)
    x, nw = _pow2_x(K, rng), lc._q(1 + 0.2 * rng.standard_normal(K))
    w = lc._q(0.05 * rng.standard_normal((9, K)))
    wgu = lc._q(rng.standard_normal((34, K)) / np.sqrt(K))
    xn = _call(cake_amd.op_rms_norm, x, nw, eps=lc.EPS)
    for rows in (2, 4, 8):
        a = _call(cake_amd.op_gemv, x, w, nw=nw, eps=lc.EPS, rows=rows)[0]
        b = _call(cake_amd.op_gemv, xn, w, rows=rows)[0]
        assert np.array_equal(lr.f32_bits(a), lr.f32_bits(b)), rows
    for rows in (4, 8):
        a = _call(cake_amd.op_gemv_gateup, x, wgu, 17, nw=nw, eps=lc.EPS,
                  rows=rows)[0]
        b = _call(cake_amd.op_gemv_gateup, xn, wgu, 17, rows=rows)[0]
        assert np.array_equal(lr.f32_bits(a), lr.f32_bits(b)), rows
    LAUNCHES["invariants bf16"] += 11


@pytest.mark.parametrize("K", [128, 4224, 8320, 16384])
def test_fused_norm_and_chain_equal_rmsnorm_then_gemv_fp8(K):
    rng = lc._rng("inv8", K)
    x, nw = _pow2_x(K, rng), lc._q(1 + 0.2 * rng.standard_normal(K))
    w8, sc = lc.random_w8(256, K, rng)
    sc = (sc * 40).astype(np.float32)
    xn = _call(cake_amd.op_rms_norm, x, nw, eps=lc.EPS)
    # the scale both kernels compute: exact sum / K + eps, then rsqrt; the
    # chain consumer gets the correctly rounded f32 of the float64 value
    s_ref = np.float32(lr.norm_scale(x, lc.EPS))
    pair = _call(cake_amd.op_gemv, xn, w8, kind="fp8", sc=sc)[0]
    fused = _call(cake_amd.op_gemv, x, w8, kind="fp8", sc=sc, nw=nw,
                  eps=lc.EPS)[0]
    assert np.array_equal(lr.f32_bits(fused), lr.f32_bits(pair))
    gp = _call(cake_amd.op_gemv_gateup, xn, w8, 128, sc=sc)[0]
    gf = _call(cake_amd.op_gemv_gateup, x, w8, 128, sc=sc, nw=nw,
               eps=lc.EPS)[0]
    assert np.array_equal(lr.f32_bits(gf), lr.f32_bits(gp))
    # norm-chain consume with the reference scale == rmsnorm with that scale
    # applied in the reference, then the plain kernels
    xr = lr.bf16(x.astype(np.float64) * np.float64(s_ref) *
                 nw).astype(np.float32)
    tie_ok = (lr.tie_margin(x.astype(np.float64) * np.float64(s_ref) * nw)
              >= lc.TIE_MARGIN)
    x2 = np.where(tie_ok, x, 0).astype(np.float32)   # drop near-tie elements
    xr = np.where(tie_ok, xr, 0).astype(np.float32)
    cons = _call(cake_amd.op_gemv, x2, w8, kind="fp8", sc=sc, nw=nw, chain=2,
                 scale_in=s_ref)[0]
    pair2 = _call(cake_amd.op_gemv, xr, w8, kind="fp8", sc=sc)[0]
    assert np.array_equal(lr.f32_bits(cons), lr.f32_bits(pair2))
    gc = _call(cake_amd.op_gemv_gateup, x2, w8, 128, sc=sc, nw=nw,
               scale_in=s_ref)[0]
    gp2 = _call(cake_amd.op_gemv_gateup, xr, w8, 128, sc=sc)[0]
    assert np.array_equal(lr.f32_bits(gc), lr.f32_bits(gp2))
    LAUNCHES["invariants fp8"] += 9


# ---- fused norm -> qkv GEMV -> rope -> KV store ------------------------------
@pytest.mark.parametrize("case", lc.rope_cases(),
                         ids=lambda c: "-".join(map(str, c)))
def test_qkv_rope(case):
    nh, nkv, hd, K, pos = case
    fam_k = _fam_name("qkv_rope", K)
    fails = []
    for fam in ("exact_dense", "random"):
        d = lc.rope_inputs(fam, nh, nkv, hd, K, pos)
        r = lr.qkv_rope_ref(d["w"], d["x"], d["nw"], lc.EPS, d["cos"],
                            d["sin"], pos, nh, nkv, hd, d["kc"], d["vc"],
                            d["vtc"])
        q, rest, kc, vc, vtc = _call(
            cake_amd.op_gemv_qkv_rope, d["x"], d["nw"], d["w"], d["cos"],
            d["sin"], d["kc"], d["vc"], d["vtc"], pos, nh, nkv, eps=lc.EPS)
        LAUNCHES[fam_k] += 1
        # k and v never land in the activation row; the guards stay
        _guards(fam_k, f"{fam}/activation row", rest, fails)
        _judge(fam_k, f"{fam}/q", False, q, r["q"],
               lc.rope_bound(r["q_mag"], r["q_acc"]), False, fails)
        _judge(fam_k, f"{fam}/k", False, kc[:, pos], r["kc"][:, pos],
               lc.rope_bound(r["k_mag"], r["k_acc"]), False, fails)
        # V and V^T: bf16 of the sum, bit for bit, in the exact family; one
        # image of the other always
        if d["exact"]:
            if not np.array_equal(lc.got_bits(vc[:, pos], False),
                                  lr.bf16_bits(r["vc"][:, pos])):
                fails.append(f"{fam}: V row differs from bf16 of the sum")
        else:
            s = r["vc"][:, pos]
            _judge(fam_k, f"{fam}/v", False, vc[:, pos], s,
                   lc.TOL_BF16 * np.abs(s) + lc.TOL_F32 * r["v_A"] +
                   lc.ABS_EPS, False, fails)
        if not np.array_equal(lr.f32_bits(vtc[:, :, pos]),
                              lr.f32_bits(vc[:, pos])):
            fails.append(f"{fam}: V^T column differs from the V row")
        other = np.ones(lc.ROPE_MAX_SEQ, dtype=bool)
        other[pos] = False
        for name, got, was in (("kc", kc[:, other], d["kc"][:, other]),
                               ("vc", vc[:, other], d["vc"][:, other]),
                               ("vtc", vtc[:, :, other],
                                d["vtc"][:, :, other])):
            if not np.array_equal(lr.f32_bits(got), lr.f32_bits(was)):
                fails.append(f"{fam}: {name} slot other than {pos} changed")
    assert not fails, "\n".join(fails)


# ---- GEMM -------------------------------------------------------------------
GEMM_CASES = [(v,) + c for v in cake_amd.GEMM_VARIANTS
              for c in lc.gemm_cases(v)]


def _run_gemm(variant, M, N, K, modes, families, ref_fn):
    fam_k = f"gemm {variant}"
    fails = []
    for epi, alias in modes:
        for fam in families:
            d = lc.gemm_inputs(fam, M, N, K, epi)
            out, g, ran = _call(cake_amd.op_gemm, d["a"], d["w"], variant,
                                res=d["res"], alias=alias)
            if ran is None:
                assert variant == "library"
                return False
            assert ran == variant
            LAUNCHES[fam_k] += 1
            ref, A = ref_fn(fam, epi, d)
            tag = f"epi{epi}/alias{int(alias)}/{fam}"
            _guards(fam_k, tag, g, fails)
            _judge(fam_k, tag, d["exact"], out, ref,
                   lc.TOL_BF16 * A + lc.ABS_EPS, False, fails)
    assert not fails, "\n".join(fails)
    return True


@pytest.mark.parametrize("case", GEMM_CASES,
                         ids=lambda c: "-".join(map(str, c)))
def test_gemm_variant(case):
    variant, M, N, K = case
    ok = _run_gemm(variant, M, N, K, lc.GEMM_MODES, lc.GEMM_FAMILIES,
                   lambda fam, epi, d: lr.gemm_ref(d["a"], d["w"], d["res"]))
    if not ok:
        SKIPPED_LIB.append((M, N, K))
        pytest.skip(f"hipBLASLt rejects {M}x{N}x{K} "
                    f"({len(SKIPPED_LIB)} shapes so far)")


@functools.lru_cache(maxsize=2)
def _product_ref(fam):
    M, N, K = lc.GEMM_PRODUCT
    d = lc.gemm_inputs(fam, M, N, K, 1)
    # integer inputs with |sum| < 2^24: the f32 product is exact as well
    t = np.float32 if d["exact"] else np.float64
    a, w, r = d["a"].astype(t), d["w"].astype(t), d["res"].astype(t)
    A = np.abs(a) @ np.abs(w).T + np.abs(r)
    assert not d["exact"] or (A < 2 ** 24).all()
    return (a @ w.T + r).astype(np.float64), A.astype(np.float64)


@pytest.mark.parametrize("variant", ["128x256", "library"])
def test_gemm_product_class_shape(variant):
    """2048 x 4096 x 4096 with the residual aliased onto C: the 8B
    o-projection class, which the policy keeps on k_gemm_128x256 (pinned in
    test_linear_ref.py).  The library must take this shape."""
    M, N, K = lc.GEMM_PRODUCT
    ok = _run_gemm(variant, M, N, K, ((1, True),), ("exact_dense", "random"),
                   lambda fam, epi, d: _product_ref(fam))
    assert ok, "hipBLASLt rejected the product-class shape"


# ---- fp8 dequant ------------------------------------------------------------
@pytest.mark.parametrize("N,K", [(128, 128), (256, 384), (4224, 4096)],
                         ids=["one-block", "2x3-blocks", "grid-stride"])
def test_dequant_fp8(N, K):
    """One IEEE f32 multiply then RNE, bit for bit, NaN codes included; the
    last shape is past one pass of the kernel's grid (2^24 elements)."""
    rng = lc._rng("dequant", N, K)
    w8 = rng.integers(0, 256, size=(N, K)).astype(np.uint8)
    w8[0, :2] = [0x7F, 0xFF]
    w8[-1, -2:] = [0xFF, 0x7F]
    sc = (3e-4 * 2.0 ** rng.uniform(-2, 2, size=(N // 128, K // 128))
          ).astype(np.float32)
    out, g = _call(cake_amd.op_dequant_fp8, w8, sc)
    LAUNCHES["dequant_fp8"] += 1
    fails = []
    _guards("dequant_fp8", "dequant", g, fails)
    assert not fails, fails
    got = lr.f32_bits(out) >> 16
    got = np.where(np.isnan(out), np.uint32(0x7FC0), got)
    want = lr.dequant_bf16_bits(w8, sc)
    assert np.isnan(out[0, 0]) and np.isnan(out[0, 1])
    bad = got != want
    WORST["dequant_fp8"] = max(WORST["dequant_fp8"],
                               np.inf if bad.any() else 0.0)
    assert not bad.any(), f"{bad.sum()} of {bad.size} elements differ"


# ---- plain kernels of the prefill and split-norm chains ---------------------
def _ulp_judge(fam, tag, safe, got, ref, fails):
    """Tie-safe inputs: RNE-to-bf16 of the float64 value, bit for bit.  Plain
    random inputs: within one bf16 ulp of it."""
    got = np.asarray(got, dtype=np.float32)
    if safe:
        bad = lc.got_bits(got, False) != lr.bf16_bits(ref)
        worst = np.inf if bad.any() else 0.0
    else:
        worst = float(np.max(np.abs(got - lr.bf16(ref)) / lc.bf16_ulp(ref)))
    WORST[fam] = max(WORST[fam], worst)
    if not worst <= 1.0:
        fails.append(f"{tag}: worst {worst} bf16 ulp from the reference")


@pytest.mark.parametrize("S,I", lc.SILU_ROWS_CASES)
def test_silu_mul_rows(S, I):
    fails = []
    for safe in (True, False):
        gu = lc.silu_rows_inputs(S, I, safe)
        out, g = _call(cake_amd.op_silu_mul_rows, gu)
        LAUNCHES["silu_mul_rows"] += 1
        _guards("silu_mul_rows", f"safe{safe}", g, fails)
        _ulp_judge("silu_mul_rows", f"safe{safe}", safe, out,
                   lc.silu_rows_ref(gu), fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("case", lc.RMS_ROWS_CASES,
                         ids=lambda c: "-".join(map(str, c)))
def test_rms_norm_rows(case):
    outer, inner, gap, cols = case
    fails = []
    for safe in (True, False):
        x, w, stride, offs = lc.rms_rows_inputs(outer, inner, gap, cols, safe)
        out, g = _call(cake_amd.op_rms_norm_rows, x, w, outer, inner, stride,
                       eps=lc.EPS)
        LAUNCHES["rms_norm rows"] += 1
        _guards("rms_norm rows", f"safe{safe}", g, fails)
        ref = lc.rms_rows_ref(x, w, offs, lc.EPS)
        rows = ~np.isnan(ref)
        _ulp_judge("rms_norm rows", f"safe{safe}", safe, out[rows], ref[rows],
                   fails)
        if not (out[~rows] == cake_amd.OP_SENTINEL).all():
            fails.append(f"safe{safe}: an element between the rows changed")
    assert not fails, "\n".join(fails)
