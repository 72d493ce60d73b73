"""CPU tests of the linear-layer references and of the GPU tests' inputs
(tests/linear_ref.py, tests/linear_cases.py): the number formats, the
exactness and tie-safety margins the GPU assertions rest on, the teeth of
every GPU case (each defect that fits a case must move the reference, on that
case's own inputs, by more than the GPU test tolerates), the host model of
the arrival counters, the coverage of every configured model's decode
dispatch, the pinned policy table, and the argument checks of the op entries
(which run before any device call)."""
import functools

import numpy as np
import pytest

import cake_amd
from cake_amd.configs import MODELS
from tests import linear_cases as lc
from tests import linear_ref as lr
from tests.helpers import quantize_bf16


# ---- number formats ---------------------------------------------------------
def test_e4m3fn_table_matches_oracle_on_all_codes():
    from oracle import f8e4m3_to_f32
    codes = np.arange(256, dtype=np.uint8)
    ours, theirs = lr.E4M3, f8e4m3_to_f32(codes).astype(np.float64)
    assert np.array_equal(np.isnan(ours), np.isnan(theirs))
    assert np.isnan(ours[[0x7F, 0xFF]]).all() and np.isnan(ours).sum() == 2
    ok = ~np.isnan(ours)
    assert np.array_equal(ours[ok], theirs[ok])
    assert lr.E4M3[0x7E] == 448.0 and lr.E4M3[0x01] == 2.0 ** -9


def test_bf16_rounds_once_and_matches_the_device_rule():
    rng = np.random.default_rng(0)
    x = (rng.standard_normal(20000) * 2.0 ** rng.integers(-20, 20, 20000)
         ).astype(np.float32)
    assert np.array_equal(lr.bf16(x.astype(np.float64)).astype(np.float32),
                          quantize_bf16(x))
    # a float64 just above a tie rounds up; via f32 it would round to even
    v = 1.0 + 2.0 ** -8 + 2.0 ** -40
    assert lr.bf16(v) == 1.0 + 2.0 ** -7
    assert lr.bf16(1.0 + 2.0 ** -8) == 1.0          # tie -> even
    assert lr.bf16(1.0 + 3 * 2.0 ** -8) == 1.0 + 2.0 ** -6


def test_dequant_reference_special_codes():
    w8 = np.zeros((128, 128), np.uint8)
    w8[0, :4] = [0x7F, 0xFF, 0x7E, 0x80]
    bits = lr.dequant_bf16_bits(w8, np.full((1, 1), 0.5, np.float32))
    assert bits[0, 0] == 0x7FC0 and bits[0, 1] == 0x7FC0
    assert bits[0, 2] == lr.bf16_bits(224.0) and bits[0, 3] == 0x8000


# ---- margins the bit-exact GPU assertions rest on --------------------------
GEMV_CASES = lc.gemv_gpu_cases()
_id = lambda c: "-".join(map(str, c))


@functools.lru_cache(maxsize=8)
def _gemv_inputs(fam, kind, N, K, epi, norm, repeats):
    return lc.gemv_inputs(fam, kind, N, K, epi, norm is not None, repeats)


@pytest.mark.parametrize("case", GEMV_CASES, ids=_id)
def test_gemv_exact_families_are_exact_and_tie_safe(case):
    kind, N, K, epi, norm, repeats = case
    for fam in lc.gemv_families(norm is not None):
        d = _gemv_inputs(fam, *case)
        if d["exact"]:
            for i in range(1, repeats):
                v, A = lc.gemv_expect(d, epi, norm, i)
                assert (A * 8 < 2 ** 24).all()
                assert np.array_equal(v * 8, np.rint(v * 8))
            # every term is a multiple of q = 2^-3 (scale 2^-2, nw 2^-1) and
            # the absolute sum stays below 2^24 q: any f32 order is exact
            _, A = lc.gemv_expect(d, epi, norm)
            assert (A * 8 < 2 ** 24).all()
            v, _ = lc.gemv_expect(d, epi, norm)
            assert np.array_equal(v * 8, np.rint(v * 8))
            if norm:
                # x in {+-1}: mean 1, and ANY scale within 2^-16 of 1 (eps <=
                # 1e-5 moves it 5e-6; f32 rounding and rsqrtf 2^-22) still
                # re-quantizes x * scale * nw to +-nw
                x, nw = d["x"][0].astype(np.float64), d["nw"]
                assert np.sum(x * x) == K
                for s in (1 - 2.0 ** -16, 1 + 2.0 ** -16,
                          lr.norm_scale(x, lc.EPS)):
                    assert np.array_equal(lr.bf16(x * s * nw), x * nw)
        elif norm:
            x = d["x"][0].astype(np.float64)
            s = lr.norm_scale(x, lc.EPS)
            assert (lr.tie_margin(x * s * d["nw"]) >= lc.TIE_MARGIN).all()
            assert np.array_equal(quantize_bf16(d["x"]), d["x"])


def test_small_family_makes_eps_matter():
    d = _gemv_inputs("random_small", "bf16", 5, 4104, 0, "fused", 1)
    m = np.mean(d["x"][0].astype(np.float64) ** 2)
    assert 0.3 * lc.EPS < m < 3 * lc.EPS


# ---- teeth ------------------------------------------------------------------
def _teeth(mutants, families, run):
    """Every mutant that fits the case must be caught by AT LEAST ONE input
    family of the case: run(fam, mut) -> (exact, base, mutated, bound,
    f32_out).  No single family can see every defect (a sparse exact x is
    blind to eps, Gaussian inputs at K = 16384 are blind to eight dropped k),
    so the guarantee is per case over its families, all of which the GPU test
    of that case runs."""
    missed = []
    for mut in mutants:
        for fam in families:
            if lc.moved(*run(fam, mut)):
                break
        else:
            missed.append(mut)
    assert not missed, f"mutants that no family of this case catches: {missed}"


@pytest.mark.parametrize("case", GEMV_CASES, ids=_id)
def test_gemv_teeth(case):
    """On the inputs of every op_gemv call of the GPU module, every repeat
    of the counter cases included (each has its own x and residual row)."""
    kind, N, K, epi, norm, repeats = case
    muts = lc.gemv_mutants(kind, N, K, epi, norm is not None, 0)
    if norm == "chain":     # the scale is an input there, not computed
        muts = [m for m in muts if m not in ("eps_dropped", "mean_padded")]
    for i in range(repeats):
        def run(fam, mut):
            d = _gemv_inputs(fam, *case)
            base, A = lc.gemv_expect(d, epi, norm, i)
            got, _ = lc.gemv_expect(d, epi, norm, i, mut=mut)
            return (d["exact"], base, got,
                    lc.gemv_tol(epi) * A + lc.ABS_EPS, epi == 2)
        _teeth(muts, lc.gemv_families(norm is not None), run)


@pytest.mark.parametrize("case", lc.gateup_gpu_cases(), ids=_id)
def test_gateup_teeth(case):
    fp8, I, K, norm = case
    muts = lc.gateup_mutants(fp8, I, K, norm is not None)
    if norm == "chain":
        muts = [m for m in muts if m not in ("eps_dropped", "mean_padded")]
    cache = {}

    def run(fam, mut):
        if fam not in cache:
            cache[fam] = lc.gateup_inputs(fam, fp8, I, K, norm is not None)
        d = cache[fam]
        scale = None
        if norm == "chain":
            scale = float(np.float32(lr.norm_scale(d["x"], lc.EPS)))

        def ref(m):
            W = d["W64"]
            if m in ("scale_row_off", "scale_col_off", "gate_scale_for_up"):
                W = lr.dequant(d["w"], d["sc"], m, I)
            return lr.gateup_ref(W, d["x"], I, d["nw"], lc.EPS, scale, m, fp8)
        val, g, u, Ag, Au = ref(None)
        if d["exact"]:       # g and u themselves are exact there
            assert (Ag * 8 < 2 ** 24).all() and (Au * 8 < 2 ** 24).all()
        return (False, val, ref(mut)[0], lc.gateup_bound(val, g, u, Ag, Au),
                False)
    _teeth(muts, lc.gemv_families(norm is not None), run)


@pytest.mark.parametrize("case", lc.rope_cases(), ids=_id)
def test_qkv_rope_teeth(case):
    nh, nkv, hd, K, pos = case

    def run(fam, mut):
        d = lc.rope_inputs(fam, nh, nkv, hd, K, pos)
        f = lambda m: lr.qkv_rope_ref(
            d["w"], d["x"], d["nw"], lc.EPS, d["cos"], d["sin"], pos, nh,
            nkv, hd, d["kc"], d["vc"], d["vtc"], m)
        a, b = f(None), f(mut)
        p = a["slot"]
        # one flat vector of everything the GPU test looks at
        pack = lambda r: np.concatenate(
            [r["q"].ravel(), r["kc"].ravel(), r["vc"].ravel(),
             r["vtc"].ravel()])
        bound = np.zeros_like(pack(a))
        nq = a["q"].size
        bound[:nq] = lc.rope_bound(a["q_mag"], a["q_acc"]).ravel()
        kb = np.zeros_like(a["kc"])
        kb[:, p] = lc.rope_bound(a["k_mag"], a["k_acc"])
        bound[nq:nq + kb.size] = kb.ravel()
        return False, pack(a), pack(b), bound, False
    muts = [m for m in lc.ROPE_MUTANTS
            if not (m == "kvhead_off" and nkv == 1)]
    _teeth(muts, ("exact_dense", "random"), run)


# 256p shares the cases and the tile of 256, the library those of 128
GEMM_TEETH = [(v, M, N, K, epi) for v in ("128", "256", "128x256")
              for (M, N, K) in lc.gemm_cases(v) for epi in (0, 1)]


@pytest.mark.parametrize("case", GEMM_TEETH, ids=_id)
def test_gemm_teeth(case):
    variant, M, N, K, epi = case

    def run(fam, mut):
        d = lc.gemm_inputs(fam, M, N, K, epi)
        base, A = lr.gemm_ref(d["a"], d["w"], d["res"])
        if d["exact"]:
            assert (A < 2 ** 24).all()
        got, _ = lr.gemm_ref(d["a"], d["w"], d["res"], mut,
                             lc.GEMM_TILE[variant])
        return d["exact"], base, got, lc.TOL_BF16 * A + lc.ABS_EPS, False
    _teeth(lc.gemm_mutants(variant, M, N, K, epi), lc.GEMM_FAMILIES, run)


def test_gemm_teeth_product_class_shape():
    """The aliased 2048 x 4096 x 4096 case, on its exact family (integer
    inputs: the f32 products below are exact)."""
    M, N, K = lc.GEMM_PRODUCT
    d = lc.gemm_inputs("exact_dense", M, N, K, 1)
    a, w, r = d["a"], d["w"], d["res"]
    base = a @ w.T + r
    assert (np.abs(a) @ np.abs(w).T + np.abs(r) < 2 ** 24).all()
    a2 = a.copy()
    a2[:, K - 64:] = 0                                  # last k-tile dropped
    assert (lr.bf16_bits(base) != lr.bf16_bits(a2 @ w.T + r)).any()
    assert (lr.bf16_bits(base) != lr.bf16_bits(a @ w.T + r.T.reshape(M, N))
            ).any()                                     # residual transposed
    sw = base.copy()                                    # tiles transposed
    sw[:128, 256:512] = (a[128:256] @ w[:256].T)[:, :256] + r[:128, 256:512]
    assert (lr.bf16_bits(base) != lr.bf16_bits(sw)).any()
    assert lr.bf16_bits(lr.SENTINEL) not in lr.bf16_bits(base)  # uncomputed


# ---- arrival counters: host model ------------------------------------------
def test_monotonic_modulo_election_breaks_at_the_u32_wrap_and_reset_fixes_it():
    """Qwen3-32B fp8, rows 4: 1280 blocks, 160 per shard; 2^32 % 160 = 96.
    A monotonic counter elects the wrong arrival (or none) once it wraps;
    re-zeroing at the election keeps every launch electing its last."""
    st = lc.chain_shard_totals(1280)[0]
    assert st == 160 and 2 ** 32 % st == 96
    start = int(lc.chain_cnt_prewrap(1280)[0])
    assert start % st == 0 and start + 2 * st > 2 ** 32 > start + st
    want = [st - 1] * 4
    assert lc.elect_trace(0, st, 4, reset=False) == want
    assert lc.elect_trace(start, st, 4, reset=False) != want
    assert lc.elect_trace(start, st, 4, reset=True) == want
    assert lc.elect_trace(0, st, 4, reset=True) == want
    # split-K: modulus 2 divides 2^32, the monotonic counter survives
    assert lc.elect_trace(lc.SPLITK_PREWRAP, 2, 4, reset=False) == [1] * 4
    assert lc.elect_trace(2 ** 32 - 8, 8, 4, reset=False) == [7] * 4


# ---- coverage map and pinned policy ----------------------------------------
def _covered():
    d = cake_amd.linear_dispatch
    s = set()
    for K in lc.GEMV_K:
        for r in lc.GEMV_ROWS:
            x = d("plain", 64, K)
            s.add((x["family"], r, x["kb"]))
    for K in lc.FP8_K:
        for r in lc.FP8_ROWS:
            x = d("plain", 128, K, fp8=True)
            s.add((x["family"], r, x["kb"]))
    for K in lc.GATEUP_K:
        assert d("gateup", 64, K)["rows"] == 4      # the engine default
        s |= {("gateup", r, d("gateup", 64, K)["kb"]) for r in (4, 8)}
    for K in lc.GATEUP_FP8_K:
        s.add(tuple(d("gateup", 128, K, fp8=True).values()))
    for K in lc.ROPE_K:
        s.add(tuple(d("qkv_rope", 256, K).values()))
    for K in lc.SPLITK_K:
        s.add(tuple(d("splitk", 64, K).values()))
    return s


PINNED = {
    "llama3-8b": dict(qkv=("qkv_rope", 4, 2), o=("gemv_reg", 2, 2),
                      gateup=("gateup", 4, 2), down=("gemv_reg", 4, 8),
                      head=("gemv_reg", 8, 2)),
    "llama3-70b": dict(qkv=("qkv_rope", 4, 4), o=("gemv_reg", 4, 4),
                       gateup=("gateup", 4, 4), down=("gemv_stream", 4, 0),
                       head=("gemv_reg", 8, 4)),
    "qwen3-0.6b": dict(qkv=("gemv_reg", 2, 2), o=("gemv_reg", 2, 2),
                       gateup=("gateup", 4, 2), down=("gemv_reg", 2, 2),
                       head=("gemv_reg", 8, 2)),
    "mistral-7b": dict(qkv=("qkv_rope", 4, 2), o=("gemv_reg", 2, 2),
                       gateup=("gateup", 4, 2), down=("gemv_reg", 4, 8),
                       head=("gemv_reg", 8, 2)),
    "qwen3-32b": dict(qkv=("gemv_reg", 4, 4), o=("gemv_reg", 4, 4),
                      gateup=("gateup", 4, 4), down=("gemv_stream", 4, 0),
                      head=("gemv_reg", 8, 4)),
    "qwen3-32b-fp8": dict(qkv=("gemv_fp8", 4, 2), o=("gemv_fp8", 4, 2),
                          gateup=("gateup_fp8", 4, 2),
                          down=("gemv_fp8_stream", 4, 0),
                          head=("gemv_reg", 8, 4)),
}
# llama3-8b prefill at M = 2048: (library first, hand-written variant)
PINNED_GEMM_8B = dict(qkv=(True, "128x256"), o=(False, "128x256"),
                      gateup=(True, "256"), down=(True, "128x256"))


def test_decode_dispatch_is_pinned_and_covered_by_the_gpu_cases():
    assert set(PINNED) == set(MODELS)
    covered = _covered()
    for name, cfg in MODELS.items():
        # by the engine's own predicates (cake_hip_decode_dispatch)
        got = cake_amd.decode_dispatch(cfg)
        assert got == PINNED[name], name
        missing = {k: v for k, v in got.items() if v not in covered}
        assert not missing, f"{name}: no GPU case runs {missing}"


def test_gemm_policy_is_pinned_for_8b_prefill():
    c = MODELS["llama3-8b"]
    H, I = c["hidden_size"], c["intermediate_size"]
    shapes = dict(qkv=(6144, H), o=(H, 4096), gateup=(2 * I, H), down=(H, I))
    for k, (N, K) in shapes.items():
        d = cake_amd.linear_dispatch("gemm", N, K, M=2048)
        assert (d["lib_first"], d["variant"]) == PINNED_GEMM_8B[k], k
    # the product-class shape of the GPU tests is the o projection's
    assert lc.GEMM_PRODUCT == (2048,) + shapes["o"]
    # small grids fall to the 128^2 kernel behind the library
    d = cake_amd.linear_dispatch("gemm", 300, 96, M=200)
    assert (d["lib_first"], d["variant"]) == (True, "128")


# ---- argument checks run before any device call ----------------------------
def test_op_entries_reject_bad_arguments_without_a_device():
    E = cake_amd.CakeHipError
    x8, w8 = np.zeros(8, np.float32), np.zeros((3, 8), np.float32)
    with pytest.raises(E, match="multiple of 8"):
        cake_amd.op_gemv(np.zeros(12, np.float32),
                         np.zeros((3, 12), np.float32))
    with pytest.raises(E, match="rows"):
        cake_amd.op_gemv(x8, w8, rows=3)
    with pytest.raises(E, match="res goes with epi 1"):
        cake_amd.op_gemv(x8, w8, epi=1)
    with pytest.raises(E, match="K % 16"):
        cake_amd.op_gemv(np.zeros(24, np.float32),
                         np.zeros((3, 24), np.float32), kind="splitk", epi=1,
                         res=np.zeros((1, 3), np.float32), cnt_init=0)
    with pytest.raises(E, match="% 128"):
        cake_amd.op_gemv(np.zeros(64, np.float32),
                         np.zeros((128, 64), np.uint8), kind="fp8",
                         sc=np.zeros((1, 0), np.float32))
    with pytest.raises(E, match="no norm"):
        cake_amd.op_gemv(np.zeros(16392, np.float32),
                         np.zeros((3, 16392), np.float32),
                         nw=np.zeros(16392, np.float32))
    with pytest.raises(E, match="repeats"):
        cake_amd.op_gemv(np.zeros((17, 8), np.float32), w8)
    with pytest.raises(E, match="16384"):
        cake_amd.op_gemv_gateup(np.zeros(16392, np.float32),
                                np.zeros((2, 16392), np.float32), 1)
    with pytest.raises(E, match="K % 64"):
        cake_amd.op_gemm(np.zeros((4, 96), np.float32),
                         np.zeros((4, 96), np.float32), "256")
    with pytest.raises(E, match="alias"):
        cake_amd.op_gemm(np.zeros((4, 64), np.float32),
                         np.zeros((4, 64), np.float32), "128", alias=True)
    with pytest.raises(E, match="% 128"):
        cake_amd.op_dequant_fp8(np.zeros((128, 64), np.uint8),
                                np.zeros((1, 0), np.float32))
    with pytest.raises(E, match="pos"):
        cake_amd.op_gemv_qkv_rope(
            x8, x8, np.zeros((32, 8), np.float32),
            np.zeros((32, 4), np.float32), np.zeros((32, 4), np.float32),
            np.zeros((1, 32, 8), np.float32), np.zeros((1, 32, 8), np.float32),
            np.zeros((1, 8, 32), np.float32), 32, 2, 1)
    with pytest.raises(E):
        cake_amd.linear_dispatch("gateup", 64, 16392)


def test_plain_kernel_inputs_are_tie_safe():
    """The bit-exact halves of the silu_mul_rows and rms_norm rows GPU tests
    rest on these margins."""
    for S, I in lc.SILU_ROWS_CASES:
        gu = lc.silu_rows_inputs(S, I, True)
        assert np.array_equal(quantize_bf16(gu), gu)
        assert np.abs(gu[:, :I]).max() <= 3
        assert (lr.tie_margin(lc.silu_rows_ref(gu)) >= lc.TIE_MARGIN).all()
    for case in lc.RMS_ROWS_CASES:
        x, w, stride, offs = lc.rms_rows_inputs(*case, True)
        ref = lc.rms_rows_ref(x, w, offs, lc.EPS)
        assert np.isnan(ref).sum() == (case[0] - 1) * case[2]
        assert (lr.tie_margin(ref[~np.isnan(ref)]) >= lc.TIE_MARGIN).all()
    E = cake_amd.CakeHipError
    with pytest.raises(E, match="multiple of 8"):
        cake_amd.op_silu_mul_rows(np.zeros((2, 24), np.float32))
    with pytest.raises(E, match="outer_stride"):
        cake_amd.op_rms_norm_rows(np.zeros(100, np.float32),
                                  np.zeros(8, np.float32), 2, 2, 12)
