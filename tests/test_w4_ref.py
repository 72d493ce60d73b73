"""CPU tests of the GPTQ 4-bit reference and of the GPU tests' inputs
(tests/w4_ref.py, tests/w4_cases.py): the format round trip, the exactness the
bit-exact GPU assertions rest on, the teeth of every GPU call (each defect
that fits a call must move the reference, on that call's own inputs, by more
than the GPU test tolerates), the attainability of the bound by an f32
emulation of the kernel, the host-only dispatch of the 4-bit path, and the
config validation messages (all before any device call)."""
import functools

import numpy as np
import pytest

import cake_amd
from cake_amd.configs import LLAMA3_8B_GPTQ, MODELS, QUANT_MODELS
from tests import w4_cases as wc
from tests import w4_ref as wr

_id = lambda c: "-".join(map(str, c))
GEMV_CASES = wc.w4_gemv_cases()
GATEUP_CASES = wc.w4_gateup_cases()
DEQUANT_CASES = wc.w4_dequant_cases()


# ---- format -----------------------------------------------------------------
def test_worked_examples_of_the_format():
    # stored zero 15: z + 1 = 16 does not wrap, q = 15 is -1 * s
    q = np.full((8, 8), 15)
    z = np.full((1, 8), 15)
    s = np.full((1, 8), 0.5)
    t = wr.pack_gptq(q, z, s)
    assert t[0].dtype == np.int32 and t[0][0, 0] == -1        # 0xFFFFFFFF
    assert (wr.dequant(*t, 8) == -0.5).all()
    assert (wr.dequant(*t, 8, "z16_wrapped") == 7.5).all()
    # 0xF0000000 is a negative int32; its top nibble is 15, not -1
    qw = np.full((1, 8), -268435456, np.int32)
    qz = np.zeros((1, 1), np.int32)
    W = wr.dequant(qw, qz, np.ones((1, 8), np.float32), 8)
    assert (W[:, 7] == 14).all() and (W[:, :7] == -1).all()
    W = wr.dequant(qw, qz, np.ones((1, 8), np.float32), 8,
                   "top_nibble_signed")
    assert (W[:, 7] == -2).all()


@pytest.mark.parametrize("case", DEQUANT_CASES, ids=_id)
def test_round_trip_pack_unpack_dequant(case):
    N, K, g = case
    for fam in ("exact_sparse", "random"):
        rng = wc._rng("roundtrip", fam, *case)
        G = K // g
        q = rng.integers(0, 16, size=(K, N))
        z = rng.integers(0, 16, size=(G, N))
        s = 2.0 ** rng.integers(-2, 2, size=(G, N)).astype(np.float64)
        qw, qz, sc = wr.pack_gptq(q, z, s)
        assert qw.shape == (K // 8, N) and qz.shape == (G, N // 8)
        q2, z2 = wr.unpack_gptq(qw, qz)
        assert np.array_equal(q, q2) and np.array_equal(z, z2)
        gi = np.arange(K) // g
        W = wr.dequant(qw, qz, sc, g)
        assert np.array_equal(W, ((q - z[gi] - 1) * s[gi]).T)
        # exact in f32: an integer in [-16, 14] times an 11-bit scale
        assert np.array_equal(W.astype(np.float32).astype(np.float64), W)
    t = wc.dequant_inputs("exact_sparse", *case)
    assert (t[0] < 0).any()                      # words with bit 31 set
    _, z = wr.unpack_gptq(t[0], t[1])
    assert (z == 15).any() and (z == 0).any()


# ---- exactness the bit-exact GPU assertions rest on ------------------------
@functools.lru_cache(maxsize=4)
def _gemv_inputs(fam, *case):
    return wc.gemv_inputs(fam, *case)


def _abs_quanta(t, g, x):
    """sum (q + z + 1) s |x| in quanta: bounds every partial sum of the true
    form AND of the kernel's s * sum(q x) + m * sum(x) form."""
    q, z = wr.unpack_gptq(t[0], t[1])
    s = np.asarray(t[2], np.float64)
    gi = np.arange(q.shape[0]) // g
    return (((q + z[gi] + 1) * s[gi]).T @ np.abs(x)) / wc.QUANTUM


@pytest.mark.parametrize("case", GEMV_CASES, ids=_id)
def test_gemv_exact_families_are_exact(case):
    N, K, g, epi, alias, rows, repeats = case
    for fam in wc.FAMILIES[:2]:
        d = _gemv_inputs(fam, *case)
        s = np.asarray(d["t"][2], np.float64)
        assert np.array_equal(np.log2(s), np.rint(np.log2(s)))
        assert s.min() >= wc.QUANTUM
        for i in range(repeats):
            x = d["x"][i].astype(np.float64)
            assert np.array_equal(x, np.rint(x))
            a = _abs_quanta(d["t"], g, x)
            if d["res"] is not None:
                a = a + np.abs(d["res"][i]) / wc.QUANTUM
            assert (a < 2 ** 24).all()
            v, _ = wc.gemv_expect(d, g, i)
            assert np.array_equal(v / wc.QUANTUM, np.rint(v / wc.QUANTUM))


# ---- teeth ------------------------------------------------------------------
def _teeth(mutants, run):
    """Every mutant that fits the call must be caught by AT LEAST ONE input
    family of the call (no single family sees every defect: sparse x is blind
    to most k, dense sums are too large to show one ulp); the GPU test of the
    call runs all of them."""
    missed = [m for m in mutants
              if not any(wc.moved(*run(fam, m)) for fam in wc.FAMILIES)]
    assert not missed, f"mutants that no family of this call catches: {missed}"


@pytest.mark.parametrize("case", GEMV_CASES, ids=_id)
def test_gemv_teeth(case):
    N, K, g, epi, alias, rows, repeats = case
    split = wc.gemv_split(N)
    for i in range(repeats):
        base = {}

        def run(fam, mut):
            d = _gemv_inputs(fam, *case)
            if fam not in base:
                base[fam] = wc.gemv_expect(d, g, i)
            v, A = base[fam]
            got, _ = wc.gemv_expect(d, g, i, mut, split)
            return d["exact"], v, got, wc.TOL_BF16 * A + wc.ABS_EPS
        _teeth(wc.gemv_mutants(N, K, g, epi), run)


@pytest.mark.parametrize("case", GATEUP_CASES, ids=_id)
def test_gateup_teeth(case):
    I, K, g, rows = case
    cache = {}

    def run(fam, mut):
        if fam not in cache:
            d = wc.gateup_inputs(fam, I, K, g)
            cache[fam] = (d, wr.gateup_ref(d["t"], g, d["x"]))
        d, (val, gt, u, Ag, Au) = cache[fam]
        got = wr.gateup_ref(d["t"], g, d["x"], mut)[0]
        return False, val, got, wc.gateup_bound(val, gt, u, Ag, Au)
    _teeth(wc.gateup_mutants(I, K, g), run)


@pytest.mark.parametrize("case", DEQUANT_CASES, ids=_id)
def test_dequant_teeth(case):
    N, K, g = case
    t = wc.dequant_inputs("exact_sparse", N, K, g)
    base = wr.dequant_bf16_bits(*t, g)
    for mut in wc._weight_mutants(N, K, g, wc.gemv_split(N)):
        got = wr.bf16_bits(wr.dequant(*t, g, mut, wc.gemv_split(N)))
        assert (got != base).any(), mut


# ---- the bound is attainable ------------------------------------------------
@pytest.mark.parametrize("case", GEMV_CASES, ids=_id)
def test_f32_emulation_of_the_kernel_stays_within_the_bound(case):
    """Two summation orders of float32 arithmetic, the kernel's own
    s * (sum q x) - (z+1) s * (sum x) form included, on the random family of
    every call (8 rows of it: the orders are per row)."""
    N, K, g, epi, alias, rows, repeats = case
    d = _gemv_inputs("random", *case)
    sub = (d["t"][0][:, :8], d["t"][1][:, :1], d["t"][2][:, :8])
    x = d["x"][0]
    res = d["res"][0][:8] if d["res"] is not None else None
    ref, A = wr.gemv_ref(sub, g, x, res)
    for order in ("kernel", "plain"):
        v = wr.gemv_emulate_f32(sub, g, x, order)
        if res is not None:
            v = (v + res.astype(np.float32)).astype(np.float32)
        got = wr.bf16(v.astype(np.float64))
        err = np.abs(got - ref) / (wc.TOL_BF16 * A + wc.ABS_EPS)
        assert err.max() <= 1.0, (order, err.max())


# ---- host-only dispatch -----------------------------------------------------
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


def test_w4_dispatch_matches_the_policy_and_is_covered_by_the_gpu_cases():
    assert cake_amd.LINEAR_FAMILIES[9:] == ("gemv_w4", "gateup_w4")
    for K, g in wc.GEMV_KG + ((14336, 128),):
        d = cake_amd.linear_dispatch_w4("plain", 64, K, g)
        assert d == dict(family="gemv_w4", rows=4, kb=wc.kb_of(K)), (K, d)
        if K <= 16384:
            d = cake_amd.linear_dispatch_w4("gateup", 64, K, g)
            assert d == dict(family="gateup_w4", rows=4, kb=wc.kb_of(K))
    assert cake_amd.linear_dispatch_w4("plain", 8, 4096, -1)["kb"] == 1
    c = LLAMA3_8B_GPTQ
    assert QUANT_MODELS["llama3-8b-gptq"] is c and "llama3-8b-gptq" not in MODELS
    H, I = c["hidden_size"], c["intermediate_size"]
    got = cake_amd.decode_dispatch(c)
    lw = cake_amd.linear_dispatch_w4
    want = dict(
        qkv=tuple(lw("plain", 6144, H, 128).values()),
        o=tuple(lw("plain", H, 4096, 128).values()),
        gateup=tuple(lw("gateup", I, H, 128).values()),
        down=tuple(lw("plain", H, I, 128).values()),
        head=("gemv_reg", 8, 2))                    # the lm_head stays bf16
    assert got == want
    assert got["qkv"] == ("gemv_w4", 4, 1) and got["down"] == ("gemv_w4", 4, 4)
    # every reached (rows, KB) runs in a GPU case (rows 0 = this policy)
    plain = {(wc.kb_of(K), 4 if rows == 0 else rows)
             for (N, K, g, epi, alias, rows, rep) in GEMV_CASES}
    for k in ("qkv", "o", "down"):
        assert (got[k][2], got[k][1]) in plain, k
    assert got["gateup"] == ("gateup_w4", 4, 1)
    gu = {(wc.kb_of(K), r) for (I_, K, g, r) in GATEUP_CASES}
    assert gu >= {(1, 4), (2, 4), (4, 4), (1, 0)}
    for K, g in wc.GEMV_KG:                 # every instantiated rows value
        ran = {c[5] for c in GEMV_CASES if c[1] == K}
        assert ran >= set(wc.rows_of(K)), K


def test_configured_models_dispatch_as_before():
    assert set(PINNED) == set(MODELS)
    for name, cfg in MODELS.items():
        assert cake_amd.decode_dispatch(cfg) == PINNED[name], name
    d = cake_amd.linear_dispatch
    assert d("plain", 64, 4096) == dict(family="gemv_reg", rows=2, kb=2)
    assert d("plain", 128, 8192, fp8=True) == dict(family="gemv_fp8", rows=4,
                                                   kb=2)


# ---- validation before any device call -------------------------------------
def _gptq(**over):
    c = dict(LLAMA3_8B_GPTQ)
    q = dict(c["quantization_config"])
    for k in [k for k in over if k in ("bits", "desc_act", "group_size")]:
        q[k] = over.pop(k)
    c["quantization_config"] = q
    c.update(over)
    return c


@pytest.mark.parametrize("over,msg", [
    (dict(bits=8), "bits 8"),
    (dict(bits=3), "bits 3"),
    (dict(desc_act=True), "desc_act"),
    (dict(group_size=48), "group_size 48"),
    (dict(group_size=0), "group_size 0"),
    (dict(group_size=1536), r"q_proj in_features 4096 .* group_size 1536"),
    (dict(intermediate_size=14400), r"down_proj in_features 14400"),
    (dict(num_key_value_heads=1, head_dim=4, num_attention_heads=2),
     r"k_proj/v_proj out_features 4"),
    (dict(intermediate_size=32800, group_size=32),
     r"down_proj in_features 32800 outside"),
])
def test_gptq_config_validation_names_the_offender(over, msg):
    E = cake_amd.CakeHipError
    c = _gptq(**over)
    with pytest.raises(E, match=msg):
        cake_amd.decode_dispatch(c)
    if "head_dim" not in over:      # (the head_dim rule of create comes first)
        with pytest.raises(E, match=msg):
            cake_amd.Engine(c)


def test_w4_op_entries_reject_bad_arguments_without_a_device():
    E = cake_amd.CakeHipError
    rng = np.random.default_rng(0)
    t = wc.weights("random", rng, 8, 64, 32)
    x = np.zeros(64, np.float32)
    with pytest.raises(E, match="multiple of 32"):
        cake_amd.op_gemv_w4(x, t[0], np.zeros((4, 1), np.int32),
                            np.zeros((4, 8), np.float32), 16)
    with pytest.raises(E, match="rows"):
        cake_amd.op_gemv_w4(x, *t, 32, rows=2)
    with pytest.raises(E, match="res goes with epi 1"):
        cake_amd.op_gemv_w4(x, *t, 32, epi=1)
    with pytest.raises(E, match="alias"):
        cake_amd.op_gemv_w4(x, *t, 32, alias=True)
    with pytest.raises(E, match="repeats"):
        cake_amd.op_gemv_w4(np.zeros((17, 64), np.float32), *t, 32)
    t12 = wc.weights("random", rng, 24, 64, 32)
    with pytest.raises(E, match="multiple of 8"):      # I = 12
        cake_amd.op_gemv_gateup_w4(x, *t12, 32)
    with pytest.raises(E, match="4 rows"):
        cake_amd.op_gemv_gateup_w4(x, *wc.weights("random", rng, 16, 64, 32),
                                   32, rows=8)
    with pytest.raises(E, match="not a multiple of group_size"):
        cake_amd.op_dequant_w4(np.zeros((12, 8), np.int32),
                               np.zeros((1, 1), np.int32),
                               np.zeros((1, 8), np.float32), 64)
    big = 16416
    with pytest.raises(E, match="rows 8 needs"):
        cake_amd.op_gemv_w4(np.zeros(big, np.float32),
                            *wc.weights("random", rng, 8, big, 32), 32,
                            rows=8)
    with pytest.raises(E, match="cake_hip_linear_dispatch_w4"):
        cake_amd._check(cake_amd._lib.cake_hip_linear_dispatch(
            0, 64, 4096, 1, 2, (cake_amd.ctypes.c_int * 5)()))
