"""Op tests of the gemma3 kernels (kernels_gemma.hip) against float64: the
post-norm + residual add in both launch forms, the GELU-tanh gate-up GEMV and
gelu_mul_rows, and the scaled embedding gathers.  Tolerances are those of the
sibling kernels' tests (tests/test_linear_ops_gpu.py, tests/linear_cases.py):
one bf16 rounding per stored value plus the f32 error terms of the sums.  One
test runs on the CPU: the gate-up case list tells GELU from SiLU."""
import numpy as np
import pytest

import cake_amd
from tests import linear_cases as lc
from tests import linear_ref as lr

gpu = pytest.mark.gpu
EPS = 1e-6
SENT = cake_amd.OP_SENTINEL

POSTNORM_H = (8, 1152, 5376, 16384)
POSTNORM_S = (1, 3, 17)          # 1: the decode launch; the others: prefill
GATEUP_I = (4, 5, 36)            # whole blocks, a ragged last block, many
GATEUP_K = (8, 1152, 2560, 5376)  # one vector; the 1B, 4B and 27B widths
GELU_ROWS = ((1, 8), (1, 36), (5, 8), (5, 36))   # 36: the scalar loop


def gelu_tanh64(g):
    g = np.asarray(g, dtype=np.float64)
    return 0.5 * g * (1.0 + np.tanh(np.sqrt(2.0 / np.pi) *
                                    (g + 0.044715 * g ** 3)))


def _guards_ok(g):
    return np.array_equal(lr.f32_bits(g), lr.f32_bits(np.full_like(g, SENT)))


# ---- post-norm + residual ---------------------------------------------------------
def postnorm_ref(x, t, w, eps):
    """(x + n, n) in float64, n = t rsqrt(mean t^2 + eps) w per row."""
    t = t.astype(np.float64)
    n = t / np.sqrt(np.mean(t * t, axis=-1, keepdims=True) + eps) * \
        w.astype(np.float64)
    return x.astype(np.float64) + n, n


def postnorm_bound(s, n, x):
    """The kernel rounds n to bf16 (half an ulp of n), adds x in f32 and
    rounds the sum (half an ulp of the sum, taken at |s| + ulp(n) so that a
    sum pushed over a binade edge by the first rounding is covered); the f32
    scale, products and sum stay under 2^-20 (|n| + |x|)."""
    un = lc.bf16_ulp(n)
    return 0.5 * un + 0.5 * lc.bf16_ulp(np.abs(s) + un) + \
        2.0 ** -20 * (np.abs(n) + np.abs(x)) + lc.ABS_EPS


@gpu
@pytest.mark.parametrize("H", POSTNORM_H)
@pytest.mark.parametrize("S", POSTNORM_S)
def test_postnorm_add(S, H):
    rng = lc._rng("postnorm", S, H)
    x = lc._q(rng.standard_normal((S, H)))
    t = lc._q(rng.standard_normal((S, H)) * 2.0 ** rng.integers(-6, 4, (S, 1)))
    w = lc._q(1.0 + 0.2 * rng.standard_normal(H))
    out, g = cake_amd.op_postnorm_add(x, t, w, eps=EPS)
    assert _guards_ok(g), "a guard element past the output was written"
    s, n = postnorm_ref(x, t, w, EPS)
    ratio = np.abs(out.astype(np.float64) - s) / postnorm_bound(s, n, x)
    worst = np.inf if np.isnan(out).any() else float(ratio.max())
    print(f"postnorm_add S {S} H {H}: worst err/bound {worst:.3f}")
    assert worst <= 1.0
    # bf16(x + n) without the inner rounding differs somewhere on a row this
    # long: the test can tell HF's two rounding points from one
    if H >= 1152:
        assert (lr.bf16(s) != lr.bf16(x.astype(np.float64) + lr.bf16(n))).any()


# ---- GELU gate-up GEMV --------------------------------------------------------------
def gateup_gelu_bound(val, g, u, Ag, Au):
    """lc.gateup_bound with the GELU-tanh gate: |gelu_tanh'| <= 1.13."""
    return (lc.TOL_BF16 * np.abs(val) + lc.TOL_F32 * (
        1.13 * Ag * np.abs(u) + np.abs(gelu_tanh64(g)) * Au) + lc.ABS_EPS)


def _gateup_cases():
    for I in GATEUP_I:
        for K in GATEUP_K:
            for norm in (False, True):
                d = lc.gateup_inputs("random", False, I, K, norm)
                _, g, u, Ag, Au = lr.gateup_ref(d["W64"], d["x"], I, d["nw"],
                                                lc.EPS)
                yield I, K, norm, d, g, u, Ag, Au


def test_gateup_cases_tell_gelu_from_silu():
    """CPU: on every (I, K, norm) case the SiLU product of the same sums
    misses the GELU bound somewhere, so a kernel with the wrong gate fails."""
    n = 0
    for I, K, norm, d, g, u, Ag, Au in _gateup_cases():
        val = gelu_tanh64(g) * u
        bound = gateup_gelu_bound(val, g, u, Ag, Au)
        assert (np.abs(lr.bf16(lr.silu(g) * u) - val) > bound).any(), \
            (I, K, norm)
        assert (np.abs(lr.bf16(val) - val) <= bound).all()
        n += 1
    assert n == len(GATEUP_I) * len(GATEUP_K) * 2


@gpu
@pytest.mark.parametrize("K", GATEUP_K)
@pytest.mark.parametrize("I", GATEUP_I)
def test_gateup_gelu(I, K):
    fails = []
    for I_, K_, norm, d, g, u, Ag, Au in _gateup_cases():
        if (I_, K_) != (I, K):
            continue
        val = gelu_tanh64(g) * u
        bound = gateup_gelu_bound(val, g, u, Ag, Au)
        for rows in (4, 8):
            out, gd = cake_amd.op_gemv_gateup_gelu(
                d["x"], d["w"], I, nw=d["nw"] if norm else None, eps=lc.EPS,
                rows=rows)      # lc.EPS: the inputs are tie-safe under it
            tag = f"I {I} K {K} norm {norm} rows {rows}"
            if not _guards_ok(gd):
                fails.append(f"{tag}: a guard element was written")
            ratio = np.abs(out.astype(np.float64) - val) / bound
            worst = np.inf if np.isnan(out).any() else float(ratio.max())
            print(f"gateup_gelu {tag}: worst err/bound {worst:.3f}")
            if not worst <= 1.0:
                fails.append(f"{tag}: err/bound {worst:.3f}")
    assert not fails, "\n".join(fails)


# ---- gelu_mul_rows --------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("S,I", GELU_ROWS)
def test_gelu_mul_rows(S, I):
    """Within one bf16 ulp of the float64 product, the rule silu_mul_rows is
    held to on plain random inputs (|gate| <= 3, as there)."""
    gu = lc.silu_rows_inputs(S, I, False)
    out, g = cake_amd.op_gelu_mul_rows(gu)
    assert _guards_ok(g)
    ref = gelu_tanh64(gu[:, :I]) * gu[:, I:].astype(np.float64)
    worst = float(np.max(np.abs(out - lr.bf16(ref)) / lc.bf16_ulp(ref)))
    print(f"gelu_mul_rows S {S} I {I}: worst {worst:.3f} bf16 ulp")
    assert worst <= 1.0
    silu = lr.bf16(lc.silu_rows_ref(gu))
    assert (np.abs(silu - lr.bf16(ref)) > lc.bf16_ulp(ref)).any()


# ---- scaled embedding -----------------------------------------------------------------
@gpu
@pytest.mark.parametrize("mode", ["rows", "token"])
def test_embed_scaled(mode):
    """Bit for bit bf16(row * bf16(sqrt(H))): a product of two bf16 values is
    exact in f32, so there is one rounding.  At H 1152 bf16(sqrt(H)) = 34 and
    sqrt(H) = 33.94: the rule with the unrounded scale gives other values."""
    H, Vt = 1152, 7
    rng = lc._rng("embed_scaled", mode)
    table = lc._q(rng.standard_normal((Vt, H)))
    ids = np.array([6, 0, 3, 3, 5] if mode == "rows" else [4], dtype=np.uint32)
    out, g = cake_amd.op_embed_scaled(table, ids, mode=mode)
    assert _guards_ok(g)
    sb = float(lr.bf16(np.sqrt(np.float64(H))))
    assert sb == 34.0 and sb != np.sqrt(H)
    want = lr.bf16(table[ids].astype(np.float64) * sb)
    assert np.array_equal(lr.f32_bits(out), lr.f32_bits(want.astype(np.float32)))
    other = lr.bf16(table[ids].astype(np.float64) * np.sqrt(np.float64(H)))
    assert (other != want).any()
