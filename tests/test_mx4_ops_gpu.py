"""GPU parity tests (-m gpu) of the MXFP4 kernels through their op entries
against the float64 reference of tests/mx4_ref.py.  K: one block, both sides of
every KB edge with a 32 tail, the largest; N 5 / 24 / 41: row tails of the
4-row blocks and of the 2-row halves at KB 1; N K <= 1.2 M.
Exact family: x = +-1, scale bytes 125..128 per (row, block), uniform codes,
integer residuals: every term is a multiple of 2^-3 and sum |.| <= 32768 * 6 *
2 * 8 quanta < 2^24, so any f32 order is exact and the output must equal
RNE-to-bf16 of the float64 sum bit for bit.  Random family: Gaussian bf16 x,
scale bytes 117..121: |got - ref| <= 2^-8 A + 2^-40 (the
in-register dequant is exact).  Gate-up: w4_cases.gateup_bound.  Dequant: every
element bit-exact.  Every output: guards intact, no sentinel left."""
import numpy as np
import pytest

import cake_amd
from tests import mx4_ref as mr
from tests.helpers import quantize_bf16
from tests.test_w4_ops_gpu import _clean, _id
from tests.w4_cases import ABS_EPS, TOL_BF16, _rng, gateup_bound, got_bits

pytestmark = pytest.mark.gpu

KS = (32, 4064, 4096, 4128, 8192, 8224, 16384, 16416, 32768)
NS = (5, 24, 41)
MODES = ((0, False), (1, False), (1, True))         # (epi, alias)
VARIANTS = ("f32", "dot2")
GEMV_CASES = [(next(n for n in (NS[(i + m) % 3], 24, 5) if n * K <= 1_200_000),
               K, epi, alias)
              for i, K in enumerate(KS) for m, (epi, alias) in enumerate(MODES)]
GATEUP_CASES = [(I, K) for K in KS if K <= 16384 for I in (5, 24)]


def _inputs(key, N, K, exact):
    """(rng, (weight, weight_scale), x) of one family."""
    rng = _rng("mx4", key, N, K, exact)
    lo, hi = (125, 129) if exact else (117, 122)
    t = mr.pack(rng.integers(0, 16, size=(N, K)),
                rng.integers(lo, hi, size=(N, K // 32)))
    x = rng.choice([-1.0, 1.0], size=K) if exact else rng.standard_normal(K)
    return rng, t, quantize_bf16(x.astype(np.float32))


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("case", GEMV_CASES, ids=_id)
def test_gemv_mx4(case, variant):
    N, K, epi, alias = case
    for exact in (True, False):
        rng, t, x = _inputs(case, N, K, exact)
        res = None
        if epi == 1 and exact:
            res = rng.integers(-40, 41, size=N).astype(np.float32)
        elif epi == 1:                      # a residual the size of the product
            v = mr.gemv_ref(*t, x)[0]
            res = quantize_bf16((np.sqrt(np.mean(v * v)) *
                                 rng.standard_normal(N)).astype(np.float32))
        out, guards = cake_amd.op_gemv_mx4(
            x, *t, epi=epi, alias=alias, variant=variant,
            res=None if res is None else res[None])
        _clean(out, guards)
        ref, A = mr.gemv_ref(*t, x, res)
        if exact:
            bad = got_bits(out[0]) != mr.bf16_bits(ref)
            assert not bad.any(), (np.flatnonzero(bad)[:8], out[0][bad][:8],
                                   ref[bad][:8])
        else:
            err = np.abs(out[0] - ref) / (TOL_BF16 * A + ABS_EPS)
            print(f"gemv_mx4 {case} {variant}: err/bound {err.max():.3f}")
            assert err.max() <= 1.0, err.max()


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("case", GATEUP_CASES, ids=_id)
def test_gateup_mx4(case, variant):
    I, K = case
    for exact in (True, False):
        _, t, x = _inputs(case, 2 * I, K, exact)
        if exact:   # 2^-6: gate sums stay in silu's curved range
            x = x * np.float32(2.0 ** -6)
        out, guards = cake_amd.op_gemv_gateup_mx4(x, *t, variant=variant)
        _clean(out, guards)
        val, g, u, Ag, Au = mr.gateup_ref(*t, x)
        err = np.abs(out - val) / gateup_bound(val, g, u, Ag, Au)
        print(f"gateup_mx4 {case} {variant} {exact}: err/bound {err.max():.3f}")
        assert err.max() <= 1.0, err.max()


@pytest.mark.parametrize("case", [(5, 32), (24, 4128), (41, 8224)], ids=_id)
def test_dequant_mx4(case):
    N, K = case
    rng = _rng("mx4dequant", case)
    codes = rng.integers(0, 16, size=(N, K))
    # bytes up to 180: no weight equals the sentinel -2^60
    sb = rng.integers(1, 181, size=(N, K // 32))
    # an all-zero block stored at byte 0; code 1 (0.5) at the smallest scale
    # (a subnormal bf16) and at a large one
    for row, byte, code in ((0, 0, 0), (N // 2, 1, 1), (N - 1, 250, 1)):
        sb[row, -1] = byte
        codes[row, K - 32:] = code
    t = mr.pack(codes, sb)
    out, guards = cake_amd.op_dequant_mx4(*t)
    _clean(out, guards)
    bad = got_bits(out) != mr.bf16_bits(mr.dequant(*t))
    assert not bad.any(), np.argwhere(bad)[:8]
