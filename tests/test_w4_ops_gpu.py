"""GPU parity tests (-m gpu) of the GPTQ 4-bit kernels through their op
entries: k_gemv_w4, k_gemv_gateup_w4 and k_dequant_w4 against the float64
reference of tests/w4_ref.py, on the calls and inputs of tests/w4_cases.py
(whose teeth tests/test_w4_ref.py proves on the CPU).  The op entries take
checkpoint-layout tensors and repack them with the loader's own routine, so
the repack is under test with the kernels.

Exact families: bit for bit RNE-to-bf16 of the exact sum.  Random family:
|got - ref| <= 2^-8 A + 2^-40 (GEMV), the gate-up bound of
tests/linear_cases.py (gate-up).  Dequant: every element bit-exact.  Every
output: guards intact, no sentinel left in the payload.

The dequant kernel's grid-stride loop wraps only past 8.4 M weights; no case
is that large (cases stay below ~1.2 M weights), so the wrap is covered by the
engine's prefill at model sizes only."""
import numpy as np
import pytest

import cake_amd
from tests import w4_cases as wc
from tests import w4_ref as wr

pytestmark = pytest.mark.gpu
_id = lambda c: "-".join(map(str, c))


def _clean(out, guards):
    assert (guards == cake_amd.OP_SENTINEL).all(), "a guard was overwritten"
    assert not (out == cake_amd.OP_SENTINEL).any(), "an element was not written"


@pytest.mark.parametrize("case", wc.w4_gemv_cases(), ids=_id)
def test_gemv_w4(case):
    N, K, g, epi, alias, rows, repeats = case
    for fam in wc.FAMILIES:
        d = wc.gemv_inputs(fam, *case)
        out, guards = cake_amd.op_gemv_w4(d["x"], *d["t"], g, epi=epi,
                                          res=d["res"], rows=rows,
                                          alias=alias)
        _clean(out, guards)
        for i in range(repeats):
            ref, A = wc.gemv_expect(d, g, i)
            if d["exact"]:
                bad = wc.got_bits(out[i]) != wr.bf16_bits(ref)
                assert not bad.any(), (fam, i, np.flatnonzero(bad)[:8],
                                       out[i][bad][:8], ref[bad][:8])
            else:
                err = np.abs(out[i] - ref) / (wc.TOL_BF16 * A + wc.ABS_EPS)
                print(f"gemv_w4 {case} repeat {i}: err/bound {err.max():.3f}")
                assert err.max() <= 1.0, (fam, i, err.max())


@pytest.mark.parametrize("case", wc.w4_gateup_cases(), ids=_id)
def test_gateup_w4(case):
    I, K, g, rows = case
    for fam in wc.FAMILIES:
        d = wc.gateup_inputs(fam, I, K, g)
        out, guards = cake_amd.op_gemv_gateup_w4(d["x"], *d["t"], g,
                                                 rows=rows)
        _clean(out, guards)
        val, gt, u, Ag, Au = wr.gateup_ref(d["t"], g, d["x"])
        err = np.abs(out - val) / wc.gateup_bound(val, gt, u, Ag, Au)
        print(f"gateup_w4 {case} {fam}: err/bound {err.max():.3f}")
        assert err.max() <= 1.0, (fam, err.max())


@pytest.mark.parametrize("case", wc.w4_dequant_cases(), ids=_id)
def test_dequant_w4(case):
    N, K, g = case
    for fam in ("exact_sparse", "random"):
        t = wc.dequant_inputs(fam, N, K, g)
        out, guards = cake_amd.op_dequant_w4(*t, g)
        _clean(out, guards)
        bad = wc.got_bits(out) != wr.dequant_bf16_bits(*t, g)
        assert not bad.any(), (fam, np.argwhere(bad)[:8])
