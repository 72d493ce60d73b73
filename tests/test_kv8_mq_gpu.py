"""Op-level GPU parity (-m gpu) of the grouped MFMA decode attention over the
fp8 KV cache (k_attn_decode_kv8_mq, kernels_kv8_mq.hip) against the float64
reference over code * scale, on the cases of tests/test_kv8_ops_gpu.py:
|got - ref| <= TOL_F32P * A + ABS_EPS element-wise.  The bound's derivation
carries over: the codes convert to bf16 exactly, their products accumulate in
f32, P enters P.V as bf16 hi + bf16 lo, and both scale multiplies are by powers
of two.  Rows outside the span hold NaN codes and 2^60 scales, so a read
outside [lo, n) or outside a block's chunk shows as NaN."""
import numpy as np
import pytest

import cake_amd
from tests.attn_cases import ABS_EPS, TOL_F32P
from tests.test_kv8_ops_gpu import decode_case

pytestmark = pytest.mark.gpu

# G = 1, 3, 4, 7, 4 and 7 on two kv heads, 16 (no padding rows)
GEOMS = [(1, 1), (3, 1), (4, 1), (7, 1), (8, 2), (14, 2), (16, 1)]
NS = (1, 2, 31, 32, 33, 64, 65, 129, 300, 2100)
NCHUNKS = (1, 4, 8, 24, 64)
WINDOWS = (0, 1, 33, 65, 129)
# pruned cross: every n, nchunk and window appears (three cyclic picks per
# geometry), then the corners: more chunks than positions, several 128-position
# steps per wave with a partial last one, a windowed span cut into 64 chunks,
# 300 positions in 4 chunks
CASES = [g + (NS[(3 * gi + i) % 10], NCHUNKS[(gi + i) % 5],
              WINDOWS[(2 * gi + i) % 5])
         for gi, g in enumerate(GEOMS) for i in range(3)] + [
    (7, 1, 1, 64, 0), (14, 2, 2, 64, 0), (7, 1, 2100, 1, 0),
    (8, 2, 2100, 64, 129), (3, 1, 300, 4, 0)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_decode_kv8_mq(case):
    nh, nkv, n, nchunk, window = case
    fails = []
    for fam in ("peaky", "flat"):
        q, k8, v8, ks, vs, ref, A = decode_case(fam, nh, nkv, n, window)
        got = cake_amd.op_attn_decode_kv8(q, k8, v8, ks, vs, n - 1,
                                          window=window, nchunk=nchunk,
                                          repeats=3, mq=True)
        ratio = np.abs(got[0] - ref) / (TOL_F32P * A + ABS_EPS)
        worst = np.inf if np.isnan(ratio).any() else float(ratio.max())
        print(f"{fam}: max err / bound = {worst:.3f}")
        if not worst <= 1.0:
            fails.append(f"{fam}: err / bound = {worst:.3f}")
        for r in (1, 2):  # one zeroing of the counters serves every launch
            if not np.array_equal(got[0].view(np.uint32),
                                  got[r].view(np.uint32)):
                fails.append(f"{fam}: launch {r} differs from launch 0")
    assert not fails, "\n".join(fails)
