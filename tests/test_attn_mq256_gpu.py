"""Op-level GPU parity (-m gpu) of the hd-256 grouped MFMA decode-attention
kernel (k_attn_decode_mq256; CAKE_ATTN_MQ256=1) against the float64 reference,
with test_attn_mq_gpu.py's checks and bound |got - ref| <= TOL_F32P * A +
ABS_EPS: P enters the P.V MFMA as bf16 hi + bf16 lo, below 2^-16 relative."""
import numpy as np
import pytest

import cake_amd
from tests import attn_cases as ac
from tests.attn_ref import attn_ref
from tests.test_attn_mq_gpu import _bits, _bound_fails

pytestmark = pytest.mark.gpu

HD = 256
# the models' ratios, 3 over two kv heads, 16 (no padding rows), 1, 5
GEOMS = [(2, 1), (3, 1), (4, 1), (8, 4), (6, 2), (16, 1), (1, 1), (5, 1)]
# 1, 2, around the wave step (16) and the block step (64), several block steps
NS = (1, 2, 15, 16, 17, 63, 64, 65, 129, 300, 2100)
NCHUNKS, WINDOWS = (1, 4, 8, 24, 64), (0, 1, 33, 64, 96)
# pruned cross (three cyclic picks per geometry cover every n, nchunk, window),
# then: more chunks than positions, 2100 in one chunk, a window in 64 chunks
CASES = [g + (NS[(3 * gi + i) % 11], NCHUNKS[(gi + i) % 5],
              WINDOWS[(2 * gi + i) % 5])
         for gi, g in enumerate(GEOMS) for i in range(3)] + [
    (3, 1, 1, 64, 0), (8, 4, 2, 64, 0), (4, 1, 2100, 1, 0),
    (8, 4, 2100, 4, 0), (6, 2, 2100, 64, 96), (2, 1, 300, 4, 0)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_decode_mq256(case, monkeypatch):
    nh, nkv, n, nchunk, window = case
    monkeypatch.setenv("CAKE_ATTN_MQ256", "1")
    assert cake_amd.attn_decode_path(nh, nkv, HD, nchunk) == 5
    assert cake_amd.attn_decode_group(nh, nkv, HD) == nh // nkv
    pos, max_seq = n - 1, ac.decode_max_seq(n)
    lo = n - window if (window and n > window) else 0
    fails = []
    for fam in ac.FAMILIES:
        q, kc, vc = ac.make_inputs(fam, nh, nkv, HD, max_seq, 1, pos, window,
                                   decode=True)
        ref, A = attn_ref(q, kc, vc, pos, window)
        outs = [cake_amd.op_attn_decode(q[0], *ac.set_stale(kc, vc, lo, n,
                                                            fill)[:2],
                                        pos, window, nchunk, repeats=3)
                for fill in (0, ac.STALE)]
        if not np.array_equal(_bits(outs[0]), _bits(outs[1])):
            fails.append(f"{fam}: output depends on slots outside [{lo},{n})")
        if not (np.array_equal(_bits(outs[0][0]), _bits(outs[0][1])) and
                np.array_equal(_bits(outs[0][0]), _bits(outs[0][2]))):
            fails.append(f"{fam}: repeats on one zeroing differ")
        fails += _bound_fails(fam, outs[0][0:1], ref, A)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("geom", [(3, 1), (8, 4)], ids=["3-1", "8-4"])
def test_decode_mq256_changing_nchunk(geom, monkeypatch):
    """Changing chunk counts on one zeroing: each launch right, counters 0."""
    nh, nkv = geom
    monkeypatch.setenv("CAKE_ATTN_MQ256", "1")
    n, seq = 300, [4, 8, 24, 8, 64, 1, 4]
    q, kc, vc = ac.make_inputs("peaky", nh, nkv, HD, 320, 1, n - 1, 0,
                               decode=True)
    ref, A = attn_ref(q, kc, vc, n - 1, 0)
    out, cnt = cake_amd.op_attn_decode_seq(q[0], kc, vc, n - 1, seq, 0)
    fails = []
    for i, c in enumerate(seq):
        fails += _bound_fails(f"launch {i} (nchunk {c})", out[i:i + 1], ref, A)
    assert not fails, "\n".join(fails)
    assert np.array_equal(_bits(out[0]), _bits(out[6]))
    assert not np.asarray(cnt).any(), cnt
