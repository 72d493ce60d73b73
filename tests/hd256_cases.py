"""Shapes of the head_dim-256 tests, shared by the GPU half
(test_hd256_ops_gpu.py) and the CPU half (test_hd256_ref.py), so that the teeth
condition is checked on exactly the inputs the GPU sees.  Inputs, families and
tolerances are those of tests/attn_cases.py and tests/linear_cases.py."""
from tests import attn_cases as ac
from tests import linear_cases as lc

HD = 256

# ---- decode: k_attn_decode_256<GB>, tile 64 ---------------------------------
# (nh, nkv): G = 2, 3, 4 (one group), 2 with four kv heads, 3 with two, 1, and
# 5 (no divisor among 4 | 3 | 2: per head)
DEC_GEOM = ((2, 1), (3, 1), (4, 1), (8, 4), (6, 2), (1, 1), (5, 1))
DEC_NCHUNKS = (1, 2, 4, 8, 24, 32, 48, 64)
DEC_SPECIALS = [            # those of attn_cases.DEC_G_CASES
    (300, 4, 0), (1, 64, 0), (2100, 64, 0), (2100, 48, 96), (129, 32, 64),
    (65, 2, 64), (65, 1, 65), (64, 8, 63)]
# (nh, nkv, hd, n, nchunk, window)
DEC_CASES = ac._decode_cases([g + (HD,) for g in DEC_GEOM], DEC_NCHUNKS,
                             DEC_SPECIALS)
# q-heads per block by G (the largest of 4, 3, 2, 1 that divides G)
GROUP_OF_G = {2: 2, 3: 3, 4: 4, 5: 1, 6: 3, 8: 4, 1: 1, 7: 1}
# nchunk sequences on one set of counters (op_attn_decode_seq)
DEC_SEQS = ((24, 48, 24, 64, 1, 2), (4, 8, 4, 32, 48, 48))

# ---- prefill: (nh, nkv, S, pos0, window, max_seq) ---------------------------
# attn_cases' MFMA shapes, except that (4, 2, 1, 45, 0, 64) has no teeth at
# hd 256 (mult64_dropped on the peaky family: 1.49) and runs at pos0 65
_SWAP = {(4, 2, 1, 45, 0, 64): (4, 2, 1, 65, 0, 96)}
PF_CASES = [_SWAP.get(c, c) for c in ac.PF_MFMA_ALL + ac.PF_MFMA_EXTRA] + [
    (3, 1, 33, 45, 40, 96), (6, 2, 129, 64, 33, 224), (12, 4, 65, 0, 0, 96)]
PF_MFMA = (1, 4, 0, 0)      # k_attn_prefill_mfma_256, held to TOL_MFMA
PF_PLAIN = (0, 0, 0, 0)     # k_attn_prefill_256, held to TOL_F32P

# ---- stores and linear kernels ----------------------------------------------
STORE_GEOM = ((2, 1, HD), (12, 4, HD))
STORE_MAX_SEQ = 96
STORE_PREFILL = ((1, 0), (5, 45), (33, 0), (33, 63))     # (S, pos0)
STORE_DECODE_POS = (0, 45, 95)
ROPE_K = lc.ROPE_K                                        # KB 1, 2, 4, 8
ROPE_POS = (0, 45, lc.ROPE_MAX_SEQ - 1)
NEW_GEMV_K = (9216, 23040)   # Falcon3-3B's and -7B's intermediate sizes


def rope_cases():
    """(nh, nkv, hd, K, pos): every K and every pos for both geometries."""
    out = []
    for gi, g in enumerate(STORE_GEOM):
        for ki, K in enumerate(ROPE_K):
            out.append(g + (K, ROPE_POS[(gi + ki) % len(ROPE_POS)]))
        out.append(g + (ROPE_K[0], ROPE_POS[(gi + 2) % len(ROPE_POS)]))
    return out
