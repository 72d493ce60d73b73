"""Shapes and seeded inputs shared by the GPU attention op tests
(test_attn_ops_gpu.py) and the CPU teeth tests (test_attn_ref.py), so the
teeth condition is checked on exactly the inputs the GPU sees."""
import zlib

import numpy as np

from tests.helpers import quantize_bf16

# |got - ref| <= tol * A + ABS_EPS, element-wise, A = P.|V|.  Derived, not
# measured: one bf16 round-to-nearest costs <= 2^-8 relative.  The MFMA
# prefill kernels round P to bf16 and the output to bf16 (worst 2^-7 * A);
# the decode kernels and the generic prefill keep P in f32 (worst 2^-8 * A).
# tol is twice the derived worst case (covers __expf, rescale, f32 order).
TOL_MFMA = 2.0 ** -6
TOL_F32P = 2.0 ** -7
ABS_EPS = 2.0 ** -40

FAMILIES = ("peaky", "ramp_up", "ramp_down", "flat")
STALE = 2.0 ** 60


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def make_inputs(family, nh, nkv, hd, max_seq, S, pos0, window, decode=False):
    """Seeded bf16-exact q (S, nh, hd), kc, vc (nkv, max_seq, hd).  EVERY
    slot carries family content (a longer earlier sequence, in product
    terms); set_stale() overwrites the invisible slots."""
    rng = np.random.default_rng(
        _seed(family, nh, nkv, hd, max_seq, S, pos0, window, decode))
    G = nh // nkv
    j = np.arange(max_seq)
    if family == "peaky":
        # score std ~ 4: a few keys dominate each softmax and their identity
        # changes from tile to tile, so running max and rescale really move
        q = 2.0 * rng.standard_normal((S, nh, hd))
        kc = 2.0 * rng.standard_normal((nkv, max_seq, hd))
        vc = rng.standard_normal((nkv, max_seq, hd))
        if decode:
            # one q row per head: plant the keys at multiples of 32 on it
            # (head (j/32) % G of each group, score ~ 14) so tile-boundary
            # keys carry weight whatever the context length
            for g in range(nkv):
                for jj in range(0, max_seq, 32):
                    qh = quantize_bf16(q[0, g * G + (jj // 32) % G])
                    kc[g, jj] = qh * (14.0 * np.sqrt(hd) / np.sum(qh * qh))
    elif family in ("ramp_up", "ramp_down"):
        # identical q rows, k_j proportional to j: score_j = +-beta * j with
        # beta = 4 * delta / sqrt(hd) ~ 0.25.  j = 64a + b is split over two
        # dims so every entry is bf16-exact up to j = 4095.
        delta = 2.0 ** np.round(np.log2(0.25 * np.sqrt(hd) / 4.0))
        sgn = 1.0 if family == "ramp_up" else -1.0
        q = np.zeros((S, nh, hd))
        q[:, :, 0] = q[:, :, 1] = 4.0
        kc = np.zeros((nkv, max_seq, hd))
        kc[:, :, 0] = sgn * delta * 64.0 * (j // 64)
        kc[:, :, 1] = sgn * delta * (j % 64)
        kc[:, :, 2:] = rng.standard_normal((nkv, max_seq, hd - 2))
        vc = rng.standard_normal((nkv, max_seq, hd))
    elif family == "flat":
        # q = 0: the output is the exact mean of V over the visible set
        q = np.zeros((S, nh, hd))
        kc = rng.standard_normal((nkv, max_seq, hd))
        vc = rng.choice([-1.0, 1.0], size=(nkv, max_seq, hd))
    else:
        raise ValueError(family)
    f = lambda a: quantize_bf16(a.astype(np.float32))
    return f(q), f(kc), f(vc)


def set_stale(kc, vc, lo, hi, fill):
    """Copy of (kc, vc, vtc) with every slot outside [lo, hi) set to 0
    (fill=0) or to +-2^60 with seeded signs."""
    kc, vc = kc.copy(), vc.copy()
    out = np.ones(kc.shape[1], dtype=bool)
    out[lo:hi] = False
    if fill == 0:
        kc[:, out] = 0.0
        vc[:, out] = 0.0
    else:
        rng = np.random.default_rng(_seed("stale", kc.shape, lo, hi))
        sk = rng.choice([-fill, fill], size=kc.shape).astype(np.float32)
        sv = rng.choice([-fill, fill], size=vc.shape).astype(np.float32)
        kc[:, out] = sk[:, out]
        vc[:, out] = sv[:, out]
    return kc, vc, np.ascontiguousarray(vc.transpose(0, 2, 1))


def round_up32(n):
    return (n + 31) // 32 * 32


# ---- MFMA prefill (hd 128; KV tile 32, 32 q rows per wave) -----------------
# (nh, nkv, S, pos0, window, max_seq)
PF_MFMA_ALL = [           # every variant runs these
    (4, 2, 33, 45, 40, 96),
    (2, 1, 257, 0, 0, 288),
    (8, 1, 129, 64, 33, 224),
    (2, 1, 31, 1, 0, 32),     # pos0 + S == max_seq: last tile ends the cache
]
PF_MFMA_EXTRA = [         # plain NW=4 / NW=8 / v1 only
    (4, 2, 1, 0, 1, 32),
    (2, 1, 32, 64, 32, 96),   # pos0 + S == max_seq
    (4, 2, 1, 45, 0, 64),
    (8, 1, 32, 1, 33, 64),
]
# (pfv, nw, split, deep)
PF_VARIANTS = [(2, nw, sp, dp) for nw in (4, 8)
               for sp, dp in ((0, 0), (1, 0), (0, 1), (0, 2))] + [(1, 8, 0, 0)]
PF_MFMA_CASES = [(v, c) for v in PF_VARIANTS for c in PF_MFMA_ALL] + [
    (v, c) for v in ((2, 4, 0, 0), (2, 8, 0, 0), (1, 8, 0, 0))
    for c in PF_MFMA_EXTRA]

# ---- generic prefill (hd != 128; one wave per row, 4 rows per block) -------
# (hd, nh, nkv, S, pos0, window); max_seq 128
PF_GENERIC_CASES = [
    (8, 2, 1, 1, 0, 0), (8, 4, 2, 5, 45, 24), (8, 8, 1, 77, 0, 1),
    (40, 4, 2, 3, 45, 0), (40, 8, 1, 77, 45, 24), (40, 2, 1, 4, 0, 1),
    (64, 8, 1, 4, 45, 24), (64, 2, 1, 77, 0, 0), (64, 4, 2, 1, 45, 1),
    (96, 2, 1, 5, 0, 0), (96, 4, 2, 3, 45, 1), (96, 8, 1, 77, 45, 24),
]

# ---- decode ----------------------------------------------------------------
DEC_N = (1, 2, 63, 64, 65, 128, 129, 300, 2100)
DEC_WINDOWS = (0, 1, 63, 64, 65, 96)


def _decode_cases(configs, nchunks, specials):
    """Pruned cross product: every n, every nchunk and every window appears
    for every config (two cyclic passes with config-dependent offsets)."""
    out = []
    for g, cfg in enumerate(configs):
        seen = set()
        trip = [(DEC_N[i], nchunks[(i + g) % len(nchunks)],
                 DEC_WINDOWS[(i + 2 * g) % 6]) for i in range(len(DEC_N))]
        trip += [(DEC_N[(2 * i + g) % 9], nchunks[i % len(nchunks)],
                  DEC_WINDOWS[(i + g + 3) % 6]) for i in range(8)]
        for t in trip + list(specials):
            if t not in seen:
                seen.add(t)
                out.append(cfg + t)
    return out


# grouped kernel (hd 128, tile 64): (nh, nkv, hd) + (n, nchunk, window);
# nchunk * grid_y <= 512 holds for all of these (grid_y <= 2)
DEC_G_CASES = _decode_cases(
    [(4, 1, 128), (8, 1, 128), (8, 2, 128), (2, 1, 128), (2, 2, 128)],
    (1, 2, 4, 8, 24, 32, 48, 64),
    [(300, 4, 0),      # several tiles per chunk
     (1, 64, 0),       # 63 empty chunks, staged combine
     (2100, 64, 0), (2100, 48, 96), (129, 32, 64), (65, 2, 64),
     (65, 1, 65), (64, 8, 63)])
# per-head fallback kernel (tile 128)
DEC_F_CASES = _decode_cases(
    [(3, 1, 128), (6, 2, 128), (4, 2, 8), (4, 2, 40), (4, 2, 64)],
    (2, 8, 12, 16),
    [(300, 2, 0), (1, 16, 0), (2100, 16, 0), (129, 8, 64), (65, 2, 64)])


def decode_max_seq(n):
    return 2112 if n > 320 else 320
