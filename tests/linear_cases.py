"""Shapes, seeded inputs, tolerances and mutant lists shared by the GPU linear
op tests (test_linear_ops_gpu.py) and the CPU teeth tests
(test_linear_ref.py), so every teeth condition is checked on exactly the
inputs the GPU sees.

Two input families:

exact   x is +-2^j on a set holding every structural boundary index of the
        kernel (sparse), or +-1 everywhere (dense); W is small integers (fp8:
        codes that are exact integers, power-of-two scales that differ per
        128x128 block).  Every partial sum is an integer below 2^24 (times a
        power of two), so every f32 sum is exact in ANY order and the GPU
        must return RNE-to-bf16 of the exact sum (or the f32 sum itself)
        bit for bit.  With a norm, x in {+-1} has mean 1, so xn == +-nw.
random  Gaussian x, W, residual; with a norm also a small-|x| set where
        mean x^2 ~ eps.  Norm inputs are made tie-safe (see tie_safe).

Tolerances are derived, not measured; element-wise |got - ref| <= tol * A +
ABS_EPS with A = sum |W||xhat| + |res|:
  bf16 out  TOL_BF16 = 2^-8: one RNE to bf16 (8 significant bits) costs at
            most 2^-8 |v| at the bottom of a binade, 2^-9 |v| at the top,
            and |v| <= A; f32 accumulation adds K * 2^-24 A <= 2^-9.2 A at
            K = 28672.  The bound is met through A >= |v|, without a factor
            of two to spare.
  f32 out   TOL_F32 = 2^-16: twice the chain depth of k_gemv_reg
            (8 KB + 9 <= 2^7 operations at 2^-24)."""
import zlib

import numpy as np

from tests import linear_ref as lr
from tests.helpers import quantize_bf16

TOL_BF16 = 2.0 ** -8
TOL_F32 = 2.0 ** -16
ABS_EPS = 2.0 ** -40
TIE_MARGIN = 2.0 ** -20
EPS = 1e-5


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def _rng(*key):
    return np.random.default_rng(_seed(*key))


def _q(a):
    return quantize_bf16(np.asarray(a, dtype=np.float32))


# ---- structural boundary indices -------------------------------------------
def boundary_ks(K, fp8=False, splitk=False, gemm=False):
    blk = 4096 if fp8 else 2048
    unit = 16 if fp8 else 8
    s = {0, 7, 8, 15, 16, K - unit - 1, K - unit, K - 1}
    for i in range(1, K // blk + 2):
        s |= {blk * i - 1, blk * i, blk * i + 1}
    if splitk:
        s |= {K // 2 - 1, K // 2}
    if gemm:
        s |= {63, 64, (K - 1) // 64 * 64, (K - 1) // 64 * 64 - 1}
    return np.array(sorted(k for k in s if 0 <= k < K))


# integers 0..8 that e4m3fn holds exactly, as codes
_F8_INT_CODES = np.array(
    [int(np.where(lr.E4M3 == v)[0][0]) for v in (0, 1, 2, 3, 4, 5, 6, 7, 8)],
    dtype=np.uint8)


def exact_x(K, dense, rng, **kw):
    if dense:
        return rng.choice([-1.0, 1.0], size=K).astype(np.float32)
    x = np.zeros(K, dtype=np.float32)
    ks = boundary_ks(K, **kw)
    x[ks] = rng.choice([-1.0, 1.0], size=ks.size) * 2.0 ** rng.integers(
        0, 4, size=ks.size)
    return x


def exact_w(N, K, rng, dense=False):
    """Non-zero integers in [-3, 3] against sparse x.  Against dense x
    (every k non-zero) W is {-1, 0, 1} with three zeros in four, which keeps
    |sum| ~ sqrt(K / 4) <= 64: in the range where one bf16 ulp is <= 1, so
    any integer change of a sum shows in the rounded output."""
    if dense:
        return rng.choice([-1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0],
                          size=(N, K)).astype(np.float32)
    w = rng.integers(-3, 4, size=(N, K)).astype(np.float32)
    w[w == 0] = 1.0
    return w


def exact_w8(N, K, rng):
    """fp8 codes of integers +-1..8 and per-block scales 2^-2..2^2 that differ
    between neighbouring blocks in both directions."""
    mag = rng.integers(1, 9, size=(N, K))
    w8 = _F8_INT_CODES[mag] | (rng.integers(0, 2, size=(N, K)).astype(
        np.uint8) << 7)
    i, j = np.meshgrid(np.arange(N // 128), np.arange(K // 128),
                       indexing="ij")
    sc = (2.0 ** ((i * 2 + j * 3) % 5 - 2)).astype(np.float32)
    return w8.astype(np.uint8), sc


def random_w8(N, K, rng):
    b = rng.integers(0, 256, size=(N, K)).astype(np.uint8)
    b[(b & 0x7F) == 0x7F] ^= 0x08         # no NaN codes
    sc = (3e-4 * 2.0 ** rng.uniform(-2, 2, size=(N // 128, K // 128))
          ).astype(np.float32)
    return b, sc


def exact_nw(K, rng):
    return (rng.choice([-1.0, 1.0], size=K) * 2.0 ** rng.integers(
        -1, 2, size=K)).astype(np.float32)


def tie_safe(x, nw, eps, scale=None):
    """Move x (bf16-exact f32) until no float64 x * scale * nw lies within
    TIE_MARGIN (relative) of a bf16 rounding boundary: the kernel's f32
    evaluation (three roundings and rsqrtf, < 2^-21) then re-quantizes to the
    same bf16 as the reference.  Moves one bf16 ulp at a time, iterated
    because every move shifts the mean."""
    x = _q(x).copy()
    for _ in range(64):
        s = lr.norm_scale(x, eps) if scale is None else scale
        near = lr.tie_margin(x.astype(np.float64) * s * nw) < TIE_MARGIN
        if not near.any():
            return x
        u = x.view(np.uint32)
        u[near] += np.uint32(0x10000)      # one bf16 ulp away from zero
    raise AssertionError("tie_safe did not converge")


# ---- GEMV cases -------------------------------------------------------------
# K classes: below one block, every 2048-block edge and edge + 8 up to the
# register kernels' 16384, the streaming kernel, and one K with an odd-sized
# last block (5000 % 2048 = 904)
GEMV_K = (72, 2048, 2056, 4096, 4104, 5000, 8192, 8200, 16384, 16392)
GEMV_ROWS = (2, 4, 8)
FP8_K = (128, 4096, 4224, 8192, 8320, 16384, 16512)
FP8_ROWS = (4, 8)
SPLITK_K = (80, 4096, 4112, 8192, 8208, 16384, 16400, 28672)
GATEUP_K = tuple(k for k in GEMV_K if k <= 16384)
GATEUP_FP8_K = tuple(k for k in FP8_K if k <= 16384)
FAMILIES = ("exact_sparse", "exact_dense", "random", "random_small")


def gemv_n(rows):
    return 2 * rows + 1                    # two full blocks and a row tail


def gemv_inputs(fam, kind, N, K, epi, norm, repeats=1):
    """dict(x (repeats,K), w | (w8, sc), W64, res, nw).  kind bf16|fp8|splitk.
    Exact families with a norm use dense x (mean exactly 1)."""
    rng = _rng("gemv", fam, kind, N, K, epi, norm, repeats)
    fp8 = kind == "fp8"
    exact = fam.startswith("exact")
    d = dict(exact=exact, fp8=fp8, nw=None, res=None, sc=None)
    if exact:
        dense = fam == "exact_dense" or norm
        d["x"] = np.stack([exact_x(K, dense, rng, fp8=fp8,
                                   splitk=kind == "splitk")
                           for _ in range(repeats)])
        if fp8:
            d["w"], d["sc"] = exact_w8(N, K, rng)
        else:
            d["w"] = exact_w(N, K, rng, dense)
        if norm:
            d["nw"] = exact_nw(K, rng)
        if epi == 1:
            d["res"] = rng.integers(-40, 41, size=(repeats, N)).astype(
                np.float32)
    else:
        amp = np.sqrt(EPS) if fam == "random_small" else 1.0
        d["x"] = _q(amp * rng.standard_normal((repeats, K)))
        if fp8:
            d["w"], d["sc"] = random_w8(N, K, rng)
        else:
            d["w"] = _q(0.05 * rng.standard_normal((N, K)))
        if norm:
            d["nw"] = _q(1.0 + 0.2 * rng.standard_normal(K))
            d["x"] = np.stack([tie_safe(r, d["nw"], EPS) for r in d["x"]])
        if fam == "random_small":
            d["w"] = align_signs(d["w"], d["x"][0] * d["nw"], fp8)
    d["W64"] = lr.dequant(d["w"], d["sc"]) if fp8 else d["w"].astype(
        np.float64)
    if not exact and epi == 1:
        # residual of the size of the product, so neither hides the other
        v = d["W64"] @ lr.xhat(d["x"][0], d["nw"], EPS)
        d["res"] = _q(np.sqrt(np.mean(v * v) + 1e-60) *
                      rng.standard_normal((repeats, N)))
    return d


def align_signs(w, xn, fp8):
    """Give every W[n, k] the sign of xn[k], so that every term of every sum
    is positive and |sum| == A.  A random-sign sum is ~ A / sqrt(K): at
    K = 16384 the bound 2^-8 A is then 0.4 |sum| and hides the 1.4x that a
    dropped eps makes of the small-|x| family.  Aligned, it cannot."""
    neg = np.asarray(xn) < 0
    if fp8:
        return ((w & 0x7F) | (neg.astype(np.uint8) << 7)[None, :]).astype(
            np.uint8)
    return (np.abs(w) * np.where(neg, -1.0, 1.0)[None, :]).astype(np.float32)


def gemv_families(norm):
    return FAMILIES if norm else FAMILIES[:3]


# Every op_gemv call of the GPU module, as (kind, N, K, epi, norm mode,
# repeats); the GPU tests and the teeth tests both enumerate from here, so the
# teeth run on exactly the (N, repeats)-seeded inputs the GPU sees.  rows only
# enters through N = gemv_n(rows).
FP8_N = 256
SPLITK_N = 5
PRODUCE_N = 640            # 160 / 80 blocks: 20 / 10 per counter shard
PRODUCE_K = (256, 16512)
REPEATS = 3


def gemv_norm_modes(kind, K):
    if K > 16384 or kind == "splitk":
        return (None,)
    return (None, "fused", "chain") if kind == "fp8" else (None, "fused")


def gemv_gpu_cases():
    out = []
    for K in GEMV_K:
        for rows in GEMV_ROWS:
            for epi in (0, 1, 2):
                for norm in gemv_norm_modes("bf16", K):
                    out.append(("bf16", gemv_n(rows), K, epi, norm, 1))
    for K in FP8_K:
        for epi in (0, 1, 2):
            for norm in gemv_norm_modes("fp8", K):
                out.append(("fp8", FP8_N, K, epi, norm, 1))
    out += [("splitk", SPLITK_N, K, 1, None, REPEATS) for K in SPLITK_K]
    out += [("fp8", PRODUCE_N, K, 1, None, REPEATS) for K in PRODUCE_K]
    return out


def gateup_i(fp8, rows):
    return 128 if fp8 else 2 * rows + 1


def gateup_gpu_cases():
    """(fp8, I, K, norm mode) of every op_gemv_gateup call."""
    out = [(False, gateup_i(False, r), K, n) for K in GATEUP_K
           for r in (4, 8) for n in (None, "fused")]
    out += [(True, gateup_i(True, 4), K, n) for K in GATEUP_FP8_K
            for n in (None, "fused", "chain")]
    return out


def gemv_mutants(kind, N, K, epi, norm, rows):
    """The defects a GEMV of this shape could have (name list)."""
    fp8 = kind == "fp8"
    blk = 4096 if fp8 else 2048
    m = ["tail_dropped", "block_dropped", "row_next", "row_prev"]
    if kind != "splitk" and K % blk:    # threads past K re-load the tail
        m += ["tail_twice"]
    if kind == "splitk":
        m += ["half_dropped"]
    if epi == 1:
        m += ["res_skipped", "res_doubled", "res_next", "res_prev"]
    if norm:
        m += ["nw_shift8", "eps_dropped"]
        if K % blk:
            m += ["mean_padded"]
    if fp8:
        if N > 128:
            m += ["scale_row_off"]
        if K > 128:
            m += ["scale_col_off"]
    return m


# ---- gate-up ----------------------------------------------------------------
def gateup_inputs(fam, fp8, I, K, norm):
    rng = _rng("gateup", fam, fp8, I, K, norm)
    exact = fam.startswith("exact")
    d = dict(exact=exact, fp8=fp8, nw=None, sc=None)
    if exact:
        dense = fam == "exact_dense" or norm
        d["x"] = exact_x(K, dense, rng, fp8=fp8)
        if fp8:
            d["w"], d["sc"] = exact_w8(2 * I, K, rng)
        else:
            d["w"] = exact_w(2 * I, K, rng, dense)
        if norm:
            d["nw"] = exact_nw(K, rng)
    else:
        amp = np.sqrt(EPS) if fam == "random_small" else 1.0
        d["x"] = _q(amp * rng.standard_normal(K))
        if fp8:
            d["w"], d["sc"] = random_w8(2 * I, K, rng)
            # gate sums of order 1 so silu is in its curved range
            d["sc"] = (d["sc"] * 40).astype(np.float32)
        else:
            d["w"] = _q(rng.standard_normal((2 * I, K)) / np.sqrt(K))
        if norm:
            d["nw"] = _q(1.0 + 0.2 * rng.standard_normal(K))
            d["x"] = tie_safe(d["x"], d["nw"], EPS)
        if fam == "random_small":
            # up rows aligned (|u| == A_u); gate rows stay random so silu
            # stays in its curved range
            d["w"][I:] = align_signs(d["w"][I:], d["x"] * d["nw"], fp8)
    d["W64"] = lr.dequant(d["w"], d["sc"]) if fp8 else d["w"].astype(
        np.float64)
    return d


def gateup_bound(val, g, u, Ag, Au):
    """2^-8 |ref| + 2^-16 (1.1 A_g |u| + |silu(g)| A_u): one RNE of the
    product, plus the f32 error of g through silu (|silu'| <= 1.1) and of u."""
    return (TOL_BF16 * np.abs(val) + TOL_F32 * (
        1.1 * Ag * np.abs(u) + np.abs(lr.silu(g)) * Au) + ABS_EPS)


def gateup_mutants(fp8, I, K, norm):
    blk = 4096 if fp8 else 2048
    m = ["tail_dropped", "block_dropped", "gate_up_swapped", "up_next",
         "up_prev", "row_next"]
    if K % blk:
        m += ["tail_twice"]
    if norm:
        m += ["nw_shift8", "eps_dropped"]
        if K % blk:
            m += ["mean_padded"]
    if fp8:
        m += ["scale_row_off", "gate_scale_for_up"]
        if K > 128:
            m += ["scale_col_off"]
    return m


# ---- fused qkv-rope ---------------------------------------------------------
ROPE_MAX_SEQ = 96
ROPE_K = (72, 2056, 4104, 8200)            # KB 1, 2, 4, 8
ROPE_GEOM = ((2, 1, 64), (4, 2, 64), (2, 1, 128), (4, 2, 128))
ROPE_POS = (0, 45, ROPE_MAX_SEQ - 1)
ROPE_MUTANTS = ("tail_dropped", "partner_off", "sin_sign", "pos_next",
                "pos_prev", "kvhead_off", "vtc_col_off", "nw_shift8")
STALE = 2.0 ** 60


def rope_cases():
    """Every K with every geometry, every pos with every K (pruned cross)."""
    out = []
    for i, K in enumerate(ROPE_K):
        for j, g in enumerate(ROPE_GEOM):
            out.append(g + (K, ROPE_POS[(i + j) % 3]))
        out.append(ROPE_GEOM[(i + 1) % 4] + (K, ROPE_POS[(i + 2) % 3]))
    return out


def rope_inputs(fam, nh, nkv, hd, K, pos):
    rng = _rng("rope", fam, nh, nkv, hd, K, pos)
    Nq = (nh + 2 * nkv) * hd
    max_seq = ROPE_MAX_SEQ
    exact = fam.startswith("exact")
    if exact:                              # V rows exact; q/k rows bounded
        x = exact_x(K, True, rng)
        w = exact_w(Nq, K, rng, True)
        nw = exact_nw(K, rng)
    else:
        nw = _q(1.0 + 0.2 * rng.standard_normal(K))
        x = tie_safe(_q(rng.standard_normal(K)), nw, EPS)
        w = _q(rng.standard_normal((Nq, K)) / np.sqrt(K))
    inv = 1.0 / np.power(10000.0, np.arange(0, hd, 2) / hd)
    # a table whose rows differ at every position, 0 included
    ang = ((np.arange(max_seq)[:, None] + 0.5) * inv[None, :]).astype(
        np.float32)
    cos, sin = np.cos(ang), np.sin(ang)

    def sentinel():                        # as the KV-store test's images
        a = rng.standard_normal((nkv, max_seq, hd))
        a = np.where(rng.random(a.shape) < 0.25,
                     rng.choice([-STALE, STALE], size=a.shape), a)
        return _q(a)
    kc, vc = sentinel(), sentinel()
    vtc = np.ascontiguousarray(sentinel().transpose(0, 2, 1))
    return dict(x=x, w=w, nw=nw, cos=cos, sin=sin, kc=kc, vc=vc, vtc=vtc,
                exact=exact)


def rope_bound(mag, acc):
    """2^-8 (|s0 c| + |s2 s|): one RNE of the rotated value, whose magnitude
    is at most |s0 c| + |s2 s|, plus the f32 accumulation of the two sums at
    TOL_F32."""
    return TOL_BF16 * mag + TOL_F32 * acc + ABS_EPS


# ---- GEMM -------------------------------------------------------------------
GEMM_K = (64, 128, 192, 256)               # 1..4 k-tiles in every pipeline
# (M, N) giving grids of 1, 6 and 9 blocks with M and N tails, per tile shape
GEMM_MN = {
    "128": ((100, 90), (200, 300), (300, 330)),
    "256": ((200, 250), (300, 700), (520, 600)),
    "256p": ((200, 250), (300, 700), (520, 600)),
    "128x256": ((100, 250), (200, 700), (300, 600)),
    "library": ((100, 90), (200, 300), (300, 330)),
}
GEMM_TILE = {"128": (128, 128), "256": (256, 256), "256p": (256, 256),
             "128x256": (128, 256), "library": (128, 128)}
GEMM_RAGGED_K = (96, 40)                   # 128^2 (and the library) only
GEMM_PRODUCT = (2048, 4096, 4096)          # 8B o-projection class
GEMM_MODES = ((0, False), (1, False), (1, True))   # (epi, alias)


def gemm_cases(variant):
    out = [(M, N, K) for (M, N) in GEMM_MN[variant] for K in GEMM_K]
    if variant in ("128", "library"):
        out += [(200, 300, K) for K in GEMM_RAGGED_K]
    return out


def gemm_inputs(fam, M, N, K, epi):
    rng = _rng("gemm", fam, M, N, K, epi)
    exact = fam.startswith("exact")
    res = None
    if exact:
        if fam == "exact_dense":
            a = rng.choice([-1.0, 1.0], size=(M, K)).astype(np.float32)
        else:
            a = np.zeros((M, K), dtype=np.float32)
            ks = boundary_ks(K, gemm=True)
            a[:, ks] = rng.choice([-1.0, 1.0], size=(M, ks.size)) * \
                2.0 ** rng.integers(0, 4, size=(M, ks.size))
        w = exact_w(N, K, rng, fam == "exact_dense")
        if epi:
            res = rng.integers(-40, 41, size=(M, N)).astype(np.float32)
    else:
        a = _q(rng.standard_normal((M, K)))
        w = _q(rng.standard_normal((N, K)) / np.sqrt(K))
        if epi:
            res = _q(rng.standard_normal((M, N)))
    return dict(a=a, w=w, res=res, exact=exact)


def gemm_mutants(variant, M, N, K, epi):
    tm, tn = GEMM_TILE[variant]
    m = ["tile_uncomputed", "ktile_dropped"]
    if M > tm and N > tn:
        m += ["tiles_transposed"]
    if epi:
        m += ["res_transposed"]
    return m


GEMM_FAMILIES = ("exact_sparse", "exact_dense", "random")


# ---- norm-chain / split-K counters ------------------------------------------
def chain_shard_totals(nblocks):
    return [(nblocks - s + 7) >> 3 for s in range(8)]


def chain_cnt_zero():
    return np.zeros(9, dtype=np.uint32)


def chain_cnt_prewrap(nblocks):
    """Phase-aligned counters one launch below 2^32: shard s at
    (2^32 // st_s) * st_s - st_s, the top word likewise with modulus 8."""
    c = [(2 ** 32 // st) * st - st for st in chain_shard_totals(nblocks)]
    c.append(2 ** 32 - 8)
    return np.array(c, dtype=np.uint32)


SPLITK_PREWRAP = 2 ** 32 - 2


def elect_trace(start, total, launches, reset):
    """Host model of one arrival word over `launches` launches of `total`
    arrivals each (u32 arithmetic): per launch, the arrival index at which
    `v % total == total - 1` elected (None if no arrival did).  `reset`: the
    elected arrival stores 0 (the fixed kernel)."""
    c, out = int(start), []
    for _ in range(launches):
        hit = None
        for i in range(total):
            v = c
            c = (c + 1) & 0xFFFFFFFF
            if v % total == total - 1:
                hit = i if hit is None else hit
                if reset:
                    c = 0
        out.append(hit)
    return out


# ---- expectations shared by the GPU tests and the teeth tests ---------------
def gemv_expect(d, epi, norm_mode, i=0, mut=None):
    """(value, A) of repeat i.  norm_mode: None | "fused" | "chain" (the
    consumer gets the float64 scale of the reference, rounded to f32)."""
    W = d["W64"]
    if mut in ("scale_row_off", "scale_col_off"):
        W = lr.dequant(d["w"], d["sc"], mut)
    scale = None
    if norm_mode == "chain":
        scale = float(np.float32(lr.norm_scale(d["x"][i], EPS)))
    res = d["res"][i] if d["res"] is not None else None
    return lr.gemv_ref(W, d["x"][i], res, d["nw"], EPS, scale, mut,
                       d["fp8"])


def gemv_tol(epi):
    return TOL_F32 if epi == 2 else TOL_BF16


def out_bits(val, f32_out):
    """The bit pattern an exact-family output must have."""
    return lr.f32_bits(val) if f32_out else lr.bf16_bits(val)


def got_bits(got, f32_out):
    """Bit pattern of a GPU output that crossed the boundary as f32."""
    u = lr.f32_bits(got)
    return u if f32_out else u >> 16


def moved(exact, base, mutated, bound, f32_out=False):
    """The teeth condition: a bit flips (exact family) or some element moves
    by more than twice the bound the GPU test grants."""
    if exact:
        return bool((out_bits(base, f32_out) !=
                     out_bits(mutated, f32_out)).any())
    return bool((np.abs(mutated - base) > 2 * bound).any())


# ---- plain kernels of the prefill and split-norm chains ---------------------
SILU_ROWS_CASES = ((1, 8), (3, 72), (2, 16400))    # last: grid-stride loop
# (outer, inner, gap between outer groups, cols)
RMS_ROWS_CASES = ((1, 5, 0, 72), (3, 4, 16, 64), (2, 2, 264, 128),
                  (1, 1, 0, 4104))


def bf16_ulp(v):
    """The spacing of bf16 values at |v| (float64)."""
    _, e = np.frexp(np.abs(np.asarray(v, dtype=np.float64)))
    return np.ldexp(1.0, e - 8)


def silu_rows_inputs(S, I, safe):
    """gu (S, 2I) = [gate | up].  |gate| <= 3 keeps the error of __expf's
    argument scaling (|g| 1.44 2^-24) below 2^-22.  safe: up is moved one
    bf16 ulp at a time until no float64 silu(g) u lies within TIE_MARGIN of a
    rounding boundary, so the kernel's f32 result rounds like the reference."""
    rng = _rng("silu_rows", S, I, safe)
    g = _q(np.clip(1.5 * rng.standard_normal((S, I)), -3, 3))
    u = _q(rng.standard_normal((S, I)))
    for _ in range(64 if safe else 0):
        near = lr.tie_margin(lr.silu(g.astype(np.float64)) * u) < TIE_MARGIN
        if not near.any():
            break
        u.view(np.uint32)[near] += np.uint32(0x10000)
    else:
        assert not safe, "silu_rows_inputs did not converge"
    return np.concatenate([g, u], axis=1)


def silu_rows_ref(gu):
    I = gu.shape[1] // 2
    g, u = gu[:, :I].astype(np.float64), gu[:, I:].astype(np.float64)
    return lr.silu(g) * u


def rms_rows_inputs(outer, inner, gap, cols, safe):
    """(flat x, w, outer_stride, row offsets).  safe: every row tie-safe."""
    rng = _rng("rms_rows", outer, inner, gap, cols, safe)
    stride = inner * cols + gap
    n = (outer - 1) * stride + inner * cols
    x = _q(rng.standard_normal(n))
    w = _q(1.0 + 0.2 * rng.standard_normal(cols))
    offs = [o * stride + i * cols for o in range(outer) for i in range(inner)]
    if safe:
        for off in offs:
            x[off:off + cols] = tie_safe(x[off:off + cols], w, EPS)
    return x, w, stride, offs


def rms_rows_ref(x, w, offs, eps):
    """float64 x * rsqrt(mean x^2 + eps) * w per row; NaN between rows."""
    out = np.full(x.size, np.nan)
    for off in offs:
        r = x[off:off + w.size].astype(np.float64)
        out[off:off + w.size] = r * lr.norm_scale(r, eps) * w
    return out
