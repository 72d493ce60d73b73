"""Float64 references of the linear-layer kernels (GEMV, fp8 GEMV, gate-up,
fused qkv-rope, GEMM, fp8 dequant), written from the definitions and
independent of oracle/.  Every reference returns, per output element, the
value and the bound term A = sum |W| |xhat| (+ |res|), so the GPU tests can
assert |got - ref| <= tol * A element-wise.

Each reference takes `mut`, the name of a deliberate defect (the teeth
mutants of tests/test_linear_ref.py): the CPU tests prove that every defect
a kernel of this family could plausibly have moves the reference by more than
the GPU tests tolerate, on the very inputs the GPU tests use."""
import numpy as np

SENTINEL = -2.0 ** 60


# ---- number formats ---------------------------------------------------------
def _e4m3fn_table():
    """All 256 e4m3fn codes (1 sign, 4 exponent bits of bias 7, 3 mantissa
    bits; no infinities, S.1111.111 is NaN) as float64."""
    t = np.empty(256, dtype=np.float64)
    for c in range(256):
        s = -1.0 if c & 0x80 else 1.0
        e, m = (c >> 3) & 0xF, c & 7
        if e == 0xF and m == 7:
            t[c] = np.nan
        elif e == 0:
            t[c] = s * m * 2.0 ** -9            # subnormal: m/8 * 2^-6
        else:
            t[c] = s * (1 + m / 8.0) * 2.0 ** (e - 7)
    return t


E4M3 = _e4m3fn_table()


def bf16(a):
    """Round float64 to the nearest bf16 (ties to even) in ONE step; returns
    float64.  (f64 -> f32 -> bf16 would round twice.)"""
    a = np.asarray(a, dtype=np.float64)
    m, e = np.frexp(a)                  # a = m * 2^e, 0.5 <= |m| < 1
    e = np.maximum(e, -125)             # bf16 subnormals share f32's 2^-133
    q = np.ldexp(1.0, e - 8)            # 8 significant bits
    with np.errstate(invalid="ignore"):
        r = np.rint(a / q) * q          # rint rounds half to even
    return np.where(np.isfinite(a), r, a)


def bf16_bits(a):
    """The 16-bit pattern of bf16(a) (as uint32), NaN canonicalised."""
    f = bf16(a).astype(np.float32)
    u = np.ascontiguousarray(f).view(np.uint32) >> 16
    return np.where(np.isnan(f), np.uint32(0x7FC0), u)


def f32_bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def tie_margin(v):
    """Relative distance of float64 v from the nearest bf16 rounding
    boundary (the midpoint of two neighbouring bf16 values); inf at 0."""
    v = np.abs(np.asarray(v, dtype=np.float64))
    m, e = np.frexp(v)
    t = v / np.ldexp(1.0, e - 8)        # in [128, 256)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.abs(t - np.floor(t) - 0.5) / t
    return np.where(v == 0, np.inf, d)


def dequant(w8, sc, mut=None, split=None):
    """fp8 codes (N,K) with blockwise 128x128 scales -> float64 weights."""
    sc = np.asarray(sc, dtype=np.float64)
    if mut == "scale_row_off":
        sc = np.roll(sc, 1, axis=0)
    elif mut == "scale_col_off":
        sc = np.roll(sc, 1, axis=1)
    elif mut == "gate_scale_for_up":    # split = I: up rows use gate's blocks
        sc = sc.copy()
        sc[split // 128:] = sc[:split // 128]
    full = np.repeat(np.repeat(sc, 128, axis=0), 128, axis=1)
    return E4M3[np.asarray(w8, dtype=np.uint8)] * full


def dequant_bf16_bits(w8, sc):
    """k_dequant_fp8 exactly: one IEEE f32 multiply, then RNE to bf16."""
    full = np.repeat(np.repeat(np.asarray(sc, np.float32), 128, axis=0), 128,
                     axis=1)
    with np.errstate(invalid="ignore"):
        p = E4M3[np.asarray(w8, np.uint8)].astype(np.float32) * full
    return bf16_bits(p.astype(np.float64))


# ---- rms_norm of the x row, as every fused kernel applies it ----------------
def norm_scale(x, eps, mut=None, kblock=2048):
    x = np.asarray(x, dtype=np.float64)
    K = x.shape[-1]
    n = K
    if mut == "mean_padded":            # mean over K rounded up to the block
        n = -(-K // kblock) * kblock
    if mut == "eps_dropped":
        eps = 0.0
    return 1.0 / np.sqrt(np.sum(x * x) / n + eps)


def xhat(x, nw=None, eps=0.0, scale=None, mut=None, kblock=2048):
    """The x the dot products see: x itself, or bf16(x * scale * nw) with
    scale = rsqrt(mean x^2 + eps) (or the given norm-chain scale)."""
    x = np.asarray(x, dtype=np.float64)
    if nw is None:
        return x
    nw = np.asarray(nw, dtype=np.float64)
    if mut == "nw_shift8":
        nw = np.roll(nw, 8)
    if scale is None:
        scale = norm_scale(x, eps, mut, kblock)
    return bf16(x * scale * nw)


# ---- GEMV -------------------------------------------------------------------
def _mut_k(W, xh, mut, unit, kblock, extra=None):
    """Defects of the k loop: returns (W, xh, extra term to add)."""
    K = xh.shape[0]
    if mut == "tail_dropped":           # last 8 (bf16) / 16 (fp8) k
        xh = xh.copy()
        xh[K - unit:] = 0
    elif mut == "tail_twice":           # the clamped duplicate leaks in
        extra = W[:, K - unit:] @ xh[K - unit:]
    elif mut == "block_dropped":        # last 2048 / 4096 block
        xh = xh.copy()
        xh[(K - 1) // kblock * kblock:] = 0
    elif mut == "half_dropped":         # second split-K slice
        xh = xh.copy()
        xh[K // 2:] = 0
    return xh, extra


def gemv_ref(W, x, res=None, nw=None, eps=0.0, scale=None, mut=None,
             fp8=False):
    """out[n] = sum_k W[n,k] xhat[k] (+ res[n]).  W float64 (N,K) (already
    dequantized).  Returns (value, A), both float64 (N,)."""
    W = np.asarray(W, dtype=np.float64)
    unit, kblock = (16, 4096) if fp8 else (8, 2048)
    xh = xhat(x, nw, eps, scale, mut, kblock)
    xm, extra = _mut_k(W, xh, mut, unit, kblock)
    v = W @ xm
    if extra is not None:
        v = v + extra
    if mut == "row_next":
        v = np.roll(v, -1)
    elif mut == "row_prev":
        v = np.roll(v, 1)
    A = np.abs(W) @ np.abs(xh)
    if res is not None:
        r = np.asarray(res, dtype=np.float64)
        A = A + np.abs(r)
        if mut == "res_skipped":
            r = 0 * r
        elif mut == "res_doubled":
            r = 2 * r
        elif mut == "res_next":
            r = np.roll(r, -1)
        elif mut == "res_prev":
            r = np.roll(r, 1)
        v = v + r
    return v, A


def sumsq_scale(q, eps):
    """Norm-chain produce: rsqrt(mean of the squared bf16 outputs + eps)."""
    q = np.asarray(q, dtype=np.float64)
    return 1.0 / np.sqrt(np.sum(q * q) / q.shape[0] + eps)


# ---- gate-up ----------------------------------------------------------------
def gateup_ref(W, x, I, nw=None, eps=0.0, scale=None, mut=None, fp8=False):
    """out[c] = silu(g_c) * u_c.  Returns (value, g, u, A_g, A_u)."""
    W = np.asarray(W, dtype=np.float64)
    unit, kblock = (16, 4096) if fp8 else (8, 2048)
    xh = xhat(x, nw, eps, scale, mut, kblock)
    xm, extra = _mut_k(W, xh, mut, unit, kblock)
    s = W @ xm
    if extra is not None:
        s = s + extra
    a = np.abs(W) @ np.abs(xh)
    g, u, Ag, Au = s[:I], s[I:], a[:I], a[I:]
    if mut == "gate_up_swapped":
        g, u = u, g
    elif mut == "up_next":
        u = np.roll(s, -1)[I:]
    elif mut == "up_prev":
        u = np.roll(s, 1)[I:]
    elif mut == "row_next":
        g, u = np.roll(g, -1), np.roll(u, -1)
    with np.errstate(over="ignore"):
        val = g / (1.0 + np.exp(-g)) * u
    return val, g, u, Ag, Au


def silu(g):
    with np.errstate(over="ignore"):
        return g / (1.0 + np.exp(-g))


# ---- fused norm -> qkv GEMV -> rope -> KV store -------------------------------
def qkv_rope_ref(W, x, nw, eps, cos, sin, pos, nh, nkv, hd, kc, vc, vtc,
                 mut=None):
    """Returns dict with q (nh,hd) and its bound, the kc/vc/vtc images after
    the store (float64; K rows at pos carry a bound, V rows are bf16 of the
    sum) and the raw sums s, A."""
    W = np.asarray(W, dtype=np.float64)
    xh = xhat(x, nw, eps, None, mut)
    xm, extra = _mut_k(W, xh, mut, 8, 2048)
    s = W @ xm + (0 if extra is None else extra)
    A = np.abs(W) @ np.abs(xh)
    half = hd // 2
    p = pos + (1 if mut == "pos_next" else -1 if mut == "pos_prev" else 0)
    p = p % cos.shape[0]
    c = np.asarray(cos, np.float64)[p]
    sn = np.asarray(sin, np.float64)[p]
    if mut == "sin_sign":
        sn = -sn
    heads = s[:(nh + nkv) * hd].reshape(nh + nkv, hd)
    Ah = A[:(nh + nkv) * hd].reshape(nh + nkv, hd)
    lo, hi = heads[:, :half], heads[:, half:]
    if mut == "partner_off":            # rope partner i + hd/2 + 1
        hi_p = np.roll(heads, -1, axis=1)[:, half:]
        lo_p = np.roll(heads, -1, axis=1)[:, :half]
    else:
        hi_p, lo_p = hi, lo
    roped = np.concatenate([lo * c - hi_p * sn, hi * c + lo_p * sn], axis=1)
    # bound terms of the issue: 2^-8 (|s0 c| + |s2 s|) + accumulation
    mag = np.concatenate([np.abs(lo * c) + np.abs(hi * sn),
                          np.abs(hi * c) + np.abs(lo * sn)], axis=1)
    acc = np.concatenate([Ah[:, :half] * np.abs(c) + Ah[:, half:] * np.abs(sn),
                          Ah[:, half:] * np.abs(c) + Ah[:, :half] * np.abs(sn)],
                         axis=1)
    kc, vc, vtc = (np.array(a, dtype=np.float64) for a in (kc, vc, vtc))
    v = s[(nh + nkv) * hd:].reshape(nkv, hd)
    ps = pos                             # the slot is the true pos ...
    if mut in ("pos_next", "pos_prev"):  # ... unless pos itself is off
        ps = p
    for h in range(nkv):
        hk = (h + 1) % nkv if mut == "kvhead_off" else h
        kc[hk, ps] = roped[nh + h]
        vc[hk, ps] = bf16(v[h])
        pt = (ps + 1) % vtc.shape[2] if mut == "vtc_col_off" else ps
        vtc[hk, :, pt] = bf16(v[h])
    return dict(q=roped[:nh], q_mag=mag[:nh], q_acc=acc[:nh], kc=kc, vc=vc,
                vtc=vtc, k_mag=mag[nh:], k_acc=acc[nh:], slot=ps,
                v_A=A[(nh + nkv) * hd:].reshape(nkv, hd))


# ---- GEMM -------------------------------------------------------------------
def gemm_ref(a, w, res=None, mut=None, tile=(128, 128)):
    """C = a @ w^T (+ res).  Returns (value, A) float64 (M,N)."""
    a = np.asarray(a, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    M, K = a.shape
    N = w.shape[0]
    am = a
    if mut == "ktile_dropped":
        am = a.copy()
        am[:, (K - 1) // 64 * 64:] = 0
    v = am @ w.T
    A = np.abs(a) @ np.abs(w).T
    tm, tn = tile
    if mut == "tiles_transposed":        # block (i,j) computed as (j,i)
        out = v.copy()
        for i in range(-(-M // tm)):
            for j in range(-(-N // tn)):
                if i == j:
                    continue
                rs = np.minimum(j * tm + np.arange(tm), M - 1)
                cs = np.minimum(i * tn + np.arange(tn), N - 1)
                blk = a[rs] @ w[cs].T
                r0, c0 = i * tm, j * tn
                out[r0:r0 + tm, c0:c0 + tn] = blk[:M - r0, :N - c0]
        v = out
    if res is not None:
        r = np.asarray(res, dtype=np.float64)
        A = A + np.abs(r)
        if mut == "res_transposed":      # res[col][row] with the same ld
            idx = (np.arange(N)[None, :] * N + np.arange(M)[:, None]) % (M * N)
            r = r.reshape(-1)[idx]
        v = v + r
    if mut == "tile_uncomputed":         # the last tile keeps its sentinel
        v = v.copy()
        v[(M - 1) // tm * tm:, (N - 1) // tn * tn:] = SENTINEL
    return v, A
