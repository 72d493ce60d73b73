"""Float64 reference of the GPTQ 4-bit linear kernels (GEMV, gate-up,
dequant), written from the format definition and independent of oracle/ and of
the loader's repack.

Format (AutoGPTQ, K = in_features, N = out_features, group g, G = K/g):
  qweight I32 (K/8, N): nibble b (bits 4b..4b+3) of word [r, j] is q(8r+b, j)
  qzeros  I32 (G, N/8): nibble j % 8 of word [gi, j/8] is z(gi, j)
  scales  F16 (G, N)
  W[j, k] = (q(k, j) - (z(k/g, j) + 1)) * s(k/g, j)
Worked examples: stored zero 15 gives z + 1 = 16 (it does not wrap to 0), so
q = 15 there is -1 * s; the word 0xF0000000 is the int32 -268435456 and its
top nibble is (w >> 28) & 0xF = 15, not -1.

Every reference takes `mut`, the name of a deliberate defect (the teeth
mutants of tests/test_w4_ref.py)."""
import numpy as np

from tests.linear_ref import bf16, bf16_bits, silu  # noqa: F401

SENTINEL = -2.0 ** 60


# ---- pack / unpack ----------------------------------------------------------
def pack_gptq(q, z, s):
    """q (K, N) and z (G, N) integers in [0, 15], s (G, N) -> checkpoint-
    layout (qweight (K/8, N) int32, qzeros (G, N/8) int32, scales (G, N)
    float32)."""
    q = np.asarray(q).astype(np.uint32)
    z = np.asarray(z).astype(np.uint32)
    K, N = q.shape
    G = z.shape[0]
    assert K % 8 == 0 and N % 8 == 0 and z.shape == (G, N)
    assert q.max() <= 15 and z.max() <= 15
    qw = np.zeros((K // 8, N), np.uint32)
    qz = np.zeros((G, N // 8), np.uint32)
    for b in range(8):
        qw |= q[b::8] << np.uint32(4 * b)
        qz |= z[:, b::8] << np.uint32(4 * b)
    return (qw.view(np.int32), qz.view(np.int32),
            np.ascontiguousarray(s, dtype=np.float32))


def unpack_gptq(qweight, qzeros, mut=None):
    """-> q (K, N), z (G, N) as int64 (a defect may leave [0, 15])."""
    qw = np.asarray(qweight, dtype=np.int32)
    qz = np.asarray(qzeros, dtype=np.int32)
    K8, N = qw.shape
    G = qz.shape[0]
    q = np.empty((K8 * 8, N), np.int64)
    z = np.empty((G, N), np.int64)
    uw, uz = qw.view(np.uint32), qz.view(np.uint32)
    for b in range(8):
        src = 7 - b if mut == "nibble_reversed" else b
        q[b::8] = (uw >> np.uint32(4 * src)) & 0xF
        z[:, b::8] = (uz >> np.uint32(4 * b)) & 0xF
    if mut == "top_nibble_signed":      # arithmetic shift of the signed word
        q[7::8] = qw.astype(np.int64) >> 28
        z[:, 7::8] = qz.astype(np.int64) >> 28
    return q, z


def dequant(qweight, qzeros, scales, g, mut=None, split=None):
    """Checkpoint tensors -> float64 W (N, K).  split: row at which a second
    projection starts in a fused tensor (mutant qkv_offset)."""
    q, z = unpack_gptq(qweight, qzeros, mut)
    s = np.asarray(scales, dtype=np.float64)
    K, N = q.shape
    G = K // g
    assert z.shape == (G, N) and s.shape == (G, N)
    zp = z + 1
    if mut == "plus1_dropped":
        zp = z
    elif mut == "z16_wrapped":
        zp = (z + 1) & 0xF
    elif mut == "zero_col_next":
        zp = np.roll(zp, -1, axis=1)
    elif mut == "zero_col_prev":
        zp = np.roll(zp, 1, axis=1)
    elif mut == "zero_word_next":
        zp = np.roll(zp, -8, axis=1)
    elif mut == "zero_group_next":
        zp = np.roll(zp, -1, axis=0)
    elif mut == "zero_group_prev":
        zp = np.roll(zp, 1, axis=0)
    elif mut == "scale_group_next":
        s = np.roll(s, -1, axis=0)
    elif mut == "scale_group_prev":
        s = np.roll(s, 1, axis=0)
    elif mut == "scales_untransposed":  # (G, N) memory read as (N, G)
        s = s.reshape(-1)[np.arange(N)[None, :] * G + np.arange(G)[:, None]]
    elif mut == "qkv_offset":           # second projection gets the first's
        s = s.copy()                    # scales
        s[:, split:] = s[:, :N - split]
    gi = np.arange(K) // g
    return ((q - zp[gi]) * s[gi]).T


def dequant_bf16_bits(qweight, qzeros, scales, g):
    """k_dequant_w4 exactly: the product is exact, one RNE to bf16."""
    return bf16_bits(dequant(qweight, qzeros, scales, g))


# ---- GEMV / gate-up ---------------------------------------------------------
def slab_of(K):
    """k covered by one pass of a block: 4096 (two half-block row sets) up
    to K = 4096, else 8192."""
    return 4096 if K <= 4096 else 8192


def _mut_k(W, x, mut):
    K = x.shape[0]
    extra = None
    last = (K - 1) // slab_of(K) * slab_of(K)
    if mut == "tail32_dropped":
        x = x.copy()
        x[K - 32:] = 0
    elif mut == "tail32_twice":         # the clamped duplicate leaks in
        extra = W[:, K - 32:] @ x[K - 32:]
    elif mut == "slab_dropped":
        x = x.copy()
        x[last:] = 0
    elif mut == "slab_twice":
        extra = W[:, last:] @ x[last:]
    return x, extra


DEQUANT_MUTANTS = ("nibble_reversed", "top_nibble_signed", "plus1_dropped",
                   "z16_wrapped", "zero_col_next", "zero_col_prev",
                   "zero_word_next", "zero_group_next", "zero_group_prev",
                   "scale_group_next", "scale_group_prev",
                   "scales_untransposed", "qkv_offset")


def gemv_ref(t, g, x, res=None, mut=None, split=None):
    """t = (qweight, qzeros, scales).  out[j] = sum_k W[j,k] x[k] (+ res[j]).
    Returns (value, A = sum |W||x| + |res|), float64 (N,); A is of the TRUE
    weights whatever the defect."""
    W0 = dequant(*t, g)
    W = dequant(*t, g, mut, split) if mut in DEQUANT_MUTANTS else W0
    x = np.asarray(x, dtype=np.float64)
    xm, extra = _mut_k(W, x, mut)
    v = W @ xm
    if extra is not None:
        v = v + extra
    if mut == "row_next":
        v = np.roll(v, -1)
    elif mut == "row_prev":
        v = np.roll(v, 1)
    A = np.abs(W0) @ np.abs(x)
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


def gateup_ref(t, g, x, mut=None):
    """Fused tensor of N = 2I rows: out[c] = silu(g_c) * u_c.  Returns (value,
    g, u, A_g, A_u) in the form of tests/linear_ref.gateup_ref."""
    W0 = dequant(*t, g)
    I = W0.shape[0] // 2
    W = dequant(*t, g, mut, I) if mut in DEQUANT_MUTANTS else W0
    x = np.asarray(x, dtype=np.float64)
    xm, extra = _mut_k(W, x, mut)
    s = W @ xm
    if extra is not None:
        s = s + extra
    a = np.abs(W0) @ np.abs(x)
    gt, u, Ag, Au = s[:I], s[I:], a[:I], a[I:]
    if mut == "gate_up_swapped":
        gt, u = u, gt
    elif mut == "row_next":
        gt, u = np.roll(gt, -1), np.roll(u, -1)
    elif mut == "row_prev":
        gt, u = np.roll(gt, 1), np.roll(u, 1)
    return silu(gt) * u, gt, u, Ag, Au


# ---- f32 emulations of the kernel's arithmetic ------------------------------
def gemv_emulate_f32(t, g, x, order):
    """The GEMV sum in float32, in the kernel's form or a plain one:
      "kernel": per 32-k lane span s * (sum q x) + m * (sum x) with
                m = -(z+1) s, two interleaved fma chains per span, spans
                summed lane-major then pairwise (wave tree);
      "plain":  w = fma(q, s, m) per element, one sequential fma chain.
    Returns float32 (N,) (before the residual and the output rounding)."""
    q, z = unpack_gptq(t[0], t[1])
    s = np.asarray(t[2], dtype=np.float32)
    K, N = q.shape
    x = np.asarray(x, dtype=np.float32)
    gi = np.arange(K) // g
    m = (-(z + 1).astype(np.float32) * s)           # exact
    out = np.empty(N, np.float32)
    f32 = np.float32
    if order == "plain":
        w = (q.astype(np.float32) * s[gi] + m[gi]).astype(np.float32)  # exact
        acc = np.zeros(N, np.float32)
        for k in range(K):
            acc = (acc.astype(np.float64) + w[k].astype(np.float64) *
                   float(x[k])).astype(np.float32)   # fma: one rounding
        return acc
    spans = K // 32
    qx = q.astype(np.float32).reshape(spans, 32, N)
    xs = x.reshape(spans, 32)
    part = np.empty((spans, N), np.float32)
    for sp in range(spans):
        d = np.zeros((2, N), np.float32)
        sx = f32(0)
        for i in range(32):
            d[i & 1] = (d[i & 1].astype(np.float64) + qx[sp, i].astype(
                np.float64) * float(xs[sp, i])).astype(np.float32)
            sx = f32(sx + xs[sp, i])
        dq = (d[0] + d[1]).astype(np.float32)
        sg, mg = s[sp * 32 // g], m[sp * 32 // g]
        a = (sg.astype(np.float64) * dq).astype(np.float32)
        part[sp] = (a.astype(np.float64) + mg.astype(np.float64) *
                    float(sx)).astype(np.float32)
    # lanes hold spans lane, lane + 256, ...; then a pairwise tree
    lanes = np.zeros((256, N), np.float32)
    for sp in range(spans):
        lanes[sp % 256] = lanes[sp % 256] + part[sp]
    v = lanes
    while v.shape[0] > 1:
        v = (v[: v.shape[0] // 2] + v[v.shape[0] // 2:]).astype(np.float32)
    out[:] = v[0]
    return out
