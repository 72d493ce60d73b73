"""Float64 reference of the MXFP4 linear kernels, written from the format
definition (OCP microscaling FP4 as AMD Quark exports it).
  weight       U8 (N, K/2): byte b of a row = code(k = 2b) | code(2b + 1) << 4
  weight_scale U8 (N, K/32): E8M0, 2^(s - 127); 255 is NaN
  code: bit 3 sign, bits 0..2 magnitude E2M1
  W[j, k] = e2m1(code(j, k)) * 2^(scale(j, k // 32) - 127)"""
import numpy as np

from tests.linear_ref import bf16_bits, silu  # noqa: F401

E2M1 = np.array([0, 0.5, 1, 1.5, 2, 3, 4, 6,
                 -0.0, -0.5, -1, -1.5, -2, -3, -4, -6], dtype=np.float64)


def pack(codes, scale_bytes):
    """codes (N, K) in [0, 15], scale_bytes (N, K/32) -> (weight (N, K/2),
    weight_scale (N, K/32)), both uint8."""
    c = np.asarray(codes).astype(np.uint8)
    s = np.asarray(scale_bytes)
    assert c.max() <= 15 and s.shape == (c.shape[0], c.shape[1] // 32)
    return (np.ascontiguousarray(c[:, 0::2] | (c[:, 1::2] << 4)),
            np.ascontiguousarray(s, dtype=np.uint8))


def dequant(weight, weight_scale):
    """-> W (N, K) float64, exact."""
    w = np.asarray(weight, dtype=np.uint8)
    codes = np.empty((w.shape[0], w.shape[1] * 2), np.uint8)
    codes[:, 0::2] = w & 0xF
    codes[:, 1::2] = w >> 4
    e = np.repeat(np.asarray(weight_scale).astype(np.int64) - 127, 32, axis=1)
    return np.ldexp(E2M1[codes], e)


def gemv_ref(weight, weight_scale, x, res=None):
    """(W x [+ res], A = sum |W||x| [+ |res|]) in float64."""
    W = dequant(weight, weight_scale)
    x = np.asarray(x, dtype=np.float64)
    v, A = W @ x, np.abs(W) @ np.abs(x)
    if res is not None:
        v, A = v + res, A + np.abs(res)
    return v, A


def gateup_ref(weight, weight_scale, x):
    """(silu(g) u, g, u, A_g, A_u) of the fused (2I, K) tensor."""
    v, A = gemv_ref(weight, weight_scale, x)
    I = v.size // 2
    return silu(v[:I]) * v[I:], v[:I], v[I:], A[:I], A[I:]
