#include "kernels_common.h"
#include "kernels.h"

#include <algorithm>

// ---------------------------------------------------------------------------
// MXFP4 (OCP microscaling FP4) GEMV family (decode) + dequant (prefill).  Its
// own translation unit, as kernels_w4.hip is (DESIGN.md engineering note).
//
// Device layout = checkpoint layout, no repack: W is (N, K/2) bytes, byte b of
// a row holds k = 2b in its low nibble and k = 2b + 1 in its high nibble, so
// read as little-endian u32 a row is K/8 words, word w holds k = 8w..8w+7 with
// nibble j at bits 4j: the out-major layout of kernels_w4.hip.  A nibble is an
// e2m1 code (bit 3 sign; magnitudes 0, .5, 1, 1.5, 2, 3, 4, 6).  sc is
// (N, K/32) E8M0 bytes, one per 32 consecutive k of a row: 2^(s - 127).
//
// k_gemv_mx4<EPI, KB, DOT2>: the work split of k_gemv_w4 (256 lanes, 4 rows
// per block, one 16-B nontemporal load = 32 weights of one row = ONE MX block,
// so one scale byte per (row, load); every load issued at kernel entry with
// addresses clamped into the buffer, a lane past K contributes through a
// zeroed x; KB counts 4096-wide k blocks, at KB 1 the two 128-lane halves own
// two rows each).  The inner loop is the hardware decode: per u32 four
// v_cvt_scalef32_pk_*_fp4 at byte_sel 0..3 with the block's scale, built as
// (u32)s << 23, as the convert's scale operand.  No mask, shift, int->float
// convert, sum(x) term or per-group pair.
//   DOT2 0: v_cvt_scalef32_pk_f32_fp4 -> two f32, two fmas against x unpacked
//           to f32 once per lane (shared by the rows).
//   DOT2 1: v_cvt_scalef32_pk_bf16_fp4 -> a packed bf16 pair into
//           v_dot2_f32_bf16 against x as loaded (a packed bf16 pair): the
//           products are exact (3 x 8 significant bits), x is never unpacked.
// Scale byte 0 decodes as scale 0 instead of 2^-127 (at most 6 * 2^-127 per
// weight; the loader refuses 255 = NaN).  EPI 0 = bf16 out, 1 = bf16 out + res
// (res may alias out).  x is already normalized (split norm, as gptq).
// ---------------------------------------------------------------------------
namespace {

// every f32 multiply and add of this file stays scalar
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(                                       \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

using u8 = unsigned char;
using bf16x2 = __attribute__((ext_vector_type(2))) __bf16;

__device__ inline float mx4_scale(u8 s) {
  union { u32 u; float f; } v{(u32)s << 23};
  return v.f;
}

template <int NR, int KB, bool DOT2>
__device__ inline void mx4_dot(const u32* __restrict__ W,
                               const u8* __restrict__ sc,
                               const u16* __restrict__ x,
                               const int (&rows)[NR], int K,
                               float (&acc)[NR]) {
  constexpr int NL = KB == 1 ? 1 : KB / 2;
  const int tl = KB == 1 ? (threadIdx.x & 127) : threadIdx.x;
  const int K8 = K >> 3, KS = K >> 5;
  int k0c[NL];
  bool live[NL];
#pragma unroll
  for (int i = 0; i < NL; ++i) {
    const int k0 = i * 8192 + tl * 32;
    live[i] = k0 < K;
    k0c[i] = min(k0, K - 32);
  }
  uint4v wv[NR][NL];
#pragma unroll
  for (int r = 0; r < NR; ++r)
#pragma unroll
    for (int i = 0; i < NL; ++i)
      wv[r][i] = __builtin_nontemporal_load(reinterpret_cast<const uint4v*>(
          W + (size_t)rows[r] * K8 + (k0c[i] >> 3)));
  u8 sb[NR][NL];
#pragma unroll
  for (int i = 0; i < NL; ++i)
#pragma unroll
    for (int r = 0; r < NR; ++r)
      sb[r][i] = sc[(size_t)rows[r] * KS + (k0c[i] >> 5)];
  // x: 16 packed bf16 pairs per load span, zero past K
  uint4v xv[NL][4];
#pragma unroll
  for (int i = 0; i < NL; ++i)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint4v v =
          *reinterpret_cast<const uint4v*>(x + k0c[i] + q * 8);
      xv[i][q] = live[i] ? v : uint4v{0u, 0u, 0u, 0u};
    }
#pragma unroll
  for (int r = 0; r < NR; ++r) acc[r] = 0.f;
  if constexpr (DOT2) {
#pragma unroll
    for (int r = 0; r < NR; ++r)
#pragma unroll
      for (int i = 0; i < NL; ++i) {
        const float s = mx4_scale(sb[r][i]);
        float d0 = 0.f, d1 = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          const u32 word = wv[r][i][w];
          union { u32 u; bf16x2 p; } x0{xv[i][w][0]}, x1{xv[i][w][1]},
              x2{xv[i][w][2]}, x3{xv[i][w][3]};
          d0 = __builtin_amdgcn_fdot2_f32_bf16(
              __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(word, s, 0), x0.p, d0,
              false);
          d1 = __builtin_amdgcn_fdot2_f32_bf16(
              __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(word, s, 1), x1.p, d1,
              false);
          d0 = __builtin_amdgcn_fdot2_f32_bf16(
              __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(word, s, 2), x2.p, d0,
              false);
          d1 = __builtin_amdgcn_fdot2_f32_bf16(
              __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(word, s, 3), x3.p, d1,
              false);
        }
        acc[r] += d0 + d1;
      }
  } else {
    // x -> f32 once per lane, shared by the rows
    float xr[NL][32];
#pragma unroll
    for (int i = 0; i < NL; ++i)
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          xr[i][q * 8 + 2 * j] = b2f((u16)(xv[i][q][j] & 0xFFFFu));
          xr[i][q * 8 + 2 * j + 1] = b2f((u16)(xv[i][q][j] >> 16));
        }
#pragma unroll
    for (int r = 0; r < NR; ++r)
#pragma unroll
      for (int i = 0; i < NL; ++i) {
        const float s = mx4_scale(sb[r][i]);
        float d0 = 0.f, d1 = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          const u32 word = wv[r][i][w];
          const f32x2 v0 =
              __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(word, s, 0);
          const f32x2 v1 =
              __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(word, s, 1);
          const f32x2 v2 =
              __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(word, s, 2);
          const f32x2 v3 =
              __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(word, s, 3);
          d0 = fmaf(v0[0], xr[i][w * 8 + 0], d0);
          d1 = fmaf(v0[1], xr[i][w * 8 + 1], d1);
          d0 = fmaf(v1[0], xr[i][w * 8 + 2], d0);
          d1 = fmaf(v1[1], xr[i][w * 8 + 3], d1);
          d0 = fmaf(v2[0], xr[i][w * 8 + 4], d0);
          d1 = fmaf(v2[1], xr[i][w * 8 + 5], d1);
          d0 = fmaf(v3[0], xr[i][w * 8 + 6], d0);
          d1 = fmaf(v3[1], xr[i][w * 8 + 7], d1);
        }
        acc[r] += d0 + d1;
      }
  }
}

// block reduction of NRED per-thread partials -> red[.][wave]
template <int NRED>
__device__ inline void mx4_reduce(const float (&acc)[NRED],
                                  float (&red)[NRED][4]) {
  const int wid = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
#pragma unroll
  for (int r = 0; r < NRED; ++r) {
    const float v = wave_sum(acc[r]);
    if (lane == 0) red[r][wid] = v;
  }
  __syncthreads();
}
// the sum for half-block `h` (KB 1: waves 2h, 2h+1; else all four)
template <int KB>
__device__ inline float mx4_red_get(const float (&row)[4], int h) {
  if (KB == 1) return row[2 * h] + row[2 * h + 1];
  return row[0] + row[1] + row[2] + row[3];
}

constexpr int MX4_ROWS = 4;  // rows (gate-up: channels) per block

template <int EPI, int KB, bool DOT2>
__global__ __launch_bounds__(256) void k_gemv_mx4(
    const u32* __restrict__ W, const u8* __restrict__ sc,
    const u16* __restrict__ x, u16* out, const u16* res, int N, int K) {
  constexpr int ROWS = MX4_ROWS;
  constexpr int RT = KB == 1 ? ROWS / 2 : ROWS;  // rows per thread
  const int t = threadIdx.x;
  const int half = KB == 1 ? (t >> 7) : 0;
  const int rbase = blockIdx.x * ROWS + half * RT;
  int rows[RT];
#pragma unroll
  for (int r = 0; r < RT; ++r) rows[r] = min(rbase + r, N - 1);
  float acc[RT];
  mx4_dot<RT, KB, DOT2>(W, sc, x, rows, K, acc);
  __shared__ float red[RT][4];
  mx4_reduce<RT>(acc, red);
  if (t < ROWS) {
    const int row = blockIdx.x * ROWS + t;  // == rbase(h) + t % RT
    if (row < N) {
      const float v = mx4_red_get<KB>(red[t % RT], t / RT);
      out[row] = EPI == 1 ? f2b(v + b2f(res[row])) : f2b(v);
    }
  }
}

// out[c] = silu(g_c) * u_c, gate rows [0, I), up rows [I, 2I) of one fused
// tensor; x already normalized.  4 channels per block, 2 rows each.
template <int KB, bool DOT2>
__global__ __launch_bounds__(256) void k_gemv_gateup_mx4(
    const u32* __restrict__ W, const u8* __restrict__ sc,
    const u16* __restrict__ x, u16* __restrict__ out, int I, int K) {
  constexpr int ROWS = MX4_ROWS;
  constexpr int RT = KB == 1 ? ROWS / 2 : ROWS;  // channels per thread
  const int t = threadIdx.x;
  const int half = KB == 1 ? (t >> 7) : 0;
  const int cbase = blockIdx.x * ROWS + half * RT;
  int rows[2 * RT];
#pragma unroll
  for (int r = 0; r < RT; ++r) {
    rows[r] = min(cbase + r, I - 1);
    rows[RT + r] = I + rows[r];
  }
  float acc[2 * RT];
  mx4_dot<2 * RT, KB, DOT2>(W, sc, x, rows, K, acc);
  __shared__ float red[2 * RT][4];
  mx4_reduce<2 * RT>(acc, red);
  if (t < ROWS) {
    const int c = blockIdx.x * ROWS + t;
    if (c < I) {
      const float gv = mx4_red_get<KB>(red[t % RT], t / RT);
      const float uv = mx4_red_get<KB>(red[RT + t % RT], t / RT);
      out[c] = f2b(gv / (1.f + __expf(-gv)) * uv);
    }
  }
}

// packed MXFP4 -> bf16 (N, K) row-major (prefill: dequant the layer's weight
// into the shared scratch, then the bf16 MFMA GEMM).  One word (8 weights of
// one MX block) per thread iteration.  The hardware decode runs at scale 1
// and the block scale is one f32 multiply by a power of two, then the integer
// RNE of f2b: exact for every scale byte, the subnormal bf16 results of
// bytes 0 and 1 included, whatever the converter does with subnormals.
__global__ void k_dequant_mx4(const u32* __restrict__ W,
                              const u8* __restrict__ sc,
                              u16* __restrict__ out, int N, int K) {
  const size_t K8 = (size_t)(K >> 3);
  const size_t total = (size_t)N * K8;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += stride) {
    const u32 word = W[i];
    const float s = mx4_scale(sc[i >> 2]);  // (row, k / 32): K8 = 4 * K/32
    const f32x2 v0 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(word, 1.f, 0);
    const f32x2 v1 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(word, 1.f, 1);
    const f32x2 v2 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(word, 1.f, 2);
    const f32x2 v3 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(word, 1.f, 3);
    short8 o;
    o[0] = (short)f2b(v0[0] * s);
    o[1] = (short)f2b(v0[1] * s);
    o[2] = (short)f2b(v1[0] * s);
    o[3] = (short)f2b(v1[1] * s);
    o[4] = (short)f2b(v2[0] * s);
    o[5] = (short)f2b(v2[1] * s);
    o[6] = (short)f2b(v3[0] * s);
    o[7] = (short)f2b(v3[1] * s);
    *reinterpret_cast<short8*>(out + i * 8) = o;
  }
}

// synthetic E8M0 scale bytes: base - 1, base or base + 1 by a hash of the
// index, a narrow band so the weights keep the RMS the caller asked for
__global__ void k_fill_scale_mx4(u8* __restrict__ out, size_t n,
                                 uint64_t seed, int base) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    uint64_t z = seed + 0x9e3779b97f4a7c15ull * (i + 1);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    z ^= z >> 31;
    out[i] = (u8)(base - 1 + (int)((z >> 40) % 3u));
  }
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

}  // namespace

// ---- host-side kernel choices (shared with cake_hip_linear_dispatch_mx4) --
int gemv_mx4_kb(int K) {  // 4096-wide k blocks in registers (K <= 32768)
  return K <= 4096 ? 1 : K <= 8192 ? 2 : K <= 16384 ? 4 : 8;
}
// Inner loop: 0 = f32 converts + fma, 1 = bf16 converts + dot2.  dot2 measured
// faster on Llama-3-8B decode (545 vs 478 tok/s), so it is the
// default; CAKE_MX4_DOT2=0|1 stays as the A/B switch.
static const int MX4_DOT2_DEFAULT = 1;
int gemv_mx4_dot2_policy() {
  static const int env = [] {
    const char* v = getenv("CAKE_MX4_DOT2");
    return v ? atoi(v) : -1;
  }();
  return env == 0 || env == 1 ? env : MX4_DOT2_DEFAULT;
}

void launch_gemv_mx4(const u32* W, const unsigned char* sc, const u16* x,
                     u16* out, const u16* res, int N, int K, int epi,
                     hipStream_t s, int dot2_override) {
  const int kb = gemv_mx4_kb(K);
  const bool d2 =
      dot2_override >= 0 ? dot2_override == 1 : gemv_mx4_dot2_policy() == 1;
  const dim3 grid((N + MX4_ROWS - 1) / MX4_ROWS);
#define MX4_L(EPI, KB, D2)                                                  \
  hipLaunchKernelGGL((k_gemv_mx4<EPI, KB, D2>), grid, dim3(256), 0, s, W,   \
                     sc, x, out, res, N, K)
#define MX4_KB(EPI, D2)                          \
  do {                                           \
    if (kb == 1) MX4_L(EPI, 1, D2);              \
    else if (kb == 2) MX4_L(EPI, 2, D2);         \
    else if (kb == 4) MX4_L(EPI, 4, D2);         \
    else MX4_L(EPI, 8, D2);                      \
  } while (0)
  if (d2) {
    if (epi == 1) MX4_KB(1, true); else MX4_KB(0, true);
  } else {
    if (epi == 1) MX4_KB(1, false); else MX4_KB(0, false);
  }
#undef MX4_KB
#undef MX4_L
}

void launch_gemv_gateup_mx4(const u32* W, const unsigned char* sc,
                            const u16* x, u16* out, int I, int K,
                            hipStream_t s, int dot2_override) {
  const int kb = gemv_mx4_kb(K);  // K = hidden <= 16384 (engine create, op)
  const bool d2 =
      dot2_override >= 0 ? dot2_override == 1 : gemv_mx4_dot2_policy() == 1;
  const dim3 grid((I + MX4_ROWS - 1) / MX4_ROWS);
#define GUMX(KB, D2)                                                        \
  hipLaunchKernelGGL((k_gemv_gateup_mx4<KB, D2>), grid, dim3(256), 0, s, W, \
                     sc, x, out, I, K)
  if (d2) {
    if (kb == 1) GUMX(1, true);
    else if (kb == 2) GUMX(2, true);
    else GUMX(4, true);
  } else {
    if (kb == 1) GUMX(1, false);
    else if (kb == 2) GUMX(2, false);
    else GUMX(4, false);
  }
#undef GUMX
}

void launch_dequant_mx4(const u32* W, const unsigned char* sc, u16* out, int N,
                        int K, hipStream_t s) {
  const size_t total = (size_t)N * (K / 8);
  const int blocks = (int)std::min<size_t>(4096, (total + 255) / 256);
  hipLaunchKernelGGL(k_dequant_mx4, dim3(blocks), dim3(256), 0, s, W, sc, out,
                     N, K);
}

void launch_fill_scale_mx4(unsigned char* out, size_t n, uint64_t seed,
                           int base, hipStream_t s) {
  const int blocks = (int)std::min<size_t>(2048, (n + 255) / 256);
  hipLaunchKernelGGL(k_fill_scale_mx4, dim3(blocks), dim3(256), 0, s, out, n,
                     seed, base);
}
