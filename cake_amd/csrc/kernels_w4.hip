#include "kernels_common.h"
#include "kernels.h"

#include <algorithm>

// ---------------------------------------------------------------------------
// GPTQ 4-bit GEMV family (decode) + dequant (prefill).  Its own translation
// unit: co-compiled template families perturb each other's register
// allocation (DESIGN.md engineering note).
//
// Device layout (engine.hip w4_repack, one host routine for the loader and the
// op entries): W is out-major, row j = K/8 words, word w of a row holds
// k = 8w..8w+7 with nibble b = k % 8 at bits 4b..4b+3 (the checkpoint's own
// nibble order, transposed); sz[j][gi] = {s, -(z+1)*s} as an f32 pair, both
// exact.  W[j,k] = q*s - (z+1)*s; q*s + m is exact in f32 (an integer in
// [-16,14] times an 11-bit scale), so a single fma dequantizes exactly.
//
// k_gemv_w4<ROWS, EPI, KB>: one 16-B nontemporal load = 32 weights of one row;
// every load of a thread (weights, then the {s,m} pairs) is issued at kernel
// entry with addresses CLAMPED into the buffer (no guards: DESIGN.md §4 load-
// issue discipline); a lane whose k-span lies past K contributes through a
// zeroed x.  g % 32 == 0 keeps a lane's 32-k span inside one group, so per
// (row, load) a thread computes s * sum(q x) + m * sum(x); sum(x) is shared
// by all rows.  KB counts 4096-wide k blocks: KB 2|4|8 = 256 lanes over
// 8192-wide slabs (KB/2 loads per row); KB 1 (K <= 4096) would idle half of
// such a block, so there the two 128-lane halves each own ROWS/2 of the
// block's rows.  EPI 0 = bf16 out, 1 = bf16 out + res (res may alias out).
// No fused-norm variant: the engine runs k_rmsnorm first (split norm).
// ---------------------------------------------------------------------------
template <int NR, int KB>
__device__ inline void w4_dot(const u32* __restrict__ W,
                              const float2* __restrict__ sz,
                              const u16* __restrict__ x, const int (&rows)[NR],
                              int K, int G, int g, float (&acc)[NR]) {
  constexpr int NL = KB == 1 ? 1 : KB / 2;
  const int tl = KB == 1 ? (threadIdx.x & 127) : threadIdx.x;
  const int K8 = K >> 3;
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
  float2 sm[NR][NL];
#pragma unroll
  for (int i = 0; i < NL; ++i) {
    const int gi = k0c[i] / g;
#pragma unroll
    for (int r = 0; r < NR; ++r) sm[r][i] = sz[(size_t)rows[r] * G + gi];
  }
  // x -> registers (f32), zero past K; sum(x) per load span
  float xr[NL][32], sx[NL];
#pragma unroll
  for (int i = 0; i < NL; ++i) {
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const short8 xv = *reinterpret_cast<const short8*>(x + k0c[i] + q * 8);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float v = live[i] ? b2f((u16)xv[j]) : 0.f;
        xr[i][q * 8 + j] = v;
        s += v;
      }
    }
    sx[i] = s;
  }
#pragma unroll
  for (int r = 0; r < NR; ++r) acc[r] = 0.f;
#pragma unroll
  for (int r = 0; r < NR; ++r)
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      float d0 = 0.f, d1 = 0.f;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const u32 word = wv[r][i][w];
        const u32 lo = word & 0x0F0F0F0Fu;         // nibbles 0,2,4,6
        const u32 hi = (word >> 4) & 0x0F0F0F0Fu;  // nibbles 1,3,5,7
#pragma unroll
        for (int b = 0; b < 4; ++b) {  // v_cvt_f32_ubyteN
          d0 = fmaf((float)((lo >> (8 * b)) & 0xFFu), xr[i][w * 8 + 2 * b],
                    d0);
          d1 = fmaf((float)((hi >> (8 * b)) & 0xFFu),
                    xr[i][w * 8 + 2 * b + 1], d1);
        }
      }
      acc[r] = fmaf(sm[r][i].x, d0 + d1, acc[r]);
      acc[r] = fmaf(sm[r][i].y, sx[i], acc[r]);
    }
}

// block reduction of NRED per-thread partials -> red[.][wave]
template <int NRED>
__device__ inline void w4_reduce(const float (&acc)[NRED],
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
__device__ inline float w4_red_get(const float (&row)[4], int h) {
  if (KB == 1) return row[2 * h] + row[2 * h + 1];
  return row[0] + row[1] + row[2] + row[3];
}

template <int ROWS, int EPI, int KB>
__global__ __launch_bounds__(256) void k_gemv_w4(
    const u32* __restrict__ W, const float2* __restrict__ sz,
    const u16* __restrict__ x, u16* out, const u16* res, int N, int K, int G,
    int g) {
  constexpr int RT = KB == 1 ? ROWS / 2 : ROWS;  // rows per thread
  const int t = threadIdx.x;
  const int half = KB == 1 ? (t >> 7) : 0;
  const int rbase = blockIdx.x * ROWS + half * RT;
  int rows[RT];
#pragma unroll
  for (int r = 0; r < RT; ++r) rows[r] = min(rbase + r, N - 1);
  float acc[RT];
  w4_dot<RT, KB>(W, sz, x, rows, K, G, g, acc);
  __shared__ float red[RT][4];
  w4_reduce<RT>(acc, red);
  if (t < ROWS) {
    const int row = blockIdx.x * ROWS + t;  // == rbase(h) + t % RT
    if (row < N) {
      const float v = w4_red_get<KB>(red[t % RT], t / RT);
      out[row] = EPI == 1 ? f2b(v + b2f(res[row])) : f2b(v);
    }
  }
}

// out[c] = silu(g_c) * u_c, gate rows [0, I), up rows [I, 2I) of one fused
// tensor; x already normalized.  ROWS channels per block, 2 rows each.
template <int ROWS, int KB>
__global__ __launch_bounds__(256) void k_gemv_gateup_w4(
    const u32* __restrict__ W, const float2* __restrict__ sz,
    const u16* __restrict__ x, u16* __restrict__ out, int I, int K, int G,
    int g) {
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
  w4_dot<2 * RT, KB>(W, sz, x, rows, K, G, g, acc);
  __shared__ float red[2 * RT][4];
  w4_reduce<2 * RT>(acc, red);
  if (t < ROWS) {
    const int c = blockIdx.x * ROWS + t;
    if (c < I) {
      const float gv = w4_red_get<KB>(red[t % RT], t / RT);
      const float uv = w4_red_get<KB>(red[RT + t % RT], t / RT);
      out[c] = f2b(gv / (1.f + __expf(-gv)) * uv);
    }
  }
}

// packed 4-bit -> bf16 (N, K) row-major (prefill: dequant the layer's weight
// into the shared scratch, then the bf16 MFMA GEMM).  One word (8 weights,
// one group since g % 8 == 0) per thread iteration: exact fma, RNE to bf16.
__global__ void k_dequant_w4(const u32* __restrict__ W,
                             const float2* __restrict__ sz,
                             u16* __restrict__ out, int N, int K, int G,
                             int g) {
  const size_t K8 = (size_t)(K >> 3);
  const size_t total = (size_t)N * K8;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += stride) {
    const size_t row = i / K8;
    const int k = (int)(i % K8) * 8;
    const u32 word = W[i];
    const float2 m = sz[row * G + k / g];
    short8 o;
#pragma unroll
    for (int b = 0; b < 8; ++b)
      o[b] = (short)f2b(fmaf((float)((word >> (4 * b)) & 0xFu), m.x, m.y));
    *reinterpret_cast<short8*>(out + i * 8) = o;
  }
}

// random nibbles for synthetic 4-bit weights
__global__ void k_fill_random_u32(u32* __restrict__ out, size_t n,
                                  uint64_t seed) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    uint64_t z = seed + 0x9e3779b97f4a7c15ull * (i + 1);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    z ^= z >> 31;
    out[i] = (u32)(z >> 32);
  }
}

// ---- host-side kernel choices (shared with cake_hip_linear_dispatch_w4) ---
int gemv_w4_kb(int K) {  // 4096-wide k blocks in registers (K <= 32768)
  return K <= 4096 ? 1 : K <= 8192 ? 2 : K <= 16384 ? 4 : 8;
}
// 4 rows per block.  8 measured slower on Llama-3-8B decode (CAKE_W4_ROWS=8:
// 478.9 vs 494 tok/s), so the knob stays an A/B switch only.
int gemv_w4_rows_policy(int N, int K) {
  static const int env_rows = [] {
    const char* v = getenv("CAKE_W4_ROWS");
    return v ? atoi(v) : 0;
  }();
  (void)N;
  if (gemv_w4_kb(K) == 8) return 4;  // 8 rows x 4 loads would not fit
  return env_rows == 8 ? 8 : 4;
}

void launch_gemv_w4(const u32* W, const float* sz, const u16* x, u16* out,
                    const u16* res, int N, int K, int group, int epi,
                    hipStream_t s, int rows_override) {
  const int kb = gemv_w4_kb(K);
  int rows = rows_override ? rows_override : gemv_w4_rows_policy(N, K);
  if (kb == 8) rows = 4;
  const int G = K / group;
  const float2* sz2 = reinterpret_cast<const float2*>(sz);
#define W4_L(R, EPI, KB)                                                   \
  hipLaunchKernelGGL((k_gemv_w4<R, EPI, KB>), dim3((N + R - 1) / R),       \
                     dim3(256), 0, s, W, sz2, x, out, res, N, K, G, group)
#define W4_KB(R, EPI)                            \
  do {                                           \
    if (kb == 1) W4_L(R, EPI, 1);                \
    else if (kb == 2) W4_L(R, EPI, 2);           \
    else W4_L(R, EPI, 4);                        \
  } while (0)
  if (kb == 8) {
    if (epi == 1) W4_L(4, 1, 8); else W4_L(4, 0, 8);
  } else if (rows == 8) {
    if (epi == 1) W4_KB(8, 1); else W4_KB(8, 0);
  } else {
    if (epi == 1) W4_KB(4, 1); else W4_KB(4, 0);
  }
#undef W4_KB
#undef W4_L
}

// 4 channels (8 weight rows) per block; 8 channels measured slower
void launch_gemv_gateup_w4(const u32* W, const float* sz, const u16* x,
                           u16* out, int I, int K, int group, hipStream_t s) {
  const int kb = gemv_w4_kb(K);  // K = hidden <= 16384 (engine create, op)
  const int G = K / group;
  const float2* sz2 = reinterpret_cast<const float2*>(sz);
  dim3 grid((I + 3) / 4);
#define GU4(KB)                                                              \
  hipLaunchKernelGGL((k_gemv_gateup_w4<4, KB>), grid, dim3(256), 0, s, W,    \
                     sz2, x, out, I, K, G, group)
  if (kb == 1) GU4(1);
  else if (kb == 2) GU4(2);
  else GU4(4);
#undef GU4
}

void launch_dequant_w4(const u32* W, const float* sz, u16* out, int N, int K,
                       int group, hipStream_t s) {
  const size_t total = (size_t)N * (K / 8);
  const int blocks = (int)std::min<size_t>(4096, (total + 255) / 256);
  hipLaunchKernelGGL(k_dequant_w4, dim3(blocks), dim3(256), 0, s, W,
                     reinterpret_cast<const float2*>(sz), out, N, K,
                     K / group, group);
}

void launch_fill_random_u32(u32* out, size_t n, uint64_t seed,
                            hipStream_t s) {
  hipLaunchKernelGGL(k_fill_random_u32, dim3(2048), dim3(256), 0, s, out, n,
                     seed);
}
