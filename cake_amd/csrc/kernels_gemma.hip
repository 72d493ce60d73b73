// Gemma 3 kernels (HF Gemma3ForCausalLM): the post-norm + residual add of
// its sandwich norms, the GELU-tanh twins of the gate-up GEMV and of
// silu_mul_rows, and the embedding gathers with the sqrt(H) scale.  A
// translation unit of its own, so that no other family's device code moves
// (kernels_common.h).  Every norm row arrives with 1 + w already folded in
// (weights.hip), as a plain bf16 weight row.
#include <algorithm>

#include "kernels_common.h"
#include "kernels.h"

// gelu_pytorch_tanh(g) = 0.5 g (1 + tanh(u)), u = sqrt(2/pi) (g + 0.044715
// g^3); with tanh(u) = 1 - 2 / (1 + e^(2u)) that is g / (1 + e^(-2u)): the
// silu form with another argument.  e^(-2u) = inf gives -0 for g < 0.
__device__ inline float gelu_tanh(float g) {
  const float u = 0.7978845608028654f * (g + 0.044715f * g * g * g);
  return g / (1.f + __expf(-2.f * u));
}

// ---------------------------------------------------------------------------
// post-norm + residual: x = bf16(x + bf16(rms_norm(t) * w)), one block per
// row (HF rounds the normed value to bf16, then adds in bf16).  cols % 8 == 0.
// Every element of x is read and written by the same thread; t is read only.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void k_postnorm_add(
    u16* __restrict__ x, const u16* __restrict__ t, const u16* __restrict__ w,
    int cols, float eps) {
  const size_t off = (size_t)blockIdx.x * cols;
  const u16* tr = t + off;
  u16* xr = x + off;
  const int tid = threadIdx.x;
  const int nvec = cols / 8;
  float ss = 0.f;
  for (int i = tid; i < nvec; i += blockDim.x) {
    short8 v = *reinterpret_cast<const short8*>(tr + i * 8);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float f = b2f((u16)v[j]);
      ss += f * f;
    }
  }
  ss = wave_sum(ss);
  __shared__ float red[16];
  const int wid = tid / WAVE, lane = tid % WAVE;
  if (lane == 0) red[wid] = ss;
  __syncthreads();
  const int nw = blockDim.x / WAVE;
  float tot = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i)
    if (i < nw) tot += red[i];
  const float scale = rsqrtf(tot / (float)cols + eps);
  for (int i = tid; i < nvec; i += blockDim.x) {
    short8 v = *reinterpret_cast<const short8*>(tr + i * 8);
    short8 wv = *reinterpret_cast<const short8*>(w + i * 8);
    short8 xv = *reinterpret_cast<const short8*>(xr + i * 8);
    short8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float n = b2f(f2b(b2f((u16)v[j]) * scale * b2f((u16)wv[j])));
      o[j] = (short)f2b(b2f((u16)xv[j]) + n);
    }
    *reinterpret_cast<short8*>(xr + i * 8) = o;
  }
}

// ---------------------------------------------------------------------------
// prefill gelu_mul over the fused gate_up buffer (S, 2I): the twin of
// k_silu_mul_rows (kernels_misc.hip), same grid and rounding points.  The
// engine's I is a multiple of 8; any other I (rows then start off a 16-byte
// boundary) takes the scalar loop.
// ---------------------------------------------------------------------------
__global__ void k_gelu_mul_rows(const u16* __restrict__ gu,
                                u16* __restrict__ out, int S, int I) {
  const int nv = I / 8;
  const int s = blockIdx.y;
  const u16* row = gu + (size_t)s * 2 * I;
  if (I % 8 != 0) {
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < I;
         c += gridDim.x * blockDim.x)
      out[(size_t)s * I + c] = f2b(gelu_tanh(b2f(row[c])) * b2f(row[I + c]));
    return;
  }
  for (int v = blockIdx.x * blockDim.x + threadIdx.x; v < nv;
       v += gridDim.x * blockDim.x) {
    short8 g8 = *reinterpret_cast<const short8*>(row + v * 8);
    short8 u8 = *reinterpret_cast<const short8*>(row + I + v * 8);
    short8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e)
      o[e] = (short)f2b(gelu_tanh(b2f((u16)g8[e])) * b2f((u16)u8[e]));
    *reinterpret_cast<short8*>(out + (size_t)s * I + v * 8) = o;
  }
}

// ---------------------------------------------------------------------------
// embedding gathers with HF's embed_scale.to(weight.dtype): every element is
// bf16(row * bf16(sqrt(H))).  One block per row; H % 8 == 0.
// ---------------------------------------------------------------------------
__global__ void k_embed_rows_scaled(const u16* __restrict__ embed,
                                    const u32* __restrict__ ids,
                                    u16* __restrict__ x, int H, float scale) {
  const u16* src = embed + (size_t)ids[blockIdx.x] * H;
  u16* dst = x + (size_t)blockIdx.x * H;
  const int nv = H / 8;
  for (int i = threadIdx.x; i < nv; i += blockDim.x) {
    short8 v = *reinterpret_cast<const short8*>(src + i * 8);
    short8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (short)f2b(b2f((u16)v[j]) * scale);
    *reinterpret_cast<short8*>(dst + i * 8) = o;
  }
}

// ---------------------------------------------------------------------------
// fused [rms_norm ->] gate_up GEMV -> gelu_mul: the twin of k_gemv_gateup
// (kernels_gemv.hip) with the GELU-tanh gate; loads, accumulation order and
// rounding points are those of the silu kernel.  KB = 2048-wide k blocks
// (gemv_kb: 2 | 4 | 8, so every load is the clamped, unguarded form).
// ---------------------------------------------------------------------------
template <int ROWS, bool NORM, int KB>
__global__ __launch_bounds__(256) void k_gemv_gateup_gelu(
    const u16* __restrict__ W, const u16* __restrict__ x,
    u16* __restrict__ out, const u16* __restrict__ nw, float eps, int I,
    int K) {
  static_assert(KB >= 2, "gemv_kb never returns 1");
  const int t = threadIdx.x;
  const int c0 = blockIdx.x * ROWS;
  const int wid = t / WAVE, lane = t % WAVE;
  __shared__ float redg[8][4], redu[8][4];

  // load issue order = consumer order: x first (feeds sumsq), then the norm
  // weights (consumed after the barrier)
  short8 xpre[KB];
#pragma unroll
  for (int i = 0; i < KB; ++i) {
    const int k0c = max(0, min(i * 2048 + t * 8, K - 8));
    xpre[i] = *reinterpret_cast<const short8*>(x + k0c);
  }
  short8 nwpre[NORM ? KB : 1];
  if (NORM) {
#pragma unroll
    for (int i = 0; i < KB; ++i) {
      const int k0c = max(0, min(i * 2048 + t * 8, K - 8));
      nwpre[i] = *reinterpret_cast<const short8*>(nw + k0c);
    }
  }
  // KB == 2 with NORM: the first slab's weight loads go out ahead of the
  // norm's two barriers, as in the silu kernel
  constexpr bool PRE = NORM && KB == 2;
  short8 gpre[PRE ? ROWS : 1], upre[PRE ? ROWS : 1];
  if constexpr (PRE) {
    const int k0c = max(0, min(t * 8, K - 8));
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
      const int rc = min(c0 + r, I - 1);
      gpre[r] = ntload8(W + (size_t)rc * K + k0c);
      upre[r] = ntload8(W + (size_t)(rc + I) * K + k0c);
    }
  }
  float xr[KB * 8];
#pragma unroll
  for (int i = 0; i < KB; ++i) {
    const bool in = i * 2048 + t * 8 < K;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      xr[i * 8 + j] = in ? b2f((u16)xpre[i][j]) : 0.f;
  }
  if (NORM) {
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < KB * 8; ++i) ss += xr[i] * xr[i];
    ss = wave_sum(ss);
    if (lane == 0) redg[0][wid] = ss;
    __syncthreads();
    const float scale =
        rsqrtf((redg[0][0] + redg[0][1] + redg[0][2] + redg[0][3]) /
                   (float)K + eps);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < KB; ++i) {
      const int k0 = i * 2048 + t * 8;
      if (k0 < K) {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          xr[i * 8 + j] =
              b2f(f2b(xr[i * 8 + j] * scale * b2f((u16)nwpre[i][j])));
      }
    }
  }

  float accg[ROWS], accu[ROWS];
#pragma unroll
  for (int r = 0; r < ROWS; ++r) accg[r] = accu[r] = 0.f;
#pragma unroll
  for (int i = 0; i < KB; ++i) {
    const int k0c = max(0, min(i * 2048 + t * 8, K - 8));
    short8 gv[ROWS], uv[ROWS];
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
      if (PRE && i == 0) {
        gv[r] = gpre[r];
        uv[r] = upre[r];
        continue;
      }
      const int rc = min(c0 + r, I - 1);
      gv[r] = ntload8(W + (size_t)rc * K + k0c);
      uv[r] = ntload8(W + (size_t)(rc + I) * K + k0c);
    }
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        accg[r] = fmaf(b2f((u16)gv[r][j]), xr[i * 8 + j], accg[r]);
        accu[r] = fmaf(b2f((u16)uv[r][j]), xr[i * 8 + j], accu[r]);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < ROWS; ++r) {
    float g = wave_sum(accg[r]);
    float u = wave_sum(accu[r]);
    if (lane == 0) { redg[r][wid] = g; redu[r][wid] = u; }
  }
  __syncthreads();
  if (t < ROWS && c0 + t < I) {
    float g = redg[t][0] + redg[t][1] + redg[t][2] + redg[t][3];
    float u = redu[t][0] + redu[t][1] + redu[t][2] + redu[t][3];
    out[c0 + t] = f2b(gelu_tanh(g) * u);
  }
}

// ---------------------------------------------------------------------------
// launch wrappers
// ---------------------------------------------------------------------------
void launch_postnorm_add(u16* x, const u16* t, const u16* w, int rows,
                         int cols, float eps, hipStream_t s) {
  // one row (decode): up to 1024 threads, so a thread holds at most two
  // vectors of a 16384-wide row; many rows (prefill): 256 per block
  const int nvec = cols / 8;
  const int threads =
      rows > 1 ? 256 : std::min(1024, std::max(64, (nvec + 63) / 64 * 64));
  hipLaunchKernelGGL(k_postnorm_add, dim3(rows), dim3(threads), 0, s, x, t, w,
                     cols, eps);
}
void launch_gelu_mul_rows(const u16* gu, u16* out, int S, int I,
                          hipStream_t s) {
  const int nv = I / 8;
  const int bx = std::max(1, std::min((nv + 255) / 256, 8));
  hipLaunchKernelGGL(k_gelu_mul_rows, dim3(bx, S), dim3(256), 0, s, gu, out,
                     S, I);
}
// bf16(sqrt(H)) as a float
static float embed_scale_bf16(int H) { return b2f(f2b(sqrtf((float)H))); }
void launch_embed_rows_scaled(const u16* embed, const u32* ids, u16* x, int S,
                              int H, hipStream_t s) {
  hipLaunchKernelGGL(k_embed_rows_scaled, dim3(S), dim3(256), 0, s, embed, ids,
                     x, H, embed_scale_bf16(H));
}
void launch_embed_token_scaled(const u16* embed, const u32* tok, u16* x, int H,
                               hipStream_t s) {
  launch_embed_rows_scaled(embed, tok, x, 1, H, s);
}
void launch_gemv_gateup_gelu(const u16* W, const u16* x, u16* out,
                             const u16* nw, float eps, int I, int K, int rows,
                             hipStream_t s) {
  if (K > 16384) return;  // guarded at engine create (K = hidden <= 16384)
  const int kb = gemv_kb(K);
#define GUG_KB2(ROWS, KB)                                                   \
  do {                                                                      \
    dim3 grid((I + ROWS - 1) / ROWS);                                       \
    if (nw)                                                                 \
      hipLaunchKernelGGL((k_gemv_gateup_gelu<ROWS, true, KB>), grid,        \
                         dim3(256), 0, s, W, x, out, nw, eps, I, K);        \
    else                                                                    \
      hipLaunchKernelGGL((k_gemv_gateup_gelu<ROWS, false, KB>), grid,       \
                         dim3(256), 0, s, W, x, out, nw, eps, I, K);        \
  } while (0)
#define GUG_KB(KB)                                                          \
  do {                                                                      \
    if (rows >= 8) GUG_KB2(8, KB);                                          \
    else GUG_KB2(4, KB);                                                    \
  } while (0)
  if (kb == 2) GUG_KB(2);
  else if (kb == 4) GUG_KB(4);
  else GUG_KB(8);
#undef GUG_KB
#undef GUG_KB2
}
