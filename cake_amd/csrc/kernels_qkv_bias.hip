#include "kernels_common.h"
#include "kernels.h"

// ---------------------------------------------------------------------------
// Biased twin of k_gemv_qkv_rope (kernels_gemv.hip) for qwen2 / qwen2.5, whose
// q, k and v projections carry an additive bias (attention.rs:95-104, 163):
// fused rms_norm -> qkv GEMV -> + bias -> rope -> KV-cache store.
//
// Same row mapping, load-issue order and epilogue as the unbiased kernel; the
// block's four bias values join the f32 sums s[0..3] ahead of the rotation
// (q, k) and ahead of the V store, so q and k are rounded once, after the
// rope, and V is RNE_bf16(sum + b).  bias is the fused (Nq) f32 row in wqkv's
// row order.  It is a separate translation unit so that the register
// allocation of the GEMV family in kernels_gemv.hip stays what it was
// (kernels_common.h, rule 19).
// ---------------------------------------------------------------------------
template <int KB>
__global__ __launch_bounds__(256) void k_gemv_qkv_rope_bias(
    const u16* __restrict__ W, const u16* __restrict__ x,
    u16* __restrict__ out, const u16* __restrict__ nw, float eps,
    u16* __restrict__ kc, u16* __restrict__ vc, u16* __restrict__ vtc,
    const float* __restrict__ cost, const float* __restrict__ sint,
    const int* __restrict__ pos, const float* __restrict__ bias, int nh,
    int nkv, int hd, int max_seq, int K) {
  const int t = threadIdx.x;
  const int wid = t / WAVE, lane = t % WAVE;
  const int half = hd / 2;
  const int hblk = hd / 4;               // pair-blocks per q/k head
  const int nqk = (nh + nkv) * hblk;     // q/k blocks ahead of v blocks
  const int b = blockIdx.x;
  // rows[] = the 4 output rows this block computes
  int rows[4];
  bool isv;
  int head = 0, i0 = 0;
  if (b < nqk) {
    isv = false;
    head = b / hblk;
    i0 = (b % hblk) * 2;
    const int base = head * hd;          // q heads then k heads, contiguous
    rows[0] = base + i0;
    rows[1] = base + i0 + 1;
    rows[2] = base + i0 + half;
    rows[3] = base + i0 + half + 1;
  } else {
    isv = true;
    const int vrow0 = (nh + nkv) * hd + (b - nqk) * 4;
    rows[0] = vrow0;
    rows[1] = vrow0 + 1;
    rows[2] = vrow0 + 2;
    rows[3] = vrow0 + 3;
  }
  __shared__ float red[4][4];

  // load-issue order of k_gemv_reg: x, norm weights, then row weights
  short8 xpre[KB];
#pragma unroll
  for (int i = 0; i < KB; ++i) {
    const int k0c = max(0, min(i * 2048 + t * 8, K - 8));
    xpre[i] = *reinterpret_cast<const short8*>(x + k0c);
  }
  short8 nwpre[KB];
#pragma unroll
  for (int i = 0; i < KB; ++i) {
    const int k0c = max(0, min(i * 2048 + t * 8, K - 8));
    nwpre[i] = *reinterpret_cast<const short8*>(nw + k0c);
  }
  short8 wpre[KB <= 2 ? 4 : 1][KB <= 2 ? KB : 1];
  if (KB <= 2) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int i = 0; i < KB; ++i) {
        const int k0c = max(0, min(i * 2048 + t * 8, K - 8));
        wpre[r][i] = ntload8(W + (size_t)rows[r] * K + k0c);
      }
  }
  // The epilogue's operands, requested BEHIND the vector load issue (ahead
  // of it hipcc parks every x/weight load behind the wait on pos): pos, the
  // block's two cos/sin pairs, and its four bias values.  rows[0] is a
  // multiple of 4 in a V block (one 16-B load) and even in a q/k block, as is
  // rows[2] = rows[0] + hd/2 (two 8-B loads); hd % 4 == 0 is the launcher's
  // contract and the (Nq) f32 row is 16-B aligned.
  const int p = *pos;
  const float rc0 = cost[(size_t)p * half + i0];
  const float rc1 = cost[(size_t)p * half + i0 + 1];
  const float rs0 = sint[(size_t)p * half + i0];
  const float rs1 = sint[(size_t)p * half + i0 + 1];
  float b0, b1, b2, b3;
  if (isv) {
    const f32x4 bv = *reinterpret_cast<const f32x4*>(bias + rows[0]);
    b0 = bv[0];
    b1 = bv[1];
    b2 = bv[2];
    b3 = bv[3];
  } else {
    const f32x2 lo = *reinterpret_cast<const f32x2*>(bias + rows[0]);
    const f32x2 hi = *reinterpret_cast<const f32x2*>(bias + rows[2]);
    b0 = lo[0];
    b1 = lo[1];
    b2 = hi[0];
    b3 = hi[1];
  }
  // pin the loads HERE: the tables and the bias row are read-only
  // __restrict__, so hipcc otherwise sinks them into thread 0's epilogue
  // branch, behind the final barrier
  asm volatile("" ::"s"(rc0), "s"(rc1), "s"(rs0), "s"(rs1));
  asm volatile("" ::"s"(b0), "s"(b1), "s"(b2), "s"(b3));

  float xr[KB * 8];
#pragma unroll
  for (int i = 0; i < KB; ++i) {
    const bool in = i * 2048 + t * 8 < K;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      xr[i * 8 + j] = in ? b2f((u16)xpre[i][j]) : 0.f;
  }
  {  // fused rms_norm (bit-exact with the unfused pair, see k_gemv_reg)
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < KB * 8; ++i) ss += xr[i] * xr[i];
    ss = wave_sum(ss);
    if (lane == 0) red[0][wid] = ss;
    __syncthreads();
    const float scale =
        rsqrtf((red[0][0] + red[0][1] + red[0][2] + red[0][3]) / (float)K +
               eps);
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

  float acc[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) acc[r] = 0.f;
  if (KB <= 2) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int i = 0; i < KB; ++i) {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          acc[r] = fmaf(b2f((u16)wpre[r][i][j]), xr[i * 8 + j], acc[r]);
      }
  } else {
#pragma unroll
    for (int i = 0; i < KB; ++i) {
      const int k0c = max(0, min(i * 2048 + t * 8, K - 8));
      short8 wv[4];
#pragma unroll
      for (int r = 0; r < 4; ++r)
        wv[r] = ntload8(W + (size_t)rows[r] * K + k0c);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          acc[r] = fmaf(b2f((u16)wv[r][j]), xr[i * 8 + j], acc[r]);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float v = wave_sum(acc[r]);
    if (lane == 0) red[r][wid] = v;
  }
  __syncthreads();
  if (t == 0) {
    float s[4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
      s[r] = red[r][0] + red[r][1] + red[r][2] + red[r][3];
    s[0] += b0;
    s[1] += b1;
    s[2] += b2;
    s[3] += b3;
    if (isv) {
      const int kvh = (rows[0] - (nh + nkv) * hd) / hd;
      const int d0 = rows[0] % hd;
      u16* dst = vc + ((size_t)kvh * max_seq + p) * hd + d0;
      u16* dstt = vtc + (size_t)kvh * hd * max_seq + (size_t)d0 * max_seq + p;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const u16 bv = f2b(s[r]);
        dst[r] = bv;
        dstt[(size_t)r * max_seq] = bv;
      }
    } else {
      u16 o[4];
      o[0] = f2b(s[0] * rc0 - s[2] * rs0);
      o[1] = f2b(s[1] * rc1 - s[3] * rs1);
      o[2] = f2b(s[2] * rc0 + s[0] * rs0);
      o[3] = f2b(s[3] * rc1 + s[1] * rs1);
      if (head < nh) {  // q -> activation buffer, in place
        u16* q = out + (size_t)head * hd + i0;
        q[0] = o[0];
        q[1] = o[1];
        q[half] = o[2];
        q[half + 1] = o[3];
      } else {          // k -> cache slot p
        const int kvh = head - nh;
        u16* dst = kc + ((size_t)kvh * max_seq + p) * hd + i0;
        dst[0] = o[0];
        dst[1] = o[1];
        dst[half] = o[2];
        dst[half + 1] = o[3];
      }
    }
  }
}

// same grid and KB policy as launch_gemv_qkv_rope
void launch_gemv_qkv_rope_bias(const u16* W, const u16* x, u16* out,
                               const u16* nw, float eps, u16* kc, u16* vc,
                               u16* vtc, const float* cost, const float* sint,
                               const int* pos, const float* bias, int nh,
                               int nkv, int hd, int max_seq, int K,
                               hipStream_t s) {
  const int nblk = (nh + 2 * nkv) * hd / 4;
  dim3 grid(nblk);
#define QKRB(KB)                                                             \
  hipLaunchKernelGGL((k_gemv_qkv_rope_bias<KB>), grid, dim3(256), 0, s, W,   \
                     x, out, nw, eps, kc, vc, vtc, cost, sint, pos, bias,    \
                     nh, nkv, hd, max_seq, K)
  const int kb = gemv_qkv_rope_kb(K);
  if (kb == 1) QKRB(1);
  else if (kb == 2) QKRB(2);
  else if (kb == 4) QKRB(4);
  else QKRB(8);
#undef QKRB
}
