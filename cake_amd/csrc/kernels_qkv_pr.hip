#include "kernels_common.h"
#include "kernels.h"

// ---------------------------------------------------------------------------
// Partial-rotary form of k_gemv_qkv_rope (kernels_gemv.hip) for models whose
// rope turns only the first rd < hd dims of a head (partial_rotary_factor:
// Phi-4-mini 0.75; phi4/attention.rs:59-66, 86):
// fused rms_norm -> qkv GEMV -> rope over [0, rd) -> KV-cache store.
//
// Same body, load-issue order and grid (Nq/4 blocks of 4 rows) as the
// full-rotation kernel; only the block map differs.  A q/k head owns hd/4
// consecutive blocks:
//   * rd/4 PAIR blocks: block j rotates rows {i0, i0+1, i0+rd/2, i0+rd/2+1},
//     i0 = 2j, with table entries (pos, i0) and (pos, i0+1);
//   * (hd-rd)/4 PASS blocks: block j owns rows rd+4j .. rd+4j+3 and stores
//     RNE_bf16 of the sums unrotated, q into the activation buffer in place,
//     k into cache slot pos.
// V blocks follow as before.  The tables are (max_seq, rd/2) f32: the row
// stride is rd/2, not hd/2.  Pass and V blocks read pair 0 so that the table
// loads stay branch-free and in range.  rd % 4 == 0 and (hd - rd) % 4 == 0 are
// the launcher's contract.  It is a separate translation unit so that the
// register allocation of the GEMV family in kernels_gemv.hip stays what it
// was (kernels_common.h, rule 19).
// ---------------------------------------------------------------------------
template <int KB>
__global__ __launch_bounds__(256) void k_gemv_qkv_rope_pr(
    const u16* __restrict__ W, const u16* __restrict__ x,
    u16* __restrict__ out, const u16* __restrict__ nw, float eps,
    u16* __restrict__ kc, u16* __restrict__ vc, u16* __restrict__ vtc,
    const float* __restrict__ cost, const float* __restrict__ sint,
    const int* __restrict__ pos, int nh, int nkv, int hd, int rd, int max_seq,
    int K) {
  const int t = threadIdx.x;
  const int wid = t / WAVE, lane = t % WAVE;
  const int half = rd / 2;               // rotated pairs = table row stride
  const int hblk = hd / 4;               // blocks per q/k head
  const int pblk = rd / 4;               // of which pair blocks, first
  const int nqk = (nh + nkv) * hblk;     // q/k blocks ahead of v blocks
  const int b = blockIdx.x;
  // rows[] = the 4 output rows this block computes; d0 = the first one's
  // offset in its head; second = the offset of rows[2] from rows[0]
  int rows[4];
  enum { PAIR, PASS, VBLK } kind;
  int head = 0, i0 = 0, d0, second;
  if (b < nqk) {
    head = b / hblk;
    const int bb = b % hblk;
    if (bb < pblk) {
      kind = PAIR;
      i0 = bb * 2;
      d0 = i0;
      second = half;
    } else {
      kind = PASS;
      d0 = rd + (bb - pblk) * 4;
      second = 2;
    }
    const int base = head * hd;          // q heads then k heads, contiguous
    rows[0] = base + d0;
    rows[1] = base + d0 + 1;
    rows[2] = base + d0 + second;
    rows[3] = base + d0 + second + 1;
  } else {
    kind = VBLK;
    const int vrow0 = (nh + nkv) * hd + (b - nqk) * 4;
    head = (b - nqk) / hblk;             // kv head
    d0 = ((b - nqk) % hblk) * 4;
    second = 2;
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
  // of it hipcc parks every x/weight load behind the wait on pos): pos and
  // the block's two cos/sin pairs.  i0 == 0 in pass and V blocks, and
  // i0 + 1 < rd/2 always (rd >= 4), so every load is inside row pos.
  const int p = *pos;
  const float rc0 = cost[(size_t)p * half + i0];
  const float rc1 = cost[(size_t)p * half + i0 + 1];
  const float rs0 = sint[(size_t)p * half + i0];
  const float rs1 = sint[(size_t)p * half + i0 + 1];
  // pin the loads HERE: the tables are read-only __restrict__, so hipcc
  // otherwise sinks them into thread 0's epilogue branch, behind the final
  // barrier
  asm volatile("" ::"s"(rc0), "s"(rc1), "s"(rs0), "s"(rs1));

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
    if (kind == VBLK) {
      u16* dst = vc + ((size_t)head * max_seq + p) * hd + d0;
      u16* dstt = vtc + (size_t)head * hd * max_seq + (size_t)d0 * max_seq + p;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const u16 bv = f2b(s[r]);
        dst[r] = bv;
        dstt[(size_t)r * max_seq] = bv;
      }
    } else {
      u16 o[4];
      if (kind == PAIR) {
        o[0] = f2b(s[0] * rc0 - s[2] * rs0);
        o[1] = f2b(s[1] * rc1 - s[3] * rs1);
        o[2] = f2b(s[2] * rc0 + s[0] * rs0);
        o[3] = f2b(s[3] * rc1 + s[1] * rs1);
      } else {  // pass-through rows: stored as projected
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = f2b(s[r]);
      }
      // q -> activation buffer, in place; k -> cache slot p
      u16* dst = head < nh
                     ? out + (size_t)head * hd + d0
                     : kc + ((size_t)(head - nh) * max_seq + p) * hd + d0;
      dst[0] = o[0];
      dst[1] = o[1];
      dst[second] = o[2];
      dst[second + 1] = o[3];
    }
  }
}

// same grid and KB policy as launch_gemv_qkv_rope
void launch_gemv_qkv_rope_pr(const u16* W, const u16* x, u16* out,
                             const u16* nw, float eps, u16* kc, u16* vc,
                             u16* vtc, const float* cost, const float* sint,
                             const int* pos, int nh, int nkv, int hd, int rd,
                             int max_seq, int K, hipStream_t s) {
  const int nblk = (nh + 2 * nkv) * hd / 4;
  dim3 grid(nblk);
#define QKRP(KB)                                                             \
  hipLaunchKernelGGL((k_gemv_qkv_rope_pr<KB>), grid, dim3(256), 0, s, W, x,  \
                     out, nw, eps, kc, vc, vtc, cost, sint, pos, nh, nkv,    \
                     hd, rd, max_seq, K)
  const int kb = gemv_qkv_rope_kb(K);
  if (kb == 1) QKRP(1);
  else if (kb == 2) QKRP(2);
  else if (kb == 4) QKRP(4);
  else QKRP(8);
#undef QKRP
}
