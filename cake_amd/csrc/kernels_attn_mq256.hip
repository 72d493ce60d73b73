// Grouped MFMA decode attention for head dim 256 and any GQA ratio
// 1 <= G <= 16 (opt-in: launch_attn_decode's mq256 argument / CAKE_ATTN_MQ256 /
// config key decode_attention "mfma_256").
//
// Why: k_attn_decode_256<1> reads every K and V row once per q head (G = 2, 3
// or 4 times in Falcon3 and Gemma 3), and its scalar grouped form
// (CAKE_ATTN256_GB) is slower still.  k_attn_decode_mq's split does not carry
// over: instantiated at 256 its 32-position step holds 64 registers of K, 64
// of V, 64 of O^T and 32 of Q, which is one wave per SIMD.  Here the step is 16
// positions, so K and V are 32 registers each and two waves share a SIMD.
//
// Work split, masking, the wave merge and the split-KV publish / election /
// combine are those of attn_mq_common.h (grid (nchunk, nkv), 4 waves, the G
// q rows of kv head blockIdx.y padded to ONE 16-row MFMA operand, no block
// barrier in the main loop, mq_epilogue<256, WSL> at the end), except that
// wave w owns positions start + 16 w + 64 i .. + 16.
//
// Per 16-position step of a wave (v_mfma_f32_16x16x32_bf16 throughout):
//   scores   D[pos][head] = K (A: 16 positions x 32 dims, 16-B global loads
//            straight into the fragment, 8 of them) x Q^T (B, persistent;
//            heads >= G are zero rows): 8 MFMAs.  Lane % 16 = head, the 4
//            registers + lane / 16 = position 4 g + r.  Scaled by rsqrt(256) in
//            f32; masked positions are selected to -inf before any max or exp.
//   softmax  mq256_softmax_step: the 16-position form of mq_softmax_step (4
//            registers per head plus the xor 16 / xor 32 steps), P split into
//            bf16 hi + bf16 lo the same way, a masked position's P exactly 0.
//   P.V      O^T[d][head] += V^T x P with hi and lo in ONE MFMA per 16-dim
//            block: the 32 k-slots are {16 positions x hi, the same 16
//            positions x lo}, lane group g holding slots {positions 4g .. 4g+3
//            hi, positions 4g .. 4g+3 lo}.  The B fragment of a lane is its own
//            [hi(4) | lo(4)], so P never moves between lanes; the A fragment
//            of lane (dim i, g) is one ds_read_b64_tr_b16 (dim i of rows
//            4g .. 4g+3) placed in both halves.  The sum over slots is
//            sum_pos V[pos][i] (hi + lo): 16 MFMAs per step, as many per
//            position as k_attn_decode_mq<128> issues.  O^T has head =
//            lane % 16 like m and l, so the rescale by alpha is lane-local; it
//            is skipped in steps where no lane's maximum moved (alpha == 1 in
//            the whole wave), which changes no bit.
//   V^T      the wave stages its 16 V rows row-major in its own LDS slice
//            (8 16-B global loads -> 16-B LDS writes per lane), rows padded to
//            256 + 16 elements = 136 dwords.  136 % 64 = 8: the 8 rows that a
//            half-wave's transpose read touches (8 B per lane, 4 lanes per row)
//            start 8 banks apart and cover all 64 banks once.
//   loads    the next step's K and V loads are issued after the score MFMAs
//            have consumed the K registers and the LDS writes the V registers;
//            they are unguarded (clamped into [start, end - 1]) and wait only
//            at their first use.
//
// LDS: the V stage needs 16 * 272 * 2 = 8704 B per wave, mq_epilogue's merge
// image 16 * 257 * 4 + 128 = 16576 B; the slice is sized for the latter.
//
// Resource report (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage):
//   210 VGPRs + 0 AGPRs, 36 SGPRs, 0 B scratch, no spills, LDS 66308 B,
//   2 waves/SIMD (two blocks per CU by registers and by LDS)
//   (k_attn_decode_mq<256>, for comparison: 252 + 64, 69636 B, 1 wave/SIMD)
// Measurements: DESIGN section 4.
#include <cstdio>

#include "kernels.h"
#include "attn_mq_common.h"

namespace {

using v4i16 = __attribute__((ext_vector_type(4))) short;
using lds_v4i16 = __attribute__((address_space(3))) v4i16*;

// One online-softmax step over a wave's 16 positions, per head = lane % 16:
// mq_softmax_step with one 16-position tile.  sc[r] is the score of position
// 4 (lane / 16) + r, -inf where masked.  p = [hi(4) | lo(4)] is the lane's B
// fragment of P (lo = bf16(p - hi), |p - hi - lo| <= 2^-17 p); a masked
// position's P is exactly 0.  Updates m and l.
struct Mq256Step {
  float alpha;  // rescale of the running O^T and l
  bf16x8 p;
};
__device__ inline Mq256Step mq256_softmax_step(const float (&sc)[4], float& m,
                                               float& l, int lhalf) {
  float tm = fmaxf(fmaxf(sc[0], sc[1]), fmaxf(sc[2], sc[3]));
  tm = fmaxf(tm, __shfl_xor(tm, 16, WAVE));
  tm = fmaxf(tm, halfswap32f(tm, lhalf));
  const float mnew = fmaxf(m, tm);
  const float alpha = (mnew == -INFINITY) ? 0.f : __expf(m - mnew);
  float tsum = 0.f, p[4], d[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    p[r] = (sc[r] == -INFINITY) ? 0.f : __expf(sc[r] - mnew);
    tsum += p[r];
  }
  union { u32 u[4]; bf16x8 v; } pf;
  pf.u[0] = pack_bf16(p[0], p[1]);
  pf.u[1] = pack_bf16(p[2], p[3]);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const u32 h = pf.u[r >> 1];
    union { u32 u; float f; } hv{(r & 1) ? (h & 0xffff0000u) : (h << 16)};
    d[r] = p[r] - hv.f;
  }
  pf.u[2] = pack_bf16(d[0], d[1]);
  pf.u[3] = pack_bf16(d[2], d[3]);
  tsum += __shfl_xor(tsum, 16, WAVE);
  tsum += halfswap32f(tsum, lhalf);
  l = l * alpha + tsum;
  m = mnew;
  return {alpha, pf.v};
}

__global__ __launch_bounds__(256, 2) void k_attn_decode_mq256(
    const u16* __restrict__ q, const u16* __restrict__ kc,
    const u16* __restrict__ vc, const int* __restrict__ pos,
    float* __restrict__ ws, u32* __restrict__ cnt, u16* __restrict__ outbuf,
    int nh, int nkv, int max_seq, int nchunk, int window) {
  constexpr int HD = 256;
  constexpr int KK = HD / 32;    // score MFMAs per step
  constexpr int DB = HD / 16;    // 16-dim blocks of O^T
  constexpr int NV = 16 * HD / 512;  // 16-B V loads per lane per step
  constexpr int VROW = HD + 16;  // padded LDS row, elements
  constexpr int WSL = 16 * (HD + 1) * 4 + 128;  // LDS bytes per wave
  static_assert(16 * VROW * 2 <= WSL && WSL % 16 == 0, "V stage fits");
  __shared__ __attribute__((aligned(16))) unsigned char smem[4 * WSL];

  const int kvh = blockIdx.y, chunk = blockIdx.x;
  const int G = nh / nkv;
  const int n = *pos + 1;
  const DecodeSpan sp = decode_span(n, window, nchunk, chunk);
  const int start = sp.start, end = sp.end;
  const int t = threadIdx.x, w = t / WAVE, lane = t % WAVE;
  const int g = lane >> 4, c16 = lane & 15, lhalf = lane >> 5;

  const u16* kbase = kc + (size_t)kvh * max_seq * HD;
  const u16* vbase = vc + (size_t)kvh * max_seq * HD;
  u16* vl = reinterpret_cast<u16*>(smem + w * WSL);
  const float scale = rsqrtf((float)HD);

  // Q^T fragments: lane holds head c16, dims kk * 32 + 8 g .. + 8
  bf16x8 qf[KK];
  {
    const u16* qrow = q + (size_t)(kvh * G + min(c16, G - 1)) * HD + 8 * g;
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
      union { uint4v u; bf16x8 v; } c;
      c.u = *reinterpret_cast<const uint4v*>(qrow + kk * 32);
      if (c16 >= G) c.u = uint4v{0u, 0u, 0u, 0u};
      qf[kk] = c.v;
    }
  }

  f32x4 acc[DB];
#pragma unroll
  for (int db = 0; db < DB; ++db) acc[db] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, l = 0.f;

  // unguarded loads, addresses clamped into [start, end - 1]
  bf16x8 kf[KK];
  uint4v vr[NV];
  auto load_kv = [&](int p0) {
    const u16* krow = kbase + (size_t)min(p0 + c16, end - 1) * HD + 8 * g;
#pragma unroll
    for (int kk = 0; kk < KK; ++kk)
      kf[kk] = *reinterpret_cast<const bf16x8*>(krow + kk * 32);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int e = i * 512 + lane * 8;
      const int pc = min(p0 + e / HD, end - 1);
      vr[i] = *reinterpret_cast<const uint4v*>(vbase + (size_t)pc * HD +
                                               e % HD);
    }
  };

  const int pw = start + 16 * w;      // this wave's first position
  if (pw < end) load_kv(pw);
  for (int p0 = pw; p0 < end; p0 += 64) {
    // ---- V rows -> this wave's LDS slice ---------------------------------
    mq_wave_sync();                   // the previous step's reads are issued
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int e = i * 512 + lane * 8;
      *reinterpret_cast<uint4v*>(vl + (e / HD) * VROW + e % HD) = vr[i];
    }
    mq_wave_sync();
    // ---- scores ------------------------------------------------------------
    float sc[4];
    {
      f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < KK; ++kk)
        s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[kk], qf[kk], s, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; ++r)
        sc[r] = (p0 + 4 * g + r < end) ? s[r] * scale : -INFINITY;
    }
    // next step's loads (clamped; the last step reloads row end - 1)
    load_kv(p0 + 64);
    // ---- online softmax, per head = lane % 16 ------------------------------
    const Mq256Step st = mq256_softmax_step(sc, m, l, lhalf);
    if (__builtin_amdgcn_ballot_w64(st.alpha != 1.f)) {
#pragma unroll
      for (int db = 0; db < DB; ++db)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[db][r] *= st.alpha;
    }
    // ---- P.V: O^T[d][head] += V^T x [P hi | P lo] --------------------------
    const u16* vrd = vl + (4 * g + (c16 >> 2)) * VROW + 4 * (c16 & 3);
#pragma unroll
    for (int db = 0; db < DB; ++db) {
      union { v4i16 h[2]; bf16x8 v; } vf;
      vf.h[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
          (lds_v4i16)(vrd + db * 16));
      vf.h[1] = vf.h[0];
      acc[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf.v, st.p, acc[db], 0,
                                                        0, 0);
    }
  }

  mq_epilogue<HD, WSL>(smem, acc, m, l, ws, cnt, outbuf, kvh, chunk, G, nchunk,
                       t);
}

}  // namespace

bool attn_decode_mq256_on(int nh, int nkv, int mq256) {
  if (mq256 < 0) {
    const char* e = getenv("CAKE_ATTN_MQ256");
    mq256 = e ? atoi(e) : 0;
  }
  if (mq256 <= 0) return false;
  return nh > 0 && nkv > 0 && nh % nkv == 0 && nh / nkv <= 16;
}

void launch_attn_decode_mq256(const u16* q, const u16* kc, const u16* vc,
                              const int* pos, float* ws, u32* cnt, u16* out,
                              int nh, int nkv, int max_seq, int nchunk,
                              int window, hipStream_t s) {
  // the combine keeps one weight per (head, chunk) in a [16][64] LDS table
  if (nchunk < 1 || nchunk > 64 || !attn_decode_mq256_on(nh, nkv, 1)) {
    fprintf(stderr, "launch_attn_decode_mq256: nchunk %d outside [1,64] or "
            "shape (nh %d, nkv %d) not served; nothing launched\n", nchunk, nh,
            nkv);
    return;
  }
  hipLaunchKernelGGL(k_attn_decode_mq256, dim3(nchunk, nkv), dim3(256), 0, s,
                     q, kc, vc, pos, ws, cnt, out, nh, nkv, max_seq, nchunk,
                     window);
}
