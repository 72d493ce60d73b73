// Grouped MFMA decode attention for any GQA ratio 1 <= G <= 16, head dims
// 64 and 128 (opt-in: launch_attn_decode's mq argument / CAKE_ATTN_MQ /
// config key decode_attention "mfma").
//
// Why: k_attn_decode_g splits its 4 waves as GB heads x R residues, which
// only divides for GB in {1, 2, 4}; G = 3, 5, 6, 7 and every hd-64 model ran
// the per-head kernel, which reads each K/V row once per q head.  Here the G
// q rows of one kv head are padded to ONE 16-row MFMA operand, so G is no
// template parameter and K/V are read once per kv head.
//
// Work split, masking, the online-softmax step, the wave merge and the
// split-KV publish / election / combine are shared with the fp8 kernel:
// attn_mq_common.h.  Here steps begin at `start`, which need not be
// tile-aligned (rows are the load granule).
//
// Per 32-position step of a wave (v_mfma_f32_16x16x32_bf16 throughout):
//   scores   D[pos][head] = K (A: 16 positions x 32 dims, 16-B global loads
//            straight into the fragment) x Q^T (B: dims x 16 heads, persistent
//            registers; heads >= G are zero rows).  Lane % 16 = head, the 4
//            registers + lane / 16 = position, so a head's tile max and sum
//            are 8 registers plus two cross-lane steps (xor 16, xor 32).
//            Products of bf16 accumulate in f32: scores are as exact as in
//            the f32 kernels.  Masked positions are selected to -inf before
//            any max or exp; their P is exactly 0.
//   P.V      O^T[d][head] += V^T (A: 16 dims x 32 positions) x P (B).  The D
//            fragment of the scores already IS the B fragment of P under the
//            k-slot permutation slot 8 g + 4 t + r <-> position 16 t + 4 g + r
//            (t = 16-position half, g = lane / 16, r = register), so P never
//            moves between lanes.  P is split into bf16 hi + bf16 lo
//            (lo = bf16(p - hi), |p - hi - lo| <= 2^-17 p): two MFMAs per V
//            fragment keep P at f32-kernel accuracy.  O^T has head = lane % 16
//            like m and l, so the rescale by alpha is lane-local.
//   V^T      the wave stages its 32 V rows row-major in its own LDS slice
//            (16-B global loads -> 16-B LDS writes) and reads the fragments
//            with the LDS transpose load ds_read_b64_tr_b16: within 16 lanes,
//            lane L addresses 4 dims (4 (L % 4) .. + 3) of row L / 4 and lane i
//            receives dim i of those 4 rows.  With rows 16 t + 4 g + (L / 4)
//            that is exactly the permuted k-slot order above.  Rows are padded
//            to HD + 16 elements (stride 72 / 40 dwords) to spread the 16 rows
//            of one read over the banks.
//   loads    the next step's K and V loads are issued after the score MFMAs
//            have consumed the K registers and the LDS writes the V registers;
//            they are unguarded (clamped to end - 1, see k_attn_decode_fused)
//            and wait only at their first use.
//
// Resource report (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage):
//   HD 128: 192 VGPRs + 32 AGPRs, 0 B scratch, LDS 36868 B, 2 waves/SIMD
//   HD 64:  108 VGPRs + 16 AGPRs, 0 B scratch, LDS 20484 B, 4 waves/SIMD
// Measurements: DESIGN section 4.
#include <cstdio>

#include "kernels.h"
#include "attn_mq_common.h"

namespace {

using v4i16 = __attribute__((ext_vector_type(4))) short;
using lds_v4i16 = __attribute__((address_space(3))) v4i16*;

template <int HD>
__global__ __launch_bounds__(256) void k_attn_decode_mq(
    const u16* __restrict__ q, const u16* __restrict__ kc,
    const u16* __restrict__ vc, const int* __restrict__ pos,
    float* __restrict__ ws, u32* __restrict__ cnt, u16* __restrict__ outbuf,
    int nh, int nkv, int max_seq, int nchunk, int window) {
  constexpr int KK = HD / 32;         // score MFMAs per 16 positions
  constexpr int DB = HD / 16;         // 16-dim blocks of O^T
  constexpr int NV = HD / 16;         // 16-B V loads per lane per step
  constexpr int VROW = HD + 16;       // padded LDS row, elements
  constexpr int WSL = 32 * VROW * 2;  // LDS bytes per wave
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
  bf16x8 kf[2][KK];
  uint4v vr[NV];
  auto load_kv = [&](int p0) {
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
      const int pc = min(p0 + 16 * tt + c16, end - 1);
      const u16* krow = kbase + (size_t)pc * HD + 8 * g;
#pragma unroll
      for (int kk = 0; kk < KK; ++kk)
        kf[tt][kk] = *reinterpret_cast<const bf16x8*>(krow + kk * 32);
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int e = i * 512 + lane * 8;
      const int pc = min(p0 + e / HD, end - 1);
      vr[i] = *reinterpret_cast<const uint4v*>(vbase + (size_t)pc * HD +
                                               e % HD);
    }
  };

  const int pw = start + 32 * w;      // this wave's first position
  if (pw < end) load_kv(pw);
  for (int p0 = pw; p0 < end; p0 += 128) {
    // ---- V rows -> this wave's LDS slice ---------------------------------
    mq_wave_sync();                   // the previous step's reads are issued
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int e = i * 512 + lane * 8;
      *reinterpret_cast<uint4v*>(vl + (e / HD) * VROW + e % HD) = vr[i];
    }
    mq_wave_sync();
    // ---- scores ------------------------------------------------------------
    float sc[2][4];
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
      f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < KK; ++kk)
        s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[tt][kk], qf[kk], s, 0,
                                                    0, 0);
#pragma unroll
      for (int r = 0; r < 4; ++r)
        sc[tt][r] =
            (p0 + 16 * tt + 4 * g + r < end) ? s[r] * scale : -INFINITY;
    }
    // next step's loads (clamped; the last step reloads row end - 1)
    load_kv(p0 + 128);
    // ---- online softmax, per head = lane % 16 ------------------------------
    const MqStep st = mq_softmax_step<false>(sc, nullptr, m, l, lhalf);
    // ---- P.V: O^T[d][head] += V^T x (P hi + P lo) --------------------------
    const u16* vrd = vl + (4 * g + (c16 >> 2)) * VROW + 4 * (c16 & 3);
#pragma unroll
    for (int db = 0; db < DB; ++db) {
      union { v4i16 h[2]; bf16x8 v; } vf;
      vf.h[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
          (lds_v4i16)(vrd + db * 16));
      vf.h[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
          (lds_v4i16)(vrd + 16 * VROW + db * 16));
      f32x4 a = acc[db];
#pragma unroll
      for (int r = 0; r < 4; ++r) a[r] *= st.alpha;
      a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf.v, st.phi, a, 0, 0, 0);
      a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf.v, st.plo, a, 0, 0, 0);
      acc[db] = a;
    }
  }

  mq_epilogue<HD, WSL>(smem, acc, m, l, ws, cnt, outbuf, kvh, chunk, G, nchunk,
                       t);
}

}  // namespace

bool attn_decode_mq_on(int nh, int nkv, int hd, int mq) {
  if (mq < 0) {
    const char* e = getenv("CAKE_ATTN_MQ");
    mq = e ? atoi(e) : 0;
  }
  if (mq <= 0) return false;
  return (hd == 64 || hd == 128) && nh > 0 && nkv > 0 && nh % nkv == 0 &&
         nh / nkv <= 16;
}

void launch_attn_decode_mq(const u16* q, const u16* kc, const u16* vc,
                           const int* pos, float* ws, u32* cnt, u16* out,
                           int nh, int nkv, int hd, int max_seq, int nchunk,
                           int window, hipStream_t s) {
  // the combine keeps one weight per (head, chunk) in a [16][64] LDS table
  if (nchunk < 1 || nchunk > 64 || !attn_decode_mq_on(nh, nkv, hd, 1)) {
    fprintf(stderr, "launch_attn_decode_mq: nchunk %d outside [1,64] or shape "
            "(nh %d, nkv %d, hd %d) not served; nothing launched\n", nchunk,
            nh, nkv, hd);
    return;
  }
  if (hd == 128)
    hipLaunchKernelGGL(k_attn_decode_mq<128>, dim3(nchunk, nkv), dim3(256), 0,
                       s, q, kc, vc, pos, ws, cnt, out, nh, nkv, max_seq,
                       nchunk, window);
  else
    hipLaunchKernelGGL(k_attn_decode_mq<64>, dim3(nchunk, nkv), dim3(256), 0,
                       s, q, kc, vc, pos, ws, cnt, out, nh, nkv, max_seq,
                       nchunk, window);
}
