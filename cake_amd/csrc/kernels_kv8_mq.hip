// Grouped MFMA decode attention over the fp8 (e4m3) KV cache, hd 128, any GQA
// ratio 1 <= G <= 16 (opt-in: config key decode_attention "mfma_kv8").
//
// Why: k_attn_decode_kv8<GB> converts every code to f32 and does scalar FMAs
// against q, once per q head (GB 4: four times per K/V element; G = 3, 5, 6, 7
// also read K/V G times).  k_attn_decode_mq serves all G heads of a kv head
// from one 16-row MFMA operand but reads the bf16 cache.  This kernel reads
// the codes once per kv head, converts them once, two per instruction, to
// bf16 (exact: an e4m3 value has 4 significant bits) and runs scores and P.V
// on v_mfma_f32_16x16x32_bf16.
//
// Work split, masking, the online-softmax step, the wave merge and the
// split-KV publish / election / combine are shared with k_attn_decode_mq:
// attn_mq_common.h.
//
// The fp8-specific choices shipped here:
//   K        lane (position c16 = lane % 16, g = lane / 16) takes codes
//            32 g .. 32 g + 31 of its row as two 16-B loads (four lanes cover
//            the 128-B row); score MFMA kk uses codes 8 kk .. + 7 of those, so
//            k-slot 8 g + e of MFMA kk is dim 32 g + 8 kk + e, and the Q^T
//            fragments are loaded in the same order.  8 codes -> one bf16x8
//            operand by four v_cvt_scalef32_pk_bf16_fp8 at scale 1.
//   K scale  applied to the finished score in f32, s * (ks[p] * rsqrt(128)),
//            as k_attn_decode_kv8 does.  The convert's scale operand is NOT
//            used for it: no exactness argument for bf16-subnormal results
//            over k in [-120, 120] is made here, so the f32 form ships.
//   V        vs[p] (a power of two: the product is exact) is folded into P in
//            f32 before the split into bf16 hi + bf16 lo; l sums the unscaled
//            p.  V^T takes the code route: the wave stages its 32 V rows AS
//            CODES in its LDS slice (4.5 KiB with padding instead of 9 KiB of
//            bf16) and reads fragments with ds_read_b64_tr_b8, then converts
//            in registers.  Chosen over convert-into-LDS because it halves
//            LDS write and read traffic and needs one transpose read per
//            16-dim block where the b16 path needs two.  ds_read_b64_tr_b8
//            within 16 lanes: lane L addresses 8 dims (8 (L % 2) .. + 7) of
//            row L / 2, and lane i receives, as bytes 0 .. 7, dim i of those 8
//            rows.  With row j = 16 (j / 4) + 4 g + j % 4 that is the k-slot
//            order of P (slot 8 g + 4 t + r <-> position 16 t + 4 g + r).
//   LDS rows row pitch 144 B; position rho of the step sits in row slot
//            sigma(rho) = rho with bits 3 and 4 swapped, so that the 16 rows
//            one half-wave reads (positions 0-7 and 16-23, or 8-15 and 24-31)
//            are 16 consecutive slots = 64 distinct banks.
//   scales   lane L < 32 loads ks[p0 + L], lane L >= 32 vs[p0 + L - 32] (one
//            clamped dword load, no alignment assumed), staged in the wave's
//            slice behind the V codes; each lane reads back the 2 x 4 K and
//            2 x 4 V scales of its own positions as 16-B LDS reads.
// The wave slices are sized by the merge image (16 heads x 129 f32), which
// the V codes and scales (4864 B) sit inside.
//
// Resource report (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage):
//   128 VGPRs + 40 AGPRs, 0 B scratch, LDS 33796 B, 3 waves/SIMD
//   (k_attn_decode_mq<128>: 192 + 32, 36868 B, 2 waves/SIMD)
// Measurements: DESIGN section 4.
#include <cstdio>

#include "kernels.h"
#include "attn_mq_common.h"

namespace {

using u8 = unsigned char;
using v2i32 = __attribute__((ext_vector_type(2))) int;
using lds_v2i32 = __attribute__((address_space(3))) v2i32*;

// 8 e4m3 codes (bytes 0..3 of w0, then of w1) -> bf16x8, exact
__device__ inline bf16x8 q8_cvt8(u32 w0, u32 w1) {
  union { bf16x2 h[4]; bf16x8 v; } c;
  c.h[0] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w0, 1.f, false);
  c.h[1] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w0, 1.f, true);
  c.h[2] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w1, 1.f, false);
  c.h[3] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w1, 1.f, true);
  return c.v;
}
// LDS row slot of position rho (0..31) of a step: bits 3 and 4 swapped
__device__ inline int q8_slot(int rho) {
  return (rho & 7) | ((rho & 16) >> 1) | ((rho & 8) << 1);
}

__global__ __launch_bounds__(256) void k_attn_decode_kv8_mq(
    const u16* __restrict__ q, const u8* __restrict__ k8,
    const u8* __restrict__ v8, const float* __restrict__ ks,
    const float* __restrict__ vs, const int* __restrict__ pos,
    float* __restrict__ ws, u32* __restrict__ cnt, u16* __restrict__ outbuf,
    int nh, int nkv, int max_seq, int nchunk, int window) {
  constexpr int HD = 128;
  constexpr int KK = HD / 32;         // score MFMAs per 16 positions
  constexpr int DB = HD / 16;         // 16-dim blocks of O^T
  constexpr int VROW = HD + 16;       // padded LDS row of codes, bytes
  constexpr int SOFF = 32 * VROW;     // the step's scales: [ks 32 | vs 32]
  constexpr int OROW = HD + 1;        // merge image row, floats
  constexpr int WSL = 16 * OROW * 4 + 192;  // LDS bytes per wave
  static_assert(SOFF + 64 * 4 <= WSL && WSL % 16 == 0, "V codes + scales fit");
  __shared__ __attribute__((aligned(16))) unsigned char smem[4 * WSL];

  const int kvh = blockIdx.y, chunk = blockIdx.x;
  const int G = nh / nkv;
  const int n = *pos + 1;
  const DecodeSpan sp = decode_span(n, window, nchunk, chunk);
  const int start = sp.start, end = sp.end;
  const int t = threadIdx.x, w = t / WAVE, lane = t % WAVE;
  const int g = lane >> 4, c16 = lane & 15, lhalf = lane >> 5;

  const size_t hb = (size_t)kvh * max_seq;
  const u8* kbase = k8 + hb * HD;
  const u8* vbase = v8 + hb * HD;
  const float* sbase = (lane < 32 ? ks : vs) + hb;
  u8* vl = smem + w * WSL;
  float* sl = reinterpret_cast<float*>(vl + SOFF);
  const float scale = rsqrtf((float)HD);

  // Q^T fragments: lane holds head c16, dims 32 g + 8 kk .. + 8 (K's order)
  bf16x8 qf[KK];
  {
    const u16* qrow = q + (size_t)(kvh * G + min(c16, G - 1)) * HD + 32 * g;
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
      union { uint4v u; bf16x8 v; } c;
      c.u = *reinterpret_cast<const uint4v*>(qrow + kk * 8);
      if (c16 >= G) c.u = uint4v{0u, 0u, 0u, 0u};
      qf[kk] = c.v;
    }
  }

  f32x4 acc[DB];
#pragma unroll
  for (int db = 0; db < DB; ++db) acc[db] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, l = 0.f;

  // unguarded loads, addresses clamped into [start, end - 1]
  uint4v kr[2][2], vr[4];
  float sr;
  auto load_kv = [&](int p0) {
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
      const int pc = min(p0 + 16 * tt + c16, end - 1);
      const u8* krow = kbase + (size_t)pc * HD + 32 * g;
      kr[tt][0] = *reinterpret_cast<const uint4v*>(krow);
      kr[tt][1] = *reinterpret_cast<const uint4v*>(krow + 16);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int pc = min(p0 + 8 * i + (lane >> 3), end - 1);
      vr[i] = *reinterpret_cast<const uint4v*>(vbase + (size_t)pc * HD +
                                               16 * (lane & 7));
    }
    sr = sbase[min(p0 + (lane & 31), end - 1)];
  };

  // this lane's V^T source address: row j = c16 / 2 of its group's 8 rows
  const u8* vrd = vl +
                  q8_slot(16 * (c16 >> 3) + 4 * g + ((c16 >> 1) & 3)) * VROW +
                  8 * (c16 & 1);
  const int pw = start + 32 * w;      // this wave's first position
  if (pw < end) load_kv(pw);
  for (int p0 = pw; p0 < end; p0 += 128) {
    // ---- V codes and the step's scales -> this wave's LDS slice ----------
    mq_wave_sync();                   // the previous step's reads are issued
#pragma unroll
    for (int i = 0; i < 4; ++i)
      *reinterpret_cast<uint4v*>(vl + q8_slot(8 * i + (lane >> 3)) * VROW +
                                 16 * (lane & 7)) = vr[i];
    sl[lane] = sr;
    mq_wave_sync();
    // ---- scores ------------------------------------------------------------
    float sc[2][4];
    f32x4 vsc[2];
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
      f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < KK; ++kk) {
        const uint4v wq = kr[tt][kk >> 1];
        const bf16x8 kf = q8_cvt8(wq[2 * (kk & 1)], wq[2 * (kk & 1) + 1]);
        s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[kk], s, 0, 0, 0);
      }
      const f32x4 ksc = *reinterpret_cast<const f32x4*>(sl + 16 * tt + 4 * g);
      vsc[tt] = *reinterpret_cast<const f32x4*>(sl + 32 + 16 * tt + 4 * g);
#pragma unroll
      for (int r = 0; r < 4; ++r)
        sc[tt][r] = (p0 + 16 * tt + 4 * g + r < end) ? s[r] * (ksc[r] * scale)
                                                     : -INFINITY;
    }
    // next step's loads (clamped; the last step reloads row end - 1)
    load_kv(p0 + 128);
    // ---- online softmax, per head = lane % 16 ------------------------------
    const MqStep st = mq_softmax_step<true>(sc, vsc, m, l, lhalf);
    // ---- P.V: O^T[d][head] += V^T x (P hi + P lo) --------------------------
#pragma unroll
    for (int db = 0; db < DB; ++db) {
      const v2i32 vw =
          __builtin_amdgcn_ds_read_tr8_b64_v2i32((lds_v2i32)(vrd + db * 16));
      const bf16x8 vf = q8_cvt8((u32)vw[0], (u32)vw[1]);
      f32x4 a = acc[db];
#pragma unroll
      for (int r = 0; r < 4; ++r) a[r] *= st.alpha;
      a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, st.phi, a, 0, 0, 0);
      a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, st.plo, a, 0, 0, 0);
      acc[db] = a;
    }
  }

  mq_epilogue<HD, WSL>(smem, acc, m, l, ws, cnt, outbuf, kvh, chunk, G, nchunk,
                       t);
}

}  // namespace

bool attn_decode_kv8_mq_on(int nh, int nkv) {
  return nh > 0 && nkv > 0 && nh % nkv == 0 && nh / nkv <= 16;
}

void launch_attn_decode_kv8_mq(const u16* q, const unsigned char* k8,
                               const unsigned char* v8, const float* ks,
                               const float* vs, const int* pos, float* ws,
                               u32* cnt, u16* out, int nh, int nkv,
                               int max_seq, int nchunk, int window,
                               hipStream_t s) {
  // the combine keeps one weight per (head, chunk) in a [16][64] LDS table
  if (nchunk < 1 || nchunk > 64 || !attn_decode_kv8_mq_on(nh, nkv)) {
    fprintf(stderr, "launch_attn_decode_kv8_mq: nchunk %d outside [1,64] or "
            "shape (nh %d, nkv %d) not served; nothing launched\n", nchunk,
            nh, nkv);
    return;
  }
  hipLaunchKernelGGL(k_attn_decode_kv8_mq, dim3(nchunk, nkv), dim3(256), 0, s,
                     q, k8, v8, ks, vs, pos, ws, cnt, out, nh, nkv, max_seq,
                     nchunk, window);
}
