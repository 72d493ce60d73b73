#include "kernels_common.h"
#include "kernels.h"

// ---------------------------------------------------------------------------
// MFMA prefill attention at head_dim 64 and 96 (Qwen2.5-0.5B, Llama-3.2-1B,
// SmolLM2, TinyLlama; Phi-3-mini).  Its own translation unit: no kernel of
// kernels_attn.hip changes by an instruction (kernels_common.h, rule 19).
//
// Semantics of k_attn_prefill_mfma2: causal, GQA, optional sliding window,
// f32 online softmax, P rounded to bf16 for PV, bf16 in and out, K from kc,
// V from the transposed cache vtc, scale rsqrt(HD).
//
// Why not k_attn_prefill_mfma2 with 128 -> HD: per score the softmax work
// (mask, max, exp, sum, bf16 pack, half exchange, rescale, barrier) does not
// shrink with the head, the MFMA work does.  So the fixed work is cut instead:
//
//   block   4 waves = 128 query rows of one head, longest blocks first
//           (reversed qb0), __launch_bounds__(256, 2): 14 heads at S = 2048
//           are 224 blocks, a 256-row block would leave CUs empty.
//   wave    32 query rows.  P^T = mfma_32x32x16_bf16(K, Q) (swapped, HD/16
//           k-steps): a softmax column (one query) is lane-local.
//   stage   64 key positions = two 32-row sub-tiles, two P accumulators (two
//           independent MFMA chains), ONE running-max / rescale step and ONE
//           barrier: per position half the barriers, alpha steps and
//           rescales of a 32-position step, and the MFMA count per stage that
//           hd 128 has per 32 positions.  A wave whose last (diagonal) stage
//           needs only sub-tile 0 skips sub-tile 1's MFMAs (wave-uniform).
//   PV      O^T = mfma(V^T, P^T): C[i = dim][j = query], HD/32 accumulators
//           of 16 f32.  This is the one departure from the hd-128 kernels,
//           which form O = P.V with the query along C's rows and so need 16
//           cross-lane alpha broadcasts (ds_bpermute) per rescale and 16 for
//           the final 1/l.  With O transposed the query stays the lane, as
//           in P^T: alpha and 1/l are lane-local scalars, no broadcast at
//           all.  The A-fragment of V^T and the B-fragment of P^T are the
//           fragments O = P.V uses, with the operands exchanged.  The store
//           writes 4 consecutive dims (8 B) per lane and register group.
//   half exchange
//           not halfswap32 (swap x with itself, then select: 2 swaps and 2
//           selects per fragment word pair): ONE v_permlane32_swap of the
//           pair (a, b) = (pk[4k + e], pk[4k + 2 + e]) leaves fragment word e
//           in a and word 2 + e in b for BOTH lane halves (the lower half
//           keeps its a and receives the upper half's a, the upper half
//           keeps its b and receives the lower half's b), so a 64-position
//           stage costs 8 swaps and no select.
//   VALU    scores live in the log2 domain (scale * log2 e folded into one
//           multiply, v_exp_f32 direct); -inf rows are guarded once per row
//           (mref), not per score; a stage that lies wholly below the wave's
//           diagonal and inside its window skips the mask; P is packed with
//           the hardware bf16 conversion (round to nearest even, as f2b).
//
// LDS, double buffered, one raw barrier per stage, register-staged in 16-B
// units (HD/32 = 2 | 3 units per lane for each of K and V^T) behind counted
// vmcnt waits as in k_attn_prefill_mfma2:
//   V^T image [HD][64], 128-B rows of 8 units; K image [64][64] at HD 64 the
//   same.  Physical unit = logical unit ^ f(row), f(row) = (row ^ (row >> 3))
//   & 7, applied on the SOURCE address, so staging writes are linear.  A
//   fragment read is one unit per lane, lanes 0..31 / 32..63 on rows r0..r0+31
//   with one logical unit u per half.  On 64 banks a unit's bank group is
//   (row * 8 + phys) mod 16 = 8 * (row & 1) + (u ^ f(row)).  Eight aligned
//   consecutive rows have eight distinct f; rows r and r + 8 have f differing
//   in bit 0 only, so within 16 aligned rows each value of f occurs twice, on
//   rows of opposite parity (r + 8 and r ^ 1): 16 consecutive lanes hit 16
//   distinct groups, and mod 8 (32 banks) 8 consecutive lanes hit 8.
//   K image at HD 96: 192-B rows are no power of two; rows are padded to 13
//   units (208 B), no XOR.  13 is odd, so 16 (8) consecutive rows at one
//   logical unit fall in 16 (8) distinct bank groups.  LDS: 32 KB at HD 64,
//   50 KB at HD 96 (2 * 64 * 208 + 2 * 96 * 128), two blocks per CU.
//
// The cache end: max_seq is a multiple of 32, a stage is 64.  No address is
// formed at or past K row max_seq or V^T column max_seq: K rows clamp to
// max_seq - 1 and V^T units to column max_seq - 8 (a unit is wholly inside
// or wholly outside).  The duplicates are finite cache content under keys
// that are masked: every key beyond the query, outside the window or beyond
// the cache scores -inf before any max or exp, its P is exactly 0, and 0
// times a finite stale V is 0, so slots outside the live context cannot move
// the output by a bit.
//
// No split-KV and no deep-pipeline variants: both measured negative at hd 128
// (profiles/r02_NOTES.md).
//
// Resource report (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage):
//   HD 64: 159 VGPRs, 0 AGPRs, 0 B scratch, LDS 32768 B, 3 waves/SIMD by
//          registers (the 2 x 32 KB blocks per CU of the launch bound fit)
//   HD 96: 200 VGPRs, 0 AGPRs, 0 B scratch, LDS 51200 B, 2 waves/SIMD
// (the live set at HD 96 is Q 24 + O 48 + P 32 + staging 24 plus the packed
// P and addresses; everything stays in VGPRs, the MFMAs take their
// accumulators from them).
//
// Measured: 50 us per launch at S = 2048 on Qwen2.5-0.5B
// (14 heads) against 3200 us of the generic kernel, 10.5 against 97 at
// S = 128: no size rule in attn_prefill_policy.
// ---------------------------------------------------------------------------
namespace {

// Every f32 multiply and add below (score scale, O rescale, row sums) stays
// scalar: this file's device functions, the kernel's lambdas included, are
// compiled without the packed-f32 VALU forms.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(                                       \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

// halfswap32f and pack_bf16 are this file's own copies of the helpers of the
// same names in kernels_common.h: those are compiled with the packed-f32 forms
// enabled, a different target-feature set from the functions in this region,
// and might no longer inline into the kernel.

// x of lane ^ 32
__device__ inline float halfswap32f(float x, int lhalf) {
  union { float f; u32 u; } a{x};
  auto r = __builtin_amdgcn_permlane32_swap(a.u, a.u, false, false);
  a.u = lhalf == 0 ? (u32)r[1] : (u32)r[0];
  return a.f;
}

// two f32 -> packed bf16 pair, round to nearest even (v_cvt_pk_bf16_f32)
__device__ inline u32 pack_bf16(float lo, float hi) {
  f32x2 v = {lo, hi};
  union { bf16x2 b; u32 u; } c{__builtin_convertvector(v, bf16x2)};
  return c.u;
}

__device__ inline int swz8(int row) { return (row ^ (row >> 3)) & 7; }

template <int HD>
__global__ __launch_bounds__(256, 2) void k_attn_prefill_mfma_n(
    const u16* __restrict__ qkv, const u16* __restrict__ kc,
    const u16* __restrict__ vtc, u16* __restrict__ out, int S, int pos0,
    int nh, int nkv, int max_seq, int qkv_stride, int out_stride,
    int window) {
  static_assert(HD == 64 || HD == 96, "head dims served here");
  constexpr int KS = HD / 16;    // k-steps of QK^T
  constexpr int NDB = HD / 32;   // 32-dim output blocks
  constexpr int NU = HD / 32;    // 16-B staging units per lane, K and V^T each
  constexpr int KUPR = HD / 8;   // units per K row
  constexpr int KROW = HD == 64 ? 64 : 104;  // K image row stride, elements
  constexpr int KBUF = 64 * KROW, VBUF = HD * 64;
  __shared__ __attribute__((aligned(16))) u16 kb[2 * KBUF];
  __shared__ __attribute__((aligned(16))) u16 vb[2 * VBUF];

  const int t = threadIdx.x;
  const int w = t / WAVE, lane = t % WAVE;
  const int lhalf = lane >> 5, lq = lane & 31;
  const int h = blockIdx.y;
  const int kvh = h / (nh / nkv);
  const int qb0 = (gridDim.x - 1 - blockIdx.x) * 128;
  const int qb = qb0 + w * 32;
  const bool wactive = qb < S;

  // Q fragments (persistent): B[k = dim][j = query lq]
  bf16x8 qf[KS];
  {
    const int row = min(qb + lq, S - 1);
    const u16* qrow = qkv + (size_t)row * qkv_stride + (size_t)h * HD;
#pragma unroll
    for (int kk = 0; kk < KS; ++kk)
      qf[kk] = *reinterpret_cast<const bf16x8*>(qrow + kk * 16 + lhalf * 8);
  }
  f32x16 oacc[NDB];
#pragma unroll
  for (int db = 0; db < NDB; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) oacc[db][r] = 0.f;
  float m = -INFINITY, l = 0.f;  // log2 domain
  const float c2 = rsqrtf((float)HD) * 1.44269504088896341f;
  const int q_abs = pos0 + qb + lq;
  const int n_wave = pos0 + min(qb + 32, S);
  const int n_blk = pos0 + min(qb0 + 128, S);
  const int nst_w = wactive ? (n_wave + 63) / 64 : 0;
  const int nst_b = (n_blk + 63) / 64;
  const int st0_w = (window > 0) ? max(0, pos0 + qb - (window - 1)) / 64 : 0;
  const int st0_b = (window > 0) ? max(0, pos0 + qb0 - (window - 1)) / 64 : 0;
  const u16* kbase = kc + (size_t)kvh * max_seq * HD;
  const u16* vtbase = vtc + (size_t)kvh * HD * max_seq;

  // staging: unit p * 256 + t of the K image (row-major, KUPR units per row)
  // and of the V^T image (8 units per dim row)
  short8 rk[NU], rv[NU];
  int krow_l[NU], ksrc_l[NU], kdst_l[NU], vsrc_l[NU], vlu_l[NU], vdst_l[NU];
#pragma unroll
  for (int p = 0; p < NU; ++p) {
    const int idx = p * 256 + t;
    const int row = idx / KUPR, pu = idx % KUPR;
    krow_l[p] = row;
    ksrc_l[p] = (HD == 64 ? pu ^ swz8(row) : pu) * 8;
    kdst_l[p] = row * KROW + pu * 8;
    const int d = idx >> 3, vu = idx & 7;
    vsrc_l[p] = d * max_seq;
    vlu_l[p] = (vu ^ swz8(d)) * 8;
    vdst_l[p] = d * 64 + vu * 8;
  }
  const int krow_max = max_seq - 1, vcol_max = max_seq - 8;
  auto load_k = [&](int tb) {
#pragma unroll
    for (int p = 0; p < NU; ++p)
      rk[p] = *reinterpret_cast<const short8*>(
          kbase + (size_t)min(tb + krow_l[p], krow_max) * HD + ksrc_l[p]);
  };
  auto load_v = [&](int tb) {
#pragma unroll
    for (int p = 0; p < NU; ++p)
      rv[p] = *reinterpret_cast<const short8*>(
          vtbase + (size_t)vsrc_l[p] + min(tb + vlu_l[p], vcol_max));
  };
  auto write_k = [&](u16* dst) {
#pragma unroll
    for (int p = 0; p < NU; ++p)
      *reinterpret_cast<short8*>(dst + kdst_l[p]) = rk[p];
  };
  auto write_v = [&](u16* dst) {
#pragma unroll
    for (int p = 0; p < NU; ++p)
      *reinterpret_cast<short8*>(dst + vdst_l[p]) = rv[p];
  };

  // fragment read offsets (elements) of this lane, per sub-tile / dim block
  const int kfrag0 = lq * KROW, kfrag1 = (32 + lq) * KROW;
  const int ksw0 = HD == 64 ? swz8(lq) : 0, ksw1 = HD == 64 ? swz8(32 + lq) : 0;

  load_k(st0_b * 64);
  load_v(st0_b * 64);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  write_k(kb);
  write_v(vb);
  load_k((st0_b + 1) * 64);
  load_v((st0_b + 1) * 64);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();

  int cur = 0;
  for (int st = st0_b; st < nst_b; ++st) {
    const u16* kcur = kb + cur * KBUF;
    const u16* vcur = vb + cur * VBUF;
    u16* kwrt = kb + (cur ^ 1) * KBUF;
    u16* vwrt = vb + (cur ^ 1) * VBUF;
    cur ^= 1;
    const bool compute = wactive && st >= st0_w && st < nst_w;
    const int pkv = st * 64;
    // sub-tile 1 holds a key some query of this wave may see
    const bool two = pkv + 32 < n_wave;
    f32x16 p0, p1;
#pragma unroll
    for (int r = 0; r < 16; ++r) p0[r] = p1[r] = 0.f;
    // one branch around the whole phase, so that the fragment reads batch
    // ahead of the two interleaved MFMA chains
    auto qk = [&](const bool both) {
      bf16x8 k0[KS], k1[KS];
#pragma unroll
      for (int kk = 0; kk < KS; ++kk) {
        const int u = kk * 2 + lhalf;
        k0[kk] = *reinterpret_cast<const bf16x8*>(kcur + kfrag0 +
                                                  (u ^ ksw0) * 8);
        if (both)
          k1[kk] = *reinterpret_cast<const bf16x8*>(kcur + kfrag1 +
                                                    (u ^ ksw1) * 8);
      }
#pragma unroll
      for (int kk = 0; kk < KS; ++kk) {
        p0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(k0[kk], qf[kk], p0, 0, 0,
                                                     0);
        if (both)
          p1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(k1[kk], qf[kk], p1, 0,
                                                       0, 0);
      }
    };
    if (compute) {
      if (two)
        qk(true);
      else
        qk(false);
    }
    // K(st + 1) registers landed (V's NU loads may still be out)
    asm volatile("s_waitcnt vmcnt(%0)" ::"i"(NU) : "memory");
    write_k(kwrt);
    float mnew = m, alpha = 1.f, tsum = 0.f;
    if (compute) {
      // no query of the wave sees past this stage's first key's window edge
      // or short of its last key: every score is visible
      const bool full = pkv + 63 <= pos0 + qb &&
                        (window == 0 || pkv > pos0 + qb + 31 - window);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        p0[r] *= c2;
        p1[r] *= c2;
      }
      if (!full) {
        // reg r -> key row (r & 3) + 8 * (r >> 2) + 4 * lhalf of the sub-tile
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kv0 = pkv + (r & 3) + 8 * (r >> 2) + 4 * lhalf;
          const int kv1 = kv0 + 32;
          const bool v0 =
              kv0 <= q_abs && (window == 0 || kv0 > q_abs - window);
          const bool v1 =
              kv1 <= q_abs && (window == 0 || kv1 > q_abs - window);
          p0[r] = v0 ? p0[r] : -INFINITY;
          p1[r] = v1 ? p1[r] : -INFINITY;
        }
      }
      float tm = -INFINITY;
#pragma unroll
      for (int r = 0; r < 16; ++r) tm = fmaxf(tm, fmaxf(p0[r], p1[r]));
      tm = fmaxf(tm, halfswap32f(tm, lhalf));
      mnew = fmaxf(m, tm);
      // a row with no visible key yet: exp2(-inf - 0) = 0 everywhere
      const float mref = (mnew == -INFINITY) ? 0.f : mnew;
      alpha = __builtin_amdgcn_exp2f(m - mref);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        p0[r] = __builtin_amdgcn_exp2f(p0[r] - mref);
        p1[r] = __builtin_amdgcn_exp2f(p1[r] - mref);
        tsum += p0[r] + p1[r];
      }
      tsum += halfswap32f(tsum, lhalf);
    }
    // V(st + 1) registers landed -> other buffer; re-issue the freed set
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    write_v(vwrt);
    load_k((st + 2) * 64);
    load_v((st + 2) * 64);
    if (compute) {
      // exact skip: no row's max grew, every alpha is 1.0 (the ballot
      // builtin, not __all: a header function without this file's target
      // attribute is not inlined into the kernel)
      const bool norescale = __builtin_amdgcn_ballot_w64(mnew != m) == 0;
      l = l * alpha + tsum;
      m = mnew;
      u32 pk[16];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        pk[i] = pack_bf16(p0[2 * i], p0[2 * i + 1]);
        pk[8 + i] = pack_bf16(p1[2 * i], p1[2 * i + 1]);
      }
      if (!norescale) {
#pragma unroll
        for (int db = 0; db < NDB; ++db)
#pragma unroll
          for (int r = 0; r < 16; ++r) oacc[db][r] *= alpha;
      }
      // PV over four 16-key windows; window kk is registers 8 * (kk & 1) ..
      // + 8 of sub-tile kk >> 1, i.e. pk[4 * kk .. 4 * kk + 4)
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        if (kk < 2 || two) {
          const auto s0 = __builtin_amdgcn_permlane32_swap(
              pk[4 * kk], pk[4 * kk + 2], false, false);
          const auto s1 = __builtin_amdgcn_permlane32_swap(
              pk[4 * kk + 1], pk[4 * kk + 3], false, false);
          union { u32 u[4]; bf16x8 v; } pf;
          pf.u[0] = s0[0];
          pf.u[1] = s1[0];
          pf.u[2] = s0[1];
          pf.u[3] = s1[1];
          const int u = kk * 2 + lhalf;
#pragma unroll
          for (int db = 0; db < NDB; ++db) {
            const int d0 = db * 32 + lq;
            const bf16x8 vf = *reinterpret_cast<const bf16x8*>(
                vcur + d0 * 64 + (u ^ swz8(d0)) * 8);
            oacc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                vf, pf.v, oacc[db], 0, 0, 0);
          }
        }
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // LDS writes visible; cur consumed
  }

  // O^T: lane = query lq, reg r of block db = dim db*32 + (r&3) + 8*(r>>2) +
  // 4*lhalf: four consecutive dims per register group, one 8-B store each
  if (wactive && qb + lq < S) {
    const float inv = 1.f / l;
    u16* orow = out + (size_t)(qb + lq) * out_stride + (size_t)h * HD;
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        uint2 o2;
        o2.x = pack_bf16(oacc[db][4 * g] * inv, oacc[db][4 * g + 1] * inv);
        o2.y = pack_bf16(oacc[db][4 * g + 2] * inv, oacc[db][4 * g + 3] * inv);
        *reinterpret_cast<uint2*>(orow + db * 32 + 8 * g + 4 * lhalf) = o2;
      }
  }
}
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
}  // namespace

void launch_attn_prefill_n(const u16* qkv, const u16* kc, const u16* vtc,
                           u16* out, int S, int pos0, int nh, int nkv, int hd,
                           int max_seq, int qkv_stride, int out_stride,
                           int window, hipStream_t s) {
  const dim3 grid((S + 127) / 128, nh);
  if (hd == 64)
    hipLaunchKernelGGL(k_attn_prefill_mfma_n<64>, grid, dim3(256), 0, s, qkv,
                       kc, vtc, out, S, pos0, nh, nkv, max_seq, qkv_stride,
                       out_stride, window);
  else
    hipLaunchKernelGGL(k_attn_prefill_mfma_n<96>, grid, dim3(256), 0, s, qkv,
                       kc, vtc, out, S, pos0, nh, nkv, max_seq, qkv_stride,
                       out_stride, window);
}
