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
// Work split, masking, wave merge and the split-KV publish / election /
// combine are those of k_attn_decode_mq<128> (kernels_attn_mq.hip): grid
// (nchunk, nkv), 4 waves, wave w owns positions start + 32 w + 128 i .. + 32
// through its own (m, l, O^T), no block barrier in the main loop, every load
// address clamped into [start, end - 1], only the chunk's end masked to -inf.
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
#include "kernels_common.h"

namespace {

using u8 = unsigned char;
using bf16x2 = __attribute__((ext_vector_type(2))) __bf16;
using v2i32 = __attribute__((ext_vector_type(2))) int;
using lds_v2i32 = __attribute__((address_space(3))) v2i32*;

// x of lane ^ 32 (v_permlane32_swap)
__device__ inline float q8_swap32(float x, int lhalf) {
  union { float f; u32 u; } a{x};
  auto r = __builtin_amdgcn_permlane32_swap(a.u, a.u, false, false);
  a.u = lhalf == 0 ? (u32)r[1] : (u32)r[0];
  return a.f;
}
// two f32 -> packed bf16 pair, round to nearest even (v_cvt_pk_bf16_f32)
__device__ inline u32 q8_pack(float lo, float hi) {
  f32x2 v = {lo, hi};
  union { bf16x2 b; u32 u; } c{__builtin_convertvector(v, bf16x2)};
  return c.u;
}
// 8 e4m3 codes (bytes 0..3 of w0, then of w1) -> bf16x8, exact
__device__ inline bf16x8 q8_cvt8(u32 w0, u32 w1) {
  union { bf16x2 h[4]; bf16x8 v; } c;
  c.h[0] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w0, 1.f, false);
  c.h[1] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w0, 1.f, true);
  c.h[2] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w1, 1.f, false);
  c.h[3] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w1, 1.f, true);
  return c.v;
}
// LDS traffic of one wave is in order; this only keeps the compiler from
// moving a lane's LDS reads across another lane's writes
__device__ inline void q8_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
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
  static_assert(4 * WSL >= (16 * 64 + 16) * 4, "combine staging fits");
  __shared__ __attribute__((aligned(16))) unsigned char smem[4 * WSL];
  __shared__ int elected;

  const int kvh = blockIdx.y, chunk = blockIdx.x;
  const int G = nh / nkv;
  const int n = *pos + 1;
  const int lo = (window > 0 && n > window) ? n - window : 0;
  const int cs = (n - lo + nchunk - 1) / nchunk;
  const int start = lo + chunk * cs;
  const int end = min(start + cs, n);
  const int t = threadIdx.x, w = t / WAVE, lane = t % WAVE;
  const int g = lane >> 4, c16 = lane & 15, lhalf = lane >> 5;
#define WS_STORE(p, v)                                                     \
  __hip_atomic_store((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

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
    q8_wave_sync();                   // the previous step's reads are issued
#pragma unroll
    for (int i = 0; i < 4; ++i)
      *reinterpret_cast<uint4v*>(vl + q8_slot(8 * i + (lane >> 3)) * VROW +
                                 16 * (lane & 7)) = vr[i];
    sl[lane] = sr;
    q8_wave_sync();
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
    float tm = -INFINITY;
#pragma unroll
    for (int tt = 0; tt < 2; ++tt)
#pragma unroll
      for (int r = 0; r < 4; ++r) tm = fmaxf(tm, sc[tt][r]);
    tm = fmaxf(tm, __shfl_xor(tm, 16, WAVE));
    tm = fmaxf(tm, q8_swap32(tm, lhalf));
    const float mnew = fmaxf(m, tm);
    const float alpha = (mnew == -INFINITY) ? 0.f : __expf(m - mnew);
    float tsum = 0.f;
    union { u32 u[4]; bf16x8 v; } phi, plo;
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
      float p[4], d[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float e =
            (sc[tt][r] == -INFINITY) ? 0.f : __expf(sc[tt][r] - mnew);
        tsum += e;
        p[r] = e * vsc[tt][r];        // exact: vs is a power of two
      }
      phi.u[2 * tt] = q8_pack(p[0], p[1]);
      phi.u[2 * tt + 1] = q8_pack(p[2], p[3]);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const u32 h = phi.u[2 * tt + (r >> 1)];
        union { u32 u; float f; } hv{(r & 1) ? (h & 0xffff0000u) : (h << 16)};
        d[r] = p[r] - hv.f;
      }
      plo.u[2 * tt] = q8_pack(d[0], d[1]);
      plo.u[2 * tt + 1] = q8_pack(d[2], d[3]);
    }
    tsum += __shfl_xor(tsum, 16, WAVE);
    tsum += q8_swap32(tsum, lhalf);
    l = l * alpha + tsum;
    m = mnew;
    // ---- P.V: O^T[d][head] += V^T x (P hi + P lo) --------------------------
#pragma unroll
    for (int db = 0; db < DB; ++db) {
      const v2i32 vw =
          __builtin_amdgcn_ds_read_tr8_b64_v2i32((lds_v2i32)(vrd + db * 16));
      const bf16x8 vf = q8_cvt8((u32)vw[0], (u32)vw[1]);
      f32x4 a = acc[db];
#pragma unroll
      for (int r = 0; r < 4; ++r) a[r] *= alpha;
      a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, phi.v, a, 0, 0, 0);
      a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, plo.v, a, 0, 0, 0);
      acc[db] = a;
    }
  }

  // ---- merge the 4 waves' (m, l, O) through LDS ---------------------------
  q8_wave_sync();
  float* fo = reinterpret_cast<float*>(smem + w * WSL);  // [16][OROW], m, l
#pragma unroll
  for (int db = 0; db < DB; ++db)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      fo[c16 * OROW + db * 16 + 4 * g + r] = acc[db][r];
  if (g == 0) {
    fo[16 * OROW + c16] = m;
    fo[16 * OROW + 16 + c16] = l;
  }
  __syncthreads();
  for (int idx = t; idx < G * HD; idx += 256) {
    const int hh = idx / HD, d = idx % HD;
    float mw[4], M = -INFINITY;
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      mw[x] = reinterpret_cast<const float*>(smem + x * WSL)[16 * OROW + hh];
      M = fmaxf(M, mw[x]);
    }
    float o = 0.f, L = 0.f;
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      const float* fx = reinterpret_cast<const float*>(smem + x * WSL);
      const float wt = (mw[x] == -INFINITY) ? 0.f : __expf(mw[x] - M);
      o += wt * fx[hh * OROW + d];
      L += wt * fx[16 * OROW + 16 + hh];
    }
    const int h = kvh * G + hh;
    if (nchunk == 1) {
      outbuf[(size_t)h * HD + d] = f2b(o / L);
    } else {
      float* wsrow = ws + ((size_t)h * nchunk + chunk) * (HD + 4);
      WS_STORE(&wsrow[d], o);
      if (d == 0) {
        WS_STORE(&wsrow[HD], M);
        WS_STORE(&wsrow[HD + 1], L);
      }
    }
  }
  if (nchunk == 1) return;

  // ---- publish, then the last-arriving block of this kv head combines ----
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every wave drains
  __syncthreads();
  if (t == 0) {
    const u32 v = __hip_atomic_fetch_add(&cnt[kvh], 1u, __ATOMIC_RELAXED,
                                         __HIP_MEMORY_SCOPE_AGENT);
    const int last = v % (u32)nchunk == (u32)(nchunk - 1);
    // every block of this launch has arrived: leave the word at zero (the
    // modulo only matters after another kernel's launches on this word)
    if (last)
      __hip_atomic_store(&cnt[kvh], 0u, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
    elected = last;
  }
  __syncthreads();
  if (!elected) return;

  // Combine, as k_attn_decode_mq: one acquire, then plain (16-B) loads of the
  // partials.  Weights: wave = head, lane = chunk; outputs: a thread owns 4
  // dims of one head.
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  float* cw = reinterpret_cast<float*>(smem);  // [16][64] chunk weights
  float* cL = cw + 16 * 64;                    // [16]
  const float* hbase = ws + (size_t)kvh * G * nchunk * (HD + 4);
  for (int hh = w; hh < G; hh += 4) {
    const float* row =
        hbase + ((size_t)hh * nchunk + min(lane, nchunk - 1)) * (HD + 4);
    const float mc = lane < nchunk ? row[HD] : -INFINITY;
    const float lc = lane < nchunk ? row[HD + 1] : 0.f;
    float M = mc;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
      M = fmaxf(M, __shfl_xor(M, off, WAVE));
    const float wt = (mc == -INFINITY) ? 0.f : __expf(mc - M);
    float L = lc * wt;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) L += __shfl_xor(L, off, WAVE);
    cw[hh * 64 + lane] = wt;
    if (lane == 0) cL[hh] = L;
  }
  __syncthreads();
  for (int idx = t; idx < G * (HD / 4); idx += 256) {
    const int hh = idx / (HD / 4), d = 4 * (idx % (HD / 4));
    const float* col = hbase + (size_t)hh * nchunk * (HD + 4) + d;
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
    for (int c = 0; c < nchunk; ++c) {
      const f32x4 v =
          *reinterpret_cast<const f32x4*>(col + (size_t)c * (HD + 4));
      const float wt = cw[hh * 64 + c];
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] += v[j] * wt;
    }
    const float L = cL[hh];
    union { u16 h[4]; unsigned long long u; } pk;
#pragma unroll
    for (int j = 0; j < 4; ++j) pk.h[j] = f2b(o[j] / L);
    *reinterpret_cast<unsigned long long*>(
        outbuf + (size_t)(kvh * G + hh) * HD + d) = pk.u;
  }
#undef WS_STORE
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
