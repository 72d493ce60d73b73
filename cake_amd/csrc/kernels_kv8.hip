// fp8 (OCP e4m3) KV cache, hd 128: the quantizing store, the dequantizing
// scratch fill, and the decode attention that reads the codes directly.
//
// Format (per layer): k8, v8 = u8 [nkv][max_seq][128] codes; ks, vs = f32
// [nkv][max_seq], one power-of-two scale 2^k per row, k the smallest integer
// with amax(row) * 2^-k <= 448 (all-zero row: k = 0; k is clamped to
// [-120, 120] so that 2^k, 2^-k and every code * 2^k stay normal or bf16-
// representable).  code = round-to-nearest-even e4m3 of x * 2^-k (an exact
// product).  Dequantization code * 2^k is exact in bf16 (4 significant bits)
// and in f32, so the bf16 scratch that prefill attends to and the f32 values
// decode attends to are the same numbers.
#include "kernels_common.h"
#include "kernels.h"

namespace {

// every f32 multiply and add of this file stays scalar
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(                                       \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

using u8 = unsigned char;

__device__ inline float bits_f(u32 u) {
  union { u32 u; float f; } v{u};
  return v.f;
}
__device__ inline u32 f_bits(float f) {
  union { float f; u32 u; } v{f};
  return v.u;
}
__device__ inline float bf(u16 h) { return bits_f((u32)h << 16); }
__device__ inline u16 tobf(float f) {  // round to nearest even; no NaN here
  const u32 u = f_bits(f);
  return (u16)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
__device__ inline float pow2f(int k) { return bits_f((u32)(k + 127) << 23); }
// lane exchange and block barrier on the builtins: the header's wrappers are
// compiled for another target and would not inline into this file's functions
__device__ inline u32 xor_lane(u32 v, int off) {
  const int lane = (int)__builtin_amdgcn_mbcnt_hi(
      ~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
  return (u32)__builtin_amdgcn_ds_bpermute((lane ^ off) << 2, (int)v);
}
__device__ inline float xor_lanef(float v, int off) {
  return bits_f(xor_lane(f_bits(v), off));
}
__device__ inline void block_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
__device__ inline float wsum(float v) {  // every lane gets the sum
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += xor_lanef(v, off);
  return v;
}
__device__ inline float wmax(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, xor_lanef(v, off));
  return v;
}

// k of a row from its amax as bf16 magnitude bits: amax = m * 2^e with m in
// [0.5, 1) (frexp), 448 = 0.875 * 2^9, so k = e - 9, plus one when m > 0.875
// (mantissa field > 96)
__device__ inline int kv8_row_k(u32 amax_bits) {
  if (amax_bits == 0) return 0;
  const int E = (int)(amax_bits >> 7), M = (int)(amax_bits & 127);
  const int k = E - 126 - 9 + (M > 96 ? 1 : 0);
  return max(-120, min(120, k));
}
// round-to-nearest-even e4m3 code of y, |y| <= 448.  Done in integer and
// one f32 add, so ties and subnormal codes are exact by construction: a
// normal result rounds the f32 mantissa to 3 bits; below 2^-6 the add of
// 2^14 (ulp 2^-9, the subnormal quantum) rounds to nearest even and leaves
// the code in the low mantissa bits (8 = the smallest normal, as it must).
__device__ inline u32 kv8_code(float y) {
  const u32 b = f_bits(y), a = b & 0x7fffffffu, sgn = (b >> 24) & 0x80u;
  u32 c;
  if (a >= 0x3c800000u) {  // |y| >= 2^-6
    const u32 r = (a + 0x7ffffu + ((a >> 20) & 1u)) >> 20;
    c = r - ((127u - 7u) << 3);
  } else {
    c = f_bits(bits_f(a) + 16384.f) & 0xffu;
  }
  return c | sgn;
}
// two codes (the low 16 bits of w) -> f32
__device__ inline f32x2 cvt2(u32 w, bool hi) {
  return hi ? __builtin_amdgcn_cvt_pk_f32_fp8(w, true)
            : __builtin_amdgcn_cvt_pk_f32_fp8(w, false);
}

// ---------------------------------------------------------------------------
// Quantizing store.  grid (ceil(S/4), nkv, 2 = K|V), block 256: one wave per
// row, lane = dims (2*lane, 2*lane+1).  Reads the bf16 row the rope-store /
// fused qkv-rope kernel left in the scratch, writes codes + scale, and writes
// the dequantized bf16 back over the scratch row (K, V and V^T).  p0 comes
// from *pos when pos != nullptr (decode, graph-capturable).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_kv8_quant_rows(
    u16* __restrict__ kc, u16* __restrict__ vc, u16* __restrict__ vtc,
    u8* __restrict__ k8, u8* __restrict__ v8, float* __restrict__ ks,
    float* __restrict__ vs, const int* __restrict__ pos, int p0, int S,
    int max_seq) {
  const int wid = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
  const int row = blockIdx.x * 4 + wid;
  if (pos) p0 = *pos;
  const int p = p0 + row;
  if (row >= S || p >= max_seq) return;
  const int kvh = blockIdx.y;
  const bool isv = blockIdx.z != 0;
  const size_t ro = (size_t)kvh * max_seq + p;
  u16* src = (isv ? vc : kc) + ro * 128;
  const u32 x2 = *reinterpret_cast<const u32*>(src + 2 * lane);
  const u32 a0 = x2 & 0x7fffu, a1 = (x2 >> 16) & 0x7fffu;
  u32 am = max(a0, a1);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    am = max(am, xor_lane(am, off));
  const int k = kv8_row_k(am);
  const float inv = pow2f(-k), sc = pow2f(k);
  const u32 c0 = kv8_code(bf((u16)(x2 & 0xffffu)) * inv);
  const u32 c1 = kv8_code(bf((u16)(x2 >> 16)) * inv);
  const u32 cc = c0 | (c1 << 8);
  *reinterpret_cast<u16*>((isv ? v8 : k8) + ro * 128 + 2 * lane) = (u16)cc;
  if (lane == 0) (isv ? vs : ks)[ro] = sc;
  const f32x2 dq = cvt2(cc, false);
  // code * 2^k has 4 significant bits: the truncation to bf16 is exact
  const u32 d0 = f_bits(dq[0] * sc) >> 16, d1 = f_bits(dq[1] * sc) >> 16;
  *reinterpret_cast<u32*>(src + 2 * lane) = d0 | (d1 << 16);
  if (isv) {
    u16* t = vtc + ((size_t)kvh * 128 + 2 * lane) * max_seq + p;
    t[0] = (u16)d0;
    t[max_seq] = (u16)d1;
  }
}

// ---------------------------------------------------------------------------
// Scratch fill from the codes: rows [lo, p0) of K, V and V^T.  grid
// (ceil((p0-lo)/64), nkv), block 256, one 64-row tile per block.  K and V:
// a 16-B code load per thread -> 32 B of bf16.  V^T: the tile goes through an
// LDS image [128 dims][64 rows] (row pitch 66), so the code read stays a
// 16-B row-major load and the V^T write is 64 consecutive positions of one
// dim per wave store.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_kv8_dequant_rows(
    u16* __restrict__ kc, u16* __restrict__ vc, u16* __restrict__ vtc,
    const u8* __restrict__ k8, const u8* __restrict__ v8,
    const float* __restrict__ ks, const float* __restrict__ vs, int lo,
    int p0, int max_seq) {
  __shared__ u16 vt[128 * 66];
  const int t = threadIdx.x, kvh = blockIdx.y;
  const int r0 = lo + blockIdx.x * 64;
  const size_t hb = (size_t)kvh * max_seq;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int idx = j * 256 + t;  // 16-B unit of the K (j < 2) or V tile
    const int r = (idx >> 3) & 63, u = idx & 7;
    const bool isv = j >= 2;
    const int p = r0 + r;
    if (p >= p0) continue;
    const size_t ro = hb + p;
    const uint4v w = *reinterpret_cast<const uint4v*>(
        (isv ? v8 : k8) + ro * 128 + u * 16);
    const float sc = (isv ? vs : ks)[ro];
    u32 o[8];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const f32x2 a = cvt2(w[q], false), b = cvt2(w[q], true);
      o[2 * q] = (f_bits(a[0] * sc) >> 16) | (f_bits(a[1] * sc) & 0xffff0000u);
      o[2 * q + 1] =
          (f_bits(b[0] * sc) >> 16) | (f_bits(b[1] * sc) & 0xffff0000u);
    }
    u16* dst = (isv ? vc : kc) + ro * 128 + u * 16;
    *reinterpret_cast<uint4v*>(dst) = uint4v{o[0], o[1], o[2], o[3]};
    *reinterpret_cast<uint4v*>(dst + 8) = uint4v{o[4], o[5], o[6], o[7]};
    if (isv) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        vt[(u * 16 + 2 * e) * 66 + r] = (u16)(o[e] & 0xffffu);
        vt[(u * 16 + 2 * e + 1) * 66 + r] = (u16)(o[e] >> 16);
      }
    }
  }
  block_sync();
  const int lane = t % WAVE, wid = t / WAVE;
  if (r0 + lane < p0) {
    u16* dst = vtc + (size_t)kvh * 128 * max_seq + r0 + lane;
    for (int d = wid; d < 128; d += 4)
      dst[(size_t)d * max_seq] = vt[d * 66 + lane];
  }
}

// ---------------------------------------------------------------------------
// Decode attention over the codes (hd 128).
//
//   grid (nchunk, nkv * subg), block 256 = 4 waves, GB q-heads of one kv head
//   per block, R = 4 / GB waves per head.
//   tile: 128 positions = a 16 KiB K image and a 16 KiB V image (a row is
//   128 B), register-staged into a double-buffered LDS image; the tile's ks /
//   vs slices ride in the K group (thread t < 128: ks, else vs).  K image
//   swizzled by 16-B unit, slot = unit ^ (row & 7), applied on the source
//   address; V linear.  Overshoot rows collapse onto end-1.  One raw barrier
//   per 128 positions.
//   work split: wave (head hs, residue r) owns 128 / R positions of every
//   tile through ALL phases and carries its own online-softmax state
//   (m, l, o), so no phase needs another wave's result; the R states of a
//   head merge once, after the tile loop.
//   phase A: lane = position; a 16-B K read gives 16 codes, converted by
//            v_cvt_pk_f32_fp8 against q broadcast from LDS (f32).  GB 4: the
//            wave's two 64-position passes share each q read.  GB 1: the wave
//            owns 32 positions, the lane halves take 64 dims each and add.
//            The score gets its K scale once: d * ks[p] * rsqrt(128).
//   phase B: wave-wide online softmax; the PV weight is stored as
//            ew * vs[p] in the wave's own LDS row, even positions first.
//   phase C: lane = (position parity, dim quad): one b32 read = 4 V codes,
//            weights read as broadcast b128.  No scale multiply in the loop.
//   combine: {o, m, l} partials and the arrival counter follow the ws / cnt
//            contract of launch_attn_decode; nchunk == 1 writes directly.
//            The last arriver combines: wave = head (x dim slice), lane =
//            chunk for m / l, then plain loads of the partial rows behind
//            one agent acquire.
// ---------------------------------------------------------------------------
template <int GB>
__global__ __launch_bounds__(256, 2) void k_attn_decode_kv8(
    const u16* __restrict__ q, const u8* __restrict__ k8,
    const u8* __restrict__ v8, const float* __restrict__ ks,
    const float* __restrict__ vs, const int* __restrict__ pos,
    float* __restrict__ ws, u32* __restrict__ cnt, u16* __restrict__ outbuf,
    int nh, int nkv, int max_seq, int nchunk, int window, int subg) {
  constexpr int TILE = 128, hd = 128;
  constexpr int R = 4 / GB;
  constexpr int PPW = TILE / R;       // positions of a tile per wave
  constexpr int NP = GB == 4 ? 2 : 1; // 64-position passes of phase A
  constexpr bool SPLITD = GB == 1;    // lane halves split the dims
  constexpr int NU = SPLITD ? 4 : 8;  // 16-B K units per lane and row
  extern __shared__ __attribute__((aligned(16))) char smem[];
  u8* kb = reinterpret_cast<u8*>(smem);                        // [2][128][128]
  u8* vb = kb + 2 * TILE * 128;                                // [2][128][128]
  float* scl = reinterpret_cast<float*>(smem + 4 * TILE * 128);  // [2][ks|vs]
  float* qlds = scl + 2 * 256;                                 // [GB][128]
  float* wl = qlds + GB * 128;                                 // [4][128]
  float* so = wl + 4 * 128;                                    // [4][132]

  const int yb = blockIdx.y;
  const int kvh = yb / subg, sub = yb % subg;
  const int h0 = kvh * (nh / nkv) + sub * GB;
  const int chunk = blockIdx.x;
  const int n = *pos + 1;
  const DecodeSpan sp = decode_span(n, window, nchunk, chunk);
  const int start = sp.start, end = sp.end;
  const int t = threadIdx.x, wid = t / WAVE, lane = t % WAVE;
  const size_t hb = (size_t)kvh * max_seq;
  const u8* kbase = k8 + hb * 128;
  const u8* vbase = v8 + hb * 128;
  const float* sbase = (t < 128 ? ks : vs) + hb;
#define WS_STORE(p, v)                                                     \
  __hip_atomic_store((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

  uint4v rk[4], rv[4];
  float rs;
  // thread t, piece j: 16-B unit j*256 + t of the tile = row j*32 + t/8,
  // slot t & 7
  auto load_k = [&](int tb) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = j * 32 + (t >> 3);
      const int row = min(tb + r, end - 1);
      rk[j] = *reinterpret_cast<const uint4v*>(
          kbase + (size_t)row * 128 + (((t & 7) ^ (r & 7)) << 4));
    }
    rs = sbase[min(tb + (t & 127), end - 1)];
  };
  auto load_v = [&](int tb) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int row = min(tb + j * 32 + (t >> 3), end - 1);
      rv[j] = *reinterpret_cast<const uint4v*>(vbase + (size_t)row * 128 +
                                               ((t & 7) << 4));
    }
  };
  auto write_k = [&](int buf) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      *reinterpret_cast<uint4v*>(kb + buf * TILE * 128 + (j * 256 + t) * 16) =
          rk[j];
    scl[buf * 256 + t] = rs;
  };
  auto write_v = [&](int buf) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      *reinterpret_cast<uint4v*>(vb + buf * TILE * 128 + (j * 256 + t) * 16) =
          rv[j];
  };

  for (int i = t; i < GB * 128; i += 256)
    qlds[i] = bf(q[(size_t)(h0 + i / 128) * hd + (i & 127)]);
  block_sync();

  const int hs = wid / R, rres = wid % R;
  const int pbase = rres * PPW;            // the wave's positions of a tile
  const int pl = SPLITD ? (lane & 31) : lane;
  const int u0 = SPLITD ? (lane >> 5) * 4 : 0;
  const int hf = lane >> 5, dq = lane & 31;  // phase C: parity, dim quad
  const float scale = rsqrtf(128.f);
  const float* qh = qlds + hs * 128;
  float* wrow = wl + wid * 128;
  float m = -INFINITY, lsum = 0.f, o[4] = {0.f, 0.f, 0.f, 0.f};
  const int nt = start < end ? (end - start + TILE - 1) / TILE : 0;
  if (nt > 0) {
    load_k(start);
    load_v(start);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    write_k(0);
    write_v(0);
    load_k(start + TILE);
    load_v(start + TILE);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    for (int ti = 0; ti < nt; ++ti) {
      const int tb = start + ti * TILE;
      const int cur = ti & 1;
      const u8* kcur = kb + cur * TILE * 128;
      const u8* vcur = vb + cur * TILE * 128;
      const float* ksl = scl + cur * 256;
      const float* vsl = ksl + 128;
      // ---- A: scores of the wave's positions -----------------------------
      float d[NP];
#pragma unroll
      for (int ps = 0; ps < NP; ++ps) d[ps] = 0.f;
#pragma unroll 2
      for (int uu = 0; uu < NU; ++uu) {
        const int u = u0 + uu;
        f32x4 qv[4];
#pragma unroll
        for (int e = 0; e < 4; ++e)
          qv[e] = *reinterpret_cast<const f32x4*>(qh + u * 16 + e * 4);
#pragma unroll
        for (int ps = 0; ps < NP; ++ps) {
          const int prow = pbase + ps * 64 + pl;
          const uint4v w = *reinterpret_cast<const uint4v*>(
              kcur + prow * 128 + ((u ^ (prow & 7)) << 4));
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const f32x2 a = cvt2(w[e], false), b = cvt2(w[e], true);
            d[ps] = fmaf(a[0], qv[e][0], d[ps]);
            d[ps] = fmaf(a[1], qv[e][1], d[ps]);
            d[ps] = fmaf(b[0], qv[e][2], d[ps]);
            d[ps] = fmaf(b[1], qv[e][3], d[ps]);
          }
        }
      }
      if (SPLITD) d[0] += xor_lanef(d[0], 32);
      // K(ti+1) and its scales landed (V(ti+1)'s 4 loads may still fly)
      asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      write_k(cur ^ 1);
      load_k(tb + 2 * TILE);
      // ---- B: the wave's own online softmax ------------------------------
      float sv[NP], tm = -INFINITY;
#pragma unroll
      for (int ps = 0; ps < NP; ++ps) {
        const int pt = pbase + ps * 64 + pl;
        sv[ps] = (tb + pt < end) ? d[ps] * (ksl[pt] * scale) : -INFINITY;
        tm = fmaxf(tm, sv[ps]);
      }
      tm = wmax(tm);
      const float mnew = fmaxf(m, tm);
      const float alpha = (mnew == -INFINITY) ? 0.f : __expf(m - mnew);
      float ts = 0.f;
#pragma unroll
      for (int ps = 0; ps < NP; ++ps) {
        const int j = ps * 64 + pl;  // position within the wave's PPW
        const float ew =
            (sv[ps] == -INFINITY) ? 0.f : __expf(sv[ps] - mnew);
        ts += ew;
        wrow[(j & 1) * (PPW / 2) + (j >> 1)] = ew * vsl[pbase + j];
      }
      ts = wsum(ts);
      if (SPLITD) ts *= 0.5f;  // both lane halves hold every position
      lsum = lsum * alpha + ts;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] *= alpha;
      m = mnew;
      // V(ti+1) landed (K(ti+2)'s 5 loads may still fly)
      asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
      write_v(cur ^ 1);
      load_v(tb + 2 * TILE);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // wrow written
      // ---- C: PV over the wave's positions -------------------------------
#pragma unroll 4
      for (int j2 = 0; j2 < PPW / 2; j2 += 4) {
        const f32x4 wv =
            *reinterpret_cast<const f32x4*>(wrow + hf * (PPW / 2) + j2);
        u32 vv[4];
#pragma unroll
        for (int e = 0; e < 4; ++e)
          vv[e] = *reinterpret_cast<const u32*>(
              vcur + (pbase + 2 * (j2 + e) + hf) * 128 + 4 * dq);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const f32x2 a = cvt2(vv[e], false), b = cvt2(vv[e], true);
          o[0] = fmaf(wv[e], a[0], o[0]);
          o[1] = fmaf(wv[e], a[1], o[1]);
          o[2] = fmaf(wv[e], b[0], o[2]);
          o[3] = fmaf(wv[e], b[1], o[3]);
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();  // [cur^1] images visible, [cur] consumed
    }
  }
  // the tail stages are never consumed: drain them once
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

  // ---- merge the parity halves, then the R wave states of each head -------
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] += xor_lanef(o[e], 32);
  if (hf == 0) {
#pragma unroll
    for (int e = 0; e < 4; ++e) so[wid * 132 + 4 * dq + e] = o[e];
    if (lane == 0) {
      so[wid * 132 + 128] = m;
      so[wid * 132 + 129] = lsum;
    }
  }
  block_sync();
  float M = -INFINITY, L = 0.f, f0 = 0.f, f1 = 0.f;  // rres == 0: the head's
  if (rres == 0) {
#pragma unroll
    for (int r = 0; r < R; ++r) M = fmaxf(M, so[(wid + r) * 132 + 128]);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const float* s = so + (wid + r) * 132;
      const float w = (s[128] == -INFINITY) ? 0.f : __expf(s[128] - M);
      L = fmaf(s[129], w, L);
      f0 = fmaf(s[2 * lane], w, f0);
      f1 = fmaf(s[2 * lane + 1], w, f1);
    }
  }
  if (nchunk == 1) {  // this block holds the heads' complete (o, m, l)
    if (rres == 0) {
      const float inv = 1.f / L;
      *reinterpret_cast<u32*>(outbuf + (size_t)(h0 + hs) * hd + 2 * lane) =
          (u32)tobf(f0 * inv) | ((u32)tobf(f1 * inv) << 16);
    }
    return;
  }
  if (rres == 0) {
    float* wsrow = ws + ((size_t)(h0 + hs) * nchunk + chunk) * (hd + 4);
    WS_STORE(&wsrow[2 * lane], f0);
    WS_STORE(&wsrow[2 * lane + 1], f1);
    if (lane == 0) {
      WS_STORE(&wsrow[hd], M);
      WS_STORE(&wsrow[hd + 1], L);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every wave drains
  block_sync();
  // epoch-free election: the counter accumulates across launches, the block
  // that draws nchunk-1 modulo nchunk is the last arriver of this launch
  if (t == 0) {
    const u32 v = __hip_atomic_fetch_add(&cnt[yb], 1u, __ATOMIC_RELAXED,
                                         __HIP_MEMORY_SCOPE_AGENT);
    so[0] = (v % (u32)nchunk == (u32)(nchunk - 1)) ? 1.f : 0.f;
  }
  block_sync();
  if (so[0] == 0.f) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  // ---- combine: wave = head hs, dims [rres, rres+1) * 128/R; lane = chunk
  // for the m / l pass (nchunk <= 64) ---------------------------------------
  const float* base = ws + (size_t)(h0 + hs) * nchunk * (hd + 4);
  const float mc = lane < nchunk ? base[lane * (hd + 4) + hd] : -INFINITY;
  const float lc = lane < nchunk ? base[lane * (hd + 4) + hd + 1] : 0.f;
  const float CM = wmax(mc);
  const float wc = (mc == -INFINITY) ? 0.f : __expf(mc - CM);
  const float CL = wsum(lc * wc);
  wrow[lane] = wc;  // zero beyond nchunk
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  constexpr int DPW = 128 / R;
  for (int dd = rres * DPW + lane; dd < (rres + 1) * DPW; dd += 64) {
    float acc = 0.f;
#pragma unroll 8
    for (int c = 0; c < nchunk; ++c)
      acc = fmaf(base[c * (hd + 4) + dd], wrow[c], acc);
    outbuf[(size_t)(h0 + hs) * hd + dd] = tobf(acc / CL);
  }
#undef WS_STORE
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

}  // namespace

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
void launch_kv8_quant(u16* kc, u16* vc, u16* vtc, unsigned char* k8,
                      unsigned char* v8, float* ks, float* vs, const int* pos,
                      int p0, int S, int nkv, int max_seq, hipStream_t s) {
  if (S < 1) return;
  hipLaunchKernelGGL(k_kv8_quant_rows, dim3((S + 3) / 4, nkv, 2), dim3(256), 0,
                     s, kc, vc, vtc, k8, v8, ks, vs, pos, p0, S, max_seq);
}
void launch_kv8_dequant(u16* kc, u16* vc, u16* vtc, const unsigned char* k8,
                        const unsigned char* v8, const float* ks,
                        const float* vs, int lo, int p0, int nkv, int max_seq,
                        hipStream_t s) {
  if (p0 <= lo) return;
  hipLaunchKernelGGL(k_kv8_dequant_rows, dim3((p0 - lo + 63) / 64, nkv),
                     dim3(256), 0, s, kc, vc, vtc, k8, v8, ks, vs, lo, p0,
                     max_seq);
}
int attn_decode_kv8_group(int nh, int nkv) {
  const int G = nh / nkv;
  return G % 4 == 0 ? 4 : G == 2 ? 2 : 1;
}
int attn_decode_kv8_grid_y(int nh, int nkv) {
  return nh / attn_decode_kv8_group(nh, nkv);
}
void launch_attn_decode_kv8(const u16* q, const unsigned char* k8,
                            const unsigned char* v8, const float* ks,
                            const float* vs, const int* pos, float* ws,
                            u32* cnt, u16* out, int nh, int nkv, int max_seq,
                            int nchunk, int window, hipStream_t s) {
  const int GB = attn_decode_kv8_group(nh, nkv);
  const int gy = nh / GB, subg = gy / nkv;
  // K dbuf + V dbuf + scales [2][256] + q [GB][128] + weights [4][128] +
  // merge scratch [4][132], all f32 past the images
  const size_t smem = 4 * 128 * 128 +
                      (size_t)(2 * 256 + GB * 128 + 4 * 128 + 4 * 132) * 4;
  static bool attr = false;
  if (!attr) {
    for (const void* f : {(const void*)&k_attn_decode_kv8<4>,
                          (const void*)&k_attn_decode_kv8<2>,
                          (const void*)&k_attn_decode_kv8<1>})
      hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize,
                          80 * 1024);
    attr = true;
  }
  const dim3 grid(nchunk, gy), block(256);
  if (GB == 4)
    hipLaunchKernelGGL(k_attn_decode_kv8<4>, grid, block, smem, s, q, k8, v8,
                       ks, vs, pos, ws, cnt, out, nh, nkv, max_seq, nchunk,
                       window, subg);
  else if (GB == 2)
    hipLaunchKernelGGL(k_attn_decode_kv8<2>, grid, block, smem, s, q, k8, v8,
                       ks, vs, pos, ws, cnt, out, nh, nkv, max_seq, nchunk,
                       window, subg);
  else
    hipLaunchKernelGGL(k_attn_decode_kv8<1>, grid, block, smem, s, q, k8, v8,
                       ks, vs, pos, ws, cnt, out, nh, nkv, max_seq, nchunk,
                       window, subg);
}
