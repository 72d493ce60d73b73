// Shared device helpers for the gfx950 kernels (split into per-family
// translation units so template-instantiation churn in one family cannot
// perturb another's codegen — guide §5.4 rule 19).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#include <cstdint>
#include <cstdlib>

#define WAVE 64

using u16 = unsigned short;
using u32 = unsigned int;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using f32x16 = __attribute__((ext_vector_type(16))) float;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using short8 = __attribute__((ext_vector_type(8))) short;
using uint4v = __attribute__((ext_vector_type(4))) unsigned int;
using f32x2 = __attribute__((ext_vector_type(2))) float;
using bf16x2 = __attribute__((ext_vector_type(2))) __bf16;

// bf16 <-> f32 (round-to-nearest-even, matches torch/HF casting)
__device__ __host__ inline u16 f2b(float f) {
  union { float f; u32 u; } v{f};
  if ((v.u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0;  // NaN
  u32 r = v.u + 0x7fffu + ((v.u >> 16) & 1u);
  return (u16)(r >> 16);
}
__device__ __host__ inline float b2f(u16 h) {
  union { u32 u; float f; } v{(u32)h << 16};
  return v.f;
}

// nontemporal 16-B weight load: decode weights are streamed exactly once
// per token — keep them from thrashing L2/L3 (guide G14)
__device__ inline short8 ntload8(const u16* p) {
  uint4v v = __builtin_nontemporal_load(reinterpret_cast<const uint4v*>(p));
  union { uint4v u; short8 s; } c{v};
  return c.s;
}
__device__ inline uint4v ntload16b(const unsigned char* p) {
  return __builtin_nontemporal_load(reinterpret_cast<const uint4v*>(p));
}
// 16 fp8 -> 16 f32 via the hardware v_cvt_pk_f32_fp8 (2 elems/instruction)
__device__ inline void f8x16_decode(uint4v w, float* out) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8(w[q], false);
    f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8(w[q], true);
    out[q * 4 + 0] = lo[0];
    out[q * 4 + 1] = lo[1];
    out[q * 4 + 2] = hi[0];
    out[q * 4 + 3] = hi[1];
  }
}

// Gumbel noise of both samplers (k_argmax_part, k_sample_part) at vocabulary
// index i; base = seed + GOLD * (draw + 1).  k = top 24 bits of the
// splitmix64 hash, u = (min(k, 2^24 - 2) + 1) * 2^-24: u lies in
// [2^-24, 1 - 2^-24], every value exact in f32, so -log(u) > 0 and the noise
// is finite.  (Without the clamp k = 2^24 - 1 gives u == 1 and +inf noise:
// that token would win whatever its logit.)
__device__ inline float gumbel_noise(uint64_t base, int i) {
  uint64_t z = base + 0xbf58476d1ce4e5b9ull * (uint64_t)(i + 1);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  z ^= z >> 31;
  const u32 k = min((u32)(z >> 40), 0xfffffeu);
  const float u = (float)(k + 1u) * 0x1p-24f;
  return -__logf(-__logf(u));
}

// lane<->lane+32 half exchange via v_permlane32_swap + cndmask (2-3 VALU)
// instead of __shfl_xor(.,32) (ds_bpermute + lgkm wait on the LDS pipe)
__device__ inline u32 halfswap32(u32 x, int lhalf) {
  auto r = __builtin_amdgcn_permlane32_swap(x, x, false, false);
  return lhalf == 0 ? (u32)r[1] : (u32)r[0];
}
__device__ inline float halfswap32f(float x, int lhalf) {
  union { float f; u32 u; } a{x};
  a.u = halfswap32(a.u, lhalf);
  return a.f;
}
// two f32 -> packed bf16 pair, round to nearest even (v_cvt_pk_bf16_f32)
__device__ inline u32 pack_bf16(float lo, float hi) {
  f32x2 v = {lo, hi};
  union { bf16x2 b; u32 u; } c{__builtin_convertvector(v, bf16x2)};
  return c.u;
}

// Split-KV chunk partition of decode attention at n = *pos + 1 live positions.
// Sliding window (cache.rs:173-205 semantics): attention spans only the last
// `window` positions; the nchunk chunks partition [lo, n), chunk `chunk` is
// [start, end) (empty when start >= end); cs is the unclipped chunk length,
// which is chunk 0's.  Every kernel that is handed the same ws / cnt must cut
// the span the same way: this is the one definition.  Forced inline because
// kernels_kv8.hip compiles its functions for another target-feature set
// (no-packed-fp32-ops), into which a plain inline function of this header
// stays a call.
struct DecodeSpan { int start, end, cs; };
__host__ __device__ __forceinline__ DecodeSpan decode_span(int n, int window,
                                                           int nchunk,
                                                           int chunk) {
  const int lo = (window > 0 && n > window) ? n - window : 0;
  const int cs = (n - lo + nchunk - 1) / nchunk;
  const int start = lo + chunk * cs;
  return {start, min(start + cs, n), cs};
}

__device__ inline float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, WAVE);
  return v;
}
__device__ inline float wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    v = fmaxf(v, __shfl_down(v, off, WAVE));
  return v;
}
