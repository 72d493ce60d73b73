// On-device top-k / top-p / repeat-penalty sampling (the rest of
// create_logits_processor, text_model.rs:102-118, and the repeat penalty the
// reference applies before every sample, text_model.rs:433-452).
//
// Contract:
//   1. penalty   l'_i = l_i * (1/pen) if l_i >= 0 else l_i * pen for every id
//                among the last `last_n` sampled tokens (each id once)
//   2. top-k     keep { l' >= the k-th largest l' }      (ties all kept)
//   3. top-p     among those, m_i = exp((l'_i - max) / T); keep the minimal
//                descending prefix reaching top_p of their mass (ties kept)
//   4. draw      first-index argmax over the kept set of l'/T + Gumbel noise
//                (the splitmix64 stream of k_argmax_part, indexed by a
//                persistent draw counter); T <= 0: argmax of l'
// The kept set is always { l' >= tau }, so 2 and 3 are one exact radix
// select each over order-preserving u32 keys, refined 11 + 11 + 10 bits from
// the top: top-k selects on per-bin counts, top-p on per-bin masses.
//
// Reproducibility: every cross-thread sum is an integer.  Masses are
// round(m * 2^40) in u64 (<= 2^18 entries fit; quantisation <= 2^-23 of the
// peak mass in total), so atomic adds commute and the token, kept count and
// tau are bitwise identical from run to run.
//
// No block waits for another: each refinement is its own launch, and every
// block of a launch re-derives the state the previous histogram implies
// (one 2048-bin scan) instead of electing a block to do it.  Launches per
// step: prep + 3 per active select + part + fin (3, 6 or 9), fixed for a
// mode, no host synchronisation — graph-capturable.
#include "kernels.h"
#include "kernels_common.h"

#include <algorithm>

namespace {

using u64 = unsigned long long;
constexpr int NBINS = 2048;    // bins of one histogram (11 bits; last pass 10)
constexpr int NHIST = 6;       // 3 refinements x 2 selects
constexpr int MAXNB = 128;     // blocks over the vocabulary
constexpr int MAXSPAN = 2048;  // vocabulary entries per block

// selection state entering a histogram pass
struct Sel {
  u64 ma;      // mass strictly above the current prefix range
  u64 target;  // k (count select) or top_p * total mass (mass select)
  u32 prefix;  // key bits decided so far (right-aligned)
  u32 ca;      // entries strictly above the current prefix range
  u32 cj;      // entries in the chosen bin (last refinement: the tie group)
  u32 kmin;    // mass select after top-k: only keys >= the k-th key
};

// order-preserving float -> u32 (sign flip): a < b <=> key(a) < key(b),
// -inf lowest.  -0.0 is canonicalised to +0.0 before it gets here.
__device__ inline u32 f2key(float f) {
  const u32 u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ inline float key2f(u32 k) {
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

// max of the nb (<= 128) per-block maxima; whole block (256 threads)
__device__ inline float global_max(const float* __restrict__ pmax, int nb) {
  __shared__ float wm[2];
  const int t = threadIdx.x;
  if (t < 2 * WAVE) {
    float v = t < nb ? pmax[t] : -INFINITY;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
      v = fmaxf(v, __shfl_xor(v, off, WAVE));
    if ((t & (WAVE - 1)) == 0) wm[t / WAVE] = v;
  }
  __syncthreads();
  return fmaxf(wm[0], wm[1]);
}

// Penalised copy of the logits into the work buffer, per-block max / min,
// histogram clear.  A block marks the history ids that fall into its own
// span in LDS (an idempotent store, so a duplicated id is penalised once)
// and penalises from the RAW logits — no read-modify-write anywhere.
__global__ void k_sample_prep(const float* __restrict__ logits, int V, int nb,
                              SampleWs b, float pen, float inv_pen,
                              int last_n, int top_k) {
  __shared__ unsigned char flag[MAXSPAN];
  __shared__ float smax[256], smin[256];
  const int span = (V + nb - 1) / nb;
  const int start = blockIdx.x * span, end = min(start + span, V);
  const int tid = threadIdx.x;
  for (int i = blockIdx.x * 256 + tid; i < NHIST * NBINS; i += nb * 256) {
    b.hmass[i] = 0;
    b.hcnt[i] = 0;
  }
  if (blockIdx.x == 0 && tid == 0) {
    Sel s0{0, (u64)(top_k > 0 ? top_k : 0), 0, 0, 0, 0};
    ((Sel*)b.sel)[0] = s0;
  }
  const u32 hcount = b.state[0];
  const int n = last_n > 0 ? (int)min((u32)last_n, hcount) : 0;
  if (n > 0) {  // block-uniform
    for (int i = tid; i < end - start; i += 256) flag[i] = 0;
    __syncthreads();
    for (int j = tid; j < n; j += 256) {
      const u32 id = b.hist[(hcount - 1u - (u32)j) & (SAMPLE_HIST_CAP - 1)];
      if (id >= (u32)start && id < (u32)end) flag[id - start] = 1;
    }
    __syncthreads();
  }
  float mx = -INFINITY, mn = INFINITY;
  for (int i = start + tid; i < end; i += 256) {
    float v = logits[i];
    if (n > 0 && flag[i - start]) v = v >= 0.f ? v * inv_pen : v * pen;
    if (v == 0.f) v = 0.f;  // -0.0 -> +0.0: one key per value
    b.work[i] = v;
    mx = fmaxf(mx, v);
    mn = fminf(mn, v);
  }
  smax[tid] = mx;
  smin[tid] = mn;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) {
      smax[tid] = fmaxf(smax[tid], smax[tid + off]);
      smin[tid] = fminf(smin[tid], smin[tid + off]);
    }
    __syncthreads();
  }
  if (tid == 0) {
    b.pmax[blockIdx.x] = smax[0];
    b.pmin[blockIdx.x] = smin[0];
  }
}

// What histogram (hc, hm) of refinement `lvl` implies for state `in`: walk
// the bins from the top; the bin holding the k-th entry (mode 0) or the
// entry at which the cumulative mass reaches the target (mode 1) extends the
// prefix.  Whole block, same result in every thread.
__device__ Sel resolve(const u32* __restrict__ hc, const u64* __restrict__ hm,
                       Sel in, int lvl, int mode, float top_p) {
  __shared__ u32 sc[256];
  __shared__ u64 sm[256];
  __shared__ Sel out;
  const int r = lvl == 2 ? 10 : 11;
  const int nbins = 1 << r, per = nbins / 256;
  const int t = threadIdx.x;
  u32 c = 0, bc[8];
  u64 m = 0, bm[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {  // this thread's bins, highest first
    const int bin = nbins - 1 - (t * per + e);
    bc[e] = e < per ? hc[bin] : 0;
    bm[e] = (e < per && mode == 1) ? hm[bin] : 0;
    c += bc[e];
    m += bm[e];
  }
  sc[t] = c;
  sm[t] = m;
  if (t == 0) {  // unreachable fallback: keep everything under the prefix
    Sel f = in;
    f.prefix = in.prefix << r;
    f.cj = 0;
    out = f;
  }
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {
    const u32 cv = t >= off ? sc[t - off] : 0;
    const u64 mv = t >= off ? sm[t - off] : 0;
    __syncthreads();
    sc[t] += cv;
    sm[t] += mv;
    __syncthreads();
  }
  u64 target = in.target;
  if (mode == 1 && lvl == 0) {
    const u64 total = sm[255];
    target = (u64)((double)total * (double)top_p);
    if (target > total) target = total;
    if (target < 1) target = 1;
  }
  u32 rc = in.ca + (sc[t] - c);
  u64 rm = in.ma + (sm[t] - m);
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int bin = nbins - 1 - (t * per + e);
    const u32 cc = bc[e];
    const u64 mm = bm[e];
    const bool hit = mode == 0 ? ((u64)rc < target && target <= (u64)rc + cc)
                               : (rm < target && target <= rm + mm);
    if (hit) {
      Sel o{rm, target, (in.prefix << r) | (u32)bin, rc, cc, in.kmin};
      out = o;
    }
    rc += cc;
    rm += mm;
  }
  __syncthreads();
  const Sel res = out;
  __syncthreads();  // `out` is reused by the next call
  return res;
}

// One refinement: histogram (count, fixed-point mass) of the next key bits
// over the entries that match the prefix decided so far.
__global__ void k_sample_hist(int V, int nb, SampleWs b, int p, int lvl,
                              int mode, int mode_prev, int lvl_prev,
                              float inv_temp, float top_p) {
  __shared__ u32 lc[NBINS];
  __shared__ u64 lm[NBINS];
  const int tid = threadIdx.x;
  for (int i = tid; i < NBINS; i += 256) {
    lc[i] = 0;
    lm[i] = 0;
  }
  Sel* sel = (Sel*)b.sel;
  Sel s;
  if (mode_prev < 0) {
    s = sel[0];
  } else {
    s = resolve(b.hcnt + (size_t)(p - 1) * NBINS,
                b.hmass + (size_t)(p - 1) * NBINS, sel[p - 1], lvl_prev,
                mode_prev, top_p);
    if (lvl == 0) {  // the previous select is complete: start the next one
      Sel n{0, 0, 0, 0, 0, s.prefix};
      s = n;
    }
    if (blockIdx.x == 0 && tid == 0) sel[p] = s;
  }
  __syncthreads();
  const int hb = lvl * 11, r = lvl == 2 ? 10 : 11, sh = 32 - hb - r;
  const u32 bmask = (1u << r) - 1u;
  const float gmax = mode == 1 ? global_max(b.pmax, nb) : 0.f;
  const int span = (V + nb - 1) / nb;
  const int start = blockIdx.x * span, end = min(start + span, V);
  for (int i = start + tid; i < end; i += 256) {
    const float v = b.work[i];
    const u32 key = f2key(v);
    if (key < s.kmin) continue;
    if (hb != 0 && (key >> (32 - hb)) != s.prefix) continue;
    const u32 bin = (key >> sh) & bmask;
    atomicAdd(&lc[bin], 1u);
    if (mode == 1) {
      const float d = v == gmax ? 0.f : v - gmax;
      const float m = __expf(d * inv_temp);
      atomicAdd(&lm[bin], (u64)__float2ull_rn(m * 0x1p40f));
    }
  }
  __syncthreads();
  for (int i = tid; i < NBINS; i += 256) {
    if (lc[i]) {
      atomicAdd(&b.hcnt[(size_t)p * NBINS + i], lc[i]);
      if (mode == 1) atomicAdd(&b.hmass[(size_t)p * NBINS + i], lm[i]);
    }
  }
}

// Gumbel-argmax (or plain argmax) over the kept set; same noise and
// first-index tie rule as k_argmax_part, the step index replaced by the
// persistent draw counter.
__global__ void k_sample_part(int V, int nb, SampleWs b, int p_last,
                              int mode_prev, float inv_temp, float top_p,
                              uint64_t seed) {
  const int tid = threadIdx.x;
  u32 tkey = 0;
  if (p_last >= 0) {
    const Sel s = resolve(b.hcnt + (size_t)p_last * NBINS,
                          b.hmass + (size_t)p_last * NBINS,
                          ((Sel*)b.sel)[p_last], 2, mode_prev, top_p);
    tkey = s.prefix;
    if (blockIdx.x == 0 && tid == 0) {
      b.state[2] = s.ca + s.cj;
      b.state[3] = __float_as_uint(key2f(tkey));
    }
  }
  const int span = (V + nb - 1) / nb;
  const int start = blockIdx.x * span, end = min(start + span, V);
  const uint64_t base =
      seed + 0x9e3779b97f4a7c15ull * (uint64_t)(b.state[1] + 1u);
  float best = -INFINITY;
  int bidx = 0x7fffffff;
  for (int i = start + tid; i < end; i += 256) {
    float v = b.work[i];
    if (f2key(v) < tkey) continue;
    if (inv_temp > 0.f) v = v * inv_temp + gumbel_noise(base, i);
    if (v > best || (v == best && i < bidx)) { best = v; bidx = i; }
  }
  __shared__ float sv[256];
  __shared__ int si[256];
  sv[tid] = best;
  si[tid] = bidx;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) {
      float ov = sv[tid + off];
      int oi = si[tid + off];
      if (ov > sv[tid] || (ov == sv[tid] && oi < si[tid])) {
        sv[tid] = ov;
        si[tid] = oi;
      }
    }
    __syncthreads();
  }
  if (tid == 0) { b.pval[blockIdx.x] = sv[0]; b.pidx[blockIdx.x] = si[0]; }
}

// Final reduce + the end-of-step bookkeeping of k_argmax_fin, plus the
// sampler's own state: history ring push and draw counter.
__global__ void k_sample_fin(int V, int nb, SampleWs b, int sel_on,
                             u32* __restrict__ tok, int* __restrict__ pos,
                             u32* __restrict__ ring, int* __restrict__ step,
                             int advance_pos, int advance_hist) {
  __shared__ float sv[MAXNB], smin[MAXNB];
  __shared__ int si[MAXNB];
  const int tid = threadIdx.x;
  sv[tid] = tid < nb ? b.pval[tid] : -INFINITY;
  si[tid] = tid < nb ? b.pidx[tid] : 0x7fffffff;
  smin[tid] = tid < nb ? b.pmin[tid] : INFINITY;
  __syncthreads();
  for (int off = MAXNB / 2; off > 0; off >>= 1) {
    if (tid < off) {
      float ov = sv[tid + off];
      int oi = si[tid + off];
      if (ov > sv[tid] || (ov == sv[tid] && oi < si[tid])) {
        sv[tid] = ov;
        si[tid] = oi;
      }
      smin[tid] = fminf(smin[tid], smin[tid + off]);
    }
    __syncthreads();
  }
  if (tid == 0) {
    // as k_argmax_fin: nothing above -inf (all -inf and/or NaN) is token 0
    const u32 t = sv[0] > -INFINITY ? (u32)si[0] : 0u;
    *tok = t;
    if (ring) {
      ring[*step] = t;
      *step += 1;
    }
    if (advance_pos) *pos += 1;
    if (!sel_on) {  // nothing dropped: tau is the smallest l'
      b.state[2] = (u32)V;
      b.state[3] = __float_as_uint(smin[0]);
    }
    if (advance_hist) {
      b.hist[b.state[0] & (SAMPLE_HIST_CAP - 1)] = t;
      b.state[0] += 1u;
    }
    b.state[1] += 1u;
  }
}

inline size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }

}  // namespace

size_t sample_ws_bytes(int V) {
  return up256((size_t)NHIST * NBINS * 8) + up256((size_t)NHIST * NBINS * 4) +
         up256(sizeof(Sel) * (NHIST + 1)) + up256((size_t)V * 4) +
         5 * up256(MAXNB * 4) + up256(SAMPLE_HIST_CAP * 4) + up256(4 * 4);
}

SampleWs sample_ws_bind(void* base, int V) {
  char* p = (char*)base;
  auto take = [&p](size_t bytes) {
    void* r = p;
    p += up256(bytes);
    return r;
  };
  SampleWs b;
  b.hmass = (unsigned long long*)take((size_t)NHIST * NBINS * 8);
  b.hcnt = (u32*)take((size_t)NHIST * NBINS * 4);
  b.sel = take(sizeof(Sel) * (NHIST + 1));
  b.work = (float*)take((size_t)V * 4);
  b.pmax = (float*)take(MAXNB * 4);
  b.pmin = (float*)take(MAXNB * 4);
  b.pval = (float*)take(MAXNB * 4);
  b.pidx = (int*)take(MAXNB * 4);
  take(MAXNB * 4);
  b.hist = (u32*)take(SAMPLE_HIST_CAP * 4);
  b.state = (u32*)take(4 * 4);
  return b;
}

void launch_sample(const float* logits, int V, const SampleWs& b, u32* tok,
                   int* pos, u32* ring, int* step, int advance_pos,
                   float inv_temp, int top_k, float top_p, float penalty,
                   int last_n, int advance_hist, uint64_t seed,
                   hipStream_t s) {
  const int nb = std::min(MAXNB, std::max(1, (V + 1023) / 1024));
  const bool sampling = inv_temp > 0.f;
  const bool k_on = sampling && top_k > 0 && top_k < V;
  const bool p_on = sampling && top_p > 0.f && top_p < 1.f;
  const bool pen_on = penalty != 1.f && last_n > 0;
  hipLaunchKernelGGL(k_sample_prep, dim3(nb), dim3(256), 0, s, logits, V, nb,
                     b, penalty, 1.0f / penalty, pen_on ? last_n : 0,
                     k_on ? top_k : 0);
  int p = 0, mode_prev = -1, lvl_prev = 0;
  for (int mode = 0; mode < 2; ++mode) {
    if (!(mode == 0 ? k_on : p_on)) continue;
    for (int lvl = 0; lvl < 3; ++lvl) {
      hipLaunchKernelGGL(k_sample_hist, dim3(nb), dim3(256), 0, s, V, nb, b,
                         p, lvl, mode, mode_prev, lvl_prev, inv_temp, top_p);
      mode_prev = mode;
      lvl_prev = lvl;
      ++p;
    }
  }
  hipLaunchKernelGGL(k_sample_part, dim3(nb), dim3(256), 0, s, V, nb, b,
                     p - 1, mode_prev, inv_temp, top_p, seed);
  hipLaunchKernelGGL(k_sample_fin, dim3(1), dim3(MAXNB), 0, s, V, nb, b,
                     p > 0 ? 1 : 0, tok, pos, ring, step, advance_pos,
                     advance_hist);
}
