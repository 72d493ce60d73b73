#include "kernels_common.h"
#include "kernels.h"


// ---------------------------------------------------------------------------
// GEMV family — decode's workhorse (HBM-bound weight streaming at 16 B/lane,
// guide §5 "GEMV / M <= 16": weights straight to VGPRs, no LDS round trip).
//
// k_gemv_reg<ROWS, EPI, NORM, KB>: x is loaded ONCE into registers (up to
// KB*8 f32/thread, K <= KB*2048) and reused for every row; with NORM the
// kernel fuses the preceding rms_norm (backends/mod.rs:244-246) into the
// x load — the normed value is re-quantized to bf16 so the fused path is
// bit-identical to rmsnorm-then-gemv.  ROWS per block is chosen by the
// launcher so the grid has >= ~2048 workgroups (256 CUs want many blocks).
// EPI: 0 = bf16 out; 1 = bf16 out + residual add; 2 = f32 out (logits).
// ---------------------------------------------------------------------------
template <int ROWS, int EPI, bool NORM, int KB>
__global__ __launch_bounds__(256) void k_gemv_reg(
    const u16* __restrict__ W, const u16* __restrict__ x,
    void* __restrict__ out, const u16* __restrict__ res,
    const u16* __restrict__ nw, float eps, int N, int K) {
  const int t = threadIdx.x;
  const int row0 = blockIdx.x * ROWS;
  const int wid = t / WAVE, lane = t % WAVE;
  __shared__ float red[ROWS > 4 ? ROWS : 4][4];

  // Load issue order = consumer order (guide T20 follow-on: a wait
  // belongs at the first consumer, and hipcc's guarded blocks degrade
  // counted waits to vmcnt(0) drains — so the group whose consumer comes
  // FIRST must issue first).  x feeds the sumsq immediately; the norm
  // weights are consumed after the reduction barrier; the row weights
  // last, in the FMA phase.  All three groups are in flight together, so
  // a drain before sumsq costs one memory latency, not three.
  // All loads below are UNGUARDED with clamped addresses (same fix as the
  // attention kernel): an `if (row < N && k0 < K)` around a load costs
  // hipcc an execz block + vmcnt(0) drain per unrolled iteration.  Out-of-
  // range k contributes 0 through xr (zeroed beyond K); out-of-range rows
  // compute garbage sums that the guarded epilogue never stores.
  // KB == 1 can be ragged (K < 2048, e.g. qwen3-0.6b H=1024): there the
  // guard SKIPS loads for fully out-of-range threads, which beats the
  // clamped duplicate loads (-2.4% A/B'd on qwen3-0.6b); KB >= 2 shapes
  // win with clamping (no execz blocks, counted waits).
  short8 xpre[KB];
#pragma unroll
  for (int i = 0; i < KB; ++i) {
    if constexpr (KB >= 2) {
      const int k0c = max(0, min(i * 2048 + t * 8, K - 8));
      xpre[i] = *reinterpret_cast<const short8*>(x + k0c);
    } else {
      const int k0 = i * 2048 + t * 8;
      if (k0 < K) xpre[i] = *reinterpret_cast<const short8*>(x + k0);
    }
  }
  // EPI == 1: the residual element of the row this thread will store,
  // requested here instead of after the final barrier (one dependent round
  // trip at the tail of every block).  The product passes res == out
  // (e->x, in place) although both are __restrict__: the early read is safe
  // because row `row0 + t` is read here and written in the epilogue by this
  // SAME thread and by no other block — keep it that way.  Every thread
  // loads (clamped to the block's last live row; only t < ROWS uses it): a
  // load under `if (t < ROWS)` would get its own vmcnt(0) drain.
  u16 respre = 0;
  if constexpr (EPI == 1)
    respre = res[min(row0 + min(t, ROWS - 1), N - 1)];
  short8 nwpre[NORM ? KB : 1];
  if (NORM) {
#pragma unroll
    for (int i = 0; i < KB; ++i) {
      if constexpr (KB >= 2) {
        const int k0c = max(0, min(i * 2048 + t * 8, K - 8));
        nwpre[i] = *reinterpret_cast<const short8*>(nw + k0c);
      } else {
        const int k0 = i * 2048 + t * 8;
        if (k0 < K) nwpre[i] = *reinterpret_cast<const short8*>(nw + k0);
      }
    }
  }
  // For short K, issue ALL weight loads too — they stay in flight across
  // the x/norm phase (plain VGPR loads survive s_barrier; guide §5
  // pipelining note), hiding the norm reduction latency entirely.
  short8 wpre[KB <= 2 ? ROWS : 1][KB <= 2 ? KB : 1];
  if (KB <= 2) {
#pragma unroll
    for (int r = 0; r < ROWS; ++r)
#pragma unroll
      for (int i = 0; i < KB; ++i) {
        if constexpr (KB >= 2) {
          const int k0c = max(0, min(i * 2048 + t * 8, K - 8));
          const int rc = min(row0 + r, N - 1);
          wpre[r][i] = ntload8(W + (size_t)rc * K + k0c);
        } else {
          const int k0 = i * 2048 + t * 8;
          if (row0 + r < N && k0 < K)
            wpre[r][i] = ntload8(W + (size_t)(row0 + r) * K + k0);
        }
      }
  }

  // phase 1: x -> f32, optionally fused rms_norm (k >= K slots zeroed so
  // the clamped duplicate loads contribute nothing anywhere downstream)
  float xr[KB * 8];
#pragma unroll
  for (int i = 0; i < KB; ++i) {
    const bool in = i * 2048 + t * 8 < K;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      xr[i * 8 + j] = in ? b2f((u16)xpre[i][j]) : 0.f;
  }
  if (NORM) {
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
          // re-quantize so fused == rmsnorm-kernel-then-gemv bit-exactly
          xr[i * 8 + j] =
              b2f(f2b(xr[i * 8 + j] * scale * b2f((u16)nwpre[i][j])));
      }
    }
  }

  // phase 2: FMA with the prefetched weights (KB<=2) or stream rows with
  // all rows' loads unrolled together (KB>2) — memory-level parallelism
  float acc[ROWS];
#pragma unroll
  for (int r = 0; r < ROWS; ++r) acc[r] = 0.f;
  if (KB <= 2) {
#pragma unroll
    for (int r = 0; r < ROWS; ++r)
#pragma unroll
      for (int i = 0; i < KB; ++i) {
        if (KB >= 2 || (row0 + r < N && i * 2048 + t * 8 < K)) {
#pragma unroll
          for (int j = 0; j < 8; ++j)
            acc[r] = fmaf(b2f((u16)wpre[r][i][j]), xr[i * 8 + j], acc[r]);
        }
      }
  } else {
#pragma unroll
    for (int i = 0; i < KB; ++i) {
      const int k0c = max(0, min(i * 2048 + t * 8, K - 8));
      short8 wv[ROWS];
#pragma unroll
      for (int r = 0; r < ROWS; ++r)
        wv[r] = ntload8(W + (size_t)min(row0 + r, N - 1) * K + k0c);
#pragma unroll
      for (int r = 0; r < ROWS; ++r) {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          acc[r] = fmaf(b2f((u16)wv[r][j]), xr[i * 8 + j], acc[r]);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < ROWS; ++r) {
    float v = wave_sum(acc[r]);
    if (lane == 0) red[r][wid] = v;
  }
  __syncthreads();
  if (t < ROWS) {
    const int row = row0 + t;
    if (row < N) {
      float v = red[t][0] + red[t][1] + red[t][2] + red[t][3];
      if (EPI == 2) {
        reinterpret_cast<float*>(out)[row] = v;
      } else if (EPI == 1) {
        reinterpret_cast<u16*>(out)[row] = f2b(v + b2f(respre));
      } else {
        reinterpret_cast<u16*>(out)[row] = f2b(v);
      }
    }
  }
}

// streaming fallback for K > 16384 (e.g. 70B down-proj K=28672): x re-read
// from L1/L2 per row
template <int ROWS, int EPI>
__global__ __launch_bounds__(256) void k_gemv_stream(
    const u16* __restrict__ W, const u16* __restrict__ x,
    void* __restrict__ out, const u16* __restrict__ res, int N, int K) {
  const int t = threadIdx.x;
  const int row0 = blockIdx.x * ROWS;
  const int wid = t / WAVE, lane = t % WAVE;
  float acc[ROWS];
#pragma unroll
  for (int r = 0; r < ROWS; ++r) acc[r] = 0.f;
  const int kiter = (K + 2047) / 2048;
  // k-outer with all rows' loads issued per iteration (ROWS+1 loads in
  // flight instead of a serial per-row chain), unguarded with clamped
  // addresses: out-of-range k zeroes x, out-of-range rows compute garbage
  // the guarded epilogue never stores.  K % 8 == 0 is the call contract
  // for this path (checked by the launcher's K % 8 dispatch).
#pragma unroll 1
  for (int i = 0; i < kiter; ++i) {
    const int k0 = i * 2048 + t * 8;
    const int k0c = max(0, min(k0, K - 8));
    short8 xv = *reinterpret_cast<const short8*>(x + k0c);
    float xf[8];
#pragma unroll
    for (int j = 0; j < 8; ++j)
      xf[j] = k0 + 8 <= K ? b2f((u16)xv[j]) : 0.f;
    short8 wv[ROWS];
#pragma unroll
    for (int r = 0; r < ROWS; ++r)
      wv[r] = ntload8(W + (size_t)min(row0 + r, N - 1) * K + k0c);
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        acc[r] = fmaf(b2f((u16)wv[r][j]), xf[j], acc[r]);
    }
  }
  // scalar tail for K % 8 != 0 (op-level shapes; model dims are % 8):
  // thread t < K % 8 handles element (K - K%8 + t) for every row; the
  // wave/block reduction below folds it in like any other partial
  if (K % 8) {
    const int k = K - K % 8 + t;
    if (t < K % 8) {
      const float xt = b2f(x[k]);
#pragma unroll
      for (int r = 0; r < ROWS; ++r)
        if (row0 + r < N)
          acc[r] = fmaf(b2f(W[(size_t)(row0 + r) * K + k]), xt, acc[r]);
    }
  }
  __shared__ float red[ROWS > 4 ? ROWS : 4][4];
#pragma unroll
  for (int r = 0; r < ROWS; ++r) {
    float v = wave_sum(acc[r]);
    if (lane == 0) red[r][wid] = v;
  }
  __syncthreads();
  if (t < ROWS) {
    const int row = row0 + t;
    if (row < N) {
      float v = red[t][0] + red[t][1] + red[t][2] + red[t][3];
      if (EPI == 2) {
        reinterpret_cast<float*>(out)[row] = v;
      } else if (EPI == 1) {
        reinterpret_cast<u16*>(out)[row] = f2b(v + b2f(res[row]));
      } else {
        reinterpret_cast<u16*>(out)[row] = f2b(v);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Fused [rms_norm ->] qkv GEMV -> rope -> KV-cache store, for the decode
// step of full-rotation models without qk-norm (llama family: rd == hd).
// Replaces the k_gemv_reg<.,0,true,.> + k_rope_store_decode launch pair —
// one less kernel per layer, and the rope math runs on the dot-product
// sums already sitting in LDS.
//
// Row mapping: a rope pair is (i, i + hd/2) within a head, so a q/k block
// owns TWO pairs {base+i0, base+i0+1, base+i0+hd/2, base+i0+hd/2+1}
// (i0 = 2*(b % (hd/4)), base = the head's first row).  V rows need no
// rotation and map consecutively.  Epilogue: q rows rope'd into the qkv
// activation buffer (attention reads them there), k rows rope'd into
// kc[kvh][p], v rows into vc[kvh][p] + the transposed vtc image.
// (kernels_attn.hip:31-76 is the unfused reference semantics.)
// ---------------------------------------------------------------------------
template <int KB>
__global__ __launch_bounds__(256) void k_gemv_qkv_rope(
    const u16* __restrict__ W, const u16* __restrict__ x,
    u16* __restrict__ out, const u16* __restrict__ nw, float eps,
    u16* __restrict__ kc, u16* __restrict__ vc, u16* __restrict__ vtc,
    const float* __restrict__ cost, const float* __restrict__ sint,
    const int* __restrict__ pos, int nh, int nkv, int hd, int max_seq,
    int K) {
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

  // same load-issue order as k_gemv_reg: x, norm weights, then row weights
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
  // The epilogue's operands: pos, then this block's two cos/sin pairs (a
  // fresh cache line every step).  They used to be read by thread 0 AFTER
  // the final barrier — two dependent round trips at the tail of every
  // block; requested here they land under the weight stream and the
  // epilogue runs from registers.  V blocks need none and read pair 0
  // (i0 == 0), which keeps the loads branch-free.  Placed BEHIND the vector
  // load issue: ahead of it, hipcc parks every x/weight load behind the
  // scalar wait on pos.
  const int p = *pos;
  const float rc0 = cost[(size_t)p * half + i0];
  const float rc1 = cost[(size_t)p * half + i0 + 1];
  const float rs0 = sint[(size_t)p * half + i0];
  const float rs1 = sint[(size_t)p * half + i0 + 1];
  // pin the loads HERE: the tables are read-only __restrict__, so hipcc
  // otherwise sinks them back into thread 0's epilogue branch, behind the
  // final barrier
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

// ---- host-side kernel choices (queried by cake_hip_linear_dispatch; the
// launchers below go through the same functions) ---------------------------
int gemv_kb(int K) {  // k_gemv_reg / k_gemv_gateup; 0 = k_gemv_stream
  if (K > 16384) return 0;
  return K <= 4096 ? 2 : K <= 8192 ? 4 : 8;
}
int gemv_fp8_kb(int K) {  // k_gemv_fp8 / k_gemv_gateup_fp8; 0 = stream
  if (K > 16384) return 0;
  return K <= 4096 ? 1 : K <= 8192 ? 2 : 4;
}
int gemv_qkv_rope_kb(int K) {
  return K <= 2048 ? 1 : K <= 4096 ? 2 : K <= 8192 ? 4 : 8;
}
int gemv_splitk_kb(int K) {  // KB of the half-K slice
  const int kpart = K / 2;
  return kpart <= 2048 ? 1 : kpart <= 4096 ? 2 : kpart <= 8192 ? 4 : 8;
}
int gemv_rows_policy(int N, int K) {
  // small row-count per block keeps the grid >= ~2048 workgroups on the
  // usual decode shapes (256 CUs need many blocks to reach HBM peak)
  static const int env_small = [] {
    const char* v = getenv("CAKE_GEMV_ROWS_SMALL");
    return v ? atoi(v) : 0;
  }();
  if (N >= 16384) return 8;                 // lm_head: maximal block count
  if (env_small) return env_small;          // A/B override
  if (K >= 8192) return 4;                  // long rows amortize x reload
  return (N >= 6144) ? 4 : 2;
}
int gemv_gateup_rows_policy() {
  static const int rows = [] {
    const char* v = getenv("CAKE_GU_ROWS");
    return v && atoi(v) == 8 ? 8 : 4;
  }();
  return rows;
}
int gemv_fp8_rows_policy(int N) {
  static const int env_rows = [] {
    const char* v = getenv("CAKE_FP8_ROWS");
    return v ? atoi(v) : 0;
  }();
  return N >= 16384 ? 8 : (env_rows ? env_rows : 4);
}

void launch_gemv_qkv_rope(const u16* W, const u16* x, u16* out, const u16* nw,
                          float eps, u16* kc, u16* vc, u16* vtc,
                          const float* cost, const float* sint,
                          const int* pos, int nh, int nkv, int hd, int rd,
                          int max_seq, int K, hipStream_t s,
                          const float* bias) {
  if (rd != hd) {  // partial rotary: its own translation unit as well
    launch_gemv_qkv_rope_pr(W, x, out, nw, eps, kc, vc, vtc, cost, sint, pos,
                            nh, nkv, hd, rd, max_seq, K, s);
    return;
  }
  if (bias) {  // qwen2: the biased twin lives in its own translation unit
    launch_gemv_qkv_rope_bias(W, x, out, nw, eps, kc, vc, vtc, cost, sint, pos,
                              bias, nh, nkv, hd, max_seq, K, s);
    return;
  }
  const int nblk = (nh + 2 * nkv) * hd / 4;
  dim3 grid(nblk);
#define QKR(KB)                                                             \
  hipLaunchKernelGGL((k_gemv_qkv_rope<KB>), grid, dim3(256), 0, s, W, x,    \
                     out, nw, eps, kc, vc, vtc, cost, sint, pos, nh, nkv,   \
                     hd, max_seq, K)
  const int kb = gemv_qkv_rope_kb(K);
  if (kb == 1) QKR(1);
  else if (kb == 2) QKR(2);
  else if (kb == 4) QKR(4);
  else QKR(8);
#undef QKR
}

// fused [rms_norm ->] gate_up GEMV -> silu_mul: block computes
// out[i] = silu(g_i) * u_i for 8 channels, g_i = dot(W[i,:], xn),
// u_i = dot(W[i+I,:], xn)  (mlp.rs:21-31 + fused gate_up of mlp.rs:38-46)
template <int ROWS, bool NORM, int KB>
__global__ __launch_bounds__(256) void k_gemv_gateup(
    const u16* __restrict__ W, const u16* __restrict__ x,
    u16* __restrict__ out, const u16* __restrict__ nw, float eps, int I,
    int K) {
  const int t = threadIdx.x;
  const int c0 = blockIdx.x * ROWS;
  const int wid = t / WAVE, lane = t % WAVE;
  __shared__ float redg[8][4], redu[8][4];

  // load issue order = consumer order (see k_gemv_reg): x first (feeds
  // sumsq), then norm weights (consumed after the barrier)
  // unguarded clamped loads for KB >= 2, guarded for ragged KB == 1
  // (see k_gemv_reg)
  short8 xpre[KB];
#pragma unroll
  for (int i = 0; i < KB; ++i) {
    if constexpr (KB >= 2) {
      const int k0c = max(0, min(i * 2048 + t * 8, K - 8));
      xpre[i] = *reinterpret_cast<const short8*>(x + k0c);
    } else {
      const int k0 = i * 2048 + t * 8;
      if (k0 < K) xpre[i] = *reinterpret_cast<const short8*>(x + k0);
    }
  }
  short8 nwpre[NORM ? KB : 1];
  if (NORM) {
#pragma unroll
    for (int i = 0; i < KB; ++i) {
      if constexpr (KB >= 2) {
        const int k0c = max(0, min(i * 2048 + t * 8, K - 8));
        nwpre[i] = *reinterpret_cast<const short8*>(nw + k0c);
      } else {
        const int k0 = i * 2048 + t * 8;
        if (k0 < K) nwpre[i] = *reinterpret_cast<const short8*>(nw + k0);
      }
    }
  }
  // KB == 2 with NORM (the 8B decode shape): the i == 0 slab's weight loads
  // go out here, ahead of the norm's two barriers, as k_gemv_reg does for
  // KB <= 2 — otherwise every block sits through the x round trip and the
  // reduction before its first weight byte is requested.
  constexpr bool PRE = NORM && KB == 2;
  short8 gpre[PRE ? ROWS : 1], upre[PRE ? ROWS : 1];
  if constexpr (PRE) {
    const int k0c = max(0, min(t * 8, K - 8));
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
      const int rc = min(c0 + r, I - 1);
      gpre[r] = ntload8(W + (size_t)rc * K + k0c);
      upre[r] = ntload8(W + (size_t)(rc + I) * K + k0c);
    }
  }
  float xr[KB * 8];
#pragma unroll
  for (int i = 0; i < KB; ++i) {
    const bool in = i * 2048 + t * 8 < K;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      xr[i * 8 + j] = in ? b2f((u16)xpre[i][j]) : 0.f;
  }
  if (NORM) {
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < KB * 8; ++i) ss += xr[i] * xr[i];
    ss = wave_sum(ss);
    if (lane == 0) redg[0][wid] = ss;
    __syncthreads();
    const float scale =
        rsqrtf((redg[0][0] + redg[0][1] + redg[0][2] + redg[0][3]) /
                   (float)K + eps);
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

  float accg[ROWS], accu[ROWS];
#pragma unroll
  for (int r = 0; r < ROWS; ++r) accg[r] = accu[r] = 0.f;
#pragma unroll
  for (int i = 0; i < KB; ++i) {
    if constexpr (KB >= 2) {
      const int k0c = max(0, min(i * 2048 + t * 8, K - 8));
      short8 gv[ROWS], uv[ROWS];
#pragma unroll
      for (int r = 0; r < ROWS; ++r) {
        if (PRE && i == 0) {
          gv[r] = gpre[r];
          uv[r] = upre[r];
          continue;
        }
        const int rc = min(c0 + r, I - 1);
        gv[r] = ntload8(W + (size_t)rc * K + k0c);
        uv[r] = ntload8(W + (size_t)(rc + I) * K + k0c);
      }
#pragma unroll
      for (int r = 0; r < ROWS; ++r) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          accg[r] = fmaf(b2f((u16)gv[r][j]), xr[i * 8 + j], accg[r]);
          accu[r] = fmaf(b2f((u16)uv[r][j]), xr[i * 8 + j], accu[r]);
        }
      }
    } else {
      const int k0 = i * 2048 + t * 8;
      if (k0 < K) {
        short8 gv[ROWS], uv[ROWS];
#pragma unroll
        for (int r = 0; r < ROWS; ++r)
          if (c0 + r < I) {
            gv[r] = ntload8(W + (size_t)(c0 + r) * K + k0);
            uv[r] = ntload8(W + (size_t)(c0 + r + I) * K + k0);
          }
#pragma unroll
        for (int r = 0; r < ROWS; ++r)
          if (c0 + r < I) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              accg[r] = fmaf(b2f((u16)gv[r][j]), xr[i * 8 + j], accg[r]);
              accu[r] = fmaf(b2f((u16)uv[r][j]), xr[i * 8 + j], accu[r]);
            }
          }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < ROWS; ++r) {
    float g = wave_sum(accg[r]);
    float u = wave_sum(accu[r]);
    if (lane == 0) { redg[r][wid] = g; redu[r][wid] = u; }
  }
  __syncthreads();
  if (t < ROWS && c0 + t < I) {
    float g = redg[t][0] + redg[t][1] + redg[t][2] + redg[t][3];
    float u = redu[t][0] + redu[t][1] + redu[t][2] + redu[t][3];
    out[c0 + t] = f2b(g / (1.f + __expf(-g)) * u);
  }
}

// ---------------------------------------------------------------------------
// FP8 GEMV family — same structure as k_gemv_reg but weights are e4m3fn
// bytes with blockwise 128x128 scale_inv (utils/fp8.rs:42-64), dequantized
// in-register: HALF the HBM bytes per decode step.  16 weights per 16-B
// lane load.  KB here = ceil(K/4096) (thread covers 16 elems per iter).
// ---------------------------------------------------------------------------

// fp8 norm chain (kernels.h NormIO): the x-producing GEMV's wave 0
// publishes its block's sumsq-of-quantized-outputs partial (sc1 store +
// drain + arrival, Guideline 16 R1), and the last-arriving block reduces
// the partials in FIXED lane/chunk order (deterministic across runs) and
// writes scale_out — replacing the split-norm rmsnorm LAUNCH ahead of the
// next fp8 GEMV (two launches/layer, ~9.6 us at 64 layers).
__device__ inline void normchain_produce(const NormIO& nio, float vsq,
                                         int n, int lane) {
  float s = wave_sum(vsq);
  const u32 ng = gridDim.x;
  // Arrival counters sharded by blockIdx residue (8 shards + a top
  // counter, nio.cnt[0..8]): the producer grids are ~1280 blocks that
  // finish nearly simultaneously, and one word saturates at ~88
  // dequeues/us — a single counter cost ~13 us per launch (measured:
  // down/o +11-15 us, a net REGRESSION vs the split-norm launches).
  // Residue sharding is placement-independent (threshold = the exact
  // block count of the residue class, not an XCD guess).
  const u32 shard = blockIdx.x & 7u;
  const u32 shard_total = (ng - shard + 7u) >> 3;
  u32 v = 0;
  if (lane == 0) {
    __hip_atomic_store(&nio.part[blockIdx.x], s, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    v = __hip_atomic_fetch_add(&nio.cnt[shard], 1u, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
  }
  v = __shfl(v, 0, WAVE);
  if (v % shard_total != shard_total - 1) return;
  // The elected arrival is the LAST of its class in this launch (launches
  // on these counters are stream-ordered), so it re-zeroes the word: a
  // monotonic u32 under a modulus that does not divide 2^32 (shard_total
  // is e.g. 160) shifts its election phase when it wraps, after ~4e5
  // tokens, and the scale would then come from a half-arrived launch.
  u32 tv = 0;
  if (lane == 0) {
    __hip_atomic_store(&nio.cnt[shard], 0u, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
    tv = __hip_atomic_fetch_add(&nio.cnt[8], 1u, __ATOMIC_RELAXED,
                                __HIP_MEMORY_SCOPE_AGENT);
  }
  tv = __shfl(tv, 0, WAVE);
  if (tv % 8u != 7u) return;
  if (lane == 0)  // modulus 8 survives the wrap; zeroed for symmetry
    __hip_atomic_store(&nio.cnt[8], 0u, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
  // Elected reduce: ONE agent acquire then PLAIN unguarded clamped loads
  // in batches of 8 (relaxed-ATOMIC loads do not batch — each emits its
  // own wait, ~20 serial uncached round trips on the elected
  // (= last-finishing) block extended the whole kernel wall by ~11-15 us;
  // same acquire-then-plain pattern as the attention combine).
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  const int per = ((int)ng + WAVE - 1) / WAVE;
  float acc = 0.f;
  for (int j0 = 0; j0 < per; j0 += 8) {
    float vals[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int i = min(lane * per + j0 + u, (int)ng - 1);
      vals[u] = nio.part[i];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int i = lane * per + j0 + u;
      acc += (i < (int)ng && j0 + u < per) ? vals[u] : 0.f;
    }
  }
  const float tot = wave_sum(acc);  // fixed tree: deterministic
  if (lane == 0)
    __hip_atomic_store(nio.scale_out,
                       rsqrtf(tot / (float)n + nio.eps), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
}

// consume side: normalize the in-register x with the precomputed scale and
// the rms weight row, re-quantized so it matches the rmsnorm-kernel-then-
// gemv pair bit-exactly given the same scale value
template <int KB>
__device__ inline void normchain_apply(float* xr, const u16* nw, float scale,
                                       int t, int K) {
#pragma unroll
  for (int i = 0; i < KB; ++i) {
    const int k0 = i * 4096 + t * 16;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      if (KB >= 2) {
        const int k0c = max(0, min(k0, K - 16)) + half * 8;
        short8 wv = *reinterpret_cast<const short8*>(nw + k0c);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int ix = i * 16 + half * 8 + j;
          xr[ix] = b2f(f2b(xr[ix] * scale * b2f((u16)wv[j])));
        }
      } else if (k0 < K) {
        short8 wv = *reinterpret_cast<const short8*>(nw + k0 + half * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int ix = i * 16 + half * 8 + j;
          xr[ix] = b2f(f2b(xr[ix] * scale * b2f((u16)wv[j])));
        }
      }
    }
  }
}

template <int ROWS, int EPI, bool NORM, int KB>
__global__ __launch_bounds__(256) void k_gemv_fp8(
    const unsigned char* __restrict__ W, const float* __restrict__ sc,
    const u16* __restrict__ x, void* __restrict__ out,
    const u16* __restrict__ res, const u16* __restrict__ nw, float eps,
    int N, int K, int nkb, NormIO nio) {
  const int t = threadIdx.x;
  const int row0 = blockIdx.x * ROWS;
  const int wid = t / WAVE, lane = t % WAVE;
  __shared__ float red[ROWS > 4 ? ROWS : 4][4];

  // prefetch all weight tiles (stay in flight across the x/norm phase);
  // unguarded clamped addresses for KB >= 2 (see k_gemv_reg: guarded
  // loads cost an execz block + vmcnt(0) drain per unrolled iteration)
  uint4v wpre[ROWS][KB];
#pragma unroll
  for (int r = 0; r < ROWS; ++r)
#pragma unroll
    for (int i = 0; i < KB; ++i) {
      if constexpr (KB >= 2) {
        const int k0c = max(0, min(i * 4096 + t * 16, K - 16));
        wpre[r][i] =
            ntload16b(W + (size_t)min(row0 + r, N - 1) * K + k0c);
      } else {
        const int k0 = i * 4096 + t * 16;
        if (row0 + r < N && k0 < K)
          wpre[r][i] = ntload16b(W + (size_t)(row0 + r) * K + k0);
      }
    }

  // x -> registers (f32), optionally fused rms_norm.  (The bf16 kernels'
  // early nw/x prefetch is a measured NEGATIVE here: fp8 runs at lower
  // occupancy and the extra live short8 registers cost more than the
  // hidden latency buys — A/B'd -5% on qwen3-32b-fp8 decode.)
  float xr[KB * 16];
#pragma unroll
  for (int i = 0; i < KB; ++i) {
    const int k0 = i * 4096 + t * 16;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      if (KB >= 2) {
        const int k0c = max(0, min(k0, K - 16)) + half * 8;
        short8 xv = *reinterpret_cast<const short8*>(x + k0c);
#pragma unroll
        for (int j = 0; j < 8; ++j)
          xr[i * 16 + half * 8 + j] = k0 < K ? b2f((u16)xv[j]) : 0.f;
      } else if (k0 < K) {
        short8 xv = *reinterpret_cast<const short8*>(x + k0 + half * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j)
          xr[i * 16 + half * 8 + j] = b2f((u16)xv[j]);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) xr[i * 16 + half * 8 + j] = 0.f;
      }
    }
  }
  if (NORM) {
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < KB * 16; ++i) ss += xr[i] * xr[i];
    ss = wave_sum(ss);
    if (lane == 0) red[0][wid] = ss;
    __syncthreads();
    const float scale =
        rsqrtf((red[0][0] + red[0][1] + red[0][2] + red[0][3]) / (float)K +
               eps);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < KB; ++i) {
      const int k0 = i * 4096 + t * 16;
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        if (KB >= 2) {
          const int k0c = max(0, min(k0, K - 16)) + half * 8;
          short8 wv = *reinterpret_cast<const short8*>(nw + k0c);
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const int ix = i * 16 + half * 8 + j;
            xr[ix] = b2f(f2b(xr[ix] * scale * b2f((u16)wv[j])));
          }
        } else if (k0 < K) {
          short8 wv =
              *reinterpret_cast<const short8*>(nw + k0 + half * 8);
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const int ix = i * 16 + half * 8 + j;
            xr[ix] = b2f(f2b(xr[ix] * scale * b2f((u16)wv[j])));
          }
        }
      }
    }
  }

  if (!NORM && nio.scale_in != nullptr)
    normchain_apply<KB>(xr, nio.nw, *nio.scale_in, t, K);
  float acc[ROWS];
#pragma unroll
  for (int r = 0; r < ROWS; ++r) acc[r] = 0.f;
#pragma unroll
  for (int r = 0; r < ROWS; ++r)
#pragma unroll
    for (int i = 0; i < KB; ++i) {
      const int k0 = i * 4096 + t * 16;
      if (KB >= 2 || (row0 + r < N && k0 < K)) {
        // one scale_inv block covers this thread's 16 k's (k0 % 16 == 0);
        // clamped indices keep the scale read in-bounds for the dup loads
        const int rc = min(row0 + r, N - 1);
        const int k0c = max(0, min(k0, K - 16));
        const float s = sc[(size_t)(rc / 128) * nkb + (k0c / 128)];
        float wd[16];
        f8x16_decode(wpre[r][i], wd);
        float a = 0.f;
#pragma unroll
        for (int j = 0; j < 16; ++j)
          a = fmaf(wd[j], xr[i * 16 + j], a);
        acc[r] = fmaf(a, s, acc[r]);
      }
    }
#pragma unroll
  for (int r = 0; r < ROWS; ++r) {
    float v = wave_sum(acc[r]);
    if (lane == 0) red[r][wid] = v;
  }
  __syncthreads();
  float vsq = 0.f;
  if (t < ROWS) {
    const int row = row0 + t;
    if (row < N) {
      float v = red[t][0] + red[t][1] + red[t][2] + red[t][3];
      if (EPI == 2) {
        reinterpret_cast<float*>(out)[row] = v;
      } else if (EPI == 1) {
        const u16 q = f2b(v + b2f(res[row]));
        reinterpret_cast<u16*>(out)[row] = q;
        vsq = b2f(q) * b2f(q);
      } else {
        reinterpret_cast<u16*>(out)[row] = f2b(v);
      }
    }
  }
  if (EPI == 1 && nio.scale_out != nullptr && wid == 0)
    normchain_produce(nio, vsq, N, lane);
}

// fp8 streaming fallback for K > 16384 (e.g. Qwen3-32B down K=25600)
template <int ROWS, int EPI>
__global__ __launch_bounds__(256) void k_gemv_fp8_stream(
    const unsigned char* __restrict__ W, const float* __restrict__ sc,
    const u16* __restrict__ x, void* __restrict__ out,
    const u16* __restrict__ res, int N, int K, int nkb, NormIO nio) {
  const int t = threadIdx.x;
  const int row0 = blockIdx.x * ROWS;
  const int wid = t / WAVE, lane = t % WAVE;
  float acc[ROWS];
#pragma unroll
  for (int r = 0; r < ROWS; ++r) acc[r] = 0.f;
  const int kiter = (K + 4095) / 4096;
  // unguarded clamped body (see k_gemv_reg): all ROWS+2 loads of an
  // iteration issue together; out-of-range k zeroes x, out-of-range rows
  // compute garbage the guarded epilogue never stores.  K % 16 == 0 on
  // this path (fp8 blocks are 128-wide).
#pragma unroll 1
  for (int i = 0; i < kiter; ++i) {
    const int k0 = i * 4096 + t * 16;
    const int k0c = max(0, min(k0, K - 16));
    float xv[16];
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      short8 xs = *reinterpret_cast<const short8*>(x + k0c + half * 8);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        xv[half * 8 + j] = k0 < K ? b2f((u16)xs[j]) : 0.f;
    }
    uint4v wv[ROWS];
#pragma unroll
    for (int r = 0; r < ROWS; ++r)
      wv[r] = ntload16b(W + (size_t)min(row0 + r, N - 1) * K + k0c);
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
      const float s =
          sc[(size_t)(min(row0 + r, N - 1) / 128) * nkb + (k0c / 128)];
      float wd[16];
      f8x16_decode(wv[r], wd);
      float a = 0.f;
#pragma unroll
      for (int j = 0; j < 16; ++j)
        a = fmaf(wd[j], xv[j], a);
      acc[r] = fmaf(a, s, acc[r]);
    }
  }
  __shared__ float red[ROWS > 4 ? ROWS : 4][4];
#pragma unroll
  for (int r = 0; r < ROWS; ++r) {
    float v = wave_sum(acc[r]);
    if (lane == 0) red[r][wid] = v;
  }
  __syncthreads();
  float vsq = 0.f;
  if (t < ROWS) {
    const int row = row0 + t;
    if (row < N) {
      float v = red[t][0] + red[t][1] + red[t][2] + red[t][3];
      if (EPI == 2) {
        reinterpret_cast<float*>(out)[row] = v;
      } else if (EPI == 1) {
        const u16 q = f2b(v + b2f(res[row]));
        reinterpret_cast<u16*>(out)[row] = q;
        vsq = b2f(q) * b2f(q);
      } else {
        reinterpret_cast<u16*>(out)[row] = f2b(v);
      }
    }
  }
  if (EPI == 1 && nio.scale_out != nullptr && wid == 0)
    normchain_produce(nio, vsq, N, lane);
}

// fp8 gate_up + silu_mul (the fused MLP front half, fp8 weights)
template <int ROWS, bool NORM, int KB>
__global__ __launch_bounds__(256) void k_gemv_gateup_fp8(
    const unsigned char* __restrict__ W, const float* __restrict__ sc,
    const u16* __restrict__ x, u16* __restrict__ out,
    const u16* __restrict__ nw, float eps, int I, int K, int nkb,
    NormIO nio) {
  const int t = threadIdx.x;
  const int c0 = blockIdx.x * ROWS;
  const int wid = t / WAVE, lane = t % WAVE;
  __shared__ float redg[8][4], redu[8][4];

  // x -> registers; unguarded clamped loads for KB >= 2 (see k_gemv_reg)
  float xr[KB * 16];
#pragma unroll
  for (int i = 0; i < KB; ++i) {
    const int k0 = i * 4096 + t * 16;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      if (KB >= 2) {
        const int k0c = max(0, min(k0, K - 16)) + half * 8;
        short8 xv = *reinterpret_cast<const short8*>(x + k0c);
#pragma unroll
        for (int j = 0; j < 8; ++j)
          xr[i * 16 + half * 8 + j] = k0 < K ? b2f((u16)xv[j]) : 0.f;
      } else if (k0 < K) {
        short8 xv = *reinterpret_cast<const short8*>(x + k0 + half * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j)
          xr[i * 16 + half * 8 + j] = b2f((u16)xv[j]);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) xr[i * 16 + half * 8 + j] = 0.f;
      }
    }
  }
  if (NORM) {
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < KB * 16; ++i) ss += xr[i] * xr[i];
    ss = wave_sum(ss);
    if (lane == 0) redg[0][wid] = ss;
    __syncthreads();
    const float scale =
        rsqrtf((redg[0][0] + redg[0][1] + redg[0][2] + redg[0][3]) /
                   (float)K + eps);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < KB; ++i) {
      const int k0 = i * 4096 + t * 16;
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        if (KB >= 2) {
          const int k0c = max(0, min(k0, K - 16)) + half * 8;
          short8 wv = *reinterpret_cast<const short8*>(nw + k0c);
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const int ix = i * 16 + half * 8 + j;
            xr[ix] = b2f(f2b(xr[ix] * scale * b2f((u16)wv[j])));
          }
        } else if (k0 < K) {
          short8 wv =
              *reinterpret_cast<const short8*>(nw + k0 + half * 8);
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const int ix = i * 16 + half * 8 + j;
            xr[ix] = b2f(f2b(xr[ix] * scale * b2f((u16)wv[j])));
          }
        }
      }
    }
  }

  if (!NORM && nio.scale_in != nullptr)
    normchain_apply<KB>(xr, nio.nw, *nio.scale_in, t, K);
  float accg[ROWS], accu[ROWS];
#pragma unroll
  for (int r = 0; r < ROWS; ++r) accg[r] = accu[r] = 0.f;
#pragma unroll
  for (int i = 0; i < KB; ++i) {
    const int k0 = i * 4096 + t * 16;
    if (KB >= 2) {
      const int k0c = max(0, min(k0, K - 16));
      uint4v gv[ROWS], uv[ROWS];
#pragma unroll
      for (int r = 0; r < ROWS; ++r) {
        const int rc = min(c0 + r, I - 1);
        gv[r] = ntload16b(W + (size_t)rc * K + k0c);
        uv[r] = ntload16b(W + (size_t)(rc + I) * K + k0c);
      }
#pragma unroll
      for (int r = 0; r < ROWS; ++r) {
        const int rc = min(c0 + r, I - 1);
        const float sg = sc[(size_t)(rc / 128) * nkb + (k0c / 128)];
        const float su = sc[(size_t)((rc + I) / 128) * nkb + (k0c / 128)];
        float gd[16], ud[16];
        f8x16_decode(gv[r], gd);
        f8x16_decode(uv[r], ud);
        float g = 0.f, u = 0.f;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          g = fmaf(gd[j], xr[i * 16 + j], g);
          u = fmaf(ud[j], xr[i * 16 + j], u);
        }
        accg[r] = fmaf(g, sg, accg[r]);
        accu[r] = fmaf(u, su, accu[r]);
      }
    } else if (k0 < K) {
      uint4v gv[ROWS], uv[ROWS];
#pragma unroll
      for (int r = 0; r < ROWS; ++r)
        if (c0 + r < I) {
          gv[r] = ntload16b(W + (size_t)(c0 + r) * K + k0);
          uv[r] = ntload16b(W + (size_t)(c0 + r + I) * K + k0);
        }
#pragma unroll
      for (int r = 0; r < ROWS; ++r)
        if (c0 + r < I) {
          const float sg = sc[(size_t)((c0 + r) / 128) * nkb + (k0 / 128)];
          const float su =
              sc[(size_t)((c0 + r + I) / 128) * nkb + (k0 / 128)];
          float gd[16], ud[16];
          f8x16_decode(gv[r], gd);
          f8x16_decode(uv[r], ud);
          float g = 0.f, u = 0.f;
#pragma unroll
          for (int j = 0; j < 16; ++j) {
            g = fmaf(gd[j], xr[i * 16 + j], g);
            u = fmaf(ud[j], xr[i * 16 + j], u);
          }
          accg[r] = fmaf(g, sg, accg[r]);
          accu[r] = fmaf(u, su, accu[r]);
        }
    }
  }
#pragma unroll
  for (int r = 0; r < ROWS; ++r) {
    float g = wave_sum(accg[r]);
    float u = wave_sum(accu[r]);
    if (lane == 0) { redg[r][wid] = g; redu[r][wid] = u; }
  }
  __syncthreads();
  if (t < ROWS && c0 + t < I) {
    float g = redg[t][0] + redg[t][1] + redg[t][2] + redg[t][3];
    float u = redu[t][0] + redu[t][1] + redu[t][2] + redu[t][3];
    out[c0 + t] = f2b(g / (1.f + __expf(-g)) * u);
  }
}

// fp8 -> bf16 blockwise dequant (prefill path: dequant the layer's weight
// into a scratch buffer, then run the bf16 MFMA GEMM — cake itself
// dequantizes at load time, fp8.rs:42-64; we dequant per layer per prefill
// to keep HBM fp8-resident for decode)
__global__ void k_dequant_fp8(const unsigned char* __restrict__ W,
                              const float* __restrict__ sc,
                              u16* __restrict__ out, int N, int K, int nkb) {
  // 16 consecutive elements per thread iteration: one 16-B weight load,
  // one scale (the 128-wide block covers the whole group; K % 16 == 0 on
  // the fp8 path), one 16-float decode, two 16-B stores.  The scalar
  // per-byte version measured 2.1 TB/s; this is a plain streaming copy.
  size_t i16 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const size_t total = ((size_t)N * K) / 16;
  for (; i16 < total; i16 += stride) {
    const size_t i = i16 * 16;
    const int r = (int)(i / K), k = (int)(i % K);
    const uint4v w = *reinterpret_cast<const uint4v*>(W + i);
    const float s = sc[(size_t)(r / 128) * nkb + k / 128];
    float wd[16];
    f8x16_decode(w, wd);
    short8 o0, o1;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      o0[j] = (short)f2b(wd[j] * s);
      o1[j] = (short)f2b(wd[8 + j] * s);
    }
    *reinterpret_cast<short8*>(out + i) = o0;
    *reinterpret_cast<short8*>(out + i + 8) = o1;
  }
}


// ---------------------------------------------------------------------------
// Split-K GEMV for the residual projections (o_proj, down_proj): the
// full-K kernels are memory-latency-bound per block (PMC: 50-88%
// SQ_WAIT_ANY), so halving each block's serial K-chain and doubling the
// grid buys overlap.  Partials go through write-through sc1 stores + an
// epoch-free arrival counter (the attention kernel's proven Guideline 16
// R1 variant); the last-arriving slice adds the residual and stores bf16.
// ws: [N][KS] f32; cnt: [N/ROWS] u32 (monotonic, modulo-KS election).
// ---------------------------------------------------------------------------
template <int ROWS, int KB, int KS>
__global__ __launch_bounds__(256) void k_gemv_splitk_res(
    const u16* __restrict__ W, const u16* __restrict__ x,
    u16* __restrict__ out, const u16* __restrict__ res,
    float* __restrict__ ws, u32* __restrict__ cnt, int N, int K) {
  const int t = threadIdx.x;
  const int row0 = blockIdx.x * ROWS;
  const int ksl = blockIdx.y;
  const int kpart = K / KS;                 // multiple of 8 by dispatch
  const int kbase = ksl * kpart;
  const int wid = t / WAVE, lane = t % WAVE;
  __shared__ float red[ROWS > 4 ? ROWS : 4][4];

  short8 wpre[ROWS][KB];
#pragma unroll
  for (int r = 0; r < ROWS; ++r)
#pragma unroll
    for (int i = 0; i < KB; ++i) {
      const int k0 = i * 2048 + t * 8;
      if (row0 + r < N && k0 < kpart)
        wpre[r][i] = ntload8(W + (size_t)(row0 + r) * K + kbase + k0);
    }
  float xr[KB * 8];
#pragma unroll
  for (int i = 0; i < KB; ++i) {
    const int k0 = i * 2048 + t * 8;
    if (k0 < kpart) {
      short8 xv = *reinterpret_cast<const short8*>(x + kbase + k0);
#pragma unroll
      for (int j = 0; j < 8; ++j) xr[i * 8 + j] = b2f((u16)xv[j]);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) xr[i * 8 + j] = 0.f;
    }
  }
  float acc[ROWS];
#pragma unroll
  for (int r = 0; r < ROWS; ++r) acc[r] = 0.f;
#pragma unroll
  for (int r = 0; r < ROWS; ++r)
#pragma unroll
    for (int i = 0; i < KB; ++i) {
      const int k0 = i * 2048 + t * 8;
      if (row0 + r < N && k0 < kpart) {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          acc[r] = fmaf(b2f((u16)wpre[r][i][j]), xr[i * 8 + j], acc[r]);
      }
    }
#pragma unroll
  for (int r = 0; r < ROWS; ++r) {
    float v = wave_sum(acc[r]);
    if (lane == 0) red[r][wid] = v;
  }
  __syncthreads();
  // publish partials (sc1 4-B agent stores) and elect the combiner
  if (t < ROWS && row0 + t < N) {
    const float v = red[t][0] + red[t][1] + red[t][2] + red[t][3];
    __hip_atomic_store(&ws[(size_t)(row0 + t) * KS + ksl], v,
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (t == 0) {
    u32 v = __hip_atomic_fetch_add(&cnt[blockIdx.x], 1u, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
    red[0][0] = (v % (u32)KS == (u32)(KS - 1)) ? 1.f : 0.f;
  }
  __syncthreads();
  if (red[0][0] == 0.f) return;
  if (t < ROWS && row0 + t < N) {
    float v = 0.f;
#pragma unroll
    for (int k = 0; k < KS; ++k)
      v += __hip_atomic_load(&ws[(size_t)(row0 + t) * KS + k],
                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    out[row0 + t] = f2b(v + b2f(res[row0 + t]));
  }
}

void launch_gemv_res_splitk(const u16* W, const u16* x, u16* out,
                            const u16* res, float* ws, u32* cnt, int N,
                            int K, hipStream_t s) {
  // K/2 per slice; pick KB for the half-K
  const int kb = gemv_splitk_kb(K);
  dim3 grid((N + 1) / 2, 2);
#define SPK(KB)                                                             \
  hipLaunchKernelGGL((k_gemv_splitk_res<2, KB, 2>), grid, dim3(256), 0, s,  \
                     W, x, out, res, ws, cnt, N, K)
  if (kb == 1) SPK(1);
  else if (kb == 2) SPK(2);
  else if (kb == 4) SPK(4);
  else SPK(8);
#undef SPK
}

template <int ROWS, int EPI>
static void gemv_dispatch_kb(const u16* W, const u16* x, void* out,
                             const u16* res, const u16* nw, float eps, int N,
                             int K, hipStream_t s) {
  dim3 grid((N + ROWS - 1) / ROWS);
  const int kb = gemv_kb(K);
  if (kb == 0) {
    hipLaunchKernelGGL((k_gemv_stream<ROWS, EPI>), grid, dim3(256), 0, s, W,
                       x, out, res, N, K);
    return;
  }
#define GEMV_KB(KB)                                                        \
  do {                                                                     \
    if (nw)                                                                \
      hipLaunchKernelGGL((k_gemv_reg<ROWS, EPI, true, KB>), grid,          \
                         dim3(256), 0, s, W, x, out, res, nw, eps, N, K);  \
    else                                                                   \
      hipLaunchKernelGGL((k_gemv_reg<ROWS, EPI, false, KB>), grid,         \
                         dim3(256), 0, s, W, x, out, res, nw, eps, N, K);  \
  } while (0)
  if (kb == 2) GEMV_KB(2);
  else if (kb == 4) GEMV_KB(4);
  else GEMV_KB(8);
#undef GEMV_KB
}

void launch_gemv(const u16* W, const u16* x, void* out, const u16* res,
                 const u16* nw, float eps, int N, int K, int epi,
                 hipStream_t s, int rows_override) {
  const int rows = rows_override ? rows_override : gemv_rows_policy(N, K);
#define GEMV_R(R, EPI) gemv_dispatch_kb<R, EPI>(W, x, out, res, nw, eps, N, K, s)
#define GEMV_EPI(EPI)                          \
  do {                                         \
    if (rows >= 8) GEMV_R(8, EPI);             \
    else if (rows == 4) GEMV_R(4, EPI);        \
    else if (rows == 2) GEMV_R(2, EPI);        \
    else GEMV_R(1, EPI);                       \
  } while (0)
  if (epi == 0) GEMV_EPI(0);
  else if (epi == 1) GEMV_EPI(1);
  else GEMV_EPI(2);
#undef GEMV_EPI
#undef GEMV_R
}
void launch_gemv_gateup(const u16* W, const u16* x, u16* out, const u16* nw,
                        float eps, int I, int K, int rows, hipStream_t s) {
  if (K > 16384) return;  // guarded at engine create (K = hidden <= 16384)
  const int kb = gemv_kb(K);
#define GU_KB2(ROWS, KB)                                                    \
  do {                                                                      \
    dim3 grid((I + ROWS - 1) / ROWS);                                       \
    if (nw)                                                                 \
      hipLaunchKernelGGL((k_gemv_gateup<ROWS, true, KB>), grid, dim3(256),  \
                         0, s, W, x, out, nw, eps, I, K);                   \
    else                                                                    \
      hipLaunchKernelGGL((k_gemv_gateup<ROWS, false, KB>), grid, dim3(256), \
                         0, s, W, x, out, nw, eps, I, K);                   \
  } while (0)
#define GU_KB(KB)                                                           \
  do {                                                                      \
    if (rows >= 8) GU_KB2(8, KB);                                           \
    else GU_KB2(4, KB);                                                     \
  } while (0)
  if (kb == 2) GU_KB(2);
  else if (kb == 4) GU_KB(4);
  else GU_KB(8);
#undef GU_KB
#undef GU_KB2
}
void launch_gemv_fp8(const unsigned char* W, const float* sc, const u16* x,
                     void* out, const u16* res, const u16* nw, float eps,
                     int N, int K, int epi, hipStream_t s, NormIO nio,
                     int rows_override) {
  const int nkb = (K + 127) / 128;
  const int rows = rows_override ? rows_override : gemv_fp8_rows_policy(N);
  const int kb = gemv_fp8_kb(K);
#define F8_KB(R, EPI, KB)                                                   \
  do {                                                                      \
    dim3 grid((N + R - 1) / R);                                             \
    if (nw)                                                                 \
      hipLaunchKernelGGL((k_gemv_fp8<R, EPI, true, KB>), grid, dim3(256),   \
                         0, s, W, sc, x, out, res, nw, eps, N, K, nkb,     \
                         nio);                                              \
    else                                                                    \
      hipLaunchKernelGGL((k_gemv_fp8<R, EPI, false, KB>), grid, dim3(256),  \
                         0, s, W, sc, x, out, res, nw, eps, N, K, nkb,      \
                         nio);                                              \
  } while (0)
#define F8_R(R, EPI)                                                        \
  do {                                                                      \
    if (kb == 0) {                                                          \
      dim3 grid((N + R - 1) / R);                                           \
      hipLaunchKernelGGL((k_gemv_fp8_stream<R, EPI>), grid, dim3(256), 0,   \
                         s, W, sc, x, out, res, N, K, nkb, nio);            \
    } else if (kb == 1) F8_KB(R, EPI, 1);                                   \
    else if (kb == 2) F8_KB(R, EPI, 2);                                     \
    else F8_KB(R, EPI, 4);                                                  \
  } while (0)
  if (epi == 0) { if (rows == 8) F8_R(8, 0); else F8_R(4, 0); }
  else if (epi == 1) { if (rows == 8) F8_R(8, 1); else F8_R(4, 1); }
  else { if (rows == 8) F8_R(8, 2); else F8_R(4, 2); }
#undef F8_R
#undef F8_KB
}
void launch_gemv_gateup_fp8(const unsigned char* W, const float* sc,
                            const u16* x, u16* out, const u16* nw, float eps,
                            int I, int K, hipStream_t s, NormIO nio) {
  const int nkb = (K + 127) / 128;
  const int kb = gemv_fp8_kb(K);  // K = hidden <= 16384 (engine create)
  dim3 grid((I + 3) / 4);
#define GU8_KB(KB)                                                          \
  do {                                                                      \
    if (nw)                                                                 \
      hipLaunchKernelGGL((k_gemv_gateup_fp8<4, true, KB>), grid, dim3(256), \
                         0, s, W, sc, x, out, nw, eps, I, K, nkb, nio);     \
    else                                                                    \
      hipLaunchKernelGGL((k_gemv_gateup_fp8<4, false, KB>), grid,           \
                         dim3(256), 0, s, W, sc, x, out, nw, eps, I, K,     \
                         nkb, nio);                                         \
  } while (0)
  if (kb == 1) GU8_KB(1);
  else if (kb == 2) GU8_KB(2);
  else GU8_KB(4);
#undef GU8_KB
}
void launch_dequant_fp8(const unsigned char* W, const float* sc, u16* out,
                        int N, int K, hipStream_t s) {
  const int nkb = (K + 127) / 128;
  hipLaunchKernelGGL(k_dequant_fp8, dim3(4096), dim3(256), 0, s, W, sc, out,
                     N, K, nkb);
}
