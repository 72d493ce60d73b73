#include "kernels_common.h"
#include "kernels.h"


// ---------------------------------------------------------------------------
// Prefill GEMM — MFMA bf16.  C[M,N] = A[M,K] @ W[N,K]^T (+ residual).
// 128x128 tile, BK=64, 256 threads (4 waves as 2x2 of 64x64 sub-tiles),
// v_mfma_f32_16x16x32_bf16, double-buffered LDS filled by
// global_load_lds_dwordx4 with the XOR source-swizzle (rule 21) so the
// fragment ds_read_b128 is bank-conflict-free (guide §5 ladder step 3).
// Row clamp handles M/N tails; requires K % 64 == 0 (all hot-path K are).
// ---------------------------------------------------------------------------
#define GEMM_BM 128
#define GEMM_BN 128
#define GEMM_BK 64

template <int EPI>  // 0: bf16 store, 1: bf16 store + residual add
__global__ __launch_bounds__(256) void k_gemm_bf16(
    const u16* __restrict__ A, const u16* __restrict__ W, u16* __restrict__ C,
    const u16* __restrict__ res, int M, int N, int K) {
  // dynamic-LDS base must be 16-B aligned (guide G17)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  u16* As = reinterpret_cast<u16*>(smem);                       // [2][128][64]
  u16* Bs = reinterpret_cast<u16*>(smem + 2 * GEMM_BM * GEMM_BK * 2);

  // XCD-aware block swizzle (guide T1, bijective variant): contiguous
  // chunks of the grid per XCD so neighbor tiles hit the same per-XCD L2
  int mt, nt;
  {
    const int nwg = gridDim.x * gridDim.y;
    const int orig = blockIdx.x + gridDim.x * blockIdx.y;
    const int q = nwg / 8, rr = nwg % 8;
    const int xcd = orig % 8, idx = orig / 8;
    const int wgid =
        (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + idx;
    mt = wgid % gridDim.x;
    nt = wgid / gridDim.x;
  }
  const int m0 = mt * GEMM_BM;
  const int n0 = nt * GEMM_BN;
  const int t = threadIdx.x;
  const int wid = t / WAVE, lane = t % WAVE;
  const int wr = wid / 2, wc = wid % 2;  // wave's 64x64 quadrant

  // staging geometry: each wave issues 4 glds per 16 KB tile; instruction j
  // of wave w writes LDS rows [(w*4+j)*8, +8) (8 rows x 128 B), lane l ->
  // row sub = l/8, 16-B unit u = l%8, with source column unit u ^ (row & 7).
  auto stage = [&](int buf, int kt) {
    const int ktbase = kt * GEMM_BK;
    u16* as = As + (size_t)buf * GEMM_BM * GEMM_BK;
    u16* bs = Bs + (size_t)buf * GEMM_BN * GEMM_BK;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = (wid * 4 + j) * 8 + lane / 8;
      const int u = (lane % 8) ^ (r & 7);
      // ragged-K tail: clamp the column so the last tile's loads stay in
      // the row (the compute loop zeroes the A fragments beyond K)
      const int kcol = min(ktbase + u * 8, K - 8);
      {  // A tile
        int grow = min(m0 + r, M - 1);
        const u16* src = A + (size_t)grow * K + kcol;
        __builtin_amdgcn_global_load_lds(
            (const __attribute__((address_space(1))) void*)(uintptr_t)src,
            (__attribute__((address_space(3))) void*)(uintptr_t)(
                as + (size_t)(wid * 4 + j) * 8 * GEMM_BK),
            16, 0, 0);
      }
      {  // W tile (B^T)
        int grow = min(n0 + r, N - 1);
        const u16* src = W + (size_t)grow * K + kcol;
        __builtin_amdgcn_global_load_lds(
            (const __attribute__((address_space(1))) void*)(uintptr_t)src,
            (__attribute__((address_space(3))) void*)(uintptr_t)(
                bs + (size_t)(wid * 4 + j) * 8 * GEMM_BK),
            16, 0, 0);
      }
    }
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  // ragged K (K % 64 != 0, K % 8 == 0 contract): the LAST tile's stage
  // clamps its loads into the rows and the A fragments beyond K are
  // zeroed here, so the clamped duplicates contribute exact zeros
  const int ntiles = (K + GEMM_BK - 1) / GEMM_BK;
  const bool ragged = (K % GEMM_BK) != 0;
  stage(0, 0);
  __syncthreads();  // drains the glds (vmcnt(0) implied by the barrier)

  for (int kt = 0; kt < ntiles; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < ntiles) stage(cur ^ 1, kt + 1);
    const u16* as = As + (size_t)cur * GEMM_BM * GEMM_BK;
    const u16* bs = Bs + (size_t)cur * GEMM_BN * GEMM_BK;
    const bool tail = ragged && kt == ntiles - 1;
#pragma unroll
    for (int ks = 0; ks < GEMM_BK / 32; ++ks) {
      bf16x8 af[4], bf[4];
      const int kk = ks * 32 + (lane / 16) * 8;
      const int ku = kk / 8;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int ar = wr * 64 + i * 16 + (lane % 16);
        af[i] = *reinterpret_cast<const bf16x8*>(
            as + (size_t)ar * GEMM_BK + (size_t)(ku ^ (ar & 7)) * 8);
        const int br = wc * 64 + i * 16 + (lane % 16);
        bf[i] = *reinterpret_cast<const bf16x8*>(
            bs + (size_t)br * GEMM_BK + (size_t)(ku ^ (br & 7)) * 8);
      }
      if (tail && kt * GEMM_BK + kk >= K) {
        const bf16x8 zb = {};
#pragma unroll
        for (int i = 0; i < 4; ++i) af[i] = zb;
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              af[i], bf[j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
  }

  // epilogue: C/D map (guide §3): col = lane&15, row = (lane>>4)*4 + reg
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = m0 + wr * 64 + i * 16 + (lane / 16) * 4 + r;
        const int col = n0 + wc * 64 + j * 16 + (lane % 16);
        if (row < M && col < N) {
          float v = acc[i][j][r];
          if (EPI == 1) v += b2f(res[(size_t)row * N + col]);
          C[(size_t)row * N + col] = f2b(v);
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// 256x256 GEMM with counted-vmcnt pipelining (guide §5 T3/T4: the counted
// wait IS the gain — never drain vmcnt(0) in the main loop).
//
// Geometry: BM=BN=256, BK=64, 8 waves (2M x 4N), per-wave 128x64 output
// (8x4 16x16 frags, 128 acc VGPRs).  LDS 128 KB: 2 tile-buffers x
// {A,B} x 2 row-halves x [128][64] bf16, my known-good XOR-unit swizzle.
//
// Schedule (uniform, every phase): stage 2 row-half pieces of tile t+1
// (4 glds/wave) -> asm s_waitcnt vmcnt(4) (retires everything except the 4
// just-issued, so tile t is fully resident) -> raw s_barrier -> 12
// ds_read_b128 + 32 MFMA (one k-step) -> next phase.  Piece issue order per
// wave: (t,A-h0)(t,A-h1) in phase ks=0, (t,B-h0)(t,B-h1) in ks=1, so the
// FIFO count proof holds; buffers alternate by tile parity and a piece is
// overwritten two tiles after its last read (>= 2 barriers apart).
// Requires K % 64 == 0; M/N tails handled by clamped loads + guarded
// stores.  Dispatched only when the grid has >= GEMM256_MIN_BLOCKS tiles.

// ---------------------------------------------------------------------------
// 128x256 GEMM with TWO-TILE lookahead (3 staging buffers, 144 KB LDS).
// The 256^2 kernel's single-tile lookahead (~1 phase of cover) measured
// 38% SQ_WAIT_ANY; staging tile t+2 while computing tile t gives ~2 phases
// of flight per piece.  8 waves as 2(M) x 4(N), per-wave 64x64 output
// (16 acc f32x4).  Pieces per tile: A (128x64 = 16 KB, 2 glds/wave),
// B (256x64 = 32 KB, 4 glds/wave); phase (t,ks0) stages A(t+2), phase
// (t,ks1) stages B(t+2).  FIFO counts: wait vmcnt(8) at ks0 (A(t+1) +
// B(t+1) + A(t+2) outstanding), vmcnt(12) at ks1.
// ---------------------------------------------------------------------------
template <int EPI>
__global__ __launch_bounds__(512) void k_gemm_128x256(
    const u16* __restrict__ A, const u16* __restrict__ W, u16* __restrict__ C,
    const u16* __restrict__ res, int M, int N, int K) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  auto apiece = [&](int buf) -> u16* {
    return reinterpret_cast<u16*>(smem + buf * 16384);
  };
  auto bpiece = [&](int buf) -> u16* {
    return reinterpret_cast<u16*>(smem + 3 * 16384 + buf * 32768);
  };
  int mt, nt;
  {
    const int nwg = gridDim.x * gridDim.y;
    const int orig = blockIdx.x + gridDim.x * blockIdx.y;
    const int q = nwg / 8, rr = nwg % 8;
    const int xcd = orig % 8, idx = orig / 8;
    const int wgid =
        (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + idx;
    mt = wgid % gridDim.x;
    nt = wgid / gridDim.x;
  }
  const int m0 = mt * 128, n0 = nt * 256;
  const int t = threadIdx.x;
  const int w = t / WAVE, lane = t % WAVE;
  const int wm = w >> 2, wn = w & 3;  // 2 x 4 waves, 64x64 each

  auto stage_a = [&](int tau) {
    u16* dst = apiece(tau % 3);
    const int kt = tau * 64;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int rloc = (w * 2 + j) * 8 + lane / 8;  // 0..127
      const int grow = min(m0 + rloc, M - 1);
      const int u = (lane % 8) ^ (rloc & 7);
      const u16* src = A + (size_t)grow * K + kt + u * 8;
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) void*)(uintptr_t)src,
          (__attribute__((address_space(3))) void*)(uintptr_t)(
              dst + (size_t)(w * 2 + j) * 8 * 64),
          16, 0, 0);
    }
  };
  auto stage_b = [&](int tau) {
    u16* dst = bpiece(tau % 3);
    const int kt = tau * 64;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int rloc = (w * 4 + j) * 8 + lane / 8;  // 0..255
      const int grow = min(n0 + rloc, N - 1);
      const int u = (lane % 8) ^ (rloc & 7);
      const u16* src = W + (size_t)grow * K + kt + u * 8;
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) void*)(uintptr_t)src,
          (__attribute__((address_space(3))) void*)(uintptr_t)(
              dst + (size_t)(w * 4 + j) * 8 * 64),
          16, 0, 0);
    }
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  const int NT = K / 64;
  stage_a(0);
  stage_b(0);
  if (NT > 1) {
    stage_a(1);
    stage_b(1);
  }
  for (int tau = 0; tau < NT; ++tau) {
    const u16* ap = apiece(tau % 3);
    const u16* bp = bpiece(tau % 3);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      if (ks == 0) {
        if (tau + 2 < NT) {
          stage_a(tau + 2);
          asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        } else {
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
      } else {
        if (tau + 2 < NT) {
          stage_b(tau + 2);
          asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
        }
        // tail tiles: everything needed was already drained at ks0
      }
      __builtin_amdgcn_s_barrier();
      bf16x8 af[4], bf[4];
      const int u = ks * 4 + (lane / 16);
#pragma unroll
      for (int mi = 0; mi < 4; ++mi) {
        const int r = wm * 64 + mi * 16 + (lane % 16);
        af[mi] = *reinterpret_cast<const bf16x8*>(
            ap + (size_t)r * 64 + (size_t)(u ^ (r & 7)) * 8);
      }
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        const int r = wn * 64 + ni * 16 + (lane % 16);
        bf[ni] = *reinterpret_cast<const bf16x8*>(
            bp + (size_t)r * 64 + (size_t)(u ^ (r & 7)) * 8);
      }
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              af[mi], bf[ni], acc[mi][ni], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
      __builtin_amdgcn_s_barrier();
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = m0 + wm * 64 + mi * 16 + (lane / 16) * 4 + r;
        const int col = n0 + wn * 64 + ni * 16 + (lane % 16);
        if (row < M && col < N) {
          float v = acc[mi][ni][r];
          if (EPI == 1) v += b2f(res[(size_t)row * N + col]);
          C[(size_t)row * N + col] = f2b(v);
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
template <int EPI>
__global__ __launch_bounds__(512) void k_gemm_256(
    const u16* __restrict__ A, const u16* __restrict__ W, u16* __restrict__ C,
    const u16* __restrict__ res, int M, int N, int K) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // piece (op, buf, half): As op=0 at 0, Bs op=1 at 64 KB
  auto piece = [&](int op, int buf, int half) -> u16* {
    return reinterpret_cast<u16*>(smem + op * 65536 +
                                  (buf * 2 + half) * 16384);
  };
  // XCD-aware bijective block swizzle (T1)
  int mt, nt;
  {
    const int nwg = gridDim.x * gridDim.y;
    const int orig = blockIdx.x + gridDim.x * blockIdx.y;
    const int q = nwg / 8, rr = nwg % 8;
    const int xcd = orig % 8, idx = orig / 8;
    const int wgid =
        (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + idx;
    mt = wgid % gridDim.x;
    nt = wgid / gridDim.x;
  }
  const int m0 = mt * 256, n0 = nt * 256;
  const int t = threadIdx.x;
  const int w = t / WAVE, lane = t % WAVE;
  const int wm = w >> 2, wn = w & 3;

  // stage the two row-half pieces of ONE operand for tile tau
  auto stage_op = [&](int op, int tau) {
    const u16* G = op == 0 ? A : W;
    const int rows = op == 0 ? M : N;
    const int base = op == 0 ? m0 : n0;
    const int buf = tau & 1;
    const int kt = tau * 64;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      u16* dst = piece(op, buf, half);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int rloc = (w * 2 + j) * 8 + lane / 8;   // 0..127
        const int grow = min(base + half * 128 + rloc, rows - 1);
        const int u = (lane % 8) ^ (rloc & 7);
        const u16* src = G + (size_t)grow * K + kt + u * 8;
        __builtin_amdgcn_global_load_lds(
            (const __attribute__((address_space(1))) void*)(uintptr_t)src,
            (__attribute__((address_space(3))) void*)(uintptr_t)(
                dst + (size_t)(w * 2 + j) * 8 * 64),
            16, 0, 0);
      }
    }
  };

  f32x4 acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  const int NT = K / 64;
  // prologue: tile 0, both operands (8 glds/wave in flight)
  stage_op(0, 0);
  stage_op(1, 0);
  for (int tau = 0; tau < NT; ++tau) {
    const int buf = tau & 1;
    const u16* ap = piece(0, buf, wm);               // this wave's A half
    const u16* bp = piece(1, buf, wn >> 1);          // this wave's B half
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      if (tau + 1 < NT) stage_op(ks, tau + 1);       // ks0: A, ks1: B
      if (ks == 0) {
        // tile tau fully resident once all but the 4 just-issued retire;
        // ks1 needs NO wait (tau drained at ks0, and waiting would force
        // the just-staged tau+1 pieces to land — serializing the
        // prefetch instead of letting it ride through ks1's compute)
        if (tau + 1 < NT)
          asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      __builtin_amdgcn_s_barrier();
      bf16x8 af[8], bf[4];
      const int u = ks * 4 + (lane / 16);            // 16-B unit 0..7
#pragma unroll
      for (int mi = 0; mi < 8; ++mi) {
        const int r = mi * 16 + (lane % 16);
        af[mi] = *reinterpret_cast<const bf16x8*>(
            ap + (size_t)r * 64 + (size_t)(u ^ (r & 7)) * 8);
      }
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        const int r = (wn & 1) * 64 + ni * 16 + (lane % 16);
        bf[ni] = *reinterpret_cast<const bf16x8*>(
            bp + (size_t)r * 64 + (size_t)(u ^ (r & 7)) * 8);
      }
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int mi = 0; mi < 8; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              af[mi], bf[ni], acc[mi][ni], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
      __builtin_amdgcn_s_barrier();
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // quiesce before exit

  // epilogue (C/D map: col = lane&15, row = (lane>>4)*4 + reg)
#pragma unroll
  for (int mi = 0; mi < 8; ++mi) {
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = m0 + wm * 128 + mi * 16 + (lane / 16) * 4 + r;
        const int col = n0 + wn * 64 + ni * 16 + (lane % 16);
        if (row < M && col < N) {
          float v = acc[mi][ni][r];
          if (EPI == 1) v += b2f(res[(size_t)row * N + col]);
          C[(size_t)row * N + col] = f2b(v);
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// 256^2 fine-phase variant (guide §5.5 8-phase template direction): the
// K-tile's 64 MFMA are split into FOUR 16-MFMA phases (mi-half x K-half
// quadrants), each phase staging one (op, row-half) piece of the next tile
// (2 glds) so the global traffic interleaves 1:1 with compute, and the
// per-tile wait is a single counted vmcnt(2) (the two loads just issued)
// instead of two vmcnt(4)s.  B fragments are register-reused across the
// two mi-half phases of a K-half (af[4]+bf[4] live = 32 VGPRs vs 48).
// "The per-phase interleave is the lever" — coarse phase splits measured
// -7..-27% in the guide's ablation.
// ---------------------------------------------------------------------------
template <int EPI>
__global__ __launch_bounds__(512) void k_gemm_256p(
    const u16* __restrict__ A, const u16* __restrict__ W, u16* __restrict__ C,
    const u16* __restrict__ res, int M, int N, int K) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  auto piece = [&](int op, int buf, int half) -> u16* {
    return reinterpret_cast<u16*>(smem + op * 65536 +
                                  (buf * 2 + half) * 16384);
  };
  int mt, nt;
  {
    const int nwg = gridDim.x * gridDim.y;
    const int orig = blockIdx.x + gridDim.x * blockIdx.y;
    const int q = nwg / 8, rr = nwg % 8;
    const int xcd = orig % 8, idx = orig / 8;
    const int wgid =
        (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + idx;
    mt = wgid % gridDim.x;
    nt = wgid / gridDim.x;
  }
  const int m0 = mt * 256, n0 = nt * 256;
  const int t = threadIdx.x;
  const int w = t / WAVE, lane = t % WAVE;
  const int wm = w >> 2, wn = w & 3;

  // stage ONE (op, half) piece of tile tau: 2 glds per wave
  auto stage_piece = [&](int op, int half, int tau) {
    const u16* G = op == 0 ? A : W;
    const int rows = op == 0 ? M : N;
    const int base = op == 0 ? m0 : n0;
    const int buf = tau & 1;
    const int kt = tau * 64;
    u16* dst = piece(op, buf, half);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int rloc = (w * 2 + j) * 8 + lane / 8;  // 0..127
      const int grow = min(base + half * 128 + rloc, rows - 1);
      const int u = (lane % 8) ^ (rloc & 7);
      const u16* src = G + (size_t)grow * K + kt + u * 8;
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) void*)(uintptr_t)src,
          (__attribute__((address_space(3))) void*)(uintptr_t)(
              dst + (size_t)(w * 2 + j) * 8 * 64),
          16, 0, 0);
    }
  };

  f32x4 acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  const int NT = K / 64;
  // prologue: all four pieces of tile 0
  stage_piece(0, 0, 0);
  stage_piece(0, 1, 0);
  stage_piece(1, 0, 0);
  stage_piece(1, 1, 0);
  for (int tau = 0; tau < NT; ++tau) {
    const int buf = tau & 1;
    const u16* ap = piece(0, buf, wm);
    const u16* bp = piece(1, buf, wn >> 1);
    bf16x8 bfr[4];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int p = ks * 2 + q;
        if (tau + 1 < NT) stage_piece(p >> 1, p & 1, tau + 1);
        if (p == 0) {
          // tile tau resident once everything but the piece just issued
          // has retired (per-wave FIFO vmcnt)
          if (tau + 1 < NT)
            asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
          else
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __builtin_amdgcn_s_barrier();
        const int u = ks * 4 + (lane / 16);  // 16-B unit 0..7
        bf16x8 af[4];
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) {
          const int r = (q * 4 + mi) * 16 + (lane % 16);
          af[mi] = *reinterpret_cast<const bf16x8*>(
              ap + (size_t)r * 64 + (size_t)(u ^ (r & 7)) * 8);
        }
        if (q == 0) {
#pragma unroll
          for (int ni = 0; ni < 4; ++ni) {
            const int r = (wn & 1) * 64 + ni * 16 + (lane % 16);
            bfr[ni] = *reinterpret_cast<const bf16x8*>(
                bp + (size_t)r * 64 + (size_t)(u ^ (r & 7)) * 8);
          }
        }
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
          for (int ni = 0; ni < 4; ++ni)
            acc[q * 4 + mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                af[mi], bfr[ni], acc[q * 4 + mi][ni], 0, 0, 0);
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_s_barrier();
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

#pragma unroll
  for (int mi = 0; mi < 8; ++mi) {
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = m0 + wm * 128 + mi * 16 + (lane / 16) * 4 + r;
        const int col = n0 + wn * 64 + ni * 16 + (lane % 16);
        if (row < M && col < N) {
          float v = acc[mi][ni][r];
          if (EPI == 1) v += b2f(res[(size_t)row * N + col]);
          C[(size_t)row * N + col] = f2b(v);
        }
      }
    }
  }
}

GemmPolicy gemm_policy(int M, int N, int K) {
  // hipBLASLt first for these plain GEMMs (CAKE_GEMM_LIB=0 restores the
  // hand-written kernels; they also remain the fallback for any shape the
  // library heuristic rejects)
  static const bool use_lib = [] {
    const char* v = getenv("CAKE_GEMM_LIB");
    return !v || atoi(v) != 0;
  }();
  // measured per-shape split (profiles/r02_NOTES.md, in-context event
  // stats): the library wins every prefill shape EXCEPT the ~1-WG/CU
  // short-K o-projection class (8B o at M=2048: 2.77 ms ours vs 3.25 ms
  // lib per prefill), which stays on the hand-written kernels.  The
  // bound is deliberately tight — on the SMALL grids below it (0.6B
  // shapes) the library is ~2x faster than our 128^2 baseline
  const long g128x256 = (long)((M + 127) / 128) * ((N + 255) / 256);
  const bool ours_wins =
      K <= 4096 && M >= 1024 && g128x256 >= 200 && g128x256 <= 256;
  GemmPolicy p;
  p.lib_first = use_lib && !ours_wins;
  // variant select: 0 = 128^2 baseline, 1 = 256^2 counted-vmcnt,
  // 2 = 128x256 3-buffer two-tile lookahead, 3 = 256^2 fine-phase
  // (CAKE_GEMM_VAR overrides)
  static const int var = [] {
    const char* v = getenv("CAKE_GEMM_VAR");
    if (v) return atoi(v);
    const char* o = getenv("CAKE_GEMM256");  // legacy knob
    if (o && atoi(o) == 0) return 0;
    return 1;
  }();
  const int mt128 = (M + 127) / 128, nt256 = (N + 255) / 256;
  const int mt256 = (M + 255) / 256;
  // mixed dispatch (default): shapes whose 256^2 grid is under the ~200-
  // block occupancy floor but whose 128x256 grid is not (e.g. the 8B
  // prefill qkv/o/down at M=2048) take the 128x256 two-tile-lookahead
  // kernel instead of falling all the way to the 128^2 baseline
  const bool mixed_128x256 =
      var == 1 && (long)mt256 * nt256 < 200 &&
      (long)mt128 * nt256 >= 200 && K % 64 == 0 &&
      !(getenv("CAKE_GEMM_MIXED") && atoi(getenv("CAKE_GEMM_MIXED")) == 0);
  if ((var == 2 || mixed_128x256) && (long)mt128 * nt256 >= 200 &&
      K % 64 == 0)
    p.variant = GEMM_V128X256;
  else if (var == 3 && (long)mt256 * nt256 >= 200 && K % 64 == 0)
    p.variant = GEMM_V256P;
  else if (var >= 1 && (long)mt256 * nt256 >= 200 && K % 64 == 0)
    p.variant = GEMM_V256;
  else
    p.variant = GEMM_V128;
  return p;
}

bool launch_gemm_variant(const u16* A, const u16* W, u16* C, const u16* res,
                         int M, int N, int K, int epi, int variant,
                         hipStream_t s) {
  if (variant == GEMM_VLIB)
    return launch_gemm_lib(A, W, C, res, M, N, K, epi, s);
  const int mt128 = (M + 127) / 128, nt256 = (N + 255) / 256;
  if (variant == GEMM_V128X256) {
    static bool attr2 = false;
    if (!attr2) {
      hipFuncSetAttribute((const void*)&k_gemm_128x256<0>,
                          hipFuncAttributeMaxDynamicSharedMemorySize, 147456);
      hipFuncSetAttribute((const void*)&k_gemm_128x256<1>,
                          hipFuncAttributeMaxDynamicSharedMemorySize, 147456);
      attr2 = true;
    }
    dim3 grid(mt128, nt256);
    if (epi == 0)
      hipLaunchKernelGGL(k_gemm_128x256<0>, grid, dim3(512), 147456, s, A, W,
                         C, res, M, N, K);
    else
      hipLaunchKernelGGL(k_gemm_128x256<1>, grid, dim3(512), 147456, s, A, W,
                         C, res, M, N, K);
    return true;
  }
  const int mt = (M + 255) / 256, nt = (N + 255) / 256;
  if (variant == GEMM_V256P) {
    static bool attr3 = false;
    if (!attr3) {
      hipFuncSetAttribute((const void*)&k_gemm_256p<0>,
                          hipFuncAttributeMaxDynamicSharedMemorySize, 131072);
      hipFuncSetAttribute((const void*)&k_gemm_256p<1>,
                          hipFuncAttributeMaxDynamicSharedMemorySize, 131072);
      attr3 = true;
    }
    dim3 grid(mt, nt);
    if (epi == 0)
      hipLaunchKernelGGL(k_gemm_256p<0>, grid, dim3(512), 131072, s, A, W, C,
                         res, M, N, K);
    else
      hipLaunchKernelGGL(k_gemm_256p<1>, grid, dim3(512), 131072, s, A, W, C,
                         res, M, N, K);
    return true;
  }
  if (variant == GEMM_V256) {
    static bool attr_set = false;
    if (!attr_set) {
      hipFuncSetAttribute((const void*)&k_gemm_256<0>,
                          hipFuncAttributeMaxDynamicSharedMemorySize, 131072);
      hipFuncSetAttribute((const void*)&k_gemm_256<1>,
                          hipFuncAttributeMaxDynamicSharedMemorySize, 131072);
      attr_set = true;
    }
    dim3 grid(mt, nt);
    if (epi == 0)
      hipLaunchKernelGGL(k_gemm_256<0>, grid, dim3(512), 131072, s, A, W, C,
                         res, M, N, K);
    else
      hipLaunchKernelGGL(k_gemm_256<1>, grid, dim3(512), 131072, s, A, W, C,
                         res, M, N, K);
    return true;
  }
  dim3 grid((M + GEMM_BM - 1) / GEMM_BM, (N + GEMM_BN - 1) / GEMM_BN);
  size_t lds = 2 * (size_t)(GEMM_BM + GEMM_BN) * GEMM_BK * 2;
  if (epi == 0)
    hipLaunchKernelGGL(k_gemm_bf16<0>, grid, dim3(256), lds, s, A, W, C, res,
                       M, N, K);
  else
    hipLaunchKernelGGL(k_gemm_bf16<1>, grid, dim3(256), lds, s, A, W, C, res,
                       M, N, K);
  return true;
}

void launch_gemm(const u16* A, const u16* W, u16* C, const u16* res, int M,
                 int N, int K, int epi, hipStream_t s) {
  const GemmPolicy p = gemm_policy(M, N, K);
  if (p.lib_first && launch_gemm_variant(A, W, C, res, M, N, K, epi,
                                         GEMM_VLIB, s))
    return;
  launch_gemm_variant(A, W, C, res, M, N, K, epi, p.variant, s);
}
