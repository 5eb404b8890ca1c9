// Weight-gradient ("dW") kernels: dW[N x K] += X^T Y over the points, for every layer of a backward.  The host side that
// plans and launches them is dw.hip; the primitives they share with the row GEMMs and the fused sweeps (x3 / x2h operand
// splits, MFMA terms, the maxima of the x2h scales) stay in gemm.hip.h.
#pragma once
#include "gemm.hip.h"

namespace rnb {

// ---- dW[N x K] += X1^T Y1 (+ X2^T Y2), reduction over the M points, split-K over workgroups ---------
//   X* [M x N] (ldx), Y* [M x K] (ldy); rows >= M are masked.  1-D grid over (job, tile, split).
//   Partial tiles are accumulated into dW with float atomics (dW zero-initialised by the caller);
//   colsum(X) of pair `bias_pair` over the same rows is added to db when db != nullptr (by the
//   tile_k == 0 blocks).
struct DwPair {
  const float* X;
  int ldx;
  const float* Y;
  int ldy;
  // x2h form of the 256-row kernel (gemm_dw_x3_kernel<., 2>): which operand is the loss adjoint (0: X, 1: Y; the other one
  // is saved forward state of known range) and where its producer left max |.| over the real rows (float bits)
  int adj = 0;
  const unsigned* amax = nullptr;
  // ... and where the forward left max |.| of the OTHER operand (saved state: PointBufs::smax), or nullptr: the fixed 2^6
  const unsigned* smax = nullptr;
  // gemm_dw_x3_kernel only: one word per 64-point tile, 1 = the tile's X rows were not written and stand for exact zeros (the
  // albedo backward's zero-tile path, color_h2.hip): the tile's points are skipped, loads and MFMAs alike.  nullptr: none
  const unsigned* dead = nullptr;
  long long dead_stride = 0;   // (tile t's word is dead[t * dead_stride]: PointBufs::alb_dead)
  const unsigned* any_dead = nullptr;   // with `dead`: one word, 0 = no tile of the launch is dead (PointBufs::amax, AMAX_ANY_DEAD)
};

template <bool GUARD, int KT>
__device__ inline void dw_main_loop(const DwPair& p, int m_begin, int m_end, int N, int K, int n_blk, int k_blk,
                                    int wm, int wn, unsigned mask, bool do_bias, double& bsum,
                                    float* __restrict__ Xs, float* __restrict__ Ys, v16f (&acc)[2][KT / 64]) {
  const int tid = threadIdx.x, lane = tid & 63;
  vf4 rx[4], ry[KT / 32];
  load_kmajor<128, GUARD>(p.X, p.ldx, m_begin, n_blk, m_end, N, tid, rx);
  load_kmajor<KT, GUARD>(p.Y, p.ldy, m_begin, k_blk, m_end, K, tid, ry);
  for (int m0 = m_begin; m0 < m_end; m0 += BK) {
    store_kmajor<128>(Xs, tid, rx);
    store_kmajor<KT>(Ys, tid, ry);
    lds_barrier();
    if (m0 + BK < m_end) {
      load_kmajor<128, GUARD>(p.X, p.ldx, m0 + BK, n_blk, m_end, N, tid, rx);
      load_kmajor<KT, GUARD>(p.Y, p.ldy, m0 + BK, k_blk, m_end, K, tid, ry);
    }
    if (do_bias) {
#pragma unroll 8
      for (int kk = 0; kk < BK; ++kk) bsum += (double)Xs[kk * 128 + tid];
    }
    mma_step<true, 128, true, KT, KT / 64, GUARD>(Xs, Ys, wm * 64, wn * (KT / 2), lane, mask, acc);
    lds_barrier();
  }
}

// One dW job = one weight matrix; a launch carries a group of jobs so that the atomic tail of one matrix
// overlaps the main loop of the next (a single 256x256 job is ONE resident wave of workgroups: all of them
// would reach their atomics together).  block_end = exclusive prefix sum of the jobs' block counts, each a
// multiple of 8 when splits is (keeps the XCD decode below valid inside the group).
struct DwJob {
  DwPair p1, p2;
  float* dW;
  float* db;
  // RNB_VARIANT_DETERMINISTIC: per-split partial tiles [splits][N][lddw] / column sums [splits][N] written with plain
  // stores (zero-initialised by the caller) and summed in split order by dw_reduce_kernel; nullptr: fp32 atomics
  float* part;
  float* partb;
  int npairs, N, K, lddw, bias_pair, splits, rows_per_split, block_end;
};
struct DwGroup {   // (kMaxDwJobs, kMaxDwExtra: dw_plan.h)
  DwJob job[kMaxDwJobs + kMaxDwExtra];
  int njobs, M;
};

// GUARD (host: N % 128 || K % KT || M % 32) as for gemm_rows_kernel, and the width KT (128 or 64) of the
// output tile along K: all jobs of a group share both.  KT = 64 keeps all four waves busy on narrow or ragged
// K (the PE-input layer has K = 64, the albedo net's first layer K = 320).
template <bool GUARD, int KT>
__global__ __launch_bounds__(256, 3) void gemm_dw_kernel(const DwGroup g) {
  constexpr int TN = KT / 64;
  __shared__ __attribute__((aligned(16))) float smem[BK * 128 + BK * KT];
  float* Xs = smem;
  float* Ys = smem + BK * 128;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = wave_id();
  const int wm = wave >> 1, wn = wave & 1;
  int ji = 0, begin = 0;
  for (int i = 0; i + 1 < g.njobs; ++i)
    if ((int)blockIdx.x >= g.job[i].block_end) { ji = i + 1; begin = g.job[i].block_end; }
  const DwJob& J = g.job[ji];
  const int blk = (int)blockIdx.x - begin;
  const int M = g.M, N = J.N, K = J.K, splits = J.splits;
  float* __restrict__ dW = J.dW;
  float* __restrict__ db = J.db;
  // Blocks of a job: tiles_n * tiles_k * splits.  Workgroups are dealt round-robin over the 8 XCDs
  // (blocks b and b+8 share an L2), so the tiles of one point-split are placed on ONE XCD in consecutive
  // dispatch slots: the X / Y chunks they share are then served by that XCD's L2 instead of being fetched
  // once per tile.  Pure placement heuristic: any mapping is correct.
  const int tiles_n = (N + 127) / 128, tiles_k = (K + KT - 1) / KT;
  const int nt = tiles_n * tiles_k;
  if (blk >= nt * splits) return;   // padding blocks that align the next job to 8
  int tile, split;
  if (splits % 8 == 0) {
    const int xcd = blk & 7, j = blk >> 3;
    tile = j % nt;
    split = (j / nt) * 8 + xcd;
  } else {
    tile = blk % nt;
    split = blk / nt;
  }
  const int tile_n = tile % tiles_n, tile_k = tile / tiles_n;
  const int n_blk = tile_n * 128, k_blk = tile_k * KT;
  const int m_begin = split * J.rows_per_split;
  const int m_end = min(M, m_begin + J.rows_per_split);
  unsigned mask = 0;
#pragma unroll
  for (int tj = 0; tj < TN; ++tj)
    if (k_blk + wn * (KT / 2) + tj * 32 < K) mask |= 1u << tj;

  v16f acc[2][TN];
  zero_acc<TN>(acc);
  double bsum = 0.0;   // bias gradients are long signed sums: keep the per-block partial in fp64
  const bool bias_blk = (db != nullptr) && tile_k == 0 && tid < 128 && (n_blk + tid < N);

  if (m_begin < m_end) {
    for (int pi = 0; pi < J.npairs; ++pi) {
      const DwPair p = pi == 0 ? J.p1 : J.p2;
      const bool do_bias = bias_blk && pi == J.bias_pair;
      dw_main_loop<GUARD, KT>(p, m_begin, m_end, N, K, n_blk, k_blk, wm, wn, mask, do_bias, bsum, Xs, Ys, acc);
    }
  }
  // atomics: each register of a 32x32 accumulator is two 128-byte row segments per wave instruction
  const int lddw = J.lddw;
  float* __restrict__ pdst = J.part ? J.part + (size_t)split * N * lddw : nullptr;
#pragma unroll
  for (int tj = 0; tj < TN; ++tj) {
    if (!((mask >> tj) & 1u)) continue;
    const int col = k_blk + wn * (KT / 2) + tj * 32 + (lane & 31);
#pragma unroll
    for (int ti = 0; ti < 2; ++ti) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = n_blk + wm * 64 + acc_row(ti, r, lane);
        if (row < N) {
          if (pdst) pdst[(size_t)row * lddw + col] = acc[ti][tj][r];
          else atomicAdd(dW + (size_t)row * lddw + col, acc[ti][tj][r]);
        }
      }
    }
  }
  if (bias_blk) {
    if (J.partb) J.partb[(size_t)split * N + n_blk + tid] = (float)bsum;
    else atomicAdd(db + n_blk + tid, (float)bsum);
  }
}

// ---- dW without LDS ----------------------------------------------------------------------------------
// Both operands of dW = X^T Y are point-major in memory, and v_mfma_f32_32x32x2_f32 wants exactly that: lane
// (i, h) supplies A[row i][k = h] and B[k = h][col i], i.e. for a pair of consecutive points the two lane
// halves read the two rows X[m + h][...] — a coalesced global load IS the fragment.  No staging, no
// barriers: the four waves of a workgroup (2 x 2 sub-tiles of 64 x KT/2) run independently and only share
// L1/L2 lines.  X comes in as 8-byte loads (lane i holds columns 2i, 2i+1 -> the wave's two row tiles are
// the even and the odd rows of its 64-row band), Y as 4-byte loads (columns i and 32 + i), so a pair of
// points costs 1 + TN loads for 2 * TN MFMAs.  Loads run two 16-point chunks ahead in a 3-slot register
// ring (<= 63 in flight per wave).  Exact shapes only: N % 128 == 0, K % KT == 0, point ranges % 16 == 0.
template <int KT, int OCC>
__global__ __launch_bounds__(256, OCC) void gemm_dw_direct_kernel(const DwGroup g) {
  constexpr int TN = KT / 64;
  constexpr int CH = 8;   // point pairs per chunk
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = wave_id();
  const int wm = wave >> 1, wn = wave & 1;
  int ji = 0, begin = 0;
  for (int q = 0; q + 1 < g.njobs; ++q)
    if ((int)blockIdx.x >= g.job[q].block_end) { ji = q + 1; begin = g.job[q].block_end; }
  const DwJob& J = g.job[ji];
  const int blk = (int)blockIdx.x - begin;
  const int M = g.M, N = J.N, K = J.K, splits = J.splits;
  const int tiles_n = N / 128, tiles_k = K / KT;
  const int nt = tiles_n * tiles_k;
  if (blk >= nt * splits) return;   // padding blocks that align the next job to 8
  int tile, split;
  if (splits % 8 == 0) {            // XCD-aware placement, see gemm_dw_kernel
    const int xcd = blk & 7, j = blk >> 3;
    tile = j % nt;
    split = (j / nt) * 8 + xcd;
  } else {
    tile = blk % nt;
    split = blk / nt;
  }
  const int tile_n = tile % tiles_n, tile_k = tile / tiles_n;
  const int m_begin = split * J.rows_per_split;
  const int m_end = min(M, m_begin + J.rows_per_split);
  if (m_begin >= m_end) return;
  const int i = lane & 31, h = lane >> 5;
  const int n_w = tile_n * 128 + wm * 64;          // first row (of dW) of this wave
  const int k_w = tile_k * KT + wn * (KT / 2);     // first column
  const int nch = (m_end - m_begin) / (2 * CH);
  const bool bias_wave = J.db != nullptr && tile_k == 0 && wn == 0;

  v16f acc[2][TN];
  zero_acc<TN>(acc);
  double bs0 = 0.0, bs1 = 0.0;   // column sums of X (bias gradient), fp64 partials

  for (int pi = 0; pi < J.npairs; ++pi) {
    const DwPair p = pi == 0 ? J.p1 : J.p2;
    const bool do_bias = bias_wave && pi == J.bias_pair;
    const unsigned xrow = (unsigned)p.ldx * 4u, yrow = (unsigned)p.ldy * 4u;   // row pitch in bytes
    const BufRsrc rx = tile_rsrc(p.X + (size_t)m_begin * p.ldx, (unsigned)(m_end - m_begin) * xrow);
    const BufRsrc ry = tile_rsrc(p.Y + (size_t)m_begin * p.ldy, (unsigned)(m_end - m_begin) * yrow);
    const unsigned vx = (unsigned)h * xrow + (unsigned)(n_w + 2 * i) * 4u;
    const unsigned vy = (unsigned)h * yrow + (unsigned)(k_w + i) * 4u;
    vf2 a[3][CH];
    float b[3][CH][TN];
#define RNB_DW_LOAD(slot, chunk)                                                     \
    {                                                                                  \
      const int c_ = min((chunk), nch - 1);                                            \
      const unsigned sx = (unsigned)c_ * (2 * CH) * xrow, sy = (unsigned)c_ * (2 * CH) * yrow; \
      _Pragma("unroll") for (int q = 0; q < CH; ++q) {                                 \
        a[slot][q] = bload2(rx, vx, sx + (unsigned)(2 * q) * xrow);                    \
        _Pragma("unroll") for (int tj = 0; tj < TN; ++tj)                              \
          b[slot][q][tj] = bload(ry, vy + (unsigned)tj * 128u, sy + (unsigned)(2 * q) * yrow); \
      }                                                                                \
    }
#define RNB_DW_MMA(slot)                                                               \
    {                                                                                  \
      _Pragma("unroll") for (int q = 0; q < CH; ++q) {                                 \
        _Pragma("unroll") for (int tj = 0; tj < TN; ++tj) {                            \
          acc[0][tj] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[slot][q].x, b[slot][q][tj], acc[0][tj], 0, 0, 0); \
          acc[1][tj] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[slot][q].y, b[slot][q][tj], acc[1][tj], 0, 0, 0); \
        }                                                                              \
      }                                                                                \
      if (do_bias) {   /* 16 points in fp32, then into the fp64 partial */                 \
        float t0 = 0.f, t1 = 0.f;                                                      \
        _Pragma("unroll") for (int q = 0; q < CH; ++q) { t0 += a[slot][q].x; t1 += a[slot][q].y; } \
        bs0 += (double)t0;                                                             \
        bs1 += (double)t1;                                                             \
      }                                                                                \
    }
    RNB_DW_LOAD(0, 0)
    RNB_DW_LOAD(1, 1)
    for (int c = 0; c < nch; c += 3) {
      RNB_DW_LOAD(2, c + 2)
      __builtin_amdgcn_sched_barrier(0);
      RNB_DW_MMA(0)
      __builtin_amdgcn_sched_barrier(0);
      RNB_DW_LOAD(0, c + 3)
      __builtin_amdgcn_sched_barrier(0);
      if (c + 1 < nch) RNB_DW_MMA(1)
      __builtin_amdgcn_sched_barrier(0);
      RNB_DW_LOAD(1, c + 4)
      __builtin_amdgcn_sched_barrier(0);
      if (c + 2 < nch) RNB_DW_MMA(2)
      __builtin_amdgcn_sched_barrier(0);
    }
#undef RNB_DW_LOAD
#undef RNB_DW_MMA
  }
  // atomics: accumulator (ti, tj, r) of lane (i, h) is dW[n_w + 2 * rho + ti][k_w + 32 * tj + i],
  // rho = (r & 3) + 8 * (r >> 2) + 4 * h
  float* __restrict__ dW = J.dW;
  const int lddw = J.lddw;
  float* __restrict__ pdst = J.part ? J.part + (size_t)split * N * lddw : nullptr;
#pragma unroll
  for (int tj = 0; tj < TN; ++tj) {
    const int col = k_w + tj * 32 + i;
#pragma unroll
    for (int ti = 0; ti < 2; ++ti) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = n_w + 2 * ((r & 3) + 8 * (r >> 2) + 4 * h) + ti;
        if (pdst) pdst[(size_t)row * lddw + col] = acc[ti][tj][r];
        else atomicAdd(dW + (size_t)row * lddw + col, acc[ti][tj][r]);
      }
    }
  }
  if (bias_wave) {
    bs0 += __shfl_xor(bs0, 32, 64);
    bs1 += __shfl_xor(bs1, 32, 64);
    if (h == 0) {
      if (J.partb) {
        J.partb[(size_t)split * N + n_w + 2 * i] = (float)bs0;
        J.partb[(size_t)split * N + n_w + 2 * i + 1] = (float)bs1;
      } else {
        atomicAdd(J.db + n_w + 2 * i, (float)bs0);
        atomicAdd(J.db + n_w + 2 * i + 1, (float)bs1);
      }
    }
  }
}

// RNB_VARIANT_DETERMINISTIC: dW = sum over splits (in split order, fp64 running sum) of the partial tiles; grid =
// (blocks over N * lddw elements, job).
template <int DUMMY>
__global__ __launch_bounds__(256) void dw_reduce_kernel(const DwGroup g) {
  const DwJob& J = g.job[blockIdx.y];
  // slabs [split][N][K] (K == lddw for whole-matrix jobs; a column range of a wider matrix has K < lddw)
  const size_t n = (size_t)J.N * J.K;
  const bool dense = J.K == J.lddw;
  if (J.splits > 64) {
    // many small slabs (the per-tile column sums of the fused albedo backward: a thousand slabs of a few hundred elements):
    // 16 elements x 16 split phases per workgroup pass, each thread a fixed subsequence of the slabs, the 16 phases summed in
    // phase order — as reproducible as one chain, 256 loads in flight per workgroup instead of one per element.  The bias
    // slabs ride as elements n .. n + N.
    __shared__ double red[16][17];
    const size_t ntot = n + ((J.db != nullptr && J.partb != nullptr) ? (size_t)J.N : 0);
    const int e = threadIdx.x & 15, ph = threadIdx.x >> 4;
    for (size_t base = (size_t)blockIdx.x * 16; base < ntot; base += (size_t)gridDim.x * 16) {   // (uniform per workgroup)
      const size_t idx = base + e;
      double s[4] = {0.0, 0.0, 0.0, 0.0};
      if (idx < ntot) {
        const float* src = idx < n ? J.part + idx : J.partb + (idx - n);
        const size_t stride = idx < n ? n : (size_t)J.N;
        int sp = ph;
        for (; sp + 48 < J.splits; sp += 64) {
#pragma unroll
          for (int u = 0; u < 4; ++u) s[u] += (double)src[(size_t)(sp + 16 * u) * stride];
        }
        for (int u = 0; sp < J.splits; sp += 16, ++u) s[u] += (double)src[(size_t)sp * stride];
      }
      red[ph][e] = (s[0] + s[1]) + (s[2] + s[3]);
      __syncthreads();
      if (threadIdx.x < 16 && base + threadIdx.x < ntot) {
        const size_t i2 = base + threadIdx.x;
        double t = 0.0;
        for (int q = 0; q < 16; ++q) t += red[q][threadIdx.x];
        if (i2 < n) J.dW[dense ? i2 : (i2 / (size_t)J.K) * (size_t)J.lddw + i2 % (size_t)J.K] = (float)t;
        else J.db[i2 - n] = (float)t;
      }
      __syncthreads();
    }
    return;
  }
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (size_t)gridDim.x * 256) {
    // four interleaved running sums (splits 0, 4, 8 .. / 1, 5, .. / ..) combined in a fixed order: as reproducible as one
    // chain, but four loads in flight instead of one
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    int sp = 0;
    for (; sp + 4 <= J.splits; sp += 4) {
#pragma unroll
      for (int u = 0; u < 4; ++u) s[u] += (double)J.part[(size_t)(sp + u) * n + idx];
    }
    for (int u = 0; sp < J.splits; ++sp, ++u) s[u] += (double)J.part[(size_t)sp * n + idx];
    const size_t dst = dense ? idx : (idx / (size_t)J.K) * (size_t)J.lddw + idx % (size_t)J.K;
    J.dW[dst] = (float)((s[0] + s[1]) + (s[2] + s[3]));
  }
  if (J.db != nullptr && J.partb != nullptr) {
    for (int r = blockIdx.x * 256 + threadIdx.x; r < J.N; r += gridDim.x * 256) {
      double s = 0.0;
      for (int sp = 0; sp < J.splits; ++sp) s += (double)J.partb[(size_t)sp * J.N + r];
      J.db[r] = (float)s;
    }
  }
}

// ---- dW for 256 x 256 weight matrices, operands staged in LDS by LDS-DMA ---------------------------------------------
// The register-direct kernel above gives every 128 x 128 tile its own workgroup, so each operand half is fetched by two
// workgroups that are not synchronised: 2.0x the unique bytes at the memory side (profiles/hbm_traffic.json, round 1).
// Here ONE workgroup of 16 waves owns the whole 256 x 256 gradient of a point range: per 32-point chunk the two operand
// slabs (32 x 256 fp32 = 32 KB each, rows of the point-major matrices as they lie in memory) are copied global -> LDS by
// global_load_lds_dwordx4 (no VGPR round trip) into two alternating buffers: one raw barrier per 32-point chunk, the
// next chunk's DMAs in flight while this one is multiplied.  The fragments are what the direct kernel loads from global: lane (i, h)
// reads X[m + h][2i, 2i + 1] (8 bytes: the wave's two row tiles are the even / odd rows of its 64-row band) and
// Y[m + h][i], Y[m + h][32 + i] — conflict-free ds_read_b64 / ds_read_b32.  Wave (wm, wn) = rows 64 wm.., columns 64 wn...
constexpr int kStOpBytes = kStChunk * 256 * 4;  // one operand slab (32 KB) of kStChunk points (dw_plan.h)
constexpr int kStBufs = 2;                      // chunk c + 1 is copied while chunk c is multiplied

__device__ inline void dw_staged_issue(const DwPair& p, int m_begin, int nchunks, int chunk, char* buf, int wave, int lane) {
  const int c = chunk < nchunks ? chunk : nchunks - 1;   // past the end: harmless re-fetch, keeps vmcnt uniform
#pragma unroll
  for (int q = 0; q < kStChunk / 16; ++q) {
    const int u = (q * 16 + wave) * 64 + lane;           // 16-byte unit of the slab: row u / 64, columns 4 (u % 64)..
    const int row = m_begin + c * kStChunk + (u >> 6);
    const float* xs = p.X + (size_t)row * p.ldx + (u & 63) * 4;
    const float* ys = p.Y + (size_t)row * p.ldy + (u & 63) * 4;
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)xs,
                                     (__attribute__((address_space(3))) void*)(buf + (q * 16 + wave) * 1024), 16, 0, 0);
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)ys,
                                     (__attribute__((address_space(3))) void*)(buf + kStOpBytes + (q * 16 + wave) * 1024), 16, 0, 0);
  }
}

template <int DUMMY>
__global__ __launch_bounds__(1024, 1) void gemm_dw_staged_kernel(const DwGroup g) {
  __shared__ __attribute__((aligned(16))) char lds[kStBufs * 2 * kStOpBytes];   // 128 KB: the only shared object
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = wave_id();
  const int wm = wave >> 2, wn = wave & 3;
  int ji = 0, begin = 0;
  for (int q = 0; q + 1 < g.njobs; ++q)
    if ((int)blockIdx.x >= g.job[q].block_end) { ji = q + 1; begin = g.job[q].block_end; }
  const DwJob& J = g.job[ji];
  const int split = (int)blockIdx.x - begin;
  if (split >= J.splits) return;
  const int m_begin = split * J.rows_per_split;
  const int m_end = min(g.M, m_begin + J.rows_per_split);
  if (m_begin >= m_end) return;
  const int nchunks = (m_end - m_begin) / kStChunk;   // ranges are multiples of the chunk (host)
  const int i = lane & 31, h = lane >> 5;
  v16f acc[2][2];
  zero_acc<2>(acc);
  double bs0 = 0.0, bs1 = 0.0;
  const bool bias_wave = J.db != nullptr && wn == 0;
  for (int pi = 0; pi < J.npairs; ++pi) {
    const DwPair p = pi == 0 ? J.p1 : J.p2;
    const bool do_bias = bias_wave && pi == J.bias_pair;
    __builtin_amdgcn_s_barrier();   // every wave is done with the buffers of the previous pair
    dw_staged_issue(p, m_begin, nchunks, 0, lds, wave, lane);
    for (int c = 0; c < nchunks; ++c) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's part of chunk c has landed
      __builtin_amdgcn_s_barrier();                      // ... every wave's; and chunk c - 1 has been read by all
      dw_staged_issue(p, m_begin, nchunks, c + 1, lds + ((c + 1) & 1) * 2 * kStOpBytes, wave, lane);
      const char* bx = lds + (c & 1) * 2 * kStOpBytes;
      const char* by = bx + kStOpBytes;
      float t0 = 0.f, t1 = 0.f;
      // fragments of point pair q + 1 are read while the four MFMAs of pair q run (explicit two-deep rotation: left to
      // itself the compiler waits for each pair's reads right in front of its MFMAs)
      const char* ax = bx + h * 1024 + (wm * 64 + 2 * i) * 4;
      const char* ay = by + h * 1024 + (wn * 64 + i) * 4;
      vf2 a0 = *reinterpret_cast<const vf2*>(ax);
      float b00 = *reinterpret_cast<const float*>(ay), b01 = *reinterpret_cast<const float*>(ay + 128);
#pragma unroll
      for (int q = 0; q < kStChunk / 2; q += 2) {
        const vf2 a1 = *reinterpret_cast<const vf2*>(ax + (q + 1) * 2048);
        const float b10 = *reinterpret_cast<const float*>(ay + (q + 1) * 2048);
        const float b11 = *reinterpret_cast<const float*>(ay + (q + 1) * 2048 + 128);
        __builtin_amdgcn_sched_barrier(0);
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.x, b00, acc[0][0], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.y, b00, acc[1][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.x, b01, acc[0][1], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.y, b01, acc[1][1], 0, 0, 0);
        if (do_bias) { t0 += a0.x; t1 += a0.y; }
        __builtin_amdgcn_sched_barrier(0);
        if (q + 2 < kStChunk / 2) {
          a0 = *reinterpret_cast<const vf2*>(ax + (q + 2) * 2048);
          b00 = *reinterpret_cast<const float*>(ay + (q + 2) * 2048);
          b01 = *reinterpret_cast<const float*>(ay + (q + 2) * 2048 + 128);
        }
        __builtin_amdgcn_sched_barrier(0);
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.x, b10, acc[0][0], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.y, b10, acc[1][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.x, b11, acc[0][1], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.y, b11, acc[1][1], 0, 0, 0);
        if (do_bias) { t0 += a1.x; t1 += a1.y; }
        __builtin_amdgcn_sched_barrier(0);
      }
      if (do_bias) { bs0 += (double)t0; bs1 += (double)t1; }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this wave's LDS reads of chunk c are complete
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // drain the over-fetched chunk before the buffers are reused
  }
  // accumulator (ti, tj, r) of lane (i, h) is dW[64 wm + 2 rho + ti][64 wn + 32 tj + i], rho = (r & 3) + 8 (r >> 2) + 4 h
  const int lddw = J.lddw;
  float* __restrict__ pdst = J.part ? J.part + (size_t)split * J.N * lddw : nullptr;
#pragma unroll
  for (int tj = 0; tj < 2; ++tj) {
    const int col = wn * 64 + tj * 32 + i;
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = wm * 64 + 2 * ((r & 3) + 8 * (r >> 2) + 4 * h) + ti;
        if (pdst) pdst[(size_t)row * lddw + col] = acc[ti][tj][r];
        else atomicAdd(J.dW + (size_t)row * lddw + col, acc[ti][tj][r]);
      }
  }
  if (bias_wave) {
    bs0 += __shfl_xor(bs0, 32, 64);
    bs1 += __shfl_xor(bs1, 32, 64);
    if (h == 0) {
      if (J.partb) {
        J.partb[(size_t)split * J.N + wm * 64 + 2 * i] = (float)bs0;
        J.partb[(size_t)split * J.N + wm * 64 + 2 * i + 1] = (float)bs1;
      } else {
        atomicAdd(J.db + wm * 64 + 2 * i, (float)bs0);
        atomicAdd(J.db + wm * 64 + 2 * i + 1, (float)bs1);
      }
    }
  }
}

// ---- dW for 256 x 256 weight matrices as six bf16 MFMA terms (RNB_VARIANT_X3) --------------------------------------
// Same ownership as the staged kernel (one workgroup = the whole 256 x 256 gradient of a point range, slabs + ordered
// reduction), but the operands are split ONCE per workgroup on their way into LDS.  Staging: wave (operand o, point
// quad q) loads rows m + 4q .. + 4 of X_o, one dwordx4 per lane = ONE whole 1 KB row per instruction (thread = 4
// consecutive columns x 4 points; 4 loads per 16-point chunk — sixteen dword loads per thread, the first version,
// filled the vector-memory queue: half of every chunk's time went into issuing them, tools/dwx3_bench), splits each
// column's four points into hi / mid / lo (x3_split4) and writes 8-byte half units.  LDS image of a chunk:
// [operand][plane][point half][unit(column)] x 16 bytes with unit(c) = 68 (c & 3) + (c >> 2): the writer's lanes (column
// group c >> 2, fixed c & 3) and the reader's lanes (32 consecutive columns, ds_read_b128 of the MFMA operand of lane
// (column, half)) are both conflict-free.  8 waves: wave (wm, wn) owns rows 64 wm .. + 64, columns 128 wn .. + 128 of dW
// (128 accumulator registers; two waves per SIMD leave each 256).  Per chunk a wave issues 18 fragment reads and 48
// MFMAs; the split of the next chunk rides in the MFMA gaps; the raw rows run TWO chunks ahead in two register sets.
constexpr int kX3Chunk = 16;
constexpr int kX3Half = 4 * 68 * 16;            // one point half of one plane: 272 units (4 column residues x 68)
constexpr int kX3Plane = 2 * kX3Half;
constexpr int kX3OpBytes = 3 * kX3Plane;        // one operand of one chunk: 25.5 KB
constexpr int kX3BufBytes = 2 * kX3OpBytes;     // both operands
// NP planes per operand (3: bf16 hi / mid / lo, six terms; 2: fp16 hi / lo, three terms — "x2h")
template <int NP> constexpr int dw_op_bytes() { return NP * kX3Plane; }
template <int NP> constexpr int dw_buf_bytes() { return 2 * NP * kX3Plane; }

// (buffer loads: the lane's column offset in one VGPR, the wave-uniform row offset in the scalar operand)
__device__ inline void dw_x3_load(BufRsrc rs, unsigned voff, int ld, int row0, vf4 (&x)[4]) {
#pragma unroll
  for (int p = 0; p < 4; ++p)
    x[p] = __builtin_bit_cast(vf4, __builtin_amdgcn_raw_buffer_load_b128(rs, voff, (unsigned)(row0 + p) * (unsigned)ld * 4u, RNB_AUX_LD));   // read once
}
// 4 columns x 4 points of one thread -> 12 half units at w (+ 68 * 16 per column, + kX3Plane per plane)
// one column (four points) -> its NP plane units; sc: the operand's scale (x2h only)
template <int NP>
__device__ inline void dw_xn_split_col(const vf4& col, float sc, vu2x (&pl)[NP]) {
  if constexpr (NP == 3) x3_split4(col, pl[0], pl[1], pl[2]);
  else x2h_split4(col * sc, pl[0], pl[1]);
}
template <int NP>
__device__ inline void dw_x3_split(const vf4 (&x)[4], float sc, vu2x (&pl)[4][NP]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) dw_xn_split_col<NP>(vf4{x[0][j], x[1][j], x[2][j], x[3][j]}, sc, pl[j]);
}
template <int NP>
__device__ inline void dw_x3_store(char* w, const vu2x (&pl)[4][NP]) {
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int q = 0; q < NP; ++q) *reinterpret_cast<vu2x*>(w + j * 68 * 16 + q * kX3Plane) = pl[j][q];
}
// the NT terms of one (ti, tj) block, small ones first
template <int NP>
__device__ inline v16f dw_xn_mfma(const vu4x (&a)[NP], const vu4x (&b)[NP], v16f c, int t) {
  constexpr int PA[6] = {NP == 3 ? 2 : 1, 0, NP == 3 ? 1 : 0, 1, 0, 0};
  constexpr int PB[6] = {0, NP == 3 ? 2 : 1, NP == 3 ? 1 : 0, 0, 1, 0};
  if constexpr (NP == 3)
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(x3bf8, a[PA[t]]), __builtin_bit_cast(x3bf8, b[PB[t]]), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(x2h8, a[PA[t]]), __builtin_bit_cast(x2h8, b[PB[t]]), c, 0, 0, 0);
}
// One chunk of one wave: the 48 MFMAs on the fragments at fx / fy (one column tile of Y at a time, the next tile's
// fragments requested before the current tile's MFMAs), and — in the MFMA gaps, three vector instructions behind each
// MFMA — the split of the raw rows `x` of a later chunk, written to `w` at the end.
template <int NP>
__device__ inline void dw_x3_chunk(const char* fx, const char* fy, v16f (&acc)[2][4], const vf4 (&x)[4], float sc, char* w) {
  constexpr int NT = NP == 3 ? 6 : 3;
  vu4x a[2][NP], b[2][NP];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int pl = 0; pl < NP; ++pl) a[t][pl] = *reinterpret_cast<const vu4x*>(fx + pl * kX3Plane + t * 128);
#pragma unroll
  for (int pl = 0; pl < NP; ++pl) b[0][pl] = *reinterpret_cast<const vu4x*>(fy + pl * kX3Plane);
#pragma unroll
  for (int tj = 0; tj < 4; ++tj) {
    if (tj + 1 < 4) {
#pragma unroll
      for (int pl = 0; pl < NP; ++pl) b[(tj + 1) & 1][pl] = *reinterpret_cast<const vu4x*>(fy + pl * kX3Plane + (tj + 1) * 128);
    }
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int ti = 0; ti < 2; ++ti) acc[ti][tj] = dw_xn_mfma<NP>(a[ti], b[tj & 1], acc[ti][tj], t);
    {   // column tj of this thread's 4 x 4 raw block: split and stored while tile tj multiplies
      vu2x pl[NP];
      dw_xn_split_col<NP>(vf4{x[0][tj], x[1][tj], x[2][tj], x[3][tj]}, sc, pl);
#pragma unroll
      for (int q = 0; q < NP; ++q) *reinterpret_cast<vu2x*>(w + tj * 68 * 16 + q * kX3Plane) = pl[q];
    }
  }
  // schedule of the region: per column tile its fragment reads (of the NEXT tile), its 2 NT MFMAs with the vector work of
  // one raw column between them, then that column's stores
  __builtin_amdgcn_sched_group_barrier(0x100, 3 * NP, 0);   // a and b[0]
#pragma unroll
  for (int tj = 0; tj < 4; ++tj) {
    if (tj + 1 < 4) __builtin_amdgcn_sched_group_barrier(0x100, NP, 0);
#pragma unroll
    for (int m = 0; m < 2 * NT; ++m) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);
    }
    __builtin_amdgcn_sched_group_barrier(0x200, NP, 0);
  }
  __builtin_amdgcn_sched_barrier(0);
}
// The same for a NARROW job (Y operand of 64 columns: the PE-input layer, the tail of the albedo net's 320-wide first
// layer): wave (wm, wn) owns rows 64 wm .. + 64, columns 32 wn .. + 32 — 12 MFMAs per chunk; the staging split of the
// thread's whole 4 x 4 raw block rides between them (st_on: lanes that stage nothing skip the stores).
template <int NP>
__device__ inline void dw_x3_chunk_narrow(const char* fx, const char* fy, v16f (&acc)[2][1], const vf4 (&x)[4], float sc, char* w,
                                          bool st_on) {
  constexpr int NT = NP == 3 ? 6 : 3;
  vu4x a[2][NP], b[NP];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int pl = 0; pl < NP; ++pl) a[t][pl] = *reinterpret_cast<const vu4x*>(fx + pl * kX3Plane + t * 128);
#pragma unroll
  for (int pl = 0; pl < NP; ++pl) b[pl] = *reinterpret_cast<const vu4x*>(fy + pl * kX3Plane);
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int ti = 0; ti < 2; ++ti) acc[ti][0] = dw_xn_mfma<NP>(a[ti], b, acc[ti][0], t);
  vu2x pl[4][NP];
  dw_x3_split<NP>(x, sc, pl);
  __builtin_amdgcn_sched_group_barrier(0x100, 3 * NP, 0);
#pragma unroll
  for (int m = 0; m < 2 * NT; ++m) {
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
    __builtin_amdgcn_sched_group_barrier(0x002, 8, 0);
  }
  __builtin_amdgcn_sched_barrier(0);
  if (st_on) dw_x3_store<NP>(w, pl);
}
__device__ inline void dw_x3_colsum(const vf4 (&x)[4], bool on, double (&bs)[4]) {
  if (!on) return;
#pragma unroll
  for (int j = 0; j < 4; ++j) bs[j] += (double)((x[0][j] + x[1][j]) + (x[2][j] + x[3][j]));
}

// DUMMY == 1 (tools/dwx3_bench only): wave 0 sums the clocks it spends waiting at the barrier / issuing a chunk's
// reads, MFMAs, split and stores / issuing the next loads, and leaves them in J.db (as uint64[8] per workgroup)
// Pairs with DwPair::dead: the live 32-point units of a segment of the split, in ascending order, as a list in LDS.  The
// chunk pipeline below then walks the list instead of the range, so the order of summation is a function of the flags (of
// the inputs) alone.  A unit never straddles a tile (tiles are 64 points, splits begin on multiples of 32).
constexpr int kDwLiveCap = 2048;   // units per segment (65,536 points); a longer split takes several segments
struct DwLive {
  int n;
  unsigned short unit[kDwLiveCap];
};
// (read AS LDS: through a generic pointer the look-up would be a flat load, which waits on the vector-memory counter behind
// the operand rows in flight — fused_common.hip.h, h2_flag_read)
typedef __attribute__((address_space(3))) const DwLive lds_DwLive;
// The list of units [0, nunits) of the segment that begins at point m0.  Every thread fetches the words of its units (independent
// loads: one global round trip for the segment), then wave 0 compacts them in place (ballot + prefix count: ordered, no
// atomics; a block of 64 is read before anything at or below it is written).
__device__ inline void dw_live_build(DwLive* lv, const unsigned* __restrict__ dead, long long stride, int m0, int nunits, int tid) {
  __syncthreads();   // every wave is done with the previous list
  for (int u = tid; u < nunits; u += (int)blockDim.x)
    lv->unit[u] = dead[(size_t)((m0 + 32 * u) >> 6) * stride] == 0u ? (unsigned short)1 : (unsigned short)0;
  __syncthreads();
  if (tid < 64) {
    int n = 0;
    for (int u0 = 0; u0 < nunits; u0 += 64) {
      const int u = u0 + tid;
      const bool live = u < nunits && lv->unit[u] != 0;
      const unsigned long long mask = __builtin_amdgcn_ballot_w64(live);
      if (live) lv->unit[n + __builtin_popcountll(mask & ((1ull << tid) - 1ull))] = (unsigned short)u;
      n += __builtin_popcountll(mask);
    }
    if (tid == 0) lv->n = n;
  }
  __syncthreads();
}

template <int DUMMY, bool NARROW, int NP = 3>
__device__ inline void dw_x3_body(const DwGroup& g, const DwJob& J, int split, char* lds, DwLive* lv) {
  constexpr int kOp = dw_op_bytes<NP>(), kBuf = dw_buf_bytes<NP>();
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = wave_id();
  const int wm = wave >> 1, wn = wave & 1;
  const int m_begin = split * J.rows_per_split;
  const int m_end = min(g.M, m_begin + J.rows_per_split);
  if (m_begin >= m_end) return;   // (workgroup-uniform)
  // narrow job: the Y operand has 64 columns (J.K == 64); everything about X and the row split stays
  constexpr bool narrow = NARROW;
  // staging role of this thread: columns 4 cg .. + 4, points 4 pq .. + 4 of operand sop
  const int cg = lane, pq = wave & 3, sop = wave >> 2;
  const bool st_on = !(narrow && sop == 1 && cg >= 16);   // a narrow Y row is 16 column groups
  char* const swr = lds + sop * kOp + (pq >> 1) * kX3Half + cg * 16 + (pq & 1) * 8;   // + buffer, column, plane
  // fragment addresses of this lane: column 64 wm (128 wn) + 32 t + i of the operand, point half h
  const int i = lane & 31, h = lane >> 5;
  const int ui = (i & 3) * 68 + (i >> 2);
  const char* const fx = lds + h * kX3Half + (ui + 16 * wm) * 16;
  const char* const fy = lds + kOp + h * kX3Half + (ui + (narrow ? 8 : 32) * wn) * 16;
  constexpr int NTJ = NARROW ? 1 : 4;
  v16f acc[2][NTJ];
#pragma unroll
  for (int ti = 0; ti < 2; ++ti)
#pragma unroll
    for (int tj = 0; tj < NTJ; ++tj)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[ti][tj][r] = 0.f;
  double bs[4] = {0.0, 0.0, 0.0, 0.0};
  // x2h: one scale for the adjoint operands of all pairs of the job (they share the accumulators), from the larger of
  // their recorded maxima; the state operands (activations, Jacobian rows, network inputs) carry kH2ActScale
  [[maybe_unused]] float s_adj = 1.f, s_state = kH2ActScale, unscale = 1.f;
  if constexpr (NP == 2) {
    unsigned mb = J.p1.amax ? *J.p1.amax : 0u;
    if (J.npairs > 1 && J.p2.amax) mb = max(mb, *J.p2.amax);
    float inv;
    x2h_dyn_scale(mb, s_adj, inv);
    // the state operands: 2^6 (the round-4 constant: results unchanged) while their recorded maximum stays below 2^8, else
    // the power of two that puts it in [2^13, 2^14) — no saved activation / Jacobian row is out of range
    unsigned sb = J.p1.smax ? *J.p1.smax : 0u;
    if (J.npairs > 1 && J.p2.smax) sb = max(sb, *J.p2.smax);
    float inv_state = 1.f / kH2ActScale;
    if ((sb >> 23) >= 127u + 8u && (sb >> 23) < 255u) x2h_dyn_scale(sb, s_state, inv_state);
    unscale = inv * inv_state;
  }
  [[maybe_unused]] unsigned long long t_bar = 0, t_chunk = 0, t_load = 0, t_all = 0;
  [[maybe_unused]] const unsigned long long t_begin = DUMMY == 1 ? __builtin_amdgcn_s_memtime() : 0;
  [[maybe_unused]] const unsigned long long r_begin = DUMMY == 1 ? __builtin_amdgcn_s_memrealtime() : 0;
  for (int pi = 0; pi < J.npairs; ++pi) {
    const DwPair p = pi == 0 ? J.p1 : J.p2;
    const int ld = sop == 0 ? p.ldx : p.ldy;
    [[maybe_unused]] const float sc = NP == 2 ? (sop == p.adj ? s_adj : s_state) : 1.f;   // this thread's operand
    const unsigned voff = st_on ? 16u * (unsigned)cg : 0u;   // (lanes that stage nothing re-read column group 0)
    const bool do_bias = DUMMY == 0 && J.db != nullptr && pi == J.bias_pair && sop == 0;
    // a pair without dead tiles: ONE segment, the whole split, its chunks in place.  With them: segments of kDwLiveCap units,
    // each walked through its list of live units (all of this is workgroup-uniform)
    // A segment in which every unit turns out live is walked in place too: no look-up per chunk, the loop of an unflagged pair.
    // and a backward without a single dead tile reads one word: nothing else differs from an unflagged pair
    const bool flagged = p.dead != nullptr && __builtin_amdgcn_readfirstlane((int)*p.any_dead) != 0;
    const int seg_rows = flagged ? kDwLiveCap * 32 : m_end - m_begin;
   for (int seg0 = m_begin; seg0 < m_end; seg0 += seg_rows) {
    int nchunks = (min(m_end, seg0 + seg_rows) - seg0) / kX3Chunk;   // even: ranges are multiples of 32 points (host)
    bool listed = false;
    if (flagged) {
      dw_live_build(lv, p.dead, p.dead_stride, seg0, nchunks / 2, tid);
      const int nlive = __builtin_amdgcn_readfirstlane(((lds_DwLive*)lv)->n);
      listed = 2 * nlive != nchunks;
      nchunks = 2 * nlive;
      if (nchunks == 0) continue;
    }
    // first row of chunk k (relative to the segment): in place, or through the list
    auto row_of = [&](int k) -> int {
      const int u = listed ? __builtin_amdgcn_readfirstlane((int)((lds_DwLive*)lv)->unit[k >> 1]) : (k >> 1);
      return u * 32 + (k & 1) * kX3Chunk;
    };
    // resource based at this segment's first row: 32-bit offsets stay inside the split whatever the total point count
    const BufRsrc src = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>((sop == 0 ? p.X : p.Y) + (size_t)seg0 * ld), 0,
                                                          0xfffffffc, 0x00020000);
    const int last = nchunks - 1;
    const int r0 = 4 * pq;   // (rows relative to the segment)
    vf4 x0[4], x1[4];   // raw rows of an even / odd chunk
    dw_x3_load(src, voff, ld, r0 + row_of(0), x0);
    dw_x3_load(src, voff, ld, r0 + row_of(min(1, last)), x1);
    __builtin_amdgcn_s_barrier();   // every wave is done with the buffers of the previous pair
    {
      vu2x pl[4][NP];
      dw_x3_split<NP>(x0, sc, pl);
      if (st_on) dw_x3_store<NP>(swr, pl);
      dw_x3_colsum(x0, do_bias, bs);
    }
    dw_x3_load(src, voff, ld, r0 + row_of(min(2, last)), x0);
    for (int c = 0; c < nchunks; c += 2) {
      // even chunk c from buffer 0; chunk c + 1 (x1) -> buffer 1; x1 <- chunk c + 3
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      [[maybe_unused]] const unsigned long long s0 = DUMMY == 1 ? __builtin_amdgcn_s_memtime() : 0;
      __builtin_amdgcn_s_barrier();
      [[maybe_unused]] const unsigned long long s1 = DUMMY == 1 ? __builtin_amdgcn_s_memtime() : 0;
      const int row3 = row_of(min(c + 3, last)), row4 = row_of(min(c + 4, last));   // (looked up ahead of the chunk's own LDS reads)
      if constexpr (narrow) dw_x3_chunk_narrow<NP>(fx, fy, acc, x1, sc, swr + kBuf, st_on);
      else dw_x3_chunk<NP>(fx, fy, acc, x1, sc, swr + kBuf);
      dw_x3_colsum(x1, do_bias, bs);   // (nchunks even: chunk c + 1 always exists)
      [[maybe_unused]] const unsigned long long s2 = DUMMY == 1 ? __builtin_amdgcn_s_memtime() : 0;
      dw_x3_load(src, voff, ld, r0 + row3, x1);
      if constexpr (DUMMY == 1) {
        const unsigned long long s3 = __builtin_amdgcn_s_memtime();
        t_bar += s1 - s0; t_chunk += s2 - s1; t_load += s3 - s2;
      }
      // odd chunk c + 1 from buffer 1; chunk c + 2 (x0) -> buffer 0 (past the end: a re-split of the last chunk that
      // nobody reads); x0 <- chunk c + 4
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      if constexpr (narrow) dw_x3_chunk_narrow<NP>(fx + kBuf, fy + kBuf, acc, x0, sc, swr, st_on);
      else dw_x3_chunk<NP>(fx + kBuf, fy + kBuf, acc, x0, sc, swr);
      dw_x3_colsum(x0, do_bias && c + 2 < nchunks, bs);
      dw_x3_load(src, voff, ld, r0 + row4, x0);
    }
   }   // (segments)
  }
  // accumulator (ti, tj, r) of lane (i, h) is dW[64 wm + 32 ti + rho][128 wn + 32 tj + i], rho = (r & 3) + 8 (r >> 2) + 4 h
  // slabs are compact [split][N][K] (K = the job's Y columns; dw_reduce_kernel scatters them into dW with lddw)
  const int lddw = J.lddw, Kj = J.K;
  float* __restrict__ pdst = J.part ? J.part + (size_t)split * J.N * Kj : nullptr;
#pragma unroll
  for (int tj = 0; tj < NTJ; ++tj) {
    const int col = narrow ? wn * 32 + i : wn * 128 + tj * 32 + i;
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = wm * 64 + ti * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        const float v = NP == 2 ? acc[ti][tj][r] * unscale : acc[ti][tj][r];
        if (pdst) __builtin_nontemporal_store(v, pdst + (size_t)row * Kj + col);
        else atomicAdd(J.dW + (size_t)row * lddw + col, v);
      }
  }
  if constexpr (DUMMY == 1) {
    if (tid == 0) {
      unsigned long long* o = reinterpret_cast<unsigned long long*>(J.db) + 8 * (size_t)blockIdx.x;
      t_all = __builtin_amdgcn_s_memtime() - t_begin;
      o[0] = t_bar; o[1] = t_chunk; o[2] = t_load; o[3] = t_all;
      o[4] = __builtin_amdgcn_s_memrealtime() - r_begin;   // 100 MHz
    }
  }
  if (DUMMY == 0 && J.db != nullptr) {   // column sums of the bias pair's X operand: the four point quads of a column meet in LDS
    double* bx = reinterpret_cast<double*>(lds);
    __syncthreads();
    if (sop == 0) {
#pragma unroll
      for (int j = 0; j < 4; ++j) bx[pq * 256 + 4 * cg + j] = bs[j];
    }
    __syncthreads();
    if (tid < 256) {
      const float v = (float)((bx[tid] + bx[256 + tid]) + (bx[512 + tid] + bx[768 + tid]));
      if (J.partb) J.partb[(size_t)split * J.N + tid] = v;
      else atomicAdd(J.db + tid, v);
    }
  }
}


template <int DUMMY, int NP = 3>
__global__ __launch_bounds__(512, 1) void gemm_dw_x3_kernel(const DwGroup g) {
  __shared__ __attribute__((aligned(16))) char lds[2 * dw_buf_bytes<NP>() > 8192 ? 2 * dw_buf_bytes<NP>() : 8192];   // 102 KB (NP = 2: 68 KB)
  __shared__ DwLive live;   // 4 KB
  int ji = 0, begin = 0;
  for (int q = 0; q + 1 < g.njobs; ++q)
    if ((int)blockIdx.x >= g.job[q].block_end) { ji = q + 1; begin = g.job[q].block_end; }
  const DwJob& J = g.job[ji];
  const int split = (int)blockIdx.x - begin;
  if (split >= J.splits) return;
  // two bodies, one per job width (workgroup-uniform): separate accumulator sets, separate register allocation
  if (J.K < 256) dw_x3_body<DUMMY, true, NP>(g, J, split, lds, &live);
  else dw_x3_body<DUMMY, false, NP>(g, J, split, lds, &live);
}

}  // namespace rnb
