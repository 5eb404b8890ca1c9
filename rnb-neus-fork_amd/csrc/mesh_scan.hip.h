// Flag scans and stable compaction shared by the mesh kernels (mesh_clean.hip, mesh_simplify.hip).
//
// The scans follow mcubes.hip: per block of 1024 items a sum (mk_flag_sum_kernel), one workgroup scans the block sums
// (mk_scan_kernel), the emit kernel recomputes the flags and adds a block-local scan (mk_flag_emit_kernel).  Output order
// = input order (stable), whatever the launch geometry.
#pragma once
#include "rnb_internal.h"

namespace rnb {

constexpr int kMkThreads = 256;
constexpr int kMkItems = 4;
constexpr int kMkTile = kMkThreads * kMkItems;

static inline int64_t mk_blocks(int64_t n) { return (n + kMkTile - 1) / kMkTile; }
static inline int64_t mk_pad64(int64_t n) { return (n + 63) / 64 * 64; }

// exclusive prefix of `v` over the 256 threads of the workgroup (thread order); *total = sum over the workgroup
__device__ inline unsigned mk_block_scan(unsigned v, unsigned* total, unsigned* red /* [4] */) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  __syncthreads();
  if (lane == 63) red[wave] = inc;
  __syncthreads();
  unsigned base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < kMkThreads / 64; ++w) {
    if (w < wave) base += red[w];
    tot += red[w];
  }
  *total = tot;
  return base + inc - v;
}

template <class Flag>
__global__ __launch_bounds__(kMkThreads) void mk_flag_sum_kernel(Flag f, int64_t n, unsigned* __restrict__ bsum) {
  __shared__ unsigned red[4];
  const int64_t i0 = (int64_t)blockIdx.x * kMkTile + (int64_t)threadIdx.x * kMkItems;
  unsigned cnt = 0;
#pragma unroll
  for (int k = 0; k < kMkItems; ++k)
    if (i0 + k < n) cnt += f(i0 + k) ? 1u : 0u;
  unsigned tot;
  mk_block_scan(cnt, &tot, red);
  if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}

// exclusive scan in place of `narr` (1 or 2) block-sum arrays, one workgroup; totals[k] = sum of array k
// (static: not a template, so every file that includes this header gets a kernel of its own)
static __global__ __launch_bounds__(1024) void mk_scan_kernel(unsigned* __restrict__ a0, int64_t n0, unsigned* __restrict__ a1,
                                                       int64_t n1, int narr, int64_t* __restrict__ totals) {
  __shared__ unsigned long long wsum[16];
  __shared__ unsigned long long carry_s;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int which = 0; which < narr; ++which) {
    unsigned* a = which == 0 ? a0 : a1;
    const int64_t nblocks = which == 0 ? n0 : n1;
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    for (int64_t base = 0; base < nblocks; base += 1024) {
      const int64_t i = base + threadIdx.x;
      const unsigned long long v = i < nblocks ? a[i] : 0;
      unsigned long long inc = v;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
      }
      if (lane == 63) wsum[wave] = inc;
      __syncthreads();
      unsigned long long before = carry_s;
      for (int w = 0; w < wave; ++w) before += wsum[w];
      if (i < nblocks) a[i] = (unsigned)(before + inc - v);
      __syncthreads();
      if (threadIdx.x == 1023) carry_s = before + inc;
      __syncthreads();
    }
    if (threadIdx.x == 0) totals[which] = (int64_t)carry_s;
    __syncthreads();
  }
}

// emit(i, flag, pos): pos = number of flagged items before i
template <class Flag, class Emit>
__global__ __launch_bounds__(kMkThreads) void mk_flag_emit_kernel(Flag f, Emit emit, int64_t n,
                                                                  const unsigned* __restrict__ boff) {
  __shared__ unsigned red[4];
  const int64_t i0 = (int64_t)blockIdx.x * kMkTile + (int64_t)threadIdx.x * kMkItems;
  unsigned bits = 0;
#pragma unroll
  for (int k = 0; k < kMkItems; ++k)
    if (i0 + k < n && f(i0 + k)) bits |= 1u << k;
  unsigned tot;
  unsigned pos = boff[blockIdx.x] + mk_block_scan((unsigned)__popc(bits), &tot, red);
#pragma unroll
  for (int k = 0; k < kMkItems; ++k) {
    if (i0 + k >= n) break;
    const bool fl = (bits >> k) & 1u;
    emit(i0 + k, fl, pos);
    pos += fl ? 1u : 0u;
  }
}

}  // namespace rnb
