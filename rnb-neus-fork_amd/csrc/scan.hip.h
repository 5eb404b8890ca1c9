// Integer exclusive scans over tiles of 1024 items (256 threads x 4), shared by marching cubes (mcubes.hip), the mesh
// tools (mesh_clean.hip, mesh_simplify.hip) and the triangle bins (mesh_eval.hip).  Integer only: no rounding to pin, so a
// file compiled without -ffp-contract=off may include it.
//
// A scan of n items is three launches: per tile a sum (scan_sum_kernel, or a kernel of the caller's that takes its sums
// from block_exclusive_scan), one workgroup scans the tile sums in place (scan_block_sums_kernel), the emit kernel
// evaluates the weights again and adds a scan inside the tile (scan_emit_kernel).  Output order = input order (stable),
// whatever the launch geometry.
//
// Every kernel here is a template, so a file that includes the header instantiates what it launches and nothing else,
// and an instance two files share (scan_block_sums_kernel<unsigned>) is one definition under the one-definition rule:
// integer code compiles to the same instructions under every file's flags, so whichever copy a launch resolves to
// computes the same bits.
#pragma once
#include "rnb_internal.h"

namespace rnb {

constexpr int kScanThreads = 256;
constexpr int kScanItems = 4;
constexpr int kScanTile = kScanThreads * kScanItems;

static inline int64_t scan_blocks(int64_t n) { return (n + kScanTile - 1) / kScanTile; }
static inline int64_t scan_pad64(int64_t n) { return (n + 63) / 64 * 64; }

// exclusive prefix of `v` over the 256 threads of the workgroup (thread order); *total = sum over the workgroup
template <class T>
__device__ inline T block_exclusive_scan(T v, T* total, T* red /* [4] */) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  T inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  __syncthreads();                 // `red` may still be read by the previous call
  if (lane == 63) red[wave] = inc;
  __syncthreads();
  T base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < kScanThreads / 64; ++w) {
    if (w < wave) base += red[w];
    tot += red[w];
  }
  *total = tot;
  return base + inc - v;
}

// Exclusive scan in place of `narr` (1 or 2) arrays of tile sums, one workgroup of 1024 going through them in chunks of
// 1024; totals[k] = sum of array k.  The running carry is 64-bit whatever T: the offsets themselves fit T whenever the
// totals pass the caller's range check.  The chunk loop's second trip (more than 2^20 items) is taken by
// tests/test_gpu_mesh_second_trips.py (two arrays of different length, one array in four trips) and, for the 64-bit
// instance, by tests/test_gpu_mesh_eval.py test_bins_past_the_first_chunk_of_the_block_sum_scan.
template <class T>
__global__ __launch_bounds__(1024) void scan_block_sums_kernel(T* __restrict__ a0, int64_t n0, T* __restrict__ a1, int64_t n1,
                                                               int narr, int64_t* __restrict__ totals) {
  __shared__ unsigned long long wsum[16];
  __shared__ unsigned long long carry_s;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int which = 0; which < narr; ++which) {
    T* a = which == 0 ? a0 : a1;
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
#pragma unroll                     // all 16 sums in wide LDS reads: a loop to `wave` is a chain of up to 15 dependent reads
      for (int w = 0; w < 16; ++w)
        if (w < wave) before += wsum[w];
      if (i < nblocks) a[i] = (T)(before + inc - v);
      __syncthreads();
      if (threadIdx.x == 1023) carry_s = before + inc;
      __syncthreads();
    }
    if (threadIdx.x == 0) totals[which] = (int64_t)carry_s;
    __syncthreads();
  }
}

// w(i) = the count of item i (a flag is the 0 / 1 case); bsum[tile] = the sum of the tile's counts.  P: the position type.
template <class P, class Weight>
__global__ __launch_bounds__(kScanThreads) void scan_sum_kernel(Weight w, int64_t n, P* __restrict__ bsum) {
  __shared__ P red[4];
  const int64_t i0 = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
  P cnt = 0;
#pragma unroll
  for (int k = 0; k < kScanItems; ++k)
    if (i0 + k < n) cnt += (P)w(i0 + k);
  P tot;
  block_exclusive_scan(cnt, &tot, red);
  if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}

// emit(i, w, pos): w = w(i), pos = the sum of the counts before i.  A thread evaluates the weights of its items once, all
// before the scan, and keeps them in registers: emit(i, ..) may overwrite what w(i) read.
template <class P, class Weight, class Emit>
__global__ __launch_bounds__(kScanThreads) void scan_emit_kernel(Weight w, Emit emit, int64_t n, const P* __restrict__ boff) {
  __shared__ P red[4];
  const int64_t i0 = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
  P wt[kScanItems], s = 0;
#pragma unroll
  for (int k = 0; k < kScanItems; ++k) {
    wt[k] = i0 + k < n ? (P)w(i0 + k) : 0;
    s += wt[k];
  }
  P tot;
  P pos = boff[blockIdx.x] + block_exclusive_scan(s, &tot, red);
#pragma unroll
  for (int k = 0; k < kScanItems; ++k) {
    if (i0 + k >= n) break;
    emit(i0 + k, wt[k], pos);
    pos += wt[k];
  }
}

}  // namespace rnb
