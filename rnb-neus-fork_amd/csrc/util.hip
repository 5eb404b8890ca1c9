// Small utility launches shared by the entry points: grid points, scaled / strided copies, max |.| of a buffer, and the
// range report of rnb_render_range.
#include "gemm.hip.h"
#include "rnb_internal.h"

namespace rnb {

// points [first, first + n) of the regular grid of extract_fields (generic path of rnb_sdf_grid)
__global__ void grid_points_kernel(GridGen g, int64_t first, int64_t n, float* __restrict__ pts) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int ix = 0, iy = 0, iz = 0;   // (a masked row of a brick list computes on the grid's first sample and stores nothing)
  grid_locate(g, first + i, first + n, ix, iy, iz);
  pts[i * 3] = linspace_at(g.bmin[0], g.bmax[0], g.res, ix);
  pts[i * 3 + 1] = linspace_at(g.bmin[1], g.bmax[1], g.res, iy);
  pts[i * 3 + 2] = linspace_at(g.bmin[2], g.bmax[2], g.res, iz);
}
__global__ void scale_copy_kernel(const float* __restrict__ src, float scale, int64_t n, float* __restrict__ dst) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = src[i] * scale;
}

// max |.| of a buffer into one slot (float bits, atomicMax; the slot only grows): the maxima of the saved state that the
// per-layer albedo path leaves for the x2h weight-gradient jobs (the fused kernels record theirs on the way)
__global__ __launch_bounds__(256) void absmax_kernel(const float* __restrict__ x, int64_t n4, unsigned* __restrict__ slot) {
  float m = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const vf4 v = *reinterpret_cast<const vf4*>(x + 4 * i);
    m = fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
  }
  amax_commit(slot, m, threadIdx.x & 63);
}

// strided [rows, ld] (first ncols columns) -> dense [M, ncols]
__global__ void copy_cols_kernel(const float* __restrict__ src, int ld, int ncols, int64_t M, float* __restrict__ out) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M * ncols) return;
  int64_t row = i / ncols;
  int col = (int)(i - row * ncols);
  out[i] = src[row * ld + col];
}
// dense [M, ncols] -> strided [Mp, ld] (rows >= M zero-filled)
__global__ void fill_cols_kernel(const float* __restrict__ src, int ncols, int64_t M, int64_t Mp, int ld,
                                 float* __restrict__ dst) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= Mp * ncols) return;
  int64_t row = i / ncols;
  int col = (int)(i - row * ncols);
  dst[row * ld + col] = row < M ? src[i] : 0.f;
}

int launch_grid_points(const GridGen& g, int64_t first, int64_t n, float* pts, hipStream_t s) {
  hipLaunchKernelGGL(grid_points_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, s, g, first, n, pts);
  RNB_CHECK_LAUNCH();
  return RNB_OK;
}
// dst[grid_out_index(first + i)] = src[i] * scale: the scatter of a brick list / the lattice on the per-layer route
__global__ void grid_scatter_kernel(GridGen g, const float* __restrict__ src, int64_t first, int64_t n, float* __restrict__ dst) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t o = grid_out_index(g, first + i, first + n);
  if (o >= 0) dst[o] = src[i] * g.out_scale;   // (shared face samples: both bricks write the same bits, see fused.hip)
}
int launch_grid_scatter(const GridGen& g, const float* src, int64_t first, int64_t n, float* dst, hipStream_t s) {
  hipLaunchKernelGGL(grid_scatter_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, s, g, src, first, n, dst);
  RNB_CHECK_LAUNCH();
  return RNB_OK;
}
int launch_scale_copy(const float* src, float scale, int64_t n, float* dst, hipStream_t s) {
  hipLaunchKernelGGL(scale_copy_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, s, src, scale, n, dst);
  RNB_CHECK_LAUNCH();
  return RNB_OK;
}
int launch_copy_cols(const float* src, int ld, int ncols, int64_t M, float* out, hipStream_t s) {
  hipLaunchKernelGGL(copy_cols_kernel, dim3(blocks_for(M * ncols, 256)), dim3(256), 0, s, src, ld, ncols, M, out);
  RNB_CHECK_LAUNCH();
  return RNB_OK;
}
int launch_fill_cols(const float* src, int ncols, int64_t M, int64_t Mp, int ld, float* dst, hipStream_t s) {
  hipLaunchKernelGGL(fill_cols_kernel, dim3(blocks_for(Mp * ncols, 256)), dim3(256), 0, s, src, ncols, M, Mp, ld, dst);
  RNB_CHECK_LAUNCH();
  return RNB_OK;
}

int launch_absmax_rows(const float* x, int64_t n, unsigned* slot, hipStream_t s) {
  hipLaunchKernelGGL(absmax_kernel, dim3(1024), dim3(256), 0, s, x, n / 4, slot);
  RNB_CHECK_LAUNCH();
  return RNB_OK;
}

// out[k] = max over a list of word slots (float bits) — the finishing step of rnb_render_range
__global__ void range_fold_kernel(const unsigned* __restrict__ words, int n, int k, float* __restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  unsigned m = 0u;
  for (int i = 0; i < n; ++i) m = max(m, words[i]);
  out[k] = __builtin_bit_cast(float, m);
}

// out[k] = how many of the n per-tile words (PointBufs::alb_dead) are set — rnb_render_range's count of skipped tiles
// `ran`: the backward's own record that it wrote the words (AMAX_DEAD_RAN); 0: they hold something else, the count is 0
__global__ void dead_count_kernel(const unsigned* __restrict__ words, long long stride, int n, const unsigned* __restrict__ ran, int k,
                                  float* __restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  int c = 0;
  for (int i = 0; i < n && *ran != 0u; ++i) c += words[(size_t)i * stride] != 0u ? 1 : 0;
  out[k] = (float)c;
}

// rnb_render_range: out[0..5] as documented in include/rnbneus.h.  The maxima of the saved state are taken by a pass over the
// buffers themselves (the hot path records them only for tiles beyond the fixed scales' range); out doubles as scratch.
int launch_range_report(const Layout& L, const float* packed, const PointBufs& pb, bool with_color, bool with_backward, float* out,
                        hipStream_t s) {
  RNB_CHECK_HIP(hipMemsetAsync(out, 0, 8 * sizeof(float), s));
  unsigned* w = reinterpret_cast<unsigned*>(out);
  const H2Tab* tab = h2_tab(L, packed);
  if (tab != nullptr) {
    hipLaunchKernelGGL(range_fold_kernel, dim3(1), dim3(64), 0, s, tab->wmax, L.nh + 1 + L.nc, 0, out);
    RNB_CHECK_LAUNCH();
  }
  const int64_t n = pb.Mp * L.Hp;
  const bool bf = is_bf16(L);   // (bf16 state is not fp32: only the fp32 buffers are scanned)
  if (!bf) {
    RNB_TRY(launch_absmax_rows(pb.e, pb.Mp * L.Ep, w + 1, s));
    for (int l = 0; l < L.nh; ++l) RNB_TRY(launch_absmax_rows(pb.a[l], n, w + 1, s));
    if (pb.gz[0] != nullptr)
      for (int l = 0; l < L.nh; ++l) RNB_TRY(launch_absmax_rows(pb.gz[l], n, w + 2, s));
  }
  if (with_color && pb.cin != nullptr) {
    RNB_TRY(launch_absmax_rows(pb.cin, pb.Mp * L.Cinp, w + 3, s));
    for (int l = 0; l < L.nc; ++l) RNB_TRY(launch_absmax_rows(pb.ac[l], pb.Mp * L.Hcp, w + 3, s));
  }
  if (with_backward && L.route.h2) {
    hipLaunchKernelGGL(range_fold_kernel, dim3(1), dim3(64), 0, s, pb.amax, (int)AMAX_MAXIMA, 4, out);
    RNB_CHECK_LAUNCH();
  }
  // (the words exist only where the backward took the zero-tile path, which it records in amax: elsewhere the count is 0)
  if (with_backward && with_color && pb.alb_dead != nullptr && pb.amax != nullptr) {
    hipLaunchKernelGGL(dead_count_kernel, dim3(1), dim3(64), 0, s, pb.alb_dead, (long long)pb.alb_dead_stride, (int)((pb.M + 63) / 64),
                       pb.amax + AMAX_DEAD_RAN, 5, out);   // (tiles with a real row)
    RNB_CHECK_LAUNCH();
  }
  return RNB_OK;
}

}  // namespace rnb
