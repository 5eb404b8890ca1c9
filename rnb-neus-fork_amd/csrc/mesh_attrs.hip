// Per-vertex mesh attributes (rnb_mesh_vertex_attrs): the small kernels around the point sweeps of one chunk of vertices —
// grid-index vertices -> fp32 model-space points, the Newton step onto the level set, and the epilogue that turns the
// sweeps' per-point state (sdf [Mp], d sdf / d x [Mp,4], albedo [Mp,4]) into the dense per-vertex outputs.
#include "rnb_internal.h"

namespace rnb {

constexpr int kMeshBlock = 256;   // threads = vertices per workgroup of the two per-vertex kernels

// Element i of the chunk's [n,3] point buffer.  Grid-index vertices are rescaled exactly as the host does it
// (models/renderer.py:34 in float64, then torch's conversion to float32): a division, a multiplication and an addition,
// each rounded on its own — contraction is off for this function, a fused multiply-add would change the last bit.
__global__ __launch_bounds__(kMeshBlock) void mesh_points_kernel(MeshPointsSrc src, int64_t first, int64_t n3,
                                                                 float* __restrict__ pts) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * kMeshBlock + threadIdx.x;
  if (i >= n3) return;
  const int64_t at = first * 3 + i;
  if (src.grid != nullptr) {
    const int d = (int)(i % 3);
    const double q = src.grid[at] / src.rm1;
    const double scaled = q * (double)src.span[d];
    pts[i] = (float)(scaled + (double)src.bmin[d]);
  } else {
    pts[i] = src.pts[at];
  }
}

// [rows, ncols] values, one row per thread, -> out rows [row0, row0 + rows) through LDS: consecutive lanes store consecutive
// elements.  Block-uniform call (two barriers); stage holds kMeshBlock * ncols elements.
template <class T>
__device__ inline void store_rows(T* __restrict__ out, int64_t row0, int rows, int ncols, const T (&v)[4], T* stage, int tid) {
  for (int c = 0; c < ncols; ++c) stage[tid * ncols + c] = v[c];
  __syncthreads();
  const int total = rows * ncols;
  for (int i = tid; i < total; i += kMeshBlock) out[row0 * ncols + i] = stage[i];
  __syncthreads();
}

// One Newton step of the chunk's points towards sdf = level: p <- p - t g with t = (sdf - level) / |g|^2, the displacement
// |t| |g| clamped to max_step (less the rounding of the stored coordinates, see below).  A point whose sdf or g is not
// finite, or whose |g|^2 is below 1e-12 (or overflows), stays.
__global__ __launch_bounds__(kMeshBlock) void mesh_newton_kernel(const float* __restrict__ sdf, const float* __restrict__ nrm,
                                                                 int64_t n, float level, float max_step, float* __restrict__ pts) {
  __shared__ float stage[kMeshBlock * 3];
  const int tid = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * kMeshBlock;
  const int64_t i = row0 + tid;
  float p[4] = {0.f, 0.f, 0.f, 0.f};
  if (i < n) {
    p[0] = pts[i * 3];
    p[1] = pts[i * 3 + 1];
    p[2] = pts[i * 3 + 2];
    const float4 g = *reinterpret_cast<const float4*>(nrm + i * 4);
    const float f = sdf[i];
    const float g2 = g.x * g.x + g.y * g.y + g.z * g.z;
    const bool ok = isfinite(f) && isfinite(g2) && g2 >= 1e-12f;   // (g2 finite: every component is)
    if (ok) {
      float t = (f - level) / g2;
      const float disp = fabsf(t) * sqrtf(g2);
      // max_step bounds the distance between the STORED fp32 points: the clamp leaves room for half an ulp (2^-24 relative)
      // of every stored coordinate, and 2^-21 relative for the rounding of the step's own arithmetic
      const float room = (fabsf(p[0]) + fabsf(p[1]) + fabsf(p[2]) + 3.f * max_step) * 5.9604645e-8f;
      const float lim = (max_step - room) * (1.f - 4.7683716e-7f);
      if (disp > lim) t = lim > 0.f ? t * (lim / disp) : 0.f;
      p[0] -= t * g.x;
      p[1] -= t * g.y;
      p[2] -= t * g.z;
    }
  }
  const int64_t left = n - row0;
  store_rows(pts, row0, (int)(left < kMeshBlock ? left : kMeshBlock), 3, p, stage, tid);
}

// The outputs of rows [0, n) of a chunk, written at vertex `first` + row of every requested array.
__global__ __launch_bounds__(kMeshBlock) void mesh_attrs_kernel(const float* __restrict__ pts, const float* __restrict__ sdf,
                                                                const float* __restrict__ nrm, const float* __restrict__ alb,
                                                                int64_t first, int64_t n, MeshOut o) {
  __shared__ float stage[kMeshBlock * 4];
  __shared__ uint8_t stage8[kMeshBlock * 3];
  const int tid = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * kMeshBlock;
  const int64_t i = row0 + tid;
  const int64_t left = n - row0;
  const int rows = (int)(left < kMeshBlock ? left : kMeshBlock);
  const int64_t out0 = first + row0;
  const bool live = i < n;
  if (o.sdf != nullptr && live) o.sdf[first + i] = sdf[i];
  if (o.points != nullptr) {
    float p[4] = {0.f, 0.f, 0.f, 0.f};
    if (live) { p[0] = pts[i * 3]; p[1] = pts[i * 3 + 1]; p[2] = pts[i * 3 + 2]; }
    store_rows(o.points, out0, rows, 3, p, stage, tid);
  }
  if (o.gradient != nullptr || o.normal != nullptr) {
    float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live) g = *reinterpret_cast<const float4*>(nrm + i * 4);
    if (o.gradient != nullptr) {
      const float v[4] = {g.x, g.y, g.z, 0.f};
      store_rows(o.gradient, out0, rows, 3, v, stage, tid);
    }
    if (o.normal != nullptr) {
      const float len = sqrtf(g.x * g.x + g.y * g.y + g.z * g.z);
      const bool ok = len > 0.f && isfinite(len);
      const float v[4] = {ok ? g.x / len : 0.f, ok ? g.y / len : 0.f, ok ? g.z / len : 0.f, 0.f};
      store_rows(o.normal, out0, rows, 3, v, stage, tid);
    }
  }
  if (o.albedo != nullptr || o.rgb != nullptr) {
    float4 a4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live) a4 = *reinterpret_cast<const float4*>(alb + i * 4);
    const float a[4] = {a4.x, a4.y, a4.z, a4.w};
    if (o.albedo != nullptr) store_rows(o.albedo, out0, rows, o.Co, a, stage, tid);
    if (o.rgb != nullptr) {
      uint8_t q[4] = {0, 0, 0, 0};
      for (int c = 0; c < 3; ++c) {
        const int src = o.Co == 1 ? 0 : (o.swap_rb ? 2 - c : c);
        q[c] = (uint8_t)rintf(255.f * fminf(fmaxf(a[src], 0.f), 1.f));
      }
      store_rows(o.rgb, out0, rows, 3, q, stage8, tid);
    }
  }
}

int launch_mesh_points(const MeshPointsSrc& src, int64_t first, int64_t n, float* pts, hipStream_t s) {
  hipLaunchKernelGGL(mesh_points_kernel, dim3(blocks_for(n * 3, kMeshBlock)), dim3(kMeshBlock), 0, s, src, first, n * 3, pts);
  RNB_CHECK_LAUNCH();
  return RNB_OK;
}

int launch_mesh_newton(const float* sdf, const float* nrm, int64_t n, float level, float max_step, float* pts, hipStream_t s) {
  hipLaunchKernelGGL(mesh_newton_kernel, dim3(blocks_for(n, kMeshBlock)), dim3(kMeshBlock), 0, s, sdf, nrm, n, level, max_step,
                     pts);
  RNB_CHECK_LAUNCH();
  return RNB_OK;
}

int launch_mesh_attrs(const float* pts, const PointBufs& pb, int64_t first, int64_t n, const MeshOut& o, hipStream_t s) {
  hipLaunchKernelGGL(mesh_attrs_kernel, dim3(blocks_for(n, kMeshBlock)), dim3(kMeshBlock), 0, s, pts, pb.sdf, pb.nrm, pb.alb,
                     first, n, o);
  RNB_CHECK_LAUNCH();
  return RNB_OK;
}

}  // namespace rnb
