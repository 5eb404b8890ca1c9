// Mesh ray casting on the device: the first hit of every ray with a binned triangle mesh (rnb_mesh_raycast in
// include/rnbneus.h; DESIGN.md "Mesh ray casting").  One kernel, rc_kernel, one lane per ray, over the bins and the
// corners [T,9] that rnb_mesh_bins_count / rnb_mesh_bins_emit (csrc/mesh_eval.hip) left in device memory.  No LDS, no
// atomics.  Compiled with -ffp-contract=off: every product and difference rounds on its own, as
// tests/mesh_raycast_ref.py evaluates them.
//
// The pair test, the walk, and the arguments for why no hit is skipped and why nothing hangs or reads out of bounds are
// in mesh_raycast.hip.h (rc_visit, rc_first_hit), which the votes kernel of mesh_cull.hip shares.
#include "mesh_raycast.hip.h"

namespace rnb {

constexpr int kRcThreads = 256;

struct RcArgs {
  const double* origins;
  const double* directions;
  const double* t_min;
  const double* t_max;
  int64_t N;
  BinnedMesh mesh;
  double* t;
  int32_t* triangle;
  double* bary;
};

__global__ __launch_bounds__(kRcThreads) void rc_kernel(RcArgs a) {
  const int64_t i = (int64_t)blockIdx.x * kRcThreads + threadIdx.x;
  if (i >= a.N) return;
  const double nan = __longlong_as_double(0x7ff8000000000000ll), inf = __longlong_as_double(0x7ff0000000000000ll);
  const double o0 = a.origins[i * 3], o1 = a.origins[i * 3 + 1], o2 = a.origins[i * 3 + 2];
  const double d0 = a.directions[i * 3], d1 = a.directions[i * 3 + 1], d2 = a.directions[i * 3 + 2];
  const RcBest best = rc_first_hit(a.mesh, o0, o1, o2, d0, d1, d2, a.t_min ? a.t_min[i] : 0.0, a.t_max ? a.t_max[i] : inf);
  const bool hit = best.tri >= 0;
  if (a.t) a.t[i] = best.t;
  if (a.triangle) a.triangle[i] = best.tri;
  if (a.bary) {
    a.bary[i * 3] = hit ? best.U / best.det : nan;
    a.bary[i * 3 + 1] = hit ? best.V / best.det : nan;
    a.bary[i * 3 + 2] = hit ? best.W / best.det : nan;
  }
}

}  // namespace rnb

#define RNB_API extern "C" __attribute__((visibility("default")))

RNB_API int rnb_mesh_raycast(const double* origins, const double* directions, const double* t_min, const double* t_max,
                             int64_t n_rays, const rnb_mesh_bins* bins, const int64_t* cell_start, const int32_t* entries,
                             int64_t n_entries, const double* corners, int64_t n_triangles, int32_t flags, double* t,
                             int32_t* triangle, double* bary, rnb_stream_t stream) {
  using namespace rnb;
  const char* who = "rnb_mesh_raycast";
  const int64_t N = n_rays;
  RNB_TRY(mesh_count(who, N, "rays"));
  RcArgs a;
  RNB_TRY(mesh_binned(who, bins, cell_start, entries, n_entries, corners, n_triangles, flags, RNB_MESH_BINS_COVER, true, N > 0, &a.mesh));
  if (N == 0) return RNB_OK;
  if (!origins || !directions) RNB_FAIL(RNB_E_NULL, "%s: NULL origins / directions", who);
  if (!t && !triangle && !bary) RNB_FAIL(RNB_E_NULL, "%s: every output is NULL", who);
  a.origins = origins; a.directions = directions; a.t_min = t_min; a.t_max = t_max; a.N = N;
  a.t = t; a.triangle = triangle; a.bary = bary;
  hipLaunchKernelGGL(rc_kernel, dim3((unsigned)((N + kRcThreads - 1) / kRcThreads)), dim3(kRcThreads), 0, (hipStream_t)stream, a);
  RNB_CHECK_LAUNCH();
  return RNB_OK;
}
