// Mesh culling by the cameras: for every (point, camera) pair whether the point is in the frame, in the mask, and
// unoccluded, and per point how many cameras gave each answer (rnb_mesh_view_votes in include/rnbneus.h, which defines
// the status op for op; DESIGN.md "Mesh culling").  One kernel, cv_kernel, one launch for all C cameras, one lane per
// pair.  Compiled with -ffp-contract=off: the projection rounds every product and sum on its own, as
// tests/mesh_cull_ref.py evaluates it, and the segment eye -> point is cast by rc_first_hit of mesh_raycast.hip.h, the
// walk and pair test of rnb_mesh_raycast: status SEEN / OCCLUDED is what `MeshIndex.visible` answers, bit for bit.
//
// LANES.  Workgroup b of the nbp x C virtual workgroups (nbp = ceil(N / 256)) takes camera c = b / nbp and the points
// [256 (b mod nbp), + 256): the 64 lanes of a wavefront are consecutive points of ONE camera.  Marching cubes emits
// vertices grid line by grid line, so the lanes' segments start at one eye and end in neighbouring cells: they walk the
// same layers and read the same bins.  The launch holds at most 2^20 workgroups, each looping over b with the stride of
// the grid; no result depends on that number.
//
// COUNTS.  counts [N,4] is zeroed by the call, then every pair adds 1 to counts[i][status] with an integer atomic:
// integer addition is associative, so the counts have the same bits whatever the order and whatever the grid.  No
// floating-point atomic anywhere.
//
// BOUNDS.  The pixel is formed only after a and b passed 0 <= a < W, 0 <= b < H in fp64 (a NaN fails both), so
// (int)floor(a) is in [0, W) and the mask index ((c H + py) W + px) inside [0, C H W); every trip count of the walk is
// fixed by the grid dims and E (mesh_raycast.hip.h), that of the workgroup loop by N and C.
#include "mesh_raycast.hip.h"

namespace rnb {

constexpr int kCvThreads = 256;
constexpr int64_t kCvMaxBlocks = 1 << 20;

struct CvArgs {
  const double* points;       // [N,3]
  const double* proj;         // [C,3,4]
  const double* eyes;         // [C,3]
  const uint8_t* masks;       // [C,H,W] or nullptr
  int64_t N, C;
  int H, W;
  BinnedMesh mesh;
  double t_seen;              // 1 - rel_tol
  int occlusion;
  int32_t* counts;            // [N,4]
  uint8_t* status;            // [C,N] or nullptr
  int64_t nbp, total;         // workgroups per camera, nbp x C
};

__global__ __launch_bounds__(kCvThreads) void cv_kernel(CvArgs a) {
  for (int64_t b = blockIdx.x; b < a.total; b += gridDim.x) {
    const int64_t c = b / a.nbp;
    const int64_t i = (b - c * a.nbp) * kCvThreads + threadIdx.x;
    if (i >= a.N) continue;
    const double X = a.points[i * 3], Y = a.points[i * 3 + 1], Z = a.points[i * 3 + 2];
    const double* __restrict__ P = a.proj + c * 12;
    int st = RNB_CULL_OUT_OF_FRAME;
    if (mesh_finite(X) && mesh_finite(Y) && mesh_finite(Z)) {
      const double x = ((P[0] * X + P[1] * Y) + P[2] * Z) + P[3];
      const double y = ((P[4] * X + P[5] * Y) + P[6] * Z) + P[7];
      const double w = ((P[8] * X + P[9] * Y) + P[10] * Z) + P[11];
      if (mesh_finite(w) && w > 0.0) {
        const double u = x / w, v = y / w;
        const double pa = u + 0.5, pb = v + 0.5;
        if (pa >= 0.0 && pa < (double)a.W && pb >= 0.0 && pb < (double)a.H) {
          const int px = (int)floor(pa), py = (int)floor(pb);
          if (a.masks && a.masks[(c * a.H + py) * a.W + px] == 0) {
            st = RNB_CULL_OUTSIDE_MASK;
          } else if (!a.occlusion) {
            st = RNB_CULL_SEEN;
          } else {
            const double e0 = a.eyes[c * 3], e1 = a.eyes[c * 3 + 1], e2 = a.eyes[c * 3 + 2];
            const RcBest best = rc_first_hit(a.mesh, e0, e1, e2, X - e0, Y - e1, Z - e2, 0.0, 1.0);
            st = best.t >= a.t_seen ? RNB_CULL_SEEN : RNB_CULL_OCCLUDED;      // +inf: nothing met; NaN: occluded
          }
        }
      }
    }
    atomicAdd(a.counts + i * 4 + st, 1);
    if (a.status) a.status[c * a.N + i] = (uint8_t)st;
  }
}

}  // namespace rnb

#define RNB_API extern "C" __attribute__((visibility("default")))

RNB_API int rnb_mesh_view_votes(const double* points, int64_t n_points, const double* projections, const double* eyes,
                                int64_t n_cameras, const uint8_t* masks, int32_t height, int32_t width,
                                const rnb_mesh_bins* bins, const int64_t* cell_start, const int32_t* entries,
                                int64_t n_entries, const double* corners, int64_t n_triangles, double rel_tol, int32_t flags,
                                int32_t* counts, uint8_t* status, rnb_stream_t stream) {
  using namespace rnb;
  const char* who = "rnb_mesh_view_votes";
  const int64_t N = n_points, C = n_cameras;
  RNB_TRY(mesh_count(who, N, "points"));
  RNB_TRY(mesh_count(who, C, "cameras"));
  if (height < 0 || width < 0 || (masks && (height < 1 || width < 1)))
    RNB_FAIL(RNB_E_INVALID, "%s: a frame of %d x %d pixels%s", who, height, width, masks ? " with masks given" : "");
  if (!(rel_tol >= 0.0 && rel_tol < 1.0)) RNB_FAIL(RNB_E_INVALID, "%s: rel_tol = %g outside [0, 1)", who, rel_tol);
  CvArgs a;
  const bool occlusion = !(flags & RNB_CULL_NO_OCCLUSION);
  RNB_TRY(mesh_binned(who, bins, cell_start, entries, n_entries, corners, n_triangles, flags,
                      RNB_MESH_BINS_COVER | RNB_CULL_NO_OCCLUSION, true, occlusion && N > 0 && C > 0, &a.mesh));
  if (N == 0) return RNB_OK;
  if (!counts) RNB_FAIL(RNB_E_NULL, "%s: NULL counts", who);
  if (C > 0) {
    if (!points || !projections) RNB_FAIL(RNB_E_NULL, "%s: NULL points / projections", who);
    if (occlusion && !eyes) RNB_FAIL(RNB_E_NULL, "%s: NULL eyes", who);
  }
  hipStream_t s = (hipStream_t)stream;
  RNB_CHECK_HIP(hipMemsetAsync(counts, 0, (size_t)N * 4 * sizeof(int32_t), s));
  if (C == 0) return RNB_OK;
  a.points = points; a.proj = projections; a.eyes = eyes; a.masks = masks; a.N = N; a.C = C; a.H = height; a.W = width;
  a.t_seen = 1.0 - rel_tol;
  a.occlusion = occlusion ? 1 : 0;
  a.counts = counts; a.status = status;
  a.nbp = (N + kCvThreads - 1) / kCvThreads;
  a.total = a.nbp * C;
  const int64_t grid = a.total < kCvMaxBlocks ? a.total : kCvMaxBlocks;
  hipLaunchKernelGGL(cv_kernel, dim3((unsigned)grid), dim3(kCvThreads), 0, s, a);
  RNB_CHECK_LAUNCH();
  return RNB_OK;
}
