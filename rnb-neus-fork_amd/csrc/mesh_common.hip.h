// What the mesh tools share (mesh_clean.hip, mesh_simplify.hip, mesh_eval.hip, mesh_raycast.hip.h, mesh_cull.hip,
// texture_bake.hip): the finiteness predicate, the 31-bit size limit and its checks, the triangle fetch with its index
// guard, the integer mixer, and the grid of the triangle bins with the binned mesh the queries and the ray walk read.
// A file that includes this header must be compiled with -ffp-contract=off: mesh_cell and the grid's magnitude round
// every operation on its own, as the numpy references evaluate them.
#pragma once
#include <math.h>

#include "rnb_internal.h"

namespace rnb {

constexpr int64_t kMeshMax = 2147483647;       // V, T, E and every other count: 31-bit (vertex ids are int32)
constexpr int64_t kMeshMaxCells = 1 << 24;

__host__ __device__ inline bool mesh_finite(double a) { return a == a && a <= 1.7976931348623157e308 && a >= -1.7976931348623157e308; }

// the finaliser of splitmix64 (include/rnbneus.h spells it out for the surface samples)
__device__ inline unsigned long long mesh_mix(unsigned long long z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// the index guard: it stands in front of every use of a triangle's indices as addresses
__device__ inline bool mesh_indices_ok(int a, int b, int c, int64_t V) {
  return !(a < 0 || b < 0 || c < 0 || a >= V || b >= V || c >= V);
}

// the three corners of triangle t, or false: an index outside [0, V) (checked before it is used) or a non-finite coordinate
__device__ inline bool mesh_corners(const double* __restrict__ vertices, int64_t V, const int32_t* __restrict__ tri, int64_t t,
                                    double (&p)[9]) {
  const int a = tri[t * 3], b = tri[t * 3 + 1], c = tri[t * 3 + 2];
  if (!mesh_indices_ok(a, b, c, V)) return false;
  const int idx[3] = {a, b, c};
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const double x = vertices[(int64_t)idx[k] * 3 + d];
      p[k * 3 + d] = x;
      ok = ok && mesh_finite(x);
    }
  return ok;
}

static int mesh_sizes(const char* who, int64_t V, int64_t T) {
  if (V < 0 || T < 0 || V > kMeshMax || T > kMeshMax)
    RNB_FAIL(RNB_E_INVALID, "%s: %lld vertices / %lld triangles outside [0, 2^31 - 1]", who, (long long)V, (long long)T);
  return RNB_OK;
}
// a count of `what` (queries, rays, entries, samples, ...)
static int mesh_count(const char* who, int64_t n, const char* what) {
  if (n < 0 || n > kMeshMax) RNB_FAIL(RNB_E_INVALID, "%s: %lld %s outside [0, 2^31 - 1]", who, (long long)n, what);
  return RNB_OK;
}

// ---- the grid of the triangle bins ------------------------------------------------------------------------------------

struct MeshGrid {
  double o[3];         // origin
  double cell;         // cubic cell size
  int d[3];            // cells per axis
  double mag;          // max |origin| + max dim x cell: the magnitude of every coordinate in the grid's box
};

// what the bound of a cell is good to (mesh_eval.hip shows it): 2^-48 of the grid's magnitude
__host__ __device__ inline double mesh_slack(const MeshGrid& g) { return g.mag * 3.552713678800501e-15; }

// the cell of a coordinate: clamp(floor((x - origin) / cell), 0, dim - 1), monotone in x, NaN -> 0
__device__ inline int mesh_cell(double x, double o, double cell, int dim) {
  const double f = floor((x - o) / cell);
  if (!(f >= 0.0)) return 0;
  if (f >= (double)dim) return dim - 1;
  return (int)f;
}

// the grid of a call, checked: RNB_E_NULL / RNB_E_INVALID before anything else happens
static int mesh_grid_from_bins(const char* who, const rnb_mesh_bins* b, MeshGrid* g, int64_t* n_cells) {
  if (!b) RNB_FAIL(RNB_E_NULL, "%s: NULL bins", who);
  int64_t n = 1;
  double omax = 0.0;
  int dmax = 1;
  for (int d = 0; d < 3; ++d) {
    if (!mesh_finite(b->origin[d])) RNB_FAIL(RNB_E_INVALID, "%s: bins origin is not finite", who);
    if (b->dims[d] < 1 || b->dims[d] > kMeshMaxCells) RNB_FAIL(RNB_E_INVALID, "%s: bins dims[%d] = %d outside [1, 2^24]", who, d, b->dims[d]);
    n *= b->dims[d];
    if (n > kMeshMaxCells) RNB_FAIL(RNB_E_INVALID, "%s: more than 2^24 cells", who);
    g->o[d] = b->origin[d];
    g->d[d] = b->dims[d];
    omax = fabs(b->origin[d]) > omax ? fabs(b->origin[d]) : omax;
    dmax = b->dims[d] > dmax ? b->dims[d] : dmax;
  }
  if (!(b->cell_size > 0.0) || !mesh_finite(b->cell_size)) RNB_FAIL(RNB_E_INVALID, "%s: bins cell_size must be positive and finite", who);
  g->cell = b->cell_size;
  g->mag = omax + (double)dmax * b->cell_size;
  if (!mesh_finite(mesh_slack(*g))) RNB_FAIL(RNB_E_INVALID, "%s: bins origin + dims x cell_size overflows", who);
  *n_cells = n;
  return RNB_OK;
}

// the binned mesh a query or a ray is answered from: the grid, the bins of rnb_mesh_bins_count / _emit and the corners [T,9]
struct BinnedMesh {
  MeshGrid g;
  const unsigned long long* cell_start;
  const int32_t* entries;
  int64_t E;
  const double* corners;
  int64_t T;
};

// The checks every call that reads a binned mesh makes before it launches, and `m` filled from its arguments.  `allowed`:
// the flag bits the call knows; `need_cover`: it walks the grid, so RNB_MESH_BINS_COVER must be among them; `reads`: it
// will read the bins (it has work to do), so with E > 0 the three arrays must be there.
static int mesh_binned(const char* who, const rnb_mesh_bins* bins, const int64_t* cell_start, const int32_t* entries, int64_t E,
                       const double* corners, int64_t T, int32_t flags, int32_t allowed, bool need_cover, bool reads,
                       BinnedMesh* m) {
  if (flags & ~allowed) RNB_FAIL(RNB_E_INVALID, "%s: unknown flag bits 0x%x", who, (unsigned)flags);
  if (need_cover && !(flags & RNB_MESH_BINS_COVER))
    RNB_FAIL(RNB_E_INVALID, "%s: the bins must cover the mesh (RNB_MESH_BINS_COVER): a triangle outside the grid's box sits in a "
                            "boundary cell the walk does not visit", who);
  RNB_TRY(mesh_count(who, T, "triangles"));
  RNB_TRY(mesh_count(who, E, "entries"));
  int64_t n_cells;
  RNB_TRY(mesh_grid_from_bins(who, bins, &m->g, &n_cells));
  if (reads && E > 0 && (!cell_start || !entries || !corners)) RNB_FAIL(RNB_E_NULL, "%s: NULL cell_start / entries / corners", who);
  m->cell_start = (const unsigned long long*)cell_start;
  m->entries = entries;
  m->E = E;
  m->corners = corners;
  m->T = T;
  return RNB_OK;
}

}  // namespace rnb
