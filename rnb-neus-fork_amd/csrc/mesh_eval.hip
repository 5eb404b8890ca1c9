// Mesh evaluation on the device: triangle bins, exact closest-point-on-mesh queries, area-weighted surface samples
// (rnb_mesh_bins_*, rnb_mesh_closest_points, rnb_mesh_sample_* in include/rnbneus.h; DESIGN.md "Mesh evaluation").
//
//   bins     me_bin_kernel<false>   one thread per triangle: range / finiteness check, +1 on every cell its box overlaps
//            scan (3 kernels)       exclusive 64-bit scan of the n_cells + 1 counts in place, an instance of the weight
//                                   scans of scan.hip.h -> cell_start, E to counts[0]
//            me_bin_kernel<true>    the same walk again: entries[cell_start[c] + cursor[c]++] = t, and corners[t] (9 doubles)
//   query    me_closest_kernel      one lane per query: Chebyshev shells of cells around the query's (clamped) cell
//   samples  me_area_kernel         A_t and the sum of each tile of 1024 triangles
//            me_area_blocks_kernel  exclusive scan of the tile sums, one workgroup, one serial chain
//            me_area_apply_kernel   C_t = tile offset + scan inside the tile
//            me_sample_kernel       one thread per sample: binary search of C, the integer mixer, the point
//
// Integer atomics on the cell counters and cursors only; no floating-point atomics anywhere.  The file is compiled with
// -ffp-contract=off: every product and sum rounds on its own, as the numpy reference evaluates them.
//
// THE CELL OF A COORDINATE is mesh_cell(x) = clamp(floor((x - origin) / cell), 0, dim - 1) of mesh_common.hip.h:
// subtraction, division by a positive number, floor and clamp are all monotone, so mesh_cell is monotone in x.  A triangle
// is entered into the cells [mesh_cell(lo), mesh_cell(hi)] of its box per axis.  What the query relies on
// (k = 1 .. dim - 1, plane(k) = origin + k cell):
//     mesh_cell(x) >= k    =>  x >= plane(k) - slack          mesh_cell(x) <= k - 1  =>  x <= plane(k) + slack
// with slack = mesh_slack(grid) = 2^-48 (max |origin| + max dim x cell): floor(fl(fl(x - o) / cell)) >= k gives
// x - o >= k cell (1 - 2^-52)^2,
// and fl(o + fl(k cell)) is within 2^-52 (|o| + 2 k cell) of o + k cell — a few 2^-52 of the grid's magnitude, against 16.
// Clamping does not touch either implication (k >= 1 on the left, k - 1 <= dim - 2 on the right).
//
// WHY THE SHELL SEARCH IS EXACT.  After the shells 0 .. R around the query's cell q, every triangle entered into a cell of
// the block [q - R, q + R]^3 has been evaluated.  A triangle that was not has, on some axis, its whole box on one side of
// the block: every one of its points has mesh_cell >= q + R + 1 or <= q - R - 1 there, hence lies beyond plane(q + R + 1) or
// plane(q - R) up to slack, hence is at least  lower = min over the sides that still have cells of (|plane - p| - slack)
// away from the query p (times 1 - 2^-48 for the rounding of the difference and of the square).  The search stops when
// lower^2 > best, strictly: a triangle at exactly the best distance is always evaluated, so the tie rule (smaller index)
// sees it.  For a query outside the box q is the clamped cell, the missing sides are the ones the query is beyond, and the
// same argument holds with the same planes.  A side without cells contributes nothing; with no side left all cells are done.
// With RNB_MESH_BINS_COVER (the count found every binned triangle inside the grid's box, up to slack) the bound is taken
// per face in squares: a point beyond the face of axis d AND inside the box is at least the gap to that plane away along
// d and at least the query's gap to the box along the other two axes — for a query outside the box by D the faces across
// D then cost D^2 each, and the search ends after ~sqrt(2 D h) / h shells instead of D / h.
//
// WHY IT CANNOT HANG.  R runs over 0 .. max(dims) - 1, the cell loops over the block clipped to the grid, the entry loop
// over [cell_start[c], cell_start[c + 1]) clipped to [0, E): every trip count is bounded by the grid dims and E before the
// loop starts, none depends on the data converging.  A query with a non-finite coordinate leaves before the loops.
#include "mesh_common.hip.h"
#include "scan.hip.h"

namespace rnb {

constexpr int kMeThreads = 256;
constexpr int kMeItems = kScanItems;          // the area scan walks the tiles of the integer scans
constexpr int kMeTile = kScanTile;

// the far side of the grid's box on axis d: the same expression wherever it is needed
__device__ inline double me_box_hi(const MeshGrid& g, int d) { return g.o[d] + (double)g.d[d] * g.cell; }

// ---- bins -----------------------------------------------------------------------------------------------------------

template <bool kEmit>
__global__ __launch_bounds__(kMeThreads) void me_bin_kernel(const double* __restrict__ vertices, int64_t V,
                                                            const int32_t* __restrict__ tri, int64_t T, MeshGrid g,
                                                            unsigned long long* cell_start, unsigned* cursor, int64_t E,
                                                            int32_t* __restrict__ entries, double* __restrict__ corners,
                                                            unsigned long long* skipped) {
  const int64_t t = (int64_t)blockIdx.x * kMeThreads + threadIdx.x;
  if (t >= T) return;
  double p[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  const bool ok = mesh_corners(vertices, V, tri, t, p);
  if (kEmit) {
#pragma unroll
    for (int k = 0; k < 9; ++k) corners[t * 9 + k] = ok ? p[k] : 0.0;
  }
  if (!ok) {
    if (!kEmit) atomicOr(skipped, 1ull);
    return;
  }
  int lo[3], hi[3];
  bool inside = true;
  const double slack = mesh_slack(g);
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const double mn = fmin(p[d], fmin(p[3 + d], p[6 + d])), mx = fmax(p[d], fmax(p[3 + d], p[6 + d]));
    lo[d] = mesh_cell(mn, g.o[d], g.cell, g.d[d]);
    hi[d] = mesh_cell(mx, g.o[d], g.cell, g.d[d]);
    inside = inside && mn >= g.o[d] - slack && mx <= me_box_hi(g, d) + slack;
  }
  if (!kEmit && !inside) atomicOr(skipped, 2ull);            // binned all the same, into the boundary cells
  for (int cz = lo[2]; cz <= hi[2]; ++cz)
    for (int cy = lo[1]; cy <= hi[1]; ++cy)
      for (int cx = lo[0]; cx <= hi[0]; ++cx) {
        const int64_t c = ((int64_t)cz * g.d[1] + cy) * g.d[0] + cx;
        if (!kEmit) {
          atomicAdd(cell_start + c, 1ull);
        } else {
          const unsigned long long pos = cell_start[c] + atomicAdd(cursor + c, 1u);
          if (pos < cell_start[c + 1] && pos < (unsigned long long)E) entries[pos] = (int32_t)t;
        }
      }
}

// the scan of the per-cell counts in place: the emit writes the running sum over the count its weight read
struct CellCount {
  const unsigned long long* a;
  __device__ unsigned long long operator()(int64_t c) const { return a[c]; }
};
struct CellStart {
  unsigned long long* a;
  __device__ void operator()(int64_t c, unsigned long long, unsigned long long pos) const { a[c] = pos; }
};

// ---- closest point --------------------------------------------------------------------------------------------------

__device__ inline double me_dot(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
__device__ inline void me_cross(const double* a, const double* b, double* c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

// squared distance of p to the segment [a, b] (a point when a == b) and the closest point
__device__ inline double me_segment(const double* p, const double* a, const double* b, double* q) {
  double ab[3], ap[3], r[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    ab[d] = b[d] - a[d];
    ap[d] = p[d] - a[d];
  }
  const double dd = me_dot(ab, ab);
  double t = 0.0;
  if (dd > 0.0) {
    t = me_dot(ap, ab) / dd;
    t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
  }
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    q[d] = a[d] + t * ab[d];
    r[d] = p[d] - q[d];
  }
  return me_dot(r, r);
}

// Squared distance of p to the triangle (a, b, c) and the closest point: tests/mesh_distance_ref.py, operation for
// operation.  Where the triangle has a normal and the projection q = a + wb (b - a) + wc (c - a) falls inside it,
// |p - q|^2 (an error of the weights moves q inside the plane only: second order in d2); then the three clamped edge
// segments ab, bc, ca; the first strict minimum in that order wins.  A pure function of the four points.
__device__ inline double me_point_triangle(const double* p, const double* tri, double* q) {
  const double *a = tri, *b = tri + 3, *c = tri + 6;
  double best = __longlong_as_double(0x7ff0000000000000ll);
  q[0] = q[1] = q[2] = __longlong_as_double(0x7ff8000000000000ll);
  double ab[3], ac[3], ap[3], n[3], x[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    ab[d] = b[d] - a[d];
    ac[d] = c[d] - a[d];
    ap[d] = p[d] - a[d];
  }
  me_cross(ab, ac, n);
  const double nn = me_dot(n, n);
  if (nn > 0.0) {
    me_cross(ap, ac, x);
    const double wb = me_dot(x, n) / nn;
    me_cross(ab, ap, x);
    const double wc = me_dot(x, n) / nn;
    const double wa = (1.0 - wb) - wc;
    if (wa >= 0.0 && wb >= 0.0 && wc >= 0.0) {
      double r[3];
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        q[d] = (a[d] + wb * ab[d]) + wc * ac[d];
        r[d] = p[d] - q[d];
      }
      best = me_dot(r, r);
    }
  }
  double qs[3];
  double d2 = me_segment(p, a, b, qs);
  if (d2 < best) { best = d2; q[0] = qs[0]; q[1] = qs[1]; q[2] = qs[2]; }
  d2 = me_segment(p, b, c, qs);
  if (d2 < best) { best = d2; q[0] = qs[0]; q[1] = qs[1]; q[2] = qs[2]; }
  d2 = me_segment(p, c, a, qs);
  if (d2 < best) { best = d2; q[0] = qs[0]; q[1] = qs[1]; q[2] = qs[2]; }
  return best;
}

struct MeQuery {
  const double* queries;
  int64_t N;
  BinnedMesh m;
  double* dist2;
  double* closest;
  int32_t* triangle;
  double slack;        // mesh_slack of the grid
  int covers;          // RNB_MESH_BINS_COVER: every binned triangle lies inside the grid's box
};

struct MeBest {
  double d2;
  double q[3];
  int t;
};

// a gap as the bounds may use it: less the slack, less 2^-48 of itself (the rounding of the difference, of the square
// and of the sums it enters), squared; 0 when nothing is left
__device__ inline double me_gap2(double gap, double slack) {
  const double e = (gap - slack) * (1.0 - 3.552713678800501e-15 /* 2^-48 */);
  return e > 0.0 ? e * e : 0.0;
}

__device__ inline void me_visit(const BinnedMesh& a, const double* p, int64_t c, MeBest& best) {
  unsigned long long s = a.cell_start[c], e = a.cell_start[c + 1];
  if (e > (unsigned long long)a.E) e = (unsigned long long)a.E;
  for (; s < e; ++s) {
    const int t = a.entries[s];
    if (t < 0 || t >= a.T) continue;
    double tri[9], q[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) tri[k] = a.corners[(int64_t)t * 9 + k];
    const double d2 = me_point_triangle(p, tri, q);
    if (d2 < best.d2 || (d2 == best.d2 && t < best.t)) {
      best.d2 = d2;
      best.t = t;
      best.q[0] = q[0]; best.q[1] = q[1]; best.q[2] = q[2];
    }
  }
}

__global__ __launch_bounds__(kMeThreads) void me_closest_kernel(MeQuery a) {
  const int64_t i = (int64_t)blockIdx.x * kMeThreads + threadIdx.x;
  if (i >= a.N) return;
  const double nan = __longlong_as_double(0x7ff8000000000000ll), inf = __longlong_as_double(0x7ff0000000000000ll);
  const double p[3] = {a.queries[i * 3], a.queries[i * 3 + 1], a.queries[i * 3 + 2]};
  MeBest best;
  best.d2 = inf;
  best.q[0] = best.q[1] = best.q[2] = nan;
  best.t = -1;
  const MeshGrid& g = a.m.g;
  const double slack = a.slack;
  if (!(mesh_finite(p[0]) && mesh_finite(p[1]) && mesh_finite(p[2]))) {
    best.d2 = nan;
  } else if (a.m.E > 0) {
    int qc[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) qc[d] = mesh_cell(p[d], g.o[d], g.cell, g.d[d]);
    double box2[3] = {0.0, 0.0, 0.0};
    if (a.covers) {
#pragma unroll
      for (int d = 0; d < 3; ++d) box2[d] = me_gap2(fmax(g.o[d] - p[d], p[d] - me_box_hi(g, d)), slack);
    }
    const int max_r = max(g.d[0], max(g.d[1], g.d[2])) - 1;
    for (int R = 0; R <= max_r; ++R) {
      const int x0 = max(qc[0] - R, 0), x1 = min(qc[0] + R, g.d[0] - 1);
      const int y0 = max(qc[1] - R, 0), y1 = min(qc[1] + R, g.d[1] - 1);
      const int z0 = max(qc[2] - R, 0), z1 = min(qc[2] + R, g.d[2] - 1);
      for (int cz = z0; cz <= z1; ++cz)
        for (int cy = y0; cy <= y1; ++cy) {
          const int64_t row = ((int64_t)cz * g.d[1] + cy) * g.d[0];
          if (cz - qc[2] == R || qc[2] - cz == R || cy - qc[1] == R || qc[1] - cy == R) {
            for (int cx = x0; cx <= x1; ++cx) me_visit(a.m, p, row + cx, best);
          } else {                                           // (R > 0 here) the two x faces of the shell
            if (qc[0] - R >= 0) me_visit(a.m, p, row + qc[0] - R, best);
            if (qc[0] + R <= g.d[0] - 1) me_visit(a.m, p, row + qc[0] + R, best);
          }
        }
      // the square of what every triangle outside the block [qc - R, qc + R] is at least away: per face with cells
      // behind it, the gap to its plane and, across it, the gaps to the box (box2: zeros unless the grid covers the mesh)
      double lower2 = inf;
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        const double across = box2[(d + 1) % 3] + box2[(d + 2) % 3];
        const int kh = qc[d] + R + 1, kl = qc[d] - R;
        if (kh <= g.d[d] - 1) lower2 = fmin(lower2, me_gap2((g.o[d] + (double)kh * g.cell) - p[d], slack) + across);
        if (kl >= 1) lower2 = fmin(lower2, me_gap2(p[d] - (g.o[d] + (double)kl * g.cell), slack) + across);
      }
      if (lower2 == inf) break;                              // no face has cells behind it: every cell is done
      if (lower2 > best.d2) break;
    }
  }
  if (a.dist2) a.dist2[i] = best.d2;
  if (a.triangle) a.triangle[i] = best.t;
  if (a.closest) {
    a.closest[i * 3] = best.q[0];
    a.closest[i * 3 + 1] = best.q[1];
    a.closest[i * 3 + 2] = best.q[2];
  }
}

// ---- surface samples ------------------------------------------------------------------------------------------------
// C_t = inclusive sum of the areas, evaluated as ONE chain per level: inside a thread item by item, across the 256 threads
// of a tile by thread 0 (off_{j+1} = off_j + total_j), across tiles by thread 0 of one workgroup.  The last C of a thread,
// tile or mesh is therefore the very number the next one starts from: C is non-decreasing, C_t == C_{t-1} exactly for a
// zero-area triangle (it can never be "the first t with C_t > u"), C_{T-1} == A, and the bits are the same on every run.

__device__ inline double me_area_of(const double* __restrict__ vertices, int64_t V, const int32_t* __restrict__ tri, int64_t t) {
  double p[9];
  if (!mesh_corners(vertices, V, tri, t, p)) return 0.0;
  const double u[3] = {p[3] - p[0], p[4] - p[1], p[5] - p[2]}, v[3] = {p[6] - p[0], p[7] - p[1], p[8] - p[2]};
  double n[3];
  me_cross(u, v, n);
  return 0.5 * sqrt(me_dot(n, n));
}

// the tile's inclusive sums (relative to the tile) of the items `v` of this thread into `inc`, its total to *total
__device__ inline void me_tile_chain(const double (&v)[kMeItems], double (&inc)[kMeItems], double* total, double* lds /* [257] */) {
  double run = 0.0;
#pragma unroll
  for (int k = 0; k < kMeItems; ++k) {
    run = run + v[k];
    inc[k] = run;
  }
  lds[threadIdx.x] = run;
  __syncthreads();
  if (threadIdx.x == 0) {
    double off = 0.0;
    for (int j = 0; j < kMeThreads; ++j) {
      const double tj = lds[j];
      lds[j] = off;
      off = off + tj;
    }
    lds[kMeThreads] = off;
  }
  __syncthreads();
  const double off = lds[threadIdx.x];
#pragma unroll
  for (int k = 0; k < kMeItems; ++k) inc[k] = off + inc[k];
  *total = lds[kMeThreads];
  __syncthreads();
}

__global__ __launch_bounds__(kMeThreads) void me_area_kernel(const double* __restrict__ vertices, int64_t V,
                                                             const int32_t* __restrict__ tri, int64_t T,
                                                             double* __restrict__ cum, double* __restrict__ bsum) {
  __shared__ double lds[kMeThreads + 1];
  const int64_t i0 = (int64_t)blockIdx.x * kMeTile + (int64_t)threadIdx.x * kMeItems;
  double v[kMeItems], inc[kMeItems], total;
#pragma unroll
  for (int k = 0; k < kMeItems; ++k) {
    v[k] = i0 + k < T ? me_area_of(vertices, V, tri, i0 + k) : 0.0;
    if (i0 + k < T) cum[i0 + k] = v[k];
  }
  me_tile_chain(v, inc, &total, lds);
  if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

__global__ __launch_bounds__(1024) void me_area_blocks_kernel(double* __restrict__ bsum, int64_t nblocks, double* __restrict__ total) {
  __shared__ double lds[1024];
  __shared__ double carry;
  if (threadIdx.x == 0) carry = 0.0;
  __syncthreads();
  for (int64_t base = 0; base < nblocks; base += 1024) {
    const int64_t i = base + threadIdx.x;
    lds[threadIdx.x] = i < nblocks ? bsum[i] : 0.0;
    __syncthreads();
    if (threadIdx.x == 0) {
      double off = carry;
      for (int j = 0; j < 1024; ++j) {
        const double tj = lds[j];
        lds[j] = off;
        off = off + tj;
      }
      carry = off;
    }
    __syncthreads();
    if (i < nblocks) bsum[i] = lds[threadIdx.x];
    __syncthreads();
  }
  if (threadIdx.x == 0) *total = carry;
}

__global__ __launch_bounds__(kMeThreads) void me_area_apply_kernel(double* __restrict__ cum, int64_t T,
                                                                   const double* __restrict__ boff) {
  __shared__ double lds[kMeThreads + 1];
  const int64_t i0 = (int64_t)blockIdx.x * kMeTile + (int64_t)threadIdx.x * kMeItems;
  double v[kMeItems], inc[kMeItems], total;
#pragma unroll
  for (int k = 0; k < kMeItems; ++k) v[k] = i0 + k < T ? cum[i0 + k] : 0.0;
  me_tile_chain(v, inc, &total, lds);
  const double off = boff[blockIdx.x];
#pragma unroll
  for (int k = 0; k < kMeItems; ++k)
    if (i0 + k < T) cum[i0 + k] = off + inc[k];
}

__device__ inline double me_unit(unsigned long long z) { return (double)(z >> 11) * 1.1102230246251565e-16 /* 2^-53 */; }

struct MeSample {
  const double* vertices;
  int64_t V;
  const int32_t* tri;
  int64_t T;
  const double* cum;
  const double* total;
  int64_t n;
  unsigned long long seed;
  double* points;
  int32_t* triangle;
  double* bary;
  double* normal;
};

__global__ __launch_bounds__(kMeThreads) void me_sample_kernel(MeSample a) {
  const int64_t k = (int64_t)blockIdx.x * kMeThreads + threadIdx.x;
  if (k >= a.n) return;
  const double A = *a.total;
  int64_t t = -1;
  double w[3] = {0, 0, 0}, pt[3] = {0, 0, 0}, nr[3] = {0, 0, 0};
  if (A > 0.0 && mesh_finite(A)) {
    const unsigned long long s = mesh_mix(a.seed);
    const double xi = me_unit(s);
    double u = (((double)k + xi) * A) / (double)a.n;
    const double below = __longlong_as_double(__double_as_longlong(A) - 1);   // the largest double under A = C_{T-1}
    if (!(u <= below)) u = below;
    // the first t with C_t > u: at most 32 halvings of [0, T)
    int64_t lo = 0, hi = a.T - 1;                                             // C_hi > u holds: C_{T-1} = A > below
    for (int step = 0; step < 32 && lo < hi; ++step) {
      const int64_t mid = lo + (hi - lo) / 2;
      if (a.cum[mid] > u) hi = mid;
      else lo = mid + 1;
    }
    t = lo;
    double p[9];
    if (t >= 0 && t < a.T && mesh_corners(a.vertices, a.V, a.tri, t, p)) {
      double r1 = me_unit(mesh_mix(s ^ (2ull * (unsigned long long)k)));
      double r2 = me_unit(mesh_mix(s ^ (2ull * (unsigned long long)k + 1ull)));
      if (1.0 - r1 < r2) {                                                    // r1 + r2 > 1, decided exactly
        r1 = 1.0 - r1;
        r2 = 1.0 - r2;
      }
      w[0] = (1.0 - r1) - r2;
      w[1] = r1;
      w[2] = r2;
      double e1[3], e2[3];
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        pt[d] = (w[0] * p[d] + w[1] * p[3 + d]) + w[2] * p[6 + d];
        e1[d] = p[3 + d] - p[d];
        e2[d] = p[6 + d] - p[d];
      }
      me_cross(e1, e2, nr);
      const double len = sqrt(me_dot(nr, nr));
      const bool ok = len > 0.0 && mesh_finite(len);
#pragma unroll
      for (int d = 0; d < 3; ++d) nr[d] = ok ? nr[d] / len : 0.0;
    } else {
      t = -1;
    }
  }
  if (a.triangle) a.triangle[k] = (int32_t)t;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    if (a.points) a.points[k * 3 + d] = pt[d];
    if (a.bary) a.bary[k * 3 + d] = w[d];
    if (a.normal) a.normal[k * 3 + d] = nr[d];
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------

static unsigned me_grid(int64_t n) { return (unsigned)((n + kMeThreads - 1) / kMeThreads); }

struct BinsWs { unsigned* cursor; unsigned long long* bsum; };
static BinsWs carve_bins(Carver& c, int64_t n_cells) {
  BinsWs w;
  w.cursor = c.take<unsigned>(n_cells);
  w.bsum = c.take<unsigned long long>(scan_blocks(n_cells + 1));
  return w;
}

static int me_bins_check(const char* who, const double* vertices, int64_t V, const int32_t* triangles, int64_t T,
                         const rnb_mesh_bins* bins, void* workspace, size_t workspace_bytes, const void* cell_start, MeshGrid* g,
                         int64_t* n_cells, BinsWs* w) {
  RNB_TRY(mesh_sizes(who, V, T));
  RNB_TRY(mesh_grid_from_bins(who, bins, g, n_cells));
  if ((T > 0 && !triangles) || (V > 0 && T > 0 && !vertices) || !cell_start) RNB_FAIL(RNB_E_NULL, "%s: NULL vertices / triangles / cell_start", who);
  if (!workspace) RNB_FAIL(RNB_E_NULL, "%s: NULL workspace", who);
  Carver cv(workspace, workspace_bytes);
  *w = carve_bins(cv, *n_cells);
  if (!cv.ok) RNB_FAIL(RNB_E_WORKSPACE, "%s: workspace %zu < %zu bytes", who, workspace_bytes, cv.off);
  return RNB_OK;
}

struct SampleWs { double* bsum; };
static SampleWs carve_sample(Carver& c, int64_t T) {
  SampleWs w;
  w.bsum = c.take<double>(scan_blocks(T));
  return w;
}

}  // namespace rnb

#define RNB_API extern "C" __attribute__((visibility("default")))

RNB_API int rnb_mesh_bins_workspace_bytes(int64_t n_cells, int64_t* bytes) {
  using namespace rnb;
  if (!bytes) RNB_FAIL(RNB_E_NULL, "rnb_mesh_bins_workspace_bytes: NULL");
  if (n_cells < 1 || n_cells > kMeshMaxCells) RNB_FAIL(RNB_E_INVALID, "rnb_mesh_bins_workspace_bytes: %lld cells outside [1, 2^24]", (long long)n_cells);
  Carver c(nullptr, 0);
  carve_bins(c, n_cells);
  *bytes = (int64_t)c.off;
  return RNB_OK;
}

RNB_API int rnb_mesh_bins_count(const double* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles,
                                const rnb_mesh_bins* bins, void* workspace, size_t workspace_bytes, int64_t* cell_start,
                                int64_t* counts, rnb_stream_t stream) {
  using namespace rnb;
  const int64_t V = n_vertices, T = n_triangles;
  MeshGrid g;
  int64_t n_cells;
  BinsWs w;
  RNB_TRY(me_bins_check("rnb_mesh_bins_count", vertices, V, triangles, T, bins, workspace, workspace_bytes, cell_start, &g, &n_cells, &w));
  if (!counts) RNB_FAIL(RNB_E_NULL, "rnb_mesh_bins_count: NULL counts");
  hipStream_t s = (hipStream_t)stream;
  unsigned long long* cs = (unsigned long long*)cell_start;
  RNB_CHECK_HIP(hipMemsetAsync(cs, 0, (size_t)(n_cells + 1) * sizeof(int64_t), s));
  RNB_CHECK_HIP(hipMemsetAsync(counts, 0, 2 * sizeof(int64_t), s));
  if (T == 0) return RNB_OK;                // no triangle: every cell empty, E = 0
  hipLaunchKernelGGL(me_bin_kernel<false>, dim3(me_grid(T)), dim3(kMeThreads), 0, s, vertices, V, triangles, T, g, cs,
                     (unsigned*)nullptr, (int64_t)0, (int32_t*)nullptr, (double*)nullptr, (unsigned long long*)(counts + 1));
  RNB_CHECK_LAUNCH();
  const int64_t n = n_cells + 1, nb = scan_blocks(n);
  using u64 = unsigned long long;
  hipLaunchKernelGGL((scan_sum_kernel<u64, CellCount>), dim3((unsigned)nb), dim3(kScanThreads), 0, s, CellCount{cs}, n, w.bsum);
  RNB_CHECK_LAUNCH();
  hipLaunchKernelGGL(scan_block_sums_kernel<u64>, dim3(1), dim3(1024), 0, s, w.bsum, nb, (u64*)nullptr, (int64_t)0, 1, counts);
  RNB_CHECK_LAUNCH();
  hipLaunchKernelGGL((scan_emit_kernel<u64, CellCount, CellStart>), dim3((unsigned)nb), dim3(kScanThreads), 0, s, CellCount{cs},
                     CellStart{cs}, n, (const u64*)w.bsum);
  RNB_CHECK_LAUNCH();
  return RNB_OK;
}

RNB_API int rnb_mesh_bins_emit(const double* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles,
                               const rnb_mesh_bins* bins, void* workspace, size_t workspace_bytes, const int64_t* cell_start,
                               int64_t n_entries, int32_t* entries, double* corners, rnb_stream_t stream) {
  using namespace rnb;
  const int64_t V = n_vertices, T = n_triangles, E = n_entries;
  MeshGrid g;
  int64_t n_cells;
  BinsWs w;
  RNB_TRY(me_bins_check("rnb_mesh_bins_emit", vertices, V, triangles, T, bins, workspace, workspace_bytes, cell_start, &g, &n_cells, &w));
  RNB_TRY(mesh_count("rnb_mesh_bins_emit", E, "entries"));
  if ((E > 0 && !entries) || (T > 0 && !corners)) RNB_FAIL(RNB_E_NULL, "rnb_mesh_bins_emit: NULL entries / corners");
  if (T == 0) return RNB_OK;
  hipStream_t s = (hipStream_t)stream;
  RNB_CHECK_HIP(hipMemsetAsync(w.cursor, 0, (size_t)n_cells * sizeof(unsigned), s));
  hipLaunchKernelGGL(me_bin_kernel<true>, dim3(me_grid(T)), dim3(kMeThreads), 0, s, vertices, V, triangles, T, g,
                     (unsigned long long*)cell_start, w.cursor, E, entries, corners, (unsigned long long*)nullptr);
  RNB_CHECK_LAUNCH();
  return RNB_OK;
}

RNB_API int rnb_mesh_closest_points(const double* queries, int64_t n_queries, const rnb_mesh_bins* bins,
                                    const int64_t* cell_start, const int32_t* entries, int64_t n_entries, const double* corners,
                                    int64_t n_triangles, int32_t flags, double* dist2, double* closest, int32_t* triangle,
                                    rnb_stream_t stream) {
  using namespace rnb;
  const char* who = "rnb_mesh_closest_points";
  const int64_t N = n_queries;
  RNB_TRY(mesh_count(who, N, "queries"));
  MeQuery a;
  RNB_TRY(mesh_binned(who, bins, cell_start, entries, n_entries, corners, n_triangles, flags, RNB_MESH_BINS_COVER, false, N > 0, &a.m));
  if (N == 0) return RNB_OK;
  if (!queries) RNB_FAIL(RNB_E_NULL, "%s: NULL queries", who);
  if (!dist2 && !closest && !triangle) RNB_FAIL(RNB_E_NULL, "%s: every output is NULL", who);
  a.queries = queries; a.N = N; a.dist2 = dist2; a.closest = closest; a.triangle = triangle;
  a.slack = mesh_slack(a.m.g);
  a.covers = (flags & RNB_MESH_BINS_COVER) ? 1 : 0;
  hipLaunchKernelGGL(me_closest_kernel, dim3(me_grid(N)), dim3(kMeThreads), 0, (hipStream_t)stream, a);
  RNB_CHECK_LAUNCH();
  return RNB_OK;
}

RNB_API int rnb_mesh_sample_workspace_bytes(int64_t n_triangles, int64_t* bytes) {
  using namespace rnb;
  if (!bytes) RNB_FAIL(RNB_E_NULL, "rnb_mesh_sample_workspace_bytes: NULL");
  RNB_TRY(mesh_sizes("rnb_mesh_sample_workspace_bytes", 0, n_triangles));
  Carver c(nullptr, 0);
  carve_sample(c, n_triangles);
  *bytes = (int64_t)c.off;
  return RNB_OK;
}

RNB_API int rnb_mesh_sample_areas(const double* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles,
                                  void* workspace, size_t workspace_bytes, double* cum_area, double* total, rnb_stream_t stream) {
  using namespace rnb;
  const int64_t V = n_vertices, T = n_triangles;
  RNB_TRY(mesh_sizes("rnb_mesh_sample_areas", V, T));
  if (!total || (T > 0 && (!triangles || !cum_area)) || (V > 0 && T > 0 && !vertices))
    RNB_FAIL(RNB_E_NULL, "rnb_mesh_sample_areas: NULL vertices / triangles / cum_area / total");
  Carver cv(workspace, workspace_bytes);
  const SampleWs w = carve_sample(cv, T);
  if (T > 0 && !workspace) RNB_FAIL(RNB_E_NULL, "rnb_mesh_sample_areas: NULL workspace");
  if (!cv.ok) RNB_FAIL(RNB_E_WORKSPACE, "rnb_mesh_sample_areas: workspace %zu < %zu bytes", workspace_bytes, cv.off);
  hipStream_t s = (hipStream_t)stream;
  if (T == 0) {
    RNB_CHECK_HIP(hipMemsetAsync(total, 0, sizeof(double), s));
    return RNB_OK;
  }
  const int64_t nb = scan_blocks(T);
  hipLaunchKernelGGL(me_area_kernel, dim3((unsigned)nb), dim3(kMeThreads), 0, s, vertices, V, triangles, T, cum_area, w.bsum);
  RNB_CHECK_LAUNCH();
  hipLaunchKernelGGL(me_area_blocks_kernel, dim3(1), dim3(1024), 0, s, w.bsum, nb, total);
  RNB_CHECK_LAUNCH();
  hipLaunchKernelGGL(me_area_apply_kernel, dim3((unsigned)nb), dim3(kMeThreads), 0, s, cum_area, T, w.bsum);
  RNB_CHECK_LAUNCH();
  return RNB_OK;
}

RNB_API int rnb_mesh_sample_surface(const double* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles,
                                    const double* cum_area, const double* total, int64_t n_samples, int64_t seed, double* points,
                                    int32_t* triangle, double* bary, double* normal, rnb_stream_t stream) {
  using namespace rnb;
  const int64_t V = n_vertices, T = n_triangles, n = n_samples;
  RNB_TRY(mesh_sizes("rnb_mesh_sample_surface", V, T));
  RNB_TRY(mesh_count("rnb_mesh_sample_surface", n, "samples"));
  if (n > 0 && T == 0) RNB_FAIL(RNB_E_INVALID, "rnb_mesh_sample_surface: samples of a mesh without triangles");
  if (n == 0) return RNB_OK;
  if (!vertices || !triangles || !cum_area || !total) RNB_FAIL(RNB_E_NULL, "rnb_mesh_sample_surface: NULL vertices / triangles / cum_area / total");
  if (!points && !triangle && !bary && !normal) RNB_FAIL(RNB_E_NULL, "rnb_mesh_sample_surface: every output is NULL");
  const MeSample a{vertices, V, triangles, T, cum_area, total, n, (unsigned long long)seed, points, triangle, bary, normal};
  hipLaunchKernelGGL(me_sample_kernel, dim3(me_grid(n)), dim3(kMeThreads), 0, (hipStream_t)stream, a);
  RNB_CHECK_LAUNCH();
  return RNB_OK;
}
