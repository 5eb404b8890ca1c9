// Mesh cleanup on the device: connected components of a triangle mesh, per-component statistics, and stable
// compaction to the kept components (rnb_mesh_* in include/rnbneus.h; DESIGN.md "Mesh cleanup").
//
// Two vertices are connected when a triangle names both; components are numbered by their smallest vertex index.
//
//   components  mk_init_kernel        parent[v] = v, referenced[v] = 0
//               mk_union_kernel       one thread per triangle: range check, mark, unite(a, b), unite(b, c)
//               mk_flatten_kernel     parent[v] = root of v (the component's smallest vertex), or -1 when unreferenced
//               flag scan (3 kernels) exclusive scan of "v is a root" -> dense id of every root; C to counts[0]
//               mk_relabel_kernel     labels[v] = dense id of its root
//   statistics  integer atomics only: counts, order-preserving 64-bit keys for the bounding box, and the area as a
//               128-bit fixed-point sum in units of 2^(e_c - 54), e_c the exponent of the component's largest triangle
//               — integer addition is associative, so the sum has the same bits whatever the arrival order
//   compaction  flag scans of "vertex kept" / "triangle kept" (count), then the same flags again with the block
//               offsets: old -> new vertex map, vertices, old indices, remapped triangles (emit); kept = in a kept
//               component (rnb_mesh_compact_*) or by a per-triangle keep (rnb_mesh_compact_triangles_*)
//
// The flag scans are those of scan.hip.h with 32-bit positions: output order = input order (stable), whatever the launch
// geometry.  The index guard and the size checks are those of mesh_common.hip.h, the union-find that of union_find.hip.h.
#include "mesh_common.hip.h"
#include "scan.hip.h"
#include "union_find.hip.h"

namespace rnb {

constexpr int kMkThreads = kScanThreads;   // the block of every kernel here

// ---- components ---------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kMkThreads) void mk_init_kernel(int* __restrict__ parent, uint8_t* __restrict__ ref, int64_t V) {
  const int64_t v = (int64_t)blockIdx.x * kMkThreads + threadIdx.x;
  if (v < V) {
    parent[v] = (int)v;
    ref[v] = 0;
  }
}

// Why this kernel cannot hang, and why its result does not depend on the schedule: union_find.hip.h.
// Every index is range-checked before it is used as an address; a triangle with an index outside [0, V) is skipped and
// raises *bad.
__global__ __launch_bounds__(kMkThreads) void mk_union_kernel(const int32_t* __restrict__ tri, int64_t T, int64_t V,
                                                              int* parent, uint8_t* ref, unsigned long long* bad) {
  const int64_t t = (int64_t)blockIdx.x * kMkThreads + threadIdx.x;
  if (t >= T) return;
  const int a = tri[t * 3], b = tri[t * 3 + 1], c = tri[t * 3 + 2];
  if (!mesh_indices_ok(a, b, c, V)) {
    atomicOr(bad, 1ull);
    return;
  }
  ref[a] = 1; ref[b] = 1; ref[c] = 1;
  uf_unite(parent, a, b);
  uf_unite(parent, b, c);
}

// after the union kernel has finished the forest only gets flatter: parent[v] = its root (its own entry, written by this
// thread alone; a walk of another thread that passes through v reads the old ancestor or the root), -1 when unreferenced
__global__ __launch_bounds__(kMkThreads) void mk_flatten_kernel(int* parent, const uint8_t* __restrict__ ref, int64_t V) {
  const int64_t v = (int64_t)blockIdx.x * kMkThreads + threadIdx.x;
  if (v >= V) return;
  if (!ref[v]) { parent[v] = -1; return; }                  // isolated: no walk passes through it
  const int r = uf_find(parent, (int)v);
  __hip_atomic_store(parent + v, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct RootFlag {
  const int* root;
  __device__ bool operator()(int64_t v) const { return root[v] == (int)v; }
};
struct RankEmit {
  unsigned* rank;
  __device__ void operator()(int64_t v, bool, unsigned pos) const { rank[v] = pos; }
};

__global__ __launch_bounds__(kMkThreads) void mk_relabel_kernel(int* __restrict__ labels, const unsigned* __restrict__ rank,
                                                                int64_t V) {
  const int64_t v = (int64_t)blockIdx.x * kMkThreads + threadIdx.x;
  if (v >= V) return;
  const int r = labels[v];                                  // its root (>= 0: rank[r] is the root's dense id) or -1
  if (r >= 0) labels[v] = (int)rank[r];
}

// ---- statistics ---------------------------------------------------------------------------------------------------

// order-preserving map double -> uint64 (numbers only: NaN is flagged apart) and back
__device__ inline unsigned long long mk_key(double x) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(x);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ inline double mk_unkey(unsigned long long k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

// flag bits per component
enum { MK_NAN_X = 1, MK_NAN_Y = 2, MK_NAN_Z = 4, MK_AREA_NAN = 8, MK_AREA_INF = 16 };

struct StatBufs {
  int64_t C;
  long long* tri_count;           // [C]
  long long* vert_count;          // [C]
  unsigned long long* area;       // [C] outputs used as integers until mk_stats_final_kernel: bits of the largest area
  unsigned long long* bbox_min;   // [C,3] keys
  unsigned long long* bbox_max;   // [C,3] keys
  unsigned* flags;                // [C]
  unsigned long long* lo;         // [C] the fixed-point area sum, low and high word
  unsigned long long* hi;
};

__global__ __launch_bounds__(kMkThreads) void mk_stats_init_kernel(StatBufs s, int with_coords) {
  const int64_t c = (int64_t)blockIdx.x * kMkThreads + threadIdx.x;
  if (c >= s.C) return;
  s.tri_count[c] = 0;
  s.vert_count[c] = 0;
  if (with_coords) {
    s.area[c] = 0;
    for (int d = 0; d < 3; ++d) {
      s.bbox_min[c * 3 + d] = ~0ull;
      s.bbox_max[c * 3 + d] = 0ull;
    }
    s.flags[c] = 0;
    s.lo[c] = 0;
    s.hi[c] = 0;
  }
}

// ---- the three accumulating passes: one kernel template -------------------------------------------------------------
// Same-address atomics serialise in L2, and one big component owns most items — whose indices interleave with those of the
// floaters (marching cubes emits vertices grid line by grid line), so runs of one component are short.  A workgroup
// therefore accumulates its kMkStatItems x 256 items in LDS first: a direct-mapped table of kMkStatSlots components
// (slot = component mod slots, claimed with a compare-and-swap; an item whose slot belongs to another component goes to
// global memory directly), flushed once at the end — a few global atomics per component and workgroup instead of a few
// per item.  Integer min / max / add / or only: the result does not depend on any of this grouping.
// An accumulator type: `flush(bufs, i)` adds it to entry i of bufs with atomics (fields still at their identity are
// skipped), `store` / `load` move it to / from entry i with plain accesses; bufs is the global StatBufs or its LDS twin.
constexpr int kMkStatItems = 16;
constexpr int kMkStatSlots = 64;

struct VertexAcc {            // vertex count, NaN flags and key range per axis
  unsigned long long n = 0;
  unsigned fl = 0;
  unsigned long long kmin[3] = {~0ull, ~0ull, ~0ull}, kmax[3] = {0, 0, 0};
  __device__ void store(const StatBufs& s, int c) const {
    s.vert_count[c] = (long long)n;
    s.flags[c] = fl;
    for (int d = 0; d < 3; ++d) {
      s.bbox_min[c * 3 + d] = kmin[d];
      s.bbox_max[c * 3 + d] = kmax[d];
    }
  }
  __device__ void load(const StatBufs& s, int c) {
    n = (unsigned long long)s.vert_count[c];
    fl = s.flags[c];
    for (int d = 0; d < 3; ++d) {
      kmin[d] = s.bbox_min[c * 3 + d];
      kmax[d] = s.bbox_max[c * 3 + d];
    }
  }
  __device__ void flush(const StatBufs& s, int c) const {
    if (n) atomicAdd((unsigned long long*)(s.vert_count + c), n);
    if (fl) atomicOr(s.flags + c, fl);
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      if (kmin[d] != ~0ull) atomicMin(s.bbox_min + (int64_t)c * 3 + d, kmin[d]);
      if (kmax[d] != 0ull) atomicMax(s.bbox_max + (int64_t)c * 3 + d, kmax[d]);
    }
  }
};
struct VertexItem {
  const int32_t* labels;
  const double* vertices;     // or nullptr: counts only
  int64_t C;
  __device__ int operator()(int64_t v, VertexAcc& a) const {
    const int c = labels[v];
    if (c < 0 || c >= C) return -1;
    a.n = 1;
    if (vertices) {
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        const double x = vertices[v * 3 + d];
        if (x != x) a.fl |= 1u << d;
        else a.kmin[d] = a.kmax[d] = mk_key(x);
      }
    }
    return c;
  }
};

// the component of triangle t (that of its first corner) or -1 for a triangle with an index out of range / no label;
// with coordinates its area 0.5 |(p1 - p0) x (p2 - p0)|
struct TriangleSrc {
  const int32_t* tri;
  const int32_t* labels;
  const double* vertices;     // or nullptr
  int64_t V, C;
  __device__ int operator()(int64_t t, double* area) const {
    const int a = tri[t * 3], b = tri[t * 3 + 1], c = tri[t * 3 + 2];
    if (!mesh_indices_ok(a, b, c, V)) return -1;
    const int l = labels[a];
    if (l < 0 || l >= C) return -1;
    if (vertices) {
      const double* p0 = vertices + (int64_t)a * 3;
      const double* p1 = vertices + (int64_t)b * 3;
      const double* p2 = vertices + (int64_t)c * 3;
      const double ux = p1[0] - p0[0], uy = p1[1] - p0[1], uz = p1[2] - p0[2];
      const double vx = p2[0] - p0[0], vy = p2[1] - p0[1], vz = p2[2] - p0[2];
      const double nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
      *area = 0.5 * sqrt(nx * nx + ny * ny + nz * nz);
    }
    return l;
  }
};

// first triangle pass: triangle counts, and per component the largest finite area (as bits: areas are >= 0) / the
// not-finite flags.  (An area is 0.5 sqrt(..): a number >= 0, +inf or NaN, so the two-sided mesh_finite says what a test
// against the upper bound alone would.)
struct CountAcc {
  unsigned long long n = 0, bits = 0;
  unsigned fl = 0;
  __device__ void store(const StatBufs& s, int c) const {
    s.tri_count[c] = (long long)n;
    s.flags[c] = fl;
    s.area[c] = bits;
  }
  __device__ void load(const StatBufs& s, int c) {
    n = (unsigned long long)s.tri_count[c];
    fl = s.flags[c];
    bits = s.area[c];
  }
  __device__ void flush(const StatBufs& s, int c) const {
    if (n) atomicAdd((unsigned long long*)(s.tri_count + c), n);
    if (fl) atomicOr(s.flags + c, fl);
    if (bits) atomicMax(s.area + c, bits);
  }
};
struct CountItem {
  TriangleSrc src;
  __device__ int operator()(int64_t t, CountAcc& a) const {
    double area = 0.0;
    const int c = src(t, &area);
    if (c < 0) return -1;
    a.n = 1;
    if (src.vertices) {
      if (area != area) a.fl = MK_AREA_NAN;
      else if (!mesh_finite(area)) a.fl = MK_AREA_INF;
      else a.bits = (unsigned long long)__double_as_longlong(area);
    }
    return c;
  }
};

// second triangle pass: every finite area in units of 2^(e_c - 54), e_c = exponent of the component's largest: below 2^55,
// rounded to nearest (an error of at most 2^-55 of the largest area per triangle), added as 128-bit integers
struct AreaAcc {
  unsigned long long lo = 0, hi = 0;
  __device__ void store(const StatBufs& s, int c) const {
    s.lo[c] = lo;
    s.hi[c] = hi;
  }
  __device__ void load(const StatBufs& s, int c) {
    lo = s.lo[c];
    hi = s.hi[c];
  }
  __device__ void flush(const StatBufs& s, int c) const {
    unsigned long long carry = 0;
    if (lo) {
      const unsigned long long old = atomicAdd(s.lo + c, lo);
      carry = old + lo < old ? 1ull : 0ull;
    }
    if (hi + carry) atomicAdd(s.hi + c, hi + carry);
  }
};
struct AreaItem {
  TriangleSrc src;
  const unsigned long long* amax_bits;   // StatBufs::area after the first pass
  __device__ int operator()(int64_t t, AreaAcc& a) const {
    double area = 0.0;
    const int c = src(t, &area);
    if (c < 0) return -1;
    const double amax = __longlong_as_double((long long)amax_bits[c]);
    if (mesh_finite(area) && amax > 0.0) a.lo = (unsigned long long)llrint(ldexp(area, 54 - ilogb(amax)));
    return c;
  }
};

template <class Acc, class Item>
__global__ __launch_bounds__(kMkThreads) void mk_stats_pass_kernel(StatBufs s, Item item, int64_t n) {
  __shared__ int key[kMkStatSlots];                            // component of the slot, -1 = free
  __shared__ long long l_count[kMkStatSlots];
  __shared__ unsigned long long l_area[kMkStatSlots], l_min[kMkStatSlots * 3], l_max[kMkStatSlots * 3], l_lo[kMkStatSlots],
      l_hi[kMkStatSlots];
  __shared__ unsigned l_flags[kMkStatSlots];
  const StatBufs l{kMkStatSlots, l_count, l_count, l_area, l_min, l_max, l_flags, l_lo, l_hi};   // (a pass counts one kind)
  if (threadIdx.x < kMkStatSlots) {
    key[threadIdx.x] = -1;
    Acc().store(l, threadIdx.x);
  }
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * (kMkThreads * kMkStatItems) + threadIdx.x;
  for (int k = 0; k < kMkStatItems; ++k) {
    const int64_t i = base + (int64_t)k * kMkThreads;
    if (i >= n) break;
    Acc one;
    const int c = item(i, one);
    if (c < 0) continue;
    const int slot = c & (kMkStatSlots - 1);
    const int owner = atomicCAS(&key[slot], -1, c);
    if (owner == -1 || owner == c) one.flush(l, slot);
    else one.flush(s, c);
  }
  __syncthreads();
  if (threadIdx.x < kMkStatSlots && key[threadIdx.x] >= 0) {
    Acc sum;
    sum.load(l, threadIdx.x);
    sum.flush(s, key[threadIdx.x]);
  }
}

__global__ __launch_bounds__(kMkThreads) void mk_stats_final_kernel(StatBufs s) {
  const int64_t c = (int64_t)blockIdx.x * kMkThreads + threadIdx.x;
  if (c >= s.C) return;
  const unsigned fl = s.flags[c];
  const double nan = __longlong_as_double(0x7ff8000000000000ll), inf = __longlong_as_double(0x7ff0000000000000ll);
  const double amax = __longlong_as_double((long long)s.area[c]);
  double a = 0.0;
  if (fl & MK_AREA_NAN) a = nan;
  else if (fl & MK_AREA_INF) a = inf;
  else if (amax > 0.0) a = ldexp((double)s.hi[c] * 18446744073709551616.0 + (double)s.lo[c], ilogb(amax) - 54);
  ((double*)s.area)[c] = a;
  for (int d = 0; d < 3; ++d) {
    const bool isnan = (fl >> d) & 1u;
    const unsigned long long kmin = s.bbox_min[c * 3 + d], kmax = s.bbox_max[c * 3 + d];
    ((double*)s.bbox_min)[c * 3 + d] = isnan ? nan : mk_unkey(kmin);
    ((double*)s.bbox_max)[c * 3 + d] = isnan ? nan : mk_unkey(kmax);
  }
}

// ---- compaction ---------------------------------------------------------------------------------------------------

struct VertexKeep {
  const int32_t* labels;
  const uint8_t* keep;
  int64_t C;
  __device__ bool operator()(int64_t v) const {
    const int l = labels[v];
    return l >= 0 && l < C && keep[l] != 0;
  }
};
struct TriangleKeep {
  const int32_t* tri;
  const int32_t* labels;
  const uint8_t* keep;
  int64_t V, C;
  __device__ bool operator()(int64_t t) const {
    const int a = tri[t * 3], b = tri[t * 3 + 1], c = tri[t * 3 + 2];
    if (!mesh_indices_ok(a, b, c, V)) return false;
    const int l = labels[a];
    return l >= 0 && l < C && keep[l] != 0;
  }
};
struct VertexEmit {
  const double* vin;      // or nullptr
  double* vout;
  int64_t* vindex;
  int32_t* newidx;
  int64_t n_out;
  __device__ void operator()(int64_t v, bool fl, unsigned pos) const {
    newidx[v] = fl ? (int32_t)pos : -1;
    if (!fl || (int64_t)pos >= n_out) return;
    vindex[pos] = v;
    if (vin) {
      vout[(int64_t)pos * 3] = vin[v * 3];
      vout[(int64_t)pos * 3 + 1] = vin[v * 3 + 1];
      vout[(int64_t)pos * 3 + 2] = vin[v * 3 + 2];
    }
  }
};
struct TriangleEmit {
  const int32_t* tri;
  const int32_t* newidx;
  int32_t* out;
  int64_t n_out;
  __device__ void operator()(int64_t t, bool fl, unsigned pos) const {
    if (!fl || (int64_t)pos >= n_out) return;                // (fl: the three indices passed the range check)
    out[(int64_t)pos * 3] = newidx[tri[t * 3]];
    out[(int64_t)pos * 3 + 1] = newidx[tri[t * 3 + 1]];
    out[(int64_t)pos * 3 + 2] = newidx[tri[t * 3 + 2]];
  }
};

// compaction by a per-triangle keep (rnb_mesh_compact_triangles_*): a triangle is kept when keep_t says so and its three
// indices are in range; a vertex when a kept triangle names it.  The marks live in the workspace's old -> new map itself:
// zeroed, then 1 for every corner of a kept triangle (plain stores of one value: any order gives the same bytes), read
// by the flag of the vertex scan, and replaced by the new index in the emit, where entry v is read and written by the
// one thread that owns v.
struct KeptTriangle {
  const int32_t* tri;
  const uint8_t* keep_t;
  int64_t V;
  __device__ bool operator()(int64_t t) const {
    if (keep_t[t] == 0) return false;
    const int a = tri[t * 3], b = tri[t * 3 + 1], c = tri[t * 3 + 2];
    return mesh_indices_ok(a, b, c, V);
  }
};
struct MarkedVertex {
  const int32_t* mark;
  __device__ bool operator()(int64_t v) const { return mark[v] != 0; }
};
struct TriangleEmitIndexed {
  TriangleEmit emit;
  int64_t* tindex;
  __device__ void operator()(int64_t t, bool fl, unsigned pos) const {
    emit(t, fl, pos);
    if (fl && (int64_t)pos < emit.n_out) tindex[pos] = t;
  }
};
__global__ __launch_bounds__(kMkThreads) void mk_mark_kernel(KeptTriangle kept, int64_t T, int32_t* mark) {
  const int64_t t = (int64_t)blockIdx.x * kMkThreads + threadIdx.x;
  if (t >= T || !kept(t)) return;
  mark[kept.tri[t * 3]] = 1; mark[kept.tri[t * 3 + 1]] = 1; mark[kept.tri[t * 3 + 2]] = 1;
}

// ---- workspaces: every stage carves from the start of the one workspace -------------------------------------------
struct ComponentsWs { uint8_t* ref; unsigned* rank; unsigned* bsum; };
struct StatsWs { unsigned* flags; unsigned long long* lo; unsigned long long* hi; };
struct CompactWs { int32_t* newidx; unsigned* bsum_v; unsigned* bsum_t; };

static ComponentsWs carve_components(Carver& c, int64_t V) {
  ComponentsWs w;
  w.ref = c.take<uint8_t>(V);
  w.rank = c.take<unsigned>(V);
  w.bsum = c.take<unsigned>(scan_pad64(scan_blocks(V)));
  return w;
}
static StatsWs carve_stats(Carver& c, int64_t C) {
  StatsWs w;
  w.flags = c.take<unsigned>(C);
  w.lo = c.take<unsigned long long>(C);
  w.hi = c.take<unsigned long long>(C);
  return w;
}
static CompactWs carve_compact(Carver& c, int64_t V, int64_t T) {
  CompactWs w;
  w.newidx = c.take<int32_t>(V);
  w.bsum_v = c.take<unsigned>(scan_pad64(scan_blocks(V)));
  w.bsum_t = c.take<unsigned>(scan_pad64(scan_blocks(T)));
  return w;
}

static unsigned mk_grid(int64_t n) { return (unsigned)((n + kMkThreads - 1) / kMkThreads); }
static unsigned mk_stat_grid(int64_t n) { return (unsigned)((n + kMkThreads * kMkStatItems - 1) / (kMkThreads * kMkStatItems)); }

}  // namespace rnb

#define RNB_API extern "C" __attribute__((visibility("default")))

RNB_API int rnb_mesh_clean_workspace_bytes(int64_t n_vertices, int64_t n_triangles, int64_t* bytes) {
  using namespace rnb;
  if (!bytes) RNB_FAIL(RNB_E_NULL, "rnb_mesh_clean_workspace_bytes: NULL");
  RNB_TRY(mesh_sizes("rnb_mesh_clean_workspace_bytes", n_vertices, n_triangles));
  Carver a(nullptr, 0), b(nullptr, 0), c(nullptr, 0);
  carve_components(a, n_vertices);
  carve_stats(b, n_vertices);             // at most one component per vertex
  carve_compact(c, n_vertices, n_triangles);
  size_t m = a.off > b.off ? a.off : b.off;
  *bytes = (int64_t)(m > c.off ? m : c.off);
  return RNB_OK;
}

RNB_API int rnb_mesh_components(const int32_t* triangles, int64_t n_triangles, int64_t n_vertices, void* workspace,
                                size_t workspace_bytes, int32_t* labels, int64_t* counts, rnb_stream_t stream) {
  using namespace rnb;
  const int64_t T = n_triangles, V = n_vertices;
  RNB_TRY(mesh_sizes("rnb_mesh_components", V, T));
  if (!counts || (T > 0 && !triangles) || (V > 0 && !labels)) RNB_FAIL(RNB_E_NULL, "rnb_mesh_components: NULL triangles / labels / counts");
  if (V > 0 && !workspace) RNB_FAIL(RNB_E_NULL, "rnb_mesh_components: NULL workspace");
  Carver cv(workspace, workspace_bytes);
  const ComponentsWs w = carve_components(cv, V);
  if (V > 0 && !cv.ok) RNB_FAIL(RNB_E_WORKSPACE, "rnb_mesh_components: workspace %zu < %zu bytes", workspace_bytes, cv.off);
  hipStream_t s = (hipStream_t)stream;
  RNB_CHECK_HIP(hipMemsetAsync(counts, 0, 2 * sizeof(int64_t), s));
  if (V == 0) return RNB_OK;              // no vertex: no component; any triangle would be out of range
  hipLaunchKernelGGL(mk_init_kernel, dim3(mk_grid(V)), dim3(kMkThreads), 0, s, labels, w.ref, V);
  RNB_CHECK_LAUNCH();
  if (T > 0) {
    hipLaunchKernelGGL(mk_union_kernel, dim3(mk_grid(T)), dim3(kMkThreads), 0, s, triangles, T, V, labels, w.ref,
                       (unsigned long long*)(counts + 1));
    RNB_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(mk_flatten_kernel, dim3(mk_grid(V)), dim3(kMkThreads), 0, s, labels, w.ref, V);
  RNB_CHECK_LAUNCH();
  const int64_t nb = scan_blocks(V);
  const RootFlag flag{labels};
  hipLaunchKernelGGL((scan_sum_kernel<unsigned, RootFlag>), dim3((unsigned)nb), dim3(kMkThreads), 0, s, flag, V, w.bsum);
  RNB_CHECK_LAUNCH();
  hipLaunchKernelGGL(scan_block_sums_kernel<unsigned>, dim3(1), dim3(1024), 0, s, w.bsum, nb, (unsigned*)nullptr, (int64_t)0, 1, counts);
  RNB_CHECK_LAUNCH();
  hipLaunchKernelGGL((scan_emit_kernel<unsigned, RootFlag, RankEmit>), dim3((unsigned)nb), dim3(kMkThreads), 0, s, flag,
                     RankEmit{w.rank}, V, w.bsum);
  RNB_CHECK_LAUNCH();
  hipLaunchKernelGGL(mk_relabel_kernel, dim3(mk_grid(V)), dim3(kMkThreads), 0, s, labels, w.rank, V);
  RNB_CHECK_LAUNCH();
  return RNB_OK;
}

RNB_API int rnb_mesh_component_stats(const int32_t* triangles, int64_t n_triangles, const double* vertices,
                                     int64_t n_vertices, const int32_t* labels, int64_t n_components, void* workspace,
                                     size_t workspace_bytes, int64_t* tri_count, int64_t* vert_count, double* area,
                                     double* bbox_min, double* bbox_max, rnb_stream_t stream) {
  using namespace rnb;
  const int64_t T = n_triangles, V = n_vertices, C = n_components;
  RNB_TRY(mesh_sizes("rnb_mesh_component_stats", V, T));
  if (C < 0 || C > V) RNB_FAIL(RNB_E_INVALID, "rnb_mesh_component_stats: %lld components of %lld vertices", (long long)C, (long long)V);
  if (C == 0) return RNB_OK;
  if (!labels || !tri_count || !vert_count || (T > 0 && !triangles))
    RNB_FAIL(RNB_E_NULL, "rnb_mesh_component_stats: NULL triangles / labels / counts");
  if (vertices && (!area || !bbox_min || !bbox_max))
    RNB_FAIL(RNB_E_NULL, "rnb_mesh_component_stats: coordinates given but no area / bbox output");
  StatBufs sb{C, (long long*)tri_count, (long long*)vert_count, (unsigned long long*)area, (unsigned long long*)bbox_min,
              (unsigned long long*)bbox_max, nullptr, nullptr, nullptr};
  if (vertices) {
    if (!workspace) RNB_FAIL(RNB_E_NULL, "rnb_mesh_component_stats: NULL workspace");
    Carver cv(workspace, workspace_bytes);
    const StatsWs w = carve_stats(cv, C);
    if (!cv.ok) RNB_FAIL(RNB_E_WORKSPACE, "rnb_mesh_component_stats: workspace %zu < %zu bytes", workspace_bytes, cv.off);
    sb.flags = w.flags; sb.lo = w.lo; sb.hi = w.hi;
  }
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(mk_stats_init_kernel, dim3(mk_grid(C)), dim3(kMkThreads), 0, s, sb, vertices ? 1 : 0);
  RNB_CHECK_LAUNCH();
  const TriangleSrc src{triangles, labels, vertices, V, C};
  hipLaunchKernelGGL((mk_stats_pass_kernel<VertexAcc, VertexItem>), dim3(mk_stat_grid(V)), dim3(kMkThreads), 0, s, sb,
                     VertexItem{labels, vertices, C}, V);
  RNB_CHECK_LAUNCH();
  if (T > 0) {
    hipLaunchKernelGGL((mk_stats_pass_kernel<CountAcc, CountItem>), dim3(mk_stat_grid(T)), dim3(kMkThreads), 0, s, sb,
                       CountItem{src}, T);
    RNB_CHECK_LAUNCH();
    if (vertices) {
      hipLaunchKernelGGL((mk_stats_pass_kernel<AreaAcc, AreaItem>), dim3(mk_stat_grid(T)), dim3(kMkThreads), 0, s, sb,
                         AreaItem{src, sb.area}, T);
      RNB_CHECK_LAUNCH();
    }
  }
  if (vertices) {
    hipLaunchKernelGGL(mk_stats_final_kernel, dim3(mk_grid(C)), dim3(kMkThreads), 0, s, sb);
    RNB_CHECK_LAUNCH();
  }
  return RNB_OK;
}

namespace rnb {
static int mk_compact_check(const char* who, const int32_t* triangles, int64_t T, int64_t V, const int32_t* labels,
                            const uint8_t* keep, int64_t C, void* workspace, size_t workspace_bytes, CompactWs* w) {
  RNB_TRY(mesh_sizes(who, V, T));
  if (C < 0 || C > V) RNB_FAIL(RNB_E_INVALID, "%s: %lld components of %lld vertices", who, (long long)C, (long long)V);
  if ((T > 0 && !triangles) || (V > 0 && !labels) || (C > 0 && !keep)) RNB_FAIL(RNB_E_NULL, "%s: NULL triangles / labels / keep", who);
  Carver cv(workspace, workspace_bytes);
  *w = carve_compact(cv, V, T);
  if (cv.off > 0 && !workspace) RNB_FAIL(RNB_E_NULL, "%s: NULL workspace", who);
  if (!cv.ok) RNB_FAIL(RNB_E_WORKSPACE, "%s: workspace %zu < %zu bytes", who, workspace_bytes, cv.off);
  return RNB_OK;
}
}  // namespace rnb

RNB_API int rnb_mesh_compact_count(const int32_t* triangles, int64_t n_triangles, int64_t n_vertices, const int32_t* labels,
                                   const uint8_t* keep, int64_t n_components, void* workspace, size_t workspace_bytes,
                                   int64_t* counts, rnb_stream_t stream) {
  using namespace rnb;
  const int64_t T = n_triangles, V = n_vertices, C = n_components;
  CompactWs w;
  RNB_TRY(mk_compact_check("rnb_mesh_compact_count", triangles, T, V, labels, keep, C, workspace, workspace_bytes, &w));
  if (!counts) RNB_FAIL(RNB_E_NULL, "rnb_mesh_compact_count: NULL counts");
  hipStream_t s = (hipStream_t)stream;
  const int64_t nbv = scan_blocks(V), nbt = scan_blocks(T);
  if (V > 0) {
    hipLaunchKernelGGL((scan_sum_kernel<unsigned, VertexKeep>), dim3((unsigned)nbv), dim3(kMkThreads), 0, s,
                       VertexKeep{labels, keep, C}, V, w.bsum_v);
    RNB_CHECK_LAUNCH();
  }
  if (T > 0) {
    hipLaunchKernelGGL((scan_sum_kernel<unsigned, TriangleKeep>), dim3((unsigned)nbt), dim3(kMkThreads), 0, s,
                       TriangleKeep{triangles, labels, keep, V, C}, T, w.bsum_t);
    RNB_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(scan_block_sums_kernel<unsigned>, dim3(1), dim3(1024), 0, s, w.bsum_v, nbv, w.bsum_t, nbt, 2, counts);
  RNB_CHECK_LAUNCH();
  return RNB_OK;
}

RNB_API int rnb_mesh_compact_emit(const int32_t* triangles, int64_t n_triangles, const double* vertices, int64_t n_vertices,
                                  const int32_t* labels, const uint8_t* keep, int64_t n_components, void* workspace,
                                  size_t workspace_bytes, int64_t n_vertices_out, int64_t n_triangles_out,
                                  double* vertices_out, int32_t* triangles_out, int64_t* vertex_index,
                                  rnb_stream_t stream) {
  using namespace rnb;
  const int64_t T = n_triangles, V = n_vertices, C = n_components;
  CompactWs w;
  RNB_TRY(mk_compact_check("rnb_mesh_compact_emit", triangles, T, V, labels, keep, C, workspace, workspace_bytes, &w));
  if (n_vertices_out < 0 || n_vertices_out > V || n_triangles_out < 0 || n_triangles_out > T)
    RNB_FAIL(RNB_E_INVALID, "rnb_mesh_compact_emit: %lld of %lld vertices / %lld of %lld triangles", (long long)n_vertices_out,
             (long long)V, (long long)n_triangles_out, (long long)T);
  if ((n_vertices_out > 0 && (!vertex_index || (vertices && !vertices_out))) || (n_triangles_out > 0 && !triangles_out))
    RNB_FAIL(RNB_E_NULL, "rnb_mesh_compact_emit: NULL output");
  hipStream_t s = (hipStream_t)stream;
  if (V > 0) {
    hipLaunchKernelGGL((scan_emit_kernel<unsigned, VertexKeep, VertexEmit>), dim3((unsigned)scan_blocks(V)), dim3(kMkThreads), 0, s,
                       VertexKeep{labels, keep, C}, VertexEmit{vertices, vertices_out, vertex_index, w.newidx, n_vertices_out},
                       V, w.bsum_v);
    RNB_CHECK_LAUNCH();
  }
  if (T > 0) {
    hipLaunchKernelGGL((scan_emit_kernel<unsigned, TriangleKeep, TriangleEmit>), dim3((unsigned)scan_blocks(T)), dim3(kMkThreads), 0, s,
                       TriangleKeep{triangles, labels, keep, V, C},
                       TriangleEmit{triangles, w.newidx, triangles_out, n_triangles_out}, T, w.bsum_t);
    RNB_CHECK_LAUNCH();
  }
  return RNB_OK;
}

namespace rnb {
static int mk_compact_triangles_check(const char* who, const int32_t* triangles, int64_t T, int64_t V, const uint8_t* keep_t,
                                      void* workspace, size_t workspace_bytes, CompactWs* w) {
  RNB_TRY(mesh_sizes(who, V, T));
  if (T > 0 && (!triangles || !keep_t)) RNB_FAIL(RNB_E_NULL, "%s: NULL triangles / keep_t", who);
  Carver cv(workspace, workspace_bytes);
  *w = carve_compact(cv, V, T);
  if (cv.off > 0 && !workspace) RNB_FAIL(RNB_E_NULL, "%s: NULL workspace", who);
  if (!cv.ok) RNB_FAIL(RNB_E_WORKSPACE, "%s: workspace %zu < %zu bytes", who, workspace_bytes, cv.off);
  return RNB_OK;
}

// the marks of the vertices a kept triangle names, in w.newidx
static int mk_mark_vertices(const KeptTriangle& kept, int64_t T, int64_t V, const CompactWs& w, hipStream_t s) {
  if (V > 0) RNB_CHECK_HIP(hipMemsetAsync(w.newidx, 0, (size_t)V * sizeof(int32_t), s));
  if (V > 0 && T > 0) {
    hipLaunchKernelGGL(mk_mark_kernel, dim3(mk_grid(T)), dim3(kMkThreads), 0, s, kept, T, w.newidx);
    RNB_CHECK_LAUNCH();
  }
  return RNB_OK;
}
}  // namespace rnb

RNB_API int rnb_mesh_compact_triangles_count(const int32_t* triangles, int64_t n_triangles, int64_t n_vertices,
                                             const uint8_t* keep_t, void* workspace, size_t workspace_bytes, int64_t* counts,
                                             rnb_stream_t stream) {
  using namespace rnb;
  const char* who = "rnb_mesh_compact_triangles_count";
  const int64_t T = n_triangles, V = n_vertices;
  CompactWs w;
  RNB_TRY(mk_compact_triangles_check(who, triangles, T, V, keep_t, workspace, workspace_bytes, &w));
  if (!counts) RNB_FAIL(RNB_E_NULL, "%s: NULL counts", who);
  hipStream_t s = (hipStream_t)stream;
  const KeptTriangle kept{triangles, keep_t, V};
  RNB_TRY(mk_mark_vertices(kept, T, V, w, s));
  const int64_t nbv = scan_blocks(V), nbt = scan_blocks(T);
  if (V > 0) {
    hipLaunchKernelGGL((scan_sum_kernel<unsigned, MarkedVertex>), dim3((unsigned)nbv), dim3(kMkThreads), 0, s, MarkedVertex{w.newidx}, V,
                       w.bsum_v);
    RNB_CHECK_LAUNCH();
  }
  if (T > 0) {
    hipLaunchKernelGGL((scan_sum_kernel<unsigned, KeptTriangle>), dim3((unsigned)nbt), dim3(kMkThreads), 0, s, kept, T, w.bsum_t);
    RNB_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(scan_block_sums_kernel<unsigned>, dim3(1), dim3(1024), 0, s, w.bsum_v, nbv, w.bsum_t, nbt, 2, counts);
  RNB_CHECK_LAUNCH();
  return RNB_OK;
}

RNB_API int rnb_mesh_compact_triangles_emit(const int32_t* triangles, int64_t n_triangles, const double* vertices,
                                            int64_t n_vertices, const uint8_t* keep_t, void* workspace, size_t workspace_bytes,
                                            int64_t n_vertices_out, int64_t n_triangles_out, double* vertices_out,
                                            int32_t* triangles_out, int64_t* vertex_index, int64_t* triangle_index,
                                            rnb_stream_t stream) {
  using namespace rnb;
  const char* who = "rnb_mesh_compact_triangles_emit";
  const int64_t T = n_triangles, V = n_vertices;
  CompactWs w;
  RNB_TRY(mk_compact_triangles_check(who, triangles, T, V, keep_t, workspace, workspace_bytes, &w));
  if (n_vertices_out < 0 || n_vertices_out > V || n_triangles_out < 0 || n_triangles_out > T)
    RNB_FAIL(RNB_E_INVALID, "%s: %lld of %lld vertices / %lld of %lld triangles", who, (long long)n_vertices_out, (long long)V,
             (long long)n_triangles_out, (long long)T);
  if ((n_vertices_out > 0 && (!vertex_index || (vertices && !vertices_out))) ||
      (n_triangles_out > 0 && (!triangles_out || !triangle_index)))
    RNB_FAIL(RNB_E_NULL, "%s: NULL output", who);
  hipStream_t s = (hipStream_t)stream;
  const KeptTriangle kept{triangles, keep_t, V};
  RNB_TRY(mk_mark_vertices(kept, T, V, w, s));       // (the count's marks again: the emit needs only its block sums)
  if (V > 0) {
    hipLaunchKernelGGL((scan_emit_kernel<unsigned, MarkedVertex, VertexEmit>), dim3((unsigned)scan_blocks(V)), dim3(kMkThreads), 0, s,
                       MarkedVertex{w.newidx}, VertexEmit{vertices, vertices_out, vertex_index, w.newidx, n_vertices_out}, V,
                       w.bsum_v);
    RNB_CHECK_LAUNCH();
  }
  if (T > 0) {
    hipLaunchKernelGGL((scan_emit_kernel<unsigned, KeptTriangle, TriangleEmitIndexed>), dim3((unsigned)scan_blocks(T)), dim3(kMkThreads), 0,
                       s, kept, TriangleEmitIndexed{TriangleEmit{triangles, w.newidx, triangles_out, n_triangles_out}, triangle_index},
                       T, w.bsum_t);
    RNB_CHECK_LAUNCH();
  }
  return RNB_OK;
}
