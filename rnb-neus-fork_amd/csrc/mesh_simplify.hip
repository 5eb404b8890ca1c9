// Mesh simplification on the device: vertex clustering on a uniform grid (Rossignac-Borrel), the representative of a
// cluster being one of its own vertices (rnb_mesh_simplify_* in include/rnbneus.h, which has the definition op for op;
// DESIGN.md "Mesh simplification"; tests/mesh_simplify_ref.py is the same definition in numpy).
//
//   count  sp_origin_kernel      (default origin only) per-axis minimum of the all-finite vertices, as ordered keys
//          sp_vertex_key_kernel  key[v] = packed cell of v, or all ones when v is not usable; per-vertex state reset
//          sp_mark_kernel        one thread per triangle: range check, usable check, referenced[corner] = 1
//          sp_cluster_kernel     referenced vertices enter the cell table; slot[v] = the slot of v's cell
//          sp_sum_kernel         leader[v] = what the slot holds at the end (the cell's smallest vertex); n and the three
//                                sums of q = floor(f 2^32) per cluster with 64-bit integer adds
//          sp_d2_kernel          d2 of every member to its cluster's mean; atomicMin on its bits
//          sp_rep_kernel         atomicMin of the index among the members whose d2 equals the minimum
//          sp_triple_kernel      per triangle the sorted leader triple (or "none": invalid / degenerate)
//          sp_dedupe_kernel      the non-degenerate triangles enter the triple table
//          sp_survive_kernel    a triangle survives when its slot holds its own index; its three clusters are used
//          flag scans            "v leads a used cluster" and "t survives" -> V', T' and the block offsets
//   emit   the same two flags with the block offsets (scan.hip.h): cluster -> output index, representatives'
//          coordinates and indices, remapped triangles, input index of every surviving triangle, cluster of every vertex
//   The index guard, the finiteness predicate, the mixer of the two tables and the size check: mesh_common.hip.h.
//
// Integer atomics only (compare-and-swap, min, add, or): every result is a function of the input alone, whatever the
// schedule, and equals the numpy reference bit for bit.  The file is compiled with -ffp-contract=off: every product and
// sum of the definition is rounded on its own.
//
// THE TWO TABLES: WHY AN INSERTION ENDS, AND WHY A KEY ENDS IN EXACTLY ONE SLOT.
// A table is an array of `cap` 32-bit slots, cap a power of two >= 2 x (number of items), every slot empty (all ones) at
// the start.  A slot holds an ITEM INDEX (a vertex, or a triangle), never a key: the key of the occupant is read from
// key[] / triple[], arrays a previous kernel wrote and this kernel never writes, so no thread ever reads data another
// thread of the same launch is still writing.  An item with key k walks the slots h(k), h(k) + 1, ... (mod cap) and at
// each slot does one compare-and-swap(empty -> my index):
//   - it succeeded: the slot is mine, stop;
//   - the occupant has key k: atomicMin(slot, my index), stop;
//   - otherwise go to the next slot.
// Invariants.  (1) A slot never becomes empty again, and every index ever stored in it has the key of the first one: the
// compare-and-swap only fills an empty slot, the atomicMin only stores an index whose key was compared equal to the
// occupant's.  So "the key of slot s" is fixed from the moment s is filled.  (2) Let s be the slot where the FIRST item
// of key k stopped.  Every slot on the walk before s was filled with a key other than k when that item passed it, and by
// (1) stays so: every later item of key k passes them too and arrives at s, where it finds key k (or won the
// compare-and-swap itself — then the other finds k there).  So all items of one key stop at one slot, and since every one
// of them either filled it or applied atomicMin, the slot ends holding the smallest index of the key: the cluster's
// leader, or the first of a family of duplicate triangles.
// Termination.  Fewer than cap / 2 + 1 slots are ever filled (one per distinct key), so every walk meets an empty slot
// or its own key after at most cap steps; the loop is bounded by cap all the same, and a walk that used them up would set
// bit 2 of counts[4] and return.  No thread waits for another: there is no spin, no lock.
// The loop itself is mesh_table_insert of mesh_table.hip.h, which mesh_topology.hip uses for its edge table.
#include "mesh_common.hip.h"
#include "mesh_table.hip.h"
#include "scan.hip.h"

namespace rnb {

constexpr unsigned kSpEmpty = kTabEmpty;
constexpr unsigned long long kSpNoKey = ~0ull;
constexpr int kMkThreads = kScanThreads;   // the block of every kernel here
enum { SP_BAD_INDEX = 1, SP_BAD_VERTEX = 2, SP_TABLE_FULL = 4 };

struct SpGrid {
  double origin[3];
  double h;
  const double* dev_origin;   // the default origin, computed on the device (then origin[] is unused)
  __device__ double org(int d) const { return dev_origin ? dev_origin[d] : origin[d]; }
};

struct SpWs {
  unsigned long long* okey;     // [3]   ordered keys of the default origin
  double* origin;               // [3]   the default origin
  unsigned long long* key;      // [V]   cell key, all ones = not usable
  uint8_t* ref;                 // [V]   referenced by a valid triangle
  uint8_t* used;                // [V]   (by leader) the cluster is named by a surviving triangle
  int32_t* lead;                // [V]   slot of the vertex's cell, then the leader of its cluster; -1 = takes no part
  unsigned* n;                  // [V]   (by leader) members
  unsigned long long* sum;      // [V,3] (by leader) sums of q
  unsigned long long* d2;       // [V]   (by leader) smallest d2, as bits
  unsigned* rep;                // [V]   (by leader) the representative
  int32_t* newidx;              // [V]   (by leader) output index of the cluster
  int32_t* triple;              // [T,3] sorted leaders, -1 = none
  unsigned* tslot;              // [T]   slot of the triangle's triple
  unsigned* vtab;               // [capV]
  unsigned* ttab;               // [capT]
  unsigned* bsum_v;
  unsigned* bsum_t;
  uint64_t cap_v, cap_t;
};

static uint64_t sp_capacity(int64_t n) { return mesh_table_capacity(n); }

static SpWs sp_carve(Carver& c, int64_t V, int64_t T) {
  SpWs w;
  w.cap_v = sp_capacity(V);
  w.cap_t = sp_capacity(T);
  w.okey = c.take<unsigned long long>(3);
  w.origin = c.take<double>(3);
  w.key = c.take<unsigned long long>(V);
  w.ref = c.take<uint8_t>(V);
  w.used = c.take<uint8_t>(V);
  w.lead = c.take<int32_t>(V);
  w.n = c.take<unsigned>(V);
  w.sum = c.take<unsigned long long>(3 * V);
  w.d2 = c.take<unsigned long long>(V);
  w.rep = c.take<unsigned>(V);
  w.newidx = c.take<int32_t>(V);
  w.triple = c.take<int32_t>(3 * T);
  w.tslot = c.take<unsigned>(T);
  w.vtab = c.take<unsigned>((int64_t)w.cap_v);
  w.ttab = c.take<unsigned>((int64_t)w.cap_t);
  w.bsum_v = c.take<unsigned>(scan_pad64(scan_blocks(V)));
  w.bsum_t = c.take<unsigned>(scan_pad64(scan_blocks(T)));
  return w;
}

// order-preserving map double -> uint64 (numbers only) and back
__device__ inline unsigned long long sp_okey(double x) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(x);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ inline double sp_unokey(unsigned long long k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

// one add of the number of lanes with `pred` per wave
__device__ inline void sp_wave_count(long long* counter, bool pred) {
  const unsigned long long m = __ballot(pred);
  if (m && (threadIdx.x & 63) == (unsigned)(__ffsll((long long)m) - 1))
    atomicAdd((unsigned long long*)counter, (unsigned long long)__popcll(m));
}

// Cell of one coordinate: u = (x - origin) / h, i = floor(u), f = u - i.  False when i is outside [-2^20, 2^20) (which
// covers a u that overflowed or is NaN).
__device__ inline bool sp_cell(double x, double o, double h, int* i, double* f) {
  const double d = x - o;
  const double u = d / h;
  const double fl = floor(u);
  if (!(fl >= -1048576.0 && fl < 1048576.0)) return false;
  *i = (int)fl;
  *f = u - fl;
  return true;
}

__global__ __launch_bounds__(kMkThreads) void sp_origin_init_kernel(unsigned long long* okey) {
  if (threadIdx.x < 3) okey[threadIdx.x] = ~0ull;
}

// per-axis minimum over the vertices whose three coordinates are finite: block minimum in LDS, one atomicMin per block
__global__ __launch_bounds__(kMkThreads) void sp_origin_kernel(const double* __restrict__ vertices, int64_t V,
                                                               unsigned long long* okey) {
  __shared__ unsigned long long lmin[3];
  if (threadIdx.x < 3) lmin[threadIdx.x] = ~0ull;
  __syncthreads();
  const int64_t v = (int64_t)blockIdx.x * kMkThreads + threadIdx.x;
  if (v < V) {
    const double x = vertices[v * 3], y = vertices[v * 3 + 1], z = vertices[v * 3 + 2];
    if (mesh_finite(x) && mesh_finite(y) && mesh_finite(z)) {
      atomicMin(&lmin[0], sp_okey(x));
      atomicMin(&lmin[1], sp_okey(y));
      atomicMin(&lmin[2], sp_okey(z));
    }
  }
  __syncthreads();
  if (threadIdx.x < 3 && lmin[threadIdx.x] != ~0ull) atomicMin(okey + threadIdx.x, lmin[threadIdx.x]);
}

__global__ __launch_bounds__(kMkThreads) void sp_origin_final_kernel(const unsigned long long* okey, double* origin) {
  if (threadIdx.x < 3) origin[threadIdx.x] = okey[threadIdx.x] == ~0ull ? 0.0 : sp_unokey(okey[threadIdx.x]);
}

__global__ __launch_bounds__(kMkThreads) void sp_fill_kernel(unsigned* __restrict__ p, uint64_t n, unsigned value) {
  const uint64_t i = (uint64_t)blockIdx.x * kMkThreads + threadIdx.x;
  if (i < n) p[i] = value;
}

__global__ __launch_bounds__(kMkThreads) void sp_vertex_key_kernel(const double* __restrict__ vertices, int64_t V, SpGrid g,
                                                                   SpWs w) {
  const int64_t v = (int64_t)blockIdx.x * kMkThreads + threadIdx.x;
  if (v >= V) return;
  unsigned long long key = 0;
  bool ok = true;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const double x = vertices[v * 3 + d];
    int i = 0;
    double f;
    ok = ok && mesh_finite(x) && sp_cell(x, g.org(d), g.h, &i, &f);
    key |= (unsigned long long)(unsigned)(i + 1048576) << (21 * d);
  }
  w.key[v] = ok ? key : kSpNoKey;
  w.ref[v] = 0;
  w.used[v] = 0;
  w.lead[v] = -1;
  w.n[v] = 0;
  w.sum[v * 3] = 0;
  w.sum[v * 3 + 1] = 0;
  w.sum[v * 3 + 2] = 0;
  w.d2[v] = ~0ull;
  w.rep[v] = kSpEmpty;
  w.newidx[v] = -1;
}

// every index is range-checked before it is used as an address
__device__ inline bool sp_valid(const int32_t* __restrict__ tri, int64_t t, int64_t V, const unsigned long long* key,
                                int* a, int* b, int* c, unsigned* why) {
  *a = tri[t * 3]; *b = tri[t * 3 + 1]; *c = tri[t * 3 + 2];
  if (!mesh_indices_ok(*a, *b, *c, V)) { *why = SP_BAD_INDEX; return false; }
  if (key[*a] == kSpNoKey || key[*b] == kSpNoKey || key[*c] == kSpNoKey) { *why = SP_BAD_VERTEX; return false; }
  return true;
}

__global__ __launch_bounds__(kMkThreads) void sp_mark_kernel(const int32_t* __restrict__ tri, int64_t T, int64_t V, SpWs w,
                                                             long long* counts) {
  const int64_t t = (int64_t)blockIdx.x * kMkThreads + threadIdx.x;
  if (t >= T) return;
  int a, b, c;
  unsigned why = 0;
  if (!sp_valid(tri, t, V, w.key, &a, &b, &c, &why)) {
    atomicOr((unsigned long long*)(counts + 4), (unsigned long long)why);
    return;
  }
  w.ref[a] = 1; w.ref[b] = 1; w.ref[c] = 1;
}

// see THE TWO TABLES above
__global__ __launch_bounds__(kMkThreads) void sp_cluster_kernel(int64_t V, SpWs w, long long* counts) {
  const int64_t v = (int64_t)blockIdx.x * kMkThreads + threadIdx.x;
  if (v >= V || !w.ref[v]) return;
  const unsigned long long k = w.key[v];
  const uint64_t s = mesh_table_insert(w.vtab, w.cap_v, (unsigned)v, mesh_mix(k), [&](unsigned cur) { return w.key[cur] == k; });
  if (s < w.cap_v) {
    w.lead[v] = (int32_t)(uint32_t)s;    // (s < cap_v <= 2^32: kept as its 32 bits until sp_sum_kernel replaces it)
    return;
  }
  w.ref[v] = 0;                        // (cannot happen: takes no part)
  atomicOr((unsigned long long*)(counts + 4), (unsigned long long)SP_TABLE_FULL);
}

// the three fractions f of a usable vertex, as sp_vertex_key_kernel computed them
__device__ inline void sp_fractions(const double* __restrict__ vertices, int64_t v, const SpGrid& g, double* f) {
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    int i;
    f[d] = 0.0;
    sp_cell(vertices[v * 3 + d], g.org(d), g.h, &i, &f[d]);
  }
}

__global__ __launch_bounds__(kMkThreads) void sp_sum_kernel(const double* __restrict__ vertices, int64_t V, SpGrid g, SpWs w,
                                                            long long* counts) {
  const int64_t v = (int64_t)blockIdx.x * kMkThreads + threadIdx.x;
  bool leads = false;
  if (v < V && w.ref[v]) {
    const int64_t l = w.vtab[(uint32_t)w.lead[v]];
    w.lead[v] = (int32_t)l;
    leads = l == v;
    double f[3];
    sp_fractions(vertices, v, g, f);
    atomicAdd(w.n + l, 1u);
#pragma unroll
    for (int d = 0; d < 3; ++d) atomicAdd(w.sum + l * 3 + d, (unsigned long long)floor(f[d] * 4294967296.0));
  }
  sp_wave_count(counts + 5, leads);
}

// d2 of member v to the mean of its cluster l
__device__ inline unsigned long long sp_d2(const double* __restrict__ vertices, int64_t v, int64_t l, const SpGrid& g,
                                           const SpWs& w) {
  double f[3], m[3];
  sp_fractions(vertices, v, g, f);
  const double n = (double)w.n[l];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const double s = (double)w.sum[l * 3 + d];
    const double a = s / n;
    m[d] = a * 2.3283064365386963e-10;            // 2^-32
  }
  const double dx = f[0] - m[0], dy = f[1] - m[1], dz = f[2] - m[2];
  const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
  const double xy = xx + yy;
  const double d2 = xy + zz;
  return (unsigned long long)__double_as_longlong(d2);
}

__global__ __launch_bounds__(kMkThreads) void sp_d2_kernel(const double* __restrict__ vertices, int64_t V, SpGrid g, SpWs w) {
  const int64_t v = (int64_t)blockIdx.x * kMkThreads + threadIdx.x;
  if (v >= V || w.lead[v] < 0) return;
  const int64_t l = w.lead[v];
  atomicMin(w.d2 + l, sp_d2(vertices, v, l, g, w));
}

__global__ __launch_bounds__(kMkThreads) void sp_rep_kernel(const double* __restrict__ vertices, int64_t V, SpGrid g, SpWs w) {
  const int64_t v = (int64_t)blockIdx.x * kMkThreads + threadIdx.x;
  if (v >= V || w.lead[v] < 0) return;
  const int64_t l = w.lead[v];
  if (sp_d2(vertices, v, l, g, w) == w.d2[l]) atomicMin(w.rep + l, (unsigned)v);
}


// the sorted leader triple of every triangle (-1 -1 -1: invalid or degenerate), for sp_dedupe_kernel to compare against
__global__ __launch_bounds__(kMkThreads) void sp_triple_kernel(const int32_t* __restrict__ tri, int64_t T, int64_t V, SpWs w,
                                                               long long* counts) {
  const int64_t t = (int64_t)blockIdx.x * kMkThreads + threadIdx.x;
  bool degenerate = false, enters = false;
  if (t < T) {
    int a, b, c, x = -1, y = -1, z = -1;
    unsigned why;
    if (sp_valid(tri, t, V, w.key, &a, &b, &c, &why) && w.lead[a] >= 0 && w.lead[b] >= 0 && w.lead[c] >= 0) {
      x = w.lead[a]; y = w.lead[b]; z = w.lead[c];
      degenerate = x == y || y == z || x == z;
      if (degenerate) {
        x = y = z = -1;
      } else {
        int s;
        if (x > y) { s = x; x = y; y = s; }
        if (y > z) { s = y; y = z; z = s; }
        if (x > y) { s = x; x = y; y = s; }
        enters = true;
      }
    }
    w.triple[t * 3] = x; w.triple[t * 3 + 1] = y; w.triple[t * 3 + 2] = z;
    w.tslot[t] = 0;
  }
  sp_wave_count(counts + 2, degenerate);
  sp_wave_count(counts + 3, enters);                   // every non-degenerate one; sp_survive_kernel takes the survivors off
}

// see THE TWO TABLES above; the key of a triangle is its sorted leader triple
__global__ __launch_bounds__(kMkThreads) void sp_dedupe_kernel(int64_t T, SpWs w, long long* counts) {
  const int64_t t = (int64_t)blockIdx.x * kMkThreads + threadIdx.x;
  if (t >= T) return;
  const int x = w.triple[t * 3], y = w.triple[t * 3 + 1], z = w.triple[t * 3 + 2];
  if (x < 0) return;
  const unsigned long long h = mesh_mix((unsigned long long)x + mesh_mix((unsigned long long)y + mesh_mix((unsigned long long)z)));
  const uint64_t s = mesh_table_insert(w.ttab, w.cap_t, (unsigned)t, h, [&](unsigned cur) {
    const int32_t* o = w.triple + (int64_t)cur * 3;        // (cur < T: only triangle indices are ever stored)
    return o[0] == x && o[1] == y && o[2] == z;
  });
  if (s < w.cap_t) {
    w.tslot[t] = (unsigned)s;
    return;
  }
  atomicOr((unsigned long long*)(counts + 4), (unsigned long long)SP_TABLE_FULL);
}

__device__ inline bool sp_survives(const SpWs& w, int64_t t) {
  return w.triple[t * 3] >= 0 && w.ttab[w.tslot[t]] == (unsigned)t;
}

__global__ __launch_bounds__(kMkThreads) void sp_survive_kernel(int64_t T, SpWs w, long long* counts) {
  const int64_t t = (int64_t)blockIdx.x * kMkThreads + threadIdx.x;
  bool lives = false;
  if (t < T && sp_survives(w, t)) {
    lives = true;
    w.used[w.triple[t * 3]] = 1; w.used[w.triple[t * 3 + 1]] = 1; w.used[w.triple[t * 3 + 2]] = 1;
  }
  // counts[3] -= survivors: the duplicates are what is left of the non-degenerate triangles
  const unsigned long long m = __ballot(lives);
  if (m && (threadIdx.x & 63) == (unsigned)(__ffsll((long long)m) - 1))
    atomicAdd((unsigned long long*)(counts + 3), (unsigned long long)(-(long long)__popcll(m)));
}

struct SpVertexFlag {      // v leads a cluster that a surviving triangle names
  const int32_t* lead;
  const uint8_t* used;
  __device__ bool operator()(int64_t v) const { return lead[v] == (int32_t)v && used[v] != 0; }
};
struct SpTriangleFlag {
  SpWs w;
  __device__ bool operator()(int64_t t) const { return sp_survives(w, t); }
};
struct SpVertexEmit {
  const double* vin;
  const unsigned* rep;
  double* vout;
  int64_t* vindex;
  int32_t* newidx;
  int64_t n_out;
  __device__ void operator()(int64_t v, bool fl, unsigned pos) const {
    newidx[v] = fl ? (int32_t)pos : -1;
    if (!fl || (int64_t)pos >= n_out) return;
    const int64_t r = rep[v];
    vindex[pos] = r;
    vout[(int64_t)pos * 3] = vin[r * 3];
    vout[(int64_t)pos * 3 + 1] = vin[r * 3 + 1];
    vout[(int64_t)pos * 3 + 2] = vin[r * 3 + 2];
  }
};
struct SpTriangleEmit {
  const int32_t* tri;
  const int32_t* lead;
  const int32_t* newidx;
  int32_t* out;
  int64_t* tindex;       // or nullptr
  int64_t n_out;
  __device__ void operator()(int64_t t, bool fl, unsigned pos) const {
    if (!fl || (int64_t)pos >= n_out) return;                // (fl: the three indices passed the range check)
    out[(int64_t)pos * 3] = newidx[lead[tri[t * 3]]];
    out[(int64_t)pos * 3 + 1] = newidx[lead[tri[t * 3 + 1]]];
    out[(int64_t)pos * 3 + 2] = newidx[lead[tri[t * 3 + 2]]];
    if (tindex) tindex[pos] = t;
  }
};

__global__ __launch_bounds__(kMkThreads) void sp_vertex_cluster_kernel(int64_t V, SpWs w, int32_t* __restrict__ out) {
  const int64_t v = (int64_t)blockIdx.x * kMkThreads + threadIdx.x;
  if (v >= V) return;
  const int l = w.lead[v];
  out[v] = l >= 0 ? w.newidx[l] : -1;
}

static unsigned sp_blocks(uint64_t n) { return (unsigned)((n + kMkThreads - 1) / kMkThreads); }

// the checks the two stages share, before any launch
static int sp_check(const char* who, const double* vertices, int64_t V, const int32_t* triangles, int64_t T,
                    const double* origin, double h, void* workspace, size_t workspace_bytes, SpGrid* g, SpWs* w) {
  RNB_TRY(mesh_sizes(who, V, T));
  if (!(h > 0.0) || !std::isfinite(h)) RNB_FAIL(RNB_E_INVALID, "%s: cell_size %g is not positive and finite", who, h);
  g->h = h;
  g->dev_origin = nullptr;
  for (int d = 0; d < 3; ++d) {
    if (origin && !std::isfinite(origin[d])) RNB_FAIL(RNB_E_INVALID, "%s: origin[%d] = %g is not finite", who, d, origin[d]);
    g->origin[d] = origin ? origin[d] : 0.0;
  }
  if ((V > 0 && !vertices) || (T > 0 && !triangles)) RNB_FAIL(RNB_E_NULL, "%s: NULL vertices / triangles", who);
  if (T == 0) return RNB_OK;
  if (!workspace) RNB_FAIL(RNB_E_NULL, "%s: NULL workspace", who);
  Carver cv(workspace, workspace_bytes);
  *w = sp_carve(cv, V, T);
  if (!cv.ok) RNB_FAIL(RNB_E_WORKSPACE, "%s: workspace %zu < %zu bytes", who, workspace_bytes, cv.off);
  if (!origin) g->dev_origin = w->origin;
  return RNB_OK;
}

}  // namespace rnb

#define RNB_API extern "C" __attribute__((visibility("default")))

RNB_API int rnb_mesh_simplify_workspace_bytes(int64_t n_vertices, int64_t n_triangles, int64_t* bytes) {
  using namespace rnb;
  if (!bytes) RNB_FAIL(RNB_E_NULL, "rnb_mesh_simplify_workspace_bytes: NULL");
  RNB_TRY(mesh_sizes("rnb_mesh_simplify_workspace_bytes", n_vertices, n_triangles));
  Carver c(nullptr, 0);
  sp_carve(c, n_vertices, n_triangles);
  *bytes = (int64_t)c.off;
  return RNB_OK;
}

RNB_API int rnb_mesh_simplify_count(const double* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles,
                                    const double* origin, double cell_size, void* workspace, size_t workspace_bytes,
                                    int64_t* counts, rnb_stream_t stream) {
  using namespace rnb;
  const char* who = "rnb_mesh_simplify_count";
  const int64_t V = n_vertices, T = n_triangles;
  SpGrid g;
  SpWs w;
  RNB_TRY(sp_check(who, vertices, V, triangles, T, origin, cell_size, workspace, workspace_bytes, &g, &w));
  if (!counts) RNB_FAIL(RNB_E_NULL, "%s: NULL counts", who);
  hipStream_t s = (hipStream_t)stream;
  RNB_CHECK_HIP(hipMemsetAsync(counts, 0, 6 * sizeof(int64_t), s));
  if (T == 0) return RNB_OK;              // no triangle: no referenced vertex, no cluster
  long long* cnt = (long long*)counts;
  const dim3 blk(kMkThreads);
  if (V > 0) {
    if (!origin) {
      hipLaunchKernelGGL(sp_origin_init_kernel, dim3(1), blk, 0, s, w.okey);
      RNB_CHECK_LAUNCH();
      hipLaunchKernelGGL(sp_origin_kernel, dim3(sp_blocks(V)), blk, 0, s, vertices, V, w.okey);
      RNB_CHECK_LAUNCH();
      hipLaunchKernelGGL(sp_origin_final_kernel, dim3(1), blk, 0, s, w.okey, w.origin);
      RNB_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(sp_fill_kernel, dim3(sp_blocks(w.cap_v)), blk, 0, s, w.vtab, w.cap_v, kSpEmpty);
    RNB_CHECK_LAUNCH();
    hipLaunchKernelGGL(sp_vertex_key_kernel, dim3(sp_blocks(V)), blk, 0, s, vertices, V, g, w);
    RNB_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(sp_fill_kernel, dim3(sp_blocks(w.cap_t)), blk, 0, s, w.ttab, w.cap_t, kSpEmpty);
  RNB_CHECK_LAUNCH();
  hipLaunchKernelGGL(sp_mark_kernel, dim3(sp_blocks(T)), blk, 0, s, triangles, T, V, w, cnt);
  RNB_CHECK_LAUNCH();
  if (V > 0) {
    hipLaunchKernelGGL(sp_cluster_kernel, dim3(sp_blocks(V)), blk, 0, s, V, w, cnt);
    RNB_CHECK_LAUNCH();
    hipLaunchKernelGGL(sp_sum_kernel, dim3(sp_blocks(V)), blk, 0, s, vertices, V, g, w, cnt);
    RNB_CHECK_LAUNCH();
    hipLaunchKernelGGL(sp_d2_kernel, dim3(sp_blocks(V)), blk, 0, s, vertices, V, g, w);
    RNB_CHECK_LAUNCH();
    hipLaunchKernelGGL(sp_rep_kernel, dim3(sp_blocks(V)), blk, 0, s, vertices, V, g, w);
    RNB_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(sp_triple_kernel, dim3(sp_blocks(T)), blk, 0, s, triangles, T, V, w, cnt);
  RNB_CHECK_LAUNCH();
  hipLaunchKernelGGL(sp_dedupe_kernel, dim3(sp_blocks(T)), blk, 0, s, T, w, cnt);
  RNB_CHECK_LAUNCH();
  hipLaunchKernelGGL(sp_survive_kernel, dim3(sp_blocks(T)), blk, 0, s, T, w, cnt);
  RNB_CHECK_LAUNCH();
  const int64_t nbv = scan_blocks(V), nbt = scan_blocks(T);
  if (V > 0) {
    hipLaunchKernelGGL((scan_sum_kernel<unsigned, SpVertexFlag>), dim3((unsigned)nbv), blk, 0, s, SpVertexFlag{w.lead, w.used}, V,
                       w.bsum_v);
    RNB_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL((scan_sum_kernel<unsigned, SpTriangleFlag>), dim3((unsigned)nbt), blk, 0, s, SpTriangleFlag{w}, T, w.bsum_t);
  RNB_CHECK_LAUNCH();
  hipLaunchKernelGGL(scan_block_sums_kernel<unsigned>, dim3(1), dim3(1024), 0, s, w.bsum_v, nbv, w.bsum_t, nbt, 2, counts);
  RNB_CHECK_LAUNCH();
  return RNB_OK;
}

RNB_API int rnb_mesh_simplify_emit(const double* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles,
                                   const double* origin, double cell_size, void* workspace, size_t workspace_bytes,
                                   int64_t n_vertices_out, int64_t n_triangles_out, double* vertices_out,
                                   int32_t* triangles_out, int64_t* vertex_index, int32_t* vertex_cluster,
                                   int64_t* triangle_index, rnb_stream_t stream) {
  using namespace rnb;
  const char* who = "rnb_mesh_simplify_emit";
  const int64_t V = n_vertices, T = n_triangles;
  SpGrid g;
  SpWs w;
  RNB_TRY(sp_check(who, vertices, V, triangles, T, origin, cell_size, workspace, workspace_bytes, &g, &w));
  if (n_vertices_out < 0 || n_vertices_out > V || n_triangles_out < 0 || n_triangles_out > T)
    RNB_FAIL(RNB_E_INVALID, "%s: %lld of %lld vertices / %lld of %lld triangles", who, (long long)n_vertices_out, (long long)V,
             (long long)n_triangles_out, (long long)T);
  if ((n_vertices_out > 0 && (!vertex_index || !vertices_out)) || (n_triangles_out > 0 && !triangles_out))
    RNB_FAIL(RNB_E_NULL, "%s: NULL output", who);
  hipStream_t s = (hipStream_t)stream;
  if (T == 0) {                           // nothing was counted: every vertex is unreferenced
    if (vertex_cluster && V > 0) RNB_CHECK_HIP(hipMemsetAsync(vertex_cluster, 0xff, (size_t)V * sizeof(int32_t), s));
    return RNB_OK;
  }
  const dim3 blk(kMkThreads);
  if (V > 0) {
    hipLaunchKernelGGL((scan_emit_kernel<unsigned, SpVertexFlag, SpVertexEmit>), dim3((unsigned)scan_blocks(V)), blk, 0, s,
                       SpVertexFlag{w.lead, w.used},
                       SpVertexEmit{vertices, w.rep, vertices_out, vertex_index, w.newidx, n_vertices_out}, V, w.bsum_v);
    RNB_CHECK_LAUNCH();
    if (vertex_cluster) {
      hipLaunchKernelGGL(sp_vertex_cluster_kernel, dim3(sp_blocks(V)), blk, 0, s, V, w, vertex_cluster);
      RNB_CHECK_LAUNCH();
    }
  }
  hipLaunchKernelGGL((scan_emit_kernel<unsigned, SpTriangleFlag, SpTriangleEmit>), dim3((unsigned)scan_blocks(T)), blk, 0, s,
                     SpTriangleFlag{w}, SpTriangleEmit{triangles, w.lead, w.newidx, triangles_out, triangle_index, n_triangles_out},
                     T, w.bsum_t);
  RNB_CHECK_LAUNCH();
  return RNB_OK;
}
