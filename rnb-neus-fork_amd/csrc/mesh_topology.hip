// Mesh topology audit on the device: the edges of a triangle mesh and how often each is used in either direction, boundary /
// manifold / flipped / non-manifold edges, boundary components, and per connected component the edge-class counts, holes and
// signed volume (rnb_mesh_topology_* in include/rnbneus.h, which has the definitions op for op; DESIGN.md 4s;
// tests/mesh_topology_ref.py is the same definition in numpy).
//
//   count   tp_key_kernel       one thread per triangle: index guard, key[3t + k] of its half-edges (all ones: the triangle is
//                               not proper), per-half-edge state reset, "named by a proper triangle" marks
//           tp_insert_kernel    the half-edges enter the edge table (mesh_table.hip.h; the argument at the head of
//                               mesh_simplify.hip covers it unchanged: items = half-edges, key = the undirected edge)
//           tp_use_kernel       lead[h] = the smallest half-edge of h's edge, looked up in the finished table;
//                               n_fwd / n_bwd [lead] += 1 (integer atomicAdd)
//           tp_class_kernel     the leaders: class of the edge, one add per wave and class; vertex flags; boundary edges
//                               raise the boundary degree of their two ends and unite them (union_find.hip.h)
//           tp_triangle_kernel  tri_flags[t]: its own class bits | the classes of its three edges (one thread owns the byte)
//           boundary            flatten / root-flag scan / relabel, as the vertex components of mesh_clean.hip
//           tp_vertex_kernel    vert_flags[v] from the flag word of v
//           flag scan           "h is a leader" -> E and the block offsets of the emit
//   emit    the same flag with the block offsets (scan.hip.h, stable): the edges in increasing order of leader
//   components  integer adds per leader / triangle / vertex into the [C,8] table, LDS first (the pattern and the reason of
//           mk_stats_pass_kernel in mesh_clean.hip: same-address atomics serialise in L2 and one component owns most
//           items); the volume in two passes, the largest |term| as bits, then every term in units of 2^(e_c - 54) as a
//           128-bit two's-complement integer sum
//
// Vertex flags: ONE 32-bit word per vertex in the workspace, raised with atomicOr, turned into the byte by the one thread
// that owns the vertex (tp_vertex_kernel) — no byte is written by two threads with different values.  Triangle flags: a
// plain store by the triangle's own thread.  Integer atomics only (compare-and-swap, min, max, add, or): every result is a
// function of the input alone, whatever the schedule.  The file is compiled with -ffp-contract=off: every product and sum of
// the volume term is rounded on its own.  Block 256, one item per thread (the scans: kScanItems); LDS only in the scans and
// the table passes.
#include "mesh_common.hip.h"
#include "mesh_table.hip.h"
#include "mesh_topology.hip.h"
#include "scan.hip.h"
#include "union_find.hip.h"

namespace rnb {

constexpr int kTpThreads = kScanThreads;
// columns of the per-component table
enum { TP_C_BOUNDARY = 0, TP_C_MANIFOLD, TP_C_FLIPPED, TP_C_NONMANIFOLD, TP_C_PROPER, TP_C_DEGENERATE, TP_C_HOLES, TP_C_VERTICES };
enum { TP_VOL_NAN = 1 };

// the two ends (p, q) of half-edge h = 3 t + k of a proper triangle: corners k and (k + 1) mod 3
__device__ inline void tp_ends(const int32_t* __restrict__ tri, unsigned h, int* p, int* q) {
  const unsigned k = h % 3u;
  const int64_t t3 = (int64_t)h - k;
  *p = tri[t3 + k];
  *q = tri[t3 + (k == 2 ? 0 : k + 1)];
}

__global__ __launch_bounds__(kTpThreads) void tp_begin_kernel(TpWs w, long long* counts, int with_boundary) {
  if (threadIdx.x < 8) counts[threadIdx.x] = threadIdx.x == 7 && !with_boundary ? -1 : 0;
  if (threadIdx.x < 64) w.info[threadIdx.x] = threadIdx.x == TP_INFO_BOUNDARY ? (unsigned)with_boundary : 0u;
}

__global__ __launch_bounds__(kTpThreads) void tp_vertex_init_kernel(TpWs w, int64_t V, int* __restrict__ parent,
                                                                   int* __restrict__ degree) {
  const int64_t v = (int64_t)blockIdx.x * kTpThreads + threadIdx.x;
  if (v >= V) return;
  w.vword[v] = 0;
  w.vref[v] = 0;
  w.broot[v] = 0;
  if (parent) {
    parent[v] = (int)v;
    degree[v] = 0;
  }
}

__global__ __launch_bounds__(kTpThreads) void tp_fill_kernel(unsigned* __restrict__ p, uint64_t n, unsigned value) {
  const uint64_t i = (uint64_t)blockIdx.x * kTpThreads + threadIdx.x;
  if (i < n) p[i] = value;
}

// every index is range-checked before it is used as an address
__global__ __launch_bounds__(kTpThreads) void tp_key_kernel(const int32_t* __restrict__ tri, int64_t T, int64_t V, TpWs w,
                                                            long long* counts) {
  const int64_t t = (int64_t)blockIdx.x * kTpThreads + threadIdx.x;
  bool invalid = false, degenerate = false;
  if (t < T) {
    const int a = tri[t * 3], b = tri[t * 3 + 1], c = tri[t * 3 + 2];
    invalid = !mesh_indices_ok(a, b, c, V);
    degenerate = !invalid && (a == b || b == c || a == c);
    const bool proper = !invalid && !degenerate;
    const int p[3] = {a, b, c}, q[3] = {b, c, a};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const unsigned long long lo = (unsigned long long)(p[k] < q[k] ? p[k] : q[k]);
      const unsigned long long hi = (unsigned long long)(p[k] < q[k] ? q[k] : p[k]);
      w.key[t * 3 + k] = proper ? (lo << 31) + hi : kTpNoKey;
      w.lead[t * 3 + k] = kTpNone;
      w.nfwd[t * 3 + k] = 0;
      w.nbwd[t * 3 + k] = 0;
    }
    if (proper) { w.vref[a] = 1; w.vref[b] = 1; w.vref[c] = 1; }   // (plain stores of one value)
  }
  tp_wave_count(counts + 5, degenerate);
  tp_wave_count(counts + 6, invalid);
}

struct TpSameKey {
  const unsigned long long* key;
  unsigned long long k;
  __device__ bool operator()(unsigned cur) const { return key[cur] == k; }   // (cur < 3T: only half-edge indices are stored)
};

__global__ __launch_bounds__(kTpThreads) void tp_insert_kernel(int64_t H, TpWs w) {
  const int64_t h = (int64_t)blockIdx.x * kTpThreads + threadIdx.x;
  if (h >= H) return;
  const unsigned long long k = w.key[h];
  if (k == kTpNoKey) return;
  if (mesh_table_insert(w.tab, w.cap, (unsigned)h, mesh_mix(k), TpSameKey{w.key, k}) >= w.cap)
    atomicOr(w.info + TP_INFO_ERROR, 1u);                   // (cannot happen: the table has two slots per half-edge)
}

__global__ __launch_bounds__(kTpThreads) void tp_use_kernel(const int32_t* __restrict__ tri, int64_t H, TpWs w) {
  const int64_t h = (int64_t)blockIdx.x * kTpThreads + threadIdx.x;
  if (h >= H) return;
  const unsigned long long k = w.key[h];
  if (k == kTpNoKey) return;
  const unsigned l = mesh_table_find(w.tab, w.cap, mesh_mix(k), TpSameKey{w.key, k});
  if (l == kTpNone) {                                       // (cannot happen: h itself entered)
    atomicOr(w.info + TP_INFO_ERROR, 1u);
    return;
  }
  w.lead[h] = l;
  int p, q;
  tp_ends(tri, (unsigned)h, &p, &q);
  atomicAdd((p < q ? w.nfwd : w.nbwd) + l, 1u);
}

__global__ __launch_bounds__(kTpThreads) void tp_class_kernel(int64_t H, TpWs w, long long* counts, int* parent,
                                                              int* degree) {
  const int64_t h = (int64_t)blockIdx.x * kTpThreads + threadIdx.x;
  const bool leads = h < H && w.lead[h] == (unsigned)h;
  unsigned cls = 0;
  if (leads) {
    cls = tp_class(w.nfwd[h], w.nbwd[h]);
    if (cls) {
      const unsigned long long k = w.key[h];
      const int a = (int)(k >> 31), b = (int)(k & 0x7fffffffull);      // (both passed the index guard in tp_key_kernel)
      atomicOr(w.vword + a, cls);
      atomicOr(w.vword + b, cls);
      if (cls == TP_BOUNDARY && parent) {
        atomicAdd(degree + a, 1);
        atomicAdd(degree + b, 1);
        uf_unite(parent, a, b);
      }
    }
  }
  tp_wave_count(counts + 1, leads && cls == TP_BOUNDARY);
  tp_wave_count(counts + 2, leads && cls == 0);
  tp_wave_count(counts + 3, leads && cls == TP_FLIPPED);
  tp_wave_count(counts + 4, leads && cls == TP_NONMANIFOLD);
}

__global__ __launch_bounds__(kTpThreads) void tp_triangle_kernel(const int32_t* __restrict__ tri, int64_t T, int64_t V, TpWs w,
                                                                 uint8_t* __restrict__ tri_flags) {
  const int64_t t = (int64_t)blockIdx.x * kTpThreads + threadIdx.x;
  if (t >= T) return;
  const int a = tri[t * 3], b = tri[t * 3 + 1], c = tri[t * 3 + 2];
  unsigned fl = 0;
  if (!mesh_indices_ok(a, b, c, V)) fl = TP_INVALID;
  else if (a == b || b == c || a == c) fl = TP_DEGENERATE;
  else {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const unsigned l = w.lead[t * 3 + k];
      if (l != kTpNone) fl |= tp_class(w.nfwd[l], w.nbwd[l]);
    }
  }
  tri_flags[t] = (uint8_t)fl;
}

// the boundary forest only gets flatter after tp_class_kernel has finished: parent[v] = its root, -1 off the boundary
__global__ __launch_bounds__(kTpThreads) void tp_flatten_kernel(int* parent, const int* __restrict__ degree, int64_t V) {
  const int64_t v = (int64_t)blockIdx.x * kTpThreads + threadIdx.x;
  if (v >= V) return;
  if (degree[v] == 0) { parent[v] = -1; return; }           // on no boundary edge: no walk passes through it
  const int r = uf_find(parent, (int)v);
  __hip_atomic_store(parent + v, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct TpRootFlag {
  const int* root;
  __device__ bool operator()(int64_t v) const { return root[v] == (int)v; }
};
struct TpRankEmit {
  unsigned* rank;
  __device__ void operator()(int64_t v, bool, unsigned pos) const { rank[v] = pos; }
};

__global__ __launch_bounds__(kTpThreads) void tp_relabel_kernel(int* __restrict__ labels, TpWs w, int64_t V) {
  const int64_t v = (int64_t)blockIdx.x * kTpThreads + threadIdx.x;
  if (v >= V) return;
  const int r = labels[v];                                  // its root (>= 0: rank[r] is the root's dense id) or -1
  w.broot[v] = r == (int)v ? 1 : 0;
  if (r >= 0) labels[v] = (int)w.rank[r];
}

__global__ __launch_bounds__(kTpThreads) void tp_vertex_kernel(TpWs w, int64_t V, uint8_t* __restrict__ vert_flags) {
  const int64_t v = (int64_t)blockIdx.x * kTpThreads + threadIdx.x;
  if (v < V) vert_flags[v] = (uint8_t)(w.vword[v] | (w.vref[v] ? 0u : (unsigned)TP_V_UNUSED));
}

__global__ __launch_bounds__(kTpThreads) void tp_end_kernel(TpWs w, long long* counts) {
  if (threadIdx.x == 0 && w.info[TP_INFO_ERROR]) counts[0] = -1;
}

struct TpLeaderFlag {
  const unsigned* lead;
  __device__ bool operator()(int64_t h) const { return lead[h] == (unsigned)h; }
};
struct TpEdgeEmit {
  TpWs w;
  int32_t* edges;
  int32_t* use;
  int32_t* etri;
  int64_t n_out;
  __device__ void operator()(int64_t h, bool fl, unsigned pos) const {
    if (!fl || (int64_t)pos >= n_out) return;
    const unsigned long long k = w.key[h];
    edges[(int64_t)pos * 2] = (int32_t)(k >> 31);
    edges[(int64_t)pos * 2 + 1] = (int32_t)(k & 0x7fffffffull);
    use[(int64_t)pos * 2] = (int32_t)w.nfwd[h];
    use[(int64_t)pos * 2 + 1] = (int32_t)w.nbwd[h];
    etri[pos] = (int32_t)(h / 3);
  }
};

// ---- the per-component table ----------------------------------------------------------------------------------------
// The LDS-first pass of mesh_clean.hip (mk_stats_pass_kernel, which says why) over this file's accumulators: a workgroup
// adds its kTpStatItems x 256 items into a direct-mapped LDS table of kTpStatSlots components and flushes it once.

constexpr int kTpStatItems = 16;
constexpr int kTpStatSlots = 64;

struct TpBufs {
  int64_t C;
  long long* table;               // [C,8]
  unsigned long long* maxbits;    // [C]
  unsigned* flags;                // [C]
  unsigned long long* lo;         // [C]
  unsigned long long* hi;         // [C]
};

struct TpColsAcc {                // one add into some columns of the component's row
  unsigned long long n[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  __device__ void store(const TpBufs& s, int c) const {
#pragma unroll
    for (int j = 0; j < 8; ++j) s.table[c * 8 + j] = (long long)n[j];
  }
  __device__ void load(const TpBufs& s, int c) {
#pragma unroll
    for (int j = 0; j < 8; ++j) n[j] = (unsigned long long)s.table[c * 8 + j];
  }
  __device__ void flush(const TpBufs& s, int c) const {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (n[j]) atomicAdd((unsigned long long*)(s.table + (int64_t)c * 8 + j), n[j]);
  }
};

__device__ inline int tp_label(const int32_t* __restrict__ labels, int v, int64_t C) {
  const int l = labels[v];
  return l < 0 || l >= C ? -1 : l;
}

struct TpEdgeItem {               // a leader: its edge's class, in the component of the edge's smaller end
  TpWs w;
  const int32_t* labels;
  int64_t C;
  __device__ int operator()(int64_t h, TpColsAcc& a) const {
    if (w.lead[h] != (unsigned)h) return -1;
    const unsigned cls = tp_class(w.nfwd[h], w.nbwd[h]);
    a.n[TP_C_BOUNDARY] = cls == TP_BOUNDARY;               // (constant indices: the accumulator stays in registers)
    a.n[TP_C_MANIFOLD] = cls == 0;
    a.n[TP_C_FLIPPED] = cls == TP_FLIPPED;
    a.n[TP_C_NONMANIFOLD] = cls == TP_NONMANIFOLD;
    return tp_label(labels, (int)(w.key[h] >> 31), C);
  }
};
struct TpTriangleItem {           // proper / degenerate, in the component of the first corner
  const int32_t* tri;
  const int32_t* labels;
  int64_t V, C;
  __device__ int operator()(int64_t t, TpColsAcc& acc) const {
    const int a = tri[t * 3], b = tri[t * 3 + 1], c = tri[t * 3 + 2];
    if (!mesh_indices_ok(a, b, c, V)) return -1;
    const bool degenerate = a == b || b == c || a == c;
    acc.n[TP_C_DEGENERATE] = degenerate;
    acc.n[TP_C_PROPER] = !degenerate;
    return tp_label(labels, a, C);
  }
};
struct TpVertexItem {             // a boundary root is one boundary component; a vertex a proper triangle names
  TpWs w;
  const int32_t* labels;
  int64_t C;
  __device__ int operator()(int64_t v, TpColsAcc& a) const {
    const bool root = w.broot[v] != 0, ref = w.vref[v] != 0;
    if (!root && !ref) return -1;
    a.n[TP_C_HOLES] = root ? 1 : 0;
    a.n[TP_C_VERTICES] = ref ? 1 : 0;
    return tp_label(labels, (int)v, C);
  }
};

// the volume term of proper triangle t, p0 . (p1 x p2) / 6 with every operation rounded on its own; returns the component,
// -1 when the triangle takes no part; *finite: the nine coordinates and the term are finite
struct TpTermSrc {
  const int32_t* tri;
  const int32_t* labels;
  const double* vertices;
  int64_t V, C;
  __device__ int operator()(int64_t t, double* term, bool* finite) const {
    const int a = tri[t * 3], b = tri[t * 3 + 1], c = tri[t * 3 + 2];
    if (!mesh_indices_ok(a, b, c, V) || a == b || b == c || a == c) return -1;
    const int l = tp_label(labels, a, C);
    if (l < 0) return -1;
    const double* p0 = vertices + (int64_t)a * 3;
    const double* p1 = vertices + (int64_t)b * 3;
    const double* p2 = vertices + (int64_t)c * 3;
    const double x0 = p0[0], y0 = p0[1], z0 = p0[2], x1 = p1[0], y1 = p1[1], z1 = p1[2], x2 = p2[0], y2 = p2[1], z2 = p2[2];
    const double cx = y1 * z2 - z1 * y2;
    const double cy = z1 * x2 - x1 * z2;
    const double cz = x1 * y2 - y1 * x2;
    const double xy = x0 * cx + y0 * cy;
    const double d = xy + z0 * cz;
    *term = d / 6.0;
    *finite = mesh_finite(x0) && mesh_finite(y0) && mesh_finite(z0) && mesh_finite(x1) && mesh_finite(y1) && mesh_finite(z1) &&
              mesh_finite(x2) && mesh_finite(y2) && mesh_finite(z2) && mesh_finite(*term);
    return l;
  }
};

struct TpMaxAcc {                 // the largest finite |term| as bits, the not-finite flag
  unsigned long long bits = 0;
  unsigned fl = 0;
  __device__ void store(const TpBufs& s, int c) const { s.maxbits[c] = bits; s.flags[c] = fl; }
  __device__ void load(const TpBufs& s, int c) { bits = s.maxbits[c]; fl = s.flags[c]; }
  __device__ void flush(const TpBufs& s, int c) const {
    if (bits) atomicMax(s.maxbits + c, bits);
    if (fl) atomicOr(s.flags + c, fl);
  }
};
struct TpMaxItem {
  TpTermSrc src;
  __device__ int operator()(int64_t t, TpMaxAcc& a) const {
    double term = 0.0;
    bool finite = false;
    const int c = src(t, &term, &finite);
    if (c < 0) return -1;
    if (finite) a.bits = (unsigned long long)__double_as_longlong(fabs(term));
    else a.fl = TP_VOL_NAN;
    return c;
  }
};

// every finite term in units of 2^(e_c - 54), e_c = exponent of the component's largest |term| (mesh_topology.hip.h has the
// accumulator: wide_scaled, wide_add, wide_to_double)
struct TpVolAcc {
  unsigned long long lo = 0, hi = 0;
  __device__ void store(const TpBufs& s, int c) const { s.lo[c] = lo; s.hi[c] = hi; }
  __device__ void load(const TpBufs& s, int c) { lo = s.lo[c]; hi = s.hi[c]; }
  __device__ void flush(const TpBufs& s, int c) const { wide_add(s.lo + c, s.hi + c, lo, hi); }
};
struct TpVolItem {
  TpTermSrc src;
  const unsigned long long* maxbits;
  __device__ int operator()(int64_t t, TpVolAcc& a) const {
    double term = 0.0;
    bool finite = false;
    const int c = src(t, &term, &finite);
    if (c < 0) return -1;
    const double tmax = __longlong_as_double((long long)maxbits[c]);
    if (finite && tmax > 0.0) {
      const long long q = wide_scaled(term, tmax);
      a.lo = (unsigned long long)q;
      a.hi = q < 0 ? ~0ull : 0ull;
    }
    return c;
  }
};

template <class Acc, class Item>
__global__ __launch_bounds__(kTpThreads) void tp_pass_kernel(TpBufs s, Item item, int64_t n) {
  __shared__ int key[kTpStatSlots];                            // component of the slot, -1 = free
  __shared__ long long l_table[kTpStatSlots * 8];
  __shared__ unsigned long long l_max[kTpStatSlots], l_lo[kTpStatSlots], l_hi[kTpStatSlots];
  __shared__ unsigned l_flags[kTpStatSlots];
  const TpBufs l{kTpStatSlots, l_table, l_max, l_flags, l_lo, l_hi};
  if (threadIdx.x < kTpStatSlots) {
    key[threadIdx.x] = -1;
    Acc().store(l, threadIdx.x);
  }
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * (kTpThreads * kTpStatItems) + threadIdx.x;
  for (int k = 0; k < kTpStatItems; ++k) {
    const int64_t i = base + (int64_t)k * kTpThreads;
    if (i >= n) break;
    Acc one;
    const int c = item(i, one);
    if (c < 0) continue;
    const int slot = c & (kTpStatSlots - 1);
    const int owner = atomicCAS(&key[slot], -1, c);
    if (owner == -1 || owner == c) one.flush(l, slot);
    else one.flush(s, c);
  }
  __syncthreads();
  if (threadIdx.x < kTpStatSlots && key[threadIdx.x] >= 0) {
    Acc sum;
    sum.load(l, threadIdx.x);
    sum.flush(s, key[threadIdx.x]);
  }
}

__global__ __launch_bounds__(kTpThreads) void tp_table_init_kernel(TpBufs s, TpWs w, int with_volume) {
  const int64_t c = (int64_t)blockIdx.x * kTpThreads + threadIdx.x;
  if (c >= s.C) return;
#pragma unroll
  for (int j = 0; j < 8; ++j) s.table[c * 8 + j] = 0;
  if (!w.info[TP_INFO_BOUNDARY]) s.table[c * 8 + TP_C_HOLES] = -1;   // the count was made without boundary components
  if (with_volume) {
    s.maxbits[c] = 0;
    s.flags[c] = 0;
    s.lo[c] = 0;
    s.hi[c] = 0;
  }
}

// the 128-bit two's-complement sum as a double with ONE rounding (wide_to_double)
__global__ __launch_bounds__(kTpThreads) void tp_volume_kernel(TpBufs s, double* __restrict__ volume) {
  const int64_t c = (int64_t)blockIdx.x * kTpThreads + threadIdx.x;
  if (c >= s.C) return;
  const double tmax = __longlong_as_double((long long)s.maxbits[c]);
  double v = 0.0;
  if (s.flags[c] & TP_VOL_NAN) v = __longlong_as_double(0x7ff8000000000000ll);
  else if (tmax > 0.0) v = wide_to_double(s.lo[c], s.hi[c], tmax);
  volume[c] = v;
}

static unsigned tp_grid(int64_t n) { return (unsigned)((n + kTpThreads - 1) / kTpThreads); }
static unsigned tp_stat_grid(int64_t n) { return (unsigned)((n + kTpThreads * kTpStatItems - 1) / (kTpThreads * kTpStatItems)); }

// the checks the three calls share, before any launch
static int tp_check(const char* who, const int32_t* triangles, int64_t T, int64_t V, void* workspace, size_t workspace_bytes,
                    TpWs* w) {
  RNB_TRY(mesh_sizes(who, V, T));
  if (T > kTpMaxTriangles)
    RNB_FAIL(RNB_E_INVALID, "%s: %lld triangles have more than 2^32 - 4 half-edges", who, (long long)T);
  if (T > 0 && !triangles) RNB_FAIL(RNB_E_NULL, "%s: NULL triangles", who);
  if (!workspace) RNB_FAIL(RNB_E_NULL, "%s: NULL workspace", who);
  Carver cv(workspace, workspace_bytes);
  *w = tp_carve(cv, V, T);
  if (!cv.ok) RNB_FAIL(RNB_E_WORKSPACE, "%s: workspace %zu < %zu bytes", who, workspace_bytes, cv.off);
  return RNB_OK;
}

}  // namespace rnb

#define RNB_API extern "C" __attribute__((visibility("default")))

RNB_API int rnb_mesh_topology_workspace_bytes(int64_t n_vertices, int64_t n_triangles, int64_t* bytes) {
  using namespace rnb;
  const char* who = "rnb_mesh_topology_workspace_bytes";
  if (!bytes) RNB_FAIL(RNB_E_NULL, "%s: NULL", who);
  RNB_TRY(mesh_sizes(who, n_vertices, n_triangles));
  if (n_triangles > kTpMaxTriangles)
    RNB_FAIL(RNB_E_INVALID, "%s: %lld triangles have more than 2^32 - 4 half-edges", who, (long long)n_triangles);
  Carver c(nullptr, 0);
  tp_carve(c, n_vertices, n_triangles);
  *bytes = (int64_t)c.off;
  return RNB_OK;
}

RNB_API int rnb_mesh_topology_count(const int32_t* triangles, int64_t n_triangles, int64_t n_vertices, void* workspace,
                                    size_t workspace_bytes, int64_t* counts, uint8_t* tri_flags, uint8_t* vert_flags,
                                    int32_t* boundary_labels, int32_t* boundary_degree, rnb_stream_t stream) {
  using namespace rnb;
  const char* who = "rnb_mesh_topology_count";
  const int64_t T = n_triangles, V = n_vertices, H = 3 * n_triangles;
  TpWs w;
  RNB_TRY(tp_check(who, triangles, T, V, workspace, workspace_bytes, &w));
  if (!counts || (T > 0 && !tri_flags) || (V > 0 && !vert_flags)) RNB_FAIL(RNB_E_NULL, "%s: NULL counts / tri_flags / vert_flags", who);
  if ((boundary_labels == nullptr) != (boundary_degree == nullptr))
    RNB_FAIL(RNB_E_NULL, "%s: boundary_labels and boundary_degree come together (both NULL: no boundary components)", who);
  const bool with_boundary = boundary_labels != nullptr;
  int* parent = V > 0 ? (int*)boundary_labels : nullptr;
  int* degree = V > 0 ? (int*)boundary_degree : nullptr;
  hipStream_t s = (hipStream_t)stream;
  long long* cnt = (long long*)counts;
  const dim3 blk(kTpThreads);
  hipLaunchKernelGGL(tp_begin_kernel, dim3(1), blk, 0, s, w, cnt, with_boundary ? 1 : 0);
  RNB_CHECK_LAUNCH();
  if (V > 0) {
    hipLaunchKernelGGL(tp_vertex_init_kernel, dim3(tp_grid(V)), blk, 0, s, w, V, parent, degree);
    RNB_CHECK_LAUNCH();
  }
  if (T > 0) {
    hipLaunchKernelGGL(tp_fill_kernel, dim3(tp_grid((int64_t)w.cap)), blk, 0, s, w.tab, w.cap, kTabEmpty);
    RNB_CHECK_LAUNCH();
    hipLaunchKernelGGL(tp_key_kernel, dim3(tp_grid(T)), blk, 0, s, triangles, T, V, w, cnt);
    RNB_CHECK_LAUNCH();
    hipLaunchKernelGGL(tp_insert_kernel, dim3(tp_grid(H)), blk, 0, s, H, w);
    RNB_CHECK_LAUNCH();
    hipLaunchKernelGGL(tp_use_kernel, dim3(tp_grid(H)), blk, 0, s, triangles, H, w);
    RNB_CHECK_LAUNCH();
    hipLaunchKernelGGL(tp_class_kernel, dim3(tp_grid(H)), blk, 0, s, H, w, cnt, parent, degree);
    RNB_CHECK_LAUNCH();
    hipLaunchKernelGGL(tp_triangle_kernel, dim3(tp_grid(T)), blk, 0, s, triangles, T, V, w, tri_flags);
    RNB_CHECK_LAUNCH();
    const int64_t nbh = scan_blocks(H);
    hipLaunchKernelGGL((scan_sum_kernel<unsigned, TpLeaderFlag>), dim3((unsigned)nbh), blk, 0, s, TpLeaderFlag{w.lead}, H, w.bsum);
    RNB_CHECK_LAUNCH();
    hipLaunchKernelGGL(scan_block_sums_kernel<unsigned>, dim3(1), dim3(1024), 0, s, w.bsum, nbh, (unsigned*)nullptr, (int64_t)0, 1,
                       counts);
    RNB_CHECK_LAUNCH();
  }
  if (V > 0) {
    if (with_boundary) {
      hipLaunchKernelGGL(tp_flatten_kernel, dim3(tp_grid(V)), blk, 0, s, parent, degree, V);
      RNB_CHECK_LAUNCH();
      const int64_t nbv = scan_blocks(V);
      const TpRootFlag flag{parent};
      hipLaunchKernelGGL((scan_sum_kernel<unsigned, TpRootFlag>), dim3((unsigned)nbv), blk, 0, s, flag, V, w.bsum_v);
      RNB_CHECK_LAUNCH();
      hipLaunchKernelGGL(scan_block_sums_kernel<unsigned>, dim3(1), dim3(1024), 0, s, w.bsum_v, nbv, (unsigned*)nullptr, (int64_t)0,
                         1, counts + 7);
      RNB_CHECK_LAUNCH();
      hipLaunchKernelGGL((scan_emit_kernel<unsigned, TpRootFlag, TpRankEmit>), dim3((unsigned)nbv), blk, 0, s, flag,
                         TpRankEmit{w.rank}, V, w.bsum_v);
      RNB_CHECK_LAUNCH();
      hipLaunchKernelGGL(tp_relabel_kernel, dim3(tp_grid(V)), blk, 0, s, parent, w, V);
      RNB_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(tp_vertex_kernel, dim3(tp_grid(V)), blk, 0, s, w, V, vert_flags);
    RNB_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(tp_end_kernel, dim3(1), blk, 0, s, w, cnt);
  RNB_CHECK_LAUNCH();
  return RNB_OK;
}

RNB_API int rnb_mesh_topology_emit(const int32_t* triangles, int64_t n_triangles, int64_t n_vertices, void* workspace,
                                   size_t workspace_bytes, int64_t n_edges, int32_t* edges, int32_t* edge_use,
                                   int32_t* edge_triangle, rnb_stream_t stream) {
  using namespace rnb;
  const char* who = "rnb_mesh_topology_emit";
  const int64_t T = n_triangles, V = n_vertices, H = 3 * n_triangles;
  TpWs w;
  RNB_TRY(tp_check(who, triangles, T, V, workspace, workspace_bytes, &w));
  if (n_edges < 0 || n_edges > H) RNB_FAIL(RNB_E_INVALID, "%s: %lld edges of %lld half-edges", who, (long long)n_edges, (long long)H);
  if (n_edges > 0 && (!edges || !edge_use || !edge_triangle)) RNB_FAIL(RNB_E_NULL, "%s: NULL output", who);
  if (n_edges == 0) return RNB_OK;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL((scan_emit_kernel<unsigned, TpLeaderFlag, TpEdgeEmit>), dim3((unsigned)scan_blocks(H)), dim3(kTpThreads), 0, s,
                     TpLeaderFlag{w.lead}, TpEdgeEmit{w, edges, edge_use, edge_triangle, n_edges}, H, w.bsum);
  RNB_CHECK_LAUNCH();
  return RNB_OK;
}

RNB_API int rnb_mesh_topology_components(const int32_t* triangles, int64_t n_triangles, const double* vertices,
                                         int64_t n_vertices, const int32_t* labels, int64_t n_components, void* workspace,
                                         size_t workspace_bytes, int64_t* table, double* volume, rnb_stream_t stream) {
  using namespace rnb;
  const char* who = "rnb_mesh_topology_components";
  const int64_t T = n_triangles, V = n_vertices, C = n_components, H = 3 * n_triangles;
  TpWs w;
  RNB_TRY(tp_check(who, triangles, T, V, workspace, workspace_bytes, &w));
  if (C < 0 || C > V) RNB_FAIL(RNB_E_INVALID, "%s: %lld components of %lld vertices", who, (long long)C, (long long)V);
  if (C == 0) return RNB_OK;
  if (!labels || !table) RNB_FAIL(RNB_E_NULL, "%s: NULL labels / table", who);
  if (vertices && !volume) RNB_FAIL(RNB_E_NULL, "%s: coordinates given but no volume output", who);
  const TpBufs sb{C, (long long*)table, w.maxbits, w.cflags, w.lo, w.hi};
  hipStream_t s = (hipStream_t)stream;
  const dim3 blk(kTpThreads);
  hipLaunchKernelGGL(tp_table_init_kernel, dim3(tp_grid(C)), blk, 0, s, sb, w, vertices ? 1 : 0);
  RNB_CHECK_LAUNCH();
  hipLaunchKernelGGL((tp_pass_kernel<TpColsAcc, TpVertexItem>), dim3(tp_stat_grid(V)), blk, 0, s, sb, TpVertexItem{w, labels, C}, V);
  RNB_CHECK_LAUNCH();
  if (T > 0) {
    hipLaunchKernelGGL((tp_pass_kernel<TpColsAcc, TpEdgeItem>), dim3(tp_stat_grid(H)), blk, 0, s, sb, TpEdgeItem{w, labels, C}, H);
    RNB_CHECK_LAUNCH();
    hipLaunchKernelGGL((tp_pass_kernel<TpColsAcc, TpTriangleItem>), dim3(tp_stat_grid(T)), blk, 0, s, sb,
                       TpTriangleItem{triangles, labels, V, C}, T);
    RNB_CHECK_LAUNCH();
    if (vertices) {
      const TpTermSrc src{triangles, labels, vertices, V, C};
      hipLaunchKernelGGL((tp_pass_kernel<TpMaxAcc, TpMaxItem>), dim3(tp_stat_grid(T)), blk, 0, s, sb, TpMaxItem{src}, T);
      RNB_CHECK_LAUNCH();
      hipLaunchKernelGGL((tp_pass_kernel<TpVolAcc, TpVolItem>), dim3(tp_stat_grid(T)), blk, 0, s, sb, TpVolItem{src, w.maxbits}, T);
      RNB_CHECK_LAUNCH();
    }
  }
  if (vertices) {
    hipLaunchKernelGGL(tp_volume_kernel, dim3(tp_grid(C)), blk, 0, s, sb, volume);
    RNB_CHECK_LAUNCH();
  }
  return RNB_OK;
}
