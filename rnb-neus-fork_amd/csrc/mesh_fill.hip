// Mesh hole filling on the device: the boundary components of the topology audit as ordered polygons, their centroids, and
// a fan of triangles around the centroid of every loop that can be walked (rnb_mesh_loops_* / rnb_mesh_fill_* in
// include/rnbneus.h, which has the definitions op for op; tests/mesh_fill_ref.py is the same definition in
// numpy).  The loops are read off what rnb_mesh_topology_count left: its half-edge arrays (mesh_topology.hip.h; read, never
// written), its boundary labels (the union-find of union_find.hip.h, numbered by smallest vertex) and boundary degrees.
//
//   count   fl_init_kernel        per vertex: no half-edge counted, no successor; per loop slot: empty
//           fl_halfedge_kernel    one thread per half-edge: a leader used once is THE boundary half-edge p -> q of its edge;
//                                 out[p] += 1, in[q] += 1, next[p] = q (a plain store: where two threads store to one p the
//                                 loop is not SIMPLE and next[] is never followed)
//           fl_vertex_kernel      per boundary vertex, into its loop's slot: size += 1, degree sum, smallest vertex
//                                 (atomicMin), status bits (atomicOr)
//           boundary-vertex scan  "v is on the boundary" -> B and the block offsets of the compaction
//           fl_loop_kernel        per loop slot: the counts, one add / max per wave
//   emit    loop-size scan        loop_offsets
//           compaction            bv[g] = the g-th boundary vertex in index order, gidx[v] = g
//           fl_link_kernel        succ[g], dist[g]: the list of a SIMPLE loop, cut at its smallest vertex
//           fl_jump_kernel        x rounds: THE RANKING, below
//           fl_place_kernel       loop_vertices of the SIMPLE loops
//           the other loops       their vertices, compacted in index order, then one stable split per bit of the loop id
//                                 (the scan of scan.hip.h over "bit is 0"): a radix sort whose result is (loop, vertex) order
//   mean    per chunk of 3 columns: largest |value| per loop as bits, then the 128-bit integer sum (mesh_topology.hip.h)
//   fill    two scans over the loops (rank of a filled loop, first new triangle), the centroid rows, the fans
//
// THE RANKING.  For a SIMPLE loop with smallest vertex r, every other vertex u starts with succ[u] = next[u], dist[u] = 1 and
// r itself with succ[r] = r, dist[r] = 0: a list that ends in r, because next[] is a permutation of the loop's vertices with
// a single cycle (one outgoing and one incoming boundary half-edge per vertex, and the loop is connected through them).  One
// round computes, for every u at once, dist'[u] = dist[u] + dist[succ[u]] and succ'[u] = succ[succ[u]] FROM THE OLD ARRAYS
// INTO NEW ONES (two pairs of buffers, swapped by the host between launches: no thread reads what another writes in the same
// launch).  Invariant: dist[u] = the number of next-steps from u to succ[u], and succ[u] = r or dist[u] = 2^k after k rounds.
// The fixed point of r (dist 0, succ itself) makes the update uniform: nothing is tested inside the kernel.  After
// ceil(log2 n) rounds every succ is r and dist[u] = the steps from u to r = n - (position of u), position 0 for r.  The host
// takes the round count from the longest SIMPLE loop, which the count reports.  Vertices of other loops are fixed points from
// the start: their next[] may be missing or ambiguous and is never read.  No thread walks a loop.
//
// Integer atomics only (add, min, max, or): every output is a function of the input alone.  Every index that comes out of
// memory — a vertex of the edge key, a label, a successor, a CSR entry — is range-checked before it is used as an address;
// a failed check raises the error word the count reports, nothing spins, and every loop has a trip count fixed before it
// starts (32 for the binary searches).  Half-edge indices are 32-bit: T <= 1,431,655,764, the audit's limit.  Block 256.
#include "mesh_common.hip.h"
#include "mesh_topology.hip.h"
#include "scan.hip.h"

namespace rnb {

constexpr int kFlThreads = kScanThreads;
constexpr int kFlCols = 3;                      // columns of one pass of the means
enum { FL_BIT_TANGLED = 1, FL_BIT_MISORIENTED = 2 };
enum { FL_N_LOOPS = 0, FL_N_BOUNDARY, FL_N_FILLED, FL_N_NEW, FL_N_TANGLED, FL_N_MISORIENTED, FL_N_TOO_LONG, FL_LONGEST_FILLED,
       FL_LONGEST_SIMPLE, FL_N_UNWALKED, FL_ERROR, FL_COUNTS = 16 };
enum { FL_MEAN_NAN = 1 };

struct FlWs {
  unsigned* info;             // [64]  word 0: a value was out of range
  long long* totals;          // [8]   totals of the scans (device side)
  unsigned* outc;             // [V]   outgoing boundary half-edges
  unsigned* inc;              // [V]   incoming boundary half-edges
  unsigned* next;             // [V]   head of an outgoing boundary half-edge, all ones = none
  unsigned* lsize;            // [V]   (by loop) vertices
  unsigned* ldeg;             // [V]   (by loop) sum of the boundary degrees
  unsigned* lstat;            // [V]   (by loop) FL_BIT_*
  unsigned* lroot;            // [V]   (by loop) smallest vertex
  unsigned* bsum_v;           // block sums of the boundary-vertex scan
  unsigned* gidx;             // [V]   rank of a boundary vertex among the boundary vertices
  unsigned* bv;               // [V]   the boundary vertices in index order
  unsigned* succ[2];          // [V]   the ranking's two pairs of buffers; afterwards the keys / values of the radix split
  unsigned* dist[2];
  unsigned* bsum_s;           // block sums of the scans over boundary vertices
  unsigned* bsum_l[2];        // block sums of the scans over loops
  unsigned* frank;            // [V]   (by loop) rank among the filled loops
  unsigned* trioff;           // [V]   (by loop) first new triangle
  unsigned long long* mbits;  // [3V]  (by loop and column) largest |value| as bits
  unsigned long long* lo;     // [3V]  the fixed-point sum
  unsigned long long* hi;
  unsigned* mflags;           // [3V]
};

static FlWs fl_carve(Carver& c, int64_t V) {
  FlWs w;
  const int64_t nb = scan_pad64(scan_blocks(V));
  w.info = c.take<unsigned>(64);
  w.totals = c.take<long long>(8);
  w.outc = c.take<unsigned>(V);
  w.inc = c.take<unsigned>(V);
  w.next = c.take<unsigned>(V);
  w.lsize = c.take<unsigned>(V);                  // at most one loop per vertex
  w.ldeg = c.take<unsigned>(V);
  w.lstat = c.take<unsigned>(V);
  w.lroot = c.take<unsigned>(V);
  w.bsum_v = c.take<unsigned>(nb);
  w.gidx = c.take<unsigned>(V);
  w.bv = c.take<unsigned>(V);
  for (int k = 0; k < 2; ++k) {
    w.succ[k] = c.take<unsigned>(V);
    w.dist[k] = c.take<unsigned>(V);
  }
  w.bsum_s = c.take<unsigned>(nb);
  w.bsum_l[0] = c.take<unsigned>(nb);
  w.bsum_l[1] = c.take<unsigned>(nb);
  w.frank = c.take<unsigned>(V);
  w.trioff = c.take<unsigned>(V);
  w.mbits = c.take<unsigned long long>(V * kFlCols);
  w.lo = c.take<unsigned long long>(V * kFlCols);
  w.hi = c.take<unsigned long long>(V * kFlCols);
  w.mflags = c.take<unsigned>(V * kFlCols);
  return w;
}

__device__ inline unsigned fl_status(unsigned bits) {
  return bits & FL_BIT_TANGLED ? RNB_LOOP_TANGLED : bits & FL_BIT_MISORIENTED ? RNB_LOOP_MISORIENTED : RNB_LOOP_SIMPLE;
}

// sum / maximum over the wave, one atomic per wave (every lane of the wave calls)
__device__ inline void fl_wave_add(long long* counter, unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0 && v) atomicAdd((unsigned long long*)counter, v);
}
__device__ inline void fl_wave_max(long long* counter, unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long t = __shfl_xor(v, o, 64);
    v = t > v ? t : v;
  }
  if ((threadIdx.x & 63) == 0 && v) atomicMax((unsigned long long*)counter, v);      // (counts are >= 0: unsigned order)
}

// ---- the count ------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kFlThreads) void fl_init_kernel(FlWs w, int64_t V, long long* counts) {
  const int64_t v = (int64_t)blockIdx.x * kFlThreads + threadIdx.x;
  if (blockIdx.x == 0) {
    if (threadIdx.x < FL_COUNTS) counts[threadIdx.x] = 0;
    if (threadIdx.x < 64) w.info[threadIdx.x] = 0;
    if (threadIdx.x < 8) w.totals[threadIdx.x] = 0;
  }
  if (v >= V) return;
  w.outc[v] = 0;
  w.inc[v] = 0;
  w.next[v] = kTpNone;
  w.lsize[v] = 0;
  w.ldeg[v] = 0;
  w.lstat[v] = 0;
  w.lroot[v] = kTpNone;
}

__global__ __launch_bounds__(kFlThreads) void fl_halfedge_kernel(int64_t H, int64_t V, TpWs tw, FlWs w) {
  const int64_t h = (int64_t)blockIdx.x * kFlThreads + threadIdx.x;
  if (h >= H || tw.lead[h] != (unsigned)h) return;
  const unsigned nf = tw.nfwd[h], nb = tw.nbwd[h];
  if (tp_class(nf, nb) != TP_BOUNDARY) return;
  const unsigned long long k = tw.key[h];
  const int64_t a = (int64_t)(k >> 31), b = (int64_t)(k & 0x7fffffffull);      // (min, max) of the edge
  if (k == kTpNoKey || a >= V || b >= V) {                  // (cannot happen after a count on this mesh)
    atomicOr(w.info, 1u);
    return;
  }
  const unsigned p = (unsigned)(nf ? a : b), q = (unsigned)(nf ? b : a);       // forward: min -> max
  atomicAdd(w.outc + p, 1u);
  atomicAdd(w.inc + q, 1u);
  w.next[p] = q;
}

// labels[v] as a loop slot: -1 off the boundary and for a value no count writes
__device__ inline int64_t fl_loop_of(const int32_t* __restrict__ labels, int64_t v, int64_t V) {
  const int l = labels[v];
  return l < 0 || l >= V ? -1 : l;
}

__global__ __launch_bounds__(kFlThreads) void fl_vertex_kernel(int64_t V, const int32_t* __restrict__ labels,
                                                               const int32_t* __restrict__ degree, FlWs w) {
  const int64_t v = (int64_t)blockIdx.x * kFlThreads + threadIdx.x;
  if (v >= V) return;
  const int64_t l = fl_loop_of(labels, v, V);
  if (l < 0) return;
  const int d = degree[v];
  atomicAdd(w.lsize + l, 1u);
  atomicAdd(w.ldeg + l, (unsigned)d);
  atomicMin(w.lroot + l, (unsigned)v);
  const unsigned bits = d != 2 ? FL_BIT_TANGLED : (w.outc[v] != 1 || w.inc[v] != 1) ? FL_BIT_MISORIENTED : 0u;
  if (bits) atomicOr(w.lstat + l, bits);
}

struct FlBoundaryFlag {
  const int32_t* labels;
  int64_t V;
  __device__ bool operator()(int64_t v) const { return fl_loop_of(labels, v, V) >= 0; }
};

__global__ __launch_bounds__(kFlThreads) void fl_loop_kernel(int64_t V, FlWs w, int64_t max_edges, long long* counts) {
  const int64_t l = (int64_t)blockIdx.x * kFlThreads + threadIdx.x;
  const unsigned n = l < V ? w.lsize[l] : 0u;
  const unsigned st = l < V ? fl_status(w.lstat[l]) : 0u;
  const bool exists = n > 0, simple = exists && st == RNB_LOOP_SIMPLE;
  const bool filled = simple && (max_edges < 0 || (int64_t)n <= max_edges);
  tp_wave_count(counts + FL_N_LOOPS, exists);
  tp_wave_count(counts + FL_N_FILLED, filled);
  tp_wave_count(counts + FL_N_TANGLED, exists && st == RNB_LOOP_TANGLED);
  tp_wave_count(counts + FL_N_MISORIENTED, exists && st == RNB_LOOP_MISORIENTED);
  tp_wave_count(counts + FL_N_TOO_LONG, simple && !filled);
  fl_wave_add(counts + FL_N_NEW, filled ? n : 0u);
  fl_wave_add(counts + FL_N_UNWALKED, exists && !simple ? n : 0u);
  fl_wave_max(counts + FL_LONGEST_FILLED, filled ? n : 0u);
  fl_wave_max(counts + FL_LONGEST_SIMPLE, simple ? n : 0u);
}

__global__ __launch_bounds__(kFlThreads) void fl_end_kernel(FlWs w, TpWs tw, int64_t V, long long* counts) {
  // (the audit's count makes no boundary components for V == 0, and none are needed)
  if (threadIdx.x == 0 && (w.info[0] || tw.info[TP_INFO_ERROR] || (V > 0 && !tw.info[TP_INFO_BOUNDARY]))) counts[FL_ERROR] = -1;
}

// ---- the emit -------------------------------------------------------------------------------------------------------------

struct FlSizeWeight {
  const unsigned* lsize;
  __device__ unsigned operator()(int64_t l) const { return lsize[l]; }
};
struct FlOffsetEmit {
  int64_t* offsets;
  int64_t L;
  __device__ void operator()(int64_t l, unsigned n, unsigned pos) const {
    offsets[l] = (int64_t)pos;
    if (l == L - 1) offsets[L] = (int64_t)pos + n;
  }
};
struct FlCompactEmit {
  FlWs w;
  int64_t B;
  __device__ void operator()(int64_t v, bool fl, unsigned pos) const {
    if (!fl || (int64_t)pos >= B) return;
    w.bv[pos] = (unsigned)v;
    w.gidx[v] = pos;
  }
};

__global__ __launch_bounds__(kFlThreads) void fl_link_kernel(int64_t B, int64_t V, const int32_t* __restrict__ labels, FlWs w) {
  const int64_t g = (int64_t)blockIdx.x * kFlThreads + threadIdx.x;
  if (g >= B) return;
  const unsigned v = w.bv[g];                               // (< V: the compaction wrote it)
  const int64_t l = fl_loop_of(labels, v, V);
  unsigned s = (unsigned)g, d = 0;
  if (l >= 0 && w.lstat[l] == 0 && w.lroot[l] != v) {
    const unsigned nx = w.next[v];
    const unsigned ng = nx < V && fl_loop_of(labels, nx, V) == l ? w.gidx[nx] : kTpNone;
    if ((int64_t)ng < B) { s = ng; d = 1; }
    else atomicOr(w.info, 1u);                              // (cannot happen: a SIMPLE loop's vertex has its one successor)
  }
  w.succ[0][g] = s;
  w.dist[0][g] = d;
}

// one round of the ranking: from the old pair of arrays into the new one
__global__ __launch_bounds__(kFlThreads) void fl_jump_kernel(int64_t B, const unsigned* __restrict__ succ_in,
                                                             const unsigned* __restrict__ dist_in, unsigned* __restrict__ succ_out,
                                                             unsigned* __restrict__ dist_out) {
  const int64_t g = (int64_t)blockIdx.x * kFlThreads + threadIdx.x;
  if (g >= B) return;
  const unsigned s = succ_in[g];                            // (< B: fl_link_kernel stores nothing else, a round keeps it)
  dist_out[g] = dist_in[g] + dist_in[s];
  succ_out[g] = succ_in[s];
}

__global__ __launch_bounds__(kFlThreads) void fl_place_kernel(int64_t B, int64_t V, const int32_t* __restrict__ labels, FlWs w,
                                                              const unsigned* __restrict__ dist,
                                                              const int64_t* __restrict__ offsets, int32_t* __restrict__ loop_vertices) {
  const int64_t g = (int64_t)blockIdx.x * kFlThreads + threadIdx.x;
  if (g >= B) return;
  const unsigned v = w.bv[g];
  const int64_t l = fl_loop_of(labels, v, V);
  if (l < 0 || w.lstat[l] != 0) return;
  const unsigned n = w.lsize[l], d = dist[g];
  const int64_t pos = offsets[l] + (d == 0 ? 0 : (int64_t)n - d);
  if (d >= n || pos < 0 || pos >= B) {                      // (cannot happen: d = the steps to the smallest vertex < n)
    atomicOr(w.info, 1u);
    return;
  }
  loop_vertices[pos] = (int32_t)v;
}

struct FlUnwalkedFlag {
  FlWs w;
  const int32_t* labels;
  int64_t V;
  __device__ bool operator()(int64_t g) const {
    const int64_t l = fl_loop_of(labels, w.bv[g], V);
    return l >= 0 && w.lstat[l] != 0;
  }
};
struct FlUnwalkedEmit {
  FlWs w;
  const int32_t* labels;
  unsigned* key;
  unsigned* val;
  int64_t M;
  __device__ void operator()(int64_t g, bool fl, unsigned pos) const {
    if (!fl || (int64_t)pos >= M) return;
    const unsigned v = w.bv[g];
    key[pos] = (unsigned)labels[v];
    val[pos] = v;
  }
};
struct FlBitZero {
  const unsigned* key;
  int bit;
  __device__ bool operator()(int64_t i) const { return ((key[i] >> bit) & 1u) == 0; }
};
// the stable split: the items whose bit is 0 keep their order in front, the others theirs behind them
struct FlSplitEmit {
  const unsigned* key_in;
  const unsigned* val_in;
  unsigned* key_out;
  unsigned* val_out;
  const long long* n_zero;
  int64_t M;
  __device__ void operator()(int64_t i, bool zero, unsigned pos) const {
    const int64_t dst = zero ? (int64_t)pos : *n_zero + (i - (int64_t)pos);
    if (dst < 0 || dst >= M) return;
    key_out[dst] = key_in[i];
    val_out[dst] = val_in[i];
  }
};

__global__ __launch_bounds__(kFlThreads) void fl_place_sorted_kernel(int64_t M, int64_t L, int64_t B, const unsigned* __restrict__ key,
                                                                     const unsigned* __restrict__ val,
                                                                     const int64_t* __restrict__ offsets,
                                                                     int32_t* __restrict__ loop_vertices) {
  const int64_t i = (int64_t)blockIdx.x * kFlThreads + threadIdx.x;
  if (i >= M) return;
  const unsigned l = key[i];
  if ((int64_t)l >= L) return;
  int64_t lo = 0, hi = i;                                   // the first item of loop l: the keys are sorted
  for (int s = 0; s < 32 && lo < hi; ++s) {
    const int64_t mid = (lo + hi) / 2;
    if (key[mid] < l) lo = mid + 1;
    else hi = mid;
  }
  const int64_t pos = offsets[l] + (i - lo);
  if (pos >= 0 && pos < B) loop_vertices[pos] = (int32_t)val[i];
}

__global__ __launch_bounds__(kFlThreads) void fl_loop_out_kernel(int64_t L, FlWs w, uint8_t* __restrict__ status,
                                                                 int32_t* __restrict__ edges) {
  const int64_t l = (int64_t)blockIdx.x * kFlThreads + threadIdx.x;
  if (l >= L) return;
  status[l] = (uint8_t)fl_status(w.lstat[l]);
  edges[l] = (int32_t)(w.ldeg[l] / 2);
}

// ---- from the CSR arrays alone: the means and the cap ---------------------------------------------------------------------

// the loop of CSR position i: the largest l with offsets[l] <= i (L >= 1)
__device__ inline int64_t fl_find_loop(const int64_t* __restrict__ offsets, int64_t L, int64_t i) {
  int64_t lo = 0, hi = L - 1;
  for (int s = 0; s < 32 && lo < hi; ++s) {
    const int64_t mid = (lo + hi + 1) / 2;
    if (offsets[mid] <= i) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(kFlThreads) void fl_mean_init_kernel(int64_t n, FlWs w) {
  const int64_t i = (int64_t)blockIdx.x * kFlThreads + threadIdx.x;
  if (i >= n) return;
  w.mbits[i] = 0;
  w.lo[i] = 0;
  w.hi[i] = 0;
  w.mflags[i] = 0;
}

// Both passes go over the CSR positions, so the lanes of a wave are mostly vertices of one loop: where the whole wave is, it
// reduces in registers and makes one atomic per column (a rim of 10^5 vertices would otherwise queue on one address).
template <class T, bool kSum>
__global__ __launch_bounds__(kFlThreads) void fl_mean_pass_kernel(const T* __restrict__ values, int64_t V, int64_t C, int c0, int nc,
                                                                  const int64_t* __restrict__ offsets,
                                                                  const int32_t* __restrict__ loop_vertices, int64_t L, int64_t B,
                                                                  FlWs w) {
  const int64_t i = (int64_t)blockIdx.x * kFlThreads + threadIdx.x;
  const int v = i < B ? loop_vertices[i] : -1;
  const bool valid = v >= 0 && v < V;                       // the guard in front of values[v]
  const int64_t l = i < B ? fl_find_loop(offsets, L, i) : -1;
  const unsigned long long act = __ballot(i < B);
  const int64_t l0 = __shfl(l, 0, 64);                      // (lane 0 is active whenever a lane of the wave is)
  const bool uniform = act != 0 && __ballot(i < B && l == l0) == act;
  for (int c = 0; c < nc; ++c) {
    const double x = valid ? (double)values[(int64_t)v * C + c0 + c] : 0.0;
    const bool finite = mesh_finite(x);
    const int64_t slot = l * kFlCols + c;
    if (!kSum) {
      unsigned long long bits = valid && finite ? (unsigned long long)__double_as_longlong(fabs(x)) : 0ull;
      unsigned fl = valid && !finite ? (unsigned)FL_MEAN_NAN : 0u;
      if (uniform) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          const unsigned long long t = __shfl_xor(bits, o, 64);
          bits = t > bits ? t : bits;
          fl |= __shfl_xor(fl, o, 64);
        }
        if ((threadIdx.x & 63) != 0) { bits = 0; fl = 0; }
      }
      if (bits) atomicMax(w.mbits + slot, bits);
      if (fl) atomicOr(w.mflags + slot, fl);
    } else {
      long long q = 0;
      if (valid && finite && l >= 0) {
        const double tmax = __longlong_as_double((long long)w.mbits[slot]);
        if (tmax > 0.0) q = wide_scaled(x, tmax);           // |q| <= 2^55: 64 of them fit a signed 64-bit sum
      }
      if (uniform) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);
        if ((threadIdx.x & 63) != 0) q = 0;
      }
      if (q) wide_add(w.lo + slot, w.hi + slot, (unsigned long long)q, q < 0 ? ~0ull : 0ull);
    }
  }
}

template <class T>
__global__ __launch_bounds__(kFlThreads) void fl_mean_out_kernel(int64_t L, int64_t C, int c0, int nc,
                                                                 const int64_t* __restrict__ offsets, FlWs w, T* __restrict__ means) {
  const int64_t l = (int64_t)blockIdx.x * kFlThreads + threadIdx.x;
  if (l >= L) return;
  const double n = (double)(offsets[l + 1] - offsets[l]);
  for (int c = 0; c < nc; ++c) {
    const int64_t slot = l * kFlCols + c;
    const double tmax = __longlong_as_double((long long)w.mbits[slot]);
    double m = 0.0;
    if (w.mflags[slot] & FL_MEAN_NAN) m = __longlong_as_double(0x7ff8000000000000ll);
    else if (tmax > 0.0) m = wide_to_double(w.lo[slot], w.hi[slot], tmax) / n;
    means[l * C + c0 + c] = (T)m;
  }
}

struct FlCsr {
  const int64_t* offsets;
  const uint8_t* status;
  int64_t max_edges;
  // the number of edges of loop l when it is filled, else 0
  __device__ unsigned filled(int64_t l) const {
    const int64_t n = offsets[l + 1] - offsets[l];
    return status[l] == RNB_LOOP_SIMPLE && n > 0 && n <= kMeshMax && (max_edges < 0 || n <= max_edges) ? (unsigned)n : 0u;
  }
};
struct FlFilledFlag {
  FlCsr csr;
  __device__ unsigned operator()(int64_t l) const { return csr.filled(l) ? 1u : 0u; }
};
struct FlFilledSize {
  FlCsr csr;
  __device__ unsigned operator()(int64_t l) const { return csr.filled(l); }
};
struct FlStoreEmit {
  unsigned* out;
  __device__ void operator()(int64_t l, unsigned, unsigned pos) const { out[l] = pos; }
};

__global__ __launch_bounds__(kFlThreads) void fl_cap_vertex_kernel(int64_t L, int64_t V, int64_t F, FlCsr csr, FlWs w,
                                                                   const double* __restrict__ centroid,
                                                                   double* __restrict__ vertices_out, int32_t* __restrict__ filled) {
  const int64_t l = (int64_t)blockIdx.x * kFlThreads + threadIdx.x;
  if (l >= L || !csr.filled(l)) return;
  const int64_t r = w.frank[l];
  if (r >= F) return;                                       // (more filled loops than the caller allocated for: not written)
#pragma unroll
  for (int k = 0; k < 3; ++k) vertices_out[(V + r) * 3 + k] = centroid[l * 3 + k];
  filled[r] = (int32_t)l;
}

__global__ __launch_bounds__(kFlThreads) void fl_cap_triangle_kernel(int64_t L, int64_t B, int64_t V, int64_t T, int64_t F,
                                                                     int64_t N, FlCsr csr, FlWs w,
                                                                     const int32_t* __restrict__ loop_vertices,
                                                                     int32_t* __restrict__ triangles_out) {
  const int64_t i = (int64_t)blockIdx.x * kFlThreads + threadIdx.x;
  if (i >= B) return;
  const int64_t l = fl_find_loop(csr.offsets, L, i);
  const int64_t n = csr.filled(l);
  if (n == 0) return;
  const int64_t o = csr.offsets[l], j = i - o;
  if (j < 0 || j >= n) return;
  const int64_t i1 = o + (j + 1 == n ? 0 : j + 1), pos = (int64_t)w.trioff[l] + j, r = w.frank[l];
  if (i1 < 0 || i1 >= B || pos >= N || r >= F) return;
  int32_t* out = triangles_out + (T + pos) * 3;
  out[0] = loop_vertices[i1];
  out[1] = loop_vertices[i];
  out[2] = (int32_t)(V + r);
}

static unsigned fl_grid(int64_t n) { return (unsigned)((n + kFlThreads - 1) / kFlThreads); }

// the checks the calls share, before any launch
static int fl_check(const char* who, int64_t V, int64_t T, void* workspace, size_t workspace_bytes, FlWs* w) {
  RNB_TRY(mesh_sizes(who, V, T));
  if (T > kTpMaxTriangles)
    RNB_FAIL(RNB_E_INVALID, "%s: %lld triangles have more than 2^32 - 4 half-edges", who, (long long)T);
  if (!workspace) RNB_FAIL(RNB_E_NULL, "%s: NULL workspace", who);
  Carver cv(workspace, workspace_bytes);
  *w = fl_carve(cv, V);
  if (!cv.ok) RNB_FAIL(RNB_E_WORKSPACE, "%s: workspace %zu < %zu bytes", who, workspace_bytes, cv.off);
  return RNB_OK;
}

static int fl_check_csr(const char* who, int64_t V, int64_t L, int64_t B, const int64_t* loop_offsets, const int32_t* loop_vertices) {
  if (L < 0 || L > V) RNB_FAIL(RNB_E_INVALID, "%s: %lld loops of %lld vertices", who, (long long)L, (long long)V);
  if (B < 0 || B > V) RNB_FAIL(RNB_E_INVALID, "%s: %lld boundary vertices of %lld vertices", who, (long long)B, (long long)V);
  if (!loop_offsets || (B > 0 && !loop_vertices)) RNB_FAIL(RNB_E_NULL, "%s: NULL loop_offsets / loop_vertices", who);
  return RNB_OK;
}

template <class T>
static int fl_means(const T* values, int64_t V, int64_t C, const int64_t* offsets, const int32_t* loop_vertices, int64_t L,
                    int64_t B, const FlWs& w, T* means, hipStream_t s) {
  const dim3 blk(kFlThreads);
  for (int64_t c0 = 0; c0 < C; c0 += kFlCols) {
    const int nc = (int)(C - c0 < kFlCols ? C - c0 : kFlCols);
    hipLaunchKernelGGL(fl_mean_init_kernel, dim3(fl_grid(L * kFlCols)), blk, 0, s, L * kFlCols, w);
    RNB_CHECK_LAUNCH();
    if (B > 0) {
      hipLaunchKernelGGL((fl_mean_pass_kernel<T, false>), dim3(fl_grid(B)), blk, 0, s, values, V, C, (int)c0, nc, offsets,
                         loop_vertices, L, B, w);
      RNB_CHECK_LAUNCH();
      hipLaunchKernelGGL((fl_mean_pass_kernel<T, true>), dim3(fl_grid(B)), blk, 0, s, values, V, C, (int)c0, nc, offsets,
                         loop_vertices, L, B, w);
      RNB_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(fl_mean_out_kernel<T>, dim3(fl_grid(L)), blk, 0, s, L, C, (int)c0, nc, offsets, w, means);
    RNB_CHECK_LAUNCH();
  }
  return RNB_OK;
}

}  // namespace rnb

#define RNB_API extern "C" __attribute__((visibility("default")))

RNB_API int rnb_mesh_fill_workspace_bytes(int64_t n_vertices, int64_t n_triangles, int64_t* bytes) {
  using namespace rnb;
  const char* who = "rnb_mesh_fill_workspace_bytes";
  if (!bytes) RNB_FAIL(RNB_E_NULL, "%s: NULL", who);
  RNB_TRY(mesh_sizes(who, n_vertices, n_triangles));
  if (n_triangles > kTpMaxTriangles)
    RNB_FAIL(RNB_E_INVALID, "%s: %lld triangles have more than 2^32 - 4 half-edges", who, (long long)n_triangles);
  Carver c(nullptr, 0);
  fl_carve(c, n_vertices);
  *bytes = (int64_t)c.off;
  return RNB_OK;
}

RNB_API int rnb_mesh_loops_count(int64_t n_triangles, int64_t n_vertices, const void* topology_workspace,
                                 size_t topology_workspace_bytes, const int32_t* boundary_labels, const int32_t* boundary_degree,
                                 int64_t max_edges, void* workspace, size_t workspace_bytes, int64_t* counts, rnb_stream_t stream) {
  using namespace rnb;
  const char* who = "rnb_mesh_loops_count";
  const int64_t T = n_triangles, V = n_vertices, H = 3 * n_triangles;
  FlWs w;
  RNB_TRY(fl_check(who, V, T, workspace, workspace_bytes, &w));
  if (!topology_workspace) RNB_FAIL(RNB_E_NULL, "%s: NULL topology workspace", who);
  Carver cv((void*)topology_workspace, topology_workspace_bytes);
  const TpWs tw = tp_carve(cv, V, T);
  if (!cv.ok) RNB_FAIL(RNB_E_WORKSPACE, "%s: topology workspace %zu < %zu bytes", who, topology_workspace_bytes, cv.off);
  if (!counts) RNB_FAIL(RNB_E_NULL, "%s: NULL counts", who);
  if (V > 0 && (!boundary_labels || !boundary_degree)) RNB_FAIL(RNB_E_NULL, "%s: NULL boundary_labels / boundary_degree", who);
  hipStream_t s = (hipStream_t)stream;
  long long* cnt = (long long*)counts;
  const dim3 blk(kFlThreads);
  hipLaunchKernelGGL(fl_init_kernel, dim3(fl_grid(V > 0 ? V : 1)), blk, 0, s, w, V, cnt);
  RNB_CHECK_LAUNCH();
  if (V > 0) {
    if (T > 0) {
      hipLaunchKernelGGL(fl_halfedge_kernel, dim3(fl_grid(H)), blk, 0, s, H, V, tw, w);
      RNB_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(fl_vertex_kernel, dim3(fl_grid(V)), blk, 0, s, V, boundary_labels, boundary_degree, w);
    RNB_CHECK_LAUNCH();
    const int64_t nbv = scan_blocks(V);
    hipLaunchKernelGGL((scan_sum_kernel<unsigned, FlBoundaryFlag>), dim3((unsigned)nbv), blk, 0, s, FlBoundaryFlag{boundary_labels, V},
                       V, w.bsum_v);
    RNB_CHECK_LAUNCH();
    hipLaunchKernelGGL(scan_block_sums_kernel<unsigned>, dim3(1), dim3(1024), 0, s, w.bsum_v, nbv, (unsigned*)nullptr, (int64_t)0, 1,
                       counts + FL_N_BOUNDARY);
    RNB_CHECK_LAUNCH();
    hipLaunchKernelGGL(fl_loop_kernel, dim3(fl_grid(V)), blk, 0, s, V, w, max_edges, cnt);
    RNB_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(fl_end_kernel, dim3(1), blk, 0, s, w, tw, V, cnt);
  RNB_CHECK_LAUNCH();
  return RNB_OK;
}

RNB_API int rnb_mesh_loops_emit(int64_t n_triangles, int64_t n_vertices, const int32_t* boundary_labels, void* workspace,
                                size_t workspace_bytes, int64_t n_loops, int64_t n_boundary_vertices, int64_t longest_simple,
                                int64_t n_unwalked, int64_t* loop_offsets, int32_t* loop_vertices, uint8_t* loop_status,
                                int32_t* loop_edges, rnb_stream_t stream) {
  using namespace rnb;
  const char* who = "rnb_mesh_loops_emit";
  const int64_t V = n_vertices, L = n_loops, B = n_boundary_vertices, M = n_unwalked;
  FlWs w;
  RNB_TRY(fl_check(who, V, n_triangles, workspace, workspace_bytes, &w));
  RNB_TRY(fl_check_csr(who, V, L, B, loop_offsets, loop_vertices));
  if (longest_simple < 0 || longest_simple > B || M < 0 || M > B)
    RNB_FAIL(RNB_E_INVALID, "%s: longest loop %lld / %lld unwalked vertices of %lld boundary vertices", who, (long long)longest_simple,
             (long long)M, (long long)B);
  if (L > 0 && (!loop_status || !loop_edges || !boundary_labels)) RNB_FAIL(RNB_E_NULL, "%s: NULL loop_status / loop_edges / labels", who);
  hipStream_t s = (hipStream_t)stream;
  const dim3 blk(kFlThreads);
  if (L == 0) {
    RNB_CHECK_HIP(hipMemsetAsync(loop_offsets, 0, sizeof(int64_t), s));
    return RNB_OK;
  }
  const int64_t nbl = scan_blocks(L);
  hipLaunchKernelGGL((scan_sum_kernel<unsigned, FlSizeWeight>), dim3((unsigned)nbl), blk, 0, s, FlSizeWeight{w.lsize}, L, w.bsum_l[0]);
  RNB_CHECK_LAUNCH();
  hipLaunchKernelGGL(scan_block_sums_kernel<unsigned>, dim3(1), dim3(1024), 0, s, w.bsum_l[0], nbl, (unsigned*)nullptr, (int64_t)0, 1,
                     (int64_t*)w.totals);
  RNB_CHECK_LAUNCH();
  hipLaunchKernelGGL((scan_emit_kernel<unsigned, FlSizeWeight, FlOffsetEmit>), dim3((unsigned)nbl), blk, 0, s, FlSizeWeight{w.lsize},
                     FlOffsetEmit{loop_offsets, L}, L, w.bsum_l[0]);
  RNB_CHECK_LAUNCH();
  hipLaunchKernelGGL(fl_loop_out_kernel, dim3(fl_grid(L)), blk, 0, s, L, w, loop_status, loop_edges);
  RNB_CHECK_LAUNCH();
  if (B == 0) return RNB_OK;
  const FlBoundaryFlag bflag{boundary_labels, V};
  hipLaunchKernelGGL((scan_emit_kernel<unsigned, FlBoundaryFlag, FlCompactEmit>), dim3((unsigned)scan_blocks(V)), blk, 0, s, bflag,
                     FlCompactEmit{w, B}, V, w.bsum_v);
  RNB_CHECK_LAUNCH();
  hipLaunchKernelGGL(fl_link_kernel, dim3(fl_grid(B)), blk, 0, s, B, V, boundary_labels, w);
  RNB_CHECK_LAUNCH();
  int rounds = 0;
  while (((int64_t)1 << rounds) < longest_simple) ++rounds;
  for (int r = 0; r < rounds; ++r) {
    hipLaunchKernelGGL(fl_jump_kernel, dim3(fl_grid(B)), blk, 0, s, B, w.succ[r & 1], w.dist[r & 1], w.succ[(r + 1) & 1],
                       w.dist[(r + 1) & 1]);
    RNB_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(fl_place_kernel, dim3(fl_grid(B)), blk, 0, s, B, V, boundary_labels, w, w.dist[rounds & 1], loop_offsets,
                     loop_vertices);
  RNB_CHECK_LAUNCH();
  if (M > 0) {
    // the ranking is done with its buffers: they hold the keys (loop ids) and values (vertices) of the split from here on
    unsigned* key[2] = {w.succ[0], w.succ[1]};
    unsigned* val[2] = {w.dist[0], w.dist[1]};
    const int64_t nbb = scan_blocks(B), nbm = scan_blocks(M);
    const FlUnwalkedFlag uflag{w, boundary_labels, V};
    hipLaunchKernelGGL((scan_sum_kernel<unsigned, FlUnwalkedFlag>), dim3((unsigned)nbb), blk, 0, s, uflag, B, w.bsum_s);
    RNB_CHECK_LAUNCH();
    hipLaunchKernelGGL(scan_block_sums_kernel<unsigned>, dim3(1), dim3(1024), 0, s, w.bsum_s, nbb, (unsigned*)nullptr, (int64_t)0, 1,
                       (int64_t*)w.totals);
    RNB_CHECK_LAUNCH();
    hipLaunchKernelGGL((scan_emit_kernel<unsigned, FlUnwalkedFlag, FlUnwalkedEmit>), dim3((unsigned)nbb), blk, 0, s, uflag,
                       FlUnwalkedEmit{w, boundary_labels, key[0], val[0], M}, B, w.bsum_s);
    RNB_CHECK_LAUNCH();
    int bits = 0;
    while (((L - 1) >> bits) != 0) ++bits;
    for (int b = 0; b < bits; ++b) {
      const FlBitZero zero{key[b & 1], b};
      hipLaunchKernelGGL((scan_sum_kernel<unsigned, FlBitZero>), dim3((unsigned)nbm), blk, 0, s, zero, M, w.bsum_s);
      RNB_CHECK_LAUNCH();
      hipLaunchKernelGGL(scan_block_sums_kernel<unsigned>, dim3(1), dim3(1024), 0, s, w.bsum_s, nbm, (unsigned*)nullptr, (int64_t)0, 1,
                         (int64_t*)w.totals);
      RNB_CHECK_LAUNCH();
      hipLaunchKernelGGL((scan_emit_kernel<unsigned, FlBitZero, FlSplitEmit>), dim3((unsigned)nbm), blk, 0, s, zero,
                         FlSplitEmit{key[b & 1], val[b & 1], key[(b + 1) & 1], val[(b + 1) & 1], w.totals, M}, M, w.bsum_s);
      RNB_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(fl_place_sorted_kernel, dim3(fl_grid(M)), blk, 0, s, M, L, B, key[bits & 1], val[bits & 1], loop_offsets,
                       loop_vertices);
    RNB_CHECK_LAUNCH();
  }
  return RNB_OK;
}

RNB_API int rnb_mesh_loops_mean(const void* values, int32_t value_type, int64_t n_vertices, int64_t n_columns,
                                const int64_t* loop_offsets, const int32_t* loop_vertices, int64_t n_loops,
                                int64_t n_boundary_vertices, void* workspace, size_t workspace_bytes, void* means,
                                rnb_stream_t stream) {
  using namespace rnb;
  const char* who = "rnb_mesh_loops_mean";
  const int64_t V = n_vertices, L = n_loops, B = n_boundary_vertices, C = n_columns;
  FlWs w;
  RNB_TRY(fl_check(who, V, 0, workspace, workspace_bytes, &w));
  if (value_type != 0 && value_type != 1) RNB_FAIL(RNB_E_INVALID, "%s: value_type %d is neither 0 (float64) nor 1 (float32)", who, value_type);
  RNB_TRY(mesh_count(who, C, "columns"));
  RNB_TRY(fl_check_csr(who, V, L, B, loop_offsets, loop_vertices));
  if (L == 0 || C == 0) return RNB_OK;
  if (!means || (B > 0 && !values)) RNB_FAIL(RNB_E_NULL, "%s: NULL values / means", who);
  hipStream_t s = (hipStream_t)stream;
  if (value_type == 0) return fl_means((const double*)values, V, C, loop_offsets, loop_vertices, L, B, w, (double*)means, s);
  return fl_means((const float*)values, V, C, loop_offsets, loop_vertices, L, B, w, (float*)means, s);
}

RNB_API int rnb_mesh_fill_emit(const double* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles,
                               const int64_t* loop_offsets, const int32_t* loop_vertices, const uint8_t* loop_status,
                               const double* loop_centroid, int64_t n_loops, int64_t n_boundary_vertices, int64_t max_edges,
                               void* workspace, size_t workspace_bytes, int64_t n_filled, int64_t n_new_triangles,
                               double* vertices_out, int32_t* triangles_out, int32_t* filled, rnb_stream_t stream) {
  using namespace rnb;
  const char* who = "rnb_mesh_fill_emit";
  const int64_t V = n_vertices, T = n_triangles, L = n_loops, B = n_boundary_vertices, F = n_filled, N = n_new_triangles;
  FlWs w;
  RNB_TRY(fl_check(who, V, T, workspace, workspace_bytes, &w));
  RNB_TRY(fl_check_csr(who, V, L, B, loop_offsets, loop_vertices));
  if (F < 0 || F > L || N < 0 || N > B) RNB_FAIL(RNB_E_INVALID, "%s: %lld filled loops / %lld new triangles", who, (long long)F, (long long)N);
  if (V + F > kMeshMax || T + N > kMeshMax)
    RNB_FAIL(RNB_E_INVALID, "%s: the filled mesh would have more than 2^31 - 1 vertices or triangles", who);
  if ((V > 0 && !vertices) || (T > 0 && !triangles)) RNB_FAIL(RNB_E_NULL, "%s: NULL vertices / triangles", who);
  if ((V + F > 0 && !vertices_out) || (T + N > 0 && !triangles_out)) RNB_FAIL(RNB_E_NULL, "%s: NULL output", who);
  if (F > 0 && (!loop_status || !loop_centroid || !filled)) RNB_FAIL(RNB_E_NULL, "%s: NULL loop_status / loop_centroid / filled", who);
  hipStream_t s = (hipStream_t)stream;
  const dim3 blk(kFlThreads);
  if (V > 0) RNB_CHECK_HIP(hipMemcpyAsync(vertices_out, vertices, (size_t)V * 3 * sizeof(double), hipMemcpyDeviceToDevice, s));
  if (T > 0) RNB_CHECK_HIP(hipMemcpyAsync(triangles_out, triangles, (size_t)T * 3 * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
  if (F == 0) return RNB_OK;
  const FlCsr csr{loop_offsets, loop_status, max_edges};
  const int64_t nbl = scan_blocks(L);
  hipLaunchKernelGGL((scan_sum_kernel<unsigned, FlFilledFlag>), dim3((unsigned)nbl), blk, 0, s, FlFilledFlag{csr}, L, w.bsum_l[0]);
  RNB_CHECK_LAUNCH();
  hipLaunchKernelGGL((scan_sum_kernel<unsigned, FlFilledSize>), dim3((unsigned)nbl), blk, 0, s, FlFilledSize{csr}, L, w.bsum_l[1]);
  RNB_CHECK_LAUNCH();
  hipLaunchKernelGGL(scan_block_sums_kernel<unsigned>, dim3(1), dim3(1024), 0, s, w.bsum_l[0], nbl, w.bsum_l[1], nbl, 2,
                     (int64_t*)w.totals);
  RNB_CHECK_LAUNCH();
  hipLaunchKernelGGL((scan_emit_kernel<unsigned, FlFilledFlag, FlStoreEmit>), dim3((unsigned)nbl), blk, 0, s, FlFilledFlag{csr},
                     FlStoreEmit{w.frank}, L, w.bsum_l[0]);
  RNB_CHECK_LAUNCH();
  hipLaunchKernelGGL((scan_emit_kernel<unsigned, FlFilledSize, FlStoreEmit>), dim3((unsigned)nbl), blk, 0, s, FlFilledSize{csr},
                     FlStoreEmit{w.trioff}, L, w.bsum_l[1]);
  RNB_CHECK_LAUNCH();
  hipLaunchKernelGGL(fl_cap_vertex_kernel, dim3(fl_grid(L)), blk, 0, s, L, V, F, csr, w, loop_centroid, vertices_out, filled);
  RNB_CHECK_LAUNCH();
  if (B > 0 && N > 0) {
    hipLaunchKernelGGL(fl_cap_triangle_kernel, dim3(fl_grid(B)), blk, 0, s, L, B, V, T, F, N, csr, w, loop_vertices, triangles_out);
    RNB_CHECK_LAUNCH();
  }
  return RNB_OK;
}
