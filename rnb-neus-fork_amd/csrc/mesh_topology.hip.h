// What the topology audit (mesh_topology.hip) leaves in its workspace and what a later call needs to read it: the layout of
// the workspace of rnb_mesh_topology_count, the class of an edge from its two use counts, and the 128-bit integer
// accumulator of the bit-reproducible sums (the signed volume there, the loop means of mesh_fill.hip).  mesh_fill.hip reads
// the half-edge arrays the count wrote; it never writes them.  Integer code apart from the one conversion at the end, which
// is exact up to its single rounding under any floating-point flags.
#pragma once
#include <math.h>

#include "mesh_table.hip.h"
#include "rnb_internal.h"
#include "scan.hip.h"

namespace rnb {

constexpr unsigned long long kTpNoKey = ~0ull;
constexpr unsigned kTpNone = 0xffffffffu;
constexpr int64_t kTpMaxTriangles = 1431655764;        // 3 T <= 2^32 - 4: a half-edge index fits a 32-bit slot, all ones stays free
enum { TP_BOUNDARY = 1, TP_FLIPPED = 2, TP_NONMANIFOLD = 4, TP_DEGENERATE = 8, TP_INVALID = 16 };   // triangle flags
enum { TP_V_UNUSED = 8 };                                                                            // vertex flags: 1, 2, 4 as above
enum { TP_INFO_BOUNDARY = 0, TP_INFO_ERROR = 1 };   // words of TpWs::info: boundary components were made; a table walk failed

struct TpWs {
  unsigned* info;             // [64]  see TP_INFO_*
  unsigned long long* key;    // [3T]  edge key of the half-edge, all ones = its triangle is not proper
  unsigned* lead;             // [3T]  smallest half-edge of the same edge, all ones = none
  unsigned* nfwd;             // [3T]  (by leader) forward uses
  unsigned* nbwd;             // [3T]  (by leader) backward uses
  unsigned* tab;              // [cap] the edge table
  unsigned* bsum;             // block sums of the leader scan
  unsigned* vword;            // [V]   vertex flag word
  uint8_t* vref;              // [V]   named by a proper triangle
  uint8_t* broot;             // [V]   smallest vertex of its boundary component
  unsigned* rank;             // [V]   dense id of a boundary root
  unsigned* bsum_v;
  // the component call's own part (the count and the emit never touch it)
  unsigned long long* maxbits;  // [V] largest |term| of the component, as bits
  unsigned long long* lo;       // [V] the fixed-point volume sum, low and high word
  unsigned long long* hi;
  unsigned* cflags;             // [V]
  uint64_t cap;
};

static TpWs tp_carve(Carver& c, int64_t V, int64_t T) {
  TpWs w;
  const int64_t H = 3 * T;
  w.cap = mesh_table_capacity(H);
  w.info = c.take<unsigned>(64);
  w.key = c.take<unsigned long long>(H);
  w.lead = c.take<unsigned>(H);
  w.nfwd = c.take<unsigned>(H);
  w.nbwd = c.take<unsigned>(H);
  w.tab = c.take<unsigned>((int64_t)w.cap);
  w.bsum = c.take<unsigned>(scan_pad64(scan_blocks(H)));
  w.vword = c.take<unsigned>(V);
  w.vref = c.take<uint8_t>(V);
  w.broot = c.take<uint8_t>(V);
  w.rank = c.take<unsigned>(V);
  w.bsum_v = c.take<unsigned>(scan_pad64(scan_blocks(V)));
  w.maxbits = c.take<unsigned long long>(V);      // at most one component per vertex
  w.lo = c.take<unsigned long long>(V);
  w.hi = c.take<unsigned long long>(V);
  w.cflags = c.take<unsigned>(V);
  return w;
}

// one add per wave: the number of lanes with `pred`
__device__ inline void tp_wave_count(long long* counter, bool pred) {
  const unsigned long long m = __ballot(pred);
  if (m && (threadIdx.x & 63) == (unsigned)(__ffsll((long long)m) - 1))
    atomicAdd((unsigned long long*)counter, (unsigned long long)__popcll(m));
}

// class bit of an edge used n_fwd times forward and n_bwd times backward (0: manifold)
__device__ inline unsigned tp_class(unsigned nf, unsigned nb) {
  const unsigned n = nf + nb;
  if (n == 1) return TP_BOUNDARY;
  if (n == 2) return nf == 1 ? 0u : TP_FLIPPED;
  return TP_NONMANIFOLD;
}

// ---- the 128-bit two's-complement sum of scaled terms -------------------------------------------------------------------
// A term x of a sum whose largest |term| is tmax > 0 enters in units of 2^(e - 54), e = ilogb(tmax): |scaled| < 2^55, rounded
// to nearest (an error of at most 2^-55 of the largest per term), sign-extended to 128 bits and added as integers.
__device__ inline long long wide_scaled(double x, double tmax) { return llrint(ldexp(x, 54 - ilogb(tmax))); }

// (lo, hi) += the 128-bit value (add_lo, add_hi), with integer atomics on the two words
__device__ inline void wide_add(unsigned long long* lo, unsigned long long* hi, unsigned long long add_lo,
                                unsigned long long add_hi) {
  unsigned long long carry = 0;
  if (add_lo) {
    const unsigned long long old = atomicAdd(lo, add_lo);
    carry = old + add_lo < old ? 1ull : 0ull;
  }
  if (add_hi + carry) atomicAdd(hi, add_hi + carry);
}

// the finished sum as a double with ONE rounding, times 2^(e - 54); tmax > 0
__device__ inline double wide_to_double(unsigned long long lo, unsigned long long hi, double tmax) {
  const bool neg = (hi >> 63) != 0;
  if (neg) {                                               // magnitude: two's-complement negation
    lo = ~lo + 1ull;
    hi = ~hi + (lo == 0 ? 1ull : 0ull);
  }
  double m;
  int shift = 0;
  if (hi == 0) m = (double)lo;
  else {                                                   // the top 64 bits, what is below them as a sticky bit
    const int lz = __clzll((long long)hi);
    shift = 64 - lz;
    unsigned long long top = lz ? (hi << lz) | (lo >> (64 - lz)) : hi;
    const bool sticky = (lz ? (lo << lz) : lo) != 0;
    top |= sticky ? 1ull : 0ull;
    m = (double)top;
  }
  const double v = ldexp(m, shift + ilogb(tmax) - 54);
  return neg ? -v : v;
}

}  // namespace rnb
