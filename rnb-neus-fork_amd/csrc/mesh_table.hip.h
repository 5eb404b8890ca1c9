// The open-addressing table "key -> smallest item index" of the mesh tools: the cell table and the triple table of
// mesh_simplify.hip, the edge table of mesh_topology.hip.  An array of `cap` 32-bit slots, cap a power of two >= 2 x (number
// of items), every slot kTabEmpty before the first insertion.  A slot holds an ITEM INDEX, never a key: `same(cur)` says
// whether item `cur` has the key of the item being inserted, from arrays a PREVIOUS kernel wrote.  Why an insertion ends,
// and why every item of one key ends in one slot which then holds the key's smallest index: the argument at the head of
// mesh_simplify.hip ("THE TWO TABLES"), which speaks of exactly this loop.  Integer only: a file compiled with any
// floating-point flags may include it.
#pragma once
#include "rnb_internal.h"

namespace rnb {

constexpr unsigned kTabEmpty = 0xffffffffu;

static inline uint64_t mesh_table_capacity(int64_t n_items) {
  uint64_t c = 64;
  while (c < 2 * (uint64_t)n_items) c <<= 1;
  return c;
}

// Item `item` with hash `hash` enters the table.  Returns the slot it stopped at, or `cap` when the walk used up its cap
// steps (which the sizing excludes: the caller raises an error bit, nothing spins).
template <class Same>
__device__ inline uint64_t mesh_table_insert(unsigned* tab, uint64_t cap, unsigned item, unsigned long long hash, Same same) {
  const uint64_t mask = cap - 1;
  uint64_t s = hash & mask;
  for (uint64_t step = 0; step < cap; ++step, s = (s + 1) & mask) {
    const unsigned cur = atomicCAS(tab + s, kTabEmpty, item);
    if (cur != kTabEmpty) {
      if (!same(cur)) continue;
      atomicMin(tab + s, item);
    }
    return s;
  }
  return cap;
}

// After the inserting kernel has finished: the smallest item of the key whose hash is `hash`, or kTabEmpty when no item of
// that key entered.  The walk is the insertion's: it passes the slots of other keys and stops at the key's one slot, or at
// the empty slot the first item of the key would have filled.
template <class Same>
__device__ inline unsigned mesh_table_find(const unsigned* __restrict__ tab, uint64_t cap, unsigned long long hash, Same same) {
  const uint64_t mask = cap - 1;
  uint64_t s = hash & mask;
  for (uint64_t step = 0; step < cap; ++step, s = (s + 1) & mask) {
    const unsigned cur = tab[s];
    if (cur == kTabEmpty) return kTabEmpty;
    if (same(cur)) return cur;
  }
  return kTabEmpty;
}

}  // namespace rnb
