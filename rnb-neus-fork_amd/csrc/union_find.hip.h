// The lock-free union-find of the mesh tools: vertex components (mesh_clean.hip) and boundary components
// (mesh_topology.hip).  parent[] is an int array with parent[x] = x for every x before the first uf_unite; the root of a
// class ends up its smallest member, whatever the schedule.  Integer only.
//
// WHY A KERNEL OF uf_unite CALLS CANNOT HANG.  Invariant: parent[x] <= x for every x at every instant.  It holds after the
// initialisation (parent[x] = x) and every write keeps it: the compare-and-swap of uf_unite replaces parent[a] == a by b < a,
// the atomicMin of uf_find only lowers an entry.  Consequences:
//   - an entry with parent[x] < x never becomes a root again (entries only decrease), and every value ever stored in parent[x]
//     is an ancestor of x in the forest of that moment, hence in the same component;
//   - every uf_find walk strictly descends (x -> parent[x] < x) and ends after at most x steps: no cycle can form, and a
//     stale read only shows an older ancestor;
//   - a compare-and-swap fails only when parent[a] != a, i.e. another thread's hook of the same root SUCCEEDED in between:
//     a failure is progress of another thread.  The retry continues from the value read, which is < a, so one uf_unite retries
//     at most a + b times, and over the whole launch at most V - 1 hooks succeed.
// No thread ever waits for a value another thread has yet to write: there is no spin-wait, no lock, no host-side
// convergence loop, and the result (roots = smallest member of each class) does not depend on the schedule.
#pragma once
#include "rnb_internal.h"

namespace rnb {

__device__ inline int uf_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Root of x.  Every step goes to parent[x] < x, so the walk ends after at most x steps whatever other threads do.  On the
// way parent[x] is lowered to its grandparent (path halving): atomicMin with an ancestor of x that is smaller than x.
__device__ inline int uf_find(int* parent, int x) {
  for (;;) {
    const int p = uf_load(parent + x);
    if (p == x) return x;
    const int gp = uf_load(parent + p);
    if (gp < p) atomicMin(parent + x, gp);
    x = p;
  }
}

// Lock-free union: hook the larger root under the smaller with one compare-and-swap on the root's own entry.
__device__ inline void uf_unite(int* parent, int a, int b) {
  for (;;) {
    a = uf_find(parent, a);
    b = uf_find(parent, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }          // a: the larger root
    const int old = atomicCAS(parent + a, a, b);
    if (old == a) return;                                   // hooked
    a = old;                                                // a stopped being a root: old < a, go on from there
  }
}

}  // namespace rnb
