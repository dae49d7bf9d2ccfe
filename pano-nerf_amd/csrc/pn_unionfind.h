// pn_unionfind.h — the schedule-independent union-find of pn_emitters.hip (pixels) and pn_meshops.hip (mesh vertices): one
// definition of the loop, so the termination argument is made once.
//
// parent[i] is an index of the same array, or -1 for an element that takes no part.  INVARIANT (P1): a stored value is
// never larger than its own index: the initialising kernel stores i itself (or -1), and the only later writer is
// atomicMin(&parent[a], b) with b < a, which can only lower it.  So parent[i] <= i at every moment, for every reader,
// however stale its copy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

__device__ __forceinline__ int32_t load_parent(const int32_t* parent, int32_t i) {
    return __hip_atomic_load(parent + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root above i.  Ends: by (P1) every step either stops (parent[i] == i) or moves to a strictly smaller index >= 0, so
// there are at most i steps, whatever other waves write meanwhile.
__device__ __forceinline__ int32_t find_root(const int32_t* parent, int32_t i) {
    for (;;) {
        const int32_t q = load_parent(parent, i);
        if (q == i) return i;
        i = q;
    }
}

// Join the trees of a and b; the smaller root survives.  The standard label-equivalence form: try to hang the larger root
// a under the smaller b with atomicMin; if a had stopped being a root in between (the atomic returned old != a), the edge
// a -> old it held has been replaced by a -> min(old, b), so what is still owed is the union of old and b: retry from the
// value the atomic returned.
// Ends: let (a, b) be the pair after the two find_root calls and the swap, a > b.  A retry continues with (old, b) where
// old = the value the atomic returned != a, hence old < a by (P1); find_root never raises an index.  So the sum a + b of
// the pair falls by at least 1 per retry and is bounded below by 0: at most a + b retries, each of finitely many steps,
// independent of the schedule.
// Result: edges always point from a larger to a smaller index of the same component and every owed union is carried by
// the wave that owes it until it is paid, so when the launch is over every component is one tree whose root is its
// smallest index - whatever the order in which the atomics landed.
__device__ inline void unite(int32_t* parent, int32_t a, int32_t b) {
    for (;;) {
        a = find_root(parent, a);
        b = find_root(parent, b);
        if (a == b) return;
        if (a < b) {
            const int32_t t = a;
            a = b;
            b = t;
        }
        const int32_t old = atomicMin(parent + a, b);
        if (old == a) return;  // a was a root and now hangs under b
        a = old;
    }
}
