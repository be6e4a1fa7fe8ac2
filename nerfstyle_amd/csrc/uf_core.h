// Lock-free union-find over vertex ids, written once for the device (mesh_clean.hip) and for the host
// (tests/uf_stress.cpp runs it from many threads).  parent[v] <= v always; a root is a v with parent[v] == v.
//
// Why the result does not depend on the interleaving: a hook is a compare-and-swap parent[hi]: hi -> lo with lo < hi, taken
// only while hi is still a root, and path halving only ever stores an ancestor through an atomic min, so every parent only
// decreases and every tree's root is its smallest id.  Once every edge has been united, a component is one tree, and its root
// is the component's minimum id whatever order the hooks were taken in.
//
// Every read of parent[] below is a relaxed atomic load or the value a compare-and-swap returned, never a plain load: on the
// device (eight XCDs whose L2s are not coherent inside one kernel) a plain load in the retry loop could be served stale for
// ever.  No fences: nothing is read through parent[] but parent[] itself, and the labels are read after the kernel's end.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define UF_FN __device__ __forceinline__
UF_FN uint32_t uf_load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// -> the value found at *p (== expect iff the swap was made)
UF_FN uint32_t uf_cas(uint32_t *p, uint32_t expect, uint32_t want) {
    __hip_atomic_compare_exchange_strong(p, &expect, want, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return expect;
}
UF_FN void uf_min(uint32_t *p, uint32_t v) { (void)__hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
#else
#define UF_FN static inline
UF_FN uint32_t uf_load(const uint32_t *p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
UF_FN uint32_t uf_cas(uint32_t *p, uint32_t expect, uint32_t want) {
    __atomic_compare_exchange_n(p, &expect, want, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED);
    return expect;
}
UF_FN void uf_min(uint32_t *p, uint32_t v) {
    uint32_t cur = uf_load(p);
    while (v < cur) {
        const uint32_t seen = uf_cas(p, cur, v);
        if (seen == cur) break;
        cur = seen;
    }
}
#endif

// The root of x's tree at some moment of the call; path halving on the way (every other node is pointed at its grandparent).
// Ends: the ids walked strictly decrease.
UF_FN uint32_t uf_find(uint32_t *parent, uint32_t x) {
    for (;;) {
        const uint32_t p = uf_load(parent + x);
        if (p == x) return x;
        const uint32_t g = uf_load(parent + p);
        if (g == p) return p;
        uf_min(parent + x, g);                      // g is an ancestor of x, and below p
        x = g;
    }
}

// Joins the trees of a and b.  A failed hook means another thread hooked `hi` first: the value the compare-and-swap returned
// is hi's new parent, and the walk goes on from there.  Ends: each retry starts from an id below the one that failed.
UF_FN void uf_unite(uint32_t *parent, uint32_t a, uint32_t b) {
    uint32_t ra = uf_find(parent, a), rb = uf_find(parent, b);
    while (ra != rb) {
        const uint32_t hi = ra > rb ? ra : rb, lo = ra > rb ? rb : ra;
        const uint32_t seen = uf_cas(parent + hi, hi, lo);
        if (seen == hi) return;                     // hooked: the larger root under the smaller id
        ra = uf_find(parent, seen);
        rb = lo;
    }
}
