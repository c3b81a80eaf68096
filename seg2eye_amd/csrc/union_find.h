// Min-union over an array of parents, written once for the three memories it runs on: a tile's parents in LDS, the
// image's parents in global memory, and a plain host array (a stand-alone program can include this header and run the same loops
// under a host sanitizer).  The memory is a policy with two members:
//   int load(int i)                 the parent of i; where other workgroups update the array, an agent-scope atomic load
//   int fetch_min(int i, int v)     parent[i] = min(parent[i], v), atomically; -> the value before
// Invariant: parent[i] <= i, and parent[i] == i exactly at a root.  Parents only ever decrease, so every loop below is bounded by the
// index it starts from, whatever other lanes do meanwhile; a value read late is still an ancestor of the node it was read for.
#pragma once

#if defined(__HIPCC__)
#define S2E_UF_FN __host__ __device__ __forceinline__
#else
#define S2E_UF_FN inline
#endif

// the root of i: follow the parents until one is its own
template <typename Mem> S2E_UF_FN int uf_find(Mem& m, int i) {
    int p = m.load(i);
    while (p != i) {
        i = p;
        p = m.load(i);
    }
    return i;
}

// the same with path halving: every node passed is hung on its grandparent (an ancestor, so fetch_min keeps the invariant and the
// set), which shortens the chains the next finds walk.  For the global array, where a step is a trip to the L2.
template <typename Mem> S2E_UF_FN int uf_find_halving(Mem& m, int i) {
    int p = m.load(i);
    while (p != i) {
        const int g = m.load(p);
        if (g != p) m.fetch_min(i, g);
        i = p;
        p = g;
    }
    return i;
}

// join the sets of a and b under the smaller of their roots.  Find both roots, fetch_min the larger root's parent with the smaller
// root; when the value before is not that root, another lane has hung it elsewhere meanwhile: go on from that value.
template <bool HALVING, typename Mem> S2E_UF_FN void uf_union(Mem& m, int a, int b) {
    for (;;) {
        a = HALVING ? uf_find_halving(m, a) : uf_find(m, a);
        b = HALVING ? uf_find_halving(m, b) : uf_find(m, b);
        if (a == b) return;
        if (a > b) { const int t = a; a = b; b = t; }
        const int before = m.fetch_min(b, a);
        if (before == b) return;
        b = before;                                          // (before < b: the loop's measure, the sum of the two indices, has gone down)
    }
}

// The neighbours of a pixel that precede it in raster order: left, up, and with 8-connectivity up-left and up-right.  Every adjacent
// pair of pixels is seen exactly once, from its later pixel.  f(dx, dy) is called for each.
template <typename F> S2E_UF_FN void uf_back_neighbours(int conn, F&& f) {
    f(-1, 0);
    f(0, -1);
    if (conn == 8) {
        f(-1, -1);
        f(1, -1);
    }
}
