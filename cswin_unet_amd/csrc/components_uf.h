// Union-find core of the connected-component kernels (components.hip), host and device.
//
// A forest over voxel indices with ONE invariant: parent[i] <= i, with equality exactly at a root.  Every write keeps it:
// a parent is only ever replaced by a smaller index (fetch_min).  The root of a component is therefore its smallest index, and
// every loop below follows a strictly decreasing index: it ends after at most (start index) steps whatever other threads do in
// the meantime.  No loop waits for another thread's progress.
//
// `Mem` is how the forest is reached: load(i) -> parent[i], fetch_min(i, v) -> old parent[i], parent[i] = min(old, v) as one
// atomic step.  components.hip has the LDS and the global (agent-scope atomic) forms; HostForest is the single-threaded one that
// tools/components_host_check.cpp runs the same code through on the CPU.
#pragma once

#if defined(__HIPCC__)
#define CC_HD __host__ __device__ __forceinline__
#else
#define CC_HD inline
#endif

// the tile of the tile pass, (z, y, x): 4096 voxels = 256 threads x 16 consecutive voxels of a row (ops.COMPONENT_TILE)
constexpr int CC_TZ = 4, CC_TY = 16, CC_TX = 64;
constexpr int CC_TILE_VOX = CC_TZ * CC_TY * CC_TX;
constexpr int CC_VOX = 16;          // voxels per thread (one 16-B load)

template <class Mem>
CC_HD int cc_find(const Mem& m, int x) {
    // terminates: p < x at every step taken (parent[i] <= i; anything else is read as a root), so x strictly decreases
    for (;;) {
        const int p = m.load(x);
        if (p >= x || p < 0) return x;
        x = p;
    }
}

// Unite the components of a and b: hang the larger of the two roots under the smaller with fetch_min.  If another thread
// re-parented that root first, fetch_min returns what it had put there (old < a): the forest now holds a -> min(old, b), and
// what is left to unite is old with b.
template <class Mem>
CC_HD void cc_union(const Mem& m, int a, int b) {
    // terminates: after a round that does not return, the new pair is (old, b) with old < a and b < a, and the finds only
    // lower both: max(a, b) strictly decreases from round to round and is >= 0
    for (;;) {
        a = cc_find(m, a);
        b = cc_find(m, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = m.fetch_min(a, b);
        if (old == a) return;
        a = old;
    }
}

// A same-class link across the face between v and its neighbour n (v - 1 row / plane / column) needs no union of its own when
// the voxel before v along an in-face axis of the SAME tile row (vp, np) carries the same class on both sides: vp ~ v and
// np ~ n are unions of the tile pass, vp ~ np is the previous voxel's link (or follows from this rule again).
CC_HD bool cc_link_needed(int id, int nb, int id_prev, int nb_prev) { return id != 0 && nb == id && !(id_prev == id && nb_prev == id); }

struct HostForest {
    int* p;
    int load(int i) const { return p[i]; }
    int fetch_min(int i, int v) const {
        const int old = p[i];
        if (v < old) p[i] = v;
        return old;
    }
};
