// Connected components of a multi-class label volume and the per-class size filter built on them (what a CT evaluation does
// with scipy.ndimage.label per class on the host: keep an organ's large components, drop the stray specks, then score).
//
// Everything is integer and exact.  vol is (D, H, W) uint8, ids 0 and >= ncls are background.  Two voxels share a component iff
// they carry the same foreground id and a chain of face neighbours of that id joins them.  The label of a voxel is
// 1 + (smallest flat index of its component), 0 for background: it does not depend on scheduling, so two runs give the same
// bits.  sizes[r] = voxel count of the component whose smallest index is r, 0 elsewhere.
//
// Union-find with integer atomics only (components_uf.h: parent[i] <= i, roots are minima, every loop strictly descends):
//   tile pass     one workgroup per CC_TZ x CC_TY x CC_TX tile, union-find in LDS; parent[v] = global index of v's tile-local
//                 root, tcnt[v] = voxel count of that tile-local component at its root, 0 elsewhere.  No cross-workgroup traffic.
//   seam pass     every voxel on a low tile face whose neighbour across the face has its id: union of the two in global memory.
//                 Workgroups of this launch write and read one another's parents, so EVERY read of parent here is a relaxed
//                 agent-scope atomic load and every write an agent-scope atomic min: both are served where all CUs meet, never
//                 from a CU's own L1 (which other CUs' writes do not refresh).  Nothing is handed over through a flag, so there
//                 is no fence: a find that reads an older parent only starts higher up the same chain, and the fetch_min that
//                 decides a union returns the true previous value.
//   flatten pass  (its own launch: the kernel boundary publishes the seam pass) labels[v] = 1 + find(v) into the output buffer,
//                 never into parent; every tile-local root adds its count ONCE to sizes[final root] -- a whole-organ component
//                 takes one atomic per tile it touches, not one per voxel.
// Filter: per-class largest component by integer atomicMax, the threshold formed on the device in float64, one streaming pass.
#include "common.h"
#include "components_uf.h"

namespace {

constexpr int CC_MAX_DIM = 2048;
constexpr int CC_MAX_CLS = 255;
constexpr long CC_MAX_N = 2147483646L;          // labels are 1 + index in int32
constexpr int CC_TAB = 256;                      // per-class table entries at the head of the workspace
constexpr int CF_VOX = 4;                        // voxels per thread of the filter pass

struct CcDims {
    int D, H, W, ncls;
    int nx, ny;          // tiles along x and y
};

struct LdsForest {
    int* p;
    __device__ __forceinline__ int load(int i) const { return __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
    __device__ __forceinline__ int fetch_min(int i, int v) const { return atomicMin(p + i, v); }
};
struct GlobalForest {          // shared by the workgroups of one launch: agent-scope atomics only
    int* p;
    __device__ __forceinline__ int load(int i) const { return __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ int fetch_min(int i, int v) const {
        return __hip_atomic_fetch_min(p + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};
struct FrozenForest {          // a forest no one writes in this launch: plain loads
    const int* p;
    __device__ __forceinline__ int load(int i) const { return p[i]; }
};

// a thread's place: tile (blockIdx.x), row (lz, ly) of the tile and the 16-voxel segment of that row
struct CcPlace {
    int lz, ly, seg, z, y, x0, nvalid;          // nvalid: how many of the 16 voxels lie inside the volume
    long v0;                                    // flat index of the first
    int bz, by, bx;
};
__device__ __forceinline__ CcPlace cc_place(const CcDims& s) {
    CcPlace p;
    const int b = blockIdx.x;
    p.bx = b % s.nx;
    const int t = b / s.nx;
    p.by = t % s.ny;
    p.bz = t / s.ny;
    const int row = threadIdx.x >> 2;
    p.seg = threadIdx.x & 3;
    p.lz = row / CC_TY;
    p.ly = row % CC_TY;
    p.z = p.bz * CC_TZ + p.lz;
    p.y = p.by * CC_TY + p.ly;
    p.x0 = p.bx * CC_TX + p.seg * CC_VOX;
    const int left = s.W - p.x0;
    p.nvalid = (p.z < s.D && p.y < s.H && left > 0) ? (left < CC_VOX ? left : CC_VOX) : 0;
    p.v0 = ((long)p.z * s.H + p.y) * s.W + p.x0;
    return p;
}

__device__ __forceinline__ unsigned char cc_fg(unsigned char b, int ncls) { return b < ncls ? b : (unsigned char)0; }

// ids of the n <= 16 voxels from flat index v on (0 beyond n; ids >= ncls read as background): one 16-B load where the
// address allows it, bytes otherwise (ragged row ends, W or a base pointer that is no multiple of 16)
__device__ __forceinline__ void cc_load16(const unsigned char* __restrict__ vol, long v, int n, int ncls, unsigned char* id) {
    if (n == CC_VOX && ((uintptr_t)(vol + v) & 15) == 0) {
        *reinterpret_cast<u32x4*>(id) = *reinterpret_cast<const u32x4*>(vol + v);
#pragma unroll
        for (int j = 0; j < CC_VOX; ++j) id[j] = cc_fg(id[j], ncls);
    } else {
#pragma unroll
        for (int j = 0; j < CC_VOX; ++j) id[j] = j < n ? cc_fg(vol[v + j], ncls) : (unsigned char)0;
    }
}

__global__ __launch_bounds__(256) void cc_tile_kernel(const unsigned char* __restrict__ vol, int* __restrict__ parent,
                                                      int* __restrict__ tcnt, CcDims s) {
    __shared__ int lpar[CC_TILE_VOX];
    __shared__ int lcnt[CC_TILE_VOX];
    __shared__ alignas(16) unsigned char lid[CC_TILE_VOX];
    const CcPlace p = cc_place(s);
    const int l0 = threadIdx.x * CC_VOX;          // = (lz * CC_TY + ly) * CC_TX + seg * 16: local and global order agree inside a tile
    alignas(16) unsigned char id[CC_VOX];
    cc_load16(vol, p.v0, p.nvalid, s.ncls, id);

    // runs of one id inside the thread's 16 voxels hang under their first voxel: no atomics
    int run = l0;
#pragma unroll
    for (int j = 0; j < CC_VOX; ++j) {
        if (!(j > 0 && id[j] != 0 && id[j] == id[j - 1])) run = l0 + j;
        lpar[l0 + j] = run;
        lcnt[l0 + j] = 0;
    }
    *reinterpret_cast<u32x4*>(lid + l0) = *reinterpret_cast<const u32x4*>(id);
    __syncthreads();

    const LdsForest F = {lpar};
    const int idm1 = p.seg > 0 ? lid[l0 - 1] : 0;          // the voxel before the segment, 0 at the tile's low x face
    if (p.seg > 0 && id[0] != 0 && idm1 == id[0]) cc_union(F, l0, l0 - 1);
#pragma unroll
    for (int axis = 0; axis < 2; ++axis) {                  // the row above (y - 1), then the plane below (z - 1), inside the tile
        const int back = axis == 0 ? CC_TX : CC_TY * CC_TX;
        if (axis == 0 ? p.ly == 0 : p.lz == 0) continue;
        alignas(16) unsigned char nb[CC_VOX];
        *reinterpret_cast<u32x4*>(nb) = *reinterpret_cast<const u32x4*>(lid + l0 - back);
        const int nbm1 = p.seg > 0 ? lid[l0 - back - 1] : 0;
#pragma unroll
        for (int j = 0; j < CC_VOX; ++j)
            if (cc_link_needed(id[j], nb[j], j ? id[j - 1] : idm1, j ? nb[j - 1] : nbm1)) cc_union(F, l0 + j, l0 + j - back);
    }
    __syncthreads();

    // nobody writes lpar any more.  parent[v] = global index of the tile-local root (-1: background), one LDS add per run of a root
    const FrozenForest R = {lpar};
    int out[CC_VOX];
    int prev = -1, n = 0;
#pragma unroll
    for (int j = 0; j < CC_VOX; ++j) {
        out[j] = -1;
        if (id[j] != 0) {
            const int r = cc_find(R, l0 + j);
            if (r != prev) {
                if (n) atomicAdd(&lcnt[prev], n);
                prev = r;
                n = 0;
            }
            ++n;
            const int rz = r / (CC_TY * CC_TX), ry = (r / CC_TX) % CC_TY, rx = r % CC_TX;
            out[j] = (int)(((long)(p.bz * CC_TZ + rz) * s.H + (p.by * CC_TY + ry)) * s.W + (p.bx * CC_TX + rx));
        }
    }
    if (n) atomicAdd(&lcnt[prev], n);
    const bool vec = p.nvalid == CC_VOX && (p.v0 & 3) == 0;          // parent and tcnt are 16-B aligned workspace arrays
    if (vec) {
#pragma unroll
        for (int q = 0; q < CC_VOX / 4; ++q) *reinterpret_cast<int4*>(parent + p.v0 + 4 * q) = make_int4(out[4 * q], out[4 * q + 1], out[4 * q + 2], out[4 * q + 3]);
    } else {
#pragma unroll
        for (int j = 0; j < CC_VOX; ++j)
            if (j < p.nvalid) parent[p.v0 + j] = out[j];
    }
    __syncthreads();
    if (vec) {
#pragma unroll
        for (int q = 0; q < CC_VOX / 4; ++q) *reinterpret_cast<int4*>(tcnt + p.v0 + 4 * q) = *reinterpret_cast<const int4*>(lcnt + l0 + 4 * q);
    } else {
#pragma unroll
        for (int j = 0; j < CC_VOX; ++j)
            if (j < p.nvalid) tcnt[p.v0 + j] = lcnt[l0 + j];
    }
}

// Seam pass.  Same thread placement as the tile pass; only threads on a low face of their tile that has a tile beyond it work.
// `parent` is deliberately not __restrict__ / const: it is only touched through GlobalForest's atomics.
__global__ __launch_bounds__(256) void cc_seam_kernel(const unsigned char* __restrict__ vol, int* parent, CcDims s) {
    const CcPlace p = cc_place(s);
    const bool fz = p.lz == 0 && p.z > 0, fy = p.ly == 0 && p.y > 0, fx = p.seg == 0 && p.x0 > 0;
    if (p.nvalid == 0 || !(fz || fy || fx)) return;
    const GlobalForest F = {parent};
    const long HW = (long)s.H * s.W;
    alignas(16) unsigned char id[CC_VOX];
    cc_load16(vol, p.v0, p.nvalid, s.ncls, id);
    const int idm1 = p.seg > 0 ? cc_fg(vol[p.v0 - 1], s.ncls) : 0;          // same tile only: 0 at the tile's low x face
#pragma unroll
    for (int axis = 0; axis < 2; ++axis) {                                   // the face towards y - 1, then towards z - 1
        if (!(axis == 0 ? fy : fz)) continue;
        const long back = axis == 0 ? (long)s.W : HW;
        alignas(16) unsigned char nb[CC_VOX];
        cc_load16(vol, p.v0 - back, p.nvalid, s.ncls, nb);
        const int nbm1 = p.seg > 0 ? cc_fg(vol[p.v0 - back - 1], s.ncls) : 0;
#pragma unroll
        for (int j = 0; j < CC_VOX; ++j)
            if (j < p.nvalid && cc_link_needed(id[j], nb[j], j ? id[j - 1] : idm1, j ? nb[j - 1] : nbm1))
                cc_union(F, (int)(p.v0 + j), (int)(p.v0 + j - back));
    }
    if (fx) {                                                                // the face towards x - 1: the in-face axis is y
        const int nb = cc_fg(vol[p.v0 - 1], s.ncls);
        const bool in_tile = p.ly > 0;
        const int idp = in_tile ? cc_fg(vol[p.v0 - s.W], s.ncls) : 0, nbp = in_tile ? cc_fg(vol[p.v0 - s.W - 1], s.ncls) : 0;
        if (cc_link_needed(id[0], nb, idp, nbp)) cc_union(F, (int)p.v0, (int)(p.v0 - 1));
    }
}

__global__ __launch_bounds__(256) void cc_flatten_kernel(const int* __restrict__ parent, const int* __restrict__ tcnt,
                                                         int* __restrict__ labels, int* __restrict__ sizes, long N) {
    const long v = (long)blockIdx.x * 256 + threadIdx.x;
    if (v >= N) return;
    const FrozenForest R = {parent};
    const int q = parent[v];
    if (q < 0) {
        labels[v] = 0;
        return;
    }
    const int r = cc_find(R, q);
    labels[v] = r + 1;
    if (sizes) {
        const int t = tcnt[v];          // > 0 exactly at the tile-local roots
        if (t > 0) atomicAdd(&sizes[r], t);
    }
}

// largest[c] = size of the biggest component of class c: sizes is non-zero exactly at component roots
__global__ __launch_bounds__(256) void cc_largest_kernel(const unsigned char* __restrict__ vol, const int* __restrict__ sizes,
                                                         int* __restrict__ largest, int ncls, long N) {
    __shared__ int tab[CC_TAB];
    tab[threadIdx.x] = 0;
    __syncthreads();
    const long v = (long)blockIdx.x * 256 + threadIdx.x;
    if (v < N) {
        const int sz = sizes[v];
        if (sz > 0) {
            const int c = cc_fg(vol[v], ncls);
            if (c) atomicMax(&tab[c], sz);
        }
    }
    __syncthreads();
    if (tab[threadIdx.x] > 0) atomicMax(&largest[threadIdx.x], tab[threadIdx.x]);
}

// out[v] = 0 where v's component is smaller than its class's threshold, vol[v] elsewhere.  vol and out may be the same buffer
// (a thread reads its own voxels before it writes them), hence no __restrict__ on the two.
__global__ __launch_bounds__(256) void cc_filter_kernel(const unsigned char* vol, const int* __restrict__ labels,
                                                        const int* __restrict__ sizes, const long long* __restrict__ min_size,
                                                        const double* __restrict__ min_fraction, const int* __restrict__ largest,
                                                        unsigned char* out, int ncls, long N, int vec_ok) {
    __shared__ long long thr[CC_TAB];
    {
        const int c = threadIdx.x;
        long long t = 0;
        if (c > 0 && c < ncls) {
            const long long frac = (long long)ceil(min_fraction[c] * (double)largest[c]);
            t = min_size[c] > frac ? min_size[c] : frac;
        }
        thr[c] = t;
    }
    __syncthreads();
    const long v0 = ((long)blockIdx.x * 256 + threadIdx.x) * CF_VOX;
    if (v0 >= N) return;
    if (vec_ok && v0 + CF_VOX <= N) {
        const unsigned w = *reinterpret_cast<const unsigned*>(vol + v0);
        unsigned o = w;
        if (w) {
            const int4 lab = *reinterpret_cast<const int4*>(labels + v0);
            const int l[CF_VOX] = {lab.x, lab.y, lab.z, lab.w};
#pragma unroll
            for (int j = 0; j < CF_VOX; ++j) {
                const int id = (w >> (8 * j)) & 0xFF;
                if (l[j] > 0 && id < ncls && (long long)sizes[l[j] - 1] < thr[id]) o &= ~(0xFFu << (8 * j));
            }
        }
        *reinterpret_cast<unsigned*>(out + v0) = o;
    } else {
        for (int j = 0; j < CF_VOX && v0 + j < N; ++j) {
            const int id = vol[v0 + j], l = labels[v0 + j];
            out[v0 + j] = (unsigned char)((l > 0 && id < ncls && (long long)sizes[l - 1] < thr[id]) ? 0 : id);
        }
    }
}

// 0 with the message set, or N
long cc_check_dims(const char* who, int D, int H, int W) {
    if (!(D >= 1 && H >= 1 && W >= 1 && D <= CC_MAX_DIM && H <= CC_MAX_DIM && W <= CC_MAX_DIM)) {
        cswin_set_error("%s: volume %dx%dx%d outside the supported 1..%d per dimension", who, D, H, W, CC_MAX_DIM);
        return 0;
    }
    const long N = (long)D * H * W;
    if (N > CC_MAX_N) {
        cswin_set_error("%s: volume %dx%dx%d has %ld voxels, more than the %ld an int32 label can name", who, D, H, W, N, CC_MAX_N);
        return 0;
    }
    return N;
}

size_t cc_up16(size_t n) { return (n + 15) & ~(size_t)15; }

bool cc_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

}  // namespace

extern "C" {

// the per-class table (zeroed by a memset node of its own, at the allocation's start), then parent and tcnt, N int32 each
size_t cswin_components_workspace(int D, int H, int W) {
    const long N = cc_check_dims("components", D, H, W);
    if (N == 0) return 0;
    return CC_TAB * sizeof(int) + 2 * cc_up16((size_t)N * sizeof(int));
}

int cswin_components_label(const unsigned char* vol, int* labels, int* sizes, void* workspace, size_t ws_bytes, int D, int H,
                           int W, int ncls, void* stream) {
    CSWIN_REQUIRE(vol && labels, CSWIN_ERR_SHAPE, "components_label: null argument");
    const long N = cc_check_dims("components_label", D, H, W);
    if (N == 0) return (D >= 1 && H >= 1 && W >= 1 && D <= CC_MAX_DIM && H <= CC_MAX_DIM && W <= CC_MAX_DIM) ? CSWIN_ERR_UNSUPPORTED : CSWIN_ERR_SHAPE;
    CSWIN_REQUIRE(ncls >= 2 && ncls <= CC_MAX_CLS, CSWIN_ERR_UNSUPPORTED, "components_label: ncls=%d outside 2..%d", ncls, CC_MAX_CLS);
    const size_t need = cswin_components_workspace(D, H, W);
    CSWIN_REQUIRE(workspace && ws_bytes >= need, CSWIN_ERR_WORKSPACE, "components_label: workspace of %zu bytes, %zu needed", ws_bytes, need);
    CSWIN_REQUIRE((uintptr_t)workspace % 16 == 0, CSWIN_ERR_ALIGN, "components_label: workspace must be 16-B aligned");
    CSWIN_REQUIRE((uintptr_t)labels % 4 == 0 && (uintptr_t)sizes % 4 == 0, CSWIN_ERR_ALIGN, "components_label: labels / sizes misaligned");
    const size_t nb = (size_t)N * sizeof(int);
    CSWIN_REQUIRE(!cc_overlap(labels, nb, vol, (size_t)N) && !cc_overlap(labels, nb, workspace, need) && !cc_overlap(vol, (size_t)N, workspace, need) &&
                      (!sizes || (!cc_overlap(sizes, nb, vol, (size_t)N) && !cc_overlap(sizes, nb, labels, nb) && !cc_overlap(sizes, nb, workspace, need))),
                  CSWIN_ERR_UNSUPPORTED, "components_label: vol, labels, sizes and the workspace must not overlap");
    hipStream_t st = (hipStream_t)stream;
    int* parent = (int*)((char*)workspace + CC_TAB * sizeof(int));
    int* tcnt = (int*)((char*)parent + cc_up16(nb));
    const CcDims s = {D, H, W, ncls, cdiv(W, CC_TX), cdiv(H, CC_TY)};
    const unsigned tiles = (unsigned)((long)s.nx * s.ny * cdiv(D, CC_TZ));          // <= 32 * 128 * 512
    if (sizes && hipMemsetAsync(sizes, 0, nb, st) != hipSuccess) {
        cswin_set_error("components_label: hipMemsetAsync failed");
        return CSWIN_ERR_HIP;
    }
    hipLaunchKernelGGL(cc_tile_kernel, dim3(tiles), dim3(256), 0, st, vol, parent, tcnt, s);
    CSWIN_LAUNCH_CHECK();
    hipLaunchKernelGGL(cc_seam_kernel, dim3(tiles), dim3(256), 0, st, vol, parent, s);
    CSWIN_LAUNCH_CHECK();
    hipLaunchKernelGGL(cc_flatten_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, (const int*)parent, (const int*)tcnt, labels, sizes, N);
    CSWIN_LAUNCH_CHECK();
    return CSWIN_OK;
}

int cswin_components_filter(const unsigned char* vol, const int* labels, const int* sizes, const long long* min_size,
                            const double* min_fraction, unsigned char* out, void* workspace, size_t ws_bytes, int D, int H, int W,
                            int ncls, void* stream) {
    CSWIN_REQUIRE(vol && labels && sizes && min_size && min_fraction && out, CSWIN_ERR_SHAPE, "components_filter: null argument");
    const long N = cc_check_dims("components_filter", D, H, W);
    if (N == 0) return (D >= 1 && H >= 1 && W >= 1 && D <= CC_MAX_DIM && H <= CC_MAX_DIM && W <= CC_MAX_DIM) ? CSWIN_ERR_UNSUPPORTED : CSWIN_ERR_SHAPE;
    CSWIN_REQUIRE(ncls >= 2 && ncls <= CC_MAX_CLS, CSWIN_ERR_UNSUPPORTED, "components_filter: ncls=%d outside 2..%d", ncls, CC_MAX_CLS);
    const size_t need = cswin_components_workspace(D, H, W);
    CSWIN_REQUIRE(workspace && ws_bytes >= need, CSWIN_ERR_WORKSPACE, "components_filter: workspace of %zu bytes, %zu needed", ws_bytes, need);
    CSWIN_REQUIRE((uintptr_t)workspace % 16 == 0, CSWIN_ERR_ALIGN, "components_filter: workspace must be 16-B aligned");
    CSWIN_REQUIRE((uintptr_t)labels % 4 == 0 && (uintptr_t)sizes % 4 == 0 && (uintptr_t)min_size % 8 == 0 && (uintptr_t)min_fraction % 8 == 0,
                  CSWIN_ERR_ALIGN, "components_filter: labels / sizes / min_size / min_fraction misaligned");
    const size_t nb = (size_t)N * sizeof(int), tab = CC_TAB * sizeof(int);
    CSWIN_REQUIRE(out == vol || !cc_overlap(out, (size_t)N, vol, (size_t)N), CSWIN_ERR_UNSUPPORTED,
                  "components_filter: out must be vol itself or not overlap it");
    CSWIN_REQUIRE(!cc_overlap(out, (size_t)N, labels, nb) && !cc_overlap(out, (size_t)N, sizes, nb) && !cc_overlap(out, (size_t)N, workspace, tab) &&
                      !cc_overlap(out, (size_t)N, min_size, (size_t)ncls * 8) && !cc_overlap(out, (size_t)N, min_fraction, (size_t)ncls * 8) &&
                      !cc_overlap(workspace, tab, vol, (size_t)N) && !cc_overlap(workspace, tab, labels, nb) && !cc_overlap(workspace, tab, sizes, nb),
                  CSWIN_ERR_UNSUPPORTED, "components_filter: out and the workspace must not overlap the other arguments");
    hipStream_t st = (hipStream_t)stream;
    int* largest = (int*)workspace;
    if (hipMemsetAsync(largest, 0, tab, st) != hipSuccess) {
        cswin_set_error("components_filter: hipMemsetAsync failed");
        return CSWIN_ERR_HIP;
    }
    hipLaunchKernelGGL(cc_largest_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, vol, sizes, largest, ncls, N);
    CSWIN_LAUNCH_CHECK();
    const int vec_ok = (uintptr_t)vol % 4 == 0 && (uintptr_t)out % 4 == 0 && (uintptr_t)labels % 16 == 0;
    hipLaunchKernelGGL(cc_filter_kernel, dim3((unsigned)((N + 256 * CF_VOX - 1) / (256 * CF_VOX))), dim3(256), 0, st, vol, labels, sizes, min_size,
                       min_fraction, (const int*)largest, out, ncls, N, vec_ok);
    CSWIN_LAUNCH_CHECK();
    return CSWIN_OK;
}

}  // extern "C"
