// Evaluation metrics of a label volume: the per-class ingredients of Dice and HD95 (utils.py:48-58; medpy.metric.binary dc /
// hd95 with connectivity 1 and unit voxel spacing) for ALL classes of a (D, H, W) prediction / label pair.
//
// Everything is integer.  With unit spacing a squared Euclidean distance between voxels is an integer, so the device returns
//   counts[c] = {|P_c|, |G_c|, |P_c n G_c|, |dP_c| + |dG_c|}                                   (64-bit)
//   hist[c][s] = number of border voxels of P_c (G_c) whose nearest border voxel of G_c (P_c) is at squared distance s
// and the host takes square roots and one percentile in float64: the result is the host path's, not an approximation of it.
// Only integer atomics are used, so two runs return the same bits.
//
// Layout.  A voxel belongs to one class, so ONE byte map per volume holds the borders of all classes: bmap[v] = id if v is a
// border voxel of its class (set, and some face neighbour is another class or outside the array -- what
// mask ^ binary_erosion(mask, cross, border_value=0) leaves), else 0.  The border pass also takes, per class, the bounding box
// of the border voxels of both volumes together: seeds and queries of a class all lie inside it, so the exact transform of a
// class only ever looks at that box (organs are small).
// Per class c and direction (seeds = border of one volume, queries = border of the other), restricted to the box:
//   x pass  g1[z][y][x] = min_x' |x - x'| over seeds of row (z, y), uint16, G1_NONE where the row has no seed
//   y pass  g2[z][y][x] = min_y' g1[z][y'][x]^2 + (y - y')^2, int32, a column of the box per lane held in LDS
//   z pass  at query voxels only: d2 = min_z' g2[z'][y][x] + (z - z')^2, hist[c][d2] += 1; nothing else is written
// The y and z minima are bounded brute force: candidates are visited by growing |dy| and the walk stops once dy^2 >= best, which
// no farther candidate can beat -- exact, and short because queries sit close to seeds.
// Classes with an empty side are skipped on the device (every kernel reads counts[c] and leaves): no host round trip.
#include "common.h"

namespace {

constexpr int SM_MAX_DIM = 2048;           // per dimension: 3 * 2047^2 + G1_NONE^2 stays inside int32
constexpr int G1_NONE = 0x7FFF;            // "no seed in this row"; its square (1 073 676 289) exceeds every real squared distance
constexpr int SM_MAX_CLS = 255;
constexpr int BC_VOX = 16;                 // voxels per thread of the border pass (one 16-B load per volume)

struct SegDims {
    int D, H, W, ndim, ncls;
};

__device__ __forceinline__ unsigned wave_sum_u32(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ void seg_box_init_kernel(int* __restrict__ box, int ncls) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < ncls * 6) box[i] = (i & 1) ? -1 : 0x7FFFFFFF;          // {z0, z1, y0, y1, x0, x1}: min slots even, max slots odd
}

// border status of voxel (z, y, x) = v of `a` with class id `id`: on the array's edge, or beside another class
__device__ __forceinline__ bool seg_is_border(const unsigned char* __restrict__ a, long v, int z, int y, int x, int id,
                                              const SegDims& s, long HW) {
    if (x == 0 || x == s.W - 1 || y == 0 || y == s.H - 1) return true;
    if (a[v - 1] != id || a[v + 1] != id || a[v - s.W] != id || a[v + s.W] != id) return true;
    if (s.ndim == 3) {
        if (z == 0 || z == s.D - 1) return true;
        if (a[v - HW] != id || a[v + HW] != id) return true;
    }
    return false;
}

// One sweep over both volumes: byte maps of the borders, the four counts per class, the per-class box of all border voxels.
// A thread owns 16 consecutive voxels.  Background (id 0) is most of a volume: its counts stay in registers and meet in one
// wave sum; foreground voxels add to per-workgroup LDS tallies; one 64-bit global atomic per touched class per workgroup.
__global__ __launch_bounds__(256) void seg_border_count_kernel(const unsigned char* __restrict__ pred,
                                                               const unsigned char* __restrict__ label,
                                                               unsigned char* __restrict__ bmP, unsigned char* __restrict__ bmG,
                                                               unsigned long long* __restrict__ counts, int* __restrict__ box,
                                                               SegDims s, long N, int vec_ok) {
    __shared__ unsigned tally[(SM_MAX_CLS + 1) * 4];
    __shared__ int lbox[(SM_MAX_CLS + 1) * 6];
    for (int i = threadIdx.x; i < s.ncls * 4; i += 256) tally[i] = 0u;
    for (int i = threadIdx.x; i < s.ncls * 6; i += 256) lbox[i] = (i & 1) ? -1 : 0x7FFFFFFF;
    __syncthreads();

    const long HW = (long)s.H * s.W;
    const long v0 = ((long)blockIdx.x * 256 + threadIdx.x) * BC_VOX;
    unsigned bg[4] = {0u, 0u, 0u, 0u};
    if (v0 < N) {
        alignas(16) unsigned char p[BC_VOX], g[BC_VOX], op[BC_VOX], og[BC_VOX];
        const bool full = v0 + BC_VOX <= N;
        if (full && vec_ok) {
            *reinterpret_cast<u32x4*>(p) = *reinterpret_cast<const u32x4*>(pred + v0);
            *reinterpret_cast<u32x4*>(g) = *reinterpret_cast<const u32x4*>(label + v0);
        } else {
#pragma unroll
            for (int j = 0; j < BC_VOX; ++j) {
                p[j] = v0 + j < N ? pred[v0 + j] : 0;
                g[j] = v0 + j < N ? label[v0 + j] : 0;
            }
        }
        int z = (int)(v0 / HW);
        const long r = v0 - (long)z * HW;
        int y = (int)(r / s.W), x = (int)(r - (long)y * s.W);
#pragma unroll
        for (int j = 0; j < BC_VOX; ++j) {
            const long v = v0 + j;
            op[j] = 0;
            og[j] = 0;
            if (v < N) {
                const int ip = p[j], ig = g[j];
                const bool okp = ip < s.ncls, okg = ig < s.ncls;          // ids >= ncls are the caller's error: never counted
                const bool bp = okp && seg_is_border(pred, v, z, y, x, ip, s, HW);
                const bool bgd = okg && seg_is_border(label, v, z, y, x, ig, s, HW);
                if (bp) op[j] = (unsigned char)ip;
                if (bgd) og[j] = (unsigned char)ig;
                if (okp) {
                    if (ip == 0) {
                        bg[0] += 1u;
                        bg[3] += bp ? 1u : 0u;
                    } else {
                        atomicAdd(&tally[ip * 4 + 0], 1u);
                        if (bp) atomicAdd(&tally[ip * 4 + 3], 1u);
                    }
                }
                if (okg) {
                    if (ig == 0) {
                        bg[1] += 1u;
                        bg[3] += bgd ? 1u : 0u;
                    } else {
                        atomicAdd(&tally[ig * 4 + 1], 1u);
                        if (bgd) atomicAdd(&tally[ig * 4 + 3], 1u);
                    }
                }
                if (okp && ip == ig) {
                    if (ip == 0) bg[2] += 1u;
                    else atomicAdd(&tally[ip * 4 + 2], 1u);
                }
#pragma unroll
                for (int side = 0; side < 2; ++side) {
                    const int id = side ? ig : ip;
                    if ((side ? bgd : bp) && id != 0) {
                        int* b = lbox + id * 6;
                        atomicMin(b + 0, z);
                        atomicMax(b + 1, z);
                        atomicMin(b + 2, y);
                        atomicMax(b + 3, y);
                        atomicMin(b + 4, x);
                        atomicMax(b + 5, x);
                    }
                }
            }
            if (++x == s.W) {
                x = 0;
                if (++y == s.H) {
                    y = 0;
                    ++z;
                }
            }
        }
        if (full && vec_ok) {
            *reinterpret_cast<u32x4*>(bmP + v0) = *reinterpret_cast<const u32x4*>(op);
            *reinterpret_cast<u32x4*>(bmG + v0) = *reinterpret_cast<const u32x4*>(og);
        } else {
#pragma unroll
            for (int j = 0; j < BC_VOX; ++j)
                if (v0 + j < N) {
                    bmP[v0 + j] = op[j];
                    bmG[v0 + j] = og[j];
                }
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const unsigned t = wave_sum_u32(bg[k]);
        if ((threadIdx.x & 63) == 0 && t) atomicAdd(&tally[k], t);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < s.ncls * 4; i += 256)
        if (tally[i]) atomicAdd(&counts[i], (unsigned long long)tally[i]);
    for (int i = threadIdx.x; i < s.ncls * 6; i += 256) {
        if (i & 1) {
            if (lbox[i] >= 0) atomicMax(&box[i], lbox[i]);
        } else if (lbox[i] != 0x7FFFFFFF) atomicMin(&box[i], lbox[i]);
    }
}

struct SegBox {
    int z0, z1, y0, y1, x0, x1;
};
// the box of class c, or false when a side of the class is empty (nothing to measure: its hist row stays zero)
__device__ __forceinline__ bool seg_class_box(const unsigned long long* __restrict__ counts, const int* __restrict__ box, int c,
                                              SegBox& b) {
    if (counts[c * 4 + 0] == 0ull || counts[c * 4 + 1] == 0ull) return false;
    b.z0 = box[c * 6 + 0], b.z1 = box[c * 6 + 1], b.y0 = box[c * 6 + 2], b.y1 = box[c * 6 + 3], b.x0 = box[c * 6 + 4], b.x1 = box[c * 6 + 5];
    return b.z1 >= b.z0;
}

// x pass: one wave per row (z, y) of the box and per direction (blockIdx.y: 0 = seeds from the label's borders, 1 = from the
// prediction's).  Two sweeps over the row in 64-voxel chunks, the seed flags of a chunk as one ballot: left to right for the
// nearest seed at or before x, right to left for the nearest at or after it.  A lane meets the same x in both sweeps, so the
// LDS row it parks the first distance in needs no barrier.
__global__ __launch_bounds__(256) void seg_edt_x_kernel(const unsigned char* __restrict__ bmP, const unsigned char* __restrict__ bmG,
                                                        unsigned short* __restrict__ g1, const unsigned long long* __restrict__ counts,
                                                        const int* __restrict__ box, SegDims s, long N, int c) {
    __shared__ unsigned short rowbuf[4][SM_MAX_DIM];
    SegBox b;
    if (!seg_class_box(counts, box, c, b)) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long row = (long)blockIdx.x * 4 + wave;
    if (row >= (long)s.D * s.H) return;
    const int z = (int)(row / s.H), y = (int)(row - (long)z * s.H);
    if (z < b.z0 || z > b.z1 || y < b.y0 || y > b.y1) return;
    const int dir = blockIdx.y;
    const unsigned char* __restrict__ seeds = (dir == 0 ? bmG : bmP) + row * s.W;
    unsigned short* __restrict__ out = g1 + (long)dir * N + row * s.W;
    const int nchunk = (b.x1 - b.x0 + 64) >> 6;
    int last = -1;
    for (int k = 0; k < nchunk; ++k) {
        const int xb = b.x0 + (k << 6), x = xb + lane;
        const bool seed = x <= b.x1 && seeds[x] == c;
        const unsigned long long mask = __ballot(seed);
        const unsigned long long m = mask & (lane == 63 ? ~0ull : ((2ull << lane) - 1ull));
        const int pos = m ? xb + 63 - __clzll((long long)m) : last;
        if (x <= b.x1) rowbuf[wave][x - b.x0] = (unsigned short)(pos < 0 ? G1_NONE : x - pos);
        if (mask) last = xb + 63 - __clzll((long long)mask);
    }
    int next = -1;
    for (int k = nchunk - 1; k >= 0; --k) {
        const int xb = b.x0 + (k << 6), x = xb + lane;
        const bool seed = x <= b.x1 && seeds[x] == c;
        const unsigned long long mask = __ballot(seed);
        const unsigned long long m = mask & (~0ull << lane);
        const int pos = m ? xb + __ffsll((long long)m) - 1 : next;
        if (x <= b.x1) {
            const int dl = rowbuf[wave][x - b.x0], dr = pos < 0 ? G1_NONE : pos - x;
            out[x] = (unsigned short)(dl < dr ? dl : dr);
        }
        if (mask) next = xb + __ffsll((long long)mask) - 1;
    }
}

// y pass: a workgroup takes TX columns of one plane z of the box (TX * H * 2 B of LDS: the host picks TX from H), one column
// per lane so that the loads of g1 and the stores of g2 are contiguous across lanes.  A plane without any seed is answered
// with the constant G1_NONE^2 instead of H-long walks.
__global__ __launch_bounds__(256) void seg_edt_y_kernel(const unsigned short* __restrict__ g1, int* __restrict__ g2,
                                                        const unsigned long long* __restrict__ counts, const int* __restrict__ box,
                                                        SegDims s, long N, int c, int TX) {
    extern __shared__ unsigned short col[];          // [hb][TX]
    SegBox b;
    if (!seg_class_box(counts, box, c, b)) return;
    const int z = blockIdx.y, dir = blockIdx.z, xt = blockIdx.x * TX;
    if (z < b.z0 || z > b.z1 || xt > b.x1 || xt + TX <= b.x0) return;
    const int cx = threadIdx.x % TX, yg = threadIdx.x / TX, G = 256 / TX;
    const int x = xt + cx, hb = b.y1 - b.y0 + 1;
    const bool live = x >= b.x0 && x <= b.x1;
    const long base = (long)dir * N + ((long)z * s.H + b.y0) * s.W + x;
    int any = 0;
    for (int yy = yg; yy < hb; yy += G) {
        const unsigned short g = live ? g1[base + (long)yy * s.W] : (unsigned short)G1_NONE;
        col[yy * TX + cx] = g;
        any |= g != G1_NONE;
    }
    any = __syncthreads_or(any);
    if (!live) return;
    if (!any) {
        for (int yy = yg; yy < hb; yy += G) g2[base + (long)yy * s.W] = G1_NONE * G1_NONE;
        return;
    }
    for (int yy = yg; yy < hb; yy += G) {
        const int g = col[yy * TX + cx];
        int best = g * g;
        for (int d = 1;; ++d) {
            const int d2 = d * d;
            const bool lo = yy - d >= 0, hi = yy + d < hb;
            if (d2 >= best || !(lo || hi)) break;
            if (lo) {
                const int t = col[(yy - d) * TX + cx];
                best = min(best, t * t + d2);
            }
            if (hi) {
                const int t = col[(yy + d) * TX + cx];
                best = min(best, t * t + d2);
            }
        }
        g2[base + (long)yy * s.W] = best;
    }
}

// z pass, at the queries only: the other volume's border voxels of class c.  Walks the planes of the box outward from the
// query's own and stops as for y; adds one to the class's histogram row at the squared distance found.
__global__ __launch_bounds__(256) void seg_edt_z_hist_kernel(const unsigned char* __restrict__ bmP, const unsigned char* __restrict__ bmG,
                                                             const int* __restrict__ g2, unsigned* __restrict__ hist,
                                                             const unsigned long long* __restrict__ counts,
                                                             const int* __restrict__ box, SegDims s, long N, int c, int nbins) {
    SegBox b;
    if (!seg_class_box(counts, box, c, b)) return;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int z = blockIdx.z >> 1, dir = blockIdx.z & 1;
    if (z < b.z0 || z > b.z1 || y < b.y0 || y > b.y1 || x < b.x0 || x > b.x1) return;
    const long HW = (long)s.H * s.W, v = (long)z * HW + (long)y * s.W + x;
    if ((dir == 0 ? bmP : bmG)[v] != c) return;
    const int* __restrict__ g = g2 + (long)dir * N + (long)y * s.W + x;
    int best = g[(long)z * HW];
    for (int d = 1;; ++d) {
        const int d2 = d * d;
        const bool lo = z - d >= b.z0, hi = z + d <= b.z1;
        if (d2 >= best || !(lo || hi)) break;
        if (lo) best = min(best, g[(long)(z - d) * HW] + d2);
        if (hi) best = min(best, g[(long)(z + d) * HW] + d2);
    }
    if (best < nbins) atomicAdd(&hist[(long)c * nbins + best], 1u);
}

bool seg_dims_ok(int D, int H, int W) { return D >= 1 && H >= 1 && W >= 1 && D <= SM_MAX_DIM && H <= SM_MAX_DIM && W <= SM_MAX_DIM; }

size_t up16(size_t n) { return (n + 15) & ~(size_t)15; }

}  // namespace

extern "C" {

// number of histogram bins: every squared distance inside the volume, 0 .. (D-1)^2 + (H-1)^2 + (W-1)^2
int cswin_seg_metrics_nbins(int D, int H, int W) {
    if (!seg_dims_ok(D, H, W)) {
        cswin_set_error("seg_metrics: volume %dx%dx%d outside the supported 1..%d per dimension", D, H, W, SM_MAX_DIM);
        return 0;
    }
    return (D - 1) * (D - 1) + (H - 1) * (H - 1) + (W - 1) * (W - 1) + 1;
}

// two border byte maps, g1 (uint16) and g2 (int32) for both directions of one class, the per-class boxes
size_t cswin_seg_metrics_workspace(int D, int H, int W, int ndim, int ncls) {
    if (!seg_dims_ok(D, H, W)) {
        cswin_set_error("seg_metrics: volume %dx%dx%d outside the supported 1..%d per dimension", D, H, W, SM_MAX_DIM);
        return 0;
    }
    if (!(ndim == 3 || (ndim == 2 && D == 1))) {
        cswin_set_error("seg_metrics: ndim must be 3, or 2 with D == 1 (got ndim=%d, D=%d)", ndim, D);
        return 0;
    }
    if (ncls < 2 || ncls > SM_MAX_CLS) {
        cswin_set_error("seg_metrics: ncls=%d outside 2..%d", ncls, SM_MAX_CLS);
        return 0;
    }
    const size_t N = (size_t)D * H * W;
    return 2 * up16(N) + up16(2 * N * sizeof(unsigned short)) + up16(2 * N * sizeof(int)) + up16((size_t)ncls * 6 * sizeof(int));
}

int cswin_seg_metrics(const unsigned char* pred, const unsigned char* label, long long* counts, unsigned int* hist,
                      void* workspace, size_t ws_bytes, int D, int H, int W, int ndim, int ncls, void* stream) {
    CSWIN_REQUIRE(pred && label && counts && hist, CSWIN_ERR_SHAPE, "seg_metrics: null argument");
    const size_t need = cswin_seg_metrics_workspace(D, H, W, ndim, ncls);          // sets the message for a bad shape
    if (need == 0) return CSWIN_ERR_SHAPE;
    CSWIN_REQUIRE(workspace && ws_bytes >= need, CSWIN_ERR_WORKSPACE, "seg_metrics: workspace of %zu bytes, %zu needed", ws_bytes, need);
    CSWIN_REQUIRE((uintptr_t)workspace % 16 == 0, CSWIN_ERR_ALIGN, "seg_metrics: workspace must be 16-B aligned");
    CSWIN_REQUIRE((uintptr_t)counts % 8 == 0 && (uintptr_t)hist % 4 == 0, CSWIN_ERR_ALIGN, "seg_metrics: counts / hist misaligned");
    hipStream_t st = (hipStream_t)stream;
    const long N = (long)D * H * W;
    const int nbins = cswin_seg_metrics_nbins(D, H, W);
    const SegDims s = {D, H, W, ndim, ncls};

    char* w = (char*)workspace;
    unsigned char* bmP = (unsigned char*)w;
    unsigned char* bmG = bmP + up16((size_t)N);
    unsigned short* g1 = (unsigned short*)(bmG + up16((size_t)N));
    int* g2 = (int*)((char*)g1 + up16(2 * (size_t)N * sizeof(unsigned short)));
    int* box = (int*)((char*)g2 + up16(2 * (size_t)N * sizeof(int)));

    if (hipMemsetAsync(counts, 0, (size_t)ncls * 4 * sizeof(long long), st) != hipSuccess ||
        hipMemsetAsync(hist, 0, (size_t)ncls * nbins * sizeof(unsigned), st) != hipSuccess) {
        cswin_set_error("seg_metrics: hipMemsetAsync failed");
        return CSWIN_ERR_HIP;
    }
    hipLaunchKernelGGL(seg_box_init_kernel, dim3(cdiv(ncls * 6, 256)), dim3(256), 0, st, box, ncls);
    CSWIN_LAUNCH_CHECK();
    const int vec_ok = (uintptr_t)pred % 16 == 0 && (uintptr_t)label % 16 == 0;
    hipLaunchKernelGGL(seg_border_count_kernel, dim3((unsigned)((N + 256 * BC_VOX - 1) / (256 * BC_VOX))), dim3(256), 0, st, pred, label,
                       bmP, bmG, (unsigned long long*)counts, box, s, N, vec_ok);
    CSWIN_LAUNCH_CHECK();

    const int TX = H <= 512 ? 64 : (H <= 1024 ? 32 : 16);          // TX * H * 2 B of LDS <= 64 KiB
    const long rows = (long)D * H;
    for (int c = 1; c < ncls; ++c) {                                  // row 0 (background) stays zero
        hipLaunchKernelGGL(seg_edt_x_kernel, dim3((unsigned)((rows + 3) / 4), 2), dim3(256), 0, st, bmP, bmG, g1,
                           (const unsigned long long*)counts, box, s, N, c);
        hipLaunchKernelGGL(seg_edt_y_kernel, dim3(cdiv(W, TX), D, 2), dim3(256), (size_t)TX * H * sizeof(unsigned short), st, g1, g2,
                           (const unsigned long long*)counts, box, s, N, c, TX);
        hipLaunchKernelGGL(seg_edt_z_hist_kernel, dim3(cdiv(W, 64), cdiv(H, 4), 2 * D), dim3(256), 0, st, bmP, bmG, g2, hist,
                           (const unsigned long long*)counts, box, s, N, c, nbins);
        CSWIN_LAUNCH_CHECK();
    }
    return CSWIN_OK;
}

}  // extern "C"
