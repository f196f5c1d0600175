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
//
// With a voxel spacing (sz, sy, sx) squared distances stop being integers and there is no histogram to index.  The second entry
// point, cswin_surface_dist, runs the same border and x passes (|dx| stays an integer) and the same y and z walks under another
// metric (SpacedMetric below, float64): the y pass keeps per voxel the (|dx|, |dy|) of its in-plane argmin, packed in the 32 bits
// the unit path keeps a squared distance in, and the z pass evaluates (dz sz)^2 + (dy sy)^2 + (dx sx)^2 -- the expression scipy's
// distance_transform_edt(sampling=...) evaluates, products and sums rounded one by one -- and stores it in a compacted list:
// segment (c, dir) starts at the exclusive prefix sum of the border counts nq[c][dir] (formed on the device after the border
// pass), slots inside a segment come from an integer atomic counter.  The multiset of a segment is the same on every run; its
// order is not, and the caller sorts.
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

// What the y and z passes minimise.  Best is the running minimum of a walk, cell_t what the y pass leaves per voxel for the z pass.
// UnitMetric: unit spacing, everything an int32; a row or plane without a seed carries G1_NONE^2.
struct UnitMetric {
    using val_t = int;
    using cell_t = int;
    struct Best {
        int v;
    };
    __device__ static cell_t no_seed() { return G1_NONE * G1_NONE; }
    __device__ val_t ystep(int d) const { return d * d; }
    __device__ Best yinit(int g) const { return {g * g}; }
    __device__ void ytake(Best& b, int t, int, val_t d2) const { b.v = min(b.v, t * t + d2); }
    __device__ cell_t ycell(const Best& b) const { return b.v; }
    __device__ val_t zstep(int d) const { return d * d; }
    __device__ Best zinit(cell_t q) const { return {q}; }
    __device__ void ztake(Best& b, cell_t q, val_t d2) const { b.v = min(b.v, q + d2); }
};

// SpacedMetric: float64 under the spacing (sz, sy, sx).  A cell is |dx| | |dy| << 16 of the in-plane argmin (both < 2048), or
// NO_SEED, whose distance is +inf.  This file is built with -ffp-contract=off: a product is rounded before it is added, as numpy
// rounds it.
struct SpacedMetric {
    double sz, sy, sx;
    using val_t = double;
    using cell_t = unsigned;
    struct Best {
        double v;
        unsigned arg;
    };
    static constexpr unsigned NO_SEED = 0xFFFFFFFFu;
    __device__ static cell_t no_seed() { return NO_SEED; }
    __device__ static double sq(int d, double w) {
        const double t = (double)d * w;
        return t * t;
    }
    __device__ static double sum(double a, double b) { return a + b; }
    __device__ val_t ystep(int d) const { return sq(d, sy); }
    __device__ Best yinit(int g) const { return g == G1_NONE ? Best{__builtin_inf(), NO_SEED} : Best{sq(g, sx), (unsigned)g}; }
    __device__ void ytake(Best& b, int t, int d, val_t d2) const {
        if (t == G1_NONE) return;
        const double v = sum(d2, sq(t, sx));
        if (v < b.v) b = {v, (unsigned)t | ((unsigned)d << 16)};
    }
    __device__ cell_t ycell(const Best& b) const { return b.arg; }
    __device__ val_t zstep(int d) const { return sq(d, sz); }
    __device__ double at(cell_t q, double dz2) const {
        return q == NO_SEED ? __builtin_inf() : sum(sum(dz2, sq((int)(q >> 16), sy)), sq((int)(q & 0xFFFFu), sx));
    }
    __device__ Best zinit(cell_t q) const { return {at(q, 0.0), 0u}; }
    __device__ void ztake(Best& b, cell_t q, val_t d2) const { b.v = fmin(b.v, at(q, d2)); }
};

// Where the z pass puts the squared distance of a query of class c, direction dir.
struct HistSink {
    unsigned* __restrict__ hist;
    int nbins;
    __device__ void put(int c, int, const UnitMetric::Best& b) const {
        if (b.v < nbins) atomicAdd(&hist[(long)c * nbins + b.v], 1u);
    }
};
// dist2[offs[c][dir] + slot], slot from the segment's counter; a slot at or past cap is dropped (the caller sees nq.sum() > cap)
struct ListSink {
    double* __restrict__ dist2;
    const long long* __restrict__ offs;
    unsigned long long* __restrict__ cursor;
    long long cap;
    __device__ void put(int c, int dir, const SpacedMetric::Best& b) const {
        const long long slot = offs[c * 2 + dir] + (long long)atomicAdd(&cursor[c * 2 + dir], 1ull);
        if (slot >= 0 && slot < cap) dist2[slot] = b.v;
    }
};

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
// SIDES: also sides[c][0] = |dP_c|, sides[c][1] = |dG_c| of the foreground classes, which counts[c][3] only has the sum of.
template <bool SIDES>
__global__ __launch_bounds__(256) void seg_border_count_kernel(const unsigned char* __restrict__ pred,
                                                               const unsigned char* __restrict__ label,
                                                               unsigned char* __restrict__ bmP, unsigned char* __restrict__ bmG,
                                                               unsigned long long* __restrict__ counts, int* __restrict__ box,
                                                               unsigned long long* __restrict__ sides, SegDims s, long N, int vec_ok) {
    __shared__ unsigned tally[(SM_MAX_CLS + 1) * 4];
    __shared__ unsigned stally[SIDES ? (SM_MAX_CLS + 1) * 2 : 1];
    __shared__ int lbox[(SM_MAX_CLS + 1) * 6];
    for (int i = threadIdx.x; i < s.ncls * 4; i += 256) tally[i] = 0u;
    if (SIDES)
        for (int i = threadIdx.x; i < s.ncls * 2; i += 256) stally[i] = 0u;
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
                        if (SIDES) atomicAdd(&stally[id * 2 + side], 1u);
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
    if (SIDES)
        for (int i = threadIdx.x; i < s.ncls * 2; i += 256)
            if (stally[i]) atomicAdd(&sides[i], (unsigned long long)stally[i]);
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
// with the metric's "no seed" cell (G1_NONE^2 / NO_SEED) instead of H-long walks.
template <class M>
__global__ __launch_bounds__(256) void seg_edt_y_kernel(const unsigned short* __restrict__ g1, typename M::cell_t* __restrict__ g2,
                                                        const unsigned long long* __restrict__ counts, const int* __restrict__ box,
                                                        SegDims s, long N, int c, int TX, M m) {
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
        for (int yy = yg; yy < hb; yy += G) g2[base + (long)yy * s.W] = M::no_seed();
        return;
    }
    for (int yy = yg; yy < hb; yy += G) {
        typename M::Best best = m.yinit(col[yy * TX + cx]);
        for (int d = 1;; ++d) {
            const typename M::val_t d2 = m.ystep(d);
            const bool lo = yy - d >= 0, hi = yy + d < hb;
            if (d2 >= best.v || !(lo || hi)) break;
            if (lo) m.ytake(best, col[(yy - d) * TX + cx], d, d2);
            if (hi) m.ytake(best, col[(yy + d) * TX + cx], d, d2);
        }
        g2[base + (long)yy * s.W] = m.ycell(best);
    }
}

// z pass, at the queries only: the other volume's border voxels of class c.  Walks the planes of the box outward from the
// query's own and stops as for y; the squared distance found goes to the sink: one more in the class's histogram row, or one
// more entry of the segment's list.
template <class M, class Sink>
__global__ __launch_bounds__(256) void seg_edt_z_kernel(const unsigned char* __restrict__ bmP, const unsigned char* __restrict__ bmG,
                                                        const typename M::cell_t* __restrict__ g2,
                                                        const unsigned long long* __restrict__ counts,
                                                        const int* __restrict__ box, SegDims s, long N, int c, M m, Sink sink) {
    SegBox b;
    if (!seg_class_box(counts, box, c, b)) return;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int z = blockIdx.z >> 1, dir = blockIdx.z & 1;
    if (z < b.z0 || z > b.z1 || y < b.y0 || y > b.y1 || x < b.x0 || x > b.x1) return;
    const long HW = (long)s.H * s.W, v = (long)z * HW + (long)y * s.W + x;
    if ((dir == 0 ? bmP : bmG)[v] != c) return;
    const typename M::cell_t* __restrict__ g = g2 + (long)dir * N + (long)y * s.W + x;
    typename M::Best best = m.zinit(g[(long)z * HW]);
    for (int d = 1;; ++d) {
        const typename M::val_t d2 = m.zstep(d);
        const bool lo = z - d >= b.z0, hi = z + d <= b.z1;
        if (d2 >= best.v || !(lo || hi)) break;
        if (lo) m.ztake(best, g[(long)(z - d) * HW], d2);
        if (hi) m.ztake(best, g[(long)(z + d) * HW], d2);
    }
    sink.put(c, dir, best);
}

// After the border pass: nq[c][dir] = |dP_c| (dir 0) / |dG_c| (dir 1) where class c > 0 has voxels on both sides, else 0 (the
// border pass left the raw tallies there); offs = exclusive prefix sum of nq in (class, dir) order; the segment counters to 0.
// One workgroup, a class per thread (ncls <= 255), a Hillis-Steele scan of the per-class totals in LDS.
__global__ __launch_bounds__(256) void seg_list_offsets_kernel(const unsigned long long* __restrict__ counts, long long* __restrict__ nq,
                                                               long long* __restrict__ offs, unsigned long long* __restrict__ cursor,
                                                               int ncls) {
    __shared__ long long scan[256];
    const int c = threadIdx.x;
    const bool both = c > 0 && c < ncls && counts[c * 4 + 0] != 0ull && counts[c * 4 + 1] != 0ull;
    const long long n0 = both ? nq[c * 2 + 0] : 0, n1 = both ? nq[c * 2 + 1] : 0;
    long long run = n0 + n1;
    scan[c] = run;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        const long long add = c >= o ? scan[c - o] : 0;
        __syncthreads();
        run += add;
        scan[c] = run;
        __syncthreads();
    }
    if (c < ncls) {
        const long long start = run - n0 - n1;
        nq[c * 2 + 0] = n0;
        nq[c * 2 + 1] = n1;
        offs[c * 2 + 0] = start;
        offs[c * 2 + 1] = start + n0;
        cursor[c * 2 + 0] = 0ull;
        cursor[c * 2 + 1] = 0ull;
    }
}

bool seg_dims_ok(int D, int H, int W) { return D >= 1 && H >= 1 && W >= 1 && D <= SM_MAX_DIM && H <= SM_MAX_DIM && W <= SM_MAX_DIM; }

size_t up16(size_t n) { return (n + 15) & ~(size_t)15; }

// the shape rules of both entry points; `what` names the caller in the message
bool seg_shape_ok(const char* what, int D, int H, int W, int ndim, int ncls) {
    if (!seg_dims_ok(D, H, W)) {
        cswin_set_error("%s: volume %dx%dx%d outside the supported 1..%d per dimension", what, D, H, W, SM_MAX_DIM);
        return false;
    }
    if (!(ndim == 3 || (ndim == 2 && D == 1))) {
        cswin_set_error("%s: ndim must be 3, or 2 with D == 1 (got ndim=%d, D=%d)", what, ndim, D);
        return false;
    }
    if (ncls < 2 || ncls > SM_MAX_CLS) {
        cswin_set_error("%s: ncls=%d outside 2..%d", what, ncls, SM_MAX_CLS);
        return false;
    }
    return true;
}

// One carving for both entry points: two border byte maps, g1 (uint16) and g2 (32-bit cells) for both directions of one class,
// the per-class boxes -- 14 B per voxel.  The list path appends its segment offsets and counters (16 B per class each).
struct SegWorkspace {
    unsigned char *bmP, *bmG;
    unsigned short* g1;
    void* g2;
    int* box;
    long long* offs;
    unsigned long long* cursor;
};
size_t seg_workspace_bytes(size_t N, int ncls) {
    return 2 * up16(N) + up16(2 * N * sizeof(unsigned short)) + up16(2 * N * sizeof(int)) + up16((size_t)ncls * 6 * sizeof(int));
}
size_t seg_list_bytes(int ncls) { return 2 * up16((size_t)ncls * 2 * sizeof(long long)); }
SegWorkspace seg_carve(void* workspace, size_t N, int ncls) {
    SegWorkspace w;
    w.bmP = (unsigned char*)workspace;
    w.bmG = w.bmP + up16(N);
    w.g1 = (unsigned short*)(w.bmG + up16(N));
    w.g2 = (char*)w.g1 + up16(2 * N * sizeof(unsigned short));
    w.box = (int*)((char*)w.g2 + up16(2 * N * sizeof(int)));
    w.offs = (long long*)((char*)w.box + up16((size_t)ncls * 6 * sizeof(int)));
    w.cursor = (unsigned long long*)((char*)w.offs + up16((size_t)ncls * 2 * sizeof(long long)));
    return w;
}

// box reset and the border pass; `sides` (SIDES only) is zeroed by the caller
template <bool SIDES>
int seg_border_pass(hipStream_t st, const unsigned char* pred, const unsigned char* label, const SegWorkspace& w, long long* counts,
                    long long* sides, const SegDims& s, long N) {
    hipLaunchKernelGGL(seg_box_init_kernel, dim3(cdiv(s.ncls * 6, 256)), dim3(256), 0, st, w.box, s.ncls);
    CSWIN_LAUNCH_CHECK();
    const int vec_ok = (uintptr_t)pred % 16 == 0 && (uintptr_t)label % 16 == 0;
    hipLaunchKernelGGL(seg_border_count_kernel<SIDES>, dim3((unsigned)((N + 256 * BC_VOX - 1) / (256 * BC_VOX))), dim3(256), 0, st, pred,
                       label, w.bmP, w.bmG, (unsigned long long*)counts, w.box, (unsigned long long*)sides, s, N, vec_ok);
    CSWIN_LAUNCH_CHECK();
    return CSWIN_OK;
}

// x, y and z pass of every foreground class under metric m, distances to `sink`
template <class M, class Sink>
int seg_class_passes(hipStream_t st, const SegWorkspace& w, const long long* counts, const SegDims& s, long N, M m, Sink sink) {
    typename M::cell_t* g2 = (typename M::cell_t*)w.g2;
    const int TX = s.H <= 512 ? 64 : (s.H <= 1024 ? 32 : 16);          // TX * H * 2 B of LDS <= 64 KiB
    const long rows = (long)s.D * s.H;
    for (int c = 1; c < s.ncls; ++c) {                                  // class 0 (background) is never measured
        hipLaunchKernelGGL(seg_edt_x_kernel, dim3((unsigned)((rows + 3) / 4), 2), dim3(256), 0, st, w.bmP, w.bmG, w.g1,
                           (const unsigned long long*)counts, w.box, s, N, c);
        hipLaunchKernelGGL(seg_edt_y_kernel<M>, dim3(cdiv(s.W, TX), s.D, 2), dim3(256), (size_t)TX * s.H * sizeof(unsigned short), st, w.g1,
                           g2, (const unsigned long long*)counts, w.box, s, N, c, TX, m);
        hipLaunchKernelGGL((seg_edt_z_kernel<M, Sink>), dim3(cdiv(s.W, 64), cdiv(s.H, 4), 2 * s.D), dim3(256), 0, st, w.bmP, w.bmG, g2,
                           (const unsigned long long*)counts, w.box, s, N, c, m, sink);
        CSWIN_LAUNCH_CHECK();
    }
    return CSWIN_OK;
}

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
    if (!seg_shape_ok("seg_metrics", D, H, W, ndim, ncls)) return 0;
    return seg_workspace_bytes((size_t)D * H * W, ncls);
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
    const SegWorkspace w = seg_carve(workspace, (size_t)N, ncls);

    if (hipMemsetAsync(counts, 0, (size_t)ncls * 4 * sizeof(long long), st) != hipSuccess ||
        hipMemsetAsync(hist, 0, (size_t)ncls * nbins * sizeof(unsigned), st) != hipSuccess) {
        cswin_set_error("seg_metrics: hipMemsetAsync failed");
        return CSWIN_ERR_HIP;
    }
    if (int rc = seg_border_pass<false>(st, pred, label, w, counts, nullptr, s, N)) return rc;
    return seg_class_passes(st, w, counts, s, N, UnitMetric{}, HistSink{hist, nbins});          // row 0 (background) stays zero
}

// cswin_seg_metrics_workspace plus the list path's segment offsets and counters
size_t cswin_surface_dist_workspace(int D, int H, int W, int ndim, int ncls) {
    if (!seg_shape_ok("surface_dist", D, H, W, ndim, ncls)) return 0;
    return seg_workspace_bytes((size_t)D * H * W, ncls) + seg_list_bytes(ncls);
}

int cswin_surface_dist(const unsigned char* pred, const unsigned char* label, long long* counts, long long* nq, double* dist2, long cap,
                       void* workspace, size_t ws_bytes, int D, int H, int W, int ndim, int ncls, double sz, double sy, double sx,
                       void* stream) {
    CSWIN_REQUIRE(pred && label && counts && nq && dist2, CSWIN_ERR_SHAPE, "surface_dist: null argument");
    CSWIN_REQUIRE(cap >= 0, CSWIN_ERR_SHAPE, "surface_dist: cap=%ld is negative", cap);
    if (ndim == 2) sz = 1.0;                                                          // a plane has no z step
    CSWIN_REQUIRE(std::isfinite(sz) && std::isfinite(sy) && std::isfinite(sx) && sz > 0 && sy > 0 && sx > 0, CSWIN_ERR_SHAPE,
                  "surface_dist: voxel spacing (%g, %g, %g) must be finite and positive", sz, sy, sx);
    const size_t need = cswin_surface_dist_workspace(D, H, W, ndim, ncls);          // sets the message for a bad shape
    if (need == 0) return CSWIN_ERR_SHAPE;
    CSWIN_REQUIRE(workspace && ws_bytes >= need, CSWIN_ERR_WORKSPACE, "surface_dist: workspace of %zu bytes, %zu needed", ws_bytes, need);
    CSWIN_REQUIRE((uintptr_t)workspace % 16 == 0, CSWIN_ERR_ALIGN, "surface_dist: workspace must be 16-B aligned");
    CSWIN_REQUIRE((uintptr_t)counts % 8 == 0 && (uintptr_t)nq % 8 == 0 && (uintptr_t)dist2 % 8 == 0, CSWIN_ERR_ALIGN,
                  "surface_dist: counts / nq / dist2 misaligned");
    hipStream_t st = (hipStream_t)stream;
    const long N = (long)D * H * W;
    const SegDims s = {D, H, W, ndim, ncls};
    const SegWorkspace w = seg_carve(workspace, (size_t)N, ncls);

    if (hipMemsetAsync(counts, 0, (size_t)ncls * 4 * sizeof(long long), st) != hipSuccess ||
        hipMemsetAsync(nq, 0, (size_t)ncls * 2 * sizeof(long long), st) != hipSuccess) {
        cswin_set_error("surface_dist: hipMemsetAsync failed");
        return CSWIN_ERR_HIP;
    }
    if (int rc = seg_border_pass<true>(st, pred, label, w, counts, nq, s, N)) return rc;
    hipLaunchKernelGGL(seg_list_offsets_kernel, dim3(1), dim3(256), 0, st, (const unsigned long long*)counts, nq, w.offs, w.cursor, ncls);
    CSWIN_LAUNCH_CHECK();
    return seg_class_passes(st, w, counts, s, N, SpacedMetric{sz, sy, sx}, ListSink{dist2, w.offs, w.cursor, (long long)cap});
}

}  // extern "C"
