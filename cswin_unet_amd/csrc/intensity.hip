// Intensity augmentation of a batch of float32 images, stages 2-5 of utils.intensity_host (the blur, stage 1, is blur.hip's):
//   noise       z[i] += noise_std n(seed, i),  n = sqrt(-2 ln u1) cos(2 pi u2) from r = mix64(mix64(seed) ^ i) (layout.hip's mix64),
//               u1 = ((r >> 40) + 1) / 2^24 in (0, 1],  u2 = ((r >> 16) & 0xFFFFFF) / 2^24 in [0, 1)
//   brightness  z *= brightness
//   contrast    m, lo, hi = mean, min, max of z;  z = clip((z - m) contrast + m, lo, hi)
//   gamma       (z = -z if inverted)  m0, s0 = mean, population std;  lo = min, rng = max - lo;
//               z = ((z - lo) / (rng + 1e-7)) ** gamma rng + lo;  z = (z - mean(z)) / (std(z) + 1e-8) s0 + m0  (z = -z again)
// every value a float64 from the float32 input on, rounded to float32 once at the end; multiply and add rounded separately, as
// numpy does (contraction is off in this file).  The definition differs from this file only in the ORDER of its sums (numpy adds
// pairwise) and in the last bit of libm's log, cos and pow; neither survives the final rounding but for an element in some 10^8.
//
// Shape: one launch per PASS over a grid of (chunks of 2048 pixels, samples), not one workgroup per sample.  The chain between two
// sets of whole-image statistics is evaluated once and kept as float64 in the workspace: the transcendental functions of the noise
// and the power cost hundreds of float64 instructions per pixel, which a per-sample workgroup would repeat in every pass and on 24
// of 256 CUs.  A pass leaves per-chunk partial statistics; the next pass's workgroups each merge their sample's partials, chunk c
// in thread c mod 256 in rising order and then the fixed tree of block_sum, so no sum depends on timing, on the batch or on the
// grid, and there is no atomic.  The passes:
//   1 head      noise, brightness;  -> y for a sample without contrast and gamma, else -> z and (sum, min, max) of z
//   2 contrast  (samples with contrast)  -> y without gamma, else -> z and (sum, min, max)
//   3 power     (samples with gamma)  sum (z - m0)^2 of the old z;  the power -> z and its sum
//   4 spread    (gamma)  sum (z - m1)^2
//   5 tail      (gamma)  the renormalisation -> y
// std is numpy's: the mean first, then the mean of the squared deviations.  A workgroup of a sample that a pass does not concern
// returns at once, and the host leaves out a pass that concerns no sample of the batch (`stages`).
#include "common.h"

#pragma clang fp contract(off)

extern "C" {
typedef struct cswin_intensity_desc {
    long long flags;                 // IN_* below
    unsigned long long seed;
    double noise_std, brightness, contrast, gamma;
} cswin_intensity_desc;
}

namespace {

constexpr int IN_NOISE = 1, IN_BRIGHTNESS = 2, IN_CONTRAST = 4, IN_GAMMA = 8, IN_INVERT = 16;
constexpr int IN_THREADS = 256, IN_PER = 8, IN_CHUNK = IN_THREADS * IN_PER;
constexpr int IN_MAX_BATCH = 2048;
constexpr long IN_MAX_ELEMS = 2048L * 2048L;
// doubles of partial statistics per (sample, chunk): (sum, min, max) after the head, the same after the contrast, then the three
// single sums of passes 3 and 4
constexpr int IN_PA = 0, IN_PB = 3, IN_PC = 6, IN_PD = 7, IN_PE = 8, IN_PART = 9;

struct IntensityArgs {
    const float* x;
    float* y;
    const cswin_intensity_desc* table;
    double* z;                       // [B][n]
    double* part;                    // [B][nchunks][IN_PART]
    int n, nchunks, stages;
};

__device__ __forceinline__ unsigned long long in_mix64(unsigned long long z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__device__ __forceinline__ double in_normal(unsigned long long seed_mixed, unsigned long long i) {
    const unsigned long long r = in_mix64(seed_mixed ^ i);
    const double u1 = (double)((r >> 40) + 1) * 0x1p-24, u2 = (double)((r >> 16) & 0xFFFFFFull) * 0x1p-24;
    return sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
}

// the three reductions of a workgroup in one fixed tree; every thread gets the results
__device__ __forceinline__ void block_stats(double& s, double& lo, double& hi, double (*red)[IN_THREADS]) {
    const int t = threadIdx.x;
    __syncthreads();                                       // the previous use of red is over
    red[0][t] = s, red[1][t] = lo, red[2][t] = hi;
    __syncthreads();
    for (int h = IN_THREADS / 2; h > 0; h >>= 1) {
        if (t < h) {
            red[0][t] = red[0][t] + red[0][t + h];
            red[1][t] = fmin(red[1][t], red[1][t + h]);
            red[2][t] = fmax(red[2][t], red[2][t + h]);
        }
        __syncthreads();
    }
    s = red[0][0], lo = red[1][0], hi = red[2][0];
}
__device__ __forceinline__ double block_sum(double s, double (*red)[IN_THREADS]) {
    const int t = threadIdx.x;
    __syncthreads();
    red[0][t] = s;
    __syncthreads();
    for (int h = IN_THREADS / 2; h > 0; h >>= 1) {
        if (t < h) red[0][t] = red[0][t] + red[0][t + h];
        __syncthreads();
    }
    return red[0][0];
}

// a sample's (sum, min, max) / single sum over its chunks' partials at doubles [off ..] of each record
__device__ __forceinline__ void merge_stats(const double* part, int nchunks, int off, double& s, double& lo, double& hi,
                                            double (*red)[IN_THREADS]) {
    s = 0.0, lo = INFINITY, hi = -INFINITY;
    for (int c = threadIdx.x; c < nchunks; c += IN_THREADS) {
        const double* p = part + (long)c * IN_PART + off;
        s = s + p[0], lo = fmin(lo, p[1]), hi = fmax(hi, p[2]);
    }
    block_stats(s, lo, hi, red);
}
__device__ __forceinline__ double merge_sum(const double* part, int nchunks, int off, double (*red)[IN_THREADS]) {
    double s = 0.0;
    for (int c = threadIdx.x; c < nchunks; c += IN_THREADS) s = s + part[(long)c * IN_PART + off];
    return block_sum(s, red);
}

template <int PASS>
__global__ __launch_bounds__(IN_THREADS) void intensity_pass_kernel(IntensityArgs a) {
    __shared__ double red[3][IN_THREADS];
    const int b = blockIdx.y, c = blockIdx.x, n = a.n, nchunks = a.nchunks;
    const cswin_intensity_desc d = a.table[b];
    // the launches follow `stages`, so a sample's flags are read through it: what the host did not plan for is off
    const int f = (int)d.flags & (a.stages | ~(IN_CONTRAST | IN_GAMMA)) & ((a.stages & IN_GAMMA) ? ~0 : ~IN_INVERT);
    const bool C = f & IN_CONTRAST, G = f & IN_GAMMA, inv = G && (f & IN_INVERT);
    if ((PASS == 2 && !C) || (PASS >= 3 && !G)) return;
    const long base = (long)b * n;
    const int i0 = c * IN_CHUNK + threadIdx.x;
    double* __restrict__ z = a.z + base;
    double* part = a.part + (long)b * nchunks * IN_PART;     // this sample's records
    double* mine = part + (long)c * IN_PART;
    const int after = C ? IN_PB : IN_PA;                     // the statistics the gamma stage starts from
    const double dn = (double)n;

    if constexpr (PASS == 1) {
        const unsigned long long sm = in_mix64(d.seed);
        double s = 0.0, lo = INFINITY, hi = -INFINITY;
#pragma unroll
        for (int k = 0; k < IN_PER; ++k) {
            const int i = i0 + k * IN_THREADS;
            if (i < n) {
                double v = (double)a.x[base + i];
                if (f & IN_NOISE) v = v + d.noise_std * in_normal(sm, (unsigned long long)i);
                if (f & IN_BRIGHTNESS) v = v * d.brightness;
                if (!(C || G)) a.y[base + i] = (float)v;
                else {
                    if (!C && inv) v = -v;
                    z[i] = v;
                    s = s + v, lo = fmin(lo, v), hi = fmax(hi, v);
                }
            }
        }
        if (C || G) {
            block_stats(s, lo, hi, red);
            if (threadIdx.x == 0) mine[IN_PA] = s, mine[IN_PA + 1] = lo, mine[IN_PA + 2] = hi;
        }
    } else if constexpr (PASS == 2) {
        double ms, mlo, mhi;
        merge_stats(part, nchunks, IN_PA, ms, mlo, mhi, red);
        const double m = ms / dn;
        double s = 0.0, lo = INFINITY, hi = -INFINITY;
#pragma unroll
        for (int k = 0; k < IN_PER; ++k) {
            const int i = i0 + k * IN_THREADS;
            if (i < n) {
                double v = (z[i] - m) * d.contrast + m;
                v = fmin(fmax(v, mlo), mhi);
                if (!G) a.y[base + i] = (float)v;
                else {
                    if (inv) v = -v;
                    z[i] = v;
                    s = s + v, lo = fmin(lo, v), hi = fmax(hi, v);
                }
            }
        }
        if (G) {
            block_stats(s, lo, hi, red);
            if (threadIdx.x == 0) mine[IN_PB] = s, mine[IN_PB + 1] = lo, mine[IN_PB + 2] = hi;
        }
    } else if constexpr (PASS == 3) {
        double ms, lo, hi;
        merge_stats(part, nchunks, after, ms, lo, hi, red);
        const double m0 = ms / dn, rng = hi - lo, den = rng + 1e-7;
        double dev = 0.0, s = 0.0;
#pragma unroll
        for (int k = 0; k < IN_PER; ++k) {
            const int i = i0 + k * IN_THREADS;
            if (i < n) {
                const double v = z[i], e = v - m0;
                dev = dev + e * e;
                const double w = pow((v - lo) / den, d.gamma) * rng + lo;
                z[i] = w;
                s = s + w;
            }
        }
        dev = block_sum(dev, red);
        s = block_sum(s, red);
        if (threadIdx.x == 0) mine[IN_PC] = dev, mine[IN_PD] = s;
    } else if constexpr (PASS == 4) {
        const double m1 = merge_sum(part, nchunks, IN_PD, red) / dn;
        double dev = 0.0;
#pragma unroll
        for (int k = 0; k < IN_PER; ++k) {
            const int i = i0 + k * IN_THREADS;
            if (i < n) {
                const double e = z[i] - m1;
                dev = dev + e * e;
            }
        }
        dev = block_sum(dev, red);
        if (threadIdx.x == 0) mine[IN_PE] = dev;
    } else {
        double ms, lo, hi;
        merge_stats(part, nchunks, after, ms, lo, hi, red);
        const double m0 = ms / dn, s0 = sqrt(merge_sum(part, nchunks, IN_PC, red) / dn);
        const double m1 = merge_sum(part, nchunks, IN_PD, red) / dn, s1 = sqrt(merge_sum(part, nchunks, IN_PE, red) / dn);
        const double den = s1 + 1e-8;
#pragma unroll
        for (int k = 0; k < IN_PER; ++k) {
            const int i = i0 + k * IN_THREADS;
            if (i < n) {
                double v = (z[i] - m1) / den * s0 + m0;
                if (inv) v = -v;
                a.y[base + i] = (float)v;
            }
        }
    }
}

inline int in_chunks(long n) { return (int)((n + IN_CHUNK - 1) / IN_CHUNK); }
inline bool in_shape_ok(int B, long n) { return B >= 1 && B <= IN_MAX_BATCH && n >= 1 && n <= IN_MAX_ELEMS; }

}  // namespace

extern "C" {

size_t cswin_intensity_workspace(int B, long slice_elems) {
    if (!in_shape_ok(B, slice_elems)) {
        cswin_set_error("intensity_workspace: B=%d, slice_elems=%ld outside 1..%d, 1..%ld", B, slice_elems, IN_MAX_BATCH, IN_MAX_ELEMS);
        return 0;
    }
    return ((size_t)B * (size_t)slice_elems + (size_t)B * in_chunks(slice_elems) * IN_PART) * sizeof(double);
}

int cswin_intensity_batch(const float* x, float* y, const void* table, void* workspace, size_t ws_bytes, int B, long slice_elems,
                          int stages, void* stream) {
    CSWIN_REQUIRE(x && y && table, CSWIN_ERR_SHAPE, "intensity_batch: null argument");
    CSWIN_REQUIRE(in_shape_ok(B, slice_elems), CSWIN_ERR_SHAPE, "intensity_batch: B=%d, slice_elems=%ld outside 1..%d, 1..%ld", B,
                  slice_elems, IN_MAX_BATCH, IN_MAX_ELEMS);
    CSWIN_REQUIRE((uintptr_t)x % 4 == 0 && (uintptr_t)y % 4 == 0 && (uintptr_t)table % 8 == 0 && (uintptr_t)workspace % 8 == 0,
                  CSWIN_ERR_ALIGN, "intensity_batch: a pointer is not aligned to its element size");
    CSWIN_REQUIRE((stages & ~(IN_CONTRAST | IN_GAMMA)) == 0, CSWIN_ERR_SHAPE, "intensity_batch: stages=%d has bits beyond contrast (%d) and gamma (%d)",
                  stages, IN_CONTRAST, IN_GAMMA);
    const bool stats = stages != 0;
    CSWIN_REQUIRE(!stats || (workspace && ws_bytes >= cswin_intensity_workspace(B, slice_elems)), CSWIN_ERR_WORKSPACE,
                  "intensity_batch: workspace of %zu bytes, %zu needed", ws_bytes, cswin_intensity_workspace(B, slice_elems));
    const int n = (int)slice_elems, nchunks = in_chunks(slice_elems);
    double* z = (double*)workspace;
    const IntensityArgs a = {x, y, (const cswin_intensity_desc*)table, z, stats ? z + (size_t)B * n : nullptr, n, nchunks, stages};
    const dim3 grid(nchunks, B), block(IN_THREADS);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(intensity_pass_kernel<1>, grid, block, 0, st, a);
    if (stages & IN_CONTRAST) hipLaunchKernelGGL(intensity_pass_kernel<2>, grid, block, 0, st, a);
    if (stages & IN_GAMMA) {
        hipLaunchKernelGGL(intensity_pass_kernel<3>, grid, block, 0, st, a);
        hipLaunchKernelGGL(intensity_pass_kernel<4>, grid, block, 0, st, a);
        hipLaunchKernelGGL(intensity_pass_kernel<5>, grid, block, 0, st, a);
    }
    CSWIN_LAUNCH_CHECK();
    return CSWIN_OK;
}

}  // extern "C"
