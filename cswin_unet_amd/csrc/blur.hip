// scipy.ndimage.gaussian_filter(x[d], sigma) of every float32 slice of a batch: the domain shift of the fine-tuning experiments
// (apply_blur_train.py:147-150, apply_blur_test.py:79-81), applied to slices that are resident on the device.
//
// The kernel does not restate scipy's rules beyond its arithmetic.  The 2r + 1 symmetric float64 taps come from scipy itself
// (utils.gaussian_taps: the response of gaussian_filter1d to a unit impulse).  The device repeats correlate1d's sums:
//   axis 0 first, its result ROUNDED TO float32 (scipy stores a pass in the input's dtype), then axis 1, rounded again;
//   every product and sum in float64, in the folded order of a symmetric kernel,
//       acc = x[i] w[0];  for k = r .. 1:  acc += (x[i - k] + x[i + k]) w[-k]
//   a separate multiply and add (this file is compiled with -ffp-contract=off: an FMA skips the product's rounding and differs
//   from scipy in the last bit of a fraction of the elements);
//   mode "reflect", d c b a | a b c d | d c b a: index i -> m = i mod 2n, m < n ? m : 2n - 1 - m, computed here from n alone, so
//   a radius larger than the axis reflects as often as it has to and no index can leave the slice.
#include "common.h"
#include "blur_plan.h"

#pragma clang fp contract(off)

namespace {

struct BlurArgs {
    const float* x;
    float* y;
    const double* taps;                    // taps[0 .. r] = w[-r] .. w[0]
    int radius, H, W, TR, cw_log2;
    unsigned w_magic;                      // fdiv_magic(W)
    const int* each;                       // EACH only: (taps offset, radius) of every slice; radius is then the largest
    int ntaps;                             // EACH only: doubles behind taps
};

__device__ __forceinline__ int bl_reflect(int i, int n) {
    if ((unsigned)i < (unsigned)n) return i;
    const int p = 2 * n;
    int m = i % p;
    if (m < 0) m += p;
    return m < n ? m : p - 1 - m;
}

// One workgroup = one slice x TR consecutive output rows at full width.  LDS: mid [TR][W], the column pass's float32 result, and
// stage [TR + 2r][CW], the input rows of the tile for one chunk of CW columns (CW a power of two; the host sizes TR and CW so
// that both fit, bl_plan).
// Column pass, per chunk: the TR + 2r input rows (reflected row index) are read from global memory ONCE into the stage, VEC
//   adjacent columns per load; then a thread forms the outputs of BL_RB consecutive rows of one column from the stage values
//   above and below, lanes along the columns (conflict-free LDS reads): a tap is fetched once for BL_RB independent sums.
// Row pass: a thread owns column j of BL_RB consecutive rows and reads mid[i][reflect(j -+ k)], one reflected index per tap and
//   side for all of them; away from the two edges that is j -+ k itself, so the lanes of a wave read consecutive words, and the
//   stores are contiguous across lanes.
// Rows of a group beyond the tile's last (a tile remainder) are computed on whatever the LDS holds and not stored.
// R: the radius at compile time (the tap loops unroll, the taps stay in registers and the stage values of neighbouring taps and
//   rows are read once), or -1 for any radius.
// EACH (R == -1 only): slice d has its own radius each[2d + 1] <= a.radius and its own taps at a.taps + each[2d]
//   (cswin_gaussian_blur_each).  The tile was planned for a.radius, so a smaller halo fits its stage; radius and offset are
//   clamped here to what the plan and the taps buffer hold, so a bad table cannot send an index out of either.
template <int VEC, int R, bool EACH = false>
__global__ __launch_bounds__(256) void gaussian_blur_kernel(BlurArgs a) {
    extern __shared__ __attribute__((aligned(16))) float bl_lds[];
    const int d = blockIdx.y, r0 = blockIdx.x * a.TR;
    const int r = R >= 0 ? R : EACH ? min(max(a.each[2 * d + 1], 0), min(a.radius, a.ntaps - 1)) : a.radius;
    const int H = a.H, W = a.W, TR = a.TR, cwl = a.cw_log2, CW = 1 << cwl;
    const int nrow = min(TR, H - r0), nstage = nrow + 2 * r, ngrp = (nrow + BL_RB - 1) / BL_RB;
    float* __restrict__ mid = bl_lds;
    float* __restrict__ stage = bl_lds + TR * W;          // W is even where VEC == 2: 8-B aligned
    const float* __restrict__ xs = a.x + (long)d * H * W;
    const double* __restrict__ taps = EACH ? a.taps + min(max(a.each[2 * d], 0), a.ntaps - 1 - r) : a.taps;
    const double w0 = taps[r];

    constexpr int VL = VEC == 2 ? 1 : 0;
    for (int cb = 0; cb < W; cb += CW) {
        for (int idx = threadIdx.x; idx < nstage << (cwl - VL); idx += 256) {
            const int row = idx >> (cwl - VL), cl = (idx & ((CW >> VL) - 1)) << VL, c = cb + cl;
            if (c < W) {                                   // VEC == 2: c and W are even, so c + 1 < W as well
                const float* src = xs + (long)bl_reflect(r0 - r + row, H) * W + c;
                if constexpr (VEC == 2) *reinterpret_cast<u32x2*>(stage + row * CW + cl) = *reinterpret_cast<const u32x2*>(src);
                else stage[row * CW + cl] = *src;
            }
        }
        __syncthreads();
        for (int idx = threadIdx.x; idx < ngrp << cwl; idx += 256) {
            const int i0 = (idx >> cwl) * BL_RB, cl = idx & (CW - 1), c = cb + cl;
            if (c < W) {
                const float* s = stage + (i0 + r) * CW + cl;
                double acc[BL_RB];
#pragma unroll
                for (int q = 0; q < BL_RB; ++q) acc[q] = (double)s[q * CW] * w0;
#pragma unroll R >= 0 ? R : 1
                for (int t = 0; t < r; ++t) {
                    const int k = r - t;
                    const double w = taps[t];
#pragma unroll
                    for (int q = 0; q < BL_RB; ++q) acc[q] = acc[q] + ((double)s[(q - k) * CW] + (double)s[(q + k) * CW]) * w;
                }
#pragma unroll
                for (int q = 0; q < BL_RB; ++q)
                    if (i0 + q < nrow) mid[(i0 + q) * W + c] = (float)acc[q];
            }
        }
        __syncthreads();                                   // the stage is free for the next chunk; after the last one mid is whole
    }

    float* __restrict__ out = a.y + ((long)d * H + r0) * W;
    for (int idx = threadIdx.x; idx < ngrp * W; idx += 256) {
        const int ig = fdiv1(idx, a.w_magic), j = idx - ig * W, i0 = ig * BL_RB;
        const float* m = mid + i0 * W;
        double acc[BL_RB];
#pragma unroll
        for (int q = 0; q < BL_RB; ++q) acc[q] = (double)m[q * W + j] * w0;
#pragma unroll R >= 0 ? R : 1
        for (int t = 0; t < r; ++t) {
            const int k = r - t, jl = bl_reflect(j - k, W), jr = bl_reflect(j + k, W);
            const double w = taps[t];
#pragma unroll
            for (int q = 0; q < BL_RB; ++q) acc[q] = acc[q] + ((double)m[q * W + jl] + (double)m[q * W + jr]) * w;
        }
#pragma unroll
        for (int q = 0; q < BL_RB; ++q)
            if (i0 + q < nrow) out[(i0 + q) * W + j] = (float)acc[q];
    }
}

}  // namespace

extern "C" {

int cswin_gaussian_blur(const float* x, float* y, const double* taps, int radius, int D, int H, int W, void* stream) {
    CSWIN_REQUIRE(x && y && taps, CSWIN_ERR_SHAPE, "gaussian_blur: null argument");
    CSWIN_REQUIRE(x != y, CSWIN_ERR_UNSUPPORTED, "gaussian_blur: x == y (the filter does not work in place)");
    CSWIN_REQUIRE(bl_dim_ok(D) && bl_dim_ok(H) && bl_dim_ok(W), CSWIN_ERR_SHAPE,
                  "gaussian_blur: (D, H, W) = (%d, %d, %d) outside the supported 1..%d per dimension", D, H, W, BL_MAX_DIM);
    CSWIN_REQUIRE(radius >= 0 && radius <= BL_MAX_RADIUS, CSWIN_ERR_UNSUPPORTED, "gaussian_blur: radius=%d outside 0..%d", radius,
                  BL_MAX_RADIUS);
    CSWIN_REQUIRE((uintptr_t)x % 4 == 0 && (uintptr_t)y % 4 == 0 && (uintptr_t)taps % 8 == 0, CSWIN_ERR_ALIGN,
                  "gaussian_blur: a pointer is not aligned to its element size");
    const int vec = (W % 2 == 0 && (uintptr_t)x % 8 == 0) ? 2 : 1;     // two columns per load: even rows stay aligned
    const BlurPlan p = bl_plan(H, W, radius, vec);
    CSWIN_REQUIRE(p.TR >= 1, CSWIN_ERR_UNSUPPORTED, "gaussian_blur: no tile of W=%d, radius=%d fits the LDS", W, radius);
    const BlurArgs a = {x, y, taps, radius, H, W, p.TR, p.cw_log2, fdiv_magic(W)};
    const dim3 grid(cdiv(H, p.TR), D), block(256);
    const size_t lds = (size_t)bl_lds_bytes(p, W, radius);
    hipStream_t st = (hipStream_t)stream;
    if (radius == 4) {                 // sigma = 1 at truncate = 4, the reference's shift
        if (vec == 2) hipLaunchKernelGGL((gaussian_blur_kernel<2, 4>), grid, block, lds, st, a);
        else hipLaunchKernelGGL((gaussian_blur_kernel<1, 4>), grid, block, lds, st, a);
    } else {
        if (vec == 2) hipLaunchKernelGGL((gaussian_blur_kernel<2, -1>), grid, block, lds, st, a);
        else hipLaunchKernelGGL((gaussian_blur_kernel<1, -1>), grid, block, lds, st, a);
    }
    CSWIN_LAUNCH_CHECK();
    return CSWIN_OK;
}

int cswin_gaussian_blur_each(const float* x, float* y, const double* taps, int ntaps, const int* table, int max_radius, int D, int H,
                             int W, void* stream) {
    CSWIN_REQUIRE(x && y && taps && table, CSWIN_ERR_SHAPE, "gaussian_blur_each: null argument");
    CSWIN_REQUIRE(x != y, CSWIN_ERR_UNSUPPORTED, "gaussian_blur_each: x == y (the filter does not work in place)");
    CSWIN_REQUIRE(bl_dim_ok(D) && bl_dim_ok(H) && bl_dim_ok(W), CSWIN_ERR_SHAPE,
                  "gaussian_blur_each: (D, H, W) = (%d, %d, %d) outside the supported 1..%d per dimension", D, H, W, BL_MAX_DIM);
    CSWIN_REQUIRE(max_radius >= 0 && max_radius <= BL_MAX_RADIUS, CSWIN_ERR_UNSUPPORTED, "gaussian_blur_each: max_radius=%d outside 0..%d",
                  max_radius, BL_MAX_RADIUS);
    CSWIN_REQUIRE(ntaps > max_radius && ntaps <= BL_MAX_DIM * (BL_MAX_RADIUS + 1), CSWIN_ERR_SHAPE,
                  "gaussian_blur_each: ntaps=%d does not hold the %d taps of the largest radius (or exceeds %d)", ntaps, max_radius + 1,
                  BL_MAX_DIM * (BL_MAX_RADIUS + 1));
    CSWIN_REQUIRE((uintptr_t)x % 4 == 0 && (uintptr_t)y % 4 == 0 && (uintptr_t)taps % 8 == 0 && (uintptr_t)table % 4 == 0, CSWIN_ERR_ALIGN,
                  "gaussian_blur_each: a pointer is not aligned to its element size");
    const int vec = (W % 2 == 0 && (uintptr_t)x % 8 == 0) ? 2 : 1;
    const BlurPlan p = bl_plan(H, W, max_radius, vec);
    CSWIN_REQUIRE(p.TR >= 1, CSWIN_ERR_UNSUPPORTED, "gaussian_blur_each: no tile of W=%d, radius=%d fits the LDS", W, max_radius);
    const BlurArgs a = {x, y, taps, max_radius, H, W, p.TR, p.cw_log2, fdiv_magic(W), table, ntaps};
    const dim3 grid(cdiv(H, p.TR), D), block(256);
    const size_t lds = (size_t)bl_lds_bytes(p, W, max_radius);
    hipStream_t st = (hipStream_t)stream;
    if (vec == 2) hipLaunchKernelGGL((gaussian_blur_kernel<2, -1, true>), grid, block, lds, st, a);
    else hipLaunchKernelGGL((gaussian_blur_kernel<1, -1, true>), grid, block, lds, st, a);
    CSWIN_LAUNCH_CHECK();
    return CSWIN_OK;
}

}  // extern "C"
