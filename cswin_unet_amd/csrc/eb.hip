// The "eb-criterion" statistic of the surgical mode (universal_train.py:669-672) per parameter tensor on the flat gradient buffer:
//
//     grad_var = torch.var(g, dim=0, keepdim=True)          unbiased, along the FIRST dimension, one value per column
//     evidence = ((g * g) / (grad_var + 1e-8)).mean()
//
// where a "column" j is one index of the remaining dimensions flattened (inner = numel / shape[0] columns of d0 = shape[0] rows,
// row stride inner).  Per column the division is common to its rows, so evidence[t] = (sum_j Q_j / (var_j + 1e-8)) / numel with
// Q_j = sum_i g_ij^2.  Two launches, no host synchronisation, instead of five launches and one host read per tensor:
//
//   cswin_eb_tiles     partial[tile] = sum over the tile's columns of Q_j / (var_j + 1e-8f)
//   cswin_eb_finalize  evidence[t] = (tensor t's tile partials added in tile order) / numel[t]
//
// The reduction runs along dimension 0 of every tensor, so it cannot walk the 16384-element chunks of flat_chunks.h: it has a STATIC
// table of its own, built and uploaded once by optim.column_tiles, which is its only producer and checks every record (columns
// inside `inner`, ncols <= width, width a power of two <= 64).  One 256-thread workgroup per record; a record is all d0 rows of up
// to 64 neighbouring columns of one tensor.  Only elements of the tensor's slot are read, never a pad word.
//
// Thread map: lanes run along the contiguous column axis, c = tid % width, and the R = 256 / width row phases r = tid / width
// split dimension 0: thread (c, r) takes rows r, r + R, r + 2R, ... of column col0 + c, in row order.  With inner >= 64 the width is
// 64, a wave is one row phase and each of its loads is one 256-B segment of a row.  The host picks the width as the smallest power
// of two that holds the tile's columns: 1 for a bias (256 phases walk its one column), 16 for the nine taps of a depthwise kernel.
//
// Variance: the SHIFTED ONE-PASS form, the shift k_j = g_0j being the column's own first row, which every phase reads:
//     d = g_ij - k_j;   S1 = sum d;   S2 = sum d^2;   var_j = (S2 - S1 * S1 / d0) / (d0 - 1)
// Chosen over two passes because the three sums of a column stay plainly additive over its row phases (no (count, mean, M2)
// merging) and the buffer is read once; chosen over the naive sum g^2 - (sum g)^2 / d0 because that loses a column whose mean
// dwarfs its spread (a bias gradient near 1 with a spread of 1e-3 has no correct bit left in fp32).  With the shift taken from the
// column, d is of the size of the spread, S2 and S1^2 / d0 cancel only as far as k_j lies from the mean in units of the spread,
// and a column of equal values has d = 0 and var = 0 exactly.  tests/test_eb_host.eb_bound derives the error from this sequence.
// Rounding can leave var a hair below 0 where it is 0 up to rounding: such a var is set to 0 (a NaN is not: see below).
//
// Order of every sum (no float atomic; two runs give the same bits): a thread's rows in row order, d^2 and g^2 entering by fmaf;
// a column's R phase partials through LDS in phase order; the tile's column terms by the xor butterfly of wave 0 (lanes past ncols
// add 0); a tensor's tiles in tile order.
//
// d0 == 1: S1 = S2 = 0 and var = 0 / 0 = NaN, as torch.var gives; the NaN is stored as it comes, neither trapped nor replaced.
#include "flat_chunks.h"

namespace {

// one workgroup's work: rows 0 .. d0 - 1 of columns col0 .. col0 + ncols - 1 of the tensor at element offset off
struct EbTile { long long off; int d0, inner, col0, ncols, tensor, width; };
static_assert(sizeof(EbTile) == 32, "the tile record is 32 bytes");

constexpr int EB_BATCH = 8;      // independent row loads a thread keeps in flight

struct EbSums { float s1, s2, q; };
__device__ __forceinline__ void eb_row(EbSums& a, float x, float k) {
    const float d = x - k;
    a.s1 += d;
    a.s2 = fmaf(d, d, a.s2);
    a.q = fmaf(x, x, a.q);
}

__global__ __launch_bounds__(256) void eb_tiles_kernel(const float* __restrict__ g, const EbTile* __restrict__ tiles, float* __restrict__ partial) {
    __shared__ float red[3][256];
    const EbTile t = tiles[blockIdx.x];
    const int c = threadIdx.x & (t.width - 1), r = threadIdx.x / t.width, R = 256 / t.width;
    EbSums a = {0.f, 0.f, 0.f};
    if (c < t.ncols) {
        const float* col = g + t.off + t.col0 + c;
        const long stride = t.inner, step = (long)R * t.inner;
        const float k = col[0];
        const float* p = col + r * stride;
        int i = r;
        for (; i + (EB_BATCH - 1) * R < t.d0; i += EB_BATCH * R, p += EB_BATCH * step) {
            float x[EB_BATCH];
#pragma unroll
            for (int e = 0; e < EB_BATCH; ++e) x[e] = p[e * step];
#pragma unroll
            for (int e = 0; e < EB_BATCH; ++e) eb_row(a, x[e], k);
        }
        for (; i < t.d0; i += R, p += step) eb_row(a, *p, k);
    }
    red[0][threadIdx.x] = a.s1;
    red[1][threadIdx.x] = a.s2;
    red[2][threadIdx.x] = a.q;
    __syncthreads();
    if (threadIdx.x >= 64) return;                           // wave 0 goes on: lane c < width owns column col0 + c
    float term = 0.f;
    if ((int)threadIdx.x < t.ncols) {
        float s1 = 0.f, s2 = 0.f, q = 0.f;
        for (int ph = 0; ph < R; ++ph) {
            s1 += red[0][ph * t.width + threadIdx.x];
            s2 += red[1][ph * t.width + threadIdx.x];
            q += red[2][ph * t.width + threadIdx.x];
        }
        float var = (s2 - s1 * s1 / (float)t.d0) / (float)(t.d0 - 1);
        var = var < 0.f ? 0.f : var;                         // keeps the NaN of d0 == 1
        term = q / (var + 1e-8f);
    }
    term = wave_sum(term);
    if (threadIdx.x == 0) partial[blockIdx.x] = term;
}

// one workgroup, thread k owns tensors k, k + 256, ...
__global__ __launch_bounds__(256) void eb_finalize_kernel(const float* __restrict__ partial, const int* __restrict__ first_tile,
                                                           const int* __restrict__ numel, int ntensors, float* __restrict__ evidence) {
    for (int t = threadIdx.x; t < ntensors; t += 256) {
        float s = 0.f;
        const int e1 = first_tile[t + 1];
        for (int e = first_tile[t]; e < e1; ++e) s += partial[e];
        evidence[t] = s / (float)numel[t];
    }
}

}  // namespace

extern "C" {

int cswin_eb_tiles(const float* g, const void* tiles, int ntiles, float* partial, void* stream) {
    CSWIN_REQUIRE(g && tiles && partial && ntiles > 0, CSWIN_ERR_SHAPE, "eb_tiles: bad arguments");
    if (int e = flat_align_check("eb_tiles", (uintptr_t)g, tiles, nullptr)) return e;
    hipLaunchKernelGGL(eb_tiles_kernel, dim3(ntiles), dim3(256), 0, (hipStream_t)stream, g, (const EbTile*)tiles, partial);
    CSWIN_LAUNCH_CHECK();
    return CSWIN_OK;
}

int cswin_eb_finalize(const float* partial, const int* first_tile, const int* numel, int ntensors, float* evidence, void* stream) {
    CSWIN_REQUIRE(partial && first_tile && numel && evidence && ntensors > 0, CSWIN_ERR_SHAPE, "eb_finalize: bad arguments");
    hipLaunchKernelGGL(eb_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partial, first_tile, numel, ntensors, evidence);
    CSWIN_LAUNCH_CHECK();
    return CSWIN_OK;
}

}  // extern "C"
