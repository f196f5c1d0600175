// Signed distance maps of a batch of label slices, for the boundary loss (Kervadec et al., MIDL 2019: one_hot2dist): for every
// sample b and class c, with M = (labels[b] == c),
//   phi[b][c] = +d(p, M) outside M,  -(d(p, ~M) - 1) inside M,  0 everywhere when M is empty or the whole slice,
// d the Euclidean distance in pixels to the nearest pixel of the set: scipy's edt(~M) * ~M - (edt(M) - 1) * M, bit for bit.
// Exact and separable like the transform of metrics.hip, but dense, 2-D and signed: a row pass leaves, per pixel and class, the
// distance along the row to the nearest pixel of the OTHER membership (g1, uint16, bit 15 = the pixel's own membership), and a
// column pass takes min_y' f(y')^2 + (y - y')^2 with f = 0 where (y', x) has the other membership and g1 otherwise.  Integers
// up to the final square root, integer atomics only: two runs give the same bits.  The launch policy is sdm_plan.h's.
#include "common.h"
#include "sdm_plan.h"

namespace {

// Row pass: one wave per row (b, y).  The label row is read once and kept as class bytes in LDS (255: no class); then, per
// class, two sweeps over the row in 64-pixel chunks with the membership flags of a chunk as one ballot (seg_edt_x_kernel's
// scheme, for both memberships at once): left to right for the nearest pixel of the other membership at or before x, right to
// left for the nearest after it.  A lane meets the same x in every sweep, so the wave's LDS rows need no barrier.
__global__ __launch_bounds__(256) void sdm_row_kernel(const long long* __restrict__ labels, unsigned short* __restrict__ g1,
                                                      unsigned* __restrict__ counts, long rows, int ncls, int H, int W) {
    __shared__ unsigned char cls[SDM_ROW_WAVES][SDM_MAX_DIM + 1];
    __shared__ unsigned short left[SDM_ROW_WAVES][SDM_MAX_DIM + 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long row = (long)blockIdx.x * SDM_ROW_WAVES + wave;
    if (row >= rows) return;
    const long b = row / H;
    const int y = (int)(row - b * H);
    const long long* __restrict__ lab = labels + row * W;
    for (int x = lane; x < W; x += 64) {
        const long long l = lab[x];
        cls[wave][x] = (unsigned long long)l < (unsigned long long)ncls ? (unsigned char)l : (unsigned char)255;
    }
    const int nchunk = (W + 63) >> 6;
    for (int c = 0; c < ncls; ++c) {
        unsigned short* __restrict__ out = g1 + (((long)b * ncls + c) * H + y) * W;
        int lastM = -1, lastN = -1;                                     // the last member / non-member before this chunk
        unsigned members = 0;
        for (int k = 0; k < nchunk; ++k) {
            const int xb = k << 6, x = xb + lane;
            const bool valid = x < W, mem = valid && cls[wave][x] == c;
            const unsigned long long maskM = __ballot(mem), maskN = __ballot(valid && !mem);
            const unsigned long long m = (mem ? maskN : maskM) & (lane == 63 ? ~0ull : ((2ull << lane) - 1ull));
            const int before = mem ? lastN : lastM;
            const int pos = m ? xb + 63 - __clzll((long long)m) : before;
            if (valid) left[wave][x] = (unsigned short)(pos < 0 ? SDM_G1_NONE : x - pos);
            if (maskM) lastM = xb + 63 - __clzll((long long)maskM);
            if (maskN) lastN = xb + 63 - __clzll((long long)maskN);
            members += (unsigned)__popcll(maskM);
        }
        int nextM = -1, nextN = -1;
        for (int k = nchunk - 1; k >= 0; --k) {
            const int xb = k << 6, x = xb + lane;
            const bool valid = x < W, mem = valid && cls[wave][x] == c;
            const unsigned long long maskM = __ballot(mem), maskN = __ballot(valid && !mem);
            const unsigned long long m = (mem ? maskN : maskM) & (~0ull << lane);
            const int after = mem ? nextN : nextM;
            const int pos = m ? xb + __ffsll((long long)m) - 1 : after;
            if (valid) {
                const int dl = left[wave][x], dr = pos < 0 ? SDM_G1_NONE : pos - x;
                out[x] = (unsigned short)((dl < dr ? dl : dr) | (mem ? SDM_G1_MEMBER : 0));
            }
            if (maskM) nextM = xb + __ffsll((long long)maskM) - 1;
            if (maskN) nextN = xb + __ffsll((long long)maskN) - 1;
        }
        if (lane == 0 && members) atomicAdd(&counts[b * ncls + c], members);
    }
}

// one cell of a column walk: the squared distance it offers a query of membership `member` dy rows away (dy2 = dy^2)
__device__ __forceinline__ void sdm_take(int& best, unsigned cell, unsigned member, int dy2) {
    const int f = (int)(cell & SDM_G1_NONE);
    if ((cell & SDM_G1_MEMBER) != member) best = min(best, dy2);       // the other membership, in the query's own column
    else if (f != SDM_G1_NONE) best = min(best, f * f + dy2);
}

// Column pass: a workgroup takes TX columns of one plane (b, c), one column per lane so that the loads of g1 and the stores of
// phi are contiguous across lanes, and holds their H x TX cells in LDS.  A query walks its column outward from its own row and
// stops once dy^2 reaches the best squared distance so far (seg_edt_y_kernel's bounded walk, four rows a trip).  A plane whose
// class is empty or the whole slice has no boundary: zeros, and g1 is not read.
__global__ __launch_bounds__(256) void sdm_col_kernel(const unsigned short* __restrict__ g1, const unsigned* __restrict__ counts,
                                                      float* __restrict__ phi, int H, int W, int TX, int col_tiles) {
    extern __shared__ unsigned short col[];          // [H][TX]
    const int tile = blockIdx.x % col_tiles;
    const long plane = blockIdx.x / col_tiles;
    const int cx = threadIdx.x % TX, yg = threadIdx.x / TX, G = 256 / TX;
    const int x = tile * TX + cx;
    const bool live = x < W;
    const long base = plane * H * W + x;
    const unsigned n = counts[plane];
    if (n == 0u || n == (unsigned)(H * W)) {
        if (live)
            for (int yy = yg; yy < H; yy += G) phi[base + (long)yy * W] = 0.f;
        return;
    }
    if (live)
        for (int yy = yg; yy < H; yy += G) col[yy * TX + cx] = g1[base + (long)yy * W];
    __syncthreads();
    if (!live) return;
    for (int yy = yg; yy < H; yy += G) {
        const unsigned own = col[yy * TX + cx], member = own & SDM_G1_MEMBER;
        const int f = (int)(own & SDM_G1_NONE);
        int best = f == SDM_G1_NONE ? 0x7FFFFFFF : f * f;
        // four rows each way per trip: the eight reads are independent and overlap; a row past the stopping distance only
        // offers a larger candidate
        for (int d = 1;; d += 4) {
            const bool lo = yy - d >= 0, hi = yy + d < H;
            if (d * d >= best || !(lo || hi)) break;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int dk = d + k, d2 = dk * dk;
                if (yy - dk >= 0) sdm_take(best, col[(yy - dk) * TX + cx], member, d2);
                if (yy + dk < H) sdm_take(best, col[(yy + dk) * TX + cx], member, d2);
            }
        }
        // the root in double, then one rounding: np.float32(np.sqrt(np.float64(d2))); inside, 1 - root in double before it
        const double r = sqrt((double)best);
        phi[base + (long)yy * W] = member ? (float)(1.0 - r) : (float)r;
    }
}

}  // namespace

extern "C" {

size_t cswin_sdm_workspace(int B, int ncls, int H, int W) {
    if (!sdm_plan(B, ncls, H, W).ok) {
        cswin_set_error("sdm_workspace: B=%d ncls=%d H=%d W=%d outside B >= 1, ncls in [%d, %d], 1 <= H, W <= %d", B, ncls, H, W,
                        SDM_MIN_NCLS, SDM_MAX_NCLS, SDM_MAX_DIM);
        return 0;
    }
    return sdm_workspace_bytes(B, ncls, H, W);
}

// labels (B, H, W) int64 -> phi (B, ncls, H, W) fp32
int cswin_signed_distance_maps(const long long* labels, float* phi, void* workspace, size_t ws_bytes, int B, int ncls, int H,
                               int W, void* stream) {
    CSWIN_REQUIRE(labels && phi && B > 0, CSWIN_ERR_SHAPE, "signed_distance_maps: bad arguments");
    CSWIN_REQUIRE(sdm_dim_ok(H) && sdm_dim_ok(W), CSWIN_ERR_SHAPE, "signed_distance_maps: H=%d W=%d outside [1, %d]", H, W, SDM_MAX_DIM);
    CSWIN_REQUIRE(sdm_ncls_ok(ncls), CSWIN_ERR_UNSUPPORTED, "signed_distance_maps: num_classes=%d outside [%d, %d]", ncls, SDM_MIN_NCLS, SDM_MAX_NCLS);
    const SdmPlan p = sdm_plan(B, ncls, H, W);
    CSWIN_REQUIRE(p.ok, CSWIN_ERR_SHAPE, "signed_distance_maps: B=%d ncls=%d H=%d W=%d is more than one launch covers", B, ncls, H, W);
    CSWIN_REQUIRE(workspace && ws_bytes >= sdm_workspace_bytes(B, ncls, H, W), CSWIN_ERR_WORKSPACE, "signed_distance_maps: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    unsigned* counts = (unsigned*)workspace;
    unsigned short* g1 = (unsigned short*)((char*)workspace + sdm_counts_bytes(B, ncls));
    if (hipMemsetAsync(counts, 0, (size_t)B * ncls * sizeof(unsigned), st) != hipSuccess) {
        cswin_set_error("signed_distance_maps: hipMemsetAsync failed");
        return CSWIN_ERR_HIP;
    }
    hipLaunchKernelGGL(sdm_row_kernel, dim3((unsigned)p.row_blocks), dim3(256), 0, st, labels, g1, counts, (long)B * H, ncls, H, W);
    CSWIN_LAUNCH_CHECK();
    hipLaunchKernelGGL(sdm_col_kernel, dim3((unsigned)p.col_blocks), dim3(256), (size_t)p.lds_bytes, st, g1, counts, phi, H, W, p.TX, p.col_tiles);
    CSWIN_LAUNCH_CHECK();
    return CSWIN_OK;
}

}  // extern "C"
