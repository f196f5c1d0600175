// Training augmentation of a batch of raw slices (datasets/dataset_synapse.py RandomGenerator: np.rot90 + np.flip, or
// scipy.ndimage.rotate(order=0, reshape=False), then the zooms to the network's size) as device gathers.
//
// Nothing here restates scipy's rotation: the host reads the source index of every output pixel off scipy itself
// (cswin_unet_amd.utils.rotation_index: -1 where scipy writes its constant 0) and passes the map; quarter turns and the flip are
// the index rule of np.flip(np.rot90(x, k), axis) below.  A sample's transform T maps an output pixel (i, j) of the transformed
// slice (H', W') -- (W, H) after an odd number of quarter turns -- to a flat source index or to "none".  Both kernels copy values:
//   cswin_augment_gather  y[s][i][j] = x[src_s][T_s(i, j)], 0 where none; the cubic zoom that follows is cswin_resize_banded
//   cswin_augment_labels  out[s][i][j] = lab[src_s][T_s(src_row[i], src_col[j])]: the label's order-0 zoom (a gather through
//                         scipy's per-axis source indices, as in cswin_argmax_zoom_back) composed with T, so the transformed
//                         label at full size is never written
// Every index that comes from a table is clamped into range on the device: a bad table cannot make a kernel read outside its inputs.
#include "common.h"

namespace {

constexpr int AUG_MAX_DIM = 2048;          // per dimension (and slices / samples per call), as resize.hip
constexpr int AUG_TILE = 16;               // a workgroup = a 16 x 16 output tile of one sample

enum { AUG_NONE = 0, AUG_ROT90_FLIP = 1, AUG_ROTATE = 2 };

struct AugDesc {                           // mirrors cswin_augment_desc (include/cswin_hip.h): 24 bytes
    int kind, k, axis, src;
    const int* map;
};

// Flat source index of pixel (i, j) of the transformed slice, or -1.  (H, W): the source slice.  For a transposing sample the
// caller passes i < W, j < H; whatever it passes, the result lies in -1 .. H * W - 1.
__device__ __forceinline__ int aug_source(const AugDesc& d, int i, int j, int H, int W) {
    if (d.kind == AUG_ROTATE) {
        if (!d.map) return -1;
        const long p = min((long)i * W + j, (long)H * W - 1);
        return min(d.map[p], H * W - 1);                                // negative: scipy's constant
    }
    int r = i, c = j;
    if (d.kind == AUG_ROT90_FLIP) {
        const int k = d.k & 3;
        const int Ht = (k & 1) ? W : H, Wt = (k & 1) ? H : W;           // shape of np.rot90(x, k)
        if (d.axis == 0) i = Ht - 1 - i;                                // undo np.flip
        else j = Wt - 1 - j;
        // np.rot90(x, k)[i][j]:  k = 1: x[j][W-1-i]   k = 2: x[H-1-i][W-1-j]   k = 3: x[H-1-j][i]
        r = k == 0 ? i : k == 1 ? j : k == 2 ? H - 1 - i : H - 1 - j;
        c = k == 0 ? j : k == 1 ? W - 1 - i : k == 2 ? W - 1 - j : i;
    }
    r = min(max(r, 0), H - 1);
    c = min(max(c, 0), W - 1);
    return r * W + c;
}

// A 16 x 16 tile per workgroup rather than a row segment: after an odd number of quarter turns the lanes of an output row read
// down a source column, and a square tile then still reads 16 contiguous floats per source row.
__global__ __launch_bounds__(256) void augment_gather_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                             const AugDesc* __restrict__ table, int B, int H, int W, int Ho, int Wo) {
    const int s = blockIdx.z;
    AugDesc d = table[s];
    d.src = min(max(d.src, 0), B - 1);
    const int i = blockIdx.y * AUG_TILE + (threadIdx.x >> 4), j = blockIdx.x * AUG_TILE + (threadIdx.x & 15);
    if (i >= Ho || j >= Wo) return;
    const int p = aug_source(d, i, j, H, W);
    y[((long)s * Ho + i) * Wo + j] = p < 0 ? 0.f : x[(long)d.src * H * W + p];
}

__global__ __launch_bounds__(256) void augment_labels_kernel(const unsigned char* __restrict__ lab, long long* __restrict__ out,
                                                             const AugDesc* __restrict__ table, const int* __restrict__ src_row,
                                                             const int* __restrict__ src_col, const int* __restrict__ src_row_t,
                                                             const int* __restrict__ src_col_t, int B, int H, int W, int h, int w) {
    const int s = blockIdx.z;
    AugDesc d = table[s];
    d.src = min(max(d.src, 0), B - 1);
    const int i = blockIdx.y * AUG_TILE + (threadIdx.x >> 4), j = blockIdx.x * AUG_TILE + (threadIdx.x & 15);
    if (i >= h || j >= w) return;
    const int tr = d.kind == AUG_ROT90_FLIP && (d.k & 1);               // transformed slice is (W, H)
    const int Ht = tr ? W : H, Wt = tr ? H : W;
    const int si = tr ? src_row_t[i] : src_row[i], sj = tr ? src_col_t[j] : src_col[j];
    int p = -1;
    if (si >= 0 && sj >= 0) p = aug_source(d, min(si, Ht - 1), min(sj, Wt - 1), H, W);
    out[((long)s * h + i) * w + j] = p < 0 ? 0 : (long long)lab[(long)d.src * H * W + p];
}

bool aug_dim_ok(int n) { return n >= 1 && n <= AUG_MAX_DIM; }

}  // namespace

extern "C" {

int cswin_augment_gather(const float* x, float* y, const void* table, int n, int B, int H, int W, int Ho, int Wo, void* stream) {
    CSWIN_REQUIRE(x && y && table, CSWIN_ERR_SHAPE, "augment_gather: null argument");
    CSWIN_REQUIRE(aug_dim_ok(n) && aug_dim_ok(B) && aug_dim_ok(H) && aug_dim_ok(W), CSWIN_ERR_SHAPE,
                  "augment_gather: n=%d samples of B=%d slices (%d, %d) outside the supported 1..%d per dimension", n, B, H, W, AUG_MAX_DIM);
    CSWIN_REQUIRE((Ho == H && Wo == W) || (Ho == W && Wo == H), CSWIN_ERR_SHAPE,
                  "augment_gather: output (%d, %d) is neither the slices' (%d, %d) nor its transpose", Ho, Wo, H, W);
    CSWIN_REQUIRE((uintptr_t)x % 4 == 0 && (uintptr_t)y % 4 == 0 && (uintptr_t)table % 8 == 0, CSWIN_ERR_ALIGN,
                  "augment_gather: a pointer is not aligned to its element size");
    hipLaunchKernelGGL(augment_gather_kernel, dim3(cdiv(Wo, AUG_TILE), cdiv(Ho, AUG_TILE), n), dim3(256), 0, (hipStream_t)stream, x, y,
                       (const AugDesc*)table, B, H, W, Ho, Wo);
    CSWIN_LAUNCH_CHECK();
    return CSWIN_OK;
}

int cswin_augment_labels(const unsigned char* lab, long long* out, const void* table, const int* src_row, const int* src_col,
                         const int* src_row_t, const int* src_col_t, int n, int B, int H, int W, int h, int w, void* stream) {
    CSWIN_REQUIRE(lab && out && table && src_row && src_col && src_row_t && src_col_t, CSWIN_ERR_SHAPE, "augment_labels: null argument");
    CSWIN_REQUIRE(aug_dim_ok(n) && aug_dim_ok(B) && aug_dim_ok(H) && aug_dim_ok(W) && aug_dim_ok(h) && aug_dim_ok(w), CSWIN_ERR_SHAPE,
                  "augment_labels: n=%d samples of B=%d slices, (%d, %d) -> (%d, %d) outside the supported 1..%d per dimension", n, B, H, W,
                  h, w, AUG_MAX_DIM);
    CSWIN_REQUIRE((uintptr_t)out % 8 == 0 && (uintptr_t)table % 8 == 0 && (uintptr_t)src_row % 4 == 0 && (uintptr_t)src_col % 4 == 0 &&
                      (uintptr_t)src_row_t % 4 == 0 && (uintptr_t)src_col_t % 4 == 0,
                  CSWIN_ERR_ALIGN, "augment_labels: a pointer is not aligned to its element size");
    hipLaunchKernelGGL(augment_labels_kernel, dim3(cdiv(w, AUG_TILE), cdiv(h, AUG_TILE), n), dim3(256), 0, (hipStream_t)stream, lab, out,
                       (const AugDesc*)table, src_row, src_col, src_row_t, src_col_t, B, H, W, h, w);
    CSWIN_LAUNCH_CHECK();
    return CSWIN_OK;
}

}  // extern "C"
