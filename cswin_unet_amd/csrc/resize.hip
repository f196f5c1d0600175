// The two resizes around the network in a volume evaluation (utils.py:70-81): scipy.ndimage.zoom(order=3) of every slice to the
// network's input size, and argmax + scipy.ndimage.zoom(order=0) of the logits back to the slice's size.
//
// Neither kernel restates scipy's rules.  zoom of a 2-D slice is the separable linear map y = R_h x R_w^T, and the host takes
// each 1-D operator R (n_out x n_in) from scipy itself (zoom of the unit vectors: spline prefilter, mirror boundary and
// coordinate rule are inside).  R decays geometrically away from its diagonal, so it travels as a band: weights[n_out][T] and
// start[n_out], row i of R = weights[i][0..T) at columns start[i] .. start[i] + T.  The order-0 zoom is a gather whose source
// index per output row / column also comes from scipy.  The device does the arithmetic only:
//   cswin_resize_banded     y[d] = float32(R_h x[d] R_w^T), every product and sum in float64, one rounding at the store
//   cswin_argmax_zoom_back  out[b][i][j] = argmax_c logits[b][c][src_row[i]][src_col[j]]  (torch.argmax's tie and NaN rules);
//                           0 where an index is negative: scipy rounds such an output's coordinate past the last sample and
//                           writes its constant there (as it leaves the matching row of R all zero)
//   cswin_argmax_zoom_back_classes  the same over a list of classes: out = the POSITION k in the list of the largest of
//                           logits[b][classes[k]][..][..], torch.argmax(logits[:, classes], 1) before the zoom (how a continual
//                           model is scored on one dataset's own classes, universal_test.py:50-54)
#include "common.h"

namespace {

constexpr int RZ_MAX_DIM = 2048;           // per dimension (and slices per call)
constexpr int RZ_MAX_CLS = 255;
constexpr int RZ_LDS_ELEMS = 8192;         // TR * W doubles = 64 KiB, the dynamic LDS a kernel gets without opt-in

typedef double f64x2 __attribute__((ext_vector_type(2)));

struct ResizeArgs {
    const void* x;
    float* y;
    const double* wh;
    const int* sh;
    const double* ww;
    const int* sw;
    int Th, Tw, H, W, h, w;
};

template <bool F64>
__device__ __forceinline__ double rz_load1(const void* __restrict__ x, long i) {
    if constexpr (F64) return static_cast<const double*>(x)[i];
    else return (double)static_cast<const float*>(x)[i];
}
template <bool F64>
__device__ __forceinline__ f64x2 rz_load2(const void* __restrict__ x, long i) {          // i even, base 16-B (8-B for fp32) aligned
    if constexpr (F64) return *reinterpret_cast<const f64x2*>(static_cast<const double*>(x) + i);
    else {
        const u32x2 v = *reinterpret_cast<const u32x2*>(static_cast<const float*>(x) + i);          // float pairs as integers: see common.h
        return f64x2{(double)__uint_as_float(v.x), (double)__uint_as_float(v.y)};
    }
}

// One workgroup = one slice x TR consecutive output rows.
// H pass: a thread owns VEC adjacent columns and walks the input rows that the tile's windows cover ONCE, from the first window's
//   start to the last one's end (overlapping windows of neighbouring output rows share their rows: 105 row reads instead of
//   16 x 68 for 512 -> 224).  Row and window are the same for every lane, so the window test is a scalar branch and the weight a
//   scalar load; TR accumulators per column live in registers and are summed in ascending input row.  The TR x W float64 image
//   goes to LDS.
// W pass: a thread owns an output column j and all TR rows of it: one weight load per tap feeds TR FMAs on LDS operands,
//   summed in ascending input column; stores are contiguous across lanes.
// Window starts are clamped into [0, n_in - T] on the device: a bad table cannot make the kernel read outside x.
template <int TR, int VEC, bool F64>
__global__ __launch_bounds__(256) void resize_banded_kernel(ResizeArgs a) {
    extern __shared__ __attribute__((aligned(16))) double img[];          // [TR][W]
    const int d = blockIdx.y, r0 = blockIdx.x * TR;
    const int H = a.H, W = a.W, Th = a.Th, Tw = a.Tw;

    int s[TR];
    int row_lo = H, row_hi = 0;
#pragma unroll
    for (int i = 0; i < TR; ++i) {
        if (r0 + i < a.h) {
            s[i] = min(max(a.sh[r0 + i], 0), H - Th);
            row_lo = min(row_lo, s[i]);
            row_hi = max(row_hi, s[i] + Th);
        } else s[i] = 2 * RZ_MAX_DIM;                                   // row - s[i] < 0 for every row: never inside a window
    }
    const double* __restrict__ wh = a.wh + (long)r0 * Th;
    const long xbase = (long)d * H * W;

    for (int c = threadIdx.x * VEC; c < W; c += 256 * VEC) {
        double acc[TR][VEC];
#pragma unroll
        for (int i = 0; i < TR; ++i)
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[i][v] = 0.0;
        for (int row = row_lo; row < row_hi; ++row) {
            double xv[VEC];
            if constexpr (VEC == 2) {
                const f64x2 t = rz_load2<F64>(a.x, xbase + (long)row * W + c);
                xv[0] = t.x;
                xv[1] = t.y;
            } else xv[0] = rz_load1<F64>(a.x, xbase + (long)row * W + c);
#pragma unroll
            for (int i = 0; i < TR; ++i) {
                const int t = row - s[i];
                if ((unsigned)t < (unsigned)Th) {
                    const double wgt = wh[i * Th + t];
#pragma unroll
                    for (int v = 0; v < VEC; ++v) acc[i][v] = fma(wgt, xv[v], acc[i][v]);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < TR; ++i) {
            if constexpr (VEC == 2) *reinterpret_cast<f64x2*>(img + i * W + c) = f64x2{acc[i][0], acc[i][1]};
            else img[i * W + c] = acc[i][0];
        }
    }
    __syncthreads();

    const int nrow = min(TR, a.h - r0);
    for (int j = threadIdx.x; j < a.w; j += 256) {
        const int sj = min(max(a.sw[j], 0), W - Tw);
        const double* __restrict__ wj = a.ww + (long)j * Tw;
        double acc[TR];
#pragma unroll
        for (int i = 0; i < TR; ++i) acc[i] = 0.0;
        for (int t = 0; t < Tw; ++t) {
            const double wgt = wj[t];
#pragma unroll
            for (int i = 0; i < TR; ++i) acc[i] = fma(wgt, img[i * W + sj + t], acc[i]);
        }
        float* __restrict__ out = a.y + ((long)d * a.h + r0) * a.w + j;
#pragma unroll
        for (int i = 0; i < TR; ++i)
            if (i < nrow) out[(long)i * a.w] = (float)acc[i];
    }
}

template <int TR>
void resize_launch(const ResizeArgs& a, int D, int vec2, int f64, hipStream_t st) {
    const dim3 grid(cdiv(a.h, TR), D), block(256);
    const size_t lds = (size_t)TR * a.W * sizeof(double);
    if (vec2) {
        if (f64) hipLaunchKernelGGL((resize_banded_kernel<TR, 2, true>), grid, block, lds, st, a);
        else hipLaunchKernelGGL((resize_banded_kernel<TR, 2, false>), grid, block, lds, st, a);
    } else {
        if (f64) hipLaunchKernelGGL((resize_banded_kernel<TR, 1, true>), grid, block, lds, st, a);
        else hipLaunchKernelGGL((resize_banded_kernel<TR, 1, false>), grid, block, lds, st, a);
    }
}

// One workgroup per output row (b, i): the argmax over the classes of source row src_row[i] once into LDS, then the gather
// along the row.  First index wins a tie; a NaN beats every number and the first NaN wins (torch.argmax).  A negative source
// index marks an output that scipy does not gather but fills with its constant 0.
// SUBSET: candidate k of nsel reads channel classes[k], clamped into [0, ncls) like the index tables, and the result is k.  k is
// the same for every lane, so the table entry is a scalar load and the channel offset scalar arithmetic; a repeated class never
// wins at its later position (the comparison is strict).  Without SUBSET, nsel = ncls and candidate k is channel k.
template <bool SUBSET>
__global__ __launch_bounds__(256) void argmax_zoom_back_kernel(const float* __restrict__ logits, unsigned char* __restrict__ out,
                                                               const int* __restrict__ src_row, const int* __restrict__ src_col,
                                                               const int* __restrict__ classes, int nsel, int ncls, int h, int w,
                                                               int H, int W) {
    __shared__ unsigned char am[RZ_MAX_DIM];
    const int i = blockIdx.x, b = blockIdx.y;
    unsigned char* __restrict__ o = out + ((long)b * H + i) * W;
    if (src_row[i] < 0) {                                               // the same for the whole workgroup
        for (int j = threadIdx.x; j < W; j += 256) o[j] = 0;
        return;
    }
    const int r = min(src_row[i], h - 1);
    const long plane = (long)h * w;
    const float* __restrict__ src = logits + (long)b * ncls * plane + (long)r * w;
    auto channel = [&](int k) -> long {
        if constexpr (SUBSET) return (long)min(max(classes[k], 0), ncls - 1) * plane;
        else return k * plane;
    };
    for (int j = threadIdx.x; j < w; j += 256) {
        float best = src[channel(0) + j];
        int arg = 0;
        for (int c = 1; c < nsel; ++c) {
            const float v = src[channel(c) + j];
            if (!(best != best) && (v > best || v != v)) {
                best = v;
                arg = c;
            }
        }
        am[j] = (unsigned char)arg;
    }
    __syncthreads();
    for (int j = threadIdx.x; j < W; j += 256) {
        const int sc = src_col[j];
        o[j] = sc < 0 ? (unsigned char)0 : am[min(sc, w - 1)];
    }
}

bool rz_dim_ok(int n) { return n >= 1 && n <= RZ_MAX_DIM; }

}  // namespace

extern "C" {

int cswin_resize_banded(const void* x, float* y, const double* wh, const int* sh, int Th, const double* ww, const int* sw, int Tw,
                        int D, int H, int W, int h, int w, int x_f64, void* stream) {
    CSWIN_REQUIRE(x && y && wh && sh && ww && sw, CSWIN_ERR_SHAPE, "resize_banded: null argument");
    CSWIN_REQUIRE(rz_dim_ok(D) && rz_dim_ok(H) && rz_dim_ok(W) && rz_dim_ok(h) && rz_dim_ok(w), CSWIN_ERR_SHAPE,
                  "resize_banded: D=%d, (%d, %d) -> (%d, %d) outside the supported 1..%d per dimension", D, H, W, h, w, RZ_MAX_DIM);
    CSWIN_REQUIRE(Th >= 1 && Th <= H && Tw >= 1 && Tw <= W, CSWIN_ERR_SHAPE,
                  "resize_banded: band widths Th=%d, Tw=%d must lie in 1..H=%d and 1..W=%d", Th, Tw, H, W);
    CSWIN_REQUIRE(x_f64 == 0 || x_f64 == 1, CSWIN_ERR_UNSUPPORTED, "resize_banded: x_f64=%d (0 = float32 input, 1 = float64)", x_f64);
    const uintptr_t xa = (uintptr_t)x;
    CSWIN_REQUIRE(xa % (x_f64 ? 8 : 4) == 0 && (uintptr_t)y % 4 == 0 && (uintptr_t)wh % 8 == 0 && (uintptr_t)ww % 8 == 0 &&
                      (uintptr_t)sh % 4 == 0 && (uintptr_t)sw % 4 == 0,
                  CSWIN_ERR_ALIGN, "resize_banded: a pointer is not aligned to its element size");
    const ResizeArgs a = {x, y, wh, sh, ww, sw, Th, Tw, H, W, h, w};
    const int vec2 = W % 2 == 0 && xa % (x_f64 ? 16 : 8) == 0;          // two columns per lane: even rows stay aligned
    hipStream_t st = (hipStream_t)stream;
    if (W * 16 <= RZ_LDS_ELEMS) resize_launch<16>(a, D, vec2, x_f64, st);
    else if (W * 8 <= RZ_LDS_ELEMS) resize_launch<8>(a, D, vec2, x_f64, st);
    else resize_launch<4>(a, D, vec2, x_f64, st);
    CSWIN_LAUNCH_CHECK();
    return CSWIN_OK;
}

int cswin_argmax_zoom_back(const float* logits, unsigned char* out, const int* src_row, const int* src_col, int B, int ncls, int h,
                           int w, int H, int W, void* stream) {
    CSWIN_REQUIRE(logits && out && src_row && src_col, CSWIN_ERR_SHAPE, "argmax_zoom_back: null argument");
    CSWIN_REQUIRE(rz_dim_ok(B) && rz_dim_ok(h) && rz_dim_ok(w) && rz_dim_ok(H) && rz_dim_ok(W), CSWIN_ERR_SHAPE,
                  "argmax_zoom_back: B=%d, (%d, %d) -> (%d, %d) outside the supported 1..%d per dimension", B, h, w, H, W, RZ_MAX_DIM);
    CSWIN_REQUIRE(ncls >= 1 && ncls <= RZ_MAX_CLS, CSWIN_ERR_SHAPE, "argmax_zoom_back: ncls=%d outside 1..%d", ncls, RZ_MAX_CLS);
    CSWIN_REQUIRE((uintptr_t)logits % 4 == 0 && (uintptr_t)src_row % 4 == 0 && (uintptr_t)src_col % 4 == 0, CSWIN_ERR_ALIGN,
                  "argmax_zoom_back: a pointer is not aligned to its element size");
    hipLaunchKernelGGL(argmax_zoom_back_kernel<false>, dim3(H, B), dim3(256), 0, (hipStream_t)stream, logits, out, src_row, src_col,
                       (const int*)nullptr, ncls, ncls, h, w, H, W);
    CSWIN_LAUNCH_CHECK();
    return CSWIN_OK;
}

int cswin_argmax_zoom_back_classes(const float* logits, unsigned char* out, const int* src_row, const int* src_col, const int* classes,
                                   int nsel, int B, int ncls, int h, int w, int H, int W, void* stream) {
    CSWIN_REQUIRE(logits && out && src_row && src_col && classes, CSWIN_ERR_SHAPE, "argmax_zoom_back_classes: null argument");
    CSWIN_REQUIRE(rz_dim_ok(B) && rz_dim_ok(h) && rz_dim_ok(w) && rz_dim_ok(H) && rz_dim_ok(W), CSWIN_ERR_SHAPE,
                  "argmax_zoom_back_classes: B=%d, (%d, %d) -> (%d, %d) outside the supported 1..%d per dimension", B, h, w, H, W,
                  RZ_MAX_DIM);
    CSWIN_REQUIRE(nsel >= 1 && nsel <= RZ_MAX_CLS, CSWIN_ERR_SHAPE, "argmax_zoom_back_classes: nsel=%d outside 1..%d", nsel, RZ_MAX_CLS);
    CSWIN_REQUIRE(ncls >= 1, CSWIN_ERR_SHAPE, "argmax_zoom_back_classes: ncls=%d must be positive", ncls);
    CSWIN_REQUIRE((uintptr_t)logits % 4 == 0 && (uintptr_t)src_row % 4 == 0 && (uintptr_t)src_col % 4 == 0 && (uintptr_t)classes % 4 == 0,
                  CSWIN_ERR_ALIGN, "argmax_zoom_back_classes: a pointer is not aligned to its element size");
    hipLaunchKernelGGL(argmax_zoom_back_kernel<true>, dim3(H, B), dim3(256), 0, (hipStream_t)stream, logits, out, src_row, src_col,
                       classes, nsel, ncls, h, w, H, W);
    CSWIN_LAUNCH_CHECK();
    return CSWIN_OK;
}

}  // extern "C"
