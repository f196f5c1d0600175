// Test-time augmentation of a volume evaluation: the views of a batch of slices before the network, and the ensemble of the
// network's answers after it (utils.predict_volume(resize="hip", tta=...)).  A view is one of the eight symmetries of the square,
// a code 0..7 (tta_plan.h: transpose, reverse rows, reverse columns); training's random_rot_flip draws from the same group.
//
//   cswin_view_batch            y[v][b] = view_{views[v]}(x[b]), a copy.
//   cswin_tta_argmax_zoom_back  P[b][k][r][s] = (1 / V) sum_v softmax_k(logits[v][b][classes[k]] at view v's image of (r, s)),
//                               out[b][i][j] = argmax_k P[b][k][src_row[i]][src_col[j]]  (torch.argmax's tie and NaN rules).
//
// Both give a workgroup a square tile of SOURCE pixels (tta_plan.h: 32 x 32 for the copy, 16 x 16 for the ensemble): the image of
// the tile under any view is a square tile of that view's frame, so every global access runs along rows, and what a transposing
// view reads along the other axis goes through a padded LDS tile.  The ensemble visits every source pixel once (V nsel expf each) and the workgroup that owns a tile writes every
// output pixel that gathers from it, so there is no intermediate map and no second launch.  No atomics anywhere: every sum has
// one fixed order and two runs give the same bits.
#include "common.h"
#include "tta_plan.h"

namespace {

// ---- view_batch ---------------------------------------------------------------------------------------------------------------
// 256 threads = 8 rows x 32 lanes, four passes over the tile.  A straight view copies row by row (a reversed row is still one
// contiguous segment per 32 lanes).  A transposing view reads the source tile along its rows into LDS and writes the view's tile
// along the view's rows: lane tx then holds source row r0 + tx, column tile[tx][..] of the LDS image (stride 33: no conflict).
__global__ __launch_bounds__(TTA_VIEW_THREADS) void view_batch_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                                     unsigned packed, int B, int h, int w) {
    __shared__ float tile[TTA_VIEW_TILE][TTA_VIEW_LD];
    const int tx = threadIdx.x & (TTA_VIEW_TILE - 1), ty = threadIdx.x / TTA_VIEW_TILE;
    const int v = blockIdx.z / B, b = blockIdx.z - v * B, c = tta_code(packed, v);
    const int r0 = blockIdx.y * TTA_VIEW_TILE, s0 = blockIdx.x * TTA_VIEW_TILE;
    const float* __restrict__ src = x + (long)b * h * w;
    float* __restrict__ dst = y + (long)blockIdx.z * h * w;              // a transposing view has h == w: the plane is h w either way
    const int wv = tta_transposes(c) ? h : w;
    if (!tta_transposes(c)) {
#pragma unroll
        for (int p = 0; p < TTA_VIEW_TILE; p += TTA_VIEW_THREADS / TTA_VIEW_TILE) {
            const int r = r0 + ty + p, s = s0 + tx;
            if (r < h && s < w) {
                const TtaPos q = tta_view_pos(c, r, s, h, w);
                dst[(long)q.i * wv + q.j] = src[(long)r * w + s];
            }
        }
        return;
    }
#pragma unroll
    for (int p = 0; p < TTA_VIEW_TILE; p += TTA_VIEW_THREADS / TTA_VIEW_TILE) {
        const int r = r0 + ty + p, s = s0 + tx;
        if (r < h && s < w) tile[ty + p][tx] = src[(long)r * w + s];
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < TTA_VIEW_TILE; p += TTA_VIEW_THREADS / TTA_VIEW_TILE) {
        const int r = r0 + tx, s = s0 + ty + p;                          // lanes along r: along j of the transposed frame
        if (r < h && s < w) {
            const TtaPos q = tta_view_pos(c, r, s, h, w);
            dst[(long)q.i * wv + q.j] = tile[tx][ty + p];
        }
    }
}

// ---- the ensemble -------------------------------------------------------------------------------------------------------------
struct TtaArgs {
    const float* logits;
    unsigned char* out;
    float* probs;
    const int* src_row;
    const int* src_col;
    const int* classes;
    unsigned packed;
    int V, nsel, B, ncls, h, w, H, W;
};

// The logits of view v at this thread's pixel, candidates k0 .. k0 + CH (those below nsel), into l[].  A straight view is read
// in place: the lanes of a tile row read one segment.  A transposing view is read by the thread of the MIRRORED position of
// the tile, (tx, ty), whose lanes then run along the view's rows; the values cross over through LDS, TTA_STAGE_CH channels per
// barrier pair.  Called by every thread of the workgroup (the barriers), `inside` or not.
template <int CH>
__device__ __forceinline__ void load_logits(const TtaArgs& a, float (*stage)[TTA_TILE][TTA_LD], int v, int b, int k0, int r0, int s0,
                                            int tx, int ty, float (&l)[CH]) {
    const int c = tta_code(a.packed, v);
    const long plane = (long)a.h * a.w;
    const float* __restrict__ base = a.logits + ((long)v * a.B + b) * a.ncls * plane;
    auto channel = [&](int k) -> long { return (a.classes ? (long)min(max(a.classes[k], 0), a.ncls - 1) : (long)k) * plane; };
    if (!tta_transposes(c)) {
        const int r = r0 + ty, s = s0 + tx;
        if (r < a.h && s < a.w) {
            const TtaPos q = tta_view_pos(c, r, s, a.h, a.w);
            const long at = (long)q.i * a.w + q.j;
#pragma unroll
            for (int k = 0; k < CH; ++k)
                if (k0 + k < a.nsel) l[k] = base[channel(k0 + k) + at];
        }
        return;
    }
    const int r = r0 + tx, s = s0 + ty;                                  // the pixel this thread fetches for thread (tx, ty)
    const TtaPos q = tta_view_pos(c, min(r, a.h - 1), min(s, a.w - 1), a.h, a.w);
    const long at = (long)q.i * a.h + q.j;                               // h == w
    const bool fetch = r < a.h && s < a.w;
#pragma unroll
    for (int g = 0; g < CH; g += TTA_STAGE_CH) {
        if (k0 + g < a.nsel) {                                           // uniform over the workgroup
            if (fetch) {
#pragma unroll
                for (int k = 0; k < TTA_STAGE_CH; ++k)
                    if (g + k < CH && k0 + g + k < a.nsel) stage[k][ty][tx] = base[channel(k0 + g + k) + at];
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < TTA_STAGE_CH; ++k)
                if (g + k < CH && k0 + g + k < a.nsel) l[g + k] = stage[k][tx][ty];
            __syncthreads();
        }
    }
}

// argmax with torch's rules: the first index wins a tie, a NaN beats every number and the first NaN wins
__device__ __forceinline__ void argmax_step(float v, int k, float& best, int& arg) {
    if (!(best != best) && (v > best || v != v)) {
        best = v;
        arg = k;
    }
}

// One workgroup per (column tile, row tile, b); thread (ty, tx) owns source pixel (r0 + ty, s0 + tx).
// Per view, in ascending v: m = max_k l_k, e_k = expf(l_k - m), S = sum_k e_k in ascending k, acc_k += e_k / S; then P_k =
// acc_k (1 / V) and the argmax.  GENERAL = false keeps l and acc in registers (nsel <= TTA_REG_CLS); GENERAL = true keeps acc in
// probs[b][k][r][s] and reads the view's logits three times, TTA_REG_CLS candidates at a time (the second expf of a candidate
// gives the same bits as the first).  Then the class tile goes to LDS and the workgroup writes every output pixel that gathers
// from it: output row i belongs to the row tile of min(src_row[i], h - 1), or to row tile 0 if it is negative (the output is
// then 0), columns alike, so every output pixel has exactly one writer whatever the tables hold.  Wave 0 lists the workgroup's
// rows and wave 1 its columns, in ascending order by ballot and prefix count (no atomics).
template <bool GENERAL>
__global__ __launch_bounds__(TTA_THREADS) void tta_ensemble_kernel(TtaArgs a) {
    __shared__ float stage[TTA_STAGE_CH][TTA_TILE][TTA_LD];
    __shared__ unsigned char cls[TTA_TILE][TTA_LD];
    __shared__ int list[2][TTA_MAX_DIM];
    __shared__ int count[2];
    const int tx = threadIdx.x & (TTA_TILE - 1), ty = threadIdx.x / TTA_TILE;
    const int b = blockIdx.z, r0 = blockIdx.y * TTA_TILE, s0 = blockIdx.x * TTA_TILE;
    const int r = r0 + ty, s = s0 + tx;
    const bool inside = r < a.h && s < a.w;
    const long plane = (long)a.h * a.w;
    const float inv = 1.0f / (float)a.V;
    float best = 0.f;
    int arg = 0;
    if constexpr (!GENERAL) {
        float acc[TTA_REG_CLS];
#pragma unroll
        for (int k = 0; k < TTA_REG_CLS; ++k) acc[k] = 0.f;
        for (int v = 0; v < a.V; ++v) {
            float l[TTA_REG_CLS];
#pragma unroll
            for (int k = 0; k < TTA_REG_CLS; ++k) l[k] = 0.f;
            load_logits<TTA_REG_CLS>(a, stage, v, b, 0, r0, s0, tx, ty, l);
            float m = l[0];
#pragma unroll
            for (int k = 1; k < TTA_REG_CLS; ++k)
                if (k < a.nsel) m = fmaxf(m, l[k]);
            float sum = 0.f;
#pragma unroll
            for (int k = 0; k < TTA_REG_CLS; ++k)
                if (k < a.nsel) {
                    l[k] = expf(l[k] - m);
                    sum += l[k];
                }
#pragma unroll
            for (int k = 0; k < TTA_REG_CLS; ++k)
                if (k < a.nsel) acc[k] += l[k] / sum;
        }
        float* __restrict__ P = a.probs ? a.probs + (long)b * a.nsel * plane + (long)r * a.w + s : nullptr;
#pragma unroll
        for (int k = 0; k < TTA_REG_CLS; ++k)
            if (k < a.nsel) {
                const float p = acc[k] * inv;
                if (k == 0) best = p;
                else argmax_step(p, k, best, arg);
                if (P && inside) P[k * plane] = p;
            }
    } else {
        float* __restrict__ P = a.probs + (long)b * a.nsel * plane + (long)min(r, a.h - 1) * a.w + min(s, a.w - 1);
        for (int v = 0; v < a.V; ++v) {
            float l[TTA_REG_CLS];
#pragma unroll
            for (int k = 0; k < TTA_REG_CLS; ++k) l[k] = 0.f;
            float m = 0.f, sum = 0.f;
            for (int k0 = 0; k0 < a.nsel; k0 += TTA_REG_CLS) {
                load_logits<TTA_REG_CLS>(a, stage, v, b, k0, r0, s0, tx, ty, l);
                if (k0 == 0) m = l[0];
#pragma unroll
                for (int k = 0; k < TTA_REG_CLS; ++k)
                    if (k0 + k < a.nsel) m = fmaxf(m, l[k]);
            }
            for (int k0 = 0; k0 < a.nsel; k0 += TTA_REG_CLS) {
                load_logits<TTA_REG_CLS>(a, stage, v, b, k0, r0, s0, tx, ty, l);
#pragma unroll
                for (int k = 0; k < TTA_REG_CLS; ++k)
                    if (k0 + k < a.nsel) sum += expf(l[k] - m);
            }
            for (int k0 = 0; k0 < a.nsel; k0 += TTA_REG_CLS) {
                load_logits<TTA_REG_CLS>(a, stage, v, b, k0, r0, s0, tx, ty, l);
                if (inside) {
#pragma unroll
                    for (int k = 0; k < TTA_REG_CLS; ++k)
                        if (k0 + k < a.nsel) {
                            const float p = expf(l[k] - m) / sum;
                            P[(k0 + k) * plane] = v == 0 ? p : P[(k0 + k) * plane] + p;
                        }
                }
            }
        }
        if (inside) {
            for (int k = 0; k < a.nsel; ++k) {
                const float p = P[k * plane] * inv;
                P[k * plane] = p;
                if (k == 0) best = p;
                else argmax_step(p, k, best, arg);
            }
        }
    }
    cls[ty][tx] = (unsigned char)arg;

    // the output rows (wave 0) and columns (wave 1) of this tile: entry = output index << 6 | local source index, or | TTA_ZERO
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (wave < 2) {
        const int* __restrict__ table = wave ? a.src_col : a.src_row;
        const int n_out = wave ? a.W : a.H, n_in = wave ? a.w : a.h, t0 = wave ? s0 : r0, tile = wave ? blockIdx.x : blockIdx.y;
        int n = 0;
        for (int i0 = 0; i0 < n_out; i0 += 64) {
            const int i = i0 + lane;
            const int src = i < n_out ? table[i] : 0;
            const int at = min(src, n_in - 1);
            const bool mine = i < n_out && (src < 0 ? tile == 0 : (at >= t0 && at < t0 + TTA_TILE));
            const unsigned long long mask = __ballot(mine);
            if (mine) list[wave][n + __popcll(mask & ((1ull << lane) - 1ull))] = i << 6 | (src < 0 ? TTA_ZERO : at - t0);
            n += __popcll(mask);
        }
        if (lane == 0) count[wave] = n;
    }
    __syncthreads();
    const int nr = count[0], nc = count[1];
    unsigned char* __restrict__ o = a.out + (long)b * a.H * a.W;
    for (int ii = ty; ii < nr; ii += TTA_TILE) {
        const int er = list[0][ii];
        for (int jj = tx; jj < nc; jj += TTA_TILE) {
            const int ec = list[1][jj];
            o[(long)(er >> 6) * a.W + (ec >> 6)] = ((er | ec) & TTA_ZERO) ? (unsigned char)0 : cls[er & (TTA_ZERO - 1)][ec & (TTA_ZERO - 1)];
        }
    }
}

const char* const TTA_REFUSALS[] = {"", "V=%d views outside 1..8", "views[%d] is not a view code in 0..7",
                                    "views[%d] transposes, which needs h == w"};

}  // namespace

extern "C" {

int cswin_view_batch(const float* x, float* y, const int* views, int V, int B, int h, int w, void* stream) {
    CSWIN_REQUIRE(x && y && views, CSWIN_ERR_SHAPE, "view_batch: null argument");
    CSWIN_REQUIRE(tta_dim_ok(B) && tta_dim_ok(h) && tta_dim_ok(w), CSWIN_ERR_SHAPE,
                  "view_batch: B=%d, (%d, %d) outside the supported 1..%d per dimension", B, h, w, TTA_MAX_DIM);
    const TtaViews p = tta_pack_views(views, V, h, w);
    if (p.refusal != TTA_OK) {
        char fmt[128];
        snprintf(fmt, sizeof fmt, "view_batch: %s (h=%%d, w=%%d)", TTA_REFUSALS[p.refusal]);
        CSWIN_REQUIRE(false, CSWIN_ERR_SHAPE, fmt, p.refusal == TTA_BAD_COUNT ? V : p.bad, h, w);
    }
    CSWIN_REQUIRE(x != y, CSWIN_ERR_UNSUPPORTED, "view_batch: x == y (a view is not made in place)");
    CSWIN_REQUIRE((uintptr_t)x % 4 == 0 && (uintptr_t)y % 4 == 0, CSWIN_ERR_ALIGN, "view_batch: a pointer is not aligned to its element size");
    const TtaGrid g = tta_view_grid(V, B, h, w);
    hipLaunchKernelGGL(view_batch_kernel, dim3(g.x, g.y, g.z), dim3(TTA_VIEW_THREADS), 0, (hipStream_t)stream, x, y, p.packed, B, h, w);
    CSWIN_LAUNCH_CHECK();
    return CSWIN_OK;
}

int cswin_tta_argmax_zoom_back(const float* logits, unsigned char* out, float* probs, const int* src_row, const int* src_col,
                               const int* views, int V, const int* classes, int nsel, int B, int ncls, int h, int w, int H, int W,
                               void* stream) {
    CSWIN_REQUIRE(logits && out && src_row && src_col && views, CSWIN_ERR_SHAPE, "tta_argmax_zoom_back: null argument");
    CSWIN_REQUIRE(tta_dim_ok(B) && tta_dim_ok(h) && tta_dim_ok(w) && tta_dim_ok(H) && tta_dim_ok(W), CSWIN_ERR_SHAPE,
                  "tta_argmax_zoom_back: B=%d, (%d, %d) -> (%d, %d) outside the supported 1..%d per dimension", B, h, w, H, W,
                  TTA_MAX_DIM);
    CSWIN_REQUIRE(nsel >= 1 && nsel <= TTA_MAX_CLS, CSWIN_ERR_SHAPE, "tta_argmax_zoom_back: nsel=%d outside 1..%d", nsel, TTA_MAX_CLS);
    CSWIN_REQUIRE(ncls >= 1 && (classes || nsel == ncls), CSWIN_ERR_SHAPE,
                  "tta_argmax_zoom_back: ncls=%d must be positive, and nsel=%d equal to it without a class list", ncls, nsel);
    const TtaViews p = tta_pack_views(views, V, h, w);
    if (p.refusal != TTA_OK) {
        char fmt[128];
        snprintf(fmt, sizeof fmt, "tta_argmax_zoom_back: %s (h=%%d, w=%%d)", TTA_REFUSALS[p.refusal]);
        CSWIN_REQUIRE(false, CSWIN_ERR_SHAPE, fmt, p.refusal == TTA_BAD_COUNT ? V : p.bad, h, w);
    }
    const TtaPlan plan = tta_plan(B, nsel, h, w);
    CSWIN_REQUIRE(probs || !plan.general, CSWIN_ERR_WORKSPACE,
                  "tta_argmax_zoom_back: nsel=%d > %d keeps its sums in probs, which is NULL", nsel, TTA_REG_CLS);
    CSWIN_REQUIRE((uintptr_t)logits % 4 == 0 && (uintptr_t)probs % 4 == 0 && (uintptr_t)src_row % 4 == 0 && (uintptr_t)src_col % 4 == 0 &&
                      (uintptr_t)classes % 4 == 0,
                  CSWIN_ERR_ALIGN, "tta_argmax_zoom_back: a pointer is not aligned to its element size");
    const TtaArgs a = {logits, out, probs, src_row, src_col, classes, p.packed, V, nsel, B, ncls, h, w, H, W};
    const dim3 grid(plan.grid.x, plan.grid.y, plan.grid.z), block(plan.threads);
    if (plan.general) hipLaunchKernelGGL(tta_ensemble_kernel<true>, grid, block, 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(tta_ensemble_kernel<false>, grid, block, 0, (hipStream_t)stream, a);
    CSWIN_LAUNCH_CHECK();
    return CSWIN_OK;
}

}  // extern "C"
