// Views and launch policy of the test-time-augmentation kernels (tta.hip), host only: plain C++, no HIP.  tta.hip launches what
// tta_view_grid / tta_plan return and maps pixels with tta_view_pos; tools/tta_plan_check.cpp prints both for request lines,
// which is how tests/test_tta_plan_host.py holds them to numpy and to the limits of the hardware.
#pragma once

#ifdef __HIPCC__
#define TTA_HD __host__ __device__
#else
#define TTA_HD
#endif

constexpr int TTA_MAX_DIM = 2048;          // per dimension (and slices per call)
constexpr int TTA_MAX_CLS = 255;           // candidates of the argmax: the result is a byte
constexpr int TTA_MAX_VIEWS = 8;           // the eight symmetries of the square
// The ensemble: a workgroup owns TTA_TILE x TTA_TILE source pixels, one per thread.  32 x 32 (1024 threads, 128-byte row segments)
// gives a batch of two 224 x 224 slices 98 workgroups for 256 CUs, and the kernel is bound by the expf and divisions of the CUs
// that have one: 46.2 us for (V, B, nsel) = (8, 2, 9), 22.7 us for (4, 4, 9).  16 x 16 gives 392: DESIGN.md has both measurements.
constexpr int TTA_TILE = 16;
constexpr int TTA_LD = TTA_TILE + 1;       // LDS row stride of a staged tile, odd: a column read (stride TTA_LD) and a row write
                                           // (stride 1) by a 32-lane group meet on at most one bank (none at a 32 x 33 tile)
constexpr int TTA_THREADS = TTA_TILE * TTA_TILE;
constexpr int TTA_ZERO = 32;               // list entry = output index << 6 | local source index, or | TTA_ZERO: the output is 0
static_assert(TTA_TILE <= TTA_ZERO && TTA_THREADS >= 128 && TTA_THREADS <= 1024, "two waves list, local indices stay below the flag");
constexpr int TTA_VIEW_TILE = 32;          // view_batch: 32 x 32 source pixels through a 32 x 33 LDS tile
constexpr int TTA_VIEW_LD = TTA_VIEW_TILE + 1;
constexpr int TTA_REG_CLS = 16;            // nsel up to here: accumulators in registers; above: in the probs buffer
constexpr int TTA_STAGE_CH = 8;            // channels of a transposing view staged through LDS per barrier pair
constexpr int TTA_VIEW_THREADS = 256;      // view_batch: 8 rows of 32 lanes, four passes over a tile

// A view code c in 0..7: bit 0 = transpose, bit 1 = reverse the rows, bit 2 = reverse the columns, applied in that order:
//   a = x.T if c & 1 else x;  a = a[::-1, :] if c & 2 else a;  a = a[:, ::-1] if c & 4 else a.
// Source pixel (r, s) of an (h, w) slice sits at the returned (i, j) of the viewed frame, which is (w, h) for a transposing view.
struct TtaPos { int i, j; };
TTA_HD inline bool tta_transposes(int c) { return c & 1; }
TTA_HD inline TtaPos tta_view_pos(int c, int r, int s, int h, int w) {
    const int hv = (c & 1) ? w : h, wv = (c & 1) ? h : w;
    const int i2 = (c & 1) ? s : r, j2 = (c & 1) ? r : s;
    return {(c & 2) ? hv - 1 - i2 : i2, (c & 4) ? wv - 1 - j2 : j2};
}

// the V codes of a call travel as one kernel argument, three bits each
TTA_HD inline int tta_code(unsigned packed, int v) { return (int)((packed >> (3 * v)) & 7u); }

inline bool tta_dim_ok(int n) { return n >= 1 && n <= TTA_MAX_DIM; }

// What the entry points refuse about a view list before anything is launched; OK = 0.
enum TtaRefusal { TTA_OK = 0, TTA_BAD_COUNT, TTA_BAD_CODE, TTA_NOT_SQUARE };
struct TtaViews { TtaRefusal refusal; int bad; unsigned packed; bool any_transposed; };
inline TtaViews tta_pack_views(const int* views, int V, int h, int w) {
    TtaViews p = {TTA_OK, -1, 0u, false};
    if (V < 1 || V > TTA_MAX_VIEWS) return {TTA_BAD_COUNT, -1, 0u, false};
    for (int v = 0; v < V; ++v) {
        if (views[v] < 0 || views[v] > 7) return {TTA_BAD_CODE, v, 0u, false};
        if (tta_transposes(views[v]) && h != w) return {TTA_NOT_SQUARE, v, 0u, false};
        p.packed |= (unsigned)views[v] << (3 * v);
        p.any_transposed |= tta_transposes(views[v]);
    }
    return p;
}

// Grid of either kernel: one workgroup per square tile of SOURCE pixels, so a transposing view's image of the tile is a square
// tile of its own frame as well and both orientations are read (and, in view_batch, written) along rows.
//   view_batch: z = V * B, the ensemble: z = B (a workgroup walks the views itself, in ascending order).
struct TtaGrid { int x, y, z; };
inline TtaGrid tta_view_grid(int V, int B, int h, int w) {
    return {(w + TTA_VIEW_TILE - 1) / TTA_VIEW_TILE, (h + TTA_VIEW_TILE - 1) / TTA_VIEW_TILE, V * B};
}

// The ensemble's launch.  general: nsel > TTA_REG_CLS, the per-class sums live in the probs buffer (which is then required) and
// every view's logits are read three times (max, sum, quotient); otherwise they are read once into registers.
// lds_bytes (static, below the 64 KiB a kernel gets without opt-in): the staged channels of a transposing view, the class tile,
// and the two lists of output rows / columns that gather from this tile (at most H and W entries).
struct TtaPlan { bool general; TtaGrid grid; int threads; long lds_bytes; };
inline TtaPlan tta_plan(int B, int nsel, int h, int w) {
    const long lds = (long)TTA_STAGE_CH * TTA_TILE * TTA_LD * 4 + (long)TTA_TILE * TTA_LD + 2L * TTA_MAX_DIM * 4 + 2 * 4;
    return {nsel > TTA_REG_CLS, {(w + TTA_TILE - 1) / TTA_TILE, (h + TTA_TILE - 1) / TTA_TILE, B}, TTA_THREADS, lds};
}
