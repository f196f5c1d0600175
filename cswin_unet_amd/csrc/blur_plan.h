// Tile plan of the Gaussian blur (blur.hip), host only: plain C++, no HIP.  blur.hip launches what bl_plan returns;
// tools/blur_plan_check.cpp prints it for (H, W, r, vec) lines, which is how tests/test_blur_host.py holds the Python
// transcription of tests/blur_cases.py to this file.
#pragma once

constexpr int BL_MAX_DIM = 2048;           // per dimension (and slices per call)
constexpr int BL_MAX_RADIUS = 32;          // sigma <= 8.1 at truncate = 4
constexpr int BL_LDS_ELEMS = 16384;        // floats = 64 KiB, the dynamic LDS a kernel gets without opt-in
constexpr int BL_MAX_TR = 32;
constexpr int BL_RB = 4;                   // outputs per thread and tap: TR is a multiple of it
constexpr int BL_BUDGETS[3] = {BL_LDS_ELEMS * 3 / 8, BL_LDS_ELEMS * 5 / 8, BL_LDS_ELEMS};      // 24, 40, 64 KiB

// Tile rows and chunk width for (W, r): (TR + 2r) CW + TR W floats of LDS.  The kernel waits on memory and on barriers more than
// it computes, so it is the number of resident workgroups that sets its speed: 24 KiB per workgroup (six on a CU) is where a
// 148 x 512 x 512 batch stops getting faster (DESIGN.md has the sweep; 64 KiB tiles take 1.7 times as long), and a wider
// or longer-tapped slice takes the next budget that holds a tile.  The chunk starts at the widest one the loads can fill
// (256 lanes x VEC, no wider than W needs) and is halved while the tile is shorter than 4r rows: the 2r halo rows are read
// again by the neighbouring tile, and a narrower stage leaves room for more rows.  At CW = 64 and the whole 64 KiB the largest
// case, W = 2048 with r = 32, has 5 rows, so a tile of BL_RB rows always exists.
// budget: index into BL_BUDGETS of the budget the plan was found in (what the launch does not need and the plan check prints).
struct BlurPlan { int TR, cw_log2, budget; };
inline BlurPlan bl_plan(int H, int W, int r, int vec) {
    for (int b = 0; b < 3; ++b) {
        const int budget = BL_BUDGETS[b];
        auto rows = [&](int cwl) { return (budget - 2 * r * (1 << cwl)) / ((1 << cwl) + W); };
        int cwl = vec == 2 ? 9 : 8;
        while (cwl > 6 && (1 << (cwl - 1)) >= W) --cwl;
        const int Hr = (H + BL_RB - 1) / BL_RB * BL_RB;                 // the whole slice in row groups
        while (cwl > 6 && rows(cwl) < 4 * r && rows(cwl) < Hr) --cwl;
        int TR = rows(cwl) / BL_RB * BL_RB;
        if (TR < BL_RB) continue;
        TR = TR > BL_MAX_TR ? BL_MAX_TR : TR;
        return {TR > Hr ? Hr : TR, cwl, b};
    }
    return {0, 0, -1};
}

// bytes of dynamic LDS of a plan's launch: mid [TR][W] and stage [TR + 2r][CW], float32
inline long bl_lds_bytes(const BlurPlan& p, int W, int r) {
    return ((long)p.TR * W + (long)(p.TR + 2 * r) * (1 << p.cw_log2)) * (long)sizeof(float);
}

inline bool bl_dim_ok(int n) { return n >= 1 && n <= BL_MAX_DIM; }
