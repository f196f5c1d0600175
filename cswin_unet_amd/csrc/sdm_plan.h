// Launch policy of the signed distance maps (sdm.hip), host only: plain C++, no HIP.  sdm.hip launches what sdm_plan returns;
// tools/sdm_plan_check.cpp prints it for (B, ncls, H, W) lines, which is how tests/test_sdm_plan_host.py checks it on the CPU.
#pragma once
#include <cstddef>

constexpr int SDM_MAX_DIM = 2047;          // H and W: a row distance and the NONE mark fit the 15 value bits of a g1 cell
constexpr int SDM_MIN_NCLS = 2;
constexpr int SDM_MAX_NCLS = 255;          // a class is a byte in the row pass, 255 marks "no class"
constexpr int SDM_LDS_BYTES = 65536;       // the dynamic LDS a kernel gets without opt-in
constexpr int SDM_ROW_WAVES = 4;           // rows per workgroup of the row pass: one wave each
constexpr int SDM_G1_NONE = 0x7FFF;        // value bits of a g1 cell whose row has no pixel of the other membership
constexpr int SDM_G1_MEMBER = 0x8000;      // bit 15 of a g1 cell: the pixel belongs to the class

inline bool sdm_dim_ok(int n) { return n >= 1 && n <= SDM_MAX_DIM; }
inline bool sdm_ncls_ok(int ncls) { return ncls >= SDM_MIN_NCLS && ncls <= SDM_MAX_NCLS; }

// Columns of a workgroup of the column pass, one per lane: the workgroup keeps the H x TX uint16 cells of its columns in LDS.
// The pass is a chain of dependent LDS reads per pixel, so it is the number of resident waves that sets its speed, not the
// width of its memory segments: TX halves where H doubles so that the image stays within 16 KiB -- eight workgroups on a CU,
// as many as its wave slots take -- down to 16 columns (32-byte segments of g1, 64-byte ones of phi), which at the tallest
// slice are 2047 * 16 * 2 = 65504 bytes.  (profiles/boundary_loss_notes.md has the measurement of both rules.)
constexpr int SDM_LDS_TARGET = 16384;
inline int sdm_tx(int H) { return H * 64 * 2 <= SDM_LDS_TARGET ? 64 : (H * 32 * 2 <= SDM_LDS_TARGET ? 32 : 16); }

// row_blocks workgroups of 256 threads, wave w of workgroup g owning row g * SDM_ROW_WAVES + w of the B * H rows;
// col_blocks = B * ncls * col_tiles workgroups of 256 threads, workgroup g owning columns [t * TX, t * TX + TX) of plane
// g / col_tiles, t = g % col_tiles; lds_bytes: the column pass's dynamic LDS.  ok = 0: nothing may be launched.
struct SdmPlan { int ok, TX, col_tiles; long row_blocks, col_blocks, lds_bytes; };
inline SdmPlan sdm_plan(int B, int ncls, int H, int W) {
    SdmPlan p = {0, 0, 0, 0, 0, 0};
    if (B < 1 || !sdm_ncls_ok(ncls) || !sdm_dim_ok(H) || !sdm_dim_ok(W)) return p;
    p.TX = sdm_tx(H);
    p.col_tiles = (W + p.TX - 1) / p.TX;
    p.row_blocks = ((long)B * H + SDM_ROW_WAVES - 1) / SDM_ROW_WAVES;
    p.col_blocks = (long)B * ncls * p.col_tiles;
    p.lds_bytes = (long)H * p.TX * 2;
    p.ok = p.row_blocks <= 0x7FFFFFFFL && p.col_blocks <= 0x7FFFFFFFL && p.lds_bytes <= SDM_LDS_BYTES;
    return p;
}

// workspace: the per-(b, c) member counts (uint32, padded to 256 bytes), then g1 (uint16, B * ncls * H * W cells), the whole
// rounded up to 16 bytes
inline size_t sdm_counts_bytes(int B, int ncls) { return ((size_t)B * ncls * 4 + 255) / 256 * 256; }
inline size_t sdm_workspace_bytes(int B, int ncls, int H, int W) {
    return (sdm_counts_bytes(B, ncls) + (size_t)B * ncls * H * W * 2 + 15) / 16 * 16;
}
