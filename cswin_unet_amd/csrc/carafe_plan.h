// Launch policy of the CARAFE kernels (carafe.hip), host only: plain C++17, no HIP.  Every function is pure in its arguments; the
// carafe_generic tuning flag arrives as one.  carafe.hip checks its pointers, asks this header and launches what the records say;
// nothing beside it decides a refusal, a lane split, a grid, a backward route or a workspace size, and the kernels size their LDS
// arrays from the same constexpr functions.  tools/carafe_plan_check.cpp prints the records, which is how
// tests/test_carafe_plan_host.py holds the Python transcription of tests/test_gpu_carafe_shapes.py to this file.
#pragma once
#include <stddef.h>

#ifdef __HIPCC__
#define CARAFE_HD __host__ __device__
#else
#define CARAFE_HD
#endif

namespace cp {

constexpr int THREADS = 256;            // per workgroup of every kernel but the fused one
constexpr int MAX_LPR = 64;             // lanes per item at most: the shuffles of bwd_e stay inside a wave
constexpr int GRID_CLAMP = 8192;        // workgroups of a grid-stride kernel
constexpr int COLSUM_CLAMP = 512;       // workgroups of colsum_partial_kernel
constexpr int COLSUM_ROWS = 64;         // rows a row group of colsum_partial_kernel is sized for
constexpr int BIAS_IN_E_CZ = 512;       // up to here the column sums of dout ride along in bwd_e
constexpr int E_CHUNKS = 2;             // 16-B chunks per lane bwd_e has column-sum accumulators for
constexpr size_t LDS_PLAIN = 64 * 1024; // static LDS a kernel gets without the opt-in

// the fused backward (the model's head): one workgroup per F_TILE x F_TILE low-resolution pixels and a one-pixel halo
constexpr int F_S = 4, F_CZ = 16;
constexpr int F_TILE = 8;
constexpr int F_HALO = F_TILE + 2;
constexpr int F_NP = F_HALO * F_HALO;   // 100 pixels whose G is needed
constexpr int F_WAVES = 8;              // two workgroups of 64 KB LDS share a CU
constexpr int F_THREADS = 64 * F_WAVES;

constexpr int ceil_div(long a, long b) { return (int)((a + b - 1) / b); }

// lanes per (pixel, sub-pixel) item: the largest power of two <= min(Cz / 4, MAX_LPR); they stride over the Cz / 4 chunks
CARAFE_HD constexpr int lpr(int Cz) {
    int l = 1;
    while (2 * l <= Cz / 4 && 2 * l <= MAX_LPR) l *= 2;
    return l;
}
constexpr int groups(int Cz) { return THREADS / lpr(Cz); }                      // items a workgroup takes per trip
constexpr int chunks_per_lane(int Cz) { return ceil_div(Cz / 4, lpr(Cz)); }     // 16-B chunks of the busiest lane
constexpr int ppb(int S) { return THREADS / (S * S); }                          // plane forward: low-resolution pixels per workgroup

// ------------------------------------------------------------------------------------
// LDS, in floats: the kernels declare their arrays by these
// ------------------------------------------------------------------------------------
// bwd_e stages its column sums as [chunk][group][4 * lpr]: groups * 4 * lpr = 4 * THREADS floats per chunk, whatever Cz
constexpr int e_stage_chunk_floats() { return 4 * THREADS; }
constexpr int e_stage_floats() { return E_CHUNKS * e_stage_chunk_floats(); }
constexpr int fused_gs_floats() { return F_NP * 9 * F_CZ; }                     // G [pixel][tap][channel]   57.6 KB
constexpr int fused_zt_floats() { return F_NP * F_CZ; }                         // z of the tile + halo       6.4 KB
constexpr int fused_bred_floats() { return F_WAVES * F_CZ; }
constexpr size_t fused_lds_bytes() { return (size_t)(fused_gs_floats() + fused_zt_floats() + fused_bred_floats()) * sizeof(float); }

constexpr int max_chunks_up_to(int Cz) {
    int m = 0;
    for (int c = 4; c <= Cz; c += 4) m = chunks_per_lane(c) > m ? chunks_per_lane(c) : m;
    return m;
}
static_assert(max_chunks_up_to(BIAS_IN_E_CZ) <= E_CHUNKS && chunks_per_lane(BIAS_IN_E_CZ + 4) > E_CHUNKS,
              "every width of the bias-in-e route fits bwd_e's accumulators, and the next one does not");
static_assert(groups(4) * 4 * lpr(4) == e_stage_chunk_floats() && groups(BIAS_IN_E_CZ) * 4 * lpr(BIAS_IN_E_CZ) == e_stage_chunk_floats(),
              "a chunk of the staging holds groups * 4 * lpr floats");
static_assert(fused_lds_bytes() <= LDS_PLAIN && (size_t)e_stage_floats() * sizeof(float) <= LDS_PLAIN, "static LDS, no opt-in");
static_assert(F_THREADS <= 1024 && F_THREADS >= 4 * F_TILE * F_TILE, "the dz gather has four lanes per interior pixel");

// ------------------------------------------------------------------------------------
// what the entry points refuse before anything is launched
// ------------------------------------------------------------------------------------
enum class Refusal { none, dimension, scale, channels, classes, not_fused };
inline const char* refusal_name(Refusal r) {
    static const char* const names[] = {"none", "dimension", "scale", "channels", "classes", "not_fused"};
    return names[(int)r];
}

inline Refusal refusal(int B, int H, int W, int Cz, int S) {
    if (B <= 0 || H <= 0 || W <= 0) return Refusal::dimension;
    if (S != 2 && S != 4) return Refusal::scale;
    if (Cz < 4 || Cz % 4 != 0) return Refusal::channels;
    return Refusal::none;
}
// the plane forward: the first C of the Cz channels
inline Refusal planes_refusal(int B, int H, int W, int Cz, int C, int S) {
    const Refusal r = refusal(B, H, W, Cz, S);
    return r != Refusal::none ? r : C <= 0 || C > Cz ? Refusal::classes : Refusal::none;
}
// the shapes the fused kernel is written for: whole tiles of the head's S and Cz
inline bool fused_shape(int H, int W, int Cz, int S) { return S == F_S && Cz == F_CZ && H % F_TILE == 0 && W % F_TILE == 0; }
// the plane backward exists as the fused kernel alone
inline Refusal bwd_planes_refusal(int B, int H, int W, int Cz, int C, int S) {
    if (B <= 0 || H <= 0 || W <= 0) return Refusal::dimension;
    if (C <= 0 || C > Cz) return Refusal::classes;
    return fused_shape(H, W, Cz, S) ? Refusal::none : Refusal::not_fused;
}

// ------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------
inline int grid_for(long items, int per_group) {
    const long b = (items + per_group - 1) / per_group;
    return (int)(b < 1 ? 1 : (b > GRID_CLAMP ? GRID_CLAMP : b));
}

struct FwdTokens { int lpr, groups, grid; };            // a group of lpr lanes per (pixel, sub-pixel)
inline FwdTokens fwd_tokens(int B, int H, int W, int Cz, int S) {
    return {lpr(Cz), groups(Cz), grid_for((long)B * H * W * S * S, groups(Cz))};
}

struct FwdPlanes { int ppb, grid; };                    // a lane per output pixel
inline FwdPlanes fwd_planes(int B, int H, int W, int S) { return {ppb(S), grid_for((long)B * H * W, ppb(S))}; }

// ------------------------------------------------------------------------------------
// backward and its workspace
// ------------------------------------------------------------------------------------
// Where dbias comes from: the fused kernel's per-tile sums, bwd_e's per-workgroup sums, or a pass of colsum_partial_kernel over
// dout.  Without a dbias to compute the generic routes launch bwd_e and bwd_z alone.
enum class Route { fused, bias_in_e, colsum };
inline const char* route_name(Route r) {
    static const char* const names[] = {"fused", "bias_in_e", "colsum"};
    return names[(int)r];
}

// colsum_partial_kernel over a (rows, C) matrix: min(C, THREADS) lanes across the columns, the row groups beside them
struct Colsum { int lanes, rgroups, grid; };
inline Colsum colsum_plan(long rows, int C) {
    Colsum c = {};
    c.lanes = C < THREADS ? C : THREADS;
    c.rgroups = THREADS / c.lanes;
    const long b = (rows + c.rgroups * COLSUM_ROWS - 1) / (c.rgroups * COLSUM_ROWS);
    c.grid = (int)(b < 1 ? 1 : (b > COLSUM_CLAMP ? COLSUM_CLAMP : b));
    return c;
}

struct BwdPlan {
    Route route;
    int lpr, groups, chunks;                        // chunks: 16-B chunks of the busiest lane of an item
    int grid_e, grid_z;                             // bias_in_e, colsum
    Colsum colsum;                                  // colsum
    int tiles_x, tiles_y, grid_fused;               // fused
    int part_rows;                                  // rows of the [part_rows][Cz] partial sums the reduce job reads
};

inline BwdPlan bwd_plan(bool generic_only, int B, int H, int W, int Cz, int S) {
    BwdPlan p = {};
    p.lpr = lpr(Cz);
    p.groups = groups(Cz);
    p.chunks = chunks_per_lane(Cz);
    if (fused_shape(H, W, Cz, S) && !generic_only) {
        p.route = Route::fused;
        p.tiles_x = W / F_TILE;
        p.tiles_y = H / F_TILE;
        p.part_rows = p.grid_fused = B * p.tiles_x * p.tiles_y;
        return p;
    }
    const long items = (long)B * H * W * S * S;
    p.grid_e = grid_for(items, p.groups);
    p.grid_z = grid_for((long)B * H * W, p.groups);
    if (Cz <= BIAS_IN_E_CZ) {
        p.route = Route::bias_in_e;
        p.part_rows = p.grid_e;
        return p;
    }
    p.route = Route::colsum;
    p.colsum = colsum_plan(items, Cz);
    p.part_rows = p.colsum.grid;
    return p;
}

// The workspace query does not see the tuning flag: the larger of what the two settings launch.
inline size_t bwd_workspace(int B, int H, int W, int Cz, int S) {
    const size_t a = (size_t)bwd_plan(false, B, H, W, Cz, S).part_rows, b = (size_t)bwd_plan(true, B, H, W, Cz, S).part_rows;
    return (a > b ? a : b) * Cz * sizeof(float);
}

}  // namespace cp
