// Launch policy of the attention kernels (attn.hip), host only: plain C++17, no HIP.  Every function is pure in its arguments and
// takes the CswinTuning it consults.  attn.hip checks its pointers, asks this header and launches what the records say; nothing
// beside it decides a window geometry, an instantiation, a query split, a grid, an LDS size or a workspace offset, and the kernels
// size their LDS regions from the same constexpr functions the launches are sized by.  tools/attn_plan_check.cpp prints the
// records, which is how tests/test_attn_plan_host.py holds the Python transcription of tests/test_gpu_attn_shapes.py to this file.
#pragma once
#include <stddef.h>

#include "tuning.h"

namespace ap {

constexpr int HD = 32;              // head dim the tiles are padded to (64/2 = 128/4 = 256/8 = 512/16)
constexpr int LDT = HD + 4;         // LDS row stride of the [token][d] images
constexpr int TILE = 16;            // tokens of an MFMA tile: a window of N tokens has nt = ceil(N / TILE) of them
constexpr int LW_SUB = 4;           // two-pass backward: token slices (= slab rows) per window of lepe_wgrad_kernel
constexpr int BLK = 64;             // two-pass backward: tokens per block
constexpr int LEPE_FLOATS = 10 * HD;            // [10][HD]: 9 LePE taps + bias of a head's channels -- the LDS patch, and a slab row
constexpr size_t LDS_PLAIN = 64 * 1024;         // dynamic LDS a kernel may ask for without the opt-in
constexpr int MAX_BRANCH = 2;

// The instantiated tile classes: a window of nt tiles runs the smallest class >= nt.  Up to ONE_WG_NT a workgroup has one wave
// per tile (attn_fwd3_kernel, attn_bwd3_kernel); above it the forward is attn_fwd_kernel and the backward the two-pass path.
constexpr int NT_CLASSES[] = {4, 6, 7, 9, 12, 15, 18};
constexpr int N_CLASSES = sizeof(NT_CLASSES) / sizeof(NT_CLASSES[0]);
constexpr int ONE_WG_NT = 7;
constexpr int MAX_NT = NT_CLASSES[N_CLASSES - 1];
constexpr int SPLIT_MIN_NT = 6;     // measured: the query split pays at N = 98, not at N = 49
constexpr int FWD_WAVES = 8;        // attn_fwd_kernel without the split: its waves walk the query tiles
static_assert(NT_CLASSES[2] == ONE_WG_NT && NT_CLASSES[3] > FWD_WAVES,
              "every attn_fwd_kernel class has more tiles than FWD_WAVES (so min(NT, 8) waves is 8) and every class splits by its "
              "own rule: a class of 8 or fewer tiles belongs to the one-wave-per-tile kernels");
static_assert((MAX_NT + 1) / 2 * 64 <= 1024 && ONE_WG_NT * 64 <= 1024, "threads per workgroup");

constexpr int nt_class(int nt) {
    for (int i = 0; i < N_CLASSES; ++i)
        if (nt <= NT_CLASSES[i]) return NT_CLASSES[i];
    return 0;
}

// ------------------------------------------------------------------------------------
// geometry: the windows of each branch and the units (branch, window, head) of the call
// ------------------------------------------------------------------------------------
enum class Refusal { none, bad_arguments, head_dim, error_mode, divisibility, index_range, window_sizes, window_tokens };
inline const char* refusal_name(Refusal r) {
    static const char* const names[] = {"none", "bad_arguments", "head_dim", "error_mode", "divisibility", "index_range", "window_sizes",
                                        "window_tokens"};
    return names[(int)r];
}

struct Branch {
    int c0;          // first channel of this branch inside C
    int heads;       // heads of this branch
    int head0;       // global index of its first head (for the lse layout)
    int H_sp, W_sp, nW, nWin;
    long units;      // B * nWin * heads
    int wg_begin;    // first workgroup of this branch
};
struct Geometry {
    Refusal refusal;
    int at;          // a refusal: the branch it is about (its H_sp, W_sp, units as far as they were computed)
    int hd;          // real head dim (8, 16, 24 or 32); refusal head_dim: the one refused
    int heads_total, N, nt, nwg;
    bool thin;       // a branch has stripes one token wide (the kernels' own br.H_sp == 1 || br.W_sp == 1)
    Branch br[MAX_BRANCH];
};

// idx: -1 the whole map, 0 vertical stripes `split` wide, 1 horizontal ones.  A branch works on C / nbranch channels.
inline Geometry geometry(int B, int reso, int C, int nbranch, const int* heads, const int* idx, int split) {
    Geometry g = {};
    auto refuse = [&](Refusal r, int i) { g.refusal = r; g.at = i; return g; };
    if (!(B > 0 && reso > 0 && C > 0 && (nbranch == 1 || nbranch == 2))) return refuse(Refusal::bad_arguments, 0);
    const int Cb = C / nbranch;
    for (int i = 0; i < nbranch; ++i) {
        const int hd = heads[i] > 0 ? Cb / heads[i] : 0;
        if (!(heads[i] > 0 && Cb == heads[i] * hd && hd >= 8 && hd <= HD && hd % 8 == 0 && (i == 0 || hd == g.hd))) {
            g.hd = hd;
            return refuse(Refusal::head_dim, i);
        }
        g.hd = hd;
        Branch& br = g.br[i];
        if (idx[i] == -1) { br.H_sp = reso; br.W_sp = reso; }
        else if (idx[i] == 0) { br.H_sp = reso; br.W_sp = split; }
        else if (idx[i] == 1) { br.H_sp = split; br.W_sp = reso; }
        else return refuse(Refusal::error_mode, i);
        if (!(br.H_sp > 0 && br.W_sp > 0 && reso % br.H_sp == 0 && reso % br.W_sp == 0)) return refuse(Refusal::divisibility, i);
        br.c0 = i * Cb;
        br.heads = heads[i];
        br.head0 = g.heads_total;
        br.nW = reso / br.W_sp;
        br.nWin = (reso / br.H_sp) * (reso / br.W_sp);
        br.units = (long)B * br.nWin * heads[i];
        br.wg_begin = g.nwg;
        // the kernels' index arithmetic divides by multiplication (fdiv, common.h): exact for n < 2^20, d < 2^12
        if (!(br.units < (1 << 20) && br.H_sp * br.W_sp < (1 << 12) && br.nWin < (1 << 12) && heads[i] < (1 << 12)))
            return refuse(Refusal::index_range, i);
        g.nwg += (int)br.units;
        g.heads_total += heads[i];
        if (i == 0) g.N = br.H_sp * br.W_sp;
        if (g.N != br.H_sp * br.W_sp) return refuse(Refusal::window_sizes, i);
        g.thin = g.thin || br.H_sp == 1 || br.W_sp == 1;
    }
    g.nt = (g.N + TILE - 1) / TILE;
    return g;
}

// ------------------------------------------------------------------------------------
// LDS footprints, in floats: the launches are sized by them and the kernels carve by them
// ------------------------------------------------------------------------------------
// both forward kernels: K and V images [16 NT][LDT] and the LePE patch
constexpr int fwd_lds_floats(int NT) { return 2 * TILE * NT * LDT + LEPE_FLOATS; }
constexpr size_t fwd_lds_bytes(int NT) { return (size_t)fwd_lds_floats(NT) * sizeof(float); }
constexpr bool fwd_opt_in(int NT) { return fwd_lds_bytes(NT) > LDS_PLAIN; }

// fused backward: smallest row stride >= N of the dS image with stride = 4 (mod 8): 16-B aligned rows, and the four row groups
// of a dS column write land in distinct banks
constexpr int ds_stride_for(int N) {
    const int s = (N + 3) / 4 * 4;
    return s % 8 == 4 ? s : s + 4;
}
// fused backward: the V image [16 NT + 1][LDT] (last row zero), later dS [N][S] + 16 NT finite floats behind it
constexpr int vs_floats_for(int NT, int N, int S) {
    const int NP = TILE * NT;
    const int a = N * S + NP, b = (NP + 1) * LDT;
    return ((a > b ? a : b) + 3) / 4 * 4;
}
constexpr int bwd3_grad_floats(int NT) { return (9 + NT) * HD; }       // Gl [9 + NT][HD]: the unit's LePE weight gradient, per-wave bias gradients
// QK [NP][LDT] | Ds [NP][LDT] | VS | lse, delta [NP] each | Wl | Gl
constexpr int bwd3_lds_floats(int NT, int vs_floats) { return 2 * TILE * NT * LDT + vs_floats + 2 * TILE * NT + LEPE_FLOATS + bwd3_grad_floats(NT); }
// the largest footprint an NT can ask for (N = 16 NT tokens): what the opt-in reserves, once per instantiation
constexpr size_t bwd3_lds_bytes_max(int NT) {
    return (size_t)bwd3_lds_floats(NT, vs_floats_for(NT, TILE * NT, ds_stride_for(TILE * NT))) * sizeof(float);
}

// ------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------
enum class Family { fwd3, fwd };
constexpr Family fwd_family(int NT) { return NT <= ONE_WG_NT ? Family::fwd3 : Family::fwd; }
constexpr bool fwd_may_split(int NT) { return NT >= SPLIT_MIN_NT; }
// waves of a forward workgroup.  QS = 2: the query tiles of a unit over two workgroups, one tile per wave
constexpr int fwd_waves(int NT, int QS) { return QS == 2 ? (NT + 1) / 2 : fwd_family(NT) == Family::fwd3 ? NT : FWD_WAVES; }

struct FwdPlan {
    Refusal refusal;        // window_tokens: more tiles than the largest class
    Family family;
    int NT, QS, threads, grid;
    size_t lds;             // dynamic LDS bytes
    bool opt_in;            // the instantiation asks for more than LDS_PLAIN
};

inline FwdPlan fwd_plan(const CswinTuning& t, const Geometry& g) {
    FwdPlan f = {};
    f.NT = nt_class(g.nt);
    if (!f.NT) { f.refusal = Refusal::window_tokens; return f; }
    f.family = fwd_family(f.NT);
    // Few units relative to the 256 CUs: split the query tiles over two workgroups per unit (see the kernels).  One wave per tile
    // (stage 3: 384 units of 7 query tiles): unless the units fill the CUs evenly or four times over.  Large windows (384 x 384
    // inputs, 128 units at batch 8) otherwise leave half the chip idle and give a wave 2 - 3 query tiles.
    const bool heuristic = f.family == Family::fwd3 ? g.nwg < 1024 && g.nwg % 256 != 0 : g.nwg <= 256;
    const int force = t.attn_fwd_qsplit;                                                                          // tuning aid: 1 or 2
    f.QS = fwd_may_split(f.NT) && (force ? force == 2 : heuristic) ? 2 : 1;
    f.threads = 64 * fwd_waves(f.NT, f.QS);
    f.grid = f.QS * g.nwg;
    f.lds = fwd_lds_bytes(f.NT);
    f.opt_in = fwd_opt_in(f.NT);
    return f;
}

// ------------------------------------------------------------------------------------
// backward and its workspace
// ------------------------------------------------------------------------------------
enum class BwdPath { bwd3, two_pass };
struct BwdPlan {
    BwdPath path;
    int NT;                 // bwd3: the instantiation
    int nblk;               // two_pass: blocks of BLK tokens per window
    int slab_rows;          // LePE gradient slab rows per window
    int ds_stride;          // LDS row stride of the dS image
    int vs_floats;          // bwd3: floats of the V / dS region
    int threads;
    size_t lds;             // bwd3: dynamic LDS bytes
    size_t lds_reserved;    // bwd3: what the opt-in reserves for the instantiation when lds > LDS_PLAIN (0: no opt-in)
    unsigned grid[4];       // bwd3: [0]; two_pass: attn_delta, attn_bwd_kv, attn_bwd_q, lepe_wgrad
    // workspace, in floats: per branch the LePE partial slabs [units][slab_rows][LEPE_FLOATS], then delta (B, heads_total, L)
    // (which only the two-pass path uses)
    size_t slab_off[MAX_BRANCH], delta_off, ws_bytes;
};

inline BwdPlan bwd_plan(const CswinTuning& t, const Geometry& g, int B, int reso, int nbranch) {
    BwdPlan b = {};
    // windows of more than 112 tokens (384 x 384: N = 144, 288) take the two passes, 64 x 64 at a time
    b.path = g.nt > ONE_WG_NT || t.attn_bwd_two_pass ? BwdPath::two_pass : BwdPath::bwd3;                         // tuning aid
    b.ds_stride = ds_stride_for(g.N);
    const size_t items = (size_t)B * g.heads_total * reso * reso;
    if (b.path == BwdPath::two_pass) {
        b.nblk = (g.N + BLK - 1) / BLK;
        b.slab_rows = LW_SUB;
        b.threads = 256;
        b.grid[0] = (unsigned)((items * 8 + 255) / 256);
        b.grid[1] = b.grid[2] = (unsigned)(g.nwg * b.nblk);
        b.grid[3] = (unsigned)(g.nwg * LW_SUB);
    } else {
        b.NT = nt_class(g.nt);
        b.slab_rows = 1;
        b.vs_floats = vs_floats_for(b.NT, g.N, b.ds_stride);
        b.threads = 64 * b.NT;
        b.lds = (size_t)bwd3_lds_floats(b.NT, b.vs_floats) * sizeof(float);
        b.lds_reserved = b.lds > LDS_PLAIN ? bwd3_lds_bytes_max(b.NT) : 0;
        b.grid[0] = (unsigned)g.nwg;
    }
    for (int i = 0; i < nbranch; ++i) b.slab_off[i] = (size_t)g.br[i].wg_begin * LEPE_FLOATS * b.slab_rows;
    b.delta_off = (size_t)g.nwg * LEPE_FLOATS * b.slab_rows;
    b.ws_bytes = (b.delta_off + items) * sizeof(float);
    return b;
}

}  // namespace ap
