// Launch policy of the GEMM family (gemm.hip, gemm16.hip, wgrad16.hip), host only: plain C++17, no HIP.  Every function is pure
// in its arguments and takes the CswinTuning it consults, so the library passes cswin_tuning() and a host program may pass that or
// its own.  The three .hip files check their arguments, ask this header and launch what the record says; nothing beside it decides a
// tile, a width, a split or a route.  tools/gemm_plan_check.cpp prints the records, which is how tests/test_gemm_plan_host.py
// holds the Python transcription of tests/test_gpu_gemm_shapes.py to this file.
#pragma once
#include <stddef.h>

#include "tuning.h"

namespace gp {

constexpr int BKMAX = 64;           // largest reduction tile (split sizes are multiples of it)
constexpr int WGRAD_BATCH = 4;      // problems of one weight-gradient batch launch
constexpr int MAX_SPLIT_WGS = 1024; // the largest per-problem workgroup target of any split policy (the workspace query covers it)
// wgrad16.hip's geometry as the policy needs it (the file asserts that they are its own)
constexpr int W16_T = 128;          // tile edge (n and k)
constexpr int W16_MS = 32;          // m rows per step
constexpr int W16_SC_SAMPLES = 64;  // DropPath factors of the samples a workgroup's rows touch
constexpr int G16_T = 64;           // gemm16.hip: tile edge and reduction step

inline int ceil_div(long a, long b) { return (int)((a + b - 1) / b); }

// floats between the split-M slabs of a weight gradient dw[N,K]: slab s = [dw partial (N*K) | dbias partial (N)] (gemm.hip's WgradSlabs)
inline long slab_stride(int N, int K) { return (long)N * K + N; }

// Wave groups (KW) for a launch of `blocks` workgroups whose reduction is r_len long: with fewer than ~2 workgroups per CU and
// a long reduction, split the k-range of each tile over 2 or 4 wave groups so every SIMD still has independent MFMA chains.
inline int k_groups(long blocks, int r_len) {
    if (blocks < 320 && r_len >= 512) return 4;
    if (blocks < 640 && r_len >= 256) return 2;
    return 1;
}

// a reduction of R in one split: r_per_split is a whole number of k-tiles
inline int one_split(int R) { return ceil_div(R, BKMAX) * BKMAX; }

// ------------------------------------------------------------------------------------
// the record every question below is answered with
// ------------------------------------------------------------------------------------
enum class Kernel {
    tiled,     // gemm_kernel / gemm_mapped_kernel at the record's tile, widths and split
    gemm16,    // gemm16_kernel: tile rows bm, `stages` steps in flight, last step of last_step reduction values
    wgrad16,   // wgrad16_kernel: a problem of its batch, dma = the LDS-DMA tile
    batch,     // a problem of gemm_wgrad_batch_kernel / gemm_block_tail_kernel (and their masked forms)
    tail       // the data gradient in gemm_block_tail_kernel's grid
};
struct Plan {
    Kernel kernel;
    int bm, bn, bk, kw;      // tile, k-tile, wave groups
    int vec, store;          // loader and epilogue width: 4 (16-B accesses) or 1
    int splits, rows, last;  // slices of the reduction, rows per slice, rows of the last one
    bool wgrad;              // a weight gradient (its slices are slabs of a workspace)
    int stages, last_step;   // gemm16
    bool dma;                // wgrad16
};

// ------------------------------------------------------------------------------------
// weight-gradient splits and the workspace
// ------------------------------------------------------------------------------------
struct Split { int splits, rows; };

// split count for the M-reduction of a weight gradient: enough workgroups to fill the chip
inline Split choose_split(const CswinTuning& t, int M, int out_rows, int out_cols, int target_override = 0) {
    // Every workgroup is resident at once and the kernel ends with the most loaded CU, so aim at a workgroup count
    // that is a whole multiple of the 256 CUs (3 per CU): slices need not be multiples of the k-tile (the loaders mask
    // the ragged last tile), only of 8.
    const int target = target_override > 0 ? target_override : t.gemm_split_wgs;                               // tuning aid
    long tiles = (long)ceil_div(out_rows, 64) * ceil_div(out_cols, 64);
    int s = (int)(target / tiles);
    if (s < 1) s = 1;
    int max_s = ceil_div(M, 2 * BKMAX);
    if (s > max_s) s = max_s;
    if (s < 1) s = 1;
    int rps = ceil_div(ceil_div(M, s), 8) * 8;
    return {ceil_div(M, rps), rps};
}

// bytes of the workspace of a split-M weight gradient dw[N,K] (+ dbias[N]): covers the stand-alone split policy and the batched
// one (up to MAX_SPLIT_WGS workgroups for a single problem)
inline size_t wgrad_workspace_bytes(const CswinTuning& t, int M, int N, int K) {
    const int s0 = choose_split(t, M, N, K).splits, s1 = choose_split(t, M, N, K, MAX_SPLIT_WGS).splits;
    return (size_t)(s0 > s1 ? s0 : s1) * slab_stride(N, K) * sizeof(float);
}

// ------------------------------------------------------------------------------------
// the tiled family: tile, k-tile and wave groups
// ------------------------------------------------------------------------------------
struct Tile { int bm, bn, bk, kw; };

// tile choice (measured on MI355X, tools/gemm_bench.py): the largest tile that still yields >= ~1.5 workgroups per CU.
// M x N outputs, a reduction of R in `splits` slices of r_per_split; wgrad: both operands row-contiguous (a weight gradient).
inline Tile choose_tile(const CswinTuning& t, int M, int N, int R, int splits, int r_per_split, bool wgrad, int precision) {
    auto blocks = [&](int bm, int bn) { return (long)ceil_div(M, bm) * ceil_div(N, bn) * splits; };
    // Tile choice.  64 x 64 is the most efficient tile (profiles/round1_gemm_bench.txt), but every workgroup of these
    // launches is resident at once and the kernel ends with the most loaded CU: with t tiles the critical CU does
    // ceil(t / 256) of them.  When that is a poor multiple (stage 3: 296 tiles -> 2 where 1.16 would do) a smaller tile
    // shortens the critical path although it is a little less efficient per flop (penalties measured with gemm_bench).
    // measured (profiles/round1_gemm_tiles.txt): a 64 x 32 tile costs ~1.2x per flop, so it only pays where it cuts the
    // critical CU's share by more than that (296 -> 592 tiles: 2 -> 1.5 units); 32 x 32 single-wave tiles never paid.
    auto cost = [&](int bm, int bn, double pen) { return (double)((blocks(bm, bn) + 255) / 256) * bm * bn * pen; };
    int tile = 1;
    if (splits == 1 && cost(64, 32, t.gemm_pen2) < cost(64, 64, 1.0)) tile = 2;
    if (t.gemm_tile) tile = t.gemm_tile;                                         // tuning aid: 1 = 64x64, 2 = 64x32
    const int r_len = r_per_split < R ? r_per_split : R;
    if (precision == 1) {
        // bf16 operands: 16x fewer MFMA cycles per tile, the kernel is bound by staging and barriers: one k-tile of 64,
        // and two wave groups only where a long reduction meets few workgroups
        return {64, 64, 64, k_groups(blocks(64, 64), r_len) >= 2 || (wgrad && r_len >= 256) ? 2 : 1};
    }
    if (tile == 2) {
        if (k_groups(blocks(64, 32), r_len) >= 2) return {64, 32, 64, 2};
        return {64, 32, 32, 1};
    }
    int kw = k_groups(blocks(64, 64), r_len);
    if (wgrad && r_len >= 256 && kw < 2) kw = 2;               // weight gradients: measured 5-8 % faster
    if (t.gemm_kw) kw = t.gemm_kw;                             // tuning aid
    if (kw == 4) return {64, 64, 64, 4};
    if (kw == 2) return {64, 64, 64, 2};
    return {64, 64, 32, 1};
}

// a launch of the tiled family.  vec: 16-B loads are legal (alignment, sizes multiples of 4); store: 16-B epilogue accesses are
inline Plan tiled_plan(const CswinTuning& t, int M, int N, int R, int splits, int r_per_split, bool wgrad, int precision, bool vec,
                       bool store) {
    const Tile c = choose_tile(t, M, N, R, splits, r_per_split, wgrad, precision);
    Plan p = {};
    p.kernel = Kernel::tiled;
    p.bm = c.bm; p.bn = c.bn; p.bk = c.bk; p.kw = c.kw;
    p.vec = vec ? 4 : 1; p.store = store ? 4 : 1;
    p.splits = splits; p.rows = r_per_split; p.last = R - (splits - 1) * r_per_split;
    p.wgrad = wgrad;
    return p;
}

// wave groups of the stride-2 convolution's data-gradient batch (gemm_conv_s2_dgrad_batch_kernel): `blocks` workgroups over the
// four parity classes, the longest reduction rmax; the bf16 loop has its one form
inline int s2_dgrad_kw(int blocks, int rmax, int precision) { return precision == 1 ? 2 : k_groups(blocks, rmax); }

// ------------------------------------------------------------------------------------
// gemm16.hip: both operands stored as bf16
// ------------------------------------------------------------------------------------
// What the LDS-DMA kernel covers: reduction lengths n x 64 (+ 32), output columns in whole 16-B bf16 chunks, 16-B aligned
// operands and the 16-B epilogue (bf16-stored outputs / auxiliaries need that path anyway).
inline bool gemm16_accepts(const CswinTuning& t, int M, int NO, int R, bool loads_aligned, bool store) {
    if (!t.gemm16_on) return false;                                                                           // tuning aid
    return (R % G16_T == 0 || R % G16_T == 32) && R >= G16_T && NO % 8 == 0 && M >= 1 && loads_aligned && store;
}
inline Plan gemm16_plan(const CswinTuning& t, int M, int NO, int R) {
    const int nblk = ceil_div(M, G16_T) * ceil_div(NO, G16_T), nsteps = ceil_div(R, G16_T);
    const bool tm128 = t.gemm16_tm == 128 || (t.gemm16_tm == 0 && nblk > 768);                                // tuning aid: 64 / 128
    int S = nsteps >= 3 ? 3 : 2;          // 48 KB: three workgroups per CU (measured against 2 and 4 stages: profiles/round2_notes.md)
    if (t.gemm16_stages >= 2 && t.gemm16_stages <= 4) S = t.gemm16_stages;                                    // tuning aid: 2 .. 4
    Plan p = {};
    p.kernel = Kernel::gemm16;
    p.bm = tm128 ? 2 * G16_T : G16_T;     // 128 x 64 tiles: three slots of 24 KB, two workgroups per CU
    p.bn = G16_T; p.bk = G16_T; p.kw = 1;
    p.vec = p.store = 4;
    p.splits = 1; p.rows = one_split(R); p.last = R;
    p.stages = tm128 ? 3 : S;
    p.last_step = R % G16_T ? R % G16_T : G16_T;
    return p;
}

// ------------------------------------------------------------------------------------
// the Linear entry points
// ------------------------------------------------------------------------------------
// loads_aligned: every input matrix of the call starts 16-B aligned; outs_aligned: every output and auxiliary operand the call's
// form has (y, y_act, bias, residual; dx, dx2, gelu_pre, add; the workspace) does.

// cswin_linear_fwd: y[M,N] = [x | x2][M,K] @ w[N,K]^T.  k_split: the seam of a concat input (0: a plain one)
inline Plan linear_fwd_plan(const CswinTuning& t, int M, int N, int K, int k_split, int precision, int io_bf16, bool loads_aligned,
                            bool outs_aligned) {
    const bool vec = K % 4 == 0 && k_split % 4 == 0 && loads_aligned, store = N % 4 == 0 && outs_aligned;
    // both operands stored as bf16: LDS-DMA kernel (gemm16.hip)
    if (precision == 1 && (io_bf16 & 5) == 5 && !k_split && gemm16_accepts(t, M, N, K, loads_aligned, store)) return gemm16_plan(t, M, N, K);
    return tiled_plan(t, M, N, K, 1, one_split(K), false, precision, vec, store);
}

// cswin_linear_bwd_data: dx[M,K] = dy[M,N] @ w[N,K]: output rows = M, output cols = K, reduction = N.  k_split: the dx | dx2 seam
// of the split form (0: one output); add: the form with an add operand
inline Plan linear_dgrad_plan(const CswinTuning& t, int M, int N, int K, int k_split, bool add, int precision, int io_bf16,
                              bool loads_aligned, bool outs_aligned) {
    const bool vec = N % 4 == 0 && K % 4 == 0 && loads_aligned, store = K % 4 == 0 && k_split % 4 == 0 && outs_aligned;
    if (precision == 1 && !k_split && !add && (io_bf16 & 5) == 5 && gemm16_accepts(t, M, K, N, loads_aligned, store)) return gemm16_plan(t, M, K, N);
    return tiled_plan(t, M, K, N, 1, one_split(N), false, precision, vec, store);
}

// One weight gradient dw[N,K] = dy[M,N]^T @ [x | x2][M,K] through the tiled family: N x K outputs, the reduction M in slabs
inline Plan wgrad_tiled_plan(const CswinTuning& t, int M, int N, int K, int k_split, int precision, bool loads_aligned, bool ws_aligned) {
    const Split s = choose_split(t, M, N, K);
    const bool vec = N % 4 == 0 && K % 4 == 0 && k_split % 4 == 0 && loads_aligned;
    const bool store = K % 4 == 0 && slab_stride(N, K) % 4 == 0 && ws_aligned;
    return tiled_plan(t, N, K, M, s.splits, s.rows, true, precision, vec, store);
}

// what the batch kernels require of a problem: 16-B loads of both operands and 16-B stores to the slabs
inline bool wgrad_aligned(int N, int K, bool ptrs_aligned) { return N % 4 == 0 && K % 4 == 0 && ptrs_aligned; }

// ------------------------------------------------------------------------------------
// weight-gradient batches and the block tail
// ------------------------------------------------------------------------------------
struct WgradProblem {
    int M, N, K, io_bf16;
    bool loads_aligned, ws_aligned;   // dy and x; the workspace
    bool has_scale; int rows_per_sample;
    bool has_mask;
    size_t ws_bytes;
    bool aligned() const { return wgrad_aligned(N, K, loads_aligned && ws_aligned); }
};
// what may ride at the end of the batch's grid: a plain fp32 data gradient dx[M,K] = dy[M,N] @ w[N,K] and njobs pending reductions
struct TailRequest {
    bool dgrad; int M, N, K;
    bool loads_aligned, dx_aligned;   // dy and w; dx
    bool order;                       // the data gradient takes a sample order
    int njobs;
};
enum class BatchKernel {
    separate,      // not every problem is aligned: one launch per problem (Plan::kernel of each says which)
    wgrad16,       // wgrad16_kernel
    plain, masked, // gemm_wgrad_batch_kernel<precision>, gemm_wgrad_batch_masked_kernel
    tail, tail_masked, tail_order   // gemm_block_tail_kernel and its masked / skip forms
};
struct BatchRoute {
    BatchKernel kernel;
    bool dgrad_first, jobs_first;   // the data gradient / the pending reductions as launches of their own, in front of the batch
    bool jobs_ride;                 // the pending reductions ride in the batch's grid (tail kernels, wgrad16)
    Plan dgrad;                     // Kernel::tail: in the batch's grid
    Plan problem[WGRAD_BATCH];
};

// cswin_wgrad16_batch's LDS-DMA tile serves a problem of the wgrad16 route (16-B aligned operands, as the route has them) when both
// operands are stored as bf16, every slab is whole 32-row steps and a slab's samples fit the tile's table of factors
inline bool w16_dma(const CswinTuning& t, const WgradProblem& p, int rows_per_split) {
    if (!t.w16_dma) return false;                                                                             // tuning aid
    return (p.io_bf16 & 1) && (p.io_bf16 & 2) && p.M % W16_MS == 0 && rows_per_split % W16_MS == 0 && p.N % 8 == 0 && p.K % 8 == 0 &&
           (!p.has_scale || rows_per_split / p.rows_per_sample + 2 <= W16_SC_SAMPLES);
}

// The launch of n aligned problems: the shares of its workgroups and the kernel family.  wgrad16: the bf16
// route (precision 1, unless the tuning aid turns it off for problems stored as fp32).
inline void aligned_batch_plans(const CswinTuning& t, const WgradProblem* p, int n, bool wgrad16, Plan* out) {
    if (wgrad16) {
        // bf16 operands: 128 x 128 tiles, ~3 workgroups per CU over the whole batch (load-bound: see wgrad16.hip)
        // Workgroups are shared out in proportion to the work (rows x tiles), so that every workgroup of the launch walks the same
        // number of rows: with equal shares per problem the C x C problem's workgroups finished after 10 k cycles and the C x 4C
        // ones after 37 k (in-kernel stamps, tools/wgrad16_stamps.py), and the launch lasts as long as its slowest workgroup.
        double work_total = 0.0;
        for (int i = 0; i < n; ++i) work_total += (double)p[i].M * ceil_div(p[i].N, W16_T) * ceil_div(p[i].K, W16_T);
        for (int i = 0; i < n; ++i) {
            const int M = p[i].M, N = p[i].N, K = p[i].K;
            const int tiles = ceil_div(N, W16_T) * ceil_div(K, W16_T);
            // tuning aids (w16_even: 1 = equal share per problem)
            int s = t.w16_even ? (t.w16_wgs / n) / tiles : (int)(t.w16_wgs * ((double)M * tiles / work_total) / tiles + 0.5);
            const int cap = (int)(p[i].ws_bytes / (slab_stride(N, K) * (long)sizeof(float)));
            if (s > cap) s = cap;
            if (s > M / 64) s = M / 64;
            if (s < 1) s = 1;
            Plan& q = out[i];
            q = Plan{};
            q.kernel = Kernel::wgrad16;
            q.bm = q.bn = W16_T; q.bk = W16_MS; q.kw = 1;
            q.vec = q.store = 4;
            q.rows = ceil_div(ceil_div(M, s), W16_MS) * W16_MS;
            q.splits = ceil_div(M, q.rows);
            q.last = M - (q.splits - 1) * q.rows;
            q.wgrad = true;
            q.dma = w16_dma(t, p[i], q.rows);
        }
        return;
    }
    // the weight gradients' configuration: two k-groups of four waves (WgradTile), bf16 operands or not
    for (int i = 0; i < n; ++i) {
        const int M = p[i].M, N = p[i].N, K = p[i].K;
        // 1024 workgroups per launch, i.e. exactly 4 per CU, shared by the problems (measured with four problems: 192 / 256 /
        // 320 per problem -> 13.80 / 13.55 / 14.09 ms per step); a quarter of the slab traffic of four stand-alone launches
        const int batch_env = t.gemm_batch_wgs;                                                                   // tuning aid
        // Equal shares per problem (the C x C problem then has 294-row workgroups beside the 1176-row ones of the C x 4C problems).
        // Shares in proportion to the work (CSWIN_GEMM_BATCH_EVEN=0), which pays for the load-bound bf16 kernel above, measured
        // SLOWER here: 13.70 against 13.28 ms/step -- this kernel is matrix-pipe bound and the extra slabs cost more than the tail.
        const int total_wgs = batch_env > 0 ? (batch_env < MAX_SPLIT_WGS ? batch_env : MAX_SPLIT_WGS) * n : MAX_SPLIT_WGS;
        int batch_target = total_wgs / n;                                                            // the workspace query covers <= 1024
        if (!t.gemm_batch_even) {                                                                                 // tuning aid
            double work = 0.0;
            for (int j = 0; j < n; ++j) work += (double)p[j].M * ceil_div(p[j].N, 64) * ceil_div(p[j].K, 64);
            batch_target = (int)(total_wgs * ((double)M * ceil_div(N, 64) * ceil_div(K, 64) / work) + 0.5);
            if (batch_target > MAX_SPLIT_WGS) batch_target = MAX_SPLIT_WGS;
            if (batch_target < 1) batch_target = 1;
        }
        const Split s = choose_split(t, M, N, K, batch_target);
        Plan& q = out[i];
        q = Plan{};
        q.kernel = Kernel::batch;
        q.bm = q.bn = q.bk = 64; q.kw = 2;
        q.vec = q.store = 4;
        q.splits = s.splits; q.rows = s.rows; q.last = M - (s.splits - 1) * s.rows;
        q.wgrad = true;
    }
}
// whether aligned problems of this precision take the wgrad16 route (any_bf16: one of them is stored as bf16)
inline bool wgrad16_route(const CswinTuning& t, int precision, bool any_bf16) { return precision == 1 && (t.wgrad16_on || any_bf16); }

// The stand-alone cswin_linear_bwd_weight.  In bf16 mode an aligned problem without a concat input goes through the batch path, as
// a batch of one (the transposing-read kernel of wgrad16.hip); everything else through the tiled family.
// k_split: the seam of a concat input [x | x2] (0: a plain one), x2_aligned: its second part starts 16-B aligned
inline Plan linear_wgrad_plan(const CswinTuning& t, const WgradProblem& p, int k_split, int precision, bool x2_aligned) {
    if (precision == 1 && !k_split && p.aligned()) {
        Plan q;
        aligned_batch_plans(t, &p, 1, wgrad16_route(t, precision, p.io_bf16 != 0), &q);
        return q;
    }
    return wgrad_tiled_plan(t, p.M, p.N, p.K, k_split, precision, p.loads_aligned && (!k_split || x2_aligned), p.ws_aligned);
}

// cswin_linear_bwd_weight_batch / cswin_linear_bwd_tail and their masked and skip forms: n problems of one precision, and what
// rides with them.  (The entry point has refused masks on unaligned problems, and an order that the data gradient cannot take.)
inline BatchRoute batch_route(const CswinTuning& t, const WgradProblem* p, int n, int precision, const TailRequest& x) {
    BatchRoute r = {};
    bool fast = true, any_bf16 = false, any_mask = false;
    for (int i = 0; i < n; ++i) {
        fast = fast && p[i].aligned();
        any_bf16 = any_bf16 || p[i].io_bf16;
        any_mask = any_mask || p[i].has_mask;
    }
    const bool extra = x.dgrad || x.njobs > 0;
    const bool g_vec = x.N % 4 == 0 && x.K % 4 == 0 && x.loads_aligned;
    const bool merge_on = t.gemm_tail_merge != 0;                                                             // tuning aid
    // In fp32 with aligned operands the data gradient and the pending reductions run in the batch's ONE launch; otherwise they are
    // launched first and the batch follows -- same results either way.
    const bool ride = extra && merge_on && fast && precision == 0 && (!x.dgrad || (g_vec && x.dx_aligned));
    const bool w16_path = fast && wgrad16_route(t, precision, any_bf16);
    const bool jobs_ride16 = merge_on && w16_path && x.njobs > 0;                     // bf16 mode: the reductions ride in wgrad16's grid
    r.dgrad_first = x.dgrad && !ride;
    r.jobs_first = x.njobs > 0 && !ride && !jobs_ride16;
    r.jobs_ride = x.njobs > 0 && (ride || jobs_ride16);
    if (x.dgrad) {
        if (ride) {       // one more problem of the launch: 64 x 64 tiles, two k-groups of four waves (TailDgradTile)
            Plan& q = r.dgrad;
            q.kernel = Kernel::tail;
            q.bm = q.bn = q.bk = 64; q.kw = 2;
            q.vec = q.store = 4;
            q.splits = 1; q.rows = one_split(x.N); q.last = x.N;
        } else {          // as cswin_linear_bwd_data poses it
            r.dgrad = linear_dgrad_plan(t, x.M, x.N, x.K, 0, false, precision, 0, x.loads_aligned, x.dx_aligned);
        }
    }
    if (!fast) {
        // Separate launches.  In bf16 mode a problem that is aligned by itself still goes through the batch path, as a batch of one.
        r.kernel = BatchKernel::separate;
        for (int i = 0; i < n; ++i) r.problem[i] = linear_wgrad_plan(t, p[i], 0, precision, true);
        return r;
    }
    aligned_batch_plans(t, p, n, w16_path, r.problem);
    if (w16_path) r.kernel = BatchKernel::wgrad16;
    else if (ride) r.kernel = x.order ? BatchKernel::tail_order : any_mask ? BatchKernel::tail_masked : BatchKernel::tail;
    else r.kernel = any_mask ? BatchKernel::masked : BatchKernel::plain;
    return r;
}

}  // namespace gp
