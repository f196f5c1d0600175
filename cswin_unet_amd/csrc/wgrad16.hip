// bf16-operand weight gradient of nn.Linear for the bf16 matmul mode (BASELINE configs[2..4]), gfx950 / CDNA4.
//
//   dW[n][k] = sum_m (row_scale . dy)[m][n] * x[m][k]        dbias[n] = sum_m (row_scale . dy)[m][n]
//   (autograd backward of cswin_unet.py:169,177,23-27; dy (M, N) and x (M, K) fp32 in memory, both m-major)
//
// Both MFMA operands of this product run along the REDUCTION index m, while both matrices are stored with m as the slow
// index.  The tiled family (gemm.hip) transposes them while staging, with one 2-byte LDS store per element: with bf16
// MFMAs (16x the fp32 rate) that staging is the whole kernel (profiles/round1_gemm_bench_bf16_operands.txt: 3.07 ms per
// step against 3.30 ms in fp32).  Here the tiles are stored in LDS the way they arrive -- [m][128 columns] bf16 rows, one
// ds_write_b64 per 16-B global chunk -- and CDNA4's transposing LDS read (tr16_frag, bf16_tile.h) delivers the m-contiguous
// fragments that v_mfma_f32_32x32x16_bf16 wants.  256-B rows are XOR-swizzled per 16-B chunk (guide T10, image (b)) so that
// the transposed reads are bank-conflict free.
//
// One workgroup = 4 waves = one 128 (n) x 128 (k) tile of dW over one slice of m; partial tiles go to the same
// [split][N*K + N] slabs as the fp32 path, reduced by cswin_rows_sum_multi.  fp32 accumulation throughout.
#include "bf16_tile.h"
#include "common.h"
#include "gemm_plan.h"

namespace {

constexpr int W16_T = gp::W16_T;    // tile edge (n and k)
constexpr int W16_MS = gp::W16_MS;  // m rows per step
constexpr int W16_MAXP = gp::WGRAD_BATCH;

struct W16Problem {
    const float* dy; const float* x; const float* row_scale;
    float* slab;                    // [splits][N*K + N]
    int M, N, K, rows_per_sample, rows_per_split, tiles_n, tiles_k, has_bias;
    int dy_bf16, x_bf16;            // the operand is stored as bf16 (bf16 activation storage)
    int dma;                        // both stored as bf16, M % 32 == 0, N % 8 == K % 8 == 0: LDS-DMA tile (below)
    long slab_stride;
};
struct W16Batch {
    W16Problem p[W16_MAXP];
    int first[W16_MAXP + 1];
    int n;
    long long* stamps;              // debug (cswin_debug_set_stamps): [workgroup][8] s_memtime / realtime stamps of thread 0, or NULL
    ReduceRiders r;                 // pending slab reductions of earlier launches: the grid's last workgroups (common.h)
};

// byte offset of 16-B chunk `ch` (8 bf16) of row `row` inside a [rows][128] bf16 image
__device__ __forceinline__ int img_off(int row, int ch) { return 256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3))); }

constexpr int W16_DMA_S = 3;                                        // LDS-DMA tile: steps in flight
constexpr int W16_STEP = 2 * W16_MS * 256;                          // bytes of one step's (dy | x) images
constexpr int W16_SC_SAMPLES = gp::W16_SC_SAMPLES;                  // DropPath factors of the samples a workgroup's rows touch
constexpr int W16_SC_BYTES = (W16_SC_SAMPLES + W16_DMA_S * W16_MS) * 4;
constexpr int W16_LDS = W16_DMA_S * W16_STEP + W16_SC_BYTES;        // 48.6 KB (register path: 2 stages + bias sums = 36 KB): 3 workgroups per CU
static_assert(W16_LDS >= 2 * W16_STEP + 8 * W16_T * 4, "the register path's stages and bias sums must fit");

// What workgroup lb of a problem works on, for both tiles below: its slice [m_begin, m_end) of the reduction (slab `split`), its
// 128 x 128 tile at (nb, kb) and its place in it -- wave tile n in [nb + 64 wi, +64), k in [kb + 64 wj, +64).
struct W16Tile {
    int split, nb, kb, m_begin, m_end, lane, wave, wi, wj, lh;
    // wave: threadIdx.x >> 6, as the caller holds it (the LDS-DMA tile passes it wave-uniform)
    __device__ __forceinline__ W16Tile(const W16Problem& P, int lb, int wave_) {
        const int tiles = P.tiles_n * P.tiles_k;
        split = lb / tiles;
        const int tile = lb - split * tiles;
        nb = (tile / P.tiles_k) * W16_T; kb = (tile % P.tiles_k) * W16_T;
        m_begin = split * P.rows_per_split;
        m_end = min(P.M, m_begin + P.rows_per_split);
        lane = threadIdx.x & 63; wave = wave_;
        wi = wave >> 1; wj = wave & 1;
        lh = lane >> 5;
    }
    // the m-contiguous fragment of a 32-column block cb (columns cb .. cb + 31) of a [m][128] image for the k16 step at row r16:
    // group (lane >> 4) & 1 takes columns cb + 16 * that, lane half lh rows r16 + 8 lh + 0 .. 7 (tr16_frag, with img_off's swizzle)
    __device__ __forceinline__ bf16x8 tr_frag(const unsigned char* img, int cb, int r16) const {
        const int col = cb + 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
        const int row = r16 + 8 * lh + ((lane & 15) >> 2);
        return tr16_frag(img + img_off(row, col >> 3) + 2 * (col & 7), img + img_off(row + 4, col >> 3) + 2 * (col & 7));
    }
    // the workgroup's slab: N x K products, then N bias sums
    __device__ __forceinline__ float* slab(const W16Problem& P) const { return P.slab + (long)split * P.slab_stride; }
};

// Partial 64 x 64 wave tile -> the workgroup's slab.  Stored from the accumulators' layout (lane = k, registers = rows n) a wave
// issues 64 dword stores; through its LDS patch (patch_put) a lane owns 4 consecutive k of one row: 16 stores of 16 B.  Call
// after a workgroup barrier (the patches overlay the operand images); K % 4 == 0 and 16-B aligned slabs are the caller's
// contract.  N and K by value: read through the problem they are loaded again between the stores.
__device__ __forceinline__ void w16_store_tile(f32x16 (&acc)[2][2], float* slab, const int N, const int K, const W16Tile& t, unsigned char* lds) {
    float* patch = reinterpret_cast<float*>(lds) + t.wave * EP_WAVE_FLOATS;
    const int n0 = t.nb + 64 * t.wi, k0 = t.kb + 64 * t.wj, rrow = t.lane >> 3, rcol = (t.lane & 7) * 4;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            patch_put(patch, acc[a][c], t.lane);
            const int k = k0 + 32 * c + rcol;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int n = n0 + 32 * a + rrow + 8 * q;
                if (n < N && k < K) *reinterpret_cast<f32x4*>(slab + (long)n * K + k) = *reinterpret_cast<const f32x4*>(&patch[(rrow + 8 * q) * EP_LD + rcol]);
            }
            wave_lds_fence();
        }
}

// One problem's tile.  DY16 / X16: that operand is STORED as bf16 -- compile-time copies of the body (chosen per workgroup in
// the kernel below): a run-time choice between 8-B and 16-B loads inside fetch() makes the prefetch loads wait for one another.
template <bool DY16, bool X16>
__device__ __forceinline__ void wgrad16_tile(const W16Problem& P, const int lb, unsigned char* lds, long long* stamps) {
    const int tid = threadIdx.x;
    const W16Tile t(P, lb, tid >> 6);
    const int nb = t.nb, kb = t.kb, m_begin = t.m_begin, m_end = t.m_end, wi = t.wi, wj = t.wj;

    // loader: thread -> 16-B fp32 chunk c (4 columns) of rows lr + 8 j, j = 0..3, of both tiles
    const int lc = tid & 31, lr = tid >> 5;
    const bool n_ok = nb + 4 * lc < P.N, k_ok = kb + 4 * lc < P.K;
    const float* dyp = P.dy + nb + 4 * lc;
    const float* xp = P.x + kb + 4 * lc;
    f32x4 gdy[4], gx[4];
    u32x2 gdyh[4], gxh[4];          // raw chunks of a bf16-stored operand (INTEGER vectors: see widen_bf16x4)
    float grs[4];
    auto fetch = [&](int m0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int m = m0 + lr + 8 * j;
            const bool ok = m < m_end;
            gdy[j] = f32x4{0.f, 0.f, 0.f, 0.f};
            gx[j] = f32x4{0.f, 0.f, 0.f, 0.f};
            gdyh[j] = u32x2{0u, 0u};
            gxh[j] = u32x2{0u, 0u};
            // bf16-stored operands arrive as raw bits in the two low lanes and are widened (dy) or passed through (x) in stash():
            // a conversion here would make every prefetch wait for its own data
            if (ok && n_ok) {
                if constexpr (DY16) {
                    gdyh[j] = *reinterpret_cast<const u32x2*>(reinterpret_cast<const __bf16*>(P.dy) + (long)m * P.N + nb + 4 * lc);
                } else {
                    gdy[j] = *reinterpret_cast<const f32x4*>(dyp + (long)m * P.N);
                }
            }
            if (ok && k_ok) {
                if constexpr (X16) {
                    gxh[j] = *reinterpret_cast<const u32x2*>(reinterpret_cast<const __bf16*>(P.x) + (long)m * P.K + kb + 4 * lc);
                } else {
                    gx[j] = *reinterpret_cast<const f32x4*>(xp + (long)m * P.K);
                }
            }
            grs[j] = (P.row_scale && ok) ? P.row_scale[m / P.rows_per_sample] : 1.0f;
        }
    };
    f32x4 bsum = {0.f, 0.f, 0.f, 0.f};
    auto stash = [&](int stage) {
        unsigned char* dimg = lds + stage * (2 * W16_MS * 256);
        unsigned char* ximg = dimg + W16_MS * 256;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r = lr + 8 * j;
            f32x4 d = gdy[j];
            if constexpr (DY16) d = widen_bf16x4(gdyh[j]);
            d *= grs[j];
            bsum += d;
            const int off = img_off(r, lc >> 1) + 8 * (lc & 1);
            *reinterpret_cast<bf16x4*>(dimg + off) = __builtin_convertvector(d, bf16x4);
            if constexpr (X16) *reinterpret_cast<u32x2*>(ximg + off) = gxh[j];
            else *reinterpret_cast<bf16x4*>(ximg + off) = __builtin_convertvector(gx[j], bf16x4);
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[a][c][e] = 0.f;

    if (m_begin < m_end) {
        fetch(m_begin);
        stash(0);
        __syncthreads();
        stamp_slot(stamps, blockIdx.x, 1);
        int stage = 0;
        for (int m0 = m_begin; m0 < m_end; m0 += W16_MS) {
            const bool more = m0 + W16_MS < m_end;
            if (more) fetch(m0 + W16_MS);
            const unsigned char* dimg = lds + stage * (2 * W16_MS * 256);
            const unsigned char* ximg = dimg + W16_MS * 256;
#pragma unroll
            for (int r16 = 0; r16 < W16_MS; r16 += 16) {
                bf16x8 af[2], bf[2];
#pragma unroll
                for (int a = 0; a < 2; ++a) af[a] = t.tr_frag(dimg, 64 * wi + 32 * a, r16);
#pragma unroll
                for (int c = 0; c < 2; ++c) bf[c] = t.tr_frag(ximg, 64 * wj + 32 * c, r16);
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int c = 0; c < 2; ++c) acc[a][c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[a], bf[c], acc[a][c], 0, 0, 0);
            }
            if (more) stash(stage ^ 1);          // the other stage was last read one step ago, before the barrier below
            __syncthreads();
            stage ^= 1;
        }
    }

    stamp_slot(stamps, blockIdx.x, 2);
    // ---- partial tile -> slab ----
    __syncthreads();                        // every wave is done with the operand images: they become the store patches
    float* slab = t.slab(P);
    w16_store_tile(acc, slab, P.N, P.K, t, lds);
    // ---- bias gradient partial: column sums of the dy tile (only the k-tile 0 workgroups own them) ----
    if (P.has_bias && kb == 0) {
        float* red = reinterpret_cast<float*>(lds + 2 * 2 * W16_MS * 256);      // [8][128]
        *reinterpret_cast<f32x4*>(&red[lr * W16_T + 4 * lc]) = bsum;
        __syncthreads();
        if (tid < W16_T && nb + tid < P.N) {
            float s = 0.f;
#pragma unroll
            for (int r = 0; r < 8; ++r) s += red[r * W16_T + tid];
            slab[(long)P.N * P.K + nb + tid] = s;
        }
    }
}

// ---- LDS-DMA tile: both operands stored as bf16 and used as they are (no row scale) ----------------------------------------
// The register path above spends ~3 k cycles per 32-row step on 256 cycles of MFMA work (tools/wgrad16_stamps.py): one
// global-load round trip per step, its prefetch reaching one step ahead, and a second register set costs a workgroup per CU.
// Here the [m][128] images are written by LDS-DMA (lds_dma, bf16_tile.h; no registers: three steps in flight at the same
// occupancy), the XOR swizzle of img_off applied to the SOURCE chunk, one counted dma_wait + dma_barrier per step.  The bias gradient
// (column sums of dy) is one more MFMA per fragment against a constant ones operand instead of a pass over the tile.
// SCALE (DropPath row factors on dy): the factors of the samples this workgroup's rows touch are read once, a 32-entry per-row
// table is refreshed per step in LDS, and the dy fragments are scaled as they leave LDS (widen, multiply, round: the same
// arithmetic, element by element, as the register path's scale-then-round).
template <bool SCALE>
__device__ __forceinline__ void wgrad16_dma_tile(const W16Problem& P, const int lb, unsigned char* lds, long long* stamps) {
    const int tid = threadIdx.x;
    const W16Tile t(P, lb, __builtin_amdgcn_readfirstlane(tid >> 6));
    const int nb = t.nb, kb = t.kb, m_begin = t.m_begin, m_end = t.m_end, lane = t.lane, wave = t.wave, wi = t.wi, wj = t.wj, lh = t.lh;
    const int nsteps = (m_end - m_begin) / W16_MS;              // whole steps: M and the split size are multiples of 32
    const int li = lane & 31;
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)lds;

    // DMA: a wave instruction moves 4 image rows (1 KB); wave w moves row groups 2 w, 2 w + 1 of both images of a step
    const int drow = lane >> 4, slot = lane & 15;
    const unsigned char* dy_src[2];
    const unsigned char* x_src[2];
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        const int row = (2 * wave + g) * 4 + drow;
        const int ch = slot ^ (((row & 3) << 2) | ((row >> 2) & 3));                    // source chunk of this lane's slot (img_off)
        const int cn = min(ch, (P.N - nb) / 8 - 1), ck = min(ch, (P.K - kb) / 8 - 1);   // columns beyond N / K: in-range data, never stored
        dy_src[g] = reinterpret_cast<const unsigned char*>(reinterpret_cast<const __bf16*>(P.dy) + (long)(m_begin + row) * P.N + nb + 8 * cn);
        x_src[g] = reinterpret_cast<const unsigned char*>(reinterpret_cast<const __bf16*>(P.x) + (long)(m_begin + row) * P.K + kb + 8 * ck);
    }
    auto issue = [&](int step) {
        const unsigned stg = lds0 + (unsigned)(step % W16_DMA_S) * W16_STEP + (unsigned)wave * 2048;
#pragma unroll
        for (int g = 0; g < 2; ++g) lds_dma(dy_src[g] + (long)step * W16_MS * P.N * 2, stg + g * 1024);
#pragma unroll
        for (int g = 0; g < 2; ++g) lds_dma(x_src[g] + (long)step * W16_MS * P.K * 2, stg + W16_MS * 256 + g * 1024);
    };

    f32x16 acc[2][2], accb[2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
#pragma unroll
        for (int e = 0; e < 16; ++e) accb[a][e] = 0.f;
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[a][c][e] = 0.f;
    }
    const bool do_bias = P.has_bias && kb == 0 && wj == 0;      // wave-uniform
    // DropPath factors: samples b0 .. of this workgroup's rows (read BEFORE the first DMA: older in the vmcnt queue)
    float* sc_tab = reinterpret_cast<float*>(lds + W16_DMA_S * W16_STEP);
    float* sc_row = sc_tab + W16_SC_SAMPLES;                     // [stage][32]
    const int b0 = SCALE ? m_begin / P.rows_per_sample : 0;
    if constexpr (SCALE) {
        const int nb_s = (m_end - 1) / P.rows_per_sample - b0 + 1;
        if (tid < nb_s) sc_tab[tid] = P.row_scale[b0 + tid];
        __syncthreads();
    }
    auto fill_rows = [&](int step) {                            // per-row factors of a step (LDS only)
        if (tid < W16_MS) sc_row[(step % W16_DMA_S) * W16_MS + tid] = sc_tab[(m_begin + step * W16_MS + tid) / P.rows_per_sample - b0];
    };
    const s16x8 ones_s = {0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80};      // bf16 1.0
    const bf16x8 ones = __builtin_bit_cast(bf16x8, ones_s);

    for (int s = 0; s < W16_DMA_S - 1 && s < nsteps; ++s) {
        issue(s);
        if constexpr (SCALE) fill_rows(s);
    }
    for (int step = 0; step < nsteps; ++step) {
        const int later = min(W16_DMA_S - 2, nsteps - 1 - step);
        if (later >= 1) dma_wait<4>();      // this step's 4 DMAs (per wave) have landed when only the next step's 4 are outstanding
        else dma_wait<0>();
        dma_barrier();                      // the step is in LDS for every wave; the stage read one step ago is free again
        if (step + W16_DMA_S - 1 < nsteps) {
            issue(step + W16_DMA_S - 1);
            if constexpr (SCALE) fill_rows(step + W16_DMA_S - 1);
        }
        if (step == 0) stamp_slot(stamps, blockIdx.x, 1);
        const unsigned char* dimg = lds + (step % W16_DMA_S) * W16_STEP;
        const unsigned char* ximg = dimg + W16_MS * 256;
#pragma unroll
        for (int r16 = 0; r16 < W16_MS; r16 += 16) {
            bf16x8 af[2], bf[2];
#pragma unroll
            for (int a = 0; a < 2; ++a) af[a] = t.tr_frag(dimg, 64 * wi + 32 * a, r16);
#pragma unroll
            for (int c = 0; c < 2; ++c) bf[c] = t.tr_frag(ximg, 64 * wj + 32 * c, r16);
            if constexpr (SCALE) {
                // a lane's 8 values are rows r16 + 8 lh + 0 .. 7 of its column
                const float* sr = &sc_row[(step % W16_DMA_S) * W16_MS + r16 + 8 * lh];
                const f32x4 s0 = *reinterpret_cast<const f32x4*>(sr), s1 = *reinterpret_cast<const f32x4*>(sr + 4);
#pragma unroll
                for (int a = 0; a < 2; ++a) {
                    const u32x4 raw = __builtin_bit_cast(u32x4, af[a]);
                    const f32x4 lo = widen_bf16x4(u32x2{raw[0], raw[1]}), hi = widen_bf16x4(u32x2{raw[2], raw[3]});
                    af[a] = __builtin_shufflevector(__builtin_convertvector(lo * s0, bf16x4), __builtin_convertvector(hi * s1, bf16x4), 0, 1, 2, 3, 4, 5, 6, 7);
                }
            }
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int c = 0; c < 2; ++c) acc[a][c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[a], bf[c], acc[a][c], 0, 0, 0);
            if (do_bias) {
#pragma unroll
                for (int a = 0; a < 2; ++a) accb[a] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[a], ones, accb[a], 0, 0, 0);
            }
        }
    }
    stamp_slot(stamps, blockIdx.x, 2);
    dma_barrier();                          // every wave is done with the operand images: they become the store patches
    float* slab = t.slab(P);
    w16_store_tile(acc, slab, P.N, P.K, t, lds);
    if (do_bias && li == 0) {               // every column of the ones product holds the row sums: take column 0
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                const int n = nb + 64 * wi + 32 * a + (g & 3) + 8 * (g >> 2) + 4 * lh;
                if (n < P.N) slab[(long)P.N * P.K + n] = accb[a][g];
            }
    }
}

__global__ __launch_bounds__(256, 3) void wgrad16_kernel(W16Batch b) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[W16_LDS];
    if ((int)blockIdx.x >= b.first[b.n]) {
        static_assert(W16_LDS >= (int)sizeof(float) * RS_G * (RS_COLS + 1), "reduction scratch");
        rows_sum_dispatch(b.r.j, b.r.first_block, b.r.njobs, (int)blockIdx.x - b.first[b.n], reinterpret_cast<float(*)[RS_COLS + 1]>(lds));
        return;
    }
    int pi = 0;
    while (pi + 1 < b.n && (int)blockIdx.x >= b.first[pi + 1]) ++pi;
    const W16Problem& P = b.p[pi];
    const int lb = (int)blockIdx.x - b.first[pi];
    stamp_slot(b.stamps, blockIdx.x, 0);
    if (P.dma) {            // SCALE, like DY16 / X16, is compile-time: the unscaled tile carries no table, no LDS reads and no rounding
        if (P.row_scale) wgrad16_dma_tile<true>(P, lb, lds, b.stamps);
        else wgrad16_dma_tile<false>(P, lb, lds, b.stamps);
    } else if (P.dy_bf16) {
        if (P.x_bf16) wgrad16_tile<true, true>(P, lb, lds, b.stamps);
        else wgrad16_tile<true, false>(P, lb, lds, b.stamps);
    } else {
        if (P.x_bf16) wgrad16_tile<false, true>(P, lb, lds, b.stamps);
        else wgrad16_tile<false, false>(P, lb, lds, b.stamps);
    }
    stamp_slot(b.stamps, blockIdx.x, 3);
}

}  // namespace

// Internal entry used by gemm.hip's weight-gradient batches in bf16 matmul mode.  Problems must be 16-B aligned with
// N % 4 == K % 4 == 0; plans[i] (gp::aligned_batch_plans, Kernel::wgrad16) gives problem i's slabs -- no more than its workspace
// holds -- and whether it takes the LDS-DMA tile.  pending[0..npending): reductions of earlier launches that ride as this grid's
// last workgroups.  The caller has checked all of it.
void cswin_wgrad16_batch(const cswin_wgrad_desc* d, int n, const gp::Plan* plans, const cswin_reduce_job* pending, int npending, void* stream,
                         long long* stamps) {
    W16Batch b = {};
    int blocks = 0;
    for (int i = 0; i < n; ++i) {
        W16Problem& P = b.p[i];
        P.dy = d[i].dy; P.x = d[i].x; P.row_scale = d[i].row_scale;
        P.slab = (float*)d[i].workspace;
        P.M = d[i].M; P.N = d[i].N; P.K = d[i].K;
        P.rows_per_sample = d[i].row_scale ? d[i].rows_per_sample : 1;
        P.rows_per_split = plans[i].rows;
        P.tiles_n = cdiv(P.N, W16_T); P.tiles_k = cdiv(P.K, W16_T);
        P.has_bias = d[i].dbias != nullptr;
        P.dy_bf16 = d[i].io_bf16 & 1;
        P.x_bf16 = (d[i].io_bf16 >> 1) & 1;
        P.slab_stride = gp::slab_stride(P.N, P.K);
        P.dma = plans[i].dma;
        b.first[i] = blocks;
        blocks += P.tiles_n * P.tiles_k * plans[i].splits;
    }
    b.first[n] = blocks;
    b.n = n;
    b.stamps = stamps;
    int rblocks = 0;
    if (npending > 0) {
        rblocks = fill_reduce_table(pending, npending, b.r.j, b.r.first_block);
        b.r.njobs = npending;
    }
    static_assert(sizeof(W16Batch) <= 4096, "kernel argument block");
    hipLaunchKernelGGL(wgrad16_kernel, dim3(blocks + rblocks), dim3(256), 0, (hipStream_t)stream, b);
}
