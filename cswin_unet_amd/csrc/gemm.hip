// fp32 MFMA GEMM family for the CSWin-UNet hot path (gfx950 / CDNA4).
//
//   C[m][n] = epilogue( sum_r A(m, r) * B(n, r) )
//
// One kernel template serves every dense contraction of the model:
//   * Linear forward        (A = X  [M,K] r-contiguous, B = W [N,K] r-contiguous)      "NT"
//   * Linear data-gradient  (A = dY [M,N] r-contiguous, B = W [N,K] row-contiguous)    "NN"
//   * Linear weight-gradient(A = dY, B = X, both row-contiguous, split over M)         "TN"
//   * 3x3 / strided convolutions on the (B, L, C) token layout as implicit GEMM: the
//     A operand is gathered on the fly from NHWC tokens (no im2col buffer, no NCHW
//     transposes -- replaces the transpose/contiguous/conv/transpose chain of
//     networks/cswin_unet.py:214-217, 235-241).
//
// Matrix cores: v_mfma_f32_32x32x2_f32 (exact fp32, 64 FLOP/clk/SIMD = 157 TF/s chip peak).
// The k index inside an MFMA is arbitrary as long as A and B agree, so an r-contiguous
// operand is read from its [row][r] LDS image with ONE ds_read_b128 per four MFMA steps
// (lane half h takes r = kk + 4h + s), and a row-contiguous operand from its [r][row]
// image with conflict-free ds_read_b32.  Global loads are 16 B per lane; LDS is single
// buffered with register prefetch of the next tile (4 workgroups of 4 waves co-reside per CU
// and cover each other's barriers).
#include <stdlib.h>

#include <type_traits>
#include "bf16_tile.h"
#include "common.h"
#include "gemm_epilogue.h"
#include "gemm_plan.h"

// both operands stored as bf16 (gemm16.hip), launched as plan (Kernel::gemm16) says; 0 = launched, 1 = a HIP error
int cswin_gemm16(const gp::Plan& plan, int mode, int epi_mode, const void* A, const void* B, const void* epilogue, int M, int NO, int R, void* stream);
// wgrad16.hip: bf16-operand weight gradients with transposing LDS reads (bf16 matmul mode)
void cswin_wgrad16_batch(const cswin_wgrad_desc* d, int n, const gp::Plan* plans, const cswin_reduce_job* pending, int npending, void* stream,
                         long long* stamps);

namespace {

// matmul precision is an ARGUMENT of every entry point (no library state): 0 = exact fp32 MFMA (the parity path);
// 1 = operands rounded to bf16 while they are staged into LDS, v_mfma_f32_32x32x16_bf16, fp32 accumulation and fp32
// storage everywhere (BASELINE configs 3-5 name bf16)
#define CSWIN_CHECK_PRECISION(p, who) CSWIN_REQUIRE((p) == 0 || (p) == 1, CSWIN_ERR_UNSUPPORTED, "%s: precision %d (0 = fp32, 1 = bf16 operands)", who, (p))

// ------------------------------------------------------------------------------------
// operand sources: a logical matrix S(i, j) whose fast (contiguous) index is j
// ------------------------------------------------------------------------------------
struct PlainSrc {
    const float* p; long ld; int rows, cols;
    const float* row_scale; int rows_per_sample;     // optional per-row multiplier (DropPath backward)
    int bf16;                                        // the matrix is stored as bf16 (p is then only an element-indexed handle)
    static constexpr bool fast_div = false;          // no divisions by multiply-high in this source (see ConvSrcT)
    struct Row { const float* base; float s; };
    typedef int Col;                                 // a column of a plain matrix is its index (the gather sources split theirs)
    __device__ Col col(int j) const { return j; }
    __device__ Row row(int i) const {
        Row r;
        r.base = (i < rows) ? p + (long)i * ld : nullptr;
        r.s = (row_scale && i < rows) ? row_scale[i / rows_per_sample] : 1.0f;
        return r;
    }
    __device__ const float* ptr(const Row& r, int j) const { return (r.base && j < cols) ? r.base + j : nullptr; }
};

// What only a plain matrix has: bf16 storage, a sample mask, a row scale.  For every other source these compile to nothing.
template <class S> constexpr bool is_plain = std::is_same<S, PlainSrc>::value;
// bf16 STORAGE of an operand (activations of the bf16 mode): every source computes addresses in elements, so the element offset
// of the fp32-typed pointer is re-applied to the bf16 base.
template <class S> __device__ __forceinline__ bool src_is_bf16(const S& s) {
    if constexpr (is_plain<S>) return s.bf16 != 0;
    else return false;
}
// 4 bf16 as two raw dwords (an INTEGER vector: see widen_bf16x4); they go to the LDS image as they are (chunk_bf16 below)
template <class S> __device__ __forceinline__ u32x2 src_load4_bf16(const S& s, const float* p) {
    if constexpr (is_plain<S>) return *reinterpret_cast<const u32x2*>(reinterpret_cast<const __bf16*>(s.p) + (p - s.p));
    else return u32x2{0u, 0u};
}
// a sample-masked reduction (RowMask below) maps its own rows: row < 0 = past the end, f = the row's DropPath factor
template <class S> __device__ __forceinline__ typename S::Row src_mapped_row(const S& s, int row, float f) {
    typename S::Row r{};
    if constexpr (is_plain<S>) {
        r.base = row >= 0 ? s.p + (long)row * s.ld : nullptr;
        r.s = f;
    }
    return r;
}
template <class S> __device__ __forceinline__ const float* src_row_scale(const S& s) {
    if constexpr (is_plain<S>) return s.row_scale;
    else return nullptr;
}

// cat([p0 (c0 cols), p1 (cols - c0)], dim=-1) without materialising it (skip-concat, cswin_unet.py:509-510)
struct ConcatSrc {
    const float* p0; const float* p1; long ld0, ld1; int rows, cols, c0;
    static constexpr bool fast_div = false;
    struct Row { const float* b0; const float* b1; float s; };
    typedef int Col;
    __device__ Col col(int j) const { return j; }
    __device__ Row row(int i) const {
        Row r;
        r.b0 = (i < rows) ? p0 + (long)i * ld0 : nullptr;
        r.b1 = (i < rows) ? p1 + (long)i * ld1 : nullptr;
        r.s = 1.0f;
        return r;
    }
    __device__ const float* ptr(const Row& r, int j) const {
        if (!r.b0 || j >= cols) return nullptr;
        return j < c0 ? r.b0 + j : r.b1 + (j - c0);
    }
};

// The gather sources below split a row index into (b, y, x) and a column index into (tap, channel), the tap into (ky, kx): integer
// divisions by run-time divisors, per 16-byte chunk and per reduction tile.  FAST: every one of them is a multiply-high by a
// reciprocal made on the host (fdiv, common.h), which is exact only inside fdiv's bound; the entry points check that bound for
// every (largest dividend, divisor) pair of a launch and otherwise instantiate FAST = false, the same code with the compiler's
// divisions.  Either way the loads issued are the same, so the results do not depend on the choice.
template <bool FAST> __device__ __forceinline__ int qdiv(int n, int d, unsigned m) {
    if constexpr (FAST) return fdiv1(n, m);
    else return n / d;
}
// the divisors' reciprocals, made beside the bound checks (conv_magics below); unused fields stay 0
struct ConvMagics { unsigned img, w, c, ks, stride; };

// implicit im2col of NHWC tokens: i = output pixel (b, oy, ox), j = tap * C + ci
template <bool FAST>
struct ConvSrcT {
    const float* x; int B, H, W, C, OH, OW, ks, stride, pad; int rows, cols;
    static constexpr bool fast_div = FAST;
    ConvMagics m;                                    // img: OH * OW, w: OW, c: C, ks: ks
    struct Row { int b, iy0, ix0; float s; };
    struct Col { int ky, kx, ci; };                  // ci < 0: past the last column
    __device__ Row row(int i) const {
        Row r;
        r.s = 1.0f;
        if (i >= rows) { r.b = -1; r.iy0 = r.ix0 = 0; return r; }
        int ohw = OH * OW;
        r.b = qdiv<FAST>(i, ohw, m.img);
        int rem = i - r.b * ohw;
        int oy = qdiv<FAST>(rem, OW, m.w);
        r.iy0 = oy * stride - pad;
        r.ix0 = (rem - oy * OW) * stride - pad;
        return r;
    }
    __device__ Col col(int j) const {
        Col c;
        if (j >= cols) { c.ky = c.kx = 0; c.ci = -1; return c; }
        int tap = qdiv<FAST>(j, C, m.c);
        c.ci = j - tap * C;
        c.ky = qdiv<FAST>(tap, ks, m.ks);
        c.kx = tap - c.ky * ks;
        return c;
    }
    __device__ const float* ptr(const Row& r, const Col& c) const {
        if (r.b < 0 || c.ci < 0) return nullptr;
        int iy = r.iy0 + c.ky, ix = r.ix0 + c.kx;
        if ((unsigned)iy >= (unsigned)H || (unsigned)ix >= (unsigned)W) return nullptr;
        return x + ((long)(r.b * H + iy) * W + ix) * C + c.ci;
    }
};

// transposed gather for the conv data-gradient: i = input pixel (b, iy, ix), j = tap * C + co over dy (NHWC, OHxOW)
template <bool FAST>
struct ConvTSrcT {
    const float* dy; int B, H, W, C, OH, OW, ks, stride, pad; int rows, cols;   // C = Cout here
    static constexpr bool fast_div = FAST;
    ConvMagics m;                                    // img: H * W, w: W, c: C, ks: ks, stride: stride
    struct Row { int b, iy, ix; float s; };
    struct Col { int ky, kx, co; };                  // co < 0: past the last column
    __device__ Row row(int i) const {
        Row r;
        r.s = 1.0f;
        if (i >= rows) { r.b = -1; r.iy = r.ix = 0; return r; }
        int hw = H * W;
        r.b = qdiv<FAST>(i, hw, m.img);
        int rem = i - r.b * hw;
        r.iy = qdiv<FAST>(rem, W, m.w);
        r.ix = rem - r.iy * W;
        return r;
    }
    __device__ Col col(int j) const {
        Col c;
        if (j >= cols) { c.ky = c.kx = 0; c.co = -1; return c; }
        int tap = qdiv<FAST>(j, C, m.c);
        c.co = j - tap * C;
        c.ky = qdiv<FAST>(tap, ks, m.ks);
        c.kx = tap - c.ky * ks;
        return c;
    }
    __device__ const float* ptr(const Row& r, const Col& c) const {
        if (r.b < 0 || c.co < 0) return nullptr;
        int ty = r.iy + pad - c.ky, tx = r.ix + pad - c.kx;
        if (ty < 0 || tx < 0) return nullptr;
        int oy = qdiv<FAST>(ty, stride, m.stride), ox = qdiv<FAST>(tx, stride, m.stride);
        if (oy * stride != ty || ox * stride != tx || oy >= OH || ox >= OW) return nullptr;
        return dy + ((long)(r.b * OH + oy) * OW + ox) * C + c.co;
    }
};

// Stride-2 3x3 pad-1 data gradient, one input-pixel parity class (py, px) at a time: an input pixel only ever meets the
// taps with ky = (iy + 1) mod 2 (+2), kx likewise, i.e. 1, 2, 2 or 4 of the 9 taps depending on its class.  Gathering
// over all 9 taps (ConvTSrcT) feeds 75 % structural zeros to the MFMAs; per class there are none.
// i = class-local pixel (b, jy, jx) <-> (iy, ix) = (2 jy + py, 2 jx + px);  j = tap_local * C + co.
template <bool FAST>
struct ConvTS2SrcT {
    const float* dy; int B, H, W, C, OH, OW, py, px, H2, W2, kys, kxs; int rows, cols;   // kys/kxs: 2 bits per local tap
    static constexpr bool fast_div = FAST;
    ConvMagics m;                                    // img: H2 * W2, w: W2, c: C
    struct Row { int b, iy, ix; float s; };
    struct Col { int ky, kx, co; };                  // co < 0: past the last column
    __device__ Row row(int i) const {
        Row r;
        r.s = 1.0f;
        if (i >= rows) { r.b = -1; r.iy = r.ix = 0; return r; }
        const int hw = H2 * W2;
        r.b = qdiv<FAST>(i, hw, m.img);
        const int rem = i - r.b * hw;
        const int jy = qdiv<FAST>(rem, W2, m.w);
        r.iy = 2 * jy + py;
        r.ix = 2 * (rem - jy * W2) + px;
        return r;
    }
    __device__ Col col(int j) const {
        Col c;
        if (j >= cols) { c.ky = c.kx = 0; c.co = -1; return c; }
        const int t = qdiv<FAST>(j, C, m.c);
        c.co = j - t * C;
        c.ky = (kys >> (2 * t)) & 3;
        c.kx = (kxs >> (2 * t)) & 3;
        return c;
    }
    __device__ const float* ptr(const Row& r, const Col& c) const {
        if (r.b < 0 || c.co < 0) return nullptr;
        const int oy = (r.iy + 1 - c.ky) >> 1, ox = (r.ix + 1 - c.kx) >> 1;
        if (oy >= OH || ox >= OW) return nullptr;
        return dy + ((long)(r.b * OH + oy) * OW + ox) * C + c.co;
    }
};

// rows (tap_local, co) of the [9][Cout][Cin] weight image that belong to one parity class
template <bool FAST>
struct TapRowsSrcT {
    const float* w; int Cout, Cin, taps; int rows, cols;      // taps: 4 bits per local tap (index into the 9 taps)
    unsigned m_cout;
    struct Row { const float* base; float s; };
    typedef int Col;
    __device__ Row row(int i) const {
        Row r;
        r.s = 1.0f;
        if (i >= rows) { r.base = nullptr; return r; }
        const int t = qdiv<FAST>(i, Cout, m_cout), co = i - t * Cout;
        r.base = w + ((long)((taps >> (4 * t)) & 15) * Cout + co) * Cin;
        return r;
    }
    __device__ Col col(int j) const { return j; }
    __device__ const float* ptr(const Row& r, int j) const { return (r.base && j < cols) ? r.base + j : nullptr; }
};

// ---- tile geometry ----
// One operand's share of a tile: ROWS output rows x BK reduction values, staged by NTH threads in 16-byte chunks.
// RC: the source is r-contiguous; its fp32 image is [row][r] with 16-B padded rows (conflict-free b128 reads), else [r][row].
template <int ROWS, int BK, bool RC_, int NTH>
struct OperandTile {
    static constexpr bool RC = RC_;
    static constexpr int LD = RC ? BK + 4 : ROWS + 4;        // leading dimension of the fp32 image
    static constexpr int ELEMS = (RC ? ROWS : BK) * LD;      // its floats
    static constexpr int Q = ROWS * BK / (4 * NTH);          // chunks per thread per tile
    static constexpr int CPR = RC ? BK / 4 : ROWS / 4;       // chunks per source row
    static constexpr int RPP = NTH / CPR;                    // source rows per pass of the workgroup
    static_assert(Q >= 1, "tile too small for this many wave groups");
};

// One tile configuration.  Waves of one k-group: 2 x 2 for 64 x 64 tiles, 2 x 1 for 64 x 32 (for launches whose 64 x 64 tile count
// is a poor multiple of the 256 CUs).  KW: wave groups that split each reduction tile between them (group g multiplies the k-slice
// [g*BK/KW, (g+1)*BK/KW), the accumulators are summed through LDS at the end): more resident waves per workgroup where M*N is too
// small to give every SIMD >= 2 independent MFMA chains, without a global split-K reduction.  LDS_FLOATS: the operand images, or the
// waves' epilogue patches if larger; the kernels own the buffer, so a launch that mixes two configurations holds ONE of the larger.
template <int BM_, int BN_, int BK_, int KW_, bool A_RC, bool B_RC>
struct Tile {
    static constexpr int BM = BM_, BN = BN_, BK = BK_, KW = KW_;
    static constexpr int WGM = BM >= 64 ? 2 : 1, WGN = BN >= 64 ? 2 : 1, NW = WGM * WGN;   // wave grid of a k-group
    static constexpr int WM = BM / WGM, WN = BN / WGN;                                      // a wave's share of the tile
    static constexpr int FM = WM / 32, FN = WN / 32;                                        // 32x32 fragments per wave
    static constexpr int THREADS = 64 * NW * KW;
    typedef OperandTile<BM, BK, A_RC, THREADS> A;
    typedef OperandTile<BN, BK, B_RC, THREADS> B;
    // PREC == 1: both operands as [row][r] bf16 images (r-contiguous: one ds_read_b128 = the 8 k-values of a lane)
    static constexpr int LD16 = BK + 8;              // in bf16 elements: 16-B aligned rows, 36-dword stride at BK = 64
    static constexpr int PATCH = FM * FN * 16 * 64;  // a wave's accumulators, as the k-group reduction lays them out
    static constexpr int LDS_FLOATS = A::ELEMS + B::ELEMS > NW * EP_WAVE_FLOATS ? A::ELEMS + B::ELEMS : NW * EP_WAVE_FLOATS;
    static_assert((BK / KW) % 8 == 0, "tile too small for this many wave groups");
    static_assert(KW == 1 || (KW / 2) * NW * PATCH <= LDS_FLOATS, "LDS too small for the k-group reduction");
};

// ---- registers -> LDS image (stash); global -> registers (fetch) is written out in gemm_body ----
// the 4 values of a chunk as they go to a bf16 image, two packed dwords (plain integers: hipcc 7.2 miscompiles element extraction
// from a bf16 vector that is merged from two branches -- all four stores received element 0).  Stored as bf16: the bits go to the
// image unchanged, unless a row factor s applies.
template <bool S16, bool SCALED> __device__ __forceinline__ u32x2 chunk_bf16(const f32x4& v, const u32x2& raw, float s) {
    if constexpr (S16 && !SCALED) return raw;
    else if constexpr (S16) return __builtin_bit_cast(u32x2, __builtin_convertvector(widen_bf16x4(raw) * s, bf16x4));
    else if constexpr (SCALED) return __builtin_bit_cast(u32x2, __builtin_convertvector(v * s, bf16x4));
    else return __builtin_bit_cast(u32x2, __builtin_convertvector(v, bf16x4));
}
// A from a row(m)-contiguous source: transpose chunk c of reduction row `row` into the [m][r] bf16 image, four 16-bit stores
template <int LD16> __device__ __forceinline__ void store_a_transposed(unsigned short* img16, int c, int row, u32x2 h) {
    unsigned short* col = &img16[4 * c * LD16 + row];
    col[0] = (unsigned short)(h[0] & 0xffffu);
    col[LD16] = (unsigned short)(h[0] >> 16);
    col[2 * LD16] = (unsigned short)(h[1] & 0xffffu);
    col[3 * LD16] = (unsigned short)(h[1] >> 16);
}
// B whose source rows run along the REDUCTION index (data gradient: W[r][k]): keep them as they arrive, [r][BN] bf16 rows of
// 128 B, and let ds_read_b64_tr_b16 do the transpose when the fragments are read (main loop).  16-B chunks are XOR-swizzled with
// bit 1 of the row so that the 4-row x 16-column transposed reads of a 32-lane half fall into 64 distinct banks.
template <int BN> __device__ __forceinline__ void store_b_swizzled(unsigned short* img16, int c, int row, u32x2 h) {
    static_assert(BN == 64, "transposed-read B image is laid out for 64-column tiles");
    *reinterpret_cast<u32x2*>(&img16[row * BN + 8 * ((c >> 1) ^ (((row >> 1) & 1) << 2)) + 4 * (c & 1)]) = h;
}
// One operand's fetched chunks into its LDS image: the fp32 image (PREC 0), or the bf16 image (PREC 1): [row][r] for an
// r-contiguous operand, else A's transposed and B's swizzled one.  p16 / ps are not touched unless S16 / SCALED (B passes no ps).
template <class G, bool IS_A, int PREC, bool S16, bool SCALED, int LD16, int BN>
__device__ __forceinline__ void stash_operand(float* img, unsigned short* img16, int c, int r, const f32x4* p, const u32x2* p16, const float* ps) {
#pragma unroll
    for (int q = 0; q < G::Q; ++q) {
        const int row = r + q * G::RPP;
        float s = 1.0f;
        if constexpr (SCALED) s = ps[q];
        if constexpr (PREC == 1) {
            const u32x2 h = chunk_bf16<S16, SCALED>(p[q], p16[q], s);
            if constexpr (G::RC) *reinterpret_cast<u32x2*>(&img16[row * LD16 + 4 * c]) = h;
            else if constexpr (IS_A) store_a_transposed<LD16>(img16, c, row, h);
            else store_b_swizzled<BN>(img16, c, row, h);
        } else {
            f32x4 v = p[q];
            if constexpr (SCALED) v *= s;
            *reinterpret_cast<f32x4*>(&img[row * G::LD + 4 * c]) = v;
        }
    }
}
// ---- the kernel ----
// A weight gradient's sample mask (DropPath: a dropped sample's rows of row_scale . dy are exact zeros).  skip: nsamples per-sample
// floats, 0 = the sample adds nothing; its rows_per_sample rows of BOTH operands are then not read.  The workgroup reduces over the
// compacted index c in [0, nk * rows_per_sample) of the nk kept samples, shared out over the host's `splits` slabs:
//   j = c / rows_per_sample (magic: fdiv, bound checked by the host),  row = kept[j] * rows_per_sample + (c - j * rows_per_sample)
struct RowMask { const float* skip; int nsamples, rows_per_sample, splits; unsigned magic; };
constexpr int MASK_MAX_SAMPLES = 256;
// the ascending list of kept samples and their DropPath factors (1 without row_scale), in LDS beside the operand images
struct KeptList { int n; int idx[MASK_MAX_SAMPLES]; float scale[MASK_MAX_SAMPLES]; };

// The first wave lists the kept samples in ascending order (ballot + popcount); every workgroup builds the same list (gemm_body)
__device__ __forceinline__ void build_kept_list(KeptList* kept, const RowMask& mk, const float* row_scale) {
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid >= 64) return;
    int n = 0;
    for (int s0 = 0; s0 < mk.nsamples; s0 += 64) {
        const int s = s0 + lane;
        const bool keep = s < mk.nsamples && mk.skip[s] != 0.0f;
        const unsigned long long bal = __ballot(keep);
        if (keep) {
            const int at = n + __popcll(bal & ((1ull << lane) - 1ull));
            kept->idx[at] = s;
            kept->scale[at] = row_scale ? row_scale[s] : 1.0f;
        }
        n += __popcll(bal);
    }
    if (tid == 0) kept->n = n;
}

// A forward or data-gradient Linear's row map (DropPath: what a dropped sample's rows of the result hold does not depend on the A
// operand).  order: 1 + nsamples ints, [0] = nk, the number of kept samples, then the kept samples ascending, then the dropped
// ones ascending (drop_path_order_kernel below).  Logical row m of the launch stands for the physical row
//   j = m / rows_per_sample (magic: fdiv, bound checked by the host),  phys = order[1 + j] * rows_per_sample + (m - j * rows_per_sample)
// of A and of everything the epilogue addresses, so the kept samples' rows fill the first row tiles.  nk == nsamples: the identity,
// whatever the rest of `order` holds (the launch is then the unmapped one, bit for bit).
struct RowMap { const int* order; int nsamples, rows_per_sample; unsigned magic; };

// One wave per row r of the step's DropPath draws u (rows, B): scales[r][s] = (u < keep[r]) / keep[r], the factors as torch computes
// them from the same draws (one correctly rounded division), and order[r] as RowMap reads it.
__global__ __launch_bounds__(64) void drop_path_order_kernel(const float* __restrict__ u, const float* __restrict__ keep,
                                                             float* __restrict__ scales, int* __restrict__ order, int B) {
    const int r = blockIdx.x, lane = threadIdx.x;
    const float k = keep[r];
    const float* ur = u + (long)r * B;
    int* ord = order + (long)r * (B + 1);
    int nk = 0;
    for (int s0 = 0; s0 < B; s0 += 64) {
        const int s = s0 + lane;
        const bool kept = s < B && ur[s] < k;
        const unsigned long long bal = __ballot(kept);
        if (kept) ord[1 + nk + __popcll(bal & ((1ull << lane) - 1ull))] = s;
        if (s < B) scales[(long)r * B + s] = __fdiv_rn(kept ? 1.0f : 0.0f, k);
        nk += __popcll(bal);
    }
    if (lane == 0) ord[0] = nk;
    int nd = nk;
    for (int s0 = 0; s0 < B; s0 += 64) {
        const int s = s0 + lane;
        const bool dropped = s < B && !(ur[s] < k);
        const unsigned long long bal = __ballot(dropped);
        if (dropped) ord[1 + nd + __popcll(bal & ((1ull << lane) - 1ull))] = s;
        nd += __popcll(bal);
    }
}

// compile-time switch of the epilogue's early operand request (gemm_body: AHEAD), 0 = every launch keeps the loads behind its last MFMA
#ifndef CSWIN_EPI_AHEAD
#define CSWIN_EPI_AHEAD 1
#endif
constexpr bool EPI_AHEAD = CSWIN_EPI_AHEAD != 0;

// debug stamps (stamp_slot, bf16_tile.h)
__device__ __forceinline__ void stamp(const Epilogue& epi, int row, int slot) { stamp_slot(epi.stamps, row, slot); }

// T: the tile configuration.  SCALE_A: multiply the A rows by their Row::s (DropPath factor) when staging (weight gradients only).
// MASKED (weight gradients of plain matrices only): the reduction runs over the kept samples' rows (RowMask); a compile-time variant.
// MAPPED (forward / data-gradient Linears of plain fp32 matrices, one split): the launch's rows are LOGICAL rows (RowMap), the kept
// samples' first.  Row tiles past the kept rows are fill tiles: no k-loop, their zero accumulators go through the epilogue.  The live
// tiles are the launch's first workgroups and take the XCD order among themselves, so that a launch with dropped samples is a
// shorter launch of the same shape, not the same launch with idle CUs in one XCD.  ord: the samples in the launch's order, in LDS.
template <class T, int VEC, int EPI, bool SCALE_A, int PREC, class ASrc, class BSrc, bool MASKED = false, bool MAPPED = false>
__device__ __forceinline__ void gemm_body(float* lds, const ASrc& A, const BSrc& B, const Epilogue& epi, int M, int N, int R,
                                          int r_per_split, int tiles_m, int tiles_n, int bid, int nblk, int stamp_row,
                                          const RowMask* mk = nullptr, KeptList* kept = nullptr, const RowMap* rm = nullptr,
                                          int* ord = nullptr) {
    typedef typename T::A TA;
    typedef typename T::B TB;
    constexpr int BM = T::BM, BN = T::BN, BK = T::BK, KW = T::KW, NW = T::NW, FM = T::FM, FN = T::FN, LD16 = T::LD16;
    constexpr bool A_RC = TA::RC, B_RC = TB::RC;
    float* As = lds;
    float* Bs = lds + TA::ELEMS;
    unsigned short* As16 = reinterpret_cast<unsigned short*>(lds);
    unsigned short* Bs16 = As16 + BM * LD16;
    static_assert(PREC == 0 || ((BM + BN) * LD16 * 2 <= T::LDS_FLOATS * 4 && (BK / KW) % 16 == 0), "bf16 tile does not fit");

    const int tid = threadIdx.x, lane = tid & 63, wave = (tid >> 6) % NW, kg = tid / (64 * NW);
    const int li = lane & 31, lh = lane >> 5;
    bool mapped = false;                             // MAPPED: at least one sample is dropped (else the launch is the unmapped one)
    int kept_rows = M, nlive = nblk;                 // the kept samples' rows and the tiles that hold them
    if constexpr (MAPPED) {
        static_assert(A_RC && VEC == 4 && PREC == 0 && !MASKED && !SCALE_A && is_plain<ASrc> && is_plain<BSrc> && EPI != EPI_SPLIT2,
                      "the row map serves forward and data-gradient Linears of plain fp32 matrices");
        // the list goes to LDS while the kept count arrives (one load latency in front of the first operand loads, not two)
        for (int s = tid; s < rm->nsamples; s += T::THREADS) ord[s] = min(max(rm->order[1 + s], 0), rm->nsamples - 1);
        const int nk = __builtin_amdgcn_readfirstlane(rm->order[0]);
        mapped = nk < rm->nsamples;
        if (mapped) {
            kept_rows = max(nk, 0) * rm->rows_per_sample;
            nlive = (kept_rows + BM - 1) / BM * tiles_n;
        }
    }
    const int lb = (!MAPPED || bid < nlive) ? xcd_block_order(bid, nlive) : bid;       // logical blocks are ordered [split][m-tile][n-tile]
    const int tiles = tiles_m * tiles_n;
    const int split = lb / tiles;
    const int tile = lb - split * tiles;
    const int m0 = (tile / tiles_n) * BM, n0 = (tile % tiles_n) * BN;
    if constexpr (MAPPED) {
        if (mapped) __syncthreads();
    }
    if constexpr (MASKED) {
        static_assert(!A_RC && !B_RC && VEC == 4 && BM == BN && is_plain<ASrc> && is_plain<BSrc>,
                      "the sample mask serves weight gradients of plain matrices (one row mapping for both operands)");
        // From the kept list's length the split ranges: with S slabs, 8 * ceil(ceil(nk rps / S) / 8) rows each.  With every sample
        // kept that is the host's own r_per_split (choose_split makes rps from a count s >= S = ceil(M / rps): M / S <= rps, and
        // rps - 8 < M / s <= M / S leaves no smaller multiple of 8), so the launch then sums exactly what the unmasked does.
        build_kept_list(kept, *mk, src_row_scale(A));
        __syncthreads();
        R = __builtin_amdgcn_readfirstlane(kept->n) * mk->rows_per_sample;
        r_per_split = ((R + mk->splits - 1) / mk->splits + 7) / 8 * 8;
    }
    const int r_begin = split * r_per_split;
    const int r_end = (MAPPED && mapped && m0 >= kept_rows) ? r_begin : min(R, r_begin + r_per_split);     // a fill tile: no k-loop
    const int wm0 = (wave / T::WGN) * T::WM, wn0 = (wave % T::WGN) * T::WN;

    const int a_c = tid % TA::CPR, a_r = tid / TA::CPR;
    const int b_c = tid % TB::CPR, b_r = tid / TB::CPR;

    typename ASrc::Row arow[TA::Q];
    typename BSrc::Row brow[TB::Q];
    if (A_RC) {
#pragma unroll
        for (int q = 0; q < TA::Q; ++q) {
            if constexpr (MAPPED) {      // a dropped sample's rows (the mixed tile has some) are not read: a null row loads zeros
                const int m = m0 + a_r + q * TA::RPP;
                int row = -1;
                if (mapped && m < kept_rows) {
                    const int j = fdiv1(m, rm->magic);
                    row = ord[j] * rm->rows_per_sample + (m - j * rm->rows_per_sample);
                }
                arow[q] = mapped ? src_mapped_row(A, row, 1.0f) : A.row(m);
            } else {
                arow[q] = A.row(m0 + a_r + q * TA::RPP);
            }
        }
    }
    if (B_RC) {
#pragma unroll
        for (int q = 0; q < TB::Q; ++q) brow[q] = B.row(n0 + b_r + q * TB::RPP);
    }

    // An operand that is not r-contiguous keeps its column (the output index m0 / n0 + 4 * chunk) through the whole reduction: a
    // gather source splits it into (tap, channel) once, here, not per tile (16-B loaders; the scalar ones serve plain matrices only)
    const typename ASrc::Col acol = A.col(m0 + 4 * a_c);
    const typename BSrc::Col bcol = B.col(n0 + 4 * b_c);

    // register prefetch of the next tile: raw loads only -- nothing may consume pa/pb before stash(), or the
    // compiler waits for the loads in front of the MFMA section
    f32x4 pa[TA::Q], pb[TB::Q];
    u32x2 pa16[TA::Q], pb16[TB::Q];                  // an operand stored as bf16: its raw chunks (pa / pb is then unused)
    float pas[TA::Q];
    // a16 (std::true_type / false_type): A is STORED as bf16.  A compile-time copy of the main loop per storage type: a run-time
    // choice between the 8-B and the 16-B load inside fetch() splits it into basic blocks and the loads end up waiting for one another.
    // A and B stay written out here, and the ladder below: helpers cost time (profiles/gemm_body_notes.md).
    auto fetch = [&](int r0, auto a16, auto b16) {
        int mrow[TA::Q];                                 // MASKED: the rows of this thread's chunks (both operands'), < 0 past the end
        float msc[TA::Q];
        if constexpr (MASKED) {
#pragma unroll
            for (int q = 0; q < TA::Q; ++q) {
                const int c = r0 + a_r + q * TA::RPP;
                mrow[q] = -1;
                msc[q] = 1.0f;
                if (c < r_end) {
                    const int j = fdiv1(c, mk->magic);
                    mrow[q] = kept->idx[j] * mk->rows_per_sample + (c - j * mk->rows_per_sample);
                    msc[q] = kept->scale[j];
                }
            }
        }
#pragma unroll
        for (int q = 0; q < TA::Q; ++q) {
            typename ASrc::Row rr;
            int j;
            if (A_RC) {
                rr = arow[q];
                j = r0 + 4 * a_c;
            } else {
                const int r = r0 + a_r + q * TA::RPP;
                if constexpr (MASKED) rr = src_mapped_row(A, mrow[q], msc[q]);
                else rr = A.row(r < r_end ? r : 0x7fffffff);
                j = m0 + 4 * a_c;
            }
            if (SCALE_A) pas[q] = rr.s;
            if (VEC == 4) {
                const float* p = A_RC ? (j < r_end ? A.ptr(rr, A.col(j)) : nullptr) : A.ptr(rr, acol);
                if constexpr (decltype(a16)::value) {
                    pa16[q] = u32x2{0u, 0u};
                    if (p) pa16[q] = src_load4_bf16(A, p);
                } else {
                    pa[q] = f32x4{0.f, 0.f, 0.f, 0.f};
                    if (p) pa[q] = *reinterpret_cast<const f32x4*>(p);
                }
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float* p = (!A_RC || j + e < r_end) ? A.ptr(rr, A.col(j + e)) : nullptr;
                    pa[q][e] = p ? *p : 0.f;
                }
            }
        }
#pragma unroll
        for (int q = 0; q < TB::Q; ++q) {
            typename BSrc::Row rr;
            int j;
            if (B_RC) {
                rr = brow[q];
                j = r0 + 4 * b_c;
            } else {
                const int r = r0 + b_r + q * TB::RPP;
                if constexpr (MASKED) rr = src_mapped_row(B, mrow[q], 1.0f);
                else rr = B.row(r < r_end ? r : 0x7fffffff);
                j = n0 + 4 * b_c;
            }
            if (VEC == 4) {
                const float* p = B_RC ? (j < r_end ? B.ptr(rr, B.col(j)) : nullptr) : B.ptr(rr, bcol);
                if constexpr (decltype(b16)::value) {
                    pb16[q] = u32x2{0u, 0u};
                    if (p) pb16[q] = src_load4_bf16(B, p);
                } else {
                    pb[q] = f32x4{0.f, 0.f, 0.f, 0.f};
                    if (p) pb[q] = *reinterpret_cast<const f32x4*>(p);
                }
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float* p = (!B_RC || j + e < r_end) ? B.ptr(rr, B.col(j + e)) : nullptr;
                    pb[q][e] = p ? *p : 0.f;
                }
            }
        }
    };
    auto stash = [&](auto a16, auto b16) {
        stash_operand<TA, true, PREC, decltype(a16)::value, SCALE_A, LD16, BN>(As, As16, a_c, a_r, pa, pa16, pas);
        stash_operand<TB, false, PREC, decltype(b16)::value, false, LD16, BN>(Bs, Bs16, b_c, b_r, pb, pb16, nullptr);
    };

    f32x16 acc[FM][FN];
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    float csum = 0.f;   // dbias partial (TN, A row-contiguous image: column tid of the A tile)
    const bool do_colsum = !A_RC && epi.colsum && n0 == 0 && tid < BM;

    // AHEAD: the operands of the wave's first epilogue fragment (bias, row factors, residual / gelu_pre chunks; MAPPED: through ord) are
    // requested where the last k-tile would fetch its successor, in front of that tile's MFMAs, not behind them.  A workgroup with one
    // k-tile requests before its only tile, a fill tile (no k-loop) before its epilogue.  Forward and data-gradient launches with 16-B
    // loaders in fp32; the weight gradients' plain epilogue has nothing to request.  Per instantiation, by the kernel traces and the
    // register table of profiles/gemm_edges_notes.md: the residual and GELU' epilogues, every data gradient and the forward launches
    // of the concat and gather sources take it; a plain matrix's forward whose epilogue has a bias alone to fetch keeps the old form
    // (measured 0 to 1.7 us slower per launch), and so does every kernel of four k-groups (the residual forward 4.8 us slower; the
    // concat and gather sources' would go from 8 to 7 waves per SIMD, one resident workgroup of 16 waves instead of two).
    constexpr bool AHEAD = EPI_AHEAD && A_RC && VEC == 4 && PREC == 0 && KW != 4 &&
                           (EPI == EPI_RES || EPI == EPI_GELUBWD || !B_RC || !is_plain<ASrc>);
    EpiOperands eq;
    auto request = [&]() {
        if (KW > 1 && kg != 0) return;               // the k-groups that leave before the epilogue
        const int mf = m0 + wm0, nf = n0 + wn0;
        if constexpr (MAPPED) {
            epilogue_request<EPI, false, true>(eq, epi, M, N, mf, nf, lane, mapped ? ord : nullptr, kept_rows, rm->rows_per_sample, rm->magic);
        } else {
            if (!epi.vec_store) return;              // the scalar path loads where it computes
            if (EPI == EPI_GELUBWD && epi.pre_bf16) epilogue_request<EPI, true, false>(eq, epi, M, N, mf, nf, lane);
            else epilogue_request<EPI, false, false>(eq, epi, M, N, mf, nf, lane);
        }
    };

    // one k-tile's MFMAs as the AHEAD launches run them (fp32, r-contiguous A): the k-loop's fp32 section below, for these alone
    auto mma_tile = [&]() {
#pragma unroll
        for (int kk = kg * (BK / KW); kk < (kg + 1) * (BK / KW); kk += 8) {
            f32x4 af[FM], bf[FN];
#pragma unroll
            for (int i = 0; i < FM; ++i) af[i] = *reinterpret_cast<const f32x4*>(&As[(wm0 + i * 32 + li) * TA::LD + kk + 4 * lh]);
#pragma unroll
            for (int j = 0; j < FN; ++j) {
                if (B_RC) {
                    bf[j] = *reinterpret_cast<const f32x4*>(&Bs[(wn0 + j * 32 + li) * TB::LD + kk + 4 * lh]);
                } else {
#pragma unroll
                    for (int s = 0; s < 4; ++s) bf[j][s] = Bs[(kk + 4 * lh + s) * TB::LD + wn0 + j * 32 + li];
                }
            }
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int i = 0; i < FM; ++i)
#pragma unroll
                    for (int j = 0; j < FN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i][s], bf[j][s], acc[i][j], 0, 0, 0);
        }
    };

    stamp(epi, stamp_row, 0);
    auto main_loop = [&](auto a16, auto b16) {
        fetch(r_begin, a16, b16);
        stash(a16, b16);
        __syncthreads();
        stamp(epi, stamp_row, 1);
        if constexpr (AHEAD) {
            // the last tile stands outside the loop, so that the epilogue's operands are held through that tile alone, where the
            // prefetch registers are free, not through the loop
            for (int r0 = r_begin; r0 + BK < r_end; r0 += BK) {
                fetch(r0 + BK, a16, b16);
                mma_tile();
                __syncthreads();
                stash(a16, b16);
                __syncthreads();
            }
            request();
            mma_tile();
            __syncthreads();
            return;
        }
        for (int r0 = r_begin; r0 < r_end; r0 += BK) {
            const bool more = r0 + BK < r_end;
            if (more) fetch(r0 + BK, a16, b16);
            if (do_colsum) {
                if constexpr (PREC == 1) {
#pragma unroll 8
                    for (int r = 0; r < BK; ++r)
                        csum += widen_bf16(As16[tid * LD16 + r]);
                } else {
#pragma unroll 8
                    for (int r = 0; r < BK; ++r) csum += As[r * TA::LD + tid];
                }
            }
            if constexpr (PREC == 1) {
#pragma unroll
                for (int kk = kg * (BK / KW); kk < (kg + 1) * (BK / KW); kk += 16) {
                    bf16x8 af[FM], bf[FN];
#pragma unroll
                    for (int i = 0; i < FM; ++i)
                        af[i] = *reinterpret_cast<const bf16x8*>(&As16[(wm0 + i * 32 + li) * LD16 + kk + 8 * lh]);
#pragma unroll
                    for (int j = 0; j < FN; ++j) {
                        if constexpr (B_RC) {
                            bf[j] = *reinterpret_cast<const bf16x8*>(&Bs16[(wn0 + j * 32 + li) * LD16 + kk + 8 * lh]);
                        } else {
                            // the 8 reduction values of this lane's column (tr16_frag, bf16_tile.h)
                            const int col = wn0 + j * 32 + 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
                            const int row = kk + 8 * lh + ((lane & 15) >> 2);
                            const int sw = ((row >> 1) & 1) << 2;               // rows row and row + 4 share bit 1
                            const unsigned short* a0 = &Bs16[row * BN + 8 * ((col >> 3) ^ sw) + (col & 7)];
                            bf[j] = tr16_frag(a0, a0 + 4 * BN);
                        }
                    }
#pragma unroll
                    for (int i = 0; i < FM; ++i)
#pragma unroll
                        for (int j = 0; j < FN; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bf[j], acc[i][j], 0, 0, 0);
                }
            } else
#pragma unroll
            for (int kk = kg * (BK / KW); kk < (kg + 1) * (BK / KW); kk += 8) {
                // one b128 from an r-contiguous image, four b32 from a row-contiguous one; written out per operand: through a
                // helper the b32 reads come out paired (ds_read2_b32), not the parent's listing (profiles/gemm_body_notes.md)
                f32x4 af[FM], bf[FN];
#pragma unroll
                for (int i = 0; i < FM; ++i) {
                    if (A_RC) {
                        af[i] = *reinterpret_cast<const f32x4*>(&As[(wm0 + i * 32 + li) * TA::LD + kk + 4 * lh]);
                    } else {
#pragma unroll
                        for (int s = 0; s < 4; ++s) af[i][s] = As[(kk + 4 * lh + s) * TA::LD + wm0 + i * 32 + li];
                    }
                }
#pragma unroll
                for (int j = 0; j < FN; ++j) {
                    if (B_RC) {
                        bf[j] = *reinterpret_cast<const f32x4*>(&Bs[(wn0 + j * 32 + li) * TB::LD + kk + 4 * lh]);
                    } else {
#pragma unroll
                        for (int s = 0; s < 4; ++s) bf[j][s] = Bs[(kk + 4 * lh + s) * TB::LD + wn0 + j * 32 + li];
                    }
                }
#pragma unroll
                for (int s = 0; s < 4; ++s)
#pragma unroll
                    for (int i = 0; i < FM; ++i)
#pragma unroll
                        for (int j = 0; j < FN; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i][s], bf[j][s], acc[i][j], 0, 0, 0);
            }
            __syncthreads();
            if (more) {
                stash(a16, b16);
                __syncthreads();
            }
        }
    };
    if (r_begin < r_end) {
        // storage variants (bf16 mode, forward / data-gradient Linears only): A (activations) and / or B (the weights' bf16 shadow)
        constexpr bool CAN_A16 = PREC == 1 && A_RC && VEC == 4 && is_plain<ASrc>;
        constexpr bool CAN_B16 = PREC == 1 && A_RC && VEC == 4 && is_plain<BSrc>;
        const bool a_is16 = CAN_A16 && src_is_bf16(A), b_is16 = CAN_B16 && src_is_bf16(B);
        if constexpr (CAN_A16 && CAN_B16) {
            if (a_is16 && b_is16) main_loop(std::true_type{}, std::true_type{});
            else if (a_is16) main_loop(std::true_type{}, std::false_type{});
            else if (b_is16) main_loop(std::false_type{}, std::true_type{});
            else main_loop(std::false_type{}, std::false_type{});
        } else if constexpr (CAN_B16) {
            if (b_is16) main_loop(std::false_type{}, std::true_type{});
            else main_loop(std::false_type{}, std::false_type{});
        } else {
            main_loop(std::false_type{}, std::false_type{});
        }
    } else if constexpr (AHEAD) {
        request();
    }

    stamp(epi, stamp_row, 2);
    if (KW > 1) {
        // Sum the wave groups' accumulators into group 0's (native C/D layout, lane-contiguous LDS patches, binary tree).  In
        // place: as a function the KW = 4 kernels' first stores come out paired, not the parent's listing (profiles/gemm_body_notes.md)
#pragma unroll
        for (int half = KW / 2; half >= 1; half >>= 1) {
            if (kg >= half && kg < 2 * half) {
                float* dst = lds + ((kg - half) * NW + wave) * T::PATCH + lane;
#pragma unroll
                for (int i = 0; i < FM; ++i)
#pragma unroll
                    for (int j = 0; j < FN; ++j)
#pragma unroll
                        for (int g = 0; g < 16; ++g) dst[((i * FN + j) * 16 + g) * 64] = acc[i][j][g];
            }
            __syncthreads();
            if (kg < half) {
                const float* src = lds + (kg * NW + wave) * T::PATCH + lane;
#pragma unroll
                for (int i = 0; i < FM; ++i)
#pragma unroll
                    for (int j = 0; j < FN; ++j)
#pragma unroll
                        for (int g = 0; g < 16; ++g) acc[i][j][g] += src[((i * FN + j) * 16 + g) * 64];
            }
            __syncthreads();
        }
        if (kg != 0) return;
    }
    Epilogue e = epi;
    e.C += (long)split * e.split_stride;
    if constexpr (MAPPED) {
        run_epilogue<EPI, FM, FN, false, false, true, AHEAD>(e, acc, M, N, m0 + wm0, n0 + wn0, lane, lds + wave * EP_WAVE_FLOATS, true, 0, 0,
                                                             mapped ? ord : nullptr, kept_rows, rm->rows_per_sample, rm->magic, &eq);
    } else if constexpr (EPI == EPI_GELUBWD) {
        if (e.pre_bf16)
            run_epilogue<EPI, FM, FN, true, false, false, AHEAD>(e, acc, M, N, m0 + wm0, n0 + wn0, lane, lds + wave * EP_WAVE_FLOATS, e.vec_store != 0, 0, 0,
                                                                 nullptr, 0, 1, 0, &eq);
        else
            run_epilogue<EPI, FM, FN, false, false, false, AHEAD>(e, acc, M, N, m0 + wm0, n0 + wn0, lane, lds + wave * EP_WAVE_FLOATS, e.vec_store != 0, 0, 0,
                                                                  nullptr, 0, 1, 0, &eq);
    } else {
        // a FAST gather source brings the reciprocals of its own row split, which is the epilogue's (rm_on: the parity classes)
        if constexpr (ASrc::fast_div)
            run_epilogue<EPI, FM, FN, false, true, false, AHEAD>(e, acc, M, N, m0 + wm0, n0 + wn0, lane, lds + wave * EP_WAVE_FLOATS, e.vec_store != 0, A.m.img,
                                                                 A.m.w, nullptr, 0, 1, 0, &eq);
        else
            run_epilogue<EPI, FM, FN, false, false, false, AHEAD>(e, acc, M, N, m0 + wm0, n0 + wn0, lane, lds + wave * EP_WAVE_FLOATS, e.vec_store != 0, 0, 0,
                                                                  nullptr, 0, 1, 0, &eq);
    }
    stamp(epi, stamp_row, 3);
    if (do_colsum && m0 + tid < M) epi.colsum[(long)split * epi.colsum_stride + m0 + tid] = csum;
}

template <int BM, int BN, int BK, int KW, bool A_RC, bool B_RC, int VEC, int EPI, bool SCALE_A, int PREC, class ASrc, class BSrc>
__global__ __launch_bounds__((Tile<BM, BN, BK, KW, A_RC, B_RC>::THREADS)) void gemm_kernel(ASrc A, BSrc B, Epilogue epi, int M, int N, int R,
                                                    int r_per_split, int tiles_m, int tiles_n) {
    typedef Tile<BM, BN, BK, KW, A_RC, B_RC> T;
    __shared__ __attribute__((aligned(16))) float lds[T::LDS_FLOATS];
    gemm_body<T, VEC, EPI, SCALE_A, PREC, ASrc, BSrc>(lds, A, B, epi, M, N, R, r_per_split, tiles_m, tiles_n, (int)blockIdx.x, (int)gridDim.x,
                                                      (int)blockIdx.x);
}

// the same launch with a row map (16-B loaders, fp32, plain matrices: see gemm_body)
template <int BM, int BN, int BK, int KW, bool B_RC, int EPI>
__global__ __launch_bounds__((Tile<BM, BN, BK, KW, true, B_RC>::THREADS)) void gemm_mapped_kernel(PlainSrc A, PlainSrc B, Epilogue epi, int M, int N, int R,
                                                    int r_per_split, int tiles_m, int tiles_n, RowMap rm) {
    typedef Tile<BM, BN, BK, KW, true, B_RC> T;
    __shared__ __attribute__((aligned(16))) float lds[T::LDS_FLOATS];
    __shared__ int ord[MASK_MAX_SAMPLES];
    gemm_body<T, 4, EPI, false, 0, PlainSrc, PlainSrc, false, true>(lds, A, B, epi, M, N, R, r_per_split, tiles_m, tiles_n, (int)blockIdx.x,
                                                                    (int)gridDim.x, (int)blockIdx.x, nullptr, nullptr, &rm, ord);
}

// Up to four independent problems of one kernel configuration in ONE launch (the weight gradients of the four Linears of a
// CSWinBlock: operands all alive at the end of the block's backward): an empty launch costs ~3 us in-stream, and the four grids'
// tails fill each other.  Each problem keeps its own XCD-aware block order inside its block range.
constexpr int WGRAD_BATCH = gp::WGRAD_BATCH;
template <class ASrc, class BSrc>
struct GemmBatch {
    ASrc A[WGRAD_BATCH];
    BSrc B[WGRAD_BATCH];
    Epilogue e[WGRAD_BATCH];
    int M[WGRAD_BATCH], N[WGRAD_BATCH], R[WGRAD_BATCH], rps[WGRAD_BATCH], tm[WGRAD_BATCH], tn[WGRAD_BATCH];
    int first[WGRAD_BATCH + 1];
    int n;
    RowMask mask[WGRAD_BATCH];   // weight-gradient batches only, read by the *_masked kernels only (skip == NULL: problem without a mask)
};
typedef GemmBatch<PlainSrc, PlainSrc> WgradBatch;

// the problem whose block range holds workgroup bid
template <class ASrc, class BSrc> __device__ __forceinline__ int batch_problem(const GemmBatch<ASrc, BSrc>& b, int bid) {
    int p = 0;
    while (p + 1 < b.n && bid >= b.first[p + 1]) ++p;
    return p;
}
// workgroup bid of the launch as a workgroup of problem p (16-B loaders, plain epilogue; MASKED: with the problem's sample mask)
template <class T, bool SCALE_A, int PREC, bool MASKED = false, class ASrc, class BSrc>
__device__ __forceinline__ void batch_body(float* lds, const GemmBatch<ASrc, BSrc>& b, int p, int bid, KeptList* kept = nullptr) {
    gemm_body<T, 4, EPI_PLAIN, SCALE_A, PREC, ASrc, BSrc, MASKED>(lds, b.A[p], b.B[p], b.e[p], b.M[p], b.N[p], b.R[p], b.rps[p], b.tm[p], b.tn[p],
                                                                  bid - b.first[p], b.first[p + 1] - b.first[p], bid, MASKED ? &b.mask[p] : nullptr, kept);
}

typedef Tile<64, 64, 64, 2, false, false> WgradTile;   // the weight gradients' configuration: two k-groups of four waves
// Workgroup bid of a weight-gradient batch.  MASKED: a problem of the launch with a sample mask takes the masked form of the body.
template <int PREC, bool MASKED>
__device__ __forceinline__ void wgrad_batch_body(float* lds, KeptList* kept, const WgradBatch& b, int bid) {
    const int p = batch_problem(b, bid);
    if constexpr (MASKED) {
        if (b.mask[p].skip) return batch_body<WgradTile, true, PREC, true>(lds, b, p, bid, kept);
    }
    batch_body<WgradTile, true, PREC>(lds, b, p, bid);
}

template <int PREC>
__global__ __launch_bounds__(WgradTile::THREADS) void gemm_wgrad_batch_kernel(WgradBatch b) {
    __shared__ __attribute__((aligned(16))) float lds[WgradTile::LDS_FLOATS];
    wgrad_batch_body<PREC, false>(lds, nullptr, b, (int)blockIdx.x);
}
__global__ __launch_bounds__(WgradTile::THREADS) void gemm_wgrad_batch_masked_kernel(WgradBatch b) {
    __shared__ __attribute__((aligned(16))) float lds[WgradTile::LDS_FLOATS];
    __shared__ KeptList kept;
    wgrad_batch_body<0, true>(lds, &kept, b, (int)blockIdx.x);
}

// The tail of a CSWinBlock's backward in ONE launch: the data gradient of the qkv Linear (dqkv . Wqkv, the last Linear whose input
// gradient is still missing) beside the block's four weight gradients.  Both only wait for dqkv, neither depends on the other, and
// alone the data gradient keeps the matrix pipe busy a third of the time (profiles/round3_sq_counters_fp32.txt: 0.34 against the
// batch's 0.50): in one launch its tiles' load waits, prologues and epilogues sit beside the weight gradients' long k-loops.
// Workgroups [0, nd) are the data gradient's 64 x 64 tiles (two k-groups of four waves, as the weight-gradient workgroups).
struct BlockTail {
    PlainSrc dA, dB;
    Epilogue de;
    int dM, dN, dR, drps, dtm, dtn, nd;
    WgradBatch w;
    ReduceRiders r;          // pending slab reductions of EARLIER launches (the previous block's): the grid's last workgroups
};
typedef Tile<64, 64, 64, 2, true, false> TailDgradTile;
static_assert(TailDgradTile::THREADS == WgradTile::THREADS, "one workgroup size for both halves of the block tail");
constexpr int BLOCK_TAIL_LDS = TailDgradTile::LDS_FLOATS > WgradTile::LDS_FLOATS ? TailDgradTile::LDS_FLOATS : WgradTile::LDS_FLOATS;
template <bool MASKED, bool MAPPED = false>
__device__ __forceinline__ void block_tail_body(float (&lds)[BLOCK_TAIL_LDS], KeptList* kept, const BlockTail& t, const RowMap* rm = nullptr,
                                                int* ord = nullptr) {
    const int bid = (int)blockIdx.x, nw = t.w.first[t.w.n];
    if (bid >= nw + t.nd) {                // riders: 256-thread reduction workgroups (the upper four waves leave)
        if (threadIdx.x >= 256) return;
        static_assert(sizeof(lds) >= sizeof(float) * RS_G * (RS_COLS + 1), "reduction scratch");
        rows_sum_dispatch(t.r.j, t.r.first_block, t.r.njobs, bid - nw - t.nd, reinterpret_cast<float(*)[RS_COLS + 1]>(lds));
        return;
    }
    if (bid >= nw) {                       // the data gradient's tiles come after the weight gradients': they fill their tail
        if constexpr (MAPPED)
            gemm_body<TailDgradTile, 4, EPI_PLAIN, false, 0, PlainSrc, PlainSrc, false, true>(lds, t.dA, t.dB, t.de, t.dM, t.dN, t.dR, t.drps, t.dtm,
                                                                                              t.dtn, bid - nw, t.nd, bid, nullptr, nullptr, rm, ord);
        else
            gemm_body<TailDgradTile, 4, EPI_PLAIN, false, 0, PlainSrc, PlainSrc>(lds, t.dA, t.dB, t.de, t.dM, t.dN, t.dR, t.drps, t.dtm, t.dtn, bid - nw,
                                                                                 t.nd, bid);
        return;
    }
    wgrad_batch_body<0, MASKED>(lds, kept, t.w, bid);
}
__global__ __launch_bounds__(WgradTile::THREADS) void gemm_block_tail_kernel(BlockTail t) {
    __shared__ __attribute__((aligned(16))) float lds[BLOCK_TAIL_LDS];
    block_tail_body<false>(lds, nullptr, t);
}
// the same launch with a sample mask on at least one of its weight gradients
__global__ __launch_bounds__(WgradTile::THREADS) void gemm_block_tail_masked_kernel(BlockTail t) {
    __shared__ __attribute__((aligned(16))) float lds[BLOCK_TAIL_LDS];
    __shared__ KeptList kept;
    block_tail_body<true>(lds, &kept, t);
}
// the masked launch whose data gradient takes a row map (the BlockTail block itself is the other two kernels')
__global__ __launch_bounds__(WgradTile::THREADS) void gemm_block_tail_skip_kernel(BlockTail t, RowMap rm) {
    __shared__ __attribute__((aligned(16))) float lds[BLOCK_TAIL_LDS];
    __shared__ KeptList kept;
    __shared__ int ord[MASK_MAX_SAMPLES];
    block_tail_body<true, true>(lds, &kept, t, &rm, ord);
}

// The four parity classes of a stride-2 3x3 convolution's data gradient (ConvTS2SrcT) are independent GEMMs over a quarter of
// the pixels each: alone they fill 1.1 - 1.2 workgroups per CU (the launch ends with the CUs that got two); together 4.6.
template <int KW> using S2DgradTile = Tile<64, 64, (KW == 1 ? 32 : 64), KW, true, false>;
template <int KW, int PREC, bool FAST>
__global__ __launch_bounds__(S2DgradTile<KW>::THREADS) void gemm_conv_s2_dgrad_batch_kernel(GemmBatch<ConvTS2SrcT<FAST>, TapRowsSrcT<FAST>> b) {
    __shared__ __attribute__((aligned(16))) float lds[S2DgradTile<KW>::LDS_FLOATS];
    batch_body<S2DgradTile<KW>, false, PREC>(lds, b, batch_problem(b, (int)blockIdx.x), (int)blockIdx.x);
}

// ======================================================================================
// host side: the launches of what gemm_plan.h decides (tile, k-groups, widths, splits, routes), then the C ABI
// ======================================================================================
using gp::one_split;

template <int BM, int BN, int BK, int KW, bool A_RC, bool B_RC, int VEC, int EPI, bool SCALE_A, int PREC, class ASrc, class BSrc>
void launch_cfg(const ASrc& A, const BSrc& B, const Epilogue& epi, int M, int N, int R, int splits, int r_per_split,
                hipStream_t st, const RowMap* rm = nullptr) {
    int tm = cdiv(M, BM), tn = cdiv(N, BN);
    dim3 grid(tm * tn * splits);
    const int pad_lds = cswin_tuning().gemm_pad_lds;                                                    // tuning aid: caps residency
    // rm: the launch's row-mapped form (the callers pass one only with what gemm_mapped_kernel is made for)
    if constexpr (A_RC && VEC == 4 && PREC == 0 && !SCALE_A && is_plain<ASrc> && is_plain<BSrc> && EPI != EPI_SPLIT2 && (B_RC || EPI != EPI_RES)) {
        if (rm) {
            hipLaunchKernelGGL((gemm_mapped_kernel<BM, BN, BK, KW, B_RC, EPI>), grid, dim3((Tile<BM, BN, BK, KW, A_RC, B_RC>::THREADS)), pad_lds, st, A, B,
                               epi, M, N, R, r_per_split, tm, tn, *rm);
            return;
        }
    }
    hipLaunchKernelGGL((gemm_kernel<BM, BN, BK, KW, A_RC, B_RC, VEC, EPI, SCALE_A, PREC, ASrc, BSrc>), grid, dim3((Tile<BM, BN, BK, KW, A_RC, B_RC>::THREADS)), pad_lds, st, A, B, epi,
                       M, N, R, r_per_split, tm, tn);
}

// The launch of a plan of the tiled family (gp::tiled_plan) at the loader width VEC: the plan's tile, k-tile, wave groups, split and
// epilogue width.  These seven configurations are all the family has.
template <bool A_RC, bool B_RC, int VEC, int EPI, bool SCALE_A, class ASrc, class BSrc>
void launch_gemm(const gp::Plan& p, const ASrc& A, const BSrc& B, const Epilogue& epi_in, int M, int N, int R, int precision,
                 hipStream_t st, const RowMap* rm = nullptr) {
    Epilogue epi = epi_in;
    epi.vec_store = p.store == 4;
    if (precision == 1) {
        if (p.kw == 2) launch_cfg<64, 64, 64, 2, A_RC, B_RC, VEC, EPI, SCALE_A, 1>(A, B, epi, M, N, R, p.splits, p.rows, st);
        else launch_cfg<64, 64, 64, 1, A_RC, B_RC, VEC, EPI, SCALE_A, 1>(A, B, epi, M, N, R, p.splits, p.rows, st);
        return;
    }
    if (p.bn == 32) {
        if (p.kw == 2) return launch_cfg<64, 32, 64, 2, A_RC, B_RC, VEC, EPI, SCALE_A, 0>(A, B, epi, M, N, R, p.splits, p.rows, st, rm);
        return launch_cfg<64, 32, 32, 1, A_RC, B_RC, VEC, EPI, SCALE_A, 0>(A, B, epi, M, N, R, p.splits, p.rows, st, rm);
    }
    if (p.kw == 4) launch_cfg<64, 64, 64, 4, A_RC, B_RC, VEC, EPI, SCALE_A, 0>(A, B, epi, M, N, R, p.splits, p.rows, st, rm);
    else if (p.kw == 2) launch_cfg<64, 64, 64, 2, A_RC, B_RC, VEC, EPI, SCALE_A, 0>(A, B, epi, M, N, R, p.splits, p.rows, st, rm);
    else launch_cfg<64, 64, 32, 1, A_RC, B_RC, VEC, EPI, SCALE_A, 0>(A, B, epi, M, N, R, p.splits, p.rows, st, rm);
}

// launch_gemm at the plan's loader width (a row map only goes with 16-B loads: the entry points refuse it otherwise)
template <bool A_RC, bool B_RC, int EPI, bool SCALE_A, class ASrc, class BSrc>
void launch_gemm_vec(const gp::Plan& p, const ASrc& A, const BSrc& B, const Epilogue& epi, int M, int N, int R, int precision,
                     hipStream_t st, const RowMap* rm = nullptr) {
    if (p.vec == 4) launch_gemm<A_RC, B_RC, 4, EPI, SCALE_A>(p, A, B, epi, M, N, R, precision, st, rm);
    else launch_gemm<A_RC, B_RC, 1, EPI, SCALE_A>(p, A, B, epi, M, N, R, precision, st);
}

// launch_gemm_vec at the epilogue mode epi_mode, one of EPIS: the modes the caller's forms can take (each is its own set of kernels)
template <bool A_RC, bool B_RC, int... EPIS, class ASrc, class BSrc>
void launch_gemm_epi(int epi_mode, const gp::Plan& p, const ASrc& A, const BSrc& B, const Epilogue& epi, int M, int N, int R,
                     int precision, hipStream_t st, const RowMap* rm = nullptr) {
    ((epi_mode == EPIS ? launch_gemm_vec<A_RC, B_RC, EPIS, false>(p, A, B, epi, M, N, R, precision, st, rm) : (void)0), ...);
}

// the plan of a launch with 16-B loaders whose reduction is one split (the convolutions' forward and data gradient)
gp::Plan one_split_plan(const Epilogue& e, int M, int N, int R, int precision) {
    return gp::tiled_plan(cswin_tuning(), M, N, R, 1, one_split(R), false, precision, true, epilogue_vec_ok(e, N));
}

long long* g_stamps = nullptr;     // debug only (cswin_debug_set_stamps)

Epilogue plain_epilogue(float* C, long ldc) {
    Epilogue e = {};
    e.C = C;
    e.ldc = ldc;
    e.stamps = g_stamps;
    return e;
}

// problem (A, B, e) with M x N outputs and a reduction of R in `splits` slices of rps as the next slot of a batch; its 64 x 64
// tiles take the next workgroups (first[b.n] is the launch's workgroup count so far).  vec_store: its epilogue's 16-B accesses are legal
template <class ASrc, class BSrc>
void push(GemmBatch<ASrc, BSrc>& b, const ASrc& A, const BSrc& B, Epilogue e, int M, int N, int R, int rps, int splits, bool vec_store) {
    const int i = b.n++;
    e.vec_store = vec_store;
    b.A[i] = A; b.B[i] = B; b.e[i] = e;
    b.M[i] = M; b.N[i] = N; b.R[i] = R; b.rps[i] = rps;
    b.tm[i] = cdiv(M, 64); b.tn[i] = cdiv(N, 64);
    b.first[i + 1] = b.first[i] + b.tm[i] * b.tn[i] * splits;
}

// The workspace of a split-M weight gradient dw[N,K] (+ dbias[N]): slab s = [dw partial (N*K) | dbias partial (N)], the slabs
// gp::slab_stride(N, K) apart, so that one reduction launch serves both.  The GEMM's epilogue writes the slabs, the job sums them.
// (Its size is gp::wgrad_workspace_bytes.)
struct WgradSlabs {
    float* base; long stride; int N, K;
    WgradSlabs(void* workspace, int N_, int K_) : base((float*)workspace), stride(gp::slab_stride(N_, K_)), N(N_), K(K_) {}
    Epilogue epilogue(bool with_dbias) const {
        Epilogue e = plain_epilogue(base, K);
        e.split_stride = stride;
        e.colsum = with_dbias ? base + (long)N * K : nullptr;
        e.colsum_stride = (int)stride;
        return e;
    }
    // conv_kk / conv_cin: a convolution's dw goes to the nn.Conv2d layout (see cswin_reduce_job)
    cswin_reduce_job job(float* dw, float* dbias, int splits, int conv_kk = 0, int conv_cin = 0) const {
        const long nk = (long)N * K;
        return cswin_reduce_job{base, dw, dbias, nk, nk + (dbias ? N : 0), stride, splits, 0, conv_kk, conv_cin};
    }
};

bool reduce_jobs_ok(const cswin_reduce_job* jobs, int njobs) {
    for (int i = 0; i < njobs; ++i)
        if (!reduce_job_ok(jobs[i])) return false;
    return true;
}

// one launch for njobs (<= CSWIN_MAX_REDUCE_JOBS) reductions that reduce_jobs_ok has passed
void launch_rows_sum(const cswin_reduce_job* jobs, int njobs, hipStream_t st) {
    ReduceJobs J = {};
    const int blocks = fill_reduce_table(jobs, njobs, J.j, J.first_block);
    J.njobs = njobs;
    hipLaunchKernelGGL(rows_sum_multi_kernel, dim3(blocks), dim3(256), 0, st, J);
}

// jobs: HOST array of njobs (<= CSWIN_MAX_REDUCE_JOBS = 48) reductions left pending by *_bwd_weight / layernorm_bwd calls with `deferred` set
int rows_sum_multi(const cswin_reduce_job* jobs, int njobs, void* stream) {
    CSWIN_REQUIRE(jobs && njobs > 0 && njobs <= CSWIN_MAX_REDUCE_JOBS, CSWIN_ERR_SHAPE, "rows_sum_multi: 1..%d jobs", CSWIN_MAX_REDUCE_JOBS);
    CSWIN_REQUIRE(reduce_jobs_ok(jobs, njobs), CSWIN_ERR_SHAPE, "rows_sum_multi: bad job (part / out / n / rows, or conv_kk without conv_cin)");
    launch_rows_sum(jobs, njobs, (hipStream_t)stream);
    CSWIN_LAUNCH_CHECK();
    return CSWIN_OK;
}

// One weight gradient dw[N,K] = (row_scale . dy)^T @ [x | x2] through the tiled GEMM as plan (gp::wgrad_tiled_plan) says; arguments
// checked by the caller.  Its slab reduction runs at once or goes to *deferred
int wgrad_tiled(const gp::Plan& plan, const float* dy, const float* x, const float* x2, int k_split, const float* row_scale, int rows_per_sample,
                float* dw, float* dbias, void* workspace, int M, int N, int K, cswin_reduce_job* deferred, int precision, hipStream_t st) {
    const WgradSlabs slabs(workspace, N, K);
    const Epilogue e = slabs.epilogue(dbias != nullptr);
    PlainSrc A = {dy, N, M, N, row_scale, rows_per_sample};      // S(i = m (reduction), j = n)
    if (x2) {
        ConcatSrc B = {x, x2, k_split, K - k_split, M, K, k_split};
        launch_gemm_vec<false, false, EPI_PLAIN, true>(plan, A, B, e, N, K, M, precision, st);
    } else {
        PlainSrc B = {x, K, M, K, nullptr, 1};
        if (row_scale) launch_gemm_vec<false, false, EPI_PLAIN, true>(plan, A, B, e, N, K, M, precision, st);
        else launch_gemm_vec<false, false, EPI_PLAIN, false>(plan, A, B, e, N, K, M, precision, st);
    }
    CSWIN_LAUNCH_CHECK();
    reduce_now_or_defer(slabs.job(dw, dbias, plan.splits), deferred, st);
    CSWIN_LAUNCH_CHECK();
    return CSWIN_OK;
}

// a problem of a weight-gradient call as the policy sees it
gp::WgradProblem wgrad_problem(const cswin_wgrad_desc& p, bool has_mask) {
    gp::WgradProblem q = {};
    q.M = p.M; q.N = p.N; q.K = p.K; q.io_bf16 = p.io_bf16;
    q.loads_aligned = aligned16(p.dy) && aligned16(p.x);
    q.ws_aligned = aligned16(p.workspace);
    q.has_scale = p.row_scale != nullptr;
    q.rows_per_sample = p.rows_per_sample;
    q.has_mask = has_mask;
    q.ws_bytes = p.ws_bytes;
    return q;
}

// what may ride at the end of the weight-gradient batch's grid: a plain fp32 data gradient dx[M,K] = dy[M,N] @ w[N,K] (dy == NULL:
// none; cswin_linear_bwd_tail) and reductions left pending by earlier launches.  who: the entry point, for its error text.
struct TailExtras {
    const char* who; const float* dy; const float* w; float* dx; int M, N, K; const cswin_reduce_job* jobs; int njobs;
    // sample masks of the weight gradients (NULL: none): skip[i] (NULL: problem i has none) holds nsamples[i] floats, see RowMask
    const float* const* skip; const int* nsamples;
    // sample order of the data gradient (NULL: none), over order_samples samples of M / order_samples rows: see RowMap
    const int* order; int order_samples;
};

// What a per-sample table over the M rows of a launch must meet -- `what` names it: the sample order of a forward / data-gradient
// Linear (RowMap) or the sample mask of a weight gradient (RowMask) --, or why the launch cannot take it: a refusal, never a run
// without it (the caller's contract is that a dropped sample's rows are NOT READ).  slack: rows past M that the kernel divides before
// it tests them.  The 16-B accesses both need are the caller's to check, on its plan.
int samples_checked(const char* who, const char* what, const void* table, int nsamples, int rows_per_sample, int M, int slack, int precision) {
    CSWIN_REQUIRE(precision == 0, CSWIN_ERR_UNSUPPORTED, "%s: a %s needs precision 0", who, what);
    CSWIN_REQUIRE(table && nsamples >= 1 && nsamples <= MASK_MAX_SAMPLES, CSWIN_ERR_SHAPE, "%s: the %s must list 1..%d samples", who, what,
                  MASK_MAX_SAMPLES);
    CSWIN_REQUIRE(M > 0 && rows_per_sample > 0 && (long)nsamples * rows_per_sample == M, CSWIN_ERR_SHAPE,
                  "%s: the %s: nsamples * rows_per_sample != M", who, what);
    CSWIN_REQUIRE(fdiv_exact((long)M + slack, rows_per_sample), CSWIN_ERR_UNSUPPORTED, "%s: the %s: M * rows_per_sample must stay below 2^32", who,
                  what);
    return CSWIN_OK;
}

// The row map of a forward / data-gradient Linear over M rows.  No HIP call is made before these checks.
int row_map_checked(RowMap* rm, const char* who, const int* order, int nsamples, int rows_per_sample, int M, int precision, int io_bf16,
                    bool two_part, bool add) {
    CSWIN_REQUIRE(precision == 0 && io_bf16 == 0, CSWIN_ERR_UNSUPPORTED, "%s: a sample order needs precision 0 and fp32 storage", who);
    CSWIN_REQUIRE(!two_part, CSWIN_ERR_UNSUPPORTED, "%s: a sample order takes no concat / split operand", who);
    CSWIN_REQUIRE(!add, CSWIN_ERR_UNSUPPORTED, "%s: a sample order takes no add operand", who);
    int rc = samples_checked(who, "sample order", order, nsamples, rows_per_sample, M, 63, precision);
    if (rc) return rc;
    *rm = RowMap{order, nsamples, rows_per_sample, fdiv_magic(rows_per_sample)};
    return CSWIN_OK;
}

// The launch of n aligned weight gradients as route r says (gp::aligned_batch_plans): wgrad16's grid, or the form r.kernel of the
// batch kernel with what rides in its grid -- the data gradient of x (with its row map dmap) and x's pending reductions.
// deferred[i] receives problem i's slab reduction.  Everything was checked by the caller: nothing here refuses.
int launch_wgrad_batch(const gp::BatchRoute& r, const cswin_wgrad_desc* d, int n, cswin_reduce_job* deferred, const TailExtras& x,
                       const RowMap& dmap, int precision, hipStream_t st) {
    for (int i = 0; i < n; ++i) deferred[i] = WgradSlabs(d[i].workspace, d[i].N, d[i].K).job(d[i].dw, d[i].dbias, r.problem[i].splits);
    if (r.kernel == gp::BatchKernel::wgrad16) {
        cswin_wgrad16_batch(d, n, r.problem, r.jobs_ride ? x.jobs : nullptr, r.jobs_ride ? x.njobs : 0, st, g_stamps);
        CSWIN_LAUNCH_CHECK();
        return CSWIN_OK;
    }
    WgradBatch b = {};
    for (int i = 0; i < n; ++i) {
        const int M = d[i].M, N = d[i].N, K = d[i].K;
        push(b, PlainSrc{d[i].dy, N, M, N, d[i].row_scale, d[i].row_scale ? d[i].rows_per_sample : 1},   // S(i = m (reduction), j = n)
             PlainSrc{d[i].x, K, M, K, nullptr, 1}, WgradSlabs(d[i].workspace, N, K).epilogue(d[i].dbias != nullptr), N, K, M, r.problem[i].rows,
             r.problem[i].splits, r.problem[i].store == 4);
        if (x.skip && x.skip[i])
            b.mask[i] = RowMask{x.skip[i], x.nsamples[i], d[i].rows_per_sample, r.problem[i].splits, fdiv_magic(d[i].rows_per_sample)};
    }
    const int blocks = b.first[n];
    BlockTail t = {};
    int rblocks = 0;
    const auto fill_tail = [&] {
        if (x.dy) {            // one more problem, in fields of its own: 64 x 64 tiles (r.dgrad is Kernel::tail)
            t.dA = PlainSrc{x.dy, x.N, x.M, x.N, nullptr, 1, 0};
            t.dB = PlainSrc{x.w, x.K, x.N, x.K, nullptr, 1, 0};      // S(i = n (reduction), j = k)
            t.de = plain_epilogue(x.dx, x.K);
            t.de.vec_store = r.dgrad.store == 4;
            t.dM = x.M; t.dN = x.K; t.dR = x.N; t.drps = r.dgrad.rows;
            t.dtm = cdiv(x.M, 64); t.dtn = cdiv(x.K, 64);
            t.nd = t.dtm * t.dtn;
        }
        t.w = b;
        if (x.njobs > 0) {
            rblocks = fill_reduce_table(x.jobs, x.njobs, t.r.j, t.r.first_block);
            t.r.njobs = x.njobs;
        }
    };
    static_assert(sizeof(BlockTail) <= 4096, "kernel argument block");
    static_assert(sizeof(BlockTail) + sizeof(RowMap) <= 4096, "kernel argument block");
    switch (r.kernel) {
        case gp::BatchKernel::tail_order:
            fill_tail();
            hipLaunchKernelGGL(gemm_block_tail_skip_kernel, dim3(blocks + t.nd + rblocks), dim3(512), 0, st, t, dmap);
            break;
        case gp::BatchKernel::tail_masked:
            fill_tail();
            hipLaunchKernelGGL(gemm_block_tail_masked_kernel, dim3(blocks + t.nd + rblocks), dim3(512), 0, st, t);
            break;
        case gp::BatchKernel::tail:
            fill_tail();
            hipLaunchKernelGGL(gemm_block_tail_kernel, dim3(blocks + t.nd + rblocks), dim3(512), 0, st, t);
            break;
        case gp::BatchKernel::masked:
            hipLaunchKernelGGL(gemm_wgrad_batch_masked_kernel, dim3(blocks), dim3(512), 0, st, b);
            break;
        default:
            if (precision == 1) hipLaunchKernelGGL(gemm_wgrad_batch_kernel<1>, dim3(blocks), dim3(512), 0, st, b);
            else hipLaunchKernelGGL(gemm_wgrad_batch_kernel<0>, dim3(blocks), dim3(512), 0, st, b);
    }
    CSWIN_LAUNCH_CHECK();
    return CSWIN_OK;
}

// One weight gradient without a concat input as plan (gp::linear_wgrad_plan) says: the tiled family, or the batch path as a batch of one
int launch_wgrad_one(const gp::Plan& plan, const cswin_wgrad_desc& p, cswin_reduce_job* deferred, hipStream_t st) {
    if (plan.kernel == gp::Kernel::tiled)
        return wgrad_tiled(plan, p.dy, p.x, nullptr, 0, p.row_scale, p.rows_per_sample, p.dw, p.dbias, p.workspace, p.M, p.N, p.K, deferred,
                           p.precision, st);
    gp::BatchRoute one = {};
    one.kernel = plan.kernel == gp::Kernel::wgrad16 ? gp::BatchKernel::wgrad16 : gp::BatchKernel::plain;
    one.problem[0] = plan;
    cswin_reduce_job job;
    int rc = launch_wgrad_batch(one, &p, 1, &job, TailExtras{}, RowMap{}, p.precision, st);
    if (rc) return rc;
    reduce_now_or_defer(job, deferred, st);
    CSWIN_LAUNCH_CHECK();
    return CSWIN_OK;
}

// n (<= 4) weight gradients and what x adds to them, in three phases: check, plan (gp::batch_route), launch.  An error return means
// that nothing was enqueued: the pending reductions of x "must not be run again" once a call has taken them, and a caller that
// sees an error could not know whether it had.
int wgrad_batch_impl(const cswin_wgrad_desc* d, int n, cswin_reduce_job* deferred, const TailExtras& x, void* stream) {
    // ---- check: everything that can refuse
    CSWIN_REQUIRE(x.njobs >= 0 && x.njobs <= CSWIN_TAIL_RIDER_JOBS && (x.njobs == 0 || x.jobs), CSWIN_ERR_SHAPE,
                  "%s: 0..%d pending reductions", x.who, CSWIN_TAIL_RIDER_JOBS);
    CSWIN_REQUIRE(d && deferred && n >= 1 && n <= WGRAD_BATCH, CSWIN_ERR_SHAPE, "linear_bwd_weight_batch: 1..%d problems and their deferred slots", WGRAD_BATCH);
    const int precision = d[0].precision;
    const bool has_dgrad = x.dy != nullptr;
    gp::TailRequest tail = {};
    tail.dgrad = has_dgrad;
    tail.M = x.M; tail.N = x.N; tail.K = x.K;
    tail.loads_aligned = aligned16(x.dy) && aligned16(x.w);
    tail.dx_aligned = aligned16(x.dx);
    tail.order = x.order != nullptr;
    tail.njobs = x.njobs;
    RowMap dmap = {};
    if (x.order) {
        CSWIN_REQUIRE(x.dy && x.order_samples >= 1 && x.M % x.order_samples == 0, CSWIN_ERR_SHAPE, "%s: nsamples * rows_per_sample != M", x.who);
        int rc = row_map_checked(&dmap, x.who, x.order, x.order_samples, x.M / x.order_samples, x.M, precision, 0, false, false);
        if (rc) return rc;
        CSWIN_REQUIRE(x.N % 4 == 0 && x.K % 4 == 0 && tail.loads_aligned && tail.dx_aligned, CSWIN_ERR_ALIGN,
                      "%s: a sample order needs N, K multiples of 4 and 16-B aligned operands", x.who);
    }
    CSWIN_CHECK_PRECISION(precision, "linear_bwd_weight_batch");
    gp::WgradProblem problems[WGRAD_BATCH];
    bool fast = true, any_mask = false;
    for (int i = 0; i < n; ++i) {
        CSWIN_REQUIRE(d[i].precision == precision, CSWIN_ERR_UNSUPPORTED, "linear_bwd_weight_batch: problems of one launch share one precision");
        CSWIN_REQUIRE(d[i].io_bf16 == 0 || (precision == 1 && (d[i].io_bf16 & ~3) == 0), CSWIN_ERR_UNSUPPORTED, "linear_bwd_weight_batch: bf16 storage needs precision 1");
        CSWIN_REQUIRE(d[i].dy && d[i].x && d[i].dw && d[i].M > 0 && d[i].N > 0 && d[i].K > 0, CSWIN_ERR_SHAPE, "linear_bwd_weight_batch: bad problem %d", i);
        CSWIN_REQUIRE(!d[i].row_scale || d[i].rows_per_sample > 0, CSWIN_ERR_SHAPE, "linear_bwd_weight_batch: rows_per_sample must be > 0");
        size_t need = gp::wgrad_workspace_bytes(cswin_tuning(), d[i].M, d[i].N, d[i].K);
        CSWIN_REQUIRE(d[i].workspace && d[i].ws_bytes >= need, CSWIN_ERR_WORKSPACE, "linear_bwd_weight_batch: workspace %zu < %zu", d[i].ws_bytes, need);
        const bool masked = x.skip && x.skip[i];
        problems[i] = wgrad_problem(d[i], masked);
        fast = fast && problems[i].aligned();
        if (masked) {
            any_mask = true;
            char what[40];
            snprintf(what, sizeof(what), "sample mask of problem %d", i);
            int rc = samples_checked(x.who, what, x.nsamples ? x.skip[i] : nullptr, x.nsamples ? x.nsamples[i] : 0, d[i].rows_per_sample, d[i].M, 0,
                                     precision);
            if (rc) return rc;
        }
    }
    CSWIN_REQUIRE(!any_mask || fast, CSWIN_ERR_ALIGN, "%s: a sample mask needs N, K multiples of 4 and 16-B aligned operands", x.who);
    CSWIN_REQUIRE(reduce_jobs_ok(x.jobs, x.njobs), CSWIN_ERR_SHAPE, "%s: bad pending reduction", x.who);
    for (int i = 0; i < n && !fast; ++i)      // separate launches take no bf16-stored problem
        CSWIN_REQUIRE(d[i].io_bf16 == 0, CSWIN_ERR_ALIGN, "linear_bwd_weight_batch: bf16 storage needs N, K multiples of 4 and 16-B alignment");
    // ---- plan (pure: what it gives is still only checked)
    const gp::BatchRoute r = gp::batch_route(cswin_tuning(), problems, n, precision, tail);
    for (int i = 0; i < n; ++i)
        CSWIN_REQUIRE((size_t)r.problem[i].splits * gp::slab_stride(d[i].N, d[i].K) * sizeof(float) <= d[i].ws_bytes, CSWIN_ERR_WORKSPACE,
                      "linear_bwd_weight_batch: %d slabs do not fit problem %d's workspace", r.problem[i].splits, i);
    // ---- launch
    hipStream_t st = (hipStream_t)stream;
    if (r.dgrad_first) {      // the data gradient as a GEMM problem (as cswin_linear_bwd_data poses it): M x K outputs, reduction N in one split
        const PlainSrc gA = {x.dy, x.N, x.M, x.N, nullptr, 1, 0}, gB = {x.w, x.K, x.N, x.K, nullptr, 1, 0};      // gB: S(i = n (reduction), j = k)
        launch_gemm_vec<true, false, EPI_PLAIN, false>(r.dgrad, gA, gB, plain_epilogue(x.dx, x.K), x.M, x.K, x.N, precision, st, x.order ? &dmap : nullptr);
        CSWIN_LAUNCH_CHECK();
    }
    if (r.jobs_first) {
        launch_rows_sum(x.jobs, x.njobs, st);
        CSWIN_LAUNCH_CHECK();
    }
    if (r.kernel != gp::BatchKernel::separate) return launch_wgrad_batch(r, d, n, deferred, x, dmap, precision, st);
    for (int i = 0; i < n; ++i) {
        int rc = launch_wgrad_one(r.problem[i], d[i], &deferred[i], st);
        if (rc) return rc;
    }
    return CSWIN_OK;
}

// The reciprocals of a gather source's divisors, and whether every division of the launch stays inside fdiv's bound: row indices
// < nrows are split by img (pixels per image) and what remains (< img) by w; column indices < ncols by c; taps < ks * ks by ks;
// pixel coordinates <= cmax by stride (0: the source has no such division).  The row bound is taken 64 rows past the last one: the
// epilogue of a FAST kernel splits the rows of its last tile before it tests them.  false: the launch takes the FAST = false form.
bool conv_magics(ConvMagics* m, long nrows, int img, int w, long ncols, int c, int ks, int cmax, int stride) {
    *m = ConvMagics{fdiv_magic(img), fdiv_magic(w), fdiv_magic(c), fdiv_magic(ks), fdiv_magic(stride)};
    return fdiv_exact(nrows + 63, img) && fdiv_exact(img - 1, w) && fdiv_exact(ncols - 1, c) && fdiv_exact((long)ks * ks - 1, ks) &&
           (stride == 0 || fdiv_exact(cmax, stride));
}
// f(std::true_type) when the bound holds, f(std::false_type) otherwise: the two forms of a gather launch
template <class F> void with_fast_div(bool fast, F f) {
    if (fast) f(std::true_type{});
    else f(std::false_type{});
}

// dw_perm: [Cout][ks*ks][Cin], or the nn.Conv2d parameter layout [Cout][Cin_param][ks][ks] when torch_layout != 0; dbias: [Cout]
int conv_wgrad_impl(const float* dy, const float* x, float* dw_perm, float* dbias, void* workspace, size_t ws_bytes, int B, int H,
                    int W, int Cin, int Cout, int ks, int stride, int pad, int torch_layout, int Cin_param,
                    cswin_reduce_job* deferred, int precision, void* stream) {
    CSWIN_CHECK_PRECISION(precision, "conv_tok_bwd_weight");
    CSWIN_REQUIRE(dy && x && dw_perm, CSWIN_ERR_SHAPE, "conv_tok_bwd_weight: null pointer");
    CSWIN_REQUIRE(Cin % 4 == 0 && Cout % 4 == 0 && aligned16(dy) && aligned16(x), CSWIN_ERR_ALIGN, "conv_tok_bwd_weight: channels %% 4 and 16-B alignment required");
    CSWIN_REQUIRE(!torch_layout || Cin < 65536, CSWIN_ERR_UNSUPPORTED, "conv_tok_bwd_weight: torch_layout needs Cin < 65536");
    int OH = (H + 2 * pad - ks) / stride + 1, OW = (W + 2 * pad - ks) / stride + 1;
    int M = B * OH * OW, K = ks * ks * Cin;
    size_t need = gp::wgrad_workspace_bytes(cswin_tuning(), M, Cout, K);
    CSWIN_REQUIRE(workspace && ws_bytes >= need, CSWIN_ERR_WORKSPACE, "conv_tok_bwd_weight: workspace %zu < %zu", ws_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    const gp::Split s = gp::choose_split(cswin_tuning(), M, Cout, K);
    const WgradSlabs slabs(workspace, Cout, K);
    const Epilogue e = slabs.epilogue(dbias != nullptr);
    const gp::Plan plan = gp::tiled_plan(cswin_tuning(), Cout, K, M, s.splits, s.rows, true, precision, true, epilogue_vec_ok(e, K));
    PlainSrc A = {dy, Cout, M, Cout, nullptr, 1};
    ConvMagics mg;
    with_fast_div(conv_magics(&mg, M, OH * OW, OW, K, Cin, ks, 0, 0), [&](auto fast) {
        ConvSrcT<decltype(fast)::value> Bm = {x, B, H, W, Cin, OH, OW, ks, stride, pad, M, K, mg};   // S(i = pixel m (reduction), j = (tap, ci))
        launch_gemm<false, false, 4, EPI_PLAIN, false>(plan, A, Bm, e, Cout, K, M, precision, st);
    });
    CSWIN_LAUNCH_CHECK();
    reduce_now_or_defer(slabs.job(dw_perm, dbias, s.splits, torch_layout ? ks * ks : 0,
                                  torch_layout ? (Cin | (Cin_param != Cin ? Cin_param << 16 : 0)) : 0), deferred, st);
    CSWIN_LAUNCH_CHECK();
    return CSWIN_OK;
}

// y[M,N] = [x | x2][M,K] @ w[N,K]^T + bias (optionally GELU to y_act, or + row_scale . residual): cswin_linear_fwd, and with
// mapped its twin with a SAMPLE ORDER (row map, see RowMap) -- plain fp32 matrices with 16-B accesses only, everything else is refused
int linear_fwd_impl(const char* who, const float* x, const float* x2, int k_split, const float* w, const float* bias, float* y, float* y_act,
                    const float* residual, const float* row_scale, int rows_per_sample, int M, int N, int K, int precision, int io_bf16,
                    bool mapped, const int* order, int nsamples, void* stream) {
    RowMap rm = {};
    if (mapped) {
        int rc = row_map_checked(&rm, who, order, nsamples, rows_per_sample, M, precision, io_bf16, x2 != nullptr, false);
        if (rc) return rc;
    }
    CSWIN_CHECK_PRECISION(precision, who);
    CSWIN_REQUIRE(io_bf16 == 0 || (precision == 1 && (!x2 || !(io_bf16 & 1)) && (io_bf16 & ~7) == 0 && K % 4 == 0 && N % 4 == 0 && !((io_bf16 & 2) && residual)), CSWIN_ERR_UNSUPPORTED,
                  "%s: bf16 storage (io_bf16 = %d: 1 = x, 2 = y / y_act, 4 = w) needs precision 1, a plain input for bit 1, K and N multiples of 4; a residual output stays fp32", who, io_bf16);
    CSWIN_REQUIRE(x && w && y && M > 0 && N > 0 && K > 0, CSWIN_ERR_SHAPE, "%s: bad arguments M=%d N=%d K=%d", who, M, N, K);
    CSWIN_REQUIRE(!x2 || (k_split > 0 && k_split < K), CSWIN_ERR_SHAPE, "%s: bad concat split %d of K=%d", who, k_split, K);
    CSWIN_REQUIRE(!row_scale || rows_per_sample > 0, CSWIN_ERR_SHAPE, "%s: rows_per_sample must be > 0", who);
    CSWIN_REQUIRE(!(y_act && residual), CSWIN_ERR_UNSUPPORTED, "%s: activation and residual epilogues are exclusive", who);
    CSWIN_REQUIRE(!(x2 && y_act), CSWIN_ERR_UNSUPPORTED, "%s: concat input does not support the activation epilogue", who);
    Epilogue e = plain_epilogue(y, N);
    e.bias = bias;
    e.Cact = y_act; e.ldact = N;
    e.residual = residual; e.ldres = N;
    e.row_scale = row_scale; e.rows_per_sample = rows_per_sample;
    e.c_bf16 = (io_bf16 & 2) != 0;
    const gp::Plan plan = gp::linear_fwd_plan(cswin_tuning(), M, N, K, x2 ? k_split : 0, precision, io_bf16,
                                              aligned16(x) && aligned16(w) && aligned16(x2), epilogue_ptrs_aligned(e));
    const bool vec_all = plan.vec == 4 && plan.store == 4;
    CSWIN_REQUIRE(!mapped || vec_all, CSWIN_ERR_ALIGN, "%s: a sample order needs N, K multiples of 4 and 16-B aligned operands", who);
    if (x2) CSWIN_REQUIRE(io_bf16 == 0 || (io_bf16 == 4 && plan.vec == 4), CSWIN_ERR_UNSUPPORTED, "%s: a concat input takes only the bf16 weight flag (4), with 16-B aligned operands", who);
    else CSWIN_REQUIRE(io_bf16 == 0 || (plan.vec == 4 && aligned16(y) && aligned16(y_act) && aligned16(bias)), CSWIN_ERR_ALIGN, "%s: bf16 storage needs 16-B aligned operands", who);
    hipStream_t st = (hipStream_t)stream;
    const int epi_mode = y_act ? EPI_ACT : (residual ? EPI_RES : EPI_PLAIN);
    const PlainSrc B = {w, K, N, K, nullptr, 1, (io_bf16 >> 2) & 1};
    if (plan.kernel == gp::Kernel::gemm16) {
        CSWIN_REQUIRE(cswin_gemm16(plan, 0, epi_mode, x, w, &e, M, N, K, stream) == 0, CSWIN_ERR_HIP, "%s: the LDS-DMA kernel could not be set up", who);
    } else if (x2) {
        const ConcatSrc A = {x, x2, k_split, K - k_split, M, K, k_split};
        launch_gemm_epi<true, true, EPI_RES, EPI_PLAIN>(epi_mode, plan, A, B, e, M, N, K, precision, st);
    } else {
        const PlainSrc A = {x, K, M, K, nullptr, 1, io_bf16 & 1};
        launch_gemm_epi<true, true, EPI_ACT, EPI_RES, EPI_PLAIN>(epi_mode, plan, A, B, e, M, N, K, precision, st, mapped ? &rm : nullptr);
    }
    CSWIN_LAUNCH_CHECK();
    return CSWIN_OK;
}

// dx[M,K] = (row_scale . dy)[M,N] @ w[N,K]   (optionally * gelu'(gelu_pre), + add; optionally split into dx | dx2): cswin_linear_bwd_data,
// and with mapped its twin with a sample order
int linear_dgrad_impl(const char* who, const float* dy, const float* w, float* dx, float* dx2, int k_split, const float* gelu_pre,
                      const float* row_scale, int rows_per_sample, const float* add, int M, int N, int K, int precision, int io_bf16,
                      bool mapped, const int* order, int nsamples, void* stream) {
    RowMap rm = {};
    if (mapped) {
        int rc = row_map_checked(&rm, who, order, nsamples, rows_per_sample, M, precision, io_bf16, dx2 != nullptr, add != nullptr);
        if (rc) return rc;
    }
    CSWIN_CHECK_PRECISION(precision, who);
    CSWIN_REQUIRE(io_bf16 == 0 || (precision == 1 && ((!dx2 && !add) || (io_bf16 & ~4) == 0) && (io_bf16 & ~15) == 0 && K % 4 == 0 && N % 4 == 0), CSWIN_ERR_UNSUPPORTED,
                  "%s: bf16 storage (io_bf16 = %d: 1 = dy, 2 = dx, 4 = w, 8 = gelu_pre) needs precision 1, K and N multiples of 4; split / add outputs take only the weight flag", who, io_bf16);
    CSWIN_REQUIRE(dy && w && dx && M > 0 && N > 0 && K > 0, CSWIN_ERR_SHAPE, "%s: bad arguments", who);
    CSWIN_REQUIRE(!dx2 || (k_split > 0 && k_split < K), CSWIN_ERR_SHAPE, "%s: bad concat split", who);
    CSWIN_REQUIRE(!row_scale || rows_per_sample > 0, CSWIN_ERR_SHAPE, "%s: rows_per_sample must be > 0", who);
    Epilogue e = plain_epilogue(dx, dx2 ? k_split : K);
    e.C2 = dx2; e.ldc2 = K - k_split; e.col_split = dx2 ? k_split : 0;
    e.gelu_pre = gelu_pre; e.ldpre = K;
    e.row_scale = row_scale; e.rows_per_sample = rows_per_sample;
    e.residual = add; e.ldres = K;
    e.c_bf16 = (io_bf16 & 2) != 0;
    e.pre_bf16 = (io_bf16 & 8) != 0;
    CSWIN_REQUIRE(io_bf16 == 0 || (aligned16(dy) && aligned16(w) && aligned16(dx) && aligned16(gelu_pre)), CSWIN_ERR_ALIGN,
                  "%s: bf16 storage needs 16-B aligned operands", who);
    const int modes = (dx2 != nullptr) + (gelu_pre != nullptr) + (add != nullptr);
    CSWIN_REQUIRE(modes <= 1, CSWIN_ERR_UNSUPPORTED, "%s: dx2 / gelu_pre / add are mutually exclusive", who);
    const gp::Plan plan = gp::linear_dgrad_plan(cswin_tuning(), M, N, K, dx2 ? k_split : 0, add != nullptr, precision, io_bf16,
                                                aligned16(dy) && aligned16(w), epilogue_ptrs_aligned(e));
    CSWIN_REQUIRE(!mapped || (plan.vec == 4 && plan.store == 4), CSWIN_ERR_ALIGN,
                  "%s: a sample order needs N, K multiples of 4 and 16-B aligned operands", who);
    hipStream_t st = (hipStream_t)stream;
    const int epi_mode = dx2 ? EPI_SPLIT2 : (gelu_pre ? EPI_GELUBWD : (add ? EPI_RES : EPI_PLAIN));
    if (plan.kernel == gp::Kernel::gemm16) {
        CSWIN_REQUIRE(cswin_gemm16(plan, 1, epi_mode, dy, w, &e, M, K, N, stream) == 0, CSWIN_ERR_HIP, "%s: the LDS-DMA kernel could not be set up", who);
    } else {
        const PlainSrc A = {dy, N, M, N, nullptr, 1, io_bf16 & 1};
        const PlainSrc B = {w, K, N, K, nullptr, 1, (io_bf16 >> 2) & 1};     // S(i = n (reduction), j = k): row-contiguous image
        launch_gemm_epi<true, false, EPI_SPLIT2, EPI_GELUBWD, EPI_RES, EPI_PLAIN>(epi_mode, plan, A, B, e, M, K, N, precision, st, mapped ? &rm : nullptr);
    }
    CSWIN_LAUNCH_CHECK();
    return CSWIN_OK;
}

}  // namespace

// ======================================================================================
// C ABI
// ======================================================================================
extern "C" {

// debug aid (not part of include/cswin_hip.h): device buffer [workgroups][8] of int64; workgroup w of a GEMM launch stamps row w
// (stamp_slot, bf16_tile.h, has the slots)
void cswin_debug_set_stamps(void* p) { g_stamps = (long long*)p; }

int cswin_linear_fwd(const float* x, const float* x2, int k_split, const float* w, const float* bias, float* y,
                     float* y_act, const float* residual, const float* row_scale, int rows_per_sample, int M, int N,
                     int K, int precision, int io_bf16, void* stream) {
    return linear_fwd_impl("linear_fwd", x, x2, k_split, w, bias, y, y_act, residual, row_scale, rows_per_sample, M, N, K, precision, io_bf16,
                           false, nullptr, 0, stream);
}

int cswin_linear_bwd_data(const float* dy, const float* w, float* dx, float* dx2, int k_split, const float* gelu_pre,
                          const float* row_scale, int rows_per_sample, const float* add, int M, int N, int K,
                          int precision, int io_bf16, void* stream) {
    return linear_dgrad_impl("linear_bwd_data", dy, w, dx, dx2, k_split, gelu_pre, row_scale, rows_per_sample, add, M, N, K, precision,
                             io_bf16, false, nullptr, 0, stream);
}

// The two calls above with a sample order: an order is refused where the launch cannot take it, never run unmapped
int cswin_linear_fwd_skip(const float* x, const float* x2, int k_split, const float* w, const float* bias, float* y, float* y_act,
                          const float* residual, const float* row_scale, int rows_per_sample, int M, int N, int K, int precision,
                          int io_bf16, const int* order, int nsamples, void* stream) {
    return linear_fwd_impl("linear_fwd_skip", x, x2, k_split, w, bias, y, y_act, residual, row_scale, rows_per_sample, M, N, K, precision,
                           io_bf16, true, order, nsamples, stream);
}

int cswin_linear_bwd_data_skip(const float* dy, const float* w, float* dx, float* dx2, int k_split, const float* gelu_pre,
                               const float* row_scale, int rows_per_sample, const float* add, int M, int N, int K, int precision,
                               int io_bf16, const int* order, int nsamples, void* stream) {
    return linear_dgrad_impl("linear_bwd_data_skip", dy, w, dx, dx2, k_split, gelu_pre, row_scale, rows_per_sample, add, M, N, K, precision,
                             io_bf16, true, order, nsamples, stream);
}

// scales (rows, B) = (u < keep[row]) / keep[row] and order (rows, 1 + B) from one step's DropPath draws u (rows, B): see drop_path_order_kernel
int cswin_drop_path_order(const float* u, const float* keep, float* scales, int* order, int rows, int B, void* stream) {
    CSWIN_REQUIRE(u && keep && scales && order && rows > 0, CSWIN_ERR_SHAPE, "drop_path_order: bad arguments");
    CSWIN_REQUIRE(B >= 1 && B <= MASK_MAX_SAMPLES, CSWIN_ERR_SHAPE, "drop_path_order: 1..%d samples", MASK_MAX_SAMPLES);
    hipLaunchKernelGGL(drop_path_order_kernel, dim3(rows), dim3(64), 0, (hipStream_t)stream, u, keep, scales, order, B);
    CSWIN_LAUNCH_CHECK();
    return CSWIN_OK;
}

size_t cswin_linear_bwd_weight_workspace(int M, int N, int K) { return gp::wgrad_workspace_bytes(cswin_tuning(), M, N, K); }

// dw[N,K] = (row_scale . dy)^T @ [x | x2];  dbias[N] = colsum(row_scale . dy)
int cswin_linear_bwd_weight(const float* dy, const float* x, const float* x2, int k_split, const float* row_scale,
                            int rows_per_sample, float* dw, float* dbias, void* workspace, size_t ws_bytes, int M,
                            int N, int K, cswin_reduce_job* deferred, int precision, void* stream) {
    CSWIN_CHECK_PRECISION(precision, "linear_bwd_weight");
    CSWIN_REQUIRE(dy && x && dw && M > 0 && N > 0 && K > 0, CSWIN_ERR_SHAPE, "linear_bwd_weight: bad arguments");
    CSWIN_REQUIRE(!x2 || (k_split > 0 && k_split < K), CSWIN_ERR_SHAPE, "linear_bwd_weight: bad concat split");
    CSWIN_REQUIRE(!row_scale || rows_per_sample > 0, CSWIN_ERR_SHAPE, "linear_bwd_weight: rows_per_sample must be > 0");
    size_t need = gp::wgrad_workspace_bytes(cswin_tuning(), M, N, K);
    CSWIN_REQUIRE(workspace && ws_bytes >= need, CSWIN_ERR_WORKSPACE, "linear_bwd_weight: workspace %zu < %zu", ws_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    const cswin_wgrad_desc d1 = {dy, x, row_scale, dw, dbias, workspace, ws_bytes, rows_per_sample, M, N, K, precision, 0};
    const gp::Plan plan = gp::linear_wgrad_plan(cswin_tuning(), wgrad_problem(d1, false), x2 ? k_split : 0, precision, aligned16(x2));
    if (x2) return wgrad_tiled(plan, dy, x, x2, k_split, row_scale, rows_per_sample, dw, dbias, workspace, M, N, K, deferred, precision, st);
    return launch_wgrad_one(plan, d1, deferred, st);
}

// n (<= 4) weight gradients without concat sources in one launch (see gemm_wgrad_batch_kernel); deferred[i] receives problem
// i's slab reduction (run them with cswin_rows_sum_multi).  Falls back to separate launches when a problem is not 16-B
// aligned / a multiple of 4 in N and K.
// With sample masks: skip[i] (or NULL) = nsamples[i] per-sample floats of problem i, M = nsamples[i] * rows_per_sample; a
// sample whose float is 0 adds nothing to dw / dbias and its rows of dy and x are not read (fp32, aligned problems only)
int cswin_linear_bwd_weight_batch_masked(const cswin_wgrad_desc* d, int n, cswin_reduce_job* deferred, const cswin_reduce_job* pending,
                                         int npending, const float* const* skip, const int* nsamples, void* stream) {
    TailExtras x = {};
    x.who = "linear_bwd_weight_batch";
    x.jobs = pending; x.njobs = npending;
    x.skip = skip; x.nsamples = nsamples;
    return wgrad_batch_impl(d, n, deferred, x, stream);
}

int cswin_linear_bwd_weight_batch(const cswin_wgrad_desc* d, int n, cswin_reduce_job* deferred, const cswin_reduce_job* pending, int npending,
                                  void* stream) {
    return cswin_linear_bwd_weight_batch_masked(d, n, deferred, pending, npending, nullptr, nullptr, stream);
}

// The tail of a CSWinBlock's backward: dx[M,K] = dy[M,N] @ w[N,K] (the qkv Linear's data gradient, plain fp32, no epilogue extras)
// and the block's weight gradients as cswin_linear_bwd_weight_batch takes them.  In fp32 with aligned operands both run in ONE
// launch (gemm_block_tail_kernel); otherwise the data gradient is launched first and the batch follows -- same results either way.
// skip / nsamples: masks of the weight gradients as for cswin_linear_bwd_weight_batch_masked; the data gradient has none.
// order: the data gradient's sample order over order_samples samples of M / order_samples rows (see RowMap); what the order cannot
// serve (precision 1, unaligned operands) is refused.
int cswin_linear_bwd_tail_skip(const float* dy, const float* w, float* dx, int M, int N, int K, const cswin_wgrad_desc* d, int n,
                               cswin_reduce_job* deferred, const cswin_reduce_job* pending, int npending, const float* const* skip,
                               const int* nsamples, const int* order, int order_samples, void* stream) {
    CSWIN_REQUIRE(dy && w && dx && M > 0 && N > 0 && K > 0, CSWIN_ERR_SHAPE, "linear_bwd_tail_skip: bad data-gradient arguments");
    CSWIN_REQUIRE(order, CSWIN_ERR_SHAPE, "linear_bwd_tail_skip: the order must list 1..%d samples", MASK_MAX_SAMPLES);
    CSWIN_REQUIRE(d && n >= 1 && n <= WGRAD_BATCH, CSWIN_ERR_SHAPE, "linear_bwd_tail_skip: 1..%d weight-gradient problems", WGRAD_BATCH);
    TailExtras x = {};
    x.who = "linear_bwd_tail_skip";
    x.dy = dy; x.w = w; x.dx = dx; x.M = M; x.N = N; x.K = K;
    x.jobs = pending; x.njobs = npending;
    x.skip = skip; x.nsamples = nsamples;
    x.order = order; x.order_samples = order_samples;
    return wgrad_batch_impl(d, n, deferred, x, stream);
}

int cswin_linear_bwd_tail_masked(const float* dy, const float* w, float* dx, int M, int N, int K, const cswin_wgrad_desc* d, int n,
                                 cswin_reduce_job* deferred, const cswin_reduce_job* pending, int npending, const float* const* skip,
                                 const int* nsamples, void* stream) {
    CSWIN_REQUIRE(dy && w && dx && M > 0 && N > 0 && K > 0, CSWIN_ERR_SHAPE, "linear_bwd_tail: bad data-gradient arguments");
    TailExtras x = {};
    x.who = "linear_bwd_tail";
    x.dy = dy; x.w = w; x.dx = dx; x.M = M; x.N = N; x.K = K;
    x.jobs = pending; x.njobs = npending;
    x.skip = skip; x.nsamples = nsamples;
    return wgrad_batch_impl(d, n, deferred, x, stream);
}

int cswin_linear_bwd_tail(const float* dy, const float* w, float* dx, int M, int N, int K, const cswin_wgrad_desc* d, int n,
                          cswin_reduce_job* deferred, const cswin_reduce_job* pending, int npending, void* stream) {
    return cswin_linear_bwd_tail_masked(dy, w, dx, M, N, K, d, n, deferred, pending, npending, nullptr, nullptr, stream);
}

// -------- convolutions on the (B, H*W, C) token layout (NHWC), implicit GEMM -----------------------------------
// w_perm: [Cout][ks*ks][Cin]  (made by cswin_conv_weight_permute from the nn.Conv2d [Cout][Cin][ks][ks] parameter)
int cswin_conv_tok_fwd(const float* x, const float* w_perm, const float* bias, float* y, int B, int H, int W, int Cin,
                       int Cout, int ks, int stride, int pad, int precision, void* stream) {
    CSWIN_CHECK_PRECISION(precision, "conv_tok_fwd");
    CSWIN_REQUIRE(x && w_perm && y && B > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0, CSWIN_ERR_SHAPE, "conv_tok_fwd: bad arguments");
    CSWIN_REQUIRE(Cin % 4 == 0 && aligned16(x) && aligned16(w_perm), CSWIN_ERR_ALIGN, "conv_tok_fwd: Cin %% 4 and 16-B alignment required");
    int OH = (H + 2 * pad - ks) / stride + 1, OW = (W + 2 * pad - ks) / stride + 1;
    int M = B * OH * OW, R = ks * ks * Cin;
    PlainSrc Bm = {w_perm, R, Cout, R, nullptr, 1};
    Epilogue e = plain_epilogue(y, Cout);
    e.bias = bias;
    const gp::Plan plan = one_split_plan(e, M, Cout, R, precision);
    ConvMagics mg;
    with_fast_div(conv_magics(&mg, M, OH * OW, OW, R, Cin, ks, 0, 0), [&](auto fast) {
        ConvSrcT<decltype(fast)::value> A = {x, B, H, W, Cin, OH, OW, ks, stride, pad, M, R, mg};
        launch_gemm<true, true, 4, EPI_PLAIN, false>(plan, A, Bm, e, M, Cout, R, precision, (hipStream_t)stream);
    });
    CSWIN_LAUNCH_CHECK();
    return CSWIN_OK;
}

// w_permT: [ks*ks][Cout][Cin]
int cswin_conv_tok_bwd_data(const float* dy, const float* w_permT, float* dx, int B, int H, int W, int Cin, int Cout,
                            int ks, int stride, int pad, int precision, void* stream) {
    CSWIN_CHECK_PRECISION(precision, "conv_tok_bwd_data");
    CSWIN_REQUIRE(dy && w_permT && dx, CSWIN_ERR_SHAPE, "conv_tok_bwd_data: null pointer");
    CSWIN_REQUIRE(Cin % 4 == 0 && Cout % 4 == 0 && aligned16(dy) && aligned16(w_permT), CSWIN_ERR_ALIGN, "conv_tok_bwd_data: channels %% 4 and 16-B alignment required");
    int OH = (H + 2 * pad - ks) / stride + 1, OW = (W + 2 * pad - ks) / stride + 1;
    if (ks == 3 && stride == 2 && pad == 1) {
        // four parity classes, each a dense GEMM over only the taps that reach it (Merge_Block.conv, cswin_unet.py:208),
        // launched together (gemm_conv_s2_dgrad_batch_kernel)
        // every class's divisions inside fdiv's bound (the largest class is (0, 0)), or the launch keeps the compiler's divisions
        bool fast_ok = true;
        for (int py = 0; py < 2; ++py)
            for (int px = 0; px < 2; ++px) {
                const int H2 = (H - py + 1) / 2, W2 = (W - px + 1) / 2;
                ConvMagics mg;
                if (H2 > 0 && W2 > 0) fast_ok = fast_ok && conv_magics(&mg, (long)B * H2 * W2, H2 * W2, W2, 4L * Cout, Cout, 1, 0, 0);
            }
        with_fast_div(fast_ok, [&](auto fast) {
            constexpr bool FAST = decltype(fast)::value;
            GemmBatch<ConvTS2SrcT<FAST>, TapRowsSrcT<FAST>> b = {};
            int rmax = 0;
            for (int py = 0; py < 2; ++py)
                for (int px = 0; px < 2; ++px) {
                    const int H2 = (H - py + 1) / 2, W2 = (W - px + 1) / 2;
                    if (H2 <= 0 || W2 <= 0) continue;
                    int kys = 0, kxs = 0, taps = 0, nt = 0;
                    for (int ky = (py ? 0 : 1); ky < 3; ky += 2)
                        for (int kx = (px ? 0 : 1); kx < 3; kx += 2) {
                            kys |= ky << (2 * nt);
                            kxs |= kx << (2 * nt);
                            taps |= (ky * 3 + kx) << (4 * nt);
                            ++nt;
                        }
                    const int Mc = B * H2 * W2, Rc = nt * Cout;
                    Epilogue e = plain_epilogue(dx, Cin);
                    e.rm_on = 1; e.rm_H = H; e.rm_W = W; e.rm_H2 = H2; e.rm_W2 = W2; e.rm_py = py; e.rm_px = px;
                    ConvMagics mg;
                    conv_magics(&mg, Mc, H2 * W2, W2, Rc, Cout, 1, 0, 0);
                    push(b, ConvTS2SrcT<FAST>{dy, B, H, W, Cout, OH, OW, py, px, H2, W2, kys, kxs, Mc, Rc, mg},
                         TapRowsSrcT<FAST>{w_permT, Cout, Cin, taps, Rc, Cin, mg.c}, e, Mc, Cin, Rc, one_split(Rc), 1, epilogue_vec_ok(e, Cin));
                    rmax = Rc > rmax ? Rc : rmax;
                }
            if (b.n > 0) {
                const int blocks = b.first[b.n];
                hipStream_t st = (hipStream_t)stream;
                const int kw = gp::s2_dgrad_kw(blocks, rmax, precision);
                if (precision == 1) hipLaunchKernelGGL((gemm_conv_s2_dgrad_batch_kernel<2, 1, FAST>), dim3(blocks), dim3(512), 0, st, b);
                else if (kw == 4) hipLaunchKernelGGL((gemm_conv_s2_dgrad_batch_kernel<4, 0, FAST>), dim3(blocks), dim3(1024), 0, st, b);
                else if (kw == 2) hipLaunchKernelGGL((gemm_conv_s2_dgrad_batch_kernel<2, 0, FAST>), dim3(blocks), dim3(512), 0, st, b);
                else hipLaunchKernelGGL((gemm_conv_s2_dgrad_batch_kernel<1, 0, FAST>), dim3(blocks), dim3(256), 0, st, b);
            }
        });
        CSWIN_LAUNCH_CHECK();
        return CSWIN_OK;
    }
    int M = B * H * W, R = ks * ks * Cout;
    PlainSrc Bm = {w_permT, Cin, R, Cin, nullptr, 1};          // S(i = (tap, co), j = ci)
    Epilogue e = plain_epilogue(dx, Cin);
    const gp::Plan plan = one_split_plan(e, M, Cin, R, precision);
    ConvMagics mg;
    with_fast_div(conv_magics(&mg, M, H * W, W, R, Cout, ks, (H > W ? H : W) + pad, stride), [&](auto fast) {
        ConvTSrcT<decltype(fast)::value> A = {dy, B, H, W, Cout, OH, OW, ks, stride, pad, M, R, mg};
        launch_gemm<true, false, 4, EPI_PLAIN, false>(plan, A, Bm, e, M, Cin, R, precision, (hipStream_t)stream);
    });
    CSWIN_LAUNCH_CHECK();
    return CSWIN_OK;
}

size_t cswin_conv_tok_bwd_weight_workspace(int B, int H, int W, int Cin, int Cout, int ks, int stride, int pad) {
    int OH = (H + 2 * pad - ks) / stride + 1, OW = (W + 2 * pad - ks) / stride + 1;
    return gp::wgrad_workspace_bytes(cswin_tuning(), B * OH * OW, Cout, ks * ks * Cin);
}

int cswin_conv_tok_bwd_weight(const float* dy, const float* x, float* dw_perm, float* dbias, void* workspace,
                              size_t ws_bytes, int B, int H, int W, int Cin, int Cout, int ks, int stride, int pad,
                              int torch_layout, cswin_reduce_job* deferred, int precision, void* stream) {
    return conv_wgrad_impl(dy, x, dw_perm, dbias, workspace, ws_bytes, B, H, W, Cin, Cout, ks, stride, pad, torch_layout, Cin, deferred,
                           precision, stream);
}

// The same for an input whose Cin channels are a zero-padded image of the parameter's Cin_param < Cin (the patch embedding: 3
// image channels in 4-channel tokens): dw is the nn.Conv2d parameter [Cout][Cin_param][ks][ks], written by the slab reduction
// itself, which drops the padded channels' columns -- no [Cout][ks*ks][Cin] image and no unpermute launch
int cswin_conv_tok_bwd_weight_cpad(const float* dy, const float* x, float* dw, float* dbias, void* workspace, size_t ws_bytes,
                                   int B, int H, int W, int Cin, int Cin_param, int Cout, int ks, int stride, int pad,
                                   cswin_reduce_job* deferred, int precision, void* stream) {
    CSWIN_REQUIRE(Cin_param > 0 && Cin_param <= Cin && Cin < 65536, CSWIN_ERR_SHAPE, "conv_tok_bwd_weight_cpad: 0 < Cin_param <= Cin < 65536");
    return conv_wgrad_impl(dy, x, dw, dbias, workspace, ws_bytes, B, H, W, Cin, Cout, ks, stride, pad, 1, Cin_param, deferred, precision,
                           stream);
}

int cswin_rows_sum_multi(const cswin_reduce_job* jobs, int njobs, void* stream) { return rows_sum_multi(jobs, njobs, stream); }

}  // extern "C"
