// Epilogue shared by the GEMM kernels of libcswin_hip (gemm.hip: tiled family; gemm16.hip: LDS-DMA bf16 kernel).  The wave's
// LDS patch, its put and its constants, and widen_bf16x4 are bf16_tile.h's.
#pragma once
#include "bf16_tile.h"
#include "common.h"

namespace {

__device__ __forceinline__ void epi_store4(float* base, long idx, f32x4 v, int bf16) {
    if (bf16) *reinterpret_cast<bf16x4*>(reinterpret_cast<__bf16*>(base) + idx) = __builtin_convertvector(v, bf16x4);
    else *reinterpret_cast<f32x4*>(base + idx) = v;
}

// ------------------------------------------------------------------------------------
// epilogue
// ------------------------------------------------------------------------------------
enum { EPI_PLAIN = 0, EPI_ACT = 1, EPI_RES = 2, EPI_GELUBWD = 3, EPI_SPLIT2 = 4 };

struct Epilogue {
    float* C; long ldc;
    float* C2; long ldc2; int col_split;      // EPI_SPLIT2: columns >= col_split are written to C2[m][n - col_split]
    const float* bias;                        // [N] or NULL (any mode)
    float* Cact; long ldact;                  // EPI_ACT: C = acc + bias (pre-activation), Cact = gelu(C)
    const float* residual; long ldres;        // EPI_RES: C = residual + row_scale * (acc + bias)
    const float* row_scale; int rows_per_sample;   // any mode: per-row multiplier (NULL = 1)
    const float* gelu_pre; long ldpre;        // EPI_GELUBWD: C = row_scale * acc * gelu'(gelu_pre[m][n])
    long split_stride;                        // C += split * split_stride (split-R partial slabs)
    float* colsum; int colsum_stride;         // TN only: partial column sums of A (dbias), [split][M]
    int rm_on, rm_H, rm_W, rm_H2, rm_W2, rm_py, rm_px;   // output row m is a parity-class pixel index -> full (b, iy, ix) row
    int vec_store;                            // 1: every output / auxiliary row is 16-B aligned and N % 4 == 0
    int c_bf16;                               // C and Cact are stored as bf16 (vector path only; bf16 activation storage)
    int pre_bf16;                             // gelu_pre is stored as bf16
    long long* stamps;                        // debug: per-workgroup s_memtime stamps [nblk][8] (NULL in production)
};

// Every fragment leaves the C/D layout through its wave's LDS patch (patch_put, bf16_tile.h), so that a lane owns 4 consecutive
// columns of one row: bias / residual / gelu' operands are read and the result is written with 16-B accesses.

// The auxiliary operands of one fragment's vector path, in registers: bias, and per row chunk p the row factor, the residual /
// gelu_pre chunk (aux16: stored as bf16) and, MAPPED, the row's place in memory.
struct EpiOperands { f32x4 bias; f32x4 aux[4]; u32x2 aux16[4]; float rs[4]; int pm[4]; };

// MAPPED: the place in memory of logical row m and, in smp, its sample (ord == NULL, the identity, or a row past the end: m and 0)
__device__ __forceinline__ int epi_mapped_row(int m, int M, const int* ord, int map_rps, unsigned map_magic, int& smp) {
    smp = 0;
    if (!ord || m >= M) return m;
    const int j = fdiv1(m, map_magic);
    smp = ord[j];
    return smp * map_rps + (m - j * map_rps);
}

// The request part of the epilogue: the loads of the fragment at (mf, nf) = (mb + 32 i, nb + 32 j), none of which depends on the
// accumulators.  gemm.hip's k-loop calls it for a wave's first fragment in front of its last tile's MFMAs (AHEAD below), so that the
// round trip -- MAPPED: ord[j] -> row_scale[ord[j]] and the aux row's address -> the aux load -- runs under matrix work instead of
// after it.  Lanes with m >= M or n >= N load nothing and a dropped row's gelu_pre is not read, as before.
template <int EPI, bool PRE16, bool MAPPED>
__device__ __forceinline__ void epilogue_request(EpiOperands& q, const Epilogue& e, int M, int N, int mf, int nf, int lane,
                                                 const int* ord = nullptr, int kept_rows = 0, int map_rps = 1, unsigned map_magic = 0) {
    const int rrow = lane >> 3, n = nf + (lane & 7) * 4;
    const bool has_rs = e.row_scale != nullptr;
    q.bias = f32x4{0.f, 0.f, 0.f, 0.f};
    if (e.bias && n < N) q.bias = *reinterpret_cast<const f32x4*>(e.bias + n);
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int m = mf + rrow + 8 * p;
        const bool ok = m < M && n < N;
        if constexpr (MAPPED) {
            int smp = 0;
            q.pm[p] = epi_mapped_row(m, M, ord, map_rps, map_magic, smp);
            const bool dropped = ord && m >= kept_rows;
            q.rs[p] = (has_rs && ok) ? e.row_scale[ord ? smp : m / e.rows_per_sample] : 1.0f;
            if (EPI == EPI_RES || EPI == EPI_GELUBWD) {
                const float* ap = EPI == EPI_RES ? e.residual : e.gelu_pre;
                const long ld = EPI == EPI_RES ? e.ldres : e.ldpre;
                q.aux[p] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (ok && !(EPI == EPI_GELUBWD && dropped)) q.aux[p] = *reinterpret_cast<const f32x4*>(ap + (long)q.pm[p] * ld + n);
            }
            continue;
        }
        q.rs[p] = (has_rs && ok) ? e.row_scale[m / e.rows_per_sample] : 1.0f;
        if (EPI == EPI_RES || EPI == EPI_GELUBWD) {
            const float* ap = EPI == EPI_RES ? e.residual : e.gelu_pre;
            const long ld = EPI == EPI_RES ? e.ldres : e.ldpre;
            q.aux[p] = f32x4{0.f, 0.f, 0.f, 0.f};
            q.aux16[p] = u32x2{0u, 0u};
            if (ok) {
                if constexpr (PRE16) q.aux16[p] = *reinterpret_cast<const u32x2*>(reinterpret_cast<const __bf16*>(ap) + (long)m * ld + n);
                else q.aux[p] = *reinterpret_cast<const f32x4*>(ap + (long)m * ld + n);
            }
        }
    }
}

// The consume step of row chunk p of a fragment (vector path): v, the chunk's four sums from the patch, meets the operands q.
// epi_value: (v + bias) . gelu'(gelu_pre) . row factor.  epi_consume_row (not MAPPED): + residual, the store of output row m
// -- row c_row(m) of C -- at columns n .. n + 3, and the activation store.  gemm16.hip's epilogue is this step on one fragment.
template <int EPI, bool PRE16>
__device__ __forceinline__ f32x4 epi_value(const EpiOperands& q, int p, f32x4 v, bool has_rs) {
    f32x4 o = v + q.bias;
    if (EPI == EPI_GELUBWD) {
        const f32x4 pre = PRE16 ? widen_bf16x4(q.aux16[p]) : q.aux[p];
#pragma unroll
        for (int c = 0; c < 4; ++c) o[c] *= gelu_grad_f(pre[c]);
    }
    if (has_rs) o *= q.rs[p];
    return o;
}
template <int EPI, bool PRE16, typename RowFn>
__device__ __forceinline__ void epi_consume_row(const Epilogue& e, const EpiOperands& q, int p, f32x4 v, bool has_rs, int m, int n, RowFn c_row) {
    f32x4 o = epi_value<EPI, PRE16>(q, p, v, has_rs);
    if (EPI == EPI_RES) o += q.aux[p];
    if (EPI == EPI_SPLIT2 && n >= e.col_split)
        *reinterpret_cast<f32x4*>(e.C2 + (long)m * e.ldc2 + (n - e.col_split)) = o;
    else
        epi_store4(e.C, c_row(m) * e.ldc + n, o, e.c_bf16);
    if (EPI == EPI_ACT) {
        f32x4 a;
#pragma unroll
        for (int c = 0; c < 4; ++c) a[c] = gelu_f(o[c]);
        epi_store4(e.Cact, (long)m * e.ldact + n, a, e.c_bf16);
    }
}

// PRE16: gelu_pre is stored as bf16 (EPI_GELUBWD) -- compile-time, so that the four auxiliary loads of a fragment stay in one
// basic block and are issued back to back.
// FDIV: the row split of rm_on by multiply-high with the reciprocals m_hw, m_w2 of rm_H2 * rm_W2 and rm_W2 (fdiv, common.h; the
// kernels of the FAST gather sources, which carry them: the launch's host side has checked fdiv's bound for M + 63 rows).
// Compile-time, and off for the dense kernels, whose epilogue and Epilogue struct are exactly what they were: hoisting their row
// divisions cost the residual-epilogue kernels registers and a step of occupancy (profiles/conv_gather_notes.md).
// MAPPED (gemm.hip's row-mapped launches, vector path only): output row m of the launch is LOGICAL.  ord (NULL: the identity) lists
// the samples in the launch's order: with j = m / map_rps (by map_magic), sample ord[j] is the row_scale index and
// ord[j] * map_rps + (m - j * map_rps) the row of every matrix the epilogue addresses.  Rows from kept_rows on belong to dropped
// samples: their accumulators are zeros by construction, gelu_pre is not read for them, and a residual epilogue stores their
// residual row as it is.
// The consume part: every fragment goes through the wave's LDS patch, meets its operands and is stored.  AHEAD: `first` already holds
// the operands of fragment (0, 0) (vector path); a later fragment's are requested while the one before it is computed and stored.
// Otherwise each fragment requests its own behind its transposition, the order these loads always had.
template <int EPI, int FM, int FN, bool PRE16 = false, bool FDIV = false, bool MAPPED = false, bool AHEAD = false>
__device__ __forceinline__ void run_epilogue(const Epilogue& e, f32x16 (&acc)[FM][FN], int M, int N, int mb, int nb,
                                             int lane, float* wbuf, bool vec, unsigned m_hw = 0, unsigned m_w2 = 0,
                                             const int* ord = nullptr, int kept_rows = 0, int map_rps = 1, unsigned map_magic = 0,
                                             const EpiOperands* first = nullptr) {
    const int rrow = lane >> 3, rcol = (lane & 7) * 4;
    const bool has_rs = e.row_scale != nullptr;
    auto out_row = [&](int m) -> long {           // class-local pixel -> row of the full (B, H*W, C) token matrix
        if (!e.rm_on) return m;
        const int hw = e.rm_H2 * e.rm_W2;
        int b, jy;
        if constexpr (FDIV) { b = fdiv1(m, m_hw); jy = fdiv1(m - b * hw, m_w2); }
        else { b = m / hw; jy = (m - b * hw) / e.rm_W2; }
        const int rem = m - b * hw;
        return ((long)b * e.rm_H + 2 * jy + e.rm_py) * e.rm_W + 2 * (rem - jy * e.rm_W2) + e.rm_px;
    };
    EpiOperands q;                                // the current fragment's operands (vector path)
    if constexpr (AHEAD) {
        if (vec) q = *first;
    }
#pragma unroll
    for (int i = 0; i < FM; ++i) {
#pragma unroll
        for (int j = 0; j < FN; ++j) {
            patch_put(wbuf, acc[i][j], lane);
            const int n = nb + j * 32 + rcol;
            if (vec) {
                EpiOperands nq;                            // AHEAD: the next fragment's operands, requested under this one's stores
                if constexpr (!AHEAD) epilogue_request<EPI, PRE16, MAPPED>(q, e, M, N, mb + i * 32, nb + j * 32, lane, ord, kept_rows, map_rps, map_magic);
                f32x4 v[4];
#pragma unroll
                for (int p = 0; p < 4; ++p) v[p] = *reinterpret_cast<const f32x4*>(&wbuf[(rrow + 8 * p) * EP_LD + rcol]);
                if constexpr (AHEAD && FM * FN > 1) {
                    const int f = i * FN + j + 1;
                    if (f < FM * FN) epilogue_request<EPI, PRE16, MAPPED>(nq, e, M, N, mb + (f / FN) * 32, nb + (f % FN) * 32, lane, ord, kept_rows, map_rps, map_magic);
                }
                int pm[4];    // MAPPED: the rows' places in memory; AHEAD: made again from ord in LDS, not held through the last k-tile
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    int smp;
                    pm[p] = (MAPPED && AHEAD) ? epi_mapped_row(mb + i * 32 + rrow + 8 * p, M, ord, map_rps, map_magic, smp) : q.pm[p];
                }
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const int m = mb + i * 32 + rrow + 8 * p;
                    if (m >= M || n >= N) continue;
                    if constexpr (MAPPED) {
                        static_assert(EPI != EPI_SPLIT2 && !PRE16 && !FDIV, "row-mapped launches: one fp32 output matrix");
                        f32x4 o = epi_value<EPI, PRE16>(q, p, v[p], has_rs);
                        if (EPI == EPI_RES && ord && m >= kept_rows) o = f32x4{0.f, 0.f, 0.f, 0.f};
                        if (EPI == EPI_RES) o += q.aux[p];
                        *reinterpret_cast<f32x4*>(e.C + (long)pm[p] * e.ldc + n) = o;
                        if (EPI == EPI_ACT) {
                            f32x4 a;
#pragma unroll
                            for (int c = 0; c < 4; ++c) a[c] = gelu_f(o[c]);
                            *reinterpret_cast<f32x4*>(e.Cact + (long)pm[p] * e.ldact + n) = a;
                        }
                    } else {
                        epi_consume_row<EPI, PRE16>(e, q, p, v[p], has_rs, m, n, out_row);
                    }
                }
                if constexpr (AHEAD && FM * FN > 1) q = nq;
            } else {
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const int m = mb + i * 32 + rrow + 8 * p;
                    if (m >= M) continue;
                    const float rsv = has_rs ? e.row_scale[m / e.rows_per_sample] : 1.0f;
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const int nn = n + c;
                        if (nn >= N) continue;
                        float o = wbuf[(rrow + 8 * p) * EP_LD + rcol + c] + (e.bias ? e.bias[nn] : 0.f);
                        if (EPI == EPI_GELUBWD) o *= gelu_grad_f(e.gelu_pre[(long)m * e.ldpre + nn]);
                        o *= rsv;
                        if (EPI == EPI_RES) o += e.residual[(long)m * e.ldres + nn];
                        if (EPI == EPI_SPLIT2 && nn >= e.col_split) e.C2[(long)m * e.ldc2 + (nn - e.col_split)] = o;
                        else e.C[out_row(m) * e.ldc + nn] = o;
                        if (EPI == EPI_ACT) e.Cact[(long)m * e.ldact + nn] = gelu_f(o);
                    }
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
    }
}


inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// every output / auxiliary operand the epilogue has starts 16-B aligned: what gemm_plan.h's Linear plans ask about the pointers (with
// the sizes, which they take themselves, this is epilogue_vec_ok)
inline bool epilogue_ptrs_aligned(const Epilogue& e) {
    return aligned16(e.C) && aligned16(e.C2) && aligned16(e.bias) && aligned16(e.Cact) && aligned16(e.residual) && aligned16(e.gelu_pre);
}

// 16-B epilogue accesses are legal when every row of every output / auxiliary operand starts 16-B aligned
inline int epilogue_vec_ok(const Epilogue& e, int n_out) {
    auto ok = [](const void* p, long ld) { return !p || (aligned16(p) && ld % 4 == 0); };
    return n_out % 4 == 0 && aligned16(e.C) && e.ldc % 4 == 0 && ok(e.C2, e.ldc2) && (!e.C2 || e.col_split % 4 == 0) &&
           ok(e.bias, 4) && ok(e.Cact, e.ldact) && ok(e.residual, e.ldres) && ok(e.gelu_pre, e.ldpre) &&
           e.split_stride % 4 == 0;
}

}  // namespace
