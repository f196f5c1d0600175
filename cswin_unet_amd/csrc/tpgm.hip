// TPGM on the flat buffers (the trainable projection of the continual-learning loop: universal_train.py:391-615, and tpgm.py:47-56
// for the gradient the projection radii receive).  Every fine-tuned tensor t is kept inside a ball around its pretrained value:
//
//   d       = p - anchor                              norm_t = sqrt(sum d^2)  (l2)   or   sum |d|  (l1: ONE scalar per tensor)
//   cmax_t  = max(8 norm_t, 80)                       head tensors: max(10 norm_t, 100)
//   c_t     = clamp(gamma_t, 1e-2, cmax_t)            ratio_t = hardtanh(c_t / (norm_t + 1e-8), 0, 1)
//   ptilde  = anchor + ratio_t d
//   dL/dgamma_t = (sum gtilde d) / (norm_t + 1e-8)    where 1e-2 <= gamma_t <= cmax_t and 0 < c_t / (norm_t + 1e-8) < 1, else 0
//                                                     (torch's clamp passes its bounds, its hardtanh does not)
//
// Three launches walk the static chunk table of flat_chunks.h (one 256-thread workgroup per chunk, an f32x4 body and a scalar tail
// of at most three elements, no pad word read or written):
//
//   cswin_tpgm_chunk_stats  partial[c] = (sum d^2 or sum |d|, sum g d) over chunk c
//   cswin_tpgm_finalize     one workgroup, thread k owns tensors k, k + 256, ...: the chunk partials added in chunk order, then
//                           either the ratios of the current gamma, or clip_grad_norm_(gamma, 1) + one torch.optim.Adam step on
//                           gamma (betas 0.9 / 0.999, eps 1e-8, no decay) and the ratios of the new gamma
//   cswin_tpgm_project      dst = anchor + ratio_t (src - anchor), and its bf16 shadow; a tensor whose ratio is exactly 1 keeps
//                           src's bits (anchor + 1 (src - anchor) is not src in fp32, and a tensor inside its ball must not drift)
//
// There is no float atomic and no host synchronisation: every sum has flat_chunks.h's fixed order, so two runs give the same bits.
// A non-finite gradient is reported, not repaired: it makes the gamma-gradient norm, the clip coefficient and every gamma NaN.
#include "flat_chunks.h"

namespace {

constexpr int FLAG_EXCLUDED = 1, FLAG_HEAD = 2;
constexpr float GAMMA_MIN = 1e-2f, NORM_EPS = 1e-8f;

template <bool L1>
__global__ __launch_bounds__(256) void tpgm_chunk_stats_kernel(const float* __restrict__ p, const float* __restrict__ anchor,
                                                                const float* __restrict__ g, const FlatChunk* __restrict__ chunks,
                                                                float* __restrict__ partial) {
    const FlatChunk c = chunks[blockIdx.x];
    const float* pp = p + c.off;
    const float* ap = anchor + c.off;
    const float* gp = g ? g + c.off : nullptr;
    chunk_sums(c.n, gp != nullptr, partial,
        [&](int i, f32x4& an, f32x4& ad) {
            const f32x4 d = reinterpret_cast<const f32x4*>(pp)[i] - reinterpret_cast<const f32x4*>(ap)[i];
            if (L1) {
#pragma unroll
                for (int e = 0; e < 4; ++e) an[e] += fabsf(d[e]);
            } else {
                an += d * d;
            }
            if (gp) ad += reinterpret_cast<const f32x4*>(gp)[i] * d;
        },
        [&](int it, float& sn, float& sd) {
            const float d = pp[it] - ap[it];
            sn += L1 ? fabsf(d) : d * d;
            if (gp) sd += gp[it] * d;
        });
}

__device__ __forceinline__ float tpgm_cmax(float norm, int flags) {
    return (flags & FLAG_HEAD) ? fmaxf(10.f * norm, 100.f) : fmaxf(8.f * norm, 80.f);
}

// hardtanh(clamp(gamma, 1e-2, cmax) / (norm + 1e-8), 0, 1); live: the gradient reaches gamma (a NaN gamma gives a NaN ratio)
__device__ __forceinline__ float tpgm_ratio(float gamma, float norm, int flags, bool& live) {
    const float cmax = tpgm_cmax(norm, flags);
    const float c = gamma < GAMMA_MIN ? GAMMA_MIN : (gamma > cmax ? cmax : gamma);
    const float r = c / (norm + NORM_EPS);
    live = gamma >= GAMMA_MIN && gamma <= cmax && r > 0.f && r < 1.f;
    return r < 0.f ? 0.f : (r > 1.f ? 1.f : r);
}

struct FinalizeArgs { float grad_scale, step, inv_sqrt_bc2; int l1, update; };

// thread k owns tensors k, k + 256, ... in both passes, so what it leaves in ratio[] / norm[] for itself needs no fence
__global__ __launch_bounds__(256) void tpgm_finalize_kernel(const float* __restrict__ partial, const int* __restrict__ first_chunk, int ntensors,
                                                             const int* __restrict__ flags, float* __restrict__ gamma, float* __restrict__ gm,
                                                             float* __restrict__ gv, FinalizeArgs a, float* __restrict__ ratio,
                                                             float* __restrict__ norm, float* __restrict__ scalars) {
    __shared__ float coef_s;
    float total = 0.f;
    for (int base = 0; base < ntensors; base += 256) {
        const int t = base + threadIdx.x;
        float dg = 0.f;
        if (t < ntensors) {
            float sn, sd;
            tensor_sums(partial, first_chunk, t, a.update, sn, sd);
            const float nt = a.l1 ? sn : sqrtf(sn);
            norm[t] = nt;
            const int f = flags[t];
            bool live = false;
            const float r = tpgm_ratio(gamma[t], nt, f, live);
            if (a.update) {
                if (!(f & FLAG_EXCLUDED) && live) dg = (a.grad_scale * sd) / (nt + NORM_EPS);
                ratio[t] = dg;                               // parked for the second pass
            } else {
                ratio[t] = (f & FLAG_EXCLUDED) ? 1.f : r;
            }
        }
        if (!a.update) continue;                             // uniform over the workgroup
        tensor_order_add(total, dg * dg, base, ntensors);
    }
    if (!a.update) return;
    if (threadIdx.x == 0) {
        const float gnorm = sqrtf(total);
        coef_s = clip_coef(1.f, gnorm);                      // clip_grad_norm_(gamma, 1.0)
        scalars[0] = gnorm;
        scalars[1] = coef_s;
    }
    __syncthreads();
    const float coef = coef_s;
    constexpr AdamBetas ADAM = {0.9f, (float)(1.0 - 0.9), 0.999f, (float)(1.0 - 0.999), 1e-8f};      // torch.optim.Adam's defaults
    for (int t = threadIdx.x; t < ntensors; t += 256) {
        const int f = flags[t];
        if (f & FLAG_EXCLUDED) {
            ratio[t] = 1.f;
            continue;
        }
        const float gg = ratio[t] * coef;                    // a zero gradient is still a gradient: gamma moves by its momentum
        float m = gm[t], v = gv[t];
        const float gn = gamma[t] - a.step * adam_quotient(m, v, gg, ADAM, a.inv_sqrt_bc2);
        gm[t] = m, gv[t] = v, gamma[t] = gn;
        bool live;
        ratio[t] = tpgm_ratio(gn, norm[t], f, live);
    }
}

// src and dst may be the same buffer (the in-place projection): every element is read and written by one thread
__global__ __launch_bounds__(256) void tpgm_project_kernel(const float* src, const float* __restrict__ anchor, float* dst,
                                                            const float* __restrict__ ratio, const FlatChunk* __restrict__ chunks,
                                                            __bf16* __restrict__ shadow) {
    const FlatChunk c = chunks[blockIdx.x];
    const float r = ratio[c.tensor];
    const bool keep = r == 1.f;                              // src's bits: copied, or (in place) nothing stored
    if (keep && src == dst) return;
    const float* sp = src + c.off;
    const float* ap = anchor + c.off;
    float* dp = dst + c.off;
    __bf16* hp = shadow ? shadow + c.off : nullptr;
    const int it = chunk_walk(c.n, [&](int i) {
        f32x4 s = reinterpret_cast<const f32x4*>(sp)[i];
        if (!keep) {
            const f32x4 av = reinterpret_cast<const f32x4*>(ap)[i];
#pragma unroll
            for (int e = 0; e < 4; ++e) s[e] = fmaf(r, s[e] - av[e], av[e]);
        }
        reinterpret_cast<f32x4*>(dp)[i] = s;
        if (hp) reinterpret_cast<bf16x4*>(hp)[i] = __builtin_convertvector(s, bf16x4);
    });
    if (it < c.n) {
        float s = sp[it];
        if (!keep) s = fmaf(r, s - ap[it], ap[it]);
        dp[it] = s;
        if (hp) hp[it] = (__bf16)s;
    }
}

}  // namespace

extern "C" {

int cswin_tpgm_chunk_stats(const float* p, const float* anchor, const float* g, const void* chunks, int nchunks, int l1, float* partial,
                           void* stream) {
    CSWIN_REQUIRE(p && anchor && chunks && partial && nchunks > 0, CSWIN_ERR_SHAPE, "tpgm_chunk_stats: bad arguments");
    if (int e = flat_align_check("tpgm_chunk_stats", (uintptr_t)p | (uintptr_t)anchor | (uintptr_t)g, chunks, nullptr)) return e;
    if (l1)
        hipLaunchKernelGGL(tpgm_chunk_stats_kernel<true>, dim3(nchunks), dim3(256), 0, (hipStream_t)stream, p, anchor, g, (const FlatChunk*)chunks, partial);
    else
        hipLaunchKernelGGL(tpgm_chunk_stats_kernel<false>, dim3(nchunks), dim3(256), 0, (hipStream_t)stream, p, anchor, g, (const FlatChunk*)chunks, partial);
    CSWIN_LAUNCH_CHECK();
    return CSWIN_OK;
}

int cswin_tpgm_finalize(const float* partial, const int* first_chunk, int ntensors, int l1, const int* flags, float* gamma, float* gm,
                        float* gv, double grad_scale, double proj_lr, double bc1, double bc2, int mode, float* ratio, float* norm,
                        float* scalars, void* stream) {
    CSWIN_REQUIRE(partial && first_chunk && flags && gamma && ratio && norm && ntensors > 0, CSWIN_ERR_SHAPE, "tpgm_finalize: bad arguments");
    CSWIN_REQUIRE(mode == 0 || mode == 1, CSWIN_ERR_SHAPE, "tpgm_finalize: mode %d (0: ratios, 1: update)", mode);
    FinalizeArgs a;
    a.l1 = l1 != 0, a.update = mode, a.grad_scale = 1.f, a.step = 0.f, a.inv_sqrt_bc2 = 1.f;
    if (mode == 1) {
        CSWIN_REQUIRE(gm && gv && scalars, CSWIN_ERR_SHAPE, "tpgm_finalize: the update needs the Adam moments and scalars");
        CSWIN_REQUIRE(bc1 > 0.0 && bc2 > 0.0, CSWIN_ERR_SHAPE, "tpgm_finalize: the bias corrections 1 - beta^t must be positive (bc1 %g, bc2 %g)", bc1, bc2);
        a.grad_scale = (float)grad_scale, a.step = (float)proj_lr / (float)bc1, a.inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
    }
    hipLaunchKernelGGL(tpgm_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partial, first_chunk, ntensors, flags, gamma, gm, gv, a, ratio,
                       norm, scalars);
    CSWIN_LAUNCH_CHECK();
    return CSWIN_OK;
}

int cswin_tpgm_project(const float* src, const float* anchor, float* dst, const float* ratio, const void* chunks, int nchunks,
                       void* shadow_bf16, void* stream) {
    CSWIN_REQUIRE(src && anchor && dst && ratio && chunks && nchunks > 0, CSWIN_ERR_SHAPE, "tpgm_project: bad arguments");
    if (int e = flat_align_check("tpgm_project", (uintptr_t)src | (uintptr_t)anchor | (uintptr_t)dst, chunks, shadow_bf16)) return e;
    hipLaunchKernelGGL(tpgm_project_kernel, dim3(nchunks), dim3(256), 0, (hipStream_t)stream, src, anchor, dst, ratio, (const FlatChunk*)chunks,
                       (__bf16*)shadow_bf16);
    CSWIN_LAUNCH_CHECK();
    return CSWIN_OK;
}

}  // extern "C"
