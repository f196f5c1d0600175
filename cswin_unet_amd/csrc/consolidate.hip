// Quadratic consolidation penalties of the continual-learning loop on the flat buffers: EWC (empirical Fisher importance), MAS
// (importance from the gradient of the squared output norm) and L2-SP (importance 1, no importance buffer).  With the anchor
// theta*, the importance F >= 0 (one float per weight), a weight w_t per tensor (0: excluded) and the strength lambda:
//
//   penalty         = (lambda / 2) sum_t w_t sum_{i in t} F_i (theta_i - theta*_i)^2
//   dpenalty/dtheta = lambda w_t F_i (theta_i - theta*_i)          added to the flat gradient BEFORE the optimiser launch
//
// The optimisers multiply the flat gradient by grad_scale, so the kernel adds (lambda w_t penalty_scale) F d with penalty_scale =
// 1 / grad_scale.  Four launches walk the static chunk table of flat_chunks.h (one 256-thread workgroup per chunk, an f32x4 body
// and a scalar tail of at most three elements, no pad word read or written):
//
//   cswin_importance_accumulate  imp += (grad_scale g)^2  or  |grad_scale g|         (the estimation pass)
//   cswin_flat_axpby             dst = a dst + b src                                  (the 1 / n normalisation, the online decay)
//   cswin_consolidate_chunks     g += c_t F d  and  partial[c] = (sum F d^2, sum d^2) over chunk c
//   cswin_consolidate_finalize   one workgroup, thread k owns tensors k, k + 256, ...: the chunk partials added in chunk order, the
//                                tensors in tensor order
//
// There is no float atomic and no host synchronisation: lambda is read from device memory, every sum has flat_chunks.h's fixed
// order, so two runs give the same bits.  Non-finite values are reported (they reach the sums), not repaired.
#include "flat_chunks.h"

namespace {

template <bool ABS>
__global__ __launch_bounds__(256) void importance_accumulate_kernel(const float* __restrict__ g, float* __restrict__ imp,
                                                                     const FlatChunk* __restrict__ chunks, float grad_scale) {
    const FlatChunk c = chunks[blockIdx.x];
    const float* gp = g + c.off;
    float* ip = imp + c.off;
    const int it = chunk_walk(c.n, [&](int i) {
        const f32x4 x = reinterpret_cast<const f32x4*>(gp)[i] * grad_scale;
        f32x4 v = reinterpret_cast<f32x4*>(ip)[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = ABS ? v[e] + fabsf(x[e]) : fmaf(x[e], x[e], v[e]);
        reinterpret_cast<f32x4*>(ip)[i] = v;
    });
    if (it < c.n) {
        const float x = gp[it] * grad_scale;
        ip[it] = ABS ? ip[it] + fabsf(x) : fmaf(x, x, ip[it]);
    }
}

// src may be null: dst = a dst
__global__ __launch_bounds__(256) void flat_axpby_kernel(float* __restrict__ dst, const float* __restrict__ src,
                                                          const FlatChunk* __restrict__ chunks, float a, float b) {
    const FlatChunk c = chunks[blockIdx.x];
    float* dp = dst + c.off;
    const float* sp = src ? src + c.off : nullptr;
    const int it = chunk_walk(c.n, [&](int i) {
        f32x4 v = reinterpret_cast<f32x4*>(dp)[i] * a;
        if (sp) {
            const f32x4 s = reinterpret_cast<const f32x4*>(sp)[i];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = fmaf(b, s[e], v[e]);
        }
        reinterpret_cast<f32x4*>(dp)[i] = v;
    });
    if (it < c.n) {
        const float v = dp[it] * a;
        dp[it] = sp ? fmaf(b, sp[it], v) : v;
    }
}

// imp null: importance 1 (L2-SP).  g null, or a coefficient of exactly 0 (lambda = 0, an excluded tensor): nothing is stored, so
// the gradient keeps its bits, a -0.0 included (fmaf(0, t, -0.0) would be +0.0)
__global__ __launch_bounds__(256) void consolidate_chunks_kernel(const float* __restrict__ p, const float* __restrict__ anchor,
                                                                  const float* __restrict__ imp, float* __restrict__ g,
                                                                  const FlatChunk* __restrict__ chunks, const float* __restrict__ lam,
                                                                  const float* __restrict__ tensor_weight, float penalty_scale,
                                                                  float* __restrict__ partial) {
    const FlatChunk c = chunks[blockIdx.x];
    const float coef = (lam[0] * tensor_weight[c.tensor]) * penalty_scale;
    const float* pp = p + c.off;
    const float* ap = anchor + c.off;
    const float* ip = imp ? imp + c.off : nullptr;
    float* gp = (g && coef != 0.f) ? g + c.off : nullptr;
    chunk_sums(c.n, true, partial,
        [&](int i, f32x4& afd, f32x4& add) {
            const f32x4 d = reinterpret_cast<const f32x4*>(pp)[i] - reinterpret_cast<const f32x4*>(ap)[i];
            const f32x4 t = ip ? reinterpret_cast<const f32x4*>(ip)[i] * d : d;
            afd += t * d;
            add += d * d;
            if (gp) {
                f32x4 gv = reinterpret_cast<f32x4*>(gp)[i];
#pragma unroll
                for (int e = 0; e < 4; ++e) gv[e] = fmaf(coef, t[e], gv[e]);
                reinterpret_cast<f32x4*>(gp)[i] = gv;
            }
        },
        [&](int it, float& sfd, float& sdd) {
            const float d = pp[it] - ap[it];
            const float t = ip ? ip[it] * d : d;
            sfd += t * d;
            sdd += d * d;
            if (gp) gp[it] = fmaf(coef, t, gp[it]);
        });
}

__global__ __launch_bounds__(256) void consolidate_finalize_kernel(const float* __restrict__ partial, const int* __restrict__ first_chunk,
                                                                    int ntensors, const float* __restrict__ lam,
                                                                    const float* __restrict__ tensor_weight, float* __restrict__ per_tensor,
                                                                    float* __restrict__ scalars) {
    float weighted = 0.f, dist = 0.f;
    for (int base = 0; base < ntensors; base += 256) {
        const int t = base + threadIdx.x;
        float sfd = 0.f, sdd = 0.f, w = 0.f;
        if (t < ntensors) {
            tensor_sums(partial, first_chunk, t, true, sfd, sdd);
            per_tensor[2 * (long)t] = sfd;
            per_tensor[2 * (long)t + 1] = sdd;
            w = tensor_weight[t];
        }
        tensor_order_add(weighted, w * sfd, base, ntensors);
        tensor_order_add(dist, sdd, base, ntensors);
    }
    if (threadIdx.x == 0) {
        scalars[0] = (0.5f * lam[0]) * weighted;
        scalars[1] = weighted;
        scalars[2] = sqrtf(dist);
    }
}

}  // namespace

extern "C" {

int cswin_importance_accumulate(const float* g, float* imp, const void* chunks, int nchunks, double grad_scale, int statistic,
                                void* stream) {
    CSWIN_REQUIRE(g && imp && chunks && nchunks > 0, CSWIN_ERR_SHAPE, "importance_accumulate: bad arguments");
    CSWIN_REQUIRE(statistic == 0 || statistic == 1, CSWIN_ERR_SHAPE, "importance_accumulate: statistic %d (0: squares, 1: absolute values)", statistic);
    if (int e = flat_align_check("importance_accumulate", (uintptr_t)g | (uintptr_t)imp, chunks, nullptr)) return e;
    if (statistic)
        hipLaunchKernelGGL(importance_accumulate_kernel<true>, dim3(nchunks), dim3(256), 0, (hipStream_t)stream, g, imp, (const FlatChunk*)chunks, (float)grad_scale);
    else
        hipLaunchKernelGGL(importance_accumulate_kernel<false>, dim3(nchunks), dim3(256), 0, (hipStream_t)stream, g, imp, (const FlatChunk*)chunks, (float)grad_scale);
    CSWIN_LAUNCH_CHECK();
    return CSWIN_OK;
}

int cswin_flat_axpby(float* dst, const float* src, const void* chunks, int nchunks, double a, double b, void* stream) {
    CSWIN_REQUIRE(dst && chunks && nchunks > 0, CSWIN_ERR_SHAPE, "flat_axpby: bad arguments");
    if (int e = flat_align_check("flat_axpby", (uintptr_t)dst | (uintptr_t)src, chunks, nullptr)) return e;
    hipLaunchKernelGGL(flat_axpby_kernel, dim3(nchunks), dim3(256), 0, (hipStream_t)stream, dst, src, (const FlatChunk*)chunks, (float)a, (float)b);
    CSWIN_LAUNCH_CHECK();
    return CSWIN_OK;
}

int cswin_consolidate_chunks(const float* p, const float* anchor, const float* imp, float* g, const void* chunks, int nchunks,
                             const float* lam, const float* tensor_weight, double penalty_scale, float* partial, void* stream) {
    CSWIN_REQUIRE(p && anchor && chunks && lam && tensor_weight && partial && nchunks > 0, CSWIN_ERR_SHAPE, "consolidate_chunks: bad arguments");
    if (int e = flat_align_check("consolidate_chunks", (uintptr_t)p | (uintptr_t)anchor | (uintptr_t)imp | (uintptr_t)g, chunks, nullptr)) return e;
    hipLaunchKernelGGL(consolidate_chunks_kernel, dim3(nchunks), dim3(256), 0, (hipStream_t)stream, p, anchor, imp, g, (const FlatChunk*)chunks, lam,
                       tensor_weight, (float)penalty_scale, partial);
    CSWIN_LAUNCH_CHECK();
    return CSWIN_OK;
}

int cswin_consolidate_finalize(const float* partial, const int* first_chunk, int ntensors, const float* lam, const float* tensor_weight,
                               float* per_tensor, float* scalars, void* stream) {
    CSWIN_REQUIRE(partial && first_chunk && lam && tensor_weight && per_tensor && scalars && ntensors > 0, CSWIN_ERR_SHAPE,
                  "consolidate_finalize: bad arguments");
    hipLaunchKernelGGL(consolidate_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partial, first_chunk, ntensors, lam, tensor_weight,
                       per_tensor, scalars);
    CSWIN_LAUNCH_CHECK();
    return CSWIN_OK;
}

}  // extern "C"
