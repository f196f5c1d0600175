// AdamW with global-norm clipping and per-tensor learning rates over the flat buffers (the optimiser of the continual-learning
// loop: universal_train.py:693-725 AdamW(weight_decay=0.01) after clip_grad_norm_(parameters, 1.0), :934-939).  Three launches,
// no host synchronisation, instead of clip_grad_norm_ + torch.optim.AdamW over 463 tensors.
//
// All three kernels walk the static chunk table of flat_chunks.h (one 256-thread workgroup per chunk, an f32x4 body and a scalar
// tail of at most three elements, no pad word read or written), where the sums' fixed order is written down:
//
//   cswin_chunk_sumsq   partial[c] = (sum g^2, sum p^2) over chunk c
//   cswin_norm_finalize tensor_sumsq[t] = the tensor's chunk partials added in chunk order; their first column added in tensor
//                       order; scalars = [total_norm, clip_coef], total_norm = grad_scale * sqrt(sum), clip_coef =
//                       min(1, max_norm / (total_norm + 1e-6))  (torch.nn.utils.clip_grad_norm_'s rule)
//   cswin_adamw_flat    per element of tensor t, in torch.optim.AdamW's order:
//                         g'   = g * (grad_scale * clip_coef)
//                         m    = b1 m + (1 - b1) g' ;  v = b2 v + (1 - b2) g'^2
//                         lr_t = lr_dev[0] * lr_mult[t]
//                         p    = p (1 - lr_t wd) - (lr_t / bc1) * m / (sqrt(v) / sqrt(bc2) + eps)
//                         shadow = bf16_rne(p)
//                       lr_mult[t] == 0 exactly: p and its shadow are NOT stored (bit-identical), m and v still move.
//
// Non-finite gradients: a NaN is REPORTED, not repaired, exactly as torch has it.  One +inf gradient makes total_norm inf and
// clip_coef 0; that element's g' is inf * 0 = NaN (its m, v and p become NaN), every other g' is 0.  A NaN gradient makes
// total_norm and clip_coef NaN (the comparison that forms the minimum keeps it) and with them every g'.
#include "flat_chunks.h"

namespace {

__global__ __launch_bounds__(256) void chunk_sumsq_kernel(const float* __restrict__ g, const float* __restrict__ p,
                                                           const FlatChunk* __restrict__ chunks, float* __restrict__ partial) {
    const FlatChunk c = chunks[blockIdx.x];
    const float* gp = g + c.off;
    const float* pp = p ? p + c.off : nullptr;
    chunk_sums(c.n, pp != nullptr, partial,
        [&](int i, f32x4& ag, f32x4& ap) {
            const f32x4 x = reinterpret_cast<const f32x4*>(gp)[i];
            ag += x * x;
            if (pp) {
                const f32x4 y = reinterpret_cast<const f32x4*>(pp)[i];
                ap += y * y;
            }
        },
        [&](int it, float& sg, float& sp) {
            sg += gp[it] * gp[it];
            if (pp) sp += pp[it] * pp[it];
        });
}

// one workgroup: flat_chunks.h's two finalize steps, then the clip coefficient
__global__ __launch_bounds__(256) void norm_finalize_kernel(const float* __restrict__ partial, const int* __restrict__ first_chunk, int ntensors,
                                                             float grad_scale, float max_norm, float* __restrict__ tensor_sumsq,
                                                             float* __restrict__ scalars) {
    float total = 0.f;
    for (int base = 0; base < ntensors; base += 256) {
        const int t = base + threadIdx.x;
        float sg = 0.f, sp = 0.f;
        if (t < ntensors) {
            tensor_sums(partial, first_chunk, t, true, sg, sp);
            tensor_sumsq[2 * (long)t] = sg;
            tensor_sumsq[2 * (long)t + 1] = sp;
        }
        tensor_order_add(total, sg, base, ntensors);
    }
    if (threadIdx.x == 0) {
        const float norm = grad_scale * sqrtf(total);
        scalars[0] = norm;
        scalars[1] = clip_coef(max_norm, norm);
    }
}

struct AdamArgs { AdamBetas k; float wd, grad_scale, bc1, inv_sqrt_bc2; };

__device__ __forceinline__ void adamw_elem(float& p, float g, float& m, float& v, float gsc, float step, float decay, const AdamArgs& a) {
    p = p * decay - step * adam_quotient(m, v, g * gsc, a.k, a.inv_sqrt_bc2);
}

__global__ __launch_bounds__(256) void adamw_flat_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                          float* __restrict__ v, const FlatChunk* __restrict__ chunks,
                                                          const float* __restrict__ lr_dev, const float* __restrict__ lr_mult,
                                                          const float* __restrict__ scalars, AdamArgs a, __bf16* __restrict__ shadow) {
    const FlatChunk c = chunks[blockIdx.x];
    const float mult = lr_mult ? lr_mult[c.tensor] : 1.f;
    const float lr_t = lr_mult ? lr_dev[0] * mult : lr_dev[0];
    const float gsc = scalars ? a.grad_scale * scalars[1] : a.grad_scale;
    const float step = lr_t / a.bc1;
    const float decay = 1.f - lr_t * a.wd;
    const bool frozen = lr_mult && mult == 0.f;              // keeps p and its shadow bit for bit: their stores are skipped
    float* pp = p + c.off;
    const float* gp = g + c.off;
    float* mp = m + c.off;
    float* vp = v + c.off;
    __bf16* sp = shadow ? shadow + c.off : nullptr;
    const int it = chunk_walk(c.n, [&](int i) {
        f32x4 pv = reinterpret_cast<f32x4*>(pp)[i];
        const f32x4 gv = reinterpret_cast<const f32x4*>(gp)[i];
        f32x4 mv = reinterpret_cast<f32x4*>(mp)[i];
        f32x4 vv = reinterpret_cast<f32x4*>(vp)[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float pe = pv[e], me = mv[e], ve = vv[e];
            adamw_elem(pe, gv[e], me, ve, gsc, step, decay, a);
            pv[e] = pe, mv[e] = me, vv[e] = ve;
        }
        reinterpret_cast<f32x4*>(mp)[i] = mv;
        reinterpret_cast<f32x4*>(vp)[i] = vv;
        if (!frozen) {
            reinterpret_cast<f32x4*>(pp)[i] = pv;
            if (sp) reinterpret_cast<bf16x4*>(sp)[i] = __builtin_convertvector(pv, bf16x4);
        }
    });
    if (it < c.n) {
        float pe = pp[it], me = mp[it], ve = vp[it];
        adamw_elem(pe, gp[it], me, ve, gsc, step, decay, a);
        mp[it] = me;
        vp[it] = ve;
        if (!frozen) {
            pp[it] = pe;
            if (sp) sp[it] = (__bf16)pe;
        }
    }
}

}  // namespace

extern "C" {

int cswin_chunk_sumsq(const float* g, const float* p, const void* chunks, int nchunks, float* partial, void* stream) {
    CSWIN_REQUIRE(g && chunks && partial && nchunks > 0, CSWIN_ERR_SHAPE, "chunk_sumsq: bad arguments");
    if (int e = flat_align_check("chunk_sumsq", (uintptr_t)g | (uintptr_t)p, chunks, nullptr)) return e;
    hipLaunchKernelGGL(chunk_sumsq_kernel, dim3(nchunks), dim3(256), 0, (hipStream_t)stream, g, p, (const FlatChunk*)chunks, partial);
    CSWIN_LAUNCH_CHECK();
    return CSWIN_OK;
}

int cswin_norm_finalize(const float* partial, const int* first_chunk, int ntensors, float grad_scale, float max_norm,
                        float* tensor_sumsq, float* scalars, void* stream) {
    CSWIN_REQUIRE(partial && first_chunk && tensor_sumsq && scalars && ntensors > 0, CSWIN_ERR_SHAPE, "norm_finalize: bad arguments");
    hipLaunchKernelGGL(norm_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partial, first_chunk, ntensors, grad_scale, max_norm,
                       tensor_sumsq, scalars);
    CSWIN_LAUNCH_CHECK();
    return CSWIN_OK;
}

int cswin_adamw_flat(float* p, const float* g, float* m, float* v, const void* chunks, int nchunks, const float* lr_dev,
                     const float* lr_mult, const float* scalars, double beta1, double beta2, double eps, float weight_decay,
                     float grad_scale, double bc1, double bc2, void* shadow_bf16, void* stream) {
    CSWIN_REQUIRE(p && g && m && v && chunks && lr_dev && nchunks > 0, CSWIN_ERR_SHAPE, "adamw_flat: bad arguments");
    CSWIN_REQUIRE(bc1 > 0.0 && bc2 > 0.0, CSWIN_ERR_SHAPE, "adamw_flat: the bias corrections 1 - beta^t must be positive (bc1 %g, bc2 %g)", bc1, bc2);
    if (int e = flat_align_check("adamw_flat", (uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v, chunks, shadow_bf16)) return e;
    AdamArgs a;
    a.k = {(float)beta1, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps};
    a.wd = weight_decay, a.grad_scale = grad_scale, a.bc1 = (float)bc1, a.inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
    hipLaunchKernelGGL(adamw_flat_kernel, dim3(nchunks), dim3(256), 0, (hipStream_t)stream, p, g, m, v, (const FlatChunk*)chunks, lr_dev, lr_mult,
                       scalars, a, (__bf16*)shadow_bf16);
    CSWIN_LAUNCH_CHECK();
    return CSWIN_OK;
}

}  // extern "C"
