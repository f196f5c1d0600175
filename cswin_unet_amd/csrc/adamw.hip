// AdamW with global-norm clipping and per-tensor learning rates over the flat buffers (the optimiser of the continual-learning
// loop: universal_train.py:693-725 AdamW(weight_decay=0.01) after clip_grad_norm_(parameters, 1.0), :934-939).  Three launches,
// no host synchronisation, instead of clip_grad_norm_ + torch.optim.AdamW over 463 tensors.
//
// All three kernels walk one STATIC chunk table, built and uploaded once by the optimiser: records {element offset into the flat
// buffers, n <= 16384, tensor index}, one 256-thread workgroup each.  Chunks never cross a tensor and never cover the pad words
// between the 8-float slots, so a NaN in a pad word reaches nothing; slots are 8-float aligned and 16384 is a multiple of 4, so
// every chunk starts 16-B aligned: an f32x4 body and a scalar tail of at most three elements, as in sgd.hip.
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
// There is no float atomic anywhere: every sum has a fixed order (a thread's trips, the xor butterfly of a wave, the four waves
// as (w0 + w1) + (w2 + w3), chunks in chunk order, tensors in tensor order), so two runs on the same input give the same bits.
//
// Non-finite gradients: a NaN is REPORTED, not repaired, exactly as torch has it.  One +inf gradient makes total_norm inf and
// clip_coef 0; that element's g' is inf * 0 = NaN (its m, v and p become NaN), every other g' is 0.  A NaN gradient makes
// total_norm and clip_coef NaN (the comparison that forms the minimum keeps it) and with them every g'.
#include "common.h"

namespace {

struct AdamChunk { long long off; int n; int tensor; };      // 16 bytes
static_assert(sizeof(AdamChunk) == 16, "the chunk record is 16 bytes");

typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

// sum over the 256 threads of a workgroup, the same value in every thread: 6 butterfly levels inside a wave, then two levels
// over the four waves.  red: 4 floats of LDS per reduced value.
__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void chunk_sumsq_kernel(const float* __restrict__ g, const float* __restrict__ p,
                                                           const AdamChunk* __restrict__ chunks, float* __restrict__ partial) {
    __shared__ float red[8];
    const AdamChunk c = chunks[blockIdx.x];
    const float* gp = g + c.off;
    const float* pp = p ? p + c.off : nullptr;
    const int n4 = c.n >> 2;
    f32x4 ag = {0.f, 0.f, 0.f, 0.f}, ap = ag;
    for (int i = threadIdx.x; i < n4; i += 256) {
        const f32x4 x = reinterpret_cast<const f32x4*>(gp)[i];
        ag += x * x;
        if (pp) {
            const f32x4 y = reinterpret_cast<const f32x4*>(pp)[i];
            ap += y * y;
        }
    }
    float sg = (ag[0] + ag[1]) + (ag[2] + ag[3]), sp = (ap[0] + ap[1]) + (ap[2] + ap[3]);
    const int it = n4 * 4 + threadIdx.x;
    if (it < c.n) {
        sg += gp[it] * gp[it];
        if (pp) sp += pp[it] * pp[it];
    }
    sg = block_sum(sg, red);
    if (pp) sp = block_sum(sp, red + 4);
    if (threadIdx.x == 0) {
        partial[2 * (long)blockIdx.x] = sg;
        if (pp) partial[2 * (long)blockIdx.x + 1] = sp;
    }
}

// one workgroup; thread k owns tensors k, k + 256, ...; thread 0 adds each trip's tensor sums in tensor order
__global__ __launch_bounds__(256) void norm_finalize_kernel(const float* __restrict__ partial, const int* __restrict__ first_chunk, int ntensors,
                                                             float grad_scale, float max_norm, float* __restrict__ tensor_sumsq,
                                                             float* __restrict__ scalars) {
    __shared__ float slot[256];
    float total = 0.f;
    for (int base = 0; base < ntensors; base += 256) {
        const int t = base + threadIdx.x;
        float sg = 0.f, sp = 0.f;
        if (t < ntensors) {
            const int c1 = first_chunk[t + 1];
            for (int c = first_chunk[t]; c < c1; ++c) {
                sg += partial[2 * (long)c];
                sp += partial[2 * (long)c + 1];
            }
            tensor_sumsq[2 * (long)t] = sg;
            tensor_sumsq[2 * (long)t + 1] = sp;
        }
        slot[threadIdx.x] = sg;
        __syncthreads();
        if (threadIdx.x == 0) {
            const int cnt = ntensors - base < 256 ? ntensors - base : 256;
            for (int k = 0; k < cnt; ++k) total += slot[k];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float norm = grad_scale * sqrtf(total);
        const float c = max_norm / (norm + 1e-6f);
        scalars[0] = norm;
        scalars[1] = c > 1.f ? 1.f : c;                      // a NaN norm stays a NaN coefficient (torch.clamp keeps it too)
    }
}

struct AdamArgs { float b1, omb1, b2, omb2, eps, wd, grad_scale, bc1, inv_sqrt_bc2; };

__device__ __forceinline__ void adamw_elem(float& p, float g, float& m, float& v, float gsc, float step, float decay, const AdamArgs& a) {
    const float gg = g * gsc;
    m = fmaf(a.b1, m, a.omb1 * gg);
    v = fmaf(a.b2, v, a.omb2 * (gg * gg));
    const float denom = fmaf(sqrtf(v), a.inv_sqrt_bc2, a.eps);
    p = p * decay - step * (m / denom);
}

__global__ __launch_bounds__(256) void adamw_flat_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                          float* __restrict__ v, const AdamChunk* __restrict__ chunks,
                                                          const float* __restrict__ lr_dev, const float* __restrict__ lr_mult,
                                                          const float* __restrict__ scalars, AdamArgs a, __bf16* __restrict__ shadow) {
    const AdamChunk c = chunks[blockIdx.x];
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
    const int n4 = c.n >> 2;
    for (int i = threadIdx.x; i < n4; i += 256) {
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
    }
    const int it = n4 * 4 + threadIdx.x;
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
    CSWIN_REQUIRE(((((uintptr_t)g) | ((uintptr_t)p)) & 15) == 0, CSWIN_ERR_ALIGN, "chunk_sumsq: buffers must be 16-B aligned");
    CSWIN_REQUIRE((((uintptr_t)chunks) & 7) == 0, CSWIN_ERR_ALIGN, "chunk_sumsq: the chunk table must be 8-B aligned");
    hipLaunchKernelGGL(chunk_sumsq_kernel, dim3(nchunks), dim3(256), 0, (hipStream_t)stream, g, p, (const AdamChunk*)chunks, partial);
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
    CSWIN_REQUIRE(((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)m) | ((uintptr_t)v)) & 15) == 0, CSWIN_ERR_ALIGN, "adamw_flat: buffers must be 16-B aligned");
    CSWIN_REQUIRE((((uintptr_t)chunks) & 7) == 0, CSWIN_ERR_ALIGN, "adamw_flat: the chunk table must be 8-B aligned");
    CSWIN_REQUIRE(!shadow_bf16 || (((uintptr_t)shadow_bf16) & 7) == 0, CSWIN_ERR_ALIGN, "adamw_flat: the bf16 shadow must be 8-B aligned");
    AdamArgs a;
    a.b1 = (float)beta1, a.omb1 = (float)(1.0 - beta1), a.b2 = (float)beta2, a.omb2 = (float)(1.0 - beta2);
    a.eps = (float)eps, a.wd = weight_decay, a.grad_scale = grad_scale, a.bc1 = (float)bc1, a.inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
    hipLaunchKernelGGL(adamw_flat_kernel, dim3(nchunks), dim3(256), 0, (hipStream_t)stream, p, g, m, v, (const AdamChunk*)chunks, lr_dev, lr_mult,
                       scalars, a, (__bf16*)shadow_bf16);
    CSWIN_LAUNCH_CHECK();
    return CSWIN_OK;
}

}  // extern "C"
