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
//
// The per-step rates of the surgical fine-tuning loop (finetune.py:116-144, 223-239) are two more entry points, added beside those:
//
//   cswin_rate_finalize cswin_norm_finalize's outputs, bit for bit, and then, over a static table of tensor groups (thread k owns
//                       groups k, k + 256, ...): a group's sum g^2 and sum p^2 = its tensors' added in the table's order;
//                       group_stat = grad_scale * sqrt(sum g^2), in the ratio mode divided by sqrt(sum p^2) where that is > 1e-8,
//                       else 0; top = the maximum over the groups in group order; lr_mult[t] = group_stat[group_of[t]] / top (all 0
//                       when top <= 0, all NaN when a statistic is NaN), default_mult for a tensor in no group
//   cswin_adam_flat     cswin_adamw_flat with `flags`: bit 0 = torch.optim.Adam's coupled L2 decay, g' = gsc g + wd p and no decay
//                       factor; bit 1 = fresh moments, m = v = 0 neither read nor written (a new optimiser every step).  flags 0 is
//                       cswin_adamw_flat itself: both launch the same kernel instance.
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
__device__ __forceinline__ void norm_finalize(const float* __restrict__ partial, const int* __restrict__ first_chunk, int ntensors, float grad_scale,
                                              float max_norm, float* tensor_sumsq, float* __restrict__ scalars) {
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

__global__ __launch_bounds__(256) void norm_finalize_kernel(const float* __restrict__ partial, const int* __restrict__ first_chunk, int ntensors,
                                                             float grad_scale, float max_norm, float* __restrict__ tensor_sumsq,
                                                             float* __restrict__ scalars) {
    norm_finalize(partial, first_chunk, ntensors, grad_scale, max_norm, tensor_sumsq, scalars);
}

// The static group table (optim.group_table builds and checks it): group k's tensors are group_tensors[group_first[k] ..
// group_first[k + 1] - 1], in tensor order; group_of[t] is tensor t's group or -1.
struct RateGroups { const int* first; const int* tensors; const int* of; int n; int statistic; float default_mult; };

// one workgroup: norm_finalize, then the groups' statistics, their maximum in group order and a multiplier per tensor
__global__ __launch_bounds__(256) void rate_finalize_kernel(const float* __restrict__ partial, const int* __restrict__ first_chunk, int ntensors,
                                                             float grad_scale, float max_norm, RateGroups gr, float* tensor_sumsq,
                                                             float* __restrict__ scalars, float* group_stat, float* __restrict__ lr_mult) {
    constexpr int ROWS = 2048;                               // table entries gathered at a time: 16 KB of LDS
    __shared__ float2 rows[ROWS];
    __shared__ float top_all;
    norm_finalize(partial, first_chunk, ntensors, grad_scale, max_norm, tensor_sumsq, scalars);
    __syncthreads();                                         // every tensor_sumsq row is visible to the workgroup from here on
    float top = -INFINITY;
    for (int base = 0; base < gr.n; base += 256) {
        const int k = base + threadIdx.x;
        const bool mine = k < gr.n;
        const int j0 = mine ? gr.first[k] : 0, j1 = mine ? gr.first[k + 1] : 0;
        // One thread walks a group of some 200 tensors here, and that walk over global memory was the kernel's time.  The entries
        // of this trip's groups are consecutive in the table: all threads gather their rows into LDS, in the table's order, and
        // each thread then adds its own group's from there, in that order.  An entry that names no tensor reads nothing and adds 0.
        const int e0 = gr.first[base], e1 = gr.first[base + 256 < gr.n ? base + 256 : gr.n];
        float sg = 0.f, sp = 0.f;
        for (int lo = e0; lo < e1; lo += ROWS) {
            const int hi = lo + ROWS < e1 ? lo + ROWS : e1;
            for (int j = lo + threadIdx.x; j < hi; j += 256) {
                const int t = gr.tensors[j];
                const bool ok = (unsigned)t < (unsigned)ntensors;
                rows[j - lo] = ok ? make_float2(tensor_sumsq[2 * (long)t], tensor_sumsq[2 * (long)t + 1]) : make_float2(0.f, 0.f);
            }
            __syncthreads();
            const int a = j0 > lo ? j0 : lo, b = j1 < hi ? j1 : hi;
#pragma unroll 8
            for (int j = a; j < b; ++j) sg += rows[j - lo].x, sp += rows[j - lo].y;
            __syncthreads();
        }
        float stat = 0.f;
        if (mine) {
            stat = grad_scale * sqrtf(sg);
            if (gr.statistic) {
                const float pn = sqrtf(sp);
                stat = pn > 1e-8f ? stat / pn : 0.f;
            }
            group_stat[k] = stat;
        }
        item_order_fold(top, stat, base, gr.n, nan_keeping_max);
    }
    if (threadIdx.x == 0) top_all = top;
    __syncthreads();                                         // and every group_stat
    top = top_all;
    for (int t = threadIdx.x; t < ntensors; t += 256) {
        const int k = gr.of[t];
        if ((unsigned)k >= (unsigned)gr.n) lr_mult[t] = gr.default_mult;
        else lr_mult[t] = top > 0.f ? group_stat[k] / top : (top == top ? 0.f : top);
    }
}

struct AdamArgs { AdamBetas k; float wd, grad_scale, bc1, inv_sqrt_bc2; };

// COUPLED: torch.optim.Adam's weight decay, grad.add(param, alpha=wd), and no decay factor; else AdamW's p * decay
template <bool COUPLED>
__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, float gsc, float step, float decay, const AdamArgs& a) {
    if constexpr (COUPLED) p = p - step * adam_quotient(m, v, fmaf(a.wd, p, g * gsc), a.k, a.inv_sqrt_bc2);
    else p = p * decay - step * adam_quotient(m, v, g * gsc, a.k, a.inv_sqrt_bc2);
}

// FRESH: m = v = 0 at every element, neither read nor written (m and v may be null); the caller's bc1, bc2 are those of step 1
template <bool COUPLED, bool FRESH>
__global__ __launch_bounds__(256) void adam_flat_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
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
    if (FRESH && frozen) return;                             // and without moments to move there is nothing to do
    float* pp = p + c.off;
    const float* gp = g + c.off;
    float* mp = FRESH ? nullptr : m + c.off;
    float* vp = FRESH ? nullptr : v + c.off;
    __bf16* sp = shadow ? shadow + c.off : nullptr;
    const int it = chunk_walk(c.n, [&](int i) {
        f32x4 pv = reinterpret_cast<f32x4*>(pp)[i];
        const f32x4 gv = reinterpret_cast<const f32x4*>(gp)[i];
        f32x4 mv = {0.f, 0.f, 0.f, 0.f}, vv = mv;
        if constexpr (!FRESH) {
            mv = reinterpret_cast<f32x4*>(mp)[i];
            vv = reinterpret_cast<f32x4*>(vp)[i];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float pe = pv[e], me = mv[e], ve = vv[e];
            adam_elem<COUPLED>(pe, gv[e], me, ve, gsc, step, decay, a);
            pv[e] = pe, mv[e] = me, vv[e] = ve;
        }
        if constexpr (!FRESH) {
            reinterpret_cast<f32x4*>(mp)[i] = mv;
            reinterpret_cast<f32x4*>(vp)[i] = vv;
        }
        if (!frozen) {
            reinterpret_cast<f32x4*>(pp)[i] = pv;
            if (sp) reinterpret_cast<bf16x4*>(sp)[i] = __builtin_convertvector(pv, bf16x4);
        }
    });
    if (it < c.n) {
        float pe = pp[it], me = 0.f, ve = 0.f;
        if constexpr (!FRESH) me = mp[it], ve = vp[it];
        adam_elem<COUPLED>(pe, gp[it], me, ve, gsc, step, decay, a);
        if constexpr (!FRESH) {
            mp[it] = me;
            vp[it] = ve;
        }
        if (!frozen) {
            pp[it] = pe;
            if (sp) sp[it] = (__bf16)pe;
        }
    }
}

constexpr int ADAM_COUPLED = 1, ADAM_FRESH = 2;              // cswin_adam_flat's flags

// what cswin_adamw_flat (flags 0) and cswin_adam_flat share: the checks, under the caller's name, and the launch
int adam_launch(const char* who, float* p, const float* g, float* m, float* v, const void* chunks, int nchunks, const float* lr_dev,
                const float* lr_mult, const float* scalars, double beta1, double beta2, double eps, float weight_decay, float grad_scale,
                double bc1, double bc2, int flags, void* shadow_bf16, void* stream) {
    CSWIN_REQUIRE((flags & ~(ADAM_COUPLED | ADAM_FRESH)) == 0, CSWIN_ERR_SHAPE, "%s: flags %d (bit 0: coupled L2 decay, bit 1: fresh moments)", who, flags);
    const bool fresh = flags & ADAM_FRESH;
    CSWIN_REQUIRE(p && g && (fresh || (m && v)) && chunks && lr_dev && nchunks > 0, CSWIN_ERR_SHAPE, "%s: bad arguments", who);
    CSWIN_REQUIRE(bc1 > 0.0 && bc2 > 0.0, CSWIN_ERR_SHAPE, "%s: the bias corrections 1 - beta^t must be positive (bc1 %g, bc2 %g)", who, bc1, bc2);
    const uintptr_t moments = fresh ? 0 : (uintptr_t)m | (uintptr_t)v;                   // fresh: not touched, so not asked for anything
    if (int e = flat_align_check(who, (uintptr_t)p | (uintptr_t)g | moments, chunks, shadow_bf16)) return e;
    AdamArgs a;
    a.k = {(float)beta1, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps};
    a.wd = weight_decay, a.grad_scale = grad_scale, a.bc1 = (float)bc1, a.inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(nchunks), dim3(256), 0, (hipStream_t)stream, p, g, m, v, (const FlatChunk*)chunks, lr_dev, lr_mult, scalars,
                           a, (__bf16*)shadow_bf16);
    };
    switch (flags) {
        case 0: go(adam_flat_kernel<false, false>); break;
        case ADAM_COUPLED: go(adam_flat_kernel<true, false>); break;
        case ADAM_FRESH: go(adam_flat_kernel<false, true>); break;
        default: go(adam_flat_kernel<true, true>); break;
    }
    CSWIN_LAUNCH_CHECK();
    return CSWIN_OK;
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

int cswin_rate_finalize(const float* partial, const int* first_chunk, int ntensors, float grad_scale, float max_norm,
                        const int* group_first, const int* group_tensors, const int* group_of, int ngroups, int statistic,
                        float default_mult, float* tensor_sumsq, float* scalars, float* group_stat, float* lr_mult, void* stream) {
    CSWIN_REQUIRE(partial && first_chunk && tensor_sumsq && scalars && ntensors > 0, CSWIN_ERR_SHAPE, "rate_finalize: bad arguments");
    CSWIN_REQUIRE(group_first && group_tensors && group_of && group_stat && lr_mult && ngroups > 0, CSWIN_ERR_SHAPE,
                  "rate_finalize: the group table, group_stat and lr_mult are required and ngroups must be positive (%d)", ngroups);
    CSWIN_REQUIRE(statistic == 0 || statistic == 1, CSWIN_ERR_SHAPE, "rate_finalize: statistic %d (0: gradient norm, 1: gradient norm / parameter norm)", statistic);
    const RateGroups gr = {group_first, group_tensors, group_of, ngroups, statistic, default_mult};
    hipLaunchKernelGGL(rate_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partial, first_chunk, ntensors, grad_scale, max_norm, gr,
                       tensor_sumsq, scalars, group_stat, lr_mult);
    CSWIN_LAUNCH_CHECK();
    return CSWIN_OK;
}

int cswin_adamw_flat(float* p, const float* g, float* m, float* v, const void* chunks, int nchunks, const float* lr_dev,
                     const float* lr_mult, const float* scalars, double beta1, double beta2, double eps, float weight_decay,
                     float grad_scale, double bc1, double bc2, void* shadow_bf16, void* stream) {
    return adam_launch("adamw_flat", p, g, m, v, chunks, nchunks, lr_dev, lr_mult, scalars, beta1, beta2, eps, weight_decay, grad_scale, bc1, bc2, 0,
                       shadow_bf16, stream);
}

int cswin_adam_flat(float* p, const float* g, float* m, float* v, const void* chunks, int nchunks, const float* lr_dev,
                    const float* lr_mult, const float* scalars, double beta1, double beta2, double eps, float weight_decay,
                    float grad_scale, double bc1, double bc2, int flags, void* shadow_bf16, void* stream) {
    return adam_launch("adam_flat", p, g, m, v, chunks, nchunks, lr_dev, lr_mult, scalars, beta1, beta2, eps, weight_decay, grad_scale, bc1, bc2, flags,
                       shadow_bf16, stream);
}

}  // extern "C"
