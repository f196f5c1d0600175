// Objective of the continual-learning workflow (universal_train.py:904-932): focal cross entropy (:141-174) + soft Dice on the
// widened (B, ncls, H, W) logits, plus temperature-T distillation (:618-623) of the first `nold` channels towards a frozen
// teacher's (B, nold, H, W) logits -- fused like loss.hip: one pass over the logits each way, no one-hot tensor, no softmax
// tensor, the new-dataset label map (:243-258) applied as a table lookup while the label is read.  `cswin_cl_loss_sums` leaves
// 3 + 3*ncls plain sums over this rank's pixels in device memory; they add across data-parallel ranks.
// The per-pixel steps are loss_pixel.h's; this file owns the label map, the distillation block, the focal term and its derivative.
#include "loss_pixel.h"

namespace {

// the label after the optional map (int32 table of n_map entries); an index outside the table is no class
template <int NC>
__device__ __forceinline__ int mapped_class(const long long* __restrict__ labels, const int* __restrict__ label_map, int n_map, long i) {
    long long l = labels[i];
    if (label_map) l = (unsigned long long)l < (unsigned long long)n_map ? (long long)label_map[l] : -1;
    return label_class<NC>(l);
}

// x^gamma for x >= 0.  gi = gamma when it is a small integer: repeated products, each correctly rounded (the tests' bound counts
// them); gi < 0: powf.  The kernel is bound by its input streams either way: powf measured no slower
// (profiles/continual_loss_timing.txt).  x^0 = 1, also at x = 0.
__device__ __forceinline__ float pow_gamma(float x, float gamma, int gi) {
    if (gi < 0) return powf(x, gamma);
    float r = 1.f;
    for (int k = 0; k < gi; ++k) r *= x;
    return r;
}

__host__ __device__ inline int gamma_int(float gamma) {
    if (!(gamma >= 0.f && gamma <= 8.f)) return -1;                     // range first: the cast of a large float is undefined
    const int gi = (int)gamma;
    return (float)gi == gamma ? gi : -1;
}

// sums layout: loss_pixel.h's 1 + 3 NC, then
// [1 + 3 NC] = sum of focal terms;  [2 + 3 NC] = sum over pixels of KL(teacher_T || student_T) over the first nold channels
template <int NC>
__global__ __launch_bounds__(256) void cl_loss_sums_kernel(const float* __restrict__ logits, const long long* __restrict__ labels,
                                                            const int* __restrict__ label_map, int n_map,
                                                            const float* __restrict__ teacher, const float* __restrict__ class_weight,
                                                            float* __restrict__ partial, int B, int nold, long HW, float inv_t,
                                                            float alpha, float gamma) {
    constexpr int NV = 3 + 3 * NC;
    __shared__ float red[4][NV];
    float acc[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) acc[i] = 0.f;
    const int gi = gamma_int(gamma);
    const long total = (long)B * HW;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long b = i / HW, p = i - b * HW;
        float v[NC];
        const float mx = load_row<NC>(logits + b * NC * HW + p, HW, v);
        if (nold > 0) {
            // distillation: both rows are shifted by their own maximum BEFORE the division by T (an offset of 1e4 must cancel
            // exactly), and log q is formed from the shifted logits, never as log(q_c): where exp underflows, q_c is an exact
            // 0 times a finite number
            const float* tp = teacher + b * nold * HW + p;
            float t[NC];
            float mt = -INFINITY, mz = -INFINITY;
#pragma unroll
            for (int c = 0; c < NC; ++c)
                if (c < nold) {
                    t[c] = tp[c * HW];
                    mt = fmaxf(mt, t[c]);
                    mz = fmaxf(mz, v[c]);
                }
            float st = 0.f, sz = 0.f;
#pragma unroll
            for (int c = 0; c < NC; ++c)
                if (c < nold) {
                    t[c] = (t[c] - mt) * inv_t;
                    st += __expf(t[c]);
                    sz += __expf((v[c] - mz) * inv_t);
                }
            const float lst = __logf(st), lsz = __logf(sz), ist = 1.0f / st;
            float kd = 0.f;
#pragma unroll
            for (int c = 0; c < NC; ++c)
                if (c < nold) kd += (__expf(t[c]) * ist) * ((t[c] - lst) - ((v[c] - mz) * inv_t - lsz));
            acc[2 + 3 * NC] += kd;
        }
        const int lab = mapped_class<NC>(labels, label_map, n_map, i);
        float vl = 0.f;
        float sum = 0.f;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            if (c == lab) vl = v[c];
            sum += softmax_term<false>(v[c], mx);
        }
        const float inv = 1.0f / sum;
        // an out-of-range label poisons the plain and the focal sum (as loss.hip's CE sum; the reference's focal loss clamps)
        if (lab < 0) {
            acc[0] = __builtin_nanf("");
            acc[1 + 3 * NC] = __builtin_nanf("");
        } else {
            const float nll = row_nll(mx, vl, sum);
            acc[0] += nll;
            // F.cross_entropy(weight=, reduction='none') = w[label] * nll;  pt = exp(-ce);  1 - pt = -expm1(-ce): for a confident
            // pixel ce ~ 1e-6 and 1 - exp(-ce) has no correct digit in fp32
            const float ce = (class_weight ? class_weight[lab] : 1.f) * nll;
            acc[1 + 3 * NC] += alpha * pow_gamma(-expm1f(-ce), gamma, gi) * ce;
        }
#pragma unroll
        for (int c = 0; c < NC; ++c) dice_terms(v[c] * inv, c == lab, acc[1 + c], acc[1 + NC + c], acc[1 + 2 * NC + c]);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const float s = wave_sum(acc[i]);
        if (lane == 0) red[wave][i] = s;
    }
    __syncthreads();
    if (threadIdx.x < NV)
        partial[(long)blockIdx.x * NV + threadIdx.x] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

// out[0..4] = loss, focal, dice, kd, ce;  coef: dice_finalize's (unweighted Dice)
__global__ void cl_loss_finalize_kernel(const float* __restrict__ sums, float* __restrict__ out, float* __restrict__ coef,
                                        float n_pixels, float batch, int ncls, float w_focal, float w_dice, float kd_weight,
                                        float temperature) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const float ce = sums[0] / n_pixels;
    const float focal = sums[1 + 3 * ncls] / n_pixels;
    // F.kl_div(..., 'batchmean') divides by the first dimension only: per image, not per pixel (universal_train.py:622)
    const float kd = sums[2 + 3 * ncls] * (temperature * temperature) / batch;
    const float dice = dice_finalize(sums, coef, ncls, nullptr);
    // a term whose weight is 0 must not carry its NaN into the loss (loss_finalize_kernel's w_ce != 0 rule)
    const float seg = (w_focal != 0.f ? w_focal * focal : 0.f) + w_dice * dice;
    const float keep = 1.f - kd_weight;
    out[0] = (keep != 0.f ? keep * seg : 0.f) + (kd_weight != 0.f ? kd_weight * kd : 0.f);
    out[1] = focal;
    out[2] = dice;
    out[3] = kd;
    out[4] = ce;
}

// dlogits_c = g * [ focal_scale * f'(ce) * w_l * (p_c - onehot_c) + dice_scale * p_c * (G_c - sum_j p_j G_j)
//                   + (c < nold) * kd_scale * (pT_c - q_c) ],  f'(ce) = alpha * ((1-pt)^gamma + gamma (1-pt)^(gamma-1) pt ce)
template <int NC>
__global__ __launch_bounds__(256) void cl_loss_bwd_kernel(const float* __restrict__ logits, const long long* __restrict__ labels,
                                                           const int* __restrict__ label_map, int n_map,
                                                           const float* __restrict__ teacher, const float* __restrict__ class_weight,
                                                           const float* __restrict__ coef, const float* __restrict__ gout,
                                                           float* __restrict__ dlogits, float focal_scale, float dice_scale,
                                                           float kd_scale, int B, int nold, long HW, float inv_t, float alpha,
                                                           float gamma) {
    float a[NC], bb[NC];
    load_coef<NC>(coef, a, bb);
    const float g = gout ? gout[0] : 1.f;
    const int gi = gamma_int(gamma);
    const long total = (long)B * HW;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long b = i / HW, p = i - b * HW;
        float v[NC];
        const float mx = load_row<NC>(logits + b * NC * HW + p, HW, v);
        float kdg[NC];                                                  // kd_scale * (pT_c - q_c), 0 past nold
#pragma unroll
        for (int c = 0; c < NC; ++c) kdg[c] = 0.f;
        if (nold > 0) {
            const float* tp = teacher + b * nold * HW + p;
            float t[NC];
            float mt = -INFINITY, mz = -INFINITY;
#pragma unroll
            for (int c = 0; c < NC; ++c)
                if (c < nold) {
                    t[c] = tp[c * HW];
                    mt = fmaxf(mt, t[c]);
                    mz = fmaxf(mz, v[c]);
                }
            float st = 0.f, sz = 0.f;
#pragma unroll
            for (int c = 0; c < NC; ++c)
                if (c < nold) {
                    t[c] = __expf((t[c] - mt) * inv_t);
                    kdg[c] = __expf((v[c] - mz) * inv_t);
                    st += t[c];
                    sz += kdg[c];
                }
            const float ist = 1.0f / st, isz = 1.0f / sz;
#pragma unroll
            for (int c = 0; c < NC; ++c)
                if (c < nold) kdg[c] = kd_scale * (kdg[c] * isz - t[c] * ist);
        }
        const int lab = mapped_class<NC>(labels, label_map, n_map, i);
        float vl = 0.f;
        float sum = 0.f;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            if (c == lab) vl = v[c];
            sum += softmax_term<false>(v[c], mx);
        }
        const float inv = 1.0f / sum;
        // an out-of-range label has no focal gradient (and makes no NaN): what test_out_of_range_labels pins for the base loss
        float cf = 0.f;
        if (lab >= 0) {
            const float w = class_weight ? class_weight[lab] : 1.f;
            const float ce = w * row_nll(mx, vl, sum);
            const float omp = -expm1f(-ce);
            float fp = pow_gamma(omp, gamma, gi);
            // gamma == 0: the second term is 0 * (1-pt)^(-1), NaN at pt == 1; it is left out
            if (gamma != 0.f) fp += gamma * (gi > 0 ? pow_gamma(omp, gamma, gi - 1) : powf(omp, gamma - 1.f)) * __expf(-ce) * ce;
            cf = focal_scale * alpha * fp * w;
        }
        float G[NC], dot = 0.f;
#pragma unroll
        for (int c = 0; c < NC; ++c) dot += dice_grad_term(v[c], inv, c == lab, a[c], bb[c], G[c]);
        float* dp = dlogits + b * NC * HW + p;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const float oh = (c == lab) ? 1.f : 0.f;
            dp[c * HW] = g * (cf * (v[c] - oh) + dice_scale * v[c] * (G[c] - dot) + kdg[c]);
        }
    }
}

#define CL_NC_SWITCH(NCV, CALL)                                                                                            \
    switch (NCV) {                                                                                                         \
        LOSS_NC_CASE(2, CALL) LOSS_NC_CASE(3, CALL) LOSS_NC_CASE(4, CALL) LOSS_NC_CASE(5, CALL) LOSS_NC_CASE(6, CALL)      \
        LOSS_NC_CASE(7, CALL) LOSS_NC_CASE(8, CALL) LOSS_NC_CASE(9, CALL) LOSS_NC_CASE(10, CALL) LOSS_NC_CASE(11, CALL)    \
        LOSS_NC_CASE(12, CALL) LOSS_NC_CASE(13, CALL) LOSS_NC_CASE(14, CALL) LOSS_NC_CASE(15, CALL) LOSS_NC_CASE(16, CALL) \
        default: cswin_set_error("cl_loss: num_classes=%d unsupported (2..16)", NCV); return CSWIN_ERR_UNSUPPORTED;        \
    }

// the checks both passes share, before any launch
int cl_loss_check(const char* who, const void* logits, const void* labels, const void* label_map, int n_map, const void* teacher,
                  int B, int ncls, int nold, long HW, float temperature, float focal_gamma) {
    CSWIN_REQUIRE(logits && labels && B > 0 && HW > 0, CSWIN_ERR_SHAPE, "%s: bad arguments", who);
    CSWIN_REQUIRE(ncls >= 2 && ncls <= 16, CSWIN_ERR_UNSUPPORTED, "%s: num_classes=%d unsupported (2..16)", who, ncls);
    CSWIN_REQUIRE(nold >= 0 && nold <= ncls, CSWIN_ERR_SHAPE, "%s: old_classes=%d outside [0, %d]", who, nold, ncls);
    CSWIN_REQUIRE(teacher || nold == 0, CSWIN_ERR_SHAPE, "%s: old_classes=%d needs teacher logits", who, nold);
    CSWIN_REQUIRE(!label_map || n_map > 0, CSWIN_ERR_SHAPE, "%s: label map of %d entries", who, n_map);
    CSWIN_REQUIRE(temperature > 0.f && temperature < INFINITY, CSWIN_ERR_UNSUPPORTED, "%s: temperature %g must be > 0", who, (double)temperature);
    CSWIN_REQUIRE(focal_gamma == 0.f || (focal_gamma >= 1.f && focal_gamma < INFINITY), CSWIN_ERR_UNSUPPORTED,
                  "%s: focal gamma %g must be 0 or >= 1", who, (double)focal_gamma);
    return CSWIN_OK;
}

}  // namespace

extern "C" {

size_t cswin_cl_loss_workspace(int B, int ncls, long HW) { return (size_t)loss_blocks((long)B * HW) * (3 + 3 * ncls) * sizeof(float); }

// logits (B, ncls, HW) fp32, labels (B, HW) int64, teacher (B, nold, HW) fp32 -> sums[3 + 3*ncls] (local batch)
int cswin_cl_loss_sums(const float* logits, const long long* labels, const int* label_map, int n_map, const float* teacher,
                       const float* class_weight, float* sums, void* workspace, size_t ws_bytes, int B, int ncls, int nold,
                       long HW, float temperature, float focal_alpha, float focal_gamma, void* stream) {
    const int rc = cl_loss_check("cl_loss_sums", logits, labels, label_map, n_map, teacher, B, ncls, nold, HW, temperature, focal_gamma);
    if (rc != CSWIN_OK) return rc;
    CSWIN_REQUIRE(sums, CSWIN_ERR_SHAPE, "cl_loss_sums: bad arguments");
    CSWIN_REQUIRE(workspace && ws_bytes >= cswin_cl_loss_workspace(B, ncls, HW), CSWIN_ERR_WORKSPACE, "cl_loss_sums: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const int nblk = loss_blocks((long)B * HW);
    CL_NC_SWITCH(ncls, hipLaunchKernelGGL((cl_loss_sums_kernel<NC>), dim3(nblk), dim3(256), 0, st, logits, labels, label_map, n_map, teacher,
                                          class_weight, (float*)workspace, B, nold, HW, 1.0f / temperature, focal_alpha, focal_gamma));
    CSWIN_LAUNCH_CHECK();
    launch_reduce_job(cswin_reduce_job{(const float*)workspace, sums, nullptr, 0, 3 + 3 * ncls, 3 + 3 * ncls, nblk, 0, 0, 0}, st);
    CSWIN_LAUNCH_CHECK();
    return CSWIN_OK;
}

// sums (possibly all-reduced) -> out5 = {loss, focal, dice, kd, ce}, coef[2*ncls]; n_pixels and batch = what the sums cover
int cswin_cl_loss_finalize(const float* sums, float* out5, float* coef, double n_pixels, double batch, int ncls, float w_focal,
                           float w_dice, float kd_weight, float temperature, void* stream) {
    CSWIN_REQUIRE(sums && out5 && coef && n_pixels > 0 && batch > 0 && ncls > 0, CSWIN_ERR_SHAPE, "cl_loss_finalize: bad arguments");
    CSWIN_REQUIRE(temperature > 0.f && temperature < INFINITY, CSWIN_ERR_UNSUPPORTED, "cl_loss_finalize: temperature %g must be > 0", (double)temperature);
    hipLaunchKernelGGL(cl_loss_finalize_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, sums, out5, coef, (float)n_pixels, (float)batch,
                       ncls, w_focal, w_dice, kd_weight, temperature);
    CSWIN_LAUNCH_CHECK();
    return CSWIN_OK;
}

int cswin_cl_loss_bwd(const float* logits, const long long* labels, const int* label_map, int n_map, const float* teacher,
                      const float* class_weight, const float* coef, const float* grad_out, float* dlogits, float focal_scale,
                      float dice_scale, float kd_scale, int B, int ncls, int nold, long HW, float temperature, float focal_alpha,
                      float focal_gamma, void* stream) {
    const int rc = cl_loss_check("cl_loss_bwd", logits, labels, label_map, n_map, teacher, B, ncls, nold, HW, temperature, focal_gamma);
    if (rc != CSWIN_OK) return rc;
    CSWIN_REQUIRE(coef && dlogits, CSWIN_ERR_SHAPE, "cl_loss_bwd: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    const int nblk = loss_blocks((long)B * HW) * 4;
    CL_NC_SWITCH(ncls, hipLaunchKernelGGL((cl_loss_bwd_kernel<NC>), dim3(nblk), dim3(256), 0, st, logits, labels, label_map, n_map, teacher,
                                          class_weight, coef, grad_out, dlogits, focal_scale, dice_scale, kd_scale, B, nold, HW,
                                          1.0f / temperature, focal_alpha, focal_gamma));
    CSWIN_LAUNCH_CHECK();
    return CSWIN_OK;
}

}  // extern "C"
