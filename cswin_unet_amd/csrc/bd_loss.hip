// Boundary objective (Kervadec et al., MIDL 2019) on top of loss.hip's: w_ce * CE + w_dice * Dice + alpha * boundary, with
//   boundary = 1 / (B HW) * sum over pixels and classes of wb_c * softmax(logits)_c * phi_c,
// phi the signed distance maps of the labels (sdm.hip) and wb the per-class weights of the term (default: 0 for class 0, 1 for
// the rest).  Fused like loss.hip: one pass over the logits and over phi each way, no one-hot tensor, no softmax tensor.
// `cswin_bd_loss_sums` leaves 2 + 3*ncls plain sums over this rank's pixels in device memory; they add across data-parallel
// ranks.  alpha is scheduled during training and the step is a captured graph, so the finalize and gradient kernels read it
// from device memory.  The per-pixel steps are loss_pixel.h's; this file owns the boundary term and its derivative.
#include "loss_pixel.h"

namespace {

// the boundary term's class weights, read once per thread; null: Kervadec's idc, every class but the background
template <int NC>
__device__ __forceinline__ void load_boundary_weights(const float* __restrict__ wb, float (&w)[NC]) {
#pragma unroll
    for (int c = 0; c < NC; ++c) w[c] = wb ? wb[c] : (c ? 1.f : 0.f);
}

// sums layout: loss_pixel.h's 1 + 3 NC, then [1 + 3 NC] = sum over pixels and classes of (wb_c * p_c) * phi_c
template <int NC>
__global__ __launch_bounds__(256) void bd_loss_sums_kernel(const float* __restrict__ logits, const long long* __restrict__ labels,
                                                            const float* __restrict__ phi, const float* __restrict__ wb,
                                                            float* __restrict__ partial, int B, long HW) {
    constexpr int NV = 2 + 3 * NC;
    __shared__ float red[4][NV];
    float acc[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) acc[i] = 0.f;
    float w[NC];
    load_boundary_weights<NC>(wb, w);
    const long total = (long)B * HW;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long b = i / HW, p = i - b * HW;
        float v[NC];
        const float mx = load_row<NC>(logits + b * NC * HW + p, HW, v);
        const float* __restrict__ dp = phi + b * NC * HW + p;
        const int lab = label_class<NC>(labels[i]);
        float vl = 0.f;                                                 // the label's input, before it becomes exp(v - mx)
        float sum = 0.f;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            if (c == lab) vl = v[c];
            sum += softmax_term<false>(v[c], mx);
        }
        const float inv = 1.0f / sum;
        // an out-of-range label poisons the CE sum (loss.hip's convention); it is outside every class's mask, so phi is the plain
        // distance there and the boundary sum stays finite
        if (lab < 0) acc[0] = __builtin_nanf("");
        else acc[0] += row_nll(mx, vl, sum);
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const float pc = v[c] * inv;
            dice_terms(pc, c == lab, acc[1 + c], acc[1 + NC + c], acc[1 + 2 * NC + c]);
            acc[1 + 3 * NC] += (w[c] * pc) * dp[c * HW];
        }
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

// out[0..3] = loss, ce, dice, boundary;  coef: dice_finalize's, with the Dice class weights
__global__ void bd_loss_finalize_kernel(const float* __restrict__ sums, float* __restrict__ out, float* __restrict__ coef,
                                        float n_pixels, int ncls, float w_ce, float w_dice, const float* __restrict__ alpha_dev,
                                        const float* __restrict__ class_weight) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const float ce = sums[0] / n_pixels;
    const float boundary = sums[1 + 3 * ncls] / n_pixels;
    const float dice = dice_finalize(sums, coef, ncls, class_weight);
    const float alpha = alpha_dev[0];
    // a term whose weight is 0 must not carry its NaN into the loss (loss_finalize_kernel's w_ce != 0 rule)
    out[0] = (w_ce != 0.f ? w_ce * ce : 0.f) + w_dice * dice + (alpha != 0.f ? alpha * boundary : 0.f);
    out[1] = ce;
    out[2] = dice;
    out[3] = boundary;
}

// dlogits_c = gout * [ ce_scale * (p_c - onehot_c) + dice_scale * p_c * (G_c - sum_j p_j G_j)
//                      + alpha * bd_scale * p_c * (T_c - sum_j p_j T_j) ],  G_c = a_c onehot_c + b_c p_c,  T_c = wb_c phi_c
template <int NC>
__global__ __launch_bounds__(256) void bd_loss_bwd_kernel(const float* __restrict__ logits, const long long* __restrict__ labels,
                                                           const float* __restrict__ phi, const float* __restrict__ wb,
                                                           const float* __restrict__ coef, const float* __restrict__ alpha_dev,
                                                           const float* __restrict__ gout, float* __restrict__ dlogits,
                                                           float ce_scale, float dice_scale, float bd_scale, int B, long HW) {
    float a[NC], bb[NC], w[NC];
    load_coef<NC>(coef, a, bb);
    load_boundary_weights<NC>(wb, w);
    const float g = gout ? gout[0] : 1.f;
    const float ab = alpha_dev[0] * bd_scale;
    const long total = (long)B * HW;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long b = i / HW, p = i - b * HW;
        float v[NC];
        const float mx = load_row<NC>(logits + b * NC * HW + p, HW, v);
        const float* __restrict__ tp = phi + b * NC * HW + p;
        float sum = 0.f;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            sum += softmax_term<false>(v[c], mx);
        }
        const float inv = 1.0f / sum;
        const int lab = label_class<NC>(labels[i]);
        float G[NC], T[NC], dot = 0.f, dotb = 0.f;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            dot += dice_grad_term(v[c], inv, c == lab, a[c], bb[c], G[c]);
            T[c] = w[c] * tp[c * HW];
            dotb += v[c] * T[c];
        }
        float* dp = dlogits + b * NC * HW + p;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const float oh = (c == lab) ? 1.f : 0.f;
            dp[c * HW] = g * (ce_scale * (v[c] - oh) + dice_scale * v[c] * (G[c] - dot) + ab * v[c] * (T[c] - dotb));
        }
    }
}

// the class counts of loss.hip's switch
#define BD_NC_SWITCH(NCV, CALL)                                                                                          \
    switch (NCV) {                                                                                                       \
        LOSS_NC_CASE(2, CALL) LOSS_NC_CASE(3, CALL) LOSS_NC_CASE(4, CALL) LOSS_NC_CASE(5, CALL) LOSS_NC_CASE(6, CALL)    \
        LOSS_NC_CASE(7, CALL) LOSS_NC_CASE(8, CALL) LOSS_NC_CASE(9, CALL) LOSS_NC_CASE(14, CALL) LOSS_NC_CASE(16, CALL)  \
        default: cswin_set_error("bd_loss: num_classes=%d unsupported", NCV); return CSWIN_ERR_UNSUPPORTED;              \
    }

}  // namespace

extern "C" {

size_t cswin_bd_loss_workspace(int B, int ncls, long HW) { return (size_t)loss_blocks((long)B * HW) * (2 + 3 * ncls) * sizeof(float); }

// logits, phi (B, ncls, HW) fp32, labels (B, HW) int64, wb ncls floats or null -> sums[2 + 3*ncls] (local batch)
int cswin_bd_loss_sums(const float* logits, const long long* labels, const float* phi, const float* wb, float* sums, void* workspace,
                       size_t ws_bytes, int B, int ncls, long HW, void* stream) {
    CSWIN_REQUIRE(logits && labels && phi && sums && B > 0 && HW > 0, CSWIN_ERR_SHAPE, "bd_loss_sums: bad arguments");
    CSWIN_REQUIRE(workspace && ws_bytes >= cswin_bd_loss_workspace(B, ncls, HW), CSWIN_ERR_WORKSPACE, "bd_loss_sums: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const int nblk = loss_blocks((long)B * HW);
    BD_NC_SWITCH(ncls, hipLaunchKernelGGL((bd_loss_sums_kernel<NC>), dim3(nblk), dim3(256), 0, st, logits, labels, phi, wb, (float*)workspace, B, HW));
    CSWIN_LAUNCH_CHECK();
    launch_reduce_job(cswin_reduce_job{(const float*)workspace, sums, nullptr, 0, 2 + 3 * ncls, 2 + 3 * ncls, nblk, 0, 0, 0}, st);
    CSWIN_LAUNCH_CHECK();
    return CSWIN_OK;
}

// sums (possibly all-reduced) -> out4 = {loss, ce, dice, boundary}, coef[2*ncls]; n_pixels = pixel count the sums cover
int cswin_bd_loss_finalize(const float* sums, float* out4, float* coef, double n_pixels, int ncls, float w_ce, float w_dice,
                           const float* alpha_dev, const float* class_weight, void* stream) {
    CSWIN_REQUIRE(sums && out4 && coef && alpha_dev && n_pixels > 0 && ncls > 0, CSWIN_ERR_SHAPE, "bd_loss_finalize: bad arguments");
    hipLaunchKernelGGL(bd_loss_finalize_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, sums, out4, coef, (float)n_pixels, ncls, w_ce, w_dice,
                       alpha_dev, class_weight);
    CSWIN_LAUNCH_CHECK();
    return CSWIN_OK;
}

// ce_scale = w_ce / n_pixels, dice_scale = w_dice / ncls (times world size under gradient averaging), bd_scale = 1 / n_pixels,
// n_pixels the LOCAL count; alpha comes from alpha_dev
int cswin_bd_loss_bwd(const float* logits, const long long* labels, const float* phi, const float* wb, const float* coef,
                      const float* alpha_dev, const float* grad_out, float* dlogits, float ce_scale, float dice_scale, float bd_scale,
                      int B, int ncls, long HW, void* stream) {
    CSWIN_REQUIRE(logits && labels && phi && coef && alpha_dev && dlogits && B > 0 && HW > 0, CSWIN_ERR_SHAPE, "bd_loss_bwd: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    const int nblk = loss_blocks((long)B * HW) * 4;
    BD_NC_SWITCH(ncls, hipLaunchKernelGGL((bd_loss_bwd_kernel<NC>), dim3(nblk), dim3(256), 0, st, logits, labels, phi, wb, coef, alpha_dev, grad_out,
                                          dlogits, ce_scale, dice_scale, bd_scale, B, HW));
    CSWIN_LAUNCH_CHECK();
    return CSWIN_OK;
}

}  // extern "C"
