// What the two segmentation objectives share on the device (loss.hip: CE + Dice; cl_loss.hip: focal + Dice + distillation): a
// pixel's class, its row of logits, its softmax and -log p[label], the three Dice sums per class, their finalize step and their
// gradient, and the launch rules.  Both make one pass over the (B, NC, HW) logits each way, one pixel per thread and trip: no
// one-hot tensor, no softmax tensor.
//
// Common part of the sums layout: [0] = sum over pixels of -log p[label];  [1 + c] = intersect_c;  [1 + NC + c] = y_sum_c;
// [1 + 2 NC + c] = z_sum_c.
//
// The per-class helpers take scalars and are called from the kernels' own unrolled loops: inlined, they leave every kernel's
// floating-point instructions, registers and occupancy as they were (profiles/loss_body_notes.md; tests/test_gpu_loss_parent.py
// holds the bits).  Two steps are NOT here although both files have them, because hipcc compiled the sums kernels' arithmetic
// differently once they sat behind a helper (the notes name the kernels and the instructions): the grid-stride pixel loop and the
// wave_sum -> red[4][NV] -> partial[] block store.  They stay written out, textually equal, in the kernels; so does the loop
// around softmax_term, for the same reason.
#pragma once
#include "common.h"

// class of a pixel, or -1 for a label outside [0, NC): the 64-bit value is compared, so 2^32 + 1 is no class 1
template <int NC>
__device__ __forceinline__ int label_class(long long label) {
    return (unsigned long long)label < (unsigned long long)NC ? (int)label : -1;
}

// v = the pixel's NC inputs (lp: its first, the channels HW apart); returns their maximum
template <int NC>
__device__ __forceinline__ float load_row(const float* __restrict__ lp, long HW, float (&v)[NC]) {
    float mx = -INFINITY;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        v[c] = lp[c * HW];
        mx = fmaxf(mx, v[c]);
    }
    return mx;
}

// one class of the softmax step: v <- exp(v - mx), mx the row maximum; returns it for the row sum.  PROBS: v is a probability
// already (DiceLoss(..., softmax=False), utils.py:32-34) and stays
template <bool PROBS>
__device__ __forceinline__ float softmax_term(float& v, float mx) {
    if (!PROBS) v = __expf(v - mx);
    return v;
}

// -log softmax(v)[label] = (mx - v[label]) + log sum_j exp(v_j - mx), as log_softmax forms it: exact however far the label's logit
// lies below the row maximum (-log of the normalised probability sticks once __expf underflows)
__device__ __forceinline__ float row_nll(float mx, float vl, float sum) { return (mx - vl) + __logf(sum); }

// one class's terms of intersect (I), y_sum (Y) and z_sum (Z) for a pixel of probability pc; hit: the class is the pixel's label
__device__ __forceinline__ void dice_terms(float pc, bool hit, float& I, float& Y, float& Z) {
    const float oh = hit ? 1.f : 0.f;
    I += pc * oh;
    Y += oh;
    Z += pc * pc;
}

// The Dice part of a finalize kernel (one thread): returns mean_c w_c (1 - (2 I_c + s) / (Z_c + Y_c + s)) and leaves
// coef[c] = a_c, coef[ncls + c] = b_c with d dice_c / d p_c(pixel) = a_c * onehot + b_c * p.  class_weight may be null: all 1,
// and the products by a constant 1 fold away.
__device__ __forceinline__ float dice_finalize(const float* __restrict__ sums, float* __restrict__ coef, int ncls,
                                               const float* __restrict__ class_weight) {
    const float smooth = 1e-5f;
    float dice = 0.f;
    for (int c = 0; c < ncls; ++c) {
        const float I = sums[1 + c], Y = sums[1 + ncls + c], Z = sums[1 + 2 * ncls + c];
        const float D = Z + Y + smooth;
        const float wc = class_weight ? class_weight[c] : 1.f;          // utils.py:44: loss += dice * weight[i]
        dice += wc * (1.f - (2.f * I + smooth) / D);
        coef[c] = wc * -2.f / D;
        coef[ncls + c] = wc * 2.f * (2.f * I + smooth) / (D * D);
    }
    return dice / ncls;
}

// the backward's copy of coef, read once per thread
template <int NC>
__device__ __forceinline__ void load_coef(const float* __restrict__ coef, float (&a)[NC], float (&bb)[NC]) {
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        a[c] = coef[c];
        bb[c] = coef[NC + c];
    }
}

// one class of the Dice gradient: v <- the probability v * inv,  G = a onehot + b p;  returns p G, the class's share of
// dot = sum_j p_j G_j.  d loss / d logit_c gets dice_scale * p_c * (G_c - dot), d loss / d p_c dice_scale * G_c
__device__ __forceinline__ float dice_grad_term(float& v, float inv, bool hit, float a, float b, float& G) {
    v *= inv;
    G = (hit ? a : 0.f) + b * v;
    return v * G;
}

// workgroups of the sums kernels (256 threads, one pixel per thread and trip); the backward kernels take four times as many
static inline int loss_blocks(long total) {
    long b = (total + 255) / 256;
    return (int)(b < 1 ? 1 : (b > 512 ? 512 : b));
}

// one class count of a dispatch switch: the call sees NC as a constant (variadic: an expanded launch macro has top-level commas)
#define LOSS_NC_CASE(n, ...) case n: { constexpr int NC = n; __VA_ARGS__; } break;
