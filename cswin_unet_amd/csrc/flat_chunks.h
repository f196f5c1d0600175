// What the kernels over the flat optimiser buffers share (adamw.hip, tpgm.hip; sgd.hip takes the argument check): the chunk record,
// the walk over a chunk and every sum's fixed order.  The table is STATIC, built and uploaded once by optim.chunk_table: one
// 256-thread workgroup per record.  Chunks never cross a tensor and never cover the pad words between the 8-float slots, so a NaN
// in a pad word reaches nothing; slots are 8-float aligned and 16384 is a multiple of 4, so every chunk starts 16-B aligned.
//
// There is no float atomic anywhere: every sum has a fixed order (a thread's trips, its four lanes as (a0 + a1) + (a2 + a3), its
// tail element, the xor butterfly of a wave, the four waves as (w0 + w1) + (w2 + w3), chunks in chunk order, tensors in tensor
// order), so two runs on the same input give the same bits.  tests/test_adamw_host.sumsq_depth transcribes this file.
#pragma once
#include "common.h"

struct FlatChunk { long long off; int n; int tensor; };      // element offset into the flat buffers, n <= 16384, tensor index
static_assert(sizeof(FlatChunk) == 16, "the chunk record is 16 bytes");

// sum over the 256 threads of a workgroup, the same value in every thread: 6 butterfly levels inside a wave, then two levels
// over the four waves.  red: 4 floats of LDS per reduced value.
__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// The chunk walk: body4(i) for every f32x4 i of an n-element chunk that this thread owns.  Returns the index of the thread's tail
// element; the chunk has one for it (at most three in all) when that index is < n.
template <class Body4>
__device__ __forceinline__ int chunk_walk(int n, Body4 body4) {
    const int n4 = n >> 2;
    for (int i = threadIdx.x; i < n4; i += 256) body4(i);
    return n4 * 4 + threadIdx.x;
}

// partial[blockIdx.x] = two sums over the chunk (the second only when `second`).  terms4(i, a0, a1) adds the terms of f32x4 i lane
// by lane, terms1(it, s0, s1) those of the tail element.
template <class Terms4, class Terms1>
__device__ __forceinline__ void chunk_sums(int n, bool second, float* __restrict__ partial, Terms4 terms4, Terms1 terms1) {
    __shared__ float red[8];
    f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0;
    const int it = chunk_walk(n, [&](int i) { terms4(i, a0, a1); });
    float s0 = (a0[0] + a0[1]) + (a0[2] + a0[3]), s1 = (a1[0] + a1[1]) + (a1[2] + a1[3]);
    if (it < n) terms1(it, s0, s1);
    s0 = block_sum(s0, red);
    if (second) s1 = block_sum(s1, red + 4);
    if (threadIdx.x == 0) {
        partial[2 * (long)blockIdx.x] = s0;
        if (second) partial[2 * (long)blockIdx.x + 1] = s1;
    }
}

// The finalize kernels are one workgroup; thread k owns tensors k, k + 256, ...  First step: tensor t's chunk partials added in
// chunk order (the second column only when `second`).
__device__ __forceinline__ void tensor_sums(const float* __restrict__ partial, const int* __restrict__ first_chunk, int t, bool second, float& s0, float& s1) {
    s0 = s1 = 0.f;
    const int c1 = first_chunk[t + 1];
    for (int c = first_chunk[t]; c < c1; ++c) {
        s0 += partial[2 * (long)c];
        if (second) s1 += partial[2 * (long)c + 1];
    }
}

// Second step, called by every thread once per trip: thread 0 folds the values of items base .. base + 255 (tensors, or groups) into
// its acc in item order, fold(acc, value)
template <class Fold>
__device__ __forceinline__ void item_order_fold(float& acc, float mine, int base, int nitems, Fold fold) {
    __shared__ float slot[256];
    slot[threadIdx.x] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int cnt = nitems - base < 256 ? nitems - base : 256;
        for (int k = 0; k < cnt; ++k) fold(acc, slot[k]);
    }
    __syncthreads();
}

// total (thread 0's) += the values of tensors base .. base + 255 in tensor order
__device__ __forceinline__ void tensor_order_add(float& total, float mine, int base, int ntensors) {
    item_order_fold(total, mine, base, ntensors, [](float& acc, float x) { acc += x; });
}

// The maximum as the rates want it: a NaN value makes acc NaN and it stays one (reported, not repaired)
__device__ __forceinline__ void nan_keeping_max(float& acc, float x) {
    if (acc == acc && !(x <= acc)) acc = x;
}

// min(1, max_norm / (norm + 1e-6)), torch.nn.utils.clip_grad_norm_'s rule; a NaN norm stays a NaN coefficient (torch.clamp keeps it too)
__device__ __forceinline__ float clip_coef(float max_norm, float norm) {
    const float c = max_norm / (norm + 1e-6f);
    return c > 1.f ? 1.f : c;
}

// torch.optim.Adam's moments of the gradient g; returns m / (sqrt(v) / sqrt(bc2) + eps), the step before its rate
struct AdamBetas { float b1, omb1, b2, omb2, eps; };         // omb = (float)(1.0 - beta), formed in double
__device__ __forceinline__ float adam_quotient(float& m, float& v, float g, const AdamBetas& k, float inv_sqrt_bc2) {
    m = fmaf(k.b1, m, k.omb1 * g);
    v = fmaf(k.b2, v, k.omb2 * (g * g));
    return m / fmaf(sqrtf(v), inv_sqrt_bc2, k.eps);
}

// The alignment every entry point over the flat buffers asks for: `buffers` is the OR of the fp32 buffers' addresses (a null optional
// one adds nothing), the chunk table and the bf16 shadow may be null.
static inline int flat_align_check(const char* who, uintptr_t buffers, const void* chunks, const void* shadow) {
    CSWIN_REQUIRE((buffers & 15) == 0, CSWIN_ERR_ALIGN, "%s: buffers must be 16-B aligned", who);
    CSWIN_REQUIRE(((uintptr_t)chunks & 7) == 0, CSWIN_ERR_ALIGN, "%s: the chunk table must be 8-B aligned", who);
    CSWIN_REQUIRE(((uintptr_t)shadow & 7) == 0, CSWIN_ERR_ALIGN, "%s: the bf16 shadow must be 8-B aligned", who);
    return CSWIN_OK;
}
