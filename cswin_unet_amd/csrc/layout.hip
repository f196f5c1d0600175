// Layout adapters at the two ends of the token pipeline and for nn.Conv2d-shaped parameters.
//   * image (B, C, H, W)  ->  NHWC tokens (B, H*W, Cpad) with zero padded channels (patch-embed input)
//   * tokens (B, H*W, Cpad) -> (B, C, H, W) taking the first C channels (segmentation logits)
//   * Conv2d weight [Cout][Cin][ks][ks] <-> implicit-GEMM images [Cout][ks*ks][Cpad] and [ks*ks][Cout][Cpad]
// All index-only (bit-exact).
#include "common.h"

namespace {

__global__ void nchw_to_tok_kernel(const float* __restrict__ x, float* __restrict__ y, int B, int C, long HW, int Cpad) {
    const long total = (long)B * HW * Cpad;
    for (long o = (long)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (long)gridDim.x * blockDim.x) {
        const int c = (int)(o % Cpad);
        const long bp = o / Cpad;
        const long p = bp % HW, b = bp / HW;
        y[o] = c < C ? x[(b * C + c) * HW + p] : 0.f;
    }
}

// y (B, C, HW) <- x (B, HW, Cpad)[..., :C]; tiled through LDS so both sides are coalesced
__global__ __launch_bounds__(256) void tok_to_nchw_kernel(const float* __restrict__ x, float* __restrict__ y, int B, int C,
                                                           long HW, int Cpad) {
    __shared__ float tile[64][17];
    const long ptiles = (HW + 63) / 64;
    for (long t = blockIdx.x; t < (long)B * ptiles; t += gridDim.x) {
        const long b = t / ptiles, p0 = (t % ptiles) * 64;
        for (int c0 = 0; c0 < C; c0 += 16) {
            for (int i = threadIdx.x; i < 64 * 16; i += 256) {
                const int pp = i / 16, cc = i % 16;
                tile[pp][cc] = (p0 + pp < HW && c0 + cc < Cpad) ? x[(b * HW + p0 + pp) * Cpad + c0 + cc] : 0.f;
            }
            __syncthreads();
            for (int i = threadIdx.x; i < 64 * 16; i += 256) {
                const int cc = i / 64, pp = i % 64;
                if (p0 + pp < HW && c0 + cc < C) y[(b * C + c0 + cc) * HW + p0 + pp] = tile[pp][cc];
            }
            __syncthreads();
        }
    }
}

__global__ void conv_w_permute_kernel(const float* __restrict__ w, float* __restrict__ wp, float* __restrict__ wpt,
                                      int Cout, int Cin, int kk, int Cpad) {
    const long total = (long)Cout * kk * Cpad;
    for (long o = (long)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (long)gridDim.x * blockDim.x) {
        const int ci = (int)(o % Cpad);
        const int tap = (int)((o / Cpad) % kk);
        const int co = (int)(o / ((long)Cpad * kk));
        const float v = ci < Cin ? w[((long)co * Cin + ci) * kk + tap] : 0.f;
        if (wp) wp[o] = v;
        if (wpt) wpt[((long)tap * Cout + co) * Cpad + ci] = v;
    }
}

__global__ void conv_w_unpermute_kernel(const float* __restrict__ dwp, float* __restrict__ dw, int Cout, int Cin, int kk,
                                        int Cpad) {
    const long total = (long)Cout * Cin * kk;
    for (long o = (long)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (long)gridDim.x * blockDim.x) {
        const int tap = (int)(o % kk);
        const int ci = (int)((o / kk) % Cin);
        const int co = (int)(o / ((long)kk * Cin));
        dw[o] = dwp[((long)co * kk + tap) * Cpad + ci];
    }
}

// wf[ci][tap'][co] = w[co][ci][kk - 1 - tap']: the weight image with which the DATA gradient of a stride-1 "same" convolution
// is itself a forward convolution of dy (Cout -> Cin channels, taps mirrored), i.e. runs on the forward implicit-GEMM kernel
__global__ void conv_w_flipT_kernel(const float* __restrict__ w, float* __restrict__ wf, int Cout, int Cin, int kk) {
    const long total = (long)Cin * kk * Cout;
    for (long o = (long)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (long)gridDim.x * blockDim.x) {
        const int co = (int)(o % Cout);
        const int tap = (int)((o / Cout) % kk);
        const int ci = (int)(o / ((long)Cout * kk));
        wf[o] = w[((long)co * Cin + ci) * kk + (kk - 1 - tap)];
    }
}

// ---- every convolution weight image of a step in ONE launch ---------------------------------------------------------------
// The images above are a few hundred KB each and the model has eight convolutions: as launches of their own they cost a step
// twelve launch latencies.  Here a table of jobs travels in the kernel arguments (as the slab reductions' does) and every
// workgroup finds its job by its index.  A job fills any of the three images of one weight; values are copied, never computed.
constexpr int CI_ELEMS = 1024;                 // image elements per workgroup
struct ConvImageJobs {
    cswin_conv_image_job j[CSWIN_MAX_CONV_IMAGE_JOBS];
    int first_block[CSWIN_MAX_CONV_IMAGE_JOBS + 1];
    int njobs;
};

__global__ __launch_bounds__(256) void conv_w_images_kernel(ConvImageJobs J) {
    int k = 0;
    while (k + 1 < J.njobs && (int)blockIdx.x >= J.first_block[k + 1]) ++k;
    const cswin_conv_image_job& j = J.j[k];
    const int kk = j.ks * j.ks, Cout = j.Cout, Cin = j.Cin, Cpad = j.Cpad;
    const long base = (long)((int)blockIdx.x - J.first_block[k]) * CI_ELEMS;
    if (j.w_perm || j.w_permT) {
        const long total = (long)Cout * kk * Cpad;
        for (long o = base + threadIdx.x; o < base + CI_ELEMS && o < total; o += 256) {
            const int ci = (int)(o % Cpad);
            const int tap = (int)((o / Cpad) % kk);
            const int co = (int)(o / ((long)Cpad * kk));
            const float v = ci < Cin ? j.w[((long)co * Cin + ci) * kk + tap] : 0.f;
            if (j.w_perm) j.w_perm[o] = v;
            if (j.w_permT) j.w_permT[((long)tap * Cout + co) * Cpad + ci] = v;
        }
    }
    if (j.w_flipT) {
        const long total = (long)Cin * kk * Cout;
        for (long o = base + threadIdx.x; o < base + CI_ELEMS && o < total; o += 256) {
            const int co = (int)(o % Cout);
            const int tap = (int)((o / Cout) % kk);
            const int ci = (int)(o / ((long)Cout * kk));
            j.w_flipT[o] = j.w[((long)co * Cin + ci) * kk + (kk - 1 - tap)];
        }
    }
}

// ---- the segmentation head's composed weight ------------------------------------------------------------------------------
// up_x4 applies `output` (1x1, no bias) after CARAFE4's `out` (1x1): Wf = W_head W_out (ncls x C), bf = W_head b_out, both
// padded with zero rows to the Cpad channels of the head's tokens.  The matrices are 9 x 64 and 64 x 64: every workgroup first
// copies the operands to LDS with all its loads in flight (a dot product that walks global memory pays one memory latency per
// term), then one thread per output element sums in plain C++.  This replaces four tiny GEMMs, two fills and two copies (and
// their mirror image backward).
constexpr int HEAD_LDS_FLOATS = 12 * 1024;     // operands beyond 48 KB are read in place

__device__ __forceinline__ const float* head_stage(const float* __restrict__ src, float* lds, int n, bool use_lds) {
    if (!use_lds || !src) return src;
    for (int i = threadIdx.x; i < n; i += 256) lds[i] = src[i];
    return lds;
}

__global__ __launch_bounds__(256) void head_compose_kernel(const float* __restrict__ w_head, const float* __restrict__ w_out,
                                                            const float* __restrict__ b_out, float* __restrict__ w_fused,
                                                            float* __restrict__ b_fused, int ncls, int E, int C, int Cpad) {
    __shared__ float lds[HEAD_LDS_FLOATS];
    const bool st = ncls * E + E * C + E <= HEAD_LDS_FLOATS;
    const float* wh = head_stage(w_head, lds, ncls * E, st);
    const float* wo = head_stage(w_out, lds + ncls * E, E * C, st);
    const float* bo = head_stage(b_out, lds + ncls * E + E * C, E, st);
    __syncthreads();
    const int total = Cpad * C + Cpad;
    for (int o = blockIdx.x * 256 + threadIdx.x; o < total; o += gridDim.x * 256) {
        float t = 0.f;
        if (o < Cpad * C) {
            const int n = o / C, c = o - n * C;
            if (n < ncls)
                for (int e = 0; e < E; ++e) t += wh[n * E + e] * wo[e * C + c];
            w_fused[o] = t;
        } else {
            const int n = o - Cpad * C;
            if (n < ncls && bo)
                for (int e = 0; e < E; ++e) t += wh[n * E + e] * bo[e];
            b_fused[n] = t;
        }
    }
}

// dW_head (ncls x E) = dWf[:ncls] W_out^T + dbf[:ncls] b_out^T;  dW_out (E x C) = W_head^T dWf[:ncls];  db_out (E) = W_head^T dbf[:ncls]
__global__ __launch_bounds__(256) void head_compose_bwd_kernel(const float* __restrict__ w_head, const float* __restrict__ w_out,
                                                                const float* __restrict__ b_out, const float* __restrict__ dw_fused,
                                                                const float* __restrict__ db_fused, float* __restrict__ dw_head,
                                                                float* __restrict__ dw_out, float* __restrict__ db_out, int ncls,
                                                                int E, int C) {
    __shared__ float lds[HEAD_LDS_FLOATS];
    const int n_head = ncls * E, n_out = E * C;
    const bool st = n_head + n_out + E + ncls * C + ncls <= HEAD_LDS_FLOATS;
    const float* wh = head_stage(w_head, lds, n_head, st);
    // W_out is read along its rows by the lanes of dW_head: one padding float per row keeps them on different banks
    const float* wo = w_out;
    const int wo_ld = st ? C + 1 : C;
    if (st) {
        float* d = lds + n_head;
        for (int i = threadIdx.x; i < n_out; i += 256) d[(i / C) * wo_ld + (i % C)] = w_out[i];
        wo = d;
    }
    float* rest = lds + n_head + E * (C + 1);
    const bool st2 = st && n_head + E * (C + 1) + E + ncls * C + ncls <= HEAD_LDS_FLOATS;
    const float* bo = head_stage(b_out, rest, E, st2);
    const float* dwf = head_stage(dw_fused, rest + E, ncls * C, st2);
    const float* dbf = head_stage(db_fused, rest + E + ncls * C, ncls, st2);
    __syncthreads();
    const int total = n_head + n_out + (db_out ? E : 0);
    for (int o = blockIdx.x * 256 + threadIdx.x; o < total; o += gridDim.x * 256) {
        float t = 0.f;
        if (o < n_head) {
            const int n = o / E, e = o - n * E;
            for (int c = 0; c < C; ++c) t += dwf[n * C + c] * wo[e * wo_ld + c];
            if (bo && dbf) t += dbf[n] * bo[e];
            dw_head[o] = t;
        } else if (o < n_head + n_out) {
            const int i = o - n_head, e = i / C, c = i - e * C;
            for (int n = 0; n < ncls; ++n) t += wh[n * E + e] * dwf[n * C + c];
            dw_out[i] = t;
        } else {
            const int e = o - n_head - n_out;
            if (dbf)
                for (int n = 0; n < ncls; ++n) t += wh[n * E + e] * dbf[n];
            db_out[e] = t;
        }
    }
}

int grid1d(long total) {
    long b = (total + 255) / 256;
    return (int)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}

// ---- dropout -------------------------------------------------------------------------------------------------------------
// counter-based generator: two rounds of a 64-bit mix (splitmix64 finaliser) of (seed, element index / 4); each 64-bit result
// gives the four 16-bit uniforms of a 16-B chunk.  Stateless, so backward regenerates the forward mask exactly.
__device__ __forceinline__ unsigned long long mix64(unsigned long long z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__global__ __launch_bounds__(256) void dropout_kernel(const float* __restrict__ x, const float* __restrict__ residual,
                                                       const float* __restrict__ row_scale, float* __restrict__ y, long n,
                                                       long elems_per_sample, float p, unsigned long long seed,
                                                       const unsigned long long* __restrict__ epoch) {
    if (epoch) seed += *epoch;                                 // device-resident step counter: a replayed hipGraph draws a new mask
    const unsigned thr = (unsigned)(p * 65536.0f);             // keep iff u16 >= thr  (P(drop) = thr / 65536)
    const float inv_keep = 1.0f / (1.0f - p);
    const long n4 = n / 4;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const unsigned long long r = mix64(mix64(seed) ^ (unsigned long long)i);
        const f32x4 xv = reinterpret_cast<const f32x4*>(x)[i];
        f32x4 o = residual ? reinterpret_cast<const f32x4*>(residual)[i] : f32x4{0.f, 0.f, 0.f, 0.f};
        const float rs = (row_scale ? row_scale[(4 * i) / elems_per_sample] : 1.0f) * inv_keep;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] += (((unsigned)(r >> (16 * e)) & 0xFFFFu) >= thr) ? rs * xv[e] : 0.f;
        reinterpret_cast<f32x4*>(y)[i] = o;
    }
}

}  // namespace

extern "C" {

int cswin_dropout(const float* x, const float* residual, const float* row_scale, float* y, long n, long elems_per_sample,
                  float p, unsigned long long seed, const unsigned long long* seed_epoch, void* stream) {
    CSWIN_REQUIRE(x && y && n > 0 && n % 4 == 0 && elems_per_sample > 0 && elems_per_sample % 4 == 0, CSWIN_ERR_SHAPE,
                  "dropout: n and elems_per_sample must be positive multiples of 4");
    CSWIN_REQUIRE(p >= 0.f && p < 1.f, CSWIN_ERR_SHAPE, "dropout: p = %f outside [0, 1)", p);
    CSWIN_REQUIRE(((((uintptr_t)x) | ((uintptr_t)y) | ((uintptr_t)residual)) & 15) == 0, CSWIN_ERR_ALIGN, "dropout: 16-B alignment required");
    long b = (n / 4 + 255) / 256;
    hipLaunchKernelGGL(dropout_kernel, dim3((int)(b > 8192 ? 8192 : b)), dim3(256), 0, (hipStream_t)stream, x, residual, row_scale, y, n,
                       elems_per_sample, p, seed, seed_epoch);
    CSWIN_LAUNCH_CHECK();
    return CSWIN_OK;
}


int cswin_nchw_to_tokens(const float* x, float* y, int B, int C, int H, int W, int Cpad, void* stream) {
    CSWIN_REQUIRE(x && y && B > 0 && C > 0 && Cpad >= C && H > 0 && W > 0, CSWIN_ERR_SHAPE, "nchw_to_tokens: bad arguments");
    hipLaunchKernelGGL(nchw_to_tok_kernel, dim3(grid1d((long)B * H * W * Cpad)), dim3(256), 0, (hipStream_t)stream, x, y, B, C, (long)H * W, Cpad);
    CSWIN_LAUNCH_CHECK();
    return CSWIN_OK;
}

int cswin_tokens_to_nchw(const float* x, float* y, int B, int C, int H, int W, int Cpad, void* stream) {
    CSWIN_REQUIRE(x && y && B > 0 && C > 0 && Cpad >= C && H > 0 && W > 0, CSWIN_ERR_SHAPE, "tokens_to_nchw: bad arguments");
    long tiles = (long)B * (((long)H * W + 63) / 64);
    hipLaunchKernelGGL(tok_to_nchw_kernel, dim3((int)(tiles > 8192 ? 8192 : tiles)), dim3(256), 0, (hipStream_t)stream, x, y, B, C, (long)H * W, Cpad);
    CSWIN_LAUNCH_CHECK();
    return CSWIN_OK;
}

// w [Cout][Cin][ks][ks] -> w_perm [Cout][ks*ks][Cpad] (may be NULL) and w_permT [ks*ks][Cout][Cpad] (may be NULL)
int cswin_conv_weight_permute(const float* w, float* w_perm, float* w_permT, int Cout, int Cin, int ks, int Cpad, void* stream) {
    CSWIN_REQUIRE(w && (w_perm || w_permT) && Cout > 0 && Cin > 0 && ks > 0 && Cpad >= Cin, CSWIN_ERR_SHAPE, "conv_weight_permute: bad arguments");
    hipLaunchKernelGGL(conv_w_permute_kernel, dim3(grid1d((long)Cout * ks * ks * Cpad)), dim3(256), 0, (hipStream_t)stream, w, w_perm, w_permT, Cout, Cin, ks * ks, Cpad);
    CSWIN_LAUNCH_CHECK();
    return CSWIN_OK;
}

int cswin_conv_weight_flipT(const float* w, float* wf, int Cout, int Cin, int ks, void* stream) {
    CSWIN_REQUIRE(w && wf && Cout > 0 && Cin > 0 && ks > 0, CSWIN_ERR_SHAPE, "conv_weight_flipT: bad arguments");
    hipLaunchKernelGGL(conv_w_flipT_kernel, dim3(grid1d((long)Cout * Cin * ks * ks)), dim3(256), 0, (hipStream_t)stream, w, wf, Cout, Cin, ks * ks);
    CSWIN_LAUNCH_CHECK();
    return CSWIN_OK;
}

int cswin_conv_weight_unpermute(const float* dw_perm, float* dw, int Cout, int Cin, int ks, int Cpad, void* stream) {
    CSWIN_REQUIRE(dw_perm && dw && Cout > 0 && Cin > 0 && ks > 0 && Cpad >= Cin, CSWIN_ERR_SHAPE, "conv_weight_unpermute: bad arguments");
    hipLaunchKernelGGL(conv_w_unpermute_kernel, dim3(grid1d((long)Cout * Cin * ks * ks)), dim3(256), 0, (hipStream_t)stream, dw_perm, dw, Cout, Cin, ks * ks, Cpad);
    CSWIN_LAUNCH_CHECK();
    return CSWIN_OK;
}

// jobs: HOST array of 1..16 records; every non-NULL image of every job is written by one launch (same bits as the three
// single-weight entry points above)
int cswin_conv_weight_images(const cswin_conv_image_job* jobs, int njobs, void* stream) {
    CSWIN_REQUIRE(jobs && njobs > 0 && njobs <= CSWIN_MAX_CONV_IMAGE_JOBS, CSWIN_ERR_SHAPE, "conv_weight_images: 1..%d jobs", CSWIN_MAX_CONV_IMAGE_JOBS);
    ConvImageJobs J = {};
    int blocks = 0;
    for (int i = 0; i < njobs; ++i) {
        const cswin_conv_image_job& j = jobs[i];
        CSWIN_REQUIRE(j.w && (j.w_perm || j.w_permT || j.w_flipT) && j.Cout > 0 && j.Cin > 0 && j.ks > 0 && j.Cpad >= j.Cin, CSWIN_ERR_SHAPE,
                      "conv_weight_images: bad job %d", i);
        J.j[i] = j;
        J.first_block[i] = blocks;
        const long perm = (j.w_perm || j.w_permT) ? (long)j.Cout * j.ks * j.ks * j.Cpad : 0;
        const long flip = j.w_flipT ? (long)j.Cin * j.ks * j.ks * j.Cout : 0;
        blocks += (int)(((perm > flip ? perm : flip) + CI_ELEMS - 1) / CI_ELEMS);
    }
    J.first_block[njobs] = blocks;
    J.njobs = njobs;
    hipLaunchKernelGGL(conv_w_images_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, J);
    CSWIN_LAUNCH_CHECK();
    return CSWIN_OK;
}

// w_head (ncls, E), w_out (E, C), b_out (E) or NULL -> w_fused (Cpad, C) = [W_head W_out ; 0], b_fused (Cpad) = [W_head b_out ; 0]
int cswin_head_compose(const float* w_head, const float* w_out, const float* b_out, float* w_fused, float* b_fused, int ncls,
                       int E, int C, int Cpad, void* stream) {
    CSWIN_REQUIRE(w_head && w_out && w_fused && b_fused && ncls > 0 && E > 0 && C > 0 && Cpad >= ncls, CSWIN_ERR_SHAPE, "head_compose: bad arguments");
    hipLaunchKernelGGL(head_compose_kernel, dim3((Cpad * C + Cpad + 255) / 256), dim3(256), 0, (hipStream_t)stream, w_head, w_out,
                       b_out, w_fused, b_fused, ncls, E, C, Cpad);
    CSWIN_LAUNCH_CHECK();
    return CSWIN_OK;
}

// gradients of the composition: dw_fused (>= ncls rows of C), db_fused (>= ncls) or NULL -> dw_head (ncls, E), dw_out (E, C),
// db_out (E) (NULL without b_out)
int cswin_head_compose_bwd(const float* w_head, const float* w_out, const float* b_out, const float* dw_fused,
                           const float* db_fused, float* dw_head, float* dw_out, float* db_out, int ncls, int E, int C,
                           void* stream) {
    CSWIN_REQUIRE(w_head && w_out && dw_fused && dw_head && dw_out && ncls > 0 && E > 0 && C > 0 && (!db_out || b_out), CSWIN_ERR_SHAPE,
                  "head_compose_bwd: bad arguments");
    const int total = ncls * E + E * C + (db_out ? E : 0);
    hipLaunchKernelGGL(head_compose_bwd_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, w_head, w_out, b_out,
                       dw_fused, db_fused, dw_head, dw_out, db_out, ncls, E, C);
    CSWIN_LAUNCH_CHECK();
    return CSWIN_OK;
}

}  // extern "C"
