/* libcswin_hip -- C ABI of the MI355X-native (gfx950) CSWin-UNet hot path.
 *
 * The reference (BoloniniD/CSWin-UNet) has no FFI of its own: its seam is the nn.Module surface
 * of networks/cswin_unet.py.  Each entry point below replaces the device work behind one piece of
 * that surface (reference file:line cited per function); cswin_unet_amd/_lib.py binds them with
 * ctypes and cswin_unet_amd/networks/cswin_unet.py calls them from modules that keep the
 * reference's class names, constructor signatures and state_dict keys.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is DEVICE memory owned by the caller
 *     (PyTorch's caching allocator in practice), fp32 unless stated, densely packed row-major.
 *   - kernels are enqueued on `stream` (a hipStream_t passed as void*), never synchronise, never
 *     allocate, keep no pointer past return; entry points are re-entrant (no global mutable state
 *     except the thread-local error string) and hipGraph-capturable.
 *   - return 0 on success, a negative CSWIN_ERR_* code otherwise; cswin_last_error() gives the
 *     message for the calling thread.  No exceptions, no exit() (the reference print+exit(0)s on a
 *     bad stripe mode, cswin_unet.py:50-51; here that is CSWIN_ERR_SHAPE).
 *   - "tokens" = the (B, L, C) layout the reference keeps between blocks; L = H*W row-major.
 */
#ifndef CSWIN_HIP_H
#define CSWIN_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped whenever a prototype or struct below changes (1: round 1; 2: round 2 -- stream / precision / storage arguments; 3: round 3 --
 * cswin_attn_fwd writes y0, cswin_attn_bwd reads it).  cswin_abi_version() returns the value the library was built with: a consumer
 * compiled against another header must refuse to call it.  Entry points that are only ADDED (cswin_seg_metrics*, cswin_resize_banded, cswin_argmax_zoom_back, cswin_augment_*,
 * cswin_chunk_sumsq, cswin_norm_finalize, cswin_adamw_flat, cswin_tpgm_*, cswin_importance_accumulate, cswin_flat_axpby, cswin_consolidate_*, cswin_argmax_zoom_back_classes, cswin_class_counts, cswin_gaussian_blur, cswin_eb_tiles,
 * cswin_eb_finalize, cswin_rate_finalize, cswin_adam_flat, cswin_components_*, cswin_drop_path_order, cswin_linear_*_skip,
 * cswin_surface_dist*, cswin_view_batch, cswin_tta_argmax_zoom_back, cswin_gaussian_blur_each, cswin_intensity_*, cswin_sdm_workspace, cswin_signed_distance_maps, cswin_bd_loss_*) do not bump it: every prototype an older consumer binds is unchanged. */
#define CSWIN_ABI_VERSION 4

#define CSWIN_OK 0
#define CSWIN_ERR_SHAPE (-1)
#define CSWIN_ERR_ALIGN (-2)
#define CSWIN_ERR_WORKSPACE (-3)
#define CSWIN_ERR_HIP (-4)
#define CSWIN_ERR_UNSUPPORTED (-5)

/* A slab reduction left pending by a producer called with `deferred` != NULL; batch up to 48 of them into one launch with
 * cswin_rows_sum_multi (a CSWinBlock backward has six to eight: four weight gradients, two LayerNorm dgamma/dbeta, the LePE conv
 * gradients; cswin_unet_amd.ops queues the jobs of a whole backward pass and reduces them in one or two launches).
 * conv_kk / conv_cin != 0: columns [0, n_first) are a convolution weight gradient in the implicit-GEMM order [Cout][k*k][Cin] and
 * are stored to `out` in the nn.Conv2d order [Cout][Cin][k][k].  For an input whose channels are a zero-padded image of the
 * parameter's (cswin_conv_tok_bwd_weight_cpad) conv_cin = Cin | Cin_param << 16: the padded channels' columns are dropped and `out`
 * is [Cout][Cin_param][k][k]. */
typedef struct cswin_reduce_job {
    const float* part;
    float* out;
    float* out2;
    long long n_first, n, stride;
    int rows, reserved;
    int conv_kk, conv_cin;
} cswin_reduce_job;

const char* cswin_last_error(void);
int cswin_abi_version(void);
int cswin_device_ok(void); /* 1 if the current HIP device is gfx950 */
/* `precision` argument of the Linear and convolution entry points (and field of cswin_wgrad_desc): 0 = exact fp32 MFMA (the
 * parity path of BASELINE configs[1]); 1 = operands rounded to bf16 while staged into LDS, bf16 MFMA, fp32 accumulation, fp32
 * tensors in HBM (the "bf16" of BASELINE configs[2..4] as far as the GEMMs go; torch.autocast(bfloat16) on the reference's
 * Linear / Conv2d is the closest reference-side equivalent).  The library keeps NO precision state: entry points are
 * re-entrant and may be called with different precisions from different threads / streams. */

/* ---- LePEAttention (cswin_unet.py:31-109), both branches of a CSWinBlock in one launch (:171-176) ----
 * qkv (B, L, 3C) = output of the qkv Linear, channel layout [q | k | v] (:169).
 * nbranch = 2: branch i works on channels [i*C/2, (i+1)*C/2) of each of q,k,v with stripe mode idx[i]
 *   (0: H_sp=reso, W_sp=split; 1: H_sp=split, W_sp=reso; :43-48) and heads[i] heads;
 * nbranch = 1: whole C, idx[0] = -1 (window = whole map).  Head dim 8, 16, 24 or 32 (equal in both branches); windows of up
 *   to 288 tokens.
 * lepe_w[i] (Cb, 9) / lepe_b[i] (Cb) = get_v depthwise 3x3 weight/bias of branch i (:55).
 * y (B, L, C): x = softmax(scale q k^T) v + lepe, scattered by windows2img and concatenated (:98-107, :174).
 * y0 (B, L, C) or NULL: the same without the lepe term (attn @ v of :103), in y's storage format.  Saved for the backward only:
 *   rowsum(dO o y0) is the row term of the softmax gradient, so the backward neither recomputes LePE(v) nor reduces P o dP
 *   across keys.  Pass NULL when no backward follows.
 * lse (B, sum(heads), L): row log-sum-exp saved for backward.  scale <= 0 selects head_dim^-0.5 (:42). */
int cswin_attn_fwd(const float* qkv, const float* const* lepe_w, const float* const* lepe_b, float* y, float* y0, float* lse,
                   int B, int reso, int C, int nbranch, const int* heads, const int* idx, int split, float scale,
                   float drop_p, unsigned long long drop_seed, const unsigned long long* drop_epoch, int qkv_bf16, void* stream);
/* drop_p in [0, 1) (0 = off): nn.Dropout on the attention probabilities (cswin_unet.py:101, attn_drop_rate): y = ((P o M) v) + lepe
 * with M = keep / (1 - drop_p), keep a counter-based hash of (drop_seed, batch, head, window, query, key).  cswin_attn_bwd called
 * with the same (drop_p, drop_seed) regenerates the mask; the softmax statistics (lse) are those of the undropped P.
 * drop_epoch: NULL, or a DEVICE counter whose value is added to drop_seed when the kernel runs: a captured hipGraph (seed frozen
 * at capture) then draws a new mask on every replay if a kernel in the graph advances the counter once per step. */
size_t cswin_attn_bwd_workspace(int B, int reso, int C, int nbranch, const int* heads, const int* idx, int split);
/* autograd backward of the above: dqkv (B, L, 3C), dlepe_w[i] (Cb, 9), dlepe_b[i] (Cb) are overwritten.
 * y0 = the forward's y0 output (NOT y).  The per-window partial slabs of the LePE conv weight / bias gradient are reduced by
 * one extra launch, or left in deferred[0..nbranch) for cswin_rows_sum_multi. */
int cswin_attn_bwd(const float* qkv, const float* const* lepe_w, const float* const* lepe_b, const float* lse,
                   const float* y0, const float* dy, float* dqkv, float* const* dlepe_w, float* const* dlepe_b,
                   void* workspace, size_t ws_bytes, int B, int reso, int C, int nbranch, const int* heads, const int* idx,
                   int split, float scale, cswin_reduce_job* deferred, float drop_p, unsigned long long drop_seed,
                   const unsigned long long* drop_epoch, int qkv_bf16, void* stream);
/* qkv_bf16: storage mode of both attention entry points.  0: every tensor fp32.  1: qkv (and dqkv) are STORED as bf16 -- the
 * output format of cswin_linear_fwd(io_bf16 bit 1).  3: additionally y and y0 (the forward outputs) are stored
 * as bf16 -- the input format of the proj Linear's io_bf16 bit 0.  In modes 0 - 3 the arithmetic of the attention kernels is
 * fp32 throughout (v_mfma_f32_16x16x4_f32).  7: mode 3 with bf16 MATRIX instructions (v_mfma_f32_16x16x32_bf16 for QK^T and
 * dO V^T, v_mfma_f32_16x16x16_bf16 for P V, dV, dK, dQ): operands (scaled q, k, v, P, dS, dO) are rounded to bf16 on their way
 * into the matrix pipe -- what the reference's softmax(dtype=attn.dtype) @ v does under a bf16 config (cswin_unet.py:100) --,
 * accumulators, softmax statistics, LePE and everything stored are as in mode 3.  dy, lse and the LePE parameters / gradients
 * are fp32. */

/* ---- img2windows / windows2img (cswin_unet.py:184-202): index-only, bit-exact ----
 * img (B, C, H, W) -> out (B*nH*nW, H_sp*W_sp, C);   win (B*nH*nW, H_sp*W_sp, C) -> out (B, H, W, C) */
int cswin_img2windows(const float* img, float* out, int B, int C, int H, int W, int H_sp, int W_sp, void* stream);
int cswin_windows2img(const float* win, float* out, int B, int C, int H, int W, int H_sp, int W_sp, void* stream);

/* ---- nn.LayerNorm over C (cswin_unet.py:168,179,218,341,497,533); any C % 4 == 0 up to 1024 (CSWIN_ERR_UNSUPPORTED
 *      otherwise): kernels specialised per width for C in {32,64,128,256,512,1024}, one wave per row for every other C ---- */
int cswin_layernorm_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd,
                        int M, int C, float eps, int y_bf16, void* stream);
/* y_bf16 != 0: y is STORED as bf16 (bf16 activation storage: the input format of cswin_linear_fwd io_bf16 bit 0 and of
 * cswin_wgrad_desc io_bf16 bit 1); mean / rstd stay fp32. */
size_t cswin_layernorm_bwd_workspace(int M, int C);
/* dx = dres (optional residual-path gradient, may alias dx) + LN backward; dgamma/dbeta overwritten (by the returned
 * job when `deferred` is given, immediately otherwise).  dx_bf16: NULL, or M * C bf16 that receive a rounded copy of dx -- the
 * bf16 mode's GEMMs read that twin (cswin_linear_bwd_data io_bf16 bit 0, cswin_wgrad_desc io_bf16 bit 0) while the residual
 * path keeps the fp32 dx. */
int cswin_layernorm_bwd(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma,
                        const float* dres, float* dx, float* dgamma, float* dbeta, void* workspace, size_t ws_bytes,
                        int M, int C, cswin_reduce_job* deferred, void* dx_bf16, void* stream);

/* ---- nn.Linear family: qkv / proj / Mlp.fc1+GELU / fc2 (cswin_unet.py:125,134,17-27), concat_linear{4,3,2}
 *      (:404,417,428 with the torch.cat of :509,518,526 fused as a two-source K loop), 1x1 convs of CARAFE ----
 * acc = [x | x2] (M, K) @ w (N, K)^T + bias.
 *   y_act != NULL : y = acc (pre-activation), y_act = GELU_erf(acc)
 *   residual != NULL : y = residual + row_scale[m / rows_per_sample] * acc     (x + drop_path(f(x)), :178-179)
 * x2 == NULL: single source.  row_scale may be NULL (= 1). */
int cswin_linear_fwd(const float* x, const float* x2, int k_split, const float* w, const float* bias, float* y,
                     float* y_act, const float* residual, const float* row_scale, int rows_per_sample, int M, int N,
                     int K, int precision, int io_bf16, void* stream);
/* io_bf16 (precision 1 only; 0 = every tensor fp32): tensors STORED as bf16 in HBM, fp32 accumulation as before.
 *   cswin_linear_fwd:      bit 0 = x, bit 1 = y and y_act, bit 2 = w;
 *   cswin_linear_bwd_data: bit 0 = dy, bit 1 = dx, bit 2 = w, bit 3 = gelu_pre.
 * Bit 2 reads the weights' bf16 SHADOW (same [N][K] layout; cswin_sgd_flat keeps it current): the GEMM rounds fp32 weights
 * to bf16 while staging them anyway, so results are bit-identical and the weight traffic halves.  Concat / split / add
 * forms accept bit 2 only.
 * dx (M, K) = add + row_scale * ((dy (M, N) @ w (N, K)) * gelu'(gelu_pre));  columns >= k_split go to dx2 if given */
int cswin_linear_bwd_data(const float* dy, const float* w, float* dx, float* dx2, int k_split, const float* gelu_pre,
                          const float* row_scale, int rows_per_sample, const float* add, int M, int N, int K,
                          int precision, int io_bf16, void* stream);
size_t cswin_linear_bwd_weight_workspace(int M, int N, int K);
/* dw (N, K) = (row_scale * dy)^T @ [x | x2];  dbias (N) = column sums (may be NULL); `deferred` as for layernorm_bwd */
int cswin_linear_bwd_weight(const float* dy, const float* x, const float* x2, int k_split, const float* row_scale,
                            int rows_per_sample, float* dw, float* dbias, void* workspace, size_t ws_bytes, int M,
                            int N, int K, cswin_reduce_job* deferred, int precision, void* stream);
/* One problem of cswin_linear_bwd_weight_batch: dw (N, K) = (row_scale * dy)^T @ x, dbias (N) = column sums of dy (or NULL). */
typedef struct cswin_wgrad_desc {
    const float* dy;         /* (M, N) */
    const float* x;          /* (M, K) */
    const float* row_scale;  /* per-sample multiplier of the dy rows, or NULL */
    float* dw;               /* (N, K) */
    float* dbias;            /* (N) or NULL */
    void* workspace;         /* cswin_linear_bwd_weight_workspace(M, N, K) bytes */
    size_t ws_bytes;
    int rows_per_sample, M, N, K;
    int precision;           /* 0 = exact fp32 MFMA, 1 = bf16 operands (all problems of one launch agree) */
    int io_bf16;             /* precision 1 only: bit 0 = dy is stored as bf16, bit 1 = x is stored as bf16 */
} cswin_wgrad_desc;
/* Up to 4 independent weight gradients (the four nn.Linear of a CSWinBlock, cswin_unet.py:125,134,17-19) in ONE launch;
 * deferred[0..n) receive their slab reductions (required: run them with cswin_rows_sum_multi, or hand them to a later call as
 * `pending`).  pending[0..npending), npending <= 16 (may be NULL / 0): reductions left pending by EARLIER calls; they are run by
 * this launch's last workgroups -- memory-bound work beside matrix-pipe-bound work instead of a launch of its own -- or, where the
 * batch does not go out as one launch, by a cswin_rows_sum_multi launch; either way they must not be run again. */
int cswin_linear_bwd_weight_batch(const cswin_wgrad_desc* problems, int n, cswin_reduce_job* deferred, const cswin_reduce_job* pending,
                                  int npending, void* stream);
/* The tail of a CSWinBlock's backward (cswin_unet.py:171 / :125 backward): dx (M, K) = dy (M, N) @ w (N, K) -- the qkv Linear's data
 * gradient, plain fp32 operands -- together with the block's weight gradients (`problems`, `deferred` exactly as above).  Both
 * only wait for dqkv and neither needs the other: in fp32 with 16-B aligned operands they share ONE launch, otherwise the data
 * gradient is launched first and the batch follows; the results are those of cswin_linear_bwd_data + cswin_linear_bwd_weight_batch.
 * pending / npending as for cswin_linear_bwd_weight_batch. */
int cswin_linear_bwd_tail(const float* dy, const float* w, float* dx, int M, int N, int K, const cswin_wgrad_desc* problems, int n,
                          cswin_reduce_job* deferred, const cswin_reduce_job* pending, int npending, void* stream);
/* The two calls above with SAMPLE MASKS on the weight gradients (DropPath: the dy rows of a dropped sample are exact zeros, so they
 * add nothing to dw / dbias).  skip: host array of n device pointers (an entry, or skip itself, may be NULL: no mask); skip[i] holds
 * nsamples[i] floats, one per sample of rows_per_sample consecutive rows, M == nsamples[i] * rows_per_sample.  A sample whose float is
 * 0 is left out of the reduction and its rows of dy and x are NOT READ (they may hold anything); the kept samples' rows are shared
 * out evenly over the launch's workgroups, so the launch gets shorter by the dropped share.  row_scale keeps its meaning.  With every
 * sample kept the results equal the unmasked call's bit for bit; otherwise the summation is regrouped (last-bit differences).
 * Masks need precision 0, nsamples <= 256, N and K multiples of 4 and 16-B aligned operands: anything else is an error return,
 * never an unmasked run.  The unmasked calls are these with skip == NULL. */
int cswin_linear_bwd_weight_batch_masked(const cswin_wgrad_desc* problems, int n, cswin_reduce_job* deferred,
                                         const cswin_reduce_job* pending, int npending, const float* const* skip, const int* nsamples,
                                         void* stream);
int cswin_linear_bwd_tail_masked(const float* dy, const float* w, float* dx, int M, int N, int K, const cswin_wgrad_desc* problems, int n,
                                 cswin_reduce_job* deferred, const cswin_reduce_job* pending, int npending, const float* const* skip,
                                 const int* nsamples, void* stream);
/* ---- DropPath: the forward and data-gradient Linears of a residual branch without the dropped samples' rows ----
 * One wave per row of the step's draws: scales (rows, B) = (u (rows, B) < keep[row]) / keep[row], bit for bit the factors torch
 * computes from the same draws, and order (rows, 1 + B): order[r][0] = the number of kept samples, then the kept sample indices
 * ascending, then the dropped ones ascending.  B <= 256. */
int cswin_drop_path_order(const float* u, const float* keep, float* scales, int* order, int rows, int B, void* stream);
/* cswin_linear_fwd / cswin_linear_bwd_data / cswin_linear_bwd_tail_masked with a SAMPLE ORDER: order = one row of
 * cswin_drop_path_order's output (1 + nsamples ints), M == nsamples * rows_per_sample.  The launch computes the kept samples' rows
 * -- bit for bit what the unmapped call gives them -- in its first workgroups; the A rows (x / dy) and the gelu_pre rows of a
 * dropped sample are NOT READ, and its rows of the result hold what zero A rows give: y = bias, y_act = GELU(bias), with a residual
 * y = the residual row itself, dx = +0.  With every sample kept the whole result equals the unmapped call's bit for bit.  An order
 * needs precision 0, io_bf16 0, no x2 / dx2 / add, nsamples <= 256, N and K multiples of 4 and 16-B aligned operands: anything
 * else is an error return, never an unmapped run.  The tail's order (over nsamples_order samples of M / nsamples_order rows) maps its
 * data gradient; skip / nsamples stay the weight gradients' masks. */
int cswin_linear_fwd_skip(const float* x, const float* x2, int k_split, const float* w, const float* bias, float* y,
                          float* y_act, const float* residual, const float* row_scale, int rows_per_sample, int M, int N,
                          int K, int precision, int io_bf16, const int* order, int nsamples, void* stream);
int cswin_linear_bwd_data_skip(const float* dy, const float* w, float* dx, float* dx2, int k_split, const float* gelu_pre,
                               const float* row_scale, int rows_per_sample, const float* add, int M, int N, int K,
                               int precision, int io_bf16, const int* order, int nsamples, void* stream);
int cswin_linear_bwd_tail_skip(const float* dy, const float* w, float* dx, int M, int N, int K, const cswin_wgrad_desc* problems, int n,
                               cswin_reduce_job* deferred, const cswin_reduce_job* pending, int npending, const float* const* skip,
                               const int* nsamples, const int* order, int nsamples_order, void* stream);
/* jobs: host array of 1..48 pending reductions (the workspaces they point into must still be alive) */
int cswin_rows_sum_multi(const cswin_reduce_job* jobs, int njobs, void* stream);

/* ---- convolutions on tokens (NHWC) as implicit GEMM: stage1_conv_embed 7x7 s4 p2 (cswin_unet.py:339),
 *      Merge_Block 3x3 s2 p1 (:208,214-217), CARAFE encoder 3x3 s1 p1 (:228-229,241) ----
 * x (B, H*W, Cin) -> y (B, OH*OW, Cout).  Weights are given in the implicit-GEMM images made by
 * cswin_conv_weight_permute from the nn.Conv2d parameter [Cout][Cin][ks][ks]. Cin % 4 == 0. */
int cswin_conv_tok_fwd(const float* x, const float* w_perm, const float* bias, float* y, int B, int H, int W, int Cin,
                       int Cout, int ks, int stride, int pad, int precision, void* stream);
int cswin_conv_tok_bwd_data(const float* dy, const float* w_permT, float* dx, int B, int H, int W, int Cin, int Cout,
                            int ks, int stride, int pad, int precision, void* stream);
size_t cswin_conv_tok_bwd_weight_workspace(int B, int H, int W, int Cin, int Cout, int ks, int stride, int pad);
/* dw: [Cout][ks*ks][Cin] (torch_layout 0, the image cswin_conv_weight_unpermute takes) or directly the nn.Conv2d parameter
 * layout [Cout][Cin][ks][ks] (torch_layout 1: the slab reduction writes it, no separate unpermute launch).  deferred: NULL, or
 * the slot that receives the slab reduction instead of its launch (as for the Linear weight gradients). */
int cswin_conv_tok_bwd_weight(const float* dy, const float* x, float* dw, float* dbias, void* workspace,
                              size_t ws_bytes, int B, int H, int W, int Cin, int Cout, int ks, int stride, int pad,
                              int torch_layout, cswin_reduce_job* deferred, int precision, void* stream);
/* w [Cout][Cin][ks][ks] -> w_perm [Cout][ks*ks][Cpad] and/or w_permT [ks*ks][Cout][Cpad] (zero padded channels) */
int cswin_conv_weight_permute(const float* w, float* w_perm, float* w_permT, int Cout, int Cin, int ks, int Cpad,
                              void* stream);
int cswin_conv_weight_unpermute(const float* dw_perm, float* dw, int Cout, int Cin, int ks, int Cpad, void* stream);
/* w [Cout][Cin][ks][ks] -> wf [Cin][ks*ks (mirrored)][Cout]: with it the data gradient of a stride-1, pad = ks/2 convolution is
 * cswin_conv_tok_fwd(dy, wf, NULL, dx, B, H, W, Cout, Cin, ks, 1, pad) (CARAFE encoder, cswin_unet.py:228,241) */
int cswin_conv_weight_flipT(const float* w, float* wf, int Cout, int Cin, int ks, void* stream);
/* Every weight image of a step in ONE launch: jobs = host array of 1..16 records; each non-NULL image of each job is written,
 * bit for bit what the three entry points above write (the model refreshes all its convolutions' images at the start of a
 * forward pass instead of one launch per convolution and direction). */
typedef struct cswin_conv_image_job {
    const float* w;          /* nn.Conv2d parameter [Cout][Cin][ks][ks] */
    float* w_perm;           /* [Cout][ks*ks][Cpad] or NULL */
    float* w_permT;          /* [ks*ks][Cout][Cpad] or NULL */
    float* w_flipT;          /* [Cin][ks*ks (mirrored)][Cout] or NULL */
    int Cout, Cin, ks, Cpad;
} cswin_conv_image_job;
int cswin_conv_weight_images(const cswin_conv_image_job* jobs, int njobs, void* stream);
/* cswin_conv_tok_bwd_weight for an input whose Cin channels are a zero-padded image of the parameter's Cin_param <= Cin (the
 * patch embedding: 3 image channels in 4-channel tokens).  dw is the nn.Conv2d parameter [Cout][Cin_param][ks][ks]; the slab
 * reduction writes it and drops the padded channels (its job carries conv_cin = Cin | Cin_param << 16): no cswin_conv_weight_unpermute
 * launch.  Workspace and deferred as for cswin_conv_tok_bwd_weight. */
int cswin_conv_tok_bwd_weight_cpad(const float* dy, const float* x, float* dw, float* dbias, void* workspace, size_t ws_bytes,
                                   int B, int H, int W, int Cin, int Cin_param, int Cout, int ks, int stride, int pad,
                                   cswin_reduce_job* deferred, int precision, void* stream);

/* ---- layout adapters at the ends of the token pipeline (Rearrange 'b c h w -> b (h w) c', cswin_unet.py:340;
 *      view/permute of up_x4, :540-541) ---- */
int cswin_nchw_to_tokens(const float* x, float* y, int B, int C, int H, int W, int Cpad, void* stream);
int cswin_tokens_to_nchw(const float* x, float* y, int B, int C, int H, int W, int Cpad, void* stream);

/* ---- CARAFE / CARAFE4 reassembly (cswin_unet.py:242-264, 292-314): softmax over the 9 taps + weighted
 *      3x3 neighbourhood sum + pixel_shuffle, on tokens.  e (B, H*W, 9*S*S) = encoder output, channel
 *      k*S*S + s;  z (B, H*W, Cz) = features to reassemble (the `out` 1x1 conv is applied BEFORE, at low
 *      resolution: it commutes with the reassembly);  out (B, (S*H)*(S*W), Cz) = bias + reassembly.
 *      Cz % 4 == 0, S in {2, 4} (CSWIN_ERR_UNSUPPORTED otherwise).  The kernels move channels 16 bytes at a time: z, bias,
 *      the token-form out and dout, dz (and the plane-form dout) must be 16-byte aligned, CSWIN_ERR_ALIGN before any launch
 *      otherwise; e, wt_save, de, dbias, the workspace and the plane-form out need their element's alignment only. ---- */
int cswin_carafe_fwd(const float* e, const float* z, const float* bias, float* out, float* wt_save, int B, int H,
                     int W, int Cz, int S, void* stream);
size_t cswin_carafe_bwd_workspace(int B, int H, int W, int Cz, int S);
/* dbias (Cz, may be NULL) = column sums of dout, formed from per-workgroup partial sums in `workspace`; `deferred` as for
 * layernorm_bwd (NULL: reduced immediately; else the job is returned, zeroed when there is no bias) */
int cswin_carafe_bwd(const float* dout, const float* z, const float* wt_save, float* de, float* dz, float* dbias,
                     void* workspace, size_t ws_bytes, int B, int H, int W, int Cz, int S, cswin_reduce_job* deferred, void* stream);
/* The reassembly written to / differentiated from (B, C, S*H, S*W) planes, the first C <= Cz channels (the logits of the fused
 * segmentation head: C classes carried in Cz = 16 channel tokens) -- the (B, (S*H)*(S*W), Cz) token tensor and the
 * cswin_tokens_to_nchw / cswin_nchw_to_tokens passes around the loss do not exist.  Same bits as the token forms followed by
 * those adapters.  The backward form exists where cswin_carafe_bwd_nchw_ok() returns 1 (S = 4, Cz = 16, H and W multiples of 8). */
int cswin_carafe_fwd_nchw(const float* e, const float* z, const float* bias, float* out, float* wt_save, int B, int H, int W,
                          int Cz, int C, int S, void* stream);
int cswin_carafe_bwd_nchw_ok(int H, int W, int Cz, int S);
int cswin_carafe_bwd_nchw(const float* dout, const float* z, const float* wt_save, float* de, float* dz, float* dbias,
                          void* workspace, size_t ws_bytes, int B, int H, int W, int Cz, int C, int S, cswin_reduce_job* deferred,
                          void* stream);

/* ---- the fused segmentation head's weights (up_x4: `output` 1x1 applied after upsample1.out 1x1, cswin_unet.py:540-543) ----
 * w_head (ncls, E), w_out (E, C), b_out (E) or NULL -> w_fused (Cpad, C) = [W_head W_out ; 0], b_fused (Cpad) = [W_head b_out ; 0];
 * and the gradients of the three from dw_fused (>= ncls rows of C) and db_fused (>= ncls, or NULL).  One small launch each. */
int cswin_head_compose(const float* w_head, const float* w_out, const float* b_out, float* w_fused, float* b_fused, int ncls,
                       int E, int C, int Cpad, void* stream);
int cswin_head_compose_bwd(const float* w_head, const float* w_out, const float* b_out, const float* dw_fused,
                           const float* db_fused, float* dw_head, float* dw_out, float* db_out, int ncls, int E, int C,
                           void* stream);

/* ---- loss of the training step: 0.4*CE + 0.6*Dice (trainer.py:55-57, utils.py:9-45) ----
 * logits (B, ncls, HW) fp32, labels (B, HW) int64.  sums[1 + 3*ncls] = {sum -log p[label], intersect_c, y_sum_c,
 * z_sum_c}: all-reduce these across data-parallel ranks for the reference's global-batch Dice. */
size_t cswin_loss_workspace(int B, int ncls, long HW);
/* inputs_are_probs != 0: `logits` already holds class probabilities (DiceLoss(..., softmax=False), utils.py:32-34): no softmax
 * is applied, the gradient is d/d(probabilities) and only the Dice term is meaningful (call with w_ce = 0).
 * class_weight: ncls device floats or NULL (= all 1): utils.py:44 `loss += dice * weight[i]`.
 * A label outside [0, ncls) -- judged on the whole int64 value, so 2^32 + 1 is outside -- makes sums[0] (hence the loss) NaN:
 * the device-side counterpart of CrossEntropyLoss raising; to the Dice sums and to the gradient such a pixel has no class.
 * sums[0] adds (max_j logit_j - logit_label) + log sum_j exp(logit_j - max) per pixel, nn.CrossEntropyLoss's log-softmax form:
 * it does not saturate when the label's logit lies far below the row maximum (100 for logits [100, 0] and label 1).
 * With inputs_are_probs the term is -log p[label] as given, again without a clamp: a label probability of exactly 0 makes sums[0]
 * and out3[1] +inf (its true value); the loss is unaffected, because that mode is called with w_ce = 0 and finalize then leaves
 * the CE term out. */
int cswin_loss_sums(const float* logits, const long long* labels, float* sums, void* workspace, size_t ws_bytes, int B,
                    int ncls, long HW, int inputs_are_probs, void* stream);
int cswin_loss_finalize(const float* sums, float* out3, float* coef, double n_pixels, int ncls, float w_ce,
                        float w_dice, const float* class_weight, void* stream);
int cswin_loss_bwd(const float* logits, const long long* labels, const float* coef, const float* grad_out,
                   float* dlogits, float ce_scale, float dice_scale, int B, int ncls, long HW, int inputs_are_probs,
                   void* stream);

/* ---- objective of the continual-learning workflow (universal_train.py:904-932): focal CE (:141-174) + soft Dice on the widened
 *      logits, temperature-T distillation (:618-623) of their first `nold` channels towards a frozen teacher ----
 * logits (B, ncls, HW) fp32, labels (B, HW) int64, teacher (B, nold, HW) fp32 (NULL only with nold == 0: no KD term),
 * label_map: n_map device int32 or NULL; a label l becomes label_map[l] for 0 <= l < n_map and no class otherwise (:243-258),
 * class_weight: ncls device floats or NULL (= all 1), the `weight` of F.cross_entropy inside the focal term.
 * sums[3 + 3*ncls]: the first 1 + 3*ncls are cswin_loss_sums' {sum -log p[label], intersect_c, y_sum_c, z_sum_c};
 * [1 + 3*ncls] = sum of alpha * (1 - pt)^gamma * ce with ce = w[label] * -log p[label], pt = exp(-ce);
 * [2 + 3*ncls] = sum over pixels of sum_{c < nold} q_c (log q_c - log pT_c), q / pT = softmax of the teacher's / the student's first
 * nold logits over T.  All are plain sums over the local pixels: all-reduce them across data-parallel ranks.
 * A label that is no class after the map makes sums[0] and the focal sum NaN (cswin_loss_sums' convention; the reference's focal
 * loss clamps it), has no class in the Dice sums and no focal gradient.  ncls 2..16, 0 <= nold <= ncls, temperature > 0 and
 * focal_gamma 0 or >= 1, otherwise CSWIN_ERR_UNSUPPORTED / CSWIN_ERR_SHAPE before any launch. */
size_t cswin_cl_loss_workspace(int B, int ncls, long HW);
int cswin_cl_loss_sums(const float* logits, const long long* labels, const int* label_map, int n_map, const float* teacher,
                       const float* class_weight, float* sums, void* workspace, size_t ws_bytes, int B, int ncls, int nold,
                       long HW, float temperature, float focal_alpha, float focal_gamma, void* stream);
/* out5 = {loss, focal, dice, kd, ce}: focal = S_focal / n_pixels, ce = S_0 / n_pixels, dice and coef[2*ncls] as cswin_loss_finalize
 * forms them without class weights, kd = S_kd * T^2 / batch (F.kl_div's 'batchmean': per IMAGE the sums cover, not per pixel),
 * loss = (1 - kd_weight) * (w_focal * focal + w_dice * dice) + kd_weight * kd; a term whose weight is 0 is left out, NaN or not. */
int cswin_cl_loss_finalize(const float* sums, float* out5, float* coef, double n_pixels, double batch, int ncls, float w_focal,
                           float w_dice, float kd_weight, float temperature, void* stream);
/* dlogits = grad_out (NULL = 1) * [focal_scale * d focal-sum + dice_scale * d sum_c dice_c + kd_scale * (pT - q) on the first nold
 * channels]; focal_scale = (1 - kd_weight) * w_focal / n_pixels, dice_scale = (1 - kd_weight) * w_dice / ncls (times the world
 * size under gradient averaging), kd_scale = kd_weight * T / B.  Every channel of dlogits is written once. */
int cswin_cl_loss_bwd(const float* logits, const long long* labels, const int* label_map, int n_map, const float* teacher,
                      const float* class_weight, const float* coef, const float* grad_out, float* dlogits, float focal_scale,
                      float dice_scale, float kd_scale, int B, int ncls, int nold, long HW, float temperature, float focal_alpha,
                      float focal_gamma, void* stream);

/* ---- signed distance maps of label slices, for the boundary loss (Kervadec et al., MIDL 2019: one_hot2dist) ----
 * labels (B, H, W) int64 -> phi (B, ncls, H, W) fp32.  Per sample b and class c, with M = (labels[b] == c): phi = +d(p, M) outside
 * M and -(d(p, ~M) - 1) inside it, d the Euclidean distance in pixels (unit spacing, per 2-D slice) to the nearest pixel of the
 * set; phi[b][c] = 0 everywhere when M is empty or the whole slice (there is no boundary).  A label outside [0, ncls), judged on
 * the whole int64 value, belongs to no class.  The value is (float)sqrt((double)d2) of the exact integer squared distance
 * (inside: (float)(1 - sqrt((double)d2))), which is scipy.ndimage.distance_transform_edt's edt(~M) * ~M - (edt(M) - 1) * M bit for
 * bit; integer atomics only, so two runs give the same bits.  Limits: B >= 1, 1 <= H, W <= 2047 (CSWIN_ERR_SHAPE), 2 <= ncls <= 255
 * (CSWIN_ERR_UNSUPPORTED); a refused call launches nothing.  cswin_sdm_workspace returns 0 (and sets the error) outside them;
 * the workspace holds the row pass's uint16 distances (2 bytes per element of phi) and a counter per (b, c). */
size_t cswin_sdm_workspace(int B, int ncls, int H, int W);
int cswin_signed_distance_maps(const long long* labels, float* phi, void* workspace, size_t ws_bytes, int B, int ncls, int H,
                               int W, void* stream);

/* ---- boundary objective: w_ce * CE + w_dice * Dice + alpha * boundary, boundary = 1 / n_pixels * sum over pixels and classes of
 *      wb_c * softmax(logits)_c * phi_c ----
 * logits and phi (B, ncls, HW) fp32, labels (B, HW) int64; phi: cswin_signed_distance_maps of the same labels (or any map);
 * wb: ncls device floats or NULL (= 0 for class 0, 1 for the others).  Logits only: there is no probabilities mode.  ncls as
 * cswin_loss_sums takes it.
 * cswin_bd_loss_workspace: bytes of cswin_bd_loss_sums' workspace. */
size_t cswin_bd_loss_workspace(int B, int ncls, long HW);
/* sums[2 + 3*ncls]: the first 1 + 3*ncls are cswin_loss_sums', out-of-range labels included (sums[0] NaN);
 * [1 + 3*ncls] = sum over the local pixels and the classes of (wb_c * p_c) * phi_c, un-normalised: all-reduce across ranks. */
int cswin_bd_loss_sums(const float* logits, const long long* labels, const float* phi, const float* wb, float* sums,
                       void* workspace, size_t ws_bytes, int B, int ncls, long HW, void* stream);
/* out4 = {loss, ce, dice, boundary}: ce, dice and coef[2*ncls] as cswin_loss_finalize forms them (class_weight: the Dice's),
 * boundary = S_boundary / n_pixels, loss = w_ce * ce + w_dice * dice + alpha * boundary with alpha = alpha_dev[0], ONE DEVICE
 * FLOAT: the weight is scheduled during training and a captured graph must see its current value.  A term whose weight is 0 is
 * left out, NaN or not. */
int cswin_bd_loss_finalize(const float* sums, float* out4, float* coef, double n_pixels, int ncls, float w_ce, float w_dice,
                           const float* alpha_dev, const float* class_weight, void* stream);
/* dlogits_c = grad_out (NULL = 1) * [cswin_loss_bwd's two terms + alpha_dev[0] * bd_scale * p_c * (wb_c phi_c - sum_j p_j wb_j phi_j)];
 * ce_scale and dice_scale as there, bd_scale = 1 / (local pixel count).  Every channel of dlogits is written once. */
int cswin_bd_loss_bwd(const float* logits, const long long* labels, const float* phi, const float* wb, const float* coef,
                      const float* alpha_dev, const float* grad_out, float* dlogits, float ce_scale, float dice_scale,
                      float bd_scale, int B, int ncls, long HW, void* stream);

/* ---- optimiser: torch.optim.SGD(momentum, weight_decay) (trainer.py:42,60) on one flat buffer ---- */
int cswin_sgd_flat(float* p, const float* g, float* m, long n, const float* lr_dev, float momentum,
                   float weight_decay, float grad_scale, void* shadow_bf16, void* stream);
/* shadow_bf16: NULL, or n bf16 that receive the updated parameters rounded to nearest even (the bf16 mode's working copy of
 * the fp32 master weights, read by the Linears' io_bf16 bit 2). */
/* table: device array of {const float* src; float* dst; long long n;} (24-byte records), one workgroup each */
int cswin_multi_copy(const void* table, int nchunks, void* stream);

/* ---- the chunk table of the six entry points below (the `chunks`, `nchunks` and `first_chunk` arguments of the AdamW and TPGM
 * sections) ----
 * chunks: device table of nchunks 16-byte records {long long off; int n; int tensor;}, 8-B aligned, one 256-thread workgroup each:
 * elements [off, off + n) of the flat buffers belong to tensor `tensor`, n <= 16384, off % 4 == 0, no chunk crosses a tensor or
 * covers a pad word, chunks of one tensor are consecutive; first_chunk[ntensors + 1] indexes them per tensor.  The table is the
 * caller's (optim.chunk_table builds it): the library cannot read it, so its bounds are the caller's responsibility.
 * No float atomics: every sum has a fixed order (within a chunk, then chunks in chunk order, then tensors in tensor order) and two
 * runs on the same input give the same bits. */

/* ---- optimiser: clip_grad_norm_(parameters, max_norm) + torch.optim.AdamW (universal_train.py:693-725, 934-939), with a learning
 * rate per parameter tensor (the "surgical" mode, :635-690, 871-896), on the flat buffers and the chunk table above ----
 *
 * partial[c] = (sum g^2, sum p^2) over chunk c (2 * nchunks floats); p == NULL: the second entries are not written. */
int cswin_chunk_sumsq(const float* g, const float* p, const void* chunks, int nchunks, float* partial, void* stream);
/* One workgroup: tensor_sumsq[t] = (sum g^2, sum p^2) of tensor t, its chunk partials added in chunk order (the second column is
 * whatever partial's holds); scalars = [total_norm, clip_coef] with total_norm = grad_scale * sqrt(sum_t sum g^2), the tensors
 * added in tensor order, and clip_coef = min(1, max_norm / (total_norm + 1e-6)), clip_grad_norm_'s rule.  Any ntensors >= 1. */
int cswin_norm_finalize(const float* partial, const int* first_chunk, int ntensors, float grad_scale, float max_norm,
                        float* tensor_sumsq, float* scalars, void* stream);
/* Per element of tensor t, in torch.optim.AdamW's order:
 *   g' = g * grad_scale * clip_coef (scalars[1]; 1 when scalars == NULL);  m = b1 m + (1 - b1) g';  v = b2 v + (1 - b2) g'^2;
 *   lr_t = lr_dev[0] * (lr_mult ? lr_mult[t] : 1);  p = p (1 - lr_t wd) - (lr_t / bc1) m / (sqrt(v) / sqrt(bc2) + eps);
 *   shadow = bf16_rne(p) when given (as cswin_sgd_flat's).
 * bc1 = 1 - beta1^t, bc2 = 1 - beta2^t come from the host (the step count never enters the device).  A tensor with lr_mult[t] == 0
 * exactly keeps p and its shadow bit for bit (the stores are skipped); its m and v move, as torch's do in an lr = 0 group.
 * Non-finite gradients are reported, not repaired: one +inf makes the norm inf and clip_coef 0, that element's g' NaN and every
 * other g' 0, as in torch.  p, g, m, v 16-B aligned, the shadow 8-B. */
int cswin_adamw_flat(float* p, const float* g, float* m, float* v, const void* chunks, int nchunks, const float* lr_dev,
                     const float* lr_mult, const float* scalars, double beta1, double beta2, double eps, float weight_decay,
                     float grad_scale, double bc1, double bc2, void* shadow_bf16, void* stream);

/* ---- per-step rates of the surgical fine-tuning loop (finetune.py:116-144, 223-239): every parameter group's learning rate is
 * lr * n_k / max_j n_j of this step's gradient, and the step is torch.optim.Adam(weight_decay) ----
 *
 * One workgroup, in place of cswin_norm_finalize: tensor_sumsq and scalars come out bit for bit as that entry point writes them, and then
 * over the static group table (group k's tensors are group_tensors[group_first[k] .. group_first[k + 1] - 1], in tensor order, not
 * necessarily contiguous; group_of[t] is tensor t's group, or -1; the table is the caller's, optim.group_table builds and checks it):
 *   sums of group k = its tensors' (sum g^2, sum p^2) added in the table's order;
 *   statistic 0: group_stat[k] = grad_scale * sqrt(sum g^2), the norm of the group's concatenated gradient (finetune.py:135-140);
 *   statistic 1: that divided by sqrt(sum p^2) where sqrt(sum p^2) > 1e-8, else 0 (universal_train.py:661-690); cswin_chunk_sumsq must
 *     have been given the parameters;
 *   top = the maximum of group_stat in group order; lr_mult[t] = group_stat[group_of[t]] / top, default_mult where group_of[t] == -1.
 * top <= 0 makes every grouped multiplier 0.  A NaN statistic makes top NaN and with it every grouped multiplier: reported, not
 * repaired.  No float atomics, every sum in a fixed order.  Any ntensors >= 1 and ngroups >= 1. */
int cswin_rate_finalize(const float* partial, const int* first_chunk, int ntensors, float grad_scale, float max_norm,
                        const int* group_first, const int* group_tensors, const int* group_of, int ngroups, int statistic,
                        float default_mult, float* tensor_sumsq, float* scalars, float* group_stat, float* lr_mult, void* stream);
/* cswin_adamw_flat with flags; flags == 0 is cswin_adamw_flat itself, bit for bit.
 *   bit 0, coupled L2 decay (torch.optim.Adam's grad.add(param, alpha=wd)): g' = (grad_scale * clip_coef) g + wd p, the moments and
 *     the quotient as above, p -= (lr_t / bc1) m / (sqrt(v) / sqrt(bc2) + eps); there is no decay factor.
 *   bit 1, fresh moments (an optimiser built anew for every step, finetune.py:237): m and v are taken as 0, neither read nor
 *     written, and may be NULL; the caller passes bc1 = 1 - beta1, bc2 = 1 - beta2.  12 bytes move per element instead of 28.
 * The frozen rule (lr_mult[t] == 0: p and its shadow are not stored), the shadow and the alignment are cswin_adamw_flat's. */
int cswin_adam_flat(float* p, const float* g, float* m, float* v, const void* chunks, int nchunks, const float* lr_dev,
                    const float* lr_mult, const float* scalars, double beta1, double beta2, double eps, float weight_decay,
                    float grad_scale, double bc1, double bc2, int flags, void* shadow_bf16, void* stream);

/* ---- TPGM, the trainable projection of the continual-learning loop (universal_train.py:391-615; the gradient of the radii is
 * tpgm.py:47-56's), on the flat buffers and the chunk table above.  Per tensor t, with d = p - anchor:
 *   norm_t = sqrt(sum d^2) (l1 == 0) or sum |d| (l1 != 0);  cmax_t = max(8 norm_t, 80), head tensors max(10 norm_t, 100);
 *   ratio_t = hardtanh(clamp(gamma_t, 1e-2, cmax_t) / (norm_t + 1e-8), 0, 1);  projected = anchor + ratio_t d.
 * No host synchronisation.
 *
 * partial[c] = (sum d^2 or sum |d|, sum g d) over chunk c (2 * nchunks floats); g == NULL: the second entries are not written.
 * p, anchor, g 16-B aligned. */
int cswin_tpgm_chunk_stats(const float* p, const float* anchor, const float* g, const void* chunks, int nchunks, int l1,
                           float* partial, void* stream);
/* One workgroup.  flags[t]: bit 0 = excluded (ratio exactly 1, gamma never moves), bit 1 = head tensor.  norm[t] is written in
 * both modes.
 * mode 0 (ratios): ratio[t] from the current gamma; gm, gv, scalars and the four doubles are not used.
 * mode 1 (update): dgamma_t = grad_scale * (sum g d) / (norm_t + 1e-8) where 1e-2 <= gamma_t <= cmax_t and the unclamped ratio lies
 *   strictly inside (0, 1), else 0; clip = min(1, 1 / (sqrt(sum_t dgamma_t^2) + 1e-6)), the tensors added in tensor order; one
 *   torch.optim.Adam step (betas 0.9 / 0.999, eps 1e-8, no decay, lr = proj_lr, bc1 = 1 - 0.9^step and bc2 = 1 - 0.999^step from the
 *   host) on every gamma that is not excluded, a zero gradient included; ratio[t] from the new gamma; scalars = [norm of dgamma, clip]. */
int cswin_tpgm_finalize(const float* partial, const int* first_chunk, int ntensors, int l1, const int* flags, float* gamma,
                        float* gm, float* gv, double grad_scale, double proj_lr, double bc1, double bc2, int mode, float* ratio,
                        float* norm, float* scalars, void* stream);
/* dst = anchor + ratio[t] (src - anchor) and shadow = bf16_rne(dst) when given.  A tensor whose ratio is exactly 1 comes out with
 * src's bits: copied when src != dst, not stored at all (nor its shadow) when src == dst.  src, anchor, dst 16-B aligned, the
 * shadow 8-B; src == dst is the only overlap allowed. */
int cswin_tpgm_project(const float* src, const float* anchor, float* dst, const float* ratio, const void* chunks, int nchunks,
                       void* shadow_bf16, void* stream);

/* ---- EWC / MAS / L2-SP: a quadratic penalty that holds every weight near its old-task value (the anchor) in proportion to an
 * importance F >= 0, on the flat buffers and the chunk table above.  With d = p - anchor, a weight w_t per tensor (0: excluded)
 * and the strength lambda:  penalty = (lambda / 2) sum_t w_t sum_i F_i d_i^2,  dpenalty/dp_i = lambda w_t F_i d_i.
 * No host synchronisation, no float atomic; every buffer 16-B aligned; a refused call touches nothing.
 *
 * The estimation pass: x = (float)grad_scale * g;  imp += x * x (statistic 0, the empirical Fisher) or imp += |x| (statistic 1, MAS). */
int cswin_importance_accumulate(const float* g, float* imp, const void* chunks, int nchunks, double grad_scale, int statistic,
                                void* stream);
/* dst = a dst + b src over the chunks; src == NULL: dst = a dst.  The 1 / n normalisation and the online decay of the importance. */
int cswin_flat_axpby(float* dst, const float* src, const void* chunks, int nchunks, double a, double b, void* stream);
/* Per element t = imp * d (t = d when imp == NULL: importance 1) and g = fma(c, t, g) with c = lam[0] * tensor_weight[tensor] *
 * penalty_scale; lam is ONE float in device memory, tensor_weight one float per tensor.  partial[c] = (sum t d, sum d^2) over
 * chunk c (2 * nchunks floats).  A chunk whose c is exactly 0 stores nothing to g (its bits stay, a -0.0 included); g == NULL: the
 * sums alone.  penalty_scale is 1 / grad_scale of the optimiser launch that follows. */
int cswin_consolidate_chunks(const float* p, const float* anchor, const float* imp, float* g, const void* chunks, int nchunks,
                             const float* lam, const float* tensor_weight, double penalty_scale, float* partial, void* stream);
/* One workgroup.  per_tensor[t] = (sum F d^2, sum d^2), the chunk partials in chunk order;  with W = sum_t w_t per_tensor[t][0] in
 * tensor order:  scalars = [(lam[0] / 2) W, W, sqrt(sum_t per_tensor[t][1])]. */
int cswin_consolidate_finalize(const float* partial, const int* first_chunk, int ntensors, const float* lam,
                               const float* tensor_weight, float* per_tensor, float* scalars, void* stream);

/* ---- the "eb-criterion" statistic of the surgical mode (universal_train.py:669-672) per parameter tensor of the flat gradient
 * buffer: evidence[t] = mean(g * g / (var(g, dim 0, unbiased) + 1e-8)), one variance per column (an index of the dimensions after
 * the first, flattened: inner = numel / shape[0] columns of d0 = shape[0] rows) ----
 *
 * tiles: ntiles 32-byte records {int64 off; int32 d0, inner, col0, ncols, tensor, width} in DEVICE memory, 8-B aligned, built and
 * checked by optim.column_tiles (its only producer: col0 + ncols <= inner, 1 <= ncols <= width, width a power of two <= 64, the
 * d0 * inner elements at `off` inside one tensor's slot).  One workgroup per record reads all d0 rows of its ncols columns of g
 * (16-B aligned) and writes partial[tile] = sum_j (sum_i g_ij^2) / (var_j + 1e-8f), var_j by a shifted one-pass form (the shift is
 * the column's first row), every sum in a fixed order.  d0 == 1 gives var = 0 / 0 = NaN, as torch.var does, and stores it. */
int cswin_eb_tiles(const float* g, const void* tiles, int ntiles, float* partial, void* stream);
/* One workgroup: evidence[t] = (partial[first_tile[t]] + ... + partial[first_tile[t + 1] - 1], in tile order) / numel[t].
 * first_tile: ntensors + 1 ints, numel: ntensors ints, both in device memory.  Any ntensors >= 1. */
int cswin_eb_finalize(const float* partial, const int* first_tile, const int* numel, int ntensors, float* evidence, void* stream);

/* ---- nn.Dropout(p) of the reference (cswin_unet.py:20,25,27 Mlp.drop; :135 proj_drop; :346 pos_drop), fused with the residual
 * add + DropPath row factor that follows it where there is one (:178-179):
 *   keep(i) = counter-based hash of (seed, i) >= p   (no mask tensor: backward regenerates it from the same seed)
 *   forward : y[i]  = (residual ? residual[i] : 0) + row_scale[i / (rows_per_sample * C)] * keep(i) / (1 - p) * x[i]
 *   backward: dx[i] =                               row_scale[...]                          * keep(i) / (1 - p) * dy[i]
 * x / y / dy / dx: n floats, 16-B aligned; row_scale: per-sample floats or NULL; elems_per_sample = L * C.  In place (y == x) is
 * allowed.  The random stream is this library's own: torch's Philox stream cannot be reproduced (parity unpinned, as for
 * DropPath); tests extract the mask by running the kernel on ones. */
int cswin_dropout(const float* x, const float* residual, const float* row_scale, float* y, long n, long elems_per_sample,
                  float p, unsigned long long seed, const unsigned long long* seed_epoch, void* stream);
/* seed_epoch: as drop_epoch of cswin_attn_fwd (device counter added to the seed; NULL: none). */
/* bf16 gradient wire for the data-parallel all-reduce (replaces DataParallel's fp32 reduce_add, trainer.py:37-38):
   fp32 -> bf16 round-to-nearest-even / bf16 -> fp32 over n elements (src of pack, dst of unpack 16-B aligned) */
int cswin_pack_bf16(const float* src, void* dst_bf16, long n, void* stream);
/* dst = bf16(scale * src): the trainer packs gradient buckets pre-divided by the world size, so the collective's bf16 sum IS the
   mean (eight ranks' sum would otherwise spend three of bf16's eight mantissa bits on the factor 8 it is divided by afterwards) */
int cswin_pack_bf16_scaled(const float* src, void* dst_bf16, long n, float scale, void* stream);
int cswin_unpack_bf16(const void* src_bf16, float* dst, long n, void* stream);

/* ---- evaluation: per-class Dice / HD95 ingredients of a label volume (utils.py:48-58; medpy.metric.binary dc / hd95,
 *      connectivity 1, unit voxel spacing) ----
 * pred, label: dense (D, H, W) class ids, every id < ncls, 2 <= ncls <= 255; each of D, H, W in 1..2048 (3 * 2047^2 stays
 * inside int32).  ndim = 3: the six face neighbours decide what a border voxel is; ndim = 2 requires D == 1 and uses the four
 * in-plane neighbours (a (1, H, W) volume with ndim = 3 is legal: there every set voxel is a border voxel, as scipy's
 * binary_erosion(border_value=0) has it).
 * counts[ncls][4] (64-bit) = {|P_c|, |G_c|, |P_c n G_c|, |dP_c| + |dG_c|};  hist[ncls][nbins] (32-bit unsigned), nbins =
 * cswin_seg_metrics_nbins(D, H, W) = (D-1)^2 + (H-1)^2 + (W-1)^2 + 1: hist[c][s] = border voxels of P_c whose nearest border
 * voxel of G_c lies at squared distance s, plus the same with P and G exchanged.  Both are zeroed by the call; rows of classes
 * with an empty side, and row 0 (background), stay zero.  Squared distances are exact integers (true Euclidean minimum) and only
 * integer atomics are used: the result is bit-reproducible.  hd95_c = 95th percentile of the multiset with hist[c][s] copies of
 * sqrt(s); dice_c = 2 counts[c][2] / (counts[c][0] + counts[c][1]).
 * The size queries are host-only and return 0 with a message for an unsupported shape. */
int    cswin_seg_metrics_nbins(int D, int H, int W);
size_t cswin_seg_metrics_workspace(int D, int H, int W, int ndim, int ncls);
int    cswin_seg_metrics(const unsigned char* pred, const unsigned char* label, long long* counts, unsigned int* hist,
                         void* workspace, size_t ws_bytes, int D, int H, int W, int ndim, int ncls, void* stream);

/* ---- evaluation: surface distances under a voxel spacing, for HD95 and ASSD in physical units (csrc/metrics.hip;
 *      medpy.metric.binary hd95 / assd with voxelspacing, connectivity 1) ----
 * Same volumes, shape rules and counts[ncls][4] as cswin_seg_metrics.  (sz, sy, sx) > 0, finite: the spacing along D, H, W
 * (scipy's `sampling` in array order); sz is ignored for ndim = 2.  The distance of a border voxel of one volume is the minimum
 * over the border voxels of the other of (dz sz)^2 + (dy sy)^2 + (dx sx)^2 in float64, the expression
 * scipy.ndimage.distance_transform_edt(sampling=...) evaluates: exact whenever the products and sums are representable (dyadic
 * spacings), otherwise within an ulp or two of it (a separable minimisation may pick a candidate that is an ulp worse).
 * nq[ncls][2] (64-bit): nq[c][0] = |dP_c|, nq[c][1] = |dG_c| for a class c >= 1 with voxels on both sides, else 0.
 * dist2[cap] (float64): squared distances in segments ordered class 1 P->G, class 1 G->P, class 2 P->G, ...; segment (c, dir)
 * starts at the exclusive prefix sum of nq and holds nq[c][dir] values in no particular order (sort it: its multiset is the same
 * on every run).  A value whose slot would be >= cap is dropped and nothing is written outside dist2[0 .. cap): the caller sees
 * an overflow as sum(nq) > cap and calls again with that capacity.  counts and nq are zeroed by the call; dist2 beyond sum(nq)
 * is left as it was.  Integer atomics only, no host synchronisation.
 * Errors: CSWIN_ERR_SHAPE for a bad shape, spacing, null pointer or cap < 0; CSWIN_ERR_WORKSPACE for a short workspace;
 * CSWIN_ERR_ALIGN for a workspace off 16 B or counts / nq / dist2 off 8 B. */
size_t cswin_surface_dist_workspace(int D, int H, int W, int ndim, int ncls);
int    cswin_surface_dist(const unsigned char* pred, const unsigned char* label, long long* counts, long long* nq, double* dist2,
                          long cap, void* workspace, size_t ws_bytes, int D, int H, int W, int ndim, int ncls, double sz, double sy,
                          double sx, void* stream);

/* ---- evaluation: connected components of a predicted label volume and the per-class size filter (csrc/components.hip) ----
 * vol: dense (D, H, W) uint8 class ids, N = D H W; ids 0 and >= ncls are background.  A component is a maximal set of voxels of
 * one foreground id joined by face neighbours (scipy.ndimage.label(vol == c), default structure, for every c; a 2-D slice is
 * D = 1).  labels[v] = 0 for background, else 1 + the smallest flat index of v's component; sizes[r] = voxel count of the
 * component whose smallest flat index is r, 0 at every other index.  Both are N int32 written in full; sizes may be NULL for the
 * label call.  Union-find with integer atomics only: the result does not depend on scheduling and is bit-reproducible.
 * cswin_components_filter(labels, sizes of the same vol): per class c in 1..ncls-1, thr_c = max(min_size[c],
 * ceil(min_fraction[c] * (double)largest_c)) in float64 on the device, largest_c = the biggest component of class c; out[v] = 0
 * where v's component is smaller than thr_c, vol[v] elsewhere (background and ids >= ncls pass through).  min_size (int64 >= 0),
 * min_fraction (float64 in [0, 1]): device tables of ncls entries, entry 0 ignored; (0, 0.0) leaves a class untouched,
 * min_fraction = 1 keeps the largest component and every other of the same size.  out == vol is allowed, any other overlap of
 * out or the workspace with an argument is CSWIN_ERR_UNSUPPORTED.
 * Both calls take a workspace of cswin_components_workspace(D, H, W) bytes (host-only; 0 with a message for an unsupported
 * shape), 16-B aligned; the other pointers need their element's alignment only.  Each of D, H, W in 1..2048 (CSWIN_ERR_SHAPE),
 * N <= 2^31 - 2 and ncls in 2..255 (CSWIN_ERR_UNSUPPORTED), a short workspace is CSWIN_ERR_WORKSPACE: all checked before any
 * launch.  No host synchronisation, no allocation; every launch goes to `stream` and can be captured into a graph. */
size_t cswin_components_workspace(int D, int H, int W);
int    cswin_components_label(const unsigned char* vol, int* labels, int* sizes, void* workspace, size_t ws_bytes, int D, int H,
                              int W, int ncls, void* stream);
int    cswin_components_filter(const unsigned char* vol, const int* labels, const int* sizes, const long long* min_size,
                               const double* min_fraction, unsigned char* out, void* workspace, size_t ws_bytes, int D, int H,
                               int W, int ncls, void* stream);

/* ---- evaluation: the two resizes around the network (utils.py:70-81: scipy.ndimage.zoom(order=3) of each slice to the network's
 *      input size, argmax and scipy.ndimage.zoom(order=0) back) ----
 * zoom of a 2-D slice is the separable linear map R_h x R_w^T; the caller takes each 1-D operator R (n_out x n_in) from scipy
 * itself (zoom of the unit vectors; cswin_unet_amd.utils.zoom_operator) and passes it as a band: row i of R_h is
 * wh[i][0..Th) at columns sh[i] .. sh[i] + Th (0 <= sh[i], sh[i] + Th <= H; Th <= H), the same for ww / sw / Tw along W.
 * x (D, H, W) float32 (x_f64 = 0) or float64 (x_f64 = 1) -> y (D, h, w) float32 = float32(R_h x[d] R_w^T): every product and sum
 * in float64 (ascending input index), one rounding at the store.  wh (h, Th), ww (w, Tw) float64; sh (h), sw (w) int32; each of
 * D, H, W, h, w in 1..2048.  No alignment beyond the element size and no workspace; starts are clamped into range on the device. */
int cswin_resize_banded(const void* x, float* y, const double* wh, const int* sh, int Th, const double* ww, const int* sw, int Tw,
                        int D, int H, int W, int h, int w, int x_f64, void* stream);
/* logits (B, ncls, h, w) fp32 -> out (B, H, W) uint8: out[b][i][j] = argmax_c logits[b][c][src_row[i]][src_col[j]] with
 * torch.argmax's rules (the first index wins a tie, a NaN beats every number).  src_row (H), src_col (W) int32: the source index
 * of every output row / column, as scipy's order-0 zoom picks it (cswin_unet_amd.utils.nearest_index); 0..H-1 / 0..W-1 themselves
 * when nothing is resized.  A negative index marks an output that scipy fills with its constant instead of gathering (the last
 * output of 512 -> 224): out is 0 there.  Indices past the end are clamped on the device.  ncls in 1..255; each of B, h, w, H, W in 1..2048. */
int cswin_argmax_zoom_back(const float* logits, unsigned char* out, const int* src_row, const int* src_col, int B, int ncls, int h,
                           int w, int H, int W, void* stream);
/* cswin_argmax_zoom_back over a list of classes: out[b][i][j] = the POSITION k < nsel of the largest of
 * logits[b][classes[k]][src_row[i]][src_col[j]], i.e. torch.argmax(logits[:, classes], 1) before the zoom -- how a continual model
 * with ncls outputs is scored on one dataset's own classes (universal_test.py:50-54).  The first k in list order wins a tie, a NaN
 * beats every number and the first NaN wins; a negative source index writes 0.  classes: device int32 [nsel], entries clamped into
 * [0, ncls) on the device; the list may be unordered and may repeat a class (the earlier position wins).  nsel in 1..255 (the
 * output byte), ncls >= 1; every other limit is cswin_argmax_zoom_back's. */
int cswin_argmax_zoom_back_classes(const float* logits, unsigned char* out, const int* src_row, const int* src_col,
                                   const int* classes, int nsel, int B, int ncls, int h, int w, int H, int W, void* stream);

/* ---- label statistics of a continual-learning stage (universal_train.py:1006-1015 class pixel counts, :204-211 the slices that
 * hold a class): per-slice class histogram in one streaming pass.
 * labels: N slices of slice_elems class ids, uint8 (label_bytes = 1) or int64 (8), densely packed.  counts: int64 [N][ncls + 1],
 * written in full (no memset, no workspace, no global atomics, bit-reproducible): column c < ncls = the elements of slice n with
 * class c, column ncls = the elements without a class, so every row sums to slice_elems.  The class of a raw id r is r itself
 * (label_map NULL, nmap 0) or label_map[r] for 0 <= r < nmap (device int32; the table of continual.new_label_map, the convention
 * of cswin_cl_loss_sums); an id outside the map, or a class outside [0, ncls), has no class.
 * ncls in 1..256, N >= 1, slice_elems in 1..2^31-1; another label_bytes is CSWIN_ERR_UNSUPPORTED; pointers aligned to their
 * element size. */
int cswin_class_counts(const void* labels, int label_bytes, const int* label_map, int nmap, long long* counts, int N,
                       long long slice_elems, int ncls, void* stream);

/* ---- Gaussian blur of a batch of slices (csrc/blur.hip): scipy.ndimage.gaussian_filter(x[d], sigma), mode "reflect" ----
 * x (D, H, W) float32 -> y (D, H, W) float32.  taps[0 .. radius] float64 = w[-radius] .. w[0], one half of scipy's symmetric
 * kernel with the centre last (cswin_unet_amd.utils.gaussian_taps).  Axis 0 is filtered first and rounded to float32, then
 * axis 1 and rounded again; every product and sum in float64 in correlate1d's folded order, acc = x[i] w[0], then
 * acc += (x[i - k] + x[i + k]) w[-k] for k = radius .. 1, multiply and add rounded separately.  The reflected indices are
 * computed on the device from H and W alone, so the radius may exceed either.  One launch, no workspace, no allocation, no
 * synchronisation.  Each of D, H, W in 1..2048 (CSWIN_ERR_SHAPE), radius in 0..32 and x != y (CSWIN_ERR_UNSUPPORTED: the filter
 * does not work in place); pointers aligned to their element size. */
int cswin_gaussian_blur(const float* x, float* y, const double* taps, int radius, int D, int H, int W, void* stream);
/* The same filter with a radius and taps of its own for every slice, in one launch.  table (D pairs of int32, device): slice d has
 * radius table[2d + 1] in 0..max_radius and the taps taps[table[2d] .. table[2d] + radius] (w[-radius] .. w[0] as above) of the
 * ntaps float64 behind `taps` (device; max_radius < ntaps <= 2048 * 33).  Radius 0 with the single tap 1.0 copies the slice (the
 * sums above then are x[i] * 1.0).  The tile plan is that of max_radius; a radius or an offset outside what max_radius and ntaps
 * allow is clamped on the device.  Slice d equals cswin_gaussian_blur of that slice with its taps, bit for bit.  Limits,
 * alignment and error codes as above. */
int cswin_gaussian_blur_each(const float* x, float* y, const double* taps, int ntaps, const int* table, int max_radius, int D, int H,
                             int W, void* stream);

/* ---- intensity augmentation of a batch of images (csrc/intensity.hip): stages 2-5 of cswin_unet_amd.utils.intensity_host ----
 * One 48-byte record per sample in a device table (8-B aligned).  flags: 1 noise, 2 brightness, 4 contrast, 8 gamma, 16 the gamma
 * stage works on -z (read only with 8); other bits are ignored.  With z the float64 of the sample's float32 pixels, i the row-major
 * pixel index within the sample:
 *   noise       z[i] += noise_std * sqrt(-2 ln u1) cos(2 pi u2),  r = mix64(mix64(seed) ^ i) (splitmix64's step, increment
 *               included),  u1 = ((r >> 40) + 1) / 2^24,  u2 = ((r >> 16) & 0xFFFFFF) / 2^24
 *   brightness  z *= brightness
 *   contrast    m, lo, hi = mean, min, max of z;  z = min(max((z - m) * contrast + m, lo), hi)
 *   gamma       m0, s0 = mean, population standard deviation;  lo = min, rng = max - lo;
 *               z = ((z - lo) / (rng + 1e-7)) ** gamma * rng + lo;  z = (z - mean(z)) / (std(z) + 1e-8) * s0 + m0
 * in this order, each only if its flag is set, all in float64 with separately rounded products and sums, y = float32(z).  The
 * whole-image sums are formed in a fixed order: a sample's result is the same on every run and whatever else the batch holds.
 * stages: the OR of the samples' contrast (4) and gamma (8) flags, which decides the launches (1 + 1 + 3 at most); a flag
 * that `stages` lacks is off for every sample.  workspace: cswin_intensity_workspace(B, slice_elems) bytes, 8-B aligned, needed
 * only where stages != 0.  x == y is allowed.  B in 1..2048, slice_elems in 1..2048 * 2048 (CSWIN_ERR_SHAPE); the parameters are
 * the caller's to check (gamma > 0, finite values).  No allocation, no synchronisation, no atomics. */
typedef struct cswin_intensity_desc {
    long long flags;
    unsigned long long seed;
    double noise_std, brightness, contrast, gamma;
} cswin_intensity_desc;
size_t cswin_intensity_workspace(int B, long slice_elems);
int cswin_intensity_batch(const float* x, float* y, const void* table, void* workspace, size_t ws_bytes, int B, long slice_elems,
                          int stages, void* stream);

/* ---- test-time augmentation of a volume evaluation (csrc/tta.hip): the eight symmetries of the square, which training's
 *      random_rot_flip draws from (datasets/dataset_synapse.py:12-19), applied before the network and ensembled after it ----
 * A view is a code c in 0..7: bit 0 transposes, bit 1 reverses the rows, bit 2 the columns, in that order
 *   (a = x.T if c & 1 else x; a = a[::-1, :] if c & 2 else a; a = a[:, ::-1] if c & 4 else a), so source pixel (r, s) of an (h, w)
 *   slice sits at (i, j) of the viewed frame (h', w') = (w, h) if c & 1 else (h, w):  (i2, j2) = (s, r) if c & 1 else (r, s),
 *   i = h'-1-i2 if c & 2 else i2,  j = w'-1-j2 if c & 4 else j2.  np.rot90(x, 1) is code 3, np.rot90(x, 3) code 5.
 * views: V codes in HOST memory (as the heads / idx of cswin_attn_fwd), V in 1..8, read before the call returns and passed to
 *   the kernel by value -- so a code outside 0..7, or a transposing code with h != w, is CSWIN_ERR_SHAPE before any launch.
 * x (B, h, w) fp32 -> y (V, B, h', w') fp32, y[v][b] = view_{views[v]}(x[b]): values are copied, never computed with.  x != y
 * (CSWIN_ERR_UNSUPPORTED); each of B, h, w in 1..2048.  One launch, no workspace. */
int cswin_view_batch(const float* x, float* y, const int* views, int V, int B, int h, int w, void* stream);
/* The ensemble of the network's answers to those views, the argmax and the order-0 zoom back in one launch.
 * logits (V, B, ncls, h', w') fp32, slice [v] in the frame of view views[v] -> out (B, H, W) uint8, and probs (B, nsel, h, w) fp32
 * or NULL.  With c_k = classes[k] (device int32 [nsel], clamped into [0, ncls) on the device, as cswin_argmax_zoom_back_classes
 * takes it) or c_k = k (classes NULL, and then nsel == ncls):
 *   P[b][k][r][s] = (1 / V) sum_v softmax_k(logits[v][b][c_.][i_v(r, s)][j_v(r, s)]),
 *   out[b][i][j]  = argmax_k P[b][k][src_row[i]][src_col[j]]  (the first k wins a tie, a NaN wins and the first NaN first),
 * the mean of the PROBABILITIES of the views.  All of it in float32, in one fixed order: per view in ascending v, m = max_k l_k,
 * e_k = expf(l_k - m), S = the sum of e_k in ascending k, p_k = e_k / S, added to the sum over views; then the multiplication by
 * 1 / V.  A +inf or NaN logit in any view makes every P of its pixel NaN (inf - inf), so out is 0 there, as torch.softmax and
 * torch.argmax give it.  src_row (H), src_col (W) int32, device: as cswin_argmax_zoom_back's (negative: out is 0; past the end:
 * clamped).  Every source pixel is ensembled once, by the workgroup that also writes every output pixel gathering from it.
 * probs, if given, receives P.  nsel <= 16 keeps the sums over views in registers; above that they are kept in probs, which is
 * then required (CSWIN_ERR_WORKSPACE if NULL).  nsel in 1..255, ncls >= 1, each of B, h, w, H, W in 1..2048, V and views as
 * above (CSWIN_ERR_SHAPE); pointers aligned to their element size.  No atomics: two runs give the same bits. */
int cswin_tta_argmax_zoom_back(const float* logits, unsigned char* out, float* probs, const int* src_row, const int* src_col,
                               const int* views, int V, const int* classes, int nsel, int B, int ncls, int h, int w, int H, int W,
                               void* stream);

/* ---- training augmentation of a batch of raw slices (datasets/dataset_synapse.py:12-47: np.rot90 + np.flip, or
 *      scipy.ndimage.rotate(order=0, reshape=False), then the zooms to the network's size) ----
 * One descriptor per sample, in a device table (24-byte records, 8-B aligned), as cswin_multi_copy takes its table.  The transform T
 * of a sample maps a pixel (i, j) of the transformed slice to a source pixel of slice `src`, or to none:
 *   kind 0: the identity.
 *   kind 1: np.flip(np.rot90(x, k), axis), k in 0..3, axis in 0..1; for odd k the transformed slice is (W, H).
 *   kind 2: map (H * W int32, device): the flat source index scipy.ndimage.rotate reads for every output pixel, negative where it
 *           writes its constant 0 (cswin_unet_amd.utils.rotation_index).  A NULL map gives all zeros.
 * src, the map's entries and every derived index are clamped into range on the device. */
typedef struct cswin_augment_desc {
    int kind, k, axis;
    int src;                 /* index of the source slice in the batch */
    const int* map;          /* kind 2 only */
} cswin_augment_desc;
/* x (B, H, W) float32 -> y (n, Ho, Wo) float32, y[s] = T_s(x[table[s].src]) with 0 where T_s has no source.  (Ho, Wo) is (H, W)
 * or (W, H): the caller lists in one call the samples whose transformed shape that is.  Values are copied, never computed with.
 * Each of n, B, H, W in 1..2048; no alignment beyond the element size, no workspace. */
int cswin_augment_gather(const float* x, float* y, const void* table, int n, int B, int H, int W, int Ho, int Wo, void* stream);
/* lab (B, H, W) uint8 -> out (n, h, w) int64: out[s][i][j] = lab[src_s][T_s(row[i], col[j])], the order-0 zoom of the transformed
 * label without ever forming it.  (row, col) = (src_row (h), src_col (w)): scipy's source indices (utils.nearest_index) from the
 * transformed shape (H, W); for a sample that kind 1 with odd k transposes, (src_row_t (h), src_col_t (w)): those from (W, H).
 * out is 0 where a row or column index is negative or T_s has no source.  Each of n, B, H, W, h, w in 1..2048. */
int cswin_augment_labels(const unsigned char* lab, long long* out, const void* table, const int* src_row, const int* src_col,
                         const int* src_row_t, const int* src_col_t, int n, int B, int H, int W, int h, int w, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CSWIN_HIP_H */
