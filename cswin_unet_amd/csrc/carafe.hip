// CARAFE content-aware reassembly (networks/cswin_unet.py:222-319) in its closed form:
//
//   Wt[b,hw,k,s] = softmax_k e[b,hw,k*S^2+s]
//   out[b, (hS+sy)(SW) + (wS+sx), c] = bias[c] + sum_k Wt[b,hw,k,s] * z[b, nbr_k(h,w), c]      (zero outside the map)
//
// where z = x @ W_out^T is the `out` 1x1 convolution applied BEFORE the reassembly, at LOW
// resolution: the 1x1 conv is linear and the reassembly weights sum over pixels only, so the two
// commute exactly (S^2 x fewer GEMM FLOPs, and the (B,C,SH,SW) tensor of the reference never exists).
// pixel_shuffle / unfold / pad / permute of the reference all collapse into index arithmetic here.
// Everything is on the (B, L, C) token layout.  HBM-bound: one pass over e and z (z neighbours
// come from L1/L2), one coalesced write of out.
#include "common.h"
#include "carafe_plan.h"
#include <stdlib.h>
#include <type_traits>

namespace {

// ---- the steps the kernels share ----
struct Pixel { int b, h, w; };

// low-resolution pixel pix = (b * H + h) * W + w
__device__ __forceinline__ Pixel decode_pixel(long pix, int H, int W) {
    return {(int)(pix / ((long)W * H)), (int)((pix / W) % H), (int)(pix % W)};
}

// row of sub-pixel (sy, sx) of pixel p in the (B, (S*H)*(S*W), Cz) token tensors
template <int S>
__device__ __forceinline__ long hires_row(Pixel p, int sy, int sx, int H, int W) {
    return ((long)p.b * H * S + p.h * S + sy) * (W * S) + p.w * S + sx;
}

// Tap k of the 3 x 3 stencil round (h, w), and whether it lies inside the map.  mirrored: the pixel whose k-th tap (h, w) is.
struct Tap { int h, w; bool inside; };
__device__ __forceinline__ Tap tap_of(int k, int h, int w, int H, int W, bool mirrored = false) {
    const int dh = k / 3 - 1, dw = k % 3 - 1;
    const int hh = mirrored ? h - dh : h + dh, ww = mirrored ? w - dw : w + dw;
    return {hh, ww, (unsigned)hh < (unsigned)H && (unsigned)ww < (unsigned)W};
}

// wt[k] = softmax over the nine taps of e[pix][k * S2 + s]
template <int S2>
__device__ __forceinline__ void softmax_taps(const float* __restrict__ e, long pix, int s, float (&wt)[9]) {
    float mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        wt[k] = e[pix * (9 * S2) + k * S2 + s];
        mx = fmaxf(mx, wt[k]);
    }
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        wt[k] = __expf(wt[k] - mx);
        sum += wt[k];
    }
    const float inv = 1.0f / sum;
#pragma unroll
    for (int k = 0; k < 9; ++k) wt[k] *= inv;
}

// bias[c..c+3] + sum_k wt[k] * z[tap k of p][c..c+3], taps outside the map read as zero
__device__ __forceinline__ f32x4 gather_taps(const float* __restrict__ z, const float* __restrict__ bias, const float (&wt)[9],
                                             Pixel p, int H, int W, int Cz, int c) {
    f32x4 acc = bias ? *reinterpret_cast<const f32x4*>(bias + c) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const Tap t = tap_of(k, p.h, p.w, H, W);
        if (t.inside) acc += wt[k] * *reinterpret_cast<const f32x4*>(z + (((long)p.b * H + t.h) * W + t.w) * Cz + c);
    }
    return acc;
}

// one group of lpr lanes handles one (low-res pixel, sub-pixel s); the lanes stride over the 16-B chunks of its Cz channels
template <int S>
__global__ __launch_bounds__(cp::THREADS) void carafe_fwd_kernel(const float* __restrict__ e, const float* __restrict__ z,
                                                                  const float* __restrict__ bias, float* __restrict__ out,
                                                                  float* __restrict__ wt_save, int B, int H, int W, int Cz) {
    constexpr int S2 = S * S;
    const int lpr = cp::lpr(Cz);                      // lanes per item
    const int groups = cp::THREADS / lpr;
    const int sub = threadIdx.x % lpr, grp = threadIdx.x / lpr;
    const long items = (long)B * H * W * S2;
    for (long it = (long)blockIdx.x * groups + grp; it < items; it += (long)gridDim.x * groups) {
        const int s = (int)(it % S2);
        const long pix = it / S2;
        const Pixel p = decode_pixel(pix, H, W);
        float wt[9];
        softmax_taps<S2>(e, pix, s, wt);
        if (wt_save && sub == 0) {
#pragma unroll
            for (int k = 0; k < 9; ++k) wt_save[pix * (9 * S2) + k * S2 + s] = wt[k];
        }
        const int sy = s / S, sx = s - sy * S;
        const long orow = hires_row<S>(p, sy, sx, H, W);
        for (int c = 4 * sub; c < Cz; c += 4 * lpr)
            *reinterpret_cast<f32x4*>(out + orow * Cz + c) = gather_taps(z, bias, wt, p, H, W, Cz, c);
    }
}

// The same reassembly written STRAIGHT to (B, C, S*H, S*W) planes, first C of the Cz channels (the segmentation head: C classes in
// 16-channel tokens).  One lane per OUTPUT pixel; a workgroup covers 256 / S^2 consecutive low-resolution pixels and all their
// sub-pixels with sx fastest, so a wave's stores are contiguous runs of one output row in every class plane, and the padded
// (B, (S*H)*(S*W), Cz) token tensor with the transposing pass after it never exists.  The weights and the sums are those of
// carafe_fwd_kernel, by the same two functions (bit-identical results).
template <int S>
__global__ __launch_bounds__(cp::THREADS) void carafe_fwd_nchw_kernel(const float* __restrict__ e, const float* __restrict__ z,
                                                                       const float* __restrict__ bias, float* __restrict__ out,
                                                                       float* __restrict__ wt_save, int B, int H, int W, int Cz, int C) {
    constexpr int S2 = S * S, PPB = cp::ppb(S);
    const int sy = threadIdx.x / (PPB * S), rem = threadIdx.x % (PPB * S);
    const int pl = rem / S, sx = rem % S, s = sy * S + sx;
    const long npix = (long)B * H * W, plane = (long)H * S * W * S;
    for (long p0 = (long)blockIdx.x * PPB; p0 < npix; p0 += (long)gridDim.x * PPB) {
        const long pix = p0 + pl;
        if (pix >= npix) continue;
        const Pixel p = decode_pixel(pix, H, W);
        float wt[9];
        softmax_taps<S2>(e, pix, s, wt);
        if (wt_save) {
#pragma unroll
            for (int k = 0; k < 9; ++k) wt_save[pix * (9 * S2) + k * S2 + s] = wt[k];
        }
        float* o = out + (long)p.b * C * plane + ((long)p.h * S + sy) * (W * S) + p.w * S + sx;
        for (int c = 0; c < C; c += 4) {
            const f32x4 acc = gather_taps(z, bias, wt, p, H, W, Cz, c);
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (c + q < C) o[(c + q) * plane] = acc[q];
        }
    }
}

// de[b,hw,k*S2+s] = Wt[k] * (dWt[k] - sum_j Wt[j] dWt[j]),  dWt[k] = sum_c dout[pix(s), c] * z[nbr_k, c]
// dbias_part != NULL (the bias_in_e route of carafe_plan.h: at most cp::E_CHUNKS chunks per lane): the kernel streams over dout
// anyway, so it also leaves the per-workgroup column sums of dout in dbias_part[block][Cz] (dbias = their sum), which saves the
// separate column-sum pass over dout.
template <int S>
__global__ __launch_bounds__(cp::THREADS) void carafe_bwd_e_kernel(const float* __restrict__ dout, const float* __restrict__ z,
                                                                    const float* __restrict__ wt_save, float* __restrict__ de,
                                                                    float* __restrict__ dbias_part, int B, int H, int W, int Cz) {
    static_assert(cp::E_CHUNKS == 2, "bacc below has a first and a second chunk");
    __shared__ float bred[cp::e_stage_floats()];     // [chunk][group][4 * lpr]
    f32x4 bacc[cp::E_CHUNKS] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    constexpr int S2 = S * S;
    const int lpr = cp::lpr(Cz);
    const int groups = cp::THREADS / lpr;
    const int sub = threadIdx.x % lpr, grp = threadIdx.x / lpr;
    const long items = (long)B * H * W * S2;
    const long items_pad = (items + groups - 1) / groups * groups;     // keep whole groups alive for the shuffles
    for (long it0 = (long)blockIdx.x * groups + grp; it0 < items_pad; it0 += (long)gridDim.x * groups) {
        const bool live = it0 < items;
        const long it = live ? it0 : items - 1;
        const int s = (int)(it % S2);
        const long pix = it / S2;
        const Pixel p = decode_pixel(pix, H, W);
        const int sy = s / S, sx = s - sy * S;
        const long orow = hires_row<S>(p, sy, sx, H, W);
        float dwt[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) dwt[k] = 0.f;
        int ci = 0;
        for (int c = 4 * sub; c < Cz; c += 4 * lpr, ++ci) {
            const f32x4 g = *reinterpret_cast<const f32x4*>(dout + orow * Cz + c);
            if (live && dbias_part) {
                if (ci == 0) bacc[0] += g;
                else bacc[1] += g;
            }
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                const Tap t = tap_of(k, p.h, p.w, H, W);
                if (t.inside) {
                    const f32x4 zv = *reinterpret_cast<const f32x4*>(z + (((long)p.b * H + t.h) * W + t.w) * Cz + c);
                    dwt[k] += g[0] * zv[0] + g[1] * zv[1] + g[2] * zv[2] + g[3] * zv[3];
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 9; ++k)
            for (int o = lpr >> 1; o > 0; o >>= 1) dwt[k] += __shfl_xor(dwt[k], o, 64);
        if (sub == 0 && live) {
            float wt[9], dot = 0.f;
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                wt[k] = wt_save[pix * (9 * S2) + k * S2 + s];
                dot += wt[k] * dwt[k];
            }
#pragma unroll
            for (int k = 0; k < 9; ++k) de[pix * (9 * S2) + k * S2 + s] = wt[k] * (dwt[k] - dot);
        }
    }
    if (dbias_part) {                                 // column sums of this workgroup's rows of dout
        const int span = 4 * lpr;                     // channels covered by one chunk
#pragma unroll
        for (int q = 0; q < cp::E_CHUNKS; ++q)
#pragma unroll
            for (int e = 0; e < 4; ++e) bred[(q * groups + grp) * span + 4 * sub + e] = bacc[q][e];
        __syncthreads();
        for (int c = threadIdx.x; c < Cz; c += cp::THREADS) {
            const int q = c / span, cc = c - q * span;
            float t = 0.f;
            for (int g2 = 0; g2 < groups; ++g2) t += bred[(q * groups + g2) * span + cc];
            dbias_part[(long)blockIdx.x * Cz + c] = t;
        }
    }
}

// dz[b,n,c] = sum_k sum_s Wt[n - off_k][k][s] * dout[pix(n - off_k, s), c]
template <int S>
__global__ __launch_bounds__(cp::THREADS) void carafe_bwd_z_kernel(const float* __restrict__ dout,
                                                                    const float* __restrict__ wt_save, float* __restrict__ dz,
                                                                    int B, int H, int W, int Cz) {
    constexpr int S2 = S * S;
    const int lpr = cp::lpr(Cz);
    const int groups = cp::THREADS / lpr;
    const int sub = threadIdx.x % lpr, grp = threadIdx.x / lpr;
    const long items = (long)B * H * W;
    for (long pix = (long)blockIdx.x * groups + grp; pix < items; pix += (long)gridDim.x * groups) {
        const Pixel p = decode_pixel(pix, H, W);
        for (int c = 4 * sub; c < Cz; c += 4 * lpr) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                const Tap src = tap_of(k, p.h, p.w, H, W, true);       // the source pixel whose k-th neighbour is (h, w)
                if (src.inside) {
                    const Pixel p2 = {p.b, src.h, src.w};
                    const long pix2 = ((long)p.b * H + src.h) * W + src.w;
#pragma unroll
                    for (int s = 0; s < S2; ++s) {
                        const float wv = wt_save[pix2 * (9 * S2) + k * S2 + s];
                        acc += wv * *reinterpret_cast<const f32x4*>(dout + hires_row<S>(p2, s / S, s % S, H, W) * Cz + c);
                    }
                }
            }
            *reinterpret_cast<f32x4*>(dz + pix * Cz + c) = acc;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Fused backward for the model's last stage (CARAFE4 + fused head: S = 4, Cz = 16; 224 x 224 logits at B = 24 are 77 MB of
// dout).  The three generic kernels below read dout three times (de, dz, dbias) and gather it with 4-B / 16-B pieces; here
// one workgroup owns an 8 x 8 tile of low-resolution pixels and reads the 16 x 16 block D[p] = dout[4h..4h+3][4w..4w+3][0..15]
// of every pixel of the tile + a one-pixel halo exactly once per use, as 256-B row segments, and the per-pixel
// contractions run on the matrix pipes (v_mfma_f32_16x16x4_f32, exact fp32):
//   G[p]   (9 x 16) = Wt[p] (9 taps x 16 sub-pixels) . D[p] (16 sub-pixels x 16 channels)     -> LDS, tile + halo
//   dWt[p] (9 x 16) = Znbr[p] (9 taps x 16 channels) . D[p]^T                                   -> softmax backward -> de
//   dz[n][c] = sum_k G[n - off_k][k][c]   (9 LDS reads per output),   dbias[c] = sum_{p, s} D[p][s][c]
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ f32x4 carafe_mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// 4 x 4 transpose of (lane group kq = bits 4-5 of the lane) x (element of v) among the four lanes 16 apart
__device__ __forceinline__ f32x4 lane_transpose4(f32x4 v, int kq) {
    const bool hi = kq & 2, odd = kq & 1;
    float s0 = hi ? v[0] : v[2], s1 = hi ? v[1] : v[3];
    s0 = __shfl_xor(s0, 32, 64);
    s1 = __shfl_xor(s1, 32, 64);
    if (hi) { v[0] = s0; v[1] = s1; } else { v[2] = s0; v[3] = s1; }
    float t0 = odd ? v[0] : v[1], t1 = odd ? v[2] : v[3];
    t0 = __shfl_xor(t0, 16, 64);
    t1 = __shfl_xor(t1, 16, 64);
    if (odd) { v[0] = t0; v[2] = t1; } else { v[1] = t0; v[3] = t1; }
    return v;
}

// Tile, halo, waves, S and Cz are carafe_plan.h's, and so are the sizes of the three LDS arrays.
// NCHW: dout is the (B, C, 4H, 4W) gradient of the logits themselves (C <= 16 planes; channels >= C read as zero, which is
// what the padded tokens held) instead of (B, (4H)*(4W), 16) tokens: same values in the same registers, no re-layout pass.
template <bool NCHW>
__global__ __launch_bounds__(cp::F_THREADS) void carafe4_bwd_fused_kernel(const float* __restrict__ dout, const float* __restrict__ z,
                                                                 const float* __restrict__ wt_save, float* __restrict__ de,
                                                                 float* __restrict__ dz, float* __restrict__ dbias_part,
                                                                 int B, int H, int W, int tiles_x, int tiles_y, int C) {
    constexpr int S = cp::F_S, S2 = S * S, Cz = cp::F_CZ;
    constexpr int TILE = cp::F_TILE, HALO = cp::F_HALO, NP = cp::F_NP, WAVES = cp::F_WAVES;
    static_assert(S2 == 16 && Cz == 16, "the 16 x 16 x 4 MFMA operand layouts");
    __shared__ __attribute__((aligned(16))) float Gs[cp::fused_gs_floats()];      // [pixel][tap][channel]
    __shared__ __attribute__((aligned(16))) float zt[cp::fused_zt_floats()];      // z of the tile + halo
    __shared__ float bred[cp::fused_bred_floats() / Cz][Cz];                      // [wave][channel]
    static_assert(sizeof(bred) / sizeof(bred[0]) == WAVES && sizeof(Gs) + sizeof(zt) + sizeof(bred) == cp::fused_lds_bytes(), "LDS as planned");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, kq = lane >> 4;
    int t = blockIdx.x;
    const int tx = t % tiles_x; t /= tiles_x;
    const int ty = t % tiles_y;
    const int b = t / tiles_y;
    const int h0 = ty * TILE - 1, w0 = tx * TILE - 1;           // top-left of the halo region

    for (int i = tid; i < NP * (Cz / 4); i += 64 * WAVES) {
        const int pl = i >> 2, c4 = i & 3;
        const int h = h0 + pl / HALO, w = w0 + pl % HALO;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if ((unsigned)h < (unsigned)H && (unsigned)w < (unsigned)W)
            v = *reinterpret_cast<const f32x4*>(z + (((long)b * H + h) * W + w) * Cz + 4 * c4);
        *reinterpret_cast<f32x4*>(&zt[pl * Cz + 4 * c4]) = v;
    }
    __syncthreads();

    float bsum = 0.f;                                            // dbias partial: lane (li = channel), its kq's share
    // Each wave walks its pixels four at a time: all global loads of the four (reassembly weights as A operand, the D block
    // in both operand layouts, the weights again in the accumulator layout) are issued before any of them is consumed, so
    // a wave has ~1 KB x 4 in flight instead of one dependent load chain per pixel.
    constexpr int PB = 4;
    for (int pl0 = wave * PB; pl0 < NP; pl0 += WAVES * PB) {
        bool inside[PB], interior[PB];
        long pix[PB];
        float av[PB][4], dv[PB][4], wv[PB][4];
        f32x4 db[PB];
#pragma unroll
        for (int u = 0; u < PB; ++u) {
            const int pl = pl0 + u;
            const int ph = pl / HALO, pw = pl - ph * HALO;
            const int h = h0 + ph, w = w0 + pw;
            inside[u] = pl < NP && (unsigned)h < (unsigned)H && (unsigned)w < (unsigned)W;        // wave-uniform
            interior[u] = inside[u] && ph >= 1 && ph <= TILE && pw >= 1 && pw <= TILE;
            pix[u] = ((long)b * H + h) * W + w;
            db[u] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < 4; ++j) av[u][j] = dv[u][j] = wv[u][j] = 0.f;
            if (!inside[u]) continue;
            const float* wp = wt_save + pix[u] * (9 * S2);
            const float* drow = dout + (((long)b * H * S + h * S) * (W * S) + w * S) * Cz;   // hi-res pixel (4h, 4w) of the tokens
            const long hstride = (long)W * S * Cz;                                           // one hi-res row down
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (li < 9) av[u][j] = wp[li * S2 + 4 * j + kq];                              // A: tap li, sub-pixel 4j + kq
                if (!NCHW) dv[u][j] = drow[j * hstride + kq * Cz + li];  // B: channel li, sub-pixel (row j, column kq): 256-B segments
            }
            if (interior[u]) {
                if (!NCHW) db[u] = *reinterpret_cast<const f32x4*>(drow + (li >> 2) * hstride + (li & 3) * Cz + 4 * kq);
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (4 * kq + r < 9) wv[u][r] = wp[(4 * kq + r) * S2 + li];
            }
        }
        if (NCHW) {
            // In planes a pixel's block is 16-B pieces of C x 4 different rows.  Lane (li = channel, kq = pixel of the group)
            // fetches row j of its pixel's block as one 16-B load -- the four pixels of a group are neighbours, so a load
            // instruction reads 64 contiguous bytes per class plane --, then the four lanes of a channel transpose (pixel x
            // column) among themselves, which leaves dv exactly as the token form loads it ...
            const int plm = pl0 + kq, phm = plm / HALO, pwm = plm - phm * HALO;
            const int hm = h0 + phm, wm = w0 + pwm;
            const bool okm = plm < NP && (unsigned)hm < (unsigned)H && (unsigned)wm < (unsigned)W && li < C;
            const float* src = dout + ((long)b * C + li) * ((long)H * S * W * S) + ((long)hm * S) * (W * S) + wm * S;
            f32x4 X[4];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                X[j] = okm ? *reinterpret_cast<const f32x4*>(src + (long)j * (W * S)) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                X[j] = lane_transpose4(X[j], kq);
#pragma unroll
                for (int u = 0; u < PB; ++u) dv[u][j] = X[j][u];
            }
            // ... and the second operand layout (lane: sub-pixel li, channels 4 kq + r) is the transpose of the block.  The matrix
            // pipe does it: with dv as the A operand (channel x sub-pixel) and the identity as B, the accumulator layout of
            // D^T . I is that operand, and x * 1 + 0 + 0 + 0 is exact.
#pragma unroll
            for (int u = 0; u < PB; ++u) {
                if (!interior[u]) continue;                                                  // wave-uniform
                f32x4 t = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int j = 0; j < 4; ++j) t = carafe_mfma4(dv[u][j], 4 * j + kq == li ? 1.f : 0.f, t);
                db[u] = t;
            }
        }
#pragma unroll
        for (int u = 0; u < PB; ++u) {
            const int pl = pl0 + u;
            if (pl >= NP) continue;
            float* Gp = &Gs[pl * 9 * Cz];
            if (!inside[u]) {
                for (int i = lane; i < 9 * Cz; i += 64) Gp[i] = 0.f;
                continue;
            }
            // ---- G = Wt . D ----
            f32x4 g = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < 4; ++j) g = carafe_mfma4(av[u][j], dv[u][j], g);
            // C layout: lane holds G[tap = 4 kq + r][channel = li]
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (4 * kq + r < 9) Gp[(4 * kq + r) * Cz + li] = g[r];
            if (!interior[u]) continue;
            bsum += dv[u][0] + dv[u][1] + dv[u][2] + dv[u][3];
            // ---- dWt = Znbr . D^T : A lane (tap li, channels 4 kq + j), B lane (sub-pixel li, channels 4 kq + j) ----
            const int ph = pl / HALO, pw = pl - ph * HALO;
            f32x4 za = {0.f, 0.f, 0.f, 0.f};
            if (li < 9) {
                const int nh = ph + li / 3 - 1, nw = pw + li % 3 - 1;                       // neighbour inside the halo region
                za = *reinterpret_cast<const f32x4*>(&zt[(nh * HALO + nw) * Cz + 4 * kq]);   // zeros outside the image
            }
            f32x4 dw = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < 4; ++j) dw = carafe_mfma4(za[j], db[u][j], dw);
            // lane holds dWt[tap = 4 kq + r][sub-pixel = li]; softmax backward over the 9 taps of this sub-pixel
            float dot = 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) dot += wv[u][r] * dw[r];
            dot += __shfl_xor(dot, 16, 64);
            dot += __shfl_xor(dot, 32, 64);
            float* dep = de + pix[u] * (9 * S2);
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (4 * kq + r < 9) dep[(4 * kq + r) * S2 + li] = wv[u][r] * (dw[r] - dot);
        }
    }
    bsum += __shfl_xor(bsum, 16, 64);
    bsum += __shfl_xor(bsum, 32, 64);
    if (lane < Cz) bred[wave][lane] = bsum;
    __syncthreads();
    if (tid < Cz && dbias_part) {
        float t2 = 0.f;
#pragma unroll
        for (int k = 0; k < WAVES; ++k) t2 += bred[k][tid];
        dbias_part[(long)blockIdx.x * Cz + tid] = t2;
    }

    // ---- dz of the 64 interior pixels: 4 lanes x 16 B per pixel ----
    if (tid < 4 * TILE * TILE) {
        const int n = tid >> 2, c4 = tid & 3;
        const int ph = 1 + n / TILE, pw = 1 + n % TILE;
        const int h = h0 + ph, w = w0 + pw;
        if (h < H && w < W) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                // source pixel whose k-th neighbour is (h, w): (h - (k/3 - 1), w - (k%3 - 1)); outside the image its G is 0
                const int sh = ph - (k / 3 - 1), sw = pw - (k % 3 - 1);
                acc += *reinterpret_cast<const f32x4*>(&Gs[((sh * HALO + sw) * 9 + k) * Cz + 4 * c4]);
            }
            *reinterpret_cast<f32x4*>(dz + (((long)b * H + h) * W + w) * Cz + 4 * c4) = acc;
        }
    }
}

// column sums of a (rows, C) matrix: partial[blk][C] then a second pass.  Lanes and row groups as in cp::colsum_plan.
__global__ __launch_bounds__(cp::THREADS) void colsum_partial_kernel(const float* __restrict__ x, float* __restrict__ partial,
                                                                      long rows, int C) {
    __shared__ float red[cp::THREADS];
    const int lanes = min(C, cp::THREADS);
    const int rgroups = cp::THREADS / lanes;
    const int c0 = threadIdx.x % lanes, rg = threadIdx.x / lanes;
    for (int cb = 0; cb < C; cb += lanes) {          // the same trip count for every thread: the barriers below are uniform
        const int c = cb + c0;
        float s = 0.f;
        if (rg < rgroups && c < C)
            for (long r = (long)blockIdx.x * rgroups + rg; r < rows; r += (long)gridDim.x * rgroups) s += x[r * C + c];
        red[threadIdx.x] = s;
        __syncthreads();
        if (rg == 0 && c < C) {
            float t = 0.f;
            for (int k = 0; k < rgroups; ++k) t += red[k * lanes + c0];
            partial[(long)blockIdx.x * C + c] = t;
        }
        __syncthreads();
    }
}

// every pointer an entry point reads or writes as f32x4 (NULL, an absent bias, passes)
bool carafe_aligned16(const void* a, const void* b, const void* c = nullptr) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0;
}

// f(S as a compile-time constant) for an S that cp::refusal accepted
template <class F> void with_scale(int S, F f) {
    if (S == 2) f(std::integral_constant<int, 2>{});
    else f(std::integral_constant<int, 4>{});
}

// dbias = the column sums of the plan's partial rows in the workspace: now, or handed to the caller as a deferred reduction
int reduce_dbias(const cp::BwdPlan& p, const void* workspace, float* dbias, int Cz, cswin_reduce_job* deferred, hipStream_t st) {
    if (!dbias) return CSWIN_OK;
    reduce_now_or_defer(cswin_reduce_job{(const float*)workspace, dbias, nullptr, 0, Cz, Cz, p.part_rows, 0, 0, 0}, deferred, st);
    CSWIN_LAUNCH_CHECK();
    return CSWIN_OK;
}

// the fused kernel on tokens (C = Cz) or planes, then its reduction
template <bool NCHW>
int launch_fused(const cp::BwdPlan& p, const float* dout, const float* z, const float* wt_save, float* de, float* dz, float* dbias,
                 void* workspace, int B, int H, int W, int Cz, int C, cswin_reduce_job* deferred, hipStream_t st) {
    hipLaunchKernelGGL(carafe4_bwd_fused_kernel<NCHW>, dim3(p.grid_fused), dim3(cp::F_THREADS), 0, st, dout, z, wt_save, de, dz,
                       dbias ? (float*)workspace : nullptr, B, H, W, p.tiles_x, p.tiles_y, C);
    CSWIN_LAUNCH_CHECK();
    return reduce_dbias(p, workspace, dbias, Cz, deferred, st);
}

}  // namespace

extern "C" {

// e (B, H*W, 9*S*S), z (B, H*W, Cz), bias (Cz) or NULL -> out (B, (S*H)*(S*W), Cz); wt_save (B, H*W, 9*S*S) or NULL
int cswin_carafe_fwd(const float* e, const float* z, const float* bias, float* out, float* wt_save, int B, int H, int W,
                     int Cz, int S, void* stream) {
    CSWIN_REQUIRE(e && z && out, CSWIN_ERR_SHAPE, "carafe_fwd: null pointer");
    CSWIN_REQUIRE(cp::refusal(B, H, W, Cz, S) == cp::Refusal::none, CSWIN_ERR_UNSUPPORTED, "carafe_fwd: unsupported shape B=%d H=%d W=%d Cz=%d S=%d (Cz %% 4 == 0, S in {2,4})", B, H, W, Cz, S);
    CSWIN_REQUIRE(carafe_aligned16(z, bias, out), CSWIN_ERR_ALIGN, "carafe_fwd: z, bias and out must be 16-B aligned");
    const cp::FwdTokens p = cp::fwd_tokens(B, H, W, Cz, S);
    hipStream_t st = (hipStream_t)stream;
    with_scale(S, [&](auto s) {
        hipLaunchKernelGGL(carafe_fwd_kernel<decltype(s)::value>, dim3(p.grid), dim3(cp::THREADS), 0, st, e, z, bias, out, wt_save, B, H, W, Cz);
    });
    CSWIN_LAUNCH_CHECK();
    return CSWIN_OK;
}

// As cswin_carafe_fwd, but out is (B, C, S*H, S*W): the first C <= Cz channels, one plane each (the logits of the fused head)
int cswin_carafe_fwd_nchw(const float* e, const float* z, const float* bias, float* out, float* wt_save, int B, int H, int W,
                          int Cz, int C, int S, void* stream) {
    CSWIN_REQUIRE(e && z && out, CSWIN_ERR_SHAPE, "carafe_fwd_nchw: null pointer");
    CSWIN_REQUIRE(cp::planes_refusal(B, H, W, Cz, C, S) == cp::Refusal::none, CSWIN_ERR_UNSUPPORTED, "carafe_fwd_nchw: unsupported shape B=%d H=%d W=%d Cz=%d C=%d S=%d (Cz %% 4 == 0, 0 < C <= Cz, S in {2,4})", B, H, W, Cz, C, S);
    CSWIN_REQUIRE(carafe_aligned16(z, bias), CSWIN_ERR_ALIGN, "carafe_fwd_nchw: z and bias must be 16-B aligned");
    const cp::FwdPlanes p = cp::fwd_planes(B, H, W, S);
    hipStream_t st = (hipStream_t)stream;
    with_scale(S, [&](auto s) {
        hipLaunchKernelGGL(carafe_fwd_nchw_kernel<decltype(s)::value>, dim3(p.grid), dim3(cp::THREADS), 0, st, e, z, bias, out, wt_save, B, H, W, Cz, C);
    });
    CSWIN_LAUNCH_CHECK();
    return CSWIN_OK;
}

size_t cswin_carafe_bwd_workspace(int B, int H, int W, int Cz, int S) { return cp::bwd_workspace(B, H, W, Cz, S); }

// dout (B, (S*H)*(S*W), Cz) -> de (B, H*W, 9*S*S), dz (B, H*W, Cz), dbias (Cz) (may be NULL)
int cswin_carafe_bwd(const float* dout, const float* z, const float* wt_save, float* de, float* dz, float* dbias,
                     void* workspace, size_t ws_bytes, int B, int H, int W, int Cz, int S, cswin_reduce_job* deferred, void* stream) {
    if (deferred) *deferred = cswin_reduce_job{};          // part == NULL: nothing pending (no bias)
    CSWIN_REQUIRE(dout && z && wt_save && de && dz, CSWIN_ERR_SHAPE, "carafe_bwd: null pointer");
    CSWIN_REQUIRE(cp::refusal(B, H, W, Cz, S) == cp::Refusal::none, CSWIN_ERR_UNSUPPORTED, "carafe_bwd: unsupported shape");
    CSWIN_REQUIRE(!dbias || (workspace && ws_bytes >= cp::bwd_workspace(B, H, W, Cz, S)), CSWIN_ERR_WORKSPACE, "carafe_bwd: workspace too small");
    CSWIN_REQUIRE(carafe_aligned16(dout, z, dz), CSWIN_ERR_ALIGN, "carafe_bwd: dout, z and dz must be 16-B aligned");
    const cp::BwdPlan p = cp::bwd_plan(cswin_tuning().carafe_generic != 0, B, H, W, Cz, S);      // tuning aid
    hipStream_t st = (hipStream_t)stream;
    if (p.route == cp::Route::fused) return launch_fused<false>(p, dout, z, wt_save, de, dz, dbias, workspace, B, H, W, Cz, Cz, deferred, st);
    float* bpart = dbias && p.route == cp::Route::bias_in_e ? (float*)workspace : nullptr;     // the column sums ride along in bwd_e
    with_scale(S, [&](auto s) {
        hipLaunchKernelGGL(carafe_bwd_e_kernel<decltype(s)::value>, dim3(p.grid_e), dim3(cp::THREADS), 0, st, dout, z, wt_save, de, bpart, B, H, W, Cz);
        hipLaunchKernelGGL(carafe_bwd_z_kernel<decltype(s)::value>, dim3(p.grid_z), dim3(cp::THREADS), 0, st, dout, wt_save, dz, B, H, W, Cz);
    });
    if (dbias && p.route == cp::Route::colsum)
        hipLaunchKernelGGL(colsum_partial_kernel, dim3(p.colsum.grid), dim3(cp::THREADS), 0, st, dout, (float*)workspace, (long)B * H * W * S * S, Cz);
    CSWIN_LAUNCH_CHECK();
    return reduce_dbias(p, workspace, dbias, Cz, deferred, st);
}

// 1 where cswin_carafe_bwd_nchw exists: the fused S = 4, Cz = 16 kernel on whole 8 x 8 tiles (the model's head at 56 x 56)
int cswin_carafe_bwd_nchw_ok(int H, int W, int Cz, int S) { return cp::fused_shape(H, W, Cz, S) ? 1 : 0; }

// cswin_carafe_bwd for a gradient that arrives as (B, C, 4H, 4W) planes, C <= Cz = 16 (channels >= C count as zero).  Workspace,
// dbias and deferred as for cswin_carafe_bwd.  Only the fused kernel reads planes: the tuning aid does not apply.
int cswin_carafe_bwd_nchw(const float* dout, const float* z, const float* wt_save, float* de, float* dz, float* dbias,
                          void* workspace, size_t ws_bytes, int B, int H, int W, int Cz, int C, int S, cswin_reduce_job* deferred,
                          void* stream) {
    if (deferred) *deferred = cswin_reduce_job{};
    CSWIN_REQUIRE(dout && z && wt_save && de && dz, CSWIN_ERR_SHAPE, "carafe_bwd_nchw: null pointer");
    CSWIN_REQUIRE(cp::bwd_planes_refusal(B, H, W, Cz, C, S) == cp::Refusal::none, CSWIN_ERR_UNSUPPORTED,
                  "carafe_bwd_nchw: needs S = 4, Cz = 16, C <= 16, H and W multiples of %d (got B=%d H=%d W=%d Cz=%d C=%d S=%d)", cp::F_TILE, B, H, W, Cz, C, S);
    CSWIN_REQUIRE(!dbias || (workspace && ws_bytes >= cp::bwd_workspace(B, H, W, Cz, S)), CSWIN_ERR_WORKSPACE, "carafe_bwd_nchw: workspace too small");
    CSWIN_REQUIRE(carafe_aligned16(dout, z, dz), CSWIN_ERR_ALIGN, "carafe_bwd_nchw: dout, z and dz must be 16-B aligned");
    return launch_fused<true>(cp::bwd_plan(false, B, H, W, Cz, S), dout, z, wt_save, de, dz, dbias, workspace, B, H, W, Cz, C, deferred,
                              (hipStream_t)stream);
}

}  // extern "C"
