"""Token convolutions, CARAFE reassembly and LayerNorm away from the two product models' shapes: maps with H != W, odd sides,
empty parity classes, channel counts and reduction lengths that are no multiple of a tile, the generic transposed gather, the
bf16-operand convolution GEMMs, Cz > 512 and the LayerNorm widths and grid loop that no model-shaped test reaches.

Every reference is float64 on the CPU (torch conv2d / layer_norm with autograd, the CARAFE closed form below); the metric is
test_gpu_parity's max|got - ref| / rms(ref), the bound its fp32 RTOL = 1e-3, and every measured error is appended to
test_gpu_parity's error log under a tag that names the case.  The tests at the top need no GPU: they check the reference
helpers themselves against independently written formulations."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle.determ import det_normal

# the fp32 bound (BASELINE's north star), the bound of test_linear_bf16_operands and the error log, none of them new
from test_gpu_parity import BF16_RTOL, LOG, RTOL

gpu = pytest.mark.gpu
DEV = "cuda"


def D(a):
    """float64 CPU leaf tensor of a numpy array / tensor."""
    t = torch.from_numpy(a) if isinstance(a, np.ndarray) else a
    return t.detach().double().clone().requires_grad_()


def T(a, grad=False):
    t = (torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a.detach().clone()).float().to(DEV)
    return t.requires_grad_() if grad else t


def measure(got, ref, what):
    """max|got - ref| / rms(ref) over every element, in float64; logged under `what`."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    err = float((got - ref).abs().max()) / (float(ref.pow(2).mean().sqrt()) + 1e-30)
    print(f"{what}: max|diff|/rms = {err:.3e}")
    try:
        os.makedirs(os.path.dirname(LOG), exist_ok=True)
        with open(LOG, "a") as f:
            f.write(f"{what}: {err:.3e}\n")
    except OSError:
        pass
    return err


def rel_err(got, ref, what):
    err = measure(got, ref, what)
    assert np.isfinite(err) and err <= RTOL, f"{what}: max|diff|/rms = {err:.3e} > {RTOL}"
    return err


def cid(case):
    """Test id of a convolution case."""
    return "B{}-H{}-W{}-i{}-o{}-k{}-s{}-p{}".format(*case)


def bf16_round(a):
    return torch.from_numpy(a).bfloat16().float().numpy()


# ------------------------------------------------------------------------------------------------
# reference helpers (float64, CPU)
# ------------------------------------------------------------------------------------------------
def tokens_to_map(x, H, W):
    """(B, H*W, C) tokens -> (B, C, H, W)."""
    return x.view(x.shape[0], H, W, x.shape[-1]).permute(0, 3, 1, 2)


def map_to_tokens(y):
    """(B, C, H, W) -> (B, H*W, C) tokens."""
    return y.permute(0, 2, 3, 1).reshape(y.shape[0], -1, y.shape[1])


def conv_reference(x, w, b, dy, H, W, stride, pad):
    """float64 nn.Conv2d on tokens with autograd: (y, dx, dw, db); dy None: y alone."""
    xr, wr, br = D(x), D(w), D(b)
    y = map_to_tokens(F.conv2d(tokens_to_map(xr, H, W), wr, br, stride, pad))
    if dy is None:
        return (y.detach(),)
    y.backward(torch.from_numpy(dy).double())
    return y.detach(), xr.grad, wr.grad, br.grad


def conv_inputs(case, rounded=False):
    B, H, W, Cin, Cout, ks, stride, pad = case
    OH, OW = (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1
    tag = "shp.conv." + ".".join(map(str, case))
    x = det_normal(tag + ".x", (B, H * W, Cin))
    w = det_normal(tag + ".w", (Cout, Cin, ks, ks), 1 / np.sqrt(Cin * ks * ks))
    b = det_normal(tag + ".b", (Cout,), 0.1)
    dy = det_normal(tag + ".dy", (B, OH * OW, Cout))
    if rounded:
        x, w, dy = bf16_round(x), bf16_round(w), bf16_round(dy)
    return x, w, b, dy


@functools.lru_cache(maxsize=None)
def conv_problem(case, rounded=False):
    """(inputs, float64 reference) of one convolution case; computed once, shared by the tests that use the case, never written."""
    x, w, b, dy = conv_inputs(case, rounded)
    return (x, w, b, dy), conv_reference(x, w, b, dy, case[1], case[2], case[6], case[7])


def carafe_closed_form(e, z, bias, H, W, S):
    """out (B, S*S*H*W, Cz) of the CARAFE reassembly in its closed form, for any H, W: softmax over the 9 taps, zero-padded
    3x3 gather of z, pixel shuffle of the S*S sub-pixels, plus bias.  e (B, H*W, 9*S*S), z (B, H*W, Cz), bias (Cz)."""
    B, _, Cz = z.shape
    wt = torch.softmax(e.view(B, H, W, 9, S * S), dim=3)                                   # (B, H, W, k, s)
    zp = F.pad(z.view(B, H, W, Cz), (0, 0, 1, 1, 1, 1))
    up = 0
    for kk in range(9):
        ky, kx = divmod(kk, 3)
        up = up + wt[:, :, :, kk, :, None] * zp[:, ky:ky + H, kx:kx + W, None, :]          # (B, H, W, s, C)
    return up.view(B, H, W, S, S, Cz).permute(0, 1, 3, 2, 4, 5).reshape(B, S * S * H * W, Cz) + bias


def carafe_unfold_form(e, z, bias, H, W, S):
    """The same operation the way the CARAFE module spells it: kernel logits through F.pixel_shuffle, softmax over the tap
    planes, the 3x3 neighbourhoods of z by F.unfold, each repeated over its S x S block of output pixels."""
    B, _, Cz = z.shape
    kern = torch.softmax(F.pixel_shuffle(e.view(B, H, W, 9 * S * S).permute(0, 3, 1, 2), S), dim=1)      # (B, 9, SH, SW)
    nb = F.unfold(z.view(B, H, W, Cz).permute(0, 3, 1, 2), 3, padding=1).view(B, Cz, 9, H, W)
    nb = nb.repeat_interleave(S, dim=3).repeat_interleave(S, dim=4)                                     # (B, Cz, 9, SH, SW)
    out = (nb * kern[:, None]).sum(2)                                                                   # (B, Cz, SH, SW)
    return out.permute(0, 2, 3, 1).reshape(B, S * S * H * W, Cz) + bias


def carafe_problem(B, H, W, S, Cz, zero_from=None):
    tag = f"shp.carafe.{B}.{H}.{W}.{S}.{Cz}"
    e = det_normal(tag + ".e", (B, H * W, 9 * S * S))
    z = det_normal(tag + ".z", (B, H * W, Cz))
    bias = det_normal(tag + ".b", (Cz,), 0.1)
    if zero_from is not None:                # what a head weight padded with zero rows gives
        z[..., zero_from:] = 0
        bias[zero_from:] = 0
    return e, z, bias


def ln_problem(M, C):
    x = (det_normal(f"shp.ln.x.{M}.{C}", (M, C)) * 2 + 30).astype(np.float32)       # row mean 15 standard deviations out
    g = (1 + det_normal(f"shp.ln.g.{C}", (C,), 0.1)).astype(np.float32)
    b = det_normal(f"shp.ln.b.{C}", (C,), 0.1)
    dy = det_normal(f"shp.ln.dy.{M}.{C}", (M, C))
    return x, g, b, dy


def ln_reference(x, g, b, dy, eps=1e-5):
    xr, gr, br = D(x), D(g), D(b)
    y = F.layer_norm(xr, (x.shape[-1],), gr, br, eps)
    y.backward(torch.from_numpy(dy).double())
    return y.detach(), xr.grad, gr.grad, br.grad


# ------------------------------------------------------------------------------------------------
# the reference helpers against independent formulations (no GPU)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,S,Cz", [(2, 3, 5, 2, 8), (1, 4, 3, 4, 4)])
def test_carafe_closed_form_equals_unfold_pixel_shuffle_form(B, H, W, S, Cz):
    e, z, bias = (torch.from_numpy(a).double() for a in carafe_problem(B, H, W, S, Cz))
    a, b = carafe_closed_form(e, z, bias, H, W, S), carafe_unfold_form(e, z, bias, H, W, S)
    assert a.shape == b.shape == (B, S * S * H * W, Cz)
    assert float((a - b).abs().max()) <= 1e-12


@pytest.mark.parametrize("case", [(2, 3, 5, 4, 8, 3, 2, 1), (1, 4, 7, 4, 4, 2, 2, 0), (1, 5, 6, 4, 4, 5, 3, 2)], ids=cid)
def test_conv_reference_equals_direct_sum_over_taps(case):
    """The token <-> map plumbing of conv_reference (H != W, stride, padding) against the convolution written out as a loop
    over output pixels and taps on the token layout itself, and dx / dw / db against their own sums."""
    B, H, W, Cin, Cout, ks, stride, pad = case
    x, w, b, dy = conv_inputs(case)
    y, dx, dw, db = conv_reference(x, w, b, dy, H, W, stride, pad)
    xd, wd, gd = (torch.from_numpy(a).double() for a in (x, w, dy))
    OH, OW = (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1
    y2 = torch.from_numpy(b).double().repeat(B, OH * OW, 1)
    dx2, dw2 = torch.zeros_like(xd), torch.zeros_like(wd)
    for oy in range(OH):
        for ox in range(OW):
            for ky in range(ks):
                for kx in range(ks):
                    iy, ix = oy * stride - pad + ky, ox * stride - pad + kx
                    if 0 <= iy < H and 0 <= ix < W:
                        o, i = oy * OW + ox, iy * W + ix
                        y2[:, o] += xd[:, i] @ wd[:, :, ky, kx].t()
                        dx2[:, i] += gd[:, o] @ wd[:, :, ky, kx]
                        dw2[:, :, ky, kx] += gd[:, o].t() @ xd[:, i]
    for got, ref in ((y, y2), (dx, dx2), (dw, dw2), (db, gd.sum((0, 1)))):
        assert float((got - ref).abs().max()) <= 1e-12 * (1 + float(ref.abs().max()))


@pytest.mark.parametrize("case,rows,cols", [((1, 7, 7, 16, 8, 2, 2, 0), [6], [6]), ((2, 13, 18, 4, 64, 7, 4, 2), [], [17])])
def test_conv_reference_dx_is_exactly_zero_where_no_output_reaches(case, rows, cols):
    """The pixel set test_conv_untouched_input_pixels_get_exact_zeros reads off the reference is the geometric one."""
    B, H, W, Cin = case[:4]
    dx = conv_problem(case)[1][1].view(B, H, W, Cin)
    want = torch.zeros(H, W, dtype=torch.bool)
    want[rows, :] = True
    want[:, cols] = True
    assert torch.equal((dx == 0).all(-1).all(0), want) and torch.equal((dx == 0).any(-1).any(0), want)


def test_layernorm_reference_equals_its_definition():
    x, g, b, dy = ln_problem(5, 36)
    y, dx, dg, db = ln_reference(x, g, b, dy)
    xd, gd, bd, dyd = (torch.from_numpy(a).double() for a in (x, g, b, dy))
    mu, var = xd.mean(-1, keepdim=True), xd.var(-1, unbiased=False, keepdim=True)
    xh = (xd - mu) / torch.sqrt(var + 1e-5)
    gy = dyd * gd
    dx2 = (gy - gy.mean(-1, keepdim=True) - xh * (gy * xh).mean(-1, keepdim=True)) / torch.sqrt(var + 1e-5)
    for got, ref in ((y, xh * gd + bd), (dx, dx2), (dg, (dyd * xh).sum(0)), (db, dyd.sum(0))):
        assert float((got - ref).abs().max()) <= 1e-11


# ------------------------------------------------------------------------------------------------
# 1. token convolutions against float64 conv2d
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ops():
    from cswin_unet_amd import ops
    return ops


@pytest.fixture()
def bf16_matmul():
    import cswin_unet_amd
    prev = cswin_unet_amd.set_matmul_precision("bf16")
    yield
    cswin_unet_amd.set_matmul_precision(prev)


# Beside each case: what its three GEMMs launch -- forward, data gradient, weight gradient -- as `tile x k-tile KWn` (n wave
# groups) of launch_gemm, read off launch_gemm / k_groups / choose_split / cswin_conv_tok_bwd_data.  R is the reduction length,
# "R%32" marks one that is no multiple of the 32-wide k-tile (so of no k-tile).  launch_gemm takes the 64x32 tile for every
# single-split launch of at most 256 64x64 tiles whose 64x32 tiles are at most 256 too (its cost model charges a tile by
# ceil(tiles / 256)), so the 64x64 tile of a forward / data-gradient launch needs 129..256 tiles of 64x64 and an N in (32, 64]:
# the last "same" case exists for that.  Weight gradients with more than one slab always take 64x64.
CONV_SAME = [                        # stride-1 "same": data gradient = cswin_conv_weight_flipT + the forward kernel
    (2, 5, 9, 4, 8, 3, 1, 1),        # fwd R=36 R%32: 64x32x32 KW1 | dx R=72 R%32: 64x32x32 KW1 | dw 1 slab: 64x32x32 KW1
    (1, 7, 6, 32, 36, 3, 1, 1),      # fwd R=288: 64x32x64 KW2 | dx R=324 R%32: 64x32x64 KW2 | dw 1 slab: 64x32x32 KW1
    (3, 6, 11, 64, 144, 3, 1, 1),    # fwd R=576: 64x32x64 KW2 | dx R=1296 R%32: 64x32x64 KW2 | dw 198 rows in 2 slabs of 104 (ragged): 64x64x32 KW1
    (2, 4, 7, 16, 12, 5, 1, 2),      # fwd R=400 R%32: 64x32x64 KW2 | dx R=300 R%32: 64x32x64 KW2 | dw 1 slab: 64x32x32 KW1
    (2, 3, 5, 24, 20, 1, 1, 0),      # fwd R=24 R%32: 64x32x32 KW1 | dx R=20 R%32: 64x32x32 KW1 | dw 1 slab: 64x32x32 KW1
    # added to the issue's list (see above): 8256 pixels = 129 row tiles
    (2, 48, 86, 64, 48, 3, 1, 1),    # fwd R=576: 64x64x64 KW4 | dx R=432 R%32: 64x64x64 KW2 | dw 8256 rows in 65 slabs of 128 (ragged): 64x64x32 KW1
]
CONV_S2 = [                          # 3x3 stride 2 pad 1: data gradient = gemm_conv_s2_dgrad_batch_kernel over the parity classes
    (2, 7, 10, 8, 16, 3, 2, 1),      # fwd R=72 R%32: 64x32x32 KW1 | dx <1,0> (R 16..64, odd H: classes of 4 and 3 rows) | dw 1 slab: 64x32x32 KW1
    (1, 9, 5, 64, 128, 3, 2, 1),     # fwd R=576: 64x32x64 KW2 | dx <4,0> (R up to 512, odd H and W) | dw 1 slab: 64x32x32 KW1
    (3, 1, 6, 4, 4, 3, 2, 1),        # fwd R=36 R%32: 64x32x32 KW1 | dx <1,0> (H = 1: both py = 1 classes empty) | dw 1 slab: 64x32x32 KW1
    (2, 12, 8, 128, 68, 3, 2, 1),    # fwd R=1152: 64x32x64 KW2 | dx <2,0> (R up to 272, taps with oy = OH dropped) | dw 1 slab: 64x32x32 KW1
]
CONV_GENERIC = [                     # everything else: data gradient = launch_gemm over the transposed gather ConvTSrc
    (2, 13, 18, 4, 64, 7, 4, 2),     # fwd R=196 R%32: 64x32x32 KW1 | dx R=3136: 64x32x64 KW2 | dw 1 slab: 64x32x32 KW1
    (2, 6, 9, 8, 12, 3, 1, 0),       # fwd R=72 R%32: 64x32x32 KW1 | dx R=108 R%32: 64x32x32 KW1 | dw 1 slab: 64x32x32 KW1
    (1, 7, 7, 16, 8, 2, 2, 0),       # fwd R=64: 64x32x32 KW1 | dx R=32: 64x32x32 KW1 | dw 1 slab: 64x32x32 KW1
    (2, 8, 5, 12, 16, 3, 2, 0),      # fwd R=108 R%32: 64x32x32 KW1 | dx R=144 R%32: 64x32x32 KW1 | dw 1 slab: 64x32x32 KW1
    (1, 10, 14, 32, 64, 5, 3, 2),    # fwd R=800: 64x32x64 KW2 | dx R=1600: 64x32x64 KW2 | dw 1 slab: 64x32x32 KW1
]
CONV_FWD_ONLY = [                    # Cout % 4 != 0: the scalar epilogue (and no backward: the gradient kernels need Cout % 4 == 0)
    (2, 5, 6, 8, 9, 3, 1, 1),        # fwd R=72 R%32: 64x32x32 KW1
    (1, 4, 9, 16, 66, 3, 2, 1),      # fwd R=144 R%32: 64x32x32 KW1
]
CONV_UNTOUCHED = [(1, 7, 7, 16, 8, 2, 2, 0), (2, 13, 18, 4, 64, 7, 4, 2)]
# precision == 1 has the 64x64x64 tile alone, with two wave groups where k_groups() >= 2 (every forward and data gradient
# below: R >= 256 in under 640 workgroups) and one otherwise (every weight gradient below: slabs shorter than 256 rows)
CONV_BF16 = [
    (1, 7, 6, 32, 36, 3, 1, 1),      # fwd KW2 | dx (flipT + forward kernel, R=324 R%32) KW2 | dw 1 slab KW1
    (3, 6, 11, 64, 144, 3, 1, 1),    # fwd KW2 | dx R=1296 KW2 | dw 2 slabs of 104 (ragged) KW1
    (1, 9, 5, 64, 128, 3, 2, 1),     # fwd KW2 | dx gemm_conv_s2_dgrad_batch_kernel<2,1> | dw 1 slab KW1
    (2, 12, 8, 128, 68, 3, 2, 1),    # fwd KW2 | dx gemm_conv_s2_dgrad_batch_kernel<2,1> | dw 1 slab KW1
    (1, 10, 14, 32, 64, 5, 3, 2),    # fwd KW2 | dx ConvTSrc R=1600 KW2 | dw 1 slab KW1
]


def conv_case(ops, case, tag, rounded=False):
    """One convolution, forward and backward, against conv_problem's reference: {y, dx, dw, db: error} and the device dx."""
    B, H, W, Cin, Cout, ks, stride, pad = case
    (x, w, b, dy), ref = conv_problem(case, rounded)
    xd, wd, bd = T(x, True), T(w, True), T(b, True)
    yd = ops.conv_tokens(xd, wd, bd, H, W, stride, pad)
    yd.backward(T(dy))
    name = tag + "." + cid(case)
    got = (yd, xd.grad, wd.grad, bd.grad)
    return {k: measure(g, r, f"{name}.{k}") for k, g, r in zip(("y", "dx", "dw", "db"), got, ref)}, xd.grad


def assert_all_within(errs, bound):
    assert all(np.isfinite(e) and e <= bound for e in errs.values()), errs


@gpu
@pytest.mark.parametrize("case", CONV_SAME + CONV_S2 + CONV_GENERIC, ids=cid)
def test_conv_tokens_vs_float64_conv2d(ops, case):
    """y, dx, dw, db of ops.conv_tokens on non-square, odd-sided maps at RTOL.  One missing or misplaced tap moves an output by
    about rms / sqrt(ks*ks*Cin) >= 2e-2 here."""
    assert_all_within(conv_case(ops, case, "shapes.conv")[0], RTOL)


@gpu
@pytest.mark.parametrize("case", CONV_UNTOUCHED, ids=cid)
def test_conv_untouched_input_pixels_get_exact_zeros(ops, case):
    """Input pixels that no output reaches (the last row / column when the stride leaves a remainder): the reference's dx is
    exactly 0 there and ConvTSrc must gather nothing, not something small."""
    ref_dx = conv_problem(case)[1][1]
    untouched = ref_dx == 0
    assert 0 < int(untouched.sum()) < untouched.numel()
    errs, dx = conv_case(ops, case, "shapes.conv_untouched")
    assert_all_within(errs, RTOL)
    assert bool((dx.cpu()[untouched] == 0).all()), f"{int((dx.cpu()[untouched] != 0).sum())} of {int(untouched.sum())} untouched dx elements are not 0"


@gpu
@pytest.mark.parametrize("case", CONV_FWD_ONLY, ids=cid)
def test_conv_tokens_forward_cout_not_multiple_of_4(ops, case):
    B, H, W, Cin, Cout, ks, stride, pad = case
    x, w, b, _ = conv_inputs(case)
    (ref,) = conv_reference(x, w, b, None, H, W, stride, pad)
    with torch.no_grad():
        y = ops.conv_tokens(T(x), T(w), T(b), H, W, stride, pad)
    rel_err(y, ref, "shapes.conv_fwd." + cid(case) + ".y")


@gpu
@pytest.mark.parametrize("case", CONV_BF16, ids=cid)
def test_conv_tokens_bf16_operands_exact_on_bf16_inputs(ops, bf16_matmul, case):
    """x, w, dy hold bf16 values, so the kernel's rounding of its operands changes nothing, their products are exact in fp32
    and the accumulation is fp32: the float64 convolution of the same values must be met at the fp32 RTOL, which shows a
    wrong tap or channel at a border (>= 2e-2) where the whole-model bf16 bounds of 3e-2 .. 5e-2 cannot."""
    assert_all_within(conv_case(ops, case, "shapes.conv_bf16exact", rounded=True)[0], RTOL)


@gpu
def test_conv_tokens_bf16_operands_round_unrounded_inputs(ops, bf16_matmul):
    """Unrounded inputs: the error of y is that of bf16 operands -- above anything fp32 MFMA gives (~1e-6), below BF16_RTOL --
    which proves that the precision == 1 kernels really ran in the test above."""
    errs, _ = conv_case(ops, (3, 6, 11, 64, 144, 3, 1, 1), "shapes.conv_bf16")
    assert 1e-5 < errs["y"] < BF16_RTOL, errs
    assert_all_within(errs, BF16_RTOL)


# ------------------------------------------------------------------------------------------------
# 2. CARAFE reassembly, non-square, against the closed form
# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("H,W,S,Cz,B", [(8, 16, 4, 16, 2),      # fused 8x8-tile backward, 1 x 2 tiles
                                        (16, 8, 4, 16, 1),      # fused 8x8-tile backward, 2 x 1 tiles
                                        (5, 9, 4, 16, 2),       # generic, S = 4
                                        (3, 7, 2, 96, 2),       # generic, S = 2, 24 chunks on 16 lanes
                                        (6, 4, 2, 256, 1),      # generic, S = 2, one chunk per lane
                                        (2, 3, 2, 516, 1)])     # Cz > 512: column sums of dout by colsum_partial_kernel
def test_carafe_non_square_vs_closed_form(ops, H, W, S, Cz, B):
    e, z, bias = carafe_problem(B, H, W, S, Cz)
    dout = det_normal(f"shp.carafe.{B}.{H}.{W}.{S}.{Cz}.dout", (B, S * S * H * W, Cz))
    er, zr, br = D(e), D(z), D(bias)
    out_r = carafe_closed_form(er, zr, br, H, W, S)
    out_r.backward(torch.from_numpy(dout).double())
    ed, zd, bd = T(e, True), T(z, True), T(bias, True)
    out_d = ops.carafe_reassemble(ed, zd, bd, H, W, S)
    out_d.backward(T(dout))
    tag = f"shapes.carafe.H{H}W{W}S{S}C{Cz}B{B}"
    rel_err(out_d, out_r, tag + ".out")
    rel_err(ed.grad, er.grad, tag + ".de")
    rel_err(zd.grad, zr.grad, tag + ".dz")
    rel_err(bd.grad, br.grad, tag + ".dbias")


@gpu
def test_carafe_nchw_head_form_non_square_vs_closed_form(ops):
    """The segmentation head's form (class planes written by the reassembly, read by cswin_carafe_bwd_nchw) on an 8 x 24 map
    against the closed form restricted to the first 9 of 16 channels."""
    B, H, W, S, Cz, C = 2, 8, 24, 4, 16, 9
    assert ops.lib().cswin_carafe_bwd_nchw_ok(H, W, Cz, S) == 1
    e, z, bias = carafe_problem(B, H, W, S, Cz, zero_from=C)
    dout = det_normal("shp.carafe.nchw.dout", (B, C, S * H, S * W))
    er, zr, br = D(e), D(z), D(bias)
    out_r = carafe_closed_form(er, zr, br, H, W, S)[..., :C].view(B, S * H, S * W, C).permute(0, 3, 1, 2)
    out_r.backward(torch.from_numpy(dout).double())
    ed, zd, bd = T(e, True), T(z, True), T(bias, True)
    out_d = ops.carafe_reassemble_nchw(ed, zd, bd, H, W, S, C)
    out_d.backward(T(dout))
    tag = f"shapes.carafe_nchw.H{H}W{W}C{C}"
    rel_err(out_d, out_r, tag + ".out")
    rel_err(ed.grad, er.grad, tag + ".de")
    rel_err(zd.grad, zr.grad, tag + ".dz")
    rel_err(bd.grad, br.grad, tag + ".dbias")


# ------------------------------------------------------------------------------------------------
# 3. LayerNorm widths, row loop, float64 reference
# ------------------------------------------------------------------------------------------------
# ln_grid caps the grid at 512 workgroups of rows_per_block rows: 4 at C = 256 / 1024 and in the generic kernel, 16 at C = 64,
# so 2051 and 8195 rows are the first sizes (with a ragged last pass) at which a workgroup takes a second row
LN_FAST = [(300, 32), (7, 1024), (2051, 256), (2051, 1024), (8195, 64)]
LN_GENERIC = [(5, 4), (33, 36), (257, 96), (130, 260), (3, 768), (2051, 192), (9, 1020)]


@gpu
@pytest.mark.parametrize("M,C", LN_FAST + LN_GENERIC)
def test_layernorm_widths_and_row_loop_vs_float64(ops, M, C):
    x, g, b, dy = ln_problem(M, C)
    ref = ln_reference(x, g, b, dy)
    xd, gd, bd = T(x, True), T(g, True), T(b, True)
    yd = ops.layer_norm(xd, gd, bd, 1e-5)
    yd.backward(T(dy))
    for name, got, want in zip(("y", "dx", "dgamma", "dbeta"), (yd, xd.grad, gd.grad, bd.grad), ref):
        rel_err(got, want, f"shapes.ln{M}x{C}.{name}")


@gpu
@pytest.mark.parametrize("M,C", [(257, 96), (300, 32)])
def test_layernorm_backward_residual_in_place_and_bf16_twin(ops, M, C):
    """cswin_layernorm_bwd as a CSWinBlock's backward calls it: dres aliases dx (the residual-path gradient is added in place)
    and dx16 receives the rounded twin of the sum."""
    x, g, b, dy = ln_problem(M, C)
    dres = det_normal(f"shp.ln.dres.{M}.{C}", (M, C))
    _, dx_r, dg_r, db_r = ln_reference(x, g, b, dy)
    xd, gd, bd = T(x), T(g), T(b)
    _, mean, rstd = ops._layernorm_fwd(xd, gd, bd, 1e-5)
    dx = T(dres)
    dx16 = torch.zeros(M, C, dtype=torch.bfloat16, device=DEV)
    dg, db = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    ops._layernorm_bwd(T(dy), xd, mean, rstd, gd, dx, dg, db, dres=dx, dx16=dx16)
    rel_err(dx, dx_r + torch.from_numpy(dres).double(), f"shapes.ln_bwd{M}x{C}.dx_plus_dres")
    rel_err(dg, dg_r, f"shapes.ln_bwd{M}x{C}.dgamma")
    rel_err(db, db_r, f"shapes.ln_bwd{M}x{C}.dbeta")
    assert torch.equal(dx16, dx.bfloat16())
