"""The implicit-GEMM convolutions' gather arithmetic (multiply-high by host-made reciprocals instead of divisions, the guarded
path beyond the reciprocal's exactness bound) at the shapes where a wrong quotient would show: two taps inside one reduction
tile, a tap boundary in the middle of a tile, channel counts that divide nothing, parity classes of unequal size, the 7 x 7
stride-4 stem on channel-padded tokens, row indices far beyond the model's and one shape past the 32-bit bound.

Every case is compared with torch.nn.functional.conv2d in float64 on the CPU (forward, input gradient, weight and bias
gradients) under test_gpu_shapes' metric and bound.  The gather change moves no load and no sum, so three cases are also
compared bit for bit with tensors recorded from the build before it (tests/golden/conv_gather_parent.npz, written by
`PYTHONPATH=. python tests/test_gpu_conv_gather.py record` on that build)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

# helpers, metric and bound of the existing float64 comparison: nothing restated here
from test_gpu_shapes import CONV_UNTOUCHED, D, RTOL, T, assert_all_within, cid, conv_case, conv_inputs, conv_problem, measure

gpu = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_gather_parent.npz")

# (B, H, W, Cin, Cout, ks, stride, pad)
HEAD = (2, 9, 11, 16, 144, 3, 1, 1)          # two taps per 32-wide reduction tile; K = 144: partial last tile; dx with 16 columns
ODD_C = (1, 6, 5, 12, 8, 3, 1, 1)            # channel count neither a power of two nor a divisor of the tile
TAP_MID = (1, 7, 6, 96, 32, 3, 2, 1)         # tap boundary in the middle of a 64-wide reduction tile
S2_EVEN = (2, 8, 8, 64, 128, 3, 2, 1)        # tap uniform per tile, stride-2 parity classes
S2_ODD = (1, 7, 9, 64, 128, 3, 2, 1)         # the same with parity classes of unequal size
STEM = (2, 29, 31, 3, 64, 7, 4, 2)           # patch_embed_conv: 3 image channels in 4-channel tokens
MANY_ROWS = (3, 181, 191, 4, 4, 3, 1, 1)     # 103 713 rows
PAST_BOUND = (2, 256, 256, 4, 4, 3, 1, 1)    # rows x pixels per image = 2^33 > 2^32: the guarded path
FEW_TILES = (1, 14, 14, 256, 512, 3, 2, 1)   # one row of tiles, K = 2304
RAGGED_K = (1, 6, 6, 72, 64, 3, 2, 1)        # K = 648, no multiple of the reduction tile

TOKEN_CASES = [HEAD, ODD_C, TAP_MID, S2_EVEN, S2_ODD, MANY_ROWS, PAST_BOUND, FEW_TILES, RAGGED_K]


@pytest.fixture(scope="module")
def ops():
    from cswin_unet_amd import ops
    return ops


def run_tokens(ops, case):
    """(y, dx, dw, db) of ops.conv_tokens on the case's seeded inputs, on the device."""
    B, H, W, Cin, Cout, ks, stride, pad = case
    x, w, b, dy = conv_inputs(case)
    xd, wd, bd = T(x, True), T(w, True), T(b, True)
    yd = ops.conv_tokens(xd, wd, bd, H, W, stride, pad)
    yd.backward(T(dy))
    return yd.detach(), xd.grad, wd.grad, bd.grad


def stem_inputs(case):
    B, H, W, Cin, Cout, ks, stride, pad = case
    OH, OW = (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1
    x, w, b, dy = conv_inputs(case)                      # x: (B, H*W, Cin) values, used as the NCHW image below
    return np.ascontiguousarray(x.reshape(B, H, W, Cin).transpose(0, 3, 1, 2)), w, b, dy, OH, OW


def run_stem(ops, case):
    """(y, dw, db) of ops.patch_embed_conv on the case's image."""
    img, w, b, dy, _, _ = stem_inputs(case)
    wd, bd = T(w, True), T(b, True)
    yd = ops.patch_embed_conv(T(img), wd, bd, case[6], case[7])
    yd.backward(T(dy))
    return yd.detach(), wd.grad, bd.grad


@functools.lru_cache(maxsize=None)
def stem_reference(case):
    img, w, b, dy, _, _ = stem_inputs(case)
    wr, br = D(w), D(b)
    y = F.conv2d(torch.from_numpy(img).double(), wr, br, case[6], case[7])
    y = y.permute(0, 2, 3, 1).reshape(y.shape[0], -1, y.shape[1])
    y.backward(torch.from_numpy(dy).double())
    return y.detach(), wr.grad, br.grad


def assert_exact_zeros(case, dx):
    """Input pixels that no output reaches: the reference's dx is exactly 0 there, and so must the device's be."""
    untouched = conv_problem(case)[1][1] == 0
    bad = int((dx.cpu()[untouched] != 0).sum())
    assert bad == 0, f"{bad} of {int(untouched.sum())} untouched dx elements are not 0"
    return int(untouched.sum())


def test_multiply_high_quotient_is_exact_inside_the_bound_and_not_beyond():
    """The arithmetic the kernels rely on (fdiv, csrc/common.h), in Python integers: floor(n * ceil(2^32 / d) / 2^32) = n // d
    for every dividend with n * d < 2^32 -- checked at the dividends where an error would first show (multiples of d and their
    predecessors, up to the bound) -- and a wrong quotient just past it for the guarded case's divisor, which is why the host
    checks the bound instead of assuming it."""
    for d in (2, 3, 7, 9, 12, 16, 49, 96, 99, 144, 3136, 34571, 65535, 65536):
        m = -(-2 ** 32 // d)
        top = (2 ** 32 - 1) // d                       # largest n with n * d < 2^32
        for q in {1, 2, top // d // 2, top // d - 1, top // d}:
            for n in (q * d - 1, q * d, q * d + 1, top):
                if 0 <= n <= top:
                    assert (n * m) >> 32 == n // d, (n, d)
    B, H, W = PAST_BOUND[:3]
    d, n = H * W, B * H * W - 1                        # the last row of PAST_BOUND split by its pixels per image
    assert n * d >= 2 ** 32 and d & (d - 1) == 0       # past the bound (a power of two happens to stay exact: the bound is sufficient,
    d = 65535                                          # not necessary), so show the failure with a neighbouring divisor
    n = next(k * d - 1 for k in range(1, 2 ** 16 + 2) if (((k * d - 1) * -(-2 ** 32 // d)) >> 32) != (k * d - 1) // d)
    assert n * d >= 2 ** 32 and n < 2 ** 32


@gpu
@pytest.mark.parametrize("case", TOKEN_CASES, ids=cid)
def test_conv_gather_vs_float64_conv2d(ops, case):
    errs, dx = conv_case(ops, case, "conv_gather")
    assert_all_within(errs, RTOL)
    assert_exact_zeros(case, dx)


@gpu
@pytest.mark.parametrize("case", CONV_UNTOUCHED, ids=cid)
def test_conv_gather_transposed_gather_leaves_exact_zeros(ops, case):
    """The generic transposed gather (neither "same" nor 3 x 3 stride 2) on maps whose last row / column no output reaches."""
    errs, dx = conv_case(ops, case, "conv_gather_untouched")
    assert_all_within(errs, RTOL)
    n = assert_exact_zeros(case, dx)
    assert 0 < n < dx.numel()


@gpu
def test_conv_gather_stem_vs_float64_conv2d(ops):
    got, ref = run_stem(ops, STEM), stem_reference(STEM)
    errs = {k: measure(g, r, f"conv_gather.stem.{cid(STEM)}.{k}") for k, g, r in zip(("y", "dw", "db"), got, ref)}
    assert_all_within(errs, RTOL)


def recorded_tensors(ops):
    """name -> device tensor of the three cases that are pinned bit for bit: one "same" convolution, one stride-2, the stem."""
    out = {}
    for tag, case in (("same", HEAD), ("s2", TAP_MID)):
        for k, t in zip(("y", "dx", "dw", "db"), run_tokens(ops, case)):
            out[f"{tag}.{k}"] = t
    for k, t in zip(("y", "dw", "db"), run_stem(ops, STEM)):
        out[f"stem.{k}"] = t
    return out


@gpu
def test_conv_gather_bits_of_the_division_free_gather_equal_the_recorded_ones(ops):
    """Removing the divisions changes addresses' arithmetic only: the loads and the order of every sum are those of the build
    the fixture was recorded from, so every output must equal it bit for bit."""
    want = np.load(GOLDEN)
    got = recorded_tensors(ops)
    assert sorted(want.files) == sorted(got)
    for name, t in got.items():
        ref = torch.from_numpy(want[name])
        assert torch.equal(t.cpu(), ref), f"{name}: {int((t.cpu() != ref).sum())} of {ref.numel()} elements differ"


if __name__ == "__main__" and sys.argv[1:2] == ["record"]:
    from cswin_unet_amd import ops as _ops
    dest = sys.argv[2] if len(sys.argv) > 2 else GOLDEN
    os.makedirs(os.path.dirname(dest), exist_ok=True)
    np.savez(dest, **{k: v.cpu().numpy() for k, v in recorded_tensors(_ops).items()})
    print("wrote", dest, os.path.getsize(dest), "bytes")
