"""Host side of the device resizes (utils.zoom_operator / nearest_index): the band tables taken from scipy reproduce
scipy.ndimage.zoom.  Runs without a GPU: the device kernel's arithmetic (csrc/resize.hip) is emulated in numpy float64.

Bounds.  The float64 band product against scipy's own float64 zoom: 1e-14 absolute on standard-normal slices (the dense product
measured <= 1.8e-15; entries outside the band are below 2**-64 ~ 5e-20 each).  After the cast to float32 the comparison is bit
for bit: a rounding tie would need the two float64 results to straddle a float32 midpoint, probability ~ 1e-15 / 6e-8 per
element; no seed here lands on one."""
import inspect

import numpy as np
import pytest
from scipy.ndimage import zoom

from resize_cases import GPU_SHAPES, HOST_SHAPES, PAIRS_1D, banded_product, gather_nearest, scipy_zoom3, slices


@pytest.mark.parametrize("shape,size", GPU_SHAPES + HOST_SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_banded_product_equals_scipy_zoom(shape, size):
    x = slices(shape, size)
    got = banded_product(x, size)
    want64 = scipy_zoom3(shape, size, widen=True)
    err = float(np.abs(got - want64).max())
    print(f"{shape} -> {size}: max |float64 diff| {err:.3g}")
    assert err <= 1e-14
    want32 = scipy_zoom3(shape, size)
    assert want32.dtype == np.float32
    unequal = int((got.astype(np.float32).view(np.uint32) != want32.view(np.uint32)).sum())
    assert unequal == 0, (unequal, got.size)


def test_float64_slices_round_like_float32_ones():
    """predict_volume casts scipy's float64 result of a float64 volume to float32: the same single rounding."""
    shape, size = GPU_SHAPES[0]
    x = slices(shape, size, "float64")
    got = banded_product(x, size).astype(np.float32)
    assert np.array_equal(got.view(np.uint32), scipy_zoom3(shape, size, "float64").astype(np.float32).view(np.uint32))


@pytest.mark.parametrize("n_in,n_out", PAIRS_1D + [(b, a) for a, b in PAIRS_1D if a != b])
def test_operator_table_invariants(n_in, n_out):
    from cswin_unet_amd.utils import zoom_operator
    w, s = zoom_operator(n_in, n_out)
    assert w.dtype == np.float64 and s.dtype == np.int32
    T = w.shape[1]
    assert w.shape == (n_out, T) and s.shape == (n_out,) and 1 <= T <= n_in
    assert s.min() >= 0 and (s + T).max() <= n_in
    # the band is the dense operator: rebuilt from scipy's unit-vector zooms, nothing >= 2**-64 lies outside it
    R = np.stack([zoom(e, n_out / n_in, order=3) for e in np.eye(n_in)], axis=1)
    dense = np.zeros_like(R)
    for i in range(n_out):
        dense[i, s[i]:s[i] + T] = w[i]
    assert np.array_equal(dense[dense != 0], R[dense != 0]) and np.abs(R - dense).max() < 2.0 ** -64
    # rows sum to 1 -- except rows that scipy itself leaves at its constant 0 (it rounds the last output coordinate of
    # 512 -> 224 past the last sample): those are all zero here as well
    ones = zoom(np.ones(n_in), n_out / n_in, order=3)
    outside = ones == 0.0
    assert np.abs(w[~outside].sum(axis=1) - 1.0).max(initial=0.0) <= 1e-14
    assert not w[outside].any()
    assert outside.sum() == (1 if (n_in, n_out) == (512, 224) else 0)
    assert zoom_operator(n_in, n_out)[0] is w                        # cached per size pair


def test_operator_rejects_a_length_scipy_does_not_produce(monkeypatch):
    """scipy sizes its output as round(n_in * factor); no integer pair up to 200 makes that differ from n_out, so the refusal is
    shown on a zoom that returns one sample too many."""
    from cswin_unet_amd import utils
    assert all(int(round(a * (b / a))) == b for a in range(1, 200) for b in range(1, 200))
    monkeypatch.setattr(utils, "zoom", lambda x, f, order: zoom(x, f, order=order)[np.r_[0:13, 12]])
    with pytest.raises(ValueError):
        utils.zoom_operator.__wrapped__(11, 13)
    with pytest.raises(ValueError):
        utils.nearest_index.__wrapped__(11, 13)
    for fn in (utils.zoom_operator, utils.nearest_index):
        with pytest.raises(ValueError):
            fn(0, 4)


@pytest.mark.parametrize("hw,HW", [((224, 224), (512, 512)), ((512, 512), (224, 224)), ((224, 224), (37, 53)), ((37, 53), (224, 224)),
                                   ((40, 56), (64, 48)), ((64, 48), (40, 56)), ((32, 40), (20, 24)), ((20, 24), (32, 40)),
                                   ((224, 224), (224, 224)), ((5, 5), (7, 7)), ((7, 7), (5, 5)), ((1, 1), (1, 1))],
                         ids=lambda v: "x".join(map(str, v)))
def test_nearest_index_gather_equals_scipy_order0(hw, HW):
    from cswin_unet_amd.utils import nearest_index
    (h, w), (H, W) = hw, HW
    lab = np.random.default_rng(h * 1000 + W).integers(1, 9, size=(h, w))          # no 0: an ungathered output shows
    ih, iw = nearest_index(h, H), nearest_index(w, W)
    assert ih.dtype == np.int32 and ih.shape == (H,) and iw.shape == (W,)
    assert np.array_equal(gather_nearest(lab, ih, iw), zoom(lab, (H / h, W / w), order=0))
    if (h, H) != (512, 224):
        assert ih.min() >= 0 and iw.min() >= 0 and np.array_equal(lab[np.ix_(ih, iw)], zoom(lab, (H / h, W / w), order=0))
    if (h, w) == (H, W):
        assert np.array_equal(ih, np.arange(H))


def test_resize_argument_is_validated_and_defaults_to_host():
    from cswin_unet_amd import utils
    for fn in (utils.predict_volume, utils.test_single_volume, utils.evaluate_volumes):
        assert inspect.signature(fn).parameters["resize"].default == "host", fn.__name__
    assert inspect.signature(utils.predict_volume).parameters["return_device"].default is False
    net = lambda x: x          # noqa: E731  (never reached)
    with pytest.raises(ValueError):
        utils.predict_volume(np.zeros((2, 8, 8), np.float32), net, (8, 8), resize="gpu")
    with pytest.raises(ValueError):
        utils.predict_volume(np.zeros((2, 8, 8), np.float32), net, (8, 8), resize="host", return_device=True)
    import torch
    with pytest.raises(ValueError):
        utils.test_single_volume(torch.zeros(1, 2, 8, 8), torch.zeros(1, 2, 8, 8), net, 9, [8, 8], resize="device")


def test_ops_refuse_cpu_tensors_and_integer_volumes():
    import torch
    from cswin_unet_amd import ops
    from cswin_unet_amd._lib import CswinHipError
    with pytest.raises(CswinHipError):
        ops.resize_slices(torch.zeros(2, 8, 8), (4, 4))
    with pytest.raises(CswinHipError):
        ops.argmax_zoom_back(torch.zeros(1, 3, 4, 4), (8, 8))
