"""Device Gaussian blur (csrc/blur.hip behind ops.gaussian_blur, the blur_sigma of ops.augment_batch, trainer._Prefetcher and
utils.predict_volume(resize="hip")) against scipy.ndimage.gaussian_filter and the host paths, on the seeded inputs of
tests/test_blur_host.py.  Every device call is followed by a synchronize so that a failing step ends its test before anything
else is enqueued.

gaussian_blur: every element finite and within one float32 ulp of scipy's, at most 1 in 1e5 not bit-equal (the criterion of
tests/test_gpu_resize.py).  The cap is a condition, not a measurement: the device does scipy's float64 operations in scipy's
order without contraction, the numpy emulation of exactly that leaves 0 elements unequal on every case (tests/test_blur_host.py),
and 0 is the expected device count as well; the count of every case is printed."""
import random

import numpy as np
import pytest
import torch
from scipy.ndimage import gaussian_filter, zoom

import augment_cases as A
import blur_cases as B
from oracle.determ import det_normal, fill_state_dict
from seg_metrics_cases import blob_pair

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = dict(rel=1e-12, abs=1e-12)


def _blur(x, sigma):
    from cswin_unet_amd import ops
    y = ops.gaussian_blur(torch.from_numpy(x.copy()).to(DEV), sigma)
    torch.cuda.synchronize()
    assert y.dtype == torch.float32 and y.is_cuda and tuple(y.shape) == x.shape and y.is_contiguous()
    return y.cpu().numpy()


def _check_against_scipy(got, want, tag):
    unequal = B.unequal_bits(got, want)
    ulps = np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
    print(f"{tag}: {unequal} of {got.size} elements not bit-equal, max difference {float(ulps.max()):.3g} ulp")
    assert np.isfinite(got).all()
    assert float(ulps.max()) <= 1.0
    assert unequal * 100000 <= got.size, (unequal, got.size)


@pytest.mark.parametrize("shape,sigma", B.GPU_CASES, ids=B.case_id)
def test_gaussian_blur_equals_scipy_gaussian_filter(shape, sigma):
    got = _blur(B.slices(shape, sigma), sigma)
    _check_against_scipy(got, B.scipy_blur_case(shape, sigma), f"{shape} sigma {sigma}")


def test_gaussian_blur_of_an_offset_base_and_a_transposed_view():
    """An odd element offset of the base pointer takes the 4-B loads; a view that is not contiguous is copied."""
    from cswin_unet_amd import ops
    shape, sigma = B.GPU_CASES[4]
    x = B.slices(shape, sigma)
    dx = torch.from_numpy(x.copy()).to(DEV)
    want = ops.gaussian_blur(dx, sigma)
    torch.cuda.synchronize()
    _check_against_scipy(want.cpu().numpy(), B.scipy_blur_case(shape, sigma), "plain")
    flat = torch.zeros(x.size + 1, device=DEV)
    flat[1:] = dx.reshape(-1)
    view = flat[1:].view(*shape)
    assert view.data_ptr() % 8 == 4
    got = ops.gaussian_blur(view, sigma)
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    xt = dx.transpose(1, 2).contiguous().transpose(1, 2)
    assert not xt.is_contiguous()
    got = ops.gaussian_blur(xt, sigma)
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    assert torch.equal(dx.cpu(), torch.from_numpy(x.copy()))             # the input is left as it was


def test_gaussian_blur_bad_arguments_raise():
    from cswin_unet_amd import ops
    from cswin_unet_amd._lib import CswinHipError, lib, ptr, stream
    from cswin_unet_amd.utils import gaussian_taps_device
    with pytest.raises(CswinHipError):
        ops.gaussian_blur(torch.zeros(2, 8, 8), 1)
    with pytest.raises(CswinHipError):
        ops.gaussian_blur(torch.zeros(2, 8, 8, dtype=torch.float64, device=DEV), 1)
    with pytest.raises(CswinHipError):
        ops.gaussian_blur(torch.zeros(2, 8, 8, dtype=torch.float16, device=DEV), 1)
    with pytest.raises(ValueError, match="host"):
        ops.gaussian_blur(torch.zeros(2, 8, 8, dtype=torch.int16, device=DEV), 1)
    with pytest.raises(CswinHipError):
        ops.gaussian_blur(torch.zeros(8, 8, device=DEV), 1)
    with pytest.raises(ValueError):
        ops.gaussian_blur(torch.zeros(2, 8, 8, device=DEV), 0)
    with pytest.raises(ValueError):
        ops.gaussian_blur(torch.zeros(2, 8, 8, device=DEV), 9)
    with pytest.raises(CswinHipError, match="1..2048"):
        ops.gaussian_blur(torch.zeros(2049, 8, 8, device=DEV), 1)
    # the entry point itself: in place is refused before anything is launched, and so is a radius above 32
    x = torch.full((2, 8, 8), 3.0, device=DEV)
    taps, r = gaussian_taps_device(1.0, 4.0, x.device)
    h = lib()
    assert h.cswin_gaussian_blur(ptr(x), ptr(x), ptr(taps), r, 2, 8, 8, stream()) != 0
    assert b"in place" in h.cswin_last_error()
    y = torch.empty_like(x)
    assert h.cswin_gaussian_blur(ptr(x), ptr(y), ptr(taps), 33, 2, 8, 8, stream()) != 0
    torch.cuda.synchronize()
    assert bool((x == 3.0).all())


# ---- augment_batch with blur ------------------------------------------------------------------------------------------
AUG_SHAPES = [((64, 64), (40, 40)), ((64, 48), (40, 56))]


def _host_generator(image, label, params, size, blur_sigma):
    """RandomGenerator(size, blur_sigma) on one sample with its draws coming out as `params`."""
    from cswin_unet_amd.datasets import RandomGenerator
    with B.scripted_draws(params):
        out = RandomGenerator(list(size), blur_sigma=blur_sigma)({"image": image, "label": label})
    return out["image"][0].numpy(), out["label"].numpy()


@pytest.mark.parametrize("shape,size", AUG_SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_augment_batch_with_blur(shape, size):
    from cswin_unet_amd import ops
    img, lab = A.batch14(shape)
    dimg, dlab = torch.from_numpy(img.copy()).to(DEV), torch.from_numpy(lab.copy()).to(DEV)
    par = torch.tensor(A.PARAMS14, dtype=torch.int32)
    got_img, got_lab = ops.augment_batch(dimg, dlab, par, size, blur_sigma=1.0)
    torch.cuda.synchronize()
    blurred = ops.gaussian_blur(dimg, 1.0)
    torch.cuda.synchronize()
    two_img, two_lab = ops.augment_batch(blurred, dlab, par, size)
    torch.cuda.synchronize()
    assert torch.equal(got_img, two_img) and torch.equal(got_lab, two_lab)
    assert tuple(got_img.shape) == (14, 1) + size and got_img.dtype == torch.float32 and got_lab.dtype == torch.int64
    gi, gl = got_img[:, 0].cpu().numpy(), got_lab.cpu().numpy()
    for b, p in enumerate(A.PARAMS14):
        want_img, want_lab = _host_generator(img[b].copy(), lab[b].copy(), p, size, 1.0)
        assert np.array_equal(gl[b], want_lab), (shape, p)
        A.check_image(gi[b], want_img, float(np.abs(gaussian_filter(img[b], 1.0)).max()), f"{shape} -> {size} {p} blurred")
    # None is the call without the argument
    none_img, none_lab = ops.augment_batch(dimg, dlab, par, size, blur_sigma=None)
    torch.cuda.synchronize()
    plain_img, plain_lab = ops.augment_batch(dimg, dlab, par, size)
    torch.cuda.synchronize()
    assert torch.equal(none_img, plain_img) and torch.equal(none_lab, plain_lab)
    assert not torch.equal(none_img, got_img) and torch.equal(none_lab, got_lab)


# ---- predict_volume ---------------------------------------------------------------------------------------------------
class _OneChannel(torch.nn.Module):          # CSwinUnet.forward: 1 -> 3 channels (vision_transformer.py:40-41)
    def __init__(self, m):
        super().__init__()
        self.m = m

    def forward(self, x):
        return self.m(x.repeat(1, 3, 1, 1))


@pytest.fixture(scope="module")
def net():
    import cswin_unet_amd.networks.cswin_unet as N
    m = N.CSWinTransformer(img_size=224, num_classes=9, embed_dim=64, depth=[1, 2, 9, 1], split_size=[1, 2, 7, 7],
                           num_heads=[2, 4, 8, 16], mlp_ratio=4., qkv_bias=True, drop_path_rate=0.).to(DEV)
    return _OneChannel(fill_state_dict(m)).eval()


VOL = (5, 64, 48)


def test_predict_volume_hip_with_blur_equals_host(net):
    from cswin_unet_amd import ops
    from cswin_unet_amd.utils import predict_volume
    vol = det_normal("resize.vol", VOL)
    # precondition, asserted: on this volume blur + zoom on the device are scipy's two steps bit for bit
    want = np.stack([zoom(gaussian_filter(s, 1.0), (224 / VOL[1], 224 / VOL[2]), order=3) for s in vol])
    got = ops.resize_slices(ops.gaussian_blur(torch.from_numpy(vol).to(DEV), 1.0), (224, 224))
    torch.cuda.synchronize()
    assert B.unequal_bits(got.cpu().numpy(), want) == 0
    host = predict_volume(vol, net, (224, 224), batch_slices=2, blur_sigma=1.0)
    hip = predict_volume(vol, net, (224, 224), batch_slices=2, resize="hip", blur_sigma=1.0)
    torch.cuda.synchronize()
    assert hip.shape == host.shape == VOL and hip.dtype == np.uint8
    assert len(np.unique(host)) > 1
    assert np.array_equal(hip, host)
    assert not np.array_equal(host, predict_volume(vol, net, (224, 224), batch_slices=2))
    dev = predict_volume(vol, net, (224, 224), batch_slices=2, resize="hip", return_device=True, blur_sigma=1.0)
    torch.cuda.synchronize()
    assert isinstance(dev, torch.Tensor) and dev.is_cuda and dev.dtype == torch.uint8 and tuple(dev.shape) == VOL
    assert np.array_equal(dev.cpu().numpy(), host)
    one = predict_volume(vol[0], net, (224, 224), resize="hip", blur_sigma=1.0)  # a single (H, W) slice
    torch.cuda.synchronize()
    assert np.array_equal(one, predict_volume(vol[0], net, (224, 224), blur_sigma=1.0))
    with pytest.raises(ValueError, match='resize="host"'):
        predict_volume(vol.astype(np.float64), net, (224, 224), resize="hip", blur_sigma=1.0)


def test_predict_volume_hip_with_blur_without_resizing(net):
    from cswin_unet_amd.utils import predict_volume
    vol = det_normal("resize.vol224", (2, 224, 224))
    host = predict_volume(vol, net, (224, 224), blur_sigma=1.0)
    hip = predict_volume(vol, net, (224, 224), resize="hip", blur_sigma=1.0)
    torch.cuda.synchronize()
    assert np.array_equal(hip, host)


def test_single_volume_hip_with_blur_equals_host(net):
    from cswin_unet_amd.utils import test_single_volume
    vol = det_normal("resize.vol", VOL)
    _, lab = blob_pair(VOL, [1, 2, 3, 4, 5, 6, 7, 8], 41)
    image, label = torch.from_numpy(vol)[None], torch.from_numpy(lab.astype(np.int64))[None]
    host = test_single_volume(image, label, net, classes=9, patch_size=[224, 224], blur_sigma=1.0)
    hip = test_single_volume(image, label, net, classes=9, patch_size=[224, 224], resize="hip", metrics="hip", blur_sigma=1.0)
    torch.cuda.synchronize()
    assert len(hip) == len(host) == 8
    for c, (g, w) in enumerate(zip(hip, host), start=1):
        print(f"class {c}: hip {g} host {w}")
        assert g[0] == w[0], (c, g, w)
        assert g[1] == pytest.approx(w[1], **TOL), (c, g, w)


# ---- loader level -----------------------------------------------------------------------------------------------------
def _drain(train, lists, augment):
    from torch.utils.data import DataLoader
    from cswin_unet_amd.datasets import RandomGenerator, RawSliceParams, Synapse_dataset, collate_raw_slices
    from cswin_unet_amd.trainer import _Prefetcher
    hip = augment == "hip"
    ds = Synapse_dataset(train, lists, "train", transform=RawSliceParams([40, 40]) if hip else RandomGenerator([40, 40], blur_sigma=1.0))
    loader = DataLoader(ds, batch_size=4, shuffle=False, num_workers=0, pin_memory=True, drop_last=True,
                        collate_fn=collate_raw_slices if hip else None)
    random.seed(7)
    np.random.seed(8)
    out = []
    for img, lab in _Prefetcher(loader, torch.device(DEV), augment, (40, 40), blur_sigma=1.0):
        torch.cuda.synchronize()
        assert img.dtype == torch.float32 and tuple(img.shape) == (4, 1, 40, 40)
        assert lab.dtype == torch.int64 and tuple(lab.shape) == (4, 40, 40)
        out.append((img.cpu().numpy(), lab.cpu().numpy()))
    return out


def test_prefetcher_hip_blurred_batches_equal_the_host_batches(tmp_path):
    from cswin_unet_amd.datasets import Synapse_dataset, write_synthetic_synapse
    train, _, lists = write_synthetic_synapse(str(tmp_path), size=64, n_slices=8, n_volumes=0)
    raw = Synapse_dataset(train, lists, "train")
    host, hip = _drain(train, lists, "host"), _drain(train, lists, "hip")
    assert len(host) == len(hip) == 2
    for n, ((himg, hlab), (dimg, dlab)) in enumerate(zip(host, hip)):
        assert np.array_equal(dlab, hlab), n
        for b in range(4):
            blurred = gaussian_filter(raw[4 * n + b]["image"], 1.0)
            A.check_image(dimg[b, 0], himg[b, 0], float(np.abs(blurred).max()), f"batch {n} sample {b}")
