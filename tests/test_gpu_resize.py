"""Device resizes of a volume evaluation (csrc/resize.hip behind ops.resize_slices / ops.argmax_zoom_back and
utils.predict_volume(resize="hip")) against scipy.ndimage.zoom and the host path, on the seeded inputs of
tests/test_resize_host.py.  Every device call is followed by a synchronize so that a failing step ends its test before anything
else is enqueued.

resize_slices: every element within one float32 ulp of scipy's and at most 1 in 1e5 not bit-equal.  The device sums the same
float64 products as the emulation of the CPU test (which leaves 0 unequal at these inputs) with fused multiply-adds and in its
own order, a relative difference of ~1e-15 before the one rounding to float32 (half-ulp 6e-8): the chance of landing on the
other side of a rounding boundary is ~2e-8 per element.  argmax_zoom_back and predict_volume are compared exactly."""
import numpy as np
import pytest
import torch
from scipy.ndimage import zoom

from oracle.determ import det_normal, fill_state_dict
from resize_cases import GPU_SHAPES, scipy_zoom3, slices
from seg_metrics_cases import blob_pair

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = dict(rel=1e-12, abs=1e-12)


def _resize(x, size):
    from cswin_unet_amd import ops
    y = ops.resize_slices(torch.from_numpy(x.copy()).to(DEV), size)
    torch.cuda.synchronize()
    assert y.dtype == torch.float32 and y.is_cuda and tuple(y.shape) == (x.shape[0],) + tuple(size)
    return y.cpu().numpy()


def _check_against_scipy(got, want, tag):
    want = want.astype(np.float32)
    unequal = int((got.view(np.uint32) != want.view(np.uint32)).sum())
    ulps = np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
    print(f"{tag}: {unequal} of {got.size} elements not bit-equal, max difference {float(ulps.max()):.3g} ulp")
    assert np.isfinite(got).all()
    assert float(ulps.max()) <= 1.0
    assert unequal * 100000 <= got.size, (unequal, got.size)


@pytest.mark.parametrize("shape,size,dtype", [(s, o, "float32") for s, o in GPU_SHAPES] + [(s, o, "float64") for s, o in GPU_SHAPES[:2]],
                         ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_resize_slices_equals_scipy_zoom(shape, size, dtype):
    got = _resize(slices(shape, size, dtype), size)
    _check_against_scipy(got, scipy_zoom3(shape, size, dtype), f"{shape} -> {size} {dtype}")


def test_resize_slices_of_a_strided_view_and_an_offset_base():
    """A view that is not contiguous is copied; an odd element offset of the base pointer takes the 4-B loads."""
    shape, size = GPU_SHAPES[0]
    x = slices(shape, size)
    from cswin_unet_amd import ops
    flat = torch.zeros(x.size + 1, device=DEV)
    flat[1:] = torch.from_numpy(x.copy()).to(DEV).reshape(-1)
    y = ops.resize_slices(flat[1:].view(*shape), size)
    torch.cuda.synchronize()
    _check_against_scipy(y.cpu().numpy(), scipy_zoom3(shape, size), "offset base")
    xt = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1))).to(DEV).transpose(1, 2)
    assert not xt.is_contiguous()
    y2 = ops.resize_slices(xt, size)
    torch.cuda.synchronize()
    assert torch.equal(y, y2)


def test_resize_slices_refuses_integers_and_cpu_tensors():
    from cswin_unet_amd import ops
    from cswin_unet_amd._lib import CswinHipError
    with pytest.raises(ValueError):
        ops.resize_slices(torch.zeros(2, 8, 8, dtype=torch.int16, device=DEV), (4, 4))
    with pytest.raises(CswinHipError):
        ops.resize_slices(torch.zeros(2, 8, 8), (4, 4))
    with pytest.raises(CswinHipError):
        ops.resize_slices(torch.zeros(2, 8, 8, dtype=torch.float16, device=DEV), (4, 4))
    with pytest.raises(CswinHipError):
        ops.resize_slices(torch.zeros(2049, 8, 8, device=DEV), (4, 4))           # more than 2048 slices in one call


# (h, w) -> (H, W); the last pair has outputs that scipy fills with its constant instead of gathering
ZOOM_BACK = [((40, 56), (64, 48)), ((224, 224), (512, 512)), ((32, 40), (20, 24)), ((40, 56), (40, 56)), ((512, 512), (224, 224))]


@pytest.mark.parametrize("hw,HW,ncls", [(a, b, n) for a, b in ZOOM_BACK for n in (2, 9, 200) if (a, n) != ((512, 512), 200)],
                         ids=lambda v: str(v) if isinstance(v, int) else "x".join(map(str, v)))
def test_argmax_zoom_back_equals_argmax_and_scipy_order0(hw, HW, ncls):
    from cswin_unet_amd import ops
    (h, w), (H, W) = hw, HW
    B = 2 if ncls * h * w <= 2 ** 21 else 1
    rng = np.random.default_rng(ncls * 7919 + h * 31 + W)
    logits = (np.round(rng.standard_normal((B, ncls, h, w)) * 4) / 4).astype(np.float32)          # multiples of 0.25: many ties
    if ncls == 9 and hw == (40, 56):
        logits[rng.random(logits.shape) < 0.02] = np.nan                                             # a NaN beats every number
        assert np.isnan(logits).any(axis=1).mean() > 0.1
    dl = torch.from_numpy(logits).to(DEV)
    got = ops.argmax_zoom_back(dl, (H, W))
    torch.cuda.synchronize()
    assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == (B, H, W)
    am = torch.argmax(dl, 1).cpu().numpy()
    ties = (logits == logits.max(axis=1, keepdims=True)).sum(axis=1) > 1
    assert ties.mean() > (0.02 if ncls > 2 else 0.05)
    for b in range(B):
        assert np.array_equal(got[b].cpu().numpy(), zoom(am[b], (H / h, W / w), order=0)), b


def test_argmax_zoom_back_bad_arguments_raise():
    from cswin_unet_amd import ops
    from cswin_unet_amd._lib import CswinHipError
    with pytest.raises(CswinHipError):
        ops.argmax_zoom_back(torch.zeros(1, 3, 4, 4), (8, 8))
    with pytest.raises(CswinHipError):
        ops.argmax_zoom_back(torch.zeros(1, 256, 4, 4, device=DEV), (8, 8))     # ncls above 255
    with pytest.raises(CswinHipError):
        ops.argmax_zoom_back(torch.zeros(3, 4, 4, device=DEV), (8, 8))


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


def test_predict_volume_hip_equals_host(net):
    from cswin_unet_amd import ops
    from cswin_unet_amd.utils import predict_volume
    vol = det_normal("resize.vol", VOL)
    # precondition, asserted: on this volume the device zoom is scipy's bit for bit, so both paths feed the network the same bits
    want = np.stack([zoom(s, (224 / VOL[1], 224 / VOL[2]), order=3) for s in vol])
    got = ops.resize_slices(torch.from_numpy(vol).to(DEV), (224, 224))
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.astype(np.float32).view(np.uint32))
    host = predict_volume(vol, net, (224, 224), batch_slices=2)
    hip = predict_volume(vol, net, (224, 224), batch_slices=2, resize="hip")
    torch.cuda.synchronize()
    assert hip.shape == host.shape == VOL and hip.dtype == np.uint8
    assert len(np.unique(host)) > 1
    assert np.array_equal(hip, host)
    dev = predict_volume(vol, net, (224, 224), batch_slices=2, resize="hip", return_device=True)
    torch.cuda.synchronize()
    assert isinstance(dev, torch.Tensor) and dev.is_cuda and dev.dtype == torch.uint8 and tuple(dev.shape) == VOL
    assert np.array_equal(dev.cpu().numpy(), host)
    one = predict_volume(vol[0], net, (224, 224), resize="hip")                  # a single (H, W) slice
    torch.cuda.synchronize()
    assert np.array_equal(one, predict_volume(vol[0], net, (224, 224)))


def test_predict_volume_hip_without_resizing(net):
    """Slices already at the network's size: identity indices, and integer volumes are accepted (nothing is zoomed)."""
    from cswin_unet_amd.utils import predict_volume
    vol = det_normal("resize.vol224", (3, 224, 224))
    host = predict_volume(vol, net, (224, 224))
    hip = predict_volume(vol, net, (224, 224), resize="hip")
    torch.cuda.synchronize()
    assert np.array_equal(hip, host)
    ints = np.rint(vol * 3).astype(np.int16)
    hip_i = predict_volume(ints, net, (224, 224), resize="hip")
    torch.cuda.synchronize()
    assert np.array_equal(hip_i, predict_volume(ints, net, (224, 224)))
    with pytest.raises(ValueError):
        predict_volume(ints[:, :64, :48], net, (224, 224), resize="hip")          # integer volumes are zoomed on the host only


def test_single_volume_hip_resize_and_metrics_equal_host(net, tmp_path):
    from cswin_unet_amd.utils import test_single_volume
    vol = det_normal("resize.vol", VOL)
    _, lab = blob_pair(VOL, [1, 2, 3, 4, 5, 6, 7, 8], 41)
    image, label = torch.from_numpy(vol)[None], torch.from_numpy(lab.astype(np.int64))[None]
    host = test_single_volume(image, label, net, classes=9, patch_size=[224, 224])
    hip = test_single_volume(image, label, net, classes=9, patch_size=[224, 224], resize="hip", metrics="hip",
                             test_save_path=str(tmp_path), case="case0")
    torch.cuda.synchronize()
    assert len(hip) == len(host) == 8
    for c, (g, w) in enumerate(zip(hip, host), start=1):
        print(f"class {c}: hip {g} host {w}")
        assert g[0] == w[0], (c, g, w)
        assert g[1] == pytest.approx(w[1], **TOL), (c, g, w)
    saved = np.load(tmp_path / "case0_pred.npz")
    assert saved["prediction"].shape == VOL and saved["prediction"].dtype == np.float32
    mixed = test_single_volume(image, label, net, classes=9, patch_size=[224, 224], resize="hip", metrics="host")
    assert mixed == host
