"""Host side of the Gaussian-blurred data path (no GPU): utils.gaussian_taps against scipy's impulse response, the reflect
rule, the numpy emulation of csrc/blur.hip against scipy.ndimage.gaussian_filter on the inputs of tests/test_gpu_blur.py (bit
for bit: the precondition of the cap that test holds the device to), and blur_sigma through RandomGenerator, predict_volume,
test_single_volume and evaluate_volumes."""
import random

import numpy as np
import pytest
import torch
from scipy.ndimage import gaussian_filter, gaussian_filter1d

import blur_cases as B


@pytest.mark.parametrize("sigma", [0.1, 0.5, 1, 1.7, 3, 8])
def test_gaussian_taps_are_scipys_impulse_response(sigma):
    from cswin_unet_amd.utils import gaussian_taps
    w, r = gaussian_taps(sigma)
    assert r == int(4.0 * sigma + 0.5) and w.shape == (2 * r + 1,) and w.dtype == np.float64
    assert np.array_equal(w, w[::-1])
    assert not w.flags.writeable and gaussian_taps(sigma)[0] is w
    impulse = np.zeros(4 * r + 3)
    impulse[2 * r + 1] = 1.0
    resp = gaussian_filter1d(impulse, sigma)
    assert np.array_equal(resp[r + 1:3 * r + 2], w)
    assert not resp[:r + 1].any() and not resp[3 * r + 2:].any()          # the window holds the whole response
    w2, r2 = gaussian_taps(sigma, truncate=2.0)
    assert r2 == int(2.0 * sigma + 0.5) and w2.shape == (2 * r2 + 1,)


@pytest.mark.parametrize("sigma", [0, -1, float("nan"), float("inf"), 9])
def test_gaussian_taps_refuse(sigma):
    from cswin_unet_amd.utils import gaussian_taps
    with pytest.raises(ValueError):
        gaussian_taps(sigma)


@pytest.mark.parametrize("n", [1, 2, 3, 7])
def test_reflect_rule_is_numpys_symmetric_padding(n):
    pad = 32
    want = np.pad(np.arange(n), pad, mode="symmetric")
    assert np.array_equal(B.reflect_index(np.arange(-pad, n + pad), n), want)


@pytest.mark.parametrize("shape,sigma", B.GPU_CASES, ids=B.case_id)
def test_emulation_is_bit_equal_to_scipy(shape, sigma):
    x = B.slices(shape, sigma)
    unequal = B.unequal_bits(B.emulate(x, sigma), B.scipy_blur_case(shape, sigma))
    print(f"{shape} sigma {sigma}: {unequal} of {x.size} elements not bit-equal")
    assert unequal == 0


def _sample(dtype=np.float32, shape=(48, 40)):
    rng = np.random.default_rng(31)
    img = rng.random(shape).astype(np.float32)
    if np.issubdtype(dtype, np.integer):
        img = np.rint(img * 1000).astype(dtype)
    lab = np.kron(rng.integers(0, 9, size=(shape[0] // 4, shape[1] // 4)), np.ones((4, 4), np.int64)).astype(np.float32)
    return img, lab


@pytest.mark.parametrize("seed", range(6))
def test_random_generator_blurs_before_its_transforms(seed):
    from cswin_unet_amd.datasets import RandomGenerator
    img, lab = _sample()

    def run(gen, image):
        random.seed(50 + seed)
        np.random.seed(60 + seed)
        out = gen({"image": image, "label": lab.copy()})
        return out, random.getstate(), np.random.get_state()

    got, rs, ns = run(RandomGenerator([32, 24], blur_sigma=1), img.copy())
    want, rs_w, ns_w = run(RandomGenerator([32, 24]), gaussian_filter(img, 1))
    plain, rs_p, ns_p = run(RandomGenerator([32, 24]), img.copy())
    assert torch.equal(got["image"], want["image"]) and torch.equal(got["label"], want["label"])
    assert not torch.equal(got["image"], plain["image"]) and torch.equal(got["label"], plain["label"])
    assert rs == rs_w == rs_p
    for a, b in ((ns, ns_w), (ns, ns_p)):
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def test_random_generator_draws_cover_every_branch():
    """The six seeds of the test above reach all three kinds."""
    from cswin_unet_amd.datasets import RawSliceParams
    img, lab = _sample()
    kinds = set()
    for seed in range(6):
        random.seed(50 + seed)
        np.random.seed(60 + seed)
        kinds.add(int(RawSliceParams([32, 24])({"image": img, "label": lab})["params"][0]))
    assert kinds == {0, 1, 2}


def test_random_generator_blurs_an_integer_image_as_float32():
    from cswin_unet_amd.datasets import RandomGenerator
    img, lab = _sample(np.int16)
    with B.scripted_draws((0, 0, 0, 0)):
        got = RandomGenerator([48, 40], blur_sigma=1)({"image": img, "label": lab})
    want = gaussian_filter(img.astype(np.float32), 1)
    assert got["image"].dtype == torch.float32 and np.array_equal(got["image"][0].numpy(), want)
    assert not np.array_equal(want, np.rint(want))                      # not scipy's rounded integer result


class StubNet(torch.nn.Module):
    """Class c where the pixel is nearest to the c-th of four levels: per-pixel, so a blur of the input moves the classes."""

    def forward(self, x):
        levels = torch.tensor([0.2, 0.4, 0.6, 0.8], dtype=x.dtype).view(1, 4, 1, 1)
        return -(x - levels) ** 2


def _volume(shape=(5, 40, 32)):
    vol = np.random.default_rng(77).random(shape).astype(np.float32)
    return vol


@pytest.mark.parametrize("patch", [(40, 32), (56, 48)], ids=["no_resize", "resize"])
def test_predict_volume_host_blurs_every_slice_with_scipy(patch):
    from cswin_unet_amd.utils import predict_volume
    vol, net = _volume(), StubNet()
    blurred = B.scipy_blur(vol, 1.0)
    got = predict_volume(vol, net, patch, batch_slices=2, device="cpu", blur_sigma=1.0)
    want = predict_volume(blurred, net, patch, batch_slices=2, device="cpu")
    plain = predict_volume(vol, net, patch, batch_slices=2, device="cpu")
    assert got.shape == vol.shape and np.array_equal(got, want)
    assert not np.array_equal(got, plain) and len(np.unique(got)) > 1
    assert np.array_equal(predict_volume(vol, net, patch, batch_slices=2, device="cpu", blur_sigma=None), plain)
    one = predict_volume(vol[0], net, patch, device="cpu", blur_sigma=1.0)
    assert np.array_equal(one, want[0])
    with pytest.raises(ValueError):
        predict_volume(vol, net, patch, device="cpu", blur_sigma=0)
    with pytest.raises(ValueError):
        predict_volume(vol, net, patch, device="cpu", blur_sigma=9)


def test_predict_volume_host_blurs_in_the_volumes_own_dtype():
    from cswin_unet_amd.utils import predict_volume
    vol, net = _volume().astype(np.float64), StubNet()
    got = predict_volume(vol, net, (40, 32), device="cpu", blur_sigma=1.0)
    assert np.array_equal(got, predict_volume(B.scipy_blur(vol, 1.0), net, (40, 32), device="cpu"))


def test_single_volume_and_evaluate_volumes_forward_blur_sigma(tmp_path):
    from cswin_unet_amd.utils import evaluate_volumes, test_single_volume
    vol, net = _volume(), StubNet()
    lab = (np.arange(vol.size).reshape(vol.shape) // 7 % 4).astype(np.int64)
    image, label = torch.from_numpy(vol)[None], torch.from_numpy(lab)[None]
    blurred = torch.from_numpy(B.scipy_blur(vol, 1.0))[None]
    kw = dict(classes=4, patch_size=[56, 48], device="cpu", metrics="host")
    got = test_single_volume(image, label, net, blur_sigma=1.0, test_save_path=str(tmp_path), case="c0", **kw)
    want = test_single_volume(blurred, label, net, **kw)
    plain = test_single_volume(image, label, net, **kw)
    assert got == want and got != plain
    assert np.array_equal(np.load(tmp_path / "c0_pred.npz")["image"], vol)          # the saved image is the one passed in
    loader = [{"image": image, "label": label, "case_name": "c0"}]
    ev = evaluate_volumes(loader, net, 4, (56, 48), metrics="host", device="cpu", blur_sigma=1.0)
    assert ev[0] == [want]
    assert evaluate_volumes(loader, net, 4, (56, 48), metrics="host", device="cpu")[0] == [plain]


@pytest.mark.parametrize("sigma", [0, -1.0, float("nan"), 9])
def test_trainer_synapse_refuses_a_bad_sigma_before_it_reads_anything(sigma, tmp_path):
    from types import SimpleNamespace
    from cswin_unet_amd.trainer import trainer_synapse
    snap = tmp_path / "snap"
    with pytest.raises(ValueError, match="gaussian_taps"):
        trainer_synapse(SimpleNamespace(blur_sigma=sigma, augment="hip"), None, str(snap))          # no dataset, no model
    assert not snap.exists()
