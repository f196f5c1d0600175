"""Device intensity augmentation (csrc/intensity.hip behind ops.intensity_batch, ops.gaussian_blur_each, the `intensity` of
trainer._Prefetcher and trainer_synapse) against utils.intensity_host, the definition, on the seeded inputs of
tests/intensity_cases.py.  Every device call is followed by a synchronize so that a failing step ends its test before anything
else is enqueued.

Criterion (intensity_cases.check): every element finite and within one float32 ulp of the definition's, at most 1 in 1e5 not
bit-equal.  The cap is a condition, not a measurement: the device evaluates the definition's float64 chain without contraction,
and differs from numpy only in the order of the whole-image sums and in the last bit of log, cos and pow, which
tests/test_intensity_host.py shows not to reach the float32 result; 0 is the expected count, and every case prints its own."""
import logging
import random
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import blur_cases as B
import intensity_cases as C
from cswin_unet_amd.datasets import IntensityAugment
from cswin_unet_amd.utils import intensity_noise_host

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _run(x, draws):
    from cswin_unet_amd import ops
    dx = torch.from_numpy(np.array(x, order="C")).to(DEV)
    y = ops.intensity_batch(dx, draws)
    torch.cuda.synchronize()
    assert y.dtype == torch.float32 and y.is_cuda and y.shape == dx.shape and y.is_contiguous()
    assert y.data_ptr() != dx.data_ptr() and torch.equal(dx.cpu(), torch.from_numpy(np.array(x, order="C")))      # the input is left alone
    return y.cpu().numpy()


@pytest.mark.parametrize("name", list(C.STAGE_SETS))
@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("shape", C.SHAPES, ids=C.shape_id)
def test_stages_equal_the_definition(shape, kind, name):
    got = _run(C.images(shape, kind), C.stage_draws(name, shape[0]))
    C.check(got, C.stage_reference(shape, kind, name), f"{C.shape_id(shape)} {kind} {name}")


@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("hw", [(5, 7), (40, 40), (64, 96), (224, 224)], ids=C.shape_id)
def test_a_batch_of_every_pattern_equals_the_definition(hw, kind):
    x, want = C.pattern_inputs(hw, kind)
    draws = C.pattern_draws()
    assert len(draws) == 48 and not any(draws[0][f] for f in ("do_blur", "do_noise", "do_brightness", "do_contrast", "do_gamma"))
    got = _run(x, draws)
    C.check(got, want, f"patterns {C.shape_id(hw)} {kind}")
    assert C.unequal_bits(got[0], x[0]) == 0                              # the all-off sample
    got4 = _run(x[:, None], draws)                                         # (B, 1, h, w)
    assert got4.shape == (48, 1) + tuple(hw) and C.unequal_bits(got4[:, 0], got) == 0


@pytest.mark.parametrize("shape", C.SHAPES, ids=C.shape_id)
def test_noise_on_a_zero_image_is_the_emulated_generator(shape):
    Bn, h, w = shape
    draws = C.batch_of([C.record(noise=1.0, seed=s) for s in [0, 2 ** 64 - 1, 0x123456789ABCDEF, 5, 6][:Bn]])
    got = _run(np.zeros(shape, np.float32), draws)
    want = np.stack([intensity_noise_host(d["seed"], h * w).reshape(h, w).astype(np.float32) for d in draws])
    C.check(got, want, f"noise {C.shape_id(shape)}")
    if Bn > 1:
        assert C.unequal_bits(got[0], got[1]) > 0                         # two seeds, two fields


def test_results_repeat_and_do_not_depend_on_the_batch():
    shape = (3, 224, 224)
    for kind in ("uniform", "pm1000"):
        x = C.images(shape, kind)
        draws = C.batch_of([C.record(seed=10 + b, **C.STAGE_SETS[n]) for b, n in enumerate(("all", "gamma_inverted", "contrast_up"))])
        a, b = _run(x, draws), _run(x, draws)
        assert C.unequal_bits(a, b) == 0
        for s in range(3):
            alone = _run(x[s:s + 1], draws[s:s + 1])
            assert C.unequal_bits(alone[0], a[s]) == 0, (kind, s)
        swapped = _run(x[::-1], draws[::-1])
        assert C.unequal_bits(swapped[::-1], a) == 0
        other = draws.copy()
        other["seed"][0] += 1
        c = _run(x, other)
        assert C.unequal_bits(c[0], a[0]) > 0 and C.unequal_bits(c[1:], a[1:]) == 0


def test_the_entry_point_replays_from_a_captured_graph():
    """cswin_intensity_batch with its table and workspace in place: no host synchronisation, no allocation, so its launches can
    be captured and replayed."""
    from cswin_unet_amd import ops
    from cswin_unet_amd._lib import call, lib, ptr, stream
    x = torch.from_numpy(np.array(C.images((4, 40, 40), "clipped"))).to(DEV)
    draws = C.stage_draws("all_inverted", 4)
    draws["do_blur"] = False
    want = ops.intensity_batch(x, draws)
    torch.cuda.synchronize()
    records, stages = ops._intensity_table(draws)
    assert stages == 12
    table = torch.from_numpy(records.view(np.int64).copy()).to(DEV)
    nbytes = lib().cswin_intensity_workspace(4, 1600)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=DEV)
    y = torch.zeros_like(x)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call("cswin_intensity_batch", ptr(x), ptr(y), ptr(table), ptr(ws), nbytes, 4, 1600, stages, stream())
    torch.cuda.synchronize()
    y.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, want)


# ---- gaussian_blur_each -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset"])
@pytest.mark.parametrize("shape", C.EACH_SHAPES, ids=C.shape_id)
def test_gaussian_blur_each(shape, offset):
    from cswin_unet_amd import ops
    x, want = C.each_inputs(shape)
    flat = torch.zeros(x.size + 1, device=DEV)
    flat[offset:offset + x.size] = torch.from_numpy(np.array(x)).to(DEV).reshape(-1)
    dx = flat[offset:offset + x.size].view(*shape)
    assert dx.data_ptr() % 8 == 4 * offset
    y = ops.gaussian_blur_each(dx, C.EACH_SIGMAS)
    torch.cuda.synchronize()
    assert y.dtype == torch.float32 and y.shape == dx.shape and y.data_ptr() != dx.data_ptr()
    got = y.cpu().numpy()
    for d, s in enumerate(C.EACH_SIGMAS):
        unequal = B.unequal_bits(got[d], want[d])
        ulps = C.max_ulps(got[d], want[d])
        print(f"{C.shape_id(shape)} slice {d} sigma {s}: {unequal} of {got[d].size} not bit-equal, max {ulps:.3g} ulp")
        assert np.isfinite(got[d]).all() and ulps <= 1.0 and unequal * 100000 <= got[d].size
        if s is None:
            assert B.unequal_bits(got[d], x[d]) == 0
        else:
            one = ops.gaussian_blur(dx[d:d + 1], s)
            torch.cuda.synchronize()
            assert torch.equal(one[0], y[d]), (d, s)
    none = ops.gaussian_blur_each(dx, [None] * shape[0])
    torch.cuda.synchronize()
    assert torch.equal(none, dx)


# ---- loader level -----------------------------------------------------------------------------------------------------------------
def _drain(train, lists, augment, intensity, seed=21):
    from torch.utils.data import DataLoader
    from cswin_unet_amd.datasets import RandomGenerator, RawSliceParams, Synapse_dataset, collate_raw_slices
    from cswin_unet_amd.trainer import _Prefetcher
    hip = augment == "hip"
    ds = Synapse_dataset(train, lists, "train", transform=(RawSliceParams if hip else RandomGenerator)([40, 40]))
    loader = DataLoader(ds, batch_size=4, shuffle=False, num_workers=0, pin_memory=True, drop_last=True,
                        collate_fn=collate_raw_slices if hip else None)
    random.seed(7)
    np.random.seed(8)
    out = []
    for img, lab in _Prefetcher(loader, torch.device(DEV), augment, (40, 40), intensity=intensity, intensity_seed=seed):
        torch.cuda.synchronize()
        assert img.dtype == torch.float32 and tuple(img.shape) == (4, 1, 40, 40)
        assert lab.dtype == torch.int64 and tuple(lab.shape) == (4, 40, 40)
        out.append((img.cpu().numpy(), lab.cpu().numpy()))
    return out


@pytest.mark.parametrize("augment", ["host", "hip"])
def test_prefetcher_applies_the_definition_to_its_batches(tmp_path, augment):
    from cswin_unet_amd.datasets import write_synthetic_synapse
    train, _, lists = write_synthetic_synapse(str(tmp_path), size=64, n_slices=8, n_volumes=0)
    spec = IntensityAugment(noise=(0.5, (0.0, 0.1)), blur=(0.5, (0.5, 1.0)), brightness=(0.5, (0.75, 1.25)), contrast=(0.5, (0.75, 1.25)),
                            gamma=(0.6, (0.7, 1.5)), p_invert=0.5)
    plain, again = _drain(train, lists, augment, None), _drain(train, lists, augment, None)
    aug = _drain(train, lists, augment, spec)
    assert len(plain) == len(aug) == 2
    rng = np.random.default_rng(21)                                        # the prefetcher's stream: one draw of 4 per batch
    for n, ((pimg, plab), (qimg, qlab), (aimg, alab)) in enumerate(zip(plain, again, aug)):
        assert C.unequal_bits(pimg, qimg) == 0 and np.array_equal(plab, qlab)
        assert np.array_equal(alab, plab)
        draws = spec.draw(4, rng)
        assert any(draws[f].any() for f in ("do_blur", "do_noise", "do_brightness", "do_contrast", "do_gamma"))
        C.check(aimg[:, 0], C.host_batch(pimg[:, 0], draws), f"{augment} batch {n}")


def test_trainer_synapse_with_intensity_augmentation(tmp_path):
    """The settings of test_gpu_augment.test_trainer_synapse_with_device_augmentation with intensity="nnunet", two steps."""
    from cswin_unet_amd.config import get_config
    from cswin_unet_amd.datasets import write_synthetic_synapse
    from cswin_unet_amd.networks.vision_transformer import CSwinUnet
    from cswin_unet_amd.trainer import trainer_synapse
    train, _, lists = write_synthetic_synapse(str(tmp_path / "data"), n_slices=8, n_volumes=0, size=256)
    cfg = get_config(**{"MODEL.DROP_PATH_RATE": 0.0})
    torch.manual_seed(0)
    net = CSwinUnet(cfg, img_size=224, num_classes=9).to(DEV)
    args = SimpleNamespace(root_path=train, list_dir=lists, img_size=224, num_classes=9, batch_size=4, base_lr=0.05,
                           max_epochs=1, num_workers=0, seed=1234, augment="hip", intensity="nnunet")
    records = []
    h = logging.Handler()
    h.emit = lambda r: records.append(r.getMessage())
    root = logging.getLogger()
    old_level = root.level
    root.setLevel(logging.INFO)
    root.addHandler(h)
    try:
        assert trainer_synapse(args, net, str(tmp_path / "snap")) == "Training Finished!"
    finally:
        root.removeHandler(h)
        root.setLevel(old_level)
    torch.cuda.synchronize()
    losses = [float(m.split("loss : ")[1].split(",")[0]) for m in records if m.startswith("iteration")]
    print("losses", losses)
    assert len(losses) == 2 and all(np.isfinite(v) for v in losses)


# ---- error paths ------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_raise_before_any_launch():
    from cswin_unet_amd import ops
    from cswin_unet_amd._lib import CswinHipError, lib, ptr, stream
    x = torch.full((2, 8, 8), 3.0, device=DEV)
    good = C.stage_draws("all", 2)
    with pytest.raises(CswinHipError):
        ops.intensity_batch(torch.zeros(2, 8, 8), good)
    for dtype in (torch.float64, torch.float16, torch.int16):
        with pytest.raises(CswinHipError):
            ops.intensity_batch(torch.zeros(2, 8, 8, dtype=dtype, device=DEV), good)
    with pytest.raises(CswinHipError):
        ops.intensity_batch(torch.zeros(8, 8, device=DEV), good)
    with pytest.raises(CswinHipError):
        ops.intensity_batch(torch.zeros(2, 3, 8, 8, device=DEV), good)
    with pytest.raises(ValueError):
        ops.intensity_batch(x, C.stage_draws("all", 3))
    with pytest.raises(ValueError):
        ops.intensity_batch(x, np.zeros((2, 12)))
    for bad in (C.record(gamma=0.0), C.record(gamma=-0.5), C.record(noise=-0.1), C.record(blur=8.2), C.record(contrast=np.inf)):
        with pytest.raises(ValueError):
            ops.intensity_batch(x, C.batch_of([C.record(), bad]))
    with pytest.raises(ValueError):
        IntensityAugment(noise=(0.1, (-0.1, 0.1)))
    with pytest.raises(ValueError):
        ops.gaussian_blur_each(x, [1.0])
    with pytest.raises(ValueError):
        ops.gaussian_blur_each(x, [1.0, 8.2])
    with pytest.raises(CswinHipError):
        ops.gaussian_blur_each(x.double(), [1.0, None])
    # the entry points themselves: a short workspace, unknown stage bits and an in-place blur are refused without a launch
    h = lib()
    y = torch.empty_like(x)
    table = torch.zeros(12, dtype=torch.int64, device=DEV)
    ws = torch.zeros(8, dtype=torch.float64, device=DEV)
    assert h.cswin_intensity_workspace(2, 64) == (2 * 64 + 2 * 9) * 8
    assert h.cswin_intensity_workspace(0, 64) == 0 and h.cswin_intensity_workspace(2, 2048 * 2048 + 1) == 0
    assert h.cswin_intensity_batch(ptr(x), ptr(y), ptr(table), ptr(ws), 64, 2, 64, 8, stream()) != 0
    assert b"workspace" in h.cswin_last_error()
    assert h.cswin_intensity_batch(ptr(x), ptr(y), ptr(table), None, 0, 2, 64, 3, stream()) != 0
    taps = torch.ones(1, dtype=torch.float64, device=DEV)
    each = torch.zeros(4, dtype=torch.int32, device=DEV)
    assert h.cswin_gaussian_blur_each(ptr(x), ptr(x), ptr(taps), 1, ptr(each), 0, 2, 8, 8, stream()) != 0
    assert b"in place" in h.cswin_last_error()
    assert h.cswin_gaussian_blur_each(ptr(x), ptr(y), ptr(taps), 1, ptr(each), 1, 2, 8, 8, stream()) != 0      # ntaps <= max_radius
    assert h.cswin_gaussian_blur_each(ptr(x), ptr(y), ptr(taps), 1, ptr(each), 33, 2, 8, 8, stream()) != 0
    torch.cuda.synchronize()
    assert bool((x == 3.0).all())
