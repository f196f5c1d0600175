"""CPU checks of the intensity augmentation: the definition utils.intensity_host, its generator, the draws of
datasets.IntensityAugment, the tables of ops.gaussian_blur_each in the numpy emulation of tests/blur_cases.py, and the argument
checks that need no device.  The device is held to the definition by tests/test_gpu_intensity.py."""
import random
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import blur_cases as B
import intensity_cases as C
from cswin_unet_amd.datasets import INTENSITY_DRAW, IntensityAugment, check_intensity_draws
from cswin_unet_amd.utils import intensity_host, intensity_noise_host, mix64_host

X = C.images((3, 17, 23), "uniform")


# ---- the definition ---------------------------------------------------------------------------------------------------------------
def test_all_off_returns_the_image_bit_for_bit():
    for kind in C.KINDS:
        x = C.images((3, 17, 23), kind)[0]
        y = intensity_host(x, C.record(seed=5))
        assert y.dtype == np.float32 and C.unequal_bits(y, x) == 0
    special = np.array([[0.0, -0.0, 1e-45, -3.4e38]], np.float32)
    assert C.unequal_bits(intensity_host(special, C.record()), special) == 0


def test_brightness_alone_is_one_float64_product():
    for b in (0.75, 1.0, 1.2345678):
        want = (X[0].astype(np.float64) * b).astype(np.float32)
        assert C.unequal_bits(intensity_host(X[0], C.record(brightness=b)), want) == 0


@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("c", [0.75, 1.25, 3.0])
def test_contrast_stays_inside_the_input_range(kind, c):
    x = C.images((3, 17, 23), kind)[1]
    y = intensity_host(x, C.record(contrast=c))
    assert y.min() >= x.min() and y.max() <= x.max()


@pytest.mark.parametrize("kind", C.KINDS[:3])
@pytest.mark.parametrize("g,invert", [(0.7, False), (1.5, False), (1.5, True), (0.9, True)])
def test_gamma_keeps_mean_and_deviation(kind, g, invert):
    """To 1e-9 relative, in float64 before the final rounding.  The mean is kept as it is.  The deviation is kept up to the 1e-8
    that the definition adds to the divisor: with s1 the deviation after the power the result has s0 s1 / (s1 + 1e-8), which is
    within 1e-9 of s0 where s1 >= 10 (the +-1000 inputs: asserted as such) and 3.5e-8 off for images in [0, 1], where s1 is
    some 0.28; there the law itself is asserted to 1e-9, so nothing but that epsilon moves the deviation."""
    x = C.images((3, 17, 23), kind)[2]
    d = C.record(gamma=g, invert=invert)
    z, s1 = _chain64(x, d)
    z0 = x.astype(np.float64)
    assert z.mean() == pytest.approx(z0.mean(), rel=1e-9, abs=1e-9 * z0.std())
    assert z.std() == pytest.approx(z0.std() * s1 / (s1 + 1e-8), rel=1e-9)
    if kind == "pm1000":
        assert s1 >= 10 and z.std() == pytest.approx(z0.std(), rel=1e-9)
    assert C.unequal_bits(z.astype(np.float32), intensity_host(x, d)) == 0
    assert not np.array_equal(z.astype(np.float32), x)


def _chain64(x, d):
    """The gamma stage of the definition without the final rounding, and the deviation after its power (a transcription kept
    beside the property it serves)."""
    z = x.astype(np.float64)
    z = -z if d["invert"] else z
    m0, s0, lo = z.mean(), z.std(), z.min()
    rng = z.max() - lo
    z = ((z - lo) / (rng + 1e-7)) ** float(d["gamma"]) * rng + lo
    s1 = z.std()
    z = (z - z.mean()) / (s1 + 1e-8) * s0 + m0
    return (-z if d["invert"] else z), s1


@pytest.mark.parametrize("g", [0.7, 1.3])
def test_inverted_gamma_is_minus_the_plain_stage_on_minus_x(g):
    for kind in C.KINDS[:3]:
        x = C.images((3, 17, 23), kind)[0]
        a = intensity_host(x, C.record(gamma=g, invert=True))
        b = -intensity_host(-x, C.record(gamma=g))
        assert C.unequal_bits(a, b) == 0


def test_constant_and_single_pixel_images_stay_finite():
    for x in (np.full((9, 11), 0.3, np.float32), np.full((1, 1), -7.5, np.float32), np.zeros((4, 4), np.float32)):
        for name, kw in C.STAGE_SETS.items():
            y = intensity_host(x, C.record(seed=3, **kw))
            assert y.shape == x.shape and np.isfinite(y).all(), (x.shape, name)
            if "noise" not in kw:
                assert np.allclose(y, x * kw.get("brightness", 1.0), rtol=1e-6, atol=1e-6), (x.shape, name)


def test_definition_rejects_what_it_does_not_take():
    with pytest.raises(ValueError):
        intensity_host(X[0].astype(np.float64), C.record())
    with pytest.raises(ValueError):
        intensity_host(X, C.record())
    with pytest.raises(ValueError):
        intensity_host(X[0], np.zeros(1, np.float64))
    for bad in (C.record(gamma=0.0), C.record(gamma=-1.0), C.record(noise=-0.1), C.record(blur=9.0), C.record(blur=0.0),
                C.record(brightness=np.nan)):
        with pytest.raises(ValueError):
            intensity_host(X[0], bad)


def test_two_evaluations_agree_after_rounding():
    """Stages 2-5 in float64 with forward sums against 80-bit long double with reversed sums on 200 random cases: the order of
    the whole-image sums and the last bits of the intermediate values do not reach the float32 result (0 elements differed when
    this was written; the assertion is the criterion's cap), and the definition itself -- numpy's pairwise sums -- agrees too."""
    total = unequal = unequal_def = 0
    for k in range(200):
        x, d = C.random_case(k)
        a = C.chain(x, d, np.float64, C.forward_sum)
        b = C.chain(x, d, np.longdouble, C.reversed_sum)
        ref = intensity_host(x, d)
        assert np.isfinite(a).all() and C.max_ulps(a, b) <= 1.0 and C.max_ulps(a, ref) <= 1.0, k
        total, unequal, unequal_def = total + x.size, unequal + C.unequal_bits(a, b), unequal_def + C.unequal_bits(a, ref)
    print(f"{unequal} (two evaluations) and {unequal_def} (against the definition) of {total} elements not bit-equal")
    assert total > 2_000_000
    assert unequal * 100000 <= total and unequal_def * 100000 <= total


# ---- the generator ----------------------------------------------------------------------------------------------------------------
def test_generator_values_are_pinned():
    assert int(mix64_host(np.uint64(0))) == 0xE220A8397B1DCDAF           # splitmix64's first output from state 0
    words = {0: [0xA706DD2F4D197E6F, 0x08B4FDA8C892B50E, 0xD7CC9674FF5FFA39, 0xC810565020D09481],
             0x123456789ABCDEF: [0x021C88D0A3FD73B6, 0xD414ADF34261BD2A, 0x146A7B4E39D42A16, 0x82C1C9DB8365803D]}
    normals = {0: [0.36824708, -1.40286537, -0.56333267, -0.27075906],
               0x123456789ABCDEF: [1.23027551, 0.58377804, -0.76937235, 0.72461251]}
    for seed, want in words.items():
        r = mix64_host(mix64_host(np.uint64(seed)) ^ np.arange(4, dtype=np.uint64))
        assert [int(v) for v in r] == want
        u1 = np.array([(w >> 40) + 1 for w in want]) / 2.0 ** 24
        u2 = np.array([(w >> 16) & 0xFFFFFF for w in want]) / 2.0 ** 24
        assert np.all((u1 > 0) & (u1 <= 1) & (u2 >= 0) & (u2 < 1))
        got = intensity_noise_host(seed, 4)
        assert got.dtype == np.float64
        assert np.allclose(got, np.sqrt(-2 * np.log(u1)) * np.cos(2 * np.pi * u2), rtol=1e-14, atol=0)
        assert np.allclose(got, normals[seed], rtol=0, atol=5e-9)
    assert np.array_equal(intensity_noise_host(9, 100)[:10], intensity_noise_host(9, 10))     # a function of (seed, i) alone


@pytest.mark.parametrize("seed", [1, 2 ** 64 - 1])
def test_generator_moments(seed):
    n = 1 << 20
    z = intensity_noise_host(seed, n)
    assert np.isfinite(z).all()
    assert abs(z.mean()) <= 5 / np.sqrt(n)
    assert abs(z.var() - 1) <= 5 * np.sqrt(2 / n)


# ---- the draws --------------------------------------------------------------------------------------------------------------------
def test_draws_repeat_and_lie_in_their_ranges():
    spec = IntensityAugment.nnunet()
    a = spec.draw(4000, np.random.default_rng(3))
    b = spec.draw(4000, np.random.default_rng(3))
    assert a.dtype == INTENSITY_DRAW and a.shape == (4000,) and a.tobytes() == b.tobytes()
    assert a.tobytes() != spec.draw(4000, np.random.default_rng(4)).tobytes()
    check_intensity_draws(a, 4000)
    for flag, field, lo, hi, p in (("do_blur", "sigma", 0.5, 1.0, 0.2), ("do_noise", "noise_std", 0.0, np.sqrt(0.1), 0.1),
                                   ("do_brightness", "brightness", 0.75, 1.25, 0.15), ("do_contrast", "contrast", 0.75, 1.25, 0.15),
                                   ("do_gamma", "gamma", 0.7, 1.5, 0.3)):
        on = a[flag]
        assert abs(on.mean() - p) < 5 * np.sqrt(p * (1 - p) / len(a)), flag
        assert np.all((a[field][on] >= lo) & (a[field][on] <= hi)), field
        neutral = 0.0 if field in ("sigma", "noise_std") else 1.0
        assert np.all(a[field][~on] == neutral), field
    assert not np.any(a["invert"] & ~a["do_gamma"])
    assert abs(a["invert"][a["do_gamma"]].mean() - 0.25) < 0.06
    assert len(np.unique(a["seed"])) == len(a) and a["seed"].max() > 2 ** 63
    assert len(spec.draw(0, np.random.default_rng(0))) == 0
    # a batch is a prefix-independent function of the generator's state: two draws of 2 are not one draw of 4, but repeat
    g1, g2 = np.random.default_rng(5), np.random.default_rng(5)
    assert np.concatenate([spec.draw(2, g1), spec.draw(2, g1)]).tobytes() == np.concatenate([spec.draw(2, g2), spec.draw(2, g2)]).tobytes()


def test_draws_leave_the_global_generators_alone():
    random.seed(11)
    np.random.seed(12)
    s1, s2 = random.getstate(), np.random.get_state()
    IntensityAugment.nnunet().draw(64, np.random.default_rng(0))
    assert random.getstate() == s1
    t2 = np.random.get_state()
    assert s2[0] == t2[0] and np.array_equal(s2[1], t2[1]) and s2[2:] == t2[2:]
    with pytest.raises(ValueError):
        IntensityAugment.nnunet().draw(4, np.random)
    with pytest.raises(ValueError):
        IntensityAugment.nnunet().draw(4, None)


@pytest.mark.parametrize("bad", [
    dict(noise=(1.5, (0.0, 0.1))), dict(noise=(-0.1, (0.0, 0.1))), dict(noise=(0.1, (-0.01, 0.1))), dict(noise=(0.1, (0.2, 0.1))),
    dict(blur=(0.2, (0.0, 1.0))), dict(blur=(0.2, (0.5, 8.2))), dict(blur=(0.2, (0.5, np.inf))), dict(blur=(2.0, (0.5, 1.0))),
    dict(brightness=(0.5, (1.25, 0.75))), dict(brightness=(0.5, (np.nan, 1.0))), dict(contrast=(1.01, (0.75, 1.25))),
    dict(gamma=(0.3, (0.0, 1.5))), dict(gamma=(0.3, (-0.5, 1.5))), dict(gamma=(0.3, 1.5)), dict(gamma="often"),
    dict(p_invert=1.5), dict(p_invert=-0.1),
])
def test_bad_specs_raise_at_construction(bad):
    with pytest.raises(ValueError):
        IntensityAugment(**bad)


def test_preset_and_default_spec():
    spec = IntensityAugment.nnunet()
    assert spec.stages == dict(noise=(0.1, 0.0, 0.1), blur=(0.2, 0.5, 1.0), brightness=(0.15, 0.75, 1.25), contrast=(0.15, 0.75, 1.25),
                               gamma=(0.3, 0.7, 1.5)) and spec.p_invert == 0.25
    off = IntensityAugment().draw(16, np.random.default_rng(0))
    assert not any(off[f].any() for f in ("do_blur", "do_noise", "do_brightness", "do_contrast", "do_gamma", "invert"))
    always = IntensityAugment(gamma=(1.0, (0.9, 0.9)), p_invert=1.0).draw(8, np.random.default_rng(0))
    assert always["do_gamma"].all() and always["invert"].all() and np.all(always["gamma"] == 0.9)


# ---- gaussian_blur_each's tables in the emulation ---------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", C.EACH_SHAPES, ids=C.shape_id)
def test_blur_each_emulation_equals_scipy_per_slice(shape):
    from cswin_unet_amd import ops
    from cswin_unet_amd.utils import gaussian_taps
    x, want = C.each_inputs(shape)
    table, taps = ops._blur_each_tables(C.EACH_SIGMAS)
    assert table.dtype == np.int32 and table.shape == (5, 2) and taps.dtype == np.float64
    assert table[:, 1].tolist() == [0, 2, 4, 3, 8] and table[0].tolist() == [0, 0] and taps[0] == 1.0
    for d, s in enumerate(C.EACH_SIGMAS[1:], start=1):
        w, r = gaussian_taps(s)
        assert np.array_equal(taps[table[d, 0]:table[d, 0] + r + 1], w[:r + 1])
    assert len(taps) == 1 + 3 + 5 + 4 + 9
    got = C.emulate_each(x, table, taps, int(table[:, 1].max()))
    assert C.unequal_bits(got[0], x[0]) == 0                               # the None slice
    for d, s in enumerate(C.EACH_SIGMAS):
        assert B.unequal_bits(got[d], want[d]) == 0, (d, s)
        if s is not None:
            assert B.unequal_bits(got[d], B.emulate(x[d:d + 1], s)[0]) == 0
    # equal sigmas share their taps; the packed buffer holds the int32 pairs in its first D float64 words
    t2, w2 = ops._blur_each_tables([1.0, None, 1.0, 1.0])
    assert t2.tolist() == [[1, 4], [0, 0], [1, 4], [1, 4]] and len(w2) == 6
    packed = np.concatenate([t2.reshape(-1).view(np.float64), w2])
    assert np.array_equal(packed[:4].view(np.int32).reshape(4, 2), t2) and np.array_equal(packed[4:], w2)
    for bad in ([0.0], [9.0], [np.nan], [-1.0]):
        with pytest.raises(ValueError):
            ops._blur_each_tables(bad)


# ---- argument checks that need no device ------------------------------------------------------------------------------------------
def test_ops_refuse_host_tensors_and_bad_records():
    from cswin_unet_amd import ops
    from cswin_unet_amd._lib import CswinHipError
    with pytest.raises(CswinHipError):
        ops.intensity_batch(torch.zeros(2, 8, 8), C.stage_draws("gamma", 2))
    with pytest.raises(CswinHipError):
        ops.gaussian_blur_each(torch.zeros(2, 8, 8), [None, 1.0])
    table = np.zeros(2, ops.INTENSITY_DESC)
    assert table.itemsize == 48 and table.view(np.int64).shape == (12,)


def test_trainer_validates_intensity_before_anything_else():
    from cswin_unet_amd.trainer import _step_options, surgical_trainer, trainer_synapse
    assert _step_options(SimpleNamespace())["intensity"] is None
    assert isinstance(_step_options(SimpleNamespace(intensity="nnunet"))["intensity"], IntensityAugment)
    spec = IntensityAugment(gamma=(1.0, (0.7, 1.5)))
    assert _step_options(SimpleNamespace(intensity=spec))["intensity"] is spec
    for bad in ("nnUNet", 1, dict(gamma=1.0)):
        with pytest.raises(ValueError, match="intensity"):
            trainer_synapse(SimpleNamespace(intensity=bad), None, "/nonexistent/never/created")
    with pytest.raises(ValueError, match="intensity"):
        surgical_trainer(SimpleNamespace(base_lr=1e-3, intensity="bogus"), None, "/nonexistent/never/created")
