"""Shared inputs, draws, references and the comparison criterion of the intensity augmentation for tests/test_intensity_host.py
(CPU) and tests/test_gpu_intensity.py (GPU).  The reference is utils.intensity_host, the definition; inputs and references are
seeded, computed once per process and read-only.

Criterion (device against the definition): every element finite and within one float32 ulp, at most 1 element in 1e5 not
bit-equal -- the cap of tests/test_gpu_blur.py and tests/test_gpu_resize.py.  The cap is a condition, not a measurement: what the
device may do differently from numpy is the order of its whole-image sums and the last bit of log, cos and pow, and
`chain(..., longdouble, reversed)` below shows on the CPU how little of that reaches the float32 result."""
import functools
import itertools

import numpy as np

from cswin_unet_amd.datasets import INTENSITY_DRAW
from cswin_unet_amd.utils import intensity_host, mix64_host

# (B, h, w) of the device tests
SHAPES = [(1, 1, 1), (3, 5, 7), (5, 17, 23), (4, 40, 40), (2, 64, 96), (3, 224, 224)]
KINDS = ("uniform", "clipped", "pm1000", "constant")


def shape_id(s):
    return "x".join(map(str, s))


@functools.lru_cache(maxsize=None)
def images(shape, kind):
    """Seeded float32 (B, h, w), read-only.  uniform: U[0, 1);  clipped: N(0.5, 0.4^2) clipped to [0, 1], so the minimum and the
    maximum are each shared by many pixels;  pm1000: U(-1000, 1000);  constant: uniform with sample 0 set to 0.3 throughout."""
    rng = np.random.default_rng(900 + 13 * sum(shape) + KINDS.index(kind))
    if kind == "clipped":
        x = np.clip(rng.standard_normal(shape) * 0.4 + 0.5, 0.0, 1.0)
    elif kind == "pm1000":
        x = rng.uniform(-1000.0, 1000.0, shape)
    else:
        x = rng.random(shape)
    x = x.astype(np.float32)
    if kind == "constant":
        x[0] = np.float32(0.3)
    x.setflags(write=False)
    return x


def record(blur=None, noise=None, brightness=None, contrast=None, gamma=None, invert=False, seed=0):
    """One INTENSITY_DRAW record: a stage is on where its parameter is given (noise: the standard deviation)."""
    d = np.zeros((), INTENSITY_DRAW)
    d["brightness"] = d["contrast"] = d["gamma"] = 1.0
    for name, field, v in (("blur", "sigma", blur), ("noise", "noise_std", noise), ("brightness", "brightness", brightness),
                           ("contrast", "contrast", contrast), ("gamma", "gamma", gamma)):
        if v is not None:
            d["do_" + name], d[field] = True, v
    d["invert"], d["seed"] = invert, seed
    return d


def batch_of(recs):
    return np.array([r[()] if isinstance(r, np.ndarray) else r for r in recs], INTENSITY_DRAW)


# name -> the stages' parameters of a batch in which every sample has these stages (the seed differs per sample)
STAGE_SETS = {
    "blur": dict(blur=0.8),
    "noise": dict(noise=0.25),
    "brightness": dict(brightness=1.2),
    "contrast_up": dict(contrast=1.25),
    "contrast_down": dict(contrast=0.75),
    "gamma": dict(gamma=0.7),
    "gamma_inverted": dict(gamma=1.5, invert=True),
    "all": dict(blur=0.6, noise=0.1, brightness=0.9, contrast=1.2, gamma=1.3),
    "all_inverted": dict(blur=1.0, noise=0.3, brightness=1.1, contrast=0.8, gamma=0.8, invert=True),
}


def stage_draws(name, B):
    return batch_of([record(seed=1000 * b + 17, **STAGE_SETS[name]) for b in range(B)])


def pattern_draws():
    """32 + 16 records: every on/off pattern of the five stages (all-off first), then the sixteen with gamma on once more,
    inverted.  The parameters vary with the sample."""
    recs = []
    for k, on in enumerate(itertools.product((False, True), repeat=5)):
        for inv in ((False, True) if on[4] else (False,)):
            b = len(recs)
            recs.append(record(blur=0.5 + 0.03 * (b % 16) if on[0] else None, noise=0.05 + 0.01 * b if on[1] else None,
                               brightness=0.75 + 0.01 * b if on[2] else None, contrast=0.75 + 0.01 * b if on[3] else None,
                               gamma=0.7 + 0.016 * b if on[4] else None, invert=inv, seed=77 + 3 * b))
    return batch_of(recs)


def host_batch(x, draws):
    """utils.intensity_host of every sample of x (B, h, w)."""
    return np.stack([intensity_host(x[b], draws[b]) for b in range(len(x))])


@functools.lru_cache(maxsize=None)
def stage_reference(shape, kind, name):
    out = host_batch(images(shape, kind), stage_draws(name, shape[0]))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def pattern_inputs(hw, kind):
    """(x (48, h, w): the kind's samples of shape (3, h, w) repeated, the definition's result for pattern_draws())."""
    src = images((3,) + tuple(hw), kind)
    draws = pattern_draws()
    x = np.ascontiguousarray(src[np.arange(len(draws)) % 3])
    want = host_batch(x, draws)
    x.setflags(write=False)
    want.setflags(write=False)
    return x, want


def unequal_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape
    return int((a.view(np.uint32) != b.view(np.uint32)).sum())


def max_ulps(got, want):
    return float((np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)).max())


def check(got, want, tag):
    """The criterion; prints the count."""
    unequal, ulps = unequal_bits(got, want), max_ulps(got, want)
    print(f"{tag}: {unequal} of {got.size} elements not bit-equal, max difference {ulps:.3g} ulp")
    assert np.isfinite(got).all(), tag
    assert ulps <= 1.0, (tag, ulps)
    assert unequal * 100000 <= got.size, (tag, unequal, got.size)
    return unequal


# ---- stages 2-5 evaluated another way ---------------------------------------------------------------------------------------------
def forward_sum(z):
    """The sum of z's elements one after the other in row-major order, in z's dtype."""
    return np.cumsum(z.ravel())[-1]


def reversed_sum(z):
    return np.cumsum(z.ravel()[::-1])[-1]


def chain(x, d, dtype, total):
    """Stages 2-5 of utils.intensity_host on one float32 image, in `dtype` (float64 or longdouble) with the whole-image sums formed
    by `total`; rounded to float32 at the end.  The mean is total / n and the deviation sqrt(total((z - mean)^2) / n)."""
    T = dtype
    z = x.astype(T)
    n = T(z.size)
    mean = lambda a: total(a) / n
    std = lambda a: np.sqrt(total((a - mean(a)) ** 2) / n)
    if d["do_noise"]:
        r = mix64_host(mix64_host(np.uint64(d["seed"])) ^ np.arange(z.size, dtype=np.uint64))
        u1 = ((r >> np.uint64(40)) + np.uint64(1)).astype(T) / T(2 ** 24)
        u2 = ((r >> np.uint64(16)) & np.uint64(0xFFFFFF)).astype(T) / T(2 ** 24)
        z = z + T(d["noise_std"]) * (np.sqrt(T(-2) * np.log(u1)) * np.cos(T(2) * T(np.pi) * u2)).reshape(z.shape)
    if d["do_brightness"]:
        z = z * T(d["brightness"])
    if d["do_contrast"]:
        m, lo, hi = mean(z), z.min(), z.max()
        z = np.clip((z - m) * T(d["contrast"]) + m, lo, hi)
    if d["do_gamma"]:
        if d["invert"]:
            z = -z
        m0, s0, lo = mean(z), std(z), z.min()
        rng = z.max() - lo
        z = ((z - lo) / (rng + T(1e-7))) ** T(d["gamma"]) * rng + lo
        z = (z - mean(z)) / (std(z) + T(1e-8)) * s0 + m0
        if d["invert"]:
            z = -z
    return z.astype(np.float32)


def random_case(k):
    """(x, record) number k of the two-evaluation check: sides 1..229; inputs in [0, 1] quantised to 1/64 (many tied minima and
    maxima) for even k, U(-300, 300) for odd k; every stage 2-5 on with probability 0.7."""
    rng = np.random.default_rng(5000 + k)
    h, w = (int(v) for v in rng.integers(1, 230, 2))
    x = (np.round(rng.random((h, w)) * 64) / 64 if k % 2 == 0 else rng.uniform(-300, 300, (h, w))).astype(np.float32)
    on = rng.random(4) < 0.7
    d = record(noise=rng.uniform(0, 0.35) if on[0] else None, brightness=rng.uniform(0.75, 1.25) if on[1] else None,
               contrast=rng.uniform(0.75, 1.25) if on[2] else None, gamma=rng.uniform(0.7, 1.5) if on[3] else None,
               invert=bool(rng.random() < 0.5), seed=int(rng.integers(0, 2 ** 63)))
    return x, d


# ---- gaussian_blur_each in the emulation of tests/blur_cases.py --------------------------------------------------------------------
EACH_SIGMAS = [None, 0.5, 1.0, 0.73, 2.0]
EACH_SHAPES = [(5, 17, 23), (5, 64, 96)]


@functools.lru_cache(maxsize=None)
def each_inputs(shape):
    """(x, scipy's gaussian_filter of slice d at EACH_SIGMAS[d], the slice itself where that is None), read-only."""
    import blur_cases as B
    from scipy.ndimage import gaussian_filter
    x = B.slices(shape, 1.0)
    want = np.stack([s if sig is None else gaussian_filter(s, sig) for s, sig in zip(x, EACH_SIGMAS)])
    want.setflags(write=False)
    return x, want


def emulate_each(x, table, taps, max_radius):
    """The device's gaussian_blur_each in numpy: slice d through blur_cases._pass with the radius and the taps that the table of
    ops._blur_each_tables gives it, clamped as the kernel clamps them."""
    import blur_cases as B
    out = []
    for d in range(len(x)):
        r = min(max(int(table[d, 1]), 0), min(max_radius, len(taps) - 1))
        off = min(max(int(table[d, 0]), 0), len(taps) - 1 - r)
        half = taps[off:off + r + 1]
        w = np.concatenate([half, half[:-1][::-1]])                  # blur_cases reads w[r - k] = w[-k] and w[r]
        out.append(B._pass(B._pass(x[d:d + 1], w, r, 1), w, r, 2)[0])
    return np.stack(out)
