"""Shared inputs, scipy references and the numpy emulation of the device blur (csrc/blur.hip behind ops.gaussian_blur) for
tests/test_blur_host.py (CPU) and tests/test_gpu_blur.py (GPU): the same seeded slices in both files, so what the emulation
shows on the CPU (0 elements unequal to scipy) is shown for the very inputs the device is measured on.  Inputs and references
are computed once per process and are read-only.

The emulation is the device's arithmetic stated in numpy: per axis, float64 products and sums in correlate1d's folded order
(acc = x[i] w[0], then acc += (x[i - k] + x[i + k]) w[-k] for k = r .. 1, multiply and add rounded separately), indices reflected
with period 2n, one rounding to float32 after each axis, axis 0 first."""
import contextlib
import functools
import random

import numpy as np
from scipy.ndimage import gaussian_filter

# ((D, H, W), sigma) of the device tests
GPU_CASES = [
    ((1, 1, 1), 1),              # r = 4 on one sample: period 2
    ((2, 3, 5), 1),              # radius larger than both axes
    ((3, 2, 9), 1.7),            # r = 7 > H
    ((2, 9, 33), 0.5),           # r = 2, odd width
    ((6, 64, 48), 1),
    ((1, 65, 130), 3),           # r = 12, row-tile remainder
    ((1, 37, 600), 1),           # more than one column chunk at every chunk width
    ((1, 20, 1100), 1),
    ((2, 512, 512), 1),          # the real pair
    ((2, 17, 23), 0.1),          # r = 0
    ((1, 40, 40), 8),            # r = 32, the limit
    ((1, 5, 70), 8),
    ((3, 224, 300), 2),
    # beyond the issue's list: the widths and radii at which the kernel's tile plan moves to its larger LDS budgets
    ((1, 6, 1500), 1),           # no four-row tile in 24 KiB: 40 KiB
    ((1, 5, 1600), 8),           # r = 32 at this width: 64 KiB
    ((1, 3, 2048), 8),           # the widest slice at the largest radius
]


def case_id(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else f"sigma{v:g}"


@functools.lru_cache(maxsize=None)
def slices(shape, sigma):
    """Seeded (D, H, W) float32 slices of a case, mean 100 and deviation 400 (read-only)."""
    x = (np.random.default_rng(2000 + 7 * sum(shape) + int(100 * sigma)).standard_normal(shape) * 400 + 100).astype(np.float32)
    x.setflags(write=False)
    return x


def scipy_blur(x, sigma):
    """gaussian_filter of every slice on its own, in the slices' dtype."""
    return np.stack([gaussian_filter(s, sigma) for s in x])


@functools.lru_cache(maxsize=None)
def scipy_blur_case(shape, sigma):
    out = scipy_blur(slices(shape, sigma), sigma)
    assert out.shape == tuple(shape) and out.dtype == np.float32
    out.setflags(write=False)
    return out


def reflect_index(i, n):
    """scipy's mode "reflect" (d c b a | a b c d | d c b a) for integer arrays i of any range: period 2n."""
    m = np.mod(i, 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def _pass(x, w, r, axis):
    """One correlate1d pass over `axis` of the float32 array x (D, H, W): float64 in the folded order, rounded to float32."""
    n = x.shape[axis]
    x64 = x.astype(np.float64)
    i = np.arange(n)
    acc = x64 * w[r]
    for k in range(r, 0, -1):
        lo, hi = np.take(x64, reflect_index(i - k, n), axis=axis), np.take(x64, reflect_index(i + k, n), axis=axis)
        acc = acc + (lo + hi) * w[r - k]
    return acc.astype(np.float32)


def emulate(x, sigma, truncate=4.0):
    """numpy emulation of csrc/blur.hip on float32 slices (D, H, W), taps from utils.gaussian_taps."""
    from cswin_unet_amd.utils import gaussian_taps
    w, r = gaussian_taps(sigma, truncate)
    return _pass(_pass(x, w, r, 1), w, r, 2)


def unequal_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape
    return int((a.view(np.uint32) != b.view(np.uint32)).sum())


@contextlib.contextmanager
def scripted_draws(params):
    """random.random and np.random.randint answer so that RandomGenerator / RawSliceParams draw (kind, k, axis, angle) = params
    (kinds of datasets.AUG_*: 0 nothing, 1 rot90 + flip, 2 rotate)."""
    kind, k, axis, angle = params
    uniforms = {0: [0.25, 0.25], 1: [0.75], 2: [0.25, 0.75]}[kind]
    ints = {0: [], 1: [k, axis], 2: [angle]}[kind]
    real_random, real_randint = random.random, np.random.randint

    def fake_randint(lo, hi=None):
        v = ints.pop(0)
        assert lo <= v < hi
        return v
    random.random, np.random.randint = (lambda: uniforms.pop(0)), fake_randint
    try:
        yield
    finally:
        random.random, np.random.randint = real_random, real_randint
    assert not uniforms and not ints
