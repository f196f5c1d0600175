"""Shared inputs and scipy references of tests/test_resize_host.py (CPU) and tests/test_gpu_resize.py (GPU): the same seeded
slices in both files, so what the float64 emulation of the banded product shows on the CPU (0 elements unequal to scipy) is
shown for the very inputs the device is measured on.  References are computed once per process and are read-only."""
import functools

import numpy as np
from scipy.ndimage import zoom

# (D, H, W) -> (h, w) of the device tests; the float64 variants are the first two
GPU_SHAPES = [
    ((6, 64, 48), (40, 56)),
    ((3, 20, 24), (32, 40)),          # upsampling on both axes: T = n_in
    ((2, 37, 53), (224, 224)),        # odd widths: no 8- or 16-B loads
    ((1, 130, 70), (56, 56)),
    ((2, 224, 300), (224, 224)),      # one axis at factor 1
    ((2, 512, 512), (224, 224)),      # the real pair; scipy leaves the last output row and column at its constant 0
    ((5, 33, 71), (17, 9)),
]
# further 2-D cases of the CPU test, so that every 1-D pair of the list below occurs
HOST_SHAPES = [((1, 224, 20), (224, 32)), ((2, 7, 7), (5, 5)), ((1, 1, 1), (1, 1))]
PAIRS_1D = [(512, 224), (37, 224), (53, 224), (64, 40), (48, 56), (20, 32), (224, 224), (7, 5), (1, 1)]


def seed_of(shape, size):
    return 1000 + sum(shape) * 7 + sum(size)


@functools.lru_cache(maxsize=None)
def slices(shape, size, dtype="float32"):
    """Seeded standard-normal (D, H, W) slices of a case (read-only)."""
    x = np.random.default_rng(seed_of(shape, size)).standard_normal(shape).astype(dtype)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def scipy_zoom3(shape, size, dtype="float32", widen=False):
    """ndimage.zoom(order=3) of every slice, in the slices' own dtype (read-only); widen: of the float32 slices cast to float64,
    which is scipy's result for them before its final rounding to float32."""
    x = slices(shape, size, dtype).astype(np.float64) if widen else slices(shape, size, dtype)
    out = np.stack([zoom(s, (size[0] / shape[1], size[1] / shape[2]), order=3) for s in x])
    assert out.shape == (shape[0],) + tuple(size) and out.dtype == x.dtype
    out.setflags(write=False)
    return out


def banded_product(x, size):
    """numpy emulation of csrc/resize.hip in float64: R_h x[d] R_w^T from zoom_operator's band tables, H pass first."""
    from cswin_unet_amd.utils import zoom_operator
    D, H, W = x.shape
    wh, sh = zoom_operator(H, size[0])
    ww, sw = zoom_operator(W, size[1])
    x = x.astype(np.float64)
    rows = sh[:, None] + np.arange(wh.shape[1])[None, :]               # (h, Th)
    cols = sw[:, None] + np.arange(ww.shape[1])[None, :]               # (w, Tw)
    img = np.einsum("it,ditw->diw", wh, x[:, rows, :])                 # (D, h, W)
    return np.einsum("jt,dijt->dij", ww, img[:, :, cols])              # (D, h, w)


def gather_nearest(lab, ih, iw):
    """lab[np.ix_(ih, iw)] with scipy's constant 0 where an index is -1 (nearest_index's mark for an output scipy does not gather)."""
    out = lab[np.ix_(np.maximum(ih, 0), np.maximum(iw, 0))]
    return np.where((ih >= 0)[:, None] & (iw >= 0)[None, :], out, 0).astype(lab.dtype)
