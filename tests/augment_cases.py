"""Shared inputs, host references and the numpy emulation of the device augmentation (csrc/augment.hip behind ops.augment_batch)
for tests/test_augment_host.py (CPU) and tests/test_gpu_augment.py (GPU).  References are computed once per process and are
read-only.

The comparison criterion for images (x = the raw slice, want = scipy's / the fixture's float32 result): an element passes if
|got - want| <= 2**-50 * max|x| or it lies within one float32 ulp of want, and of the elements with |want| >= 2**-20 * max|x| at
most 1 in 1e5 may differ in bits (the cap of tests/test_gpu_resize.py).  The absolute floor matters only after a rotation: in
the zero corners it leaves, scipy's own cubic zoom is prefilter ringing of ~1e-10 and below, the band tables of zoom_operator
drop operator entries below 2**-64, and there the dropped entries are the whole value.  Labels are compared exactly."""
import contextlib
import functools
import os
import random

import numpy as np

from cswin_unet_amd.datasets import AUG_NONE as NONE, AUG_ROT90_FLIP as ROT90_FLIP, AUG_ROTATE as ROTATE

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ANGLES = (-20, -7, 0, 1, 19)
# (kind, k, axis, angle) of the 14-sample batch: the identity, all 8 quarter-turn / flip pairs, five angles
PARAMS14 = [(NONE, 0, 0, 0)] + [(ROT90_FLIP, k, axis, 0) for k in range(4) for axis in range(2)] + [(ROTATE, 0, 0, a) for a in ANGLES]
# (H, W) -> (h, w): square; non-square (both shape groups occur); odd widths and upsampling; nothing to resize
BATCH_SHAPES = [((64, 64), (40, 40)), ((40, 56), (32, 32)), ((37, 53), (224, 224)), ((48, 48), (48, 48))]


def source_index(H, W, kind, k, axis, angle):
    """The index rule of csrc/augment.hip, stated once: int array (H', W') of the flat source index of every pixel of the
    transformed slice, -1 where there is none.  (H', W') = (W, H) after an odd number of quarter turns."""
    from cswin_unet_amd.utils import rotation_index
    if kind == ROTATE:
        return rotation_index(H, W, angle).astype(np.int64)
    if kind == NONE:
        return np.arange(H * W, dtype=np.int64).reshape(H, W)
    Ht, Wt = (W, H) if k % 2 else (H, W)
    i, j = np.meshgrid(np.arange(Ht), np.arange(Wt), indexing="ij")
    if axis == 0:
        i = Ht - 1 - i
    else:
        j = Wt - 1 - j
    r = (i, j, H - 1 - i, H - 1 - j)[k]
    c = (j, W - 1 - i, W - 1 - j, i)[k]
    return (r * W + c).astype(np.int64)


def gather(x, src):
    """x.ravel()[src] with 0 where src is negative, in x's dtype."""
    return np.where(src >= 0, x.ravel()[np.maximum(src, 0)], 0).astype(x.dtype)


def emulate(image, label, params, size):
    """numpy emulation of the whole device pipeline for one sample: image gather, float64 banded product rounded once to float32
    (resize_cases.banded_product; skipped when nothing is resized), label gather fused with the order-0 zoom."""
    from cswin_unet_amd.utils import nearest_index
    from resize_cases import banded_product, gather_nearest
    src = source_index(*image.shape, *params)
    img = gather(image, src)
    if img.shape != tuple(size):
        img = banded_product(img[None], size)[0].astype(np.float32)
    ih, iw = nearest_index(src.shape[0], size[0]), nearest_index(src.shape[1], size[1])
    picked = gather_nearest(src, ih, iw)                                # a -1 row / column index gives 0 = pixel 0: masked below
    picked = np.where((ih >= 0)[:, None] & (iw >= 0)[None, :], picked, -1)
    return img, gather(label, picked).astype(np.int64)


@contextlib.contextmanager
def _scripted_randint(values):
    """np.random.randint answers with `values` in turn: runs the host functions with explicit parameters."""
    values, real = list(values), np.random.randint

    def fake(lo, hi=None):
        v = values.pop(0)
        assert lo <= v < hi
        return v
    np.random.randint = fake
    try:
        yield
    finally:
        np.random.randint = real
    assert not values


def host_augment(image, label, params, size):
    """What RandomGenerator yields for one sample when its draws come out as `params`: the dataset module's own random_rot_flip /
    random_rotate / _resize_pair and its final conversions.  Returns (float32 (h, w), int64 (h, w))."""
    from cswin_unet_amd.datasets import dataset_synapse as D
    kind, k, axis, angle = params
    pair = (image, label)
    if kind == ROT90_FLIP:
        with _scripted_randint([k, axis]):
            pair = D.random_rot_flip(*pair)
    elif kind == ROTATE:
        with _scripted_randint([angle]):
            pair = D.random_rotate(*pair)
    img, lab = D._resize_pair(*pair, list(size))
    return img.astype(np.float32), lab.astype(np.float32).astype(np.int64)


def check_image(got, want, xmax, tag):
    """The criterion of the module docstring; prints its figures before asserting."""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    assert np.isfinite(got).all(), tag
    diff = np.abs(got.astype(np.float64) - want.astype(np.float64))
    ok = (diff <= 2.0 ** -50 * xmax) | (diff <= np.spacing(np.abs(want)).astype(np.float64))
    unequal = got.view(np.uint32) != want.view(np.uint32)
    big = np.abs(want) >= 2.0 ** -20 * xmax
    print(f"{tag}: {int(unequal.sum())} of {got.size} elements not bit-equal ({int((unequal & big).sum())} of {int(big.sum())} at or "
          f"above 2^-20 max|x|), max |diff| {float(diff.max()):.3g}, {int((~ok).sum())} outside the criterion")
    assert ok.all(), (tag, int((~ok).sum()))
    assert int((unequal & big).sum()) * 100000 <= int(big.sum()), (tag, int((unequal & big).sum()), int(big.sum()))


@functools.lru_cache(maxsize=None)
def batch14(shape, with_255=False):
    """Seeded raw batch of the 14-sample test: float32 images (14, H, W) in [0, 1), uint8 labels of 9 classes in blocks of 4 x 4
    (so that order-0 rotation and zoom keep structure); with_255: a few blocks of every label hold the id 255."""
    H, W = shape
    rng = np.random.default_rng(4000 + 13 * H + W)
    img = rng.random((len(PARAMS14), H, W)).astype(np.float32)
    coarse = rng.integers(0, 9, size=(len(PARAMS14), -(-H // 4), -(-W // 4)))
    if with_255:
        coarse[rng.random(coarse.shape) < 0.05] = 255
    lab = np.kron(coarse, np.ones((4, 4), np.int64))[:, :H, :W].astype(np.uint8)
    img.setflags(write=False)
    lab.setflags(write=False)
    return img, lab


@functools.lru_cache(maxsize=None)
def host_batch14(shape, size, with_255=False):
    """host_augment of every sample of batch14 (read-only): (float32 (14, h, w), int64 (14, h, w))."""
    img, lab = batch14(shape, with_255)
    out = [host_augment(img[b], lab[b], PARAMS14[b], size) for b in range(len(PARAMS14))]
    imgs, labs = np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
    imgs.setflags(write=False)
    labs.setflags(write=False)
    return imgs, labs


G9_N = 12


@functools.lru_cache(maxsize=None)
def g9_input(i):
    """Raw sample i of tests/golden/g9_augment.npz (tools/make_golden.py g9_augment): float32 image, float32 blocky label."""
    from oracle.determ import det_labels, det_normal
    size = (512, 512) if i % 3 else (224, 224)
    img = det_normal(f"aug.img{i}", size).astype(np.float32) * 0.25 + 0.5
    lab = det_labels(f"aug.lab{i}", (1,) + size, 9)[0].astype(np.float32)
    lab = np.kron(lab[:size[0] // 16, :size[1] // 16], np.ones((16, 16), np.float32))
    img.setflags(write=False)
    lab.setflags(write=False)
    return img, lab


def g9_seed(i):
    random.seed(100 + i)
    np.random.seed(200 + i)


@functools.lru_cache(maxsize=None)
def g9_params(i):
    """(kind, k, axis, angle) RawSliceParams draws for g9's sample i under the fixture's seeds."""
    from cswin_unet_amd.datasets import RawSliceParams
    img, lab = g9_input(i)
    g9_seed(i)
    return tuple(RawSliceParams([224, 224])({"image": img.copy(), "label": lab})["params"].tolist())


@functools.lru_cache(maxsize=None)
def g9():
    g = np.load(os.path.join(GOLD, "g9_augment.npz"))
    return {k: g[k] for k in g.files}
