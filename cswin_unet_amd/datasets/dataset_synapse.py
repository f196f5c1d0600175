"""Synapse slice / volume reader and training augmentation.

Host-side counterpart of the reference's datasets/dataset_synapse.py:12-83: same public names, sample schema and -- this is
what makes a seeded run reproduce the reference's batches -- the same consumption order of the two RNG streams
(`random.random()` picks the branch, `np.random.randint` draws k / axis / angle).  tests/test_host_next_rows.py checks the
outputs against tests/golden/g9_augment.npz, which was produced by the reference itself.  The arithmetic (rot90, flip,
order-0 rotate, cubic / nearest zoom) is numpy / scipy, exactly the libraries the reference calls; nothing here touches the GPU.

Training slices: `<base_dir>/<name>.npz` holding `image` (H, W) float32 in [0, 1] and `label` (or `segmentation`) (H, W)
class ids (:62-69).  Test volumes: `<base_dir>/<name>.npy.h5` with `image`/`label` or `images`/`segmentations` (:70-77);
h5py is optional in this image, so `<name>.npz` volumes are accepted as well.
"""
import os
import random

import numpy as np
import torch
from scipy import ndimage
from torch.utils.data import Dataset

_NEAREST, _CUBIC = 0, 3


def random_rot_flip(image, label):
    """Quarter turns (k drawn from {0..3}) followed by a flip along a drawn axis; the same transform for both arrays (:12-19)."""
    quarter_turns = np.random.randint(0, 4)
    flip_axis = None
    out = []
    for arr in (image, label):
        arr = np.rot90(arr, quarter_turns)
        if flip_axis is None:
            flip_axis = np.random.randint(0, 2)         # drawn after the rotations, like the reference
        out.append(arr)
    return tuple(np.flip(arr, axis=flip_axis).copy() for arr in out)


def random_rotate(image, label):
    """Rotation by an integer angle from [-20, 20), nearest neighbour for image and label alike, shape kept (:22-26)."""
    degrees = np.random.randint(-20, 20)
    turn = lambda arr: ndimage.rotate(arr, degrees, order=_NEAREST, reshape=False)
    return turn(image), turn(label)


def _resize_pair(image, label, size):
    """Cubic zoom of the image and nearest zoom of the label to `size` when the shape differs (:41-43)."""
    h, w = image.shape
    if (h, w) == tuple(size):
        return image, label
    factors = (size[0] / h, size[1] / w)
    return ndimage.zoom(image, factors, order=_CUBIC), ndimage.zoom(label, factors, order=_NEAREST)


class RandomGenerator(object):
    """{'image': (H, W), 'label': (H, W)} -> {'image': float32 (1, h, w), 'label': int64 (h, w)} (:29-47).
    blur_sigma: None, or the sigma of the blurred copy of the dataset (apply_blur_train.py:147-150): the image, cast to float32
    unless it is floating already, goes through ndimage.gaussian_filter before the transforms, as if the blurred slice had been
    read from disk.  The random draws are the same either way."""

    def __init__(self, output_size, blur_sigma=None):
        self.output_size, self.blur_sigma = output_size, blur_sigma

    def __call__(self, sample):
        pair = (sample['image'], sample['label'])
        if self.blur_sigma is not None:
            image = np.asarray(pair[0])
            image = image if np.issubdtype(image.dtype, np.floating) else image.astype(np.float32)
            pair = (ndimage.gaussian_filter(image, self.blur_sigma), pair[1])
        # one uniform draw decides "rot90 + flip"; only if that fails a second draw decides "small rotation"
        if random.random() > 0.5:
            pair = random_rot_flip(*pair)
        elif random.random() > 0.5:
            pair = random_rotate(*pair)
        image, label = _resize_pair(*pair, self.output_size)
        image_t = torch.from_numpy(image.astype(np.float32)).unsqueeze(0)
        label_t = torch.from_numpy(label.astype(np.float32)).long()
        return {'image': image_t, 'label': label_t}


# `kind` of RawSliceParams' parameters: the one Python definition (ops.augment_batch imports it); csrc/augment.hip mirrors it
AUG_NONE, AUG_ROT90_FLIP, AUG_ROTATE = 0, 1, 2


class RawSliceParams(object):
    """RandomGenerator's random draws without its arithmetic, for `augment="hip"`: {'image': (H, W) float32, 'label': (H, W)} ->
    {'image': float32 (H, W) as it is, 'label': uint8 (H, W), 'params': int32 (4,) = (kind, k, axis, angle)}; ops.augment_batch
    applies the transforms and the zooms to `output_size` to the collated batch on the device.  Both RNG streams are consumed in
    RandomGenerator's order and counts (one or two `random.random()`, then k and axis or the angle from `np.random.randint`), so a
    seeded run draws the transforms RandomGenerator would apply.  ValueError for what the device path does not take: an image
    that is not float32 (scipy computes in the image's own dtype) or labels that are not integral values in 0..255."""

    def __init__(self, output_size):
        self.output_size = output_size

    def __call__(self, sample):
        image, label = np.asarray(sample['image']), np.asarray(sample['label'])
        kind, k, axis, angle = AUG_NONE, 0, 0, 0
        if random.random() > 0.5:
            kind, k = AUG_ROT90_FLIP, np.random.randint(0, 4)
            axis = np.random.randint(0, 2)
        elif random.random() > 0.5:
            kind, angle = AUG_ROTATE, np.random.randint(-20, 20)
        if image.dtype != np.float32 or image.ndim != 2 or image.shape != label.shape:
            raise ValueError(f"RawSliceParams: image {image.dtype} {image.shape} / label {label.shape}: the device augmentation takes "
                             f"float32 (H, W) slices with labels of the same shape; use augment=\"host\" for this dataset")
        if label.dtype.kind not in "biuf" or label.min() < 0 or label.max() > 255 or (label.dtype.kind == "f" and
                                                                                      np.any(label != np.rint(label))):
            raise ValueError("RawSliceParams: labels are not integral class ids in 0..255; use augment=\"host\" for this dataset")
        return {'image': torch.from_numpy(np.ascontiguousarray(image)), 'label': torch.from_numpy(label.astype(np.uint8)),
                'params': torch.tensor([kind, k, axis, angle], dtype=torch.int32)}


# one sample's draw of IntensityAugment: what utils.intensity_host (the definition) and ops.intensity_batch (the device) read
INTENSITY_DRAW = np.dtype([("do_blur", "?"), ("do_noise", "?"), ("do_brightness", "?"), ("do_contrast", "?"), ("do_gamma", "?"),
                           ("invert", "?"), ("sigma", "<f8"), ("noise_std", "<f8"), ("brightness", "<f8"), ("contrast", "<f8"),
                           ("gamma", "<f8"), ("seed", "<u8")])


def check_intensity_draws(draws, n=None):
    """`draws` as a one-dimensional INTENSITY_DRAW array (a single record becomes an array of one), every parameter of a stage
    that is on checked as IntensityAugment checks its ranges: ValueError for a wrong dtype or count, a sigma outside
    utils.gaussian_taps' limits, a noise_std that is negative, a gamma that is not positive, or any value that is not finite."""
    draws = np.atleast_1d(np.asarray(draws))
    if draws.dtype != INTENSITY_DRAW or draws.ndim != 1:
        raise ValueError(f"intensity draws must be a one-dimensional array of datasets.INTENSITY_DRAW records, got {draws.dtype} {draws.shape}")
    if n is not None and len(draws) != n:
        raise ValueError(f"{len(draws)} intensity draws for {n} samples")
    from ..utils import gaussian_taps
    for b, d in enumerate(draws):
        if d["do_blur"]:
            gaussian_taps(float(d["sigma"]))
        for flag, name, ok in (("do_noise", "noise_std", lambda v: v >= 0), ("do_brightness", "brightness", lambda v: True),
                               ("do_contrast", "contrast", lambda v: True), ("do_gamma", "gamma", lambda v: v > 0)):
            v = float(d[name])
            if d[flag] and not (np.isfinite(v) and ok(v)):
                raise ValueError(f"intensity draw {b}: {name} = {v!r} is outside what the stage takes")
    return draws


class IntensityAugment(object):
    """Appearance augmentation of a training batch, nnU-Net's: per sample and stage a coin with the stage's probability, then a
    uniform draw from its range.  Stages in the order they are applied (utils.intensity_host is the definition):
      blur        scipy.ndimage.gaussian_filter with sigma ~ U(blur_sigma)
      noise       additive Gaussian noise of variance ~ U(noise_variance), ABSOLUTE (not relative to the image's range)
      brightness  a factor ~ U(brightness)
      contrast    a factor ~ U(contrast) about the mean, clipped to the image's own range
      gamma       a power ~ U(gamma) on the image scaled to [0, 1], mean and deviation restored; with probability p_invert on -image
    Every argument is (probability, (low, high)).  ValueError at construction for a probability outside [0, 1], low > high, a
    negative variance, a gamma <= 0 or a sigma outside utils.gaussian_taps' limits.  `nnunet()` is nnU-Net's default set."""

    def __init__(self, noise=(0.0, (0.0, 0.0)), blur=(0.0, (1.0, 1.0)), brightness=(0.0, (1.0, 1.0)), contrast=(0.0, (1.0, 1.0)),
                 gamma=(0.0, (1.0, 1.0)), p_invert=0.0):
        from ..utils import gaussian_taps
        self.stages = {}
        for name, spec in (("noise", noise), ("blur", blur), ("brightness", brightness), ("contrast", contrast), ("gamma", gamma)):
            try:
                p, (lo, hi) = spec
                p, lo, hi = float(p), float(lo), float(hi)
            except (TypeError, ValueError):
                raise ValueError(f"IntensityAugment: {name} = {spec!r} is not (probability, (low, high))") from None
            if not 0.0 <= p <= 1.0:
                raise ValueError(f"IntensityAugment: {name} probability {p!r} outside [0, 1]")
            if not (np.isfinite(lo) and np.isfinite(hi) and lo <= hi):
                raise ValueError(f"IntensityAugment: {name} range ({lo!r}, {hi!r}) is not finite with low <= high")
            if name == "noise" and lo < 0:
                raise ValueError(f"IntensityAugment: noise variance range ({lo!r}, {hi!r}) is negative")
            if name == "gamma" and lo <= 0:
                raise ValueError(f"IntensityAugment: gamma range ({lo!r}, {hi!r}) must be positive")
            if name == "blur":
                gaussian_taps(lo), gaussian_taps(hi)                        # ValueError for a sigma the blur does not take
            self.stages[name] = (p, lo, hi)
        self.p_invert = float(p_invert)
        if not 0.0 <= self.p_invert <= 1.0:
            raise ValueError(f"IntensityAugment: p_invert {p_invert!r} outside [0, 1]")

    @classmethod
    def nnunet(cls):
        return cls(noise=(0.1, (0.0, 0.1)), blur=(0.2, (0.5, 1.0)), brightness=(0.15, (0.75, 1.25)), contrast=(0.15, (0.75, 1.25)),
                   gamma=(0.3, (0.7, 1.5)), p_invert=0.25)

    def draw(self, n, generator):
        """n INTENSITY_DRAW records from `generator`, a numpy.random.Generator (the module-level `random` and `np.random` streams,
        which RawSliceParams and RandomGenerator share with the reference, are not touched).  The generator is consumed in a fixed
        pattern -- 12 arrays of n whatever the coins show -- so the records depend on its state and n alone.  A stage that is
        off keeps its neutral parameter."""
        if not isinstance(generator, np.random.Generator):
            raise ValueError(f"IntensityAugment.draw: generator must be a numpy.random.Generator, got {type(generator).__name__}")
        out = np.zeros(int(n), INTENSITY_DRAW)
        for name, field, neutral in (("blur", "sigma", 0.0), ("noise", "noise_std", 0.0), ("brightness", "brightness", 1.0),
                                     ("contrast", "contrast", 1.0), ("gamma", "gamma", 1.0)):
            p, lo, hi = self.stages[name]
            on, value = generator.random(len(out)) < p, generator.uniform(lo, hi, len(out))
            out["do_" + name] = on
            out[field] = np.where(on, np.sqrt(value) if name == "noise" else value, neutral)
        out["invert"] = out["do_gamma"] & (generator.random(len(out)) < self.p_invert)
        out["seed"] = generator.integers(0, 2 ** 64, len(out), dtype=np.uint64)
        return out


def collate_raw_slices(samples):
    """default_collate for RawSliceParams' samples; slices of different shapes in one batch raise a ValueError that names them."""
    from torch.utils.data import default_collate
    shapes = sorted({tuple(s['image'].shape) for s in samples})
    if len(shapes) > 1:
        raise ValueError(f"augment=\"hip\" needs one slice shape per batch, got {shapes}; use augment=\"host\" for this dataset")
    return default_collate(samples)


def _first_key(data, *names):
    for n in names:
        if n in data:
            return data[n][:]
    raise KeyError(f"none of {names} in {list(data.keys())}")


class Synapse_dataset(Dataset):
    """split == 'train': 2-D slices from .npz; any other split: whole volumes (:50-83).  `list_dir/<split>.txt` names the cases."""

    def __init__(self, base_dir, list_dir, split, transform=None, is_kits=False, is_lits=False):
        self.data_dir, self.split, self.transform, self.is_kits = base_dir, split, transform, is_kits
        with open(os.path.join(list_dir, split + '.txt')) as f:
            self.sample_list = f.readlines()

    def __len__(self):
        return len(self.sample_list)

    def _read_slice(self, name):
        data = np.load(os.path.join(self.data_dir, name + '.npz'))
        return data['image'], _first_key(data, 'label', 'segmentation')

    def _read_volume(self, name):
        h5 = self.data_dir + "/{}.npy.h5".format(name)
        if not os.path.exists(h5):
            data = np.load(os.path.join(self.data_dir, name + '.npz'))
            return _first_key(data, 'image', 'images'), _first_key(data, 'label', 'segmentations')
        try:
            import h5py
        except ImportError as e:
            raise RuntimeError(f"{h5}: reading test volumes in HDF5 needs h5py, which is not installed; "
                               f"convert the volume to {name}.npz (image, label)") from e
        with h5py.File(h5, "r") as data:
            return _first_key(data, 'image', 'images'), _first_key(data, 'label', 'segmentations')

    def __getitem__(self, idx):
        name = self.sample_list[idx].strip('\n')
        image, label = (self._read_slice if self.split == "train" else self._read_volume)(name)
        sample = {'image': image, 'label': label}
        if self.transform:
            sample = self.transform(sample)
        sample['case_name'] = name
        return sample


def write_synthetic_synapse(root, n_slices=8, n_volumes=1, size=512, depth=6, num_classes=9, seed=1234):
    """A stand-in dataset in the Synapse schema (the real data is not in the container): blocky
    label maps and images correlated with them.  Returns (base_dir_train, base_dir_test, list_dir)."""
    rng = np.random.default_rng(seed)
    train, test, lists = (os.path.join(root, d) for d in ("train_npz", "test_vol", "lists"))
    for d in (train, test, lists):
        os.makedirs(d, exist_ok=True)

    def one(shape):
        coarse = rng.integers(0, num_classes, size=tuple(s // 32 for s in shape))
        lab = np.kron(coarse, np.ones((32, 32), np.int64)).astype(np.float32)
        img = (lab / (num_classes - 1) * 0.6 + 0.2 + 0.05 * rng.standard_normal(shape)).clip(0, 1).astype(np.float32)
        return img, lab

    names = []
    for i in range(n_slices):
        img, lab = one((size, size))
        names.append(f"case{i // 4:04d}_slice{i % 4:03d}")
        np.savez(os.path.join(train, names[-1] + ".npz"), image=img, label=lab)
    with open(os.path.join(lists, "train.txt"), "w") as f:
        f.write("\n".join(names) + "\n")
    vols = []
    for v in range(n_volumes):
        pairs = [one((size, size)) for _ in range(depth)]
        vols.append(f"case{100 + v:04d}")
        np.savez(os.path.join(test, vols[-1] + ".npz"), image=np.stack([p[0] for p in pairs]),
                 label=np.stack([p[1] for p in pairs]))
    with open(os.path.join(lists, "test_vol.txt"), "w") as f:
        f.write("\n".join(vols) + "\n")
    return train, test, lists
