"""Shared by tests/test_components_host.py and tests/test_gpu_components.py (not a test module): the volumes the connected-
component kernels are tried on, the canonical labels and sizes built from scipy.ndimage.label, and the filter rule written out
component by component with scipy -- a second construction beside utils.filter_components_host, which the host test compares."""
import math

import numpy as np
from scipy.ndimage import label

from seg_metrics_cases import _ellipsoid


def canonical_labels(vol, ncls):
    """(labels int32, sizes int32) of vol's shape as include/cswin_hip.h defines them: labels = 0 for ids 0 and >= ncls, else
    1 + the smallest flat index of the voxel's face-connected component of its class; sizes = the component's voxel count at that
    smallest index, 0 elsewhere.  scipy's own numbering is never relied on: np.unique's first occurrence of a scipy label in
    C order is the component's smallest flat index."""
    vol = np.asarray(vol)
    labels, sizes = np.zeros(vol.size, np.int32), np.zeros(vol.size, np.int32)
    for c in range(1, ncls):
        lab, n = label(vol == c)
        if n == 0:
            continue
        flat = lab.ravel()
        ids, first, counts = np.unique(flat, return_index=True, return_counts=True)
        fg = ids > 0
        root = np.zeros(n + 1, np.int64)
        root[ids[fg]] = first[fg]
        on = flat > 0
        labels[on] = (root[flat[on]] + 1).astype(np.int32)
        sizes[first[fg]] = counts[fg]
    return labels.reshape(vol.shape), sizes.reshape(vol.shape)


def scipy_filter(vol, ncls, min_size, min_fraction):
    """The filter rule of the issue, one component at a time: min_size / min_fraction are sequences of ncls entries (entry 0
    unused).  A component of class c is kept iff its size >= max(min_size[c], ceil(min_fraction[c] * largest_c))."""
    vol = np.asarray(vol)
    out = vol.copy()
    for c in range(1, ncls):
        lab, n = label(vol == c)
        comps = [lab == k for k in range(1, n + 1)]
        if not comps:
            continue
        largest = max(int(m.sum()) for m in comps)
        thr = max(int(min_size[c]), math.ceil(float(min_fraction[c]) * float(largest)))
        for m in comps:
            if int(m.sum()) < thr:
                out[m] = 0
    return out


def rule_tables(rule, ncls):
    """(min_size, min_fraction) lists of a rule, written independently of utils.component_rule_tables."""
    if rule == "largest":
        return [0] * ncls, [0.0] + [1.0] * (ncls - 1)
    ms, mf = [0] * ncls, [0.0] * ncls
    for c, spec in rule.items():
        ms[c], mf[c] = spec.get("min_size", 0), spec.get("min_fraction", 0.0)
    return ms, mf


def noise(shape, ncls, density, seed):
    """Every voxel foreground with probability `density`, its class uniform in 1..ncls (ncls itself is out of range: background)."""
    rng = np.random.default_rng(seed)
    return np.where(rng.random(shape) < density, rng.integers(1, ncls + 1, shape), 0).astype(np.uint8)


def serpentine(shape):
    """One class-1 path: every second row of every second layer is full, consecutive full rows are joined by one voxel at
    alternating ends, consecutive full layers by one voxel at (z + 1, 0, 0).  One component with the deepest chains there are."""
    D, H, W = shape
    v = np.zeros(shape, np.uint8)
    for z in range(0, D, 2):
        v[z, 0::2, :] = 1
        for y in range(1, H, 2):
            v[z, y, W - 1 if (y // 2) % 2 == 0 else 0] = 1
        if z + 1 < D:
            v[z + 1, 0, 0] = 1
    return v


def checkerboard(shape):
    z, y, x = np.indices(shape)
    return (1 + ((x + y + z) & 1)).astype(np.uint8)


def organ_volume(shape=(12, 40, 36), seed=21, speck_fraction=0.02):
    """Nine-class volume in the style of seg_metrics_cases.blob_pair: one ellipsoid for each class 1..8, class 3 a second time
    as an exact copy shifted along x (two equal largest components, like paired organs), then single-voxel specks of random
    foreground classes on background voxels."""
    rng = np.random.default_rng(seed)
    vol = np.zeros(shape, np.uint8)
    dims = np.asarray(shape, np.float64)
    for cid in (1, 2, 4, 5, 6, 7, 8):
        _ellipsoid(vol, rng.uniform(0.15, 0.85, 3) * (dims - 1), np.maximum(rng.uniform(0.08, 0.2, 3) * dims, 1.0), cid)
    bg = np.flatnonzero(vol.ravel() == 0)
    pick = rng.choice(bg, max(8, int(speck_fraction * vol.size)), replace=False)
    vol.ravel()[pick] = rng.integers(1, 9, pick.size).astype(np.uint8)
    blob = np.zeros((5, 7, 6), np.uint8)
    _ellipsoid(blob, np.asarray([2.0, 3.0, 2.5]), np.asarray([2.0, 3.0, 2.5]), 3)
    for x0 in (2, 20):                                      # two copies, each inside a cleared box: nothing else touches them
        vol[0:7, 29:38, x0 - 1:x0 + 7] = 0
        vol[1:6, 30:37, x0:x0 + 6] = blob
    return vol


def speckled_two_class(shape=(6, 40, 48), seed=5):
    """(prediction-to-be, label): the label is one class-1 box; the prediction is the label plus 120 far specks of class 1 --
    more than 5 % of all border voxels, so that they decide the unfiltered HD95.  Filtering the prediction with "largest" gives
    the label back."""
    rng = np.random.default_rng(seed)
    lab = np.zeros(shape, np.uint8)
    lab[1:5, 8:20, 10:24] = 1
    pred = lab.copy()
    far = pred[:, 28:, 30:]          # a view: written through
    pick = rng.choice(far.size, 120, replace=False)
    z, y, x = np.unravel_index(pick, far.shape)
    far[z, y, x] = 1
    return pred, lab


class StubNet:
    """A `net` for predict_volume that ignores the image's values: slice k of the volume gets the one-hot logits of
    class_map[k] (D, H, W), handed out in call order.  No model, no parameters."""

    def __init__(self, class_map, ncls):
        import torch
        self.onehot = torch.nn.functional.one_hot(torch.from_numpy(np.asarray(class_map, np.int64)), ncls).permute(0, 3, 1, 2).float()
        self.pos = 0

    def eval(self):
        self.pos = 0
        return self

    def __call__(self, x):
        out = self.onehot[self.pos:self.pos + x.shape[0]].to(x.device).contiguous()
        self.pos += x.shape[0]
        return out
