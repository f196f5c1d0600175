"""Shared by tests/test_seg_metrics_host.py and tests/test_gpu_seg_metrics.py (not a test module): seeded blob volumes and the
scipy construction of what ops.seg_metrics returns, with the same erosion and distance transform as utils._surface_distances."""
import numpy as np
from scipy.ndimage import binary_erosion, distance_transform_edt, generate_binary_structure


def _ellipsoid(vol, center, radii, value):
    """vol[...] = value inside the axis-aligned ellipsoid (any rank), touching only its bounding box."""
    lo = [max(0, int(np.floor(c - r))) for c, r in zip(center, radii)]
    hi = [min(n, int(np.ceil(c + r)) + 1) for c, r, n in zip(center, radii, vol.shape)]
    if any(a >= b for a, b in zip(lo, hi)):
        return
    grids = np.ogrid[tuple(slice(a, b) for a, b in zip(lo, hi))]
    inside = sum(((g - c) / max(r, 0.5)) ** 2 for g, c, r in zip(grids, center, radii)) <= 1.0
    sub = vol[tuple(slice(a, b) for a, b in zip(lo, hi))]
    sub[inside] = value


def blob_pair(shape, class_ids, seed, jitter=2.0, rmin=0.08, rmax=0.22):
    """(pred, label) uint8 volumes of `shape`: one ellipsoid per id in class_ids (later ones overwrite earlier ones); the
    prediction's ellipsoid is the label's with its centre moved by up to `jitter` voxels and its radii scaled by 0.8 .. 1.2."""
    rng = np.random.default_rng(seed)
    pred, label = np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)
    dims = np.asarray(shape, np.float64)
    for cid in class_ids:
        center = rng.uniform(0.15, 0.85, len(shape)) * (dims - 1)
        radii = np.maximum(rng.uniform(rmin, rmax, len(shape)) * dims, 1.0)
        _ellipsoid(label, center, radii, cid)
        _ellipsoid(pred, center + rng.uniform(-jitter, jitter, len(shape)), radii * rng.uniform(0.8, 1.2, len(shape)), cid)
    return pred, label


def special_pair(shape, seed):
    """Nine-class pair with the awkward classes: 1 touches the array boundary (a corner), 2-4 ordinary blobs, 5 only in the
    prediction, 6 only in the label, 7 absent from both, 8 a single voxel on each side."""
    pred, label = blob_pair(shape, [2, 3, 4], seed)
    dims = np.asarray(shape, np.float64)
    corner = np.zeros(len(shape))
    _ellipsoid(label, corner, np.maximum(0.2 * dims, 1.5), 1)
    _ellipsoid(pred, corner, np.maximum(0.25 * dims, 1.5), 1)
    far = tuple(n - 1 for n in shape)
    _ellipsoid(pred, np.asarray(far, np.float64), np.maximum(0.12 * dims, 1.0), 5)
    mid = tuple(n // 2 for n in shape)
    low = tuple([shape[0] - 1] + [n // 2 for n in shape[1:]])
    _ellipsoid(label, np.asarray(low, np.float64), np.maximum(0.1 * dims, 1.0), 6)
    pred[pred == 6] = 0
    label[label == 5] = 0
    pred[mid] = 8
    label[tuple(min(n - 1, m + 3) for n, m in zip(shape, mid))] = 8
    assert (pred == 8).sum() == 1 and (label == 8).sum() == 1 and not (pred == 7).any() and not (label == 7).any()
    assert (pred == 5).any() and not (label == 5).any() and (label == 6).any() and not (pred == 6).any()
    return pred, label


def _border(mask):
    return mask ^ binary_erosion(mask, structure=generate_binary_structure(mask.ndim, 1), iterations=1)


def nbins_of(shape):
    return int(sum((n - 1) ** 2 for n in shape)) + 1


def scipy_counts_hist(pred, label, ncls, ndim=None):
    """counts int64 [ncls, 4] and hist int32 [ncls, nbins] as include/cswin_hip.h defines them, built with scipy.  pred / label:
    (D, H, W) or (H, W); ndim = 2 on a (1, H, W) volume means the 2-D rule on the squeezed plane."""
    pred, label = np.asarray(pred), np.asarray(label)
    nbins = nbins_of(pred.shape)
    ndim = pred.ndim if ndim is None else ndim
    if ndim == 2 and pred.ndim == 3:
        assert pred.shape[0] == 1
        pred, label = pred[0], label[0]
    counts, hist = np.zeros((ncls, 4), np.int64), np.zeros((ncls, nbins), np.int32)
    present = set(np.unique(pred).tolist()) | set(np.unique(label).tolist())
    for c in sorted(present):
        P, G = pred == c, label == c
        Pb, Gb = _border(P), _border(G)
        counts[c] = [P.sum(), G.sum(), (P & G).sum(), Pb.sum() + Gb.sum()]
        if c == 0 or not P.any() or not G.any():
            continue
        for a, b in ((Pb, Gb), (Gb, Pb)):
            d = distance_transform_edt(~b)[a]
            hist[c] += np.bincount(np.rint(d ** 2).astype(np.int64), minlength=nbins).astype(np.int32)
    return counts, hist
