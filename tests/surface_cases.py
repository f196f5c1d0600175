"""Shared by tests/test_surface_host.py and tests/test_gpu_surface.py (not a test module): the scipy construction of what
ops.surface_distances returns, with the erosion and the distance transform of utils._surface_distances."""
import numpy as np
from scipy.ndimage import distance_transform_edt

from seg_metrics_cases import _border

DYADIC = [(1.0, 1.0, 1.0), (2.0, 2.0, 2.0), (4.0, 0.5, 0.25)]
GENERAL = [(2.5, 0.73, 0.73), (0.05, 1.0, 1.0), (0.3, 0.7, 1.1)]          # thick slices; thin slices; all different


def scipy_surface_lists(pred, label, ncls, spacing, ndim=None):
    """(counts int64 [ncls, 4], nq int64 [ncls, 2], segments) as include/cswin_hip.h defines them: segments[(c, dir)] is the
    ascending float64 array of DISTANCES (not squared) of class c, dir 0 = prediction's border to the label's, 1 = the reverse,
    for every class with voxels on both sides.  spacing has one entry per axis of the rule in use; ndim = 2 on a (1, H, W)
    volume means the 2-D rule on the squeezed plane."""
    pred, label = np.asarray(pred), np.asarray(label)
    ndim = pred.ndim if ndim is None else ndim
    if ndim == 2 and pred.ndim == 3:
        assert pred.shape[0] == 1
        pred, label = pred[0], label[0]
    assert len(spacing) == pred.ndim
    counts, nq, segments = np.zeros((ncls, 4), np.int64), np.zeros((ncls, 2), np.int64), {}
    for c in sorted(set(np.unique(pred).tolist()) | set(np.unique(label).tolist())):
        P, G = pred == c, label == c
        Pb, Gb = _border(P), _border(G)
        counts[c] = [P.sum(), G.sum(), (P & G).sum(), Pb.sum() + Gb.sum()]
        if c == 0 or not P.any() or not G.any():
            continue
        nq[c] = [Pb.sum(), Gb.sum()]
        for d, (a, b) in enumerate(((Pb, Gb), (Gb, Pb))):
            segments[(c, d)] = np.sort(distance_transform_edt(~b, sampling=spacing)[a])
    return counts, nq, segments


def flat_squared(nq, segments):
    """The segments as one float64 list of squared distances in the order of dist2 (each segment ascending)."""
    parts = [segments[(c, d)] ** 2 for c in range(nq.shape[0]) for d in range(2) if nq[c, d]]
    return np.concatenate(parts) if parts else np.zeros(0, np.float64)
