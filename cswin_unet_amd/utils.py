"""Loss module, segmentation metrics and the volume inference loop.

Mirrors the reference's utils.py names and call signatures:
  * ``DiceLoss(n_classes)(inputs, target, weight=None, softmax=False)``  (utils.py:9-45)  -- on the HIP path the softmax,
    one-hot, per-class sums and the gradient are one fused pass (csrc/loss.hip); there is no eager fallback.
  * ``calculate_metric_percase(pred, gt)``  (utils.py:48-58)  -- Dice and HD95.  The reference gets both from
    medpy 0.4.0 (``metric.binary.dc`` / ``hd95``), which is not installed here and not part of /root/reference: they are
    restated from medpy's published definitions.  PARITY UNPINNED for these two functions (no reference fixture holds
    their outputs); tests check them against hand-computed cases only.
  * ``test_single_volume(image, label, net, classes, patch_size, ...)``  (utils.py:61-102)  -- same per-slice arithmetic
    (cubic zoom in, argmax, nearest zoom out), but the slices of a volume go through the network in batches instead of
    one launch per slice.  ``metrics="hip"`` takes Dice / HD95 of all classes from one device call (``volume_metrics``:
    ops.seg_metrics returns integer counts and an integer histogram of squared surface distances, the host finishes in
    float64) instead of the per-class scipy loop; ``evaluate_volumes`` is the aggregating loop of test.py:155-164.
    ``voxelspacing`` / ``assd=True`` (not in the reference) score in physical units and add medpy's ASSD, on either path: the
    device then returns a list of float64 squared surface distances (ops.surface_distances) instead of the histogram.
    ``resize="hip"`` keeps the volume on the device: both zooms are linear maps whose 1-D operators ``zoom_operator`` /
    ``nearest_index`` take from scipy itself, applied by ops.resize_slices / ops.argmax_zoom_back (csrc/resize.hip).
    ``class_indices`` scores a continual model on one dataset's own output channels (universal_test.py:50-54): the argmax runs
    over ``net(x)[:, class_indices]``, on the device through the class list of ops.argmax_zoom_back.
    ``blur_sigma`` scores on the blurred copy of the data (apply_blur_test.py:79-81: ``gaussian_filter`` of every slice) without
    writing that copy: scipy per slice on the host path, ops.gaussian_blur (csrc/blur.hip, same bits) with ``resize="hip"``.
    ``components`` (not in the reference) drops, per class, the small face-connected components of the finished prediction before
    it is scored: ``filter_components_host`` (scipy.ndimage.label) on the host path, ops.filter_components (csrc/components.hip,
    same result) on the resident volume with ``resize="hip"``.
    ``tta`` (not in the reference) asks the network for several views of every slice -- symmetries of the square, the group
    ``random_rot_flip`` trains on (``tta_views``) -- and takes the argmax of the mean of the views' softmax probabilities:
    numpy in float64 on the host path, which is the definition, ops.view_batch / ops.tta_argmax_zoom_back (csrc/tta.hip) with
    ``resize="hip"``.
"""
import functools
import logging

import numpy as np
import torch
import torch.nn as nn
from scipy.ndimage import binary_erosion, distance_transform_edt, gaussian_filter, gaussian_filter1d, generate_binary_structure, rotate, zoom
from scipy.ndimage import label as ndimage_label

from . import ops


class DiceLoss(nn.Module):
    def __init__(self, n_classes):
        super().__init__()
        self.n_classes = n_classes

    def forward(self, inputs, target, weight=None, softmax=False):
        """sum_c weight[c] * (1 - (2 sum(p t) + s) / (sum(p p) + sum(t t) + s)) / n_classes, sums over the whole batch
        (utils.py:22-45).  ``softmax=True`` (how trainer.py:56 calls it): inputs are logits, the softmax is fused;
        ``softmax=False``: inputs are taken as probabilities as they are.  ``weight``: per-class factors (default all 1)."""
        if inputs.shape[1] != self.n_classes:
            raise AssertionError('predict {} & target shape do not match ({} classes)'.format(tuple(inputs.shape), self.n_classes))
        cw = None
        if weight is not None:
            if len(weight) != self.n_classes:
                raise AssertionError('weight has {} entries for {} classes'.format(len(weight), self.n_classes))
            cw = torch.as_tensor([float(w) for w in weight], dtype=torch.float32, device=inputs.device)
        loss, _ = ops.ce_dice_loss(inputs, target, w_ce=0.0, w_dice=1.0, inputs_are_probs=not softmax, class_weight=cw)
        return loss


def _surface_distances(result, reference, voxelspacing=None, connectivity=1):
    """Distances from the border voxels of `result` to the border of `reference` (medpy.metric.binary.__surface_distances)."""
    result, reference = np.atleast_1d(result.astype(bool)), np.atleast_1d(reference.astype(bool))
    if not result.any():
        raise RuntimeError('The first supplied array does not contain any binary object.')
    if not reference.any():
        raise RuntimeError('The second supplied array does not contain any binary object.')
    footprint = generate_binary_structure(result.ndim, connectivity)
    result_border = result ^ binary_erosion(result, structure=footprint, iterations=1)
    reference_border = reference ^ binary_erosion(reference, structure=footprint, iterations=1)
    dt = distance_transform_edt(~reference_border, sampling=voxelspacing)
    return dt[result_border]


def dice_coefficient(result, reference):
    """2 |A n B| / (|A| + |B|), 0 when both are empty (medpy.metric.binary.dc)."""
    result, reference = np.atleast_1d(result.astype(bool)), np.atleast_1d(reference.astype(bool))
    inter = np.count_nonzero(result & reference)
    size = np.count_nonzero(result) + np.count_nonzero(reference)
    return 2.0 * inter / float(size) if size else 0.0


def hd95(result, reference, voxelspacing=None, connectivity=1):
    """95th percentile of the symmetric surface distances (medpy.metric.binary.hd95)."""
    a = _surface_distances(result, reference, voxelspacing, connectivity)
    b = _surface_distances(reference, result, voxelspacing, connectivity)
    return float(np.percentile(np.hstack((a, b)), 95))


def _hd95_assd(a, b):
    """(hd95, assd) of the two directed lists of surface distances: the 95th percentile of both together, and the mean of the two
    directed means (medpy's assd; not the mean of the pooled list, which weighs the longer surface more)."""
    return float(np.percentile(np.hstack((a, b)), 95)), float(np.mean((a.mean(), b.mean())))


def assd(result, reference, voxelspacing=None, connectivity=1):
    """Average symmetric surface distance: the mean of the two average surface distances result -> reference and
    reference -> result (medpy.metric.binary.assd / asd)."""
    a = _surface_distances(result, reference, voxelspacing, connectivity)
    b = _surface_distances(reference, result, voxelspacing, connectivity)
    return _hd95_assd(a, b)[1]


def calculate_metric_percase(pred, gt, voxelspacing=None, assd=False):
    """(dice, hd95) of one class; (1, 0) when only the prediction is non-empty, (0, 0) otherwise (utils.py:48-58).
    voxelspacing (not in the reference, which scores in voxels): medpy's, the spacing per axis in array order; HD95 is then in
    its units.  assd=True: triples (dice, hd95, assd) -- (1, 0, 0) and (0, 0, 0) in the two degenerate branches."""
    pred, gt = np.asarray(pred).copy(), np.asarray(gt).copy()
    pred[pred > 0] = 1
    gt[gt > 0] = 1
    if pred.sum() > 0 and gt.sum() > 0:
        if not assd:
            return dice_coefficient(pred, gt), hd95(pred, gt, voxelspacing)
        return (dice_coefficient(pred, gt),) + _hd95_assd(_surface_distances(pred, gt, voxelspacing), _surface_distances(gt, pred, voxelspacing))
    elif pred.sum() > 0 and gt.sum() == 0:
        return (1, 0, 0) if assd else (1, 0)
    return (0, 0, 0) if assd else (0, 0)


def _hist_percentile(hist, q=95.0):
    """np.percentile(x, q) (linear interpolation) of the multiset x that holds hist[s] copies of sqrt(s), from the cumulative
    histogram: the two order statistics around the virtual index q/100 * (n - 1) and numpy's own lerp."""
    hist = np.asarray(hist, np.int64)
    cum = np.cumsum(hist)
    n = int(cum[-1]) if cum.size else 0
    if n == 0:
        raise RuntimeError('empty histogram')
    idx = (n - 1) * (q / 100.0)
    lo = int(np.floor(idx))
    hi = min(lo + 1, n - 1)
    t = idx - lo
    a = np.sqrt(np.float64(np.searchsorted(cum, lo, side="right")))          # order statistic k lies in the first bin with cum > k
    b = np.sqrt(np.float64(np.searchsorted(cum, hi, side="right")))
    d = b - a
    return float(a + d * t if t < 0.5 else b - d * (1 - t))


def metrics_from_counts_hist(counts, hist):
    """[(dice, hd95)] for classes 1 .. ncls-1 from what ops.seg_metrics returns (numpy: counts [ncls, 4] = |P|, |G|, |P n G|,
    |dP| + |dG|; hist [ncls, >= largest used bin + 1] of squared surface distances), with the three branches of
    calculate_metric_percase."""
    counts, hist = np.asarray(counts), np.asarray(hist)
    out = []
    for c in range(1, counts.shape[0]):
        npred, ngt, inter = int(counts[c, 0]), int(counts[c, 1]), int(counts[c, 2])
        if npred > 0 and ngt > 0:
            out.append((2.0 * inter / float(npred + ngt), _hist_percentile(hist[c])))
        elif npred > 0:
            out.append((1, 0))
        else:
            out.append((0, 0))
    return out


def metrics_from_surface_lists(counts, nq, dist2, assd=False):
    """[(dice, hd95)] or, with assd, [(dice, hd95, assd)] for classes 1 .. ncls-1 from what ops.surface_distances returns, as
    numpy arrays: counts [ncls, 4], nq [ncls, 2] and the first nq.sum() entries of dist2 with every segment sorted ascending
    (the order makes the sums, and so the result, the same on every run).  One square root of the whole list, then per class the
    host path's own arithmetic on the two directed lists (_hd95_assd) and the three branches of calculate_metric_percase."""
    counts, nq = np.asarray(counts), np.asarray(nq)
    dist2, total = np.asarray(dist2, np.float64), int(nq.sum())
    if dist2.shape[0] < total:
        raise ValueError(f"metrics_from_surface_lists: {dist2.shape[0]} distances for nq.sum() = {total}")
    d = np.sqrt(dist2[:total])
    starts = np.concatenate(([0], np.cumsum(nq.ravel())))
    out = []
    for c in range(1, counts.shape[0]):
        npred, ngt, inter = int(counts[c, 0]), int(counts[c, 1]), int(counts[c, 2])
        if npred > 0 and ngt > 0:
            a, b = d[starts[2 * c]:starts[2 * c + 1]], d[starts[2 * c + 1]:starts[2 * c + 2]]
            hd, asd = _hd95_assd(a, b)
            out.append((2.0 * inter / float(npred + ngt), hd) + ((asd,) if assd else ()))
        elif npred > 0:
            out.append((1, 0, 0) if assd else (1, 0))
        else:
            out.append((0, 0, 0) if assd else (0, 0))
    return out


def _class_ids_u8(a, classes, what, device):
    """Integral class ids in [0, classes) of any dtype (numpy or tensor) -> uint8 tensor on `device`; ValueError otherwise."""
    if isinstance(a, torch.Tensor) and a.is_cuda:
        t = a
        bad = bool((t != t.round()).any()) if t.is_floating_point() else False
        lo, hi = (float(t.min()), float(t.max())) if t.numel() else (0.0, 0.0)
    else:
        t = a.detach().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
        bad = bool(np.any(t != np.rint(t))) if t.dtype.kind == "f" else t.dtype.kind not in "biu"
        lo, hi = (float(t.min()), float(t.max())) if t.size else (0.0, 0.0)
    if bad:
        raise ValueError(f"{what}: class ids must be integral")
    if lo < 0 or hi >= classes:
        raise ValueError(f"{what}: class ids span [{lo:g}, {hi:g}], outside [0, {classes})")
    if isinstance(t, torch.Tensor):
        return t.to(torch.uint8).to(device)
    return torch.from_numpy(np.ascontiguousarray(t.astype(np.uint8))).to(device)


def _sorted_surface_lists(p8, l8, classes, spacing):
    """ops.surface_distances, again with the exact capacity if the default was too small, every (class, direction) segment sorted
    with torch.sort; (counts, nq, dist2[:nq.sum()]) as numpy arrays."""
    counts, nq, dist2 = ops.surface_distances(p8, l8, classes, spacing)
    nq_host = nq.cpu().numpy()
    total = int(nq_host.sum())
    if total > dist2.numel():
        counts, nq, dist2 = ops.surface_distances(p8, l8, classes, spacing, cap=total)
    start = 0
    for n in nq_host.ravel().tolist():
        if n > 1:
            dist2[start:start + n] = torch.sort(dist2[start:start + n]).values
        start += n
    return counts.cpu().numpy(), nq_host, dist2[:total].cpu().numpy()


def volume_metrics(pred, label, classes, device="cuda", voxelspacing=None, assd=False):
    """[(dice, hd95)] for classes 1 .. classes-1 of a (D, H, W) or (H, W) prediction / label pair -- what the loop of
    calculate_metric_percase(pred == i, label == i) returns -- from one ops.seg_metrics call.  pred / label: numpy arrays or
    tensors of any dtype holding integral ids in [0, classes) (ValueError otherwise).  HIP device only.
    voxelspacing (a number, or one entry per axis in array order: ops.voxel_spacing) and assd=True (triples with the average
    symmetric surface distance) are calculate_metric_percase's.  With either, one ops.surface_distances call returns the list of
    squared distances under the spacing (unit spacing for None) instead of the integer histogram; its segments are sorted on the
    device, downloaded, and metrics_from_surface_lists finishes.  If the list's default capacity (ops.surface_cap) was too small
    the call is repeated once with the exact size."""
    classes = int(classes)
    if not 2 <= classes <= 255:
        raise ValueError(f"volume_metrics: classes={classes} outside 2..255")
    if tuple(pred.shape) != tuple(label.shape):
        raise ValueError(f"volume_metrics: prediction {tuple(pred.shape)} and label {tuple(label.shape)} differ in shape")
    if voxelspacing is not None or assd:
        voxelspacing = ops.voxel_spacing(voxelspacing, len(pred.shape))
    p8, l8 = _class_ids_u8(pred, classes, "prediction", device), _class_ids_u8(label, classes, "label", device)
    if voxelspacing is not None:
        return metrics_from_surface_lists(*_sorted_surface_lists(p8, l8, classes, voxelspacing), assd=assd)
    counts, hist = ops.seg_metrics(p8, l8, classes)
    used = (hist != 0).any(dim=0).nonzero()
    last = int(used.max()) if used.numel() else 0                  # download only the bins in use
    return metrics_from_counts_hist(counts.cpu().numpy(), hist[:, :last + 1].cpu().numpy())


@functools.lru_cache(maxsize=None)
def zoom_operator(n_in, n_out):
    """The 1-D operator R (n_out x n_in) of ``scipy.ndimage.zoom(x, n_out / n_in, order=3)`` along an axis of n_in samples, as a
    band: ``(weights float64 [n_out][T], start int32 [n_out])`` with row i of R = weights[i] at columns start[i] .. start[i] + T.
    Column k of R is scipy's own zoom of the float64 unit vector e_k, so the spline prefilter, its mirror boundary and the
    (n_in - 1) / (n_out - 1) coordinate rule are scipy's; zoom of a 2-D slice X is R_h X R_w^T.  R decays geometrically away from
    its diagonal: a row's window covers every entry with |r| >= 2**-64 (what lies outside is below float64 rounding of the
    result), T is the widest window (at most n_in), windows are shifted to lie inside [0, n_in) and filled with the true entries
    of R.  A row may be all zero: scipy rounds the last output coordinate of 512 -> 224 past the last sample and writes its
    constant 0 there.  ValueError if scipy's output length for this pair is not n_out.  The arrays are cached: do not write to them."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise ValueError(f"zoom_operator: sizes {n_in} -> {n_out} must be positive")
    cols = [zoom(e, n_out / n_in, order=3) for e in np.eye(n_in, dtype=np.float64)]
    if any(c.shape != (n_out,) for c in cols):
        raise ValueError(f"zoom_operator: scipy zooms {n_in} samples by {n_out}/{n_in} to {cols[0].shape[0]}, not {n_out}")
    R = np.stack(cols, axis=1)
    big = np.abs(R) >= 2.0 ** -64
    lo = big.argmax(axis=1)                                         # a row without any such entry gets the window [0, 1)
    hi = np.where(big.any(axis=1), n_in - 1 - big[:, ::-1].argmax(axis=1), lo)
    T = min(n_in, int((hi - lo).max()) + 1)
    start = np.clip(lo, 0, n_in - T).astype(np.int32)
    weights = np.ascontiguousarray(R[np.arange(n_out)[:, None], start[:, None] + np.arange(T)[None, :]])
    weights.setflags(write=False)
    start.setflags(write=False)
    return weights, start


@functools.lru_cache(maxsize=None)
def nearest_index(n_in, n_out):
    """int32 [n_out]: the source index ``scipy.ndimage.zoom(x, n_out / n_in, order=0)`` picks for every output sample along an
    axis of n_in samples, read off scipy's zoom of arange(n_in) + 1.  An output whose coordinate scipy rounds past the last
    sample is not gathered at all: scipy writes its constant 0 there (the last output of 512 -> 224), and the entry is -1.
    ``zoom(lab, ..., order=0)`` is ``lab[np.ix_(ih, iw)]`` where both indices are >= 0 and 0 elsewhere.  Cached."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise ValueError(f"nearest_index: sizes {n_in} -> {n_out} must be positive")
    src = zoom(np.arange(1, n_in + 1, dtype=np.float64), n_out / n_in, order=0)
    if src.shape != (n_out,):
        raise ValueError(f"nearest_index: scipy zooms {n_in} samples by {n_out}/{n_in} to {src.shape[0]}, not {n_out}")
    idx = src.astype(np.int32) - 1
    if np.any(idx + 1 != src) or idx.min() < -1 or idx.max() >= n_in:
        raise ValueError(f"nearest_index: scipy's order-0 zoom of 1..{n_in} is not an index vector")
    idx.setflags(write=False)
    return idx


@functools.lru_cache(maxsize=None)
def rotation_index(H, W, angle):
    """int32 [H, W] map m: the flat source index ``scipy.ndimage.rotate(x, angle, order=0, reshape=False)`` reads for every
    output pixel of an (H, W) slice, -1 where scipy writes its constant 0.  It is read off scipy's rotation of the float64 image
    arange(1, H * W + 1): order 0 copies values exactly, so that rotation of x is
    ``np.where(m >= 0, x.ravel()[np.maximum(m, 0)], 0)`` for every dtype.  angle: an integer number of degrees (the augmentation
    draws -20..19: at most 40 maps per shape, 1 MiB each at 512 x 512, filled as they are asked for).  ValueError for sizes
    outside 1..2048 and if scipy's result is not an index map.  Cached: do not write to it."""
    H, W = int(H), int(W)
    if not (1 <= H <= 2048 and 1 <= W <= 2048):
        raise ValueError(f"rotation_index: slice ({H}, {W}) outside 1..2048 per dimension")
    if int(angle) != angle:
        raise ValueError(f"rotation_index: angle {angle!r} is not an integer number of degrees")
    src = rotate(np.arange(1, H * W + 1, dtype=np.float64).reshape(H, W), int(angle), order=0, reshape=False)
    idx = src.astype(np.int32) - 1
    if src.shape != (H, W) or np.any(idx + 1 != src) or idx.min() < -1 or idx.max() >= H * W:
        raise ValueError(f"rotation_index: scipy's order-0 rotation of 1..{H * W} by {angle} degrees is not an index map")
    idx.setflags(write=False)
    return idx


@functools.lru_cache(maxsize=None)
def _gaussian_taps(sigma, truncate):
    r = int(truncate * sigma + 0.5)
    if r > 32:
        raise ValueError(f"gaussian_taps: sigma={sigma:g}, truncate={truncate:g} give radius {r}; 0..32 is supported")
    impulse = np.zeros(4 * r + 3, np.float64)
    impulse[2 * r + 1] = 1.0
    w = np.ascontiguousarray(gaussian_filter1d(impulse, sigma, truncate=truncate)[r + 1:3 * r + 2])
    if w.shape != (2 * r + 1,) or not np.array_equal(w, w[::-1]):
        raise ValueError(f"gaussian_taps: scipy's impulse response for sigma={sigma:g} is not a symmetric kernel of {2 * r + 1} taps")
    w.setflags(write=False)
    return w, r


def gaussian_taps(sigma, truncate=4.0):
    """``(weights float64 [2r + 1], r)``: the taps of ``scipy.ndimage.gaussian_filter1d(x, sigma, truncate=truncate)`` and its
    radius r = int(truncate * sigma + 0.5).  The weights are scipy's own: its response to a float64 unit impulse in the middle of
    4r + 3 samples (no boundary reaches the 2r + 1 read out), so the exponential and its normalisation are not restated here.
    ValueError for a sigma or truncate that is not finite and positive, for taps that are not exactly symmetric (the device
    folds them, as scipy's correlate1d does) and for r > 32.  Cached: do not write to the array."""
    sigma, truncate = float(sigma), float(truncate)
    if not (np.isfinite(sigma) and sigma > 0):
        raise ValueError(f"gaussian_taps: sigma={sigma!r} must be finite and positive")
    if not (np.isfinite(truncate) and truncate > 0):
        raise ValueError(f"gaussian_taps: truncate={truncate!r} must be finite and positive")
    return _gaussian_taps(sigma, truncate)


_device_tables = {}


def zoom_operator_device(n_in, n_out, device):
    """zoom_operator's (weights, start) as tensors on `device`, uploaded once per (size pair, device)."""
    key = ("zoom", int(n_in), int(n_out), torch.device(device))
    if key not in _device_tables:
        w, s = zoom_operator(n_in, n_out)
        _device_tables[key] = (torch.from_numpy(w.copy()).to(device), torch.from_numpy(s.copy()).to(device))
    return _device_tables[key]


def nearest_index_device(n_in, n_out, device):
    """nearest_index as a tensor on `device`, uploaded once per (size pair, device)."""
    key = ("nearest", int(n_in), int(n_out), torch.device(device))
    if key not in _device_tables:
        _device_tables[key] = torch.from_numpy(nearest_index(n_in, n_out).copy()).to(device)
    return _device_tables[key]


def rotation_index_device(H, W, angle, device):
    """rotation_index as a tensor on `device`, uploaded once per (H, W, angle, device)."""
    key = ("rotation", int(H), int(W), int(angle), torch.device(device))
    if key not in _device_tables:
        _device_tables[key] = torch.from_numpy(rotation_index(H, W, angle).copy()).to(device)
    return _device_tables[key]


def gaussian_taps_device(sigma, truncate, device):
    """gaussian_taps' first half ``w[-r] .. w[0]`` (what cswin_gaussian_blur reads) as a float64 tensor on `device`, and r;
    uploaded once per (sigma, truncate, device), blocking for the reason ops.augment_batch's docstring gives."""
    key = ("gauss", float(sigma), float(truncate), torch.device(device))
    if key not in _device_tables:
        w, r = gaussian_taps(sigma, truncate)
        _device_tables[key] = (torch.from_numpy(w[:r + 1].copy()).to(device), r)
    return _device_tables[key]


def signed_distance_maps_host(labels, ncls):
    """The boundary loss's signed distance maps (Kervadec et al., MIDL 2019: one_hot2dist), the definition ops.signed_distance_maps
    is held to bit for bit.  labels (B, H, W) integers -> float32 (B, ncls, H, W): per sample and class, with M = (labels[b] == c),
    edt(~M) * ~M - (edt(M) - 1) * M in float64 with scipy.ndimage.distance_transform_edt per 2-D slice at unit spacing -- +d(p, M)
    outside the mask, -(d(p, ~M) - 1) inside -- rounded to float32; zeros where M is empty or the whole slice (no boundary: scipy's
    transform of an all-true mask is no distance).  A label outside [0, ncls) equals no c: its pixel is outside every mask."""
    lab = np.asarray(labels.cpu() if torch.is_tensor(labels) else labels)
    if lab.ndim != 3 or not np.issubdtype(lab.dtype, np.integer):
        raise ValueError(f"signed_distance_maps_host: labels must be (B, H, W) integers, got {lab.dtype} {lab.shape}")
    phi = np.zeros((lab.shape[0], int(ncls)) + lab.shape[1:], np.float32)
    for b in range(lab.shape[0]):
        for c in range(int(ncls)):
            m = lab[b] == c
            if m.any() and not m.all():
                phi[b, c] = distance_transform_edt(~m) * ~m - (distance_transform_edt(m) - 1.0) * m
    return phi


def mix64_host(z):
    """csrc/layout.hip's mix64 on numpy uint64 (any shape): the whole splitmix64 step, increment included."""
    z = np.asarray(z, np.uint64)
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def intensity_noise_host(seed, n):
    """The n standard normals n(seed, i), i < n, of the intensity augmentation's noise stage, float64: Box-Muller's cosine branch
    on the two 24-bit uniforms of r = mix64(mix64(seed) ^ i), u1 = ((r >> 40) + 1) / 2^24 in (0, 1], u2 = ((r >> 16) & 0xFFFFFF)
    / 2^24 in [0, 1).  csrc/intensity.hip generates the same on the device."""
    r = mix64_host(mix64_host(np.uint64(seed)) ^ np.arange(n, dtype=np.uint64))
    u1 = ((r >> np.uint64(40)) + np.uint64(1)).astype(np.float64) / 2.0 ** 24
    u2 = ((r >> np.uint64(16)) & np.uint64(0xFFFFFF)).astype(np.float64) / 2.0 ** 24
    return np.sqrt(-2 * np.log(u1)) * np.cos(2 * np.pi * u2)


def intensity_host(x, draw):
    """THE DEFINITION of the intensity augmentation (ops.intensity_batch is held to it): x one float32 image (h, w), draw one
    datasets.INTENSITY_DRAW record.  The stages in this order, each only if its flag is on:
      blur        scipy.ndimage.gaussian_filter(x, sigma) on the float32 image, float32 result (ops.gaussian_blur's semantics)
      noise       z[i] += noise_std * intensity_noise_host(seed, h * w)[i], i the row-major pixel index
      brightness  z *= brightness
      contrast    m, lo, hi = mean, min, max of z;  z = clip((z - m) * contrast + m, lo, hi)
      gamma       (z = -z if invert)  m0, s0 = mean, std (ddof=0);  lo = min, rng = max - lo;
                  z = ((z - lo) / (rng + 1e-7)) ** gamma * rng + lo;  z = (z - mean(z)) / (std(z) + 1e-8) * s0 + m0  (z = -z again)
    Apart from the blur everything is float64 from the float32 values, rounded to float32 once at the end; with every flag off the
    image comes back bit for bit."""
    from .datasets import check_intensity_draws
    x = np.asarray(x)
    if x.dtype != np.float32 or x.ndim != 2:
        raise ValueError(f"intensity_host: x is {x.dtype} {x.shape}; one float32 image (h, w) is augmented")
    d = check_intensity_draws(draw, 1)[0]
    if d["do_blur"]:
        x = gaussian_filter(x, float(d["sigma"]))
    z = x.astype(np.float64)
    if d["do_noise"]:
        z = z + float(d["noise_std"]) * intensity_noise_host(d["seed"], z.size).reshape(z.shape)
    if d["do_brightness"]:
        z = z * float(d["brightness"])
    if d["do_contrast"]:
        m, lo, hi = z.mean(), z.min(), z.max()
        z = np.clip((z - m) * float(d["contrast"]) + m, lo, hi)
    if d["do_gamma"]:
        if d["invert"]:
            z = -z
        m0, s0 = z.mean(), z.std()
        lo = z.min()
        rng = z.max() - lo
        z = ((z - lo) / (rng + 1e-7)) ** float(d["gamma"]) * rng + lo
        z = (z - z.mean()) / (z.std() + 1e-8) * s0 + m0
        if d["invert"]:
            z = -z
    return z.astype(np.float32)


def component_rule_tables(rule, ncls):
    """The per-class tables of a component filter rule: ``(min_size int64 [ncls], min_fraction float64 [ncls])``.  rule is
    "largest" (min_fraction 1 for every foreground class) or a mapping {class_id: {"min_size": int, "min_fraction": float}} with
    either key optional; classes that are not named get (0, 0.0) and stay untouched, entry 0 (background) is never used.  A
    component of class c is kept iff its voxel count is >= max(min_size[c], ceil(min_fraction[c] * largest component of c)).
    ValueError for ncls outside 2..255, another rule, a class id outside 1..ncls-1, a negative or non-integral min_size, a
    min_fraction outside [0, 1] and an unknown key."""
    ncls = int(ncls)
    if not 2 <= ncls <= 255:
        raise ValueError(f"component rule: ncls={ncls} outside 2..255")
    ms, mf = np.zeros(ncls, np.int64), np.zeros(ncls, np.float64)
    if isinstance(rule, str):
        if rule != "largest":
            raise ValueError(f'component rule: {rule!r} is not "largest" or a mapping of class ids')
        mf[1:] = 1.0
        return ms, mf
    if not hasattr(rule, "items"):
        raise ValueError(f'component rule: {rule!r} is not "largest" or a mapping of class ids')
    for c, spec in rule.items():
        if isinstance(c, bool) or not isinstance(c, (int, np.integer)) or not 1 <= c < ncls:
            raise ValueError(f"component rule: {c!r} is not a foreground class id in [1, {ncls})")
        if not hasattr(spec, "items") or set(spec) - {"min_size", "min_fraction"}:
            raise ValueError(f'component rule: class {c}: {spec!r} must be a mapping with the keys "min_size" and / or "min_fraction"')
        size, frac = spec.get("min_size", 0), spec.get("min_fraction", 0.0)
        if isinstance(size, bool) or not isinstance(size, (int, np.integer)) or not 0 <= size < 2 ** 63:
            raise ValueError(f"component rule: class {c}: min_size={size!r} must be a non-negative integer")
        if isinstance(frac, bool) or not isinstance(frac, (int, float, np.integer, np.floating)) or not 0.0 <= frac <= 1.0:
            raise ValueError(f"component rule: class {c}: min_fraction={frac!r} must lie in [0, 1]")
        ms[c], mf[c] = int(size), float(frac)
    return ms, mf


def filter_components_host(vol, ncls, rule):
    """The component filter in scipy: per class c the rule names, ``scipy.ndimage.label(vol == c)`` (face neighbours), the
    threshold max(min_size, ceil(min_fraction * largest)) in float64, and every smaller component set to 0.  vol: integer array
    (D, H, W) or (H, W); ids 0 and >= ncls pass through.  Returns a new array of vol's dtype.  The host path of
    predict_volume(components=...) and what ops.filter_components computes on the device."""
    ms, mf = component_rule_tables(rule, ncls)
    vol = np.asarray(vol)
    out = vol.copy()
    for c in range(1, int(ncls)):
        if ms[c] == 0 and mf[c] == 0.0:
            continue
        lab, n = ndimage_label(vol == c)
        if n == 0:
            continue
        sizes = np.bincount(lab.ravel(), minlength=n + 1)
        thr = max(int(ms[c]), int(np.ceil(np.float64(mf[c]) * np.float64(sizes[1:].max()))))
        keep = sizes >= thr
        keep[0] = True                                                  # everything that is not class c
        out[~keep[lab]] = 0
    return out


TTA_VIEW_NAMES = {"identity": 0, "transpose": 1, "flip_rows": 2, "rot90": 3, "flip_cols": 4, "rot270": 5, "rot180": 6, "anti_transpose": 7}


def tta_views(spec):
    """The views of a test-time-augmentation spec as a tuple of codes 0..7, or None for None.  A code c is a symmetry of the
    square: bit 0 transposes, bit 1 reverses the rows, bit 2 the columns, in that order (apply_view) -- the group that training's
    random_rot_flip draws from.  spec: "flips" = (0, 2, 4, 6), the views that keep a slice's shape; "d4" = all eight; or a
    sequence of 1..8 distinct codes or names (TTA_VIEW_NAMES: "rot90" = 3 is np.rot90(x, 1), "rot270" = 5 is np.rot90(x, 3)).
    ValueError naming the entry for anything else (another string, a bool, a code outside 0..7, a repeated view)."""
    if spec is None:
        return None
    if isinstance(spec, str):
        if spec not in ("flips", "d4"):
            raise ValueError(f'tta: {spec!r} is not "flips", "d4" or a sequence of view codes or names')
        return (0, 2, 4, 6) if spec == "flips" else tuple(range(8))
    try:
        entries = list(spec)
    except TypeError:
        raise ValueError(f'tta: {spec!r} is not "flips", "d4" or a sequence of view codes or names') from None
    if not 1 <= len(entries) <= 8:
        raise ValueError(f"tta: {len(entries)} views; 1..8 distinct ones are supported")
    codes = []
    for k, e in enumerate(entries):
        if isinstance(e, str) and e in TTA_VIEW_NAMES:
            c = TTA_VIEW_NAMES[e]
        elif not isinstance(e, (bool, str)) and isinstance(e, (int, np.integer)) and 0 <= e <= 7:
            c = int(e)
        else:
            raise ValueError(f"tta: entry {k}, {e!r}, is not a view code in 0..7 or one of {sorted(TTA_VIEW_NAMES)}")
        if c in codes:
            raise ValueError(f"tta: entry {k}, {e!r}, repeats view {c}")
        codes.append(c)
    return tuple(codes)


def apply_view(x, code):
    """View `code` of the last two axes of a numpy array (a numpy view, nothing is copied)."""
    a = np.swapaxes(x, -1, -2) if code & 1 else x
    a = np.flip(a, -2) if code & 2 else a
    return np.flip(a, -1) if code & 4 else a


def undo_view(a, code):
    """The inverse of apply_view: undo_view(apply_view(x, c), c) is x."""
    a = np.flip(a, -1) if code & 4 else a
    a = np.flip(a, -2) if code & 2 else a
    return np.swapaxes(a, -1, -2) if code & 1 else a


def tta_view_position(code, r, s, h, w):
    """(i, j) of source pixel (r, s) of an (h, w) slice in the frame of view `code`: apply_view(x, code)[i, j] is x[r, s].  The
    index map of csrc/tta_plan.h (tta_view_pos), which the kernels read the views' logits through."""
    hv, wv = (w, h) if code & 1 else (h, w)
    i2, j2 = (s, r) if code & 1 else (r, s)
    return (hv - 1 - i2 if code & 2 else i2), (wv - 1 - j2 if code & 4 else j2)


def _check_tta_patch(views, patch_size):
    if views is not None and patch_size[0] != patch_size[1] and any(c & 1 for c in views):
        bad = [c for c in views if c & 1]
        raise ValueError(f"predict_volume: tta views {bad} transpose the network's input, which needs a square patch_size, "
                         f"got {tuple(patch_size)}")


def ensemble_views_host(logits, views, class_indices):
    """The definition of the ensemble on downloaded logits (V * b, ncls, h', w'): float64 softmax over the listed channels per
    view, back to the source frame, the mean over the views, torch.argmax (first index, first NaN).  Returns (cls int64 (b, h, w),
    P float64 (b, nsel, h, w))."""
    V = len(views)
    L = logits.detach().double().cpu().numpy()
    L = L if class_indices is None else L[:, list(class_indices)]
    L = L.reshape((V, L.shape[0] // V) + L.shape[1:])
    P = 0.0
    with np.errstate(invalid="ignore", over="ignore"):
        for v, c in enumerate(views):
            e = np.exp(L[v] - L[v].max(axis=1, keepdims=True))
            P = P + undo_view(e / e.sum(axis=1, keepdims=True), c)
        P = np.ascontiguousarray(P / V)
    return torch.argmax(torch.from_numpy(P), dim=1).numpy(), P


def _predict_volume_hip_tta(vol, net, patch_size, batch_slices, device, class_indices, blur_sigma, components, views):
    """_predict_volume_hip with a view ensemble: per batch (gaussian_blur ->) resize_slices -> view_batch -> ONE network call on
    V * b samples -> tta_argmax_zoom_back into the resident uint8 volume.  b = max(1, batch_slices // V), so the network's batch
    stays what the caller sized it for."""
    D, x, y = vol.shape
    if blur_sigma is not None and vol.dtype != np.float32:
        raise ValueError(f'predict_volume: blur_sigma with resize="hip" takes float32 volumes, got {vol.dtype} (scipy blurs in the '
                         f'volume\'s own dtype); use resize="host"')
    dvol = torch.from_numpy(np.ascontiguousarray(vol)).to(device)
    resize = x != patch_size[0] or y != patch_size[1]
    if not resize:
        dvol = dvol.float()
    pred = torch.empty((D, x, y), dtype=torch.uint8, device=dvol.device)
    b = max(1, batch_slices // len(views))
    for d0 in range(0, D, b):
        sl = dvol[d0:d0 + b]
        if blur_sigma is not None:
            sl = ops.gaussian_blur(sl, blur_sigma)
        inp = ops.resize_slices(sl, patch_size) if resize else sl
        seen = ops.view_batch(inp, views)
        logits = net(seen.view(-1, 1, seen.shape[2], seen.shape[3]))
        pred[d0:d0 + b] = ops.tta_argmax_zoom_back(logits, views, (x, y), classes=class_indices)
    if components is not None and D > 0:
        ops.filter_components(pred, _class_count(logits, class_indices), components, out=pred)
    return pred


def _predict_volume_hip(vol, net, patch_size, batch_slices, device, class_indices=None, blur_sigma=None, components=None):
    """predict_volume's loop with the volume resident on the device: upload once, per batch (gaussian_blur ->) resize_slices ->
    net -> argmax_zoom_back (over class_indices, if given) into a uint8 (D, H, W) device volume, which filter_components then
    cleans in place if a component rule is given."""
    D, x, y = vol.shape
    if blur_sigma is not None and vol.dtype != np.float32:
        raise ValueError(f'predict_volume: blur_sigma with resize="hip" takes float32 volumes, got {vol.dtype} (scipy blurs in the '
                         f'volume\'s own dtype); use resize="host"')
    dvol = torch.from_numpy(np.ascontiguousarray(vol)).to(device)
    resize = x != patch_size[0] or y != patch_size[1]
    if not resize:
        dvol = dvol.float()
    pred = torch.empty((D, x, y), dtype=torch.uint8, device=dvol.device)
    for d0 in range(0, D, batch_slices):
        sl = dvol[d0:d0 + batch_slices]
        if blur_sigma is not None:
            sl = ops.gaussian_blur(sl, blur_sigma)
        inp = ops.resize_slices(sl, patch_size) if resize else sl
        logits = net(inp.unsqueeze(1))
        pred[d0:d0 + batch_slices] = ops.argmax_zoom_back(logits, (x, y), classes=class_indices)
    if components is not None and D > 0:
        ops.filter_components(pred, _class_count(logits, class_indices), components, out=pred)
    return pred


def _class_count(logits, class_indices):
    """How many classes a finished class map can hold: the listed output channels, or all of them."""
    return logits.shape[1] if class_indices is None else len(class_indices)


@torch.no_grad()
def predict_volume(image, net, patch_size=(224, 224), batch_slices=16, device="cuda", resize="host", return_device=False,
                   class_indices=None, blur_sigma=None, components=None, tta=None):
    """image (D, H, W) or (H, W) numpy -> integer class map of the same shape.  Per slice: cubic zoom to patch_size if the
    size differs, network, argmax over classes (softmax is monotonic, utils.py:75), nearest zoom back (:70-81).
    resize: "host" = scipy's zooms per slice around batched network calls; "hip" = the volume is uploaded once, both zooms and
    the argmax run on the device (same values; float32 / float64 volumes, integer ones only when nothing is resized) and only the
    finished volume comes back, as the uint8 array it is on the device (the host path returns int64) -- or, with
    return_device=True, stays there as a uint8 tensor.
    class_indices: None, or the output channels of one dataset in a continual model (continual.task_class_indices): the argmax
    runs over net(x)[:, class_indices] and the result is the position in that list, the dataset's own class id
    (universal_test.py:50-54); the hip path passes the list to ops.argmax_zoom_back instead of slicing the logits.
    blur_sigma: None, or the sigma of scipy.ndimage.gaussian_filter applied to every slice on its own before the cubic zoom
    (apply_blur_test.py:79-81): scipy in the volume's own dtype on the host path, ops.gaussian_blur per batch of slices with
    resize="hip" (also when nothing is resized), which takes float32 volumes only (ValueError otherwise).
    components: None (nothing is filtered), or a component filter rule (component_rule_tables: "largest" or a mapping per class id)
    applied to the finished class map of the whole volume -- with class_indices that means the dataset's own ids: per class, the
    face-connected components smaller than the rule's threshold become 0.  scipy on the host path (filter_components_host),
    ops.filter_components on the resident volume with resize="hip".  ValueError for a rule that names a class the map cannot hold.
    tta: None (one forward pass per slice, the code above call for call), or a test-time-augmentation spec (tta_views: "flips",
    "d4", or a sequence of view codes / names): the network sees every view of every slice, in one call on V * b samples with
    b = max(1, batch_slices // V), and the class is the argmax of the MEAN over the views of the softmax probabilities, each
    taken back to the slice's own frame -- probabilities, not logits: they are bounded, so one over-confident view cannot outvote
    the rest.  The host path is the definition: np.flip / np.swapaxes around the scipy zooms, softmax and mean in float64 on
    the downloaded logits, torch.argmax.  resize="hip" makes the views with ops.view_batch and ensembles with
    ops.tta_argmax_zoom_back in float32 (csrc/tta.hip), which can move a class only where the two best probabilities are
    within ~1e-6.  A transposing view (an odd code) needs a square patch_size: ValueError before the network runs.
    class_indices, blur_sigma, components and return_device compose as without tta."""
    views = tta_views(tta)
    _check_tta_patch(views, patch_size)
    if resize not in ("host", "hip"):
        raise ValueError(f'predict_volume: resize must be "host" or "hip", got {resize!r}')
    if return_device and resize != "hip":
        raise ValueError('predict_volume: return_device needs resize="hip"')
    if blur_sigma is not None:
        gaussian_taps(blur_sigma)                                       # ValueError for a sigma neither path takes
    if components is not None:
        component_rule_tables(components, 255 if class_indices is None else max(2, len(class_indices)))      # malformed rules fail before the network runs
    image = np.asarray(image)
    single = image.ndim == 2
    vol = image[None] if single else image
    net.eval()
    if resize == "hip":
        if views is None:
            pred = _predict_volume_hip(vol, net, tuple(patch_size), batch_slices, device, class_indices, blur_sigma, components)
        else:
            pred = _predict_volume_hip_tta(vol, net, tuple(patch_size), batch_slices, device, class_indices, blur_sigma, components, views)
        pred = pred if return_device else pred.cpu().numpy()
        return pred[0] if single else pred
    D, x, y = vol.shape
    resize = x != patch_size[0] or y != patch_size[1]
    pred = np.zeros((D, x, y), np.int64)
    if views is not None:
        batch_slices = max(1, batch_slices // len(views))
    for d0 in range(0, D, batch_slices):
        sl = vol[d0:d0 + batch_slices]
        if blur_sigma is not None:
            sl = np.stack([gaussian_filter(s, blur_sigma) for s in sl])
        if resize:
            sl = np.stack([zoom(s, (patch_size[0] / x, patch_size[1] / y), order=3) for s in sl])
        if views is None:
            inp = torch.from_numpy(np.ascontiguousarray(sl)).unsqueeze(1).float().to(device)
            logits = net(inp)
            out = torch.argmax(logits if class_indices is None else logits[:, list(class_indices)], dim=1).cpu().numpy()
        else:
            seen = np.concatenate([apply_view(sl, c) for c in views])
            logits = net(torch.from_numpy(np.ascontiguousarray(seen)).unsqueeze(1).float().to(device))
            out, _ = ensemble_views_host(logits, views, class_indices)
        for i, o in enumerate(out):
            pred[d0 + i] = zoom(o, (x / patch_size[0], y / patch_size[1]), order=0) if resize else o
    if components is not None and D > 0:
        pred = filter_components_host(pred, _class_count(logits, class_indices), components)
    return pred[0] if single else pred


def test_single_volume(image, label, net, classes, patch_size=[256, 256], test_save_path=None, case=None, z_spacing=1,
                       batch_slices=16, device="cuda", metrics="host", resize="host", class_indices=None, blur_sigma=None,
                       components=None, voxelspacing=None, assd=False, tta=None):
    """Per-class (dice, hd95) of one volume, classes 1..classes-1 (utils.py:61-102).  image / label: (1, D, H, W) tensors
    as the DataLoader yields them.  With test_save_path the volumes are written as .npz (SimpleITK, which the reference
    uses for .nii.gz, is not installed here).  metrics: "host" = the per-class scipy loop, "hip" = one volume_metrics call on
    the device (same values).  resize: predict_volume's; with resize="hip" and metrics="hip" the prediction goes from the one to
    the other as a device tensor and is downloaded only to be saved.  class_indices: predict_volume's; it must name `classes`
    channels (ValueError otherwise), the labels being that dataset's own ids 0..classes-1.  blur_sigma: predict_volume's; the
    saved .npz keeps the image as it was passed in.  components: predict_volume's component filter rule, checked against
    `classes` (ValueError for a class id >= classes); the prediction is filtered before it is scored -- on the device with
    resize="hip", so with metrics="hip" it still never leaves it -- and the saved .npz holds the filtered prediction.
    voxelspacing, assd: calculate_metric_percase's / volume_metrics', for either value of `metrics`: the spacing of the volume's
    axes (D, H, W) that HD95 (and ASSD) are measured in, and (dice, hd95, assd) triples.  A bad spacing raises ValueError before
    the network runs.  z_spacing is unrelated: it only goes into the saved .npz.  tta: predict_volume's view ensemble, checked
    (tta_views, and a square patch for a transposing view) before anything else runs."""
    _check_tta_patch(tta_views(tta), patch_size)
    if class_indices is not None and len(class_indices) != classes:
        raise ValueError(f"test_single_volume: class_indices has {len(class_indices)} entries for classes={classes}")
    if metrics not in ("host", "hip"):
        raise ValueError(f'test_single_volume: metrics must be "host" or "hip", got {metrics!r}')
    if resize not in ("host", "hip"):
        raise ValueError(f'test_single_volume: resize must be "host" or "hip", got {resize!r}')
    if components is not None:
        component_rule_tables(components, classes)
    image, label = image.squeeze(0).cpu().detach().numpy(), label.squeeze(0).cpu().detach().numpy()
    if voxelspacing is not None:
        voxelspacing = ops.voxel_spacing(voxelspacing, label.ndim)
    on_device = resize == "hip" and metrics == "hip"
    prediction = predict_volume(image, net, tuple(patch_size), batch_slices, device, resize=resize, return_device=on_device,
                                class_indices=class_indices, blur_sigma=blur_sigma, components=components, tta=tta)
    if not on_device:
        prediction = prediction.astype(label.dtype)
    if metrics == "hip":
        metric_list = volume_metrics(prediction, label, classes, device, voxelspacing=voxelspacing, assd=assd)
    else:
        metric_list = [calculate_metric_percase(prediction == i, label == i, voxelspacing=voxelspacing, assd=assd) for i in range(1, classes)]
    if on_device and test_save_path is not None:
        prediction = prediction.cpu().numpy()
    if test_save_path is not None:
        np.savez_compressed(f"{test_save_path}/{case}_pred.npz", image=image.astype(np.float32),
                            prediction=prediction.astype(np.float32), label=label.astype(np.float32),
                            spacing=np.asarray((1, 1, z_spacing), np.float32))
    return metric_list


test_single_volume.__test__ = False     # not a pytest test (the name is the reference's)


def evaluate_volumes(loader, net, classes, patch_size, metrics="hip", test_save_path=None, z_spacing=1, batch_slices=16,
                     device="cuda", resize="host", class_indices=None, blur_sigma=None, components=None, voxelspacing=None, assd=False,
                     tta=None):
    """The volume loop of the reference's inference() (test.py:155-164): test_single_volume per batch of `loader` (dicts with
    "image", "label" (1, D, H, W) and "case_name", batch size 1), the per-volume and final lines it logs.  Returns
    (per_volume, class_mean, mean_dice, mean_hd95): the metric list of every volume, the (classes-1, 2) table of per-class
    means over the volumes, and that table's column means.  class_indices, blur_sigma, components, tta: test_single_volume's
    (a bad tta raises ValueError before the loader is read).
    voxelspacing: test_single_volume's, one spacing for every volume or a dict case name -> spacing (KeyError naming a case it
    lacks).  assd=True: the metric lists hold triples, class_mean is (classes-1, 3), the log lines gain mean_assd and the return
    a fifth element, mean_assd."""
    _check_tta_patch(tta_views(tta), patch_size)
    per_volume = []
    for i_batch, batch in enumerate(loader):
        name = batch["case_name"]
        name = name if isinstance(name, str) else name[0]
        spacing = voxelspacing
        if isinstance(voxelspacing, dict):
            if name not in voxelspacing:
                raise KeyError(f"evaluate_volumes: voxelspacing has no entry for case {name!r}")
            spacing = voxelspacing[name]
        metric_i = test_single_volume(batch["image"], batch["label"], net, classes=classes, patch_size=list(patch_size),
                                      test_save_path=test_save_path, case=name, z_spacing=z_spacing, batch_slices=batch_slices,
                                      device=device, metrics=metrics, resize=resize, class_indices=class_indices,
                                      blur_sigma=blur_sigma, components=components, voxelspacing=spacing, assd=assd, tta=tta)
        per_volume.append(metric_i)
        m = np.mean(metric_i, axis=0)
        logging.info('idx %d case %s mean_dice %f mean_hd95 %f' % (i_batch, name, m[0], m[1]) + (' mean_assd %f' % m[2] if assd else ''))
    if not per_volume:
        raise ValueError("evaluate_volumes: the loader yielded no volume")
    class_mean = sum(np.array(m, dtype=np.float64) for m in per_volume) / len(per_volume)
    for i in range(1, classes):
        logging.info('Mean class %d mean_dice %f mean_hd95 %f' % (i, class_mean[i - 1][0], class_mean[i - 1][1])
                     + (' mean_assd %f' % class_mean[i - 1][2] if assd else ''))
    means = tuple(float(v) for v in np.mean(class_mean, axis=0))
    logging.info('Testing performance in best val model: mean_dice : %f mean_hd95 : %f' % means[:2] + (' mean_assd : %f' % means[2] if assd else ''))
    return (per_volume, class_mean) + means
