"""Host side of the device metrics path (no GPU): utils.metrics_from_counts_hist turns the integer counts and the histogram of
squared surface distances that ops.seg_metrics returns into the (dice, hd95) pairs of calculate_metric_percase.  Here counts and
hist are built with scipy (tests/seg_metrics_cases.py), so the host finish is pinned independently of the kernels.

Tolerances: Dice is one float64 division of the same integers on both sides: equal exactly.  HD95: both sides take correctly
rounded float64 square roots of the same integers and interpolate once in float64; they can differ by a few ulp (~1e-15), so
rel = abs = 1e-12 is a derived bound, not a measured one."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from seg_metrics_cases import blob_pair, nbins_of, scipy_counts_hist, special_pair

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = dict(rel=1e-12, abs=1e-12)


def _host_list(pred, label, ncls):
    from cswin_unet_amd.utils import calculate_metric_percase
    return [calculate_metric_percase(pred == i, label == i) for i in range(1, ncls)]


def _check(got, want):
    assert len(got) == len(want)
    for c, (g, w) in enumerate(zip(got, want), start=1):
        assert g[0] == w[0], (c, g, w)
        assert g[1] == pytest.approx(w[1], **TOL), (c, g, w)


CASES = {
    "special3d": lambda: special_pair((12, 40, 36), 1) + (9,),
    "special2d": lambda: special_pair((48, 52), 2) + (9,),
    "blobs3d": lambda: blob_pair((9, 33, 41), [1, 2, 3, 4, 5], 3) + (6,),
    "blobs2d": lambda: blob_pair((40, 40), [1, 2, 3], 4) + (4,),
    "identical": lambda: (lambda p: (p, p.copy(), 9))(special_pair((10, 30, 30), 5)[0]),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_metrics_from_counts_hist_matches_host_per_class(name):
    from cswin_unet_amd.utils import metrics_from_counts_hist
    pred, label, ncls = CASES[name]()
    counts, hist = scipy_counts_hist(pred, label, ncls)
    got = metrics_from_counts_hist(counts, hist)
    want = _host_list(pred, label, ncls)
    _check(got, want)
    if name.startswith("special"):
        assert want[4] == (1, 0) and want[5] == (0, 0) and want[6] == (0, 0) and want[7][0] == 0.0 and want[7][1] > 0
        assert got[4] == (1, 0) and got[5] == (0, 0) and got[6] == (0, 0)
    if name == "identical":
        assert all(g == (1.0, 0.0) for g, w in zip(got, want) if w[0] > 0)
    for c in range(1, ncls):                                         # the histogram's own invariant
        both = counts[c, 0] > 0 and counts[c, 1] > 0
        assert hist[c].sum() == (counts[c, 3] if both else 0)


def test_trimmed_histogram_gives_the_same_result():
    from cswin_unet_amd.utils import metrics_from_counts_hist
    pred, label, ncls = CASES["special3d"]()
    counts, hist = scipy_counts_hist(pred, label, ncls)
    last = int(np.nonzero(hist.any(axis=0))[0].max())
    assert metrics_from_counts_hist(counts, hist[:, :last + 1]) == metrics_from_counts_hist(counts, hist)


def test_histogram_percentile_matches_numpy_on_the_expanded_multiset():
    from cswin_unet_amd.utils import _hist_percentile
    rng = np.random.default_rng(7)
    hists = [np.array([0, 0, 1]), np.array([1]), np.array([0, 1, 0, 0, 1]), np.array([2]), np.array([0, 0, 0, 977, 0]),
             np.array([19, 1]), np.array([1, 19]), np.array([10, 0, 0, 10])]
    for _ in range(200):
        nb = int(rng.integers(1, 400))
        h = rng.integers(0, 6, nb) * (rng.random(nb) < rng.uniform(0.05, 1.0))
        if h.sum() == 0:
            h[int(rng.integers(0, nb))] = int(rng.integers(1, 4))
        hists.append(h.astype(np.int64))
    for h in hists:
        want = float(np.percentile(np.repeat(np.sqrt(np.arange(len(h), dtype=np.float64)), h), 95))
        assert _hist_percentile(h) == pytest.approx(want, **TOL), h
    with pytest.raises(RuntimeError):
        _hist_percentile(np.zeros(5, np.int64))


def test_no_cpu_fallback():
    from cswin_unet_amd import ops
    from cswin_unet_amd._lib import CswinHipError
    from cswin_unet_amd.utils import volume_metrics
    pred, label = blob_pair((4, 16, 16), [1, 2], 0)
    with pytest.raises(CswinHipError):
        volume_metrics(pred, label, 3, device="cpu")
    with pytest.raises(CswinHipError):
        ops.seg_metrics(torch.from_numpy(pred), torch.from_numpy(label), 3)
    with pytest.raises(CswinHipError):
        volume_metrics(torch.from_numpy(pred).float(), torch.from_numpy(label).float(), 3, device="cpu")


def test_bad_class_ids_raise_value_error():
    from cswin_unet_amd.utils import volume_metrics
    pred, label = blob_pair((4, 16, 16), [1, 2], 0)
    with pytest.raises(ValueError):
        volume_metrics(pred, label, 2, device="cpu")                  # id 2 out of range
    with pytest.raises(ValueError):
        volume_metrics(pred.astype(np.int64) - 1, label, 3, device="cpu")          # negative id
    half = label.astype(np.float32)
    half[0, 0, 0] = 0.5
    with pytest.raises(ValueError):
        volume_metrics(pred, half, 3, device="cpu")
    with pytest.raises(ValueError):
        volume_metrics(pred, torch.from_numpy(half), 3, device="cpu")
    with pytest.raises(ValueError):
        volume_metrics(pred, label[:, :8], 3, device="cpu")
    with pytest.raises(ValueError):
        volume_metrics(pred, label, 256, device="cpu")


def test_abi_additions():
    from cswin_unet_amd import _lib
    h = _lib.lib()
    header = open(os.path.join(ROOT, "include", "cswin_hip.h")).read()
    for name in ("cswin_seg_metrics_nbins", "cswin_seg_metrics_workspace", "cswin_seg_metrics"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES and hasattr(h, name)
    assert h.cswin_abi_version() == 4 == _lib.ABI_VERSION
    assert _lib.SIGNATURES["cswin_seg_metrics_workspace"][0] is ctypes.c_size_t


def test_size_queries_are_host_only():
    from cswin_unet_amd import _lib
    h = _lib.lib()
    assert h.cswin_seg_metrics_nbins(148, 512, 512) == 147 ** 2 + 2 * 511 ** 2 + 1 == nbins_of((148, 512, 512))
    assert h.cswin_seg_metrics_nbins(1, 40, 40) == 2 * 39 ** 2 + 1
    assert h.cswin_seg_metrics_workspace(148, 512, 512, 3, 9) > 2 * 148 * 512 * 512
    assert h.cswin_seg_metrics_workspace(1, 224, 224, 2, 9) > 0
    assert h.cswin_seg_metrics_workspace(2, 64, 64, 2, 9) == 0                   # ndim = 2 needs D == 1
    assert b"ndim" in h.cswin_last_error()
    assert h.cswin_seg_metrics_workspace(4, 4096, 64, 3, 9) == 0 and b"2048" in h.cswin_last_error()
    assert h.cswin_seg_metrics_workspace(4, 64, 64, 3, 256) == 0 and b"ncls" in h.cswin_last_error()
    assert h.cswin_seg_metrics_nbins(0, 64, 64) == 0


def test_test_single_volume_rejects_unknown_metrics_mode():
    from cswin_unet_amd.utils import test_single_volume
    with pytest.raises(ValueError):
        test_single_volume(torch.zeros(1, 2, 8, 8), torch.zeros(1, 2, 8, 8), None, 3, metrics="device")
