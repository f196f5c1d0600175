"""Host side of the spacing-aware surface metrics (no GPU): utils.assd, calculate_metric_percase(voxelspacing=, assd=),
ops.voxel_spacing, the finish utils.metrics_from_surface_lists on lists built with scipy (tests/surface_cases.py), the argument
checks that run before anything touches a device, and the C entry points' error contract (every check of cswin_surface_dist
returns before the first HIP call, so it is callable here with placeholder pointers).

Tolerances: hand-made cases use spacings and gaps whose products are exact in float64 and are compared with ==.  Where the finish
is compared with the host loop both sides hold the same distances up to one rounding (sqrt(d * d) against d) and sum them in
another order, a few ulp; rel = abs = 1e-12 is the project's bound for that (tests/test_gpu_seg_metrics.py)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from seg_metrics_cases import blob_pair, special_pair
from surface_cases import DYADIC, GENERAL, flat_squared, scipy_surface_lists

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = dict(rel=1e-12, abs=1e-12)


def _planes(gap):
    a, b = np.zeros((10, 6, 7), bool), np.zeros((10, 6, 7), bool)
    a[2], b[2 + gap] = True, True
    return a, b


def test_assd_and_hd95_of_parallel_planes_are_gap_times_spacing():
    from cswin_unet_amd.utils import assd, calculate_metric_percase, hd95
    a, b = _planes(3)
    assert assd(a, b) == 3.0 and hd95(a, b) == 3.0
    for sp, want in (((2.5, 1.0, 1.0), 7.5), ((0.25, 3.0, 3.0), 0.75), (2.0, 6.0)):
        assert assd(a, b, voxelspacing=sp) == want and hd95(a, b, voxelspacing=sp) == want
        assert calculate_metric_percase(a, b, voxelspacing=sp, assd=True) == (0.0, want, want)
        assert calculate_metric_percase(a, b, voxelspacing=sp) == (0.0, want)
    assert assd(a, a) == 0.0


def test_assd_is_the_mean_of_the_directed_means_not_the_pooled_mean():
    from cswin_unet_amd.utils import assd
    a, b = np.zeros((3, 12), bool), np.zeros((3, 12), bool)
    a[1, 0] = True                                   # a -> b: [0]
    b[1, 0] = b[1, 10] = True                        # b -> a: [0, 10]
    assert assd(a, b) == 2.5 == assd(b, a)           # (0 + 5) / 2; the pooled mean would be 10 / 3
    assert assd(a, b, voxelspacing=(1.0, 0.5)) == 1.25
    with pytest.raises(RuntimeError):
        assd(a, np.zeros_like(a))


def test_calculate_metric_percase_branches_with_assd():
    from cswin_unet_amd.utils import calculate_metric_percase
    a, b = _planes(2)
    empty = np.zeros_like(a)
    assert calculate_metric_percase(a, b, assd=True) == (0.0, 2.0, 2.0)
    assert calculate_metric_percase(a, empty, assd=True) == (1, 0, 0)
    assert calculate_metric_percase(empty, b, assd=True) == (0, 0, 0)
    assert calculate_metric_percase(empty, empty, assd=True) == (0, 0, 0)
    assert calculate_metric_percase(a, b) == (0.0, 2.0) and calculate_metric_percase(a, empty) == (1, 0)          # defaults unchanged
    assert calculate_metric_percase(empty, b) == (0, 0)


def test_voxel_spacing_normalisation_and_errors():
    from cswin_unet_amd.ops import voxel_spacing
    assert voxel_spacing(None, 3) == (1.0, 1.0, 1.0) and voxel_spacing(None, 2) == (1.0, 1.0)
    assert voxel_spacing(2, 3) == (2.0, 2.0, 2.0) and voxel_spacing(np.float32(0.5), 2) == (0.5, 0.5)
    assert voxel_spacing([2.5, 0.73, 0.73], 3) == (2.5, 0.73, 0.73)
    assert voxel_spacing(np.array([3, 1]), 2) == (3.0, 1.0) and voxel_spacing(torch.tensor([3.0, 1.0]), 2) == (3.0, 1.0)
    assert all(type(v) is float for v in voxel_spacing(np.array([3, 1]), 2))
    for bad, ndim in (((1, 1), 3), ((1, 1, 1), 2), ((), 2), ((1, 0, 1), 3), ((1, -2.0, 1), 3), ((1, float("nan"), 1), 3),
                      ((1, float("inf")), 2), (0, 3), (-1.0, 2), (float("nan"), 3), ("abc", 3), ((1, None, 1), 3)):
        with pytest.raises(ValueError):
            voxel_spacing(bad, ndim)


def test_finish_on_hand_made_segments():
    from cswin_unet_amd.utils import metrics_from_surface_lists
    rng = np.random.default_rng(5)
    seg = {(1, 0): np.sort(rng.uniform(0, 9, 37)), (1, 1): np.sort(rng.uniform(0, 9, 5)),
           (3, 0): np.array([4.0]), (3, 1): np.array([0.5, 0.5, 4.0])}
    seg = {k: v ** 2 for k, v in seg.items()}                       # the lists hold squared distances
    counts = np.array([[900, 900, 800, 50], [40, 30, 20, 42], [7, 0, 0, 7], [1, 3, 0, 4], [0, 5, 0, 5]], np.int64)
    nq = np.array([[0, 0], [37, 5], [0, 0], [1, 3], [0, 0]], np.int64)
    dist2 = np.concatenate([seg[(1, 0)], seg[(1, 1)], seg[(3, 0)], seg[(3, 1)]])
    got = metrics_from_surface_lists(counts, nq, dist2, assd=True)
    assert len(got) == 4 and got[1] == (1, 0, 0) and got[3] == (0, 0, 0)
    for c in (1, 3):
        a, b = np.sqrt(seg[(c, 0)]), np.sqrt(seg[(c, 1)])
        want = (2.0 * counts[c, 2] / (counts[c, 0] + counts[c, 1]), float(np.percentile(np.hstack((a, b)), 95)), float(np.mean((a.mean(), b.mean()))))
        assert got[c - 1] == want                                    # the same numpy calls on the same values
    assert got[2] == (0.0, float(np.percentile([4.0, 0.5, 0.5, 4.0], 95)), (4.0 + 5.0 / 3) / 2)
    pairs = metrics_from_surface_lists(counts, nq, dist2)
    assert pairs == [g[:2] for g in got] and pairs[1] == (1, 0)
    assert metrics_from_surface_lists(counts, nq, np.concatenate([dist2, [np.nan, -1.0]]), assd=True)[2] == got[2]          # the tail is never read
    with pytest.raises(ValueError):
        metrics_from_surface_lists(counts, nq, dist2[:-1])


@pytest.mark.parametrize("spacing", DYADIC[2:] + GENERAL[:1])
def test_finish_on_scipy_lists_matches_the_host_loop(spacing):
    from cswin_unet_amd.utils import calculate_metric_percase, metrics_from_surface_lists
    pred, label = special_pair((12, 40, 36), 1)
    counts, nq, segments = scipy_surface_lists(pred, label, 9, spacing)
    assert [k for k in sorted(segments)] == [(c, d) for c in (1, 2, 3, 4, 8) for d in (0, 1)]
    assert (nq.sum(axis=1) == np.where((counts[:, 0] > 0) & (counts[:, 1] > 0) & (np.arange(9) > 0), counts[:, 3], 0)).all()
    got = metrics_from_surface_lists(counts, nq, flat_squared(nq, segments), assd=True)
    want = [calculate_metric_percase(pred == i, label == i, voxelspacing=spacing, assd=True) for i in range(1, 9)]
    assert got[4] == (1, 0, 0) == want[4] and got[5] == (0, 0, 0) == want[5] and got[6] == (0, 0, 0)
    for g, w in zip(got, want):
        assert g[0] == w[0] and g[1] == pytest.approx(w[1], **TOL) and g[2] == pytest.approx(w[2], **TOL), (g, w)
    assert want[7][0] == 0.0 and want[7][1] == want[7][2] > 0         # the single voxels: one distance each way


def test_default_capacity():
    from cswin_unet_amd.ops import SURFACE_CAP_EXACT, SURFACE_CAP_FRACTION, surface_cap
    assert surface_cap(12 * 40 * 36) == 2 * 12 * 40 * 36              # the exact worst case: every voxel a border voxel on both sides
    assert surface_cap(SURFACE_CAP_EXACT // 2) == SURFACE_CAP_EXACT and surface_cap(SURFACE_CAP_EXACT // 2 + 1) == SURFACE_CAP_EXACT
    n = 148 * 512 * 512
    assert surface_cap(n) == n // SURFACE_CAP_FRACTION > SURFACE_CAP_EXACT


def test_arguments_are_checked_before_any_device_work():
    from cswin_unet_amd import ops
    from cswin_unet_amd._lib import CswinHipError
    from cswin_unet_amd.utils import evaluate_volumes, test_single_volume, volume_metrics
    pred, label = blob_pair((4, 16, 16), [1, 2], 0)
    tp, tl = torch.from_numpy(pred), torch.from_numpy(label)
    with pytest.raises(CswinHipError):
        ops.surface_distances(tp, tl, 3, (1, 1, 1))                  # CPU tensors: no fallback
    with pytest.raises(CswinHipError):
        volume_metrics(pred, label, 3, device="cpu", voxelspacing=(2.5, 1, 1))
    with pytest.raises(CswinHipError):
        volume_metrics(pred, label, 3, device="cpu", assd=True)
    for bad in ((1, 1), (1, 0, 1), (1, -1, 1), (1, float("nan"), 1)):
        with pytest.raises(ValueError):
            volume_metrics(pred, label, 3, device="cpu", voxelspacing=bad)
        with pytest.raises(ValueError):
            test_single_volume(tp[None].float(), tl[None].float(), None, 3, voxelspacing=bad)          # before the network (None) runs
    with pytest.raises(ValueError):
        volume_metrics(pred[0], label[0], 3, device="cpu", voxelspacing=(1, 1, 1))          # a plane takes two entries
    loader = [{"image": tp[None].float(), "label": tl[None].float(), "case_name": ["case7"]}]
    with pytest.raises(KeyError, match="case7"):
        evaluate_volumes(loader, None, 3, [16, 16], voxelspacing={"case1": (1, 1, 1)}, assd=True)
    from cswin_unet_amd.continual import evaluate_tasks
    with pytest.raises(KeyError, match="case7"):                      # both keywords reach evaluate_volumes through the task loop
        evaluate_tasks(None, {0: loader}, [3], [16, 16], num_classes=3, voxelspacing={"case1": (1, 1, 1)}, assd=True)
    with pytest.raises(ValueError, match="voxelspacing"):
        evaluate_tasks(None, {0: loader}, [3], [16, 16], num_classes=3, voxelspacing=(1, 1), assd=True)


def test_abi_additions_and_size_query():
    from cswin_unet_amd import _lib
    h = _lib.lib()
    header = open(os.path.join(ROOT, "include", "cswin_hip.h")).read()
    for name in ("cswin_surface_dist_workspace", "cswin_surface_dist"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES and hasattr(h, name)
    assert "cswin_surface_dist*" in header.split("#define CSWIN_ABI_VERSION")[0]          # on the "only ADDED" list
    assert h.cswin_abi_version() == 4 == _lib.ABI_VERSION
    assert _lib.SIGNATURES["cswin_surface_dist_workspace"] == (ctypes.c_size_t, [ctypes.c_int] * 5)
    for dims in ((148, 512, 512, 3, 9), (1, 224, 224, 2, 9), (5, 33, 71, 3, 200)):          # the histogram path's, plus offsets and counters
        assert h.cswin_surface_dist_workspace(*dims) == h.cswin_seg_metrics_workspace(*dims) + 2 * ((dims[4] * 16 + 15) // 16 * 16)
    assert h.cswin_surface_dist_workspace(2, 64, 64, 2, 9) == 0 and b"ndim" in h.cswin_last_error()
    assert h.cswin_surface_dist_workspace(4, 4096, 64, 3, 9) == 0 and b"2048" in h.cswin_last_error()
    assert h.cswin_surface_dist_workspace(4, 64, 64, 3, 256) == 0 and b"ncls" in h.cswin_last_error()


def test_entry_point_error_codes():
    """Every argument check returns before the first HIP call, so placeholder host pointers are never dereferenced."""
    from cswin_unet_amd import _lib
    h = _lib.lib()
    SHAPE, ALIGN, WORKSPACE = -1, -2, -3
    D, H, W, ncls = 4, 16, 16, 3
    need = h.cswin_surface_dist_workspace(D, H, W, 3, ncls)
    buf = ctypes.create_string_buffer(need + 64)
    base = (ctypes.addressof(buf) + 15) // 16 * 16
    p = ctypes.c_void_p

    def call(pred=base, label=base, counts=base, nq=base, dist2=base, cap=10, ws=base, ws_bytes=need, ndim=3, n=ncls, sp=(1.0, 1.0, 1.0)):
        return h.cswin_surface_dist(p(pred), p(label), p(counts), p(nq), p(dist2), cap, p(ws), ws_bytes, D, H, W, ndim, n, *sp, None)

    for name in ("pred", "label", "counts", "nq", "dist2"):
        assert call(**{name: None}) == SHAPE and b"null" in h.cswin_last_error(), name
    assert call(cap=-1) == SHAPE and b"cap" in h.cswin_last_error()
    for sp in ((0.0, 1.0, 1.0), (1.0, -1.0, 1.0), (1.0, 1.0, float("nan")), (float("inf"), 1.0, 1.0)):
        assert call(sp=sp) == SHAPE and b"spacing" in h.cswin_last_error(), sp
    assert call(ndim=2) == SHAPE and b"ndim" in h.cswin_last_error()          # D = 4
    assert call(n=1) == SHAPE and b"ncls" in h.cswin_last_error()
    assert call(ws_bytes=need - 1) == WORKSPACE and call(ws=None) == WORKSPACE
    assert call(ws=base + 8) == ALIGN
    for name in ("counts", "nq", "dist2"):
        assert call(**{name: base + 4}) == ALIGN, name
