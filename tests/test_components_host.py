"""Host side of the component filter: utils.filter_components_host and the canonical labels of tests/components_cases.py on
cases small enough to check by hand, the rule parser and its errors, the `components` keyword of predict_volume on the host path
with a stub network, and the union-find core of the kernels (csrc/components_uf.h) run single-threaded through the kernels' three
passes by tools/components_host_check.cpp.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from components_cases import StubNet, canonical_labels, organ_volume, rule_tables, scipy_filter, speckled_two_class

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _filter(vol, ncls, rule):
    from cswin_unet_amd.utils import filter_components_host
    return filter_components_host(vol, ncls, rule)


def test_diagonal_blobs_stay_two_components():
    v = np.zeros((1, 4, 4), np.uint8)
    v[0, 0:2, 0:2] = 1
    v[0, 2:4, 2:4] = 1                                  # touches the first blob at a corner only
    labels, sizes = canonical_labels(v, 2)
    assert sorted(np.unique(labels).tolist()) == [0, 1, 11]          # roots at flat 0 and flat 2 * 4 + 2
    assert sizes.ravel()[0] == 4 and sizes.ravel()[10] == 4 and sizes.sum() == 8
    v[0, 3, 3] = 0                                      # now 4 and 3 voxels
    assert np.array_equal(_filter(v, 2, "largest"), np.where(canonical_labels(v, 2)[0] == 1, 1, 0))
    w = np.zeros((2, 2, 2), np.uint8)
    w[0, 0, 0] = w[1, 1, 0] = 1                         # an edge contact across z
    assert np.unique(canonical_labels(w, 2)[0]).tolist() == [0, 1, 7]


def test_adjacent_classes_do_not_merge():
    v = np.zeros((1, 2, 6), np.uint8)
    v[0, :, 0:3] = 1
    v[0, :, 3:6] = 2
    labels, sizes = canonical_labels(v, 3)
    assert labels[0, 0, 0] == 1 and labels[0, 1, 2] == 1 and labels[0, 0, 3] == 4 and labels[0, 1, 5] == 4
    assert sizes.ravel()[0] == 6 and sizes.ravel()[3] == 6 and sizes.sum() == 12
    assert np.array_equal(_filter(v, 3, "largest"), v)


def test_ids_past_ncls_are_ignored():
    v = np.zeros((1, 3, 5), np.uint8)
    v[0, 0, 0:3] = 1
    v[0, 2, 4] = 1
    v[0, 1, :] = 7                                      # >= ncls: never labelled, never removed, and it does not join anything
    labels, sizes = canonical_labels(v, 4)
    assert (labels[0, 1] == 0).all() and sizes[0, 1].sum() == 0
    out = _filter(v, 4, "largest")
    assert (out[0, 1] == 7).all() and out[0, 2, 4] == 0 and (out[0, 0, 0:3] == 1).all()


def test_equal_largest_components_are_both_kept():
    v = np.zeros((1, 1, 12), np.uint8)
    v[0, 0, 0:3] = v[0, 0, 5:8] = 1
    v[0, 0, 10] = 1
    out = _filter(v, 2, "largest")
    assert out[0, 0].tolist() == [1, 1, 1, 0, 0, 1, 1, 1, 0, 0, 0, 0]


def test_min_size_and_min_fraction_combine_by_max():
    v = np.zeros((1, 1, 30), np.uint8)
    v[0, 0, 0:10] = 1                                   # sizes 10, 5, 3, 1
    v[0, 0, 12:17] = 1
    v[0, 0, 20:23] = 1
    v[0, 0, 28] = 1
    kept = lambda rule: sorted({int(s) for s in canonical_labels(_filter(v, 2, {1: rule}), 2)[1].ravel() if s})
    assert kept({"min_size": 3}) == [3, 5, 10]
    assert kept({"min_fraction": 0.45}) == [5, 10]                      # ceil(4.5) = 5
    assert kept({"min_size": 2, "min_fraction": 0.45}) == [5, 10]       # the fraction is the larger bound
    assert kept({"min_size": 6, "min_fraction": 0.3}) == [10]           # the size is
    assert kept({"min_fraction": 0.3}) == [3, 5, 10]                    # ceil(3.0) = 3: a size equal to the bound stays
    assert kept({"min_size": 11}) == []                                 # nothing reaches it, not even the largest
    assert kept({}) == [1, 3, 5, 10]


@pytest.mark.parametrize("rule", ["largest", {3: {"min_fraction": 0.5}, 5: {"min_size": 4}}, {c: {"min_size": 3, "min_fraction": 0.25} for c in range(1, 9)}])
def test_host_filter_equals_the_component_by_component_rule(rule):
    vol = organ_volume()
    sizes3 = sorted(canonical_labels(vol == 3, 2)[1].ravel().tolist())[-2:]
    assert sizes3[0] == sizes3[1] > 20                                  # the duplicated organ: a tie for the largest
    got = _filter(vol, 9, rule)
    assert got.dtype == vol.dtype and np.array_equal(got, scipy_filter(vol, 9, *rule_tables(rule, 9)))
    if rule == "largest":
        assert (canonical_labels(got == 3, 2)[1] > 0).sum() == 2 and (got != vol).any()
    as64 = _filter(vol.astype(np.int64), 9, rule)                       # the host path's dtype
    assert as64.dtype == np.int64 and np.array_equal(as64, got)


def test_rule_parsing():
    from cswin_unet_amd.utils import component_rule_tables
    ms, mf = component_rule_tables("largest", 4)
    assert ms.dtype == np.int64 and mf.dtype == np.float64 and ms.tolist() == [0, 0, 0, 0] and mf.tolist() == [0.0, 1.0, 1.0, 1.0]
    ms, mf = component_rule_tables({2: {"min_size": 7}, 3: {"min_fraction": 0.5, "min_size": np.int64(2)}}, 4)
    assert ms.tolist() == [0, 0, 7, 2] and mf.tolist() == [0.0, 0.0, 0.0, 0.5]
    assert component_rule_tables({}, 2)[0].tolist() == [0, 0]
    for bad in ("biggest", None, 3, [1, 2],
                {0: {"min_size": 1}}, {4: {"min_size": 1}}, {-1: {"min_size": 1}}, {"1": {"min_size": 1}}, {1.0: {"min_size": 1}},
                {1: {"min_size": -1}}, {1: {"min_size": 2.5}}, {1: {"min_fraction": 1.5}}, {1: {"min_fraction": -0.1}},
                {1: {"min_fraction": float("nan")}}, {1: {"size": 3}}, {1: 5}):
        with pytest.raises(ValueError):
            component_rule_tables(bad, 4)
    for ncls in (1, 256):
        with pytest.raises(ValueError):
            component_rule_tables("largest", ncls)


def test_predict_volume_host_path_filters_the_finished_map():
    from cswin_unet_amd.utils import predict_volume
    pred, _ = speckled_two_class()
    image = np.zeros(pred.shape, np.float32)
    kw = dict(patch_size=pred.shape[1:], batch_slices=4, device="cpu", resize="host")
    plain = predict_volume(image, StubNet(pred, 2), **kw)
    assert plain.dtype == np.int64 and np.array_equal(plain, pred)
    assert np.array_equal(predict_volume(image, StubNet(pred, 2), components=None, **kw), plain)
    got = predict_volume(image, StubNet(pred, 2), components="largest", **kw)
    assert got.dtype == np.int64 and np.array_equal(got, scipy_filter(plain, 2, [0, 0], [0.0, 1.0])) and (got != plain).any()
    one = predict_volume(image[2], StubNet(pred[2:3], 2), components={1: {"min_size": 2}}, **kw)          # a single slice: 2-D rule
    assert one.shape == pred.shape[1:] and np.array_equal(one, scipy_filter(pred[2], 2, [0, 2], [0.0, 0.0]))
    with pytest.raises(ValueError):
        predict_volume(image, StubNet(pred, 2), components={2: {"min_size": 1}}, **kw)                    # the map holds ids 0 and 1
    with pytest.raises(ValueError):
        predict_volume(image, StubNet(pred, 2), components="smallest", **kw)


def test_single_volume_checks_the_rule_against_classes():
    import torch
    from cswin_unet_amd.utils import test_single_volume
    pred, lab = speckled_two_class()
    image, label = torch.zeros((1,) + pred.shape), torch.from_numpy(lab)[None]
    kw = dict(classes=2, patch_size=list(pred.shape[1:]), batch_slices=4, device="cpu")
    with pytest.raises(ValueError):
        test_single_volume(image, label, StubNet(pred, 2), components={2: {"min_size": 1}}, **kw)
    raw = test_single_volume(image, label, StubNet(pred, 2), **kw)
    flt = test_single_volume(image, label, StubNet(pred, 2), components="largest", **kw)
    assert flt == [(1.0, 0.0)] and raw[0][0] < 1.0 and raw[0][1] > 0.0          # the filtered prediction is the label itself


def test_union_find_core_on_the_host(tmp_path):
    """tools/components_host_check.cpp: find / union / the skipped-link rule of csrc/components_uf.h, single-threaded, through the
    tile, seam and flatten passes against a flood fill -- noise, serpentines, checkerboard, solid, degenerate shapes."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "components_host_check")
    subprocess.run([cxx, "-O1", "-std=c++17", "-I", os.path.join(ROOT, "cswin_unet_amd", "csrc"),
                    os.path.join(ROOT, "tools", "components_host_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0 and "all cases agree" in run.stdout, run.stdout + run.stderr
