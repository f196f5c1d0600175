"""Host side of the component filter: utils.filter_components_host and the canonical labels of tests/components_cases.py on
cases small enough to check by hand, the rule parser and its errors, the `components` keyword of predict_volume on the host path
with a stub network, and the union-find core of the kernels (csrc/components_uf.h) run single-threaded through the kernels' three
passes by tools/components_host_check.cpp.  Then what tests/test_gpu_components_shapes.py rests on: the vectorised filter reference
against the two older ones, the properties the contention volumes are there for, and the case tables against the kernels' branch
conditions restated in Python.  No GPU."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import components_cases as C
from components_cases import StubNet, canonical_labels, filter_ref, organ_volume, rule_tables, scipy_filter, speckled_two_class

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
    tile, seam and flatten passes against a flood fill -- noise, serpentines, checkerboard, solid, degenerate shapes, percolating
    noise, W % 4 == 2, ids at and past ncls across a seam in x, y and z.  A device mismatch on such a volume then points at
    concurrency, not at the link rule."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "components_host_check")
    subprocess.run([cxx, "-O1", "-std=c++17", "-I", os.path.join(ROOT, "cswin_unet_amd", "csrc"),
                    os.path.join(ROOT, "tools", "components_host_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0 and "all cases agree" in run.stdout, run.stdout + run.stderr


# ---- what tests/test_gpu_components_shapes.py rests on ---------------------------------------------------------------------------
def _small_filter_volumes():
    """Every small volume the device filter is tried on, with its ncls and rule."""
    for name, (build, ncls, rule) in C.FILTER_CASES.items():
        yield name, build(), ncls, rule
    for W in C.LABEL_W:
        yield f"label.W{W}", C.label_volume(W), C.LABEL_NCLS, {1: {"min_fraction": 0.5}, 2: {"min_size": 4}}
    for name, (shape, ids, ncls) in C.LABEL_IDS.items():
        yield name, C.ids_volume(shape, ids, 41), ncls, "largest"
    for axis in range(3):
        for name, (a, b) in C.SEAM_IDS.items():
            yield f"seam.{axis}.{name}", C.seam_lanes(axis, a, b), 3, "largest"


def test_filter_ref_equals_the_two_older_references():
    from test_gpu_components import ORGAN_RULES
    vol = organ_volume()
    for name, rule in ORGAN_RULES.items():
        want = scipy_filter(vol, 9, *rule_tables(rule, 9))
        assert np.array_equal(filter_ref(vol, 9, *rule_tables(rule, 9)), want) and np.array_equal(_filter(vol, 9, rule), want), name
        assert (want != vol).any()
    changed = set()
    for name, v, ncls, rule in _small_filter_volumes():
        ms, mf = rule_tables(rule, ncls)
        got = filter_ref(v, ncls, ms, mf)
        assert got.dtype == v.dtype and np.array_equal(got, scipy_filter(v, ncls, ms, mf)), name
        assert np.array_equal(got, _filter(v, ncls, rule)), name
        assert np.array_equal(got[v >= ncls], v[v >= ncls])                  # ids past ncls come back as they went in
        if (got != v).any():
            changed.add(name)
    assert changed >= set(C.FILTER_CASES) - {"n3"}                           # every rule removes something; three voxels are too few


def test_filter_cases_hold_what_they_are_there_for():
    def sizes_in(v, c):
        return sorted(s for s in canonical_labels(v == c, 2)[1].ravel().tolist() if s)

    def sizes_of(name, c):
        return sizes_in(C.FILTER_CASES[name][0](), c)

    def kept(name, c):
        build, ncls, rule = C.FILTER_CASES[name]
        return sizes_in(filter_ref(build(), ncls, *rule_tables(rule, ncls)), c)
    # the two products that are not exact in float64 land on either side of the integer
    assert 0.1 * 30.0 == 3.0 and math.ceil(0.1 * 30.0) == 3 and 0.07 * 100.0 > 7.0 and math.ceil(0.07 * 100.0) == 8
    assert sizes_of("ceil", 1) == [2, 3, 3, 4, 4, 30] and kept("ceil", 1) == [3, 3, 4, 4, 30]          # equal to the threshold: stays
    assert sizes_of("ceil_up", 1) == [6, 7, 7, 8, 100] and kept("ceil_up", 1) == [8, 100]
    assert sizes_of("tie", 1) == [7, 11, 12, 12] and kept("tie", 1) == [12, 12]
    v, ncls, rule = C.FILTER_CASES["huge"][0](), 3, C.FILTER_CASES["huge"][2]
    out = filter_ref(v, ncls, *rule_tables(rule, ncls))
    assert rule[1]["min_size"] > 2 ** 31 and (v == 1).any() and not (out == 1).any() and np.array_equal(out[v != 1], v[v != 1])
    v, ncls, rule = C.FILTER_CASES["absent"]
    assert 2 in rule and not (v() == 2).any()
    v, ncls, rule = C.FILTER_CASES["ncls255"]
    assert ncls == 255 and 254 in rule and set(np.unique(v()).tolist()) == {0, 253, 254, 255}
    assert sorted(C.FILTER_N) == [3, 30, 63, 105, 1025] and all(math.prod(s) == n for n, s in C.FILTER_N.items())
    for n in C.FILTER_N:
        ids = set(np.unique(C.FILTER_CASES[f"n{n}"][0]()).tolist())
        assert ids >= {1, 3, 255} and (n == 3 or ids >= {0, 1, 2, 3, 255}), n


@pytest.mark.parametrize("name", C.PERCOLATING)
def test_contention_volumes_percolate(name):
    build, ncls = C.CONTENTION[name]
    vol = build()
    big, ncomp, tiles = C.component_census(vol, ncls)
    print(f"{name} {vol.shape}: {ncomp} components in {tiles} tiles; class: (largest, tiles touched) {big}")
    assert sorted(big) == list(range(1, ncls)) and tiles >= 512
    for c, (size, touched) in big.items():
        assert 10 * touched >= 9 * tiles and size > vol.size // (4 * (ncls - 1)), (c, size, touched)
    assert ncomp - len(big) >= 10 ** 4
    if name == "noise3d":                                                    # the figures of the issue
        assert ncomp == 165468 and sorted(s for s, _ in big.values()) == [602958, 607863] and max(t for _, t in big.values()) == 727
    else:
        assert big[1] == (289492, 512)


@pytest.mark.parametrize("name", ["solid", "serpentine"])
def test_contention_volumes_of_one_component(name):
    build, ncls = C.CONTENTION[name]
    vol = build()
    big, ncomp, tiles = C.component_census(vol, ncls)
    print(f"{name} {vol.shape}: {ncomp} component, {big[1][0]} voxels in {big[1][1]} of {tiles} tiles")
    assert ncomp == 1 and big[1] == (int((vol == 1).sum()), tiles) and tiles in (512, 729)
    if name == "solid":
        assert big[1][0] == vol.size and all(n % t == 0 for n, t in zip(vol.shape, C.TILE))
    else:
        assert any(n % t for n, t in zip(vol.shape, C.TILE))


def test_component_case_tables_reach_every_branch():
    from cswin_unet_amd import ops
    assert C.TILE == ops.COMPONENT_TILE and C.TILE[2] % C.SEG == 0
    # labelling: W against the segment, the 16-B load and the int4 store; every seam face; the neighbour loads' own alignment
    assert {W % 16 == 0 for W in C.LABEL_W} == {True, False} and {W % 4 for W in C.LABEL_W} >= {0, 1, 2} and 66 in C.LABEL_W
    per_w = {(W, off): C.label_branches(C.LABEL_SHAPE(W), off) for W in C.LABEL_W for off in C.LABEL_VOL_OFF}
    took = set().union(*per_w.values())
    names = {n for n, _ in took}
    assert len(names) == 15 and all((n, side) in took for n in names for side in C.BOTH), sorted(took)
    assert {side for n, side in per_w[(66, 0)] if n == "store int4"} == {False, True}                 # W % 4 == 2: row by row
    assert ("tile load 16 B", True) not in per_w[(64, 1)] and ("tile load 16 B", True) not in per_w[(64, 4)]
    assert ("tile load 16 B", False) not in per_w[(64, 0)] and ("store int4", False) not in per_w[(64, 4)]
    # the neighbour's address has an alignment of its own: at W = 66 some y-face threads load their row in one piece, none the row above
    assert ("fy own load 16 B", True) in per_w[(66, 0)] and ("fy neighbour load 16 B", True) not in per_w[(66, 0)]
    assert all(math.prod(-(-n // t) for n, t in zip(C.LABEL_SHAPE(W), C.TILE)) == 4 * -(-W // 64) for W in C.LABEL_W)
    for shape in C.LINES:
        assert max(shape) == 2048 and math.prod(shape) == 2048
    for shape, ids, ncls in C.LABEL_IDS.values():
        assert {i < ncls for i in ids if i} == {True, False} and 255 in ids
    assert {c[2] for c in C.LABEL_IDS.values()} == {2, 255}
    assert any(a != b for a, b in C.SEAM_IDS.values()) and any(a == b for a, b in C.SEAM_IDS.values()) and all(min(p) >= 3 for p in C.SEAM_IDS.values())
    for axis in range(3):
        v = C.seam_lanes(axis, 3, 200)
        t = C.TILE[axis]
        lo, hi = np.take(v, t - 1, axis), np.take(v, t, axis)                # the two planes at the seam
        pairs = {(int(a), int(b)) for a, b in zip(lo.ravel(), hi.ravel())}
        assert pairs == {(3, 200), (3, 3), (1, 3), (3, 1), (1, 1), (0, 0)} and v.shape[axis] == 2 * t
        assert {(int(a), int(b)) for a, b in zip(*(np.take(C.seam_lanes(axis, 255, 255), k, axis).ravel() for k in (t - 1, t)))} >= {(255, 255)}
        _, sizes = canonical_labels(v, 3)
        assert (sizes > 0).sum() == 9                                        # the control lane is the only one joined across the seam
    # filter: every N % 4, N < 4, one voxel past a workgroup's 1024; both paths, the tail behind a vector body, the early-out
    assert {n % 4 for n in C.FILTER_N} == {1, 2, 3} and min(C.FILTER_N) < 4 and 1025 in C.FILTER_N and 256 * C.CF_VOX == 1024
    assert C.word_gaps().size % 4 == 0 and C.FILTER_CASES["ceil"][0]().size % 4 == 0                  # N % 4 == 0: no tail
    took = set()
    for name, (build, ncls, _) in C.FILTER_CASES.items():
        for vo, oo, lo in C.FILTER_ALIGN:
            took |= C.filter_branches(build(), ncls, vo, oo, lo)
    names = {n for n, _ in took}
    assert names == {"vec_ok", "v0 + 4 <= N", "w == 0", "vector id < ncls", "scalar id < ncls"}
    assert all((n, side) in took for n in names for side in C.BOTH), sorted(took)
    gaps = C.filter_branches(C.word_gaps(), 3, 0, 0, 0)
    assert ("w == 0", True) in gaps and ("w == 0", False) in gaps and ("vector id < ncls", False) in gaps
    assert ("v0 + 4 <= N", False) in C.filter_branches(C.FILTER_CASES["n3"][0](), 3, 0, 0, 0)          # N < 4: no vector body at all
    assert ("v0 + 4 <= N", True) not in C.filter_branches(C.FILTER_CASES["n3"][0](), 3, 0, 0, 0)
    assert {vec for vo, oo, lo in C.FILTER_ALIGN for n, vec in C.filter_branches(C.word_gaps(), 3, vo, oo, lo) if n == "vec_ok"} == {False, True}
    assert [C.filter_branches(C.word_gaps(), 3, *a) >= {("vec_ok", True)} for a in C.FILTER_ALIGN] == [True, False, False, False, True, False]
