"""Spacing-aware surface distances on the device (cswin_surface_dist in csrc/metrics.hip behind ops.surface_distances /
utils.volume_metrics(voxelspacing=, assd=)) against scipy-built lists (tests/surface_cases.py) and the host functions of utils.py.

Bounds.  counts and nq are integers: torch.equal.  With dyadic spacings (DYADIC) every product and sum of
(dz sz)^2 + (dy sy)^2 + (dx sx)^2 is exact in float64, so the sorted square roots of a segment must be np.array_equal to scipy's.
With general spacings (GENERAL) the separable minimisation may settle on a candidate whose rounded value is an ulp above the
minimum scipy's transform reports (2e-16 relative); sorting two lists whose values differ by eps moves no element by more than
eps, so sorted segments, HD95 and ASSD are compared element for element with the project's rel = abs = 1e-12
(tests/test_gpu_seg_metrics.py), no element left out.  Dice is one division of the same integers: ==.
Every device call is followed by a synchronize so that a failing step ends its test before anything else is enqueued."""
import numpy as np
import pytest
import torch

from oracle.determ import det_normal, fill_state_dict
from seg_metrics_cases import blob_pair, nbins_of, special_pair
from surface_cases import DYADIC, GENERAL, scipy_surface_lists

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = dict(rel=1e-12, abs=1e-12)

CASES = {
    "special3d": lambda: special_pair((12, 40, 36), 1) + (9, None),
    "special2d": lambda: special_pair((48, 52), 2) + (9, None),
    "identical": lambda: (lambda p: (p, p.copy(), 9, None))(special_pair((10, 30, 30), 5)[0]),
    "odd_5x33x71": lambda: blob_pair((5, 33, 71), [1, 2, 3, 4, 5, 6, 7, 8], 11) + (9, None),
    "plane_ndim3": lambda: blob_pair((1, 40, 40), [1, 2, 3], 12) + (9, 3),
    "plane_ndim2": lambda: blob_pair((1, 40, 40), [1, 2, 3], 12) + (9, 2),
    "odd_37x130x64": lambda: blob_pair((37, 130, 64), [1, 2, 3, 4, 5, 6, 7, 8], 13) + (9, None),
    "ncls200": lambda: blob_pair((37, 130, 64), [1, 5, 17, 64, 65, 128, 199, 3], 15, rmin=0.05, rmax=0.15) + (200, None),
    "wide_row": lambda: blob_pair((3, 20, 300), [1, 2, 3], 16) + (4, None),
}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _rule_ndim(pred, ndim):
    return pred.ndim if ndim is None else ndim


def _lists(pred, label, ncls, spacing, ndim=None, cap=None):
    """ops.surface_distances on the device; (counts, nq) as CPU tensors, dist2 as a numpy array of all `cap` entries."""
    from cswin_unet_amd import ops
    counts, nq, dist2 = ops.surface_distances(_dev(pred), _dev(label), ncls, spacing, ndim, cap)
    torch.cuda.synchronize()
    assert counts.dtype == torch.int64 and nq.dtype == torch.int64 and dist2.dtype == torch.float64
    assert counts.shape == (ncls, 4) and nq.shape == (ncls, 2)
    return counts.cpu(), nq.cpu(), dist2.cpu().numpy()


def _seg_counts_hist(pred, label, ncls, ndim):
    from cswin_unet_amd import ops
    counts, hist = ops.seg_metrics(_dev(pred), _dev(label), ncls, ndim)
    torch.cuda.synchronize()
    return counts.cpu(), hist.cpu()


def _segments(nq, dist2):
    """{(c, dir): ascending distances} of the device's list."""
    starts = np.concatenate(([0], np.cumsum(nq.numpy().ravel())))
    return {(k // 2, k % 2): np.sort(np.sqrt(dist2[starts[k]:starts[k + 1]])) for k in range(2 * nq.shape[0]) if starts[k + 1] > starts[k]}


def _check_against_scipy(name, triple, exact):
    pred, label, ncls, ndim = CASES[name]()
    spacing = triple[3 - _rule_ndim(pred, ndim):]                    # a plane takes the in-plane entries
    counts, nq, dist2 = _lists(pred, label, ncls, spacing, ndim)
    wc, wnq, want = scipy_surface_lists(pred, label, ncls, spacing, ndim)
    assert torch.equal(counts, torch.from_numpy(wc)), (counts[:10].tolist(), wc[:10].tolist())
    assert torch.equal(counts, _seg_counts_hist(pred, label, ncls, ndim)[0])
    assert torch.equal(nq, torch.from_numpy(wnq)), (nq[:10].tolist(), wnq[:10].tolist())
    both = (counts[:, 0] > 0) & (counts[:, 1] > 0) & (torch.arange(ncls) > 0)
    assert torch.equal(nq.sum(dim=1), torch.where(both, counts[:, 3], torch.zeros_like(counts[:, 3])))
    assert int(nq.sum()) <= dist2.shape[0]
    got = _segments(nq, dist2)
    assert sorted(got) == sorted(want) and len(want) >= 2
    worst = 0.0
    for key in sorted(want):
        g, w = got[key], want[key]
        assert g.shape == w.shape, key
        worst = max(worst, float(np.max(np.abs(g - w) / np.maximum(w, 1e-300))))
        if exact:
            assert np.array_equal(g, w), (key, int((g != w).sum()), g.shape[0])
        else:
            assert g == pytest.approx(w, **TOL), key
    print(f"{name} {spacing}: {int(nq.sum())} distances, worst relative difference {worst:.3g}")
    if name == "identical":
        assert all(not g.any() for g in got.values())
    return counts, nq, dist2


@pytest.mark.parametrize("triple", DYADIC, ids=str)
@pytest.mark.parametrize("name", sorted(CASES))
def test_dyadic_spacing_equals_scipy_exactly(name, triple):
    _check_against_scipy(name, triple, exact=True)


@pytest.mark.parametrize("triple", [(40.0, 0.73, 0.73)] + GENERAL, ids=str)
@pytest.mark.parametrize("name", sorted(CASES))
def test_general_spacing_matches_scipy(name, triple):
    """(40, .73, .73): the nearest seed is in the query's own plane whenever that plane has one; (0.05, 1, 1): it is many planes
    away and the z walk's early stop is exercised across the whole box; (2.5, .73, .73) and the all-different triple between."""
    _check_against_scipy(name, triple, exact=False)


@pytest.mark.parametrize("name", sorted(CASES))
def test_unit_spacing_reproduces_the_histogram(name):
    pred, label, ncls, ndim = CASES[name]()
    counts, nq, dist2 = _lists(pred, label, ncls, 1.0, ndim)
    sc, hist = _seg_counts_hist(pred, label, ncls, ndim)
    assert torch.equal(counts, sc)
    starts = np.concatenate(([0], np.cumsum(nq.numpy().ravel())))
    nbins = nbins_of(pred.shape)
    assert hist.shape == (ncls, nbins)
    for c in range(ncls):
        seg = dist2[starts[2 * c]:starts[2 * c + 2]]
        assert np.array_equal(seg, np.rint(seg))                     # unit spacing: integers, exactly
        binned = np.bincount(seg.astype(np.int64), minlength=nbins)
        assert torch.equal(torch.from_numpy(binned).to(torch.int32), hist[c]), c


def _host_list(pred, label, ncls, spacing, assd=True):
    from cswin_unet_amd.utils import calculate_metric_percase
    return [calculate_metric_percase(pred == i, label == i, voxelspacing=spacing, assd=assd) for i in range(1, ncls)]


def _check_metric_lists(got, want):
    assert len(got) == len(want)
    for c, (g, w) in enumerate(zip(got, want), start=1):
        print(f"class {c}: hip {g} host {w}")
        assert len(g) == len(w) and g[0] == w[0], (c, g, w)
        assert tuple(g[1:]) == pytest.approx(tuple(w[1:]), **TOL), (c, g, w)


def _volume_metrics(*args, **kwargs):
    from cswin_unet_amd.utils import volume_metrics
    out = volume_metrics(*args, device=DEV, **kwargs)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name,spacing", [("special3d", GENERAL[0]), ("special3d", GENERAL[1]), ("special2d", (0.73, 1.9)),
                                          ("odd_5x33x71", GENERAL[2]), ("plane_ndim3", DYADIC[2]), ("special3d", None)], ids=str)
def test_volume_metrics_equals_host_loop(name, spacing):
    pred, label, ncls, _ = CASES[name]()
    want = _host_list(pred, label, ncls, spacing)
    _check_metric_lists(_volume_metrics(pred, label, ncls, voxelspacing=spacing, assd=True), want)
    # tensors as well as arrays, float32 labels as the h5 test volumes deliver them
    _check_metric_lists(_volume_metrics(torch.from_numpy(pred.astype(np.int64)), label.astype(np.float32), ncls, voxelspacing=spacing, assd=True), want)
    if spacing is not None:
        pairs = _volume_metrics(_dev(pred), _dev(label), ncls, voxelspacing=spacing)
        _check_metric_lists(pairs, _host_list(pred, label, ncls, spacing, assd=False))
    if name.startswith("special"):
        assert want[4] == (1, 0, 0) and want[5] == (0, 0, 0) and want[6] == (0, 0, 0) and want[7][0] == 0.0 and want[7][2] > 0


def test_identical_pair_is_all_zero():
    pred, label, ncls, _ = CASES["identical"]()
    got = _volume_metrics(pred, label, ncls, voxelspacing=GENERAL[2], assd=True)
    present = [int((pred == c).any()) for c in range(1, ncls)]
    assert sum(present) >= 4
    assert got == [(1.0, 0.0, 0.0) if p else (0, 0, 0) for p in present]


@pytest.mark.parametrize("name", ["special3d", "odd_5x33x71", "special2d"])
def test_doubling_the_spacing_doubles_hd95_and_assd_exactly(name):
    pred, label, ncls, _ = CASES[name]()
    one = _volume_metrics(pred, label, ncls, voxelspacing=1, assd=True)
    two = _volume_metrics(pred, label, ncls, voxelspacing=(2.0,) * pred.ndim, assd=True)
    assert two == [(d, 2 * h, 2 * a) for d, h, a in one] and any(h > 0 and a > 0 for _, h, a in one)
    assert _volume_metrics(pred, label, ncls, assd=True) == one          # no spacing with assd: unit spacing
    hist_path = _volume_metrics(pred, label, ncls)
    _check_metric_lists([m[:2] for m in one], hist_path)


def test_two_calls_are_bit_identical():
    from cswin_unet_amd.utils import _sorted_surface_lists
    pred, label, ncls, _ = CASES["odd_37x130x64"]()
    runs = []
    for _ in range(2):
        out = _sorted_surface_lists(_dev(pred), _dev(label), ncls, GENERAL[0])
        torch.cuda.synchronize()
        runs.append(out + (_volume_metrics(pred, label, ncls, voxelspacing=GENERAL[0], assd=True),))
    assert runs[0][2].shape[0] == runs[0][1].sum() > 1000
    assert all(np.array_equal(a, b) for a, b in zip(runs[0][:3], runs[1][:3]))
    assert runs[0][3] == runs[1][3]


def test_small_cap_drops_values_and_writes_nothing_past_it():
    """The C entry point on a buffer with a canary tail; then ops.surface_distances with the same cap."""
    from cswin_unet_amd import _lib
    pred, label, ncls, _ = CASES["special3d"]()
    _, wnq, want = scipy_surface_lists(pred, label, ncls, GENERAL[0])
    total = int(wnq.sum())
    D, H, W = pred.shape
    nbytes = _lib.lib().cswin_surface_dist_workspace(D, H, W, 3, ncls)
    p8, l8 = _dev(pred), _dev(label)
    for cap in (total // 2, int(wnq[1].sum()), 0, total):
        assert cap < total or cap == total
        counts = torch.empty(ncls, 4, dtype=torch.int64, device=DEV)
        nq = torch.empty(ncls, 2, dtype=torch.int64, device=DEV)
        buf = torch.full((total + 256,), -7.0, dtype=torch.float64, device=DEV)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        _lib.call("cswin_surface_dist", _lib.ptr(p8), _lib.ptr(l8), _lib.ptr(counts), _lib.ptr(nq), _lib.ptr(buf), cap, _lib.ptr(ws),
                  nbytes, D, H, W, 3, ncls, *GENERAL[0], _lib.stream())
        torch.cuda.synchronize()
        assert torch.equal(nq.cpu(), torch.from_numpy(wnq))          # nq reports the full sizes: the caller sees nq.sum() > cap
        assert (int(nq.sum()) > cap) == (cap < total)
        host = buf.cpu().numpy()
        assert (host[cap:] == -7.0).all(), cap                       # the canary, and everything from cap on
        assert (host[:cap] >= 0).all()                               # every slot below cap was written
        starts = np.concatenate(([0], np.cumsum(wnq.ravel())))
        for k in range(2 * ncls):                                    # segments that fit are complete and right
            if starts[k + 1] > starts[k] and starts[k + 1] <= cap:
                assert np.sort(np.sqrt(host[starts[k]:starts[k + 1]])) == pytest.approx(want[(k // 2, k % 2)], **TOL)
    _, nq, dist2 = _lists(pred, label, ncls, GENERAL[0], cap=total // 2)
    assert dist2.shape == (total // 2,) and int(nq.sum()) == total > total // 2


def test_volume_metrics_retries_when_the_default_cap_is_too_small(monkeypatch):
    from cswin_unet_amd import ops
    pred, label, ncls, _ = CASES["special3d"]()
    full = _volume_metrics(pred, label, ncls, voxelspacing=GENERAL[0], assd=True)
    calls = []
    real = ops.surface_distances
    monkeypatch.setattr(ops, "surface_cap", lambda nvox: 7)
    monkeypatch.setattr(ops, "surface_distances", lambda *a, **k: calls.append(k.get("cap")) or real(*a, **k))
    again = _volume_metrics(pred, label, ncls, voxelspacing=GENERAL[0], assd=True)
    assert len(calls) == 2 and calls[0] is None and calls[1] > 7
    assert again == full
    _check_metric_lists(again, _host_list(pred, label, ncls, GENERAL[0]))


def test_bad_arguments_raise():
    from cswin_unet_amd import ops
    from cswin_unet_amd._lib import CswinHipError
    from cswin_unet_amd.utils import evaluate_volumes, volume_metrics
    p = torch.zeros(2, 8, 8, dtype=torch.uint8, device=DEV)
    for bad in ((1, 1), (1, 1, 1, 1), (1, 0, 1), (1, -0.5, 1), (1, float("nan"), 1), 0, -2.0):
        with pytest.raises(ValueError):
            ops.surface_distances(p, p, 9, bad)
        with pytest.raises(ValueError):
            volume_metrics(p, p, 9, device=DEV, voxelspacing=bad)
    with pytest.raises(ValueError):
        ops.surface_distances(p[0], p[0], 9, (1, 1, 1))              # a plane takes two entries
    with pytest.raises(ValueError):
        ops.surface_distances(p, p, 9, 1.0, cap=-1)
    with pytest.raises(CswinHipError):
        ops.surface_distances(p.cpu(), p.cpu(), 9, 1.0)
    with pytest.raises(CswinHipError):
        ops.surface_distances(p, p.float(), 9, 1.0)
    with pytest.raises(CswinHipError):
        ops.surface_distances(p, p, 9, (1, 1), ndim=2)               # ndim = 2 needs D == 1
    with pytest.raises(CswinHipError):
        ops.surface_distances(p, p, 1, 1.0)
    with pytest.raises(CswinHipError):
        ops.surface_distances(p, p[:, :4], 9, 1.0)
    loader = [{"image": torch.zeros(1, 2, 8, 8), "label": torch.zeros(1, 2, 8, 8), "case_name": ["case3"]}]
    with pytest.raises(KeyError, match="case3"):
        evaluate_volumes(loader, None, 9, [8, 8], metrics="hip", resize="hip", voxelspacing={"case0": (1, 1, 1)})
    torch.cuda.synchronize()


class _OneChannel(torch.nn.Module):          # CSwinUnet.forward: 1 -> 3 channels (vision_transformer.py:40-41)
    def __init__(self, m):
        super().__init__()
        self.m = m

    def forward(self, x):
        return self.m(x.repeat(1, 3, 1, 1))


def _golden_net():
    import cswin_unet_amd.networks.cswin_unet as N
    net = N.CSWinTransformer(img_size=224, num_classes=9, embed_dim=64, depth=[1, 2, 9, 1], split_size=[1, 2, 7, 7],
                             num_heads=[2, 4, 8, 16], mlp_ratio=4., qkv_bias=True, drop_path_rate=0.).to(DEV)
    return _OneChannel(fill_state_dict(net)).eval()


def test_evaluation_loop_with_spacing_hip_equals_host():
    """The two synthetic volumes of test_gpu_seg_metrics.test_evaluate_volumes_equals_mean_of_host_results, each with its own
    spacing: the device metrics on the resident prediction against the scipy loop on the same prediction."""
    from cswin_unet_amd.utils import evaluate_volumes, test_single_volume
    net = _golden_net()
    loader = []
    for i in range(2):
        vol = det_normal(f"segm.vol{i}", (3, 1, 224, 224))[:, 0]
        _, lab = blob_pair((3, 224, 224), [1, 2, 3, 4, 5, 6, 7, 8], 20 + i)
        loader.append({"image": torch.from_numpy(vol)[None], "label": torch.from_numpy(lab.astype(np.float32))[None],
                       "case_name": [f"case{i}"]})
    spacing = {"case0": (2.5, 0.73, 0.73), "case1": (3.0, 0.9, 0.8), "unused": (1, 1, 1)}
    kw = dict(resize="hip", voxelspacing=spacing, assd=True)
    hip = evaluate_volumes(loader, net, 9, [224, 224], metrics="hip", **kw)
    torch.cuda.synchronize()
    host = evaluate_volumes(loader, net, 9, [224, 224], metrics="host", **kw)
    torch.cuda.synchronize()
    assert len(hip) == len(host) == 5 and hip[1].shape == (8, 3) == host[1].shape
    for got, want in zip(hip[0], host[0]):
        _check_metric_lists(got, want)
    assert hip[1] == pytest.approx(host[1], **TOL)
    assert hip[2:] == pytest.approx(host[2:], **TOL) and hip[2] == host[2]
    assert hip[2:] == pytest.approx(tuple(hip[1].mean(axis=0)), **TOL)
    assert any(0 < m[0] < 1 and m[1] > 0 and m[2] > 0 for m in host[0][0])          # a real comparison
    one = test_single_volume(loader[1]["image"], loader[1]["label"], net, classes=9, patch_size=[224, 224], metrics="hip",
                             resize="hip", voxelspacing=spacing["case1"], assd=True)
    torch.cuda.synchronize()
    assert one == hip[0][1]
    # the defaults: the four-tuple of pairs from the histogram path, as before
    plain = evaluate_volumes(loader, net, 9, [224, 224], metrics="hip", resize="hip")
    torch.cuda.synchronize()
    assert len(plain) == 4 and plain[1].shape == (8, 2) and all(len(m) == 2 for v in plain[0] for m in v)
    want = [test_single_volume(b["image"], b["label"], net, classes=9, patch_size=[224, 224], metrics="hip", resize="hip") for b in loader]
    torch.cuda.synchronize()
    assert plain[0] == want
    assert plain[1] == pytest.approx((np.array(want[0], np.float64) + np.array(want[1], np.float64)) / 2, **TOL)
    assert [[m[0] for m in v] for v in plain[0]] == [[m[0] for m in v] for v in hip[0]]          # Dice does not depend on the spacing
