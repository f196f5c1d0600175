"""Device metrics path (csrc/metrics.hip behind ops.seg_metrics / utils.volume_metrics) against the host functions of utils.py
and against scipy-built counts / histograms (tests/seg_metrics_cases.py), computed in the same test.

The device returns integers, so counts and hist are compared with torch.equal.  (dice, hd95): Dice equal exactly; HD95 within
rel = abs = 1e-12 (both sides: correctly rounded float64 square roots of the same integers and one float64 interpolation -- a
few ulp, ~1e-15, is all that can differ).  Every device call is followed by a synchronize so that a failing step ends its test
before anything else is enqueued."""
import numpy as np
import pytest
import torch

from oracle.determ import det_normal, fill_state_dict
from seg_metrics_cases import blob_pair, scipy_counts_hist, special_pair

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = dict(rel=1e-12, abs=1e-12)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _seg_metrics(pred, label, ncls, ndim=None):
    from cswin_unet_amd import ops
    counts, hist = ops.seg_metrics(_dev(pred), _dev(label), ncls, ndim)
    torch.cuda.synchronize()
    return counts.cpu(), hist.cpu()


def _host_list(pred, label, ncls):
    from cswin_unet_amd.utils import calculate_metric_percase
    return [calculate_metric_percase(pred == i, label == i) for i in range(1, ncls)]


def _check_lists(got, want):
    assert len(got) == len(want)
    for c, (g, w) in enumerate(zip(got, want), start=1):
        print(f"class {c}: hip {g} host {w}")
        assert g[0] == w[0], (c, g, w)
        assert g[1] == pytest.approx(w[1], **TOL), (c, g, w)


def _check_raw(pred, label, ncls, ndim=None):
    counts, hist = _seg_metrics(pred, label, ncls, ndim)
    wc, wh = scipy_counts_hist(pred, label, ncls, ndim)
    assert counts.dtype == torch.int64 and hist.dtype == torch.int32
    bad = (counts != torch.from_numpy(wc)).nonzero()
    assert torch.equal(counts, torch.from_numpy(wc)), (bad[:8].tolist(), counts[:10].tolist(), wc[:10].tolist())
    diff = (hist != torch.from_numpy(wh)).nonzero()
    assert torch.equal(hist, torch.from_numpy(wh)), (diff.shape[0], [(int(c), int(s), int(hist[c, s]), int(wh[c, s])) for c, s in diff[:8]])
    for c in range(ncls):
        both = c > 0 and counts[c, 0] > 0 and counts[c, 1] > 0
        assert int(hist[c].sum()) == (int(counts[c, 3]) if both else 0), c
    return counts, hist


RAW_CASES = {
    "special3d": lambda: special_pair((12, 40, 36), 1) + (9, None),
    "special2d": lambda: special_pair((48, 52), 2) + (9, None),
    "identical": lambda: (lambda p: (p, p.copy(), 9, None))(special_pair((10, 30, 30), 5)[0]),
    "odd_5x33x71": lambda: blob_pair((5, 33, 71), [1, 2, 3, 4, 5, 6, 7, 8], 11) + (9, None),
    "plane_ndim3": lambda: blob_pair((1, 40, 40), [1, 2, 3], 12) + (9, 3),
    "plane_ndim2": lambda: blob_pair((1, 40, 40), [1, 2, 3], 12) + (9, 2),
    "odd_37x130x64": lambda: blob_pair((37, 130, 64), [1, 2, 3, 4, 5, 6, 7, 8], 13) + (9, None),
    "ncls2": lambda: blob_pair((7, 45, 50), [1], 14) + (2, None),
    "ncls200": lambda: blob_pair((37, 130, 64), [1, 5, 17, 64, 65, 128, 199, 3], 15, rmin=0.05, rmax=0.15) + (200, None),
    "wide_row": lambda: blob_pair((3, 20, 300), [1, 2, 3], 16) + (4, None),
}


@pytest.mark.parametrize("name", sorted(RAW_CASES))
def test_counts_and_hist_equal_scipy(name):
    pred, label, ncls, ndim = RAW_CASES[name]()
    _check_raw(pred, label, ncls, ndim)


def test_plane_differs_between_ndim_3_and_2():
    """A (1, H, W) volume: with ndim = 3 every set voxel is a border voxel (its z neighbours are outside), with ndim = 2 only
    the in-plane outline is."""
    pred, label = blob_pair((1, 40, 40), [1, 2, 3], 12)
    c3, _ = _seg_metrics(pred, label, 4, 3)
    c2, _ = _seg_metrics(pred, label, 4, 2)
    assert torch.equal(c3[:, :3], c2[:, :3]) and torch.equal(c3[:, 3], c3[:, 0] + c3[:, 1]) and (c2[:, 3] <= c3[:, 3]).all() and (c2[:, 3] < c3[:, 3]).any()
    c2d, h2d = _seg_metrics(pred[0], label[0], 4)                    # an (H, W) tensor: ndim defaults to its rank
    assert torch.equal(c2d, c2)
    assert torch.equal(h2d, _seg_metrics(pred, label, 4, 2)[1])


def test_two_calls_are_bit_identical():
    pred, label = blob_pair((37, 130, 64), [1, 2, 3, 4, 5, 6, 7, 8], 13)
    a, b = _seg_metrics(pred, label, 9), _seg_metrics(pred, label, 9)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_bad_arguments_raise():
    from cswin_unet_amd import ops
    from cswin_unet_amd._lib import CswinHipError
    p = torch.zeros(2, 8, 8, dtype=torch.uint8, device=DEV)
    with pytest.raises(CswinHipError):
        ops.seg_metrics(p, p, 9, ndim=2)                             # ndim = 2 needs D == 1
    with pytest.raises(CswinHipError):
        ops.seg_metrics(p, p.float(), 9)
    with pytest.raises(CswinHipError):
        ops.seg_metrics(p, p, 1)


def test_golden_argmax_volume_3d_and_slicewise(golden):
    """Real data: the reference-generated eval argmax map against itself rolled by (0, 3, -2)."""
    from cswin_unet_amd.utils import volume_metrics
    pred = np.ascontiguousarray(golden("g6_eval")["argmax"])
    assert pred.shape == (2, 224, 224)
    label = np.roll(pred, (0, 3, -2), axis=(0, 1, 2))
    _check_lists(volume_metrics(pred, label, 9, device=DEV), _host_list(pred, label, 9))
    for i in range(pred.shape[0]):
        _check_lists(volume_metrics(pred[i], label[i], 9, device=DEV), _host_list(pred[i], label[i], 9))
    # float32 labels as the h5 test volumes deliver them, tensors as well as arrays
    _check_lists(volume_metrics(torch.from_numpy(pred.astype(np.int64)), label.astype(np.float32), 9, device=DEV), _host_list(pred, label, 9))
    _check_raw(pred, label, 9)


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


def test_single_volume_hip_equals_host(golden):
    """The inputs of test_gpu_parity.test_volume_inference_vs_reference_argmax (the label is the reference's argmax map, so the
    prediction all but coincides with it), then the same with the label moved so that every class overlaps only partly."""
    from cswin_unet_amd.utils import test_single_volume
    g = golden("g6_eval")
    net = _golden_net()
    vol = det_normal("model.x", (2, 1, 224, 224))[:, 0]
    image = torch.from_numpy(vol)[None]
    label = torch.from_numpy(g["argmax"].astype(np.int64))[None]
    host = test_single_volume(image, label, net, classes=9, patch_size=[224, 224])
    hip = test_single_volume(image, label, net, classes=9, patch_size=[224, 224], metrics="hip")
    assert len(hip) == 8
    _check_lists(hip, host)
    moved = torch.from_numpy(np.roll(g["argmax"].astype(np.int64), (1, -4), axis=(1, 2)))[None]
    host = test_single_volume(image, moved, net, classes=9, patch_size=[224, 224])
    _check_lists(test_single_volume(image, moved, net, classes=9, patch_size=[224, 224], metrics="hip"), host)
    assert any(0 < d < 1 for d, _ in host)                           # a real comparison, not all-or-nothing classes


def test_evaluate_volumes_equals_mean_of_host_results():
    from cswin_unet_amd.utils import evaluate_volumes, test_single_volume
    net = _golden_net()
    loader = []
    for i in range(2):
        vol = det_normal(f"segm.vol{i}", (3, 1, 224, 224))[:, 0]
        _, lab = blob_pair((3, 224, 224), [1, 2, 3, 4, 5, 6, 7, 8], 20 + i)
        loader.append({"image": torch.from_numpy(vol)[None], "label": torch.from_numpy(lab.astype(np.float32))[None],
                       "case_name": [f"case{i}"]})
    per_volume, class_mean, mean_dice, mean_hd95 = evaluate_volumes(loader, net, 9, [224, 224], metrics="hip")
    host = [test_single_volume(b["image"], b["label"], net, classes=9, patch_size=[224, 224]) for b in loader]
    assert len(per_volume) == 2
    for got, want in zip(per_volume, host):
        _check_lists(got, want)
    want_mean = (np.array(host[0], np.float64) + np.array(host[1], np.float64)) / 2
    assert class_mean.shape == (8, 2)
    assert class_mean == pytest.approx(want_mean, **TOL)
    assert mean_dice == pytest.approx(want_mean[:, 0].mean(), **TOL) and mean_hd95 == pytest.approx(want_mean[:, 1].mean(), **TOL)
    per_host = evaluate_volumes(loader, net, 9, [224, 224], metrics="host")[0]
    assert per_host == host


def test_full_size_volume():
    """148 x 512 x 512 with three foreground classes (the host side stays under a minute)."""
    from cswin_unet_amd.utils import volume_metrics
    pred, label = blob_pair((148, 512, 512), [1, 2, 3], 31, jitter=4.0, rmin=0.06, rmax=0.2)
    got = volume_metrics(pred, label, 4, device=DEV)
    torch.cuda.synchronize()
    _check_lists(got, _host_list(pred, label, 4))
