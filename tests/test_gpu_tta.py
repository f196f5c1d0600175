"""Test-time augmentation on the device (csrc/tta.hip behind ops.view_batch / ops.tta_argmax_zoom_back and
utils.predict_volume(resize="hip", tta=...)) against numpy and the float64 definition of tests/tta_cases.py, whose host side
tests/test_tta_host.py checks.  Every device call is followed by a synchronize so that a failing step ends its test before
anything else is enqueued.

view_batch and the vote geometry are compared exactly, no element excused.  Probabilities: every element within
tta_cases.prob_tolerance of the float64 definition.  Class maps on seeded logits and through the network: a pixel may differ only
where the reference's two best probabilities are within 1e-5, at most 0.1 % of the pixels may be excused so, and the reference's
own share of such pixels is asserted first.

Measured maxima of |P - P64| on an MI355X (bound 1e-5, three-255: 9.4e-5): d4-9 8.4e-8, flips-16 1.2e-7, d4-17-general 5.4e-8,
identity-9 3.0e-7, three-255 2.4e-7, d4-14-of-20 6.7e-8; no pixel of any case within 1e-5 of a tie, no class differs."""
import ctypes

import numpy as np
import pytest
import torch
from scipy.ndimage import zoom

import tta_cases as T
from oracle.determ import det_normal, fill_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda"
ERR_SHAPE, ERR_WORKSPACE = -1, -3


def put(a):
    return torch.from_numpy(np.array(a)).to(DEV)


# ---- 1. view_batch -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,codes", T.VIEW_SHAPES, ids=lambda v: "x".join(map(str, v)) if len(v) == 3 else f"{len(v)}codes")
def test_view_batch_is_numpys_view_bit_for_bit(shape, codes):
    from cswin_unet_amd import ops
    x = det_normal("tta.view", shape)
    dx = put(x)
    lists = [(c,) for c in codes] + [tuple(codes), tuple(reversed(codes))[:3]]
    for views in lists:
        y = ops.view_batch(dx, views)
        torch.cuda.synchronize()
        assert y.dtype == torch.float32 and y.is_contiguous() and tuple(y.shape) == (len(views),) + shape
        got = y.cpu().numpy()
        for v, c in enumerate(views):
            assert np.array_equal(got[v].view(np.uint32), np.ascontiguousarray(T.view_np(x, c)).view(np.uint32)), (shape, views, v)
    assert torch.equal(dx.cpu(), torch.from_numpy(x))                   # the input is left as it was
    xt = dx.transpose(1, 2).contiguous().transpose(1, 2)               # a view that is not contiguous is copied
    if shape[1] > 1:
        assert not xt.is_contiguous()
    y = ops.view_batch(xt, (codes[-1],))
    torch.cuda.synchronize()
    assert np.array_equal(y.cpu().numpy()[0], T.view_np(x, codes[-1]))


# ---- 2. geometry -------------------------------------------------------------------------------------------------------------
def _vote_id(case):
    views, hw, size, classes = case
    return f"v{''.join(map(str, views))}-{hw[0]}x{hw[1]}" + (f"-to-{size[0]}x{size[1]}" if size else "") + ("-classes" if classes else "")


@pytest.mark.parametrize("case", T.vote_cases(), ids=_vote_id)
def test_votes_land_where_each_view_puts_them(case):
    """Exact equality with the closed-form winner (the definition's, which tests/test_tta_host.py holds to the closed form),
    every output pixel, with and without the zoom back."""
    from cswin_unet_amd import ops
    views, (h, w), size, classes = case
    B = 2
    L = T.vote_logits(views, B, h, w)
    P = T.ensemble_np(L, views, classes)
    cls = T.classes_of(P)
    if len(views) > 1 and classes is None:
        assert np.array_equal(cls, T.fixed_class(B, h, w))
    want = T.zoom_back(cls, size or (h, w))
    got = ops.tta_argmax_zoom_back(put(L.reshape((-1,) + L.shape[2:])), views, size or (h, w), classes=classes)
    torch.cuda.synchronize()
    assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape and got.is_contiguous()
    assert np.array_equal(got.cpu().numpy(), want), _vote_id(case)
    assert len(np.unique(want)) >= min(9, h * w)


# ---- 3, 4, 6. probabilities, class maps, determinism --------------------------------------------------------------------------
@pytest.mark.parametrize("tag,views,B,ncls,n,classes", T.PROB_CASES, ids=[c[0] for c in T.PROB_CASES])
def test_probabilities_and_classes_on_seeded_logits(tag, views, B, ncls, n, classes):
    from cswin_unet_amd import ops
    logits, P, cls, gap = T.prob_case(tag)
    nsel = ncls if classes is None else len(classes)
    dl = put(logits.reshape(-1, ncls, n, n))
    out, probs = ops.tta_argmax_zoom_back(dl, views, (n, n), classes=classes, return_probs=True)
    torch.cuda.synchronize()
    assert probs.dtype == torch.float32 and tuple(probs.shape) == P.shape == (B, nsel, n, n) and tuple(out.shape) == (B, n, n)
    err = np.abs(probs.cpu().numpy().astype(np.float64) - P)
    tol = T.prob_tolerance(nsel)
    print(f"{tag}: max |P - P64| = {err.max():.3e} (bound {tol:.3e}), at P = {P.reshape(-1)[err.argmax()]:.4f}")
    assert np.isfinite(err).all() and err.max() <= tol
    T.compare_classes(out.cpu().numpy(), cls, gap, tag)
    # the map without the probabilities, and both a second time: the same bits
    again, probs2 = ops.tta_argmax_zoom_back(dl, views, (n, n), classes=classes, return_probs=True)
    alone = ops.tta_argmax_zoom_back(dl, views, (n, n), classes=classes)
    torch.cuda.synchronize()
    assert torch.equal(again, out) and torch.equal(alone, out)
    assert torch.equal(probs2.view(torch.int32), probs.view(torch.int32))
    # zoomed: the same class map, gathered
    size = (2 * n + 3, n - 5)
    zoomed = ops.tta_argmax_zoom_back(dl, views, size, classes=classes)
    torch.cuda.synchronize()
    assert np.array_equal(zoomed.cpu().numpy(), T.zoom_back(out.cpu().numpy().astype(np.int64), size))


# ---- 5. special values -------------------------------------------------------------------------------------------------------
def test_a_nan_or_inf_logit_in_any_view_gives_position_zero():
    from cswin_unet_amd import ops
    views, B, ncls, n = T.CODES, 2, 9, 33
    L = (3.0 * det_normal("tta.special", (len(views), B, ncls, n, n))).copy()
    L[:, :, 0] -= 4.0                                                  # position 0 does not win by itself
    marks = [(0, 0, 3, 0, 0, np.nan), (5, 1, 8, 32, 1, np.nan), (3, 0, 0, 16, 31, np.inf), (7, 1, 4, 2, 30, np.inf),
             (2, 0, 5, 7, 7, -np.inf), (6, 1, 2, 20, 11, np.nan), (6, 1, 6, 20, 11, np.inf)]
    for v, b, k, i, j, val in marks:
        L[v, b, k, i, j] = val
    P = T.ensemble_np(L, views)
    cls = T.classes_of(P)
    bad = np.isnan(P).any(1)
    assert bad.sum() == 5 and (cls[bad] == 0).all() and (cls[~bad] != 0).mean() > 0.9      # -inf alone is an ordinary loser
    for classes in (None, (8, 0, 3, 4, 5, 2, 6)):
        Pc = T.ensemble_np(L, views, classes)
        out, probs = ops.tta_argmax_zoom_back(put(L.reshape(-1, ncls, n, n)), views, (n, n), classes=classes, return_probs=True)
        torch.cuda.synchronize()
        got, gp = out.cpu().numpy(), probs.cpu().numpy()
        badc = np.isnan(Pc).any(1)
        assert badc.sum() == 5 and (got[badc] == 0).all()
        assert np.array_equal(np.isnan(gp), np.isnan(Pc))
        T.compare_classes(got, T.classes_of(Pc), np.where(badc, 1.0, T.top_two_gap(np.nan_to_num(Pc))), f"special {classes}")
    # the host path of the definition agrees
    from cswin_unet_amd.utils import ensemble_views_host
    assert np.array_equal(ensemble_views_host(torch.from_numpy(L.reshape(-1, ncls, n, n)), views, None)[0], cls)


# ---- 7. through the network ----------------------------------------------------------------------------------------------------
class _OneChannel(torch.nn.Module):          # CSwinUnet.forward: 1 -> 3 channels (vision_transformer.py:40-41)
    def __init__(self, m):
        super().__init__()
        self.m = m

    def forward(self, x):
        return self.m(x.repeat(1, 3, 1, 1))


@pytest.fixture(scope="module")
def net():
    import cswin_unet_amd.networks.cswin_unet as N
    m = N.CSWinTransformer(img_size=224, num_classes=9, embed_dim=64, depth=[1, 2, 9, 1], split_size=[1, 2, 7, 7],
                           num_heads=[2, 4, 8, 16], mlp_ratio=4., qkv_bias=True, drop_path_rate=0.).to(DEV)
    return _OneChannel(fill_state_dict(m)).eval()


VOL = (3, 64, 48)


def _host_gap_per_voxel(vol, net, patch, views, batch_slices):
    """The host path's float64 top-two gap at the source pixel of every voxel: predict_volume's host steps, restated up to the
    probabilities."""
    from cswin_unet_amd.utils import apply_view, ensemble_views_host, nearest_index
    D, x, y = vol.shape
    rows, cols = nearest_index(patch[0], x), nearest_index(patch[1], y)
    b = max(1, batch_slices // len(views))
    gaps = []
    with torch.no_grad():
        for d0 in range(0, D, b):
            sl = np.stack([zoom(s, (patch[0] / x, patch[1] / y), order=3) for s in vol[d0:d0 + b]])
            seen = np.concatenate([apply_view(sl, c) for c in views])
            logits = net(torch.from_numpy(np.ascontiguousarray(seen)).unsqueeze(1).float().to(DEV))
            torch.cuda.synchronize()
            _, P = ensemble_views_host(logits, views, None)
            g = T.top_two_gap(P)[:, np.maximum(rows, 0)][:, :, np.maximum(cols, 0)]
            g[:, rows < 0] = 1.0                                       # scipy's constant 0 on both paths
            g[:, :, cols < 0] = 1.0
            gaps.append(g)
    return np.concatenate(gaps)


@pytest.fixture(scope="module")
def volume_runs(net):
    """The volume, its plain hip prediction, and per spec (host, hip, gap): made once for the tests below."""
    from cswin_unet_amd.utils import predict_volume, tta_views
    from cswin_unet_amd import ops
    vol = det_normal("resize.vol", VOL)
    # precondition, asserted: on this volume the device's cubic zoom is scipy's bit for bit, so both paths feed the network alike
    small = ops.resize_slices(torch.from_numpy(vol).to(DEV), (224, 224))
    torch.cuda.synchronize()
    want = np.stack([zoom(s, (224 / VOL[1], 224 / VOL[2]), order=3) for s in vol])
    assert np.array_equal(small.cpu().numpy().view(np.uint32), want.view(np.uint32))
    runs = {None: predict_volume(vol, net, (224, 224), batch_slices=16, resize="hip")}
    torch.cuda.synchronize()
    for spec in ("flips", "d4"):
        host = predict_volume(vol, net, (224, 224), batch_slices=16, tta=spec)
        torch.cuda.synchronize()
        hip = predict_volume(vol, net, (224, 224), batch_slices=16, resize="hip", tta=spec)
        torch.cuda.synchronize()
        runs[spec] = (host, hip, _host_gap_per_voxel(vol, net, (224, 224), tta_views(spec), 16))
    return vol, runs


@pytest.mark.parametrize("spec", ["flips", "d4"])
def test_predict_volume_hip_with_tta_equals_host(volume_runs, spec):
    vol, runs = volume_runs
    host, hip, gap = runs[spec]
    assert host.shape == hip.shape == gap.shape == VOL and hip.dtype == np.uint8 and host.dtype == np.int64
    T.compare_classes(hip, host, gap, f"predict_volume tta={spec}")
    assert len(np.unique(host)) > 2
    if spec == "d4":
        assert not np.array_equal(hip, runs[None])                      # the ensemble is not the single view


def test_predict_volume_hip_with_tta_composes(volume_runs, net):
    from cswin_unet_amd.utils import predict_volume
    vol, runs = volume_runs
    dev = predict_volume(vol, net, (224, 224), batch_slices=16, resize="hip", tta="flips", return_device=True)
    torch.cuda.synchronize()
    assert dev.is_cuda and dev.dtype == torch.uint8 and tuple(dev.shape) == VOL
    assert np.array_equal(dev.cpu().numpy(), runs["flips"][1])
    one = predict_volume(vol[1], net, (224, 224), resize="hip", tta="flips")
    torch.cuda.synchronize()
    assert one.shape == VOL[1:] and one.dtype == np.uint8
    T.compare_classes(one, runs["flips"][0][1], runs["flips"][2][1], "single slice")


# ---- 8, 9. an equivariant stub, and the evaluation loop -----------------------------------------------------------------------
class _Affine(torch.nn.Module):
    """9 logits that are an affine map of the pixel's value: equivariant under every view (torch arithmetic, test only)."""
    num_classes = 9

    def forward(self, x):
        k = torch.arange(9, dtype=x.dtype, device=x.device).view(1, 9, 1, 1)
        return x * (1.5 - 0.4 * k) + 0.07 * k * (9.5 - k)


def _affine_gap(vol):
    L = _Affine()(torch.from_numpy(vol).unsqueeze(1)).double().numpy()
    e = np.exp(L - L.max(1, keepdims=True))
    return T.top_two_gap(e / e.sum(1, keepdims=True))


def test_an_equivariant_stub_gives_the_same_map_with_and_without_tta():
    from cswin_unet_amd.utils import predict_volume
    vol = det_normal("tta.affine", (4, 40, 40))
    net = _Affine()
    plain = predict_volume(vol, net, (40, 40), batch_slices=16, resize="hip")
    torch.cuda.synchronize()
    d4 = predict_volume(vol, net, (40, 40), batch_slices=16, resize="hip", tta="d4")
    torch.cuda.synchronize()
    assert plain.dtype == d4.dtype == np.uint8 and len(np.unique(plain)) > 3
    T.compare_classes(d4, plain, _affine_gap(vol), "equivariant stub, d4 against none")


def test_evaluate_volumes_with_tta_scores_the_ensembles_prediction():
    from cswin_unet_amd.utils import evaluate_volumes, predict_volume, volume_metrics
    net = _Affine()
    vols = [det_normal("tta.eval.a", (4, 40, 40)), det_normal("tta.eval.b", (3, 40, 40))]
    labels = [np.clip(np.abs(v * 2).astype(np.int64), 0, 8) for v in vols]
    batches = [dict(image=torch.from_numpy(v)[None], label=torch.from_numpy(l)[None], case_name=f"case{i}")
               for i, (v, l) in enumerate(zip(vols, labels))]
    kw = dict(metrics="hip", resize="hip", components="largest", batch_slices=16)
    plain = evaluate_volumes(batches, net, 9, (40, 40), **kw)
    torch.cuda.synchronize()
    got = evaluate_volumes(batches, net, 9, (40, 40), tta="flips", **kw)
    torch.cuda.synchronize()
    assert len(got) == len(plain) == 4 and len(got[0]) == len(plain[0]) == 2 and np.shape(got[1]) == np.shape(plain[1]) == (8, 2)
    assert [np.shape(m) for m in got[0]] == [np.shape(m) for m in plain[0]]
    want = []
    for v, l in zip(vols, labels):
        pred = predict_volume(v, net, (40, 40), batch_slices=16, resize="hip", tta="flips", components="largest")
        torch.cuda.synchronize()
        want.append(volume_metrics(pred, l, 9))
        torch.cuda.synchronize()
    assert got[0] == want
    assert np.array_equal(got[1], sum(np.array(m, dtype=np.float64) for m in want) / 2)
    assert got[2:] == tuple(float(x) for x in np.mean(got[1], axis=0))


# ---- 10. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals():
    from cswin_unet_amd import _lib, ops
    from cswin_unet_amd._lib import CswinHipError, ptr, stream
    from cswin_unet_amd.utils import nearest_index_device, predict_volume

    class Never(torch.nn.Module):
        def forward(self, x):
            raise AssertionError("the network must not run")

    vol = np.zeros((2, 20, 16), np.float32)
    for spec in ("d4", ["transpose"]):
        with pytest.raises(ValueError, match="square"):
            predict_volume(vol, Never(), (32, 24), resize="hip", tta=spec)
        with pytest.raises(ValueError, match="square"):
            predict_volume(vol, Never(), (20, 16), resize="hip", tta=spec)
    x = torch.zeros(2, 6, 8, device=DEV)
    with pytest.raises(CswinHipError, match="h == w"):
        ops.view_batch(x, (0, 3))
    with pytest.raises(CswinHipError, match="views.1."):
        ops.view_batch(x, (0, 8))
    with pytest.raises(CswinHipError):
        ops.view_batch(x, ())
    with pytest.raises(CswinHipError):
        ops.view_batch(x, tuple(range(8)) + (0,))
    with pytest.raises(CswinHipError):
        ops.view_batch(x, (True,))
    with pytest.raises(CswinHipError):
        ops.view_batch(torch.zeros(6, 8, device=DEV), (0,))
    logits = torch.zeros(6, 5, 6, 8, device=DEV)
    with pytest.raises(CswinHipError, match="multiple"):
        ops.tta_argmax_zoom_back(logits, (0, 2, 4, 6), (12, 12))
    with pytest.raises(CswinHipError, match="h == w"):
        ops.tta_argmax_zoom_back(logits, (0, 7), (12, 12))
    with pytest.raises(CswinHipError, match="views.2."):
        ops.tta_argmax_zoom_back(logits, (0, 2, 9), (12, 12))
    with pytest.raises(CswinHipError):
        ops.tta_argmax_zoom_back(logits, (0, 2), (12, 12), classes=[0, 5])
    with pytest.raises(CswinHipError):
        ops.tta_argmax_zoom_back(logits[0], (0,), (12, 12))

    # the C entry points: an error code and nothing written (the buffers keep their pattern)
    h = _lib.lib()
    out = torch.full((3, 12, 12), 0xA5, dtype=torch.uint8, device=DEV)
    probs = torch.full((3, 5, 6, 8), 7.0, device=DEV)
    y = torch.full((2, 2, 6, 8), 7.0, device=DEV)
    rows, cols = nearest_index_device(6, 12, DEV), nearest_index_device(8, 12, DEV)

    def ens(views, V=None, nsel=5, probs_=probs, ncls=5, hh=6):
        table = (ctypes.c_int * max(1, len(views)))(*views)
        return h.cswin_tta_argmax_zoom_back(ptr(logits), ptr(out), ptr(probs_), ptr(rows), ptr(cols), table, len(views) if V is None else V,
                                            None, nsel, 3, ncls, hh, 8, 12, 12, stream())

    def view(views, V=None):
        table = (ctypes.c_int * max(1, len(views)))(*views)
        return h.cswin_view_batch(ptr(x), ptr(y), table, len(views) if V is None else V, 2, 6, 8, stream())

    for fn, kw, what in ((ens, dict(views=(0, 1)), "views[1] transposes"), (ens, dict(views=(8, 0)), "views[0] is not a view code"),
                         (ens, dict(views=(0, -1)), "views[1] is not"), (ens, dict(views=(0,), V=0), "V=0"), (ens, dict(views=(0,), V=9), "V=9"),
                         (ens, dict(views=(0, 2), nsel=0), "nsel=0"), (ens, dict(views=(0, 2), nsel=4), "nsel=4"),
                         (ens, dict(views=(0, 2), hh=0), "outside the supported"), (view, dict(views=(0, 5)), "views[1] transposes"),
                         (view, dict(views=(0, 8)), "views[1] is not a view code"), (view, dict(views=(0,), V=0), "V=0"),
                         (view, dict(views=(0,), V=9), "V=9")):
        rc, msg = fn(**kw), h.cswin_last_error().decode()
        assert rc == ERR_SHAPE and what in msg, (rc, what, msg)
        assert msg.startswith("tta_argmax_zoom_back" if fn is ens else "view_batch"), msg
    assert ens((0, 2), nsel=17, ncls=17, probs_=None) == ERR_WORKSPACE and "probs" in h.cswin_last_error().decode()
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all()) and bool((probs == 7.0).all()) and bool((y == 7.0).all())
    assert ens((0, 2)) == 0 and view((2, 4)) == 0                       # and the same calls with good views run
    torch.cuda.synchronize()
    assert bool((out == 0).all()) and bool((probs == 0.2).all()) and bool((y == 0).all())
