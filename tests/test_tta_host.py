"""Host side of test-time augmentation (cswin_unet_amd.utils: tta_views, apply_view / undo_view / tta_view_position, the host
path of predict_volume(tta=...), the tta argument of the volume loop) and the references of tests/tta_cases.py that the device
tests rest on.  No GPU."""
import numpy as np
import pytest
import torch
from scipy.ndimage import zoom

import tta_cases as T
from cswin_unet_amd import ops, utils
from cswin_unet_amd._lib import CswinHipError


# ---- tta_views ---------------------------------------------------------------------------------------------------------------
def test_tta_views_accepts_every_spec():
    assert utils.tta_views(None) is None
    assert utils.tta_views("flips") == (0, 2, 4, 6)
    assert utils.tta_views("d4") == (0, 1, 2, 3, 4, 5, 6, 7)
    assert utils.TTA_VIEW_NAMES == T.NAMES
    for name, code in T.NAMES.items():
        assert utils.tta_views([name]) == (code,)
        assert utils.tta_views((code,)) == (code,)
    assert utils.tta_views([6, "rot90", np.int64(0)]) == (6, 3, 0)
    assert utils.tta_views(list(T.NAMES)) == tuple(T.NAMES.values())
    assert utils.tta_views(range(8)) == T.CODES
    assert utils.tta_views(np.array([4, 1])) == (4, 1) and all(type(c) is int for c in utils.tta_views(np.array([4, 1])))


@pytest.mark.parametrize("spec,names", [((0, 0), "0"), (["rot90", 3], "3"), ([], "0 views"), (tuple(range(8)) + (0,), "9 views"),
                                        (["rot45"], "rot45"), ([True], "True"), ([0, 8], "8"), ([-1], "-1"), ([1.0], "1.0"),
                                        ("rot90", "rot90"), ("D4", "D4"), (3, "3"), ([None], "None")],
                         ids=["duplicate", "duplicate-by-name", "empty", "nine", "unknown-name", "bool", "code-8", "negative", "float",
                              "a-name-alone", "case", "not-a-sequence", "none-entry"])
def test_tta_views_refuses_and_names_the_entry(spec, names):
    with pytest.raises(ValueError, match=names):
        utils.tta_views(spec)


# ---- the index map -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,codes", [((5, 5), T.CODES), ((3, 7), T.STRAIGHT), ((1, 1), T.CODES)], ids=["5x5", "3x7", "1x1"])
def test_the_index_map_is_numpys(shape, codes):
    h, w = shape
    x = np.arange(h * w, dtype=np.float32).reshape(h, w)
    for c in codes:
        t = c & 1
        a = x.T if t else x
        a = a[::-1, :] if c & 2 else a
        a = a[:, ::-1] if c & 4 else a                                  # the definition, written out
        assert np.array_equal(utils.apply_view(x, c), a) and np.array_equal(T.view_np(x, c), a)
        assert a.shape == ((w, h) if t else (h, w))
        for r in range(h):
            for s in range(w):
                i, j = utils.tta_view_position(c, r, s, h, w)
                assert a[i, j] == x[r, s], (c, r, s)
        assert np.array_equal(utils.undo_view(utils.apply_view(x, c), c), x)
        assert np.array_equal(T.back_np(T.view_np(x, c), c), x)
        assert np.array_equal(utils.apply_view(utils.apply_view(x, c), T.inverse_code(c)), x)
    if h == w:
        assert np.array_equal(utils.apply_view(x, T.NAMES["rot90"]), np.rot90(x, 1))
        assert np.array_equal(utils.apply_view(x, T.NAMES["rot270"]), np.rot90(x, 3))
        assert np.array_equal(utils.apply_view(x, T.NAMES["rot180"]), np.rot90(x, 2))
        assert np.array_equal(utils.apply_view(x, T.NAMES["anti_transpose"]), np.rot90(x, 2).T)
        if h > 1:
            assert len({utils.apply_view(x, c).tobytes() for c in T.CODES}) == 8


def test_views_act_on_the_last_two_axes_of_a_batch():
    x = np.random.default_rng(0).standard_normal((3, 2, 4, 4))
    for c in T.CODES:
        got = utils.apply_view(x, c)
        assert all(np.array_equal(got[a, b], T.view_np(x[a, b], c)) for a in range(3) for b in range(2))
        assert np.array_equal(utils.undo_view(got, c), x)


# ---- the reference of the device tests ---------------------------------------------------------------------------------------
def test_the_host_ensemble_is_the_written_definition():
    """utils.ensemble_views_host against tta_cases.ensemble_np on logits whose views differ, with and without a class list, and
    the special values: a NaN or +inf logit in any view gives position 0."""
    views = (3, 0, 6, 5)
    L = (3.0 * np.random.default_rng(1).standard_normal((4, 2, 7, 6, 6))).astype(np.float32)
    L[1, 0, 4, 2, 3] = np.nan
    L[2, 1, 5, 0, 0] = np.inf
    for classes in (None, [6, 4, 3, 3, 5]):
        cls, P = utils.ensemble_views_host(torch.from_numpy(L.reshape(8, 7, 6, 6)), views, classes)
        want = T.ensemble_np(L, views, classes)
        assert np.array_equal(P, want, equal_nan=True) and np.array_equal(cls, T.classes_of(want))
        bad = np.isnan(want).any(1)
        assert bad.sum() == 2 and (cls[bad] == 0).all() and np.isnan(want[:, :, ~bad.any(0)]).sum() == 0
    # the NaN lands where the view's inverse puts it: view 0 (index 1) is the identity, view 6 (index 2) turns (0, 0) into (5, 5)
    bad = np.isnan(T.ensemble_np(L, views)).any(1)
    assert bad[0, 2, 3] and bad[1, 5, 5]


@pytest.mark.parametrize("tag", [c[0] for c in T.PROB_CASES])
def test_the_seeded_cases_have_few_near_ties(tag):
    """What the device class-map test presupposes, checked here on the CPU for every case."""
    _, P, cls, gap = T.prob_case(tag)
    share = (gap <= T.GAP).mean()
    print(f"{tag}: {gap.size} pixels, near-tie share {share:.2e}, smallest gap {gap.min():.3e}")
    assert share <= T.EXCUSED
    assert np.isfinite(P).all() and abs(P.sum(1) - 1).max() < 1e-12
    assert len(np.unique(cls)) > min(8, P.shape[1] // 2)                 # the classes are spread: a constant map would hide errors


def test_vote_logits_have_their_closed_form_winner():
    for views, hw, size, classes in T.vote_cases():
        L = T.vote_logits(views, 2, *hw)
        P = T.ensemble_np(L, views, classes)
        cls, fixed = T.classes_of(P), T.fixed_class(2, *hw)
        if len(views) > 1:
            want = fixed if classes is None else np.array([classes.index(k) for k in range(9)])[fixed]
            assert np.array_equal(cls, want), (views, hw)
            if classes is None:                                         # (a repeated class ties with itself, exactly: the first wins)
                assert T.top_two_gap(P).min() >= 0.5 * (1 - 1 / len(views)) - 1e-6
            else:
                others = np.array(classes)[None, :, None, None] != fixed[:, None]
                assert (np.take_along_axis(P, want[:, None], 1) - P)[others].min() >= 0.25 - 1 / 6 - 1e-6
        else:
            assert np.array_equal(cls, np.minimum(fixed, (np.arange(hw[0])[:, None] + 2 * np.arange(hw[1])[None]) % 9))


# ---- predict_volume on the host ----------------------------------------------------------------------------------------------
class _PerPixel(torch.nn.Module):
    """9 logits that depend on the pixel's value only: equivariant under every view."""
    num_classes = 9

    def __init__(self):
        super().__init__()
        self.calls = 0

    def forward(self, x):
        self.calls += 1
        k = torch.arange(9, dtype=x.dtype).view(1, 9, 1, 1)              # products and sums only: the same bits wherever a pixel lies
        return x * (1.0 - 0.37 * k) + (x * x) * (0.11 * k - 0.4) + 0.05 * k * (8 - k)


class _Positional(torch.nn.Module):
    """14 fixed "logit" planes: channel c of pixel (i, j) is a hash of (c, i, j, the input's value there), as
    tests/test_continual_eval_host.py's stub."""
    num_classes = 14

    def __init__(self):
        super().__init__()
        self.calls = 0

    def forward(self, x):
        self.calls += 1
        B, _, H, W = x.shape
        g = torch.Generator().manual_seed(5)
        base = torch.randn(14, H, W, generator=g)
        return base[None] * (1.0 + x) + torch.roll(base, 3, dims=0)[None]


def _volume(shape, seed=3):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def test_an_equivariant_network_gives_the_same_answer_with_and_without_tta():
    net, vol = _PerPixel(), _volume((5, 12, 12))
    logits = net(torch.from_numpy(vol).unsqueeze(1)).double().numpy()
    P = np.exp(logits - logits.max(1, keepdims=True))
    P /= P.sum(1, keepdims=True)
    assert T.top_two_gap(P).min() >= 1e-9                               # the precondition: no pixel near a tie
    plain = utils.predict_volume(vol, net, (12, 12), batch_slices=4, device="cpu")
    for spec in ("d4", "flips", ["rot90"]):
        got = utils.predict_volume(vol, net, (12, 12), batch_slices=4, device="cpu", tta=spec)
        assert got.dtype == plain.dtype and np.array_equal(got, plain), spec
    assert len(np.unique(plain)) > 3


def _restated(vol, net, patch, codes, class_indices=None):
    """The ensemble restated with np.rot90 / np.flip: view -> network -> float64 softmax -> back -> mean -> argmax -> zoom."""
    make = {0: lambda a: a, 1: lambda a: np.flip(np.rot90(a, 1), 0), 2: lambda a: np.flip(a, 0), 3: lambda a: np.rot90(a, 1),
            4: lambda a: np.flip(a, 1), 5: lambda a: np.rot90(a, 3), 6: lambda a: np.rot90(a, 2), 7: lambda a: np.flip(np.rot90(a, 1), 1)}
    undo = {0: lambda a: a, 1: lambda a: np.rot90(np.flip(a, 0), 3), 2: lambda a: np.flip(a, 0), 3: lambda a: np.rot90(a, 3),
            4: lambda a: np.flip(a, 1), 5: lambda a: np.rot90(a, 1), 6: lambda a: np.rot90(a, 2), 7: lambda a: np.rot90(np.flip(a, 1), 3)}
    D, x, y = vol.shape
    out = np.zeros(vol.shape, np.int64)
    for d in range(D):
        s = zoom(vol[d], (patch[0] / x, patch[1] / y), order=3) if (x, y) != tuple(patch) else vol[d]
        P = 0.0
        for c in codes:
            lg = net(torch.from_numpy(np.ascontiguousarray(make[c](s)))[None, None].float())[0].double().numpy()
            lg = lg if class_indices is None else lg[list(class_indices)]
            e = np.exp(lg - lg.max(0, keepdims=True))
            P = P + np.stack([undo[c](p) for p in e / e.sum(0, keepdims=True)])
        cls = np.argmax(P / len(codes), 0)
        out[d] = zoom(cls, (x / patch[0], y / patch[1]), order=0) if (x, y) != tuple(patch) else cls
    return out


@pytest.mark.parametrize("spec,shape,patch,idx", [("d4", (5, 16, 16), (16, 16), None), ("d4", (3, 20, 14), (12, 12), None),
                                                  (["rot270", "transpose", 0], (3, 16, 16), (16, 16), [0, 12, 13, 5]),
                                                  ("flips", (5, 16, 12), (16, 12), None), ("flips", (3, 20, 14), (12, 9), [11, 0, 9]),
                                                  ([7], (2, 9, 9), (9, 9), None)],
                         ids=["d4", "d4-zoomed", "names-classes", "flips-non-square", "flips-zoomed-non-square-classes", "anti-transpose"])
def test_a_position_dependent_network_follows_the_restatement(spec, shape, patch, idx):
    net, vol = _Positional(), _volume(shape)
    codes = utils.tta_views(spec)
    got = utils.predict_volume(vol, net, patch, batch_slices=8, device="cpu", tta=spec, class_indices=idx)
    assert net.calls == -(-shape[0] // max(1, 8 // len(codes)))          # one call per batch of max(1, batch_slices // V) slices
    want = _restated(vol, net, patch, codes, idx)
    assert got.shape == shape and got.dtype == np.int64 and np.array_equal(got, want)
    plain = utils.predict_volume(vol, net, patch, batch_slices=8, device="cpu", class_indices=idx)
    assert not np.array_equal(got, plain)
    assert got.max() < (14 if idx is None else len(idx))
    single = utils.predict_volume(vol[0], net, patch, device="cpu", tta=spec, class_indices=idx)
    assert single.shape == shape[1:] and np.array_equal(single, want[0])


def test_a_transposing_view_with_a_non_square_patch_is_refused_before_the_network_runs():
    net, vol = _Positional(), _volume((2, 16, 12))
    image, label = torch.from_numpy(vol)[None], torch.zeros((1,) + vol.shape, dtype=torch.int64)

    def loader():
        raise AssertionError("the loader must not be read")
        yield

    for spec in ("d4", ["rot90"], [0, 7]):
        with pytest.raises(ValueError, match="square"):
            utils.predict_volume(vol, net, (16, 12), device="cpu", tta=spec)
        with pytest.raises(ValueError, match="square"):
            utils.predict_volume(np.zeros((2, 16, 16), np.float32), net, (16, 12), device="cpu", tta=spec)
        with pytest.raises(ValueError, match="square"):
            utils.test_single_volume(image, label, net, classes=14, patch_size=[16, 12], device="cpu", tta=spec)
        with pytest.raises(ValueError, match="square"):
            utils.evaluate_volumes(loader(), net, 14, (16, 12), metrics="host", device="cpu", tta=spec)
    with pytest.raises(ValueError, match="rot45"):
        utils.predict_volume(vol, net, (16, 12), device="cpu", tta=["rot45"])
    with pytest.raises(ValueError, match="rot45"):
        utils.evaluate_volumes(loader(), net, 14, (16, 12), metrics="host", device="cpu", tta=["rot45"])
    assert net.calls == 0
    utils.predict_volume(vol, net, (16, 12), device="cpu", tta="flips")
    assert net.calls == 1


def test_tta_none_is_the_call_without_the_argument():
    net, vol = _Positional(), _volume((4, 16, 12))
    label = np.zeros(vol.shape, np.int64)
    label[:, 4:9, 3:8] = 2
    label[1:3, 10:14, 2:6] = 1
    image, lab = torch.from_numpy(vol)[None], torch.from_numpy(label)[None]
    assert np.array_equal(utils.predict_volume(vol, net, (16, 12), device="cpu", tta=None), utils.predict_volume(vol, net, (16, 12), device="cpu"))
    kw = dict(classes=14, patch_size=[16, 12], device="cpu")
    assert utils.test_single_volume(image, lab, net, tta=None, **kw) == utils.test_single_volume(image, lab, net, **kw)
    batches = [dict(image=image, label=lab, case_name="a"), dict(image=image.flip(1), label=lab.flip(1), case_name=["b"])]
    with_none = utils.evaluate_volumes(batches, net, 14, (16, 12), metrics="host", device="cpu", tta=None)
    without = utils.evaluate_volumes(batches, net, 14, (16, 12), metrics="host", device="cpu")
    assert with_none[0] == without[0] and np.array_equal(with_none[1], without[1]) and with_none[2:] == without[2:]
    flips = utils.evaluate_volumes(batches, net, 14, (16, 12), metrics="host", device="cpu", tta="flips")
    assert len(flips) == len(without) and np.shape(flips[1]) == np.shape(without[1]) and flips[0] != without[0]


def test_the_new_ops_have_no_cpu_fallback():
    with pytest.raises(CswinHipError):
        ops.view_batch(torch.zeros(2, 4, 4), (0, 2))
    with pytest.raises(CswinHipError):
        ops.tta_argmax_zoom_back(torch.zeros(4, 3, 4, 4), (0, 2), (8, 8))
    assert "view_batch" in ops.__all__ and "tta_argmax_zoom_back" in ops.__all__
