"""Connected components and the component filter on the device (csrc/components.hip behind ops.connected_components /
ops.filter_components and the `components` keyword of the volume evaluation) against scipy (tests/components_cases.py).

Everything is an exact integer result: labels, sizes and filtered volumes are compared with torch.equal, no tolerance anywhere.
The shapes are sized from ops.COMPONENT_TILE so that ragged tiles, several tiles along every axis and every seam direction
occur.  Every device call is followed by a synchronize so that a failing step ends its test before anything else is enqueued."""
import ctypes

import numpy as np
import pytest
import torch

from components_cases import (StubNet, canonical_labels, checkerboard, noise, organ_volume, rule_tables, scipy_filter, serpentine,
                              speckled_two_class)

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _tile():
    from cswin_unet_amd import ops
    return ops.COMPONENT_TILE


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _check_labels(vol, ncls, dvol=None):
    """labels and sizes of the device against canonical_labels; returns the device pair."""
    from cswin_unet_amd import ops
    dvol = _dev(vol) if dvol is None else dvol
    labels, sizes = ops.connected_components(dvol, ncls, return_sizes=True)
    torch.cuda.synchronize()
    only = ops.connected_components(dvol, ncls)
    torch.cuda.synchronize()
    wl, ws = canonical_labels(vol, ncls)
    assert labels.dtype == torch.int32 and sizes.dtype == torch.int32 and labels.shape == dvol.shape == sizes.shape
    gl, gs = labels.cpu(), sizes.cpu()
    bad = (gl != torch.from_numpy(wl)).nonzero()
    print(f"{tuple(vol.shape)} ncls {ncls}: {int((ws > 0).sum())} components, largest {int(ws.max())}, {bad.shape[0]} label mismatches")
    assert torch.equal(gl, torch.from_numpy(wl)), [(idx.tolist(), int(gl[tuple(idx)]), int(wl[tuple(idx)])) for idx in bad[:8]]
    bad = (gs != torch.from_numpy(ws)).nonzero()
    assert torch.equal(gs, torch.from_numpy(ws)), [(idx.tolist(), int(gs[tuple(idx)]), int(ws[tuple(idx)])) for idx in bad[:8]]
    assert torch.equal(only.cpu(), gl)                                  # the call without sizes labels the same
    return labels, sizes


def _noise_shapes():
    Tz, Ty, Tx = _tile()
    return [(5, 9, 11), (2 * Tz + 1, 2 * Ty + 3, 2 * Tx + 5)]


@pytest.mark.parametrize("which", [0, 1])
def test_seeded_noise(which):
    shape = _noise_shapes()[which]
    _check_labels(noise(shape, 4, 0.55, 100 + which), 4)


@pytest.mark.parametrize("which", ["slice", "layers"])
def test_serpentine_is_one_component(which):
    Tz, Ty, Tx = _tile()
    shape = (1, 4 * Ty + 1, 4 * Tx + 2) if which == "slice" else (2 * Tz + 1, Ty + 1, Tx + 1)
    vol = serpentine(shape)
    labels, sizes = _check_labels(vol, 2)
    torch.cuda.synchronize()
    assert int(sizes.flatten()[0]) == int(vol.sum()) and int((sizes > 0).sum()) == 1


def test_checkerboard_has_no_unions():
    Tz, Ty, Tx = _tile()
    vol = checkerboard((Tz + 1, Ty + 2, Tx + 3))
    labels, sizes = _check_labels(vol, 3)
    torch.cuda.synchronize()
    assert torch.equal(labels.flatten().cpu(), torch.arange(1, vol.size + 1, dtype=torch.int32)) and bool((sizes == 1).all())


def test_solid_is_one_component():
    Tz, Ty, Tx = _tile()
    vol = np.ones((Tz + 1, 2 * Ty, 2 * Tx + 1), np.uint8)
    labels, sizes = _check_labels(vol, 2)
    torch.cuda.synchronize()
    assert bool((labels == 1).all()) and int(sizes.flatten()[0]) == vol.size


@pytest.mark.parametrize("shape", ["1x1x1", "1x1xW", "1xHx1", "Dx1x1", "HxW"])
def test_degenerate_shapes(shape):
    Tz, Ty, Tx = _tile()
    dims = {"1x1x1": (1, 1, 1), "1x1xW": (1, 1, 2 * Tx + 7), "1xHx1": (1, 2 * Ty + 5, 1), "Dx1x1": (2 * Tz + 3, 1, 1),
            "HxW": (Ty + 3, Tx + 9)}[shape]
    _check_labels(noise(dims, 2, 0.7, 7), 3)
    _check_labels(np.ones(dims, np.uint8), 2)


def test_unaligned_input_takes_the_scalar_loads():
    Tz, Ty, Tx = _tile()
    shape = (Tz + 1, Ty + 1, 2 * Tx)                                    # rows that would be 16-B aligned in an aligned buffer
    vol = noise(shape, 4, 0.6, 9)
    buf = torch.zeros(vol.size + 16, dtype=torch.uint8, device=DEV)
    view = buf[1:1 + vol.size].view(shape)
    view.copy_(_dev(vol))
    torch.cuda.synchronize()
    assert view.data_ptr() % 16 == 1 and view.is_contiguous()
    _check_labels(vol, 4, dvol=view)
    from cswin_unet_amd import ops
    out = ops.filter_components(view, 4, "largest")
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), torch.from_numpy(scipy_filter(vol, 4, *rule_tables("largest", 4))))


ORGAN_RULES = {
    "largest": "largest",
    "min_size": {c: {"min_size": 2 + c} for c in range(1, 9)},
    "half": {c: {"min_fraction": 0.5} for c in (1, 3, 5, 8)},
}


@pytest.fixture(scope="module")
def organ():
    return organ_volume()          # built once; no test writes to it


def test_organ_labels(organ):
    _check_labels(organ, 9)
    _check_labels(organ, 5)                                             # classes 5..8 become background


@pytest.mark.parametrize("rule", sorted(ORGAN_RULES))
def test_organ_filter_rules(organ, rule):
    from cswin_unet_amd import ops
    want = scipy_filter(organ, 9, *rule_tables(ORGAN_RULES[rule], 9))
    dvol = _dev(organ)
    out = ops.filter_components(dvol, 9, ORGAN_RULES[rule])
    torch.cuda.synchronize()
    again = ops.filter_components(dvol, 9, ORGAN_RULES[rule])
    torch.cuda.synchronize()
    assert out.dtype == torch.uint8 and torch.equal(dvol.cpu(), torch.from_numpy(organ.copy()))          # the input is left alone
    print(f"rule {rule}: {int((out.cpu() != torch.from_numpy(organ.copy())).sum())} voxels dropped, {int((want != organ).sum())} by scipy")
    assert torch.equal(out.cpu(), torch.from_numpy(want)) and (want != organ).any()
    assert torch.equal(out, again)                                      # two runs, the same bits
    if rule != "min_size":                                              # the duplicated class-3 organ ties for the largest: both stay
        assert (canonical_labels(out.cpu().numpy() == 3, 2)[1] > 0).sum() == 2
    ret = ops.filter_components(dvol, 9, ORGAN_RULES[rule], out=dvol)   # in place
    torch.cuda.synchronize()
    assert ret is dvol and torch.equal(dvol, out)


def test_labels_are_the_same_bits_on_every_run(organ):
    from cswin_unet_amd import ops
    dvol = _dev(organ)
    a = ops.connected_components(dvol, 9, return_sizes=True)
    torch.cuda.synchronize()
    b = ops.connected_components(dvol, 9, return_sizes=True)
    torch.cuda.synchronize()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_error_returns_before_any_launch():
    from cswin_unet_amd import _lib, ops
    from cswin_unet_amd._lib import CswinHipError
    h = _lib.lib()
    D, H, W = 3, 5, 7
    N = D * H * W
    need = h.cswin_components_workspace(D, H, W)
    assert need >= 2 * 4 * N and h.cswin_components_workspace(0, H, W) == 0 and h.cswin_components_workspace(D, 2049, W) == 0
    vol = torch.zeros(N + 8, dtype=torch.uint8, device=DEV)
    labels, sizes = torch.full((N,), -7, dtype=torch.int32, device=DEV), torch.full((N,), -7, dtype=torch.int32, device=DEV)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    ms, mf = torch.zeros(256, dtype=torch.int64, device=DEV), torch.zeros(256, dtype=torch.float64, device=DEV)
    out = torch.full((N,), 9, dtype=torch.uint8, device=DEV)
    P = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    st = _lib.stream()
    SHAPE, WORKSPACE, UNSUPPORTED = -1, -3, -5
    label = lambda ncls=4, nbytes=need, d=D: h.cswin_components_label(P(vol), P(labels), P(sizes), P(ws), nbytes, d, H, W, ncls, st)
    filt = lambda o, ncls=4, nbytes=need: h.cswin_components_filter(P(vol), P(labels), P(sizes), P(ms), P(mf), o, P(ws), nbytes, D, H, W, ncls, st)
    assert label(ncls=1) == UNSUPPORTED and label(ncls=256) == UNSUPPORTED and b"ncls" in h.cswin_last_error()
    assert label(nbytes=need - 1) == WORKSPACE and label(d=0) == SHAPE and label(d=2049) == SHAPE
    assert filt(P(out), ncls=1) == UNSUPPORTED and filt(P(out), ncls=256) == UNSUPPORTED
    assert filt(P(out), nbytes=need - 1) == WORKSPACE
    assert filt(P(vol, 1)) == UNSUPPORTED and filt(P(labels)) == UNSUPPORTED and b"overlap" in h.cswin_last_error()
    torch.cuda.synchronize()
    assert bool((labels == -7).all()) and bool((sizes == -7).all()) and bool((out == 9).all())          # nothing was launched
    for bad in (torch.zeros((2, 3, 4), dtype=torch.uint8), torch.zeros((2, 3, 4), dtype=torch.int32, device=DEV),
                torch.zeros((4,), dtype=torch.uint8, device=DEV)):
        with pytest.raises(CswinHipError):
            ops.connected_components(bad, 4)
    with pytest.raises(ValueError):
        ops.filter_components(vol[:N].view(D, H, W), 4, {4: {"min_size": 1}})
    with pytest.raises(CswinHipError):
        ops.connected_components(vol[:N].view(D, H, W), 256)


def test_single_volume_end_to_end_matches_the_host_path_and_lowers_hd95():
    from cswin_unet_amd.utils import test_single_volume
    pred, lab = speckled_two_class()
    lab = lab.copy()
    lab[1:5, 8:20, 22:24] = 0                                           # the label differs a little from the prediction's organ
    image, label = torch.zeros((1,) + pred.shape), torch.from_numpy(lab)[None]
    kw = dict(classes=2, patch_size=list(pred.shape[1:]), batch_slices=4, device=DEV)
    hip = test_single_volume(image, label, StubNet(pred, 2), resize="hip", metrics="hip", components="largest", **kw)
    torch.cuda.synchronize()
    host = test_single_volume(image, label, StubNet(pred, 2), resize="host", metrics="host", components="largest", **kw)
    torch.cuda.synchronize()
    raw = test_single_volume(image, label, StubNet(pred, 2), resize="hip", metrics="hip", components=None, **kw)
    torch.cuda.synchronize()
    print(f"filtered hip {hip} host {host}; unfiltered {raw}")
    assert hip == host
    assert hip[0][1] < raw[0][1] and hip[0][0] > raw[0][0]
