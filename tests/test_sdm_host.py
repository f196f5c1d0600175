"""Host side of the boundary loss (no GPU): utils.signed_distance_maps_host against an all-pairs brute-force minimum in integers,
and the float64 restatement of the boundary objective that tests/test_gpu_boundary_loss.py holds the device to -- bd_ref,
bd_final_ref and bd_grad_ref, extensions of loss_ref / final_ref / grad_ref of tests/test_gpu_step_tail.py -- with the check that
the bound of the new sum sees the bugs it is there for."""
import functools

import numpy as np
import pytest
import torch

from oracle.determ import det_normal

import sdm_cases as S
from test_gpu_shapes import D
from test_gpu_step_tail import U, cdiv, dice_terms, final_ref, loss_blocks, loss_graph, loss_ref, trips


# ------------------------------------------------------------------------------------------------
# the maps
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", S.HOST_KINDS)
@pytest.mark.parametrize("shape", S.HOST_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_maps_equal_the_all_pairs_minimum(shape, kind):
    from cswin_unet_amd.utils import signed_distance_maps_host
    ncls = 4
    lab = S.host_labels(kind, *shape, ncls=ncls)
    got, want = signed_distance_maps_host(lab, ncls), S.brute_maps(lab, ncls)
    assert got.dtype == np.float32 and got.shape == (2, ncls) + shape
    assert np.array_equal(got, want)
    member = lab[:, None] == np.arange(ncls)[None, :, None, None]
    assert (got[member] <= 0).all() and (got[~member] >= 0).all()
    if kind == "full":
        assert not got[1].any() and not got[0, ncls - 1].any()                 # the full and the absent class, and the classes beside the full one
    if kind == "absent":
        assert not got[:, ncls - 1].any()
    if kind == "one_pixel" and shape != (1, 1):
        assert got[0, ncls - 1, shape[0] // 2, shape[1] // 2] == 0 and got[0, ncls - 1].max() >= 1
    if kind == "oor":
        bad = (lab < 0) | (lab >= ncls)
        assert bad.sum() >= 1
        if shape != (1, 1):
            assert (got[np.broadcast_to(bad[:, None], got.shape)] > 0).any()   # outside every mask: a plain distance
        assert np.array_equal(got, signed_distance_maps_host(np.where(bad, 77, lab), ncls))


def test_host_maps_take_tensors_and_refuse_other_shapes():
    from cswin_unet_amd.utils import signed_distance_maps_host
    lab = S.host_labels("random", 7, 13)
    assert np.array_equal(signed_distance_maps_host(torch.from_numpy(lab), 4), signed_distance_maps_host(lab, 4))
    with pytest.raises(ValueError):
        signed_distance_maps_host(lab[0], 4)
    with pytest.raises(ValueError):
        signed_distance_maps_host(lab.astype(np.float32), 4)


def test_far_case_reaches_315_and_device_cases_cover_the_plan():
    phi = S.gpu_reference("far224")
    assert 315.0 < float(phi.max()) < 316.0 and float(phi.min()) < -300.0     # the background's inside distance to the one pixel
    assert not phi[:, 2:].any()
    heights = {c[3] for c in S.GPU_CASES}
    for step in S.TX_STEPS:
        assert {step, step + 1} <= heights and S.tx_of(step) == 2 * S.tx_of(step + 1)
    assert S.SDM_MAX_DIM in heights and S.SDM_MAX_DIM in {c[4] for c in S.GPU_CASES}
    assert {2, 16, 255} <= {c[2] for c in S.GPU_CASES}
    ref = S.gpu_reference("absentfull224")
    assert not ref[:, 8].any() and not ref[1].any() and ref[0, :8].any()
    assert len({c[0] for c in S.GPU_CASES}) == len(S.GPU_CASES)


# ------------------------------------------------------------------------------------------------
# float64 restatement of the boundary objective
# ------------------------------------------------------------------------------------------------
def default_wb(ncls):
    """Kervadec's idc: every class but the background."""
    return np.array([0.0] + [1.0] * (ncls - 1))


def bd_ref(x, lab, phi, wb=None, _wrong=None):
    """(sums, bound) of cswin_bd_loss_sums: loss_ref's 1 + 3*ncls entries and bounds, then sum over pixels and classes of
    t = wb_c * p_c * phi_c with the bound of loss_ref's rule, 2^-24 * (sum a |t| + depth * sum |t|): a = r_c + 2, the roundings of
    the probability (loss_ref's r_c) and the two products -- wb and phi are exact --, and loss_ref's depth.  The terms are signed,
    so the bound works on |t|.  x, phi (B, ncls, HW), lab (B, HW); wb None: default_wb.

    _wrong (the sensitivity test alone): "drop_class" (the last class's term missing), "sign_in_mask" (+(d - 1) inside the mask),
    "no_minus_one" (-d inside the mask where the definition has -(d - 1))."""
    B, ncls, HW = x.shape
    base, bbase = loss_ref(x, lab)
    v = x.astype(np.float64)
    d = v - v.max(1, keepdims=True)
    e = np.exp(d)
    p = e / e.sum(1, keepdims=True)
    eps = 2.0 + 2.5 * np.abs(d)
    r = eps + ((p * eps).sum(1) + (ncls - 1))[:, None] + 3.0             # loss_ref's r_c
    w = default_wb(ncls) if wb is None else np.asarray(wb, np.float64)
    f = np.asarray(phi, np.float64)
    inside = np.asarray(lab, np.int64)[:, None, :] == np.arange(ncls)[None, :, None]
    if _wrong == "sign_in_mask":
        f = np.where(inside, -f, f)
    if _wrong == "no_minus_one":
        f = np.where(inside, f - 1.0, f)
    t = w[None, :, None] * p * f
    if _wrong == "drop_class":
        t = t[:, :-1]
        r = r[:, :-1]
    blocks = loss_blocks(B * HW)
    depth = trips(B * HW, blocks)[1] + 6 + 3 + cdiv(blocks, 16) + 16
    bound = U * (((r + 2.0) * np.abs(t)).sum() + depth * np.abs(t).sum())
    return np.concatenate([base, [t.sum()]]), np.concatenate([bbase, [bound]])


def bd_final_ref(sums, n_pixels, w_ce, w_dice, alpha, cw=None, bsums=None):
    """cswin_bd_loss_finalize in float64: ((loss, ce, dice, boundary), their bounds, coef).  final_ref on the first 1 + 3*ncls sums;
    boundary = S / n carries its sum's bound and 2 roundings; the loss adds alpha * boundary: the product and one more addition."""
    sums = np.asarray(sums, np.float64)
    bs = np.zeros_like(sums) if bsums is None else np.asarray(bsums, np.float64)
    out, bout, coef = final_ref(sums[:-1], n_pixels, w_ce, w_dice, cw, bs[:-1])
    bd = sums[-1] / n_pixels
    b_bd = bs[-1] / n_pixels + 2 * U * abs(bd)
    loss = out[0] + (alpha * bd if alpha != 0 else 0.0)
    b_loss = bout[0] + (abs(alpha) * b_bd + U * abs(alpha * bd) + U * (abs(out[0]) + abs(alpha * bd)) if alpha != 0 else 0.0)
    return np.array([loss, out[1], out[2], bd]), np.array([b_loss, bout[1], bout[2], b_bd]), coef


def bd_graph(x, phi, wb=None):
    """sum over pixels and classes of wb_c * softmax(x)_c * phi_c as a float64 tensor on the autograd graph of x."""
    ncls = x.shape[1]
    w = torch.as_tensor(default_wb(ncls) if wb is None else np.asarray(wb, np.float64))
    return (w[None, :, None] * torch.softmax(x, 1) * torch.as_tensor(np.asarray(phi, np.float64))).sum()


def bd_grad_ref(x, lab, phi, wb, ce_scale, dice_scale, bd_coef, g=1.0, cw=None):
    """d/dx of g * (ce_scale * sum -log p[label] + dice_scale * sum_c w_c dice_c + bd_coef * sum wb p phi), by float64 autograd;
    bd_coef = alpha * bd_scale."""
    xl = D(x)
    nll, I, Y, Z = loss_graph(xl, lab)
    (g * (ce_scale * nll + dice_scale * dice_terms(I, Y, Z, cw) + bd_coef * bd_graph(xl, phi, wb))).backward()
    return xl.grad


# ---- the boundary loss's device cases: (id, B, (H, W), ncls, label kind, wb given, Dice class weights given) -------------------------
NC_SWITCH = (2, 3, 4, 5, 6, 7, 8, 9, 14, 16)
BD_NCLS = [(f"nc{n}", 3, (7, 13), n, "coarse", n % 2 == 0, n % 3 == 0) for n in NC_SWITCH]
BD_PIXELS = [
    ("px1", 1, (1, 1), 9, "coarse", False, False),
    ("px255", 3, (5, 17), 9, "coarse", True, False),
    ("px257", 1, (1, 257), 9, "coarse", False, True),
    ("px524289", 3, (1, 174763), 2, "coarse", False, False),     # one past 4 * 512 * 256: the backward's second trip has one live thread
]
# The labels are coarse_labels (random cells of 3 pixels), not blob_labels, on the small rows: at 7 x 13 the discs and rectangles
# draw over one another and classes vanish, which would leave most of a class count's terms zero.  One row has the organs.
BD_BLOBS = [("blobs", 2, (48, 56), 9, "blobs", False, True)]
BD_FAR = [("far", 2, (224, 224), 3, "far", True, False)]        # |phi| up to 315; wb given: the background, whose inside is the far part, counts
BD_CASES = BD_NCLS + BD_PIXELS + BD_BLOBS + BD_FAR


@functools.lru_cache(maxsize=None)
def bd_inputs(tag):
    """(x (B, ncls, HW) float32, labels (B, H, W) int64, phi (B, ncls, HW) float32 from the host definition, wb or None, cw or None)
    of a row of BD_CASES; computed once, never written."""
    from cswin_unet_amd.utils import signed_distance_maps_host
    _, B, (H, W), ncls, kind, has_wb, has_cw = next(c for c in BD_CASES if c[0] == tag)
    x = det_normal(f"boundary.{tag}.x", (B, ncls, H * W))
    lab = S.far_labels(B, H, W) if kind == "far" else S.blob_labels(B, H, W, ncls, 77) if kind == "blobs" else S.coarse_labels(B, H, W, ncls, 300 + ncls + H, cell=3 if H > 1 else 40)
    phi = signed_distance_maps_host(lab, ncls).reshape(B, ncls, H * W)
    wb = np.linspace(0.25, 2.0, ncls).astype(np.float32) if has_wb else None
    cw = np.linspace(2.0, 0.5, ncls).astype(np.float32) if has_cw else None
    return x, lab, phi, wb, cw


@pytest.mark.parametrize("tag", ["nc3", "nc9", "nc14", "px255"])
def test_bd_ref_agrees_with_autograd_and_explicit_loops(tag):
    x, lab, phi, wb, cw = bd_inputs(tag)
    B, ncls, HW = x.shape
    sums, bound = bd_ref(x, lab.reshape(B, HW), phi, wb)
    assert sums.shape == bound.shape == (2 + 3 * ncls,) and np.isfinite(bound).all() and bound[-1] > 0
    assert np.array_equal(sums[:-1], loss_ref(x, lab.reshape(B, HW))[0])
    xt = torch.from_numpy(x).double()
    assert abs(float(bd_graph(xt, phi, wb)) - sums[-1]) <= 1e-12 * np.abs(phi).sum()
    p = torch.softmax(xt, 1).numpy()
    w = default_wb(ncls) if wb is None else wb.astype(np.float64)
    loop = sum(w[c] * float((p[:, c] * phi[:, c].astype(np.float64)).sum()) for c in range(ncls))
    assert abs(loop - sums[-1]) <= 1e-12 * np.abs(phi).sum()
    # the closed-form gradient of the issue against autograd: p_c (T_c - sum_j p_j T_j), T = wb * phi
    xl = D(x)
    bd_graph(xl, phi, wb).backward()
    T = w[None, :, None] * phi.astype(np.float64)
    closed = p * (T - (p * T).sum(1, keepdims=True))
    assert float(np.abs(closed - xl.grad.numpy()).max()) <= 1e-12 * max(1.0, float(np.abs(phi).max()))
    out, bout, _ = bd_final_ref(sums, B * HW, 0.4, 0.6, 0.25, cw, bound)
    base, _, _ = final_ref(sums[:-1], B * HW, 0.4, 0.6, cw)
    assert abs(out[0] - (base[0] + 0.25 * sums[-1] / (B * HW))) <= 1e-15 and out[3] == sums[-1] / (B * HW) and (bout > 0).all()
    zero, bzero, _ = bd_final_ref(sums, B * HW, 0.4, 0.6, 0.0, cw, bound)
    assert zero[0] == base[0] and np.array_equal(bzero[:3], final_ref(sums[:-1], B * HW, 0.4, 0.6, cw, bound[:-1])[1])


def test_bound_of_the_boundary_sum_is_a_few_dozen_roundings():
    for tag in [c[0] for c in BD_CASES if c[0] != "px524289"]:
        x, lab, phi, wb, _ = bd_inputs(tag)
        B, ncls, HW = x.shape
        w = default_wb(ncls) if wb is None else wb.astype(np.float64)
        p = torch.softmax(torch.from_numpy(x).double(), 1).numpy()
        mass = np.abs(w[None, :, None] * p * phi).sum()
        _, bound = bd_ref(x, lab.reshape(B, HW), phi, wb)
        if mass > 0:
            assert 10 <= bound[-1] / (U * mass) <= 200, (tag, bound[-1] / (U * mass))
        else:
            assert bound[-1] == 0


BD_BUGS = [("drop_class", ("nc2", "nc9", "nc16", "blobs")), ("sign_in_mask", ("nc3", "nc9", "blobs", "far")),
           ("no_minus_one", ("nc3", "nc9", "px255", "blobs", "far"))]


@pytest.mark.parametrize("bug,tags", BD_BUGS, ids=[b[0] for b in BD_BUGS])
def test_boundary_bound_sees_the_bugs_these_shapes_are_for(bug, tags):
    """Each planted bug -- a dropped class, a sign flip inside the mask, -d in place of -(d - 1) -- moves the boundary sum by at
    least four times its bound at each row meant to catch it."""
    for tag in tags:
        x, lab, phi, wb, _ = bd_inputs(tag)
        B, ncls, HW = x.shape
        ref, bound = bd_ref(x, lab.reshape(B, HW), phi, wb)
        bad, _ = bd_ref(x, lab.reshape(B, HW), phi, wb, _wrong=bug)
        ratio = abs(bad[-1] - ref[-1]) / bound[-1]
        print(f"{tag} {bug}: moved {abs(bad[-1] - ref[-1]):.3e}, bound {bound[-1]:.3e}, ratio {ratio:.3g}")
        assert ratio >= 4.0, (tag, bug, ratio)
        assert np.array_equal(bad[:-1], ref[:-1])


def test_boundary_case_table_reaches_every_class_count_and_clamp():
    assert [c[3] for c in BD_NCLS] == list(NC_SWITCH) and all(c[1] == 3 and c[2] == (7, 13) for c in BD_NCLS)
    px = {c[1] * c[2][0] * c[2][1] for c in BD_PIXELS}
    assert px == {1, 255, 257, 4 * 512 * 256 + 1}
    assert loss_blocks(4 * 512 * 256 + 1) * 4 * 256 == 4 * 512 * 256                   # the backward grid, full: one pixel takes a second trip
    assert {c[5] for c in BD_CASES} == {False, True} and {c[6] for c in BD_CASES} == {False, True}
    x, lab, phi, _, _ = bd_inputs("far")
    assert float(np.abs(phi).max()) > 300
    for tag in ("nc3", "nc9"):
        assert float(bd_inputs(tag)[2].min()) <= -1.0                                 # inside distances past the boundary pixel
