"""The boundary objective's three kernels (csrc/bd_loss.hip) against their float64 restatement (tests/test_sdm_host.py: bd_ref,
bd_final_ref, bd_grad_ref), called directly with guarded buffers: every class count of the switch, the pixel counts round the
grid clamps, distance maps from the host definition with |phi| up to 315; every sum within its own bound, the four outputs within
the bounds that follow, the gradient by the suite's measure.  With alpha = 0 everything the base loss has is held to the base
loss's bounds.  Then the weights, grad_out, out-of-range labels, two emulated ranks, and ops.boundary_loss against the direct
calls and with cached maps."""
import numpy as np
import pytest
import torch

from oracle.determ import det_normal

import sdm_cases as S
from test_gpu_parity import RTOL
from test_gpu_shapes import D, measure
from test_gpu_attn_shapes import Guarded, settle
from test_gpu_step_tail import OOR_LABELS, U, close, dice_terms, final_ref, grad_ref, hip, loss_graph, loss_ref, put, release_inputs  # noqa: F401 (fixtures)
from test_sdm_host import BD_CASES, bd_final_ref, bd_grad_ref, bd_graph, bd_inputs, bd_ref

gpu = pytest.mark.gpu
DEV = "cuda"
ERR_SHAPE, ERR_WORKSPACE, ERR_UNSUPPORTED = -1, -3, -5
f32 = lambda v: float(np.float32(v))                     # a weight as the device float holds it


def run_bd(hip, x, lab, phi, wb=None, cw=None, alpha=0.01, w_ce=0.4, w_dice=0.6, n_pixels=None, ce_scale=None, dice_scale=None, bd_scale=None,
           gout=None, sums_in=None, what="", nan_ok=False):
    """sums -> finalize -> bwd on guarded buffers; returns numpy sums, out4, coef and the dlogits tensor (CPU).  sums_in: finalize
    and bwd run on these sums instead of the local ones (an emulated all-reduce)."""
    B, ncls, HW = x.shape
    xd, ld, pd = put(x), put(np.ascontiguousarray(lab).reshape(B, HW)), put(phi)
    wbd, cwd = (None if w is None else put(np.asarray(w, np.float32)) for w in (wb, cw))
    ad = put(np.array([alpha], np.float32))
    nbytes = hip.lib().cswin_bd_loss_workspace(B, ncls, HW)
    assert nbytes % 4 == 0
    o = dict(sums=Guarded((2 + 3 * ncls,)), workspace=Guarded((nbytes // 4,)), out4=Guarded((4,)), coef=Guarded((2 * ncls,)), dlogits=Guarded((B, ncls, HW)))
    hip.call("cswin_bd_loss_sums", hip.ptr(xd), hip.ptr(ld), hip.ptr(pd), hip.ptr(wbd), hip.ptr(o["sums"].t), hip.ptr(o["workspace"].t), nbytes, B, ncls, HW,
             hip.stream())
    sums = o["sums"].t.cpu().numpy().copy()
    fin = o["sums"].t if sums_in is None else put(np.asarray(sums_in, np.float32))
    hip.call("cswin_bd_loss_finalize", hip.ptr(fin), hip.ptr(o["out4"].t), hip.ptr(o["coef"].t), float(B * HW if n_pixels is None else n_pixels), ncls,
             w_ce, w_dice, hip.ptr(ad), hip.ptr(cwd), hip.stream())
    gd = None if gout is None else put(np.array([gout], np.float32))
    hip.call("cswin_bd_loss_bwd", hip.ptr(xd), hip.ptr(ld), hip.ptr(pd), hip.ptr(wbd), hip.ptr(o["coef"].t), hip.ptr(ad), hip.ptr(gd), hip.ptr(o["dlogits"].t),
             w_ce / (B * HW) if ce_scale is None else ce_scale, w_dice / ncls if dice_scale is None else dice_scale,
             1.0 / (B * HW) if bd_scale is None else bd_scale, B, ncls, HW, hip.stream())
    if nan_ok:                                                       # a poisoned CE sum: the guards hold, the NaN is the result
        torch.cuda.synchronize()
        assert all(g.intact() for g in o.values())
    else:
        settle(what, o)
    return sums, o["out4"].t.cpu().numpy().copy(), o["coef"].t.cpu().numpy().copy(), o["dlogits"].t.cpu()


@gpu
@pytest.mark.parametrize("case", BD_CASES, ids=[c[0] for c in BD_CASES])
def test_every_sum_output_and_gradient_vs_float64(hip, case):
    tag, B, (H, W), ncls, kind, has_wb, has_cw = case
    x, lab, phi, wb, cw = bd_inputs(tag)
    lab2, n, alpha = lab.reshape(B, H * W), B * H * W, f32(0.3)
    sums, out4, coef, dl = run_bd(hip, x, lab, phi, wb, cw, alpha, what=f"boundary.{tag}")
    ref, bound = bd_ref(x, lab2, phi, wb)
    close(sums, ref, bound, f"boundary.{tag}.sums")
    want, bwant, cref = bd_final_ref(ref, n, 0.4, 0.6, alpha, cw, bound)
    close(out4, want, bwant, f"boundary.{tag}.out4")
    assert measure(dl, bd_grad_ref(x, lab2, phi, wb, 0.4 / n, 0.6 / ncls, alpha / n, 1.0, cw), f"boundary.{tag}.dlogits") <= RTOL


@gpu
@pytest.mark.parametrize("tag", ["nc2", "nc9", "nc16", "px257", "far"])
def test_alpha_zero_is_the_base_loss_within_the_base_bounds(hip, tag):
    """The first 1 + 3*ncls sums, loss / ce / dice and the gradient against loss_ref / final_ref / grad_ref alone."""
    x, lab, phi, wb, cw = bd_inputs(tag)
    B, ncls, HW = x.shape
    lab2 = lab.reshape(B, HW)
    sums, out4, _, dl = run_bd(hip, x, lab, phi, wb, cw, 0.0, what=f"boundary.zero.{tag}")
    ref, bound = loss_ref(x, lab2)
    close(sums[:-1], ref, bound, f"boundary.zero.{tag}.sums")
    want, bwant, _ = final_ref(ref, B * HW, 0.4, 0.6, cw, bound)
    close(out4[:3], want, bwant, f"boundary.zero.{tag}.out3")
    assert measure(dl, grad_ref(x, lab2, False, 0.4 / (B * HW), 0.6 / ncls, 1.0, cw), f"boundary.zero.{tag}.dlogits") <= RTOL


@gpu
def test_weights_scales_and_grad_out(hip):
    """wb and the Dice class weights given and null in every combination; grad_out null and 1.7; the three scales chosen
    independently of the loss weights, the boundary term alone included."""
    x, lab, phi, _, _ = bd_inputs("nc7")
    B, ncls, HW = x.shape
    lab2, n = lab.reshape(B, HW), B * HW
    wbs = (None, np.array([0.5, 0.0, 2.0, 1.0, 0.25, 3.0, 1.5], np.float32))
    cws = (None, np.array([1.0, 0.5, 2.0, 0.25, 1.5, 0.0, 3.0], np.float32))
    for wb in wbs:
        for cw in cws:
            for gout, ce_scale, dice_scale, bd_scale, alpha in ((None, 0.4 / n, 0.6 / ncls, 1.0 / n, f32(0.01)), (1.7, 0.4 / n, 0.6 / ncls, 1.0 / n, f32(0.5)),
                                                                (1.7, 0.0, 0.0, 2.5e-3, f32(1.0)), (None, 3.0e-3, 0.37, 0.5 / n, f32(0.07))):
                what = f"boundary.bwd.wb{wb is not None}.cw{cw is not None}.g{gout}.a{alpha:.2f}.s{bd_scale:.1e}"
                sums, out4, _, dl = run_bd(hip, x, lab, phi, wb, cw, alpha, ce_scale=ce_scale, dice_scale=dice_scale, bd_scale=bd_scale, gout=gout, what=what)
                ref, bound = bd_ref(x, lab2, phi, wb)
                close(sums, ref, bound, what + ".sums")
                want, bwant, _ = bd_final_ref(ref, n, 0.4, 0.6, alpha, cw, bound)
                close(out4, want, bwant, what + ".out4")
                g = bd_grad_ref(x, lab2, phi, wb, ce_scale, dice_scale, alpha * bd_scale, 1.0 if gout is None else gout, cw)
                assert measure(dl, g, what + ".dlogits") <= RTOL


@gpu
@pytest.mark.parametrize("bad", OOR_LABELS, ids=[str(b) for b in OOR_LABELS])
def test_out_of_range_labels(hip, bad):
    """CE is NaN, the boundary sum is finite and within its bound -- the pixel is outside every mask, in phi as in the loss --,
    and with w_ce = 0 the loss and the gradient are those of the restatement."""
    from cswin_unet_amd.utils import signed_distance_maps_host
    ncls = 6
    x, lab, _, _, _ = bd_inputs("nc6")
    B, _, HW = x.shape
    lab = np.array(lab)
    lab[0, 2, 4] = lab[2, 6, 12] = ncls if bad == "ncls" else bad
    phi = signed_distance_maps_host(lab, ncls).reshape(B, ncls, HW)
    lab2, alpha = lab.reshape(B, HW), f32(0.2)
    sums, out4, _, _ = run_bd(hip, x, lab, phi, alpha=alpha, what=f"boundary.oor{bad}.ce", nan_ok=True)
    ref, bound = bd_ref(x, lab2, phi)
    assert np.isnan(ref[0]) and np.isnan(sums[0]) and np.isnan(out4[0]) and np.isnan(out4[1]), (sums[0], out4)
    close(sums[1:], ref[1:], bound[1:], f"boundary.oor{bad}.sums")
    assert np.isfinite(sums[-1]) and np.isfinite(out4[3])
    sums, out4, _, dl = run_bd(hip, x, lab, phi, alpha=alpha, w_ce=0.0, w_dice=1.0, what=f"boundary.oor{bad}.dice", nan_ok=True)
    want, bwant, _ = bd_final_ref(ref, B * HW, 0.0, 1.0, alpha, None, bound)
    close(out4[[0, 2, 3]], want[[0, 2, 3]], bwant[[0, 2, 3]], f"boundary.oor{bad}.out4")
    assert not torch.isnan(dl).any()
    assert measure(dl, bd_grad_ref(x, lab2, phi, None, 0.0, 1.0 / ncls, alpha / (B * HW)), f"boundary.oor{bad}.dlogits") <= RTOL


@gpu
def test_two_ranks_emulated_on_one_device(hip):
    """The data-parallel contract without a process group: the halves' sums added, finalize on the global pixel count, the
    backward per half with dice_scale = w_dice / ncls * 2 and the LOCAL counts in ce_scale and bd_scale; half of each local
    gradient is the float64 gradient of the global-batch loss for that half."""
    from cswin_unet_amd.utils import signed_distance_maps_host
    ncls, B, (H, W), w_ce, w_dice, alpha = 4, 4, (7, 13), 0.4, 0.6, f32(0.3)
    HW = H * W
    x, lab = det_normal("boundary.ranks.x", (B, ncls, HW)), S.coarse_labels(B, H, W, ncls, 91, cell=3)
    phi, lab2 = signed_distance_maps_host(lab, ncls).reshape(B, ncls, HW), lab.reshape(B, HW)
    halves = [(x[:2], lab[:2], phi[:2]), (x[2:], lab[2:], phi[2:])]
    local = [run_bd(hip, xh, lh, ph, alpha=alpha, what=f"boundary.ranks.sums{r}")[0] for r, (xh, lh, ph) in enumerate(halves)]
    total = (local[0] + local[1]).astype(np.float32)
    ref, _ = bd_ref(x, lab2, phi)
    b2 = sum(bd_ref(xh, lh.reshape(2, HW), ph)[1] for xh, lh, ph in halves) + U * np.abs(ref)
    close(total, ref, b2, "boundary.ranks.sums")
    xl = D(x)
    nll, I, Y, Z = loss_graph(xl, lab2)
    (w_ce * nll / (B * HW) + w_dice * dice_terms(I, Y, Z) / ncls + alpha * bd_graph(xl, phi) / (B * HW)).backward()
    for r, (xh, lh, ph) in enumerate(halves):
        _, out4, _, dl = run_bd(hip, xh, lh, ph, alpha=alpha, n_pixels=B * HW, ce_scale=w_ce / (2 * HW), dice_scale=w_dice / ncls * 2, bd_scale=1.0 / (2 * HW),
                                sums_in=total, what=f"boundary.ranks.bwd{r}")
        want, bwant, _ = bd_final_ref(ref, B * HW, w_ce, w_dice, alpha, None, b2)
        close(out4, want, bwant, f"boundary.ranks.out4.{r}")
        assert measure(0.5 * dl, xl.grad[2 * r:2 * r + 2], f"boundary.ranks.dlogits{r}") <= RTOL


@gpu
def test_workspace_is_exact_and_refusals_touch_nothing(hip):
    x, lab, phi, _, _ = bd_inputs("px257")
    B, ncls, HW = x.shape
    xd, ld, pd, ad = put(x), put(lab.reshape(B, HW)), put(phi), put(np.array([0.1], np.float32))
    nbytes = hip.lib().cswin_bd_loss_workspace(B, ncls, HW)
    assert nbytes == 2 * (2 + 3 * ncls) * 4                          # two workgroups' partial sums
    o = dict(sums=Guarded((2 + 3 * ncls,)), workspace=Guarded((nbytes // 4,)), out4=Guarded((4,)), coef=Guarded((2 * ncls,)), dlogits=Guarded((B, 17, HW)))
    sums_args = lambda n, nb, **kw: (hip.ptr(kw.get("x", xd)), hip.ptr(kw.get("lab", ld)), hip.ptr(kw.get("phi", pd)), None, hip.ptr(o["sums"].t), hip.ptr(o["workspace"].t),
                                     nb, B, n, HW, hip.stream())
    hip.refused(ERR_WORKSPACE, "bd_loss_sums one byte short", o, "cswin_bd_loss_sums", *sums_args(ncls, nbytes - 1))
    hip.refused(ERR_SHAPE, "bd_loss_sums null phi", o, "cswin_bd_loss_sums", hip.ptr(xd), hip.ptr(ld), None, None, hip.ptr(o["sums"].t), hip.ptr(o["workspace"].t), nbytes,
                B, ncls, HW, hip.stream())
    coef = put(np.ones(2 * 17, np.float32))
    hip.refused(ERR_SHAPE, "bd_loss_finalize null alpha", o, "cswin_bd_loss_finalize", hip.ptr(coef), hip.ptr(o["out4"].t), hip.ptr(o["coef"].t), float(HW), ncls, 0.4, 0.6,
                None, None, hip.stream())
    hip.refused(ERR_SHAPE, "bd_loss_bwd null alpha", o, "cswin_bd_loss_bwd", hip.ptr(xd), hip.ptr(ld), hip.ptr(pd), None, hip.ptr(coef), None, None, hip.ptr(o["dlogits"].t),
                1.0, 1.0, 1.0, B, ncls, HW, hip.stream())
    for n in (1, 10, 17):
        big = put(np.zeros((B, n, HW), np.float32))
        ws = Guarded((hip.lib().cswin_bd_loss_workspace(B, n, HW) // 4,))
        oo = dict(sums=Guarded((2 + 3 * n,)), workspace=ws, dlogits=Guarded((B, n, HW)))
        hip.refused(ERR_UNSUPPORTED, f"bd_loss_sums ncls={n}", oo, "cswin_bd_loss_sums", hip.ptr(big), hip.ptr(ld), hip.ptr(big), None, hip.ptr(oo["sums"].t), hip.ptr(ws.t),
                    ws.n * 4, B, n, HW, hip.stream())
        hip.refused(ERR_UNSUPPORTED, f"bd_loss_bwd ncls={n}", oo, "cswin_bd_loss_bwd", hip.ptr(big), hip.ptr(ld), hip.ptr(big), None, hip.ptr(coef), hip.ptr(ad), None,
                    hip.ptr(oo["dlogits"].t), 1.0, 1.0, 1.0, B, n, HW, hip.stream())


def _ops_inputs(tag):
    x, lab, phi, wb, cw = bd_inputs(tag)
    _, B, (H, W), ncls = next(c for c in BD_CASES if c[0] == tag)[:4]
    dev = lambda a: None if a is None else torch.from_numpy(np.array(a)).to(DEV)
    return x, lab, phi, wb, cw, dev(x.reshape(B, ncls, H, W)), dev(lab), dev(wb), dev(cw)


@gpu
@pytest.mark.parametrize("tag", ["nc4", "nc9", "px255"])
def test_ops_boundary_loss_equals_the_direct_calls(hip, tag):
    """ops.boundary_loss -- maps made on the device -- against the three entry points given the host definition's maps: the same
    bits in stats and gradient; the loss it returns is stats[0]; grad_out reaches the kernel."""
    from cswin_unet_amd import ops
    x, lab, phi, wb, cw, xd, ld, wbd, cwd = _ops_inputs(tag)
    alpha = f32(0.3)
    sums, out4, _, dl = run_bd(hip, x, lab, phi, wb, cw, alpha, gout=1.7, what=f"boundary.ops.{tag}")
    xg = xd.clone().requires_grad_(True)
    loss, stats = ops.boundary_loss(xg, ld, alpha, class_weight=cwd, boundary_class_weight=wbd)
    (1.7 * loss).backward()
    assert stats.shape == (4,) and not stats.requires_grad and float(loss.detach()) == float(stats[0])
    assert np.array_equal(stats.cpu().numpy().view(np.uint32), out4.view(np.uint32))
    assert np.array_equal(xg.grad.cpu().numpy().reshape(x.shape).view(np.uint32), dl.numpy().view(np.uint32))


@gpu
def test_ops_boundary_loss_with_cached_maps_is_bit_equal(hip):
    from cswin_unet_amd import ops
    x, lab, phi, wb, cw, xd, ld, wbd, cwd = _ops_inputs("nc9")
    maps = ops.signed_distance_maps(ld, 9)
    assert np.array_equal(maps.cpu().numpy().reshape(phi.shape), phi)
    res = []
    for kw in (dict(), dict(dist_maps=maps)):
        xg = xd.clone().requires_grad_(True)
        loss, stats = ops.boundary_loss(xg, ld, 0.25, w_ce=0.3, w_dice=0.7, **kw)
        loss.backward()
        res.append((stats.cpu().numpy().view(np.uint32), xg.grad.cpu().numpy().view(np.uint32)))
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
    # cached maps carry the labels in any shape the loss kernels take
    xg = xd.clone().requires_grad_(True)
    loss, stats = ops.boundary_loss(xg, ld.reshape(ld.shape[0], -1), 0.25, w_ce=0.3, w_dice=0.7, dist_maps=maps)
    assert np.array_equal(stats.cpu().numpy().view(np.uint32), res[0][0])


@gpu
def test_ops_boundary_loss_argument_checks():
    from cswin_unet_amd import ops
    x, lab, phi, wb, cw, xd, ld, wbd, cwd = _ops_inputs("nc4")
    with pytest.raises(ValueError, match="labels"):
        ops.boundary_loss(xd, ld[:2], 0.1)
    with pytest.raises(ValueError, match="labels"):
        ops.boundary_loss(xd, ld.cpu(), 0.1)
    with pytest.raises(ValueError, match="distance maps"):
        ops.boundary_loss(xd, ld.reshape(3, -1), 0.1)
    with pytest.raises(ValueError, match="dist_maps"):
        ops.boundary_loss(xd, ld, 0.1, dist_maps=torch.zeros(3, 4, 7, 12, device=DEV))
    with pytest.raises(ValueError, match="boundary_class_weight"):
        ops.boundary_loss(xd, ld, 0.1, boundary_class_weight=torch.ones(5, device=DEV))
    with pytest.raises(ValueError, match="class_weight"):
        ops.boundary_loss(xd, ld, 0.1, class_weight=torch.ones(3, device=DEV))
