"""cswin_cl_loss_sums / _finalize / _bwd (csrc/cl_loss.hip) at every class count, on both sides of every launch branch and on inputs
built to break the arithmetic, against the float64 restatement of test_continual_host (cl_torch / cl_ref) -- called directly
through cswin_unet_amd._lib with guarded buffers and an exact workspace, as test_gpu_step_tail calls the base loss.

Sums and the five outputs are held to the bounds cl_ref / cl_final_ref derive in float64 from the magnitudes summed; gradients to
the suite's measure max|got - ref| / rms(ref) <= RTOL."""
import functools

import numpy as np
import pytest
import torch

from oracle.determ import det_labels, det_normal

from test_gpu_parity import RTOL
from test_gpu_shapes import measure
from test_gpu_attn_shapes import Guarded, settle
from test_gpu_step_tail import (ERR_SHAPE, ERR_UNSUPPORTED, ERR_WORKSPACE, U, close, final_ref, grad_ref, hip, loss_ref, put,  # noqa: F401
                                release_inputs)
from test_continual_host import CL_CASES, CL_NCLS, case_of, cl_final_ref, cl_grad_ref, cl_inputs, cl_ref, map_labels

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def ref_of(tag):
    """(sums, bound) of a row of CL_CASES in float64; computed once, never written."""
    x, lab, t, cw, lmap = cl_inputs(tag)
    o = case_of(tag)[6]
    return cl_ref(x, lab, t, o["T"], o["alpha"], o["gamma"], cw, lmap)


def run_cl(hip, x, lab, t, cw=None, lmap=None, T=3.0, alpha=1.0, gamma=4.0, w_focal=0.2, w_dice=0.8, kd_weight=0.5, n_pixels=None, batch=None,
           scales=None, gout=None, sums_in=None, what="", nan_ok=False):
    """sums -> finalize -> bwd on guarded buffers; returns numpy sums, out5, coef and the dlogits tensor (CPU).  scales: the three
    of cswin_cl_loss_bwd (default: what ops.continual_loss passes for one rank); sums_in: finalize and bwd run on these sums."""
    B, ncls, HW = x.shape
    nold = 0 if t is None else t.shape[1]
    xd, ld = put(x), put(np.asarray(lab, np.int64))
    td = None if t is None else put(t)
    cwd = None if cw is None else put(np.asarray(cw, np.float32))
    md = None if lmap is None else put(np.asarray(lmap, np.int32))
    n_map = 0 if lmap is None else len(lmap)
    nbytes = hip.lib().cswin_cl_loss_workspace(B, ncls, HW)
    assert nbytes % 4 == 0
    o = dict(sums=Guarded((3 + 3 * ncls,)), workspace=Guarded((nbytes // 4,)), out5=Guarded((5,)), coef=Guarded((2 * ncls,)), dlogits=Guarded((B, ncls, HW)))
    hip.call("cswin_cl_loss_sums", hip.ptr(xd), hip.ptr(ld), hip.ptr(md), n_map, hip.ptr(td), hip.ptr(cwd), hip.ptr(o["sums"].t), hip.ptr(o["workspace"].t),
             nbytes, B, ncls, nold, HW, T, alpha, gamma, hip.stream())
    sums = o["sums"].t.cpu().numpy().copy()
    fin = o["sums"].t if sums_in is None else put(np.asarray(sums_in, np.float32))
    n = B * HW if n_pixels is None else n_pixels
    hip.call("cswin_cl_loss_finalize", hip.ptr(fin), hip.ptr(o["out5"].t), hip.ptr(o["coef"].t), float(n), float(B if batch is None else batch), ncls,
             w_focal, w_dice, kd_weight, T, hip.stream())
    if scales is None:
        scales = ((1 - kd_weight) * w_focal / (B * HW), (1 - kd_weight) * w_dice / ncls, kd_weight * T / B)
    gd = None if gout is None else put(np.array([gout], np.float32))
    hip.call("cswin_cl_loss_bwd", hip.ptr(xd), hip.ptr(ld), hip.ptr(md), n_map, hip.ptr(td), hip.ptr(cwd), hip.ptr(o["coef"].t), hip.ptr(gd),
             hip.ptr(o["dlogits"].t), scales[0], scales[1], scales[2], B, ncls, nold, HW, T, alpha, gamma, hip.stream())
    if nan_ok:
        torch.cuda.synchronize()
        assert all(g.intact() for g in o.values())
    else:
        settle(what, o)
    return sums, o["out5"].t.cpu().numpy().copy(), o["coef"].t.cpu().numpy().copy(), o["dlogits"].t.cpu()


@pytest.mark.parametrize("case", CL_CASES, ids=[c[0] for c in CL_CASES])
def test_every_sum_output_and_gradient_vs_float64(hip, case):
    """Every entry of sums within its own bound, the five outputs within the bounds that follow, the gradient by the suite's
    measure: every class count with nold cycling through 1, 2, ncls - 1, ncls; 1, 255, 257, 133 563 and 526 338 pixels; confident
    pixels (ce ~ 3e-7, gamma 4), logit gaps past 87.4 T at T = 3 and T = 1, an offset of 1e4, a class of weight 0, an absent class,
    gamma 0 / 1 / 2 / 4 with alpha 0.75, class weights and the label map given and not."""
    tag, B, (H, W), ncls, nold, kind, o = case
    x, lab, t, cw, lmap = cl_inputs(tag)
    T, alpha, gamma = o["T"], o["alpha"], o["gamma"]
    sums, out5, coef, dl = run_cl(hip, x, lab, t, cw, lmap, T, alpha, gamma, what=f"cl.{tag}")
    ref, bound = ref_of(tag)
    close(sums, ref, bound, f"cl.{tag}.sums")
    want, bwant, cref = cl_final_ref(ref, B * H * W, B, 0.2, 0.8, 0.5, T, bsums=bound)
    close(out5, want, bwant, f"cl.{tag}.out5")
    n = B * H * W
    g = cl_grad_ref(x, lab, t, 0.5 * 0.2 / n, 0.5 * 0.8 / ncls, 0.5 * T / B, 1.0, T, alpha, gamma, cw, lmap)
    assert measure(dl, g, f"cl.{tag}.dlogits") <= RTOL


def test_case_table_holds_what_the_kernel_branches_on():
    assert sorted({c[3] for c in CL_NCLS}) == list(range(2, 17))
    assert {(c[3], c[4]) for c in CL_NCLS} >= {(12, 9), (14, 12)}
    for n in range(2, 17):
        assert {c[4] for c in CL_NCLS if c[3] == n} - {9 if n == 12 else 12 if n == 14 else 1} <= {1, 2, n - 1, n}     # and the two stage totals
    kinds = {(1 if c[4] == 1 else 2 if c[4] == 2 else "n-1" if c[4] == c[3] - 1 else "n") for c in CL_NCLS}
    assert kinds >= {1, 2, "n-1", "n"}
    px = {c[1] * c[2][0] * c[2][1] for c in CL_CASES}
    assert {1, 255, 257, 133563, 526338} <= px and 133563 > 512 * 256 and 526338 > 4 * 512 * 256
    assert all((c[2][0] * c[2][1]) % 2 == 1 and (c[1] == 1 or (c[2][0] * c[2][1]) % c[1]) for c in CL_CASES)
    assert {c[6]["gamma"] for c in CL_CASES} >= {0.0, 1.0, 2.0, 4.0} and {c[6]["T"] for c in CL_CASES} >= {1.0, 3.0}
    assert {(c[6]["cw"], c[6]["lmap"]) for c in CL_CASES} == {(False, False), (False, True), (True, False), (True, True)}


# ---- reductions to the base loss ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["nc12.old9", "nc9.old2", "px257.nc2"])
def test_gamma0_without_weights_and_kd_is_the_base_loss(hip, tag):
    """gamma = 0, no weights, kd_weight = 0, w_focal = 0.4, w_dice = 0.6: loss and dlogits are the float64 base loss's within the
    base test's bounds, and the first 1 + 3*ncls sums are within the bounds the base kernel is held to."""
    x, lab, t, _, lmap = cl_inputs(tag)
    lab = map_labels(lab, lmap)
    B, ncls, HW = x.shape
    sums, out5, _, dl = run_cl(hip, x, lab, t, None, None, 3.0, 1.0, 0.0, w_focal=0.4, w_dice=0.6, kd_weight=0.0, what=f"cl.base.{tag}")
    ref, bound = loss_ref(x, lab)
    close(sums[:1 + 3 * ncls], ref, bound, f"cl.base.{tag}.sums")
    close(sums[1 + 3 * ncls:2 + 3 * ncls], ref[:1], bound[:1], f"cl.base.{tag}.focal_sum")
    want, bwant, _ = final_ref(ref, B * HW, 0.4, 0.6, bsums=bound)
    close(out5[[0, 4, 2]], want, bwant, f"cl.base.{tag}.out")
    assert measure(dl, grad_ref(x, lab, False, 0.4 / (B * HW), 0.6 / ncls), f"cl.base.{tag}.dlogits") <= RTOL


@pytest.mark.parametrize("tag", ["nc12.old9", "nc14.old12", "nc7.old7", "offset1e4"])
def test_teacher_equal_to_the_student_has_no_kd(hip, tag):
    """teacher == logits[:, :nold]: the KD sum is below its bound and the KD gradient is 0 within RTOL of the focal + Dice
    gradient's rms."""
    x, lab, _, cw, lmap = cl_inputs(tag)
    o = case_of(tag)[6]
    B, ncls, HW = x.shape
    nold = case_of(tag)[4]
    t = np.ascontiguousarray(x[:, :nold])
    T, alpha, gamma = o["T"], o["alpha"], o["gamma"]
    ref, bound = cl_ref(x, lab, t, T, alpha, gamma, cw, lmap)
    assert abs(ref[-1]) <= 1e-9
    sums, out5, _, dl = run_cl(hip, x, lab, t, cw, lmap, T, alpha, gamma, scales=(0.0, 0.0, 0.5 * T / B), what=f"cl.same.{tag}")
    close(sums, ref, bound, f"cl.same.{tag}.sums")
    print(f"cl.same.{tag}: kd sum {sums[-1]:.3e} bound {bound[-1]:.3e}; max |kd gradient| {float(dl.abs().max()):.3e}")
    g = cl_grad_ref(x, lab, t, 0.5 * 0.2 / (B * HW), 0.5 * 0.8 / ncls, 0.0, 1.0, T, alpha, gamma, cw, lmap)
    assert float(dl.abs().max()) <= RTOL * float(g.pow(2).mean().sqrt())


# ---- scales and grad_out --------------------------------------------------------------------------------------------------------
def test_bwd_scales_and_grad_out(hip):
    """grad_out NULL and 1.7; each of the three scales 0 in turn silences exactly its term (the reference drops the same term)."""
    tag = "nc12.old9"
    x, lab, t, cw, lmap = cl_inputs(tag)
    full = (3.0e-3, 0.37, 0.41)
    for gout in (None, 1.7):
        for off in (None, 0, 1, 2):
            sc = tuple(0.0 if k == off else v for k, v in enumerate(full))
            what = f"cl.bwd.g{gout}.off{off}"
            _, _, _, dl = run_cl(hip, x, lab, t, cw, lmap, scales=sc, gout=gout, what=what)
            ref = cl_grad_ref(x, lab, t, sc[0], sc[1], sc[2], 1.0 if gout is None else gout, cw=cw, lmap=lmap)
            assert measure(dl, ref, what) <= RTOL
            if off == 2:
                assert float(dl[:, 9:].abs().max()) > 0 and measure(dl[:, :9], ref[:, :9], what + ".old") <= RTOL
    _, _, _, dl = run_cl(hip, x, lab, t, cw, lmap, scales=(0.0, 0.0, 0.0), gout=1.7, what="cl.bwd.allzero")
    assert float(dl.abs().max()) == 0.0
    _, _, _, dl = run_cl(hip, x, lab, t, cw, lmap, scales=(0.0, 0.0, 0.41), what="cl.bwd.kdonly")
    assert float(dl[:, 9:].abs().max()) == 0.0 and float(dl[:, :9].abs().max()) > 0


def test_finalize_forms(hip):
    """Global pixel and image counts other than the local ones, other weights, and weights of 0 against poisoned sums."""
    tag = "nc12.old9"
    x, lab, t, cw, lmap = cl_inputs(tag)
    ref, bound = ref_of(tag)
    s32 = ref.astype(np.float32)
    for what, n, batch, wf, wd, kw, T in (("plain", 273, 3, 0.2, 0.8, 0.5, 3.0), ("global", 4 * 273, 12, 0.3, 0.7, 0.25, 2.0), ("nokd", 273, 3, 0.2, 0.8, 0.0, 3.0),
                                          ("kdonly", 273, 3, 0.2, 0.8, 1.0, 3.0)):
        _, out5, coef, _ = run_cl(hip, x, lab, t, cw, lmap, T=T, w_focal=wf, w_dice=wd, kd_weight=kw, n_pixels=n, batch=batch, sums_in=s32, what=f"cl.fin.{what}")
        want, bwant, cref = cl_final_ref(s32, n, batch, wf, wd, kw, T)
        close(out5, want, bwant, f"cl.fin.{what}.out5")
        close(coef, cref, 8 * U * np.abs(cref), f"cl.fin.{what}.coef")
    bad = s32.copy()
    bad[0] = bad[-2] = np.nan
    _, out5, _, _ = run_cl(hip, x, lab, t, cw, lmap, w_focal=0.0, w_dice=0.8, sums_in=bad, what="cl.fin.poisoned", nan_ok=True)
    want, bwant, _ = cl_final_ref(s32, 273, 3, 0.0, 0.8, 0.5, 3.0)
    assert np.isnan(out5[1]) and np.isnan(out5[4]) and abs(out5[0] - want[0]) <= bwant[0]
    _, out5, _, _ = run_cl(hip, x, lab, t, cw, lmap, kd_weight=1.0, sums_in=bad, what="cl.fin.poisoned.kdonly", nan_ok=True)
    assert np.isfinite(out5[0]) and abs(out5[0] - out5[3]) <= 4 * U * abs(out5[3])
    bad = s32.copy()
    bad[-1] = np.nan
    _, out5, _, _ = run_cl(hip, x, lab, t, cw, lmap, kd_weight=0.0, sums_in=bad, what="cl.fin.poisoned.kd", nan_ok=True)
    assert np.isnan(out5[3]) and np.isfinite(out5[0])


# ---- labels that are no class ---------------------------------------------------------------------------------------------------
OOR = [("raw-1", -1, False), ("rawncls", "ncls", False), ("2pow32plus1", 2 ** 32 + 1, False), ("outside_map", 4, True), ("map2pow32plus1", 2 ** 32 + 1, True)]


@pytest.mark.parametrize("name,bad,mapped", OOR, ids=[o[0] for o in OOR])
def test_out_of_range_labels(hip, name, bad, mapped):
    """Raw -1, ncls and 2^32 + 1 (class 1 to a kernel that truncates first) and an index outside the label map: NaN in the focal, ce
    and loss outputs, finite dice and kd, no NaN in dlogits, which is the gradient of the restatement where such a pixel has no
    class and no focal term; with w_focal = 0 the loss is finite."""
    tag = "nc12.old9" if mapped else "nc10.old9"
    x, lab, t, cw, lmap = cl_inputs(tag)
    B, ncls, HW = x.shape
    T = 3.0
    lab = np.array(lab)
    lab[0, 17] = lab[2, 90] = ncls if bad == "ncls" else bad
    o = case_of(tag)[6]
    sums, out5, _, dl = run_cl(hip, x, lab, t, cw, lmap, T, o["alpha"], o["gamma"], what=f"cl.oor.{name}", nan_ok=True)
    ref, bound = cl_ref(x, lab, t, T, o["alpha"], o["gamma"], cw, lmap)
    live = np.r_[1:1 + 3 * ncls, 2 + 3 * ncls]
    assert np.isnan(ref[0]) and np.isnan(ref[-2]) and np.isnan(sums[0]) and np.isnan(sums[-2])
    close(sums[live], ref[live], bound[live], f"cl.oor.{name}.sums")
    assert np.isnan(out5[[0, 1, 4]]).all() and np.isfinite(out5[[2, 3]]).all(), out5
    want, bwant, _ = cl_final_ref(ref, B * HW, B, 0.0, 0.8, 0.5, T, bsums=bound)
    close(out5[[2, 3]], want[[2, 3]], bwant[[2, 3]], f"cl.oor.{name}.out")
    assert not torch.isnan(dl).any()
    g = cl_grad_ref(x, lab, t, 0.5 * 0.2 / (B * HW), 0.5 * 0.8 / ncls, 0.5 * T / B, 1.0, T, o["alpha"], o["gamma"], cw, lmap)
    assert measure(dl, g, f"cl.oor.{name}.dlogits") <= RTOL
    _, out5, _, _ = run_cl(hip, x, lab, t, cw, lmap, T, o["alpha"], o["gamma"], w_focal=0.0, what=f"cl.oor.{name}.nofocal", nan_ok=True)
    close(out5[[0]], want[[0]], bwant[[0]], f"cl.oor.{name}.loss")


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_touch_nothing(hip):
    x, lab, t, cw, lmap = cl_inputs("px257.nc12")
    B, ncls, HW = x.shape
    nold = t.shape[1]
    ld, td = put(np.asarray(lab, np.int64)), put(t)
    xbig = put(np.zeros((B, 17, HW), np.float32))
    nbytes = hip.lib().cswin_cl_loss_workspace(B, 17, HW)
    exact = hip.lib().cswin_cl_loss_workspace(B, ncls, HW)
    o = dict(sums=Guarded((3 + 3 * 17,)), workspace=Guarded((nbytes // 4,)), dlogits=Guarded((B, 17, HW)))
    coef = put(np.ones(2 * 17, np.float32))

    def sums_args(n=ncls, old=nold, T=3.0, gamma=4.0, nb=nbytes, teacher=td):
        return (hip.ptr(xbig), hip.ptr(ld), None, 0, hip.ptr(teacher), None, hip.ptr(o["sums"].t), hip.ptr(o["workspace"].t), nb, B, n, old, HW, T, 1.0, gamma, hip.stream())

    def bwd_args(n=ncls, old=nold, T=3.0, gamma=4.0, teacher=td):
        return (hip.ptr(xbig), hip.ptr(ld), None, 0, hip.ptr(teacher), None, hip.ptr(coef), None, hip.ptr(o["dlogits"].t), 1.0, 1.0, 1.0, B, n, old, HW, T, 1.0, gamma,
                hip.stream())

    for what, code, kw in (("ncls=1", ERR_UNSUPPORTED, dict(n=1, old=1)), ("ncls=17", ERR_UNSUPPORTED, dict(n=17)), ("nold>ncls", ERR_SHAPE, dict(old=ncls + 1)),
                           ("nold<0", ERR_SHAPE, dict(old=-1)), ("gamma=0.5", ERR_UNSUPPORTED, dict(gamma=0.5)), ("gamma<0", ERR_UNSUPPORTED, dict(gamma=-1.0)),
                           ("T=0", ERR_UNSUPPORTED, dict(T=0.0)), ("T<0", ERR_UNSUPPORTED, dict(T=-3.0)), ("null teacher", ERR_SHAPE, dict(teacher=None))):
        hip.refused(code, f"cl_loss_sums {what}", o, "cswin_cl_loss_sums", *sums_args(**kw))
        hip.refused(code, f"cl_loss_bwd {what}", o, "cswin_cl_loss_bwd", *bwd_args(**kw))
    hip.refused(ERR_WORKSPACE, "cl_loss_sums one byte short", o, "cswin_cl_loss_sums", *sums_args(nb=exact - 1))
    of = dict(out5=Guarded((5,)), coef=Guarded((2 * ncls,)))
    s = put(np.ones(3 + 3 * ncls, np.float32))
    for what, code, args in (("T=0", ERR_UNSUPPORTED, (273.0, 3.0, ncls, 0.2, 0.8, 0.5, 0.0)), ("batch=0", ERR_SHAPE, (273.0, 0.0, ncls, 0.2, 0.8, 0.5, 3.0)),
                             ("n=0", ERR_SHAPE, (0.0, 3.0, ncls, 0.2, 0.8, 0.5, 3.0))):
        hip.refused(code, f"cl_loss_finalize {what}", of, "cswin_cl_loss_finalize", hip.ptr(s), hip.ptr(of["out5"].t), hip.ptr(of["coef"].t), *args, hip.stream())
    # nold == 0 with a null teacher is the documented way to run without a KD term: the KD sum is 0, nothing of the teacher is read
    sums, out5, _, dl = run_cl(hip, x, lab, None, cw, lmap, what="cl.nold0")
    ref, bound = cl_ref(x, lab, None, 3.0, 1.0, 4.0, cw, lmap)
    close(sums, ref, bound, "cl.nold0.sums")
    assert sums[-1] == 0.0 and out5[3] == 0.0
    g = cl_grad_ref(x, lab, np.zeros((B, 0, HW), np.float32), 0.5 * 0.2 / (B * HW), 0.5 * 0.8 / ncls, 0.0, cw=cw, lmap=lmap)
    assert measure(dl, g, "cl.nold0.dlogits") <= RTOL


# ---- data parallel --------------------------------------------------------------------------------------------------------------
def test_two_ranks_emulated_on_one_device(hip):
    """ops.continual_loss's data-parallel contract without a process group: the halves' sums added, finalize with the global pixel
    and image counts, the backward per half with the scales Python passes for world = 2; half of each local gradient is the
    float64 gradient of the global-batch objective for that half."""
    from test_continual_host import cl_objective
    ncls, nold, B, HW, T = 12, 9, 4, 91, 3.0
    x, t = det_normal("cl.ranks.x", (B, ncls, HW)), det_normal("cl.ranks.t", (B, nold, HW))
    lab = det_labels("cl.ranks.lab", (B, 7, 13), 4).reshape(B, HW)
    lmap = np.array([0, 9, 10, 11], np.int32)
    cw = (0.25 + np.abs(det_normal("cl.ranks.cw", (ncls,)))).astype(np.float32)
    halves = [(x[:2], lab[:2], t[:2]), (x[2:], lab[2:], t[2:])]
    local = [run_cl(hip, xh, lh, th, cw, lmap, what=f"cl.ranks.sums{r}")[0] for r, (xh, lh, th) in enumerate(halves)]
    total = (local[0] + local[1]).astype(np.float32)
    ref, _ = cl_ref(x, lab, t, T, 1.0, 4.0, cw, lmap)
    b2 = sum(cl_ref(xh, lh, th, T, 1.0, 4.0, cw, lmap)[1] for xh, lh, th in halves) + U * np.abs(ref)
    close(total, ref, b2, "cl.ranks.sums")
    xl = torch.from_numpy(x.astype(np.float64)).requires_grad_()
    obj = cl_objective(xl, lab, t, B * HW, B, 0.2, 0.8, 0.5, T, 1.0, 4.0, cw, lmap)
    obj[0].backward()
    want, bwant, _ = cl_final_ref(ref, B * HW, B, 0.2, 0.8, 0.5, T, bsums=b2)
    assert np.allclose(want, [float(v) for v in obj], rtol=1e-12, atol=1e-14)
    for r, (xh, lh, th) in enumerate(halves):
        _, out5, _, dl = run_cl(hip, xh, lh, th, cw, lmap, n_pixels=B * HW, batch=B, scales=(0.5 * 0.2 / (2 * HW), 0.5 * 0.8 / ncls * 2, 0.5 * T / 2),
                                sums_in=total, what=f"cl.ranks.bwd{r}")
        close(out5, want, bwant, f"cl.ranks.out5.{r}")
        assert measure(0.5 * dl, xl.grad[2 * r:2 * r + 2], f"cl.ranks.dlogits{r}") <= RTOL


def test_public_op_matches_the_objective(hip):
    """ops.continual_loss end to end (autograd, label map and class weights as device tensors): the five stats and the gradient
    of the loss times 1.7, against the float64 objective; the teacher receives no gradient."""
    from cswin_unet_amd import ops
    from cswin_unet_amd.continual import new_label_map
    from test_continual_host import cl_objective
    tag = "nc12.old9"
    x, lab, t, cw, lmap = cl_inputs(tag)
    B, ncls, HW = x.shape
    H, W = case_of(tag)[2]
    table = new_label_map(9, 4, "cuda")
    assert np.array_equal(table.cpu().numpy(), lmap)
    xd = torch.from_numpy(x).cuda().view(B, ncls, H, W).requires_grad_()
    td = torch.from_numpy(t).cuda().view(B, 9, H, W).requires_grad_()
    loss, stats = ops.continual_loss(xd, torch.from_numpy(lab).cuda().view(B, H, W), td, class_weight=torch.from_numpy(cw).cuda(), label_map=table)
    (1.7 * loss).backward()
    assert td.grad is None and not stats.requires_grad
    ref, bound = ref_of(tag)
    want, bwant, _ = cl_final_ref(ref, B * HW, B, 0.2, 0.8, 0.5, 3.0, bsums=bound)
    close(stats.cpu().numpy(), want, bwant, "cl.op.stats")
    assert float(loss) == float(stats[0])
    xl = torch.from_numpy(x.astype(np.float64)).requires_grad_()
    (1.7 * cl_objective(xl, lab, t, B * HW, B, cw=cw, lmap=lmap)[0]).backward()
    assert measure(xd.grad.view(B, ncls, HW).cpu(), xl.grad, "cl.op.dlogits") <= RTOL
