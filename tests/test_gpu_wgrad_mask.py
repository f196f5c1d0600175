"""Sample masks of the weight gradients (cswin_linear_bwd_weight_batch_masked / cswin_linear_bwd_tail_masked, include/cswin_hip.h):
a sample whose mask float is 0 is left out of the M reduction, its rows of dy and x are not read, and the kept samples' rows are
shared out over the launch's slabs on the device.

Shapes: 5 samples of 52 rows (M = 260, N = 96, K = 72), so that sample borders fall inside the 64-row k-tiles and inside the 8-row
granules of the split ranges (3 slabs of 88 rows unmasked); 12 samples of 196 rows with N = K = 64 for many slabs per problem (19);
40 samples of 13 rows (5 slabs) with one sample kept for slabs that stay empty.  Reference: the float64 product over the kept rows
on the CPU.  Bound: max|got - ref| / rms(ref) <= RTOL = 1e-3, the one tests/test_gpu_gemm_shapes.py applies to these entry points'
unmasked forms.  The dropped samples' rows of BOTH operands hold NaN: one read of them makes the result non-finite."""
import ctypes

import numpy as np
import pytest
import torch

from oracle.determ import det_normal
from test_gpu_parity import RTOL                        # the suite's fp32 bound, not a new one
from test_gpu_shapes import measure                     # max|got - ref| / rms(ref) in float64, printed and logged

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")


def vp(a):
    return ctypes.cast(a, ctypes.c_void_p)


class Problem:
    """One weight gradient on the device.  mask: per-sample floats or None; scale: the row_scale factors or None.  The rows of the
    samples with mask == 0 are NaN in dy and in x."""

    def __init__(self, tag, ns, rps, N, K, mask=None, scale=None, bias=True, poison=True):
        M = ns * rps
        self.ns, self.rps, self.M, self.N, self.K, self.bias = ns, rps, M, N, K, bias
        dy, x = det_normal(f"wmask.{tag}.dy", (M, N)), det_normal(f"wmask.{tag}.x", (M, K))
        self.mask_h = None if mask is None else np.asarray(mask, np.float32)
        self.scale_h = None if scale is None else np.asarray(scale, np.float32)
        keep = np.ones(ns, bool) if mask is None else self.mask_h != 0
        rows = np.repeat(keep, rps)
        f = np.repeat(self.scale_h, rps)[:, None].astype(np.float64) if scale is not None else 1.0
        sdy = (dy.astype(np.float64) * f)[rows]
        self.dw_ref = torch.from_numpy(sdy.T @ x.astype(np.float64)[rows])
        self.db_ref = torch.from_numpy(sdy.sum(0))
        if poison:
            dy, x = dy.copy(), x.copy()
            dy[~rows], x[~rows] = NAN, NAN
        self.dy, self.x = torch.from_numpy(dy).to(DEV), torch.from_numpy(x).to(DEV)
        self.mask = None if mask is None else torch.from_numpy(self.mask_h).to(DEV)
        self.scale = None if scale is None else torch.from_numpy(self.scale_h).to(DEV)


def launch(probs, masked, tail=None, pending=None, precision=0, nsamples=None):
    """The problems through the masked (or the unmasked) entry point, then their slab reductions.  tail = (dy, w): the data
    gradient rides (cswin_linear_bwd_tail*); pending: a ReduceJob array that rides.  -> [(dw, dbias)], dx"""
    from cswin_unet_amd._lib import ReduceJob, WgradDesc, call, lib, ptr, stream
    n = len(probs)
    wg, jobs, keep, outs = (WgradDesc * n)(), (ReduceJob * n)(), [], []
    for i, p in enumerate(probs):
        dw = torch.full((p.N, p.K), NAN, device=DEV)
        db = torch.full((p.N,), NAN, device=DEV) if p.bias else None
        nbytes = lib().cswin_linear_bwd_weight_workspace(p.M, p.N, p.K)
        ws = torch.full((nbytes // 4 + 4,), NAN, device=DEV)
        keep.append(ws)
        wg[i].dy, wg[i].x, wg[i].row_scale = p.dy.data_ptr(), p.x.data_ptr(), (p.scale.data_ptr() if p.scale is not None else None)
        wg[i].dw, wg[i].dbias, wg[i].workspace, wg[i].ws_bytes = dw.data_ptr(), (db.data_ptr() if p.bias else None), ws.data_ptr(), nbytes
        wg[i].rows_per_sample, wg[i].M, wg[i].N, wg[i].K, wg[i].precision = p.rps, p.M, p.N, p.K, precision
        outs.append((dw, db))
    pend = (vp(pending), len(pending)) if pending is not None else (None, 0)
    extra = ()
    if masked:
        skip = (ctypes.c_void_p * n)(*[p.mask.data_ptr() if p.mask is not None else None for p in probs])
        ns = (ctypes.c_int * n)(*(nsamples or [p.ns for p in probs]))
        extra = (skip, ns)
    sfx = "_masked" if masked else ""
    dx = None
    if tail is not None:
        tdy, tw = tail
        dx = torch.full((tdy.shape[0], tw.shape[1]), NAN, device=DEV)
        call("cswin_linear_bwd_tail" + sfx, ptr(tdy), ptr(tw), ptr(dx), tdy.shape[0], tdy.shape[1], tw.shape[1], vp(wg), n, vp(jobs),
             *pend, *extra, stream())
    else:
        call("cswin_linear_bwd_weight_batch" + sfx, vp(wg), n, vp(jobs), *pend, *extra, stream())
    call("cswin_rows_sum_multi", vp(jobs), n, stream())
    torch.cuda.synchronize()
    return outs, dx


def check(what, probs, outs):
    for i, (p, (dw, db)) in enumerate(zip(probs, outs)):
        assert bool(torch.isfinite(dw).all()), f"{what}.{i}: dw is not finite (a dropped sample's rows were read)"
        errs = {"dw": measure(dw, p.dw_ref, f"wmask.{what}.{i}.dw")}
        if db is not None:
            assert bool(torch.isfinite(db).all()), f"{what}.{i}: dbias is not finite"
            errs["dbias"] = measure(db, p.db_ref, f"wmask.{what}.{i}.dbias")
        assert all(np.isfinite(e) and e <= RTOL for e in errs.values()), (what, i, errs)


SMALL = dict(ns=5, rps=52, N=96, K=72)
MANY = dict(ns=12, rps=196, N=64, K=64)
DROPS = {"first": [0, 1, 1, 1, 1], "last": [1, 1, 1, 1, 0], "neighbours": [1, 0, 0, 1, 1], "all_but_one": [0, 0, 1, 0, 0]}


@pytest.mark.parametrize("shape", [SMALL, MANY], ids=["small", "many_splits"])
@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "row_scale"])
def test_every_sample_kept_equals_the_unmasked_launch(shape, scaled):
    """Same split boundaries, so every bit of dw and dbias (the slabs' reduced result) is the unmasked entry point's."""
    ns = shape["ns"]
    scale = [1.25, 0.5, 2.0, 1.0, 0.75, 1.5, 1.25, 1.0, 0.5, 2.0, 1.25, 1.0][:ns] if scaled else None
    p = Problem(f"all.{ns}", mask=[1.25] * ns, scale=scale, **shape)
    got, _ = launch([p], True)
    want, _ = launch([p], False)
    check(f"all.{ns}.{int(scaled)}", [p], got)
    assert torch.equal(got[0][0], want[0][0]) and torch.equal(got[0][1], want[0][1])


@pytest.mark.parametrize("drop", sorted(DROPS))
@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "row_scale"])
def test_dropped_samples_are_left_out_and_not_read(drop, scaled):
    m = np.array(DROPS[drop], np.float32) * 1.25
    p = Problem(f"drop.{drop}", mask=m, scale=m * np.array([1, 0.5, 2, 1, 3], np.float32) if scaled else None, **SMALL)
    check(f"drop.{drop}.{int(scaled)}", [p], launch([p], True)[0])


def test_dropped_samples_over_many_splits():
    m = [1, 0, 1, 1, 0, 0, 1, 1, 1, 0, 1, 1]
    p = Problem("many.drop", mask=m, scale=m, **MANY)
    check("many.drop", [p], launch([p], True)[0])


def test_every_sample_dropped_gives_exact_zeros():
    p = Problem("none", mask=[0.0] * 5, scale=[0.0] * 5, **SMALL)
    (dw, db), = launch([p], True)[0]
    assert int(torch.count_nonzero(dw)) == 0 and int(torch.count_nonzero(db)) == 0
    assert bool(torch.isfinite(dw).all()) and bool(torch.isfinite(db).all())


def test_fewer_kept_rows_than_slabs():
    """40 samples of 13 rows go out as 5 slabs; one kept sample fills two 8-row ranges, the other three slabs are empty."""
    m = np.zeros(40, np.float32)
    m[17] = 1.5
    p = Problem("few", ns=40, rps=13, N=96, K=72, mask=m, scale=m)
    check("few", [p], launch([p], True)[0])


def _batch_of_four():
    m1, m2 = np.array([1, 0, 1, 1, 0], np.float32) * 1.25, np.array([0, 1, 1, 0, 1], np.float32) * 2.0
    return [Problem("b4.0", 5, 52, 96, 72, mask=m1, scale=m1), Problem("b4.1", 5, 52, 72, 96, mask=m1),
            Problem("b4.2", 5, 52, 64, 64, mask=m2, scale=m2, bias=False), Problem("b4.3", 5, 52, 96, 32, mask=None)]


def test_batch_of_four_with_two_masks_and_one_without():
    probs = _batch_of_four()
    check("batch4", probs, launch(probs, True)[0])


def test_tail_of_four_with_data_gradient_and_rider():
    """The data gradient's tiles and the riding reduction do not see the masks: bit-identical to the unmasked call's."""
    from cswin_unet_amd._lib import ReduceJob
    probs = _batch_of_four()
    tw = torch.from_numpy(det_normal("wmask.tail.w", (96, 32), 1 / np.sqrt(32))).to(DEV)
    part = torch.from_numpy(det_normal("wmask.tail.part", (7, 300))).to(DEV)

    def run(masked):
        out = torch.full((300,), NAN, device=DEV)
        pend = (ReduceJob * 1)()
        pend[0].part, pend[0].out, pend[0].n_first, pend[0].n, pend[0].stride, pend[0].rows = part.data_ptr(), out.data_ptr(), 300, 300, 300, 7
        outs, dx = launch(probs, masked, tail=(probs[3].dy, tw), pending=pend)
        return outs, dx, out

    outs, dx, rider = run(True)
    check("tail4", probs, outs)
    # the unmasked call reads the NaN rows into its weight gradients; its data gradient (of the unmasked problem's dy) and its rider
    # see none of them
    _, dx_u, rider_u = run(False)
    assert torch.equal(dx, dx_u) and torch.equal(rider, rider_u)
    assert measure(dx, probs[3].dy.double().cpu() @ tw.double().cpu(), "wmask.tail4.dx") <= RTOL
    # a column sum of 7 fp32 values: 6 roundings of at most 2^-24 of a partial sum each, partial sums within a few rms
    assert measure(rider, part.double().sum(0), "wmask.tail4.rider") <= 1e-6


def test_what_a_mask_cannot_keep_is_refused():
    """precision 1, nsamples * rows_per_sample != M and more than 256 samples are error returns, never an unmasked run."""
    from cswin_unet_amd._lib import CswinHipError
    p = Problem("err", mask=[1, 0, 1, 1, 1], poison=False, **SMALL)
    with pytest.raises(CswinHipError, match="precision 0"):
        launch([p], True, precision=1)
    with pytest.raises(CswinHipError, match="nsamples"):
        launch([p], True, nsamples=[4])
    big = Problem("err257", ns=257, rps=4, N=32, K=32, mask=np.ones(257, np.float32), poison=False)
    with pytest.raises(CswinHipError, match="256 samples"):
        launch([big], True)
    check("err.ok", [p], launch([p], True)[0])           # the same problem with legal arguments runs


def test_block_gradients_with_dropped_samples(monkeypatch):
    """ops.cswin_block at B = 6, reso 14, C = 64 with zeros in rs1 / rs2: every parameter gradient against the same block run
    through the unmasked entry points, at the bound tests/test_gpu_parity.py holds block gradients to (rel_err: RTOL)."""
    import cswin_unet_amd.networks.cswin_unet as N
    from cswin_unet_amd import ops
    from oracle.determ import fill_state_dict
    from test_gpu_parity import rel_err
    B, reso, dim = 6, 14, 64
    blk = N.CSWinBlock(dim, reso, 2, 7, qkv_bias=True).to(DEV)
    fill_state_dict(blk)
    a, n1, n2, fc1, fc2 = blk.attns, blk.norm1, blk.norm2, blk.mlp.fc1, blk.mlp.fc2
    idx, hd, lw, lb = [m.idx for m in a], [m.num_heads for m in a], [m.get_v.weight for m in a], [m.get_v.bias for m in a]
    rs1 = torch.tensor([1.25, 0.0, 1.25, 1.25, 0.0, 1.25], device=DEV)
    rs2 = torch.tensor([0.0, 1.25, 1.25, 0.0, 0.0, 1.25], device=DEV)
    x0 = torch.from_numpy(det_normal("wmask.block.x", (B, reso * reso, dim))).to(DEV)
    dy = torch.from_numpy(det_normal("wmask.block.dy", (B, reso * reso, dim))).to(DEV)
    called = []
    real_call = ops.call
    monkeypatch.setattr(ops, "call", lambda name, *args: (called.append(name), real_call(name, *args))[1])

    def run():
        blk.zero_grad(set_to_none=True)
        x = x0.clone().requires_grad_()
        y = ops.cswin_block(x, reso, 7, idx, hd, a[0].scale, n1, blk.qkv, blk.proj, n2, fc1, fc2, lw, lb, rs1, rs2)
        y.backward(dy)
        torch.cuda.synchronize()
        return x.grad, {n: p.grad.clone() for n, p in blk.named_parameters()}

    dx, g = run()
    assert "cswin_linear_bwd_tail_masked" in called and "cswin_linear_bwd_tail" not in called
    del called[:]
    monkeypatch.setattr(ops, "MAX_MASK_SAMPLES", 0)      # no batch is small enough: the unmasked entry point
    dx_u, g_u = run()
    assert "cswin_linear_bwd_tail" in called and "cswin_linear_bwd_tail_masked" not in called
    assert torch.equal(dx, dx_u)                         # the data gradients do not see the masks
    assert len(g) == len(g_u) == len(list(blk.parameters()))
    for n in g:
        rel_err(g[n], g_u[n], f"wmask.block.grad.{n}")
