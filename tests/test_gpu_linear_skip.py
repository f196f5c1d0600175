"""Sample orders of the forward and data-gradient Linears (cswin_drop_path_order, cswin_linear_fwd_skip, cswin_linear_bwd_data_skip,
cswin_linear_bwd_tail_skip; include/cswin_hip.h): a launch with an order computes the kept samples' rows in its first row tiles --
bit for bit what the call without an order gives them --, reads no A row and no gelu_pre row of a dropped sample, and leaves in
the dropped samples' rows what zero A rows give: the bias, GELU(bias), the residual row, +0.

Every comparison here is exact (torch.equal against the entry point without an order, or against the stated value); there is no
tolerance.  Shapes (samples, rows per sample, output columns, reduction): rows per sample 49 (several samples in a 64-row tile), 64
(tile-aligned) and 196 (a sample straddles tiles), 3 and 24 samples, and sizes at which the host picks each of its five fp32 tile
configurations for these launches (asserted with the transcription of its rules in tests/test_gpu_gemm_shapes.py).  The A rows and
gelu_pre rows of dropped samples hold NaN: one read of them makes the output non-finite."""
import ctypes

import numpy as np
import pytest
import torch

from oracle.determ import det_normal
from test_gpu_gemm_shapes import one_split, tiled_config        # the host's tile choice, transcribed

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")

# (samples, rows per sample, output columns, reduction) -> the configuration the host picks, forward and data gradient alike
SHAPES = [
    ((3, 49, 96, 64), (64, 32, 32, 1)),
    ((3, 64, 96, 64), (64, 32, 32, 1)),
    ((3, 196, 96, 64), (64, 32, 32, 1)),
    ((24, 49, 64, 256), (64, 32, 64, 2)),
    ((24, 49, 512, 64), (64, 64, 32, 1)),
    ((3, 196, 1024, 64), (64, 64, 32, 1)),
    ((24, 64, 384, 256), (64, 64, 64, 2)),
    ((24, 49, 512, 256), (64, 64, 64, 2)),
    ((24, 49, 512, 512), (64, 64, 64, 4)),
]
FORMS = [("fwd", "plain"), ("fwd", "gelu"), ("fwd", "res"), ("dgrad", "plain"), ("dgrad", "scaled"), ("dgrad", "gelu")]


def drop_patterns(ns):
    """name -> kept flags: first, last, two neighbours, all but one, every sample dropped."""
    one = lambda *drop: np.array([i not in drop for i in range(ns)])
    return {"first": one(0), "last": one(ns - 1), "neighbours": one(1, 2) if ns > 3 else one(0, 1), "all_but_one": ~one(ns // 2),
            "every": np.zeros(ns, bool)}


def order_of(keep):
    keep = np.asarray(keep, bool)
    idx = np.arange(len(keep))
    return np.concatenate([[int(keep.sum())], idx[keep], idx[~keep]]).astype(np.int32)


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Case:
    """One Linear, forward or data gradient, on the device.  The weight is (N, K) either way; the forward reads x (M, K) and
    writes (M, N), the data gradient reads dy (M, N) and writes (M, K)."""

    def __init__(self, entry, form, ns, rps, cols, red):
        self.entry, self.form, self.ns, self.rps, self.M, self.cols, self.red = entry, form, ns, rps, ns * rps, cols, red
        tag = f"skip.{entry}.{form}.{ns}.{rps}.{cols}.{red}"
        M = self.M
        self.a = det_normal(tag + ".a", (M, red))
        wshape = (cols, red) if entry == "fwd" else (red, cols)
        self.w = T(det_normal(tag + ".w", wshape, 1 / np.sqrt(red)))
        self.bias = T(det_normal(tag + ".b", (cols,))) if entry == "fwd" else None
        self.residual = T(det_normal(tag + ".res", (M, cols))) if form == "res" else None
        self.pre = det_normal(tag + ".pre", (M, cols)) if (entry, form) == ("dgrad", "gelu") else None
        self.scaled = form in ("res", "scaled") or (entry, form) == ("dgrad", "gelu")     # the forms the blocks run with a row scale

    def run(self, keep=None, *, skip, poison=False, zero_a=False):
        """-> the outputs (y[, y_act]) or (dx,).  keep: per-sample flags (None: all); the row scale is 1.25 for a kept sample and 0
        for a dropped one.  poison: NaN in the dropped samples' rows of A and gelu_pre."""
        from cswin_unet_amd._lib import call, ptr, stream
        keep = np.ones(self.ns, bool) if keep is None else keep
        rows = np.repeat(keep, self.rps)
        a = np.zeros_like(self.a) if zero_a else self.a.copy()
        pre = None if self.pre is None else self.pre.copy()
        if poison:
            a[~rows] = NAN
            if pre is not None:
                pre[~rows] = NAN
        a, pre = T(a), (None if pre is None else T(pre))
        rs = T(np.where(keep, 1.25, 0.0).astype(np.float32)) if self.scaled else None
        order = T(order_of(keep))
        out = torch.full((self.M, self.cols), NAN, device=DEV)
        tail = (ptr(order), self.ns, stream()) if skip else (stream(),)
        sfx = "_skip" if skip else ""
        if self.entry == "fwd":
            act = torch.full_like(out, NAN) if self.form == "gelu" else None
            call("cswin_linear_fwd" + sfx, ptr(a), None, 0, ptr(self.w), ptr(self.bias), ptr(out), ptr(act), ptr(self.residual), ptr(rs), self.rps,
                 self.M, self.cols, self.red, 0, 0, *tail)
            outs = (out, act) if act is not None else (out,)
        else:
            call("cswin_linear_bwd_data" + sfx, ptr(a), ptr(self.w), ptr(out), None, 0, ptr(pre), ptr(rs), self.rps, None, self.M, self.red,
                 self.cols, 0, 0, *tail)
            outs = (out,)
        torch.cuda.synchronize()
        return outs


@pytest.mark.parametrize("shape,config", SHAPES, ids=["-".join(map(str, s)) for s, _ in SHAPES])
def test_kept_rows_are_the_unmapped_launch_and_dropped_rows_what_zero_rows_give(shape, config):
    ns, rps, cols, red = shape
    assert tiled_config(ns * rps, cols, red, 1, one_split(red), False, 0) == config
    for entry, form in FORMS:
        c = Case(entry, form, *shape)
        plain = c.run(skip=False)                                   # every sample computed, no order
        zero = c.run(skip=False, zero_a=True)                       # what zero A rows give, by the same device functions
        every = c.run(skip=True)                                    # an order with every sample kept: the identity
        for o, p in zip(every, plain):
            assert torch.equal(o, p), (entry, form, "all kept")
        for name, keep in drop_patterns(ns).items():
            what = (entry, form, name)
            got = c.run(keep, skip=True, poison=True)
            rows = T(np.repeat(keep, rps))
            for o, p in zip(got, plain):
                assert bool(torch.isfinite(o).all()), what
                assert torch.equal(o[rows], p[rows]), what
            d = got[0][~rows]
            if entry == "dgrad":
                assert int(torch.count_nonzero(d)) == 0 and not bool(torch.signbit(d).any()), what          # +0
            elif form == "res":
                assert torch.equal(d, c.residual[~rows]), what
            else:
                assert torch.equal(d, c.bias.expand_as(d)), what
                if form == "gelu":
                    assert torch.equal(got[1][~rows], zero[1][~rows]), what                                  # GELU(bias)


@pytest.mark.parametrize("B", [1, 24, 64, 65, 256])
def test_drop_path_order_kernel(B):
    from cswin_unet_amd import ops
    g = torch.Generator().manual_seed(100 + B)
    keep = torch.tensor([1.0, 0.5, 0.95, 0.8, 0.85, 0.3, 0.9], dtype=torch.float32)
    u = torch.rand(len(keep), B, generator=g)
    u[1] = 0.5 + 0.5 * u[1]                              # row 1: every sample dropped (u >= keep); row 0 (keep = 1): none
    scales, order = ops.drop_path_order(u.to(DEV), keep[:, None].to(DEV))
    torch.cuda.synchronize()
    want = ((u < keep[:, None]).to(torch.float32) / keep[:, None]).to(DEV)
    assert torch.equal(scales, ((u.to(DEV) < keep[:, None].to(DEV)).to(torch.float32) / keep[:, None].to(DEV)))
    assert torch.equal(scales, want)
    ref = np.stack([order_of(r) for r in (u < keep[:, None]).numpy()])
    assert order.dtype == torch.int32 and np.array_equal(order.cpu().numpy(), ref)
    assert ref[0, 0] == B and ref[1, 0] == 0


def test_tail_with_an_order_on_its_data_gradient():
    """cswin_linear_bwd_tail_skip against cswin_linear_bwd_tail_masked: the same weight gradients bit for bit, the data gradient's
    kept rows bit for bit, its dropped rows +0 without reading dy's."""
    from cswin_unet_amd._lib import ReduceJob, WgradDesc, call, lib, ptr, stream
    ns, rps, N, K = 5, 52, 96, 32
    M = ns * rps
    keep = np.array([1, 0, 1, 1, 0], bool)
    rows = np.repeat(keep, rps)
    dy = det_normal("skip.tail.dy", (M, N))
    dy[~rows] = 0.0                                       # the masked weight gradients leave these rows out; the unmapped dgrad reads them
    x = T(det_normal("skip.tail.x", (M, K)))
    w = T(det_normal("skip.tail.w", (N, K), 1 / np.sqrt(K)))
    mask = T(keep.astype(np.float32) * 1.25)
    order = T(order_of(keep))
    dyp = dy.copy()
    dyp[~rows] = NAN

    def run(skip, dyt):
        wg, jobs = (WgradDesc * 1)(), (ReduceJob * 1)()
        dw, db, dx = torch.full((N, K), NAN, device=DEV), torch.full((N,), NAN, device=DEV), torch.full((M, K), NAN, device=DEV)
        nbytes = lib().cswin_linear_bwd_weight_workspace(M, N, K)
        ws = torch.empty(nbytes // 4 + 4, device=DEV)
        wg[0].dy, wg[0].x, wg[0].dw, wg[0].dbias, wg[0].workspace, wg[0].ws_bytes = dyt.data_ptr(), x.data_ptr(), dw.data_ptr(), db.data_ptr(), ws.data_ptr(), nbytes
        wg[0].rows_per_sample, wg[0].M, wg[0].N, wg[0].K = rps, M, N, K
        masks, counts = (ctypes.c_void_p * 1)(mask.data_ptr()), (ctypes.c_int * 1)(ns)
        args = (ptr(dyt), ptr(w), ptr(dx), M, N, K, ctypes.cast(wg, ctypes.c_void_p), 1, ctypes.cast(jobs, ctypes.c_void_p), None, 0, masks, counts)
        if skip:
            call("cswin_linear_bwd_tail_skip", *args, ptr(order), ns, stream())
        else:
            call("cswin_linear_bwd_tail_masked", *args, stream())
        call("cswin_rows_sum_multi", ctypes.cast(jobs, ctypes.c_void_p), 1, stream())
        torch.cuda.synchronize()
        return dw, db, dx

    dw0, db0, dx0 = run(False, T(dy))
    dw1, db1, dx1 = run(True, T(dyp))
    assert torch.equal(dw0, dw1) and torch.equal(db0, db1)
    r = T(rows)
    assert torch.equal(dx1[r], dx0[r]) and int(torch.count_nonzero(dx1[~r])) == 0 and not bool(torch.signbit(dx1[~r]).any())
    full = T(order_of(np.ones(ns, bool)))
    order = full                                           # every sample kept: the whole data gradient is the masked call's
    assert torch.equal(run(True, T(dy))[2], dx0)


def test_what_an_order_cannot_serve_is_refused():
    """precision 1, concat / split / add operands, nsamples * rows_per_sample != M, more than 256 samples and unaligned operands
    are error returns of the *_skip entry points, never a run without the order."""
    from cswin_unet_amd._lib import CswinHipError, call, ptr, stream
    ns, rps, N, K = 4, 16, 32, 64
    M = ns * rps
    x, w, y, dx = (torch.zeros(s, device=DEV) for s in ((M, K), (N, K), (M, N), (M, K)))
    big = torch.zeros(M * N + 4, device=DEV)
    order = T(order_of(np.ones(ns, bool)))

    def fwd(**kw):
        a = dict(x=x, x2=None, ks=0, y=y, M=M, K=K, prec=0, io=0, order=order, ns=ns)
        a.update(kw)
        call("cswin_linear_fwd_skip", ptr(a["x"]), ptr(a["x2"]), a["ks"], ptr(w), None, ptr(a["y"]), None, None, None, rps, a["M"], N, a["K"],
             a["prec"], a["io"], ptr(a["order"]), a["ns"], stream())

    def dgrad(**kw):
        a = dict(dx2=None, ks=0, add=None, prec=0, ns=ns, dy=y)
        a.update(kw)
        call("cswin_linear_bwd_data_skip", ptr(a["dy"]), ptr(w), ptr(dx), ptr(a["dx2"]), a["ks"], None, None, rps, ptr(a["add"]), M, N, K, a["prec"],
             0, ptr(order), a["ns"], stream())

    for f in (fwd, dgrad):
        with pytest.raises(CswinHipError, match=r"\(-5\).*precision 0"):
            f(prec=1)
        with pytest.raises(CswinHipError, match=r"\(-1\).*nsamples \* rows_per_sample"):
            f(ns=3)
        with pytest.raises(CswinHipError, match=r"\(-1\).*1\.\.256 samples"):
            f(ns=257)
    with pytest.raises(CswinHipError, match=r"\(-5\).*concat"):
        fwd(x2=x, ks=32, K=2 * K)
    with pytest.raises(CswinHipError, match=r"\(-5\).*concat / split"):
        dgrad(dx2=dx, ks=32)
    with pytest.raises(CswinHipError, match=r"\(-5\).*add"):
        dgrad(add=dx)
    with pytest.raises(CswinHipError, match=r"\(-1\).*1\.\.256 samples"):
        fwd(order=None)
    with pytest.raises(CswinHipError, match=r"\(-2\).*16-B aligned"):
        fwd(y=big[1:1 + M * N].view(M, N))
    with pytest.raises(CswinHipError, match=r"\(-2\).*16-B aligned"):
        dgrad(dy=big[1:1 + M * N].view(M, N))
    with pytest.raises(CswinHipError, match=r"\(-5\).*fp32 storage"):
        fwd(io=1, prec=1)
    fwd()                                                  # the same calls with legal arguments run
    dgrad()
    torch.cuda.synchronize()


def test_block_with_orders_equals_block_without(monkeypatch):
    """ops.cswin_block at B = 6, reso 14, C = 64 with zeros in rs1 / rs2: y, dx and every parameter gradient with the sample orders
    equal those without (torch.equal: a dropped row's zero may change its sign, nothing else may move)."""
    import cswin_unet_amd.networks.cswin_unet as N
    from cswin_unet_amd import ops
    from oracle.determ import fill_state_dict
    B, reso, dim = 6, 14, 64
    blk = N.CSWinBlock(dim, reso, 2, 7, qkv_bias=True).to(DEV)
    fill_state_dict(blk)
    a, n1, n2, fc1, fc2 = blk.attns, blk.norm1, blk.norm2, blk.mlp.fc1, blk.mlp.fc2
    idx, hd, lw, lb = [m.idx for m in a], [m.num_heads for m in a], [m.get_v.weight for m in a], [m.get_v.bias for m in a]
    k1, k2 = np.array([1, 0, 1, 1, 0, 1], bool), np.array([0, 1, 1, 0, 0, 1], bool)
    rs1, rs2 = T(k1.astype(np.float32) * 1.25), T(k2.astype(np.float32) * 1.25)
    orders = (T(order_of(k1)), T(order_of(k2)))
    x0 = T(det_normal("skip.block.x", (B, reso * reso, dim)))
    dy = T(det_normal("skip.block.dy", (B, reso * reso, dim)))
    called = []
    real_call = ops.call
    monkeypatch.setattr(ops, "call", lambda name, *args: (called.append(name), real_call(name, *args))[1])

    def run(orders):
        blk.zero_grad(set_to_none=True)
        del called[:]
        x = x0.clone().requires_grad_()
        y = ops.cswin_block(x, reso, 7, idx, hd, a[0].scale, n1, blk.qkv, blk.proj, n2, fc1, fc2, lw, lb, rs1, rs2, orders=orders)
        y.backward(dy)
        torch.cuda.synchronize()
        return y.detach(), x.grad, {n: p.grad.clone() for n, p in blk.named_parameters()}, list(called)

    y1, dx1, g1, names1 = run(orders)
    assert names1.count("cswin_linear_fwd_skip") == 4 and names1.count("cswin_linear_bwd_data_skip") == 3
    assert names1.count("cswin_linear_bwd_tail_skip") == 1 and "cswin_linear_fwd" not in names1 and "cswin_linear_bwd_data" not in names1
    y0, dx0, g0, names0 = run(None)
    assert not any(n.endswith("_skip") for n in names0)
    assert torch.equal(y1, y0) and torch.equal(dx1, dx0)
    assert len(g1) == len(g0) == len(list(blk.parameters()))
    for n in g0:
        assert torch.equal(g1[n], g0[n]), n


def test_model_predraw_hands_every_live_block_its_orders():
    """CSWinTransformer._predraw_drop_path: the factors are torch's from the same draws, and each block's orders list its zeros."""
    import cswin_unet_amd.networks.cswin_unet as N
    net = N.CSWinTransformer(img_size=224, num_classes=9, embed_dim=32, depth=[1, 1, 2, 1], split_size=[1, 2, 7, 7], num_heads=[2, 4, 8, 16],
                             qkv_bias=True, drop_path_rate=0.5).to(DEV).train()
    torch.manual_seed(7)
    net._predraw_drop_path(24, torch.device(DEV))
    torch.manual_seed(7)
    keep = net._dp_keep
    want = (torch.rand(keep.shape[0], 24, device=DEV) < keep).to(torch.float32) / keep
    live = [b for st in (net.stage1, net.stage2, net.stage3, net.stage4, net.stage_up4, net.stage_up3, net.stage_up2, net.stage_up1) for b in st
            if b._dp_preset]
    assert 2 * len(live) == keep.shape[0] and len(live) >= 4
    for i, b in enumerate(live):
        rs1, rs2, o1, o2 = b._dp_preset
        assert torch.equal(rs1, want[2 * i]) and torch.equal(rs2, want[2 * i + 1])
        for rs, o in ((rs1, o1), (rs2, o2)):
            assert np.array_equal(o.cpu().numpy(), order_of((rs != 0).cpu().numpy()))
        assert b._keep_orders(rs1) is not None and b._keep_orders(rs1.clone()) is None
