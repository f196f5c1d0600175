"""GPU parity tests (run with ``-m gpu`` on an MI355X): the HIP path, called through the C ABI, against
 (a) the committed golden vectors generated from the imported reference (tests/golden), and
 (b) the CPU oracle on the same seeded inputs at sizes the oracle finishes in seconds.
Tolerance: 1e-3 relative (to tensor RMS) in fp32 as BASELINE.json's north_star states; the index-only
ops are compared bit-exactly."""
import os

import numpy as np
import pytest
import torch

from oracle import cswin_oracle as O
from oracle.determ import det_labels, det_normal, fill_param, fill_state_dict, check_packed

pytestmark = pytest.mark.gpu
RTOL = 1e-3
DEV = "cuda"
LOG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out", "parity_errors.log")


def T(a, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t.requires_grad_() if grad else t


def rel_err(got, ref, what):
    got = got.detach().float().cpu()
    ref = ref.detach().float().cpu()
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    rms = float(ref.pow(2).mean().sqrt()) + 1e-30
    err = float((got - ref).abs().max()) / rms
    try:
        os.makedirs(os.path.dirname(LOG), exist_ok=True)
        with open(LOG, "a") as f:
            f.write(f"{what}: {err:.3e}\n")
    except OSError:
        pass
    assert np.isfinite(err) and err <= RTOL, f"{what}: max|diff|/rms = {err:.3e} > {RTOL}"
    return err


@pytest.fixture(scope="module")
def N():
    import cswin_unet_amd.networks.cswin_unet as net
    return net


@pytest.fixture(scope="module")
def ops():
    from cswin_unet_amd import ops
    return ops


def test_library_is_the_hip_one():
    from cswin_unet_amd import _lib
    h = _lib.lib()
    assert h.cswin_abi_version() == 4
    assert h.cswin_device_ok() == 1, h.cswin_last_error().decode()
    with pytest.raises(_lib.CswinHipError):         # no CPU fallback
        from cswin_unet_amd import ops
        ops.layer_norm(torch.zeros(4, 64), torch.ones(64), torch.zeros(64))


ATTN = [(56, 0, 1, 32, 1), (56, 1, 1, 32, 1), (28, 0, 2, 64, 2), (28, 1, 2, 64, 2),
        (14, 0, 7, 128, 4), (14, 1, 7, 128, 4), (7, -1, 7, 512, 16)]
ATTN384 = [(96, 0, 1, 32, 1), (24, 0, 12, 128, 4), (24, 1, 12, 128, 4), (12, -1, 12, 512, 16)]


@pytest.mark.parametrize("reso,idx,split,dim,heads", ATTN + ATTN384)
def test_window_index_ops_bit_exact(N, golden, reso, idx, split, dim, heads):
    g = golden("g1_index_maps")
    key = f"r{reso}_i{idx}_s{split}"
    H_sp, W_sp = O.window_shape(reso, idx, split)
    C = 8
    enc = (torch.arange(reso * reso, dtype=torch.float32)[:, None] * C + torch.arange(C, dtype=torch.float32)[None])
    img = enc.t().reshape(1, C, reso, reso).repeat(2, 1, 1, 1)
    img[1] += 0.5
    win = N.img2windows(img.to(DEV), H_sp, W_sp)
    gather = torch.from_numpy(g[key + ".gather"].astype(np.int64))                   # [nWin, N]
    expect = enc[gather]                                                              # [nWin, N, C]
    assert torch.equal(win.cpu(), torch.cat([expect, expect + 0.5]))
    back = N.windows2img(win, H_sp, W_sp, reso, reso)
    assert torch.equal(back.cpu(), img.permute(0, 2, 3, 1))
    with pytest.raises(Exception):
        N.img2windows(img.to(DEV), 5, W_sp)


@pytest.mark.parametrize("M,C", [(3136 * 2, 64), (784 * 3, 128), (197, 256), (49, 512), (5, 64), (1, 512)])
def test_layernorm(ops, M, C):
    x = (det_normal(f"ln.x.{M}.{C}", (M, C), 2.0) + 0.3).astype(np.float32)
    g, b = (1 + det_normal("ln.g", (C,), 0.1)).astype(np.float32), det_normal("ln.b", (C,), 0.1)
    dy = det_normal(f"ln.dy.{M}.{C}", (M, C))
    xr, gr, br = (torch.from_numpy(a).requires_grad_() for a in (x, g, b))
    yr = torch.nn.functional.layer_norm(xr, (C,), gr, br, 1e-5)
    yr.backward(torch.from_numpy(dy))
    xd, gd, bd = T(x, True), T(g, True), T(b, True)
    yd = ops.layer_norm(xd, gd, bd, 1e-5)
    yd.backward(T(dy))
    rel_err(yd, yr, f"ln{M}x{C}.y")
    rel_err(xd.grad, xr.grad, f"ln{M}x{C}.dx")
    rel_err(gd.grad, gr.grad, f"ln{M}x{C}.dgamma")
    rel_err(bd.grad, br.grad, f"ln{M}x{C}.dbeta")


LIN = [(3136 * 2, 192, 64), (784 * 2, 384, 128), (392, 768, 256), (98, 1536, 512), (98, 2048, 512), (98, 512, 2048),
       (1, 9, 64), (37, 36, 100), (300, 16, 64), (129, 65, 33)]


@pytest.mark.parametrize("M,Nn,K", LIN)
def test_linear_fwd_bwd(ops, M, Nn, K):
    x, w, b = det_normal("lin.x", (M, K)), det_normal("lin.w", (Nn, K), 1 / np.sqrt(K)), det_normal("lin.b", (Nn,))
    dy = det_normal("lin.dy", (M, Nn))
    xr, wr, br = (torch.from_numpy(a).requires_grad_() for a in (x, w, b))
    yr = torch.nn.functional.linear(xr, wr, br)
    yr.backward(torch.from_numpy(dy))
    xd, wd, bd = T(x, True), T(w, True), T(b, True)
    yd = ops.linear(xd, wd, bd)
    yd.backward(T(dy))
    tag = f"linear{M}x{Nn}x{K}"
    rel_err(yd, yr, tag + ".y")
    rel_err(xd.grad, xr.grad, tag + ".dx")
    rel_err(wd.grad, wr.grad, tag + ".dw")
    rel_err(bd.grad, br.grad, tag + ".db")


@pytest.mark.parametrize("shapes", [[(4704, 256, 1024), (4704, 1024, 256), (4704, 256, 256), (4704, 768, 256)],
                                    [(3000, 64, 64)], [(777, 130, 100), (777, 64, 100)], [(1176, 512, 2048), (1176, 2048, 512)]])
def test_linear_weight_gradient_batch(shapes):
    """cswin_linear_bwd_weight_batch through the C ABI: 1-4 problems in one launch (with and without DropPath row scales and
    bias), including a problem whose N is not a multiple of 4 (falls back to separate launches), vs torch."""
    import ctypes
    from cswin_unet_amd._lib import ReduceJob, WgradDesc, call, lib, stream
    n = len(shapes)
    wg, jobs, keep, refs = (WgradDesc * n)(), (ReduceJob * n)(), [], []
    for i, (M, N_, K) in enumerate(shapes):
        dy, x = det_normal(f"wb.dy{i}", (M, N_)), det_normal(f"wb.x{i}", (M, K))
        rps = M // 3
        rs = np.array([0.0, 1.25, 0.5], np.float32) if i % 2 == 0 else None
        with_bias = i != 1
        dyd, xd = T(dy), T(x)
        rsd = T(rs) if rs is not None else None
        dw = torch.empty(N_, K, device=DEV)
        db = torch.empty(N_, device=DEV) if with_bias else None
        nbytes = lib().cswin_linear_bwd_weight_workspace(M, N_, K)
        ws = torch.empty(nbytes // 4 + 4, device=DEV)
        keep += [dyd, xd, rsd, ws]
        wg[i].dy, wg[i].x, wg[i].row_scale = dyd.data_ptr(), xd.data_ptr(), (rsd.data_ptr() if rsd is not None else None)
        wg[i].dw, wg[i].dbias, wg[i].workspace, wg[i].ws_bytes = dw.data_ptr(), (db.data_ptr() if with_bias else None), ws.data_ptr(), nbytes
        wg[i].rows_per_sample, wg[i].M, wg[i].N, wg[i].K = rps, M, N_, K
        scale = np.ones((M, 1), np.float32) if rs is None else np.repeat(rs, rps)[:M, None] if M % 3 == 0 else None
        if scale is None:                                  # M not divisible by 3: build the per-row scale explicitly
            scale = np.array([rs[min(m // rps, 2)] for m in range(M)], np.float32)[:, None]
        refs.append((dw, db, (torch.from_numpy(dy * scale).T @ torch.from_numpy(x)), torch.from_numpy(dy * scale).sum(0)))
    call("cswin_linear_bwd_weight_batch", ctypes.cast(wg, ctypes.c_void_p), n, ctypes.cast(jobs, ctypes.c_void_p), None, 0, stream())
    call("cswin_rows_sum_multi", ctypes.cast(jobs, ctypes.c_void_p), n, stream())
    for i, (dw, db, dw_ref, db_ref) in enumerate(refs):
        rel_err(dw, dw_ref, f"wgrad_batch.{i}.dw")
        if db is not None:
            rel_err(db, db_ref, f"wgrad_batch.{i}.db")


@pytest.mark.parametrize("M,C", [(4704, 256), (784 * 3, 128), (300, 64), (1176, 512), (196, 96)])
def test_block_tail_launch_matches_the_two_launches(M, C):
    """cswin_linear_bwd_tail: the qkv data gradient in the weight-gradient batch's launch (gemm_block_tail_kernel) against
    cswin_linear_bwd_data followed by cswin_linear_bwd_weight_batch on the same operands: the weight gradients run the same
    configuration either way (bit-exact), the data gradient another tile shape (same products, other summation order)."""
    import ctypes
    from cswin_unet_amd._lib import ReduceJob, WgradDesc, call, lib, ptr, stream
    dqkv, wq = T(det_normal("tail.dqkv", (M, 3 * C))), T(det_normal("tail.wq", (3 * C, C), 1 / np.sqrt(C)))
    probs = [(T(det_normal("tail.dy0", (M, C))), T(det_normal("tail.x0", (M, 4 * C))), True),     # fc2
             (T(det_normal("tail.dy1", (M, 4 * C))), T(det_normal("tail.x1", (M, C))), True),     # fc1
             (T(det_normal("tail.dy2", (M, C))), T(det_normal("tail.x2", (M, C))), False),        # proj, no bias
             (dqkv, T(det_normal("tail.x3", (M, C))), True)]                                       # qkv
    rs = T(np.array([0.0, 1.25, 0.5, 1.0], np.float32))
    rps = (M + 3) // 4

    def run(merged):
        wg, jobs, keep, outs = (WgradDesc * 4)(), (ReduceJob * 4)(), [], []
        for i, (dy, x, with_bias) in enumerate(probs):
            N_, K = dy.shape[1], x.shape[1]
            dw, db = torch.empty(N_, K, device=DEV), (torch.empty(N_, device=DEV) if with_bias else None)
            nbytes = lib().cswin_linear_bwd_weight_workspace(M, N_, K)
            ws = torch.empty(nbytes // 4 + 4, device=DEV)
            keep.append(ws)
            wg[i].dy, wg[i].x, wg[i].row_scale = dy.data_ptr(), x.data_ptr(), (rs.data_ptr() if i == 0 else None)
            wg[i].dw, wg[i].dbias, wg[i].workspace, wg[i].ws_bytes = dw.data_ptr(), (db.data_ptr() if with_bias else None), ws.data_ptr(), nbytes
            wg[i].rows_per_sample, wg[i].M, wg[i].N, wg[i].K = rps, M, N_, K
            outs += [dw] + ([db] if with_bias else [])
        dx = torch.full((M, C), float("nan"), device=DEV)
        # three reductions left pending by "earlier" launches ride along: slabs of few rows (the weight-gradient form), of many
        # rows (LayerNorm dgamma / dbeta form, with a second output) and a short ragged one
        pend = (ReduceJob * 3)()
        pouts = []
        for k, (rows, n, nf) in enumerate(((6, 8192, 8192), (300, 512, 256), (5, 37, 37))):
            part, o1 = T(det_normal(f"tail.part{k}", (rows, n))), torch.full((nf,), float("nan"), device=DEV)
            o2 = torch.full((n - nf,), float("nan"), device=DEV) if n > nf else None
            pend[k].part, pend[k].out, pend[k].out2 = part.data_ptr(), o1.data_ptr(), (o2.data_ptr() if o2 is not None else None)
            pend[k].n_first, pend[k].n, pend[k].stride, pend[k].rows = nf, n, n, rows
            keep.append(part)
            pouts.append((part, o1, o2, nf))
        if merged:
            call("cswin_linear_bwd_tail", ptr(dqkv), ptr(wq), ptr(dx), M, 3 * C, C, ctypes.cast(wg, ctypes.c_void_p), 4,
                 ctypes.cast(jobs, ctypes.c_void_p), ctypes.cast(pend, ctypes.c_void_p), len(pend), stream())
        else:
            call("cswin_linear_bwd_data", ptr(dqkv), ptr(wq), ptr(dx), None, 0, None, None, 1, None, M, 3 * C, C, 0, 0, stream())
            call("cswin_linear_bwd_weight_batch", ctypes.cast(wg, ctypes.c_void_p), 4, ctypes.cast(jobs, ctypes.c_void_p), None, 0, stream())
            call("cswin_rows_sum_multi", ctypes.cast(pend, ctypes.c_void_p), 3, stream())
        call("cswin_rows_sum_multi", ctypes.cast(jobs, ctypes.c_void_p), 4, stream())
        torch.cuda.synchronize()
        for part, o1, o2, nf in pouts:
            ref = part.double().sum(0)
            assert _rel_l2(o1, ref[:nf]) < 1e-6 and (o2 is None or _rel_l2(o2, ref[nf:]) < 1e-6)
            outs += [o1] + ([o2] if o2 is not None else [])
        return dx, outs

    dx1, o1 = run(True)
    dx0, o0 = run(False)
    assert bool(torch.isfinite(dx1).all())
    assert _rel_l2(dx1, dx0) < 1e-6, _rel_l2(dx1, dx0)
    rel_err(dx1, (dqkv.double() @ wq.double()).float().cpu(), f"tail.dx.{M}x{C}")
    for a, b in zip(o1, o0):
        assert torch.equal(a, b)


@pytest.mark.parametrize("prec", [0, 1])
def test_weight_gradient_batch_carries_pending_reductions(prec):
    """`pending` of cswin_linear_bwd_weight_batch: reductions left by earlier launches run as the last workgroups of this launch's
    grid (fp32: gemm_block_tail_kernel without a data gradient; bf16 operands: wgrad16_kernel).  Same weight gradients as without
    riders, and the riders' outputs equal the column sums of their slabs."""
    import ctypes
    from cswin_unet_amd._lib import ReduceJob, WgradDesc, call, lib, stream
    M = 4704
    shapes = [(256, 1024), (768, 256)]
    dys = [T(det_normal(f"pend.dy{i}", (M, n_))) for i, (n_, k_) in enumerate(shapes)]
    xs = [T(det_normal(f"pend.x{i}", (M, k_))) for i, (n_, k_) in enumerate(shapes)]

    def run(with_pending):
        wg, jobs, keep, outs = (WgradDesc * 2)(), (ReduceJob * 2)(), [], []
        for i, (n_, k_) in enumerate(shapes):
            dw, db = torch.empty(n_, k_, device=DEV), torch.empty(n_, device=DEV)
            nbytes = lib().cswin_linear_bwd_weight_workspace(M, n_, k_)
            ws = torch.empty(nbytes // 4 + 4, device=DEV)
            keep.append(ws)
            wg[i].dy, wg[i].x, wg[i].dw, wg[i].dbias = dys[i].data_ptr(), xs[i].data_ptr(), dw.data_ptr(), db.data_ptr()
            wg[i].workspace, wg[i].ws_bytes, wg[i].rows_per_sample, wg[i].M, wg[i].N, wg[i].K, wg[i].precision = ws.data_ptr(), nbytes, 1, M, n_, k_, prec
            outs += [dw, db]
        pend, pouts = (ReduceJob * 3)(), []
        for k, (rows, n, nf) in enumerate(((9, 8192, 8192), (200, 512, 256), (3, 50, 50))):
            part, o1 = T(det_normal(f"pend.part{k}", (rows, n))), torch.full((nf,), float("nan"), device=DEV)
            o2 = torch.full((n - nf,), float("nan"), device=DEV) if n > nf else None
            pend[k].part, pend[k].out, pend[k].out2 = part.data_ptr(), o1.data_ptr(), (o2.data_ptr() if o2 is not None else None)
            pend[k].n_first, pend[k].n, pend[k].stride, pend[k].rows = nf, n, n, rows
            keep.append(part)
            pouts.append((part, o1, o2, nf))
        call("cswin_linear_bwd_weight_batch", ctypes.cast(wg, ctypes.c_void_p), 2, ctypes.cast(jobs, ctypes.c_void_p),
             ctypes.cast(pend, ctypes.c_void_p) if with_pending else None, 3 if with_pending else 0, stream())
        call("cswin_rows_sum_multi", ctypes.cast(jobs, ctypes.c_void_p), 2, stream())
        torch.cuda.synchronize()
        if with_pending:
            for part, o1, o2, nf in pouts:
                ref = part.double().sum(0)
                assert _rel_l2(o1, ref[:nf]) < 1e-6 and (o2 is None or _rel_l2(o2, ref[nf:]) < 1e-6)
        return outs

    for a, b in zip(run(True), run(False)):
        assert torch.equal(a, b)


def test_linear_concat_residual_droppath(ops):
    B, L, C = 3, 196, 256
    skip, x = det_normal("cl.skip", (B, L, C)), det_normal("cl.x", (B, L, C))
    w, b = det_normal("cl.w", (C, 2 * C), 1 / np.sqrt(2 * C)), det_normal("cl.b", (C,))
    res, dy = det_normal("cl.res", (B, L, C)), det_normal("cl.dy", (B, L, C))
    rs = np.array([0.0, 1.25, 1.25], np.float32)
    ref = [torch.from_numpy(a).requires_grad_() for a in (skip, x, w, b, res)]
    yr = ref[4] + torch.from_numpy(rs).view(-1, 1, 1) * torch.nn.functional.linear(torch.cat(ref[:2], -1), ref[2], ref[3])
    yr.backward(torch.from_numpy(dy))
    dev = [T(a, True) for a in (skip, x, w, b, res)]
    yd = ops.linear(dev[0], dev[2], dev[3], x2=dev[1], residual=dev[4], row_scale=T(rs))
    yd.backward(T(dy))
    rel_err(yd, yr, "concat_linear.y")
    for n, d, r in zip(("dskip", "dx", "dw", "db", "dres"), dev, ref):
        rel_err(d.grad, r.grad, "concat_linear." + n)


def test_mlp_fused(ops):
    B, L, C = 2, 784, 128
    x, res, dy = (det_normal("mlp." + n, (B, L, C)) for n in ("x", "res", "dy"))
    w1, b1 = det_normal("mlp.w1", (4 * C, C), 1 / np.sqrt(C)), det_normal("mlp.b1", (4 * C,), 0.1)
    w2, b2 = det_normal("mlp.w2", (C, 4 * C), 1 / np.sqrt(4 * C)), det_normal("mlp.b2", (C,), 0.1)
    rs = np.array([1.1111, 0.0], np.float32)
    ref = [torch.from_numpy(a).requires_grad_() for a in (x, w1, b1, w2, b2, res)]
    F = torch.nn.functional
    yr = ref[5] + torch.from_numpy(rs).view(-1, 1, 1) * F.linear(F.gelu(F.linear(ref[0], ref[1], ref[2])), ref[3], ref[4])
    yr.backward(torch.from_numpy(dy))
    dev = [T(a, True) for a in (x, w1, b1, w2, b2, res)]
    yd = ops.mlp(*dev[:5], residual=dev[5], row_scale=T(rs))
    yd.backward(T(dy))
    rel_err(yd, yr, "mlp.y")
    for n, d, r in zip(("dx", "dw1", "db1", "dw2", "db2", "dres"), dev, ref):
        rel_err(d.grad, r.grad, "mlp." + n)


@pytest.mark.parametrize("reso,idx,split,dim,heads", ATTN)
def test_attention_vs_golden(N, golden, reso, idx, split, dim, heads):
    g = golden("g2_attention")
    key = f"r{reso}_i{idx}_s{split}"
    L = reso * reso
    att = N.LePEAttention(dim, resolution=reso, idx=idx, split_size=split, num_heads=heads).to(DEV)
    fill_state_dict(att, prefix=f"attn.{key}.")
    q, k, v = (T(det_normal(f"attn.{key}.{n}", (2, L, dim)), True) for n in "qkv")
    y = att([q, k, v])
    y.backward(T(det_normal(f"attn.{key}.dy", (2, L, dim))))
    for name, t in [("y", y), ("dq", q.grad), ("dk", k.grad), ("dv", v.grad), ("dw", att.get_v.weight.grad),
                    ("db", att.get_v.bias.grad)]:
        err = check_packed(t, g, f"{key}.{name}.", RTOL, what="attention ")
        with open(LOG, "a") as f:
            f.write(f"attn_golden.{key}.{name}: {err:.3e}\n")


def test_integration_md_ctypes_stub_runs(N):
    """The reference-side stub of INTEGRATION.md (a maintainer's own ctypes binding of cswin_attn_fwd) is executed as written and
    must reproduce what the CSWinBlock's attention computes from the same qkv."""
    import re as _re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "INTEGRATION.md")).read()
    stub = [b for b in _re.findall(r"```python\n(.*?)```", text, flags=_re.S) if "lib.cswin_attn_fwd.argtypes" in b][0]
    stub = stub.replace('"cswin_unet_amd/libcswin_hip.so"', repr(os.path.join(root, "cswin_unet_amd", "libcswin_hip.so")))
    ns = {}
    exec(compile(stub, "INTEGRATION.md", "exec"), ns)
    blk = N.CSWinBlock(dim=128, reso=28, num_heads=4, split_size=2, qkv_bias=True, drop_path=0.).to(DEV)
    fill_state_dict(blk).eval()
    x = T(det_normal("stub.x", (2, 28 * 28, 128)))
    with torch.no_grad():
        qkv = blk.qkv(blk.norm1(x)).contiguous()                                   # (B, L, 3C), [q | k | v]
        y, y0, lse = ns["lepe_attention_both_branches"](qkv, [a.get_v for a in blk.attns], 28, 2, 4)
        q, k, v = qkv.reshape(2, -1, 3, 128).permute(2, 0, 1, 3)
        ref = torch.cat([blk.attns[0]([q[..., :64].contiguous(), k[..., :64].contiguous(), v[..., :64].contiguous()]),
                         blk.attns[1]([q[..., 64:].contiguous(), k[..., 64:].contiguous(), v[..., 64:].contiguous()])], dim=2)
    torch.cuda.synchronize()
    assert _rel_l2(y, ref) < 1e-6, _rel_l2(y, ref)
    assert bool(torch.isfinite(y0).all()) and bool(torch.isfinite(lse).all())


@pytest.mark.parametrize("reso,idx,split,dim,heads", ATTN384)
def test_attention_384_fwd_bwd_vs_golden(N, golden, reso, idx, split, dim, heads):
    """384x384 stripe shapes (N = 96, 288, 144): forward with online tiles over up to 18 key tiles, backward through the
    large-window two-pass path (delta pre-pass, dK/dV pass, dQ pass, LePE gradient pass) for N > 112."""
    g = golden("g2_attention")
    key = f"r{reso}_i{idx}_s{split}"
    L = reso * reso
    att = N.LePEAttention(dim, resolution=reso, idx=idx, split_size=split, num_heads=heads).to(DEV)
    fill_state_dict(att, prefix=f"attn.{key}.")
    q, k, v = (T(det_normal(f"attn.{key}.{n}", (2, L, dim)), True) for n in "qkv")
    y = att([q, k, v])
    y.backward(T(det_normal(f"attn.{key}.dy", (2, L, dim))))
    for name, t in [("y", y), ("dq", q.grad), ("dk", k.grad), ("dv", v.grad), ("dw", att.get_v.weight.grad),
                    ("db", att.get_v.bias.grad)]:
        err = check_packed(t, g, f"{key}.{name}.", RTOL, what="attention384 ")
        with open(LOG, "a") as f:
            f.write(f"attn384_golden.{key}.{name}: {err:.3e}\n")


@pytest.mark.parametrize("reso,idx,split,dim,heads", [(24, 1, 8, 64, 2), (16, -1, 16, 128, 4), (20, 1, 10, 64, 2), (24, 0, 6, 48, 2),
                                                      (56, 0, 1, 48, 2), (28, 1, 2, 96, 4), (14, 0, 7, 192, 8),
                                                        (7, -1, 7, 384, 16), (24, 1, 12, 192, 8), (28, 0, 2, 32, 2),
                                                        (14, 1, 7, 32, 4)])
def test_attention_other_head_dims_vs_oracle(N, reso, idx, split, dim, heads):
    """Head dims 24 (cswin_base: embed_dim 96), 16 and 8.  The reference cannot build these models (its decoder widths are
    hard-coded for embed_dim 64, cswin_unet.py:404-439), so this case is pinned against the oracle only."""
    key = f"hd.r{reso}_i{idx}_s{split}_c{dim}"
    L = reso * reso
    att = N.LePEAttention(dim, resolution=reso, idx=idx, split_size=split, num_heads=heads).to(DEV)
    fill_state_dict(att, prefix=f"attn.{key}.")
    qkv = [det_normal(f"attn.{key}.{n}", (2, L, dim)) for n in "qkv"]
    dy = det_normal(f"attn.{key}.dy", (2, L, dim))
    dev = [T(a, True) for a in qkv]
    y = att(dev)
    y.backward(T(dy))
    ref = [torch.from_numpy(a).requires_grad_() for a in qkv]
    w = att.get_v.weight.detach().cpu().clone().requires_grad_()
    b = att.get_v.bias.detach().cpu().clone().requires_grad_()
    yr = O.lepe_attention(*ref, w, b, reso, idx, split, heads)
    yr.backward(torch.from_numpy(dy))
    rel_err(y, yr, key + ".y")
    for n, d, r in zip(("dq", "dk", "dv"), dev, ref):
        rel_err(d.grad, r.grad, f"{key}.{n}")
    rel_err(att.get_v.weight.grad, w.grad, key + ".dw")
    rel_err(att.get_v.bias.grad, b.grad, key + ".db")


@pytest.mark.parametrize("dim,reso,heads,split,last", [(64, 56, 2, 1, False), (128, 28, 4, 2, False),
                                                        (256, 14, 8, 7, False), (512, 7, 16, 7, True)])
def test_block_vs_golden(N, golden, dim, reso, heads, split, last):
    g = golden("g3_blocks")
    key = f"c{dim}_r{reso}"
    blk = N.CSWinBlock(dim=dim, reso=reso, num_heads=heads, split_size=split, mlp_ratio=4., qkv_bias=True,
                       drop_path=0., last_stage=last).to(DEV)
    fill_state_dict(blk, prefix=f"block.{key}.")
    x = T(det_normal(f"block.{key}.x", (2, reso * reso, dim)), True)
    y = blk(x)
    y.backward(T(det_normal(f"block.{key}.dy", (2, reso * reso, dim))))
    check_packed(y, g, f"{key}.y.", RTOL, what="block ")
    check_packed(x.grad, g, f"{key}.dx.", RTOL, what="block ")
    for n, p in blk.named_parameters():
        err = check_packed(p.grad, g, f"{key}.grad.{n}.", RTOL, what=f"block {key} {n} ")
        with open(LOG, "a") as f:
            f.write(f"block_golden.{key}.{n}: {err:.3e}\n")


def test_block_droppath_injected_mask(N, monkeypatch):
    """DropPath parity with an injected per-sample mask (timm's RNG stream is unpinned)."""
    dim, reso, heads, split = 128, 28, 4, 2
    blk = N.CSWinBlock(dim=dim, reso=reso, num_heads=heads, split_size=split, qkv_bias=True, drop_path=0.25).to(DEV)
    fill_state_dict(blk, prefix="block.c128_r28.")
    blk.train()
    scales = [np.array([0.0, 4 / 3, 4 / 3], np.float32), np.array([4 / 3, 0.0, 4 / 3], np.float32)]
    it = iter(scales)
    monkeypatch.setattr(blk.drop_path, "sample_scale", lambda b, dev: T(next(it)))
    x = det_normal("dp.x", (3, reso * reso, dim))
    dy = det_normal("dp.dy", (3, reso * reso, dim))
    xd = T(x, True)
    yd = blk(xd)
    yd.backward(T(dy))
    P = {"b." + n: p.detach().cpu().clone().requires_grad_() for n, p in blk.named_parameters()}
    xr = torch.from_numpy(x).requires_grad_()

    class TwoScales:                      # oracle applies one keep_scale to both branches; emulate two draws
        pass
    F = torch.nn.functional
    h = F.layer_norm(xr, (dim,), P["b.norm1.weight"], P["b.norm1.bias"])
    qkv = F.linear(h, P["b.qkv.weight"], P["b.qkv.bias"])
    q, k, v = qkv.split(dim, -1)
    parts = [O.lepe_attention(q[..., s], k[..., s], v[..., s], P[f"b.attns.{i}.get_v.weight"], P[f"b.attns.{i}.get_v.bias"],
                              reso, i, split, heads // 2) for i, s in enumerate((slice(0, dim // 2), slice(dim // 2, dim)))]
    x1 = xr + torch.from_numpy(scales[0]).view(-1, 1, 1) * F.linear(torch.cat(parts, 2), P["b.proj.weight"], P["b.proj.bias"])
    h = F.layer_norm(x1, (dim,), P["b.norm2.weight"], P["b.norm2.bias"])
    h = F.linear(F.gelu(F.linear(h, P["b.mlp.fc1.weight"], P["b.mlp.fc1.bias"])), P["b.mlp.fc2.weight"], P["b.mlp.fc2.bias"])
    yr = x1 + torch.from_numpy(scales[1]).view(-1, 1, 1) * h
    yr.backward(torch.from_numpy(dy))
    rel_err(yd, yr, "droppath.y")
    rel_err(xd.grad, xr.grad, "droppath.dx")
    for n, p in blk.named_parameters():
        rel_err(p.grad, P["b." + n].grad, "droppath.grad." + n)


def test_patch_embed_grey_input_equals_repeated_channels(N):
    """A 1-channel image through the stem == the reference's x.repeat(1, 3, 1, 1) through it (vision_transformer.py:40-41): the
    repeat is folded into the kernel (weights summed over the input channel), output and every gradient agree to fp32
    summation-order noise."""
    stem = N._PatchEmbed(torch.nn.Conv2d(3, 64, 7, 4, 2), N.TokenRearrange(), torch.nn.LayerNorm(64)).to(DEV)
    fill_state_dict(stem, prefix="stem.stage1_conv_embed.")
    x = T(det_normal("stemgrey.x", (2, 1, 224, 224)))
    dy = T(det_normal("stemgrey.dy", (2, 56 * 56, 64)))
    outs = []
    for inp in (x, x.repeat(1, 3, 1, 1)):
        stem.zero_grad(set_to_none=True)
        y = stem(inp)
        y.backward(dy)
        outs.append([y.detach().clone()] + [p.grad.clone() for p in stem.parameters()])
    for n, a, b in zip(["y"] + [n for n, _ in stem.named_parameters()], *outs):
        assert _rel_l2(a, b) < 1e-5, (n, _rel_l2(a, b))


def test_patch_embed_vs_golden(N, golden):
    g = golden("g4_convs")
    stem = N._PatchEmbed(torch.nn.Conv2d(3, 64, 7, 4, 2), N.TokenRearrange(), torch.nn.LayerNorm(64)).to(DEV)
    fill_state_dict(stem, prefix="stem.stage1_conv_embed.")
    y = stem(T(det_normal("stem.x", (2, 3, 224, 224))))
    y.backward(T(det_normal("stem.dy", (2, 3136, 64))))
    check_packed(y, g, "stem.y.", RTOL)
    for n, p in stem.named_parameters():
        check_packed(p.grad, g, f"stem.grad.{n}.", RTOL, what=n + " ")


def _run_module_vs_golden(mod, key, in_shape, out_shape, g):
    mod = mod.to(DEV)
    fill_state_dict(mod, prefix=key + ".")
    x = T(det_normal(key + ".x", in_shape), True)
    y = mod(x)
    assert tuple(y.shape) == tuple(out_shape)
    y.backward(T(det_normal(key + ".dy", out_shape)))
    errs = {"y": check_packed(y, g, key + ".y.", RTOL, what=key + " "),
            "dx": check_packed(x.grad, g, key + ".dx.", RTOL, what=key + " ")}
    for n, p in mod.named_parameters():
        errs[n] = check_packed(p.grad, g, f"{key}.grad.{n}.", RTOL, what=f"{key} {n} ")
    with open(LOG, "a") as f:
        for n, e in errs.items():
            f.write(f"{key}.{n}: {e:.3e}\n")


@pytest.mark.parametrize("i,c,r", [(1, 64, 56), (2, 128, 28), (3, 256, 14)])
def test_merge_vs_golden(N, golden, i, c, r):
    _run_module_vs_golden(N.Merge_Block(c, 2 * c), f"merge{i}", (2, r * r, c), (2, r * r // 4, 2 * c), golden("g4_convs"))


@pytest.mark.parametrize("name,c,cout,r,S,B", [("upsample4", 512, 256, 7, 2, 2), ("upsample3", 256, 128, 14, 2, 2),
                                               ("upsample2", 128, 64, 28, 2, 2), ("upsample1", 64, 64, 56, 4, 2),
                                               ("carafe4_small", 16, 8, 5, 4, 1), ("carafe2_small", 16, 8, 6, 2, 1)])
def test_carafe_vs_golden(N, golden, name, c, cout, r, S, B):
    mod = N.CARAFE(c, cout) if S == 2 else N.CARAFE4(c, cout)
    _run_module_vs_golden(mod, name, (B, r * r, c), (B, S * S * r * r, cout), golden("g4_convs"))


@pytest.mark.parametrize("H,S,Cz,B", [(16, 4, 16, 3), (12, 4, 16, 2), (8, 4, 32, 2), (7, 2, 96, 2), (14, 2, 256, 1), (24, 4, 16, 1)])
def test_carafe_reassembly_paths_vs_closed_form(ops, H, S, Cz, B):
    """ops.carafe_reassemble forward / backward against the closed form (softmax over the 9 taps, 3x3 neighbourhood gather of z,
    zero outside the map): H = 16 / 24 with S = 4, Cz = 16 take the fused 8x8-tile MFMA backward, H = 12 (not a multiple of 8)
    and Cz = 32 the generic kernels, S = 2 with Cz = 96 / 256 the generic kernels with one and two 16-B chunks per lane (the
    column sums of dout ride along in the de kernel)."""
    e = det_normal("cr.e", (B, H * H, 9 * S * S))
    z = det_normal("cr.z", (B, H * H, Cz))
    bias = det_normal("cr.b", (Cz,), 0.1)
    dout = det_normal("cr.dout", (B, S * S * H * H, Cz))
    er, zr, br = (torch.from_numpy(a).requires_grad_() for a in (e, z, bias))
    wt = torch.softmax(er.view(B, H, H, 9, S * S), dim=3)                                  # (B, H, W, k, s)
    zp = torch.nn.functional.pad(zr.view(B, H, H, Cz), (0, 0, 1, 1, 1, 1))
    up = 0
    for kk in range(9):
        ky, kx = divmod(kk, 3)
        up = up + wt[:, :, :, kk, :, None] * zp[:, ky:ky + H, kx:kx + H, None, :]          # (B, H, W, s, C)
    out_r = up.view(B, H, H, S, S, Cz).permute(0, 1, 3, 2, 4, 5).reshape(B, S * S * H * H, Cz) + br
    out_r.backward(torch.from_numpy(dout))
    ed, zd, bd = T(e, True), T(z, True), T(bias, True)
    out_d = ops.carafe_reassemble(ed, zd, bd, H, H, S)
    out_d.backward(T(dout))
    tag = f"carafe_paths.H{H}S{S}C{Cz}"
    rel_err(out_d, out_r, tag + ".out")
    rel_err(ed.grad, er.grad, tag + ".de")
    rel_err(zd.grad, zr.grad, tag + ".dz")
    rel_err(bd.grad, br.grad, tag + ".dbias")


def test_loss_vs_oracle(ops):
    B, C, H = 3, 9, 64
    logits = det_normal("loss.logits", (B, C, H, H), 2.0)
    lab = det_labels("loss.lab", (B, H, H), C)
    lr = torch.from_numpy(logits).requires_grad_()
    loss_r, ce_r, dice_r = O.ce_dice_loss(lr, torch.from_numpy(lab), C)
    (loss_r * 1.7).backward()
    ld = T(logits, True)
    loss_d, stats = ops.ce_dice_loss(ld, T(lab))
    (loss_d * 1.7).backward()
    assert abs(float(loss_d) - float(loss_r)) < 1e-4 * abs(float(loss_r))
    assert abs(float(stats[1]) - float(ce_r)) < 1e-4 and abs(float(stats[2]) - float(dice_r)) < 1e-4
    rel_err(ld.grad, lr.grad, "loss.dlogits")


def _golden_model(N, drop_path=0.):
    net = N.CSWinTransformer(img_size=224, num_classes=9, embed_dim=64, depth=[1, 2, 9, 1], split_size=[1, 2, 7, 7],
                             num_heads=[2, 4, 8, 16], mlp_ratio=4., qkv_bias=True, drop_path_rate=drop_path).to(DEV)
    return fill_state_dict(net)


def test_full_model_vs_golden(N, ops, golden):
    g = golden("g5_model")
    from cswin_unet_amd.optim import FlatSGD
    net = _golden_model(N)
    net.train()
    img = T(det_normal("model.x", (2, 1, 224, 224))).repeat(1, 3, 1, 1)
    lab = T(det_labels("model.labels", (2, 224, 224), 9))
    opt = FlatSGD(net.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4)
    losses = []
    for it in range(3):
        logits = net(img)
        loss, stats = ops.ce_dice_loss(logits, lab)
        opt.zero_grad()
        loss.backward()
        if it == 0:
            check_packed(logits, g, "logits.", RTOL, what="model ")
            assert abs(float(stats[1]) - float(g["loss_ce"])) < 1e-3 * float(g["loss_ce"])
            assert abs(float(stats[2]) - float(g["loss_dice"])) < 1e-3 * float(g["loss_dice"])
            params = dict(net.named_parameters())
            with open(LOG, "a") as f:
                for m in [k[len("gradnorm."):] for k in g.files if k.startswith("gradnorm.")]:
                    sq = sum(float((p.grad.double() ** 2).sum()) for n, p in params.items() if n.startswith(m + "."))
                    ref = float(g["gradnorm." + m])
                    f.write(f"model.gradnorm.{m}: {abs(np.sqrt(sq) - ref) / ref:.3e}\n")
                    assert abs(np.sqrt(sq) - ref) <= RTOL * ref, (m, np.sqrt(sq), ref)
            for k in sorted({k[len("grad."):].rsplit(".", 1)[0] for k in g.files if k.startswith("grad.")}):
                check_packed(params[k].grad, g, f"grad.{k}.", RTOL, what=k + " ")
        opt.step()
        opt.set_lr(O.poly_lr(0.05, it, 100))              # trainer.py:61-63: schedule applied after the step
        losses.append(float(loss))
    assert np.allclose(losses, g["sgd_losses"], rtol=2e-3), (losses, g["sgd_losses"])
    chk = sum(float(p.detach().double().abs().sum()) for p in net.parameters())
    assert abs(chk - float(g["sgd_weight_checksum"])) <= 1e-4 * float(g["sgd_weight_checksum"])


def test_eval_argmax_vs_golden(N, golden):
    g = golden("g6_eval")
    net = _golden_model(N).eval()
    with torch.no_grad():
        logits = net(T(det_normal("model.x", (2, 1, 224, 224))).repeat(1, 3, 1, 1))
    check_packed(logits, g, "logits.", RTOL, what="eval ")
    agree = (logits.argmax(1).cpu().numpy().astype(np.uint8) == g["argmax"]).mean()
    assert agree >= 0.999, agree            # "Dice vs ref": identical segmentation map


def test_model_384_forward_vs_golden(N, golden):
    net = N.CSWinTransformer(img_size=384, num_classes=9, embed_dim=64, depth=[1, 2, 9, 1], split_size=[1, 2, 12, 12],
                             num_heads=[2, 4, 8, 16], qkv_bias=True).to(DEV)
    fill_state_dict(net).eval()
    with torch.no_grad():
        logits = net(T(det_normal("model384.x", (1, 3, 384, 384))))
    check_packed(logits, golden("g7_model384"), "logits.", RTOL, what="model384 ")


def test_full_size_properties(N, ops):
    """BASELINE sizes (B=24): size-independent properties instead of an oracle run.
    * attention is linear in V (and in the LePE bias-free part): f(q,k,a v1 + b v2) = a f(v1) + b f(v2) with bias 0
    * softmax rows sum to one: with V = const and LePE = 0 the output is that constant
    * img2windows -> windows2img is the identity (bit-exact)."""
    B, reso, dim, heads, split = 24, 14, 256, 8, 7
    L = reso * reso
    g = torch.Generator(device="cpu").manual_seed(1234)
    qkv1 = torch.randn(B, L, 3 * dim, generator=g).to(DEV)
    qkv2 = qkv1.clone()
    qkv2[..., 2 * dim:] = torch.randn(B, L, dim, generator=g).to(DEV)
    w = [torch.randn(dim // 2, 1, 3, 3, generator=g).to(DEV) for _ in range(2)]
    zb = [torch.zeros(dim // 2, device=DEV) for _ in range(2)]
    f = lambda t: ops.stripe_attention(t, reso, split, [0, 1], [heads // 2] * 2, w, zb)
    mix = qkv1.clone()
    mix[..., 2 * dim:] = 0.75 * qkv1[..., 2 * dim:] - 1.5 * qkv2[..., 2 * dim:]
    rel_err(f(mix), 0.75 * f(qkv1) - 1.5 * f(qkv2), "prop.attn_linear_in_v")
    const = qkv1.clone()
    const[..., 2 * dim:] = 3.25
    zw = [torch.zeros_like(t) for t in w]
    out = ops.stripe_attention(const, reso, split, [0, 1], [heads // 2] * 2, zw, zb)
    rel_err(out, torch.full_like(out, 3.25), "prop.softmax_rows_sum_to_one")
    img = torch.randn(B, 64, 56, 56, generator=g).to(DEV)
    for hs, ws in ((56, 1), (1, 56), (7, 7)):
        assert torch.equal(N.windows2img(N.img2windows(img, hs, ws), hs, ws, 56, 56), img.permute(0, 2, 3, 1))


@pytest.mark.parametrize("use_graph", [False, True])
def test_trainer_three_steps_vs_golden(N, golden, use_graph):
    """The product training step (HipEngine: fused loss, two-phase backward, flat SGD, hipGraphs when use_graph) reproduces
    the reference's 3-step SGD loss trajectory and weight checksum (golden g5; drop_path 0)."""
    from cswin_unet_amd.trainer import DataParallelTrainer
    g = golden("g5_model")
    net = _golden_model(N)
    net.train()
    img = T(det_normal("model.x", (2, 1, 224, 224))).repeat(1, 3, 1, 1)
    lab = T(det_labels("model.labels", (2, 224, 224), 9))
    tr = DataParallelTrainer(net, 9, base_lr=0.05, max_iterations=100, use_graph=use_graph)
    assert tr.engine.split_backward and 0 < tr.engine.n_enc < len(tr.engine.opt.params)
    losses = [float(tr.train_step(img, lab)[0]) for _ in range(3)]
    assert np.allclose(losses, g["sgd_losses"], rtol=2e-3), (losses, g["sgd_losses"])
    chk = sum(float(p.detach().double().abs().sum()) for p in net.parameters())
    assert abs(chk - float(g["sgd_weight_checksum"])) <= 1e-4 * float(g["sgd_weight_checksum"])


def test_bf16_mode_training_tracks_fp32(N):
    """BASELINE's metric pairs the throughput with "Dice vs ref": 25 SGD steps on a learnable synthetic task (the label of a pixel
    is a function of its intensity) with the product trainer, once in fp32 and once in the bf16 mode (bf16 MFMAs incl. attention,
    bf16 activation storage, weight shadow), same initial weights and data.  Both must learn (loss and the Dice term fall), and
    the bf16 trajectory must stay within 1 % of the fp32 one at every step (measured: 0.3 %)."""
    import cswin_unet_amd
    from cswin_unet_amd.trainer import DataParallelTrainer
    torch.manual_seed(0)
    img = torch.randn(4, 1, 224, 224, device=DEV)
    img = torch.nn.functional.avg_pool2d(img, 9, 1, 4)                      # smooth blobs
    lab = torch.bucketize(img[:, 0], torch.tensor([-0.15, -0.05, 0.05, 0.15], device=DEV)).long()     # 5 classes by intensity
    img3 = img.repeat(1, 3, 1, 1) * 5
    traj = {}
    for mode in ("fp32", "bf16"):
        prev = cswin_unet_amd.set_matmul_precision(mode)
        try:
            net = N.CSWinTransformer(img_size=224, num_classes=9, embed_dim=64, depth=[1, 2, 2, 1], split_size=[1, 2, 7, 7],
                                     num_heads=[2, 4, 8, 16], qkv_bias=True, drop_path_rate=0.).to(DEV)
            fill_state_dict(net).train()
            tr = DataParallelTrainer(net, 9, base_lr=0.05, max_iterations=1000, use_graph=True)
            traj[mode] = np.array([[float(v) for v in tr.train_step(img3, lab)] for _ in range(25)])
        finally:
            cswin_unet_amd.set_matmul_precision(prev)
    f, b = traj["fp32"], traj["bf16"]
    with open(LOG, "a") as fh:
        fh.write(f"bf16_tracks_fp32: loss fp32 {f[0, 0]:.4f} -> {f[-1, 0]:.4f}, bf16 {b[0, 0]:.4f} -> {b[-1, 0]:.4f}; "
                 f"dice fp32 {f[0, 2]:.4f} -> {f[-1, 2]:.4f}, bf16 {b[0, 2]:.4f} -> {b[-1, 2]:.4f}; max rel dev {np.abs(b[:, 0] / f[:, 0] - 1).max():.3e}\n")
    assert f[-1, 0] < 0.8 * f[0, 0] and b[-1, 0] < 0.8 * b[0, 0], (f[:, 0], b[:, 0])
    assert f[-1, 2] < f[0, 2] and b[-1, 2] < b[0, 2]
    assert np.abs(b[:, 0] / f[:, 0] - 1).max() < 1e-2, np.abs(b[:, 0] / f[:, 0] - 1)


def test_trainer_rccl_path_single_rank(N, golden):
    """Same trajectory with the collectives actually issued (1-rank RCCL group: all-reduce is the identity): exercises the
    broadcast, the 28-float loss all-reduce between the hipGraphs and the per-phase bucketed gradient all-reduces."""
    import torch.distributed as dist
    from cswin_unet_amd.trainer import DataParallelTrainer
    g = golden("g5_model")
    if not dist.is_initialized():
        dist.init_process_group("nccl", init_method="tcp://127.0.0.1:29531", rank=0, world_size=1)
    try:
        net = _golden_model(N)
        net.train()
        img = T(det_normal("model.x", (2, 1, 224, 224))).repeat(1, 3, 1, 1)
        lab = T(det_labels("model.labels", (2, 224, 224), 9))
        tr = DataParallelTrainer(net, 9, base_lr=0.05, max_iterations=100, group=dist.group.WORLD, force_collectives=True)
        assert tr.collectives
        losses = [float(tr.train_step(img, lab)[0]) for _ in range(3)]
        assert np.allclose(losses, g["sgd_losses"], rtol=2e-3), (losses, g["sgd_losses"])
        # bf16 gradients on the wire (BASELINE configs[2]): convert / all-reduce / convert back per bucket on the RCCL path
        net2 = _golden_model(N)
        net2.train()
        tr2 = DataParallelTrainer(net2, 9, base_lr=0.05, max_iterations=100, group=dist.group.WORLD, force_collectives=True,
                                  allreduce_dtype=torch.bfloat16)
        losses2 = [float(tr2.train_step(img, lab)[0]) for _ in range(3)]
        assert abs(losses2[0] - g["sgd_losses"][0]) < 2e-3 * g["sgd_losses"][0]
        assert np.allclose(losses2, g["sgd_losses"], rtol=3e-2), (losses2, g["sgd_losses"])
    finally:
        dist.destroy_process_group()


def test_model_384_training_step_vs_oracle(N, ops, golden):
    """BASELINE configs[3] shape (384x384, split [1,2,12,12]) end to end at B=1: logits vs the reference golden, loss and a
    sample of parameter gradients vs the CPU oracle (backward goes through the large-window attention path)."""
    cfg = dict(O.TINY_224, img_size=384, split_size=(1, 2, 12, 12))
    net = N.CSWinTransformer(img_size=384, num_classes=9, embed_dim=64, depth=[1, 2, 9, 1], split_size=[1, 2, 12, 12],
                             num_heads=[2, 4, 8, 16], qkv_bias=True).to(DEV)
    fill_state_dict(net).train()
    img = det_normal("model384.x", (1, 3, 384, 384))
    lab = det_labels("model384.lab", (1, 384, 384), 9)
    logits = net(T(img))
    check_packed(logits, golden("g7_model384"), "logits.", RTOL, what="model384 ")
    loss, _ = ops.ce_dice_loss(logits, T(lab))
    loss.backward()
    P = O.golden_params(cfg)
    ref_loss, _, _ = O.ce_dice_loss(O.cswin_forward(P, torch.from_numpy(img), cfg), torch.from_numpy(lab))
    ref_loss.backward()
    assert abs(float(loss) - float(ref_loss)) < 1e-3 * abs(float(ref_loss))
    params = dict(net.named_parameters())
    for n in ["stage3.4.qkv.weight", "stage3.4.attns.1.get_v.weight", "stage4.0.attns.0.get_v.bias", "stage_up3.2.proj.weight",
              "stage1_conv_embed.0.weight", "merge2.conv.weight", "upsample1.encoder.weight", "output.weight"]:
        rel_err(params[n].grad, P[n].grad, "model384.grad." + n)


def test_model_base_width_training_step_vs_oracle(N, ops):
    """cswin_base widths (embed_dim 96 -> channels 96/192/384/768, head dim 24, heads [4,8,16,32]) with a short depth, one
    training step at B=2 vs the CPU oracle.  Exercises the generic-C LayerNorm, head-dim-24 attention, CARAFE with
    Cz/4 not a power of two and GEMMs with K, N multiples of 96.  Pinned against the oracle only: the reference model
    cannot be constructed for embed_dim != 64 (cswin_unet.py:404-439 hard-code the decoder widths)."""
    cfg = dict(O.TINY_224, embed_dim=96, depth=(1, 2, 2, 1), num_heads=(4, 8, 16, 32))
    net = N.CSWinTransformer(img_size=224, num_classes=9, embed_dim=96, depth=[1, 2, 2, 1], split_size=[1, 2, 7, 7],
                             num_heads=[4, 8, 16, 32], qkv_bias=True).to(DEV)
    fill_state_dict(net).train()
    img = det_normal("modelbase.x", (2, 3, 224, 224))
    lab = det_labels("modelbase.lab", (2, 224, 224), 9)
    logits = net(T(img))
    loss, _ = ops.ce_dice_loss(logits, T(lab))
    loss.backward()
    P = O.golden_params(cfg)
    ref_logits = O.cswin_forward(P, torch.from_numpy(img), cfg)
    ref_loss, _, _ = O.ce_dice_loss(ref_logits, torch.from_numpy(lab))
    ref_loss.backward()
    rel_err(logits, ref_logits, "modelbase.logits")
    assert abs(float(loss) - float(ref_loss)) < 1e-3 * abs(float(ref_loss))
    params = dict(net.named_parameters())
    assert set(params) == set(P)
    for n in params:
        rel_err(params[n].grad, P[n].grad, "modelbase.grad." + n)


def test_dice_loss_module_vs_oracle(golden):
    """utils.DiceLoss(n)(logits, target, softmax=True) (reference utils.py:9-45) on the fused loss kernels."""
    from cswin_unet_amd.utils import DiceLoss
    logits = det_normal("dl.logits", (3, 9, 64, 64), 2.0)
    lab = det_labels("dl.lab", (3, 64, 64), 9)
    x = T(logits, True)
    loss = DiceLoss(9)(x, T(lab), softmax=True)
    loss.backward()
    xr = torch.from_numpy(logits).requires_grad_()
    ref = O.dice_from_sums(O.dice_sums(xr, torch.from_numpy(lab), 9))
    ref.backward()
    assert abs(float(loss) - float(ref)) < 1e-5 * abs(float(ref))
    rel_err(x.grad, xr.grad, "dice_loss.dlogits")


def test_volume_inference_vs_reference_argmax(N, golden):
    """test_single_volume slice loop (reference utils.py:61-102) with the real network: the predicted label volume must be
    the reference's eval-mode argmax map (g6)."""
    from cswin_unet_amd.utils import predict_volume, test_single_volume
    g = golden("g6_eval")
    net = _golden_model(N).eval()

    class OneChannel(torch.nn.Module):          # CSwinUnet.forward: 1 -> 3 channels (vision_transformer.py:40-41)
        def __init__(self, m):
            super().__init__()
            self.m = m

        def forward(self, x):
            return self.m(x.repeat(1, 3, 1, 1))

    vol = det_normal("model.x", (2, 1, 224, 224))[:, 0]
    pred = predict_volume(vol, OneChannel(net), (224, 224), batch_slices=2)
    assert (pred.astype(np.uint8) == g["argmax"]).mean() >= 0.999
    m = test_single_volume(torch.from_numpy(vol)[None], torch.from_numpy(g["argmax"].astype(np.int64))[None], OneChannel(net),
                           classes=9, patch_size=[224, 224])
    assert len(m) == 8 and all(d >= 0.999 or d == 0 for d, _ in m)


def test_trainer_synapse_on_synthetic_dataset(N, tmp_path):
    """trainer_synapse (reference trainer.py:20-95) end to end on a schema-conformant synthetic dataset: loss decreases,
    checkpoint in the reference format is written and loads back."""
    from types import SimpleNamespace
    from cswin_unet_amd.checkpoint import load_checkpoint
    from cswin_unet_amd.config import get_config
    from cswin_unet_amd.datasets import write_synthetic_synapse
    from cswin_unet_amd.networks.vision_transformer import CSwinUnet
    from cswin_unet_amd.trainer import trainer_synapse
    train, _, lists = write_synthetic_synapse(str(tmp_path / "data"), n_slices=8, n_volumes=0, size=256)
    cfg = get_config(**{"MODEL.DROP_PATH_RATE": 0.0})
    torch.manual_seed(0)
    net = CSwinUnet(cfg, img_size=224, num_classes=9).to(DEV)
    args = SimpleNamespace(root_path=train, list_dir=lists, img_size=224, num_classes=9, batch_size=4, base_lr=0.05,
                           max_epochs=3, num_workers=0, seed=1234)
    import logging
    records = []
    h = logging.Handler()
    h.emit = lambda r: records.append(r.getMessage())
    root = logging.getLogger()
    old_level = root.level
    root.setLevel(logging.INFO)
    root.addHandler(h)
    try:
        assert trainer_synapse(args, net, str(tmp_path / "snap")) == "Training Finished!"
    finally:
        root.removeHandler(h)
        root.setLevel(old_level)
    losses = [float(m.split("loss : ")[1].split(",")[0]) for m in records if m.startswith("iteration")]
    assert len(losses) == 6 and losses[-1] < losses[0]
    ck = tmp_path / "snap" / "epoch_2.pth"
    assert ck.exists()
    other = CSwinUnet(cfg, img_size=224, num_classes=9)
    msg = load_checkpoint(other, str(ck))
    assert not msg.missing_keys and not msg.unexpected_keys


@pytest.mark.parametrize("ncls,B", [(4, 1), (3, 3)])
def test_model_other_class_counts_and_batches_vs_oracle(N, ops, ncls, B):
    """KiTS / LiTS class counts of the reference's dataset table (train.py:88-103: 4 and 3 classes) and odd batch sizes:
    logits, loss and every parameter gradient of one training step vs the CPU oracle (short depth to keep the oracle fast)."""
    cfg = dict(O.TINY_224, depth=(1, 1, 2, 1), num_classes=ncls)
    net = N.CSWinTransformer(img_size=224, num_classes=ncls, embed_dim=64, depth=[1, 1, 2, 1], split_size=[1, 2, 7, 7],
                             num_heads=[2, 4, 8, 16], qkv_bias=True).to(DEV)
    fill_state_dict(net).train()
    img = det_normal(f"modelc{ncls}.x", (B, 3, 224, 224))
    lab = det_labels(f"modelc{ncls}.lab", (B, 224, 224), ncls)
    logits = net(T(img))
    loss, _ = ops.ce_dice_loss(logits, T(lab))
    loss.backward()
    P = O.golden_params(cfg)
    ref_logits = O.cswin_forward(P, torch.from_numpy(img), cfg)
    ref_loss, _, _ = O.ce_dice_loss(ref_logits, torch.from_numpy(lab), ncls)
    ref_loss.backward()
    rel_err(logits, ref_logits, f"modelc{ncls}.logits")
    assert abs(float(loss) - float(ref_loss)) < 1e-3 * abs(float(ref_loss))
    params = dict(net.named_parameters())
    assert set(params) == set(P)
    for n in params:
        rel_err(params[n].grad, P[n].grad, f"modelc{ncls}.grad." + n)


# ---------------------------------------------------------------------------------------------------------------------
# bf16-operand matmul mode (BASELINE configs[2..4] name bf16).  Same fp32 oracle, looser STATED bound: operands are rounded
# to 8 mantissa bits (relative 2^-9 each), products accumulate in fp32; observed max|diff|/rms is ~5e-3 per GEMM.
# ---------------------------------------------------------------------------------------------------------------------
BF16_RTOL = 3e-2


@pytest.fixture()
def bf16_matmul():
    import cswin_unet_amd
    prev = cswin_unet_amd.set_matmul_precision("bf16")
    yield
    cswin_unet_amd.set_matmul_precision(prev)


def _rel(got, ref):
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    return float((got - ref).abs().max()) / (float(ref.pow(2).mean().sqrt()) + 1e-30)


@pytest.mark.parametrize("M,Nn,K", [(4704, 768, 256), (1176, 512, 2048), (3000, 64, 64), (777, 130, 100)])
def test_linear_bf16_operands(ops, bf16_matmul, M, Nn, K):
    x, w, b = det_normal("lb.x", (M, K)), det_normal("lb.w", (Nn, K), 1 / np.sqrt(K)), det_normal("lb.b", (Nn,), 0.1)
    dy = det_normal("lb.dy", (M, Nn))
    xr, wr, br = (torch.from_numpy(a).requires_grad_() for a in (x, w, b))
    yr = torch.nn.functional.linear(xr, wr, br)
    yr.backward(torch.from_numpy(dy))
    xd, wd, bd = T(x, True), T(w, True), T(b, True)
    yd = ops.linear(xd, wd, bd)
    yd.backward(T(dy))
    errs = {"y": _rel(yd, yr), "dx": _rel(xd.grad, xr.grad), "dw": _rel(wd.grad, wr.grad), "db": _rel(bd.grad, br.grad)}
    with open(LOG, "a") as f:
        f.write(f"linear_bf16 M{M} N{Nn} K{K}: {errs}\n")
    assert all(np.isfinite(e) and e < BF16_RTOL for e in errs.values()), errs
    assert errs["y"] > 1e-5          # the bf16 path really ran (fp32 MFMA would be ~1e-6)


def _rel_l2(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).pow(2).sum().sqrt() / (ref.pow(2).sum().sqrt() + 1e-300))


# Derived bf16 bounds.  One GEMM with both operands rounded to bf16 (RNE: relative error uniform in +-2^-9, sigma 2^-9 / sqrt 3)
# has a relative L2 error of sqrt(2) * 2^-9 / sqrt(3) = 1.6e-3.  A forward pass chains ~60 such contractions (26 blocks x 4 Linears
# behind residual connections that dilute each contribution) and a gradient ~120; independent errors add in quadrature:
# 1.6e-3 * sqrt(60) = 1.2e-2 for the logits, 1.6e-3 * sqrt(120) = 1.8e-2 for a gradient.  Bounds = 2.5x those (LayerNorm rescaling
# and the softmax make some links amplify): logits 3e-2, gradients 5e-2 in relative L2 (measured: 1.2e-2 and 0.7 - 1.9e-2).  The
# elementwise maximum of the logits over ~1e6 elements sits 5 - 6 sigma out (bound 6x the L2 one; measured 6.9e-2); parameter
# gradients are heavy-tailed (elements of many times the RMS carry proportionally larger absolute errors), so for them only the
# L2 bound is meaningful.
BF16_LOGITS_L2, BF16_GRAD_L2 = 3e-2, 5e-2


def test_model_bf16_operands_training_step(N, ops, golden, bf16_matmul):
    """Whole model, one step, bf16 GEMM / conv operands against the fp32 reference outputs (g5: strided samples of the reference
    tensors), relative L2 over the samples and elementwise maximum, with the derived bounds above; the loss within 1 %."""
    g = golden("g5_model")
    net = _golden_model(N).train()
    x = T(det_normal("model.x", (2, 1, 224, 224))).repeat(1, 3, 1, 1)
    lab = T(det_labels("model.labels", (2, 224, 224), 9))
    logits = net(x)

    def packed_err(t, prefix):
        a = t.detach().float().cpu().numpy().reshape(-1)
        ref, stride = g[prefix + "vals"], int(g[prefix + "stride"])
        rms = float(np.sqrt(float(g[prefix + "sqsum"]) / a.size)) + 1e-30
        d = a[::stride].astype(np.float64) - ref
        l2, mx = float(np.sqrt(np.mean(d * d))) / rms, float(np.abs(d).max()) / rms
        with open(LOG, "a") as f:
            f.write(f"model_bf16.{prefix} l2 {l2:.3e} max {mx:.3e}\n")
        return l2, mx

    l2, mx = packed_err(logits, "logits.")
    assert 1e-4 < l2 < BF16_LOGITS_L2 and mx < 6 * BF16_LOGITS_L2, (l2, mx)
    loss, stats = ops.ce_dice_loss(logits, lab)
    assert abs(float(loss) - float(g["loss"])) < 1e-2 * abs(float(g["loss"]))
    loss.backward()
    params = dict(net.named_parameters())
    for n in ["stage3.4.qkv.weight", "merge2.conv.weight", "upsample1.encoder.weight", "output.weight", "concat_linear3.weight"]:
        l2, mx = packed_err(params[n].grad, f"grad.{n}.")
        assert l2 < BF16_GRAD_L2, (n, l2, mx)


def _bf16_step_vs_oracle(N, ops, cfg, net, img, lab, tag, grads):
    logits = net(T(img))
    loss, _ = ops.ce_dice_loss(logits, T(lab))
    loss.backward()
    P = O.golden_params(cfg)
    ref_logits = O.cswin_forward(P, torch.from_numpy(img), cfg)
    ref_loss, _, _ = O.ce_dice_loss(ref_logits, torch.from_numpy(lab))
    ref_loss.backward()
    e = _rel_l2(logits, ref_logits)
    with open(LOG, "a") as f:
        f.write(f"{tag}.logits l2 {e:.3e}\n")
    assert 1e-4 < e < BF16_LOGITS_L2, e
    assert abs(float(loss) - float(ref_loss)) < 1e-2 * abs(float(ref_loss))
    params = dict(net.named_parameters())
    for n in grads:
        e = _rel_l2(params[n].grad, P[n].grad)
        with open(LOG, "a") as f:
            f.write(f"{tag}.grad.{n} l2 {e:.3e}\n")
        assert e < BF16_GRAD_L2, (n, e)


@pytest.mark.parametrize("M,Nn,K", [(4704, 768, 256), (1176, 512, 2048), (3000, 64, 64), (100, 72, 64), (37, 8, 128), (160, 200, 192), (1000, 288, 96), (333, 96, 32)])
def test_linear_bf16_storage_flags_bit_exact(M, Nn, K):
    """io_bf16 of cswin_linear_fwd / cswin_linear_bwd_data / cswin_wgrad_desc (include/cswin_hip.h): a tensor STORED as bf16 must
    give bit-identical results to the same values held in fp32 (the operands are rounded to bf16 either way, and a bf16 -> fp32
    -> bf16 round trip is exact), and an OUTPUT stored as bf16 must equal the fp32 output rounded to nearest even."""
    import ctypes
    from cswin_unet_amd._lib import ReduceJob, WgradDesc, call, lib, ptr, stream
    x16 = T(det_normal("st16.x", (M, K))).bfloat16()
    dy16 = T(det_normal("st16.dy", (M, Nn))).bfloat16()
    w16 = T(det_normal("st16.w", (Nn, K)) * 0.05).bfloat16()           # the weights' bf16 shadow (io bit 2) ...
    w, b = w16.float(), T(det_normal("st16.b", (Nn,)))                  # ... and fp32 master weights holding the same values
    x32, dy32 = x16.float(), dy16.float()
    E = lambda *sh, dt=torch.float32: torch.empty(*sh, dtype=dt, device=DEV)
    eq = lambda a, c: bool((a.view(torch.int16) == c.view(torch.int16)).all()) if a.dtype == torch.bfloat16 else bool((a == c).all())

    def close(a, c32, io):
        """Bits 0 and 2 together select the LDS-DMA kernel (csrc/gemm16.hip): same operands and products, but its fp32 sum runs
        over k in one sequence where the tiled family may add two half sums -- fp32 summation-order noise (<= 2e-5 of the RMS);
        a bf16-stored output may then differ from the rounded reference by one bf16 ulp."""
        if (io & 5) != 5:
            return eq(a, c32.to(a.dtype))
        d = (a.float() - c32).abs()
        rms = float(c32.pow(2).mean().sqrt())
        if a.dtype == torch.bfloat16:
            return bool((d <= c32.abs() * 2.0 ** -7 + 1e-4 * rms).all()) and float((a.float() - c32.bfloat16().float()).abs().mean()) < 1e-4 * rms
        return float(d.max()) <= 2e-5 * rms
    # forward, plain and GELU pair: x stored bf16 (1), outputs stored bf16 (2), both (3)
    y32, p32, a32 = E(M, Nn), E(M, Nn), E(M, Nn)
    call("cswin_linear_fwd", ptr(x32), None, 0, ptr(w), ptr(b), ptr(y32), None, None, None, 1, M, Nn, K, 1, 0, stream())
    call("cswin_linear_fwd", ptr(x32), None, 0, ptr(w), ptr(b), ptr(p32), ptr(a32), None, None, 1, M, Nn, K, 1, 0, stream())
    for io in (1, 2, 3, 4, 5, 6, 7):
        dt = torch.bfloat16 if io & 2 else torch.float32
        y, pre, act = E(M, Nn, dt=dt), E(M, Nn, dt=dt), E(M, Nn, dt=dt)
        xin, win = (x16 if io & 1 else x32), (w16 if io & 4 else w)
        call("cswin_linear_fwd", ptr(xin), None, 0, ptr(win), ptr(b), ptr(y), None, None, None, 1, M, Nn, K, 1, io, stream())
        call("cswin_linear_fwd", ptr(xin), None, 0, ptr(win), ptr(b), ptr(pre), ptr(act), None, None, 1, M, Nn, K, 1, io, stream())
        assert close(y, y32, io) and close(pre, p32, io) and close(act, a32, io), ("fwd", io)
    # forward with residual + row scale: x stored bf16, output fp32
    res, rs = T(det_normal("st16.res", (M, Nn))), T(np.array([0.5, 0.0, 1.5], np.float32))
    rps = (M + 2) // 3
    r32, r16 = E(M, Nn), E(M, Nn)
    call("cswin_linear_fwd", ptr(x32), None, 0, ptr(w), ptr(b), ptr(r32), None, ptr(res), ptr(rs), rps, M, Nn, K, 1, 0, stream())
    for io in (1, 4, 5):
        call("cswin_linear_fwd", ptr(x16 if io & 1 else x32), None, 0, ptr(w16 if io & 4 else w), ptr(b), ptr(r16), None, ptr(res), ptr(rs),
             rps, M, Nn, K, 1, io, stream())
        assert close(r16, r32, io), ("fwd residual", io)
    # concat input (skip connection): only the weight flag
    if K % 8 == 0:
        xa, xb = x32[:, :K // 2].contiguous(), x32[:, K // 2:].contiguous()
        c32, c16 = E(M, Nn), E(M, Nn)
        call("cswin_linear_fwd", ptr(xa), ptr(xb), K // 2, ptr(w), ptr(b), ptr(c32), None, None, None, 1, M, Nn, K, 1, 0, stream())
        call("cswin_linear_fwd", ptr(xa), ptr(xb), K // 2, ptr(w16), ptr(b), ptr(c16), None, None, None, 1, M, Nn, K, 1, 4, stream())
        assert eq(c16, c32), "fwd concat with the weight shadow"
    # data gradient: dy stored bf16 (1), dx stored bf16 (2), GELU' argument stored bf16 (8), with and without the row scale
    pre16 = T(det_normal("st16.pre", (M, K))).bfloat16()
    pre32f = pre16.float()
    for io, use_pre, use_rs in [(1, False, False), (2, False, False), (3, False, True), (8, True, False), (10, True, True), (11, True, True),
                                (4, False, True), (5, False, False), (14, True, True), (15, True, False)]:
        dx32 = E(M, K)
        call("cswin_linear_bwd_data", ptr(dy32), ptr(w), ptr(dx32), None, 0, ptr(pre32f) if use_pre else None,
             ptr(rs) if use_rs else None, rps if use_rs else 1, None, M, Nn, K, 1, 0, stream())
        dx = E(M, K, dt=torch.bfloat16 if io & 2 else torch.float32)
        call("cswin_linear_bwd_data", ptr(dy16 if io & 1 else dy32), ptr(w16 if io & 4 else w), ptr(dx), None, 0,
             ptr(pre16 if io & 8 else pre32f) if use_pre else None, ptr(rs) if use_rs else None, rps if use_rs else 1, None,
             M, Nn, K, 1, io, stream())
        assert close(dx, dx32, io), ("bwd_data", io)
    # weight gradient batch: dy stored bf16 (1), x stored bf16 (2)
    nbytes = lib().cswin_linear_bwd_weight_workspace(M, Nn, K)

    def wgrad(io, with_rs):
        wg, jobs = (WgradDesc * 1)(), (ReduceJob * 1)()
        dw, db, ws = E(Nn, K), E(Nn), E(nbytes // 4 + 4)
        dyt, xt = (dy16 if io & 1 else dy32), (x16 if io & 2 else x32)
        wg[0].dy, wg[0].x, wg[0].row_scale = dyt.data_ptr(), xt.data_ptr(), (rs.data_ptr() if with_rs else None)
        wg[0].dw, wg[0].dbias, wg[0].workspace, wg[0].ws_bytes = dw.data_ptr(), db.data_ptr(), ws.data_ptr(), nbytes
        wg[0].rows_per_sample, wg[0].M, wg[0].N, wg[0].K, wg[0].precision, wg[0].io_bf16 = rps, M, Nn, K, 1, io
        call("cswin_linear_bwd_weight_batch", ctypes.cast(wg, ctypes.c_void_p), 1, ctypes.cast(jobs, ctypes.c_void_p), None, 0, stream())
        call("cswin_rows_sum_multi", ctypes.cast(jobs, ctypes.c_void_p), 1, stream())
        torch.cuda.synchronize()
        return dw, db

    for with_rs in (False, True):
        dw0, db0 = wgrad(0, with_rs)
        for io in (1, 2, 3):
            dw, db = wgrad(io, with_rs)
            # io = 3 without a row scale runs the LDS-DMA tile, which forms the bias gradient with one more MFMA per fragment
            # (dy against a ones operand) instead of fp32 register sums: same addends, another summation order
            # (with a row scale its addends are the bf16-rounded scaled values: 2^-9 relative each, random in sign)
            db_ok = eq(db, db0) if io != 3 else float((db - db0).abs().max()) <= (6e-3 if with_rs else 1e-5) * float(db0.abs().max())
            assert eq(dw, dw0) and db_ok, ("wgrad", io, with_rs)
    # flags outside the contract are refused, not ignored
    from cswin_unet_amd._lib import CswinHipError
    with pytest.raises(CswinHipError):
        call("cswin_linear_fwd", ptr(x16), None, 0, ptr(w), ptr(b), ptr(y32), None, None, None, 1, M, Nn, K, 0, 1, stream())
    with pytest.raises(CswinHipError):
        call("cswin_linear_fwd", ptr(x16), None, 0, ptr(w), ptr(b), ptr(r32), None, ptr(res), None, 1, M, Nn, K, 1, 2, stream())


@pytest.mark.parametrize("M,C", [(4704, 256), (1000, 64), (300, 512), (77, 96)])
def test_layernorm_bf16_output_bit_exact(M, C):
    """y_bf16 of cswin_layernorm_fwd: the bf16-stored output is the fp32 output rounded to nearest even; statistics unchanged."""
    from cswin_unet_amd._lib import call, ptr, stream
    x, g, b = T(det_normal("ln16.x", (M, C)) * 2 + 0.5), T(det_normal("ln16.g", (C,))), T(det_normal("ln16.b", (C,)))
    outs = []
    for dt in (torch.float32, torch.bfloat16):
        y = torch.empty(M, C, dtype=dt, device=DEV)
        m, r = torch.empty(M, device=DEV), torch.empty(M, device=DEV)
        call("cswin_layernorm_fwd", ptr(x), ptr(g), ptr(b), ptr(y), ptr(m), ptr(r), M, C, 1e-5, int(dt == torch.bfloat16), stream())
        outs.append((y, m, r))
    (y32, m32, r32), (y16, m16, r16) = outs
    assert bool((y16.view(torch.int16) == y32.bfloat16().view(torch.int16)).all())
    assert bool((m16 == m32).all()) and bool((r16 == r32).all())


def test_weight_shadow_follows_the_parameters(N, bf16_matmul):
    """optim.FlatSGD keeps a bf16 shadow of the flat parameter buffer for the bf16 mode's GEMMs (cswin_sgd_flat shadow_bf16,
    io_bf16 bit 2): equal to the rounded parameters after construction, after every step and after a write from outside
    the optimiser (load_state_dict: noticed through the parameter's version counter on the next use), and a model forward
    that reads the shadow agrees with one that rounds the fp32 weights itself."""
    from cswin_unet_amd._lib import _shadows, shadow_ptr
    from cswin_unet_amd.optim import FlatSGD
    blk = N.CSWinBlock(dim=128, reso=28, num_heads=4, split_size=2, qkv_bias=True, drop_path=0.).to(DEV)
    fill_state_dict(blk)
    x = T(det_normal("shadow.x", (2, 28 * 28, 128)), True)
    saved = list(_shadows)
    del _shadows[:]
    try:
        assert shadow_ptr(blk.qkv.weight) is None
        y0 = blk(x).detach().clone()                                  # no shadow registered: fp32 weights, rounded by the GEMMs
        opt = FlatSGD(blk.parameters(), lr=0.1, momentum=0.9, weight_decay=1e-4)
        same = lambda: bool((opt.flat_param16.view(torch.int16) == opt.flat_param.bfloat16().view(torch.int16)).all())
        assert same() and shadow_ptr(blk.qkv.weight) is not None
        y1 = blk(x)
        # same operand values either way; with both operands stored as bf16 the Linears run in csrc/gemm16.hip, whose fp32 sums
        # run in another order: summation noise, now and then amplified to one bf16 ulp of a stored activation
        assert 0 <= _rel_l2(y1, y0) < 1e-3, "reading the shadow changed the forward"
        y1.backward(T(det_normal("shadow.dy", tuple(y1.shape))))
        opt.step()
        assert same()
        with torch.no_grad():                                         # a write from outside the optimiser
            blk.qkv.weight.copy_(blk.qkv.weight * 0.5)
        assert not same()
        sp = shadow_ptr(blk.qkv.weight)                               # next use of that weight: version moved -> re-packed
        assert same() and sp is not None
    finally:
        _shadows[:] = saved


@pytest.mark.parametrize("reso,idx,split,dim,heads", [(56, 0, 1, 64, 2), (28, 1, 2, 128, 4), (14, 0, 7, 256, 8), (7, -1, 7, 512, 16),
                                                      (24, 1, 12, 64, 2)])
def test_attention_bf16_qkv_storage_bit_exact(ops, reso, idx, split, dim, heads):
    """qkv_bf16 of cswin_attn_fwd / cswin_attn_bwd: q, k, v STORED as bf16 give bit-identical y / LePE gradients to the same
    values held in fp32 (all arithmetic is fp32 either way) and dqkv equals the fp32 dqkv rounded to nearest even.  Covers the
    thin-stripe, 7 x 7, whole-map (last stage) and large-window (two-pass backward) kernels."""
    B = 2
    C = dim if idx == -1 else dim // 2
    nh = heads if idx == -1 else heads // 2
    qkv16 = T(det_normal(f"att16.{reso}.{idx}.qkv", (B, reso * reso, 3 * C))).bfloat16()
    lw = T(det_normal(f"att16.{reso}.lw", (C, 1, 3, 3)) * 0.3)
    lb = T(det_normal(f"att16.{reso}.lb", (C,)) * 0.1)
    dy = T(det_normal(f"att16.{reso}.{idx}.dy", (B, reso * reso, C)))
    outs = []
    for q in (qkv16, qkv16.float()):
        q = q.clone().requires_grad_()
        w_, b_ = lw.clone().requires_grad_(), lb.clone().requires_grad_()
        y = ops.stripe_attention(q, reso, split, [idx], [nh], [w_], [b_])
        y.backward(dy)
        outs.append((y.detach(), q.grad, w_.grad, b_.grad))
    (y16, dq16, dw16, db16), (y32, dq32, dw32, db32) = outs
    assert dq16.dtype == torch.bfloat16 and y16.dtype == torch.float32
    assert bool((y16 == y32).all()), "attention output differs"
    assert bool((dw16 == dw32).all()) and bool((db16 == db32).all()), "LePE gradients differ"
    assert bool((dq16.view(torch.int16) == dq32.bfloat16().view(torch.int16)).all()), "dqkv is not the rounded fp32 dqkv"


@pytest.mark.parametrize("reso,idx,split,dim,heads", [(28, 1, 2, 128, 4), (14, 0, 7, 256, 8), (7, -1, 7, 512, 16), (24, 1, 12, 64, 2)])
def test_attention_bf16_y_storage_bit_exact(reso, idx, split, dim, heads):
    """Storage mode 3 of cswin_attn_fwd / cswin_attn_bwd (y stored as bf16 as well): the forward's y is the fp32 y rounded to
    nearest even, and the backward fed the bf16 y equals the mode-1 backward fed the same values in fp32, bit for bit."""
    import ctypes
    from cswin_unet_amd._lib import call, lib, ptr, stream
    from cswin_unet_amd.ops import _int_array, _ptr_array
    B = 2
    C = dim if idx == -1 else dim // 2
    nh = heads if idx == -1 else heads // 2
    L = reso * reso
    qkv16 = T(det_normal(f"atty.{reso}.{idx}.qkv", (B, L, 3 * C))).bfloat16()
    lw, lb = T(det_normal(f"atty.{reso}.lw", (C, 9)) * 0.3), T(det_normal(f"atty.{reso}.lb", (C,)) * 0.1)
    dy = T(det_normal(f"atty.{reso}.{idx}.dy", (B, L, C)))
    ha, ia = _int_array([nh]), _int_array([idx])
    E = lambda *sh, dt=torch.float32: torch.empty(*sh, dtype=dt, device=DEV)
    y32, y16, lse32, lse16 = E(B, L, C), E(B, L, C, dt=torch.bfloat16), E(B, nh, L), E(B, nh, L)
    z32, z16 = E(B, L, C), E(B, L, C, dt=torch.bfloat16)          # y0 = P V, the output without the LePE term (the backward's input)
    call("cswin_attn_fwd", ptr(qkv16), _ptr_array([lw]), _ptr_array([lb]), ptr(y32), ptr(z32), ptr(lse32), B, reso, C, 1, ha, ia, split, 0.0, 0.0, 0, None, 1, stream())
    call("cswin_attn_fwd", ptr(qkv16), _ptr_array([lw]), _ptr_array([lb]), ptr(y16), ptr(z16), ptr(lse16), B, reso, C, 1, ha, ia, split, 0.0, 0.0, 0, None, 3, stream())
    assert bool((y16.view(torch.int16) == y32.bfloat16().view(torch.int16)).all()) and bool((lse16 == lse32).all())
    assert bool((z16.view(torch.int16) == z32.bfloat16().view(torch.int16)).all())
    nbytes = lib().cswin_attn_bwd_workspace(B, reso, C, 1, ha, ia, split)
    res = []
    for mode, y in ((1, z16.float()), (3, z16)):
        dq, dw_, db_, ws = E(B, L, 3 * C, dt=torch.bfloat16), E(C, 9), E(C), E(nbytes // 4 + 4)
        call("cswin_attn_bwd", ptr(qkv16), _ptr_array([lw]), _ptr_array([lb]), ptr(lse32), ptr(y), ptr(dy), ptr(dq), _ptr_array([dw_]),
             _ptr_array([db_]), ptr(ws), nbytes, B, reso, C, 1, ha, ia, split, 0.0, None, 0.0, 0, None, mode, stream())
        torch.cuda.synchronize()
        res.append((dq, dw_, db_))
    (a, b, c), (d, e, f) = res
    assert bool((a.view(torch.int16) == d.view(torch.int16)).all()) and bool((b == e).all()) and bool((c == f).all())
    from cswin_unet_amd._lib import CswinHipError
    with pytest.raises(CswinHipError):
        call("cswin_attn_fwd", ptr(qkv16), _ptr_array([lw]), _ptr_array([lb]), ptr(y16), ptr(z16), ptr(lse16), B, reso, C, 1, ha, ia, split, 0.0, 0.0, 0, None, 2, stream())


@pytest.mark.parametrize("reso,idx,split,dim,heads", [(56, 0, 1, 64, 2), (28, 1, 2, 128, 4), (14, 0, 7, 256, 8), (7, -1, 7, 512, 16),
                                                      (24, 1, 12, 64, 2), (16, -1, 16, 128, 4)])      # the last two: large-window backward
def test_attention_bf16_matrix_instructions_vs_fp32(reso, idx, split, dim, heads):
    """Mode 7 of cswin_attn_fwd / cswin_attn_bwd (bf16 MFMAs) against mode 3 (same bf16-stored q, k, v, y; fp32 MFMAs).  Mode 7
    rounds the scaled q, the probabilities, dS and dO to bf16 (relative 2^-9 uniform, sigma 1.1e-3 each) on their way into the
    matrix pipe; k, v are bf16 already.  An output element is a sum of such products, so the error is a few sigma of the output
    RMS: bounds 5e-3 (y) and 8e-3 (dqkv) in L2 (measured 1.2 - 1.6e-3 and 1.5 - 2.2e-3); the LePE gradients do not pass through the
    matrix pipe and must not move."""
    import ctypes
    from cswin_unet_amd._lib import call, lib, ptr, stream
    from cswin_unet_amd.ops import _int_array, _ptr_array
    B = 2
    C = dim if idx == -1 else dim // 2
    nh = heads if idx == -1 else heads // 2
    L = reso * reso
    qkv16 = T(det_normal(f"attm.{reso}.{idx}.qkv", (B, L, 3 * C))).bfloat16()
    lw, lb = T(det_normal(f"attm.{reso}.lw", (C, 9)) * 0.3), T(det_normal(f"attm.{reso}.lb", (C,)) * 0.1)
    dy = T(det_normal(f"attm.{reso}.{idx}.dy", (B, L, C)))
    ha, ia = _int_array([nh]), _int_array([idx])
    E = lambda *sh, dt=torch.float32: torch.empty(*sh, dtype=dt, device=DEV)
    nbytes = lib().cswin_attn_bwd_workspace(B, reso, C, 1, ha, ia, split)
    res = {}
    for mode in (3, 7):
        y, z, lse = E(B, L, C, dt=torch.bfloat16), E(B, L, C, dt=torch.bfloat16), E(B, nh, L)
        call("cswin_attn_fwd", ptr(qkv16), _ptr_array([lw]), _ptr_array([lb]), ptr(y), ptr(z), ptr(lse), B, reso, C, 1, ha, ia, split, 0.0, 0.0, 0, None, mode, stream())
        dq, dw_, db_, ws = E(B, L, 3 * C, dt=torch.bfloat16), E(C, 9), E(C), E(nbytes // 4 + 4)
        call("cswin_attn_bwd", ptr(qkv16), _ptr_array([lw]), _ptr_array([lb]), ptr(lse), ptr(z), ptr(dy), ptr(dq), _ptr_array([dw_]),
             _ptr_array([db_]), ptr(ws), nbytes, B, reso, C, 1, ha, ia, split, 0.0, None, 0.0, 0, None, mode, stream())
        torch.cuda.synchronize()
        res[mode] = (y.float(), lse, dq.float(), dw_, db_)
    names, bounds = ("y", "lse", "dqkv", "dlepe_w", "dlepe_b"), (5e-3, 1e-3, 8e-3, 1e-6, 1e-6)
    for n, a, b, bound in zip(names, res[7], res[3], bounds):
        e = _rel_l2(a, b)
        with open(LOG, "a") as f:
            f.write(f"attn_m16.r{reso}.{n} l2 {e:.3e}\n")
        assert e < bound, (n, e)
    assert _rel_l2(res[7][0], res[3][0]) > 1e-5, "mode 7 is bit-identical to mode 3: the bf16 matrix path did not run"


@pytest.mark.parametrize("dim,reso,heads,split,last", [(64, 56, 2, 1, False), (256, 14, 8, 7, False), (512, 7, 16, 7, True)])
def test_block_bf16_activation_storage(N, bf16_matmul, dim, reso, heads, split, last):
    """bf16 mode stores both LayerNorm outputs, qkv, the attention output, the MLP hidden pair and the gradients of qkv and of the
    hidden layer as bf16 (ops._CSWinBlock; include/cswin_hip.h io_bf16 / qkv_bf16 / y_bf16).  As GEMM operands those tensors
    were rounded to bf16 anyway; what storage adds is one rounding (relative 2^-9 uniform: sigma 1.1e-3 per element) of q, k, v
    and of y (in the backward's delta) inside the attention kernels and of the GELU argument before GELU'.  So against the
    same block with fp32 storage (same bf16 operands) every output must agree to a few sigma in L2 -- bound 1e-2 -- and must NOT be
    identical (the storage path is live); against the fp32 oracle the whole-model bounds above apply."""
    import cswin_unet_amd
    blk = N.CSWinBlock(dim=dim, reso=reso, num_heads=heads, split_size=split, mlp_ratio=4., qkv_bias=True, drop_path=0.,
                       last_stage=last).to(DEV)
    fill_state_dict(blk)
    x = det_normal(f"store16.{dim}.x", (2, reso * reso, dim))
    dy = T(det_normal(f"store16.{dim}.dy", (2, reso * reso, dim)))

    def run(storage):
        prev = cswin_unet_amd.set_activation_storage(storage)
        try:
            blk.zero_grad(set_to_none=True)
            xi = T(x, True)
            y = blk(xi)
            y.backward(dy)
            return [y.detach().clone(), xi.grad.clone()] + [p.grad.clone() for p in blk.parameters()]
        finally:
            cswin_unet_amd.set_activation_storage(prev)

    a, b = run("bf16"), run("fp32")
    names = ["y", "dx"] + [n for n, _ in blk.named_parameters()]
    differ = False
    for n, u, v in zip(names, a, b):
        e = _rel_l2(u, v)
        with open(LOG, "a") as f:
            f.write(f"store16.c{dim}.{n} l2 {e:.3e}\n")
        assert e < 1e-2, (n, e)
        differ |= e > 1e-6
    assert differ, "bf16 storage produced bit-identical results: the storage path did not run"


def test_model_bf16_384_step_vs_oracle(N, ops, bf16_matmul):
    """BASELINE configs[3] in its own precision: 384 x 384 (split [1,2,12,12]: large-window attention paths), bf16 operands, B = 1,
    against the fp32 oracle with the derived bounds."""
    cfg = dict(O.TINY_224, img_size=384, split_size=(1, 2, 12, 12))
    net = N.CSWinTransformer(img_size=384, num_classes=9, embed_dim=64, depth=[1, 2, 9, 1], split_size=[1, 2, 12, 12],
                             num_heads=[2, 4, 8, 16], qkv_bias=True).to(DEV)
    fill_state_dict(net).train()
    _bf16_step_vs_oracle(N, ops, cfg, net, det_normal("model384.x", (1, 3, 384, 384)), det_labels("model384.lab", (1, 384, 384), 9),
                         "bf16_384", ["stage3.4.qkv.weight", "stage3.4.attns.1.get_v.weight", "stage_up3.2.proj.weight",
                                      "merge2.conv.weight", "upsample1.encoder.weight", "output.weight"])


def test_model_bf16_base_width_step_vs_oracle(N, ops, bf16_matmul):
    """BASELINE configs[4] widths (embed_dim 96, head dim 24) with a short depth in bf16 operands, B = 2, against the fp32 oracle."""
    cfg = dict(O.TINY_224, embed_dim=96, depth=(1, 2, 2, 1), num_heads=(4, 8, 16, 32))
    net = N.CSWinTransformer(img_size=224, num_classes=9, embed_dim=96, depth=[1, 2, 2, 1], split_size=[1, 2, 7, 7],
                             num_heads=[4, 8, 16, 32], qkv_bias=True).to(DEV)
    fill_state_dict(net).train()
    _bf16_step_vs_oracle(N, ops, cfg, net, det_normal("modelbase.x", (2, 3, 224, 224)), det_labels("modelbase.lab", (2, 224, 224), 9),
                         "bf16_base", ["stage3.1.qkv.weight", "stage2.0.mlp.fc1.weight", "merge3.conv.weight", "stage_up2.1.proj.weight",
                                       "upsample2.encoder.weight", "output.weight"])


# ------------------------------------------------------------------------------------------------------------------
# BASELINE full sizes: one whole training step against the CPU oracle (every B-dependent dispatch branch: GEMM tile and
# split-K choices, the attention query-split heuristic, the batched weight-gradient launch, CARAFE slab sizing)
# ------------------------------------------------------------------------------------------------------------------
FULL_GRADS = ["stage1_conv_embed.0.weight", "stage1.0.qkv.weight", "stage1.0.attns.0.get_v.weight", "merge1.conv.weight",
              "stage2.1.mlp.fc1.weight", "stage2.0.attns.1.get_v.bias", "merge2.conv.weight", "stage3.0.proj.weight",
              "stage3.4.qkv.weight", "stage3.8.mlp.fc2.weight", "stage3.4.attns.1.get_v.weight", "stage3.2.norm1.weight",
              "merge3.conv.weight", "stage4.0.qkv.bias", "stage4.0.attns.0.get_v.weight", "norm.weight",
              "stage_up4.0.mlp.fc1.weight", "upsample4.encoder.weight", "upsample4.out.weight", "concat_linear4.weight",
              "stage_up3.5.qkv.weight", "stage_up3.0.norm2.bias", "upsample3.down.weight", "concat_linear3.weight",
              "stage_up2.1.proj.weight", "upsample2.encoder.weight", "concat_linear2.weight", "stage_up1.0.mlp.fc2.weight",
              "upsample1.encoder.weight", "upsample1.down.weight", "upsample1.out.weight", "norm_up.weight", "output.weight"]


def _full_size_step(N, ops, img_size, batch, split, tag):
    cfg = dict(O.TINY_224, img_size=img_size, split_size=tuple(split))
    net = N.CSWinTransformer(img_size=img_size, num_classes=9, embed_dim=64, depth=[1, 2, 9, 1], split_size=list(split),
                             num_heads=[2, 4, 8, 16], qkv_bias=True, drop_path_rate=0.).to(DEV)
    fill_state_dict(net).train()
    g = torch.Generator().manual_seed(20260)
    img = torch.randn(batch, 3, img_size, img_size, generator=g)
    lab = torch.randint(0, 9, (batch, img_size, img_size), generator=g)
    logits = net(img.to(DEV))
    loss, stats = ops.ce_dice_loss(logits, lab.to(DEV))
    loss.backward()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    P = O.golden_params(cfg)
    ref_logits = O.cswin_forward(P, img, cfg)
    ref_loss, ref_ce, ref_dice = O.ce_dice_loss(ref_logits, lab)
    ref_loss.backward()
    rel_err(logits, ref_logits, f"{tag}.logits")
    assert abs(float(loss) - float(ref_loss)) < 1e-3 * abs(float(ref_loss))
    assert abs(float(stats[1]) - float(ref_ce)) < 1e-3 * abs(float(ref_ce))
    assert abs(float(stats[2]) - float(ref_dice)) < 1e-3 * abs(float(ref_dice))
    params = dict(net.named_parameters())
    for n in FULL_GRADS:
        rel_err(params[n].grad, P[n].grad, f"{tag}.grad.{n}")


def test_full_size_training_step_b24_vs_oracle(N, ops):
    """BASELINE configs[1] exactly as bench.py times it (cswin_tiny_224_lite, B = 24, fp32): logits, loss, CE, Dice and 33
    parameter gradients covering every stage, both CARAFE kinds, the merges, the skips and the head at RTOL 1e-3."""
    _full_size_step(N, ops, 224, 24, (1, 2, 7, 7), "full224b24")


def test_full_size_training_step_384_b8_vs_oracle(N, ops):
    """BASELINE configs[3] shape at the batch bench.py uses for it (384 x 384, split [1,2,12,12], B = 8)."""
    _full_size_step(N, ops, 384, 8, (1, 2, 12, 12), "full384b8")


def _full_size_step_bf16(N, ops, net, cfg, img, lab, tag, grads, logits_bound, grad_bound):
    """One whole bf16-mode training step at a BASELINE size against the fp32 CPU oracle, L2 bounds as derived for the small bf16
    model tests (sigma = 1.6e-3 per GEMM, errors add in quadrature along the chain; logged to parity_errors.log)."""
    logits = net(img.to(DEV))
    loss, stats = ops.ce_dice_loss(logits, lab.to(DEV))
    loss.backward()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    P = O.golden_params(cfg)
    ref_logits = O.cswin_forward(P, img, cfg)
    ref_loss, _, _ = O.ce_dice_loss(ref_logits, lab)
    ref_loss.backward()
    e = _rel_l2(logits, ref_logits)
    with open(LOG, "a") as f:
        f.write(f"{tag}.logits l2 {e:.3e}\n")
    assert 1e-4 < e < logits_bound, e
    assert abs(float(loss) - float(ref_loss)) < 1e-2 * abs(float(ref_loss))
    params = dict(net.named_parameters())
    for n in grads:
        e = _rel_l2(params[n].grad, P[n].grad)
        with open(LOG, "a") as f:
            f.write(f"{tag}.grad.{n} l2 {e:.3e}\n")
        assert e < grad_bound, (n, e)


def test_full_size_training_step_b24_bf16_vs_oracle(N, ops, bf16_matmul):
    """BASELINE configs[2]'s per-GPU workload exactly as bench.py's bf16_mode key times it (cswin_tiny_224_lite, B = 24, bf16
    operands / activations / attention products): logits and the 33 gradients of FULL_GRADS against the fp32 oracle."""
    net = N.CSWinTransformer(img_size=224, num_classes=9, embed_dim=64, depth=[1, 2, 9, 1], split_size=[1, 2, 7, 7],
                             num_heads=[2, 4, 8, 16], qkv_bias=True, drop_path_rate=0.).to(DEV)
    fill_state_dict(net).train()
    g = torch.Generator().manual_seed(20260)
    img = torch.randn(24, 3, 224, 224, generator=g)
    lab = torch.randint(0, 9, (24, 224, 224), generator=g)
    _full_size_step_bf16(N, ops, net, dict(O.TINY_224), img, lab, "full224b24.bf16", FULL_GRADS, BF16_LOGITS_L2, BF16_GRAD_L2)


def test_full_size_training_step_384_b8_bf16_vs_oracle(N, ops, bf16_matmul):
    """BASELINE configs[3] (384 x 384, split [1,2,12,12], B = 8 per GPU) in its own precision."""
    cfg = dict(O.TINY_224, img_size=384, split_size=(1, 2, 12, 12))
    net = N.CSWinTransformer(img_size=384, num_classes=9, embed_dim=64, depth=[1, 2, 9, 1], split_size=[1, 2, 12, 12],
                             num_heads=[2, 4, 8, 16], qkv_bias=True, drop_path_rate=0.).to(DEV)
    fill_state_dict(net).train()
    g = torch.Generator().manual_seed(20261)
    img = torch.randn(8, 3, 384, 384, generator=g)
    lab = torch.randint(0, 9, (8, 384, 384), generator=g)
    _full_size_step_bf16(N, ops, net, cfg, img, lab, "full384b8.bf16", FULL_GRADS, BF16_LOGITS_L2, BF16_GRAD_L2)


# cswin_base_224 at its OWN size (BASELINE configs[4]: embed_dim 96, depth [2, 4, 32, 2], heads [4, 8, 16, 32], B = 8 per GPU): 148 chained
# GEMMs per direction, head dim 24, the B-dependent GEMM / attention dispatch of that shape.  Oracle only (the reference cannot
# construct embed_dim != 64).
BASE_CFG = dict(O.TINY_224, embed_dim=96, depth=(2, 4, 32, 2), num_heads=(4, 8, 16, 32))
BASE_GRADS = ["stage1_conv_embed.0.weight", "stage1.1.qkv.weight", "stage1.0.attns.0.get_v.weight", "merge1.conv.weight",
              "stage2.3.mlp.fc1.weight", "stage2.0.attns.1.get_v.bias", "merge2.conv.weight", "stage3.0.proj.weight",
              "stage3.15.qkv.weight", "stage3.31.mlp.fc2.weight", "stage3.20.attns.1.get_v.weight", "stage3.7.norm1.weight",
              "merge3.conv.weight", "stage4.1.qkv.bias", "stage4.0.attns.0.get_v.weight", "norm.weight",
              "stage_up4.1.mlp.fc1.weight", "upsample4.encoder.weight", "concat_linear4.weight", "stage_up3.0.qkv.weight",
              "stage_up3.31.norm2.bias", "stage_up3.16.proj.weight", "upsample3.down.weight", "concat_linear3.weight",
              "stage_up2.2.proj.weight", "upsample2.encoder.weight", "concat_linear2.weight", "stage_up1.1.mlp.fc2.weight",
              "upsample1.encoder.weight", "upsample1.out.weight", "norm_up.weight", "output.weight"]


def _base_model(N):
    net = N.CSWinTransformer(img_size=224, num_classes=9, embed_dim=96, depth=[2, 4, 32, 2], split_size=[1, 2, 7, 7],
                             num_heads=[4, 8, 16, 32], qkv_bias=True, drop_path_rate=0.).to(DEV)
    return fill_state_dict(net).train()


def test_cswin_base_full_depth_step_b8_vs_oracle(N, ops):
    """fp32: logits, loss, CE, Dice and 32 gradients spread over all 76 blocks at RTOL 1e-3."""
    net = _base_model(N)
    g = torch.Generator().manual_seed(20262)
    img = torch.randn(8, 3, 224, 224, generator=g)
    lab = torch.randint(0, 9, (8, 224, 224), generator=g)
    logits = net(img.to(DEV))
    loss, stats = ops.ce_dice_loss(logits, lab.to(DEV))
    loss.backward()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    P = O.golden_params(BASE_CFG)
    ref_logits = O.cswin_forward(P, img, BASE_CFG)
    ref_loss, ref_ce, ref_dice = O.ce_dice_loss(ref_logits, lab)
    ref_loss.backward()
    rel_err(logits, ref_logits, "baseb8.logits")
    assert abs(float(loss) - float(ref_loss)) < 1e-3 * abs(float(ref_loss))
    assert abs(float(stats[1]) - float(ref_ce)) < 1e-3 * abs(float(ref_ce)) and abs(float(stats[2]) - float(ref_dice)) < 1e-3 * abs(float(ref_dice))
    params = dict(net.named_parameters())
    assert set(params) == set(P)
    for n in BASE_GRADS:
        rel_err(params[n].grad, P[n].grad, f"baseb8.grad.{n}")


def test_cswin_base_full_depth_step_b8_bf16_vs_oracle(N, ops, bf16_matmul):
    """bf16 mode.  The small-model bounds (3e-2 logits, 5e-2 gradients) were derived for ~60 chained GEMMs; 148 of them scale the
    quadrature sum by sqrt(148 / 60) = 1.57: 5e-2 and 8e-2."""
    net = _base_model(N)
    g = torch.Generator().manual_seed(20262)
    img = torch.randn(8, 3, 224, 224, generator=g)
    lab = torch.randint(0, 9, (8, 224, 224), generator=g)
    _full_size_step_bf16(N, ops, net, BASE_CFG, img, lab, "baseb8.bf16", BASE_GRADS, 5e-2, 8e-2)



def test_use_chk_with_drop_path_matches_plain_backward(N, ops):
    """Activation checkpointing (use_chk, cswin_unet.py:329-331,468-532) with stochastic depth: the recompute in backward
    must reuse the DropPath factors the forward drew (they used to be popped and re-drawn)."""
    img = T(det_normal("chk.x", (3, 3, 224, 224)))
    lab = T(det_labels("chk.lab", (3, 224, 224), 9))
    grads = []
    for chk in (False, True):
        net = N.CSWinTransformer(img_size=224, num_classes=9, embed_dim=64, depth=[1, 2, 2, 1], split_size=[1, 2, 7, 7],
                                 num_heads=[2, 4, 8, 16], qkv_bias=True, drop_path_rate=0.5, use_chk=chk).to(DEV)
        fill_state_dict(net).train()
        torch.manual_seed(77)                               # same Bernoulli draws in both runs
        logits = net(img)
        loss, _ = ops.ce_dice_loss(logits, lab)
        loss.backward()
        grads.append({n: p.grad.clone() for n, p in net.named_parameters()})
        if chk:
            assert any(b._dp_preset for b in net.stage3)     # the factors were pre-drawn and are still there
    for n in grads[0]:
        assert torch.allclose(grads[0][n], grads[1][n], rtol=1e-5, atol=1e-7), n


def test_engine_backward_places_the_gradients_autograd_would_accumulate(N, ops):
    """ops.engine_backward (the context HipEngine wraps around each backward phase): slab reductions are queued and run in a few
    batched launches, and gradients of leaf parameters are written straight into the optimiser's flat gradient buffer.  The flat
    buffer must end up holding what a plain loss.backward() leaves in .grad, also for composed weights (fused head matrix, summed stem
    kernel: reduced immediately, copied afterwards)."""
    from cswin_unet_amd.optim import FlatSGD
    img = T(det_normal("eng.x", (2, 3, 224, 224)))
    lab = T(det_labels("eng.lab", (2, 224, 224), 9))

    def model():
        net = N.CSWinTransformer(img_size=224, num_classes=9, embed_dim=64, depth=[1, 2, 2, 1], split_size=[1, 2, 7, 7],
                                 num_heads=[2, 4, 8, 16], qkv_bias=True, drop_path_rate=0.0).to(DEV)
        return fill_state_dict(net).train()

    net = model()
    loss, _ = ops.ce_dice_loss(net(img), lab)
    loss.backward()
    want = {n: p.grad.clone() for n, p in net.named_parameters()}

    net = model()
    opt = FlatSGD(net.parameters(), lr=0.0)
    loss, _ = ops.ce_dice_loss(net(img), lab)
    opt.zero_grad()
    with ops.engine_backward(opt):
        grads = torch.autograd.grad(loss, opt.params)
    in_place = 0
    for p, g, o in zip(opt.params, grads, opt.offsets):
        p.grad = g
        in_place += g.data_ptr() == opt.flat_grad.data_ptr() + 4 * o
    assert in_place > 0.9 * len(opt.params), (in_place, len(opt.params))     # all but the composed weights
    opt.gather_grads()
    torch.cuda.synchronize()
    names = [n for n, p in net.named_parameters() if p.requires_grad]
    for n, p, o in zip(names, opt.params, opt.offsets):
        got = opt.flat_grad[o:o + p.numel()].view(p.shape)
        assert _rel_l2(got, want[n]) < 1e-6, (n, _rel_l2(got, want[n]))       # same slabs; the batched reduction may sum them in another order


def _engine_model(N, frozen=()):
    net = N.CSWinTransformer(img_size=224, num_classes=9, embed_dim=64, depth=[1, 2, 2, 1], split_size=[1, 2, 7, 7],
                             num_heads=[2, 4, 8, 16], qkv_bias=True, drop_path_rate=0.0).to(DEV)
    fill_state_dict(net).train()
    params = dict(net.named_parameters())
    for n in frozen:
        params[n].requires_grad_(False)
    return net


def _engine_reference(N, ops, img, lab, frozen=()):
    """name -> gradient a plain loss.backward() leaves on every trainable parameter."""
    net = _engine_model(N, frozen)
    loss, _ = ops.ce_dice_loss(net(img), lab)
    loss.backward()
    return {n: p.grad.clone() for n, p in net.named_parameters() if p.requires_grad}


def _assert_flat_grad(net, opt, want):
    torch.cuda.synchronize()
    names = [n for n, p in net.named_parameters() if p.requires_grad]
    assert names == list(want) and len(names) == len(opt.params)
    for n, p, o in zip(names, opt.params, opt.offsets):
        got = opt.flat_grad[o:o + p.numel()].view(p.shape)
        assert _rel_l2(got, want[n]) < 1e-6, (n, _rel_l2(got, want[n]))


def test_engine_backward_with_frozen_parameters(N, ops):
    """Partial fine-tuning through the engine: a frozen parameter is a leaf without a slot in the optimiser's flat buffer.  Its
    gradient goes to a fresh tensor that autograd drops as soon as the op returns, so a reduction writing there must not wait
    (it would write into memory the allocator has handed to somebody else): while the pass is open, every waiting reduction
    writes inside flat_grad only, and the trainable parameters' gradients are those of a plain loss.backward()."""
    from cswin_unet_amd.optim import FlatSGD
    frozen = ("stage3.0.qkv.weight", "stage3.1.norm1.weight", "stage3.1.norm1.bias", "stage3.0.mlp.fc2.bias")
    img = T(det_normal("eng.x", (2, 3, 224, 224)))
    lab = T(det_labels("eng.lab", (2, 224, 224), 9))
    want = _engine_reference(N, ops, img, lab, frozen)

    net = _engine_model(N, frozen)
    assert set(frozen) <= set(dict(net.named_parameters())) and len(want) == len(list(net.parameters())) - len(frozen)
    opt = FlatSGD(net.parameters(), lr=0.0)
    loss, _ = ops.ce_dice_loss(net(img), lab)
    opt.zero_grad()
    with ops.engine_backward(opt) as bwd:
        grads = torch.autograd.grad(loss, opt.params)
        lo, waiting = opt.flat_grad.data_ptr(), bwd.queued_outputs()
        assert waiting and all(lo <= a < lo + 4 * opt.numel for a in waiting)
    for p, g in zip(opt.params, grads):
        p.grad = g
    opt.gather_grads()
    _assert_flat_grad(net, opt, want)


def test_flat_sgd_alternates_between_plain_and_engine_backward(N, ops):
    """One FlatSGD, stepped after a plain loss.backward() (every gradient gathered), after an engine pass (only the composed
    weights' gradients gathered) and after a plain one again: the gather table follows the number of rows each time.  lr = 0, so
    the three steps see the same weights and must leave the same gradients in flat_grad."""
    from cswin_unet_amd.optim import FlatSGD
    img = T(det_normal("eng.x", (2, 3, 224, 224)))
    lab = T(det_labels("eng.lab", (2, 224, 224), 9))
    want = _engine_reference(N, ops, img, lab)
    net = _engine_model(N)
    opt = FlatSGD(net.parameters(), lr=0.0)
    for engine in (False, True, False):
        loss, _ = ops.ce_dice_loss(net(img), lab)
        opt.zero_grad()
        if engine:
            with ops.engine_backward(opt):
                grads = torch.autograd.grad(loss, opt.params)
            for p, g in zip(opt.params, grads):
                p.grad = g
        else:
            loss.backward()
        opt.step()
        _assert_flat_grad(net, opt, want)


def test_engine_backward_refuses_a_leaf_parameter_used_twice(ops):
    """Two ops sharing one leaf weight: outside a pass autograd accumulates the two gradients (bit-equal to the sum of the same
    two ops run on separate copies of the weight); inside engine_backward both would be written to the one slot, the second
    over the first while its reduction may still wait, so the pass refuses."""
    from cswin_unet_amd._lib import CswinHipError
    from cswin_unet_amd.optim import FlatSGD
    x = T(det_normal("twice.x", (4, 49, 64)))
    w, w1, w2 = (torch.nn.Parameter(T(det_normal("twice.w", (64, 64)))) for _ in range(3))
    b = torch.nn.Parameter(T(det_normal("twice.b", (64,))))

    def loss(wa, wb):
        return ops.linear(ops.linear(x, wa, b), wb).square().sum()

    loss(w1, w2).backward()
    separate, b_want = w1.grad + w2.grad, b.grad.clone()
    b.grad = None
    loss(w, w).backward()
    assert torch.equal(w.grad, separate) and torch.equal(b.grad, b_want)

    opt = FlatSGD([w, b], lr=0.0)
    opt.zero_grad()
    with pytest.raises(CswinHipError, match="offset 0"):
        with ops.engine_backward(opt):
            torch.autograd.grad(loss(w, w), opt.params)
    loss(w, w).backward()                              # the refused pass left nothing behind
    assert torch.equal(w.grad, separate) and torch.equal(b.grad, b_want)


def test_use_chk_in_bf16_mode_matches_plain_backward(N, ops, bf16_matmul):
    """The same in the bf16 mode: the recompute runs the bf16-storage forward again, the backward finds (or does not find) the bf16
    gradient twins in another order than without checkpointing; with identical DropPath draws the gradients must agree to the
    summation-order noise of the kernels (twin hits only choose between two kernels computing the same product)."""
    img = T(det_normal("chk16.x", (2, 3, 224, 224)))
    lab = T(det_labels("chk16.lab", (2, 224, 224), 9))
    grads = []
    for chk in (False, True):
        net = N.CSWinTransformer(img_size=224, num_classes=9, embed_dim=64, depth=[1, 2, 2, 1], split_size=[1, 2, 7, 7],
                                 num_heads=[2, 4, 8, 16], qkv_bias=True, drop_path_rate=0.3, use_chk=chk).to(DEV)
        fill_state_dict(net).train()
        torch.manual_seed(78)
        loss, _ = ops.ce_dice_loss(net(img), lab)
        loss.backward()
        grads.append({n: p.grad.clone() for n, p in net.named_parameters()})
    for n in grads[0]:
        assert _rel_l2(grads[1][n], grads[0][n]) < 2e-2, (n, _rel_l2(grads[1][n], grads[0][n]))


def test_out_of_range_label_poisons_the_loss(ops):
    """nn.CrossEntropyLoss raises on a target outside [0, ncls); the fused loss makes the step's loss NaN instead of silently
    biasing it (no host sync on the step path)."""
    logits = T(det_normal("lab.logits", (2, 9, 32, 32)))
    lab = det_labels("lab.lab", (2, 32, 32), 9).copy()
    loss, _ = ops.ce_dice_loss(logits, T(lab))
    assert torch.isfinite(loss)
    lab[1, 3, 5] = 255
    loss, _ = ops.ce_dice_loss(logits, T(lab))
    assert torch.isnan(loss)


def test_dice_loss_ignores_an_out_of_range_label():
    """The reference DiceLoss one-hots with == (utils.py:13-19): a label outside [0, n_classes) matches no class and is simply
    ignored.  The fused kernels poison the CE sum for such a label; a loss without a CE term (utils.DiceLoss: w_ce = 0) must not
    inherit that NaN, in value or in gradient."""
    from cswin_unet_amd.utils import DiceLoss
    ncls = 4
    logits = det_normal("diceoor.logits", (2, ncls, 24, 24))
    lab = det_labels("diceoor.lab", (2, 24, 24), ncls).copy()
    lab[0, 3, 5] = 255
    lab[1, 0, 0] = ncls

    def restated(lg, target):
        pr = torch.softmax(lg, 1)
        loss = 0.0
        for c in range(ncls):
            t = (target == c).float()
            loss = loss + (1 - (2 * (pr[:, c] * t).sum() + 1e-5) / ((pr[:, c] ** 2).sum() + (t * t).sum() + 1e-5))
        return loss / ncls
    lg = T(logits, grad=True)
    loss = DiceLoss(ncls)(lg, T(lab), softmax=True)
    loss.backward()
    ref_in = torch.from_numpy(logits).requires_grad_()
    ref = restated(ref_in, torch.from_numpy(lab))
    ref.backward()
    assert torch.isfinite(loss) and abs(float(loss) - float(ref)) < 1e-5
    rel_err(lg.grad, ref_in.grad, "diceoor.dlogits")


def test_graph_replay_sees_weights_written_from_outside(N, bf16_matmul):
    """A captured step has the bf16 weight shadow's address baked in and runs no Python when replayed: a weight written from
    outside the step (load_state_dict / copy_ on a parameter) must reach the shadow before the next replay.  The first loss after
    such a write has to be the loss of the NEW weights (checked against a fresh eager trainer on the same weights)."""
    from cswin_unet_amd.trainer import DataParallelTrainer
    mk = lambda: fill_state_dict(N.CSWinTransformer(img_size=224, num_classes=9, embed_dim=64, depth=[1, 1, 1, 1], split_size=[1, 2, 7, 7],
                                                    num_heads=[2, 4, 8, 16], qkv_bias=True, drop_path_rate=0.).to(DEV)).train()
    img = T(det_normal("stale.x", (2, 1, 224, 224))).repeat(1, 3, 1, 1)
    lab = T(det_labels("stale.labels", (2, 224, 224), 9))
    net = mk()
    tr = DataParallelTrainer(net, 9, base_lr=0.0, max_iterations=100, use_graph=True)      # lr 0: the steps leave the weights alone
    l0 = float(tr.train_step(img, lab)[0])
    assert abs(float(tr.train_step(img, lab)[0]) - l0) < 1e-6 * abs(l0)
    with torch.no_grad():
        for n_, p_ in net.named_parameters():
            if n_.endswith("qkv.weight") or n_.endswith("fc1.weight"):
                p_.copy_(p_ * 1.5)
    l1 = float(tr.train_step(img, lab)[0])                         # replayed graph, new weights
    net2 = mk()
    with torch.no_grad():
        for (n_, p_), (_, q_) in zip(net2.named_parameters(), net.named_parameters()):
            p_.copy_(q_)
    l2 = float(DataParallelTrainer(net2, 9, base_lr=0.0, max_iterations=100, use_graph=False).train_step(img, lab)[0])
    assert abs(l1 - l0) > 1e-4 * abs(l0), "the write did not change the loss: the test does not see the shadow"
    assert abs(l1 - l2) < 2e-4 * abs(l2), (l0, l1, l2)


def test_live_dropout_stays_under_hipgraph_and_redraws(N):
    """A model with live nn.Dropouts (drop_rate, attn_drop_rate > 0; cswin_unet.py:25,27,101,135) keeps its captured step: the host
    seeds are frozen at capture, the device-resident epoch that every dropout kernel adds to its seed is advanced inside the graph.
    With lr = 0 the weights never move, so two replays differ only through their masks: the losses must differ from step to step
    (fresh masks), stay close to the mask-free loss (p is small), and a second engine replays a different sequence."""
    from cswin_unet_amd.trainer import DataParallelTrainer
    mk = lambda dr: fill_state_dict(N.CSWinTransformer(img_size=224, num_classes=9, embed_dim=64, depth=[1, 1, 1, 1], split_size=[1, 2, 7, 7],
                                                       num_heads=[2, 4, 8, 16], qkv_bias=True, drop_rate=dr, attn_drop_rate=dr,
                                                       drop_path_rate=0.).to(DEV)).train()
    img = T(det_normal("livedrop.x", (2, 1, 224, 224))).repeat(1, 3, 1, 1)
    lab = T(det_labels("livedrop.labels", (2, 224, 224), 9))
    ref = float(DataParallelTrainer(mk(0.0), 9, base_lr=0.0, max_iterations=100, use_graph=True).train_step(img, lab)[0])
    torch.manual_seed(7)
    tr = DataParallelTrainer(mk(0.05), 9, base_lr=0.0, max_iterations=100, use_graph=True)
    assert tr.engine.use_graph
    losses = [float(tr.train_step(img, lab)[0]) for _ in range(5)]
    assert tr.engine._graphs is not None, "the step was not captured"
    assert len({round(v, 6) for v in losses}) == 5, losses                       # every replay drew another mask set
    assert all(abs(v - ref) < 0.1 * abs(ref) for v in losses) and all(abs(v - ref) > 1e-6 * abs(ref) for v in losses), (ref, losses)


def test_bf16_wire_pack_unpack():
    from cswin_unet_amd._lib import call, ptr, stream
    for n in (4096 * 4, 1000003):
        x = torch.randn(n + 4, device=DEV)[:n] * 3.0
        x = x.clone()
        wire = torch.empty(n, dtype=torch.bfloat16, device=DEV)
        call("cswin_pack_bf16", ptr(x), ptr(wire), n, stream())
        assert torch.equal(wire, x.to(torch.bfloat16))
        back = torch.empty(n, dtype=torch.float32, device=DEV)
        call("cswin_unpack_bf16", ptr(wire), ptr(back), n, stream())
        assert torch.equal(back, wire.float())


# ------------------------------------------------------------------------------------------------------------------
# boundary holes closed in round 2: nn.Dropout sites (drop_rate > 0), DiceLoss(softmax=False, weight=...)
# ------------------------------------------------------------------------------------------------------------------
def _dropout_factor(shape, p, seed):
    """The mask / (1 - p) tensor cswin_dropout applies for this seed (extracted by running the kernel on ones)."""
    from cswin_unet_amd._lib import call, ptr, stream
    ones = torch.ones(shape, device=DEV)
    out = torch.empty_like(ones)
    from cswin_unet_amd.ops import dropout_epoch                   # the device-resident epoch every dropout launch of ops adds to its seed
    call("cswin_dropout", ptr(ones), None, None, ptr(out), ones.numel(), ones.numel() // shape[0], float(p), int(seed),
         ptr(dropout_epoch(ones.device)), stream())
    return out


def test_dropout_kernel_statistics_and_backward(ops):
    p, seed = 0.3, 123456789
    x = T(det_normal("drop.x", (4, 196, 256)), grad=True)
    res = T(det_normal("drop.res", (4, 196, 256)), grad=True)
    rs = torch.tensor([1.0, 0.0, 2.5, 1.25], device=DEV)
    f = _dropout_factor((4, 196, 256), p, seed)
    keep = (f > 0).float().mean().item()
    assert abs(keep - (1 - p)) < 5e-3 and set(torch.unique(f).tolist()) == {0.0, float(np.float32(1.0) / np.float32(1 - p))}
    assert not torch.equal(f, _dropout_factor((4, 196, 256), p, seed + 1))          # another seed, another mask
    y = ops.dropout(x, p, residual=res, row_scale=rs, seed=seed)
    ref = res + rs[:, None, None] * f * x
    assert torch.allclose(y, ref, rtol=1e-6, atol=1e-6)
    dy = T(det_normal("drop.dy", (4, 196, 256)))
    y.backward(dy)
    assert torch.allclose(x.grad, rs[:, None, None] * f * dy, rtol=1e-6, atol=1e-6) and torch.equal(res.grad, dy)


def test_block_with_drop_rate_matches_composition(N, ops):
    """CSWinBlock with drop_rate > 0 (live proj_drop and Mlp.drop, cswin_unet.py:25,27,135) against the same block computed by
    the oracle with the masks the kernels drew (parity of the random stream itself is unpinned, as for DropPath)."""
    dim, reso, heads, split, p = 128, 28, 4, 2, 0.25
    blk = N.CSWinBlock(dim, reso, heads, split, qkv_bias=True, drop=p).to(DEV)
    fill_state_dict(blk).train()
    x = T(det_normal("dropblk.x", (2, reso * reso, dim)), grad=True)
    # seeds: 11 proj_drop, 22 Mlp.drop after GELU, 33 Mlp.drop after fc2
    import cswin_unet_amd.ops as O_
    real_dropout, real_draw = O_.dropout, O_._draw_seeds
    O_.dropout = lambda x_, p_, residual=None, row_scale=None, seed=None: real_dropout(x_, p_, residual, row_scale, 11)
    O_._draw_seeds = lambda n: (22, 33)
    try:
        y = blk(x)
        dy = T(det_normal("dropblk.dy", tuple(y.shape)))
        y.backward(dy)
    finally:
        O_.dropout, O_._draw_seeds = real_dropout, real_draw
    f1 = _dropout_factor((2, reso * reso, dim), p, 11).cpu()
    f2 = _dropout_factor((2, reso * reso, 4 * dim), p, 22).cpu()
    f3 = _dropout_factor((2, reso * reso, dim), p, 33).cpu()
    P = {k: v.detach().cpu().clone().requires_grad_() for k, v in blk.state_dict().items()}
    xr = x.detach().cpu().clone().requires_grad_()
    yr = O.cswin_block(xr, P, "", dim, reso, heads, split, drop_factors=(f1, f2, f3))
    yr.backward(dy.cpu())
    rel_err(y, yr, "dropblk.y")
    rel_err(x.grad, xr.grad, "dropblk.dx")
    for n in ("qkv.weight", "proj.weight", "mlp.fc1.weight", "mlp.fc2.bias", "norm2.weight"):
        rel_err(dict(blk.named_parameters())[n].grad, P[n].grad, "dropblk.grad." + n)


@pytest.mark.parametrize("dim,reso,heads,split,last", [(64, 14, 2, 7, False), (128, 7, 4, 7, True)])
def test_fused_block_equals_fine_grained_composition(N, ops, dim, reso, heads, split, last):
    """The one-node block (ops.cswin_block) against the same block composed from the public fine-grained ops -- the form a block
    with drop_rate > 0 takes -- with the same parameters and given per-sample DropPath factors, fp32 mode, B = 2.  Two branches at
    M = 392; one branch at M = 98, no multiple of the 64-row tile (the weight-gradient batch's unaligned route).  Both forms issue
    the same forward launches with the same arguments: y is bit-identical.  The fused backward takes the qkv data gradient from
    the tail kernel's fixed tile, the composition from the GEMM heuristic (another summation order): dx and every parameter
    gradient agree to the suite's bound."""
    blk = N.CSWinBlock(dim, reso, heads, split, qkv_bias=True, last_stage=last).to(DEV)
    fill_state_dict(blk)
    a, n1, n2, fc1, fc2 = blk.attns, blk.norm1, blk.norm2, blk.mlp.fc1, blk.mlp.fc2
    idx, hd, lw, lb = [m.idx for m in a], [m.num_heads for m in a], [m.get_v.weight for m in a], [m.get_v.bias for m in a]
    rs1, rs2 = torch.tensor([1.25, 0.5], device=DEV), torch.tensor([0.75, 1.5], device=DEV)
    x0 = det_normal(f"fusedcomp.{dim}.x", (2, reso * reso, dim))
    dy = T(det_normal(f"fusedcomp.{dim}.dy", (2, reso * reso, dim)))

    def fused(x):
        return ops.cswin_block(x, reso, split, idx, hd, a[0].scale, n1, blk.qkv, blk.proj, n2, fc1, fc2, lw, lb, rs1, rs2)

    def composed(x):
        qkv = ops.linear(ops.layer_norm(x, n1.weight, n1.bias, n1.eps), blk.qkv.weight, blk.qkv.bias)
        att = ops.stripe_attention(qkv, reso, split, idx, hd, lw, lb, a[0].scale)
        x1 = ops.linear(att, blk.proj.weight, blk.proj.bias, residual=x, row_scale=rs1)
        return ops.mlp(ops.layer_norm(x1, n2.weight, n2.bias, n2.eps), fc1.weight, fc1.bias, fc2.weight, fc2.bias, residual=x1, row_scale=rs2)

    def run(form):
        blk.zero_grad(set_to_none=True)
        x = T(x0, True)
        y = form(x)
        y.backward(dy)
        return y.detach(), x.grad, {n: p.grad for n, p in blk.named_parameters()}

    (y, dx, g), (yc, dxc, gc) = run(fused), run(composed)
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    with open(LOG, "a") as f:
        f.write(f"fusedcomp.c{dim}.y max|diff| {float((y - yc).abs().max()):.3e}\n")
    assert torch.equal(y, yc)
    rel_err(dx, dxc, f"fusedcomp.c{dim}.dx")
    assert len(g) == len(gc) == len(list(blk.parameters()))
    for n in g:
        rel_err(g[n], gc[n], f"fusedcomp.c{dim}.grad.{n}")


@pytest.mark.parametrize("reso,idx,split,dim,heads", [(28, 1, 2, 128, 4), (14, 0, 7, 256, 8), (7, -1, 7, 512, 16), (24, 1, 12, 64, 2)])
def test_attention_probability_dropout(ops, reso, idx, split, dim, heads):
    """attn_drop_rate > 0 (nn.Dropout on the softmax matrix, cswin_unet.py:57,101): the mask is a counter-based hash inside the
    kernels, regenerated by the backward (fused kernel; large-window kernels for reso 24).  Parity of the random stream with
    torch is unpinned, as for every dropout; what is pinned:
      * statistics: with q = k = 0 (uniform P = 1/N), v = 1 and no LePE, y = (kept keys) / (N (1 - p)): mean 1, variance
        p / ((1 - p) N) over the queries;
      * the backward is the derivative of THIS forward (same seed): directional derivative by central differences;
      * p = 0 is the plain kernel (bit-identical)."""
    import ctypes
    from cswin_unet_amd._lib import call, lib, ptr, stream
    from cswin_unet_amd.ops import _int_array, _ptr_array
    B, p_drop, seed = 2, 0.25, 1234567
    C = dim if idx == -1 else dim // 2
    nh = heads if idx == -1 else heads // 2
    L = reso * reso
    Ntok = L if idx == -1 else reso * split
    ha, ia = _int_array([nh]), _int_array([idx])
    E = lambda *sh: torch.empty(*sh, dtype=torch.float32, device=DEV)
    nbytes = lib().cswin_attn_bwd_workspace(B, reso, C, 1, ha, ia, split)

    def fwd(qkv, lw, lb, p, sd, want_y0=False):
        y, z, lse = E(B, L, C), E(B, L, C), E(B, nh, L)
        call("cswin_attn_fwd", ptr(qkv), _ptr_array([lw]), _ptr_array([lb]), ptr(y), ptr(z) if want_y0 else None, ptr(lse), B, reso, C, 1, ha, ia,
             split, 0.0, p, sd, None, 0, stream())
        return (y, lse, z) if want_y0 else (y, lse)

    # statistics
    qkv = torch.zeros(B, L, 3 * C, device=DEV)
    qkv[..., 2 * C:] = 1.0
    zw, zb = torch.zeros(C, 9, device=DEV), torch.zeros(C, device=DEV)
    y, _ = fwd(qkv, zw, zb, p_drop, seed)
    vals = y[..., ::32].double()                 # one channel per head: all channels of a head share the mask
    n = vals.numel()
    var = p_drop / ((1 - p_drop) * Ntok)
    assert abs(float(vals.mean()) - 1.0) < 5 * (var / n) ** 0.5 + 1e-6
    assert abs(float(vals.var()) / var - 1.0) < 0.15
    y2, _ = fwd(qkv, zw, zb, p_drop, seed + 1)
    assert not bool((y2 == y).all()), "another seed drew the same mask"
    # gradient consistency
    qkv = T(det_normal(f"adrop.{reso}.qkv", (B, L, 3 * C)) * 0.7)
    lw, lb = T(det_normal(f"adrop.{reso}.lw", (C, 9)) * 0.3), T(det_normal(f"adrop.{reso}.lb", (C,)) * 0.1)
    dy, d = T(det_normal(f"adrop.{reso}.dy", (B, L, C))), T(det_normal(f"adrop.{reso}.dir", (B, L, 3 * C)))
    y, lse, z = fwd(qkv, lw, lb, p_drop, seed, want_y0=True)
    dq, dw_, db_, ws = E(B, L, 3 * C), E(C, 9), E(C), E(nbytes // 4 + 4)
    call("cswin_attn_bwd", ptr(qkv), _ptr_array([lw]), _ptr_array([lb]), ptr(lse), ptr(z), ptr(dy), ptr(dq), _ptr_array([dw_]),
         _ptr_array([db_]), ptr(ws), nbytes, B, reso, C, 1, ha, ia, split, 0.0, None, p_drop, seed, None, 0, stream())
    eps = 1e-2
    yp, _ = fwd(qkv + eps * d, lw, lb, p_drop, seed)
    ym, _ = fwd(qkv - eps * d, lw, lb, p_drop, seed)
    num = float(((yp.double() - ym.double()) * dy.double()).sum()) / (2 * eps)
    ana = float((dq.double() * d.double()).sum())
    assert abs(num - ana) < 2e-3 * (abs(ana) + float(dq.double().norm() * d.double().norm()) * 1e-2), (num, ana)
    # p = 0 is the plain kernel
    y0, _ = fwd(qkv, lw, lb, 0.0, seed)
    yref = ops.stripe_attention(qkv, reso, split, [idx], [nh], [lw.view(C, 1, 3, 3)], [lb])
    assert bool((y0 == yref).all())


def test_block_attn_drop_runs_and_is_seeded(N):
    """CSWinBlock(attn_drop > 0).train(): forward / backward run through the fused block op (no NotImplementedError any more),
    torch.manual_seed reproduces the draw, eval() is deterministic and equals attn_drop = 0."""
    blk = N.CSWinBlock(128, 28, 4, 2, qkv_bias=True, attn_drop=0.2).to(DEV)
    fill_state_dict(blk)
    x = T(det_normal("adropblk.x", (2, 28 * 28, 128)), True)
    blk.train()
    torch.manual_seed(5)
    y1 = blk(x)
    y1.backward(T(det_normal("adropblk.dy", tuple(y1.shape))))
    assert x.grad is not None and bool(torch.isfinite(x.grad).all())
    torch.manual_seed(5)
    y2 = blk(x)
    torch.manual_seed(6)
    y3 = blk(x)
    assert bool((y1 == y2).all()) and not bool((y1 == y3).all())
    blk.eval()
    ref = N.CSWinBlock(128, 28, 4, 2, qkv_bias=True, attn_drop=0.0).to(DEV)
    fill_state_dict(ref)
    ref.eval()
    assert bool((blk(x) == ref(x)).all())


def test_dice_loss_probabilities_and_class_weights():
    """utils.DiceLoss(n)(probs, target, weight=w, softmax=False) (utils.py:32-45) vs a direct restatement."""
    from cswin_unet_amd.utils import DiceLoss
    ncls = 4
    logits = det_normal("dicew.logits", (2, ncls, 24, 24))
    lab = det_labels("dicew.lab", (2, 24, 24), ncls)
    w = [0.5, 1.0, 2.0, 0.25]

    def restated(pr, target):
        loss = 0.0
        for c in range(ncls):
            t = (target == c).float()
            loss = loss + w[c] * (1 - (2 * (pr[:, c] * t).sum() + 1e-5) / ((pr[:, c] ** 2).sum() + (t * t).sum() + 1e-5))
        return loss / ncls
    probs = T(torch.softmax(torch.from_numpy(logits), 1).numpy(), grad=True)
    loss = DiceLoss(ncls)(probs, T(lab), weight=w, softmax=False)
    loss.backward()
    pr = torch.softmax(torch.from_numpy(logits), 1).requires_grad_()
    ref = restated(pr, torch.from_numpy(lab))
    ref.backward()
    assert abs(float(loss) - float(ref)) < 1e-5
    rel_err(probs.grad, pr.grad, "dicew.dprobs")
    lg = T(logits, grad=True)                                   # softmax=True with weights
    loss2 = DiceLoss(ncls)(lg, T(lab), weight=w, softmax=True)
    loss2.backward()
    lr_ = torch.from_numpy(logits).requires_grad_()
    ref2 = restated(torch.softmax(lr_, 1), torch.from_numpy(lab))
    ref2.backward()
    assert abs(float(loss2) - float(ref2)) < 1e-5
    rel_err(lg.grad, lr_.grad, "dicew.dlogits")


@pytest.mark.parametrize("shapes", [[(4704, 256, 1024), (4704, 1024, 256), (4704, 256, 256), (4704, 768, 256)],
                                    [(75264, 64, 256), (75264, 192, 64)], [(1176, 512, 2048)], [(777, 132, 100), (3000, 64, 64)]])
def test_linear_weight_gradient_batch_bf16(bf16_matmul, shapes):
    """bf16 matmul mode of cswin_linear_bwd_weight_batch (csrc/wgrad16.hip: transposing LDS reads + bf16 MFMA, fp32 accumulate).
    Two bounds: (a) against the same product of the bf16-ROUNDED operands in fp32 -- what the kernel is specified to compute --
    1e-4 of RMS (only the summation order differs); (b) against the exact fp32 product: operand rounding is 2^-9 relative
    per factor, random in sign, so the result is within ~2^-8 of its RMS: bound 1e-2."""
    import ctypes
    from cswin_unet_amd._lib import ReduceJob, WgradDesc, call, lib, stream
    n = len(shapes)
    wg, jobs, keep, refs = (WgradDesc * n)(), (ReduceJob * n)(), [], []
    for i, (M, N_, K) in enumerate(shapes):
        dy, x = det_normal(f"wb16.dy{i}", (M, N_)), det_normal(f"wb16.x{i}", (M, K))
        rps = (M + 2) // 3
        rs = np.array([0.0, 1.25, 0.5], np.float32) if i % 2 == 0 else None
        with_bias = i != 1
        dyd, xd = T(dy), T(x)
        rsd = T(rs) if rs is not None else None
        dw = torch.empty(N_, K, device=DEV)
        db = torch.empty(N_, device=DEV) if with_bias else None
        nbytes = lib().cswin_linear_bwd_weight_workspace(M, N_, K)
        ws = torch.empty(nbytes // 4 + 4, device=DEV)
        keep += [dyd, xd, rsd, ws]
        wg[i].dy, wg[i].x, wg[i].row_scale = dyd.data_ptr(), xd.data_ptr(), (rsd.data_ptr() if rsd is not None else None)
        wg[i].dw, wg[i].dbias, wg[i].workspace, wg[i].ws_bytes = dw.data_ptr(), (db.data_ptr() if with_bias else None), ws.data_ptr(), nbytes
        wg[i].rows_per_sample, wg[i].M, wg[i].N, wg[i].K, wg[i].precision = rps, M, N_, K, 1
        scale = np.ones((M, 1), np.float32) if rs is None else np.array([rs[m // rps] for m in range(M)], np.float32)[:, None]
        dys = torch.from_numpy(dy * scale)
        xt = torch.from_numpy(x)
        r16 = lambda t: t.to(torch.bfloat16).to(torch.float64)
        refs.append((dw, db, (r16(dys).T @ r16(xt)).float(), (dys.double().T @ xt.double()).float(), dys.double().sum(0).float()))
    call("cswin_linear_bwd_weight_batch", ctypes.cast(wg, ctypes.c_void_p), n, ctypes.cast(jobs, ctypes.c_void_p), None, 0, stream())
    call("cswin_rows_sum_multi", ctypes.cast(jobs, ctypes.c_void_p), n, stream())
    for i, (dw, db, ref16, ref32, db_ref) in enumerate(refs):
        got = dw.cpu()
        rms = float(ref32.pow(2).mean().sqrt())
        e16, e32 = float((got - ref16).abs().max()) / rms, float((got - ref32).abs().max()) / rms
        # max over up to 1e6 elements of an error with sigma = sqrt(2) * 2^-9 / sqrt(3) = 1.6e-3 of the RMS: 8 sigma
        assert e16 < 1e-4 and e32 < 1.3e-2, (i, shapes[i], e16, e32)
        if db is not None:                                   # the bias gradient is summed in fp32 from the fp32 dy
            assert float((db.cpu() - db_ref).abs().max()) / float(db_ref.pow(2).mean().sqrt() + 1e-30) < 1e-4, i
