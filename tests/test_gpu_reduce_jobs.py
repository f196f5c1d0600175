"""One slab reduction, two ways to run it: every weight-gradient entry point either reduces its split-M slabs at once
(deferred = NULL) or hands the job to the caller, who runs it later through cswin_rows_sum_multi.  Both go through the same
flagging of the job (16-B loads, few-rows mode, workgroup count), so for every kind of job the two must agree bit for bit:
  * plain jobs on the 16-row-group path (n < 4096 columns, or more slabs / fewer columns than the few-rows mode takes)
  * plain jobs in the few-rows mode (n >= 4096, <= 16 slabs, everything 16-B aligned)
  * convolution jobs that write the nn.Conv2d layout from the unpadded slab order (never few-rows)
  * channel-padded convolution jobs, which reduce as plain ones do, with and without the few-rows mode
All in fp32 through the C ABI; outputs are pre-filled with NaN, so a column nobody wrote shows."""
import ctypes

import numpy as np
import pytest
import torch

from oracle.determ import det_normal

pytestmark = pytest.mark.gpu
DEV = "cuda"
FP32 = 0


def T(name, shape):
    return torch.from_numpy(np.ascontiguousarray(det_normal(name, shape))).to(DEV)


def _both_ways(launch, outs):
    """launch(deferred) runs the entry point with the given `deferred` argument; returns the outputs of the immediate and of the
    deferred reduction."""
    from cswin_unet_amd._lib import ReduceJob, call, stream
    res = []
    for deferred in (False, True):
        for o in outs:
            o.fill_(float("nan"))
        job = (ReduceJob * 1)()
        launch(ctypes.cast(job, ctypes.c_void_p) if deferred else None)
        if deferred:
            assert job[0].part and job[0].rows >= 1
            call("cswin_rows_sum_multi", ctypes.cast(job, ctypes.c_void_p), 1, stream())
        torch.cuda.synchronize()
        res.append([o.clone() for o in outs])
    return res


def _assert_same(res, names, what):
    for name, now, later in zip(names, *res):
        assert not torch.isnan(now).any() and not torch.isnan(later).any(), f"{what}: {name} has unwritten elements"
        assert torch.equal(now, later), f"{what}: {name} differs, max|diff| {float((now - later).abs().max()):.3e}"


# (M, N, K): n = N*K + N columns; few-rows mode needs n >= 4096
@pytest.mark.parametrize("M,N,K", [(300, 72, 64), (37, 8, 128), (256, 64, 64)])
def test_linear_weight_gradient_reduction_now_or_deferred(M, N, K):
    from cswin_unet_amd._lib import call, lib, ptr, stream
    dy, x = T("reduce.dy", (M, N)), T("reduce.x", (M, K))
    nbytes = lib().cswin_linear_bwd_weight_workspace(M, N, K)
    ws = torch.empty(nbytes // 4 + 4, device=DEV)
    dw, db = torch.empty(N, K, device=DEV), torch.empty(N, device=DEV)

    def launch(deferred):
        call("cswin_linear_bwd_weight", ptr(dy), ptr(x), None, 0, None, 1, ptr(dw), ptr(db), ptr(ws), nbytes, M, N, K, deferred,
             FP32, stream())

    _assert_same(_both_ways(launch, [dw, db]), ("dw", "dbias"), f"linear M={M} N={N} K={K}")


def test_conv_weight_gradient_parameter_layout_reduction_now_or_deferred():
    from cswin_unet_amd._lib import call, lib, ptr, stream
    B, H, W, Cin, Cout, ks, stride, pad = 2, 8, 8, 8, 16, 3, 1, 1
    x, dy = T("reduce.cx", (B, H * W, Cin)), T("reduce.cdy", (B, H * W, Cout))
    nbytes = lib().cswin_conv_tok_bwd_weight_workspace(B, H, W, Cin, Cout, ks, stride, pad)
    ws = torch.empty(nbytes // 4 + 4, device=DEV)
    dw, db = torch.empty(Cout, Cin, ks, ks, device=DEV), torch.empty(Cout, device=DEV)

    def launch(deferred):
        call("cswin_conv_tok_bwd_weight", ptr(dy), ptr(x), ptr(dw), ptr(db), ptr(ws), nbytes, B, H, W, Cin, Cout, ks, stride, pad, 1,
             deferred, FP32, stream())

    _assert_same(_both_ways(launch, [dw, db]), ("dw", "dbias"), "conv, parameter layout")


# Cout = 64: n = 64 * 72 + 64 = 4672 >= 4096 columns in one slab, the few-rows mode; Cout = 16: n = 1168, the 16-row-group path
@pytest.mark.parametrize("Cout", [64, 16])
def test_conv_weight_gradient_channel_padded_reduction_now_or_deferred(Cout):
    from cswin_unet_amd._lib import call, lib, ptr, stream
    B, H, W, Cin, Cin_param, ks, stride, pad = 2, 8, 8, 8, 3, 3, 1, 1
    x, dy = T("reduce.px", (B, H * W, Cin)), T("reduce.pdy", (B, H * W, Cout))
    x[..., Cin_param:] = 0
    nbytes = lib().cswin_conv_tok_bwd_weight_workspace(B, H, W, Cin, Cout, ks, stride, pad)
    ws = torch.empty(nbytes // 4 + 4, device=DEV)
    dw, db = torch.empty(Cout, Cin_param, ks, ks, device=DEV), torch.empty(Cout, device=DEV)

    def launch(deferred):
        call("cswin_conv_tok_bwd_weight_cpad", ptr(dy), ptr(x), ptr(dw), ptr(db), ptr(ws), nbytes, B, H, W, Cin, Cin_param, Cout, ks,
             stride, pad, deferred, FP32, stream())

    _assert_same(_both_ways(launch, [dw, db]), ("dw", "dbias"), f"conv, channel-padded, Cout={Cout}")


def _carafe_buffers(B, H, W, Cz, S, C=None):
    """Inputs and outputs of a CARAFE backward: dout as tokens (C None) or as C class planes; wt_save from the forward."""
    from cswin_unet_amd._lib import call, lib, ptr, stream
    e, z = T("reduce.carafe.e", (B, H * W, 9 * S * S)), T("reduce.carafe.z", (B, H * W, Cz))
    dout = T("reduce.carafe.dout", (B, S * S * H * W, Cz) if C is None else (B, C, S * H, S * W))
    out, wt = torch.empty(B, S * S * H * W, Cz, device=DEV), torch.empty_like(e)
    call("cswin_carafe_fwd", ptr(e), ptr(z), None, ptr(out), ptr(wt), B, H, W, Cz, S, stream())
    nbytes = lib().cswin_carafe_bwd_workspace(B, H, W, Cz, S)
    ws = torch.empty(nbytes // 4 + 4, device=DEV)
    return dout, z, wt, torch.empty_like(e), torch.empty_like(z), torch.empty(Cz, device=DEV), ws, nbytes


def _job_after_call_without_dbias(launch):
    """The job a producer leaves when there is no bias gradient to reduce: part == NULL, whatever the slot held before."""
    from cswin_unet_amd._lib import ReduceJob
    job = (ReduceJob * 1)()
    ctypes.memset(job, 0xFF, ctypes.sizeof(job))
    launch(ctypes.cast(job, ctypes.c_void_p))
    torch.cuda.synchronize()
    assert not job[0].part and job[0].rows == 0


# Cz = 16 off the 8 x 8 tile: per-workgroup column sums from bwd_e; 512: the last width that has them; 516: colsum_partial_kernel
@pytest.mark.parametrize("Cz", [16, 512, 516])
def test_carafe_bias_gradient_reduction_now_or_deferred(Cz):
    from cswin_unet_amd._lib import call, ptr, stream
    B, H, W, S = 2, 5, 9, 2
    dout, z, wt, de, dz, db, ws, nbytes = _carafe_buffers(B, H, W, Cz, S)

    def launch(deferred, dbias=db):
        call("cswin_carafe_bwd", ptr(dout), ptr(z), ptr(wt), ptr(de), ptr(dz), ptr(dbias), ptr(ws), nbytes, B, H, W, Cz, S, deferred, stream())

    _assert_same(_both_ways(launch, [db]), ("dbias",), f"carafe Cz={Cz}")
    _job_after_call_without_dbias(lambda job: launch(job, None))


@pytest.mark.parametrize("C", [None, 9])
def test_carafe_fused_bias_gradient_reduction_now_or_deferred(C):
    """The fused backward on a 1 x 2 tile map, gradient as tokens (C None) and as nine class planes."""
    from cswin_unet_amd._lib import call, ptr, stream
    B, H, W, S, Cz = 2, 8, 16, 4, 16
    dout, z, wt, de, dz, db, ws, nbytes = _carafe_buffers(B, H, W, Cz, S, C)

    def launch(deferred, dbias=db):
        io = (ptr(dout), ptr(z), ptr(wt), ptr(de), ptr(dz), ptr(dbias), ptr(ws), nbytes, B, H, W, Cz)
        if C is None:
            call("cswin_carafe_bwd", *io, S, deferred, stream())
        else:
            call("cswin_carafe_bwd_nchw", *io, C, S, deferred, stream())

    _assert_same(_both_ways(launch, [db]), ("dbias",), f"fused carafe, {'tokens' if C is None else 'planes'}")
    _job_after_call_without_dbias(lambda job: launch(job, None))


# (257, 96): the one-wave-per-row kernel; (300, 32): a width with a kernel of its own
@pytest.mark.parametrize("M,C", [(257, 96), (300, 32)])
def test_layernorm_parameter_gradient_reduction_now_or_deferred(M, C):
    from cswin_unet_amd._lib import call, lib, ptr, stream
    x, dy, gamma, beta = T("reduce.ln.x", (M, C)), T("reduce.ln.dy", (M, C)), T("reduce.ln.g", (C,)), T("reduce.ln.b", (C,))
    y, mean, rstd = torch.empty_like(x), torch.empty(M, device=DEV), torch.empty(M, device=DEV)
    call("cswin_layernorm_fwd", ptr(x), ptr(gamma), ptr(beta), ptr(y), ptr(mean), ptr(rstd), M, C, 1e-5, 0, stream())
    nbytes = lib().cswin_layernorm_bwd_workspace(M, C)
    ws = torch.empty(nbytes // 4 + 4, device=DEV)
    dx, dg, db = torch.empty_like(x), torch.empty(C, device=DEV), torch.empty(C, device=DEV)

    def launch(deferred):
        call("cswin_layernorm_bwd", ptr(dy), ptr(x), ptr(mean), ptr(rstd), ptr(gamma), None, ptr(dx), ptr(dg), ptr(db), ptr(ws), nbytes, M, C,
             deferred, None, stream())

    _assert_same(_both_ways(launch, [dg, db]), ("dgamma", "dbeta"), f"layernorm M={M} C={C}")
