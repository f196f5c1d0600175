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
