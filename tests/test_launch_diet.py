"""GPU tests of the entry points that took launches out of the training step, each against the path it replaced (which stays
callable through its own entry points):
  * CARAFE reassembly writing / reading (B, C, SH, SW) planes  vs  token reassembly + cswin_tokens_to_nchw / cswin_nchw_to_tokens
  * all convolution weight images in one launch               vs  cswin_conv_weight_permute / _flipT
  * the channel-padded convolution weight gradient             vs  cswin_conv_tok_bwd_weight + cswin_conv_weight_unpermute
  * the composed head weight / bias and their three gradients  vs  the torch composition (matmul_nn, linear, pad)
Data movement is compared with torch.equal; the composition, whose dot products run in another order, at the suite's 1e-3
max|diff| / RMS bound (measured on MI355X: composed weight 7.4e-7, bias 2.2e-7, the three gradients 8.8e-8 to 3.8e-7)."""
import ctypes

import numpy as np
import pytest
import torch

from oracle.determ import det_normal

pytestmark = pytest.mark.gpu
RTOL = 1e-3
DEV = "cuda"


def T(name, shape, grad=False, scale=1.0):
    t = (torch.from_numpy(np.ascontiguousarray(det_normal(name, shape))) * scale).to(DEV)
    return t.requires_grad_() if grad else t


def rel_err(got, ref, what):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    err = float((got - ref).abs().max()) / (float(ref.pow(2).mean().sqrt()) + 1e-30)
    print(f"{what}: max|diff|/rms = {err:.3e}")
    assert np.isfinite(err) and err <= RTOL, f"{what}: max|diff|/rms = {err:.3e} > {RTOL}"
    return err


@pytest.fixture(scope="module")
def ops():
    from cswin_unet_amd import ops
    return ops


@pytest.mark.parametrize("ncls", [9, 5, 16])
def test_carafe4_nchw_forward_and_backward_bit_exact(ops, ncls):
    B, H, S, Cz = 2, 16, 4, 16
    assert ops.lib().cswin_carafe_bwd_nchw_ok(H, H, Cz, S) == 1
    e0, z0, b0 = T("diet.e", (B, H * H, 9 * S * S)), T("diet.z", (B, H * H, Cz)), T("diet.b", (Cz,))
    z0[..., ncls:] = 0                                  # what a weight padded with zero rows gives
    b0[ncls:] = 0
    g = T("diet.g", (B, ncls, S * H, S * H))
    res = []
    for new in (False, True):
        e, z, b = (t.clone().requires_grad_() for t in (e0, z0, b0))
        if new:
            out = ops.carafe_reassemble_nchw(e, z, b, H, H, S, ncls)
        else:
            out = ops.tokens_to_nchw(ops.carafe_reassemble(e, z, b, H, H, S), ncls, S * H, S * H)
        out.backward(g)
        res.append((out.detach(), e.grad, z.grad, b.grad))
    for name, old, got in zip(("out", "de", "dz", "dbias"), *res):
        assert torch.equal(old, got), f"{name} (ncls={ncls}): max|diff| {float((old - got).abs().max()):.3e}"


@pytest.mark.parametrize("S,Cz,C,H,W", [(2, 32, 7, 9, 11), (4, 16, 9, 5, 7), (2, 128, 128, 6, 6)])
def test_carafe_nchw_forward_any_shape_bit_exact(ops, S, Cz, C, H, W):
    """The forward kernel alone (the backward form exists for the head's shape only): odd maps, S = 2, C == Cz."""
    from cswin_unet_amd._lib import call, ptr, stream
    B = 3
    e, z, b = T("diet.e2", (B, H * W, 9 * S * S)), T("diet.z2", (B, H * W, Cz)), T("diet.b2", (Cz,))
    tok, wt0 = torch.empty(B, H * W * S * S, Cz, device=DEV), torch.empty_like(e)
    call("cswin_carafe_fwd", ptr(e), ptr(z), ptr(b), ptr(tok), ptr(wt0), B, H, W, Cz, S, stream())
    ref = torch.empty(B, C, S * H, S * W, device=DEV)
    call("cswin_tokens_to_nchw", ptr(tok), ptr(ref), B, C, S * H, S * W, Cz, stream())
    out, wt1 = torch.full_like(ref, float("nan")), torch.empty_like(e)
    call("cswin_carafe_fwd_nchw", ptr(e), ptr(z), ptr(b), ptr(out), ptr(wt1), B, H, W, Cz, C, S, stream())
    assert torch.equal(out, ref) and torch.equal(wt0, wt1)


CONVS = [(64, 3, 7, 4, 4, 2), (128, 64, 3, 64, 2, 1), (256, 128, 3, 128, 2, 1), (36, 128, 3, 128, 1, 1), (144, 16, 3, 16, 1, 1)]


def _single_images(w, cpad, want_flip):
    from cswin_unet_amd._lib import call, ptr, stream
    Cout, Cin, ks, _ = w.shape
    wp, wpt = torch.empty(Cout, ks * ks, cpad, device=DEV), torch.empty(ks * ks, Cout, cpad, device=DEV)
    call("cswin_conv_weight_permute", ptr(w), ptr(wp), ptr(wpt), Cout, Cin, ks, cpad, stream())
    wf = None
    if want_flip:
        wf = torch.empty(Cin, ks * ks, Cout, device=DEV)
        call("cswin_conv_weight_flipT", ptr(w), ptr(wf), Cout, Cin, ks, stream())
    return wp, wpt, wf


def test_conv_weight_images_one_launch_bit_exact(ops):
    ws = [T(f"diet.w{i}", (co, ci, ks, ks)) for i, (co, ci, ks, _, _, _) in enumerate(CONVS)]
    specs = [(w, c[3], c[4], c[5]) for w, c in zip(ws, CONVS)]
    for round_ in range(2):                             # second round: the weights were changed from outside (checkpoint load)
        if round_:
            with torch.no_grad():
                for i, w in enumerate(ws):
                    w.copy_(T(f"diet.w{i}.reloaded", tuple(w.shape)))
        with ops.conv_weight_images(specs):
            for w, (co, ci, ks, cpad, stride, pad) in zip(ws, CONVS):
                wp, wpt, wf = ops._images_of(w, cpad)
                same, image_input = stride == 1, cpad != ci          # an image input takes no gradient: forward image only
                rp, rpt, rf = _single_images(w, cpad, same)
                assert torch.equal(wp, rp)
                assert (wpt is None) == (same or image_input) and (wpt is None or torch.equal(wpt, rpt))
                assert (wf is None) != same and (not same or torch.equal(wf, rf))
        assert ops._images_of(ws[0], CONVS[0][3]) is None       # the images belong to the pass that made them


@pytest.mark.parametrize("co,ci,ks,cpad,stride,pad", CONVS[1:])
def test_conv_tokens_with_prepared_images_bit_exact(ops, co, ci, ks, cpad, stride, pad):
    B, H = 2, 12
    w0, b0, x0 = T("diet.cw", (co, ci, ks, ks)), T("diet.cb", (co,)), T("diet.cx", (B, H * H, ci))
    res = []
    for prepared in (False, True):
        w, b, x = (t.clone().requires_grad_() for t in (w0, b0, x0))
        if prepared:
            with ops.conv_weight_images([(w, cpad, stride, pad)]):
                y = ops.conv_tokens(x, w, b, H, H, stride, pad)
        else:
            y = ops.conv_tokens(x, w, b, H, H, stride, pad)
        y.backward(torch.ones_like(y) * 0.5 + y.detach())
        res.append((y.detach(), x.grad, w.grad, b.grad))
    for name, old, got in zip(("y", "dx", "dw", "db"), *res):
        assert torch.equal(old, got), name


@pytest.mark.parametrize("B,H,cin", [(2, 32, 3), (24, 224, 3), (2, 32, 1)])
def test_patch_embed_weight_gradient_without_unpermute_bit_exact(ops, B, H, cin):
    """cswin_conv_tok_bwd_weight_cpad vs slab reduction to the padded image + cswin_conv_weight_unpermute: same sums in the
    same order (few or many split-K slabs), the padded channel dropped."""
    from cswin_unet_amd._lib import call, lib, precision, ptr, stream
    Cout, ks, stride, pad, cpad = 64, 7, 4, 2, 4
    OH = (H + 2 * pad - ks) // stride + 1
    x = T("diet.px", (B, H * H, cpad))
    x[..., cin:] = 0
    dy = T("diet.pdy", (B, OH * OH, Cout))
    nbytes = lib().cswin_conv_tok_bwd_weight_workspace(B, H, H, cpad, Cout, ks, stride, pad)
    ws = torch.empty(nbytes // 4 + 4, device=DEV)
    dwp, db0 = torch.empty(Cout, ks * ks, cpad, device=DEV), torch.empty(Cout, device=DEV)
    call("cswin_conv_tok_bwd_weight", ptr(dy), ptr(x), ptr(dwp), ptr(db0), ptr(ws), nbytes, B, H, H, cpad, Cout, ks, stride, pad, 0,
         None, precision(), stream())
    dw0 = torch.empty(Cout, cin, ks, ks, device=DEV)
    call("cswin_conv_weight_unpermute", ptr(dwp), ptr(dw0), Cout, cin, ks, cpad, stream())
    for deferred in (False, True):
        dw1, db1 = torch.full_like(dw0, float("nan")), torch.full_like(db0, float("nan"))
        job = (ops.ReduceJob * 1)()
        call("cswin_conv_tok_bwd_weight_cpad", ptr(dy), ptr(x), ptr(dw1), ptr(db1), ptr(ws), nbytes, B, H, H, cpad, cin, Cout, ks,
             stride, pad, ctypes.cast(job, ctypes.c_void_p) if deferred else None, precision(), stream())
        if deferred:
            call("cswin_rows_sum_multi", ctypes.cast(job, ctypes.c_void_p), 1, stream())
        assert torch.equal(dw1, dw0) and torch.equal(db1, db0), deferred


@pytest.mark.parametrize("ncls,E,C", [(9, 64, 64), (4, 96, 96), (16, 64, 32)])
def test_head_compose_vs_torch_composition(ops, ncls, E, C):
    cpad = max(16, 1 << (ncls - 1).bit_length())
    wh0, wo0, bo0 = T("diet.wh", (ncls, E, 1, 1), scale=0.1), T("diet.wo", (E, C, 1, 1), scale=0.1), T("diet.bo", (E,))
    gw, gb = T("diet.gw", (cpad, C)), T("diet.gb", (cpad,))
    res = []
    for new in (False, True):
        wh, wo, bo = (t.clone().requires_grad_() for t in (wh0, wo0, bo0))
        if new:
            wf, bf = ops.head_compose(wh, wo, bo, cpad)
        else:
            w_head = wh.flatten(1)
            wf = torch.nn.functional.pad(ops.matmul_nn(w_head, wo.flatten(1)), (0, 0, 0, cpad - ncls))
            bf = torch.nn.functional.pad(ops.linear(bo[None, :], w_head)[0], (0, cpad - ncls))
        torch.autograd.backward([wf, bf], [gw, gb])
        res.append((wf.detach(), bf.detach(), wh.grad, wo.grad, bo.grad))
    assert torch.equal(res[1][0][ncls:], torch.zeros(cpad - ncls, C, device=DEV)) and not res[1][1][ncls:].any()
    for name, old, got in zip(("w_fused", "b_fused", "d output.weight", "d out.weight", "d out.bias"), *res):
        rel_err(got, old, f"head_compose {name} (ncls={ncls})")
    # and against float64, which is what both approximate
    ref = (wh0.flatten(1).double() @ wo0.flatten(1).double())
    rel_err(res[1][0][:ncls], ref, "head_compose w_fused vs float64")


def test_model_step_places_head_gradients_in_the_flat_buffer(ops):
    """The head's three parameters are leaves of _HeadCompose: inside engine_backward their gradients are written straight into
    the optimiser's slots, and equal what a plain backward gives."""
    from cswin_unet_amd.networks.cswin_unet import CSWinTransformer
    from cswin_unet_amd.optim import FlatSGD
    from oracle.determ import det_labels, fill_state_dict
    net = CSWinTransformer(img_size=224, num_classes=9, embed_dim=64, depth=[1, 1, 1, 1], split_size=[1, 2, 7, 7],
                           num_heads=[2, 4, 8, 16], qkv_bias=True, drop_path_rate=0.).to(DEV)
    fill_state_dict(net)
    img, lab = T("diet.img", (2, 3, 224, 224)), torch.from_numpy(det_labels("diet.lab", (2, 224, 224), 9)).to(DEV)
    loss, _ = ops.ce_dice_loss(net(img), lab)
    loss.backward()
    plain = {k: p.grad.clone() for k, p in net.named_parameters()}
    opt = FlatSGD(net.parameters(), lr=0.01)
    opt.zero_grad()
    loss, _ = ops.ce_dice_loss(net(img), lab)
    with ops.engine_backward(opt):
        loss.backward()
    base = opt.flat_grad.data_ptr()
    offs = {p.data_ptr(): o for p, o in zip(opt.params, opt.offsets)}
    for k, p in net.named_parameters():
        if k in ("output.weight", "upsample1.out.weight", "upsample1.out.bias", "stage1_conv_embed.0.weight"):
            assert p.grad.data_ptr() == base + 4 * offs[p.data_ptr()], k
        assert torch.equal(p.grad, plain[k]), k
