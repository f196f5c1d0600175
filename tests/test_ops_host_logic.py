"""The host logic of ops.py without a device: every Function body of a training step runs on CPU tensors with the three module
globals that touch the GPU replaced -- `call` records instead of launching, `dev_f32` only makes tensors contiguous, `stream`
returns no stream.  The buffers hold garbage (nothing is computed); what is checked is the plumbing: autograd reaches every
parameter with a gradient of its shape, and every launch passes exactly the arguments its C signature lists.  The built library
is needed for the host-side workspace queries only (as in test_abi.test_workspace_queries_are_host_only)."""
import pytest
import torch


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_model_step_host_logic(monkeypatch, mode):
    from cswin_unet_amd import _lib, ops
    from cswin_unet_amd.networks.cswin_unet import CSWinTransformer
    calls = []
    monkeypatch.setattr(ops, "call", lambda name, *args: calls.append((name, args)))
    monkeypatch.setattr(ops, "dev_f32", lambda t, what="tensor": None if t is None else t.contiguous())
    monkeypatch.setattr(ops, "stream", lambda: None)
    prev = _lib.set_precision(_lib.PREC_BF16 if mode == "bf16" else _lib.PREC_FP32)
    try:
        torch.manual_seed(0)
        net = CSWinTransformer(img_size=224, num_classes=9, embed_dim=64, depth=[1, 1, 1, 1], split_size=[1, 2, 7, 7],
                               num_heads=[2, 4, 8, 16], qkv_bias=True, drop_path_rate=0.1).train()
        loss, _ = ops.ce_dice_loss(net(torch.randn(1, 3, 224, 224)), torch.randint(0, 9, (1, 224, 224)))
        loss.backward()
    finally:
        _lib.set_precision(prev)
        ops.clear_twins()
    params = dict(net.named_parameters())
    assert len(params) == 175
    for n, p in params.items():
        assert p.grad is not None and p.grad.shape == p.shape, n
    assert {"cswin_linear_fwd", "cswin_attn_bwd", "cswin_layernorm_bwd", "cswin_loss_bwd"} <= {name for name, _ in calls}
    for name, args in calls:
        assert len(args) == len(_lib.SIGNATURES[name][1]), (name, len(args))


# (B, HW, ncls, world, kd_weight, T): world 1 and 2, kd_weight 0, 1 and between, HW odd and a power of two
SCALE_CASES = [(3, 91, 9, 1, 0.5, 3.0), (24, 224 * 224, 12, 2, 0.0, 1.0), (2, 513 * 513, 2, 2, 1.0, 2.5)]


@pytest.mark.parametrize("B,HW,ncls,world,kd_weight,temperature", SCALE_CASES)
def test_gradient_scales_are_the_expressions_of_the_two_former_functions(B, HW, ncls, world, kd_weight, temperature):
    """The floats the objectives hand to cswin_loss_bwd / cswin_cl_loss_bwd, == against the expressions _CeDiceLoss and
    _ContinualLoss kept in ctx.meta before the objectives existed (and HipEngine._loss_grad wrote out a second time)."""
    import types
    from cswin_unet_amd import ops
    w_ce, w_dice, w_focal = 0.4, 0.6, 0.2
    got = ops.CeDiceObjective(w_ce, w_dice).grad_scales(B, HW, ncls, world)
    assert got == (w_ce / float(B * HW), w_dice / ncls * world)
    spec = types.SimpleNamespace(w_focal=w_focal, w_dice=w_dice, kd_weight=kd_weight, temperature=temperature)
    got = ops.ContinualObjective(spec).grad_scales(B, HW, ncls, world)
    assert got == ((1.0 - kd_weight) * w_focal / float(B * HW), (1.0 - kd_weight) * w_dice / ncls * world, kd_weight * temperature / B)
    keep = 1.0 - kd_weight                                   # the engine's former spelling, on logits of B * ncls * HW elements
    assert got == (keep * w_focal / float((B * ncls * HW) // ncls), keep * w_dice / ncls * world, kd_weight * temperature / B)
    spec.kd_weight = 0.25                                    # read at call time
    assert ops.ContinualObjective(spec).grad_scales(B, HW, ncls, world)[2] == 0.25 * temperature / B
