"""The eb-criterion mode of the surgical learning rates end to end (continual.surgical_lr_weights(method="eb-criterion"),
optim.FlatAdamW.tensor_evidence, HipEngine.set_lr_weights) on the depth-[1, 1, 1, 1] model, batch, teacher, label map and class
weights of tests/test_gpu_continual_step.py.  The statistic is held to test_eb_host's float64 reference and derived bound on the
.grad tensors of a plain backward of the same loss."""
import math

import numpy as np
import pytest
import torch

from test_eb_host import eb_bound, eb_ref
from test_gpu_adamw_step import BASE_LR, _trainer
from test_gpu_continual_step import _batch, _distill, _models

pytestmark = pytest.mark.gpu


def _kept(names):
    return [n for n in names if "bn" not in n.lower() and "norm" not in n.lower()]


def _second_batch():
    img, lab = _batch()
    return (0.5 * img.flip(-1)).contiguous(), lab.flip(-1).contiguous()


def _parent_surgical_lr_weights(model, opt, batches, distill):
    """continual.surgical_lr_weights as it was before it took a method, statement for statement."""
    from cswin_unet_amd import ops
    from cswin_unet_amd.continual import Distill, rgn_weights
    d = Distill.of(distill)
    names = dict((p.data_ptr(), n) for n, p in model.named_parameters())
    names = [names[p.data_ptr()] for p in opt.params]
    was_training = model.training
    model.eval()
    norms = []
    try:
        for img, lab in batches:
            logits = model(img)
            with torch.no_grad():
                teacher_logits = d.teacher(img).contiguous()
            loss, _ = ops.continual_loss(logits, lab, teacher_logits, w_focal=1.0, w_dice=0.0, kd_weight=0.0, temperature=d.temperature,
                                         focal_gamma=d.focal_gamma, focal_alpha=d.focal_alpha, class_weight=d.class_weight,
                                         label_map=d.label_map)
            opt.zero_grad()
            loss.backward()
            opt.gather_grads()
            norms.append(opt.tensor_norms())
            opt.zero_grad()
    finally:
        model.train(was_training)
    host = torch.stack(norms).cpu().tolist() if norms else []
    return rgn_weights(names, host)


@pytest.fixture(scope="module")
def runs():
    """One model and optimiser: the float64 statistic of a plain backward, then the function on one batch, on another and on both."""
    from cswin_unet_amd import ops
    from cswin_unet_amd.continual import surgical_lr_weights
    from cswin_unet_amd.optim import FlatAdamW
    img, lab = _batch()
    net, teacher = _models()
    d = _distill(teacher)
    opt = FlatAdamW(net.parameters(), lr=BASE_LR)
    names = [n for n, _ in net.named_parameters()]
    net.eval()
    with torch.no_grad():
        t = teacher(img).contiguous()
    loss, _ = ops.continual_loss(net(img), lab, t, w_focal=1.0, w_dice=0.0, kd_weight=0.0, temperature=d.temperature, focal_gamma=d.focal_gamma,
                                 focal_alpha=d.focal_alpha, class_weight=d.class_weight, label_map=d.label_map)
    loss.backward()
    ref = {}
    for n, p in net.named_parameters():
        g = p.grad.detach().cpu().numpy()
        ref[n] = (eb_ref(g, tuple(p.shape)), eb_bound(g, tuple(p.shape)), tuple(p.shape))
    opt.zero_grad()
    net.train()
    out = dict(names=names, ref=ref, net=net, opt=opt, d=d, state=(opt.scalars.clone(), opt.tensor_sumsq.clone(), opt.step_count))
    out["one"] = surgical_lr_weights(net, opt, [(img, lab)], d, method="eb-criterion", return_metrics=True)
    out["after_one"] = (net.training, all(p.grad is None for p in net.parameters()))
    out["other"] = surgical_lr_weights(net, opt, [_second_batch()], d, method="eb-criterion", return_metrics=True)
    out["both"] = surgical_lr_weights(net, opt, [(img, lab), _second_batch()], d, method="eb-criterion", return_metrics=True)
    return out


def test_metrics_against_float64_on_one_batch(runs):
    """Keys: the parameter names without "bn" / "norm", in order; every metric within eb_bound of eb_ref of the plain backward's
    .grad; the weights are eb_weights of the metrics, 0.0 or 1.0; training mode restored, every .grad None."""
    from cswin_unet_amd.continual import eb_weights
    weights, metrics = runs["one"]
    names, keep = runs["names"], _kept(runs["names"])
    assert list(weights) == keep and list(metrics) == keep and 0 < len(keep) < len(names)
    assert runs["after_one"] == (True, True)
    worst, nan = 0.0, 0
    for n in keep:
        ref, bound, shape = runs["ref"][n]
        if shape[0] == 1:
            assert math.isnan(ref) and math.isnan(metrics[n]), (n, metrics[n])
            nan += 1
            continue
        err = abs(metrics[n] - ref)
        assert math.isfinite(metrics[n]) and err <= bound, f"{n} {shape}: |{metrics[n]!r} - {ref!r}| = {err:.3e} > {bound:.3e}"
        worst = max(worst, err / bound if bound > 0 else 0.0)
    aligned = [metrics.get(n, 0.0) for n in names]
    assert weights == eb_weights(names, [aligned]) and set(weights.values()) <= {0.0, 1.0}
    assert all(weights[n] == (1.0 if metrics[n] >= 0.95 else 0.0) for n in keep)
    ones = sum(v == 1.0 for v in weights.values())
    print(f"eb-criterion on one batch: {len(keep)} of {len(names)} tensors, {ones} at or above 0.95, {len(keep) - ones} below ({nan} NaN); "
          f"largest |error| / bound {worst:.4f}; metric range {min(v for v in metrics.values() if v == v):.4g} .. {max(v for v in metrics.values() if v == v):.4g}")


def test_two_batches_give_the_mean_of_the_single_runs(runs):
    (_, m0), (_, m1), (w, m) = runs["one"], runs["other"], runs["both"]
    assert list(m) == list(m0) == list(m1) and any(m0[n] != m1[n] for n in m)
    for n in m:
        want = float(np.array([m0[n], m1[n]]).mean(0))
        assert m[n] == want or (math.isnan(m[n]) and math.isnan(want)), (n, m[n], want)
        assert w[n] == (1.0 if m[n] >= 0.95 else 0.0)


def test_rgn_and_the_default_are_unchanged(runs):
    """method="RGN" and the keyword left out give what the function gave before it took a method, as dicts with equal floats; the
    metrics of the RGN mode are the weights before the division by their maximum."""
    from cswin_unet_amd.continual import surgical_lr_weights
    net, opt, d = runs["net"], runs["opt"], runs["d"]
    batches = [_batch(), _second_batch()]
    want = _parent_surgical_lr_weights(net, opt, batches, d)
    assert max(want.values()) == 1.0
    assert surgical_lr_weights(net, opt, batches, d) == want
    got, ratios = surgical_lr_weights(net, opt, batches, d, method="RGN", return_metrics=True)
    assert got == want and list(got) == list(want) and list(ratios) == list(want)
    top = max(ratios.values())
    assert all(got[n] == ratios[n] / top for n in got)
    with pytest.raises(ValueError, match="method"):
        surgical_lr_weights(net, opt, batches, d, method="EB")
    assert net.training and all(p.grad is None for p in net.parameters())


def test_tensor_evidence_disturbs_and_allocates_nothing(runs):
    """scalars, tensor_sumsq and the step count are as they were before the first call; a second call allocates the result alone."""
    opt = runs["opt"]
    scalars, sumsq, steps = runs["state"]
    assert torch.equal(opt.scalars, scalars) and torch.equal(opt.tensor_sumsq, sumsq) and opt.step_count == steps == 0
    first = opt.tensor_evidence()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    second = opt.tensor_evidence()
    grown = torch.cuda.memory_allocated() - before
    torch.cuda.synchronize()
    assert second.shape == (len(opt.params),) and second.dtype == torch.float32 and second.device.type == "cuda"
    assert 0 < grown <= 4 * len(opt.params) + 512, grown                 # the caching allocator rounds a block up to 512 bytes
    assert torch.equal(first.view(torch.int32), second.view(torch.int32))
    del second
    assert torch.cuda.memory_allocated() == before
    assert torch.equal(opt.scalars, scalars) and torch.equal(opt.tensor_sumsq, sumsq) and opt.step_count == 0


def test_engine_freezes_what_the_criterion_drops():
    """HipEngine.set_lr_weights(weights) and one train_step: every tensor of weight 0 (the unnamed norm tensors included) keeps its
    bits, and a tensor of weight 1 moves if there is one."""
    from cswin_unet_amd.continual import surgical_lr_weights
    img, lab = _batch()
    net, teacher = _models()
    tr = _trainer(net, teacher, False)
    eng = tr.engine
    weights = surgical_lr_weights(net, eng.opt, [(img, lab)], eng.distill, method="eb-criterion")
    assert set(weights.values()) <= {0.0, 1.0} and list(weights) == _kept(eng.param_names)
    eng.set_lr_weights(weights)
    before = {n: p.detach().clone() for n, p in net.named_parameters()}
    tr.train_step(img, lab)
    torch.cuda.synchronize()
    after = dict(net.named_parameters())
    frozen = [n for n in eng.param_names if weights.get(n, 0.0) == 0.0]
    live = [n for n in eng.param_names if weights.get(n, 0.0) == 1.0]
    for n in frozen:
        assert torch.equal(after[n].detach().view(torch.int32), before[n].view(torch.int32)), f"frozen {n} moved"
    moved = [n for n in live if not torch.equal(after[n].detach(), before[n])]
    print(f"eb-criterion through the engine: {len(frozen)} tensors frozen, {len(live)} live, {len(moved)} of them moved")
    assert not live or moved
