"""The training step with the reference's continual-learning recipe (universal_train.py:693-725, 934-939): AdamW(weight_decay=0.01)
after clip_grad_norm_(1.0), optionally with a learning rate per tensor, on the depth-[1, 1, 1, 1] model, batch, teacher, label map
and class weights of tests/test_gpu_continual_step.py.  The optimiser is isolated by taking the gradients from the engine: the
float64 reference (test_adamw_host.adamw_ref) is applied to a copy of the engine's own flat_grad and initial weights."""
import numpy as np
import pytest
import torch

from test_adamw_host import U, adamw_bound, adamw_ref, clip_ref, norm_bounds, sumsq_depth
from test_gpu_continual_step import DEV, NEW, OLD, _batch, _distill, _models

pytestmark = pytest.mark.gpu
BASE_LR = 1e-4                                    # the reference's kind of rate for this recipe


def _trainer(net, teacher, use_graph):
    from cswin_unet_amd.trainer import DataParallelTrainer
    return DataParallelTrainer(net, OLD + NEW - 1, optimizer="adamw", base_lr=BASE_LR, weight_decay=0.01, max_grad_norm=1.0, lr_schedule="constant",
                               distill=_distill(teacher), use_graph=use_graph)


def _stats(tr, img, lab):
    return np.array([float(v) for v in tr.train_step(img, lab)])


@pytest.fixture(scope="module")
def runs():
    """Three steps eagerly and from hipGraphs, and the eager run's state round the first step: computed once."""
    img, lab = _batch()
    out = {}
    for name, use_graph in (("eager", False), ("graph", True)):
        net, teacher = _models()
        tr = _trainer(net, teacher, use_graph)
        opt = tr.engine.opt
        assert type(opt).__name__ == "FlatAdamW" and opt.max_grad_norm == 1.0 and opt.weight_decay == 0.01 and tr.lr_schedule == "constant"
        rows = []
        for k in range(3):
            if name == "eager" and k == 0:
                out["p0"] = opt.flat_param.clone()
            rows.append(_stats(tr, img, lab))
            if name == "eager" and k == 0:
                out.update(g1=opt.flat_grad.clone(), p1=opt.flat_param.clone(), scalars1=opt.scalars.clone(), norm1=opt.grad_norm.clone(),
                           model1={k_: v.clone() for k_, v in net.state_dict().items()}, opt1=opt.state_dict(),
                           layout=(list(opt.offsets), [p.numel() for p in opt.params]), lr=float(opt.lr_dev.cpu()[0]))
        assert opt.step_count == 3 and float(opt.lr_dev.cpu()[0]) == float(np.float32(BASE_LR))      # "constant": the step leaves the rate alone
        out[name] = np.array(rows)
    return out


def test_trainer_takes_the_reference_recipe(runs):
    """The constructor call of the issue (a TypeError before the feature), and the trajectory it gives: printed, not gated -- whether
    the objective falls at this rate is not known."""
    e = runs["eager"]
    print("AdamW + clip, lr 1e-4, three steps: loss", e[:, 0], "kd", e[:, 3])
    assert e.shape == (3, 5) and np.isfinite(e).all()
    assert e[1, 0] != e[0, 0]                                             # the step moved the weights


def test_eager_and_graph_steps_give_the_same_trajectory(runs):
    """Three steps with use_graph=False and use_graph=True at the tolerance of tests/test_gpu_continual_step.py: 2e-4 of each
    statistic; kd, 0 at the first step, is held to 2e-4 of the loss at the first two steps and of itself at the third."""
    e, g = runs["eager"], runs["graph"]
    print("eager", e, "graph", g, sep="\n")
    assert np.isfinite(e).all() and np.isfinite(g).all()
    scale = np.abs(e).copy()
    scale[:2, 3] = np.abs(e[:2, 0])
    assert (np.abs(e - g) <= 2e-4 * scale).all(), np.abs(e - g) / scale


def _layout_mask(layout, total):
    mask = np.zeros(total, bool)
    for o, n in zip(*layout):
        mask[o:o + n] = True
    return mask


def test_one_step_matches_float64_adamw_on_the_engines_gradients(runs):
    """After one step every parameter is within the derived bound of adamw_ref applied in float64 to a copy of the engine's
    flat_grad and initial weights, at the clip coefficient the kernel was given; that coefficient and engine.opt.grad_norm are
    within their own bounds of the float64 norm of the same copy."""
    from test_gpu_step_tail import close
    p0, g, p1 = (runs[k].cpu().numpy().astype(np.float64) for k in ("p0", "g1", "p1"))
    offsets, numels = runs["layout"]
    mask = _layout_mask(runs["layout"], p0.size)
    assert (g[~mask] == 0).all()
    _, total, coef = clip_ref([g[o:o + n] for o, n in zip(offsets, numels)], 1.0, 1.0)
    chunks = [-(-n // 16384) for n in numels]
    btotal, bcoef = norm_bounds(total, coef, max(numels), max(chunks), len(numels))
    sc = runs["scalars1"].cpu().numpy().astype(np.float64)
    print(f"grad norm {sc[0]!r} (float64 {total!r}, bound {btotal:.3e}); clip_coef {sc[1]!r} (float64 {coef!r}, bound {bcoef:.3e})")
    assert float(runs["norm1"].cpu()[0]) == sc[0] and abs(sc[0] - total) <= btotal
    assert abs(sc[1] - coef) <= bcoef and (sc[1] == 1.0 or coef < 1.0)
    zeros = np.zeros_like(p0)
    kw = dict(wd=0.01, grad_scale=1.0, clip=sc[1])
    want = adamw_ref(p0, g, zeros, zeros, 1, runs["lr"], **kw)[0]
    bound = adamw_bound(p0, g, zeros, zeros, 1, runs["lr"], **kw)[0]
    close(p1[mask], want[mask], bound[mask], "adamw.step.one_step.p")
    assert (np.abs(p1 - p0)[mask] > 0).mean() > 0.99


def test_zero_rate_freezes_the_encoder_bit_for_bit():
    """set_lr_weights with 0 for every encoder tensor (names left out of the dict get the default 0): after two steps the encoder
    is bit-identical and the decoder moved."""
    img, lab = _batch()
    net, teacher = _models()
    tr = _trainer(net, teacher, False)
    eng = tr.engine
    assert 0 < eng.n_enc < len(eng.param_names) and list(eng.param_names) == [n for n, _ in net.named_parameters()]
    tr.engine.set_lr_weights({n: 1.0 for n in eng.param_names[eng.n_enc:]})
    before = {n: p.detach().clone() for n, p in net.named_parameters()}
    m0 = eng.opt.flat_m.clone()
    for _ in range(2):
        tr.train_step(img, lab)
    torch.cuda.synchronize()
    after = dict(net.named_parameters())
    for n in eng.param_names[:eng.n_enc]:
        assert torch.equal(after[n].detach().view(torch.int32), before[n].view(torch.int32)), f"frozen {n} moved"
    moved = [not torch.equal(after[n].detach(), before[n]) for n in eng.param_names[eng.n_enc:]]
    assert all(moved), [n for n, mv in zip(eng.param_names[eng.n_enc:], moved) if not mv]
    lo, hi = eng.opt.flat_range(0, eng.n_enc)
    assert not torch.equal(eng.opt.flat_m[lo:hi], m0[lo:hi])             # the frozen tensors' moments still move
    with pytest.raises(KeyError):
        tr.engine.set_lr_weights({"no.such.weight": 1.0})


def test_surgical_lr_weights_on_one_batch():
    """Keys: the parameter names without "bn" / "norm"; values in [0, 1] with maximum exactly 1; each within the sums-of-squares
    bound of the ratio ||g|| / ||p|| formed in float64 from the .grad tensors of a plain backward of the same loss (the focal
    criterion alone, model in eval mode), normalised by its maximum.  A weight is a quotient of two ratios, each the quotient of
    two square roots of sums: per sum half its relative bound plus the square root at 2 units."""
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
    ratio, rel = {}, {}
    for n, p in net.named_parameters():
        gn, pn = float(p.grad.double().norm()), float(p.detach().double().norm())
        ratio[n] = gn / pn if pn > 1e-8 else 0.0
        rel[n] = 2 * ((sumsq_depth(p.numel(), -(-p.numel() // 16384)) + 2) / 2 + 2) * U
    opt.zero_grad()
    net.train()
    got = surgical_lr_weights(net, opt, [(img, lab)], d)
    assert net.training and all(p.grad is None for p in net.parameters())
    keep = [n for n in names if "bn" not in n.lower() and "norm" not in n.lower()]
    assert list(got) == keep and 0 < len(keep) < len(names)
    top = max(keep, key=lambda n: ratio[n])
    assert max(got.values()) == 1.0 and min(got.values()) >= 0.0 and got[top] == 1.0
    worst = 0.0
    for n in keep:
        want = ratio[n] / ratio[top]
        bound = (rel[n] + rel[top]) * want
        worst = max(worst, abs(got[n] - want) / bound if bound > 0 else float(got[n] != want))
        assert abs(got[n] - want) <= bound, (n, got[n], want, bound)
    print(f"surgical_lr_weights: {len(keep)} of {len(names)} tensors, largest |error| / bound {worst:.3f}")


def test_state_dict_round_trip_reproduces_the_third_step(runs):
    """The model's and the optimiser's state after the first step, loaded into a fresh trainer, give the second and third steps'
    stats bit for bit: the third step's loss is that of weights the restored m, v and step count produced."""
    img, lab = _batch()
    net, teacher = _models()
    tr = _trainer(net, teacher, False)
    net.load_state_dict(runs["model1"])
    tr.engine.opt.load_state_dict(runs["opt1"])
    assert tr.engine.opt.step_count == 1 and torch.equal(tr.engine.opt.flat_param, runs["p1"])
    sd = tr.engine.opt.state_dict()
    assert set(sd) == {"m", "v", "step", "lr", "lr_weights"} and sd["lr_weights"] is None and torch.equal(sd["m"], runs["opt1"]["m"])
    rows = np.array([_stats(tr, img, lab) for _ in range(2)])
    assert np.array_equal(rows, runs["eager"][1:]), (rows, runs["eager"][1:])


def test_flat_adamw_surface_on_three_tensors(monkeypatch):
    """step(), tensor_norms(), grad_norm, the multipliers and the state dict on a three-tensor optimiser; apply() refuses to be
    captured (the capture state is stubbed: nothing is captured here).  The norms are held to norm_bounds' relative bound of a
    square root of a sum over the largest tensor (two chunks)."""
    from cswin_unet_amd.optim import FlatAdamW
    gen = torch.Generator().manual_seed(7)
    numels = (5, 1027, 16385)
    params = [torch.nn.Parameter(torch.randn(n, generator=gen).to(DEV)) for n in numels]
    opt = FlatAdamW(params, lr=1e-3, max_grad_norm=1.0)
    w = [0.0, 1.0, 0.5]
    opt.set_lr_weights(w)
    for p in params:
        p.grad = torch.randn(p.numel(), generator=gen).to(DEV)
    before = [p.detach().clone() for p in params]
    opt.step()
    norms = opt.tensor_norms().cpu().double()
    want = torch.tensor([[float(p.grad.double().norm()), float(p.detach().double().norm())] for p in params], dtype=torch.float64)
    rel = norm_bounds(1.0, 1.0, max(numels), 2, len(numels))[0]
    assert float(((norms - want).abs() / want).max()) <= rel
    total = float(torch.stack([p.grad.double().norm() for p in params]).norm())
    assert abs(float(opt.grad_norm.cpu()[0]) - total) <= rel * total and opt.step_count == 1
    assert torch.equal(params[0].detach(), before[0]) and not torch.equal(params[1].detach(), before[1])
    sd = opt.state_dict()
    assert sd["step"] == 1 and torch.equal(sd["lr_weights"].cpu(), torch.tensor(w))
    with pytest.raises(ValueError):
        opt.set_lr_weights([1.0, 2.0])
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="capture"):
        opt.apply()
    assert opt.step_count == 1
