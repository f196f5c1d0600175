"""The consolidation penalties on the training engine (continual.Consolidation over HipEngine / DataParallelTrainer), eagerly and
from hipGraphs: the depth-[1, 1, 1, 1] model and the B = 2 batch of test_gpu_continual_step, mostly before its expansion (the plain
9-class CE + Dice step), and the 12-class distill trainer for the carry across expand_classes.  The host oracle and the bounds are
test_consolidate_host's, the optimiser references the existing ones (test_adamw_host.adamw_ref; torch.optim.SGD in float64 at the
bound of test_gpu_step_tail's SGD test)."""
import numpy as np
import pytest
import torch

from oracle.determ import det_labels, det_normal

from test_adamw_host import U, adamw_bound, adamw_ref, cdiv, clip_ref, norm_bounds
from test_consolidate_host import STATISTICS, estimate_bound, grad_bound, importance_ref, penalty_ref, scalar_bounds
from test_gpu_continual_step import LR, NEW, OLD, _batch, _distill, _models
from test_gpu_parity import DEV, T
from test_gpu_step_tail import bits16, bits32, close
from test_gpu_tpgm_step import Raising, _elem_mask, move_off_the_anchor, split

pytestmark = pytest.mark.gpu
SGD_LR, ADAMW_LR = 0.05, 1e-4
LAM = 10.0
EXCLUDED = "output.weight"


def _batch9(k=0):
    """The k-th (image, 9-class label) batch: 0 is test_gpu_continual_step's image."""
    if k == 0:
        return _batch()[0], T(det_labels("clstep.labels9", (2, 224, 224), OLD))
    return T(det_normal(f"consstep.x{k}", (2, 1, 224, 224))).repeat(1, 3, 1, 1), T(det_labels(f"consstep.labels{k}", (2, 224, 224), OLD))


def _trainer(kind, use_graph):
    from cswin_unet_amd.trainer import DataParallelTrainer
    net = _models(expand=False)[0]
    kw = dict(base_lr=SGD_LR) if kind == "sgd" else dict(optimizer="adamw", base_lr=ADAMW_LR, weight_decay=0.01, max_grad_norm=1.0, lr_schedule="constant")
    return net, DataParallelTrainer(net, OLD, max_iterations=100, use_graph=use_graph, **kw)


def _synthetic_importance(flat):
    """A dense importance in [0, 1) (the estimated Fisher of this model is some 1e-8: its penalty would hide below the gradient)."""
    gen = torch.Generator().manual_seed(20)
    flat.flat_importance.copy_(torch.rand(flat.flat_importance.numel(), generator=gen).to(DEV))


def _three(tr, img, lab, cons=None):
    rows, pen = [], []
    for _ in range(3):
        rows.append(tr.train_step(img, lab).clone())
        if cons is not None:
            pen.append(cons.flat.scalars.clone())
    return torch.stack(rows).cpu().numpy().astype(np.float64), (torch.stack(pen).cpu().numpy().astype(np.float64) if pen else None)


@pytest.mark.parametrize("case", ["weight0", "importance0"])
def test_a_penalty_of_zero_is_the_plain_trajectory(case):
    """lambda = 0 over a dense importance, and lambda = 10 over an all-zero importance: three steps and the final parameters equal
    those of a trainer with nothing attached.  Values are compared: an F = 0 element may turn a -0.0 gradient into +0.0."""
    from cswin_unet_amd.continual import Consolidation
    img, lab = _batch9()
    net_a, tr_a = _trainer("sgd", False)
    plain, _ = _three(tr_a, img, lab)
    net_b, tr_b = _trainer("sgd", False)
    cons = Consolidation(tr_b, "ewc", weight=0.0 if case == "weight0" else LAM)
    assert tr_b.engine.consolidation is cons.flat
    if case == "weight0":
        _synthetic_importance(cons.flat)
    with_cons, pen = _three(tr_b, img, lab, cons)
    print(case, "plain", plain, "attached", with_cons, "scalars", pen, sep="\n")
    assert np.array_equal(plain, with_cons) and plain[2, 0] != plain[0, 0]
    assert torch.equal(tr_a.engine.flat_param, tr_b.engine.flat_param)
    assert (pen[:, 0] == 0).all() and pen[0, 2] == 0 and pen[2, 2] > 0          # no penalty, and the weights did leave the anchor
    assert (pen[1:, 1] > 0).all() if case == "weight0" else (pen[:, 1] == 0).all()
    cons.detach()
    assert tr_b.engine.consolidation is None


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_one_step_by_hand_penalises_the_gradient_before_the_optimiser(kind):
    """forward_sums, finalize and backward_phases by hand, a copy of flat_grad, then apply(0.5): flat_grad afterwards is g + lambda
    2 F d within grad_bound (an excluded tensor keeps its bits); the parameters are the float64 optimiser's, fed that penalised
    gradient, within the optimiser's existing bound; AdamW's clip coefficient is the penalised gradient's."""
    from cswin_unet_amd.continual import Consolidation
    img, lab = _batch9()
    net, tr = _trainer(kind, False)
    eng, opt = tr.engine, tr.engine.opt
    cons = Consolidation(tr, "ewc", weight=LAM, exclude=(EXCLUDED,))
    flat = cons.flat
    _synthetic_importance(flat)
    move_off_the_anchor(opt, "consstep")
    grad_scale = 0.5
    eng.forward_sums(img, lab, 1.0)
    eng.finalize(lab.numel())
    for _ in eng.backward_phases(1.0):
        pass
    g0, p0 = opt.flat_grad.clone(), opt.flat_param.clone()
    eng.apply(grad_scale)
    torch.cuda.synchronize()
    g1, p1 = opt.flat_grad.clone(), opt.flat_param.clone()
    mask = _elem_mask(opt)
    names = list(eng.param_names)
    tw = np.array([0.0 if n == EXCLUDED else 1.0 for n in names])
    assert tw.sum() == len(names) - 1 and np.array_equal(flat.tensor_weight.cpu().numpy(), tw.astype(np.float32))
    w_elem = np.zeros(opt.numel)
    for o, p, w in zip(opt.offsets, opt.params, tw):
        w_elem[o:o + p.numel()] = w
    h = lambda t: t.cpu().numpy().astype(np.float64)
    d = h(p0) - h(flat.flat_anchor)
    add = float(np.float32(LAM)) * (1.0 / grad_scale) * w_elem * h(flat.flat_importance) * d
    what = f"consolidate.step.{kind}"
    close(h(g1)[mask], (h(g0) + add)[mask], grad_bound(add, h(g0))[mask], what + ".grad")
    off = mask & (w_elem == 0)
    assert off.any() and (bits32(g1)[off] == bits32(g0)[off]).all() and (bits32(g1)[~mask] == bits32(g0)[~mask]).all()
    moved = np.abs(h(g1) - h(g0))[mask & (w_elem == 1)]
    assert (moved > 0).mean() > 0.9 and np.linalg.norm(add) > 0.1 * np.linalg.norm(h(g0))          # the penalty is no rounding matter here
    # the penalty left in device memory: (lambda / 2) sum w F d^2 of the weights before the update
    ref = penalty_ref(split(p0, opt), split(flat.flat_anchor, opt), split(flat.flat_importance, opt), float(np.float32(LAM)), tw)
    numels = [p.numel() for p in opt.params]
    close(h(flat.scalars), [ref["penalty"], ref["weighted"], ref["dist"]], scalar_bounds(ref, numels, [cdiv(n, 16384) for n in numels], tw), what + ".scalars")
    assert float(cons.penalty) == float(flat.scalars[0]) > 0
    lr = float(opt.lr_dev.cpu()[0]) if kind == "adamw" else SGD_LR
    if kind == "sgd":
        leaf = torch.from_numpy(h(p0)).requires_grad_()
        ref = torch.optim.SGD([leaf], lr=float(np.float32(lr)), momentum=0.9, weight_decay=1e-4)
        g64 = torch.from_numpy(h(g1)) * grad_scale
        leaf.grad = g64.clone()
        ref.step()
        A = g64.abs().numpy() + np.abs(1e-4 * h(p0))
        close(h(p1)[mask], leaf.detach().numpy()[mask], (4 * U * (np.abs(h(p0)) + float(np.float32(lr)) * A))[mask], what + ".p")
    else:
        tensors = split(g1, opt)
        _, total, coef = clip_ref(tensors, grad_scale, 1.0)
        _, total0, coef0 = clip_ref(split(g0, opt), grad_scale, 1.0)
        btotal, bcoef = norm_bounds(total, coef, max(numels), max(-(-n // 16384) for n in numels), len(numels))
        sc = h(opt.scalars)
        print(f"{what}: grad norm {sc[0]!r} (float64 {total!r}, unpenalised {total0!r}); clip_coef {sc[1]!r} (float64 {coef!r}, unpenalised {coef0!r})")
        assert abs(sc[0] - total) <= btotal and abs(sc[1] - coef) <= bcoef and coef < 1.0
        assert abs(total0 - total) > 100 * btotal and abs(coef0 - coef) > 100 * bcoef                   # not the unpenalised gradient's
        zeros = np.zeros(opt.numel)
        kw = dict(wd=0.01, grad_scale=grad_scale, clip=sc[1])
        close(h(p1)[mask], adamw_ref(h(p0), h(g1), zeros, zeros, 1, lr, **kw)[0][mask], adamw_bound(h(p0), h(g1), zeros, zeros, 1, lr, **kw)[0][mask], what + ".p")
    assert (np.abs(h(p1) - h(p0))[mask] > 0).mean() > 0.9


@pytest.fixture(scope="module")
def runs():
    """Consolidation on (EWC estimated on the first batch, a dense importance on top so that the penalty is live), three steps on
    the second batch eagerly and from hipGraphs; the eager run's state after its first step; the graph run goes on for the weight
    change between replays."""
    from cswin_unet_amd.continual import Consolidation
    out = {}
    for name, use_graph in (("eager", False), ("graph", True)):
        net, tr = _trainer("sgd", use_graph)
        cons = Consolidation(tr, "ewc", weight=LAM)
        cons.estimate([_batch9(0)])
        assert float(cons.flat.flat_importance.max()) > 0
        _synthetic_importance(cons.flat)
        img, lab = _batch9(1)
        rows, pen = [], []
        for k in range(3):
            rows.append(tr.train_step(img, lab).clone())
            pen.append(cons.flat.scalars.clone())
            if name == "eager" and k == 0:
                out["state1"] = dict(model={k_: v.clone() for k_, v in net.state_dict().items()}, opt=tr.engine.opt.state_dict(), cons=cons.state_dict(),
                                     iter_num=tr.iter_num)
        out[name] = torch.stack(rows).cpu().numpy().astype(np.float64)
        out[name + ".pen"] = torch.stack(pen).cpu().numpy().astype(np.float64)
        if use_graph:
            assert tr.engine._graphs is not None
            tr.set_consolidation_weight(2 * LAM)
            tr.train_step(img, lab)
            out["doubled"] = cons.flat.scalars.cpu().numpy().copy()
            tr.set_consolidation_weight(0.0)
            before = tr.engine.flat_param.clone()
            tr.train_step(img, lab)
            out["zeroed"] = cons.flat.scalars.cpu().numpy().copy()
            out["lam_dev"] = float(cons.flat.lam_dev.cpu()[0])
            out["moved_at_zero"] = not torch.equal(before, tr.engine.flat_param)
    return out


def test_eager_and_graph_steps_give_the_same_trajectory(runs):
    """Three steps with use_graph=False and use_graph=True, consolidation on: the tolerance of the existing eager-against-graph
    trainer tests (2e-4 of each statistic).  The penalty, 0 at the first step (the anchor is the weights), is live afterwards."""
    e, g = runs["eager"], runs["graph"]
    print("eager", e, runs["eager.pen"], "graph", g, runs["graph.pen"], sep="\n")
    assert np.isfinite(e).all() and np.isfinite(g).all() and e[2, 0] != e[0, 0]
    assert (np.abs(e - g) <= 2e-4 * np.abs(e)).all(), np.abs(e - g) / np.abs(e)
    for pen in (runs["eager.pen"], runs["graph.pen"]):
        assert pen[0, 0] == 0 and pen[0, 2] == 0 and (pen[1:, 0] > 0).all() and np.isfinite(pen).all()


def test_set_consolidation_weight_between_graph_replays(runs):
    """The next step's penalty is formed with the new strength: scalars[0] is fl(fl(lambda / 2) scalars[1]) of that strength, bit
    for bit; at strength 0 it is 0 and the step still moves the weights."""
    f = np.float32
    third, doubled, zeroed = runs["graph.pen"][2].astype(f), runs["doubled"], runs["zeroed"]
    assert third[0] == f(0.5) * f(LAM) * third[1] and third[1] > 0
    assert doubled[0] == f(0.5) * f(2 * LAM) * doubled[1] and doubled[1] > 0 and doubled[0] != f(0.5) * f(LAM) * doubled[1]
    assert zeroed[0] == 0 and zeroed[1] > 0 and runs["lam_dev"] == 0.0 and runs["moved_at_zero"]


def test_state_dict_round_trip_reproduces_the_third_step(runs):
    """The model's, the optimiser's and the consolidation's state after the first step, loaded into a fresh trainer, give the second
    and third steps' stats and penalties bit for bit."""
    from cswin_unet_amd.continual import Consolidation
    s = runs["state1"]
    net, tr = _trainer("sgd", False)
    net.load_state_dict(s["model"])
    tr.engine.opt.load_state_dict(s["opt"])
    tr.iter_num = s["iter_num"]
    cons = Consolidation(tr, "ewc", weight=s["cons"]["weight"], state=s["cons"])
    assert set(s["cons"]) == {"method", "weight", "exclude", "tensors"} and list(s["cons"]["tensors"]) == list(tr.engine.param_names)
    assert all(v["anchor"].shape == p.shape == v["importance"].shape for v, p in zip(s["cons"]["tensors"].values(), tr.engine.opt.params))
    img, lab = _batch9(1)
    rows, pen = [], []
    for _ in range(2):
        rows.append(tr.train_step(img, lab).clone())
        pen.append(cons.flat.scalars.clone())
    rows, pen = torch.stack(rows).cpu().numpy().astype(np.float64), torch.stack(pen).cpu().numpy().astype(np.float64)
    assert np.array_equal(rows, runs["eager"][1:]), (rows, runs["eager"][1:])
    assert np.array_equal(pen, runs["eager.pen"][1:]), (pen, runs["eager.pen"][1:])


@pytest.fixture(scope="module")
def estimated():
    """EWC and MAS estimated on two different batches by one 9-class trainer, every gradient the accumulate launch saw read back."""
    from cswin_unet_amd.continual import Consolidation
    net, tr = _trainer("sgd", False)
    eng, opt = tr.engine, tr.engine.opt
    tr.train_step(*_batch9(0))                                          # a momentum buffer that is not zero
    batches = [_batch9(0), _batch9(1)]
    out = {"names": list(eng.param_names), "layout": (list(opt.offsets), [p.numel() for p in opt.params])}
    for method in ("ewc", "mas"):
        cons = Consolidation(tr, method, weight=LAM)
        seen, launch = [], cons.flat.accumulate

        def recording(grad_scale=1.0, _launch=launch, _seen=seen):
            _seen.append(opt.flat_grad.clone())
            _launch(grad_scale)
        cons.flat.accumulate = recording
        keep = (bits32(opt.flat_param), bits32(opt.flat_mom), bits16(opt.flat_param16))
        was_cut = eng.core.detach_decoder_inputs
        assert net.training and was_cut
        cons.estimate(batches)
        ok = dict(training=net.training, cut=eng.core.detach_decoder_inputs == was_cut, no_grad=all(p.grad is None for p in opt.params),
                  bits=all((a == b).all() for a, b in zip(keep, (bits32(opt.flat_param), bits32(opt.flat_mom), bits16(opt.flat_param16)))),
                  anchor=bool(torch.equal(cons.flat.flat_anchor, opt.flat_param)), scratch=cons.flat.scratch is None)
        imp = cons.flat.flat_importance.clone()
        with pytest.raises(RuntimeError, match="the batch source broke"):
            cons.estimate(Raising(batches[1]))
        ok_raise = dict(training=net.training, cut=eng.core.detach_decoder_inputs == was_cut, no_grad=all(p.grad is None for p in opt.params),
                        bits=all((a == b).all() for a, b in zip(keep, (bits32(opt.flat_param), bits32(opt.flat_mom), bits16(opt.flat_param16)))),
                        importance=bool(torch.equal(cons.flat.flat_importance, imp)), scratch=cons.flat.scratch is None)
        net.eval()
        cons.estimate(batches[:1], decay=1.0)                           # the mode it found is the mode it leaves
        ok["eval_kept"] = not net.training
        net.train()
        out[method] = dict(grads=[g.cpu().numpy() for g in seen[:2]], importance=imp.cpu().numpy(), ok=ok, ok_raise=ok_raise, calls=len(seen),
                           online=cons.flat.flat_importance.cpu().numpy(), online_grad=seen[3].cpu().numpy(), state=cons.state_dict())
        report = cons.report().cpu().numpy().copy()
        out[method]["report"] = report
        cons.detach()
    return out


@pytest.mark.parametrize("method", ["ewc", "mas"])
def test_estimate_on_two_batches_vs_float64(estimated, method):
    """The importance is the float64 mean of g^2 (|g| for MAS) over the gradients the two accumulate launches were given, within
    the accumulate bound; afterwards the training mode and the decoder cut are as before, every .grad is None and the weights, the
    shadow and the optimiser's state keep their bits -- also when the batch source raises, which leaves the importance alone too.
    A second, online, estimation with decay 1 adds that batch's statistic."""
    e = estimated[method]
    offsets, numels = estimated["layout"]
    mask = np.zeros(e["importance"].size, bool)
    for o, n in zip(offsets, numels):
        mask[o:o + n] = True
    stat = STATISTICS[method]
    assert e["calls"] == 4 and all(e["ok"].values()) and all(e["ok_raise"].values()), (e["ok"], e["ok_raise"])
    assert not np.array_equal(e["grads"][0], e["grads"][1])
    total = importance_ref(e["grads"], stat, count=1)
    want = total / 2
    close(e["importance"][mask], want[mask], estimate_bound(total, 2, stat, 2)[mask], f"consolidate.estimate.{method}")
    assert (e["importance"][mask] >= 0).all() and (e["importance"][mask] > 0).mean() > 0.5
    prev = e["importance"].astype(np.float64)
    new = importance_ref([e["online_grad"]], stat, count=1)
    close(e["online"][mask], (prev + new)[mask], estimate_bound(new, 1, stat, 1, 1.0, prev)[mask], f"consolidate.online.{method}")
    assert (e["report"] == 0).all()                                      # at the anchor


def test_state_carries_across_expand_classes(estimated):
    """A state estimated on the 9-class model, loaded into the 12-class distill trainer: output.weight's importance rows [:9] are the
    old ones and [9:] zero, every other tensor's importance and anchor are copied, and report() gives sum F d^2 = 0 as before the
    expansion (the widened model's old rows are the anchor's).  The distill engine's own loss then drives an online estimation."""
    from cswin_unet_amd.continual import Consolidation
    from cswin_unet_amd.trainer import DataParallelTrainer
    state = estimated["ewc"]["state"]
    net, teacher = _models()
    with torch.no_grad():                                                # the widened model of the weights the state was estimated at (one step in)
        for n, p in net.named_parameters():
            old = state["tensors"][n]["anchor"]
            p[:old.shape[0]].copy_(old)
    tr = DataParallelTrainer(net, OLD + NEW - 1, base_lr=LR, max_iterations=100, use_graph=False, distill=_distill(teacher))
    cons = Consolidation(tr, "ewc", weight=LAM, state=state)
    new = cons.state_dict()["tensors"]
    name = [n for n in new if n.endswith("output.weight")]
    assert name == ["output.weight"] and new[name[0]]["importance"].shape[0] == OLD + NEW - 1 and state["tensors"][name[0]]["importance"].shape[0] == OLD
    for n, v in new.items():
        old = state["tensors"][n]
        rows = slice(0, OLD) if n == name[0] else slice(None)
        assert torch.equal(v["importance"][rows], old["importance"]) and torch.equal(v["anchor"][rows], old["anchor"]), n
    head = new[name[0]]
    assert (head["importance"][OLD:] == 0).all() and float(head["importance"][:OLD].max()) > 0
    assert torch.equal(head["anchor"][OLD:], dict(net.named_parameters())[name[0]].detach()[OLD:])
    report = cons.report().cpu().numpy()
    assert report[1] == estimated["ewc"]["report"][1] == 0 and report[0] == 0
    img, lab = _batch()
    cons.consolidate([(img, lab)], 1.0)
    grown = cons.state_dict()["tensors"][name[0]]["importance"]
    assert float(grown[OLD:].max()) > 0 and bool((grown[:OLD] >= head["importance"][:OLD]).all()) and net.training
    assert all(p.grad is None for p in net.parameters())
