"""TPGM on the training engine (continual.TPGM over HipEngine / DataParallelTrainer), eagerly and from hipGraphs: the depth-[1, 1, 1, 1]
model, the batch and the distillation setup of test_gpu_continual_step.  One fixture per mode runs the whole sequence once:

    two train steps, two iterations (every ratio is 1: the initial radii are wide), an iteration whose batch iterator raises,
    a third train step; then the weights are moved 0.01 N(0, 1) off the anchor, the radii set to half the measured norms, and
    one iteration, a state_dict round trip and the final projection follow.

The host oracle and the bounds are test_tpgm_host's."""
import numpy as np
import pytest
import torch

from oracle.determ import det_normal

from test_adamw_host import cdiv
from test_gpu_continual_step import LR, NEW, OLD, _batch, _distill, _models
from test_gpu_parity import T
from test_gpu_step_tail import bits16, bits32, close
from test_tpgm_host import (EXCLUDED, NORM_EPS, U, norm_bound, norms_ref, project_bound, project_ref, ratio_bound, ratios_ref, update_ref)

pytestmark = pytest.mark.gpu
PROJ_LR = 0.05


def split(flat_tensor, opt):
    """Per-tensor float numpy views of a flat buffer (the pad words left out)."""
    a = flat_tensor.detach().cpu().numpy()
    return [a[o:o + p.numel()] for o, p in zip(opt.offsets, opt.params)]


def move_off_the_anchor(opt, tag="tpgmstep"):
    """theta += 0.01 N(0, 1), the same on every call: norms of 0.01 sqrt(n), so that half of them lies above the radii's floor 1e-2."""
    with torch.no_grad():
        for k, p in enumerate(opt.params):
            p.add_(T(det_normal(f"{tag}.noise{k}", tuple(p.shape), 0.01)))
    opt.refresh_shadow()


def oracle_step(opt, flat, theta, grad, before, step, grad_scale, coef):
    """update_ref for the engine's layout from (gamma, m, v) `before`, fed the saved theta and the engine's own flat_grad."""
    numel = [p.numel() for p in opt.params]
    return update_ref(split(theta, opt), split(flat.flat_anchor, opt), split(grad, opt), before[0], before[1], before[2], np.array(flat.flags_host), False,
                      grad_scale, step, float(np.float32(flat.proj_lr)), [cdiv(n, 16384) for n in numel], coef=coef)


def check_step(ref, got, what):
    """gamma, m, v, norm and the new ratio of one update against the oracle, all within its bounds; the largest error / bound."""
    for name in ("gamma", "m", "v", "norm", "ratio"):
        close(got[name], ref[name][0], ref[name][1], f"{what}.{name}")


class Raising:
    """A batch source whose second batch raises."""

    def __init__(self, batch):
        self.batch = batch

    def __iter__(self):
        yield self.batch
        raise RuntimeError("the batch source broke")


def _state(flat):
    return {k: getattr(flat, a).detach().cpu().numpy().copy() for k, a in (("gamma", "gamma"), ("m", "gamma_m"), ("v", "gamma_v"), ("norm", "norm"),
                                                                             ("ratio", "ratio"), ("scalars", "scalars"))}


def _sequence(use_graph):
    from cswin_unet_amd.continual import TPGM
    from cswin_unet_amd.optim import tpgm_init_gamma
    from cswin_unet_amd.trainer import DataParallelTrainer
    img, lab = _batch()
    ncls = OLD + NEW - 1
    out = {}
    net, teacher = _models()
    tr = DataParallelTrainer(net, ncls, base_lr=LR, max_iterations=100, use_graph=use_graph, distill=_distill(teacher))
    opt = tr.engine.opt
    sizes = {k: getattr(tr.engine, k).numel() for k in ("sums", "stats")}
    tp = TPGM(tr, proj_lr=PROJ_LR)
    flat = tp.flat
    assert sizes == {k: getattr(tr.engine, k).numel() for k in ("sums", "stats")} and flat.opt is opt
    # the initial radii: max(3, 2 ||theta||), head tensors max(10, 5 ||theta||)
    pn = norms_ref(split(opt.flat_param, opt), [np.zeros(p.numel()) for p in opt.params], False)
    out["gamma0"] = (flat.gamma.cpu().numpy(), np.array([tpgm_init_gamma(n, v) for n, v in zip(tr.engine.param_names, pn)]),
                     np.array([norm_bound(v, p.numel(), cdiv(p.numel(), 16384), False)[0] for v, p in zip(pn, opt.params)]))
    out["names"] = list(tr.engine.param_names)
    gamma0 = flat.gamma.clone()
    traj = [tr.train_step(img, lab).clone() for _ in range(2)]
    keep = (bits32(opt.flat_param), bits16(opt.flat_param16))
    tp.iterate([(img, lab)], 2)
    out["restored"] = bool((bits32(opt.flat_param) == keep[0]).all() and (bits16(opt.flat_param16) == keep[1]).all())
    with pytest.raises(RuntimeError, match="the batch source broke"):
        tp.iterate(Raising((img, lab)), 3)
    out["restored_after_raise"] = bool((bits32(opt.flat_param) == keep[0]).all() and (bits16(opt.flat_param16) == keep[1]).all()) and not flat._active
    out["wide_radii_stand_still"] = bool(torch.equal(flat.gamma, gamma0)) and tuple(tp.ratio_stats()) == (1.0, 1.0, 1.0) and flat.step_count == 3
    traj.append(tr.train_step(img, lab).clone())
    out["traj"] = torch.stack(traj).cpu().numpy().astype(np.float64)
    # the same three steps without any TPGM
    net_b, teacher_b = _models()
    trb = DataParallelTrainer(net_b, ncls, base_lr=LR, max_iterations=100, use_graph=use_graph, distill=_distill(teacher_b))
    out["traj_plain"] = torch.stack([trb.train_step(img, lab).clone() for _ in range(3)]).cpu().numpy().astype(np.float64)

    # off the anchor, radii at half the norms
    move_off_the_anchor(opt)
    norms = flat.tensor_norms().cpu().numpy()
    tp.set_constraints((0.5 * norms.astype(np.float64)).astype(np.float32))
    sd = tp.state_dict()
    theta = opt.flat_param.clone()
    keep = (bits32(opt.flat_param), bits16(opt.flat_param16))
    flat.begin()
    projected = opt.flat_param.clone()
    flat.end()
    out["begin_end_restores"] = bool((bits32(opt.flat_param) == keep[0]).all())
    before = _state(flat)
    step = flat.step_count + 1
    tp.iterate([(img, lab)], 1)
    after = _state(flat)
    out["restored_off_anchor"] = bool((bits32(opt.flat_param) == keep[0]).all() and (bits16(opt.flat_param16) == keep[1]).all())
    out["iter_stats"] = tr.engine.stats.cpu().numpy().astype(np.float64)
    out["one_iteration"] = (oracle_step(opt, flat, theta, tr.engine.flat_grad, (before["gamma"], before["m"], before["v"]), step, 1.0, float(after["scalars"][1])),
                            oracle_step(opt, flat, theta, tr.engine.flat_grad, (before["gamma"], before["m"], before["v"]), step, 1.0, None), after)
    # the statistics of a forward pass under the projected weights, on the other trainer
    trb.engine.opt.flat_param.copy_(projected)
    trb.engine.opt.refresh_shadow()
    trb.engine.forward_sums(img, lab, 1.0)
    trb.engine.finalize(lab.numel())
    out["projected_stats"] = trb.engine.stats.cpu().numpy().astype(np.float64)
    # a second object that is given the first one's state before the iteration
    tp2 = TPGM(tr, proj_lr=0.5)
    tp2.load_state_dict(sd)
    tp2.iterate([(img, lab)], 1)
    out["round_trip"] = all(bool(torch.equal(getattr(tp2.flat, a), getattr(flat, a))) for a in ("gamma", "gamma_m", "gamma_v", "ratio")) and \
        tp2.flat.step_count == flat.step_count and tp2.flat.proj_lr == PROJ_LR
    del tp2
    # the final projection at half of each norm
    gamma = (0.5 * norms.astype(np.float64)).astype(np.float32)
    tp.set_constraints(gamma)
    tp.apply()
    out["apply"] = (split(theta, opt), split(flat.flat_anchor, opt), gamma, np.array(flat.flags_host), split(opt.flat_param, opt), flat.ratio.cpu().numpy(),
                    flat.tensor_norms().cpu().numpy())
    out["apply_touched_nothing_else"] = bool((bits32(opt.flat_param)[~_elem_mask(opt)] == keep[0][~_elem_mask(opt)]).all())
    return out


def _elem_mask(opt):
    mask = np.zeros(opt.numel, bool)
    for o, p in zip(opt.offsets, opt.params):
        mask[o:o + p.numel()] = True
    return mask


@pytest.fixture(scope="module", params=[False, True], ids=["eager", "graph"])
def seq(request):
    return _sequence(request.param)


def test_initial_radii_follow_the_init_rule(seq):
    got, want, bnorm = seq["gamma0"]
    heads = [n for n in seq["names"] if "output" in n]
    assert heads == ["output.weight"] and (want >= 3.0).all() and want[seq["names"].index("output.weight")] >= 10.0
    close(got, want, 5.0 * bnorm + U * want, "tpgm.step.gamma0")      # 5 ||theta|| at most, and the rounding to float32


def test_iterate_restores_the_parameters_and_the_shadow(seq):
    assert seq["restored"] and seq["restored_after_raise"] and seq["begin_end_restores"] and seq["restored_off_anchor"]


def test_training_and_iterations_interleave(seq):
    """Two train steps, two iterations (and a broken third), another train step: the train steps' trajectory is that of a run
    without the iterations, at the tolerance of test_eager_and_graph_steps_give_the_same_trajectory (2e-4 of each statistic, kd
    held to 2e-4 of the loss while it is 0 or rounding noise) -- every radius starts wide enough for a ratio of 1, so the iterations
    ran the unprojected weights, moved no radius and left the optimiser alone."""
    e, g = seq["traj_plain"], seq["traj"]
    print("plain", e, "with iterations", g, sep="\n")
    assert seq["wide_radii_stand_still"]
    assert np.isfinite(e).all() and np.isfinite(g).all() and e[2, 0] != e[0, 0]
    scale = np.abs(e).copy()
    scale[:2, 3] = np.abs(e[:2, 0])
    assert (np.abs(e - g) <= 2e-4 * scale).all(), np.abs(e - g) / scale


def test_one_iteration_against_the_host_oracle(seq):
    """The oracle's gamma, Adam moments, norms and ratios, fed the engine's own flat_grad and the saved theta, against the device's
    within the derived bounds; the gradient norm and the clip coefficient by themselves."""
    held, free, got = seq["one_iteration"]
    live = held["live"]
    print("live radii", int(live.sum()), "of", live.size, "gnorm, coef", got["scalars"], "float64", free["gnorm"][0], free["coef"][0])
    assert live.sum() > 0.9 * live.size and (held["q"][live] < 0.6).all()
    (gnorm, bG), (coef, bcoef) = free["gnorm"], free["coef"]
    close(got["scalars"][:1], [gnorm], [bG], "tpgm.step.gnorm")
    if coef == 1.0 and 1.0 / (gnorm + bG + 1e-6) > 1.0:
        assert got["scalars"][1] == 1.0
    else:
        close(got["scalars"][1:], [coef], [bcoef], "tpgm.step.coef")
    check_step(held, got, "tpgm.step.iteration")
    assert (np.abs(got["gamma"] - held["gamma"][0])[live] <= held["gamma"][1][live]).all() and (got["m"][live] != 0).mean() > 0.9


def test_statistics_under_the_projected_weights(seq):
    """[loss, focal, dice, kd, ce] of the iteration's forward pass against a second trainer whose parameters were overwritten with
    the projected buffer (drop-path is 0), at the eager-against-graph tolerance."""
    a, b = seq["iter_stats"], seq["projected_stats"]
    print("iteration", a, "overwritten trainer", b)
    assert np.isfinite(a).all() and np.isfinite(b).all()
    scale = np.abs(b).copy()
    if scale[3] < 0.01 * scale[0]:
        scale[3] = scale[0]
    assert (np.abs(a - b) <= 2e-4 * scale).all(), np.abs(a - b) / scale
    assert not np.allclose(a, seq["traj"][2], rtol=1e-3)                # and they are not those of the unprojected weights


def test_state_dict_round_trip_reproduces_the_next_iteration(seq):
    assert seq["round_trip"]


def test_apply_projects_to_half_of_each_norm(seq):
    """apply() after set_constraints(half of each measured norm): the parameters equal project_ref within the bound of the
    projection (the ratio's own bound included), nothing else in the buffer moved, and the norms measured afterwards equal gamma:
    by the triangle inequality within the 2-norm of the elements' bounds, the bound of the norm kernel and gamma 1e-8 / norm."""
    thetas, anchors, gamma, flags, got, ratio_dev, norms_after = seq["apply"]
    assert seq["apply_touched_nothing_else"]
    numel = [p.size for p in thetas]
    norms = norms_ref(thetas, anchors, False)
    nb = np.array([norm_bound(x, n, cdiv(n, 16384), False) for x, n in zip(norms, numel)])
    ratio, live, q = ratios_ref(gamma.astype(np.float64), norms, flags)
    br = ratio_bound(ratio, q, nb[:, 1], flags)
    close(ratio_dev, ratio, br, "tpgm.step.apply.ratio")
    assert live.sum() > 0.9 * live.size and (np.abs(ratio[live] - 0.5) < 1e-6).all() and not (flags & EXCLUDED).any()
    want = project_ref(thetas, anchors, ratio)
    worst = 0.0
    for t, (w, g, p, a) in enumerate(zip(want, got, thetas, anchors)):
        b = project_bound(p, a, ratio[t], br[t])
        err = np.abs(g.astype(np.float64) - w)
        assert (err <= b).all(), (t, float(err.max()), float(b[np.argmax(err)]))
        worst = max(worst, float((err / np.maximum(b, 1e-300)).max()))
        after = ratio[t] * norms[t]
        bound = float(np.sqrt((b * b).sum())) + norm_bound(after, numel[t], cdiv(numel[t], 16384), False)[0] + after * NORM_EPS / max(norms[t], NORM_EPS)
        assert abs(norms_after[t] - after) <= bound, (t, norms_after[t], after, bound)
        if live[t]:
            slack = gamma[t] * NORM_EPS / norms[t] + 8 * 2.0 ** -53 * gamma[t]        # the 1e-8 under the quotient, and float64's own roundings
            assert abs(after - gamma[t]) <= slack and abs(norms_after[t] - gamma[t]) <= bound + slack
    print("apply: largest |error| / bound", worst)
