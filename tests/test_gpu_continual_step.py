"""The training step with the continual-learning objective (HipEngine(distill=...)): a 9-class teacher, the student widened to 12
classes by continual.expand_classes, B = 2, a label map and class weights, on the smallest model the trainer tests use."""
import numpy as np
import pytest
import torch

from oracle.determ import det_labels, det_normal, fill_state_dict

from test_gpu_parity import DEV, T
from test_gpu_step_tail import U
from test_continual_host import cl_final_ref, cl_ref

pytestmark = pytest.mark.gpu

OLD, NEW, KD_WEIGHT, TEMP = 9, 4, 0.5, 3.0
# KD is a per-IMAGE sum over 50 176 pixels (batchmean), so its curvature in the weights is several 1e4 times that of the per-pixel
# means and plain SGD needs a step that much smaller than the base loss's 0.05 (the reference clips the gradient norm and uses
# AdamW).  At the 3e-6 used here kd, 0 at the first step, is comparable to the loss at the third; measured on an MI355X:
# loss 0.576278, 0.576659, 1.492824 and kd 0, 8.17e-4, 1.83196.
LR = 3e-6
COUNTS = [80000.0, 0, 0, 0, 0, 0, 0, 0, 0, 9000.0, 7000.0, 4352.0]


def _models(expand=True):
    """(student widened to 12 classes, frozen 9-class teacher): the same weights every time."""
    import cswin_unet_amd.networks.cswin_unet as N
    from cswin_unet_amd.continual import expand_classes, freeze_teacher
    net = fill_state_dict(N.CSWinTransformer(img_size=224, num_classes=OLD, embed_dim=64, depth=[1, 1, 1, 1], split_size=[1, 2, 7, 7],
                                             num_heads=[2, 4, 8, 16], qkv_bias=True, drop_path_rate=0.).to(DEV)).train()
    teacher = freeze_teacher(net)
    if not expand:
        return net, teacher
    torch.manual_seed(1234)
    assert expand_classes(net, NEW) == OLD and net.num_classes == OLD + NEW - 1
    return net, teacher


def _batch():
    img = T(det_normal("clstep.x", (2, 1, 224, 224))).repeat(1, 3, 1, 1)
    lab = T(det_labels("clstep.labels", (2, 224, 224), NEW))
    return img, lab


def _distill(teacher):
    from cswin_unet_amd.continual import Distill, extreme_class_weights, new_label_map
    return Distill(teacher=teacher, kd_weight=KD_WEIGHT, temperature=TEMP, class_weight=extreme_class_weights(COUNTS, [0, 9, 10, 11]).to(DEV),
                   label_map=new_label_map(OLD, NEW, DEV))


@pytest.fixture(scope="module")
def runs():
    """Three steps eagerly and from hipGraphs with distill, and twice without: computed once."""
    from cswin_unet_amd.trainer import DataParallelTrainer
    img, lab = _batch()
    out = {}
    for name, use_graph in (("eager", False), ("graph", True)):
        net, teacher = _models()
        before = [p.detach().clone() for p in teacher.parameters()]
        d = _distill(teacher)
        if name == "eager":
            with torch.no_grad():
                out["logits"], out["teacher_logits"] = net(img).clone(), teacher(img).clone()
        tr = DataParallelTrainer(net, OLD + NEW - 1, base_lr=LR, max_iterations=100, use_graph=use_graph, distill=d)
        assert tr.engine.sums.numel() == 3 + 3 * 12 and tr.engine.stats.numel() == 5
        out[name] = np.array([[float(v) for v in tr.train_step(img, lab)] for _ in range(3)])
        out[name + ".teacher_same"] = all(torch.equal(a, b) for a, b in zip(before, teacher.parameters()))
        out[name + ".teacher_frozen"] = all(p.grad is None and not p.requires_grad for p in teacher.parameters())
        out["distill"] = d
    # without the option, on the same model before its expansion (the base loss has no 12-class instantiation)
    lab9 = T(det_labels("clstep.labels9", (2, 224, 224), OLD))
    for name, kw in (("none", dict(distill=None)), ("today", {})):
        net = _models(expand=False)[0]
        tr = DataParallelTrainer(net, OLD, base_lr=0.05, max_iterations=100, use_graph=True, **kw)
        assert tr.engine.sums.numel() == 1 + 3 * OLD and tr.engine.stats.numel() == 3 and tr.engine.distill is None
        out[name] = torch.stack([tr.train_step(img, lab9).clone() for _ in range(3)]).cpu()
    return out


def test_step0_has_no_kd_and_matches_the_public_op(runs):
    """Right after expansion the student's first 9 logit channels are the teacher's: kd is below its bound, loss is
    (1 - kd_weight) * (w_focal * focal + w_dice * dice), and the step's stats are ops.continual_loss's on eagerly computed logits."""
    from cswin_unet_amd import ops
    img, lab = _batch()
    d = runs["distill"]
    x, t = runs["logits"], runs["teacher_logits"]
    assert x.shape == (2, 12, 224, 224) and t.shape == (2, 9, 224, 224)
    print("max |student[:, :9] - teacher| =", float((x[:, :OLD] - t).abs().max()))
    ref, bound = cl_ref(x.cpu().numpy().reshape(2, 12, -1), lab.cpu().numpy().reshape(2, -1), t.cpu().numpy().reshape(2, 9, -1), TEMP, 1.0, 4.0,
                        d.class_weight.cpu().numpy(), d.label_map.cpu().numpy())
    want, bwant, _ = cl_final_ref(ref, lab.numel(), 2, 0.2, 0.8, KD_WEIGHT, TEMP, bsums=bound)
    s0 = runs["eager"][0]
    print("step 0 stats", s0, "float64", want, "bounds", bwant)
    assert abs(s0[3]) <= bwant[3] + abs(want[3])
    assert abs(s0[0] - (1 - KD_WEIGHT) * (0.2 * s0[1] + 0.8 * s0[2])) <= bwant[0] + KD_WEIGHT * bwant[3] + 8 * U * abs(s0[0])
    assert (np.abs(s0 - want) <= bwant).all(), (s0, want, bwant)
    _, stats = ops.continual_loss(x, lab, t, kd_weight=KD_WEIGHT, temperature=TEMP, class_weight=d.class_weight, label_map=d.label_map)
    assert np.array_equal(np.array([float(v) for v in stats]), s0), (stats, s0)


def test_eager_and_graph_steps_give_the_same_trajectory(runs):
    """Three steps with use_graph=False and use_graph=True: the tolerance of the existing eager-against-graph trainer test (2e-4 of
    each statistic).  kd is 0 at the first step and rounding noise of a per-image sum at the second, so there it is held to 2e-4 of
    the loss, which it enters with weight kd_weight; at the third step it is live and held to 2e-4 of itself."""
    e, g = runs["eager"], runs["graph"]
    print("eager", e, "graph", g, sep="\n")
    assert np.isfinite(e).all() and np.isfinite(g).all()
    assert e[2, 0] != e[0, 0] and e[2, 3] > 0.01 * e[2, 0]               # the steps moved the loss; KD is live at the third
    scale = np.abs(e).copy()
    scale[:2, 3] = np.abs(e[:2, 0])
    assert (np.abs(e - g) <= 2e-4 * scale).all(), np.abs(e - g) / scale


def test_teacher_is_untouched(runs):
    assert runs["eager.teacher_same"] and runs["graph.teacher_same"]
    assert runs["eager.teacher_frozen"] and runs["graph.teacher_frozen"]


def test_distill_none_is_todays_step(runs):
    """distill=None and the keyword left out take the same branch, so this pins little by itself: that the option exists and
    defaults to None, that two runs of the step on the same 9-class model (before its expansion: the base loss has no 12-class
    instantiation) give the same three-step stats bit for bit, and, in the runs fixture, the buffer sizes of the step without the
    option.  That the base path is unchanged is shown by the existing suite passing unmodified."""
    assert runs["none"].shape == (3, 3) and torch.equal(runs["none"], runs["today"])
