"""The training step with the boundary objective (HipEngine(boundary=...)) on the smallest model the trainer tests use
(tests/test_gpu_continual_step.py's), B = 2, organ-like labels: captured and eager steps agree, the weight alpha is a device
float that a replayed graph reads, the option left out is the step as it was, and trainer_synapse schedules the weight per epoch.

"The step as it was" is held to the build before the feature: tests/golden/boundary_step_parent.npz holds the bits of the
three-step stats, the buffer sizes and the SHA-256 of the parameters after the third step, written by
`PYTHONPATH=. python tests/test_gpu_boundary_step.py record` on that build (the record path uses nothing the feature added but
the label maker of tests/sdm_cases.py, which is plain numpy)."""
import hashlib
import logging
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle.determ import det_normal, fill_state_dict

import sdm_cases as S
from test_gpu_parity import DEV, T

pytestmark = pytest.mark.gpu

NCLS = 9
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "boundary_step_parent.npz")
GRAPH_RTOL = 2e-4                                        # what tests/test_gpu_continual_step.py allows between eager and captured steps


def _model():
    import cswin_unet_amd.networks.cswin_unet as N
    return fill_state_dict(N.CSWinTransformer(img_size=224, num_classes=NCLS, embed_dim=64, depth=[1, 1, 1, 1], split_size=[1, 2, 7, 7],
                                              num_heads=[2, 4, 8, 16], qkv_bias=True, drop_path_rate=0.).to(DEV)).train()


def _batch():
    img = T(det_normal("bdstep.x", (2, 1, 224, 224))).repeat(1, 3, 1, 1)
    lab = torch.from_numpy(S.blob_labels(2, 224, 224, NCLS, 4242)).to(DEV)
    return img, lab


def _trainer(use_graph, base_lr=0.05, **kw):
    from cswin_unet_amd.trainer import DataParallelTrainer
    return DataParallelTrainer(_model(), NCLS, base_lr=base_lr, max_iterations=100, use_graph=use_graph, **kw)


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def _default_step(**kw):
    """Three captured steps without the option: the bits of the stats, of ops.ce_dice_loss on the first step's logits, the
    buffer sizes and the digest of the parameters afterwards."""
    from cswin_unet_amd import ops
    img, lab = _batch()
    with torch.no_grad():
        _, first = ops.ce_dice_loss(_model()(img), lab)
    tr = _trainer(True, **kw)
    stats = np.stack([_bits(tr.train_step(img, lab)) for _ in range(3)])
    return dict(stats=stats, step0_op=_bits(first), sizes=np.array([tr.engine.sums.numel(), tr.engine.stats.numel()], np.int64),
                params_sha256=np.frombuffer(hashlib.sha256(_bits(tr.engine.flat_param).tobytes()).digest(), np.uint8).copy())


@pytest.fixture(scope="module")
def runs():
    """Three steps eagerly and from hipGraphs with boundary=0.01, and twice without: computed once."""
    img, lab = _batch()
    out = {}
    for name, use_graph in (("eager", False), ("graph", True)):
        tr = _trainer(use_graph, boundary=0.01)
        assert tr.engine.sums.numel() == 2 + 3 * NCLS and tr.engine.stats.numel() == 4
        out[name] = np.array([[float(v) for v in tr.train_step(img, lab)] for _ in range(3)])
        out[name + ".params"] = tr.engine.flat_param.detach().clone()
    for name, kw in (("none", dict(boundary=None)), ("today", {})):
        out[name] = _default_step(**kw)
    return out


def test_step0_matches_the_public_op_and_the_terms_add_up(runs):
    from cswin_unet_amd import ops
    img, lab = _batch()
    with torch.no_grad():
        logits = _model()(img)
    _, stats = ops.boundary_loss(logits, lab, 0.01)
    s0 = runs["eager"][0]
    print("step 0 stats", s0)
    assert np.array_equal(np.array([float(v) for v in stats]), s0), (stats, s0)
    assert abs(s0[0] - (0.4 * s0[1] + 0.6 * s0[2] + np.float32(0.01) * s0[3])) <= 1e-6 * abs(s0[0])
    assert abs(s0[3]) > 0.1                                               # organs a few dozen pixels across: the term is live


def test_eager_and_graph_steps_give_the_same_trajectory(runs):
    e, g = runs["eager"], runs["graph"]
    print("eager", e, "graph", g, sep="\n")
    assert np.isfinite(e).all() and np.isfinite(g).all() and e[2, 0] != e[0, 0]
    assert (np.abs(e - g) <= GRAPH_RTOL * np.abs(e)).all(), np.abs(e - g) / np.abs(e)
    pe, pg = runs["eager.params"], runs["graph.params"]
    rms = float(pe.double().pow(2).mean().sqrt())
    err = float((pe - pg).abs().max()) / rms
    print(f"parameters after three steps: max |eager - graph| / rms = {err:.3e}")
    assert err <= GRAPH_RTOL


def test_set_boundary_weight_reaches_a_replayed_graph():
    """At a learning rate of 0 the parameters stay, so every step sees the same forward.  A captured engine built with 0.01 and
    set to 0.5 between replays must then give the loss and the gradient of a fresh eager engine built with 0.5: alpha is not baked
    into the graph."""
    img, lab = _batch()
    tr = _trainer(True, base_lr=0.0, boundary=0.01)
    a = tr.train_step(img, lab).cpu().numpy().copy()
    a2 = tr.train_step(img, lab).cpu().numpy().copy()                     # a replay: nothing changed
    g_a = tr.engine.flat_grad.detach().clone()
    tr.set_boundary_weight(0.5)
    b = tr.train_step(img, lab).cpu().numpy().copy()
    g_b = tr.engine.flat_grad.detach().clone()
    fresh = _trainer(False, base_lr=0.0, boundary=0.5)
    c = fresh.train_step(img, lab).cpu().numpy().copy()
    g_c = fresh.engine.flat_grad.detach().clone()
    print("alpha 0.01", a, "set to 0.5", b, "fresh 0.5", c, sep="\n")
    assert (np.abs(a - a2) <= GRAPH_RTOL * np.abs(a)).all()
    assert (np.abs(b - c) <= GRAPH_RTOL * np.abs(c)).all()
    assert (np.abs(b[1:] - a[1:]) <= GRAPH_RTOL * np.abs(a[1:])).all()    # the terms themselves did not move
    moved = (np.float32(0.5) - np.float32(0.01)) * a[3]
    assert abs((b[0] - a[0]) - moved) <= GRAPH_RTOL * abs(b[0]) and abs(moved) > 100 * GRAPH_RTOL * abs(b[0])
    rms = float(g_c.double().pow(2).mean().sqrt())
    err_bc, diff_ab = float((g_b - g_c).abs().max()) / rms, float((g_b - g_a).abs().max()) / rms
    print(f"gradient: |set - fresh| / rms = {err_bc:.3e}, |set - before| / rms = {diff_ab:.3e}")
    assert err_bc <= GRAPH_RTOL and diff_ab > 100 * GRAPH_RTOL
    assert tr.engine.objective.alpha == 0.5 and float(tr.engine.objective.alpha_dev) == 0.5


def test_boundary_none_is_the_parents_step_bit_for_bit(runs):
    """boundary=None and the keyword left out: three captured steps give the stats, the buffer sizes and the parameters that
    the build before the feature recorded, bit for bit; and the first step's stats are ops.ce_dice_loss's on the same logits."""
    want = np.load(GOLDEN)
    for name in ("none", "today"):
        got = runs[name]
        print(name, got["stats"].view(np.float32))
        assert got["sizes"].tolist() == [1 + 3 * NCLS, 3] == want["sizes"].tolist()
        assert np.array_equal(got["stats"][0], got["step0_op"])
        for key in ("stats", "step0_op", "params_sha256"):
            assert np.array_equal(got[key], want[key]), (name, key)


def test_boundary_with_distill_raises_and_fields_come_as_a_dict():
    from cswin_unet_amd.continual import Distill, freeze_teacher
    from cswin_unet_amd.trainer import HipEngine
    net = _model()
    with pytest.raises(ValueError, match="distill"):
        HipEngine(net, NCLS, 0.05, 0.9, 1e-4, 0.4, 0.6, use_graph=False, distill=Distill(teacher=freeze_teacher(net)), boundary=0.01)
    wb = torch.linspace(0.5, 2.0, NCLS, device=DEV)
    eng = HipEngine(net, NCLS, 0.05, 0.9, 1e-4, 0.4, 0.6, use_graph=False, boundary=dict(alpha=0.2, boundary_class_weight=wb, w_dice=0.5))
    o = eng.objective
    assert (o.alpha, o.w_ce, o.w_dice) == (0.2, 0.4, 0.5) and o.boundary_class_weight is wb and float(o.alpha_dev) == np.float32(0.2)
    plain = HipEngine(_model(), NCLS, 0.05, 0.9, 1e-4, 0.4, 0.6, use_graph=False)
    with pytest.raises(ValueError, match="boundary"):
        plain.set_boundary_weight(0.1)
    for bad in (True, float("nan"), float("inf"), "0.1", dict(alpha=float("nan")), dict(alpha=0.1, dist_maps=torch.zeros(1, device=DEV)),
                dict(alpha=0.1, gamma=2.0)):
        with pytest.raises(ValueError, match="boundary"):
            HipEngine(net, NCLS, 0.05, 0.9, 1e-4, 0.4, 0.6, use_graph=False, boundary=bad)
    for bad in (True, float("nan")):
        with pytest.raises(ValueError, match="boundary"):
            eng.set_boundary_weight(bad)


def test_trainer_synapse_schedules_the_boundary_weight(tmp_path):
    """Two epochs on synthetic slices with boundary_weight=kervadec_alpha and the device augmentation (the labels exist on the
    device only): the weight moves from 0.01 to 0.02, and every log line carries four stats."""
    from cswin_unet_amd.config import get_config
    from cswin_unet_amd.datasets import write_synthetic_synapse
    from cswin_unet_amd.networks.vision_transformer import CSwinUnet
    from cswin_unet_amd.trainer import kervadec_alpha, trainer_synapse
    train, _, lists = write_synthetic_synapse(str(tmp_path / "data"), n_slices=8, n_volumes=0, size=256)
    cfg = get_config(**{"MODEL.DROP_PATH_RATE": 0.0})
    torch.manual_seed(0)
    net = CSwinUnet(cfg, img_size=224, num_classes=9).to(DEV)
    args = SimpleNamespace(root_path=train, list_dir=lists, img_size=224, num_classes=9, batch_size=4, base_lr=0.05,
                           max_epochs=2, num_workers=0, seed=1234, augment="hip", boundary_weight=kervadec_alpha)
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
    torch.cuda.synchronize()
    alphas = [float(m.split("boundary weight : ")[1]) for m in records if m.startswith("epoch")]
    lines = [m for m in records if m.startswith("iteration")]
    stats = [[float(part.split(": ")[1]) for part in m.split(" : ", 1)[1].split(", ")] for m in lines]
    print("alphas", alphas, "stats", stats)
    assert alphas == [0.01, 0.02]
    assert len(stats) == 4 and all(len(s) == 4 and all(np.isfinite(v) for v in s) for s in stats)
    assert all("loss_boundary" in m for m in lines)
    with pytest.raises(ValueError, match="boundary_weight"):
        trainer_synapse(SimpleNamespace(boundary_weight="often", augment="hip"), None, str(tmp_path / "never"))
    assert not (tmp_path / "never").exists()


if __name__ == "__main__":
    assert sys.argv[1:] == ["record"], "usage: PYTHONPATH=. python tests/test_gpu_boundary_step.py record   (on the build before the feature)"
    got = _default_step()
    assert got["sizes"].tolist() == [1 + 3 * NCLS, 3] and np.array_equal(got["stats"][0], got["step0_op"])
    np.savez(os.environ.get("BOUNDARY_STEP_GOLDEN", GOLDEN), **got)
    print("recorded", got["stats"].view(np.float32), got["params_sha256"].tobytes().hex())
