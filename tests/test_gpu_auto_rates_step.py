"""The training step of the reference's surgical fine-tuning (finetune.py:146-254) on the tiny model, B = 2 at 224 x 224:
torch.optim.Adam with coupled weight decay and, at every step, a learning rate per parameter group from that step's own gradient
(HipEngine(optimizer="adam").set_auto_rates).  The optimiser is isolated by taking the gradients from the engine: the float64
references of test_auto_rates_host are applied to a copy of the engine's own flat_grad and initial weights."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from test_auto_rates_host import adam_bound, adam_ref, group_rates_bound, group_rates_ref, one_group_at_one
from test_gpu_multirank import _free_port

pytestmark = pytest.mark.gpu
DEV = "cuda"
LR, WD = 1e-3, 1e-4                               # the first pair of finetune.py's grid
MODES = ("kept", "fresh")


def _model():
    from cswin_unet_amd.networks import cswin_unet as N
    from oracle.determ import fill_state_dict
    net = N.CSWinTransformer(img_size=224, num_classes=9, embed_dim=64, depth=[1, 2, 9, 1], split_size=[1, 2, 7, 7], num_heads=[2, 4, 8, 16],
                             mlp_ratio=4., qkv_bias=True, drop_path_rate=0.).to(DEV)
    return fill_state_dict(net).train()


def _batch():
    from oracle.determ import det_labels, det_normal
    img = torch.from_numpy(det_normal("model.x", (2, 1, 224, 224))).repeat(1, 3, 1, 1).to(DEV)
    return img, torch.from_numpy(det_labels("model.labels", (2, 224, 224), 9)).to(DEV)


def _trainer(net, moments, use_graph, lr=LR, group=None, auto=True):
    from cswin_unet_amd.continual import finetune_groups
    from cswin_unet_amd.trainer import DataParallelTrainer, HipEngine
    eng = HipEngine(net, 9, lr, 0.9, WD, 0.2, 0.8, use_graph=use_graph, optimizer="adam", moments=moments)
    tr = DataParallelTrainer(net, 9, base_lr=lr, engine=eng, lr_schedule="constant", group=group)
    if auto:
        tr.set_auto_rates(finetune_groups(net))
    return tr


def _stats(tr, img, lab):
    return np.array([float(v) for v in tr.train_step(img, lab)])


@pytest.fixture(scope="module")
def runs():
    """Three steps eagerly in both moment modes and from hipGraphs with kept moments, and each eager run's state round the first
    step: computed once."""
    img, lab = _batch()
    out = {}
    for name, moments, use_graph in (("kept", "kept", False), ("fresh", "fresh", False), ("graph", "kept", True)):
        net = _model()
        tr = _trainer(net, moments, use_graph)
        opt = tr.engine.opt
        assert type(opt).__name__ == "FlatAdamW" and not opt.decoupled and opt.moments == moments and opt.weight_decay == WD and opt.max_grad_norm is None
        assert len(opt.params) == 463 and len(opt.group_names) == 22 and opt.group_stats.shape == (22,)
        rows = []
        for k in range(3):
            if k == 0:
                out[name + ".p0"] = opt.flat_param.clone()
            rows.append(_stats(tr, img, lab))
            if k == 0 and not use_graph:
                out[name + ".1"] = dict(g=opt.flat_grad.clone(), p=opt.flat_param.clone(), stat=opt.group_stats.clone(), mult=opt.lr_weights.clone(),
                                        m=opt.flat_m.clone(), v=opt.flat_v.clone(), model={k_: v.clone() for k_, v in net.state_dict().items()},
                                        opt=opt.state_dict(), names=list(tr.engine.param_names), groups=list(opt.group_names),
                                        layout=(list(opt.offsets), [p.numel() for p in opt.params]), lr=float(opt.lr_dev.cpu()[0]))
        assert opt.step_count == 3 and float(opt.lr_dev.cpu()[0]) == float(np.float32(LR))
        out[name] = np.array(rows)
    return out


def _mask(layout, total):
    mask = np.zeros(total, bool)
    for o, n in zip(*layout):
        mask[o:o + n] = True
    return mask


@pytest.mark.parametrize("moments", MODES)
def test_one_step_matches_float64_on_the_engines_gradients(runs, moments):
    """After one step the 22 statistics and the 463 multipliers are within their derived bounds of the float64 group norms of a copy
    of the engine's flat_grad, in finetune.py's group order with exactly one group at 1; and every parameter is within the derived
    bound of adam_ref (coupled decay, the moments mode) applied to the same copy at the multipliers the kernel was given."""
    from cswin_unet_amd.continual import FINETUNE_GROUPS
    from test_gpu_step_tail import close
    s = runs[moments + ".1"]
    p0, g, p1 = runs[moments + ".p0"].cpu().numpy().astype(np.float64), s["g"].cpu().numpy().astype(np.float64), s["p"].cpu().numpy().astype(np.float64)
    offsets, numels = s["layout"]
    mask = _mask(s["layout"], p0.size)
    assert (g[~mask] == 0).all() and s["groups"] == [name for name, _ in FINETUNE_GROUPS]
    from cswin_unet_amd.continual import finetune_groups
    where = {n: k for k, members in enumerate(finetune_groups(_model_on_cpu()).values()) for n in members}
    group_of = [where[n] for n in s["names"]]
    sg = np.array([float((g[o:o + n] ** 2).sum()) for o, n in zip(offsets, numels)])
    sp = np.array([float((p0[o:o + n] ** 2).sum()) for o, n in zip(offsets, numels)])
    chunks = [-(-n // 16384) for n in numels]
    want_stat, want_mult = group_rates_ref(sg, sp, group_of, 22, "grad")
    bstat, bmult = group_rates_bound(sg, sp, numels, chunks, group_of, 22, "grad")
    stat, mult = s["stat"].cpu().numpy(), s["mult"].cpu().numpy()
    close(stat, want_stat, bstat, f"auto.step.{moments}.group_stat")
    close(mult, want_mult, bmult, f"auto.step.{moments}.lr_mult")
    assert one_group_at_one(mult, group_of) and (mult > 0).all() and (mult <= 1).all()
    print("group rates / lr:", dict(zip(s["groups"], (stat / stat.max()).round(4).tolist())))
    mult_e = np.ones_like(p0)
    for o, n, mu in zip(offsets, numels, mult.astype(np.float64)):
        mult_e[o:o + n] = mu
    zeros = np.zeros_like(p0)
    kw = dict(wd=WD, mult=mult_e, coupled=True, fresh=moments == "fresh")
    want = adam_ref(p0, g, zeros, zeros, 1, s["lr"], **kw)
    bound = adam_bound(p0, g, zeros, zeros, 1, s["lr"], **kw)
    close(p1[mask], want[0][mask], bound[0][mask], f"auto.step.{moments}.p")
    assert (np.abs(p1 - p0)[mask] > 0).mean() > 0.99
    m, v = s["m"].cpu().numpy(), s["v"].cpu().numpy()
    if moments == "fresh":
        assert (m == 0).all() and (v == 0).all()                          # never written
    else:
        close(m[mask], want[1][mask], bound[1][mask], "auto.step.kept.m")
        close(v[mask], want[2][mask], bound[2][mask], "auto.step.kept.v")


def _model_on_cpu():
    from cswin_unet_amd.networks import cswin_unet as N
    return N.CSWinTransformer(img_size=224, num_classes=9, embed_dim=64, depth=[1, 2, 9, 1], split_size=[1, 2, 7, 7], num_heads=[2, 4, 8, 16])


def test_the_two_moment_modes_part_after_the_first_step(runs):
    """The first step of Adam IS a fresh optimiser's step: the same weights bit for bit; from the second on the runs differ."""
    assert torch.equal(runs["kept.1"]["p"], runs["fresh.1"]["p"]) and np.array_equal(runs["kept"][:2], runs["fresh"][:2])
    assert runs["kept"][2, 0] != runs["fresh"][2, 0]
    print("loss, kept moments", runs["kept"][:, 0], "fresh moments", runs["fresh"][:, 0])
    assert np.isfinite(runs["kept"]).all() and np.isfinite(runs["fresh"]).all()


def test_eager_and_graph_steps_give_the_same_trajectory(runs):
    """Three steps with use_graph=False and use_graph=True at the tolerance of tests/test_gpu_adamw_step.py: 2e-4 of each statistic.
    The rates are formed inside the replayed step, so a graph that froze the first step's multipliers would part from the eager run."""
    e, g = runs["kept"], runs["graph"]
    print("eager", e, "graph", g, sep="\n")
    assert e.shape == (3, 3) and np.isfinite(e).all() and np.isfinite(g).all()
    assert (np.abs(e - g) <= 2e-4 * np.abs(e)).all(), np.abs(e - g) / np.abs(e)
    assert e[1, 0] != e[0, 0]


def test_state_dict_round_trip_reproduces_the_third_step(runs):
    """The model's and the optimiser's state after the first step, loaded into a fresh engine that was never told about the rates,
    give the second and third steps' stats bit for bit; a state dict from before the new keys loads as it always did."""
    img, lab = _batch()
    s = runs["kept.1"]
    net = _model()
    tr = _trainer(net, "kept", False, auto=False)
    opt = tr.engine.opt
    assert opt.lr_weights is None
    net.load_state_dict(s["model"])
    opt.load_state_dict(s["opt"])
    assert opt.step_count == 1 and torch.equal(opt.flat_param, s["p"]) and opt.group_names == s["groups"] and torch.equal(opt.lr_weights, s["mult"])
    sd = opt.state_dict()
    assert set(sd) == {"m", "v", "step", "lr", "lr_weights", "decoupled", "moments", "auto_rates"}
    assert sd["decoupled"] is False and sd["moments"] == "kept" and sd["auto_rates"]["statistic"] == "grad" and len(sd["auto_rates"]["groups"]) == 463
    rows = np.array([_stats(tr, img, lab) for _ in range(2)])
    assert np.array_equal(rows, runs["kept"][1:]), (rows, runs["kept"][1:])
    old = {k: s["opt"][k] for k in ("m", "v", "step", "lr")}
    old["lr_weights"] = None
    opt.load_state_dict(old)
    assert opt.lr_weights is None and not opt.decoupled and opt.moments == "kept" and opt.step_count == 1
    with pytest.raises(RuntimeError, match="set_auto_rates"):
        opt.group_stats


def test_one_group_per_tensor_in_the_ratio_mode_is_rgn_weights():
    """set_auto_rates over one group per tensor with statistic "ratio", the tensors continual.rgn_weights drops (names with "bn" or
    "norm") in no group: the multipliers of a step equal rgn_weights of tensor_norms() of the same gradient and weights (the rate is
    0, so the step leaves them).  Bound: both sides start from the same sums of squares; group_rates_bound covers the device's
    operations from exact sums, and the host path (a float32 square root per norm, then float64) stays inside the same bound, so the
    two may differ by twice that."""
    from cswin_unet_amd.continual import rgn_weights
    img, lab = _batch()
    net = _model()
    tr = _trainer(net, "kept", False, lr=0.0, auto=False)
    names = tr.engine.param_names
    keep = [n for n in names if "bn" not in n.lower() and "norm" not in n.lower()]
    assert 0 < len(keep) < len(names)
    tr.set_auto_rates({n: [n] for n in keep}, "ratio", default=0.0)
    opt = tr.engine.opt
    p0 = opt.flat_param.clone()
    tr.train_step(img, lab)
    assert torch.equal(opt.flat_param, p0) and len(opt.group_names) == len(keep)
    mult = opt.lr_weights.cpu().numpy().astype(np.float64)
    norms = opt.tensor_norms().cpu()
    want = rgn_weights(names, [norms])
    assert list(want) == keep
    numels = [p.numel() for p in opt.params]
    group_of = [keep.index(n) if n in want else -1 for n in names]
    sq = norms.double().numpy() ** 2
    _, bmult = group_rates_bound(sq[:, 0], sq[:, 1], numels, [-(-n // 16384) for n in numels], group_of, len(keep), "ratio")
    worst = 0.0
    for t, n in enumerate(names):
        if n in want:
            assert abs(mult[t] - want[n]) <= 2 * bmult[t], (n, mult[t], want[n], bmult[t])
            worst = max(worst, abs(mult[t] - want[n]) / (2 * bmult[t]))
        else:
            assert mult[t] == 0.0, n
    print(f"ratio per tensor vs rgn_weights: {len(keep)} of {len(names)} tensors, largest |difference| / bound {worst:.3f}")
    assert max(want.values()) == 1.0 and (mult == 1.0).sum() == 1
    with pytest.raises(KeyError):
        tr.set_auto_rates({"g": ["no.such.weight"]})
    tr.engine.set_lr_weights({n: 1.0 for n in keep})                      # the two replace each other
    with pytest.raises(RuntimeError, match="set_auto_rates"):
        opt.group_stats


def test_surgical_trainer_on_synthetic_dataset(tmp_path):
    """surgical_trainer end to end for one (lr, wd) pair: 8 slices of which half are drawn, batch 2, one epoch = two steps; the
    checkpoint has finetune.py:251's name and loads back."""
    import logging
    from cswin_unet_amd.checkpoint import load_checkpoint
    from cswin_unet_amd.config import get_config
    from cswin_unet_amd.datasets import write_synthetic_synapse
    from cswin_unet_amd.networks.vision_transformer import CSwinUnet
    from cswin_unet_amd.trainer import surgical_trainer
    train, _, lists = write_synthetic_synapse(str(tmp_path / "data"), n_slices=8, n_volumes=0, size=256)
    cfg = get_config(**{"MODEL.DROP_PATH_RATE": 0.0})
    torch.manual_seed(0)
    net = CSwinUnet(cfg, img_size=224, num_classes=9).to(DEV)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    args = SimpleNamespace(root_path=train, list_dir=lists, img_size=224, num_classes=9, batch_size=2, base_lr=LR, weight_decay=WD, max_epochs=1,
                           num_workers=0, seed=1234, subset_fraction=0.5)
    records = []
    h = logging.Handler()
    h.emit = lambda r: records.append(r.getMessage())
    root = logging.getLogger()
    old_level = root.level
    root.setLevel(logging.INFO)
    root.addHandler(h)
    try:
        assert surgical_trainer(args, net, str(tmp_path / "snap")) == "Surgical Training Finished!"
    finally:
        root.removeHandler(h)
        root.setLevel(old_level)
    assert not hasattr(args, "optimizer")                                 # the caller's args are not written to
    losses = [float(m.split("loss : ")[1].split(",")[0]) for m in records if m.startswith("iteration") and "loss :" in m]
    rates = [m for m in records if "group rates" in m]
    assert len(losses) == 2 and np.isfinite(losses).all() and len(rates) == 2 and "'stem'" in rates[0] and "'output'" in rates[0]
    ck = tmp_path / "snap" / f"model_lr{LR}_wd{WD}_epoch0.pth"
    assert ck.exists() and [f for f in os.listdir(tmp_path / "snap") if f.endswith(".pth")] == [ck.name]
    other = CSwinUnet(cfg, img_size=224, num_classes=9)
    msg = load_checkpoint(other, str(ck))
    assert not msg.missing_keys and not msg.unexpected_keys
    assert any(not torch.equal(v, before[k].cpu()) for k, v in other.state_dict().items())      # it holds the trained weights


def _rank_main(rank, world, port, backend, out):
    import torch.distributed as dist
    n_dev = torch.cuda.device_count()
    torch.cuda.set_device(rank % n_dev)
    dist.init_process_group(backend, init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    net = _model()
    if rank != 0:                       # replicas must come from rank 0's broadcast, not from identical construction
        with torch.no_grad():
            for p in net.parameters():
                p.mul_(0.5)
    img, lab = _batch()
    img, lab = img[rank:rank + 1].contiguous(), lab[rank:rank + 1].contiguous()
    tr = _trainer(net, "kept", True, group=dist.group.WORLD)
    assert tr.collectives and tr.world == 2
    losses = [float(tr.train_step(img, lab)[0]) for _ in range(2)]
    opt = tr.engine.opt
    torch.cuda.synchronize()
    out.put((rank, losses, opt.group_stats.cpu().numpy().tobytes(), opt.lr_weights.cpu().numpy().tobytes(), opt.flat_param.cpu().numpy().tobytes()))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_form_the_same_rates_and_stay_identical():
    """Two rank processes, one image each: the update runs after the all-reduce, so both ranks form the same statistics and
    multipliers from the same averaged gradient and their parameters are bit-identical after two steps."""
    import queue
    import time
    import torch.multiprocessing as mp
    backend = "nccl" if torch.cuda.device_count() >= 2 else "gloo"
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_main, args=(r, 2, port, backend, q), daemon=True) for r in range(2)]
    for p in procs:
        p.start()
    res = {}
    try:
        t0 = time.time()
        while len(res) < 2 and time.time() - t0 < 300:
            try:
                item = q.get(timeout=2)
                res[item[0]] = item[1:]
            except queue.Empty:
                if any(p.exitcode not in (None, 0) for p in procs):          # a dead rank: do not wait for the other
                    break
    finally:
        for p in procs:
            p.join(60 if len(res) == 2 else 5)
            if p.is_alive():
                p.kill()
                p.join(10)
    assert all(p.exitcode == 0 for p in procs) and len(res) == 2, [p.exitcode for p in procs]
    assert res[0][0] == res[1][0] and np.isfinite(res[0][0]).all(), (backend, res[0][0], res[1][0])
    for k, name in ((1, "group_stats"), (2, "lr_weights"), (3, "flat_param")):
        assert res[0][k] == res[1][k], (backend, name)
    stat = np.frombuffer(res[0][1], np.float32)
    assert stat.shape == (22,) and (stat > 0).all()
