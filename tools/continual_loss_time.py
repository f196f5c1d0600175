#!/usr/bin/env python3
"""Time the fused continual-learning objective (ops.continual_loss, csrc/cl_loss.hip) against the same objective composed from
torch ops on the same device, and the training step with and without the `distill` option; record it in
profiles/continual_loss_timing.txt.

    python tools/continual_loss_time.py [--out FILE] [--repeats 30]

Every measurement runs in a fresh child process (this script with --child NAME), so no allocator state, captured graph or warmed
cache of one carries into the next; the child warms up, then takes the median of --repeats device-event windows of CALLS calls
each (a single call of the fused op is about 0.2 ms, too short a window), divided by CALLS and each ended by a synchronise; clocks
are left as found.  Every call reads the same tensors (about 110 MB for the objective), so they may stay cache-resident.  A child that fails ends the run: nothing further is started and nothing is written.

  fused / torch: forward + backward of the objective at B 24, 224 x 224, 12 classes, 9 old ones, class weights and the label map
  given; fused_powf is the fused op at gamma 2.5, which takes the powf path instead of repeated products.  fused_base is ops.ce_dice_loss
  (the base objective, csrc/loss.hip) on the same labels at 9 classes, windowed the same way.  The torch composition is universal_train.py:904-932 with one-hot Dice sums taken over all classes at once (kinder to
  torch than the reference's per-class loop); the two losses must agree to 1e-4 relative or the run fails.
  step / step_distill / teacher: the configuration of tests/test_gpu_continual_step.py (depth [1, 1, 1, 1], B 2, hipGraphs):
  train_step on the 9-class model without the option, on the 12-class student with it, and the teacher's forward alone."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, HW, NCLS, NOLD, TEMP, GAMMA = 24, 224, 12, 9, 3.0, 4.0
CHILDREN = ("fused", "fused_powf", "fused_base", "torch", "step", "step_distill", "teacher")
BASE_NCLS = 9
CALLS = 20


def device_ms(fn, repeats, warmup=5):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(CALLS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / CALLS)
    return statistics.median(times), min(times), max(times)


def torch_objective(logits, labels, teacher, cw, lmap):
    import torch
    import torch.nn.functional as F
    lab = lmap.long()[labels]
    ce = F.cross_entropy(logits, lab, weight=cw, reduction='none')
    pt = torch.exp(-ce)
    focal = ((1 - pt) ** GAMMA * ce).mean()
    p = torch.softmax(logits, 1)
    oh = F.one_hot(lab, NCLS).permute(0, 3, 1, 2).float()
    inter, y, z = (p * oh).sum((0, 2, 3)), (oh * oh).sum((0, 2, 3)), (p * p).sum((0, 2, 3))
    dice = (1 - (2 * inter + 1e-5) / (z + y + 1e-5)).sum() / NCLS
    kd = F.kl_div(F.log_softmax(logits[:, :NOLD] / TEMP, dim=1), F.softmax(teacher / TEMP, dim=1), reduction='batchmean') * TEMP ** 2
    return 0.5 * (0.2 * focal + 0.8 * dice) + 0.5 * kd


def child(name, repeats):
    import torch
    from cswin_unet_amd import _lib, ops
    from cswin_unet_amd.continual import Distill, expand_classes, extreme_class_weights, freeze_teacher, new_label_map
    assert torch.cuda.is_available() and _lib.lib().cswin_device_ok() == 1, "needs a gfx950 HIP device"
    dev = "cuda"
    res = {"name": name, "device": torch.cuda.get_device_name(0)}
    lmap = new_label_map(NOLD, NCLS - NOLD + 1, dev)
    cw = extreme_class_weights([9.0e5] + [0.0] * (NOLD - 1) + [4.0e4, 2.5e4, 9.0e3], [0, 9, 10, 11]).to(dev)
    if name in ("fused", "fused_powf", "fused_base", "torch"):
        g = torch.Generator().manual_seed(2025)
        logits = (2.0 * torch.randn(B, BASE_NCLS if name == "fused_base" else NCLS, HW, HW, generator=g)).to(dev).requires_grad_()
        teacher = (2.0 * torch.randn(B, NOLD, HW, HW, generator=g)).to(dev)
        labels = torch.randint(0, NCLS - NOLD + 1, (B, HW, HW), generator=g).to(dev)
        if name == "fused_base":
            f = lambda: ops.ce_dice_loss(logits, labels)[0]
        elif name != "torch":
            gamma = GAMMA if name == "fused" else 2.5
            f = lambda: ops.continual_loss(logits, labels, teacher, focal_gamma=gamma, class_weight=cw, label_map=lmap)[0]
        else:
            f = lambda: torch_objective(logits, labels, teacher, cw, lmap)

        def fwd_bwd():
            logits.grad = None
            f().backward()

        res["loss"] = float(f())
        res["ms"] = device_ms(fwd_bwd, repeats)
        res["peak_MiB"] = torch.cuda.max_memory_allocated() / 2 ** 20
    else:
        from cswin_unet_amd.networks.cswin_unet import CSWinTransformer
        from cswin_unet_amd.trainer import DataParallelTrainer, synthetic_batch
        from oracle.determ import fill_state_dict
        net = fill_state_dict(CSWinTransformer(img_size=224, num_classes=NOLD, embed_dim=64, depth=[1, 1, 1, 1], split_size=[1, 2, 7, 7],
                                               num_heads=[2, 4, 8, 16], qkv_bias=True, drop_path_rate=0.).to(dev)).train()
        img, _ = synthetic_batch(2, 224, NOLD, 7, dev)
        img = img.repeat(1, 3, 1, 1)
        if name == "teacher":
            teacher = freeze_teacher(net)

            def fwd():
                with torch.no_grad():
                    teacher(img)
            res["ms"] = device_ms(fwd, repeats)
        else:
            distill = None
            ncls = NOLD
            if name == "step_distill":
                teacher = freeze_teacher(net)
                torch.manual_seed(1)
                expand_classes(net, NCLS - NOLD + 1)
                distill, ncls = Distill(teacher=teacher, class_weight=cw, label_map=lmap), NCLS
            _, lab = synthetic_batch(2, 224, NCLS - NOLD + 1 if distill else NOLD, 7, dev)
            tr = DataParallelTrainer(net, ncls, base_lr=1e-6, max_iterations=10000, use_graph=True, distill=distill)
            res["ms"] = device_ms(lambda: tr.train_step(img, lab), repeats)
            res["loss"] = float(tr.stats[0])
    print("RESULT " + json.dumps(res), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "continual_loss_timing.txt"))
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--child", choices=CHILDREN)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.repeats)
    got = {}
    for name in CHILDREN:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--repeats", str(a.repeats)], capture_output=True, text=True, timeout=180)
        line = next((ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")), None)
        if p.returncode != 0 or line is None:
            print(p.stdout[-2000:], p.stderr[-4000:], f"child {name} failed ({p.returncode}); nothing written", sep="\n")
            return 1
        got[name] = json.loads(line[7:])
        print(name, got[name], flush=True)
    fu, to = got["fused"], got["torch"]
    agree = abs(fu["loss"] - to["loss"]) <= 1e-4 * abs(to["loss"])
    ms = lambda r: f"{r['ms'][0]:.3f} ms (min {r['ms'][1]:.3f}, max {r['ms'][2]:.3f})"
    st, sd, te, fp = got["step"], got["step_distill"], got["teacher"], got["fused_powf"]
    lines = [f"continual loss timing: B {B}, {HW} x {HW}, ncls {NCLS}, nold {NOLD}, T {TEMP}, gamma {GAMMA}, class weights and label map given, {fu['device']}",
             f"each line: a fresh process, 5 warm-up calls, median of {a.repeats} device-event windows of {CALLS} calls each (per call), clocks as found",
             "every call reads the same tensors (about 110 MB for the objective): they may stay cache-resident",
             f"loss fused {fu['loss']:.7f} | torch {to['loss']:.7f}: {'agree' if agree else 'DISAGREE'} (1e-4 relative)",
             f"forward + backward, ops.continual_loss (3 launches forward, 1 backward): {ms(fu)}, peak memory {fu['peak_MiB']:.0f} MiB",
             f"forward + backward, the same objective from torch ops (one-hot, two softmaxes, autograd): {ms(to)}, peak memory {to['peak_MiB']:.0f} MiB",
             f"forward + backward, ops.continual_loss at gamma 2.5 (powf instead of repeated products): {ms(fp)}",
             f"forward + backward, ops.ce_dice_loss (the base objective, csrc/loss.hip) at {BASE_NCLS} classes: {ms(got['fused_base'])}",
             f"torch / fused: {to['ms'][0] / fu['ms'][0]:.2f}x" +("" if to['ms'][0] > fu['ms'][0] else "  (the fused path is NOT faster)"),
             "training step, depth [1, 1, 1, 1], B 2, 224 x 224, hipGraphs (the configuration of tests/test_gpu_continual_step.py):",
             f"  without distill (9 classes): {ms(st)}",
             f"  with distill (12 classes, 9-class teacher): {ms(sd)}",
             f"  teacher forward alone (eager, no_grad): {ms(te)}",
             f"  difference {sd['ms'][0] - st['ms'][0]:.3f} ms against a teacher forward of {te['ms'][0]:.3f} ms eager (inside the step it is replayed from graph A)"]
    text = "\n".join(lines) + "\n"
    print(text)
    if not agree:
        print("FAILED: the two losses disagree; nothing written")
        return 1
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
