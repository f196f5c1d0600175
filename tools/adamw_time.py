#!/usr/bin/env python3
"""Time FlatAdamW.apply with clipping (csrc/adamw.hip: three launches) against torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW
on the same device and, for scale, against FlatSGD.apply, at the layout of the full model (depth [1, 2, 9, 1]: 463 tensors,
23 568 492 parameters); record it in profiles/adamw_timing.txt.

    python tools/adamw_time.py [--out FILE] [--repeats 50]

One process holds the three optimisers on three copies of the parameters with the same gradients.  After a warm-up every
repetition times one device-event window of CALLS updates of each of the three, in turn, each window ended by a synchronise;
the medians are per update; clocks are left as found.  torch.optim.AdamW runs fused if this torch offers it on the device, foreach
otherwise, and the file says which.  The condition recorded is that ours is not slower than the torch pair.

    python tools/adamw_time.py --eb [--out FILE] [--repeats 20]

times, on the same layout and gradient, FlatAdamW.tensor_evidence() (csrc/eb.hip: two launches, no host read) against the
reference's eb-criterion loop (universal_train.py:669-672: torch.var, mul, add, div, mean and .item() per tensor, over the 349
tensors whose names hold neither "bn" nor "norm", as views of the same flat gradient) and records it in
profiles/eb_criterion_timing.txt.  The loop is the yardstick; nothing is gated on the ratio."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CALLS = 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--eb", action="store_true", help="time tensor_evidence() against the reference's per-tensor loop instead")
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=None)
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, "profiles", "eb_criterion_timing.txt" if a.eb else "adamw_timing.txt")
    a.repeats = a.repeats or (20 if a.eb else 50)
    import torch
    from cswin_unet_amd import _lib
    from cswin_unet_amd.networks.cswin_unet import CSWinTransformer
    from cswin_unet_amd.optim import FlatAdamW, FlatSGD
    assert torch.cuda.is_available() and _lib.lib().cswin_device_ok() == 1, "needs a gfx950 HIP device"
    dev = "cuda"
    net = CSWinTransformer(img_size=224, num_classes=9, embed_dim=64, depth=[1, 2, 9, 1], split_size=[1, 2, 7, 7], num_heads=[2, 4, 8, 16],
                           qkv_bias=True, drop_path_rate=0.)
    shapes = [tuple(p.shape) for p in net.parameters()]
    nparam = sum(p.numel() for p in net.parameters())
    assert len(shapes) == 463 and nparam == 23568492, (len(shapes), nparam)
    gen = torch.Generator().manual_seed(2026)
    values = [0.02 * torch.randn(s, generator=gen) for s in shapes]
    grads = [torch.randn(s, generator=gen) for s in shapes]           # global norm ~ 4855: the clip is live
    copies = lambda: [torch.nn.Parameter(v.clone().to(dev)) for v in values]
    ours, sgd, theirs = copies(), copies(), copies()
    adamw = FlatAdamW(ours, lr=1e-4, weight_decay=0.01, max_grad_norm=1.0)
    flat_sgd = FlatSGD(sgd, lr=1e-4)
    for opt, params in ((adamw, ours), (flat_sgd, sgd)):
        for p, g in zip(params, grads):
            p.grad = g.to(dev)
        opt.gather_grads()
        opt.zero_grad()
    if a.eb:
        return eb_main(a, torch, net, adamw, nparam)
    for p, g in zip(theirs, grads):
        p.grad = g.to(dev)
    try:
        torch_opt, variant = torch.optim.AdamW(theirs, lr=1e-4, weight_decay=0.01, fused=True), "fused"
        torch_opt.step()
    except (RuntimeError, TypeError, ValueError) as e:
        print("fused AdamW is not available:", e)
        torch_opt, variant = torch.optim.AdamW(theirs, lr=1e-4, weight_decay=0.01, foreach=True), "foreach"

    def torch_pair():
        # the gradients are rescaled in place, so a second clip in the same window finds a norm of 1: the launches are the same
        torch.nn.utils.clip_grad_norm_(theirs, 1.0)
        torch_opt.step()

    cases = [("FlatAdamW.apply, max_grad_norm=1 (chunk_sumsq + norm_finalize + adamw_flat)", lambda: adamw.apply(1.0)),
             (f"clip_grad_norm_ + torch.optim.AdamW({variant}=True)", torch_pair),
             ("FlatSGD.apply (sgd_flat)", lambda: flat_sgd.apply(1.0))]
    for _, fn in cases:
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in cases]
    for _ in range(a.repeats):
        for t, (_, fn) in zip(times, cases):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(CALLS):
                fn()
            e1.record()
            torch.cuda.synchronize()
            t.append(e0.elapsed_time(e1) / CALLS)
    med = [statistics.median(t) for t in times]
    lines = [f"AdamW update timing: {len(shapes)} tensors, {nparam} parameters ({adamw.numel} floats with the slots' pad words, {adamw.nchunks} chunks), "
             f"{torch.cuda.get_device_name(0)}, torch {torch.__version__}",
             f"one process, 5 warm-up updates each, then {a.repeats} repetitions of one device-event window of {CALLS} updates per case, the cases in turn; "
             f"median per update (min, max); clocks as found",
             "the gradient norm is far above 1, so the clip is live in ours; torch's second and later clips find an already clipped gradient (same launches)"]
    for (what, _), t, m in zip(cases, times, med):
        lines.append(f"  {what}: {m:.4f} ms (min {min(t):.4f}, max {max(t):.4f})")
    gbytes = adamw.numel * 32 / 1e9
    lines.append(f"ours moves 32 B / element in the fp32 mode (no bf16 shadow): the update reads p, g, m, v and writes p, m, v (28 B), the norm pass reads g (4 B) = "
                 f"{gbytes:.2f} GB per update: {gbytes / med[0]:.2f} TB/s at the median")
    lines.append("every update of a case touches the same buffers (about 0.4 GB for ours): part of them may stay in the last-level cache between updates")
    ok = med[0] <= med[1]
    lines.append(f"condition (ours not slower than the torch pair): {'met' if ok else 'NOT MET'}: torch pair / ours = {med[1] / med[0]:.2f}x; ours / FlatSGD.apply = {med[0] / med[2]:.2f}x")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text)
    return 0


def eb_main(a, torch, net, adamw, nparam):
    """The --eb mode: adamw.flat_grad holds the gathered N(0, 1) gradient."""
    names = [n for n, _ in net.named_parameters()]
    views = [adamw.flat_grad[o:o + p.numel()].view(p.shape) for n, p, o in zip(names, adamw.params, adamw.offsets)
             if "bn" not in n.lower() and "norm" not in n.lower()]
    assert len(views) == 349, len(views)

    def ours():
        return adamw.tensor_evidence()

    def loop():
        out = []
        for g in views:
            grad_var = torch.var(g, dim=0, keepdim=True)
            tmp = (g * g) / (grad_var + 1e-8)
            out.append(tmp.mean().item())
        return out

    cases = [("FlatAdamW.tensor_evidence() (eb_tiles + eb_finalize, all 463 tensors, no host read)", ours),
             ("the reference's loop (torch.var, mul, add, div, mean, .item() per tensor; 349 tensors)", loop)]
    for _, fn in cases:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    kept = [i for i, n in enumerate(names) if "bn" not in n.lower() and "norm" not in n.lower()]
    got, want = ours().cpu()[kept].double(), torch.tensor(loop(), dtype=torch.float64)
    agree = float(((got - want).abs() / want.abs().clamp_min(1e-30)).max())
    times = [[] for _ in cases]
    for _ in range(a.repeats):
        for t, (_, fn) in zip(times, cases):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(CALLS):
                fn()
            e1.record()
            torch.cuda.synchronize()
            t.append(e0.elapsed_time(e1) / CALLS)
    med = [statistics.median(t) for t in times]
    ntiles = adamw._eb[1]
    lines = [f"eb-criterion timing: {len(adamw.params)} tensors, {nparam} parameters ({adamw.numel} floats with the slots' pad words, {ntiles} column tiles), "
             f"{torch.cuda.get_device_name(0)}, torch {torch.__version__}",
             f"one process, 3 warm-up calls each, then {a.repeats} repetitions of one device-event window of {CALLS} calls per case, the cases in turn; "
             f"median per call (min, max); clocks as found",
             f"both read the same flat gradient (N(0, 1)); largest relative difference of the 349 statistics: {agree:.2e}"]
    for (what, _), t, m in zip(cases, times, med):
        lines.append(f"  {what}: {m:.4f} ms (min {min(t):.4f}, max {max(t):.4f})")
    gbytes = nparam * 4 / 1e9
    lines.append(f"ours reads every gradient element once ({gbytes:.3f} GB): {gbytes / med[0]:.2f} TB/s at the median; every call reads the same buffer, "
                 f"which may stay in the last-level cache between calls")
    lines.append(f"the loop / ours = {med[1] / med[0]:.1f}x" + ("" if med[0] <= med[1] else "  (ours is SLOWER than the loop)"))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
