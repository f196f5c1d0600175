#!/usr/bin/env python3
"""Time the per-step-rate modes of FlatAdamW.apply (csrc/adamw.hip: cswin_rate_finalize, cswin_adam_flat) against the default
apply with clipping, at the layout of the full model (depth [1, 2, 9, 1]: 463 tensors, 23 568 492 parameters), by the method of
tools/adamw_time.py; record it in profiles/auto_rates_timing.txt.

    python tools/auto_rates_time.py [--out FILE] [--repeats 50]

One process holds four optimisers on four copies of the parameters with the same gradient, all with max_grad_norm=1 and lr 1e-6
(the weights barely move over the run, so every window finds the same kind of input):

    default      FlatAdamW(...).apply: chunk_sumsq + norm_finalize + adamw_flat, the calls the step made before the rates existed
    grad/kept    decoupled=False, set_auto_rates(the 22 groups of continual.finetune_groups): chunk_sumsq + rate_finalize + adam_flat
    ratio/kept   decoupled=False, set_auto_rates(one group per tensor, "ratio"): the norm pass reads the parameters as well
    grad/fresh   as grad/kept with moments="fresh": the update neither reads nor writes m and v

After a warm-up every repetition times one device-event window of CALLS updates of each, in turn, each window ended by a
synchronise; the medians are per update; clocks are left as found.  Nothing is gated: the file says whether grad/kept, which
launches three kernels over the same bytes as the default, lies within the default's own spread (max - min of its repetitions)."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CALLS = 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "auto_rates_timing.txt"))
    ap.add_argument("--repeats", type=int, default=50)
    a = ap.parse_args()
    import torch
    from cswin_unet_amd import _lib
    from cswin_unet_amd.continual import finetune_groups
    from cswin_unet_amd.networks.cswin_unet import CSWinTransformer
    from cswin_unet_amd.optim import FlatAdamW
    assert torch.cuda.is_available() and _lib.lib().cswin_device_ok() == 1, "needs a gfx950 HIP device"
    dev = "cuda"
    net = CSWinTransformer(img_size=224, num_classes=9, embed_dim=64, depth=[1, 2, 9, 1], split_size=[1, 2, 7, 7], num_heads=[2, 4, 8, 16],
                           qkv_bias=True, drop_path_rate=0.)
    names = [n for n, _ in net.named_parameters()]
    shapes = [tuple(p.shape) for p in net.parameters()]
    nparam = sum(p.numel() for p in net.parameters())
    assert len(shapes) == 463 and nparam == 23568492, (len(shapes), nparam)
    where = {n: g for g, members in finetune_groups(net).items() for n in members}
    by_group = [where[n] for n in names]
    gen = torch.Generator().manual_seed(2026)
    values = [0.02 * torch.randn(s, generator=gen) for s in shapes]
    grads = [torch.randn(s, generator=gen) for s in shapes]           # global norm ~ 4855: the clip is live
    specs = [("default: FlatAdamW.apply, max_grad_norm=1 (chunk_sumsq + norm_finalize + adamw_flat)", {}, None, 28 + 4),
             ("grad/kept: 22 groups (chunk_sumsq + rate_finalize + adam_flat, coupled)", dict(decoupled=False), (by_group, "grad"), 28 + 4),
             ("ratio/kept: 463 groups (chunk_sumsq with p + rate_finalize + adam_flat, coupled)", dict(decoupled=False), (list(range(463)), "ratio"), 28 + 8),
             ("grad/fresh: 22 groups (chunk_sumsq + rate_finalize + adam_flat, coupled, fresh moments)", dict(decoupled=False, moments="fresh"),
              (by_group, "grad"), 12 + 4)]
    cases = []
    for what, kw, auto, nbytes in specs:
        params = [torch.nn.Parameter(v.clone().to(dev)) for v in values]
        opt = FlatAdamW(params, lr=1e-6, weight_decay=0.01, max_grad_norm=1.0, **kw)
        if auto is not None:
            opt.set_auto_rates(*auto)
        for p, g in zip(params, grads):
            p.grad = g.to(dev)
        opt.gather_grads()
        opt.zero_grad()
        cases.append((what, opt, nbytes))
    for _, opt, _ in cases:
        for _ in range(5):
            opt.apply(1.0)
    torch.cuda.synchronize()
    times = [[] for _ in cases]
    for _ in range(a.repeats):
        for t, (_, opt, _) in zip(times, cases):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(CALLS):
                opt.apply(1.0)
            e1.record()
            torch.cuda.synchronize()
            t.append(e0.elapsed_time(e1) / CALLS)
    med = [statistics.median(t) for t in times]
    numel, nchunks = cases[0][1].numel, cases[0][1].nchunks
    lines = [f"Per-step rates timing: {len(shapes)} tensors, {nparam} parameters ({numel} floats with the slots' pad words, {nchunks} chunks), "
             f"{torch.cuda.get_device_name(0)}, torch {torch.__version__}",
             f"one process, 5 warm-up updates each, then {a.repeats} repetitions of one device-event window of {CALLS} updates per case, the cases in turn; "
             f"median per update (min, max); clocks as found",
             "fp32 mode (no bf16 shadow); every case clips (the gradient norm is far above 1) and has three launches; bytes per element: the update's "
             "reads and writes plus the norm pass's reads"]
    for (what, _, nbytes), t, m in zip(cases, times, med):
        lines.append(f"  {what}: {m:.4f} ms (min {min(t):.4f}, max {max(t):.4f}); {nbytes} B / element = {numel * nbytes / 1e9:.2f} GB, "
                     f"{numel * nbytes / 1e9 / m:.2f} TB/s at the median")
    lines.append("every update of a case touches the same buffers: part of them may stay in the last-level cache between updates")
    spread = max(times[0]) - min(times[0])
    diff = med[1] - med[0]
    lines.append(f"grad/kept against the default (same three launches, same 32 B / element): median {diff:+.4f} ms; the default's own spread (max - min of its "
                 f"repetitions) is {spread:.4f} ms: {'within' if abs(diff) <= spread else 'NOT within'} it")
    lines.append(f"ratio/kept / default = {med[2] / med[0]:.2f}x; grad/fresh / default = {med[3] / med[0]:.2f}x")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
