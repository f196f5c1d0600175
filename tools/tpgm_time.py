#!/usr/bin/env python3
"""Time optim.FlatTPGM (csrc/tpgm.hip) at the layout of the full model (depth [1, 2, 9, 1]: 463 tensors, 23 568 492 parameters)
against the per-tensor torch loop restated from the formulas of DESIGN.md, "TPGM", on the same device; record both in
profiles/tpgm_timing.txt.

    python tools/tpgm_time.py [--out FILE] [--repeats 30]

Three operations, each on both sides:
    begin              save theta, project into the parameters          | torch: clone every parameter, then the projection loop
    update + reproject dL/dgamma, clip, Adam on gamma, project again    | torch: per-tensor dot and norm, clip_grad_norm_ + Adam on 463
                                                                          scalar parameters, then the projection loop
    apply              the final projection, in place                   | torch: the projection loop in place
The torch projection loop is the reference's shape: per tensor a subtraction, a norm, one .item() host read for the clamp, the
ratio, and a copy.  The parameters sit 0.01 N(0, 1) off the anchor with the radii at half the norms, so every tensor is projected.
One process; after a warm-up every repetition times one device-event window per case, the cases in turn, each window ended by
a synchronise; what a case needs restored (the parameters before an apply) is restored outside its window.  Clocks are left as found."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tpgm_timing.txt"))
    ap.add_argument("--repeats", type=int, default=30)
    a = ap.parse_args()
    import torch
    from cswin_unet_amd import _lib
    from cswin_unet_amd.networks.cswin_unet import CSWinTransformer
    from cswin_unet_amd.optim import FlatAdamW, FlatTPGM, tpgm_is_head
    assert torch.cuda.is_available() and _lib.lib().cswin_device_ok() == 1, "needs a gfx950 HIP device"
    dev = "cuda"
    net = CSWinTransformer(img_size=224, num_classes=9, embed_dim=64, depth=[1, 2, 9, 1], split_size=[1, 2, 7, 7], num_heads=[2, 4, 8, 16],
                           qkv_bias=True, drop_path_rate=0.)
    names = [n for n, _ in net.named_parameters()]
    shapes = [tuple(p.shape) for p in net.parameters()]
    nparam = sum(p.numel() for p in net.parameters())
    assert len(shapes) == 463 and nparam == 23568492, (len(shapes), nparam)
    gen = torch.Generator().manual_seed(2026)
    anchors = [0.02 * torch.randn(s, generator=gen) for s in shapes]
    moved = [v + 0.01 * torch.randn(s, generator=gen) for v, s in zip(anchors, shapes)]
    grads = [torch.randn(s, generator=gen) for s in shapes]

    # ours: the anchor is taken at construction, then the parameters move
    ours = [torch.nn.Parameter(v.clone().to(dev)) for v in anchors]
    opt = FlatAdamW(ours, lr=1e-4)
    tpgm = FlatTPGM(opt, names, proj_lr=0.01)
    with torch.no_grad():
        for p, v in zip(ours, moved):
            p.copy_(v.to(dev))
    for p, g in zip(ours, grads):
        p.grad = g.to(dev)
    opt.gather_grads()
    opt.zero_grad()
    half = 0.5 * tpgm.tensor_norms()
    tpgm.set_constraints(half)
    theta0 = opt.flat_param.clone()

    # torch: the same values as separate tensors
    heads = [tpgm_is_head(n) for n in names]
    t_anchor = [v.to(dev) for v in anchors]
    t_param = [v.clone().to(dev) for v in moved]
    t_moved = [v.to(dev) for v in moved]
    t_grad = [g.to(dev) for g in grads]
    t_gamma = [torch.nn.Parameter(h.reshape(1).clone()) for h in half]
    t_adam = torch.optim.Adam(t_gamma, lr=0.01)
    hardtanh = torch.nn.Hardtanh(0, 1)

    def torch_project(src, dst):
        with torch.no_grad():
            for s, d, anc, gam, head in zip(src, dst, t_anchor, t_gamma, heads):
                t = s - anc
                norm = torch.norm(t)
                cmax = max(norm.item() * 10, 100.0) if head else max(norm.item() * 8, 80.0)
                ratio = hardtanh(torch.clamp(gam, min=1e-2, max=cmax) / (norm + 1e-8))
                d.copy_(t * ratio + anc)

    saved = {}

    def torch_begin():
        saved["theta"] = [p.clone() for p in t_param]
        torch_project(saved["theta"], t_param)

    def torch_update_reproject():
        for s, anc, g, gam, head in zip(t_moved, t_anchor, t_grad, t_gamma, heads):
            t = s - anc
            norm = torch.norm(t)
            cmax = max(norm.item() * 10, 100.0) if head else max(norm.item() * 8, 80.0)
            q = torch.clamp(gam.detach(), min=1e-2, max=cmax) / (norm + 1e-8)
            live = (gam.detach() >= 1e-2) & (gam.detach() <= cmax) & (q > 0) & (q < 1)
            gam.grad = torch.where(live, (g * t).sum() / (norm + 1e-8), torch.zeros_like(q))
        torch.nn.utils.clip_grad_norm_(t_gamma, 1.0)
        t_adam.step()
        torch_project(t_moved, t_param)

    def torch_apply():
        torch_project(t_param, t_param)

    def ours_begin():
        tpgm.begin()

    def ours_update_reproject():
        tpgm.update(1.0)
        tpgm.reproject()

    def restore_ours():
        tpgm.end()
        opt.flat_param.copy_(theta0)
        tpgm.set_constraints(half)

    def restore_torch():
        with torch.no_grad():
            for p, v, gam, h in zip(t_param, t_moved, t_gamma, half):
                p.copy_(v)
                gam.fill_(float(h))

    def begun():
        restore_ours()
        tpgm.begin()

    # (name, preparation outside the window, the timed call)
    cases = [("FlatTPGM.begin (copy + chunk_stats + finalize + project)", restore_ours, ours_begin),
             ("torch: clone every parameter + per-tensor projection loop", restore_torch, torch_begin),
             ("FlatTPGM.update + reproject (chunk_stats + finalize + project)", begun, ours_update_reproject),
             ("torch: per-tensor dots, clip_grad_norm_ + Adam on 463 radii, projection loop", restore_torch, torch_update_reproject),
             ("FlatTPGM.apply (chunk_stats + finalize + project in place)", restore_ours, tpgm.apply),
             ("torch: per-tensor projection loop in place", restore_torch, torch_apply)]
    for _, prep, fn in cases:
        for _ in range(3):
            prep()
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in cases]
    for _ in range(a.repeats):
        for t, (_, prep, fn) in zip(times, cases):
            prep()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            t.append(e0.elapsed_time(e1))
    restore_ours()
    med = [statistics.median(t) for t in times]
    lines = [f"TPGM timing: {len(shapes)} tensors, {nparam} parameters ({opt.numel} floats with the slots' pad words, {tpgm.nchunks} chunks), "
             f"{torch.cuda.get_device_name(0)}, torch {torch.__version__}",
             f"one process, 3 warm-up calls each, then {a.repeats} repetitions of one device-event window of ONE call per case, the cases in turn; "
             f"median per call (min, max); clocks as found",
             "parameters 0.01 N(0, 1) off the anchor, radii at half the norms: every tensor is projected; the torch loops are restated from the "
             "formulas (one .item() host read per tensor, as the reference has it), and a device-event window around them includes the time the "
             "device waits for the host"]
    for (what, _, _), t, m in zip(cases, times, med):
        lines.append(f"  {what}: {m:.4f} ms (min {min(t):.4f}, max {max(t):.4f})")
    for k, what in ((0, "begin"), (2, "update + reproject"), (4, "apply")):
        lines.append(f"measured quotient, {what}: torch loop / ours = {med[k + 1] / med[k]:.1f}x at the medians above (this window, this device; nothing beyond it is claimed)")
    gb = opt.numel * 4 / 1e9
    lines.append(f"ours moves, per element: begin 28 B, update + reproject 24 B, apply 20 B at most = {7 * gb:.2f} / {6 * gb:.2f} / {5 * gb:.2f} GB; "
                 f"at the medians {7 * gb / med[0]:.2f} / {6 * gb / med[2]:.2f} / {5 * gb / med[4]:.2f} TB/s; the buffers of one call (0.3 GB) may stay "
                 f"in the last-level cache between calls")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
