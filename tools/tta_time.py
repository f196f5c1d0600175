#!/usr/bin/env python3
"""Time the test-time-augmentation kernels (csrc/tta.hip: ops.view_batch, ops.tta_argmax_zoom_back) alone and inside
utils.predict_volume(resize="hip", tta=...), and record it in profiles/tta_timing.txt.

    python tools/tta_time.py [--out FILE] [--repeats 10] [--calls 20]

Kernels: (V, B, ncls, h -> H) = (8, 2, 9, 224 -> 512) and (4, 4, 9, 224 -> 512), resident seeded tensors.  One launch of either
takes tens of microseconds, so a timed window is --calls launches between two device synchronisations, divided by --calls; the
median of --repeats windows after a warm-up window.  Beside each time the bytes the kernel must move -- view_batch reads
B h w 4 and writes V B h w 4; the ensemble reads V B nsel h w 4 and writes B H W -- and that traffic over the time against the
8.0 TB/s HBM peak and the 6.29 TB/s a float4 copy reaches (the figures of tools/gaussian_blur_time.py).  At these sizes the
logits (29 and 58 MB) fit the 256 MiB Infinity Cache, so a rate above HBM's is a cache rate, and is named so.

Whole volume: predict_volume(resize="hip") on the seeded 148 x 512 x 512 volume of tools/predict_volume_time.py with tta None,
"flips" and "d4", median of --repeats after a warm-up; the parts of a tta run alone on resident tensors, a whole volume's worth
of batches per repeat (the network on V b samples, view_batch, the ensemble); the floor V x (the single-view network time) and
what the two kernels add over it.  Run it under `timeout`; an exception ends the run, so nothing is enqueued after a failed step."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPE, PATCH, NCLS, BATCH = (148, 512, 512), (224, 224), 9, 16
KERNEL_CASES = [(8, 2), (4, 4)]
HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12


def timed_ms(fn, repeats, warmup=1):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), min(times), max(times)


def fmt(t, scale=1.0, unit="ms"):
    return f"{t[0] * scale:.2f} {unit} (min {t[1] * scale:.2f}, max {t[2] * scale:.2f})"


def rate(nbytes, t_ms):
    r = nbytes / (t_ms * 1e-3)
    return f"{nbytes / 1e6:.1f} MB, {r / 1e12:.2f} TB/s = {100 * r / HBM_PEAK:.0f} % of the 8.0 TB/s peak, {100 * r / HBM_COPY:.0f} % of a copy's 6.29 TB/s"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tta_timing.txt"))
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()

    from cswin_unet_amd import _lib, ops
    from cswin_unet_amd.networks.cswin_unet import CSWinTransformer
    from cswin_unet_amd.utils import predict_volume, tta_views
    from oracle.determ import det_normal, fill_state_dict
    assert torch.cuda.is_available() and _lib.lib().cswin_device_ok() == 1, "needs a gfx950 HIP device"

    lines = [f"test-time augmentation timing, {torch.cuda.get_device_name(0)}",
             f"kernels alone, resident tensors, {a.calls} launches per window, per launch, median of {a.repeats} windows:"]
    h, w = PATCH
    for V, B in KERNEL_CASES:
        views = tta_views("d4")[:V] if V == 8 else tta_views("flips")
        x = torch.from_numpy(det_normal("tta_time.x", (B, h, w))).cuda()
        logits = torch.from_numpy(3.0 * det_normal("tta_time.logits", (V * B, NCLS, h, w))).cuda()
        t_view = timed_ms(lambda: [ops.view_batch(x, views) for _ in range(a.calls)], a.repeats)
        t_ens = timed_ms(lambda: [ops.tta_argmax_zoom_back(logits, views, SHAPE[1:]) for _ in range(a.calls)], a.repeats)
        t_prob = timed_ms(lambda: [ops.tta_argmax_zoom_back(logits, views, SHAPE[1:], return_probs=True) for _ in range(a.calls)], a.repeats)
        t_arg = timed_ms(lambda: [ops.argmax_zoom_back(logits[:B], SHAPE[1:]) for _ in range(a.calls)], a.repeats)
        us = 1e3 / a.calls
        lines += [f"  (V, B, ncls, h -> H) = ({V}, {B}, {NCLS}, {h} -> {SHAPE[1]}), views {views}:",
                  f"    ops.view_batch: {fmt(t_view, us, 'us')}; {rate((1 + V) * B * h * w * 4, t_view[0] / a.calls)}",
                  f"    ops.tta_argmax_zoom_back: {fmt(t_ens, us, 'us')}; "
                  f"{rate(V * B * NCLS * h * w * 4 + B * SHAPE[1] * SHAPE[2], t_ens[0] / a.calls)}",
                  f"    ops.tta_argmax_zoom_back(return_probs=True) (+ {B * NCLS * h * w * 4 / 1e6:.1f} MB written): {fmt(t_prob, us, 'us')}",
                  f"    ops.argmax_zoom_back on one view's {B} slices, for scale: {fmt(t_arg, us, 'us')}"]
        print("\n".join(lines[-5:]), flush=True)
        del x, logits

    class OneChannel(torch.nn.Module):
        def __init__(self, m):
            super().__init__()
            self.m = m

        def forward(self, x):
            return self.m(x.repeat(1, 3, 1, 1))

    net = CSWinTransformer(img_size=PATCH[0], num_classes=NCLS, embed_dim=64, depth=[1, 2, 9, 1], split_size=[1, 2, 7, 7],
                           num_heads=[2, 4, 8, 16], qkv_bias=True, drop_path_rate=0.).cuda()
    net = OneChannel(fill_state_dict(net)).eval()
    vol = det_normal("predict_volume_time.vol", SHAPE)
    dvol = torch.from_numpy(vol).cuda()
    D = SHAPE[0]
    lines.append(f"predict_volume(resize=\"hip\"), seeded float32 volume {D} x {SHAPE[1]} x {SHAPE[2]} -> {h} x {w}, tiny network, {NCLS} classes, "
                 f"batch_slices {BATCH}, median of {a.repeats} (profiles/predict_volume_timing.txt has the single-view time of the commit before "
                 f"the ensemble: 50.81 ms, network 40.57 ms):")
    whole, preds = {}, {}
    for spec in (None, "flips", "d4"):
        preds[spec] = predict_volume(vol, net, PATCH, BATCH, resize="hip", tta=spec)
        whole[spec] = timed_ms(lambda: predict_volume(vol, net, PATCH, BATCH, resize="hip", tta=spec), a.repeats, warmup=0)
        print(f"predict_volume tta={spec}: {fmt(whole[spec])}", flush=True)
    with torch.no_grad():
        single = [ops.resize_slices(dvol[d:d + BATCH], PATCH) for d in range(0, D, BATCH)]
        t_net1 = timed_ms(lambda: [net(s.unsqueeze(1)) for s in single], a.repeats)
        del single
        lines.append(f"  tta=None: {fmt(whole[None])}; its network calls alone ({-(-D // BATCH)} batches of {BATCH}): {fmt(t_net1)}")
        for spec in ("flips", "d4"):
            views = tta_views(spec)
            V, b = len(views), max(1, BATCH // len(views))
            small = [ops.resize_slices(dvol[d:d + b], PATCH) for d in range(0, D, b)]
            seen = [ops.view_batch(s, views) for s in small]
            t_view = timed_ms(lambda: [ops.view_batch(s, views) for s in small], a.repeats)
            t_net = timed_ms(lambda: [net(s.view(-1, 1, h, w)) for s in seen], a.repeats)
            logits = [net(s.view(-1, 1, h, w)) for s in seen]
            t_ens = timed_ms(lambda: [ops.tta_argmax_zoom_back(lg, views, SHAPE[1:]) for lg in logits], a.repeats)
            del small, seen, logits
            floor = V * t_net1[0]
            differ = int((preds[spec] != preds[None]).sum())
            lines += [f"  tta=\"{spec}\" ({V} views, {-(-D // b)} batches of {b} slices = {V * b} samples): {fmt(whole[spec])} = "
                      f"{whole[spec][0] / whole[None][0]:.2f} x tta=None; {differ} of {preds[spec].size} voxels differ from tta=None",
                      f"    network on the views alone: {fmt(t_net)}; floor V x single-view network = {floor:.2f} ms",
                      f"    ops.view_batch alone: {fmt(t_view)}  ({t_view[0] * 1e3 / D:.1f} us per slice)",
                      f"    ops.tta_argmax_zoom_back alone: {fmt(t_ens)}  ({t_ens[0] * 1e3 / D:.1f} us per slice)",
                      f"    the two kernels over the floor: {100 * (t_view[0] + t_ens[0]) / floor:.2f} %; the whole call over the floor: "
                      f"{whole[spec][0] / floor:.2f}"]
            print("\n".join(lines[-5:]), flush=True)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(text)
    print(f"wrote {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
