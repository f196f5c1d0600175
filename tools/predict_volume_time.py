#!/usr/bin/env python3
"""Time utils.predict_volume with the resizes on the device (resize="hip": ops.resize_slices -> network -> ops.argmax_zoom_back,
csrc/resize.hip) against the host path (resize="host": scipy.ndimage.zoom per slice, the code of the parent commit unchanged) on
a Synapse-sized volume, and record it in profiles/predict_volume_timing.txt.

    python tools/predict_volume_time.py [--out FILE] [--repeats 10] [--host-repeats 10]

The volume is a seeded float32 148 x 512 x 512 array, the network the tiny configuration at 224 x 224 with closed-form weights,
batches of 16 slices.  Every timing is a host clock around work between two device synchronisations, one warm-up call, the
median of --repeats (host path: --host-repeats; it takes seconds per call).  The parts are timed alone on resident tensors, a
whole volume's worth of batches per repeat: the network, resize_slices and argmax_zoom_back.  The number of voxels at which the
two predictions differ is reported (resize_slices may round at most 1 element in 1e5 to the neighbouring float32, which can move
an argmax that was nearly tied); above 1 in 1e5 the tool exits non-zero without writing.  Run it under `timeout`; an exception
ends the run, so nothing is enqueued after a failed step."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPE, PATCH, NCLS, BATCH = (148, 512, 512), (224, 224), 9, 16


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


def fmt(t):
    return f"{t[0]:.2f} ms (min {t[1]:.2f}, max {t[2]:.2f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predict_volume_timing.txt"))
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--host-repeats", type=int, default=10)
    a = ap.parse_args()

    from cswin_unet_amd import _lib, ops
    from cswin_unet_amd.networks.cswin_unet import CSWinTransformer
    from cswin_unet_amd.utils import predict_volume
    from oracle.determ import det_normal, fill_state_dict
    assert torch.cuda.is_available() and _lib.lib().cswin_device_ok() == 1, "needs a gfx950 HIP device"

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

    hip_pred = predict_volume(vol, net, PATCH, BATCH, resize="hip")
    hip = timed_ms(lambda: predict_volume(vol, net, PATCH, BATCH, resize="hip"), a.repeats, warmup=0)
    dev = timed_ms(lambda: predict_volume(vol, net, PATCH, BATCH, resize="hip", return_device=True), a.repeats)
    print(f"predict_volume resize=hip {fmt(hip)}; kept on the device {fmt(dev)}", flush=True)

    dvol = torch.from_numpy(vol).cuda()
    starts = range(0, SHAPE[0], BATCH)
    with torch.no_grad():
        small = [ops.resize_slices(dvol[d:d + BATCH], PATCH) for d in starts]
        logits = [net(s.unsqueeze(1)) for s in small]
        t_resize = timed_ms(lambda: [ops.resize_slices(dvol[d:d + BATCH], PATCH) for d in starts], a.repeats)
        t_net = timed_ms(lambda: [net(s.unsqueeze(1)) for s in small], a.repeats)
        t_back = timed_ms(lambda: [ops.argmax_zoom_back(lg, SHAPE[1:]) for lg in logits], a.repeats)
    t_up = timed_ms(lambda: torch.from_numpy(vol).cuda(), a.repeats)
    pred8 = torch.zeros(SHAPE, dtype=torch.uint8, device="cuda")
    t_down = timed_ms(lambda: pred8.cpu().numpy(), a.repeats)
    del small, logits
    print(f"resize_slices {fmt(t_resize)}; network {fmt(t_net)}; argmax_zoom_back {fmt(t_back)}", flush=True)

    host_pred = predict_volume(vol, net, PATCH, BATCH)
    host = timed_ms(lambda: predict_volume(vol, net, PATCH, BATCH), a.host_repeats, warmup=0)
    differ = int((host_pred != hip_pred).sum())
    ok = differ * 100000 <= hip_pred.size and host_pred.shape == hip_pred.shape == SHAPE

    n = SHAPE[0]
    lines = [f"predict_volume timing: seeded float32 volume {SHAPE[0]} x {SHAPE[1]} x {SHAPE[2]} -> {PATCH[0]} x {PATCH[1]}, tiny network, "
             f"{NCLS} classes, batches of {BATCH}, {torch.cuda.get_device_name(0)}",
             f"agreement resize=hip vs resize=host (every voxel of the prediction): {'PASS' if ok else 'FAIL'} ({differ} of {hip_pred.size} differ)",
             f"predict_volume(resize=\"host\") (scipy zoom per slice around the network; the parent commit's path), host clock, median of "
             f"{a.host_repeats}: {fmt(host)}",
             f"predict_volume(resize=\"hip\") (upload, resize_slices -> network -> argmax_zoom_back per batch, download), "
             f"median of {a.repeats}: {fmt(hip)}",
             f"predict_volume(resize=\"hip\", return_device=True) (no download), median of {a.repeats}: {fmt(dev)}",
             f"speed-up hip vs host: {host[0] / hip[0]:.1f}x",
             f"parts alone, resident tensors, {len(starts)} batches ({n} slices) per repeat, median of {a.repeats}:",
             f"  ops.resize_slices ({SHAPE[1]} x {SHAPE[2]} -> {PATCH[0]} x {PATCH[1]}): {fmt(t_resize)}  ({t_resize[0] * 1e3 / n:.1f} us per slice)",
             f"  network forward ({PATCH[0]} x {PATCH[1]}): {fmt(t_net)}",
             f"  ops.argmax_zoom_back ({NCLS} x {PATCH[0]} x {PATCH[1]} -> {SHAPE[1]} x {SHAPE[2]}): {fmt(t_back)}  ({t_back[0] * 1e3 / n:.1f} us per slice)",
             f"  upload of the float32 volume ({vol.nbytes / 2 ** 20:.0f} MiB, pageable): {fmt(t_up)}",
             f"  download of the uint8 prediction ({pred8.numel() / 2 ** 20:.0f} MiB): {fmt(t_down)}",
             f"predict_volume(resize=\"hip\") / network forward: {hip[0] / t_net[0]:.2f}"]
    text = "\n".join(lines) + "\n"
    print(text)
    if not ok:
        print("FAILED: the two predictions differ at more than 1 voxel in 1e5; nothing written")
        return 1
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
