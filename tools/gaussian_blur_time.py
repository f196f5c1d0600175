#!/usr/bin/env python3
"""Time the device Gaussian blur (ops.gaussian_blur, csrc/blur.hip) alone, inside ops.augment_batch and inside
utils.predict_volume(resize="hip"), against scipy.ndimage.gaussian_filter per slice on the host (the only way the parent commit
offers), and record it in profiles/gaussian_blur_timing.txt.

    python tools/gaussian_blur_time.py [--out FILE] [--repeats 10] [--host-repeats 10]

Seeded float32 arrays of 24 and 148 slices of 512 x 512, sigma 1 (radius 4) and sigma 3 (radius 12); the tiny network at
224 x 224 with closed-form weights, batches of 16 slices.  Every timing is a host clock around work between two device
synchronisations, one warm-up call, the median of --repeats (scipy: --host-repeats).  The blur reads and writes every element
once, 8 D H W bytes: that traffic over the time, against the 8.0 TB/s HBM peak and the 6.29 TB/s a float4 copy reaches, is a
streaming kernel's share of the memory bound.  The number of voxels at which the prediction of the device-blurred volume differs
from that of the volume blurred by scipy first is reported; above 1 in 1e5 the tool exits non-zero without writing.  Run it under
`timeout`; an exception ends the run, so nothing is enqueued after a failed step."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPE, PATCH, NCLS, BATCH = (148, 512, 512), (224, 224), 9, 16
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


def fmt(t):
    return f"{t[0]:.3f} ms (min {t[1]:.3f}, max {t[2]:.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gaussian_blur_timing.txt"))
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--host-repeats", type=int, default=10)
    a = ap.parse_args()

    from scipy.ndimage import gaussian_filter
    from cswin_unet_amd import _lib, ops
    from cswin_unet_amd.datasets import AUG_NONE, AUG_ROT90_FLIP, AUG_ROTATE
    from cswin_unet_amd.networks.cswin_unet import CSWinTransformer
    from cswin_unet_amd.utils import predict_volume
    from oracle.determ import det_normal, fill_state_dict
    assert torch.cuda.is_available() and _lib.lib().cswin_device_ok() == 1, "needs a gfx950 HIP device"

    vol = det_normal("predict_volume_time.vol", SHAPE)
    dvol = torch.from_numpy(vol).cuda()
    lines = [f"gaussian blur timing: seeded float32 slices of {SHAPE[1]} x {SHAPE[2]}, {torch.cuda.get_device_name(0)}",
             f"ops.gaussian_blur alone on resident slices, median of {a.repeats}; bytes = 8 D H W (one read, one write); "
             f"scipy.ndimage.gaussian_filter per slice on the host, median of {a.host_repeats}:"]
    for D in (24, SHAPE[0]):
        for sigma in (1.0, 3.0):
            x = dvol[:D]
            t = timed_ms(lambda: ops.gaussian_blur(x, sigma), a.repeats)
            h = timed_ms(lambda: [gaussian_filter(s, sigma) for s in vol[:D]], a.host_repeats)
            rate = 8.0 * x.numel() / (t[0] * 1e-3)
            line = (f"  {D} slices, sigma {sigma:g} (radius {int(4 * sigma + 0.5)}): {fmt(t)}, {rate / 1e12:.2f} TB/s = "
                    f"{100 * rate / HBM_PEAK:.0f} % of the 8.0 TB/s peak, {100 * rate / HBM_COPY:.0f} % of a copy's 6.29 TB/s; "
                    f"scipy {fmt(h)}, {h[0] / t[0]:.0f}x")
            print(line, flush=True)
            lines.append(line)

    # a training batch: 24 samples 512 x 512 -> 224 x 224, the three kinds in turn
    B = 24
    rng = np.random.default_rng(5)
    par = torch.tensor([[(AUG_NONE, AUG_ROT90_FLIP, AUG_ROTATE)[b % 3], b % 4, b % 2, (b % 5) * 7 - 14] for b in range(B)], dtype=torch.int32)
    dimg = dvol[:B].contiguous()
    dlab = torch.from_numpy(rng.integers(0, NCLS, size=(B,) + SHAPE[1:]).astype(np.uint8)).cuda()
    t_aug = timed_ms(lambda: ops.augment_batch(dimg, dlab, par, PATCH), a.repeats)
    t_aug_b = timed_ms(lambda: ops.augment_batch(dimg, dlab, par, PATCH, blur_sigma=1.0), a.repeats)
    lines += [f"ops.augment_batch, {B} samples {SHAPE[1]} x {SHAPE[2]} -> {PATCH[0]} x {PATCH[1]}, median of {a.repeats}:",
              f"  without blur: {fmt(t_aug)}", f"  blur_sigma=1.0: {fmt(t_aug_b)}  (+{t_aug_b[0] - t_aug[0]:.3f} ms)"]
    print("\n".join(lines[-3:]), flush=True)

    class OneChannel(torch.nn.Module):
        def __init__(self, m):
            super().__init__()
            self.m = m

        def forward(self, x):
            return self.m(x.repeat(1, 3, 1, 1))

    net = CSWinTransformer(img_size=PATCH[0], num_classes=NCLS, embed_dim=64, depth=[1, 2, 9, 1], split_size=[1, 2, 7, 7],
                           num_heads=[2, 4, 8, 16], qkv_bias=True, drop_path_rate=0.).cuda()
    net = OneChannel(fill_state_dict(net)).eval()
    kw = dict(resize="hip", return_device=True)

    def parent_path():
        return predict_volume(np.stack([gaussian_filter(s, 1.0) for s in vol]), net, PATCH, BATCH, **kw)

    pred_dev = predict_volume(vol, net, PATCH, BATCH, blur_sigma=1.0, **kw).cpu().numpy()
    pred_par = parent_path().cpu().numpy()
    differ = int((pred_dev != pred_par).sum())
    ok = differ * 100000 <= pred_dev.size and pred_dev.shape == pred_par.shape == SHAPE
    t_plain = timed_ms(lambda: predict_volume(vol, net, PATCH, BATCH, **kw), a.repeats)
    t_blur = timed_ms(lambda: predict_volume(vol, net, PATCH, BATCH, blur_sigma=1.0, **kw), a.repeats)
    t_par = timed_ms(parent_path, a.host_repeats)
    lines += [f"predict_volume(resize=\"hip\", return_device=True), {SHAPE[0]} x {SHAPE[1]} x {SHAPE[2]} -> {PATCH[0]} x {PATCH[1]}, tiny network, "
              f"batches of {BATCH}, median of {a.repeats}:",
              f"  unblurred volume: {fmt(t_plain)}",
              f"  blur_sigma=1.0 (ops.gaussian_blur per batch): {fmt(t_blur)}  (+{t_blur[0] - t_plain[0]:.3f} ms)",
              f"  volume blurred by scipy per slice first, then passed in (the parent commit's path), median of {a.host_repeats}: {fmt(t_par)}",
              f"agreement of the last two predictions (every voxel): {'PASS' if ok else 'FAIL'} ({differ} of {pred_dev.size} differ)"]
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
