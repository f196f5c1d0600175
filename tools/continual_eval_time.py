#!/usr/bin/env python3
"""Time the two device pieces around a continual-learning stage and record them in profiles/continual_eval_timing.txt:

  * ops.argmax_zoom_back on 16 x 14 x 224 x 224 logits -> 512 x 512 with and without classes=[0, 9, 10, 11] (csrc/resize.hip);
  * ops.class_counts (csrc/label_stats.hip) on 2048 uint8 slices of 512 x 512 holding seeded blobs, and on 2048 constant slices,
    beside the reference's formulation of the same quantities with torch on the same device: one `(labels == c).sum()` per class
    (universal_train.py:1010-1011) and one `torch.unique` per slice (:207);
  * utils.predict_volume(resize="hip") on the 148 x 512 x 512 volume of tools/predict_volume_time.py with a 14-class network,
    with and without class_indices=[0, 9, 10, 11].

    python tools/continual_eval_time.py [--out FILE] [--repeats 10] [--plain-lib FILE]

--plain-lib: a shared library with the per-lane-atomics form of the class-count kernel, which the wave-uniform fast path is
measured against on the same labels (the counts must be equal):
    hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -DCSWIN_CLASS_COUNTS_FAST=0 -x hip -shared \\
          cswin_unet_amd/csrc/label_stats.hip cswin_unet_amd/csrc/capi.cpp -o FILE

Every timing is a host clock around work between two device synchronisations, one warm-up call, the median of --repeats.  Run it
under `timeout`; an exception ends the run, so nothing is enqueued after a failed step."""
import argparse
import ctypes
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPE, PATCH, NCLS, BATCH = (148, 512, 512), (224, 224), 14, 16
KITS23 = [0, 9, 10, 11]
NSLICES, SIDE, LABEL_CLASSES = 2048, 512, 9


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


def blob_slices(n, side, seed):
    """uint8 (n, side, side) on the device: per slice eight seeded ellipses of ids 1..8 on background 0, later over earlier."""
    g = torch.Generator().manual_seed(seed)
    centre = (0.15 + 0.7 * torch.rand(n, 8, 2, generator=g)) * (side - 1)
    radius = (0.04 + 0.14 * torch.rand(n, 8, 2, generator=g)) * side
    centre, radius = centre.cuda(), radius.cuda()
    yy = torch.arange(side, device="cuda", dtype=torch.float32).view(1, side, 1)
    xx = torch.arange(side, device="cuda", dtype=torch.float32).view(1, 1, side)
    out = torch.zeros((n, side, side), dtype=torch.uint8, device="cuda")
    for n0 in range(0, n, 128):
        sl = slice(n0, n0 + 128)
        for k in range(8):
            inside = ((yy - centre[sl, k, 0].view(-1, 1, 1)) / radius[sl, k, 0].view(-1, 1, 1)) ** 2 + \
                     ((xx - centre[sl, k, 1].view(-1, 1, 1)) / radius[sl, k, 1].view(-1, 1, 1)) ** 2 <= 1.0
            out[sl][inside] = k + 1
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "continual_eval_timing.txt"))
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--plain-lib", default=None)
    a = ap.parse_args()

    from cswin_unet_amd import _lib, ops
    from cswin_unet_amd.networks.cswin_unet import CSWinTransformer
    from cswin_unet_amd.utils import predict_volume
    from oracle.determ import det_normal, fill_state_dict
    assert torch.cuda.is_available() and _lib.lib().cswin_device_ok() == 1, "needs a gfx950 HIP device"
    lines = [f"continual evaluation and label statistics, {torch.cuda.get_device_name(0)}; host clock between two synchronisations, "
             f"one warm-up, median of {a.repeats}"]

    # ---- the argmax over a class list ------------------------------------------------------------------------------------
    g = torch.Generator().manual_seed(7)
    logits = (torch.round(torch.randn(BATCH, NCLS, *PATCH, generator=g) * 4) / 4).cuda()
    t_all = timed_ms(lambda: ops.argmax_zoom_back(logits, SHAPE[1:]), a.repeats)
    t_sub = timed_ms(lambda: ops.argmax_zoom_back(logits, SHAPE[1:], classes=KITS23), a.repeats)
    want = torch.argmax(logits[:, KITS23], 1)
    same = torch.equal(ops.argmax_zoom_back(logits, PATCH, classes=KITS23).long(), want)
    lines += [f"ops.argmax_zoom_back, {BATCH} x {NCLS} x {PATCH[0]} x {PATCH[1]} -> {SHAPE[1]} x {SHAPE[2]}:",
              f"  all {NCLS} classes: {fmt(t_all)}",
              f"  classes={KITS23}: {fmt(t_sub)}  (equal to torch.argmax(logits[:, classes], 1) without the zoom: {same})"]
    print("\n".join(lines), flush=True)
    del logits

    # ---- the per-slice class histogram -----------------------------------------------------------------------------------
    blobs = blob_slices(NSLICES, SIDE, 11)
    const = (torch.arange(NSLICES, device="cuda") % LABEL_CLASSES).to(torch.uint8).view(-1, 1, 1).expand(NSLICES, SIDE, SIDE).contiguous()
    torch.cuda.synchronize()
    gib = blobs.numel() / 2 ** 30
    plain = None
    if a.plain_lib:
        plain = ctypes.CDLL(os.path.abspath(a.plain_lib)).cswin_class_counts
        plain.restype, plain.argtypes = _lib.SIGNATURES["cswin_class_counts"]

    def run_plain(lab):
        out = torch.empty((NSLICES, LABEL_CLASSES + 1), dtype=torch.int64, device="cuda")
        rc = plain(_lib.ptr(lab), 1, None, 0, _lib.ptr(out), NSLICES, SIDE * SIDE, LABEL_CLASSES, _lib.stream())
        assert rc == 0, rc
        return out

    def torch_sums(lab):
        return torch.stack([(lab == c).sum() for c in range(LABEL_CLASSES)])

    def torch_unique(lab):
        return [torch.unique(s) for s in lab]

    ok = True
    lines.append(f"ops.class_counts, {NSLICES} uint8 slices of {SIDE} x {SIDE} ({gib:.2f} GiB), ncls = {LABEL_CLASSES}:")
    for name, lab in (("seeded blobs", blobs), ("constant slices", const)):
        counts = ops.class_counts(lab, LABEL_CLASSES)
        t_hip = timed_ms(lambda: ops.class_counts(lab, LABEL_CLASSES), a.repeats)
        lines.append(f"  {name}: {fmt(t_hip)}  ({gib * 2 ** 30 / t_hip[0] / 1e6:.0f} GB/s)")
        if plain is not None:
            t_plain = timed_ms(lambda: run_plain(lab), a.repeats)
            eq = torch.equal(run_plain(lab), counts)
            ok &= eq
            lines.append(f"    per-lane LDS atomics only (no wave-uniform fast path): {fmt(t_plain)}  (counts equal: {eq})")
        sums = torch_sums(lab)
        eq = torch.equal(sums, counts.sum(0)[:LABEL_CLASSES])
        ok &= eq
        t_sums = timed_ms(lambda: torch_sums(lab), a.repeats)
        lines.append(f"    torch, one (labels == c).sum() per class, {LABEL_CLASSES} classes, no .item(): {fmt(t_sums)}  (sums equal: {eq})")
        t_uni = timed_ms(lambda: torch_unique(lab), max(1, a.repeats // 3))
        lines.append(f"    torch, one torch.unique per slice, median of {max(1, a.repeats // 3)}: {fmt(t_uni)}")
        print("\n".join(lines[-4:]), flush=True)
    del blobs, const

    # ---- a whole volume ----------------------------------------------------------------------------------------------------
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
    t_full = timed_ms(lambda: predict_volume(vol, net, PATCH, BATCH, resize="hip"), a.repeats)
    t_task = timed_ms(lambda: predict_volume(vol, net, PATCH, BATCH, resize="hip", class_indices=KITS23), a.repeats)
    lines += [f"predict_volume(resize=\"hip\"), float32 volume {SHAPE[0]} x {SHAPE[1]} x {SHAPE[2]}, tiny network with {NCLS} classes, batches of {BATCH}:",
              f"  all classes: {fmt(t_full)}",
              f"  class_indices={KITS23}: {fmt(t_task)}"]
    text = "\n".join(lines) + "\n"
    print(text)
    if not ok:
        print("FAILED: the counts of two formulations differ; nothing written")
        return 1
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
