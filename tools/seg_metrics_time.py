#!/usr/bin/env python3
"""Time the device metrics path (utils.volume_metrics -> ops.seg_metrics, csrc/metrics.hip) on a full-size volume against the
host path and against inference, and record it in profiles/seg_metrics_timing.txt.

    python tools/seg_metrics_time.py [--out FILE] [--repeats 10] [--kernel-stats DIR] [--skip-host]
    python tools/seg_metrics_time.py --one-call          # warm-up + ONE volume_metrics call, for a profiler run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o out -- python tools/seg_metrics_time.py --one-call
    python tools/seg_metrics_time.py --voxelspacing 2.5 0.73 0.73 [--out FILE] [--repeats 10] [--skip-host]

The pair is a seeded nine-class 148 x 512 x 512 blob volume (Synapse-sized).  volume_metrics is timed with device events around
the whole call (validation, upload, kernels, download of counts and the used histogram bins, float64 finish), which ends in a
synchronising download; median of --repeats after warm-up.  The host path is the per-class calculate_metric_percase loop over
classes 1..8, once (about two minutes).  predict_volume of a 148-slice 224 x 224 volume with the tiny network gives the scale
of inference.  The two metric lists must agree (Dice exactly, HD95 within 1e-12: square roots of the same integers and one
float64 interpolation on both sides) or the tool exits non-zero without writing.  Run it under `timeout`; every step ends in a
synchronise and an exception ends the run, so nothing is enqueued after a failed step.

--voxelspacing times the spacing-aware path on the same pair instead (profiles/surface_metrics_timing.txt):
volume_metrics(voxelspacing=..., assd=True) whole, ops.surface_distances alone, the finish alone (per-segment torch.sort,
download, numpy), ops.seg_metrics of the same run for comparison, and once the host loop with voxelspacing, which it must agree
with (Dice exactly, HD95 and ASSD within 1e-12)."""
import argparse
import csv
import glob
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPE, NCLS, SEED = (148, 512, 512), 9, 2024


def blob_pair(shape, ncls, seed):
    """One ellipsoid per foreground class; the prediction's is the label's moved by up to 3 voxels, radii scaled 0.85 .. 1.15."""
    rng = np.random.default_rng(seed)
    pred, label = np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)
    dims = np.asarray(shape, np.float64)

    def put(vol, center, radii, value):
        lo = [max(0, int(np.floor(c - r))) for c, r in zip(center, radii)]
        hi = [min(n, int(np.ceil(c + r)) + 1) for c, r, n in zip(center, radii, shape)]
        box = tuple(slice(a, b) for a, b in zip(lo, hi))
        grids = np.ogrid[box]
        vol[box][sum(((g - c) / r) ** 2 for g, c, r in zip(grids, center, radii)) <= 1.0] = value

    for cid in range(1, ncls):
        center = rng.uniform(0.2, 0.8, 3) * (dims - 1)
        radii = rng.uniform(0.06, 0.18, 3) * dims
        put(label, center, radii, cid)
        put(pred, center + rng.uniform(-3, 3, 3), radii * rng.uniform(0.85, 1.15, 3), cid)
    return pred, label


def device_ms(fn, repeats, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times), min(times), max(times)


def kernel_rows(stats_dir):
    """Rows (name, calls, total us, average us) of the metrics kernels from a rocprofv3 --stats run's *kernel_stats.csv."""
    files = sorted(glob.glob(os.path.join(stats_dir, "**", "*kernel_stats.csv"), recursive=True))
    if not files:
        return None
    rows = []
    for r in csv.DictReader(open(files[0])):
        if "seg_" in r["Name"]:
            rows.append((r["Name"].replace("(anonymous namespace)::", "").split("(")[0], int(r["Calls"]),
                         float(r["TotalDurationNs"]) / 1e3, float(r["AverageNs"]) / 1e3))
    return sorted(rows, key=lambda r: -r[2])


def surface_main(a, pred, label):
    from cswin_unet_amd import _lib, ops
    from cswin_unet_amd.utils import _class_ids_u8, calculate_metric_percase, metrics_from_surface_lists, volume_metrics
    sp, n = tuple(a.voxelspacing), max(a.repeats, 10)
    hip = volume_metrics(pred, label, NCLS, voxelspacing=sp, assd=True)
    vm = device_ms(lambda: volume_metrics(pred, label, NCLS, voxelspacing=sp, assd=True), n)
    p8, l8 = torch.from_numpy(pred).cuda(), torch.from_numpy(label).cuda()
    km = device_ms(lambda: ops.surface_distances(p8, l8, NCLS, sp), n)
    sm = device_ms(lambda: ops.seg_metrics(p8, l8, NCLS), n)
    counts, nq, dist2 = ops.surface_distances(p8, l8, NCLS, sp)
    nq_host = nq.cpu().numpy()
    total = int(nq_host.sum())
    assert total <= dist2.numel(), "the default capacity overflowed"

    def finish():
        d = dist2.clone()
        start = 0
        for k in nq_host.ravel().tolist():
            if k > 1:
                d[start:start + k] = torch.sort(d[start:start + k]).values
            start += k
        return metrics_from_surface_lists(counts.cpu().numpy(), nq_host, d[:total].cpu().numpy(), assd=True)

    fm = device_ms(finish, n)

    phases = {}

    def lap(name, t0):
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        phases.setdefault(name, []).append((t1 - t0) * 1e3)
        return t1

    for _ in range(n + 2):                                            # volume_metrics' own steps, each ended by a synchronise
        torch.cuda.synchronize()
        t = time.perf_counter()
        q8, m8 = _class_ids_u8(pred, NCLS, "prediction", "cuda"), _class_ids_u8(label, NCLS, "label", "cuda")
        t = lap("range check on the host + upload of both volumes", t)
        lists = ops.surface_distances(q8, m8, NCLS, sp)
        t = lap("ops.surface_distances", t)
        finish()
        t = lap("sort + download + numpy finish", t)
        del lists
    phase_lines = [f"  {k}: {statistics.median(v[2:]):.2f} ms" for k, v in phases.items()]
    ws = _lib.lib().cswin_surface_dist_workspace(*SHAPE, 3, NCLS)
    print(f"volume_metrics(voxelspacing) {vm[0]:.2f} ms, ops.surface_distances {km[0]:.2f} ms, finish {fm[0]:.2f} ms, ops.seg_metrics {sm[0]:.2f} ms",
          flush=True)
    if a.skip_host:
        print("--skip-host: no agreement check, nothing written")
        return 0
    t0 = time.perf_counter()
    host = [calculate_metric_percase(pred == i, label == i, voxelspacing=sp, assd=True) for i in range(1, NCLS)]
    host_s = time.perf_counter() - t0
    ok = len(hip) == len(host) and all(g[0] == h[0] and all(abs(x - y) <= 1e-12 + 1e-12 * abs(y) for x, y in zip(g[1:], h[1:]))
                                       for g, h in zip(hip, host))
    lines = [f"surface metrics timing: seeded (seed {SEED}) {NCLS}-class blob pair {SHAPE[0]} x {SHAPE[1]} x {SHAPE[2]}, voxel spacing {sp}, "
             f"{torch.cuda.get_device_name(0)}",
             f"agreement hip vs host (Dice exact, HD95 and ASSD within 1e-12): {'PASS' if ok else 'FAIL'}"]
    lines += [f"  class {c}: hip dice {g[0]:.17g} hd95 {g[1]:.17g} assd {g[2]:.17g} | host dice {h[0]:.17g} hd95 {h[1]:.17g} assd {h[2]:.17g}"
              for c, (g, h) in enumerate(zip(hip, host), 1)]
    lines += [f"host path (calculate_metric_percase(voxelspacing=, assd=True) over classes 1..{NCLS - 1}, one repeat): {host_s:.1f} s",
              f"utils.volume_metrics(voxelspacing=, assd=True) (validate + upload + kernels + sort + download + float64 finish), device events, "
              f"median of {n}: {vm[0]:.2f} ms (min {vm[1]:.2f}, max {vm[2]:.2f})",
              f"ops.surface_distances alone (device-resident uint8 inputs, kernels only), median of {n}: {km[0]:.2f} ms (min {km[1]:.2f}, max {km[2]:.2f})",
              f"finish alone (copy of the list, {int((nq_host > 1).sum())} torch.sort calls, download, numpy sqrt / percentile / means), "
              f"median of {n}: {fm[0]:.2f} ms (min {fm[1]:.2f}, max {fm[2]:.2f}) = {fm[0] / vm[0]:.2f} of volume_metrics",
              f"ops.seg_metrics alone (unit spacing, histogram path), same run, median of {n}: {sm[0]:.2f} ms (min {sm[1]:.2f}, max {sm[2]:.2f})",
              f"wall clock of volume_metrics' steps, each ended by a synchronise, median of {n}:", *phase_lines,
              f"surface distances in the list: {total} (default capacity {dist2.numel()}, {pred.size} voxels)",
              f"workspace: {ws} bytes ({ws / 2 ** 20:.1f} MiB)",
              f"speed-up volume_metrics vs host: {host_s * 1e3 / vm[0]:.0f}x"]
    text = "\n".join(lines) + "\n"
    print(text)
    if not ok:
        print("FAILED: disagreement; nothing written")
        return 1
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default: profiles/seg_metrics_timing.txt, with --voxelspacing profiles/surface_metrics_timing.txt")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--kernel-stats", default=None, help="output directory of a separate rocprofv3 --kernel-trace --stats run of --one-call")
    ap.add_argument("--skip-host", action="store_true", help="no host timing and no agreement check: nothing is written")
    ap.add_argument("--one-call", action="store_true")
    ap.add_argument("--voxelspacing", type=float, nargs=3, default=None, metavar=("SZ", "SY", "SX"),
                    help="time the spacing-aware path (ops.surface_distances) under this spacing instead")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "surface_metrics_timing.txt" if a.voxelspacing else "seg_metrics_timing.txt")

    from cswin_unet_amd import _lib, ops
    from cswin_unet_amd.utils import calculate_metric_percase, predict_volume, volume_metrics
    assert torch.cuda.is_available() and _lib.lib().cswin_device_ok() == 1, "needs a gfx950 HIP device"
    pred, label = blob_pair(SHAPE, NCLS, SEED)
    if a.voxelspacing:
        return surface_main(a, pred, label)

    if a.one_call:
        volume_metrics(pred, label, NCLS)
        torch.cuda.synchronize()
        volume_metrics(pred, label, NCLS)
        torch.cuda.synchronize()
        return 0

    hip = volume_metrics(pred, label, NCLS)
    vm = device_ms(lambda: volume_metrics(pred, label, NCLS), max(a.repeats, 10))
    p8, l8 = torch.from_numpy(pred).cuda(), torch.from_numpy(label).cuda()
    km = device_ms(lambda: ops.seg_metrics(p8, l8, NCLS), max(a.repeats, 10))
    ws = _lib.lib().cswin_seg_metrics_workspace(*SHAPE, 3, NCLS)
    print(f"volume_metrics {vm[0]:.2f} ms, ops.seg_metrics {km[0]:.2f} ms", flush=True)

    from cswin_unet_amd.networks.cswin_unet import CSWinTransformer
    from oracle.determ import det_normal, fill_state_dict

    class OneChannel(torch.nn.Module):
        def __init__(self, m):
            super().__init__()
            self.m = m

        def forward(self, x):
            return self.m(x.repeat(1, 3, 1, 1))

    net = CSWinTransformer(img_size=224, num_classes=NCLS, embed_dim=64, depth=[1, 2, 9, 1], split_size=[1, 2, 7, 7],
                           num_heads=[2, 4, 8, 16], qkv_bias=True, drop_path_rate=0.).cuda()
    net = OneChannel(fill_state_dict(net)).eval()
    vol = det_normal("seg_metrics_time.vol", (SHAPE[0], 224, 224))
    pv = device_ms(lambda: predict_volume(vol, net, (224, 224)), 3, warmup=1)
    print(f"predict_volume {pv[0]:.1f} ms", flush=True)

    if a.skip_host:
        print("--skip-host: no agreement check, nothing written")
        return 0
    t0 = time.perf_counter()
    host = [calculate_metric_percase(pred == i, label == i) for i in range(1, NCLS)]
    host_s = time.perf_counter() - t0
    ok = len(hip) == len(host) and all(g[0] == h[0] and abs(g[1] - h[1]) <= 1e-12 + 1e-12 * abs(h[1]) for g, h in zip(hip, host))

    lines = [f"seg_metrics timing: seeded (seed {SEED}) {NCLS}-class blob pair {SHAPE[0]} x {SHAPE[1]} x {SHAPE[2]}, {torch.cuda.get_device_name(0)}",
             f"agreement hip vs host (Dice exact, HD95 within 1e-12): {'PASS' if ok else 'FAIL'}"]
    lines += [f"  class {c}: hip dice {g[0]:.17g} hd95 {g[1]:.17g} | host dice {h[0]:.17g} hd95 {h[1]:.17g}" for c, (g, h) in enumerate(zip(hip, host), 1)]
    lines += [f"utils.volume_metrics (validate + upload + kernels + download + float64 finish), device events, median of {max(a.repeats, 10)}: "
              f"{vm[0]:.2f} ms (min {vm[1]:.2f}, max {vm[2]:.2f})",
              f"ops.seg_metrics alone (device-resident uint8 inputs, kernels only), median of {max(a.repeats, 10)}: {km[0]:.2f} ms (min {km[1]:.2f}, max {km[2]:.2f})",
              f"workspace: {ws} bytes ({ws / 2 ** 20:.1f} MiB)",
              f"host path (calculate_metric_percase over classes 1..{NCLS - 1}, one repeat): {host_s:.1f} s",
              f"speed-up volume_metrics vs host: {host_s * 1e3 / vm[0]:.0f}x (floor: 10x)",
              f"predict_volume, {SHAPE[0]} slices 224 x 224, tiny network, batch 16, median of 3: {pv[0]:.1f} ms",
              f"volume_metrics / predict_volume: {vm[0] / pv[0]:.3f}"]
    if a.kernel_stats:
        rows = kernel_rows(a.kernel_stats)
        if rows is None:
            lines.append(f"per-kernel split: no *kernel_stats.csv under {os.path.relpath(a.kernel_stats, ROOT)}")
        else:
            lines.append("per-kernel split (separate rocprofv3 --kernel-trace --stats run of --one-call: two volume_metrics calls):")
            lines += [f"  {n:28s} {c:5d} calls  total {t:10.1f} us  average {av:9.1f} us" for n, c, t, av in rows]
    text = "\n".join(lines) + "\n"
    print(text)
    if not ok or host_s * 1e3 / vm[0] < 10:
        print("FAILED: disagreement or below the 10x floor; nothing written")
        return 1
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
