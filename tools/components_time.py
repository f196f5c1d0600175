"""Time of the component filter on the device against the scipy host path, on two volumes a Synapse evaluation would see in size:

  organs  148 x 512 x 512, nine classes: one ellipsoid per class 1..8 plus 0.05 % single-voxel specks of random classes
  solid   the same size with every voxel in class 1 -- one component of N voxels, the contention worst case of the union-find

Per volume: device time of ops.connected_components (labels + sizes) and of ops.filter_components (label + filter, rule
"largest"), device events around `--repeats` windows of `--inner` calls after `--warmup` warm-up calls, per call: the median and
the spread; the wall time of utils.filter_components_host on the same volume in the same run; whether the two outputs are equal.
For the organ volume also ops.seg_metrics of the filtered prediction against the clean volume, the call the filter sits in front
of.  Prints one JSON line per volume and writes them to --out if given.  Needs a HIP device: there is no fallback.

    python tools/components_time.py --out components_time.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _ellipsoid(vol, center, radii, value):
    lo = [max(0, int(np.floor(c - r))) for c, r in zip(center, radii)]
    hi = [min(n, int(np.ceil(c + r)) + 1) for c, r, n in zip(center, radii, vol.shape)]
    grids = np.ogrid[tuple(slice(a, b) for a, b in zip(lo, hi))]
    inside = sum(((g - c) / r) ** 2 for g, c, r in zip(grids, center, radii)) <= 1.0
    vol[tuple(slice(a, b) for a, b in zip(lo, hi))][inside] = value


def organ_volume(shape, seed=0, speck_fraction=0.0005):
    """(clean, speckled): eight ellipsoidal organs, and the same with speck_fraction of the background voxels set to random classes"""
    rng = np.random.default_rng(seed)
    clean = np.zeros(shape, np.uint8)
    dims = np.asarray(shape, np.float64)
    for cid in range(1, 9):
        _ellipsoid(clean, rng.uniform(0.2, 0.8, 3) * (dims - 1), rng.uniform(0.06, 0.16, 3) * dims, cid)
    speckled = clean.copy()
    bg = np.flatnonzero(clean.ravel() == 0)
    pick = rng.choice(bg, int(speck_fraction * clean.size), replace=False)
    speckled.ravel()[pick] = rng.integers(1, 9, pick.size).astype(np.uint8)
    return clean, speckled


def device_ms(fn, warmup, repeats, inner):
    """per-call device time: `repeats` windows of `inner` back-to-back calls between two events"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / inner)
    return {"median_ms": float(np.median(times)), "min_ms": float(min(times)), "max_ms": float(max(times))}


def measure(name, vol, ncls, clean, args):
    from cswin_unet_amd import ops
    from cswin_unet_amd.utils import filter_components_host
    dvol = torch.from_numpy(vol).cuda()
    out = torch.empty_like(dvol)
    row = {"volume": name, "shape": list(vol.shape), "ncls": ncls, "rule": "largest", "repeats": args.repeats, "calls_per_window": args.inner}
    row["label"] = device_ms(lambda: ops.connected_components(dvol, ncls, return_sizes=True), args.warmup, args.repeats, args.inner)
    row["label_and_filter"] = device_ms(lambda: ops.filter_components(dvol, ncls, "largest", out=out), args.warmup, args.repeats, args.inner)
    labels, sizes = ops.connected_components(dvol, ncls, return_sizes=True)
    row["components"] = int((sizes > 0).sum())
    row["largest_component"] = int(sizes.max())
    del labels, sizes
    t0 = time.perf_counter()
    want = filter_components_host(vol, ncls, "largest")
    row["host_s"] = time.perf_counter() - t0
    row["equal_to_host"] = bool(torch.equal(out.cpu(), torch.from_numpy(want)))
    row["host_over_device"] = row["host_s"] * 1e3 / row["label_and_filter"]["median_ms"]
    if clean is not None:
        dclean = torch.from_numpy(clean).cuda()
        row["seg_metrics"] = device_ms(lambda: ops.seg_metrics(out, dclean, ncls), args.warmup, args.repeats, args.inner)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", type=int, nargs=3, default=[148, 512, 512])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10, help="calls per timed window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("components_time.py needs a HIP device")
    shape = tuple(args.shape)
    clean, speckled = organ_volume(shape)
    rows = [measure("organs", speckled, 9, clean, args), measure("solid", np.ones(shape, np.uint8), 9, None, args)]
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
