#!/usr/bin/env python3
"""Time the training input pipeline with the augmentation on the device (augment="hip": the workers draw parameters, the
prefetcher uploads raw slices and runs ops.augment_batch, csrc/augment.hip + csrc/resize.hip) against the host path
(augment="host": RandomGenerator's scipy calls in the workers, the code of the parent commit unchanged), and record it in
profiles/augment_timing.txt.

    python tools/augment_time.py [--out FILE] [--repeats 20] [--epochs 5] [--workers 8 16]

The data is a synthetic Synapse-schema set of 240 slices at 512 x 512 in a temporary directory, batches of 24 -> 224 x 224.
  (a) RandomGenerator per sample in this process (seeded), median over the set and per branch
  (b) ops.augment_batch per batch on resident tensors and the upload of one raw batch from pinned memory: host clock around
      work between two device synchronisations, one warm-up (it also fills the rotation maps), median of --repeats
  (c) images/s of DataLoader + trainer._Prefetcher drained with no training step, per mode and worker count: host clock over
      a whole epoch (worker start-up included, as the trainer re-creates its workers every epoch), median of --epochs.  The
      workers never touch the device.  The same is measured with the workers kept alive across epochs
      (persistent_workers=True, which trainer_synapse does not use: it re-seeds its workers every epoch like the reference),
      to separate the rate of the pipeline from what an epoch's start costs, and with the raw batches only uploaded
      ("raw upload only": RawSliceParams in the workers, the prefetcher in its host mode, no ops.augment_batch), to separate
      the kernels from the transport.  Every epoch's seconds are recorded, whole and up to the first batch being complete
      on the device (one synchronisation after the first batch), so the file shows which epochs wait and where.
The step times of BENCH_r03.json are printed beside (c) as the rate the pipeline has to feed.  Run it under `timeout`; an
exception ends the run, so nothing is enqueued after a failed step."""
import argparse
import json
import os
import random
import re
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_SLICES, SIDE, PATCH, BATCH = 240, 512, (224, 224), 24
BRANCH = {0: "none", 1: "rot90 + flip", 2: "rotate"}


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


def host_per_sample(ds_raw):
    """(a): per-sample time of RandomGenerator, with the branch RawSliceParams reports for the same seeds."""
    from cswin_unet_amd.datasets import RandomGenerator, RawSliceParams
    host, raw = RandomGenerator(list(PATCH)), RawSliceParams(list(PATCH))
    times = {k: [] for k in BRANCH}
    for i in range(len(ds_raw)):
        s = ds_raw[i]
        sample = {"image": s["image"], "label": s["label"]}
        random.seed(1000 + i)
        np.random.seed(2000 + i)
        kind = int(raw(dict(sample))["params"][0])
        random.seed(1000 + i)
        np.random.seed(2000 + i)
        t0 = time.perf_counter()
        host(sample)
        times[kind].append((time.perf_counter() - t0) * 1e3)
    return times


MODES = ("host", "hip", "raw upload only")


def drain(train, lists, mode, workers, epochs, device, persistent=False):
    """(c): loader + prefetcher over whole epochs, the loader built as trainer_synapse builds it.  Returns (images/s median,
    min, max) and, per measured epoch, (seconds of the epoch, seconds until the first batch is complete on the device)."""
    from torch.utils.data import DataLoader
    from cswin_unet_amd.datasets import RandomGenerator, RawSliceParams, Synapse_dataset, collate_raw_slices
    from cswin_unet_amd.trainer import _Prefetcher
    hip, augment = mode != "host", "hip" if mode == "hip" else "host"
    ds = Synapse_dataset(train, lists, "train", transform=(RawSliceParams if hip else RandomGenerator)(list(PATCH)))
    loader = DataLoader(ds, batch_size=BATCH, shuffle=True, num_workers=workers, pin_memory=True, drop_last=True,
                        worker_init_fn=lambda w: random.seed(1234 + w), collate_fn=collate_raw_slices if hip else None,
                        persistent_workers=persistent)
    rates, seconds = [], []
    for _ in range(epochs + 1):                                                      # the first epoch is the warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n, first = 0, None
        for img, lab in _Prefetcher(loader, device, augment, PATCH):
            if first is None:
                torch.cuda.synchronize()
                first = time.perf_counter() - t0
            n += img.shape[0]
        torch.cuda.synchronize()
        total = time.perf_counter() - t0
        rates.append(n / total)
        seconds.append((total, first))
    rates = rates[1:]
    return (statistics.median(rates), min(rates), max(rates)), seconds[1:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_timing.txt"))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--workers", type=int, nargs="+", default=[8, 16])
    a = ap.parse_args()

    from cswin_unet_amd import _lib, ops
    from cswin_unet_amd.datasets import RawSliceParams, Synapse_dataset, collate_raw_slices, write_synthetic_synapse
    assert torch.cuda.is_available() and _lib.lib().cswin_device_ok() == 1, "needs a gfx950 HIP device"
    device = torch.device("cuda", 0)
    bench = json.load(open(os.path.join(ROOT, "BENCH_r03.json")))
    step_fp32 = float(bench["parsed"]["ms_per_step"])
    step_bf16 = float(re.search(r'"dtype": "bf16[^{}]*?"ms_per_step": ([0-9.]+)', bench["run"]["stdout_tail"]).group(1))

    with tempfile.TemporaryDirectory() as root:
        train, _, lists = write_synthetic_synapse(root, n_slices=N_SLICES, n_volumes=0, size=SIDE)
        ds_raw = Synapse_dataset(train, lists, "train")
        per = host_per_sample(ds_raw)
        every = [t for v in per.values() for t in v]
        print(f"(a) RandomGenerator per sample: median {statistics.median(every):.2f} ms over {len(every)}", flush=True)

        random.seed(1)
        np.random.seed(2)
        raw = RawSliceParams(list(PATCH))
        batch = collate_raw_slices([raw({"image": ds_raw[i]["image"], "label": ds_raw[i]["label"]}) for i in range(BATCH)])
        pimg, plab, params = batch["image"].pin_memory(), batch["label"].pin_memory(), batch["params"]
        dimg, dlab = pimg.to(device), plab.to(device)
        t_aug = timed_ms(lambda: ops.augment_batch(dimg, dlab, params, PATCH), a.repeats)
        t_up = timed_ms(lambda: (pimg.to(device, non_blocking=True), plab.to(device, non_blocking=True)), a.repeats)
        host_img = torch.empty(BATCH, 1, *PATCH).pin_memory()
        host_lab = torch.empty(BATCH, *PATCH, dtype=torch.int64).pin_memory()
        t_up_host = timed_ms(lambda: (host_img.to(device, non_blocking=True), host_lab.to(device, non_blocking=True)), a.repeats)
        kinds = [int(k) for k in params[:, 0]]
        print(f"(b) augment_batch {fmt(t_aug)}; raw upload {fmt(t_up)}; finished-batch upload {fmt(t_up_host)}", flush=True)

        rates, seconds = {}, {}
        for workers in a.workers:
            for mode in MODES:
                for persistent in (False, True):
                    key = (mode, workers, persistent)
                    rates[key], seconds[key] = drain(train, lists, mode, workers, a.epochs, device, persistent)
                    r = rates[key]
                    print(f"(c) {mode} num_workers={workers} persistent_workers={persistent}: {r[0]:.0f} img/s "
                          f"(min {r[1]:.0f}, max {r[2]:.0f})", flush=True)

    raw_mb = (pimg.numel() * 4 + plab.numel()) / 1e6
    fin_mb = (host_img.numel() * 4 + host_lab.numel() * 8) / 1e6
    lines = [f"augmentation timing: synthetic set of {N_SLICES} slices {SIDE} x {SIDE} -> {PATCH[0]} x {PATCH[1]}, batches of {BATCH}, "
             f"{torch.cuda.get_device_name(0)}",
             f"(a) datasets.RandomGenerator per sample, one process, host clock: median {statistics.median(every):.2f} ms over "
             f"{len(every)} samples ({1e3 / statistics.median(every):.0f} img/s per core at the median, "
             f"{1e3 * len(every) / sum(every):.0f} img/s per core at the mean)"]
    for k, name in BRANCH.items():
        if per[k]:
            lines.append(f"      {name}: median {statistics.median(per[k]):.2f} ms over {len(per[k])} samples")
    lines += [f"(b) ops.augment_batch, one batch of {BATCH} resident raw slices (branches: {kinds.count(0)} none, {kinds.count(1)} rot90 + flip, "
              f"{kinds.count(2)} rotate), median of {a.repeats}: {fmt(t_aug)}  ({t_aug[0] * 1e3 / BATCH:.1f} us per sample)",
              f"    upload of the raw batch from pinned memory ({raw_mb:.1f} MB: float32 images + uint8 labels): {fmt(t_up)}",
              f"    upload of a finished host batch from pinned memory ({fin_mb:.1f} MB: float32 images + int64 labels): {fmt(t_up_host)}",
              f"(c) DataLoader + _Prefetcher drained with no training step, images/s over a whole epoch ({N_SLICES // BATCH} batches, "
              f"worker start-up included), median of {a.epochs} epochs after one warm-up epoch:"]
    for persistent in (False, True):
        if persistent:
            lines.append("    the same with persistent_workers=True (workers forked once; not what trainer_synapse does):")
        for workers in a.workers:
            h, d, u = (rates[m, workers, persistent] for m in MODES)
            lines.append(f"      num_workers={workers}: augment=\"host\" {h[0]:.0f} img/s (min {h[1]:.0f}, max {h[2]:.0f}); "
                         f"augment=\"hip\" {d[0]:.0f} img/s (min {d[1]:.0f}, max {d[2]:.0f}); hip / host {d[0] / h[0]:.2f}x; "
                         f"raw upload only {u[0]:.0f} img/s (min {u[1]:.0f}, max {u[2]:.0f})")
    lines.append("    every measured epoch, in order: seconds of the epoch (seconds until the first batch is complete on the device)")
    for persistent in (False, True):
        for workers in a.workers:
            for mode in MODES:
                lines.append(f"      {mode}, num_workers={workers}, persistent_workers={persistent}: " +
                             ", ".join(f"{t:.2f} ({f:.2f})" for t, f in seconds[mode, workers, persistent]))
    lines += [f"the rate the pipeline has to feed (BENCH_r03.json, {BATCH} images per step): fp32 {step_fp32:.2f} ms = {BATCH * 1e3 / step_fp32:.0f} img/s, "
              f"bf16 mode {step_bf16:.2f} ms = {BATCH * 1e3 / step_bf16:.0f} img/s",
              "claim checked: (c, hip) exceeds (c, host) in this run, workers re-created every epoch as the trainer does: " +
              ", ".join(f"num_workers={w}: {'yes' if rates['hip', w, False][0] > rates['host', w, False][0] else 'NO'}" for w in a.workers)]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
