#!/usr/bin/env python3
"""Time ops.intensity_batch (csrc/intensity.hip, with ops.gaussian_blur_each for the blur stage) on a resident batch of
24 x 224 x 224 float32 images, and record it in profiles/intensity_timing.txt beside the 0.320 ms of ops.augment_batch in
profiles/augment_timing.txt.

    python tools/intensity_time.py [--out FILE] [--repeats 20]

Host clock around work between two device synchronisations, one warm-up, median of --repeats.  Mixes of the 24 records:
  preset      one seeded draw of IntensityAugment.nnunet() per repeat -- what a training step meets; the draw (host numpy) is inside
              the timed call, as it is in the prefetcher, and the median is over differing draws
  expected    the preset's probabilities as counts of 24, fixed: 5 samples blur, 2 noise, 4 brightness, 4 contrast, 7 gamma (2 of
              them inverted), spread so that stages overlap on some samples
  every stage each stage alone on all 24 samples, then all stages on all 24
The step times of BENCH_r03.json are printed as what the prefetcher's stream has to fit into.  Run it under `timeout`; an
exception ends the run, so nothing is enqueued after a failed step."""
import argparse
import json
import os
import re
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BATCH, SIDE = 24, 224


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


def fixed_draws(on):
    """24 records with the stages of `on` (name -> indices of the samples that have it) at mid-range parameters."""
    from cswin_unet_amd.datasets import INTENSITY_DRAW
    d = np.zeros(BATCH, INTENSITY_DRAW)
    d["brightness"] = d["contrast"] = d["gamma"] = 1.0
    d["seed"] = np.arange(BATCH, dtype=np.uint64) * np.uint64(7919) + np.uint64(3)
    for name, field, value in (("blur", "sigma", 0.75), ("noise", "noise_std", 0.2), ("brightness", "brightness", 1.1),
                               ("contrast", "contrast", 0.9), ("gamma", "gamma", 1.2)):
        idx = list(on.get(name, ()))
        d["do_" + name][idx], d[field][idx] = True, value
    d["invert"][list(on.get("invert", ()))] = True
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "intensity_timing.txt"))
    ap.add_argument("--repeats", type=int, default=20)
    a = ap.parse_args()

    from cswin_unet_amd import _lib, ops
    from cswin_unet_amd.datasets import IntensityAugment
    assert torch.cuda.is_available() and _lib.lib().cswin_device_ok() == 1, "needs a gfx950 HIP device"
    device = torch.device("cuda", 0)
    bench = json.load(open(os.path.join(ROOT, "BENCH_r03.json")))
    step_fp32 = float(bench["parsed"]["ms_per_step"])
    step_bf16 = float(re.search(r'"dtype": "bf16[^{}]*?"ms_per_step": ([0-9.]+)', bench["run"]["stdout_tail"]).group(1))

    x = torch.from_numpy(np.random.default_rng(0).random((BATCH, 1, SIDE, SIDE)).astype(np.float32)).to(device)
    every = range(BATCH)
    mixes = [("expected mix (5 blur, 2 noise, 4 brightness, 4 contrast, 7 gamma of which 2 inverted)",
              fixed_draws(dict(blur=(0, 5, 10, 15, 20), noise=(1, 12), brightness=(2, 5, 13, 21), contrast=(3, 10, 14, 22),
                               gamma=(4, 5, 11, 12, 16, 19, 23), invert=(11, 19)))),
             ("nothing on (one copy launch)", fixed_draws({}))]
    mixes += [(f"{name} alone on all {BATCH}", fixed_draws({name: every})) for name in ("blur", "noise", "brightness", "contrast", "gamma")]
    mixes.append((f"every stage on all {BATCH}", fixed_draws(dict(blur=every, noise=every, brightness=every, contrast=every, gamma=every,
                                                                   invert=range(0, BATCH, 2)))))
    spec, rng = IntensityAugment.nnunet(), np.random.default_rng(1234)
    t_preset = timed_ms(lambda: ops.intensity_batch(x, spec.draw(BATCH, rng)), a.repeats, warmup=3)
    t_draw = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        spec.draw(BATCH, rng)
        t_draw.append((time.perf_counter() - t0) * 1e3)
    lines = [f"intensity augmentation timing: ops.intensity_batch on a resident batch of {BATCH} x {SIDE} x {SIDE} float32, "
             f"{torch.cuda.get_device_name(0)}; host clock between two synchronisations, median of {a.repeats} after a warm-up",
             f"  preset, a fresh draw of IntensityAugment.nnunet() per call (draw included): {fmt(t_preset)}",
             f"    the draw alone (host): median {statistics.median(t_draw):.3f} ms"]
    print(lines[-2], flush=True)
    results = {}
    for name, draws in mixes:
        results[name] = timed_ms(lambda: ops.intensity_batch(x, draws), a.repeats)
        lines.append(f"  {name}: {fmt(results[name])}")
        print(lines[-1], flush=True)
    expected, full = results[mixes[0][0]], results[mixes[-1][0]]
    lines += [f"beside it: ops.augment_batch on the same batch size, 0.320 ms (profiles/augment_timing.txt)",
              f"what the prefetcher's stream has to fit into (BENCH_r03.json, one batch per step): fp32 {step_fp32:.2f} ms, bf16 mode {step_bf16:.2f} ms",
              f"  expected mix: {100 * expected[0] / step_fp32:.1f} % of the fp32 step, {100 * expected[0] / step_bf16:.1f} % of the bf16 step",
              f"  every stage on every sample: {100 * full[0] / step_fp32:.1f} % of the fp32 step, {100 * full[0] / step_bf16:.1f} % of the bf16 step"]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
