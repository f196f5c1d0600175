#!/usr/bin/env python3
"""Time the boundary loss's device work at the bench shape (24, 9, 224, 224) and record it in profiles/boundary_loss_timing.txt.

    python tools/boundary_loss_timing.py [--out FILE] [--repeats 30] [--kernel-stats DIR] [--headline FILE]

Every measurement runs in a fresh child process (this script with --child NAME): the child warms up, then takes the median of
--repeats device-event windows of CALLS calls each, divided by CALLS and each ended by a synchronise; clocks are left as found.
A child that fails ends the run: nothing further is started and nothing is written.

  maps_blobs / maps_far: ops.signed_distance_maps (memset + row pass + column pass) on disc-and-rectangle organs and on the
  far-pixel labels, one class pixel in a corner, the column walk's worst case.  The split into the two passes comes from a
  separate profiler run per label set, since the entry point launches both:
      rocprofv3 --kernel-trace --stats --output-format csv -d DIR/blobs -o out -- python tools/boundary_loss_timing.py --one-call blobs
  (and the same with `far`); pass DIR as --kernel-stats.
  sums / bwd, base and boundary: cswin_loss_sums / cswin_loss_bwd (csrc/loss.hip, which this feature leaves textually as it
  was) and cswin_bd_loss_sums / cswin_bd_loss_bwd on the same logits and labels, called directly, LOSS_CALLS calls per window
  (a call is a few dozen microseconds: 20 of them would time the enqueue as much as the kernels).  Their kernel times come
  from a third profiler run, `--one-call loss` into DIR/loss.
  step / step_boundary: one HipEngine step of the bench model (cswin_tiny_224_lite, B 24, hipGraphs) without the option and with
  boundary=0.01, BOTH ON THIS TREE: without the option the step runs the code it ran before the feature, but it is not a run of
  the earlier build.  The only figures from the earlier build are the --headline lines.
--headline FILE: lines of bench.py output (JSON), each prefixed with `parent` or `new`, from alternating runs of the two builds
in one session; their images/s are recorded with the parent's own spread as the noise."""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

B, NCLS, HW = 24, 9, 224
CHILDREN = ("maps_blobs", "maps_far", "sums_base", "sums_boundary", "bwd_base", "bwd_boundary", "step", "step_boundary")
CALLS = 20
LOSS_CALLS = 1000


def device_ms(fn, repeats, calls=CALLS, warmup=5):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / calls)
    return statistics.median(times), min(times), max(times)


def labels(kind):
    import torch
    import sdm_cases as S
    lab = S.blob_labels(B, HW, HW, NCLS, 2025) if kind == "blobs" else S.far_labels(B, HW, HW)
    return torch.from_numpy(lab).cuda()


def loss_calls():
    """(sums, bwd) launchers of the base and of the boundary objective on the same logits and organ labels, and their out tensors."""
    import torch
    from cswin_unet_amd import ops
    from cswin_unet_amd._lib import call, lib, ptr, stream
    g = torch.Generator().manual_seed(2025)
    logits = (2.0 * torch.randn(B, NCLS, HW * HW, generator=g)).cuda()
    lab = labels("blobs")
    n = HW * HW
    phi = ops.signed_distance_maps(lab, NCLS)
    alpha = torch.full((1,), 0.01, device="cuda")
    dl = torch.empty_like(logits)
    made = {}
    for boundary in (False, True):
        nbytes = (lib().cswin_bd_loss_workspace if boundary else lib().cswin_loss_workspace)(B, NCLS, n)
        ws = torch.empty(nbytes // 4 + 4, device="cuda")
        sums, out, coef = torch.zeros(2 + 3 * NCLS, device="cuda"), torch.zeros(4, device="cuda"), torch.zeros(2 * NCLS, device="cuda")
        if boundary:
            do_sums = lambda ws=ws, sums=sums, nbytes=nbytes: call("cswin_bd_loss_sums", ptr(logits), ptr(lab), ptr(phi), None, ptr(sums), ptr(ws), nbytes, B, NCLS, n, stream())
            do_sums()
            call("cswin_bd_loss_finalize", ptr(sums), ptr(out), ptr(coef), float(B * n), NCLS, 0.4, 0.6, ptr(alpha), None, stream())
            do_bwd = lambda coef=coef: call("cswin_bd_loss_bwd", ptr(logits), ptr(lab), ptr(phi), None, ptr(coef), ptr(alpha), None, ptr(dl), 0.4 / (B * n),
                                            0.6 / NCLS, 1.0 / (B * n), B, NCLS, n, stream())
        else:
            do_sums = lambda ws=ws, sums=sums, nbytes=nbytes: call("cswin_loss_sums", ptr(logits), ptr(lab), ptr(sums), ptr(ws), nbytes, B, NCLS, n, 0, stream())
            do_sums()
            call("cswin_loss_finalize", ptr(sums), ptr(out), ptr(coef), float(B * n), NCLS, 0.4, 0.6, None, stream())
            do_bwd = lambda coef=coef: call("cswin_loss_bwd", ptr(logits), ptr(lab), ptr(coef), None, ptr(dl), 0.4 / (B * n), 0.6 / NCLS, B, NCLS, n, 0, stream())
        made["boundary" if boundary else "base"] = (do_sums, do_bwd, out)
    return made


def one_call(kind):
    """Three calls of the maps, or twenty of each loss kernel, for a profiler run."""
    import torch
    from cswin_unet_amd import ops
    if kind == "loss":
        for do_sums, do_bwd, _ in loss_calls().values():
            for _ in range(20):
                do_sums()
                do_bwd()
        torch.cuda.synchronize()
        return 0
    lab = labels(kind)
    for _ in range(3):
        ops.signed_distance_maps(lab, NCLS)
    torch.cuda.synchronize()
    return 0


def child(name, repeats):
    import torch
    from cswin_unet_amd import _lib, ops
    from cswin_unet_amd._lib import call, lib, ptr, stream
    assert torch.cuda.is_available() and lib().cswin_device_ok() == 1, "needs a gfx950 HIP device"
    res = {"name": name, "device": torch.cuda.get_device_name(0)}
    if name.startswith("maps_"):
        lab = labels(name[5:])
        phi = ops.signed_distance_maps(lab, NCLS)
        res["max_abs_phi"] = float(phi.abs().max())
        res["ms"] = device_ms(lambda: ops.signed_distance_maps(lab, NCLS), repeats)
    elif name.startswith(("sums_", "bwd_")):
        do_sums, do_bwd, out = loss_calls()["boundary" if name.endswith("boundary") else "base"]
        res["ms"] = device_ms(do_sums if name.startswith("sums_") else do_bwd, repeats, calls=LOSS_CALLS)
        res["loss"] = float(out[0])
    else:
        from cswin_unet_amd.config import get_config
        from cswin_unet_amd.networks.vision_transformer import CSwinUnet
        from cswin_unet_amd.trainer import DataParallelTrainer, synthetic_batch
        cfg = get_config(os.path.join(ROOT, "configs", "cswin_tiny_224_lite.yaml"))
        torch.manual_seed(0)
        net = CSwinUnet(cfg, img_size=HW, num_classes=NCLS).cuda().train()
        img, _ = synthetic_batch(B, HW, NCLS, 7, "cuda")
        lab = labels("blobs")
        kw = dict(boundary=0.01) if name == "step_boundary" else {}
        tr = DataParallelTrainer(net, NCLS, base_lr=1e-6, max_iterations=100000, use_graph=True, **kw)
        res["ms"] = device_ms(lambda: tr.train_step(img, lab), repeats, calls=5, warmup=3)
        res["loss"] = float(tr.stats[0])
    print("RESULT " + json.dumps(res), flush=True)
    return 0


def kernel_rows(stats_dir, mark="sdm_"):
    """{kernel: average us} of the kernels whose name holds `mark` from a rocprofv3 --stats run's *kernel_stats.csv, or None."""
    files = sorted(glob.glob(os.path.join(stats_dir, "**", "*kernel_stats.csv"), recursive=True))
    if not files:
        return None
    name = lambda r: r["Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0].split("<")[0]
    return {name(r): float(r["AverageNs"]) / 1e3 for r in csv.DictReader(open(files[0])) if mark in r["Name"]}


def headline_lines(path):
    runs = {"parent": [], "new": []}
    for ln in open(path):
        who, _, rest = ln.strip().partition(" ")
        if who in runs and rest.startswith("{"):
            runs[who].append(json.loads(rest))
    return runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "boundary_loss_timing.txt"))
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--child", choices=CHILDREN)
    ap.add_argument("--one-call", choices=("blobs", "far", "loss"))
    ap.add_argument("--kernel-stats", default=None, help="directory with blobs/, far/ and loss/ outputs of separate rocprofv3 --kernel-trace --stats runs of --one-call")
    ap.add_argument("--headline", default=None, help="file of `parent {json}` / `new {json}` bench.py lines from alternating runs")
    a = ap.parse_args()
    if a.one_call:
        return one_call(a.one_call)
    if a.child:
        return child(a.child, a.repeats)
    got = {}
    for name in CHILDREN:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--repeats", str(a.repeats)], capture_output=True, text=True, timeout=400)
        line = next((ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")), None)
        if p.returncode != 0 or line is None:
            print(p.stdout[-2000:], p.stderr[-4000:], f"child {name} failed ({p.returncode}); nothing written", sep="\n")
            return 1
        got[name] = json.loads(line[7:])
        print(name, got[name], flush=True)
    ms = lambda r: f"{r['ms'][0]:.3f} ms (min {r['ms'][1]:.3f}, max {r['ms'][2]:.3f})"
    mb, mf = got["maps_blobs"], got["maps_far"]
    lines = [f"boundary loss timing: B {B}, ncls {NCLS}, {HW} x {HW}, {mb['device']}",
             f"each line: a fresh process, warm-up calls, median of {a.repeats} device-event windows of {CALLS} calls each (the steps: 5), per call, clocks as found",
             "every call reads the same tensors: they may stay cache-resident",
             f"signed distance maps (memset, row pass, column pass; phi 43 MB, g1 22 MB), organs (|phi| up to {mb['max_abs_phi']:.1f}): {ms(mb)}",
             f"signed distance maps, one class pixel in a corner (|phi| up to {mf['max_abs_phi']:.1f}): {ms(mf)}    far / organs: {mf['ms'][0] / mb['ms'][0]:.2f}x"]
    lines.append("  (the far labels leave seven of the nine classes empty: a store of zeros, no walk; the two live classes walk up to 223 rows)")
    if a.kernel_stats:
        for kind in ("blobs", "far"):
            rows = kernel_rows(os.path.join(a.kernel_stats, kind))
            if rows is None:
                lines.append(f"  per-kernel split, {kind}: not measured (no kernel_stats.csv)")
            else:
                lines.append(f"  per-kernel split, {kind} (separate rocprofv3 --kernel-trace --stats run, average of 3 calls): " +
                             ", ".join(f"{k} {v:.1f} us" for k, v in sorted(rows.items())))
    else:
        lines.append("  per-kernel split: not measured")
    sb, sn, bb, bn = got["sums_base"], got["sums_boundary"], got["bwd_base"], got["bwd_boundary"]
    lines += [f"loss entry points on the same logits and organ labels, called directly, windows of {LOSS_CALLS} calls, both on this tree (loss.hip is textually what it was before the feature):",
              f"  cswin_loss_sums {ms(sb)} | cswin_bd_loss_sums {ms(sn)}: {sn['ms'][0] / sb['ms'][0]:.2f}x",
              f"  cswin_loss_bwd {ms(bb)} | cswin_bd_loss_bwd {ms(bn)}: {bn['ms'][0] / bb['ms'][0]:.2f}x"]
    rows = kernel_rows(os.path.join(a.kernel_stats, "loss"), "loss_") if a.kernel_stats else None
    if rows:
        k = lambda n: f"{n} {rows[n]:.1f} us" if n in rows else f"{n} not seen"
        lines.append("  kernel times (separate rocprofv3 --kernel-trace --stats run, average of 20 calls; the sums entry points also launch the slab reduction): " +
                     ", ".join(k(n) for n in ("loss_sums_kernel", "bd_loss_sums_kernel", "loss_bwd_kernel", "bd_loss_bwd_kernel")))
    else:
        lines.append("  kernel times: not measured")
    lines += ["training step, cswin_tiny_224_lite, B 24, hipGraphs, organ labels, both on this tree:",
              f"  without the option (the code the step ran before the feature; not a run of the earlier build): {ms(got['step'])}",
              f"  boundary=0.01: {ms(got['step_boundary'])}    difference {got['step_boundary']['ms'][0] - got['step']['ms'][0]:.3f} ms"]
    if a.headline:
        runs = headline_lines(a.headline)
        ips = {k: [r["value"] for r in v] for k, v in runs.items()}
        lines.append("bench.py headline (the default step; the feature is off), the two builds alternating in one session, images/s:")
        for who in ("parent", "new"):
            lines.append(f"  {who}: " + ", ".join(f"{v:.1f}" for v in ips[who]) + (f"    median {statistics.median(ips[who]):.1f}" if ips[who] else " not measured"))
        if len(ips["parent"]) >= 2 and ips["new"]:
            spread = max(ips["parent"]) - min(ips["parent"])
            diff = statistics.median(ips["new"]) - statistics.median(ips["parent"])
            lines.append(f"  noise (spread of the parent's own runs): {spread:.1f} images/s; new - parent (medians): {diff:+.1f} images/s")
    else:
        lines.append("bench.py headline before and after: not measured")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
