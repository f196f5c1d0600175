#!/usr/bin/env python3
"""The stripe-attention fwd+bwd kernels of one stage, called directly.

    attn_one.py stage [reps]        run stage 1 .. 4 of the 224 model (batch 24, fp32) a few times, for rocprofv3 --pmc passes
    attn_one.py time [windows]      time forward and backward at those four shapes and at stage 3 of the 384 model (batch 8: 288-token
                                    windows, attn_fwd_kernel and the two-pass backward), each in fp32 (mode 0) and mode 7

`time`: one process; after three warm-up calls every repetition times one device-event window of CALLS = 20 back-to-back calls
per case (one call is 15 - 120 us, too short a window by itself), the cases in turn, each window ended by a synchronise; median
(min, max) per call and case in microseconds.  Clocks are left as found.  To compare two builds, run it once per build in turn,
each run a fresh process."""
import os, sys, ctypes, statistics
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cswin_unet_amd._lib import call, lib, ptr, stream
dev = "cuda"
E, heads, split = 64, [2, 4, 8, 16], [1, 2, 7, 7]


def stage_shape(si, batch=24):
    """(batch, reso, C, split, idx, heads per branch) of stage si + 1 of the 224 model"""
    single = si == 3
    return batch, 56 >> si, E << si, split[si], ([-1] if single else [0, 1]), ([heads[si]] if single else [heads[si] // 2] * 2)


def setup(batch, reso, C, sp, idx, hb, mode=0):
    """(forward, backward) closures on random inputs in the storage format of `mode`"""
    L, nb, cb = reso * reso, len(idx), C // len(idx)
    qdt, ydt = (torch.bfloat16 if mode & 1 else torch.float32), (torch.bfloat16 if mode & 2 else torch.float32)
    qkv = torch.randn(batch, L, 3 * C, device=dev).to(qdt); w = [torch.randn(cb, 9, device=dev) / 3 for _ in idx]; b = [torch.randn(cb, device=dev) * .02 for _ in idx]
    dy = torch.randn(batch, L, C, device=dev); y = torch.empty(batch, L, C, device=dev, dtype=ydt); y0 = torch.empty_like(y); lse = torch.empty(batch, sum(hb), L, device=dev)
    dqkv = torch.empty_like(qkv); dw = [torch.empty_like(t) for t in w]; db = [torch.empty_like(t) for t in b]
    ia, ha = (ctypes.c_int * nb)(*idx), (ctypes.c_int * nb)(*hb)
    pa = lambda ts: (ctypes.c_void_p * nb)(*[t.data_ptr() for t in ts])
    nbytes = lib().cswin_attn_bwd_workspace(batch, reso, C, nb, ha, ia, sp); ws = torch.empty(nbytes // 4 + 4, device=dev)
    fwd = lambda: call("cswin_attn_fwd", ptr(qkv), pa(w), pa(b), ptr(y), ptr(y0), ptr(lse), batch, reso, C, nb, ha, ia, sp, 0.0, 0.0, 0, None, mode, stream())
    bwd = lambda: call("cswin_attn_bwd", ptr(qkv), pa(w), pa(b), ptr(lse), ptr(y0), ptr(dy), ptr(dqkv), pa(dw), pa(db), ptr(ws), nbytes, batch, reso, C, nb,
                       ha, ia, sp, 0.0, None, 0.0, 0, None, mode, stream())
    return fwd, bwd


CALLS = 20


def time_all(repeats):
    shapes = [(f"224 stage {si + 1}", stage_shape(si)) for si in range(4)] + [("384 stage 3", (8, 24, 256, 12, [0, 1], [4, 4]))]
    cases = []
    for name, shape in shapes:
        for mode in (0, 7):
            fwd, bwd = setup(*shape, mode=mode)
            cases += [(f"{name} mode {mode} fwd", fwd), (f"{name} mode {mode} bwd", bwd)]
    for _, fn in cases:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in cases]
    for _ in range(repeats):
        for t, (_, fn) in zip(times, cases):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(CALLS):
                fn()
            e1.record()
            torch.cuda.synchronize()
            t.append(1e3 * e0.elapsed_time(e1) / CALLS)
    for (name, _), t in zip(cases, times):
        print(f"{name}: {statistics.median(t):.1f} us (min {min(t):.1f}, max {max(t):.1f})")


if sys.argv[1] == "time":
    time_all(int(sys.argv[2]) if len(sys.argv) > 2 else 50)
else:
    si = int(sys.argv[1]) - 1; reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    shape = stage_shape(si)
    fwd, bwd = setup(*shape)
    for _ in range(reps):
        fwd()
        bwd()
    torch.cuda.synchronize()
    L, C, batch = shape[1] ** 2, shape[2], shape[0]
    print("algorithmic MB: fwd", 16 * L * C * batch / 1e6, "bwd", 28 * L * C * batch / 1e6)
