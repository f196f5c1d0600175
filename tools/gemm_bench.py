#!/usr/bin/env python3
"""Device-time micro-benchmark of the GEMM family on the model's shapes (GPU box): each entry point is captured 20x
into a hipGraph and replayed, so host launch overhead is excluded.  CSWIN_GEMM_TILE=1|2|3 forces a tile shape."""
import os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cswin_unet_amd._lib import call, lib, ptr, stream, precision

def timed(fn, reps=20, rounds=5):
    fn(); torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps): fn()
    g.replay(); torch.cuda.synchronize()
    best = 1e9
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); g.replay(); e1.record(); torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1e-3 / reps)
    return best

B = int(os.environ.get("BATCH", "24"))
import cswin_unet_amd
cswin_unet_amd.set_matmul_precision(os.environ.get("MATMUL", "fp32"))      # MATMUL=bf16: bf16 operands (streaming-bound proxy)

def conv_mode():
    """`gemm_bench.py conv`: the three conv entry points at the convolutions of configs/cswin_tiny_224_lite.yaml (E = 64, 224 x 224):
    the 7x7 stride-4 stem on 4-channel tokens (no input gradient), the three stride-2 merges, the stride-1 CARAFE encoders of the
    decoder and of the head, whose input gradient is a forward convolution of dy with the mirrored weights, as ops.conv_tokens runs it."""
    E = 64
    cases = [("stem", 224, 4, E, 7, 4, 2)]
    cases += [(f"merge{i+1}", 56 >> i, E << i, 2 * E << i, 3, 2, 1) for i in range(3)]
    cases += [(f"up{4-i}.enc", 7 << i, 2 * E >> i, 36, 3, 1, 1) for i in range(3)] + [("head.enc", 56, E // 4, 144, 3, 1, 1)]
    R = lambda *s: torch.randn(*s, device="cuda")
    for name, side, Cin, Cout, ks, stride, pad in cases:
        O = (side + 2 * pad - ks) // stride + 1
        x, dy, b, w = R(B, side * side, Cin), R(B, O * O, Cout), R(Cout), R(Cout, Cin, ks, ks)
        wp, wpt, wf = torch.empty(Cout, ks * ks, Cin, device="cuda"), torch.empty(ks * ks, Cout, Cin, device="cuda"), torch.empty(Cin, ks * ks, Cout, device="cuda")
        call("cswin_conv_weight_permute", ptr(w), ptr(wp), ptr(wpt), Cout, Cin, ks, Cin, stream())
        call("cswin_conv_weight_flipT", ptr(w), ptr(wf), Cout, Cin, ks, stream())
        y, dx, dw, db = torch.empty(B, O * O, Cout, device="cuda"), torch.empty_like(x), torch.empty_like(w), torch.empty(Cout, device="cuda")
        nbytes = lib().cswin_conv_tok_bwd_weight_workspace(B, side, side, Cin, Cout, ks, stride, pad)
        ws = torch.empty(nbytes // 4 + 4, device="cuda")
        geo = (B, side, side, Cin, Cout, ks, stride, pad)
        tf = timed(lambda: call("cswin_conv_tok_fwd", ptr(x), ptr(wp), ptr(b), ptr(y), *geo, precision(), stream()))
        if name == "stem":
            tdx = 0.0
        elif stride == 1:
            tdx = timed(lambda: call("cswin_conv_tok_fwd", ptr(dy), ptr(wf), None, ptr(dx), B, side, side, Cout, Cin, ks, 1, pad, precision(), stream()))
        else:
            tdx = timed(lambda: call("cswin_conv_tok_bwd_data", ptr(dy), ptr(wpt), ptr(dx), *geo, precision(), stream()))
        tdw = timed(lambda: call("cswin_conv_tok_bwd_weight", ptr(dy), ptr(x), ptr(dw), ptr(db), ptr(ws), nbytes, *geo, 1, None, precision(), stream()))
        fl = 2.0 * B * O * O * Cout * ks * ks * Cin
        tf_s = lambda t: f"{t*1e6:7.1f}us {fl/t/1e12:6.1f}TF" if t else "      -              "
        print(f"{name:9s} {side:3d}x{side:<3d} Cin={Cin:4d} Cout={Cout:4d} k{ks} s{stride}  fwd {tf_s(tf)} | dx {tf_s(tdx)} | dw {tf_s(tdw)}")

if sys.argv[1:2] == ["conv"]:
    conv_mode()
    sys.exit(0)
shapes = []
for si, (L, C) in enumerate([(3136, 64), (784, 128), (196, 256), (49, 512)]):
    M = B * L
    shapes += [(f"s{si+1}.qkv", M, 3 * C, C), (f"s{si+1}.proj", M, C, C), (f"s{si+1}.fc1", M, 4 * C, C), (f"s{si+1}.fc2", M, C, 4 * C)]
tot = {"fwd": 0, "dx": 0, "dw": 0}
flops = 0
counts = {"s1": 2, "s2": 4, "s3": 18, "s4": 2}
for name, M, N, K in shapes:
    x = torch.randn(M, K, device="cuda"); w = torch.randn(N, K, device="cuda"); b = torch.randn(N, device="cuda")
    dy = torch.randn(M, N, device="cuda"); y = torch.empty(M, N, device="cuda"); dx = torch.empty(M, K, device="cuda")
    dw = torch.empty(N, K, device="cuda"); db = torch.empty(N, device="cuda")
    nbytes = lib().cswin_linear_bwd_weight_workspace(M, N, K)
    ws = torch.empty(nbytes // 4 + 4, device="cuda")
    tf = timed(lambda: call("cswin_linear_fwd", ptr(x), None, 0, ptr(w), ptr(b), ptr(y), None, None, None, 1, M, N, K, precision(), 0, stream()))
    tdx = timed(lambda: call("cswin_linear_bwd_data", ptr(dy), ptr(w), ptr(dx), None, 0, None, None, 1, None, M, N, K, precision(), 0, stream()))
    tdw = timed(lambda: call("cswin_linear_bwd_weight", ptr(dy), ptr(x), None, 0, None, 1, ptr(dw), ptr(db), ptr(ws), nbytes, M, N, K, None, precision(), stream()))
    fl = 2.0 * M * N * K
    c = counts[name[:2]]
    tot["fwd"] += c * tf; tot["dx"] += c * tdx; tot["dw"] += c * tdw; flops += 3 * c * fl
    by = 4.0 * (M * K + N * K + M * N)        # minimal bytes of one pass (each operand once)
    print(f"{name:8s} M={M:6d} N={N:5d} K={K:5d}  fwd {tf*1e6:7.1f}us {fl/tf/1e12:6.1f}TF {by/tf/1e12:4.2f}TB/s | dx {tdx*1e6:7.1f}us {fl/tdx/1e12:6.1f}TF {by/tdx/1e12:4.2f}TB/s | dw {tdw*1e6:7.1f}us {fl/tdw/1e12:6.1f}TF {by/tdw/1e12:4.2f}TB/s")
s = sum(tot.values())
print("per-step totals (ms):", {k: round(v * 1e3, 3) for k, v in tot.items()}, "sum", round(s * 1e3, 3), f"-> {flops/s/1e12:.1f} TF/s over {flops/1e9:.0f} GFLOP")
