"""The nn.Linear GEMM family away from the models' shapes: cswin_linear_fwd, cswin_linear_bwd_data, cswin_linear_bwd_weight,
cswin_linear_bwd_weight_batch and cswin_linear_bwd_tail at every fp32 tile configuration (64x32x32, 64x32x64 KW2, 64x64x32,
64x64x64 KW2 / KW4), both loader widths, both epilogue widths, ragged tiles and slabs, every form of the header, the bf16 tiled
loops, the LDS-DMA kernels of gemm16.hip (2 / 3 stages, half last step, 128-row tile) and both tiles of wgrad16.hip.

The reference is linear_ref below: float64 on the CPU, autograd for the gradients.  The metric is test_gpu_parity's
max|got - ref| / rms(ref), the bound its fp32 RTOL = 1e-3 -- also for the bf16 kernels, which are fed bf16-valued operands:
the operand rounding is then the identity, every product is exact in fp32 and only the fp32 summation separates the result
from float64.  Every output is a view into a NaN-filled buffer whose guard words must survive, every weight-gradient workspace
is exactly as large as cswin_linear_bwd_weight_workspace() says, and every measured error is appended to test_gpu_parity's
error log under a tag that names the case.  The entry points are called through cswin_unet_amd._lib, not through ops.py: only
a direct call can pass an operand 4 bytes off a 16-byte boundary, an exact workspace or a chosen io_bf16.

The tests at the top need no GPU: they check the reference against an independently written formulation, show that the bound
sees the bugs these shapes are meant to catch, pin the transcription of the launch rules (gemm_plan) to the case tables and to
the library's own workspace query."""
import ctypes
import functools
import math
import os

import numpy as np
import pytest
import torch

from oracle.determ import det_normal

from test_gpu_parity import BF16_RTOL, LOG, RTOL        # the fp32 bound, the bf16-operand bound and the error log, none of them new
from test_gpu_shapes import D, measure                  # float64 leaf; max|got - ref| / rms(ref) in float64, printed and logged
from test_gpu_attn_shapes import GUARD, Guarded, settle  # NaN guard bands round an output; their check after a launch

gpu = pytest.mark.gpu
DEV = "cuda"
# read once per process by the library (csrc/tuning.h): any of them voids gemm_plan
TUNING_PREFIXES = ("CSWIN_GEMM_", "CSWIN_WGRAD16", "CSWIN_W16_", "CSWIN_GEMM16")


def cdiv(a, b):
    return -(-a // b)


def bf16_round(a):
    """Nearest-even bf16 rounding of a float32 numpy array, returned as float32 numpy."""
    return torch.from_numpy(np.ascontiguousarray(a)).float().bfloat16().float().numpy()


# ------------------------------------------------------------------------------------------------
# float64 reference of the Linear family (include/cswin_hip.h), differentiable by autograd
# ------------------------------------------------------------------------------------------------
def gelu64(t):
    return 0.5 * t * (1.0 + torch.erf(t / math.sqrt(2.0)))


def linear_ref(x, w, bias=None, dy=None, *, x2=None, residual=None, row_scale=None, rows_per_sample=1, gelu_pre=None, add=None, _wrong=None):
    """Every form of the header in one graph.  z = [x | x2] (x = GELU_erf(gelu_pre) when gelu_pre is given), s[m] =
    row_scale[m // rows_per_sample] (1 without), acc = z w^T + bias:
        y = residual + s acc,   y_act = GELU_erf(y)                                          cswin_linear_fwd
    and, with L = sum(y o dy) + sum(z o add), by autograd
        dx | dx2 = dL/dz = add + (s dy) w       dpre = dL/dgelu_pre = (s dy) w o gelu'(gelu_pre)     cswin_linear_bwd_data
        dw = (s dy)^T [x | x2]                  dbias = column sums of s dy                          cswin_linear_bwd_weight
    Arguments are numpy arrays or tensors; absent ones are None.  Returns a dict of float64 tensors.
    _wrong (the sensitivity test alone): "drop_last_k" (forward reduction), "drop_last_n" (data-gradient reduction),
    "drop_last_m" (weight-gradient reduction), "scale_boundary" (sample boundaries one row early), "seam" (the first column
    after the concat seam read one column late)."""
    leaf = lambda a: None if a is None else D(a)
    const = lambda a: None if a is None else D(a).detach()
    x, x2, w, bias, pre = leaf(x), leaf(x2), leaf(w), leaf(bias), leaf(gelu_pre)
    residual, add, dy, row_scale = const(residual), const(add), const(dy), const(row_scale)
    src = gelu64(pre) if pre is not None else x
    z = src if x2 is None else torch.cat([src, x2], 1)
    M = z.shape[0]
    zz, ww = z, w
    if _wrong == "drop_last_k":
        zz, ww = z[:, :-1], w[:, :-1]
    if _wrong == "seam":
        zz = torch.cat([src, x2[:, 1:2], x2[:, 1:]], 1)
    acc = zz @ ww.t()
    if bias is not None:
        acc = acc + bias
    if row_scale is not None:
        m = torch.arange(M) + (1 if _wrong == "scale_boundary" else 0)
        acc = row_scale[(m // rows_per_sample).clamp(max=len(row_scale) - 1)][:, None] * acc
    y = acc if residual is None else residual + acc
    out = dict(y=y.detach(), y_act=gelu64(y).detach())
    if dy is None:
        return out
    if _wrong == "drop_last_n":
        dy = torch.cat([dy[:, :-1], torch.zeros_like(dy[:, -1:])], 1)
    if _wrong == "drop_last_m":
        dy = torch.cat([dy[:-1], torch.zeros_like(dy[-1:])], 0)
    loss = (y * dy).sum()
    if add is not None:
        loss = loss + (z * add).sum()
    loss.backward()
    out["dw"] = w.grad
    if bias is not None:
        out["dbias"] = bias.grad
    if pre is not None:
        out["dpre"] = pre.grad
    else:
        out["dx"] = x.grad
    if x2 is not None:
        out["dx2"] = x2.grad
    return out


def linear_loops(x, w, bias, dy, x2, residual, row_scale, rows_per_sample, gelu_pre, add):
    """The same quantities without autograd, torch.cat or broadcasting over rows: numpy float64, one sample at a time, the two
    sources multiplied separately, gelu' from its closed form.  Every argument is given."""
    f = lambda a: np.asarray(a, np.float64)
    x2, w, bias, dy, residual, add = f(x2), f(w), f(bias), f(dy), f(residual), f(add)
    erf = np.vectorize(math.erf)
    if gelu_pre is not None:
        pre = f(gelu_pre)
        src = 0.5 * pre * (1.0 + erf(pre / math.sqrt(2.0)))
        dgelu = 0.5 * (1.0 + erf(pre / math.sqrt(2.0))) + pre * np.exp(-0.5 * pre * pre) / math.sqrt(2.0 * math.pi)
    else:
        src, dgelu = f(x), 1.0
    M, K0 = src.shape
    y, dsrc, dx2 = np.zeros_like(dy), np.zeros_like(src), np.zeros_like(x2)
    dw, dbias = np.zeros_like(w), np.zeros_like(bias)
    for b in range(cdiv(M, rows_per_sample)):
        for m in range(b * rows_per_sample, min(M, (b + 1) * rows_per_sample)):
            acc = w[:, :K0] @ src[m] + w[:, K0:] @ x2[m] + bias
            y[m] = residual[m] + float(row_scale[b]) * acc
            g = float(row_scale[b]) * dy[m]
            dsrc[m] = g @ w[:, :K0] + add[m, :K0]
            dx2[m] = g @ w[:, K0:] + add[m, K0:]
            dw[:, :K0] += np.outer(g, src[m])
            dw[:, K0:] += np.outer(g, x2[m])
            dbias += g
    out = dict(y=y, y_act=0.5 * y * (1.0 + erf(y / math.sqrt(2.0))), dx2=dx2, dw=dw, dbias=dbias)
    out["dpre" if gelu_pre is not None else "dx"] = dsrc * dgelu
    return out


# ------------------------------------------------------------------------------------------------
# launch plan
# ------------------------------------------------------------------------------------------------
# A transcription of the host rules of cswin_unet_amd/csrc/gemm_plan.h, the header gemm.hip, gemm16.hip and wgrad16.hip launch from,
# with no tuning variable set: k_groups, one_split, choose_split (stand-alone target 768 workgroups, a batch's per-problem target
# 1024 / n), choose_tile (the cost model between the 64x64 and the 64x32 tile at a penalty of 1.20, the k-tile and wave groups of
# each, the weight gradients' KW >= 2 from 256 rows per slab, the bf16 loops' 64x64x64), the loader and epilogue widths of each
# entry point's plan, wgrad_workspace_bytes, wgrad_aligned and batch_route's ride / fast / wgrad16 decisions, gemm16_accepts and
# gemm16_plan's stage count and 128-row tile, the split count and the dma predicate of the wgrad16 route.
# tests/test_gemm_plan_host.py holds it to the header line for line (tools/gemm_plan_check.cpp), on these tables and on sweeps.
def k_groups(blocks, r_len):
    if blocks < 320 and r_len >= 512:
        return 4
    if blocks < 640 and r_len >= 256:
        return 2
    return 1


def one_split(R):
    return cdiv(R, 64) * 64


def choose_split(M, out_rows, out_cols, target=768):
    """(splits, rows per split) of a weight gradient's reduction over M."""
    tiles = cdiv(out_rows, 64) * cdiv(out_cols, 64)
    s = max(1, target // tiles)
    s = max(1, min(s, cdiv(M, 128)))
    rps = cdiv(cdiv(M, s), 8) * 8
    return cdiv(M, rps), rps


def wgrad_workspace_bytes(M, N, K):
    return max(choose_split(M, N, K)[0], choose_split(M, N, K, 1024)[0]) * (N * K + N) * 4


def tiled_config(Mo, No, R, splits, rps, wgrad, precision):
    """(BM, BN, BK, KW) of launch_gemm for Mo x No outputs and a reduction of R in `splits` slices of rps."""
    blocks = lambda bm, bn: cdiv(Mo, bm) * cdiv(No, bn) * splits
    cost = lambda bm, bn, pen: float((blocks(bm, bn) + 255) // 256) * bm * bn * pen
    narrow = splits == 1 and cost(64, 32, 1.20) < cost(64, 64, 1.0)
    r_len = min(rps, R)
    if precision == 1:
        return (64, 64, 64, 2 if k_groups(blocks(64, 64), r_len) >= 2 or (wgrad and r_len >= 256) else 1)
    if narrow:
        return (64, 32, 64, 2) if k_groups(blocks(64, 32), r_len) >= 2 else (64, 32, 32, 1)
    kw = k_groups(blocks(64, 64), r_len)
    if wgrad and r_len >= 256 and kw < 2:
        kw = 2
    return (64, 64, 64, kw) if kw >= 2 else (64, 64, 32, 1)


def _tiled(Mo, No, R, splits, rps, wgrad, precision, vec, store):
    bm, bn, bk, kw = tiled_config(Mo, No, R, splits, rps, wgrad, precision)
    return dict(kernel="tiled", wgrad=wgrad, tile=(bm, bn), bk=bk, kw=kw, vec=4 if vec else 1, store=4 if store else 1, splits=splits, rows=rps,
                last=R - (splits - 1) * rps, ragged=Mo % bm != 0 and No % bn != 0 and (R - (splits - 1) * rps) % bk != 0)


def _gemm16(M, NO, R):
    tiles = cdiv(M, 64) * cdiv(NO, 64)
    return dict(kernel="gemm16", tile=(128 if tiles > 768 else 64, 64), bk=64, kw=1, vec=4, store=4, splits=1, rows=one_split(R), last=R,
                stages=3 if tiles > 768 or cdiv(R, 64) >= 3 else 2, last_step=R % 64 or 64)


def gemm16_accepts(NO, R, aligned, store):
    return R % 64 in (0, 32) and R >= 64 and NO % 8 == 0 and aligned and store


def gemm_plan(entry, M, N, K, *, k_split=0, off=(), form="plain", precision=0, io=0):
    """What one call of cswin_linear_fwd ("fwd"), cswin_linear_bwd_data ("dgrad") or the stand-alone cswin_linear_bwd_weight
    ("dw") launches: kernel, tile, k-tile (bk), wave groups (kw), loader width (vec), epilogue width (store), splits, rows per
    split and the length of the last split.  off: the operands based 4 bytes off a 16-byte boundary, by their names in the
    header (only those the form has count).  form: fwd plain / gelu / res; dgrad plain / gelu / add / split; k_split != 0 is
    the concat input of fwd and dw and the dx | dx2 seam of dgrad's split form."""
    on = lambda *names: not any(n in off for n in names)
    if entry == "fwd":
        vec = K % 4 == 0 and k_split % 4 == 0 and on("x", "w") and (not k_split or on("x2"))
        store = N % 4 == 0 and on("y", "bias") and (form != "gelu" or on("y_act")) and (form != "res" or on("residual"))
        if precision == 1 and (io & 5) == 5 and not k_split and gemm16_accepts(N, K, on("x", "w"), store):
            return _gemm16(M, N, K)
        return _tiled(M, N, K, 1, one_split(K), False, precision, vec, store)
    if entry == "dgrad":
        vec = N % 4 == 0 and K % 4 == 0 and on("dy", "w")
        store = K % 4 == 0 and on("dx") and (form != "gelu" or on("gelu_pre")) and (form != "add" or on("add")) and \
            (form != "split" or (k_split % 4 == 0 and on("dx2")))
        if precision == 1 and (io & 5) == 5 and form in ("plain", "gelu") and gemm16_accepts(K, N, on("dy", "w"), store):
            return _gemm16(M, K, N)
        return _tiled(M, K, N, 1, one_split(N), False, precision, vec, store)
    assert entry == "dw"
    aligned = N % 4 == 0 and K % 4 == 0 and on("dy", "x", "workspace")
    if precision == 1 and not k_split and aligned:
        return wgrad16_plan([(M, N, K)], [io], [None])[0]
    splits, rps = choose_split(M, N, K)
    vec = N % 4 == 0 and K % 4 == 0 and k_split % 4 == 0 and on("dy", "x") and (not k_split or on("x2"))
    return _tiled(N, K, M, splits, rps, True, precision, vec, K % 4 == 0 and N % 4 == 0 and on("workspace"))


def wgrad16_plan(problems, ios, samples):
    """The wgrad16 path of a batch.  samples[i]: rows_per_sample of a problem with a row scale, else None."""
    work = sum(float(M) * cdiv(N, 128) * cdiv(K, 128) for M, N, K in problems)
    plans = []
    for (M, N, K), io, rps_sample in zip(problems, ios, samples):
        tiles = cdiv(N, 128) * cdiv(K, 128)
        s = int(768 * (float(M) * tiles / work) / tiles + 0.5)
        s = min(s, wgrad_workspace_bytes(M, N, K) // ((N * K + N) * 4), M // 64)
        s = max(s, 1)
        rows = cdiv(cdiv(M, s), 32) * 32
        splits = cdiv(M, rows)
        dma = io == 3 and M % 32 == 0 and rows % 32 == 0 and N % 8 == 0 and K % 8 == 0 and (rps_sample is None or rows // rps_sample + 2 <= 64)
        plans.append(dict(kernel="wgrad16", tile=(128, 128), bk=32, kw=1, vec=4, store=4, splits=splits, rows=rows, last=M - (splits - 1) * rows, dma=dma))
    return plans


def batch_plan(problems, *, precision=0, ios=None, samples=None, off_workspace=(), tail=None, tail_off=()):
    """cswin_linear_bwd_weight_batch / cswin_linear_bwd_tail: (one plan per problem, the tail's data-gradient plan or None).
    off_workspace: indices of the problems whose workspace is 4 bytes off; tail = (M, N, K) of the data gradient, tail_off its
    misaligned operands."""
    n = len(problems)
    ios, samples = ios or [0] * n, samples or [None] * n
    ok = [N % 4 == 0 and K % 4 == 0 and i not in off_workspace for i, (M, N, K) in enumerate(problems)]
    fast = all(ok)
    dplan = None
    if tail:
        tM, tN, tK = tail
        ride = fast and precision == 0 and tN % 4 == 0 and tK % 4 == 0 and not any(o in tail_off for o in ("dy", "w", "dx"))
        dplan = dict(kernel="tail", tile=(64, 64), bk=64, kw=2, vec=4, store=4, splits=1, rows=one_split(tN), last=tN) if ride else \
            gemm_plan("dgrad", tM, tN, tK, off=tail_off, precision=precision)
    if not fast:
        return [gemm_plan("dw", M, N, K, off=("workspace",) if i in off_workspace else (), precision=precision, io=ios[i])
                for i, (M, N, K) in enumerate(problems)], dplan
    if precision == 1:
        return wgrad16_plan(problems, ios, samples), dplan
    plans = []
    for M, N, K in problems:
        splits, rps = choose_split(M, N, K, 1024 // n)
        assert splits * (N * K + N) * 4 <= wgrad_workspace_bytes(M, N, K)
        plans.append(dict(kernel="batch", tile=(64, 64), bk=64, kw=2, vec=4, store=4, splits=splits, rows=rps, last=M - (splits - 1) * rps))
    return plans, dplan


def plan_str(p):
    if p["kernel"] == "gemm16":
        return f"gemm16 {p['tile'][0]}x64 S{p['stages']} last{p['last_step']}"
    slabs = f" {p['splits']}x{p['rows']}({p['last']})"
    if p["kernel"] == "wgrad16":
        return ("wgrad16 dma" if p["dma"] else "wgrad16 reg") + slabs
    s = f"{p['tile'][0]}x{p['tile'][1]}x{p['bk']} KW{p['kw']} V{p['vec']} E{p['store']}"
    return s + slabs if p.get("wgrad", True) else s


# ------------------------------------------------------------------------------------------------
# case tables
# ------------------------------------------------------------------------------------------------
# (A) fp32.  ((M, N, K), operands 4 bytes off a 16-byte boundary) and beside each row what the rules give for the plain forms of
# cswin_linear_fwd, cswin_linear_bwd_data and the stand-alone cswin_linear_bwd_weight: tile x k-tile, wave groups, loader width V,
# epilogue width E, and for the weight gradient splits x rows per split (last split).  The figures are computed from the rules,
# not read off a device; test_case_tables_reach_every_configuration holds gemm_plan to them.
CASES = [
    (((3, 4, 8), ()),           ("64x32x32 KW1 V4 E4", "64x32x32 KW1 V4 E4", "64x32x32 KW1 V4 E4 1x8(3)")),        # R < k-tile
    (((1, 9, 64), ()),          ("64x32x32 KW1 V4 E1", "64x32x32 KW1 V1 E4", "64x32x32 KW1 V1 E1 1x8(1)")),        # one row
    (((129, 65, 33), ()),       ("64x32x32 KW1 V1 E1", "64x32x32 KW1 V1 E1", "64x64x32 KW1 V1 E1 2x72(57)")),
    (((70, 40, 260), ()),       ("64x32x64 KW2 V4 E4", "64x32x32 KW1 V4 E4", "64x32x32 KW1 V4 E4 1x72(70)")),      # R % 64 = 4
    (((70, 40, 261), ()),       ("64x32x64 KW2 V1 E4", "64x32x32 KW1 V1 E1", "64x32x32 KW1 V1 E1 1x72(70)")),      # scalar loads, vector stores
    (((70, 42, 259), ()),       ("64x32x64 KW2 V1 E1", "64x32x32 KW1 V1 E1", "64x32x32 KW1 V1 E1 1x72(70)")),
    (((800, 644, 100), ()),     ("64x64x32 KW1 V4 E4", "64x32x64 KW2 V4 E4", "64x64x32 KW1 V4 E4 7x120(80)")),
    (((801, 640, 260), ()),     ("64x64x64 KW2 V4 E4", "64x32x64 KW2 V4 E4", "64x64x32 KW1 V4 E4 7x120(81)")),
    (((770, 650, 516), ()),     ("64x64x64 KW4 V4 E1", "64x32x64 KW2 V1 E4", "64x64x32 KW1 V1 E1 7x112(98)")),     # vector loads, scalar stores
    (((801, 642, 261), ()),     ("64x64x64 KW2 V1 E1", "64x32x64 KW2 V1 E1", "64x64x32 KW1 V1 E1 7x120(81)")),
    (((770, 650, 517), ()),     ("64x64x64 KW4 V1 E1", "64x32x64 KW2 V1 E1", "64x64x32 KW1 V1 E1 7x112(98)")),
    (((800, 100, 644), ()),     ("64x32x64 KW2 V4 E4", "64x64x32 KW1 V4 E4", "64x64x32 KW1 V4 E4 7x120(80)")),
    (((801, 260, 640), ()),     ("64x32x64 KW2 V4 E4", "64x64x64 KW2 V4 E4", "64x64x32 KW1 V4 E4 7x120(81)")),
    (((801, 261, 642), ()),     ("64x32x64 KW2 V1 E1", "64x64x64 KW2 V1 E1", "64x64x32 KW1 V1 E1 7x120(81)")),
    (((770, 516, 650), ()),     ("64x32x64 KW2 V1 E4", "64x64x64 KW4 V1 E1", "64x64x32 KW1 V1 E1 7x112(98)")),
    (((1600, 642, 644), ()),    ("64x32x64 KW2 V4 E1", "64x32x64 KW2 V1 E4", "64x64x64 KW2 V1 E1 6x272(240)")),
    (((5000, 100, 36), ()),     ("64x64x32 KW1 V4 E4", "64x32x32 KW1 V4 E4", "64x64x32 KW1 V4 E4 40x128(8)")),     # the shortest legal last slab
    # sizes that divide by 4, one operand 4 bytes off: scalar loaders for an input, the scalar epilogue for an output or auxiliary
    (((70, 40, 260), ("x", "dy")),                      ("64x32x64 KW2 V1 E4", "64x32x32 KW1 V1 E4", "64x32x32 KW1 V1 E4 1x72(70)")),
    (((70, 40, 260), ("y", "dx", "workspace")),         ("64x32x64 KW2 V4 E1", "64x32x32 KW1 V4 E1", "64x32x32 KW1 V4 E1 1x72(70)")),
    (((800, 644, 100), ("bias", "w")),                  ("64x64x32 KW1 V1 E1", "64x32x64 KW2 V1 E4", "64x64x32 KW1 V4 E4 7x120(80)")),
    # an auxiliary operand off: the forms that read it (residual + row scale; add) take the scalar epilogue, the plain forms beside do not
    (((800, 100, 644), ("residual", "add")),            ("64x32x64 KW2 V4 E4", "64x64x32 KW1 V4 E4", "64x64x32 KW1 V4 E4 7x120(80)")),
]
ROWS = [c for c, _ in CASES]
# the rows at which every form runs (the others run the plain and the row-scaled forms): each entry point then has each form at a
# 64x32 and a 64x64 tile and at an all-vector and an all-scalar row
FORM_ROWS = [((129, 65, 33), ()), ((70, 40, 260), ()), ((70, 42, 259), ()), ((800, 644, 100), ()), ((801, 642, 261), ()), ((800, 100, 644), ()),
             ((801, 261, 642), ())]
FP32_CONFIGS = [(64, 32, 32, 1), (64, 32, 64, 2), (64, 64, 32, 1), (64, 64, 64, 2), (64, 64, 64, 4)]
DW_CONFIGS = [(64, 32, 32, 1), (64, 64, 32, 1), (64, 64, 64, 2)]       # the others need one split of >= 256 rows with > 768 tiles: never cheaper

# (B) cswin_linear_bwd_weight_batch, fp32: the problems of a launch, and splits x rows (last) of each
BATCHES = [
    ([(300, 72, 64), (300, 64, 72), (300, 8, 200), (300, 132, 4)],  ["3x104(92)"] * 4),
    ([(523, 100, 36), (523, 36, 100), (523, 36, 36)],               ["5x112(75)"] * 3),
    ([(37, 8, 128)],                                                ["1x40(37)"]),
    ([(129, 68, 36), (129, 36, 68)],                                ["2x72(57)"] * 2),
]
BATCH_ODD = [(300, 72, 64), (300, 30, 64), (300, 8, 200)]           # N = 30: no problem of this launch may take the batch kernel
TAIL = dict(M=300, C=24)                                            # a CSWinBlock's tail: dqkv (M, 3C), the four Linears' weight gradients

# (C) bf16 operands (precision 1).  Tiled family with fp32 storage: (row, entry, plan)
TILED16 = [
    ((37, 36, 100), "fwd", "64x64x64 KW1 V4 E4"), ((70, 40, 260), "fwd", "64x64x64 KW2 V4 E4"),
    ((800, 100, 644), "dgrad", "64x64x64 KW1 V4 E4"), ((801, 260, 640), "dgrad", "64x64x64 KW2 V4 E4"),
    ((129, 65, 33), "dw", "64x64x64 KW1 V1 E1 2x72(57)"), ((1600, 642, 644), "dw", "64x64x64 KW2 V1 E1 6x272(240)"),
]
# both operands stored as bf16 (io_bf16 bits 0 and 2): (row, entry, plan).  A dgrad row (M, N, K) has NO = K outputs per row and R = N.
GEMM16 = [
    ((70, 96, 64), "fwd", "gemm16 64x64 S2 last64"), ((70, 64, 96), "fwd", "gemm16 64x64 S2 last32"),
    ((70, 160, 192), "fwd", "gemm16 64x64 S3 last64"), ((70, 192, 160), "fwd", "gemm16 64x64 S3 last32"),
    ((130, 72, 128), "fwd", "gemm16 64x64 S2 last64"), ((3137, 1024, 96), "fwd", "gemm16 128x64 S3 last32"),
    ((70, 64, 96), "dgrad", "gemm16 64x64 S2 last64"), ((70, 96, 64), "dgrad", "gemm16 64x64 S2 last32"),
    ((70, 192, 160), "dgrad", "gemm16 64x64 S3 last64"), ((70, 160, 192), "dgrad", "gemm16 64x64 S3 last32"),
    ((130, 128, 72), "dgrad", "gemm16 64x64 S2 last64"), ((3137, 96, 1024), "dgrad", "gemm16 128x64 S3 last32"),
    # declined by gemm16 (N % 8 != 0; R % 64 = 36): the tiled family's loop for two bf16-stored operands
    ((70, 44, 128), "fwd", "64x64x64 KW1 V4 E4"), ((70, 44, 128), "dgrad", "64x64x64 KW1 V4 E4"),
    ((70, 40, 100), "fwd", "64x64x64 KW1 V4 E4"), ((70, 40, 100), "dgrad", "64x64x64 KW1 V4 E4"),
]
# wgrad16 through the batch entry point: (problems, io_bf16 of each, rows_per_sample of each or None, plan of each)
W16_BLOCK = lambda M: [(M, 64, 256), (M, 256, 64), (M, 64, 64), (M, 192, 64)]
WGRAD16 = [
    ([(300, 136, 72)], [0], [None], ["wgrad16 reg 3x128(44)"]), ([(300, 136, 72)], [1], [37], ["wgrad16 reg 3x128(44)"]),
    ([(300, 136, 72)], [2], [None], ["wgrad16 reg 3x128(44)"]), ([(300, 136, 72)], [3], [37], ["wgrad16 reg 3x128(44)"]),
    ([(320, 136, 72)], [3], [None], ["wgrad16 dma 3x128(64)"]), ([(320, 136, 72)], [3], [37], ["wgrad16 dma 3x128(64)"]),
    ([(320, 136, 72)], [3], [2], ["wgrad16 reg 3x128(64)"]),            # 66 samples a slab: more than the DMA tile's table holds
    ([(320, 132, 72)], [3], [None], ["wgrad16 reg 3x128(64)"]),         # N % 8 != 0
    ([(2080, 128, 128)], [3], [None], ["wgrad16 dma 17x128(32)"]),      # the last slab is a single 32-row step
    (W16_BLOCK(1024), [3] * 4, [None, 37, None, 100], ["wgrad16 dma 8x128(128)"] * 4),
    (W16_BLOCK(1000), [3] * 4, [None, 37, None, 100], ["wgrad16 reg 8x128(104)"] * 4),          # M % 32 != 0
]

def tail_problems():
    M, C = TAIL["M"], TAIL["C"]
    return [(M, C, 4 * C), (M, 4 * C, C), (M, C, C), (M, 3 * C, C)]         # fc2, fc1, proj, qkv


def all_wgrad_shapes():
    shapes = {shape for shape, _ in ROWS} | {s for s, e, _ in TILED16 if e == "dw"} | set(BATCH_ODD) | set(tail_problems())
    for problems, _ in BATCHES:
        shapes |= set(problems)
    for problems, _, _, _ in WGRAD16:
        shapes |= set(problems)
    return sorted(shapes)


SCALES = (1.25, 0.0, 0.7, 1.9, 0.45, 1.6)          # a zero, no power of two among the others, neighbours at least 0.35 apart
SCALES_POW2 = (2.0, 0.0, 1.0, 0.5)                 # bf16 weight gradients: the factor is applied before the operand is rounded


def rid(row):
    (M, N, K), off = row
    return f"{M}x{N}x{K}" + ("-off." + ".".join(off) if off else "")


def sample_rows(M):
    """rows_per_sample of a row: no divisor of M, no multiple of 8 (a boundary inside a 64-row tile and inside a slab)."""
    return 37 if M > 64 else 2


def row_scales(M, rows_per_sample, pow2=False):
    vals = SCALES_POW2 if pow2 else SCALES
    rs = np.array([vals[b % len(vals)] for b in range(cdiv(M, rows_per_sample))], np.float32)
    if rs[-1] == 0.0:
        rs[-1] = vals[2]         # the zero is never the last sample's: a weight gradient that loses its last row must show
    return rs


def seams(K):
    """(a multiple of 4 that is no multiple of a k-tile, a non-multiple of 4)."""
    return (36, 37) if K >= 64 else (4, 5)


def ref_seam(K):
    """Where the references that go through linear_ref's concat input cut x (their results do not depend on it)."""
    return seams(K)[1] if K >= 8 else K // 2


@functools.lru_cache(maxsize=None)
def gemm_inputs(shape, rounded=False):
    """x, w (scaled by 1 / sqrt(K)), bias, dy, residual, add, gelu_pre: float32 numpy; rounded: x, w, dy, gelu_pre hold bf16 values."""
    M, N, K = shape
    tag = f"gshp.{M}x{N}x{K}"
    r = bf16_round if rounded else (lambda a: a)
    return dict(x=r(det_normal(tag + ".x", (M, K))), w=r(det_normal(tag + ".w", (N, K), 1.0 / math.sqrt(K))), bias=det_normal(tag + ".b", (N,), 0.5),
                dy=r(det_normal(tag + ".dy", (M, N))), residual=det_normal(tag + ".res", (M, N)), add=det_normal(tag + ".add", (M, K)),
                pre=r(det_normal(tag + ".pre", (M, K))))


@functools.lru_cache(maxsize=None)
def ref_plain(shape, rounded=False):
    """y, y_act, dx, dw, dbias of the plain forms; computed once, shared by the tests that use it, never written."""
    i = gemm_inputs(shape, rounded)
    return linear_ref(i["x"], i["w"], i["bias"], i["dy"])


@functools.lru_cache(maxsize=None)
def ref_scaled(shape, rounded=False, pow2=False):
    """y = residual + s acc, dx = add + (s dy) w (and dxs = (s dy) w), dw, dbias of s dy, through linear_ref's concat input."""
    i, M, K = gemm_inputs(shape, rounded), shape[0], shape[2]
    rps, ks = sample_rows(M), ref_seam(K)
    out = linear_ref(i["x"][:, :ks], i["w"], i["bias"], i["dy"], x2=i["x"][:, ks:], residual=i["residual"], row_scale=row_scales(M, rps, pow2),
                     rows_per_sample=rps, add=i["add"])
    out["dx"] = torch.cat([out["dx"], out.pop("dx2")], 1)
    out["dxs"] = out["dx"] - torch.from_numpy(i["add"]).double()
    return out


@functools.lru_cache(maxsize=None)
def ref_gelu(shape, rounded=False):
    """dpre = (s dy) w o gelu'(gelu_pre)."""
    i, M = gemm_inputs(shape, rounded), shape[0]
    rps = sample_rows(M)
    return linear_ref(None, i["w"], None, i["dy"], gelu_pre=i["pre"], row_scale=row_scales(M, rps), rows_per_sample=rps)


# ------------------------------------------------------------------------------------------------
# the reference against an independent formulation, what the bound can see, the plan against the tables (no GPU)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K,ks,rps,gelu", [(7, 5, 9, 4, 3, False), (10, 6, 7, 3, 4, True)])
def test_linear_ref_agrees_with_explicit_loops(M, N, K, ks, rps, gelu):
    tag = f"gshp.self.{M}x{N}x{K}"
    x, w, b = det_normal(tag + ".x", (M, K)), det_normal(tag + ".w", (N, K), 1.0 / math.sqrt(K)), det_normal(tag + ".b", (N,), 0.5)
    dy, res, add = det_normal(tag + ".dy", (M, N)), det_normal(tag + ".res", (M, N)), det_normal(tag + ".add", (M, K))
    rs = row_scales(M, rps)
    args = dict(x2=x[:, ks:], residual=res, row_scale=rs, rows_per_sample=rps, add=add)
    ref = linear_ref(None if gelu else x[:, :ks], w, b, dy, gelu_pre=x[:, :ks] if gelu else None, **args)
    want = linear_loops(None if gelu else x[:, :ks], w, b, dy, x[:, ks:], res, rs, rps, x[:, :ks] if gelu else None, add)
    assert set(ref) == set(want)
    for k in ref:
        assert float((ref[k] - torch.from_numpy(want[k])).abs().max()) <= 1e-11, k
    # the single-source forms are the concat form's numbers
    one = linear_ref(x, w, b, dy, residual=res, row_scale=rs, rows_per_sample=rps, add=add)
    if not gelu:
        assert float((one["y"] - ref["y"]).abs().max()) <= 1e-11 and float((one["dw"] - ref["dw"]).abs().max()) <= 1e-11
        assert float((one["dx"] - torch.cat([ref["dx"], ref["dx2"]], 1)).abs().max()) <= 1e-11


SHAPES = sorted({shape for shape, _ in ROWS} | {shape for shape, _, _ in TILED16 + GEMM16} | set(all_wgrad_shapes()))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bound_sees_the_bugs_these_shapes_are_for(shape):
    """A reduction that loses its last index (in the forward, the data gradient or the weight gradient), a sample boundary of
    the row scale that is one row off and a concat seam that is one column off each move the output they touch by more than
    10 RTOL in the suite's metric, at every row.  A condition on the inputs: a row that fails it gets a shorter reduction or
    row scales that lie further apart, never another bound."""
    M, N, K = shape
    i = gemm_inputs(shape)
    rps, ks = sample_rows(M), ref_seam(K)
    args = dict(x2=i["x"][:, ks:], residual=i["residual"], row_scale=row_scales(M, rps), rows_per_sample=rps)
    run = lambda wrong=None: linear_ref(i["x"][:, :ks], i["w"], i["bias"], i["dy"], _wrong=wrong, **args)
    ref = run()
    metric = lambda got, want: float((got - want).abs().max() / want.pow(2).mean().sqrt())
    touched = dict(drop_last_k=("y",), drop_last_n=("dx", "dx2"), drop_last_m=("dw", "dbias"), seam=("y", "dw"))
    if M > rps:                                      # a single sample has no boundary
        touched["scale_boundary"] = ("y", "dx", "dx2", "dw", "dbias")
    for wrong, outs in touched.items():
        bad = run(wrong)
        for k in outs:
            seen = metric(bad[k], ref[k])
            print(f"{'x'.join(map(str, shape))} {wrong} {k}: {seen:.3e}")
            assert seen > 10 * RTOL, (wrong, k, seen)


def test_case_tables_reach_every_configuration():
    assert len(set(ROWS)) == len(ROWS) == 21 and set(FORM_ROWS) <= set(ROWS)
    plans = {}
    for row, want in CASES:
        (M, N, K), off = row
        got = tuple(plan_str(gemm_plan(e, M, N, K, off=off)) for e in ("fwd", "dgrad", "dw"))
        assert got == want, (rid(row), got)
        for e in ("fwd", "dgrad", "dw"):
            plans[row, e] = gemm_plan(e, M, N, K, off=off)
        rps = sample_rows(M)
        assert M % rps != 0 and rps % 8 != 0
    cfg = lambda p: p["tile"] + (p["bk"], p["kw"])
    for e, configs in (("fwd", FP32_CONFIGS), ("dgrad", FP32_CONFIGS), ("dw", DW_CONFIGS)):
        mine = [p for (row, ee), p in plans.items() if ee == e]
        assert {cfg(p) for p in mine} == set(configs), e
        for c in configs:
            assert any(cfg(p) == c and p["ragged"] for p in mine), f"{e} {c}: no row with M % 64, N % tile and R % k-tile all non-zero"
        assert {p["vec"] for p in mine} == {1, 4} and {p["store"] for p in mine} == {1, 4}, e
        # sizes that divide by 4 and a misaligned operand: scalar loaders, or the scalar epilogue
        unaligned = [(p["vec"], p["store"]) for (row, ee), p in plans.items() if ee == e and row[1] and row[0][1] % 4 == 0 and row[0][2] % 4 == 0]
        assert (1, 4) in unaligned and (4, 1) in unaligned, e
        # every form at both tiles, at an all-vector and at an all-scalar row
        forms = [plans[row, e] for row in FORM_ROWS]
        assert {p["tile"] for p in forms} == {(64, 32), (64, 64)}, e
        assert (4, 4) in {(p["vec"], p["store"]) for p in forms} and (1, 1) in {(p["vec"], p["store"]) for p in forms}, e
    sized = {(p["vec"], p["store"]) for (row, e), p in plans.items() if not row[1]}
    assert (1, 4) in sized and (4, 1) in sized                   # K odd with N % 4 == 0, and the reverse
    assert min(p["last"] for (row, e), p in plans.items() if e == "dw" and p["splits"] > 1) == 8
    aux = dict(off=("residual", "add"))
    assert (gemm_plan("fwd", 800, 100, 644, form="res", **aux)["store"], gemm_plan("dgrad", 800, 100, 644, form="add", **aux)["store"]) == (1, 1)
    # a seam that keeps the vector loaders and one that does not; a boundary of the row scale inside a slab
    for (M, N, K), off in FORM_ROWS:
        a, b = seams(K)
        assert 0 < a < b < K and a % 4 == 0 and a % 32 != 0 and b % 4 != 0
        assert gemm_plan("fwd", M, N, K, k_split=b)["vec"] == 1 and gemm_plan("dgrad", M, N, K, k_split=b, form="split")["store"] == 1
        if K % 4 == 0:
            assert gemm_plan("fwd", M, N, K, k_split=a)["vec"] == 4 and gemm_plan("dw", M, N, K, k_split=a)["vec"] == (4 if N % 4 == 0 else 1)
    # (B)
    for problems, want in BATCHES:
        got, _ = batch_plan(problems)
        assert [plan_str(p).split()[-1] for p in got] == want and all(p["kernel"] == "batch" for p in got), problems
    assert all(p["kernel"] == "tiled" for p in batch_plan(BATCH_ODD)[0]) and all(p["kernel"] == "tiled" for p in batch_plan(BATCHES[3][0], off_workspace=(1,))[0])
    M, C = TAIL["M"], TAIL["C"]
    assert batch_plan(tail_problems(), tail=(M, 3 * C, C))[1]["kernel"] == "tail"
    assert plan_str(batch_plan(tail_problems(), tail=(M, 3 * C, C), tail_off=("dx",))[1]) == "64x32x32 KW1 V4 E1"
    # (C)
    for shape, e, want in TILED16:
        assert plan_str(gemm_plan(e, *shape, precision=1)) == want, (shape, e)
    assert {plan_str(gemm_plan(e, *shape, precision=1)).split()[1] for shape, e, _ in TILED16 if e != "dw"} == {"KW1", "KW2"}
    for shape, e, want in GEMM16:
        for io in (5, 7):
            assert plan_str(gemm_plan(e, *shape, precision=1, io=io)) == want, (shape, e)
    for e in ("fwd", "dgrad"):
        mine = [(s, w) for s, ee, w in GEMM16 if ee == e and w.startswith("gemm16")]
        assert {w for _, w in mine} == {f"gemm16 64x64 S{s} last{k}" for s in (2, 3) for k in (32, 64)} | {"gemm16 128x64 S3 last32"}, e
        assert any((s[1] if e == "fwd" else s[2]) % 64 == 8 for s, _ in mine) and all(s[0] % 64 for s, _ in mine)
        assert any(w.startswith("gemm16 128") and s[0] % 128 == 65 for s, w in mine)
    for problems, ios, samples, want in WGRAD16:
        got, _ = batch_plan(problems, precision=1, ios=ios, samples=samples)
        assert [plan_str(p) for p in got] == want, (problems, [plan_str(p) for p in got])
    # the split policy against the library's own workspace query, which needs no GPU
    from cswin_unet_amd._lib import lib
    for M, N, K in all_wgrad_shapes():
        assert lib().cswin_linear_bwd_weight_workspace(M, N, K) == wgrad_workspace_bytes(M, N, K), (M, N, K)


# ------------------------------------------------------------------------------------------------
# the entry points, called directly with guarded buffers
# ------------------------------------------------------------------------------------------------
class Guarded4(Guarded):
    """Guarded, with the view 4 bytes off a 16-byte boundary."""

    def __init__(self, shape, dtype=torch.float32):
        assert dtype == torch.float32
        self.n = math.prod(shape)
        self.lo = GUARD + 1
        self.buf = torch.full((self.n + 2 * GUARD + 4,), float("nan"), dtype=dtype, device=DEV)
        self.t = self.buf[self.lo:self.lo + self.n].view(shape)
        assert self.t.data_ptr() % 16 == 4

    def intact(self):
        return bool(torch.isnan(self.buf[:self.lo]).all()) and bool(torch.isnan(self.buf[self.lo + self.n:]).all())


def put(a, off=False, bf16=False):
    """Device copy of a numpy array / tensor; off: based 4 bytes off a 16-byte boundary; bf16: stored as bf16."""
    if a is None:
        return None
    t = (torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a.detach().cpu().contiguous()).float()
    t = t.bfloat16() if bf16 else t
    if not off:
        t = t.to(DEV)
        assert t.data_ptr() % 16 == 0
        return t
    shift = 4 // t.element_size()
    buf = torch.zeros(t.numel() + 16, dtype=t.dtype, device=DEV)
    v = buf[shift:shift + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def out(shape, off=False, bf16=False):
    return Guarded4(shape) if off else Guarded(shape, torch.bfloat16 if bf16 else torch.float32)


@pytest.fixture(scope="module")
def lin():
    """The direct-call helpers; skips when a tuning variable makes the library depart from gemm_plan."""
    present = [v for v in os.environ if v.startswith(TUNING_PREFIXES)]
    if present:
        pytest.skip(f"{', '.join(present)} set: the launch plan these tests rely on does not hold")
    from cswin_unet_amd._lib import CswinHipError, ReduceJob, WgradDesc, call, lib, ptr, stream
    vp = lambda obj: ctypes.c_void_p(ctypes.addressof(obj))

    def finish(what, o, fn, refused):
        if refused:
            with pytest.raises(CswinHipError):
                fn()
            settle("refused " + what, o, untouched=True)
            return None
        fn()
        return o

    class Lin:
        Error, Job = CswinHipError, ReduceJob

        @staticmethod
        def fwd(shape, x, w, bias=None, *, k_split=0, act=False, residual=None, rs=None, rps=1, precision=0, io=0, off=(), what="", refused=False):
            """{y, y_act} of cswin_linear_fwd on numpy inputs; x (M, K) is cut at k_split into the two sources."""
            M, N, K = shape
            xs, x2 = (put(x[:, :k_split], "x" in off, io & 1), put(x[:, k_split:], "x2" in off)) if k_split else (put(x, "x" in off, io & 1), None)
            wd, bd, rd, sd = put(w, "w" in off, io & 4), put(bias, "bias" in off), put(residual, "residual" in off), put(rs)
            o = dict(y=out((M, N), "y" in off, io & 2))
            if act:
                o["y_act"] = out((M, N), "y_act" in off, io & 2)
            fn = lambda: call("cswin_linear_fwd", ptr(xs), ptr(x2), k_split, ptr(wd), ptr(bd), ptr(o["y"].t), ptr(o["y_act"].t) if act else None, ptr(rd),
                              ptr(sd), rps, M, N, K, precision, io, stream())
            if finish(f"linear_fwd {what}", o, fn, refused):
                settle(f"linear_fwd {what}", o)
                return {k: g.t for k, g in o.items()}

        @staticmethod
        def dgrad(shape, dy, w, *, k_split=0, pre=None, rs=None, rps=1, add=None, precision=0, io=0, off=(), what="", refused=False):
            """{dx, dx2} of cswin_linear_bwd_data; k_split != 0: the split form."""
            M, N, K = shape
            dyd, wd, pd = put(dy, "dy" in off, io & 1), put(w, "w" in off, io & 4), put(pre, "gelu_pre" in off, io & 8)
            ad, sd = put(add, "add" in off), put(rs)
            o = dict(dx=out((M, k_split or K), "dx" in off, io & 2))
            if k_split:
                o["dx2"] = out((M, K - k_split), "dx2" in off)
            fn = lambda: call("cswin_linear_bwd_data", ptr(dyd), ptr(wd), ptr(o["dx"].t), ptr(o["dx2"].t) if "dx2" in o else None, k_split, ptr(pd), ptr(sd), rps,
                              ptr(ad), M, N, K, precision, io, stream())
            if finish(f"linear_bwd_data {what}", o, fn, refused):
                settle(f"linear_bwd_data {what}", o)
                return {k: g.t for k, g in o.items()}

        @staticmethod
        def dw(shape, dy, x, *, k_split=0, rs=None, rps=1, dbias=True, deferred=False, precision=0, off=(), what="", refused=False, short=0):
            """({dw, dbias}, the deferred job's rows or None) of cswin_linear_bwd_weight with a workspace of exactly the queried size."""
            M, N, K = shape
            nbytes = lib().cswin_linear_bwd_weight_workspace(M, N, K)
            assert nbytes > 0 and nbytes % 4 == 0
            dyd = put(dy, "dy" in off)
            xs, x2 = (put(x[:, :k_split], "x" in off), put(x[:, k_split:], "x2" in off)) if k_split else (put(x, "x" in off), None)
            sd = put(rs)
            o = dict(dw=out((N, K)), workspace=out((nbytes // 4,), "workspace" in off))
            if dbias:
                o["dbias"] = out((N,))
            job = ReduceJob()
            fn = lambda: call("cswin_linear_bwd_weight", ptr(dyd), ptr(xs), ptr(x2), k_split, ptr(sd), rps, ptr(o["dw"].t), ptr(o["dbias"].t) if dbias else None,
                              ptr(o["workspace"].t), nbytes - short, M, N, K, vp(job) if deferred else None, precision, stream())
            if finish(f"linear_bwd_weight {what}", o, fn, refused):
                if deferred:
                    assert torch.isnan(o["dw"].t).all(), "a deferred reduction ran at once"
                    call("cswin_rows_sum_multi", vp(job), 1, stream())
                settle(f"linear_bwd_weight {what}", o)
                return {k: g.t for k, g in o.items() if k != "workspace"}, (job.rows if deferred else None)

        @staticmethod
        def batch(problems, *, precision=0, pending=None, tail=None, what="", refused=False, npending=None):
            """cswin_linear_bwd_weight_batch, or cswin_linear_bwd_tail when tail = dict(dy, w, off) is given.  problems: dicts with
            shape, dy, x and optionally rs, rps, dbias (default True), io, off_workspace, short, precision.  pending: (job array, the
            buffers its jobs write) of an earlier reduce=False call.  Returns (per problem {dw, dbias, rows}, dx or None, the pending
            jobs' buffers)."""
            n = len(problems)
            wg, jobs, keep, o = (WgradDesc * n)(), (ReduceJob * n)(), [], {}
            for i, p in enumerate(problems):
                M, N, K = p["shape"]
                io = p.get("io", 0)
                nbytes = lib().cswin_linear_bwd_weight_workspace(M, N, K)
                dyd, xd, sd = put(p["dy"], bf16=io & 1), put(p["x"], bf16=io & 2), put(p.get("rs"))
                keep += [dyd, xd, sd]
                o[f"dw{i}"], o[f"workspace{i}"] = out((N, K)), out((nbytes // 4,), p.get("off_workspace", False))
                if p.get("dbias", True):
                    o[f"dbias{i}"] = out((N,))
                d = wg[i]
                d.dy, d.x, d.row_scale, d.dw = dyd.data_ptr(), xd.data_ptr(), (sd.data_ptr() if sd is not None else None), o[f"dw{i}"].t.data_ptr()
                d.dbias = o[f"dbias{i}"].t.data_ptr() if f"dbias{i}" in o else None
                d.workspace, d.ws_bytes, d.rows_per_sample = o[f"workspace{i}"].t.data_ptr(), nbytes - p.get("short", 0), p.get("rps", 1)
                d.M, d.N, d.K, d.precision, d.io_bf16 = M, N, K, p.get("precision", precision), io
            pend = (vp(pending[0]), len(pending[0]) if npending is None else npending) if pending else (None, 0)
            if tail:
                tM, tN = tail["dy"].shape
                tK = tail["w"].shape[1]
                toff = tail.get("off", ())
                tdy, tw = put(tail["dy"], "dy" in toff), put(tail["w"], "w" in toff)
                o["dx"] = out((tM, tK), "dx" in toff)
                fn = lambda: call("cswin_linear_bwd_tail", ptr(tdy), ptr(tw), ptr(o["dx"].t), tM, tN, tK, vp(wg), n, vp(jobs), *pend, stream())
            else:
                fn = lambda: call("cswin_linear_bwd_weight_batch", vp(wg), n, vp(jobs), *pend, stream())
            if pending:
                o.update({f"pending{k}": g for k, g in enumerate(pending[1])})
            if not finish(f"{'linear_bwd_tail' if tail else 'linear_bwd_weight_batch'} {what}", o, fn, refused):
                return None
            call("cswin_rows_sum_multi", vp(jobs), n, stream())
            settle(f"linear_bwd_weight_batch {what}", {k: g for k, g in o.items() if not k.startswith("workspace")})
            for k, g in o.items():
                assert not k.startswith("workspace") or g.intact(), f"linear_bwd_weight_batch {what}: a guard word of {k} was overwritten"
            res = [dict(dw=o[f"dw{i}"].t, dbias=o[f"dbias{i}"].t if f"dbias{i}" in o else None, rows=jobs[i].rows) for i in range(n)]
            return res, (o["dx"].t if tail else None), ([g.t for g in pending[1]] if pending else None)

        @staticmethod
        def pending_jobs(problems, what=""):
            """Weight gradients launched but NOT reduced: (their job array, the Guarded dw / dbias the jobs will write, the
            workspaces they read -- keep them alive)."""
            n = len(problems)
            wg, jobs, keep, outs = (WgradDesc * n)(), (ReduceJob * n)(), [], []
            for i, p in enumerate(problems):
                M, N, K = p["shape"]
                nbytes = lib().cswin_linear_bwd_weight_workspace(M, N, K)
                dyd, xd, ws, dwg, dbg = put(p["dy"]), put(p["x"]), out((nbytes // 4,)), out((N, K)), out((N,))
                keep += [dyd, xd, ws]
                outs += [dwg, dbg]
                d = wg[i]
                d.dy, d.x, d.row_scale, d.dw, d.dbias = dyd.data_ptr(), xd.data_ptr(), None, dwg.t.data_ptr(), dbg.t.data_ptr()
                d.workspace, d.ws_bytes, d.rows_per_sample, d.M, d.N, d.K, d.precision, d.io_bf16 = ws.t.data_ptr(), nbytes, 1, M, N, K, 0, 0
            call("cswin_linear_bwd_weight_batch", vp(wg), n, vp(jobs), None, 0, stream())
            torch.cuda.synchronize()
            assert all(g.untouched() for g in outs), f"{what}: a pending reduction has run"
            return jobs, outs, keep

    return Lin


def check(errs, bound=RTOL):
    assert errs and all(np.isfinite(e) and e <= bound for e in errs.values()), errs


def measure16(got, ref, what):
    """An output stored as bf16: max over the elements of (|got - ref| - 2^-8 |ref|) / rms(ref), which must stay below RTOL.
    Round-to-nearest-even is within 2^-9 relative of the fp32 value, which is within RTOL rms of the reference; the factor of
    two covers a value that the fp32 error carries across a binade.  Logged under `what`."""
    assert got.dtype == torch.bfloat16
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    err = float(((got - ref).abs() - 2.0 ** -8 * ref.abs()).max()) / (float(ref.pow(2).mean().sqrt()) + 1e-30)
    err = err if np.isfinite(err) else float("inf")
    print(f"{what}: max(|diff| - 2^-8 |ref|)/rms = {err:.3e}")
    try:
        os.makedirs(os.path.dirname(LOG), exist_ok=True)
        with open(LOG, "a") as f:
            f.write(f"{what}: {err:.3e} (bf16 storage, beyond 2^-8 |ref|)\n")
    except OSError:
        pass
    return err


def cmp(got, ref, what):
    return measure16(got, ref, what) if got.dtype == torch.bfloat16 else measure(got, ref, what)


# ------------------------------------------------------------------------------------------------
# (A) fp32, every form against float64
# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("row", ROWS, ids=rid)
def test_linear_fwd_fp32_vs_float64(lin, row):
    """plain and residual + row scale at every row; the GELU pair, the concat input at a seam that keeps the vector loaders and
    the concat input with a residual at one that does not at FORM_ROWS."""
    shape, off = row
    M, N, K = shape
    i, plain, scaled = gemm_inputs(shape), ref_plain(shape), ref_scaled(shape)
    rps, tag = sample_rows(M), "gemmshape.A." + rid(row) + ".fwd."
    rs = row_scales(M, rps)
    errs = {}
    errs["plain"] = measure(lin.fwd(shape, i["x"], i["w"], i["bias"], off=off, what=tag + "plain")["y"], plain["y"], tag + "plain.y")
    got = lin.fwd(shape, i["x"], i["w"], i["bias"], residual=i["residual"], rs=rs, rps=rps, off=off, what=tag + "res")
    errs["res"] = measure(got["y"], scaled["y"], tag + "res.y")
    if row in FORM_ROWS:
        a, b = seams(K)
        got = lin.fwd(shape, i["x"], i["w"], i["bias"], act=True, what=tag + "gelu")
        errs["gelu.y"], errs["gelu.y_act"] = measure(got["y"], plain["y"], tag + "gelu.y"), measure(got["y_act"], plain["y_act"], tag + "gelu.y_act")
        errs["concat"] = measure(lin.fwd(shape, i["x"], i["w"], i["bias"], k_split=a, what=tag + "concat")["y"], plain["y"], tag + "concat.y")
        got = lin.fwd(shape, i["x"], i["w"], i["bias"], k_split=b, residual=i["residual"], rs=rs, rps=rps, what=tag + "concat_res")
        errs["concat_res"] = measure(got["y"], scaled["y"], tag + "concat_res.y")
    check(errs)


@gpu
@pytest.mark.parametrize("row", ROWS, ids=rid)
def test_linear_bwd_data_fp32_vs_float64(lin, row):
    """plain, plain with a row scale and add + row scale at every row; GELU' with a row scale and the dx | dx2 split at both seams
    at FORM_ROWS."""
    shape, off = row
    M, N, K = shape
    i, plain, scaled = gemm_inputs(shape), ref_plain(shape), ref_scaled(shape)
    rps, tag = sample_rows(M), "gemmshape.A." + rid(row) + ".dgrad."
    rs = row_scales(M, rps)
    errs = {}
    errs["plain"] = measure(lin.dgrad(shape, i["dy"], i["w"], off=off, what=tag + "plain")["dx"], plain["dx"], tag + "plain.dx")
    errs["scaled"] = measure(lin.dgrad(shape, i["dy"], i["w"], rs=rs, rps=rps, off=off, what=tag + "scaled")["dx"], scaled["dxs"], tag + "scaled.dx")
    errs["add"] = measure(lin.dgrad(shape, i["dy"], i["w"], rs=rs, rps=rps, add=i["add"], off=off, what=tag + "add")["dx"], scaled["dx"], tag + "add.dx")
    if row in FORM_ROWS:
        got = lin.dgrad(shape, i["dy"], i["w"], pre=i["pre"], rs=rs, rps=rps, what=tag + "gelu")
        errs["gelu"] = measure(got["dx"], ref_gelu(shape)["dpre"], tag + "gelu.dx")
        for ks in seams(K):
            got = lin.dgrad(shape, i["dy"], i["w"], k_split=ks, what=tag + f"split{ks}")
            errs[f"split{ks}.dx"] = measure(got["dx"], plain["dx"][:, :ks], tag + f"split{ks}.dx")
            errs[f"split{ks}.dx2"] = measure(got["dx2"], plain["dx"][:, ks:], tag + f"split{ks}.dx2")
    check(errs)


@gpu
@pytest.mark.parametrize("row", ROWS, ids=rid)
def test_linear_bwd_weight_fp32_vs_float64(lin, row):
    """plain and row-scaled with dbias at every row, the second through `deferred`, whose job must hold the plan's split count;
    without dbias and with the concat input at both seams at FORM_ROWS."""
    shape, off = row
    M, N, K = shape
    i, plain, scaled = gemm_inputs(shape), ref_plain(shape), ref_scaled(shape)
    rps, tag = sample_rows(M), "gemmshape.A." + rid(row) + ".dw."
    rs = row_scales(M, rps)
    errs = {}
    got, _ = lin.dw(shape, i["dy"], i["x"], off=off, what=tag + "plain")
    errs["plain.dw"], errs["plain.dbias"] = measure(got["dw"], plain["dw"], tag + "plain.dw"), measure(got["dbias"], plain["dbias"], tag + "plain.dbias")
    got, rows = lin.dw(shape, i["dy"], i["x"], rs=rs, rps=rps, deferred=True, off=off, what=tag + "scaled")
    assert rows == gemm_plan("dw", M, N, K, off=off)["splits"], "the deferred job's rows are not the plan's split count"
    errs["scaled.dw"], errs["scaled.dbias"] = measure(got["dw"], scaled["dw"], tag + "scaled.dw"), measure(got["dbias"], scaled["dbias"], tag + "scaled.dbias")
    if row in FORM_ROWS:
        got, _ = lin.dw(shape, i["dy"], i["x"], dbias=False, what=tag + "nobias")
        errs["nobias.dw"] = measure(got["dw"], plain["dw"], tag + "nobias.dw")
        a, b = seams(K)
        got, rows = lin.dw(shape, i["dy"], i["x"], k_split=a, deferred=True, what=tag + "concat")
        assert rows == gemm_plan("dw", M, N, K, k_split=a)["splits"]
        errs["concat.dw"], errs["concat.dbias"] = measure(got["dw"], plain["dw"], tag + "concat.dw"), measure(got["dbias"], plain["dbias"], tag + "concat.dbias")
        got, _ = lin.dw(shape, i["dy"], i["x"], k_split=b, rs=rs, rps=rps, dbias=False, what=tag + "concat_scaled")
        errs["concat_scaled.dw"] = measure(got["dw"], scaled["dw"], tag + "concat_scaled.dw")
    check(errs)


# ------------------------------------------------------------------------------------------------
# (B) fp32 batch and tail
# ------------------------------------------------------------------------------------------------
def batch_problems(shapes, rounded=False, pow2=False, ios=None, samples=None):
    """(problems for lin.batch, their float64 references): row scales on every other problem (or where samples[i] is set), dbias
    on all but the last of a launch of several."""
    problems, refs = [], []
    for j, shape in enumerate(shapes):
        M = shape[0]
        i = gemm_inputs(shape, rounded)
        sampled = samples[j] is not None if samples else j % 2 == 1
        rps = (samples[j] if samples and samples[j] else sample_rows(M)) if sampled else 1
        p = dict(shape=shape, dy=i["dy"], x=i["x"], dbias=len(shapes) == 1 or j + 1 < len(shapes), io=ios[j] if ios else 0)
        if sampled:
            p.update(rs=row_scales(M, rps, pow2), rps=rps)
            refs.append(linear_ref(i["x"], i["w"], i["bias"], i["dy"], row_scale=p["rs"], rows_per_sample=rps) if rps != sample_rows(M)
                        else ref_scaled(shape, rounded, pow2))
        else:
            refs.append(ref_plain(shape, rounded))
        problems.append(p)
    return problems, refs


def compare_batch(tag, res, refs, plans):
    errs = {}
    for j, (r, ref, plan) in enumerate(zip(res, refs, plans)):
        assert r["rows"] == plan["splits"], f"{tag}: problem {j} left a job of {r['rows']} rows, the plan has {plan['splits']} splits"
        errs[f"dw{j}"] = measure(r["dw"], ref["dw"], f"{tag}.dw{j}")
        if r["dbias"] is not None:
            errs[f"dbias{j}"] = measure(r["dbias"], ref["dbias"], f"{tag}.dbias{j}")
    return errs


@gpu
@pytest.mark.parametrize("k", range(len(BATCHES)), ids=lambda k: f"batch{k}")
def test_linear_bwd_weight_batch_fp32_vs_float64(lin, k):
    """One launch of 4, 3, 1 and 2 problems: row scales on every other problem, no dbias on the last, every dw and dbias against
    float64 and every deferred job's rows against the plan."""
    shapes = BATCHES[k][0]
    problems, refs = batch_problems(shapes)
    res, _, _ = lin.batch(problems, what=f"batch{k}")
    check(compare_batch(f"gemmshape.B.batch{k}", res, refs, batch_plan(shapes)[0]))


@gpu
def test_linear_bwd_weight_batch_falls_back_to_separate_launches(lin):
    """A problem with N % 4 != 0, and a workspace 4 bytes off a 16-byte boundary: every problem of the launch goes alone."""
    problems, refs = batch_problems(BATCH_ODD)
    res, _, _ = lin.batch(problems, what="batch.odd")
    check(compare_batch("gemmshape.B.odd", res, refs, batch_plan(BATCH_ODD)[0]))
    shapes = BATCHES[3][0]
    problems, refs = batch_problems(shapes)
    problems[1]["off_workspace"] = True
    res, _, _ = lin.batch(problems, what="batch.off")
    check(compare_batch("gemmshape.B.off", res, refs, batch_plan(shapes, off_workspace=(1,))[0]))


@gpu
@pytest.mark.parametrize("off", [(), ("dx",)], ids=["one_launch", "dx_off"])
def test_linear_bwd_tail_fp32_vs_float64(lin, off):
    """The block tail at M = 300, C = 24 with two pending reductions: in one launch, and with dx 4 bytes off, where the data
    gradient is launched on its own.  dx, the four weight gradients and what the riders reduce against float64."""
    M, C = TAIL["M"], TAIL["C"]
    shapes = tail_problems()
    problems, refs = batch_problems(shapes)
    earlier = [(M, C, C), (M, 3 * C, C)]
    jobs, outs, keep = lin.pending_jobs([dict(shape=s, dy=gemm_inputs(s)["dy"], x=gemm_inputs(s)["x"]) for s in earlier], what="tail")
    t = gemm_inputs((M, 3 * C, C))
    res, dx, riders = lin.batch(problems, pending=(jobs, outs), tail=dict(dy=t["dy"], w=t["w"], off=off), what="tail" + "".join(off))
    tag = "gemmshape.B.tail" + ("." + ".".join(off) if off else "")
    plans, dplan = batch_plan(shapes, tail=(M, 3 * C, C), tail_off=off)
    assert dplan["kernel"] == ("tiled" if off else "tail")
    errs = compare_batch(tag, res, refs, plans)
    errs["dx"] = measure(dx, ref_plain((M, 3 * C, C))["dx"], tag + ".dx")
    for j, s in enumerate(earlier):
        errs[f"rider{j}.dw"] = measure(riders[2 * j], ref_plain(s)["dw"], f"{tag}.rider{j}.dw")
        errs[f"rider{j}.dbias"] = measure(riders[2 * j + 1], ref_plain(s)["dbias"], f"{tag}.rider{j}.dbias")
    check(errs)


# ------------------------------------------------------------------------------------------------
# (C) bf16 operands, exact on bf16-valued inputs
# ------------------------------------------------------------------------------------------------
def fwd16_forms(lin, shape, io, tag):
    """plain, the GELU pair and (fp32 outputs only) residual + row scale of cswin_linear_fwd at precision 1."""
    M = shape[0]
    i, plain = gemm_inputs(shape, True), ref_plain(shape, True)
    rps = sample_rows(M)
    errs = {}
    errs["plain"] = cmp(lin.fwd(shape, i["x"], i["w"], i["bias"], precision=1, io=io, what=tag + "plain")["y"], plain["y"], tag + "plain.y")
    got = lin.fwd(shape, i["x"], i["w"], i["bias"], act=True, precision=1, io=io, what=tag + "gelu")
    errs["gelu.y"], errs["gelu.y_act"] = cmp(got["y"], plain["y"], tag + "gelu.y"), cmp(got["y_act"], plain["y_act"], tag + "gelu.y_act")
    if not io & 2:
        got = lin.fwd(shape, i["x"], i["w"], i["bias"], residual=i["residual"], rs=row_scales(M, rps), rps=rps, precision=1, io=io, what=tag + "res")
        errs["res"] = cmp(got["y"], ref_scaled(shape, True)["y"], tag + "res.y")
    return errs


def dgrad16_forms(lin, shape, io, tag):
    """plain, GELU' with a row scale and gelu_pre in fp32 and, with bf16 storage, GELU' with gelu_pre stored as bf16."""
    M = shape[0]
    i, plain = gemm_inputs(shape, True), ref_plain(shape, True)
    rps = sample_rows(M)
    rs = row_scales(M, rps)
    errs = {}
    errs["plain"] = cmp(lin.dgrad(shape, i["dy"], i["w"], precision=1, io=io, what=tag + "plain")["dx"], plain["dx"], tag + "plain.dx")
    for io_pre in ((io, io | 8) if io else (io,)):
        name = "gelu16" if io_pre & 8 else "gelu"
        got = lin.dgrad(shape, i["dy"], i["w"], pre=i["pre"], rs=rs, rps=rps, precision=1, io=io_pre, what=tag + name)
        errs[name] = cmp(got["dx"], ref_gelu(shape, True)["dpre"], tag + name + ".dx")
    return errs


@gpu
@pytest.mark.parametrize("shape,entry,plan", TILED16, ids=[f"{'x'.join(map(str, s))}-{e}" for s, e, _ in TILED16])
def test_tiled_family_bf16_operands_exact_on_bf16_inputs(lin, shape, entry, plan):
    """precision 1 with every tensor stored fp32: KW1 and KW2 of the forward, of the data gradient with its transposing LDS read
    and of the weight gradient, which only a problem that is not 4-divisible (or is misaligned, or has two sources) reaches."""
    M, N, K = shape
    tag = f"gemmshape.C.tiled.{M}x{N}x{K}.{entry}."
    if entry == "fwd":
        return check(fwd16_forms(lin, shape, 0, tag))
    if entry == "dgrad":
        return check(dgrad16_forms(lin, shape, 0, tag))
    i, rps = gemm_inputs(shape, True), sample_rows(M)
    errs = {}
    got, rows = lin.dw(shape, i["dy"], i["x"], precision=1, deferred=True, what=tag + "plain")
    assert rows == gemm_plan("dw", M, N, K, precision=1)["splits"]
    errs["plain.dw"], errs["plain.dbias"] = measure(got["dw"], ref_plain(shape, True)["dw"], tag + "plain.dw"), measure(got["dbias"], ref_plain(shape, True)["dbias"], tag + "plain.dbias")
    got, _ = lin.dw(shape, i["dy"], i["x"], rs=row_scales(M, rps, True), rps=rps, precision=1, what=tag + "scaled")
    ref = ref_scaled(shape, True, True)
    errs["scaled.dw"], errs["scaled.dbias"] = measure(got["dw"], ref["dw"], tag + "scaled.dw"), measure(got["dbias"], ref["dbias"], tag + "scaled.dbias")
    check(errs)


@gpu
@pytest.mark.parametrize("io", [5, 7])
@pytest.mark.parametrize("shape,entry,plan", GEMM16, ids=[f"{'x'.join(map(str, s))}-{e}" for s, e, _ in GEMM16])
def test_both_operands_stored_bf16_exact_on_bf16_inputs(lin, shape, entry, plan, io):
    """io_bf16 5 and 7 (and 13 / 15 for a bf16-stored gelu_pre): gemm16.hip with 2 and 3 stages, a full and a half last step,
    ragged M, N % 64 == 8 and the 128-row tile whose upper half holds one row; the two shapes it declines take the tiled loop."""
    M, N, K = shape
    tag = f"gemmshape.C.{'gemm16' if plan.startswith('gemm16') else 'tiled16'}.{M}x{N}x{K}.{entry}.io{io}."
    check((fwd16_forms if entry == "fwd" else dgrad16_forms)(lin, shape, io, tag))


@gpu
@pytest.mark.parametrize("k", range(len(WGRAD16)), ids=lambda k: f"w16-{k}")
def test_wgrad16_exact_on_bf16_inputs(lin, k):
    """wgrad16.hip through the batch entry point: the register path at every storage combination, the LDS-DMA tile with and
    without a row scale, its fall-backs, a last slab of one 32-row step and launches of four problems."""
    shapes, ios, samples, _ = WGRAD16[k]
    problems, refs = batch_problems(shapes, rounded=True, pow2=True, ios=ios, samples=samples)
    res, _, _ = lin.batch(problems, precision=1, what=f"w16-{k}")
    check(compare_batch(f"gemmshape.C.wgrad16.{k}", res, refs, batch_plan(shapes, precision=1, ios=ios, samples=samples)[0]))


@gpu
def test_bf16_kernels_round_their_operands(lin):
    """On unrounded inputs every bf16 kernel family must miss float64 by the operand rounding, no more and no less: above 1e-5
    (the fp32 kernels stay below it) and below BF16_RTOL."""
    errs = {}
    shape = (70, 40, 260)
    i = gemm_inputs(shape)
    errs["tiled"] = measure(lin.fwd(shape, i["x"], i["w"], i["bias"], precision=1, what="unrounded tiled")["y"], ref_plain(shape)["y"], "gemmshape.C.unrounded.tiled.y")
    shape = (70, 160, 192)
    i = gemm_inputs(shape)
    errs["gemm16"] = measure(lin.fwd(shape, i["x"], i["w"], i["bias"], precision=1, io=5, what="unrounded gemm16")["y"], ref_plain(shape)["y"], "gemmshape.C.unrounded.gemm16.y")
    errs["gemm16.dx"] = measure(lin.dgrad(shape, i["dy"], i["w"], precision=1, io=5, what="unrounded gemm16")["dx"], ref_plain(shape)["dx"], "gemmshape.C.unrounded.gemm16.dx")
    for shape, io in (((300, 136, 72), 0), ((320, 136, 72), 3)):
        i = gemm_inputs(shape)
        res, _, _ = lin.batch([dict(shape=shape, dy=i["dy"], x=i["x"], io=io)], precision=1, what="unrounded wgrad16")
        errs[f"wgrad16.io{io}"] = measure(res[0]["dw"], ref_plain(shape)["dw"], f"gemmshape.C.unrounded.wgrad16.io{io}.dw")
    assert all(1e-5 < e < BF16_RTOL for e in errs.values()), errs


# ------------------------------------------------------------------------------------------------
# (D) refusals touch nothing
# ------------------------------------------------------------------------------------------------
@gpu
def test_linear_refusals_touch_nothing(lin):
    """Host-side refusals: each call raises and leaves every guarded output and workspace NaN; the last call, accepted, shows that
    nothing before it left a pending reduction run or a buffer written."""
    shape = (70, 40, 260)
    M, N, K = shape
    i = gemm_inputs(shape)
    rs, rps = row_scales(M, 37), 37
    # bf16 storage without bf16 operands
    lin.fwd(shape, i["x"], i["w"], i["bias"], precision=0, io=1, refused=True, what="io 1 at precision 0")
    lin.dgrad(shape, i["dy"], i["w"], precision=0, io=2, refused=True, what="io 2 at precision 0")
    # bf16 storage with K % 4 != 0
    odd = (70, 40, 261)
    j = gemm_inputs(odd)
    lin.fwd(odd, j["x"], j["w"], j["bias"], precision=1, io=1, refused=True, what="io 1 with K % 4 != 0")
    lin.dgrad(odd, j["dy"], j["w"], precision=1, io=1, refused=True, what="io 1 with K % 4 != 0")
    # a concat input stored as bf16
    lin.fwd(shape, i["x"], i["w"], i["bias"], k_split=36, precision=1, io=1, refused=True, what="concat with io bit 0")
    # y_act together with residual
    lin.fwd(shape, i["x"], i["w"], i["bias"], act=True, residual=i["residual"], refused=True, what="y_act with residual")
    # two of dx2 / gelu_pre / add
    lin.dgrad(shape, i["dy"], i["w"], pre=i["pre"], add=i["add"], refused=True, what="gelu_pre with add")
    lin.dgrad(shape, i["dy"], i["w"], k_split=36, add=i["add"], refused=True, what="dx2 with add")
    lin.dgrad(shape, i["dy"], i["w"], k_split=36, pre=i["pre"], refused=True, what="dx2 with gelu_pre")
    # a workspace 4 bytes short
    lin.dw(shape, i["dy"], i["x"], short=4, refused=True, what="workspace 4 bytes short")
    one = dict(shape=shape, dy=i["dy"], x=i["x"])
    lin.batch([dict(one, short=4)], refused=True, what="workspace 4 bytes short")
    # five problems; mixed precisions
    lin.batch([one] * 5, refused=True, what="5 problems")
    lin.batch([one, dict(one, precision=1)], refused=True, what="mixed precisions")
    # 17 pending reductions
    jobs, outs, keep = lin.pending_jobs([one], what="17 pending")
    many = (lin.Job * 17)(*([jobs[0]] * 17))
    lin.batch([one], pending=(many, outs), refused=True, what="17 pending reductions")
    # the block tail at precision 1 with a bf16-stored problem that is not aligned (N % 4 != 0): refused before the tail's data
    # gradient is written and before the pending reduction is run
    bad, tail = (128, 30, 64), dict(dy=det_normal("gshp.refused.tail.dy", (128, 96)), w=det_normal("gshp.refused.tail.w", (96, 32)))
    b = gemm_inputs(bad, rounded=True)
    lin.batch([dict(shape=bad, dy=b["dy"], x=b["x"], io=3)], precision=1, pending=(jobs, outs), tail=tail, refused=True,
              what="bf16-stored unaligned problem under a tail")
    # the same problem, accepted: nothing above left the library in a state that refuses it
    res, _, _ = lin.batch([one], pending=(jobs, outs), what="accepted")
    check(dict(dw=measure(res[0]["dw"], ref_plain(shape)["dw"], "gemmshape.D.accepted.dw")))
