"""The attention kernels away from the models' window sizes: every 16-token tile class from 1 to 18, every forward instantiation
(fwd3 NT 4 / 6 / 7 and fwd NT 9 / 12 / 15 / 18, with and without the query split), the fused backward at NT 4 / 6 / 7 and the
two-pass backward with 2 .. 5 blocks of 64, thin stripes in all three, head dims 8 / 16 / 24 / 32 and all four storage /
arithmetic modes.

The reference is attn_ref below: float64 on the CPU, autograd for the gradients.  The metric is test_gpu_parity's
max|got - ref| / rms(ref), the bound its fp32 RTOL = 1e-3, and every measured error is appended to test_gpu_parity's error log
under a tag that names the case.  The tests at the top need no GPU: they check the reference against independently written
formulations, show that the bound sees the bugs these shapes are meant to catch, pin the transcription of the launch rules
(attn_plan) to the case table, and bound what mode 7's operand rounding may cost at these shapes."""
import functools
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import cswin_oracle as O
from oracle.determ import det_normal

from test_gpu_parity import LOG, RTOL          # the fp32 bound and the error log, neither of them new
from test_gpu_shapes import D, measure         # float64 leaf; max|got - ref| / rms(ref) in float64, printed and logged

gpu = pytest.mark.gpu
DEV = "cuda"
TUNING_VARS = ("CSWIN_ATTN_FWD_QSPLIT", "CSWIN_ATTN_BWD_TWO_PASS")     # read once per process by the library: they void attn_plan


def cid(case):
    B, reso, split, idx, C, heads = case
    return f"B{B}-r{reso}-s{split}-i{'.'.join(map(str, idx))}-C{C}-h{'.'.join(map(str, heads))}"


def bf16_round(t):
    """Nearest-even bf16 rounding of a float64 / float32 tensor, returned in the input's dtype."""
    return t.float().bfloat16().to(t.dtype)


def rel_l2(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).pow(2).sum().sqrt() / (ref.pow(2).sum().sqrt() + 1e-300))


# ------------------------------------------------------------------------------------------------
# float64 reference of cswin_attn_fwd (include/cswin_hip.h), differentiable by autograd
# ------------------------------------------------------------------------------------------------
def lepe_taps(vg, w, b):
    """Depthwise 3x3 cross-correlation of vg (M, H, W, Cb), zero padded at the border of the (H, W) grid; w (Cb, 9), b (Cb)."""
    H, W = vg.shape[1:3]
    vp = F.pad(vg, (0, 0, 1, 1, 1, 1))
    out = b
    for t in range(9):
        ky, kx = divmod(t, 3)
        out = out + vp[:, ky:ky + H, kx:kx + W, :] * w[:, t]
    return out


def attn_ref(qkv, lepe_w, lepe_b, reso, split, idx, heads, scale=None, mask=None, _wrong=None):
    """qkv (B, L, 3C) = [q | k | v]; branch i works on channels [i C/nb, (i+1) C/nb) of each with stripe mode idx[i] and heads[i]
    heads; lepe_w[i] (Cb, 9), lepe_b[i] (Cb).  mask: None, or one (B nWin, heads, N, N) factor tensor per branch that multiplies
    the probabilities.  Returns y (B, L, C), y0 (B, L, C) = (P o M) V without the LePE term and lse (B, sum(heads), L), the row
    log-sum-exp of the undropped scale q k^T at the token's position in the image.
    _wrong (the sensitivity test alone): "drop_last_key", "extra_zero_key" or "image_border_lepe"."""
    B, L, C3 = qkv.shape
    C, nb = C3 // 3, len(idx)
    Cb = C // nb
    ys, y0s, lses = [], [], []
    for i in range(nb):
        H_sp, W_sp = O.window_shape(reso, idx[i], split)
        N, h = H_sp * W_sp, heads[i]
        hd = Cb // h
        sc = scale or hd ** -0.5
        q, k, v = (qkv[..., j * C + i * Cb:j * C + (i + 1) * Cb] for j in range(3))
        heads_view = lambda t: O.img2windows(t, reso, H_sp, W_sp).reshape(-1, N, h, hd).permute(0, 2, 1, 3)      # (B', h, N, hd)
        qw, kw, vw = heads_view(q), heads_view(k), heads_view(v)
        if _wrong == "drop_last_key":
            kw, vw = kw[:, :, :-1], vw[:, :, :-1]
        s = sc * torch.einsum("whnd,whmd->whnm", qw, kw)
        lse = torch.logsumexp(s, dim=-1)                                                                       # (B', h, N)
        if _wrong == "extra_zero_key":
            lse = torch.logaddexp(lse, torch.zeros_like(lse))
        p = torch.exp(s - lse[..., None])
        if mask is not None:
            p = p * mask[i]
        y0 = O.windows2img((p @ vw).permute(0, 2, 1, 3).reshape(-1, N, Cb), reso, H_sp, W_sp)                    # (B, L, Cb)
        if _wrong == "image_border_lepe":
            lepe = lepe_taps(v.reshape(B, reso, reso, Cb), lepe_w[i], lepe_b[i]).reshape(B, L, Cb)
        else:
            vg = O.img2windows(v, reso, H_sp, W_sp).reshape(-1, H_sp, W_sp, Cb)
            lepe = O.windows2img(lepe_taps(vg, lepe_w[i], lepe_b[i]).reshape(-1, N, Cb), reso, H_sp, W_sp)
        ys.append(y0 + lepe)
        y0s.append(y0)
        lses.append(O.windows2img(lse.permute(0, 2, 1), reso, H_sp, W_sp).permute(0, 2, 1))                      # (B, h, L)
    return torch.cat(ys, 2), torch.cat(y0s, 2), torch.cat(lses, 1)


# ------------------------------------------------------------------------------------------------
# launch plan
# ------------------------------------------------------------------------------------------------
# A transcription of the launch rules of cswin_unet_amd/csrc/attn_plan.h, the header attn.hip launches from: ap::geometry (window
# shape, units, nt = ceil(N / 16)), ap::nt_class (the instantiated tile classes), ap::fwd_plan (the family and the query split:
# one wave per tile and NT >= 6: nwg < 1024 && nwg % 256 != 0; larger windows: nwg <= 256) and ap::bwd_plan (two_pass = nt > 7,
# nblk = ceil(N / 64)), with neither tuning variable set.  `thin` is the kernels' own br.H_sp == 1 || br.W_sp == 1.
# tests/test_attn_plan_host.py (no GPU) holds it to the header, field by field, through tools/attn_plan_check.cpp.
def attn_plan(B, reso, split, idx, C, heads):
    nwg, N, thin = 0, None, False
    for i, h in zip(idx, heads):
        H_sp, W_sp = O.window_shape(reso, i, split)
        assert reso % H_sp == 0 and reso % W_sp == 0 and N in (None, H_sp * W_sp)
        N = H_sp * W_sp
        nwg += B * (reso // H_sp) * (reso // W_sp) * h
        thin = thin or H_sp == 1 or W_sp == 1
    hd = C // len(idx) // heads[0]
    assert C == len(idx) * heads[0] * hd and all(h == heads[0] for h in heads) and hd in (8, 16, 24, 32)
    nt = (N + 15) // 16
    assert 1 <= nt <= 18
    if nt <= 7:
        NT = 4 if nt <= 4 else 6 if nt <= 6 else 7
        fwd = ("fwd3", NT, 2 if NT >= 6 and nwg < 1024 and nwg % 256 != 0 else 1)
        bwd = ("bwd3", NT)
    else:
        NT = 9 if nt <= 9 else 12 if nt <= 12 else 15 if nt <= 15 else 18
        fwd = ("fwd", NT, 2 if nwg <= 256 else 1)
        bwd = ("two_pass", (N + 63) // 64)
    return dict(N=N, nt=nt, last_tile=N - 16 * (nt - 1), nwg=nwg, fwd=fwd, bwd=bwd, thin=thin, hd=hd)


# (B, reso, split, idx per branch, C, heads per branch), and beside each row what the dispatch rules give for it: N, ceil(N / 16),
# nwg, the forward instantiation and the backward.  The figures are computed from the rules, not read off a device;
# test_case_table_reaches_every_instantiation holds attn_plan to them.
CASES = [
    ((2, 3, 3, (-1,), 24, (3,)),        (9, 1, 6, ("fwd3", 4, 1), ("bwd3", 4))),          # three padded tiles
    ((3, 4, 4, (-1,), 32, (1,)),        (16, 1, 3, ("fwd3", 4, 1), ("bwd3", 4))),         # hd 32
    ((2, 5, 5, (-1,), 48, (2,)),        (25, 2, 4, ("fwd3", 4, 1), ("bwd3", 4))),         # hd 24
    ((2, 12, 3, (0, 1), 32, (2, 2)),    (36, 3, 32, ("fwd3", 4, 1), ("bwd3", 4))),
    ((2, 8, 8, (-1,), 64, (2,)),        (64, 4, 4, ("fwd3", 4, 1), ("bwd3", 4))),         # full
    ((5, 15, 5, (0, 1), 48, (3, 3)),    (75, 5, 90, ("fwd3", 6, 2), ("bwd3", 6))),        # divisors 3, 3, 5
    ((1, 20, 4, (0, 1), 16, (1, 1)),    (80, 5, 10, ("fwd3", 6, 2), ("bwd3", 6))),        # full; tile 6 all padding
    ((2, 9, 9, (-1,), 24, (3,)),        (81, 6, 6, ("fwd3", 6, 2), ("bwd3", 6))),         # 1 token in last tile
    ((8, 9, 9, (-1,), 256, (32,)),      (81, 6, 256, ("fwd3", 6, 1), ("bwd3", 6))),       # % 256 clause
    ((1, 97, 1, (0, 1), 16, (1, 1)),    (97, 7, 194, ("fwd3", 7, 2), ("bwd3", 7))),       # thin, 1 token in last tile
    ((2, 10, 10, (-1,), 80, (5,)),      (100, 7, 10, ("fwd3", 7, 2), ("bwd3", 7))),       # hd 16
    ((8, 10, 10, (-1,), 256, (32,)),    (100, 7, 256, ("fwd3", 7, 1), ("bwd3", 7))),
    ((8, 28, 4, (1,), 152, (19,)),      (112, 7, 1064, ("fwd3", 7, 1), ("bwd3", 7))),     # >= 1024 clause, full, nWin 7
    ((1, 28, 4, (0, 1), 64, (1, 1)),    (112, 7, 14, ("fwd3", 7, 2), ("bwd3", 7))),       # hd 32
    ((1, 113, 1, (0, 1), 16, (1, 1)),   (113, 8, 226, ("fwd", 9, 2), ("two_pass", 2))),   # thin; tile 9 all padding
    ((2, 11, 11, (-1,), 56, (7,)),      (121, 8, 14, ("fwd", 9, 2), ("two_pass", 2))),
    ((3, 11, 11, (-1,), 768, (96,)),    (121, 8, 288, ("fwd", 9, 1), ("two_pass", 2))),
    ((2, 16, 8, (0, 1), 128, (2, 2)),   (128, 8, 16, ("fwd", 9, 2), ("two_pass", 2))),    # full blocks, hd 32
    ((1, 66, 2, (0, 1), 16, (1, 1)),    (132, 9, 66, ("fwd", 9, 2), ("two_pass", 3))),    # 4 tokens in last tile and block
    ((1, 129, 1, (1,), 8, (1,)),        (129, 9, 129, ("fwd", 9, 2), ("two_pass", 3))),   # thin; 1 token in last tile and block
    ((1, 40, 4, (1,), 24, (1,)),        (160, 10, 10, ("fwd", 12, 2), ("two_pass", 3))),  # hd 24
    ((2, 13, 13, (-1,), 24, (3,)),      (169, 11, 6, ("fwd", 12, 2), ("two_pass", 3))),
    ((11, 24, 8, (0,), 64, (8,)),       (192, 12, 264, ("fwd", 12, 1), ("two_pass", 3))),
    ((1, 193, 1, (0,), 8, (1,)),        (193, 13, 193, ("fwd", 15, 2), ("two_pass", 4))),  # thin; 1 token in last tile and block
    ((1, 56, 4, (0, 1), 16, (1, 1)),    (224, 14, 28, ("fwd", 15, 2), ("two_pass", 4))),  # full
    ((2, 15, 15, (-1,), 16, (1,)),      (225, 15, 2, ("fwd", 15, 2), ("two_pass", 4))),   # hd 16, 1 token in last tile
    ((17, 15, 15, (-1,), 128, (16,)),   (225, 15, 272, ("fwd", 15, 1), ("two_pass", 4))),
    ((9, 16, 16, (-1,), 256, (32,)),    (256, 16, 288, ("fwd", 18, 1), ("two_pass", 4))),
    ((1, 257, 1, (1,), 8, (1,)),        (257, 17, 257, ("fwd", 18, 1), ("two_pass", 5))),  # thin; 1 token in last tile and block
    ((1, 68, 4, (0, 1), 16, (1, 1)),    (272, 17, 34, ("fwd", 18, 2), ("two_pass", 5))),
    ((2, 24, 12, (0, 1), 48, (1, 1)),   (288, 18, 8, ("fwd", 18, 2), ("two_pass", 5))),   # hd 24, the largest window
]
ROWS = [c for c, _ in CASES]
ROW = {plan[0]: case for case, plan in reversed(CASES)}        # first row of each window size
PEAKED = [ROWS[-1], (2, 9, 9, (-1,), 24, (3,))]                # also run with q and k times 3: scores of standard deviation ~9
SCALED = (2, 12, 3, (0, 1), 32, (2, 2))                        # also run with an explicit scale = 0.2
# (case, factor on q and k, scale) of the fp32 parity test
RUNS = [(c, 1, None) for c in ROWS] + [(c, 3, None) for c in PEAKED] + [(SCALED, 1, 0.2)]
AUTOGRAD_ROWS = [(2, 12, 3, (0, 1), 32, (2, 2)), (5, 15, 5, (0, 1), 48, (3, 3)), (1, 113, 1, (0, 1), 16, (1, 1)),
                 (2, 9, 9, (-1,), 24, (3,)), (2, 13, 13, (-1,), 24, (3,)), (2, 15, 15, (-1,), 16, (1,))]
# one row per forward instantiation and per backward path (test_mode_subset_reaches_every_instantiation), head dims 8, 16 and
# 24 in both kernel families
MODE_ROWS = [
    (2, 5, 5, (-1,), 48, (2,)),          # fwd3<4,1>  bwd3<4>     hd 24
    (5, 15, 5, (0, 1), 48, (3, 3)),      # fwd3<6,2>  bwd3<6>     hd 8
    (8, 9, 9, (-1,), 256, (32,)),        # fwd3<6,1>
    (1, 97, 1, (0, 1), 16, (1, 1)),      # fwd3<7,2>  bwd3<7>     thin
    (2, 10, 10, (-1,), 80, (5,)),        # fwd3<7,2>              hd 16
    (8, 10, 10, (-1,), 256, (32,)),      # fwd3<7,1>
    (2, 16, 8, (0, 1), 128, (2, 2)),     # fwd<9,2>   two_pass 2  hd 32
    (3, 11, 11, (-1,), 768, (96,)),      # fwd<9,1>               hd 8
    (1, 40, 4, (1,), 24, (1,)),          # fwd<12,2>  two_pass 3  hd 24
    (11, 24, 8, (0,), 64, (8,)),         # fwd<12,1>
    (2, 15, 15, (-1,), 16, (1,)),        # fwd<15,2>  two_pass 4  hd 16
    (17, 15, 15, (-1,), 128, (16,)),     # fwd<15,1>
    (1, 257, 1, (1,), 8, (1,)),          # fwd<18,1>  two_pass 5  thin
    (2, 24, 12, (0, 1), 48, (1, 1)),     # fwd<18,2>              hd 24
]
DROP_ROWS = [ROW[75], (2, 9, 9, (-1,), 24, (3,)), (8, 9, 9, (-1,), 256, (32,)), ROW[97], ROW[121], ROW[132], ROW[225]]
# test_bound_sees_the_bugs_these_shapes_are_for asks for inputs at which the bound sees each bug.  At 288 keys one extra key of
# score 0 takes 1 / (1 + 288 e^0.5) = 0.2 % of a row: 0.0099 in the suite's metric at the row's first draw, 0.0111 at its second.
DRAW = {ROWS[-1]: ".1"}
ALL_FWD = [("fwd3", 4, 1)] + [("fwd3", nt, qs) for nt in (6, 7) for qs in (1, 2)] + [("fwd", nt, qs) for nt in (9, 12, 15, 18) for qs in (1, 2)]
ALL_BWD = [("bwd3", nt) for nt in (4, 6, 7)] + [("two_pass", n) for n in (2, 3, 4, 5)]


def attn_inputs(case, qk_mul=1):
    """qkv (unit variance; q and k times qk_mul), lepe_w[i] (Cb, 9) ~ 0.3, lepe_b[i] (Cb) ~ 0.1, dy; float32 numpy."""
    B, reso, split, idx, C, heads = case
    tag, Cb = "ashp." + cid(case) + DRAW.get(case, ""), C // len(idx)
    qkv = det_normal(tag + ".qkv", (B, reso * reso, 3 * C))
    qkv[..., :2 * C] *= qk_mul
    lw = [det_normal(f"{tag}.lw{i}", (Cb, 9), 0.3) for i in range(len(idx))]
    lb = [det_normal(f"{tag}.lb{i}", (Cb,), 0.1) for i in range(len(idx))]
    return qkv, lw, lb, det_normal(tag + ".dy", (B, reso * reso, C))


def reference(case, qkv, lw, lb, dy, scale=None, mask=None):
    """{y, y0, lse, dq, dk, dv, dlepe_w<i>, dlepe_b<i>} of attn_ref in float64 on float32 numpy inputs."""
    B, reso, split, idx, C, heads = case
    qr, wr, br = D(qkv), [D(a) for a in lw], [D(a) for a in lb]
    y, y0, lse = attn_ref(qr, wr, br, reso, split, idx, heads, scale, mask)
    y.backward(torch.from_numpy(dy).double())
    ref = dict(y=y.detach(), y0=y0.detach(), lse=lse.detach(), dq=qr.grad[..., :C], dk=qr.grad[..., C:2 * C], dv=qr.grad[..., 2 * C:])
    for i in range(len(idx)):
        ref[f"dlepe_w{i}"], ref[f"dlepe_b{i}"] = wr[i].grad, br[i].grad
    return ref


@functools.lru_cache(maxsize=None)
def attn_problem(case, qk_mul=1, scale=None):
    """(inputs, float64 reference) of one run; computed once, shared by the tests that use it, never written."""
    inputs = attn_inputs(case, qk_mul)
    return inputs, reference(case, *inputs, scale=scale)


# ------------------------------------------------------------------------------------------------
# the reference against independent formulations, and what the bound can see (no GPU)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,scale", [((2, 6, 3, (0, 1), 32, (2, 2)), None), ((1, 5, 5, (-1,), 24, (3,)), 0.2), ((2, 9, 1, (1,), 8, (1,)), None)], ids=str)
def test_attn_ref_agrees_with_the_oracle(case, scale):
    """attn_ref (explicit taps, einsum, exp of s - lse) against O.lepe_attention (F.conv2d, torch.softmax), float64, per branch."""
    B, reso, split, idx, C, heads = case
    qkv, lw, lb, _ = (attn_inputs(case))
    qkv, lw, lb = torch.from_numpy(qkv).double(), [torch.from_numpy(a).double() for a in lw], [torch.from_numpy(a).double() for a in lb]
    y, y0, _ = attn_ref(qkv, lw, lb, reso, split, idx, heads, scale)
    Cb = C // len(idx)
    want = torch.cat([O.lepe_attention(*(qkv[..., j * C + i * Cb:j * C + (i + 1) * Cb] for j in range(3)), lw[i].view(Cb, 1, 3, 3), lb[i],
                                       reso, idx[i], split, heads[i], scale) for i in range(len(idx))], 2)
    assert float((y - want).abs().max()) <= 1e-12
    zero_w, zero_b = [torch.zeros_like(a) for a in lw], [torch.zeros_like(a) for a in lb]
    assert float((attn_ref(qkv, zero_w, zero_b, reso, split, idx, heads, scale)[0] - y0).abs().max()) <= 1e-12        # y0 is y without LePE


@pytest.mark.parametrize("case,scale", [((2, 6, 3, (0, 1), 32, (2, 2)), None), ((1, 5, 5, (-1,), 24, (3,)), 0.2), ((2, 9, 1, (1,), 8, (1,)), None)], ids=str)
def test_attn_ref_lse_against_brute_force(case, scale):
    B, reso, split, idx, C, heads = case
    qkv = torch.from_numpy(attn_inputs(case)[0]).double()
    zeros = [torch.zeros(C // len(idx), 9).double() for _ in idx], [torch.zeros(C // len(idx)).double() for _ in idx]
    lse = attn_ref(qkv, *zeros, reso, split, idx, heads, scale)[2]
    want, Cb, head0 = torch.full_like(lse, float("nan")), C // len(idx), 0
    for i in range(len(idx)):
        g = torch.from_numpy(O.stripe_gather_index(reso, *O.window_shape(reso, idx[i], split)).astype(np.int64))     # [nWin, N] image tokens
        hd = Cb // heads[i]
        for b in range(B):
            for w in range(g.shape[0]):
                for h in range(heads[i]):
                    ch = i * Cb + h * hd
                    s = (scale or hd ** -0.5) * qkv[b, g[w], ch:ch + hd] @ qkv[b, g[w], C + ch:C + ch + hd].t()
                    want[b, head0 + h, g[w]] = torch.logsumexp(s, dim=-1)
        head0 += heads[i]
    assert lse.shape == (B, sum(heads), reso * reso) and float((lse - want).abs().max()) <= 1e-12


@pytest.mark.parametrize("case", ROWS, ids=cid)
def test_bound_sees_the_bugs_these_shapes_are_for(case):
    """A padded key that leaks into the softmax, a real key that is masked out, and a LePE tap that crosses a window border each
    move y0 or y by more than 10 RTOL in the suite's metric, at every row."""
    B, reso, split, idx, C, heads = case
    qkv, lw, lb, _ = attn_inputs(case)
    args = (torch.from_numpy(qkv).double(), [torch.from_numpy(a).double() for a in lw], [torch.from_numpy(a).double() for a in lb], reso, split, idx, heads)
    y, y0, _ = attn_ref(*args)
    metric = lambda got, ref: float((got - ref).abs().max() / ref.pow(2).mean().sqrt())
    wrongs = ["drop_last_key", "extra_zero_key"]
    if any(O.window_shape(reso, i, split) != (reso, reso) for i in idx):
        wrongs.append("image_border_lepe")                   # more than one window per image
    for wrong in wrongs:
        yw, y0w, _ = attn_ref(*args, _wrong=wrong)
        seen = max(metric(yw, y), metric(y0w, y0))
        print(f"{cid(case)} {wrong}: {seen:.3e}")
        assert seen > 10 * RTOL, (wrong, seen)


def test_case_table_reaches_every_instantiation():
    assert len(CASES) == 31 and len(set(ROWS)) == 31
    plans = []
    for case, (N, nt, nwg, fwd, bwd) in CASES:
        p = attn_plan(*case)
        assert (p["N"], p["nt"], p["nwg"], p["fwd"], p["bwd"]) == (N, nt, nwg, fwd, bwd), cid(case)
        plans.append(p)
    assert {p["fwd"] for p in plans} == set(ALL_FWD) and len(ALL_FWD) == 13
    assert {p["bwd"] for p in plans} == set(ALL_BWD)
    assert {p["nt"] for p in plans} == set(range(1, 19))
    for NT in (4, 6, 7, 9, 12, 15, 18):
        mine = [p for p in plans if p["fwd"][1] == NT]
        assert any(p["last_tile"] == 16 for p in mine), f"NT {NT}: no row with a full last tile"
        assert any(1 <= p["last_tile"] <= 15 for p in mine), f"NT {NT}: no row with a ragged last tile"
    assert any(p["bwd"][0] == "two_pass" and p["N"] % 64 == 1 for p in plans)
    for kind, key in (("fwd3", "fwd"), ("fwd", "fwd"), ("two_pass", "bwd")):
        assert any(p["thin"] and p[key][0] == kind for p in plans), f"no thin stripe in {kind}"
    for hd in (8, 16, 24, 32):
        assert any(p["hd"] == hd and p["fwd"][0] == "fwd3" for p in plans), f"head dim {hd} not in fwd3 / bwd3"
        assert any(p["hd"] == hd and p["fwd"][0] == "fwd" for p in plans), f"head dim {hd} not in fwd / two_pass"
    small = [p for p in plans if p["fwd"][0] == "fwd3" and p["fwd"][1] >= 6 and p["fwd"][2] == 1]
    assert any(p["nwg"] >= 1024 for p in small) and any(p["nwg"] < 1024 and p["nwg"] % 256 == 0 for p in small)
    for rows in (PEAKED, [SCALED], AUTOGRAD_ROWS, MODE_ROWS, DROP_ROWS):
        assert set(rows) <= set(ROWS)
    assert sum(len(c[3]) == 2 for c in AUTOGRAD_ROWS) == 3 and len(AUTOGRAD_ROWS) == 6


def test_mode_subset_reaches_every_instantiation():
    plans = [attn_plan(*c) for c in MODE_ROWS]
    assert {p["fwd"] for p in plans} == set(ALL_FWD) and {p["bwd"] for p in plans} == set(ALL_BWD)
    for hd in (8, 16, 24):
        assert any(p["hd"] == hd and p["fwd"][0] == "fwd3" for p in plans) and any(p["hd"] == hd and p["fwd"][0] == "fwd" for p in plans)
    drop = [attn_plan(*c) for c in DROP_ROWS]
    assert [p["N"] for p in drop] == [75, 81, 81, 97, 121, 132, 225] and {p["fwd"][2] for p in drop if p["N"] == 81} == {1, 2}


# ------------------------------------------------------------------------------------------------
# float64 emulation of mode 7 (bf16 matrix instructions) beside mode 3
# ------------------------------------------------------------------------------------------------
M7_BOUNDS = dict(y=5e-3, lse=1e-3, dqkv=8e-3)      # test_attention_bf16_matrix_instructions_vs_fp32's, relative L2


def attn_bf16_emulation(case, qkv, lw, lb, dy, operands16):
    """cswin_attn_fwd + cswin_attn_bwd with bf16-valued q, k, v and y, y0, dqkv stored as bf16 (modes 3 and 7), everything else
    in float64.  operands16: the scaled q, P, dO and dS are rounded to bf16 where they enter a matrix product, as the header says
    of mode 7 (k and v hold bf16 values already); accumulators, softmax statistics, delta, LePE and its transpose are not.
    Returns {y, lse, dqkv} (the LePE parameter gradients do not pass through a matrix product)."""
    B, reso, split, idx, C, heads = case
    rnd = bf16_round if operands16 else (lambda t: t)
    Cb = C // len(idx)
    ys, lses, dq, dk, dv = [], [], [], [], []
    for i in range(len(idx)):
        H_sp, W_sp = O.window_shape(reso, idx[i], split)
        N, h = H_sp * W_sp, heads[i]
        hd = Cb // h
        scale = float(np.float32(hd) ** np.float32(-0.5))
        to_win = lambda t: O.img2windows(t, reso, H_sp, W_sp)
        to_heads = lambda t: to_win(t).reshape(-1, N, h, hd).permute(0, 2, 1, 3)
        to_img = lambda t: O.windows2img(t.permute(0, 2, 1, 3).reshape(-1, N, Cb), reso, H_sp, W_sp)
        q, k, v = (qkv[..., j * C + i * Cb:j * C + (i + 1) * Cb] for j in range(3))
        dO_img = dy[..., i * Cb:(i + 1) * Cb]
        qs, kw, vw, dO = rnd(to_heads(q) * scale), to_heads(k), to_heads(v), to_heads(dO_img)
        s = qs @ kw.transpose(-1, -2)
        lse = torch.logsumexp(s, dim=-1)
        p = torch.exp(s - lse[..., None])
        y0 = rnd(p) @ vw
        vg = to_win(v).reshape(-1, H_sp, W_sp, Cb).clone().requires_grad_()
        lepe = lepe_taps(vg, lw[i], lb[i])
        lepe.backward(to_win(dO_img).reshape(-1, H_sp, W_sp, Cb))
        ys.append(bf16_round(to_img(y0) + O.windows2img(lepe.detach().reshape(-1, N, Cb), reso, H_sp, W_sp)))
        lses.append(O.windows2img(lse.permute(0, 2, 1), reso, H_sp, W_sp).permute(0, 2, 1))
        delta = (dO * bf16_round(y0)).sum(-1, keepdim=True)                    # y0 is read back as stored
        dS = rnd(p * (rnd(dO) @ vw.transpose(-1, -2) - delta))
        dq.append(to_img(scale * (dS @ kw)))
        dk.append(to_img(dS.transpose(-1, -2) @ qs))
        dv.append(to_img(rnd(p).transpose(-1, -2) @ rnd(dO)) + O.windows2img(vg.grad.reshape(-1, N, Cb), reso, H_sp, W_sp))
    return dict(y=torch.cat(ys, 2), lse=torch.cat(lses, 1), dqkv=bf16_round(torch.cat(dq + dk + dv, 2)))


@functools.lru_cache(maxsize=None)
def mode7_emulated_distance(case):
    qkv, lw, lb, dy = attn_inputs(case)
    args = (bf16_round(torch.from_numpy(qkv)).double(), [torch.from_numpy(a).double() for a in lw], [torch.from_numpy(a).double() for a in lb],
            torch.from_numpy(dy).double())
    plain, rounded = attn_bf16_emulation(case, *args, operands16=False), attn_bf16_emulation(case, *args, operands16=True)
    return {k: rel_l2(rounded[k], plain[k]) for k in M7_BOUNDS}


@pytest.mark.parametrize("case", MODE_ROWS, ids=cid)
def test_mode7_bounds_leave_room_at_these_shapes(case):
    """The mode-7 bounds were measured at hd = 32 and N >= 49.  The rounding they allow for, emulated in float64 at each row of
    the subset, must stay under half of them, so that a failure of the GPU test is a defect and not a tight bound."""
    dist = mode7_emulated_distance(case)
    print(cid(case), "mode-7 emulation:", {k: f"{v:.3e}" for k, v in dist.items()})
    for k, bound in M7_BOUNDS.items():
        assert dist[k] < bound / 2, (k, dist[k])


# ------------------------------------------------------------------------------------------------
# the entry points, called directly with guarded buffers
# ------------------------------------------------------------------------------------------------
GUARD = 64        # elements of NaN before and after every output: 256 B (128 B for bf16), so the view stays 16-byte aligned


class Guarded:
    """A NaN-filled buffer with GUARD elements before and after the view `.t` that the kernels are given."""

    def __init__(self, shape, dtype=torch.float32):
        self.n = math.prod(shape)
        self.buf = torch.full((self.n + 2 * GUARD,), float("nan"), dtype=dtype, device=DEV)
        self.t = self.buf[GUARD:GUARD + self.n].view(shape)
        assert self.t.data_ptr() % 16 == 0

    def intact(self):
        return bool(torch.isnan(self.buf[:GUARD]).all()) and bool(torch.isnan(self.buf[GUARD + self.n:]).all())

    def untouched(self):
        return bool(torch.isnan(self.buf).all())

    def written(self):
        return not bool(torch.isnan(self.t).any())


def settle(what, bufs, untouched=False):
    torch.cuda.synchronize()
    for name, g in bufs.items():
        if untouched:
            assert g.untouched(), f"{what}: {name} was written by a refused call"
        else:
            assert g.intact(), f"{what}: a guard word of {name} was overwritten"
            assert name == "workspace" or g.written(), f"{what}: {name} has elements that were never written"


@pytest.fixture(scope="module")
def attn():
    """The direct-call helpers; skips when a tuning variable makes the library depart from attn_plan."""
    present = [v for v in TUNING_VARS if v in os.environ]
    if present:
        pytest.skip(f"{', '.join(present)} set: the launch plan these tests rely on does not hold")
    from cswin_unet_amd._lib import CswinHipError, call, lib, ptr, stream
    from cswin_unet_amd.ops import _int_array, _ptr_array

    class Attn:
        Error = CswinHipError

        @staticmethod
        def dev(qkv, lw, lb, dy, mode=0):
            """Device copies of numpy inputs in the storage format of `mode`."""
            f = lambda a: torch.from_numpy(np.ascontiguousarray(a)).float().to(DEV)
            return (f(qkv).bfloat16() if mode else f(qkv)), [f(a) for a in lw], [f(a) for a in lb], f(dy)

        @staticmethod
        def outputs_fwd(case, mode):
            B, reso, split, idx, C, heads = case
            odt = torch.bfloat16 if mode & 2 else torch.float32
            return dict(y=Guarded((B, reso * reso, C), odt), y0=Guarded((B, reso * reso, C), odt), lse=Guarded((B, sum(heads), reso * reso)))

        @staticmethod
        def outputs_bwd(case, mode, ws_bytes=None):
            B, reso, split, idx, C, heads = case
            Cb = C // len(idx)
            nbytes = lib().cswin_attn_bwd_workspace(B, reso, C, len(idx), _int_array(heads), _int_array(idx), split) if ws_bytes is None else ws_bytes
            assert nbytes > 0 and nbytes % 4 == 0
            out = dict(dqkv=Guarded((B, reso * reso, 3 * C), torch.bfloat16 if mode & 1 else torch.float32), workspace=Guarded((nbytes // 4,)))
            for i in range(len(idx)):
                out[f"dlepe_w{i}"], out[f"dlepe_b{i}"] = Guarded((Cb, 9)), Guarded((Cb,))
            return out, nbytes

        @staticmethod
        def call_fwd(case, mode, qkv, lw, lb, o, scale=None, drop=(0.0, 0)):
            B, reso, split, idx, C, heads = case
            call("cswin_attn_fwd", ptr(qkv), _ptr_array(lw), _ptr_array(lb), ptr(o["y"].t), ptr(o["y0"].t), ptr(o["lse"].t), B, reso, C, len(idx),
                 _int_array(heads), _int_array(idx), split, float(scale or 0.0), drop[0], drop[1], None, mode, stream())

        @staticmethod
        def call_bwd(case, mode, qkv, lw, lb, lse, y0, dy, o, ws_bytes, scale=None, drop=(0.0, 0)):
            B, reso, split, idx, C, heads = case
            n = len(idx)
            call("cswin_attn_bwd", ptr(qkv), _ptr_array(lw), _ptr_array(lb), ptr(lse), ptr(y0), ptr(dy), ptr(o["dqkv"].t),
                 _ptr_array([o[f"dlepe_w{i}"].t for i in range(n)]), _ptr_array([o[f"dlepe_b{i}"].t for i in range(n)]), ptr(o["workspace"].t),
                 ws_bytes, B, reso, C, n, _int_array(heads), _int_array(idx), split, float(scale or 0.0), None, drop[0], drop[1], None, mode, stream())

        @classmethod
        def fwd(cls, case, mode, qkv, lw, lb, scale=None, drop=(0.0, 0)):
            """(y, y0, lse) of cswin_attn_fwd; guards checked, every element written."""
            o = cls.outputs_fwd(case, mode)
            cls.call_fwd(case, mode, qkv, lw, lb, o, scale, drop)
            settle(f"attn_fwd mode {mode} {cid(case)}", o)
            return o["y"].t, o["y0"].t, o["lse"].t

        @classmethod
        def bwd(cls, case, mode, qkv, lw, lb, lse, y0, dy, scale=None, drop=(0.0, 0)):
            """{dqkv, dlepe_w<i>, dlepe_b<i>} of cswin_attn_bwd with a workspace of exactly cswin_attn_bwd_workspace() bytes."""
            o, nbytes = cls.outputs_bwd(case, mode)
            cls.call_bwd(case, mode, qkv, lw, lb, lse, y0, dy, o, nbytes, scale, drop)
            settle(f"attn_bwd mode {mode} {cid(case)}", o)
            return {k: g.t for k, g in o.items() if k != "workspace"}

    return Attn


def compare_all(tag, case, y, y0, lse, grads, ref):
    """Every tensor the entry points write against the reference: {name: error}, each logged under tag.name."""
    C = case[4]
    got = dict(y=y, y0=y0, lse=lse, dq=grads["dqkv"][..., :C], dk=grads["dqkv"][..., C:2 * C], dv=grads["dqkv"][..., 2 * C:])
    got.update({k: v for k, v in grads.items() if k != "dqkv"})
    assert set(got) == set(ref)
    return {k: measure(got[k], ref[k], f"{tag}.{k}") for k in sorted(got)}


def assert_all_within(errs, bound):
    assert all(np.isfinite(e) and e <= bound for e in errs.values()), errs


def run_id(run):
    case, qk_mul, scale = run
    return cid(case) + (f"-qk{qk_mul}" if qk_mul != 1 else "") + (f"-scale{scale}" if scale else "")


@gpu
@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_attention_fp32_everything_written_vs_float64(attn, run):
    """(a) mode 0: y, y0, lse, dq, dk, dv and the LePE gradients at RTOL, each a view into a NaN-filled buffer whose guard words
    must survive, the workspace exactly as large as cswin_attn_bwd_workspace() says."""
    case, qk_mul, scale = run
    inputs, ref = attn_problem(case, qk_mul, scale)
    qkv, lw, lb, dy = attn.dev(*inputs)
    y, y0, lse = attn.fwd(case, 0, qkv, lw, lb, scale)
    grads = attn.bwd(case, 0, qkv, lw, lb, lse, y0, dy, scale)
    assert_all_within(compare_all("attnshape." + run_id(run), case, y, y0, lse, grads, ref), RTOL)


@gpu
@pytest.mark.parametrize("case", AUTOGRAD_ROWS, ids=cid)
def test_stripe_attention_autograd_vs_float64(attn, case):
    """(b) ops.stripe_attention with .backward: _StripeAttention's own allocation and the reduction of the LePE slabs."""
    from cswin_unet_amd import ops
    B, reso, split, idx, C, heads = case
    inputs, ref = attn_problem(case)
    qkv, lw, lb, dy = attn.dev(*inputs)
    qkv.requires_grad_()
    lw4 = [w.view(-1, 1, 3, 3).clone().requires_grad_() for w in lw]
    lb = [b.requires_grad_() for b in lb]
    y = ops.stripe_attention(qkv, reso, split, list(idx), list(heads), lw4, lb)
    y.backward(dy)
    got = dict(y=y, dq=qkv.grad[..., :C], dk=qkv.grad[..., C:2 * C], dv=qkv.grad[..., 2 * C:])
    for i in range(len(idx)):
        got[f"dlepe_w{i}"], got[f"dlepe_b{i}"] = lw4[i].grad.view(-1, 9), lb[i].grad
    assert_all_within({k: measure(v, ref[k], f"attnshape.autograd.{cid(case)}.{k}") for k, v in got.items()}, RTOL)


def bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def same_bits(a, b):
    return a.dtype == b.dtype and bool((bits(a) == bits(b)).all())


@gpu
@pytest.mark.parametrize("case", MODE_ROWS, ids=cid)
def test_attention_storage_modes_bit_exact(attn, case):
    """(c) the assertions of test_attention_bf16_qkv_storage_bit_exact and test_attention_bf16_y_storage_bit_exact at one row per
    forward instantiation and backward path.  Mode 1 against mode 0 on bf16-valued q, k, v: same y, y0, lse and LePE gradients,
    dqkv the rounded fp32 dqkv.  Mode 3 against mode 1: y, y0 the rounded fp32 ones, same lse, and the backward fed the bf16 y0
    equal to the mode-1 backward fed the same values widened."""
    qkv16, lw, lb, dy = attn.dev(*attn_inputs(case), mode=1)
    qkv32 = qkv16.float()
    y_0, z_0, lse_0 = attn.fwd(case, 0, qkv32, lw, lb)
    y_1, z_1, lse_1 = attn.fwd(case, 1, qkv16, lw, lb)
    assert same_bits(y_1, y_0) and same_bits(z_1, z_0) and same_bits(lse_1, lse_0), "mode 1 forward differs from mode 0"
    g_0 = attn.bwd(case, 0, qkv32, lw, lb, lse_0, z_0, dy)
    g_1 = attn.bwd(case, 1, qkv16, lw, lb, lse_1, z_1, dy)
    for k in g_0:
        assert same_bits(g_1[k], g_0[k].bfloat16() if k == "dqkv" else g_0[k]), f"mode 1 {k} differs from mode 0"
    y_3, z_3, lse_3 = attn.fwd(case, 3, qkv16, lw, lb)
    assert same_bits(y_3, y_1.bfloat16()) and same_bits(z_3, z_1.bfloat16()) and same_bits(lse_3, lse_1), "mode 3 forward is not the rounded mode 1"
    g_3 = attn.bwd(case, 3, qkv16, lw, lb, lse_3, z_3, dy)
    g_1w = attn.bwd(case, 1, qkv16, lw, lb, lse_3, z_3.float(), dy)
    for k in g_3:
        assert same_bits(g_3[k], g_1w[k]), f"mode 3 {k} differs from mode 1 fed the widened y0"


@gpu
@pytest.mark.parametrize("case", MODE_ROWS, ids=cid)
def test_attention_bf16_matrix_instructions_at_these_shapes(attn, case):
    """(d) mode 7 against mode 3 at the bounds of test_attention_bf16_matrix_instructions_vs_fp32 (relative L2: y 5e-3, lse 1e-3,
    dqkv 8e-3, LePE gradients 1e-6), which test_mode7_bounds_leave_room_at_these_shapes shows to leave a factor 2 here."""
    qkv16, lw, lb, dy = attn.dev(*attn_inputs(case), mode=1)
    res = {}
    for mode in (3, 7):
        y, z, lse = attn.fwd(case, mode, qkv16, lw, lb)
        res[mode] = dict(attn.bwd(case, mode, qkv16, lw, lb, lse, z, dy), y=y, lse=lse)
    emu = mode7_emulated_distance(case)
    bounds = dict(M7_BOUNDS, **{k: 1e-6 for k in res[3] if k.startswith("dlepe")})
    errs = {k: rel_l2(res[7][k], res[3][k]) for k in bounds}
    with open(LOG, "a") as f:
        for k, e in errs.items():
            f.write(f"attnshape.m7.{cid(case)}.{k} l2 {e:.3e}" + (f" (float64 emulation {emu[k]:.3e})\n" if k in emu else "\n"))
    print(cid(case), errs)
    assert all(errs[k] < bounds[k] for k in bounds), errs
    assert not (same_bits(res[7]["y"], res[3]["y"]) and same_bits(res[7]["dqkv"], res[3]["dqkv"])), "mode 7 is bit-identical to mode 3"


def extract_mask(attn, case, p, seed):
    """The dropout factors the forward kernel applies, one (B nWin, heads, N, N) float64 tensor per branch.  q = k = 0 makes P
    uniformly 1 / N, the LePE parameters are zero, and in launch j the token with in-window index n carries v = 1 in channel d of
    every head when n = j hd + d: then y[query, h hd + d] N is the factor of (query, key j hd + d) of head h."""
    B, reso, split, idx, C, heads = case
    plan, nb, L = attn_plan(*case), len(idx), reso * reso
    N, hd, Cb = plan["N"], plan["hd"], C // nb
    shapes = [O.window_shape(reso, i, split) for i in idx]
    n_of_l = []                                                    # in-window index of image token l, per branch
    for H_sp, W_sp in shapes:
        g = O.stripe_gather_index(reso, H_sp, W_sp).astype(np.int64)
        n = np.empty(L, np.int64)
        n[g.reshape(-1)] = np.tile(np.arange(N), g.shape[0])
        n_of_l.append(torch.from_numpy(n))
    zw, zb = [torch.zeros(Cb, 9, device=DEV) for _ in idx], [torch.zeros(Cb, device=DEV) for _ in idx]
    masks = [torch.zeros(B * (L // N), heads[i], N, N, dtype=torch.float64) for i in range(nb)]
    first = {}
    for j in range((N + hd - 1) // hd):
        qkv = torch.zeros(B, L, 3 * C)
        for i in range(nb):
            onehot = (n_of_l[i][:, None] == j * hd + torch.arange(hd)[None, :]).float()          # (L, hd)
            qkv[:, :, 2 * C + i * Cb:2 * C + (i + 1) * Cb] = onehot.repeat(1, heads[i])
        y, _, _ = attn.fwd(case, 0, qkv.to(DEV), zw, zb, drop=(p, seed))
        if j == 0:
            first["y"], first["qkv"] = y.clone(), qkv.to(DEV)
        y = y.double().cpu() * N
        for i, (H_sp, W_sp) in enumerate(shapes):
            m = O.img2windows(y[..., i * Cb:(i + 1) * Cb], reso, H_sp, W_sp).reshape(-1, N, heads[i], hd).permute(0, 2, 1, 3)
            keys = min(hd, N - j * hd)
            masks[i][..., j * hd:j * hd + keys] = m[..., :keys]
    y_other, _, _ = attn.fwd(case, 0, first["qkv"], zw, zb, drop=(p, seed + 1))
    assert not bool((y_other == first["y"]).all()), "another seed drew the same mask"
    return masks


@gpu
@pytest.mark.parametrize("case", DROP_ROWS, ids=cid)
def test_attention_dropout_vs_float64_with_the_kernels_mask(attn, case):
    """(e) p = 0.25: the mask is read off the forward kernel, checked to be a mask, and given to attn_ref; y, y0, lse (undropped),
    dq, dk, dv and the LePE gradients must then agree at RTOL, which also pins that the backward regenerates the forward's
    mask at padded sizes."""
    p, seed = 0.25, 20240607
    masks = extract_mask(attn, case, p, seed)
    keep = 1.0 / (1.0 - p)
    kept = total = 0
    for i, m in enumerate(masks):
        assert float(torch.minimum(m.abs(), (m - keep).abs()).max()) <= 1e-6, "a factor is neither 0 nor 1 / (1 - p)"
        masks[i] = torch.where(m > 0.5 * keep, float(np.float32(1.0) / np.float32(1.0 - p)), 0.0).double()
        kept, total = kept + int((m > 0.5 * keep).sum()), total + m.numel()
    assert abs(kept / total - (1 - p)) <= 5 * math.sqrt(p * (1 - p) / total), (kept, total)
    inputs = attn_inputs(case)
    ref = reference(case, *inputs, mask=masks)
    qkv, lw, lb, dy = attn.dev(*inputs)
    y, y0, lse = attn.fwd(case, 0, qkv, lw, lb, drop=(p, seed))
    grads = attn.bwd(case, 0, qkv, lw, lb, lse, y0, dy, drop=(p, seed))
    assert_all_within(compare_all("attnshape.drop." + cid(case), case, y, y0, lse, grads, ref), RTOL)


@gpu
def test_attention_refusals_touch_nothing(attn):
    """(f) host-side refusals: a window of 289 tokens, head dims 12 and 40, a stripe width that does not divide the map, a
    workspace one byte short."""
    for case in [(1, 17, 17, (-1,), 8, (1,)), (1, 4, 4, (-1,), 12, (1,)), (1, 4, 4, (-1,), 40, (1,)), (2, 20, 8, (1,), 48, (2,))]:
        qkv, lw, lb, _ = attn.dev(*attn_inputs(case))
        o = attn.outputs_fwd(case, 0)
        with pytest.raises(attn.Error):
            attn.call_fwd(case, 0, qkv, lw, lb, o)
        settle("refused attn_fwd " + cid(case), o, untouched=True)
    case = (2, 9, 9, (-1,), 24, (3,))
    qkv, lw, lb, dy = attn.dev(*attn_inputs(case))
    y, y0, lse = attn.fwd(case, 0, qkv, lw, lb)
    o, nbytes = attn.outputs_bwd(case, 0)
    with pytest.raises(attn.Error):
        attn.call_bwd(case, 0, qkv, lw, lb, lse, y0, dy, o, nbytes - 1)
    settle("refused attn_bwd", o, untouched=True)
    attn.call_bwd(case, 0, qkv, lw, lb, lse, y0, dy, o, nbytes)              # the same buffers, the full size: accepted
    settle("attn_bwd", o)
