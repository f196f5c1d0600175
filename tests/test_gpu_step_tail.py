"""The kernels that close a training step, away from the model's shapes: the loss (cswin_loss_sums / _finalize / _bwd), the
optimiser side (cswin_sgd_flat, cswin_multi_copy, cswin_pack_bf16_scaled, cswin_unpack_bf16), cswin_dropout, the layout adapters
(cswin_nchw_to_tokens, cswin_tokens_to_nchw), the window permutes (cswin_img2windows, cswin_windows2img) and the head
composition (cswin_head_compose / _bwd) -- at every instantiation, on both sides of every alignment branch and past every grid
clamp.

References are float64 on the CPU (autograd for gradients) or exact integer arithmetic where the operation is exact.  Gradients
and matrix products use test_gpu_parity's measure max|got - ref| / rms(ref) <= RTOL.  The scalar sums and losses get a bound
per case that loss_ref derives in float64 from the magnitudes actually summed (see loss_ref); the host tests show that this
bound sees the bugs the cases are there for.  Every output is a view into a NaN-filled buffer whose guard words must survive,
workspaces are exactly as large as the library says, every measured error goes to the error log under a tag naming the case,
and the entry points are called through cswin_unet_amd._lib: only a direct call passes n % 4 != 0, a pointer 4 bytes off a
16-byte boundary or an exact workspace.

The tests at the top need no GPU."""
import functools
import itertools
import math

import numpy as np
import pytest
import torch

from oracle.determ import det_labels, det_normal

from test_gpu_parity import LOG, RTOL                    # the fp32 bound and the error log, neither of them new
from test_gpu_shapes import D, measure                   # float64 leaf; max|got - ref| / rms(ref) in float64, printed and logged
from test_gpu_attn_shapes import GUARD, Guarded, settle  # NaN guard bands round an output; their check after a launch

gpu = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24                                           # unit roundoff of fp32
ERR_SHAPE, ERR_ALIGN, ERR_WORKSPACE, ERR_UNSUPPORTED = -1, -2, -3, -5       # include/cswin_hip.h
SMOOTH = 1e-5


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------
# launch rules (a transcription of the host code: it MUST FOLLOW csrc/loss_pixel.h, loss.hip, sgd.hip, layout.hip and the end of attn.hip)
# ------------------------------------------------------------------------------------------------
NC_SWITCH = (2, 3, 4, 5, 6, 7, 8, 9, 14, 16)
SUMS_CLAMP, BWD_CLAMP = 512, 2048                        # workgroups of 256 threads, one pixel per thread and trip
FLAT_CLAMP = 4096                                        # sgd_flat / pack / unpack (16-B chunks), nchw_to_tokens and the window permutes (elements)
DROPOUT_CLAMP = 8192                                     # 16-B chunks
TOK2NCHW_CLAMP = 8192                                    # 64-pixel tiles
HEAD_LDS_FLOATS = 12 * 1024


def loss_blocks(total):
    return max(1, min(SUMS_CLAMP, cdiv(total, 256)))


def trips(total, blocks):
    """(fewest, most) trips of a thread through a grid-stride loop over `total` items."""
    return total // (blocks * 256), cdiv(total, blocks * 256)


def head_staging(ncls, E, C):
    """(forward operands staged in LDS, backward st, backward st2) of cswin_head_compose[_bwd]."""
    fwd = ncls * E + E * C + E <= HEAD_LDS_FLOATS
    st = ncls * E + E * C + E + ncls * C + ncls <= HEAD_LDS_FLOATS
    st2 = st and ncls * E + E * (C + 1) + E + ncls * C + ncls <= HEAD_LDS_FLOATS
    return fwd, st, st2


# ------------------------------------------------------------------------------------------------
# case tables
# ------------------------------------------------------------------------------------------------
# loss: (tag, B, (H, W), ncls, probabilities mode, input) and what the row is there for.  HW = 7 * 13 is odd, not square, and with
# B = 3 the batch stride ncls * HW differs from HW.
LOSS_NCLS = [(f"nc{n}.{'probs' if pr else 'logits'}", 3, (7, 13), n, pr, "normal") for n in NC_SWITCH for pr in (False, True)]  # every NC x PROBS
LOSS_PIXELS = [
    ("px1", 1, (1, 1), 9, False, "normal"),              # a single pixel: 255 idle threads, 1 - NV idle reducers
    ("px255", 3, (5, 17), 9, False, "normal"),           # one short of a workgroup
    ("px257", 1, (1, 257), 9, False, "normal"),          # one past a workgroup: a second workgroup with one live thread
    ("px133563", 3, (211, 211), 16, False, "normal"),    # just past 512 * 256: sums threads take two trips or one; widest NV
    ("px526338", 2, (513, 513), 2, False, "normal"),     # just past 2048 * 256: the same for the backward (sums: five trips or four)
]
LOSS_WIDE = [
    ("wide40", 3, (7, 13), 9, False, "wide"),            # N(0, 40^2): spreads far past 87, where exp(v - max) underflows
    ("offset1e4", 3, (7, 13), 9, False, "offset"),       # a common offset of 1e4: only differences may matter
    ("equalrow", 3, (7, 13), 9, False, "equal"),         # rows of all-equal logits: -log p = log ncls exactly
]
LOSS_CASES = LOSS_NCLS + LOSS_PIXELS + LOSS_WIDE
LOSS_REFUSED_NCLS = (1, 10, 17)
OOR_LABELS = (-1, "ncls", 255, 2 ** 32 + 1)              # 2^32 + 1: class 1 to a kernel that truncates before it checks

# cswin_sgd_flat: n and what it reaches
SGD_SIZES = [
    (1, "tail only, no 16-B chunk"), (3, "tail only"), (4, "one chunk, no tail"), (5, "one chunk and a tail of 1"),
    (1023, "255 chunks (one short of a workgroup) and a tail of 3"), (1027, "256 chunks (a full workgroup) and a tail of 3"),
    (FLAT_CLAMP * 256 * 4 + 7, "one chunk past the 4096-workgroup clamp (a second trip for one thread) and a tail of 3"),
]
SGD_ARGS = list(itertools.product((0.0, 0.9), (0.0, 1e-4), (1.0, 0.125), (False, True)))    # momentum, weight decay, grad_scale, shadow
SGD_LRS = (0.05, 0.02, 0.007)

# cswin_multi_copy: chunk lengths (n < 4; vector body only; body and tail; the full 16384-float chunk and one short of it) x
# byte offsets of (source, destination) from a 16-byte boundary: only (0, 0) takes the 16-B path
COPY_SIZES = (1, 3, 4, 5, 16383, 16384)
COPY_ALIGN = ((0, 0), (4, 0), (0, 4), (4, 4))
GATHER_PARAMS = (1, 7, 9, 16385)                         # elements: pad words in every slot; 16385 = a full chunk and a chunk of 1

# bf16 wire: exponent x kept mantissa (even / odd last kept bit, all ones: the carry into the exponent) x discarded half
WIRE_EXP = (0, 1, 126, 127, 128, 254)                    # 0: denormal
WIRE_KEPT = (0x2A, 0x2B, 0x7F)
WIRE_LOW = (0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF)     # exact, just above, just below a tie, tie, just above a tie, just below the next
WIRE_SPECIAL = (0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0x7F800001, 0xFFC12345, 0x7F7FFFFF)
WIRE_SCALES = (1.0, 0.5, 1.0 / 3.0)

# cswin_dropout: (tag, n, p, elems_per_sample, residual, row scale, epoch)
DROP_BIG = DROPOUT_CLAMP * 256 * 4 + 4                   # one chunk past the 8192-workgroup clamp
DROP_CASES = [
    ("p0", 4096 + 4, 0.0, 4, False, False, 0),           # thr = 0: keeps everything
    ("p1e-6", 4096 + 4, 1e-6, 4, False, False, 0),       # thr = int(0.065536) = 0: keeps everything
    ("p0.3.n4", 4, 0.3, 4, True, False, 0),              # one 16-B chunk
    ("p0.3.rows", 4096 + 4, 0.3, 4, True, True, 0),      # elems_per_sample = 4: a row scale per chunk, one of them zero
    ("p0.3.epoch", 4096 + 4, 0.3, 1028, True, True, 12345),     # a device epoch added to the seed; a sample boundary inside a workgroup
    ("p0.999", 4096 + 4, 0.999, 4, False, False, 0),     # thr = 65470, scale 1000
    ("p0.3.big", DROP_BIG, 0.3, DROP_BIG // 3, True, True, 0),  # past the grid clamp: 33.6 MB a buffer, the largest of this file
]
DROP_SEED = 0x9E3779B97F4A7C15 ^ 0x1234567

# layout adapters
TOK_HW = ((1, 1), (7, 9), (8, 8), (5, 13), (7, 13))      # HW = 1, 63, 64, 65, 91: below, at and past the 64-pixel tile; non-square
TOK_C = (1, 3, 9, 16, 17, 33)                            # below, at and past the 16-channel tile
TOK_B = (1, 3)
TOK_BIG = (3, 224, 896, 2, 4)                            # B, H, W, C, Cpad: 2 408 448 elements > 4096 * 256 and 9408 tiles > 8192


def tok_cpads(C):
    return sorted({C, cdiv(C, 4) * 4, cdiv(C, 16) * 16})


# window permutes: (B, C, H, W, H_sp, W_sp)
WINDOW_CASES = [
    (2, 5, 6, 15, 3, 5),                                 # H != W, H_sp != W_sp, odd C
    (1, 3, 8, 4, 8, 1),                                  # a vertical stripe
    (2, 9, 256, 240, 16, 240),                           # 1 105 920 elements > 4096 * 256: a second trip
]
WINDOW_REFUSED = [(2, 5, 6, 15, 4, 5), (2, 5, 6, 15, 3, 4)]

# head composition: (ncls, E, C, Cpad)
HEAD_CASES = [
    (9, 128, 128, 16),                                   # 17 664 floats of operands: read in place, forward and backward
    (2, 108, 108, 16),                                   # backward: st true, st2 false (W_out's padded image leaves no room for the rest)
    (3, 17, 33, 16),                                     # everything staged; odd sizes
    (16, 64, 32, 16),                                    # Cpad == ncls: no zero rows
]


# ------------------------------------------------------------------------------------------------
# float64 reference of the loss (utils.py's CE + soft-Dice from its definition) and the bound of its sums
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def loss_inputs(tag):
    """(x (B, ncls, HW) float32, labels (B, HW) int64) of a row of LOSS_CASES; computed once, never written."""
    _, B, (H, W), ncls, probs, kind = next(c for c in LOSS_CASES if c[0] == tag)
    x = det_normal(f"tail.loss.{tag}.x", (B, ncls, H * W), 40.0 if kind == "wide" else 1.0)
    if kind == "offset":
        x = (x + np.float32(1e4)).astype(np.float32)
    if kind == "equal":
        x = x.copy()
        x[:, :, ::3] = x[:, :1, ::3]
    if probs:
        x = torch.softmax(torch.from_numpy(x).double(), 1).float().numpy()
    lab = det_labels(f"tail.loss.{tag}.lab", (B, H, W), ncls).reshape(B, H * W)
    return x, lab


def loss_ref(x, lab, probs=False, _wrong=None):
    """(sums, bound): the 1 + 3*ncls sums in the documented order [sum -log p[label], intersect_c, y_sum_c, z_sum_c] in numpy
    float64 -- softmax, one-hot by ==, three sums per class -- and for each a bound on what the fp32 kernel may differ by.

    The bound of a sum of terms t_i is 2^-24 * (sum_i a_i |t_i| + depth * sum_i |t_i|):
      a_i, the roundings a term carries before it is added.  exp(d), d = v - max <= 0, is v_exp_f32 (1 ulp) of fl(fl(d) * log2 e):
      the subtraction, the constant and the product each move the argument by up to |d| 2^-24 relative to e^d, so
      eps_c = 2 + 2.5 |d_c|.  The row sum inherits sum_j p_j eps_j and adds ncls - 1 roundings; the reciprocal and the product
      by it add 3; so a probability is off by r_c = eps_c + sum_j p_j eps_j + ncls + 2 units.  intersect carries r_label, a
      z term 2 r_c + 1, a y term nothing (ones: the sum is exact below 2^24).  The CE term (max - v_label) + log(sum) carries
      half a unit of the difference, the row sum's relative error as an ABSOLUTE error of the logarithm, 2.5 units of
      |log sum| (v_log_f32, the product by ln 2 and its constant), one unit of 1 for the logarithm's argument and half a unit
      of itself.  In probabilities mode the inputs are exact: r_c = 0, a z term carries 1, the CE term 2.5 |log p| + 1.
      depth, the additions a term passes through: the thread's trips, 6 levels of the wave sum, 3 additions of the 4 waves,
      then the slab reduction's ceil(blocks / 16) rows per row group and its 16 row groups.
    An out-of-range label belongs to no class and makes sums[0] NaN.

    _wrong (the sensitivity test alone): "drop_last" (the last pixel), "drop_class" (the last class's term missing from the row
    sum), "batch_stride" (HW for ncls * HW), "drop_trip2" (pixels past the first grid-stride trip), "swap_yz", "ce_clamp"
    (-log max(p, 1e-37) with p from an fp32 exp that underflows)."""
    B, ncls, HW = x.shape
    v = x.astype(np.float64)
    if _wrong == "batch_stride":
        b, c, p = np.meshgrid(np.arange(B), np.arange(ncls), np.arange(HW), indexing="ij")
        v = v.reshape(-1)[b * HW + c * HW + p]
    lab = np.asarray(lab, np.int64)
    valid = (lab >= 0) & (lab < ncls)
    oh = (lab[:, None, :] == np.arange(ncls)[None, :, None]).astype(np.float64)
    w = np.ones((B, HW))
    if _wrong == "drop_last":
        w[-1, -1] = 0.0
    if _wrong == "drop_trip2":
        w.reshape(-1)[loss_blocks(B * HW) * 256:] = 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        if probs:
            p, r = v, np.zeros_like(v)
            nll = -np.log((p * oh).sum(1))
            a_nll = 2.5 * np.abs(nll) + 1.0
            a_z = np.ones_like(v)
        else:
            mx = v.max(1, keepdims=True)
            d = v - mx
            e = np.exp(d)
            s = (e[:, :-1] if _wrong == "drop_class" else e).sum(1, keepdims=True)
            p = e / s
            eps = 2.0 + 2.5 * np.abs(d)
            rsum = (p * eps).sum(1) + (ncls - 1)
            r = eps + rsum[:, None] + 3.0
            dl = -(d * oh).sum(1)                                   # max - v[label] >= 0
            nll = dl + np.log(s[:, 0])
            a_nll = 0.5 * dl + rsum + 2.5 * np.abs(np.log(s[:, 0])) + 1.0 + 0.5 * np.abs(nll)
            a_z = 2.0 * r + 1.0
            if _wrong == "ce_clamp":
                e32 = np.where(d < math.log(2.0 ** -126), 0.0, e)  # what an fp32 exponential leaves of it
                nll = -np.log(np.maximum((e32 * oh).sum(1) / s[:, 0], 1e-37))
        nll = np.where(valid, nll, 0.0)
    t0, tI, tY, tZ = nll * w, p * oh * w[:, None], oh * w[:, None], p * p * w[:, None]
    sums = np.concatenate([[t0.sum()], tI.sum((0, 2)), tY.sum((0, 2)), tZ.sum((0, 2))])
    if _wrong == "swap_yz":
        sums = np.concatenate([sums[:1 + ncls], sums[1 + 2 * ncls:], sums[1 + ncls:1 + 2 * ncls]])
    blocks = loss_blocks(B * HW)
    depth = trips(B * HW, blocks)[1] + 6 + 3 + cdiv(blocks, 16) + 16
    assert B * HW < 2 ** 24
    bound = U * np.concatenate([[(np.where(valid, a_nll, 0.0) * w).sum() + depth * np.abs(t0).sum()],
                                (r * tI).sum((0, 2)) + depth * tI.sum((0, 2)), np.zeros(ncls), (a_z * tZ).sum((0, 2)) + depth * tZ.sum((0, 2))])
    if not (valid | (w == 0)).all():
        sums[0] = np.nan
    return sums, bound


def final_ref(sums, n_pixels, w_ce, w_dice, cw=None, bsums=None):
    """cswin_loss_finalize in float64: ((loss, ce, dice), their bounds, coef).  The bounds carry the sums' bounds bsums (none:
    exact sums) through ce = S0 / n and dice = mean_c w_c (1 - (2 I + s) / (Z + Y + s)) and add the kernel's own roundings:
    2 on ce, 4 on each ratio, one per class on 1 - ratio and on the running sum, 2 on the final combination."""
    sums = np.asarray(sums, np.float64)
    ncls = (len(sums) - 1) // 3
    bs = np.zeros_like(sums) if bsums is None else np.asarray(bsums, np.float64)
    cw = np.ones(ncls) if cw is None else np.asarray(cw, np.float64)
    I, Y, Z = sums[1:1 + ncls], sums[1 + ncls:1 + 2 * ncls], sums[1 + 2 * ncls:]
    bI, bY, bZ = bs[1:1 + ncls], bs[1 + ncls:1 + 2 * ncls], bs[1 + 2 * ncls:]
    ce = sums[0] / n_pixels
    Dn = Z + Y + SMOOTH
    R = (2 * I + SMOOTH) / Dn
    dice = float((cw * (1 - R)).sum() / ncls)
    loss = (w_ce * ce if w_ce != 0 else 0.0) + w_dice * dice
    b_ce = bs[0] / n_pixels + 2 * U * abs(ce)
    bR = 2 * bI / Dn + R * (bY + bZ) / Dn + 4 * U * R
    b_dice = float((np.abs(cw) * (bR + U * (1 + R))).sum() + ncls * U * np.abs(cw * (1 - R)).sum()) / ncls + U * abs(dice)
    b_loss = (abs(w_ce) * b_ce + 2 * U * abs(w_ce * ce) if w_ce != 0 else 0.0) + abs(w_dice) * b_dice + 2 * U * abs(w_dice * dice)
    coef = np.concatenate([cw * -2 / Dn, cw * 2 * (2 * I + SMOOTH) / (Dn * Dn)])
    return np.array([loss, ce, dice]), np.array([b_loss, b_ce, b_dice]), coef


def loss_graph(x, lab, probs=False):
    """(sum -log p[label], I, Y, Z) as float64 tensors on the autograd graph of x (B, ncls, HW); a pixel whose label is out of
    range matches no class."""
    ncls = x.shape[1]
    lab = torch.as_tensor(np.asarray(lab, np.int64))
    p = x if probs else torch.softmax(x, 1)
    logp = torch.log(x) if probs else torch.log_softmax(x, 1)
    oh = (lab[:, None, :] == torch.arange(ncls)[None, :, None])
    nll = -torch.where(oh, logp, torch.zeros_like(logp)).sum()
    ohd = oh.double()
    return nll, (p * ohd).sum((0, 2)), ohd.sum((0, 2)), (p * p).sum((0, 2))


def dice_terms(I, Y, Z, cw=None):
    t = 1 - (2 * I + SMOOTH) / (Z + Y + SMOOTH)
    return (t if cw is None else t * torch.as_tensor(np.asarray(cw, np.float64))).sum()


def grad_ref(x, lab, probs, ce_scale, dice_scale, g=1.0, cw=None):
    """d/dx of g * (ce_scale * sum -log p[label] + dice_scale * sum_c w_c dice_c), by float64 autograd."""
    xl = D(x)
    nll, I, Y, Z = loss_graph(xl, lab, probs)
    (g * ((0.0 if probs else ce_scale) * nll + dice_scale * dice_terms(I, Y, Z, cw))).backward()
    return xl.grad


# ------------------------------------------------------------------------------------------------
# integer references: bf16 rounding, the dropout generator
# ------------------------------------------------------------------------------------------------
def rne_bf16(bits):
    """(bf16 patterns, is-NaN mask) of fp32 patterns (uint32), round to nearest even in integer arithmetic."""
    b = np.asarray(bits, np.uint32).astype(np.uint64)
    r = ((b + np.uint64(0x7FFF) + ((b >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)) & np.uint64(0xFFFF)
    return r.astype(np.uint16), (b & np.uint64(0x7FFFFFFF)) > np.uint64(0x7F800000)


def wire_table():
    rows = [s << 31 | e << 23 | k << 16 | lo for s in (0, 1) for e in WIRE_EXP for k in WIRE_KEPT for lo in WIRE_LOW]
    return np.array(rows + [v for v in WIRE_SPECIAL if v not in rows], np.uint32)      # the largest finite fp32 is a row already


def scaled_bits(bits, scale):
    """Patterns of fl32(value * scale): one IEEE multiply in numpy float32, denormals kept."""
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        return (np.asarray(bits, np.uint32).view(np.float32) * np.float32(scale)).view(np.uint32)


_GOLD, _M1, _M2 = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)


def mix64(z):
    """splitmix64's step on a uint64 array: add the golden-ratio increment, then its finaliser (arithmetic mod 2^64)."""
    z = np.asarray(z, np.uint64) + _GOLD
    z = (z ^ (z >> np.uint64(30))) * _M1
    z = (z ^ (z >> np.uint64(27))) * _M2
    return z ^ (z >> np.uint64(31))


def keep_mask(seed, epoch, n, p):
    """Elements kept by cswin_dropout: r = mix64(mix64(seed + epoch) ^ (i // 4)); element i takes the 16-bit field i % 4 of r,
    lowest first, and is kept iff the field >= uint32(float32(p) * 65536)."""
    base = mix64(np.array([(seed + epoch) % 2 ** 64], np.uint64))
    r = mix64(base ^ np.arange(n // 4, dtype=np.uint64))
    fields = (r[:, None] >> (np.uint64(16) * np.arange(4, dtype=np.uint64))[None, :]) & np.uint64(0xFFFF)
    return fields.reshape(-1) >= np.uint64(int(np.float32(p) * np.float32(65536.0)))


# ------------------------------------------------------------------------------------------------
# host-only tests: the references against independent formulations, what the bounds can see, the tables against the rules
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["nc3.logits", "nc9.logits", "nc5.probs", "wide40", "px255"])
def test_loss_ref_agrees_with_torch_and_explicit_loops(tag):
    """loss_ref (numpy), loss_graph (autograd) and nn.CrossEntropyLoss + a per-class Dice loop give the same numbers."""
    x, lab = loss_inputs(tag)
    probs = next(c for c in LOSS_CASES if c[0] == tag)[4]
    B, ncls, HW = x.shape
    sums, bound = loss_ref(x, lab, probs)
    assert sums.shape == bound.shape == (1 + 3 * ncls,) and (bound >= 0).all() and np.isfinite(bound).all()
    xt, lt = torch.from_numpy(x).double(), torch.from_numpy(lab)
    got = torch.cat([t.reshape(-1) for t in loss_graph(xt, lab, probs)]).numpy()
    assert np.abs(got - sums).max() <= 1e-12 * np.abs(sums).max()
    pr = xt if probs else torch.softmax(xt, 1)
    for c in range(ncls):
        t = (lt == c).double()
        want = [float((pr[:, c] * t).sum()), float((t * t).sum()), float((pr[:, c] * pr[:, c]).sum())]
        assert np.allclose([sums[1 + c], sums[1 + ncls + c], sums[1 + 2 * ncls + c]], want, rtol=1e-12, atol=0)
    if not probs:
        ce = float(torch.nn.CrossEntropyLoss()(xt, lt))
        out, _, _ = final_ref(sums, B * HW, 0.4, 0.6)
        assert abs(out[1] - ce) <= 1e-12 * abs(ce)
        dice = sum(1 - (2 * sums[1 + c] + SMOOTH) / (sums[1 + 2 * ncls + c] + sums[1 + ncls + c] + SMOOTH) for c in range(ncls)) / ncls
        assert abs(out[0] - (0.4 * ce + 0.6 * dice)) <= 1e-12
        # the closed-form gradient coefficients against autograd of the Dice term
        xl = D(x)
        _, I, Y, Z = loss_graph(xl, lab)
        dice_terms(I, Y, Z).backward()
        _, _, coef = final_ref(sums, B * HW, 0.4, 0.6)
        p = torch.softmax(xt, 1)
        oh = (lt[:, None, :] == torch.arange(ncls)[None, :, None]).double()
        G = torch.from_numpy(coef[:ncls])[None, :, None] * oh + torch.from_numpy(coef[ncls:])[None, :, None] * p
        closed = p * (G - (p * G).sum(1, keepdim=True))
        assert float((closed - xl.grad).abs().max()) <= 1e-12


def test_cross_entropy_of_a_far_label_is_the_logit_gap():
    """nn.CrossEntropyLoss gives 100 for logits [100, 0] and label 1; so does the reference, and the clamp form does not."""
    x, lab = np.array([[[100.0], [0.0]]], np.float32), np.array([[1]], np.int64)
    assert abs(loss_ref(x, lab)[0][0] - 100.0) < 1e-12
    assert abs(float(torch.nn.CrossEntropyLoss()(torch.tensor([[100.0, 0.0]]).double(), torch.tensor([1]))) - 100.0) < 1e-12
    assert abs(loss_ref(x, lab, _wrong="ce_clamp")[0][0] - -math.log(1e-37)) < 1e-9


BUGS = [  # (planted bug, the rows meant to catch it, the sums that must see it: "ce", "I", "Y", "Z")
    ("drop_last", ("px1", "px255", "px257"), ("ce", "Y")),
    ("drop_class", ("nc2.logits", "nc9.logits", "nc16.logits"), ("ce", "I", "Z")),
    ("batch_stride", ("nc2.logits", "nc9.logits", "nc14.probs", "px255"), ("ce", "I", "Z")),
    ("drop_trip2", ("px133563", "px526338"), ("ce", "I", "Y", "Z")),
    ("swap_yz", ("nc2.logits", "nc9.logits", "nc16.probs", "px526338"), ("Y", "Z")),
    ("ce_clamp", ("wide40",), ("ce",)),
]


@pytest.mark.parametrize("bug,tags,seen_by", BUGS, ids=[b[0] for b in BUGS])
def test_bound_sees_the_bugs_these_shapes_are_for(bug, tags, seen_by):
    """Each planted bug moves the sums named for it by at least four times their bound, at each row meant to catch it (for the
    per-class sums: the class that moves most; for swap_yz: every class).  The loss's own bound sees the CE clamp as well."""
    for tag in tags:
        x, lab = loss_inputs(tag)
        case = next(c for c in LOSS_CASES if c[0] == tag)
        ncls, probs = case[3], case[4]
        ref, bound = loss_ref(x, lab, probs)
        bad, _ = loss_ref(x, lab, probs, _wrong=bug)
        part = dict(ce=slice(0, 1), I=slice(1, 1 + ncls), Y=slice(1 + ncls, 1 + 2 * ncls), Z=slice(1 + 2 * ncls, 1 + 3 * ncls))
        for name in seen_by:
            if name == "ce" and probs:
                continue                                            # the CE sum of probabilities is not what these rows are for
            moved, b = np.abs(bad - ref)[part[name]], bound[part[name]]
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = np.where(b > 0, moved / b, np.where(moved > 0, np.inf, 0.0))
            seen = ratio.min() if bug == "swap_yz" else ratio.max()
            print(f"{tag} {bug} {name}: moved {moved.max():.3e}, bound {b.max():.3e}, ratio {seen:.3g}")
            assert seen >= 4.0, (tag, bug, name, seen)
        if bug == "ce_clamp":
            n = x.shape[0] * x.shape[2]
            out, bout, _ = final_ref(ref, n, 0.4, 0.6, bsums=bound)
            out_bad, _, _ = final_ref(bad, n, 0.4, 0.6, bsums=bound)
            assert abs(out_bad[0] - out[0]) >= 4 * bout[0] and abs(out_bad[1] - out[1]) >= 4 * bout[1]


def test_sums_bound_is_a_few_dozen_roundings_of_what_was_summed():
    """The bound is neither zero nor slack: between 10 and 200 units of 2^-24 sum|terms| at every row (y sums: exact)."""
    for tag, B, (H, W), ncls, probs, kind in LOSS_CASES:
        if B * H * W > 70000:
            continue                                                # the large rows' bounds are exercised by the test above
        x, lab = loss_inputs(tag)
        sums, bound = loss_ref(x, lab, probs)
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = bound / (U * np.abs(sums))
        live = np.r_[0:1 + ncls, 1 + 2 * ncls:1 + 3 * ncls]
        live = [k for k in live if sums[k] > 0 and not (probs and k == 0)]
        assert (bound[1 + ncls:1 + 2 * ncls] == 0).all()
        assert all(10 <= rel[k] <= 200 for k in live), (tag, rel[live])


def test_rne_reference_against_torch_cpu_cast():
    """The integer RNE agrees with torch's CPU bfloat16 cast on every finite row of the wire table, scaled or not, and on
    100 000 random patterns; it does what the table is there for at the rows one can work out by hand."""
    rng = np.random.RandomState(7)
    pats = np.concatenate([wire_table()] + [scaled_bits(wire_table(), s) for s in WIRE_SCALES[1:]] + [rng.randint(0, 2 ** 32, 100000, dtype=np.uint64).astype(np.uint32)])
    want, nan = rne_bf16(pats)
    got = torch.from_numpy(pats.view(np.float32).copy()).bfloat16().view(torch.int16).numpy().view(np.uint16)
    assert (got[~nan] == want[~nan]).all()
    hand = {0x3F808000: 0x3F80, 0x3F818000: 0x3F82, 0x3F808001: 0x3F81, 0x3F807FFF: 0x3F80, 0x7F7FFFFF: 0x7F80, 0xFF7F8000: 0xFF80,
            0x80000000: 0x8000, 0x00008000: 0x0000, 0x00018000: 0x0002, 0x7F800000: 0x7F80}
    for k, v in hand.items():
        assert int(rne_bf16(np.array([k], np.uint32))[0][0]) == v, hex(k)
    assert rne_bf16(np.array([0x7F800001, 0x7FC00000, 0xFFC12345], np.uint32))[1].all()
    t = wire_table()
    assert len(t) == 2 * len(WIRE_EXP) * len(WIRE_KEPT) * len(WIRE_LOW) + len(WIRE_SPECIAL) - 1 == len(set(t.tolist())) and set(WIRE_SPECIAL) <= set(t.tolist())


def test_mix64_restatement_against_hand_computed_vectors():
    """splitmix64 from state 0 yields E220A8397B1DCDAF, 6E789E6AA1B965F4, 06C45D188009454F (its published first outputs): the
    step applied to 0, to the increment and to twice the increment.  An independent big-integer evaluation agrees elsewhere."""
    gold = 0x9E3779B97F4A7C15
    got = mix64(np.array([0, gold, 2 * gold % 2 ** 64], np.uint64))
    assert [int(v) for v in got] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]

    def by_hand(z):
        m = 2 ** 64
        z = (z + gold) % m
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) % m
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) % m
        return z ^ (z >> 31)
    zs = [1, 2 ** 63, 2 ** 64 - 1, DROP_SEED, 0xDEADBEEFCAFEF00D]
    assert [int(v) for v in mix64(np.array(zs, np.uint64))] == [by_hand(z) for z in zs]
    # the mask: fields in element order, the threshold from float32 arithmetic, a short run the prefix of a long one
    seed, epoch = DROP_SEED, 12345
    r = by_hand(by_hand((seed + epoch) % 2 ** 64) ^ 5)
    thr = int(np.float32(0.3) * np.float32(65536.0))
    assert thr == 19660 and int(np.float32(1e-6) * np.float32(65536.0)) == 0 and int(np.float32(0.999) * np.float32(65536.0)) == 65470
    assert keep_mask(seed, epoch, 64, 0.3)[20:24].tolist() == [((r >> 16 * e) & 0xFFFF) >= thr for e in range(4)]
    assert (keep_mask(seed, 0, 64, 0.3) == keep_mask(seed, 0, 4096, 0.3)[:64]).all()
    assert keep_mask(seed, 0, 4096, 0.0).all() and keep_mask(seed, 0, 4096, 1e-6).all()
    assert abs(keep_mask(seed, 0, 1 << 16, 0.3).mean() - (1 - thr / 65536)) < 0.01


def test_case_tables_reach_every_branch_instantiation_and_clamp():
    # loss: every NC_SWITCH value in both modes; pixel counts round a workgroup; mixed trip counts past both clamps
    assert {(c[3], c[4]) for c in LOSS_NCLS} == {(n, pr) for n in NC_SWITCH for pr in (False, True)}
    assert all(B == 3 and H * W == 91 and H != W for _, B, (H, W), _, _, _ in LOSS_NCLS)
    totals = {tag: B * H * W for tag, B, (H, W), _, _, _ in LOSS_PIXELS}
    assert sorted(totals.values()) == [1, 255, 257, 133563, 526338]
    assert trips(133563, loss_blocks(133563)) == (1, 2) and loss_blocks(133563) == SUMS_CLAMP
    assert trips(526338, 4 * loss_blocks(526338)) == (1, 2) and 4 * loss_blocks(526338) == BWD_CLAMP
    assert trips(133563, 4 * loss_blocks(133563)) == (0, 1)         # before that the backward gives each pixel a thread
    assert {c[3] for c in LOSS_PIXELS if c[0] in ("px133563", "px526338")} == {16, 2}
    assert not set(LOSS_REFUSED_NCLS) & set(NC_SWITCH)
    from cswin_unet_amd._lib import lib
    for tag, B, (H, W), ncls, _, _ in LOSS_CASES:
        assert lib().cswin_loss_workspace(B, ncls, H * W) == loss_blocks(B * H * W) * (1 + 3 * ncls) * 4, tag
    x, _ = loss_inputs("wide40")
    gap = x.max(1) - x.min(1)
    assert (gap > 87.4).mean() > 0.5 and gap.max() > 200            # most pixels have a class whose exp underflows
    x, _ = loss_inputs("equalrow")
    assert (x[:, :, ::3] == x[:, :1, ::3]).all() and loss_inputs("offset1e4")[0].min() > 9900
    # sgd_flat: only a tail, only chunks, both; a workgroup short by one chunk and a full one; the clamp together with the tail; both sides of the shadow branch
    ns = [n for n, _ in SGD_SIZES]
    assert ns == [1, 3, 4, 5, 1023, 1027, 4096 * 256 * 4 + 7]
    assert {n % 4 for n in ns} == {0, 1, 3} and {n // 4 == 0 for n in ns} == {True, False}
    grid = lambda n: max(1, min(FLAT_CLAMP, cdiv(n // 4, 256)))
    assert 1023 // 4 == 255 and 1027 // 4 == 256 and grid(1027) == 1 and grid(ns[-1]) == FLAT_CLAMP and trips(ns[-1] // 4, grid(ns[-1])) == (1, 2) and ns[-1] % 4 == 3
    assert len(SGD_ARGS) == 16 and {a[3] for a in SGD_ARGS} == {False, True}
    # multi_copy: n < 4, n % 4 == 0, a tail, the full chunk; the 16-B path and the three ways of missing it
    assert {n < 4 for n in COPY_SIZES} == {True, False} and {n % 4 for n in COPY_SIZES} == {0, 1, 3} and max(COPY_SIZES) == 16384
    assert {(s % 16 == 0, d % 16 == 0) for s, d in COPY_ALIGN} == {(True, True), (False, True), (True, False), (False, False)}
    assert all(n % 8 != 0 for n in GATHER_PARAMS) and any(n > 16384 for n in GATHER_PARAMS)
    # dropout: the clamp, p's that keep everything, a row scale per chunk, an epoch
    assert trips(DROP_BIG // 4, min(DROPOUT_CLAMP, cdiv(DROP_BIG // 4, 256))) == (1, 2) and DROP_BIG * 4 < 34 * 2 ** 20
    assert {c[2] for c in DROP_CASES} == {0.0, 1e-6, 0.3, 0.999} and any(c[1] == 4 for c in DROP_CASES)
    assert any(c[3] == 4 and c[5] for c in DROP_CASES) and any(c[6] for c in DROP_CASES) and all(c[1] % 4 == 0 and c[3] % 4 == 0 for c in DROP_CASES)
    # layout adapters: HW and C on both sides of their tiles, C == Cpad, both clamps
    assert sorted(h * w for h, w in TOK_HW) == [1, 63, 64, 65, 91] and any(h != w for h, w in TOK_HW)
    assert {c % 16 == 0 for c in TOK_C} == {True, False} and max(TOK_C) > 32
    assert all(C in tok_cpads(C) for C in TOK_C) and tok_cpads(17) == [17, 20, 32] and tok_cpads(16) == [16]
    B, H, W, C, Cpad = TOK_BIG
    assert B * H * W * Cpad > FLAT_CLAMP * 256 and B * cdiv(H * W, 64) > TOK2NCHW_CLAMP
    assert any(B * C * H * W > FLAT_CLAMP * 256 for B, C, H, W, _, _ in WINDOW_CASES)
    assert all(H != W and hs != ws and H % hs == 0 and W % ws == 0 for _, _, H, W, hs, ws in WINDOW_CASES)
    assert all(H % hs or W % ws for _, _, H, W, hs, ws in WINDOW_REFUSED)
    # head: read in place; st && !st2; all staged; Cpad == ncls
    assert [head_staging(n, E, C) for n, E, C, _ in HEAD_CASES] == [(False, False, False), (True, True, False), (True, True, True), (True, True, True)]
    assert any(cp == n for n, _, _, cp in HEAD_CASES) and any(cp > n for n, _, _, cp in HEAD_CASES)


# ------------------------------------------------------------------------------------------------
# the entry points, called directly with guarded buffers
# ------------------------------------------------------------------------------------------------
class GuardedAt(Guarded):
    """Guarded, with the view `off` elements past a 16-byte boundary."""

    def __init__(self, shape, dtype=torch.float32, off=0):
        self.n = math.prod(shape)
        self.lo = GUARD + off
        self.buf = torch.full((self.n + 2 * GUARD + 16,), float("nan"), dtype=dtype, device=DEV)
        self.t = self.buf[self.lo:self.lo + self.n].view(shape)
        assert self.t.data_ptr() % 16 == off * self.buf.element_size()

    def intact(self):
        return bool(torch.isnan(self.buf[:self.lo]).all()) and bool(torch.isnan(self.buf[self.lo + self.n:]).all())


_inputs = []       # the device inputs of the running test: a kernel is given raw addresses, which keep no tensor alive


@pytest.fixture(autouse=True)
def release_inputs():
    yield
    _inputs.clear()


def put(a, off=0):
    """Device copy of a numpy array / tensor, `off` elements past a 16-byte boundary; it lives until the test ends."""
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a.detach().cpu().contiguous()
    buf = torch.zeros(t.numel() + 16, dtype=t.dtype, device=DEV)
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == off * t.element_size()
    _inputs.append(v)
    return v


def bits32(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def bits16(t):
    return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


@pytest.fixture(scope="module")
def hip():
    from cswin_unet_amd import _lib

    class Hip:
        call, ptr, stream, lib = staticmethod(_lib.call), staticmethod(_lib.ptr), staticmethod(_lib.stream), staticmethod(_lib.lib)

        @staticmethod
        def refused(code, what, bufs, name, *args):
            got = getattr(_lib.lib(), name)(*args)
            assert got == code, f"{what}: {name} returned {got}, expected {code}"
            settle("refused " + what, bufs, untouched=True)
    return Hip


def close(got, ref, bound, what):
    """|got - ref| <= bound element by element; the error relative to the largest reference magnitude is logged under `what`."""
    got, ref, bound = np.asarray(got, np.float64).reshape(-1), np.asarray(ref, np.float64).reshape(-1), np.asarray(bound, np.float64).reshape(-1)
    measure(torch.from_numpy(got), torch.from_numpy(ref), what)
    over = np.abs(got - ref) - bound
    with np.errstate(divide="ignore", invalid="ignore"):
        k = int(np.argmax(np.where(bound > 0, np.abs(got - ref) / bound, np.where(over > 0, np.inf, 0.0))))
    print(f"{what}: worst entry {k}: got {got[k]!r} ref {ref[k]!r} |diff| {abs(got[k] - ref[k]):.3e} bound {bound[k]:.3e}")
    assert np.isfinite(got).all() and (over <= 0).all(), f"{what}: entry {k}: |{got[k]!r} - {ref[k]!r}| = {abs(got[k] - ref[k]):.3e} > {bound[k]:.3e}"


# ---- loss ---------------------------------------------------------------------------------------------------------------------
def run_loss(hip, x, lab, probs=False, w_ce=0.4, w_dice=0.6, cw=None, n_pixels=None, ce_scale=None, dice_scale=None, gout=None,
             sums_in=None, what="", nan_ok=False):
    """sums -> finalize -> bwd on guarded buffers; returns numpy sums, out3, coef and the dlogits tensor (CPU).  sums_in: finalize
    and bwd run on these sums instead of the local ones (an emulated all-reduce)."""
    B, ncls, HW = x.shape
    xd, ld = put(x), put(lab)
    nbytes = hip.lib().cswin_loss_workspace(B, ncls, HW)
    assert nbytes % 4 == 0
    o = dict(sums=Guarded((1 + 3 * ncls,)), workspace=Guarded((nbytes // 4,)), out3=Guarded((3,)), coef=Guarded((2 * ncls,)), dlogits=Guarded((B, ncls, HW)))
    hip.call("cswin_loss_sums", hip.ptr(xd), hip.ptr(ld), hip.ptr(o["sums"].t), hip.ptr(o["workspace"].t), nbytes, B, ncls, HW, int(probs), hip.stream())
    sums = o["sums"].t.cpu().numpy().copy()
    fin = o["sums"].t if sums_in is None else put(np.asarray(sums_in, np.float32))
    cwd = None if cw is None else put(np.asarray(cw, np.float32))
    hip.call("cswin_loss_finalize", hip.ptr(fin), hip.ptr(o["out3"].t), hip.ptr(o["coef"].t), float(B * HW if n_pixels is None else n_pixels), ncls,
             w_ce, w_dice, hip.ptr(cwd), hip.stream())
    gd = None if gout is None else put(np.array([gout], np.float32))
    hip.call("cswin_loss_bwd", hip.ptr(xd), hip.ptr(ld), hip.ptr(o["coef"].t), hip.ptr(gd), hip.ptr(o["dlogits"].t),
             w_ce / (B * HW) if ce_scale is None else ce_scale, w_dice / ncls if dice_scale is None else dice_scale, B, ncls, HW, int(probs), hip.stream())
    if nan_ok:                                                       # a poisoned CE sum: the guards hold, the NaN is the result
        torch.cuda.synchronize()
        assert all(g.intact() for g in o.values())
    else:
        settle(what, o)
    return sums, o["out3"].t.cpu().numpy().copy(), o["coef"].t.cpu().numpy().copy(), o["dlogits"].t.cpu()


@gpu
@pytest.mark.parametrize("case", LOSS_CASES, ids=[c[0] for c in LOSS_CASES])
def test_loss_every_sum_loss_and_gradient_vs_float64(hip, case):
    """Every entry of sums against float64 within its own bound, loss / ce / dice within the bounds that follow from them, the
    gradient by the suite's measure.  Probabilities mode runs without a CE term.

    Measured on an MI355X: while the CE term was -log max(p, 1e-37), wide40's CE sum came out as 13 818.49 where float64 has
    16 213.26 (bound 0.027; tail.loss.wide40.sums 7.8e-01).  Formed as (max - v[label]) + log(sum) every sum is inside its
    bound (tail.loss.wide40.sums 3.2e-07, .out3 1.1e-07, .dlogits 3.3e-07)."""
    tag, B, (H, W), ncls, probs, kind = case
    x, lab = loss_inputs(tag)
    w_ce, w_dice = (0.0, 1.0) if probs else (0.4, 0.6)
    sums, out3, coef, dl = run_loss(hip, x, lab, probs, w_ce, w_dice, what=f"tail.loss.{tag}")
    ref, bound = loss_ref(x, lab, probs)
    close(sums, ref, bound, f"tail.loss.{tag}.sums")
    want, bwant, cref = final_ref(ref, B * H * W, w_ce, w_dice, bsums=bound)
    close(out3, want, bwant, f"tail.loss.{tag}.out3")
    assert measure(dl, grad_ref(x, lab, probs, w_ce / (B * H * W), w_dice / ncls), f"tail.loss.{tag}.dlogits") <= RTOL


@gpu
def test_loss_workspace_is_exact_and_refusals_touch_nothing(hip):
    x, lab = loss_inputs("px257")
    B, ncls, HW = x.shape
    xd, ld = put(x), put(lab)
    nbytes = hip.lib().cswin_loss_workspace(B, ncls, HW)
    o = dict(sums=Guarded((1 + 3 * ncls,)), workspace=Guarded((nbytes // 4,)), dlogits=Guarded((B, ncls, HW)))
    args = lambda n, nb: (hip.ptr(xd), hip.ptr(ld), hip.ptr(o["sums"].t), hip.ptr(o["workspace"].t), nb, B, n, HW, 0, hip.stream())
    hip.refused(ERR_WORKSPACE, "loss_sums one byte short", o, "cswin_loss_sums", *args(ncls, nbytes - 1))
    coef = put(np.ones(2 * 17, np.float32))
    for n in LOSS_REFUSED_NCLS:
        big = hip.lib().cswin_loss_workspace(B, n, HW)
        ws = Guarded((max(big, nbytes) // 4,))
        oo = dict(sums=Guarded((1 + 3 * n,)), workspace=ws, dlogits=Guarded((B, max(n, ncls), HW)))
        hip.refused(ERR_UNSUPPORTED, f"loss_sums ncls={n}", oo, "cswin_loss_sums", hip.ptr(put(np.zeros((B, n, HW), np.float32))), hip.ptr(ld), hip.ptr(oo["sums"].t),
                    hip.ptr(ws.t), big, B, n, HW, 0, hip.stream())
        hip.refused(ERR_UNSUPPORTED, f"loss_bwd ncls={n}", oo, "cswin_loss_bwd", hip.ptr(put(np.zeros((B, n, HW), np.float32))), hip.ptr(ld), hip.ptr(coef), None,
                    hip.ptr(oo["dlogits"].t), 1.0, 1.0, B, n, HW, 0, hip.stream())


def finalize(hip, sums, n_pixels, w_ce, w_dice, cw=None, what=""):
    ncls = (len(sums) - 1) // 3
    o = dict(out3=Guarded((3,)), coef=Guarded((2 * ncls,)))
    sd, cwd = put(np.asarray(sums, np.float32)), None if cw is None else put(np.asarray(cw, np.float32))
    hip.call("cswin_loss_finalize", hip.ptr(sd), hip.ptr(o["out3"].t), hip.ptr(o["coef"].t), float(n_pixels), ncls, w_ce, w_dice, hip.ptr(cwd), hip.stream())
    torch.cuda.synchronize()
    assert all(g.intact() for g in o.values()), what
    return o["out3"].t.cpu().numpy().astype(np.float64), o["coef"].t.cpu().numpy().astype(np.float64)


@gpu
def test_loss_finalize_forms(hip):
    """With and without class weights, n_pixels other than the local count, w_ce = 0 with a poisoned CE sum, and a class that is
    absent from labels and predictions.  The reference works from the fp32 sums the kernel is given."""
    x, lab = loss_inputs("nc5.logits")
    ncls, n = 5, x.shape[0] * x.shape[2]
    sums = loss_ref(x, lab)[0].astype(np.float32)
    cw = np.array([0.5, 2.0, 0.0, 1.25, 3.0], np.float32)
    for what, w, npx, w_ce, w_dice in (("plain", None, n, 0.4, 0.6), ("weights", cw, n, 0.4, 0.6), ("global_n", cw, 4 * n + 3, 0.25, 1.5), ("dice_only", None, n, 0.0, 1.0)):
        out3, coef = finalize(hip, sums, npx, w_ce, w_dice, w, what)
        want, bwant, cref = final_ref(sums, npx, w_ce, w_dice, w)
        close(out3, want, bwant, f"tail.finalize.{what}.out3")
        close(coef, cref, 8 * U * np.abs(cref), f"tail.finalize.{what}.coef")
    poisoned = sums.copy()
    poisoned[0] = np.nan
    out3, coef = finalize(hip, poisoned, n, 0.0, 0.6, cw, "poisoned")
    want, bwant, _ = final_ref(sums, n, 0.0, 0.6, cw)
    assert np.isnan(out3[1]) and np.isfinite(out3[0]) and abs(out3[0] - 0.6 * want[2]) <= bwant[0] and abs(out3[2] - want[2]) <= bwant[2]
    out3, _ = finalize(hip, poisoned, n, 0.4, 0.6, cw, "poisoned.ce")
    assert np.isnan(out3[0])
    # a class that no label names and no pixel predicts: logit -40 everywhere, D ~ smooth, its Dice term ~ 0
    xa = np.array(x)
    xa[:, 3] = -40.0
    la = np.where(lab == 3, 0, lab)
    s, out3, coef, dl = run_loss(hip, xa, la, what="tail.loss.absent")
    ref, bound = loss_ref(xa, la)
    close(s, ref, bound, "tail.loss.absent.sums")
    want, bwant, _ = final_ref(ref, n, 0.4, 0.6, bsums=bound)
    close(out3, want, bwant, "tail.loss.absent.out3")
    assert ref[1 + ncls + 3] == 0 and ref[1 + 2 * ncls + 3] < 1e-30 and abs((ref[1 + 2 * ncls + 3] + SMOOTH) / SMOOTH - 1) < 1e-20
    assert measure(dl, grad_ref(xa, la, False, 0.4 / n, 0.6 / ncls), "tail.loss.absent.dlogits") <= RTOL


@gpu
@pytest.mark.parametrize("probs", [False, True], ids=["logits", "probs"])
def test_loss_bwd_scales_and_grad_out(hip, probs):
    """grad_out NULL and 1.7; ce_scale and dice_scale chosen independently of the loss weights; class weights in the coefficients."""
    x, lab = loss_inputs("nc7.probs" if probs else "nc7.logits")
    cw = np.array([1.0, 0.5, 2.0, 0.25, 1.5, 0.0, 3.0], np.float32)
    for gout, ce_scale, dice_scale, w in ((None, 0.4 / 273, 0.6 / 7, None), (1.7, 0.4 / 273, 0.6 / 7, None), (1.7, 3.0e-3, 0.0, None), (None, 0.0, 1.9, cw), (1.7, 1.1e-2, 0.37, cw)):
        what = f"tail.lossbwd.{'probs' if probs else 'logits'}.g{gout}.ce{ce_scale:.2e}.dice{dice_scale}.{'cw' if w is not None else 'nocw'}"
        _, _, _, dl = run_loss(hip, x, lab, probs, 0.0 if probs else 0.4, 0.6, cw=w, ce_scale=ce_scale, dice_scale=dice_scale, gout=gout, what=what)
        ref = grad_ref(x, lab, probs, ce_scale, dice_scale, 1.0 if gout is None else gout, w)
        if float(ref.abs().max()) == 0.0:
            assert float(dl.abs().max()) == 0.0, what
        else:
            assert measure(dl, ref, what) <= RTOL


@gpu
def test_loss_two_ranks_emulated_on_one_device(hip):
    """_CeDiceLoss's data-parallel contract without a process group: the halves' sums added, finalize on the global pixel
    count, loss_bwd per half with dice_scale = w_dice / ncls * 2 and ce_scale = w_ce / (B_local * HW); half of each local
    gradient is the float64 gradient of the global-batch loss for that half."""
    ncls, B, HW, w_ce, w_dice = 4, 4, 91, 0.4, 0.6
    x, lab = det_normal("tail.loss.ranks.x", (B, ncls, HW)), det_labels("tail.loss.ranks.lab", (B, 7, 13), ncls).reshape(B, HW)
    halves = [(x[:2], lab[:2]), (x[2:], lab[2:])]
    local = [run_loss(hip, xh, lh, what=f"tail.loss.ranks.sums{r}")[0] for r, (xh, lh) in enumerate(halves)]
    total = (local[0] + local[1]).astype(np.float32)
    ref, bound = loss_ref(x, lab)
    b2 = sum(loss_ref(xh, lh)[1] for xh, lh in halves) + U * np.abs(ref)
    close(total, ref, b2, "tail.loss.ranks.sums")
    xl = D(x)
    nll, I, Y, Z = loss_graph(xl, lab)
    (w_ce * nll / (B * HW) + w_dice * dice_terms(I, Y, Z) / ncls).backward()
    for r, (xh, lh) in enumerate(halves):
        _, out3, _, dl = run_loss(hip, xh, lh, n_pixels=B * HW, ce_scale=w_ce / (2 * HW), dice_scale=w_dice / ncls * 2, sums_in=total, what=f"tail.loss.ranks.bwd{r}")
        want, bwant, _ = final_ref(ref, B * HW, w_ce, w_dice, bsums=b2)
        close(out3, want, bwant, f"tail.loss.ranks.out3.{r}")
        assert measure(0.5 * dl, xl.grad[2 * r:2 * r + 2], f"tail.loss.ranks.dlogits{r}") <= RTOL


@gpu
@pytest.mark.parametrize("bad", OOR_LABELS, ids=[str(b) for b in OOR_LABELS])
def test_out_of_range_labels(hip, bad):
    """-1, ncls, 255 and 2^32 + 1 each poison CE + Dice; with w_ce = 0 the loss is finite and loss and gradient are those of the
    float64 restatement, where such a pixel matches no class.

    Measured on an MI355X: a kernel that truncates the label to 32 bits before the range check takes 2^32 + 1 for class 1 and
    returns sums[0] = 598.45, loss 1.388 instead of NaN.  With the 64-bit check both are NaN, and the Dice-only run gives
    tail.loss.oor4294967297.sums 3.5e-08, .out3 6.1e-08, .dlogits 1.1e-06."""
    ncls = 6
    x, lab = loss_inputs("nc6.logits")
    lab = np.array(lab)
    lab[0, 17] = lab[2, 90] = ncls if bad == "ncls" else bad
    B, _, HW = x.shape
    sums, out3, _, _ = run_loss(hip, x, lab, what=f"tail.loss.oor{bad}.ce", nan_ok=True)
    ref, bound = loss_ref(x, lab)
    assert np.isnan(ref[0]) and np.isnan(sums[0]) and np.isnan(out3[0]), (sums[0], out3)
    close(sums[1:], ref[1:], bound[1:], f"tail.loss.oor{bad}.sums")
    sums, out3, _, dl = run_loss(hip, x, lab, w_ce=0.0, w_dice=1.0, what=f"tail.loss.oor{bad}.dice", nan_ok=True)
    want, bwant, _ = final_ref(ref, B * HW, 0.0, 1.0, bsums=bound)
    close(out3[[0, 2]], want[[0, 2]], bwant[[0, 2]], f"tail.loss.oor{bad}.out3")
    assert not torch.isnan(dl).any()
    assert measure(dl, grad_ref(x, lab, False, 0.0, 1.0 / ncls), f"tail.loss.oor{bad}.dlogits") <= RTOL


# ---- SGD, gather, wire format -------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("weight_decay", [0.0, 1e-4])
@pytest.mark.parametrize("momentum", [0.0, 0.9])
@pytest.mark.parametrize("n", [s[0] for s in SGD_SIZES])
def test_sgd_flat_three_steps_vs_torch_sgd_float64(hip, n, momentum, weight_decay):
    """Three steps from m = 0 with lr_dev rewritten on the device in between.  Each step is compared element by element with
    torch.optim.SGD in float64 started from the state the kernel had (so the bound of one step applies):
    |dp| <= 4 * 2^-24 * (|p| + |lr| A), |dm| <= 4 * 2^-24 * A, A = |mu m| + |g s| + |wd p| -- the update is at most four roundings
    under -ffp-contract=fast.  An uninterrupted float64 run is compared with the final state by the suite's measure.  The
    shadow is bit for bit the RNE bf16 of the p the same launch wrote."""
    p0, g = det_normal(f"tail.sgd.{n}.p", (n,)), [det_normal(f"tail.sgd.{n}.g{k}", (n,)) for k in range(3)]
    for mu, wd, gs, shadow in [a for a in SGD_ARGS if a[:2] == (momentum, weight_decay)]:
        what = f"tail.sgd.n{n}.mu{mu}.wd{wd}.gs{gs}.{'shadow' if shadow else 'noshadow'}"
        o = dict(p=Guarded((n,)), m=Guarded((n,)))
        if shadow:
            o["shadow"] = Guarded((n,), torch.bfloat16)
        o["p"].t.copy_(torch.from_numpy(p0))
        o["m"].t.zero_()
        lr_dev = put(np.array([SGD_LRS[0]], np.float32))
        free = torch.from_numpy(p0).double().requires_grad_()
        opt_free = torch.optim.SGD([free], lr=1.0, momentum=mu, weight_decay=wd)
        p_prev, m_prev = torch.from_numpy(p0).double(), torch.zeros(n, dtype=torch.float64)
        for k in range(3):
            if k:
                lr_dev.mul_(SGD_LRS[k] / SGD_LRS[k - 1])                # rewritten on the device: the host passes no learning rate
            lr = float(lr_dev.cpu()[0])
            gd = put(g[k])
            hip.call("cswin_sgd_flat", hip.ptr(o["p"].t), hip.ptr(gd), hip.ptr(o["m"].t), n, hip.ptr(lr_dev), mu, wd, gs,
                     hip.ptr(o["shadow"].t) if shadow else None, hip.stream())
            settle(what, o)
            g64 = torch.from_numpy(g[k]).double() * gs
            leaf = p_prev.clone().requires_grad_()
            opt = torch.optim.SGD([leaf], lr=lr, momentum=mu, weight_decay=wd)
            if mu and k:
                opt.state[leaf]["momentum_buffer"] = m_prev.clone()
            leaf.grad = g64.clone()
            opt.step()
            m_ref = opt.state[leaf]["momentum_buffer"] if mu else g64 + wd * p_prev
            A = (mu * m_prev).abs() + g64.abs() + (wd * p_prev).abs()
            p_got, m_got = o["p"].t.cpu().double(), o["m"].t.cpu().double()
            dp, dm = (p_got - leaf.detach()).abs(), (m_got - m_ref).abs()
            assert bool((dp <= 4 * U * (p_prev.abs() + abs(lr) * A)).all()), (what, k, float(dp.max()))
            assert bool((dm <= 4 * U * A).all()), (what, k, float(dm.max()))
            if shadow:
                want, nan = rne_bf16(bits32(o["p"].t))
                assert not nan.any() and (bits16(o["shadow"].t) == want).all(), what
            for grp in opt_free.param_groups:
                grp["lr"] = lr
            free.grad = g64.clone()
            opt_free.step()
            p_prev, m_prev = p_got, m_got
        assert measure(o["p"].t, free.detach(), what + ".p") <= RTOL
        if mu:
            assert measure(o["m"].t, opt_free.state[free]["momentum_buffer"], what + ".m") <= RTOL


@gpu
def test_sgd_flat_refuses_misaligned_buffers(hip):
    n = 8
    o = dict(p=GuardedAt((n,), off=1), g=GuardedAt((n,), off=1), m=GuardedAt((n,), off=1), shadow=GuardedAt((n,), torch.bfloat16, off=1),
             p0=Guarded((n,)), g0=Guarded((n,)), m0=Guarded((n,)), shadow0=Guarded((n,), torch.bfloat16))
    lr = put(np.array([0.1], np.float32))
    ptrs = lambda **k: [hip.ptr(o[k.get(name, name + "0")].t) for name in ("p", "g", "m")]
    for name in ("p", "g", "m"):
        pp, gg, mm = ptrs(**{name: name})
        hip.refused(ERR_ALIGN, f"sgd_flat {name} 4 bytes off", o, "cswin_sgd_flat", pp, gg, mm, n, hip.ptr(lr), 0.9, 1e-4, 1.0, hip.ptr(o["shadow0"].t), hip.stream())
    pp, gg, mm = ptrs()
    hip.refused(ERR_ALIGN, "sgd_flat shadow 2 bytes off", o, "cswin_sgd_flat", pp, gg, mm, n, hip.ptr(lr), 0.9, 1e-4, 1.0, hip.ptr(o["shadow"].t), hip.stream())


@gpu
def test_multi_copy_every_length_and_alignment(hip):
    """One table, 24 chunks: arbitrary bit patterns (NaN payloads among them) must arrive unchanged and nowhere else."""
    rng = np.random.RandomState(11)
    rows, outs, srcs = [], {}, {}
    for n, (so, do) in itertools.product(COPY_SIZES, COPY_ALIGN):
        pat = rng.randint(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
        pat[::5] = np.array([0x7F800001, 0xFFC12345, 0x7FC00000, 0x80000000], np.uint32)[np.arange(len(pat[::5])) % 4]
        src = put(pat.view(np.int32), so // 4)
        dst = GuardedAt((n,), off=do // 4)
        rows.append((src.data_ptr(), dst.t.data_ptr(), n))
        srcs[n, so, do], outs[f"{n}.{so}.{do}"] = pat, dst
    table = put(np.asarray(rows, np.int64))
    hip.call("cswin_multi_copy", hip.ptr(table), len(rows), hip.stream())
    torch.cuda.synchronize()
    for (n, so, do), pat in srcs.items():
        g = outs[f"{n}.{so}.{do}"]
        assert g.intact(), f"multi_copy n={n} src+{so} dst+{do}: a guard word was overwritten"
        assert (bits32(g.t) == pat).all(), f"multi_copy n={n} src+{so} dst+{do}"


@gpu
def test_flat_sgd_gathers_gradients_from_odd_offsets(hip):
    """FlatSGD.gather_grads with .grad tensors that are views at odd element offsets into a larger buffer: slots receive exactly
    their gradients, pad words of flat_grad stay 0, and pad words of flat_param are still 0 after a step."""
    from cswin_unet_amd.optim import FlatSGD
    params = [torch.nn.Parameter(torch.from_numpy(det_normal(f"tail.gather.p{n}", (n,))).to(DEV)) for n in GATHER_PARAMS]
    opt = FlatSGD(params, lr=0.1, momentum=0.9, weight_decay=1e-4)
    pool = torch.from_numpy(det_normal("tail.gather.pool", (sum(GATHER_PARAMS) + 64,))).to(DEV)
    at = 1
    for p in params:
        p.grad = pool[at:at + p.numel()]
        assert p.grad.data_ptr() % 16 != 0 and (p.grad.data_ptr() // 4) % 2 == 1
        at += p.numel() + (p.numel() % 2)                               # the next view starts at an odd element again
    flat = opt.gather_grads()
    torch.cuda.synchronize()
    pad = torch.ones(opt.numel, dtype=torch.bool)
    for p, off in zip(params, opt.offsets):
        assert (bits32(flat[off:off + p.numel()]) == bits32(p.grad)).all()
        pad[off:off + p.numel()] = False
    assert int(pad.sum()) == opt.numel - sum(GATHER_PARAMS) > 0
    assert (bits32(flat)[pad.numpy()] == 0).all()
    opt.apply()
    torch.cuda.synchronize()
    assert (bits32(opt.flat_param)[pad.numpy()] == 0).all() and (bits32(opt.flat_mom)[pad.numpy()] == 0).all()
    for p, off in zip(params, opt.offsets):
        want = torch.from_numpy(det_normal(f"tail.gather.p{p.numel()}", (p.numel(),))).double()
        want = want - 0.1 * (p.grad.cpu().double() + 1e-4 * want)
        assert measure(opt.flat_param[off:off + p.numel()], want, f"tail.gather.p{p.numel()}") <= RTOL


def check_packed(got, src_bits, scale, what):
    """bf16 patterns `got` against the integer RNE of fl32(src * scale): NaN stays NaN, everything else bit for bit."""
    want, nan = rne_bf16(scaled_bits(src_bits, scale))
    is_nan = (got & 0x7FFF) > 0x7F80
    bad = np.where(nan, ~is_nan, got != want)
    assert not bad.any(), f"{what}: {[(hex(int(s)), hex(int(g)), hex(int(w))) for s, g, w in zip(src_bits[bad][:8], got[bad][:8], want[bad][:8])]} (source, got, want)"


@gpu
@pytest.mark.parametrize("scale", WIRE_SCALES, ids=["1", "0.5", "third"])
def test_pack_bf16_scaled_bit_patterns(hip, scale):
    """The wire table through the 16-B body (the table padded to a multiple of 4) and through the scalar tail: for every tail
    length r = 1, 2, 3 the rows go r at a time through launches of n = 4 + r."""
    tab = wire_table()
    body = np.concatenate([tab, tab[:(-len(tab)) % 4]])
    dst = Guarded((len(body),), torch.bfloat16)
    hip.call("cswin_pack_bf16_scaled", hip.ptr(put(body.view(np.int32))), hip.ptr(dst.t), len(body), scale, hip.stream())
    torch.cuda.synchronize()
    assert dst.intact()
    check_packed(bits16(dst.t), body, scale, f"pack_bf16 x{scale} body")
    if scale == 1.0:                                                  # cswin_pack_bf16 is the scaled entry point at scale 1: body and a tail of 3
        plain = Guarded((len(body),), torch.bfloat16)
        hip.call("cswin_pack_bf16", hip.ptr(put(body.view(np.int32))), hip.ptr(plain.t), len(body) - 1, hip.stream())
        torch.cuda.synchronize()
        assert plain.intact() and (bits16(plain.t)[-1:] == 0x7FC0).all()
        check_packed(bits16(plain.t)[:-1], body[:-1], 1.0, "pack_bf16 body and tail")
    for r in (1, 2, 3):
        nblk = cdiv(len(tab), r)
        src = np.zeros((nblk, 8), np.uint32)
        src[:, :4] = tab[:4]
        idx = np.minimum(np.arange(nblk * r).reshape(nblk, r), len(tab) - 1)
        src[:, 4:4 + r] = tab[idx]
        sd, out = put(src.view(np.int32)), Guarded((nblk, 8), torch.bfloat16)
        for j in range(nblk):
            hip.call("cswin_pack_bf16_scaled", hip.ptr(sd[j]), hip.ptr(out.t[j]), 4 + r, scale, hip.stream())
        torch.cuda.synchronize()
        got = bits16(out.t).reshape(nblk, 8)
        assert out.intact() and (got[:, 4 + r:] == 0x7FC0).all(), f"pack_bf16 tail {r}: wrote past n"
        check_packed(got[:, :4 + r].reshape(-1), src[:, :4 + r].reshape(-1), scale, f"pack_bf16 x{scale} tail {r}")
    for n in (1, 2, 3):
        out = Guarded((4,), torch.bfloat16)
        hip.call("cswin_pack_bf16_scaled", hip.ptr(put(tab[-4:].view(np.int32))), hip.ptr(out.t), n, scale, hip.stream())
        torch.cuda.synchronize()
        got = bits16(out.t)
        assert out.intact() and (got[n:] == 0x7FC0).all()
        check_packed(got[:n], tab[-4:][:n], scale, f"pack_bf16 x{scale} n={n}")


@gpu
def test_unpack_bf16_every_pattern_and_wire_refusals(hip):
    pats = np.arange(65536, dtype=np.uint32)
    src = put(pats.astype(np.uint16).view(np.int16))
    for n in (65536, 65535, 1, 2, 3):
        out = Guarded((65536,))
        hip.call("cswin_unpack_bf16", hip.ptr(src), hip.ptr(out.t), n, hip.stream())
        torch.cuda.synchronize()
        assert out.intact()
        got = bits32(out.t)
        assert (got[:n] == pats[:n] << 16).all(), f"unpack_bf16 n={n}: {[hex(int(p)) for p in pats[:n][got[:n] != pats[:n] << 16][:8]]}"
        assert (got[n:] == 0x7FC00000).all(), f"unpack_bf16 n={n} wrote past n"
    f, f1 = Guarded((8,)), GuardedAt((8,), off=1)
    h, h1 = Guarded((8,), torch.bfloat16), GuardedAt((8,), torch.bfloat16, off=1)
    o = dict(f=f, f1=f1, h=h, h1=h1)
    zf, zh = put(np.zeros(8, np.float32)), put(np.zeros(8, np.int16))
    hip.refused(ERR_ALIGN, "pack_bf16 src 4 bytes off", o, "cswin_pack_bf16_scaled", hip.ptr(put(np.zeros(8, np.float32), 1)), hip.ptr(h.t), 8, 1.0, hip.stream())
    hip.refused(ERR_ALIGN, "pack_bf16 dst 2 bytes off", o, "cswin_pack_bf16_scaled", hip.ptr(zf), hip.ptr(h1.t), 8, 1.0, hip.stream())
    hip.refused(ERR_ALIGN, "unpack_bf16 dst 4 bytes off", o, "cswin_unpack_bf16", hip.ptr(zh), hip.ptr(f1.t), 8, hip.stream())
    hip.refused(ERR_ALIGN, "unpack_bf16 src 2 bytes off", o, "cswin_unpack_bf16", hip.ptr(put(np.zeros(8, np.int16), 1)), hip.ptr(f.t), 8, hip.stream())
    hip.refused(ERR_SHAPE, "pack_bf16 n = 0", o, "cswin_pack_bf16_scaled", hip.ptr(zf), hip.ptr(h.t), 0, 1.0, hip.stream())


# ---- dropout ------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("case", DROP_CASES, ids=[c[0] for c in DROP_CASES])
def test_dropout_mask_is_the_documented_generator(hip, case):
    """The kept set is exactly the restated generator's, read off a launch without residual on an input bounded away from 0
    (|x| >= 0.25, scale >= 0.5: a kept product cannot vanish); that launch's y = rs * x, rs = fl32(row_scale * fl32(1 / (1 - p))),
    is within 2 ulp of y.  With a residual, y = residual + rs * x is within 2 ulp taken at the largest of |residual|, |rs x| and
    |y|: the product's rounding is an ulp of the product, which a cancelling residual does not shrink."""
    tag, n, p, eps, has_res, has_rs, epoch = case
    x = det_normal(f"tail.drop.{tag}.x", (n,))
    x = (np.where(x < 0, -1.0, 1.0) * (0.25 + np.abs(x))).astype(np.float32)
    res = det_normal(f"tail.drop.{tag}.res", (n,)) if has_res else None
    rows = cdiv(n, eps)
    rs = (0.5 + np.abs(det_normal(f"tail.drop.{tag}.rs", (rows,)))).astype(np.float32) if has_rs else None
    if has_rs:
        rs[1 % rows] = 0.0
    xd, rsd = put(x), None if rs is None else put(rs)
    ep = None if not epoch else put(np.array([epoch], np.int64))
    keep = keep_mask(DROP_SEED, epoch, n, p)
    if p in (0.0, 1e-6):
        assert keep.all()
    inv_keep = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    scale = np.full(n, inv_keep, np.float32) if rs is None else (rs * inv_keep)[np.arange(n) // eps]
    prod = np.where(keep, scale.astype(np.float64) * x, 0.0)

    def launch(residual, what):
        y = Guarded((n,))
        hip.call("cswin_dropout", hip.ptr(xd), None if residual is None else hip.ptr(put(residual)), hip.ptr(rsd), hip.ptr(y.t), n, eps, p, DROP_SEED,
                 hip.ptr(ep), hip.stream())
        settle(f"dropout {tag} {what}", dict(y=y))
        return y.t.cpu().numpy().astype(np.float64)

    def ulps(got, want, mag, what):
        worst = float((np.abs(got - want) / np.maximum(np.spacing(mag.astype(np.float32)).astype(np.float64), 1e-45)).max())
        print(f"tail.drop.{tag}.{what}: kept {keep.mean():.4f}, worst error {worst:.2f} ulp")
        try:
            with open(LOG, "a") as f:
                f.write(f"tail.drop.{tag}.{what}.ulp: {worst:.3e}\n")
        except OSError:
            pass
        assert worst <= 2.0, (tag, what, worst)

    got = launch(None, "mask")
    live = scale != 0
    assert ((got != 0) == keep)[live].all(), f"dropout {tag}: the kept set differs at {int(((got != 0) != keep)[live].sum())} elements"
    assert (got[~live] == 0).all()
    ulps(got, prod, np.abs(prod), "product")
    if has_res:
        want = prod + res.astype(np.float64)
        ulps(launch(res, "residual"), want, np.maximum(np.maximum(np.abs(prod), np.abs(want)), np.abs(res)), "residual")
    if tag == "p0.3.big":                                             # the mask of a short run is the prefix of a long run's
        short = Guarded((4096,))
        hip.call("cswin_dropout", hip.ptr(put(np.ones(4096, np.float32))), None, None, hip.ptr(short.t), 4096, 4096, p, DROP_SEED, None, hip.stream())
        settle("dropout short", dict(y=short))
        assert ((short.t.cpu().numpy() != 0) == keep[:4096]).all()


@gpu
def test_dropout_refusals_touch_nothing(hip):
    y, y1 = Guarded((8,)), GuardedAt((8,), off=1)
    o = dict(y=y, y1=y1)
    x = put(np.ones(8, np.float32))
    a = lambda xx, rr, yy, n, eps, p: (hip.ptr(xx), hip.ptr(rr), None, hip.ptr(yy), n, eps, p, DROP_SEED, None, hip.stream())
    hip.refused(ERR_SHAPE, "dropout n % 4 != 0", o, "cswin_dropout", *a(x, None, y.t, 6, 4, 0.3))
    hip.refused(ERR_SHAPE, "dropout elems_per_sample % 4 != 0", o, "cswin_dropout", *a(x, None, y.t, 8, 6, 0.3))
    hip.refused(ERR_SHAPE, "dropout p = 1", o, "cswin_dropout", *a(x, None, y.t, 8, 4, 1.0))
    hip.refused(ERR_ALIGN, "dropout y 4 bytes off", o, "cswin_dropout", *a(x, None, y1.t, 8, 4, 0.3))
    hip.refused(ERR_ALIGN, "dropout x 4 bytes off", o, "cswin_dropout", *a(put(np.ones(8, np.float32), 1), None, y.t, 8, 4, 0.3))
    hip.refused(ERR_ALIGN, "dropout residual 4 bytes off", o, "cswin_dropout", *a(x, put(np.ones(8, np.float32), 1), y.t, 8, 4, 0.3))


# ---- layout adapters, window permutes ---------------------------------------------------------------------------------------
def tok_roundtrip(hip, B, H, W, C, Cpad, what):
    x = torch.from_numpy(det_normal(f"tail.tok.{B}.{H}x{W}.{C}", (B, C, H, W)))
    tok = Guarded((B, H * W, Cpad))
    hip.call("cswin_nchw_to_tokens", hip.ptr(put(x)), hip.ptr(tok.t), B, C, H, W, Cpad, hip.stream())
    settle("nchw_to_tokens " + what, dict(y=tok))
    want = torch.zeros(B, H * W, Cpad)
    want[:, :, :C] = x.reshape(B, C, H * W).permute(0, 2, 1)
    assert (bits32(tok.t) == bits32(want)).all(), "nchw_to_tokens " + what         # bit for bit: padded channels are +0
    src = torch.from_numpy(det_normal(f"tail.tok.back.{B}.{H}x{W}.{Cpad}", (B, H * W, Cpad)))
    img = Guarded((B, C, H, W))
    hip.call("cswin_tokens_to_nchw", hip.ptr(put(src)), hip.ptr(img.t), B, C, H, W, Cpad, hip.stream())
    settle("tokens_to_nchw " + what, dict(y=img))
    assert (bits32(img.t) == bits32(src[:, :, :C].permute(0, 2, 1).reshape(B, C, H, W))).all(), "tokens_to_nchw " + what


@gpu
@pytest.mark.parametrize("hw", TOK_HW, ids=[f"{h}x{w}" for h, w in TOK_HW])
def test_layout_adapters_bit_exact(hip, hw):
    for B, C in itertools.product(TOK_B, TOK_C):
        for Cpad in tok_cpads(C):
            tok_roundtrip(hip, B, hw[0], hw[1], C, Cpad, f"B{B} {hw[0]}x{hw[1]} C{C} Cpad{Cpad}")


@gpu
def test_layout_adapters_past_their_grid_clamps(hip):
    B, H, W, C, Cpad = TOK_BIG
    tok_roundtrip(hip, B, H, W, C, Cpad, "past the clamps")


def windows_ref(img, H_sp, W_sp):
    """img2windows as the model documents it: B C H W -> view (B, C, H/H_sp, H_sp, W/W_sp, W_sp) -> permute (0, 2, 4, 3, 5, 1) ->
    (B * H/H_sp * W/W_sp, H_sp * W_sp, C)."""
    B, C, H, W = img.shape
    return img.view(B, C, H // H_sp, H_sp, W // W_sp, W_sp).permute(0, 2, 4, 3, 5, 1).contiguous().reshape(-1, H_sp * W_sp, C)


def image_ref(win, H_sp, W_sp, H, W):
    """windows2img: B' (H_sp W_sp) C -> view (B, H/H_sp, W/W_sp, H_sp, W_sp, C) -> permute (0, 1, 3, 2, 4, 5) -> B H W C."""
    B = win.shape[0] // ((H // H_sp) * (W // W_sp))
    return win.view(B, H // H_sp, W // W_sp, H_sp, W_sp, -1).permute(0, 1, 3, 2, 4, 5).contiguous().view(B, H, W, -1)


@gpu
@pytest.mark.parametrize("case", WINDOW_CASES, ids=lambda c: "x".join(map(str, c)))
def test_window_permutes_bit_exact_and_round_trip(hip, case):
    B, C, H, W, hs, ws = case
    img = torch.from_numpy(det_normal("tail.win." + ".".join(map(str, case)), (B, C, H, W)))
    win = Guarded((B * (H // hs) * (W // ws), hs * ws, C))
    hip.call("cswin_img2windows", hip.ptr(put(img)), hip.ptr(win.t), B, C, H, W, hs, ws, hip.stream())
    settle("img2windows", dict(out=win))
    want = windows_ref(img, hs, ws)
    assert (bits32(win.t) == bits32(want)).all()
    back = Guarded((B, H, W, C))
    hip.call("cswin_windows2img", hip.ptr(win.t), hip.ptr(back.t), B, C, H, W, hs, ws, hip.stream())
    settle("windows2img", dict(out=back))
    assert (bits32(back.t) == bits32(image_ref(want, hs, ws, H, W))).all()
    assert (bits32(back.t) == bits32(img.permute(0, 2, 3, 1))).all()              # the round trip is the NHWC image


@gpu
def test_window_permutes_refuse_windows_that_do_not_divide(hip):
    for B, C, H, W, hs, ws in WINDOW_REFUSED:
        o = dict(out=Guarded((B * C * H * W,)))
        src = put(np.zeros(B * C * H * W, np.float32))
        for name in ("cswin_img2windows", "cswin_windows2img"):
            hip.refused(ERR_SHAPE, f"{name} {H}x{W} by {hs}x{ws}", o, name, hip.ptr(src), hip.ptr(o["out"].t), B, C, H, W, hs, ws, hip.stream())


# ---- head composition ---------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("case", HEAD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_head_compose_and_backward_vs_float64(hip, case):
    """With b_out, without, and the backward also without db_fused; rows ncls..Cpad of w_fused and b_fused are exact zeros."""
    ncls, E, C, Cpad = case
    tag = "tail.head." + "x".join(map(str, case))
    wh, wo, bo = det_normal(tag + ".wh", (ncls, E), E ** -0.5), det_normal(tag + ".wo", (E, C), C ** -0.5), det_normal(tag + ".bo", (E,), 0.5)
    dwf, dbf = det_normal(tag + ".dwf", (Cpad, C)), det_normal(tag + ".dbf", (Cpad,))
    whd, wod, bod, dwfd, dbfd = put(wh), put(wo), put(bo), put(dwf), put(dbf)
    Wh, Wo, Bo, dWf, dBf = (torch.from_numpy(a).double() for a in (wh, wo, bo, dwf[:ncls], dbf[:ncls]))
    for bias, dbias in ((True, True), (True, False), (False, False), (False, True)):
        what = f"{tag}.{'bias' if bias else 'nobias'}.{'db' if dbias else 'nodb'}"
        o = dict(w_fused=Guarded((Cpad, C)), b_fused=Guarded((Cpad,)), dw_head=Guarded((ncls, E)), dw_out=Guarded((E, C)))
        if bias:
            o["db_out"] = Guarded((E,))
        hip.call("cswin_head_compose", hip.ptr(whd), hip.ptr(wod), hip.ptr(bod) if bias else None, hip.ptr(o["w_fused"].t), hip.ptr(o["b_fused"].t),
                 ncls, E, C, Cpad, hip.stream())
        hip.call("cswin_head_compose_bwd", hip.ptr(whd), hip.ptr(wod), hip.ptr(bod) if bias else None, hip.ptr(dwfd), hip.ptr(dbfd) if dbias else None,
                 hip.ptr(o["dw_head"].t), hip.ptr(o["dw_out"].t), hip.ptr(o["db_out"].t) if bias else None, ncls, E, C, hip.stream())
        settle(what, o)
        assert measure(o["w_fused"].t[:ncls], Wh @ Wo, what + ".w_fused") <= RTOL
        assert (bits32(o["w_fused"].t[ncls:]) == 0).all() and (bits32(o["b_fused"].t[ncls:]) == 0).all()
        if bias:
            assert measure(o["b_fused"].t[:ncls], Wh @ Bo, what + ".b_fused") <= RTOL
        else:
            assert (bits32(o["b_fused"].t) == 0).all()
        both = bias and dbias
        assert measure(o["dw_head"].t, dWf @ Wo.t() + (torch.outer(dBf, Bo) if both else 0.0), what + ".dw_head") <= RTOL
        assert measure(o["dw_out"].t, Wh.t() @ dWf, what + ".dw_out") <= RTOL
        if both:
            assert measure(o["db_out"].t, Wh.t() @ dBf, what + ".db_out") <= RTOL
        elif bias:
            assert (bits32(o["db_out"].t) == 0).all()


@gpu
def test_head_compose_refusals_touch_nothing(hip):
    o = dict(a=Guarded((16, 8)), b=Guarded((16,)), c=Guarded((8,)))
    z = put(np.zeros(256, np.float32))
    hip.refused(ERR_SHAPE, "head_compose Cpad < ncls", o, "cswin_head_compose", hip.ptr(z), hip.ptr(z), None, hip.ptr(o["a"].t), hip.ptr(o["b"].t), 9, 8, 8, 8, hip.stream())
    hip.refused(ERR_SHAPE, "head_compose_bwd db_out without b_out", o, "cswin_head_compose_bwd", hip.ptr(z), hip.ptr(z), None, hip.ptr(z), hip.ptr(z),
                hip.ptr(o["a"].t), hip.ptr(o["b"].t), hip.ptr(o["c"].t), 2, 8, 8, hip.stream())
