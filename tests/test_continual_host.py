"""Host side of the continual-learning objective (ops.continual_loss, csrc/cl_loss.hip, cswin_unet_amd/continual.py); no GPU.

cl_torch is the float64 restatement of universal_train.py:904-932 with the torch calls of the cited lines on .double() CPU tensors:
F.cross_entropy(weight=, reduction='none') -> exp -> alpha (1 - pt)^gamma ce (:165-173), a softmax Dice, and
F.kl_div(log_softmax(student[:, :nold] / T), softmax(teacher / T), 'batchmean') * T^2 (:618-623).  cl_ref restates the same in
numpy, in the sums layout of cswin_cl_loss_sums, and derives for the focal and the KD sum a bound from the magnitudes summed --
the method of test_gpu_step_tail.loss_ref, whose bounds hold the first 1 + 3*ncls sums:

  focal term f(ce) = alpha (1 - pt)^gamma ce, ce = w nll.  nll carries loss_ref's a_nll units (2^-24) of ABSOLUTE error, the
  product by w half a unit of ce, so ce is off by w a_nll + ce units and f by f'(ce) times that; -expm1f(-ce) adds 2.5 units of
  f per factor (1 - pt), the gamma - 1 products, the product by ce and by alpha one each: (3.5 gamma + 2) |f|.
  KD term q_c (lq_c - lp_c), lq_c = dt_c - log St, dt_c = (t_c - max t) / T.  dt_c carries 1.5 units of itself (difference,
  1/T, product), exp(dt_c) therefore eps_c = 2 + 4 |dt_c| (loss_ref's 2 + 2.5 |d| plus the argument's 1.5 |d|), the row sum
  r = sum_j q_j eps_j + nold - 1, its logarithm r + 2.5 |log St| + 1 absolute, lq_c 1.5 |dt_c| + that + 0.5 |lq_c|; the same for
  the student; the difference adds half a unit of itself; q_c carries eps_c + r + 3; the nold terms pass nold - 1 additions.  A
  q_c that underflows is flushed: 2^-126 |lq_c - lp_c| absolute.
  Both then pass the additions every sum passes (loss_ref's depth)."""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle.determ import det_labels, det_normal

from test_gpu_step_tail import SMOOTH, U, cdiv, final_ref, loss_blocks, loss_ref, trips

TINY = 2.0 ** -126


# ------------------------------------------------------------------------------------------------
# case table: (tag, B, (H, W), ncls, nold, kind, options).  HW = 7 * 13 is odd and no multiple of B = 3.
# options: T, gamma, alpha, cw (class weights given), lmap (label map given)
# ------------------------------------------------------------------------------------------------
def _opts(**kw):
    o = dict(T=3.0, gamma=4.0, alpha=1.0, cw=False, lmap=False)
    o.update(kw)
    return o


def _switch_nold(n, k):
    return (1, 2, n - 1, n)[k % 4]


CL_NCLS = [(f"nc{n}.old{_switch_nold(n, n)}", 3, (7, 13), n, _switch_nold(n, n), "normal",
            _opts(cw=bool(n % 2), lmap=_switch_nold(n, n) < n and n % 3 != 1, gamma=(4.0, 2.0, 1.0)[n % 3]))
           for n in range(2, 17)]                                                   # every NC; nold cycles through 1, 2, n - 1, n
CL_NCLS += [("nc12.old9", 3, (7, 13), 12, 9, "normal", _opts(cw=True, lmap=True)),   # stage 1: 9 + 4 - 1
            ("nc14.old12", 3, (7, 13), 14, 12, "normal", _opts(cw=True, lmap=True))]  # stage 2: 12 + 3 - 1
CL_PIXELS = [(f"px{B * H * W}.nc{n}", B, (H, W), n, o, "normal", _opts(cw=n == 12))
             for n, o in ((12, 9), (2, 2))
             for B, (H, W) in ((1, (1, 1)), (3, (5, 17)), (1, (1, 257)), (3, (211, 211)))]  # 1, 255, 257, 133 563 > 512 * 256: a second trip of the sums loop
CL_PIXELS += [("px526338.nc2", 2, (513, 513), 2, 2, "normal", _opts())]               # > 4 * 512 * 256: a second trip of the backward loop
CL_HARD = [
    ("confident.cw", 3, (7, 13), 12, 9, "confident", _opts(cw=True)),   # every pixel confident, weights ~3e-4: ce ~ 3e-7, gamma 4
    ("confident", 3, (7, 13), 12, 9, "confident", _opts()),             # the same without weights: nll itself ~ 1e-6
    ("gap.T3", 3, (7, 13), 12, 9, "gap", _opts(T=3.0)),                 # teacher and student gaps of 300 > 87.4 * 3
    ("gap.T1", 3, (7, 13), 12, 9, "gap", _opts(T=1.0)),                 # ... and > 87.4 at T = 1
    ("offset1e4", 3, (7, 13), 12, 9, "offset", _opts(cw=True)),         # a common offset of 1e4 on logits and teacher
    ("weight0", 3, (7, 13), 12, 9, "weight0", _opts(cw=True)),          # a class of weight 0 that occurs in the labels
    ("absent", 3, (7, 13), 12, 9, "absent", _opts(lmap=True)),          # a class no label names and no pixel predicts
] + [(f"gamma{g}", 3, (7, 13), 12, 9, "normal", _opts(gamma=float(g), alpha=0.75, cw=bool(g % 4), lmap=g in (1, 4))) for g in (0, 1, 2, 4)]
CL_CASES = CL_NCLS + CL_PIXELS + CL_HARD


def case_of(tag):
    return next(c for c in CL_CASES if c[0] == tag)


@functools.lru_cache(maxsize=None)
def cl_inputs(tag):
    """(x (B, ncls, HW) f32, raw labels (B, HW) int64, teacher (B, nold, HW) f32, class weights (ncls,) f32 or None, label map
    int32 or None) of a row of CL_CASES; computed once, never written."""
    _, B, (H, W), ncls, nold, kind, o = case_of(tag)
    HW = H * W
    x = det_normal(f"cl.{tag}.x", (B, ncls, HW))
    t = det_normal(f"cl.{tag}.t", (B, nold, HW))
    new = ncls - nold + 1
    if o["lmap"]:
        lab = det_labels(f"cl.{tag}.lab", (B, H, W), new).reshape(B, HW)
        lmap = np.arange(new, dtype=np.int32) + np.int32(nold - 1)
        lmap[0] = 0
        final = lmap[lab].astype(np.int64)
    else:
        lab = det_labels(f"cl.{tag}.lab", (B, H, W), ncls).reshape(B, HW)
        lmap, final = None, lab
    cw = None
    if o["cw"]:
        cw = (0.25 + np.abs(det_normal(f"cl.{tag}.cw", (ncls,)))).astype(np.float32)
        cw[0] = 0.5
    if kind == "confident":
        # label's logit 9.3 (with weights ~3e-4: nll ~ 1e-3, ce ~ 3e-7: five units of 2^-24) or 16.2 (nll ~ 1e-6) above eleven others near 0
        x = (0.01 * x).astype(np.float32)
        np.put_along_axis(x, final[:, None, :], np.float32(9.3 if o["cw"] else 16.2), 1)
        if o["cw"]:
            cw = (3e-4 * (1.0 + 0.1 * np.abs(det_normal(f"cl.{tag}.cw", (ncls,))))).astype(np.float32)
    if kind == "gap":
        x, t = x.copy(), t.copy()
        x[:, 1] -= 300.0
        x[:, 7, ::2] -= 500.0
        t[:, 2] -= 300.0
        t[:, 7, 1::2] -= 700.0
    if kind == "offset":
        x, t = (x + np.float32(1e4)).astype(np.float32), (t + np.float32(1e4)).astype(np.float32)
    if kind == "weight0":
        cw = cw.copy()
        cw[int(np.bincount(final.ravel()).argmax())] = 0.0              # the most frequent class
    if kind == "absent":
        x = x.copy()
        x[:, nold + 1] = -40.0
        lab = np.where(final == nold + 1, 0, lab)
    return x, lab, t, cw, lmap


def map_labels(lab, lmap):
    """The label after the optional table: lmap[l] for 0 <= l < len(lmap), -1 (no class) otherwise."""
    lab = np.asarray(lab, np.int64)
    if lmap is None:
        return lab
    inside = (lab >= 0) & (lab < len(lmap))
    return np.where(inside, np.asarray(lmap, np.int64)[np.where(inside, lab, 0)], -1)


# ------------------------------------------------------------------------------------------------
# float64 restatements
# ------------------------------------------------------------------------------------------------
def cl_torch(x, lab, t, T=3.0, alpha=1.0, gamma=4.0, cw=None, lmap=None):
    """(focal sum, I, Y, Z, kd as the reference forms it (batchmean, * T^2), plain nll sum) as float64 tensors on the autograd graph
    of x (B, ncls, HW), with the torch calls of universal_train.py:165-173 and :618-623.  A pixel whose label is no class has no
    focal term here (the kernel's NaN is asserted separately) and matches no class in Dice."""
    ncls, nold = x.shape[1], t.shape[1]
    lab = torch.from_numpy(map_labels(lab, lmap))
    valid = (lab >= 0) & (lab < ncls)
    tgt = torch.where(valid, lab, torch.zeros_like(lab))
    w = None if cw is None else torch.as_tensor(np.asarray(cw, np.float64))
    ce = F.cross_entropy(x, tgt, weight=w, reduction='none')
    pt = torch.exp(-ce)
    focal = alpha * (1 - pt) ** gamma * ce if gamma != 0 else alpha * ce
    focal = torch.where(valid, focal, torch.zeros_like(focal)).sum()
    nll = torch.where(valid, F.cross_entropy(x, tgt, reduction='none'), torch.zeros_like(ce)).sum()
    p = torch.softmax(x, 1)
    oh = (lab[:, None, :] == torch.arange(ncls)[None, :, None]).double()
    kd = x.sum() * 0.0
    if nold:
        tt = torch.as_tensor(np.asarray(t, np.float64))
        kd = F.kl_div(F.log_softmax(x[:, :nold] / T, dim=1), F.softmax(tt / T, dim=1), reduction='batchmean') * T ** 2
    return focal, (p * oh).sum((0, 2)), oh.sum((0, 2)), (p * p).sum((0, 2)), kd, nll


def dice_sum(I, Y, Z):
    return (1 - (2 * I + SMOOTH) / (Z + Y + SMOOTH)).sum()


def cl_objective(x, lab, t, n_pixels, batch, w_focal=0.2, w_dice=0.8, kd_weight=0.5, T=3.0, alpha=1.0, gamma=4.0, cw=None, lmap=None):
    """(loss, focal, dice, kd, ce) of universal_train.py:928-932 as float64 tensors; n_pixels and batch: what x covers."""
    f, I, Y, Z, kd, nll = cl_torch(x, lab, t, T, alpha, gamma, cw, lmap)
    focal, dice, ce = f / n_pixels, dice_sum(I, Y, Z) / x.shape[1], nll / n_pixels
    kd = kd * x.shape[0] / batch                                       # batchmean over `batch` images
    return (1 - kd_weight) * (w_focal * focal + w_dice * dice) + kd_weight * kd, focal, dice, kd, ce


def cl_grad_ref(x, lab, t, focal_scale, dice_scale, kd_scale, g=1.0, T=3.0, alpha=1.0, gamma=4.0, cw=None, lmap=None):
    """d/dx of g * (focal_scale * focal sum + dice_scale * sum_c dice_c + kd_scale * T * KD sum) by float64 autograd: what
    cswin_cl_loss_bwd documents (the KD sum's derivative is (pT - q) / T)."""
    xl = torch.from_numpy(np.asarray(x, np.float64)).requires_grad_()
    f, I, Y, Z, kd, _ = cl_torch(xl, lab, t, T, alpha, gamma, cw, lmap)
    skd = kd * x.shape[0] / T ** 2
    (g * (focal_scale * f + dice_scale * dice_sum(I, Y, Z) + kd_scale * T * skd)).backward()
    return xl.grad


def cl_ref(x, lab, t, T=3.0, alpha=1.0, gamma=4.0, cw=None, lmap=None, _wrong=None):
    """(sums[3 + 3*ncls], bound) in numpy float64 (see the module docstring).  _wrong (the sensitivity test alone): "omp_fp32"
    (1 - exp(-ce) in fp32), "log_q" (log of the fp32 teacher probability instead of the logit form), "kd_all_channels" (student
    softmax over all ncls channels), "weight_after_pt" (pt = exp(-nll), the class weight applied to the result)."""
    B, ncls, HW = x.shape
    nold = t.shape[1] if t is not None else 0
    lab = map_labels(lab, lmap)
    base, bbase = loss_ref(x, lab)
    # loss_ref's inputs never underflow; here a probability may (a logit 300 below the row maximum): what fp32 flushes is off by
    # at most 2^-126 per pixel, in the intersect and the z sums
    bbase = bbase + np.concatenate([[0.0], np.full(ncls, B * HW * TINY), np.zeros(ncls), np.full(ncls, B * HW * TINY)])
    v = x.astype(np.float64)
    valid = (lab >= 0) & (lab < ncls)
    safe = np.where(valid, lab, 0)
    oh = (lab[:, None, :] == np.arange(ncls)[None, :, None]).astype(np.float64)
    mx = v.max(1, keepdims=True)
    d = v - mx
    e = np.exp(d)
    s = e.sum(1)
    p = e / s[:, None]
    eps = 2.0 + 2.5 * np.abs(d)
    rsum = (p * eps).sum(1) + (ncls - 1)
    dl = -(d * oh).sum(1)
    nll = dl + np.log(s)
    a_nll = 0.5 * dl + rsum + 2.5 * np.abs(np.log(s)) + 1.0 + 0.5 * np.abs(nll)
    w = np.ones_like(nll) if cw is None else np.asarray(cw, np.float64)[safe]
    ce = w * nll
    omp = -np.expm1(-ce)
    if _wrong == "omp_fp32":
        omp = (np.float32(1.0) - np.exp((-ce).astype(np.float32))).astype(np.float64)
    if _wrong == "weight_after_pt":
        omp = -np.expm1(-nll)
    f = alpha * omp ** gamma * ce
    fprime = alpha * (omp ** gamma + (gamma * omp ** (gamma - 1) * np.exp(-ce) * ce if gamma != 0 else 0.0))
    a_f = fprime * (w * a_nll + ce) + (3.5 * gamma + 2.0) * f
    f, a_f = np.where(valid, f, 0.0), np.where(valid, a_f, 0.0)
    blocks = loss_blocks(B * HW)
    depth = trips(B * HW, blocks)[1] + 6 + 3 + cdiv(blocks, 16) + 16
    focal, b_focal = f.sum(), U * (a_f.sum() + depth * f.sum())
    if not valid.all():
        focal = np.nan
    kd, b_kd = 0.0, 0.0
    if nold:
        zt, zs = np.asarray(t, np.float64), v[:, :nold]
        dt, dz = (zt - zt.max(1, keepdims=True)) / T, (zs - zs.max(1, keepdims=True)) / T
        if _wrong == "kd_all_channels":
            dz = ((v - mx) / T)
        et, ez = np.exp(dt), np.exp(dz)
        St, Sz = et.sum(1, keepdims=True), ez.sum(1, keepdims=True)
        q, pz = et / St, (ez / Sz)[:, :nold]
        dz = dz[:, :nold]
        lq, lp = dt - np.log(St), dz - np.log(Sz)
        if _wrong == "log_q":
            et32 = np.exp(dt.astype(np.float32))
            with np.errstate(divide="ignore", invalid="ignore"):
                q = (et32 / et32.sum(1, keepdims=True)).astype(np.float64)
                lq = np.log(q)
        Dc = lq - lp
        with np.errstate(invalid="ignore"):
            term = q * Dc
        k = term.sum(1)
        epsT, epsZ = 2.0 + 4.0 * np.abs(dt), 2.0 + 4.0 * np.abs(dz)
        rT, rZ = (q * epsT).sum(1, keepdims=True) + (nold - 1), (pz * epsZ).sum(1, keepdims=True) + (nold - 1)
        e_lq = 1.5 * np.abs(dt) + rT + 2.5 * np.abs(np.log(St)) + 1.0 + 0.5 * np.abs(lq)
        e_lp = 1.5 * np.abs(dz) + rZ + 2.5 * np.abs(np.log(Sz)) + 1.0 + 0.5 * np.abs(lp)
        with np.errstate(invalid="ignore"):
            a_term = q * (e_lq + e_lp + 0.5 * np.abs(Dc)) + np.abs(term) * (epsT + rT + 3.5) + TINY / U * np.abs(Dc)
        a_k = a_term.sum(1) + (nold - 1) * np.abs(term).sum(1)
        kd, b_kd = k.sum(), U * (a_k.sum() + depth * np.abs(k).sum())
    return np.concatenate([base, [focal, kd]]), np.concatenate([bbase, [b_focal, b_kd]])


def cl_final_ref(sums, n_pixels, batch, w_focal, w_dice, kd_weight, T, bsums=None, _wrong=None):
    """cswin_cl_loss_finalize in float64: (out5 = [loss, focal, dice, kd, ce], their bounds, coef).  ce, dice and coef are
    final_ref's; focal = S_f / n adds 2 roundings, kd = S_kd T^2 / batch 4, the combination 3 per product pair and 4 at the end.
    _wrong = "kd_per_pixel": KD divided by the pixels instead of the images."""
    sums = np.asarray(sums, np.float64)
    ncls = (len(sums) - 3) // 3
    bs = np.zeros_like(sums) if bsums is None else np.asarray(bsums, np.float64)
    (_, ce, dice), (_, b_ce, b_dice), coef = final_ref(sums[:1 + 3 * ncls], n_pixels, 1.0, 1.0, bsums=bs[:1 + 3 * ncls])
    focal = sums[1 + 3 * ncls] / n_pixels
    b_focal = bs[1 + 3 * ncls] / n_pixels + 2 * U * abs(focal)
    kd = sums[2 + 3 * ncls] * T * T / (n_pixels if _wrong == "kd_per_pixel" else batch)
    b_kd = bs[2 + 3 * ncls] * T * T / batch + 4 * U * abs(kd)
    keep = 1.0 - kd_weight
    seg = (w_focal * focal if w_focal != 0 else 0.0) + w_dice * dice
    loss = (keep * seg if keep != 0 else 0.0) + (kd_weight * kd if kd_weight != 0 else 0.0)
    b_seg = (abs(w_focal) * b_focal + 3 * U * abs(w_focal * focal) if w_focal != 0 else 0.0) + abs(w_dice) * b_dice + 3 * U * abs(w_dice * dice)
    b_loss = (abs(keep) * b_seg if keep != 0 else 0.0) + (abs(kd_weight) * b_kd if kd_weight != 0 else 0.0)
    b_loss += 4 * U * ((abs(keep * seg) if keep != 0 and np.isfinite(seg) else 0.0) + (abs(kd_weight * kd) if kd_weight != 0 else 0.0))
    return np.array([loss, focal, dice, kd, ce]), np.array([b_loss, b_focal, b_dice, b_kd, b_ce]), coef


# ------------------------------------------------------------------------------------------------
# the restatements against each other and against explicit loops
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["nc6.old5", "nc12.old9", "gamma0", "gamma1", "gap.T3", "weight0"])
def test_restatement_agrees_with_explicit_per_pixel_loops(tag):
    x, lab, t, cw, lmap = cl_inputs(tag)
    _, B, (H, W), ncls, nold, _, o = case_of(tag)
    T, alpha, gamma = o["T"], o["alpha"], o["gamma"]
    sums, bound = cl_ref(x, lab, t, T, alpha, gamma, cw, lmap)
    assert sums.shape == bound.shape == (3 + 3 * ncls,) and np.isfinite(bound).all() and (bound >= 0).all()
    f, I, Y, Z, kd, nll = (float(v) if v.dim() == 0 else v.numpy() for v in cl_torch(torch.from_numpy(x).double(), lab, t, T, alpha, gamma, cw, lmap))
    got = np.concatenate([[nll], I, Y, Z, [f, kd * B / T ** 2]])
    assert np.abs(got - sums).max() <= 1e-12 * np.abs(sums).max(), np.abs(got - sums).max()
    # explicit loops over pixels and classes, math.* only
    lm = map_labels(lab, lmap)
    focal = kdsum = nllsum = 0.0
    for b in range(B):
        for i in range(H * W):
            row = [float(x[b, c, i]) for c in range(ncls)]
            m = max(row)
            lse = m + math.log(sum(math.exp(r - m) for r in row))
            l = int(lm[b, i])
            one = lse - row[l]
            ce = one * (float(cw[l]) if cw is not None else 1.0)
            focal += alpha * (1.0 - math.exp(-ce)) ** gamma * ce if gamma else alpha * ce
            nllsum += one
            zs, zt = [r / T for r in row[:nold]], [float(t[b, c, i]) / T for c in range(nold)]
            ms, mt = max(zs), max(zt)
            ls = ms + math.log(sum(math.exp(z - ms) for z in zs))
            lt = mt + math.log(sum(math.exp(z - mt) for z in zt))
            kdsum += sum(math.exp(zt[c] - lt) * ((zt[c] - lt) - (zs[c] - ls)) for c in range(nold))
    # (1 - exp(-ce))^gamma in plain float64 loses digits for tiny ce; these rows have none
    assert abs(focal - sums[1 + 3 * ncls]) <= 1e-12 * abs(focal) and abs(nllsum - sums[0]) <= 1e-12 * abs(nllsum)
    assert abs(kdsum - sums[2 + 3 * ncls]) <= 1e-12 * max(abs(kdsum), 1.0)
    # the objective's five outputs from the sums equal the torch objective
    n = B * H * W
    out, _, _ = cl_final_ref(sums, n, B, 0.2, 0.8, 0.5, T)
    want = [float(v) for v in cl_objective(torch.from_numpy(x).double(), lab, t, n, B, 0.2, 0.8, 0.5, T, alpha, gamma, cw, lmap)]
    assert np.allclose(out, want, rtol=1e-12, atol=1e-14)


def test_closed_form_gradient_agrees_with_autograd():
    """The formula cswin_cl_loss_bwd documents, written out in float64, against autograd of the restatement."""
    tag = "nc12.old9"
    x, lab, t, cw, lmap = cl_inputs(tag)
    B, ncls, HW = x.shape
    nold, T, alpha, gamma = t.shape[1], 3.0, 1.0, 4.0
    fs, ds, ks = 0.3 / (B * HW), 0.7 / ncls, 0.5 * T / B
    ref = cl_grad_ref(x, lab, t, fs, ds, ks, 1.7, T, alpha, gamma, cw, lmap).numpy()
    sums, _ = cl_ref(x, lab, t, T, alpha, gamma, cw, lmap)
    _, _, coef = cl_final_ref(sums, B * HW, B, 0.2, 0.8, 0.5, T)
    v = x.astype(np.float64)
    p = np.exp(v - v.max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    lm = map_labels(lab, lmap)
    oh = (lm[:, None, :] == np.arange(ncls)[None, :, None]).astype(np.float64)
    w = np.asarray(cw, np.float64)[lm]
    ce = w * -np.log((p * oh).sum(1))
    pt = np.exp(-ce)
    fp = alpha * ((1 - pt) ** gamma + gamma * (1 - pt) ** (gamma - 1) * pt * ce)
    G = coef[:ncls][None, :, None] * oh + coef[ncls:][None, :, None] * p
    grad = fs * (fp * w)[:, None, :] * (p - oh) + ds * p * (G - (p * G).sum(1, keepdims=True))
    pT = np.exp(v[:, :nold] / T - (v[:, :nold] / T).max(1, keepdims=True))
    pT /= pT.sum(1, keepdims=True)
    q = np.exp(t.astype(np.float64) / T - (t.astype(np.float64) / T).max(1, keepdims=True))
    q /= q.sum(1, keepdims=True)
    grad[:, :nold] += ks * (pT - q)
    assert np.abs(1.7 * grad - ref).max() <= 1e-12 * np.abs(ref).max()


# ------------------------------------------------------------------------------------------------
# what the bounds can see
# ------------------------------------------------------------------------------------------------
SUM_BUGS = [  # (planted bug, the rows meant to catch it, the sum that must see it)
    ("omp_fp32", ("confident.cw",), "focal"),
    ("log_q", ("gap.T3", "gap.T1"), "kd"),
    ("kd_all_channels", ("nc12.old9", "nc14.old12", "nc5.old2"), "kd"),
    ("weight_after_pt", ("nc12.old9", "gamma2", "weight0"), "focal"),
]


@pytest.mark.parametrize("bug,tags,seen_by", SUM_BUGS, ids=[b[0] for b in SUM_BUGS])
def test_bound_sees_the_planted_bugs(bug, tags, seen_by):
    """Each planted bug moves the sum named for it by at least four times its bound at each row meant to catch it (a NaN, which
    log(0) * 0 gives, counts as seen)."""
    for tag in tags:
        x, lab, t, cw, lmap = cl_inputs(tag)
        o = case_of(tag)[6]
        ref, bound = cl_ref(x, lab, t, o["T"], o["alpha"], o["gamma"], cw, lmap)
        bad, _ = cl_ref(x, lab, t, o["T"], o["alpha"], o["gamma"], cw, lmap, _wrong=bug)
        k = len(ref) - (2 if seen_by == "focal" else 1)
        moved = abs(bad[k] - ref[k])
        ratio = np.inf if not np.isfinite(bad[k]) else moved / bound[k]
        print(f"{tag} {bug} {seen_by}: ref {ref[k]:.6e} bad {bad[k]:.6e} bound {bound[k]:.3e} ratio {ratio:.3g}")
        assert ratio >= 4.0, (tag, bug, ratio)


def test_bound_sees_a_per_pixel_batchmean():
    """KD divided by the pixels instead of the images moves the kd output and the loss by far more than four times their bounds."""
    for tag in ("nc12.old9", "px255.nc12"):
        x, lab, t, cw, lmap = cl_inputs(tag)
        _, B, (H, W), ncls, nold, _, o = case_of(tag)
        ref, bound = cl_ref(x, lab, t, o["T"], o["alpha"], o["gamma"], cw, lmap)
        out, bout, _ = cl_final_ref(ref, B * H * W, B, 0.2, 0.8, 0.5, o["T"], bsums=bound)
        bad, _, _ = cl_final_ref(ref, B * H * W, B, 0.2, 0.8, 0.5, o["T"], bsums=bound, _wrong="kd_per_pixel")
        assert abs(bad[3] - out[3]) >= 4 * bout[3] and abs(bad[0] - out[0]) >= 4 * bout[0], (tag, out, bad, bout)


def test_new_bounds_are_a_few_dozen_roundings_of_what_was_summed():
    """Neither zero nor slack on ordinary rows: between 10 and 400 units of 2^-24 times the sum of |terms| (the KD terms change
    sign, so the KD sum itself is smaller than what was summed: its bound is measured against sum_c q_c |log q_c - log pT_c|)."""
    for tag in ("nc12.old9", "nc14.old12", "nc5.old2", "gamma1", "px255.nc2"):
        x, lab, t, cw, lmap = cl_inputs(tag)
        o = case_of(tag)[6]
        sums, bound = cl_ref(x, lab, t, o["T"], o["alpha"], o["gamma"], cw, lmap)
        assert 10 <= bound[-2] / (U * sums[-2]) <= 400, (tag, bound[-2] / (U * sums[-2]))
        T, nold = o["T"], t.shape[1]
        lq = torch.log_softmax(torch.from_numpy(t).double() / T, 1)
        lp = torch.log_softmax(torch.from_numpy(x[:, :nold]).double() / T, 1)
        mag = float((lq.exp() * (lq - lp).abs()).sum())
        assert 10 <= bound[-1] / (U * mag) <= 400, (tag, bound[-1] / (U * mag))


# ------------------------------------------------------------------------------------------------
# continual.py
# ------------------------------------------------------------------------------------------------
class _StandIn(torch.nn.Module):
    """A CPU-computable stand-in with the attributes expand_classes touches: features -> `output`, a bias-free 1x1 conv."""

    def __init__(self, num_classes=9, E=8):
        super().__init__()
        self.num_classes = num_classes
        self.body = torch.nn.Conv2d(3, E, 3, padding=1)
        self.output = torch.nn.Conv2d(E, num_classes, kernel_size=1, bias=False)

    def forward(self, x):
        return self.output(torch.relu(self.body(x)))


def test_expand_classes_keeps_the_old_rows_and_the_old_logits():
    from cswin_unet_amd.continual import expand_classes, freeze_teacher
    torch.manual_seed(3)
    net = _StandIn(9)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    teacher = freeze_teacher(net)
    assert not teacher.training and all(not p.requires_grad for p in teacher.parameters())
    assert all(p.data_ptr() != q.data_ptr() for p, q in zip(teacher.parameters(), net.parameters()))
    assert expand_classes(net, 4) == 9 and net.num_classes == 12
    after = net.state_dict()
    assert list(after) == list(before)
    for k in before:
        if k == "output.weight":
            assert tuple(after[k].shape) == (12, 8, 1, 1) and torch.equal(after[k][:9], before[k])
            assert float(after[k][9:].abs().min()) > 0 and net.output.weight.requires_grad
        else:
            assert torch.equal(after[k], before[k])
    assert net.output.bias is None and net.output.kernel_size == (1, 1)
    x = torch.randn(2, 3, 5, 7)
    assert torch.equal(net(x)[:, :9], teacher(x))
    with pytest.raises(ValueError):
        expand_classes(net, 0)


def test_expand_classes_on_the_real_model_and_its_wrapper():
    import os
    from cswin_unet_amd.config import get_config
    from cswin_unet_amd.continual import expand_classes
    from cswin_unet_amd.networks.vision_transformer import CSwinUnet
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    m = CSwinUnet(get_config(os.path.join(root, "configs", "cswin_tiny_224_lite.yaml")), img_size=224, num_classes=9)
    keys, old_w = list(m.state_dict()), m.cswin_unet.output.weight.detach().clone()
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert expand_classes(m, 4) == 9
    assert m.num_classes == m.cswin_unet.num_classes == m.cswin_unet.output.out_channels == 12
    sd = m.state_dict()
    assert list(sd) == keys and torch.equal(sd["cswin_unet.output.weight"][:9], old_w)
    assert all(tuple(sd[k].shape) == shapes[k] for k in keys if k != "cswin_unet.output.weight")
    assert expand_classes(m, 3) == 12 and m.cswin_unet.output.out_channels == 14


def test_new_label_map_is_the_references_three_assignments():
    from cswin_unet_amd.continual import new_label_map
    for old, new in ((9, 4), (12, 3)):
        table = new_label_map(old, new)
        assert table.dtype == torch.int32 and table.numel() == new
        labels = torch.arange(new).repeat(3)
        mapped = labels.clone()                                         # universal_train.py:245-256
        mapped[labels == 1] = old
        mapped[labels == 2] = old + 1
        if new > 3:
            mapped[labels == 3] = old + 2
        assert torch.equal(table.long()[labels], mapped)


def test_extreme_class_weights_against_a_hand_computed_vector():
    from cswin_unet_amd.continual import extreme_class_weights
    counts = [1.0e6, 123.0, 0.0, 400.0, 0.0, 2500.0]
    w = extreme_class_weights(counts, [0, 2, 3, 5])                    # class 1: not active; class 2: active with no pixel
    raw = [1 / math.sqrt(1.0e6 + 1e-6), 0.0, 0.0, 1 / math.sqrt(400 + 1e-6), 0.0, 1 / math.sqrt(2500 + 1e-6)]
    s = raw[0] + raw[3] + raw[5]
    want = [r / s * 4 for r in raw]
    assert w.dtype == torch.float32 and np.allclose(w.numpy(), want, rtol=1e-6, atol=0)
    assert w[1] == 0 and w[2] == 0 and w[4] == 0 and abs(float(w.sum()) - 4.0) < 1e-5
    w = extreme_class_weights([10.0, 1000.0, 1000.0], [0, 1, 2])       # background would get 2.5: capped at 0.5
    assert float(w[0]) == 0.5 and np.allclose(w[1:].numpy(), [3 * 0.1 / (1 + 0.1 + 0.1)] * 2, rtol=1e-5)


def test_new_entry_points_load_without_a_gpu():
    from cswin_unet_amd import _lib
    h = _lib.lib()
    for name in ("cswin_cl_loss_workspace", "cswin_cl_loss_sums", "cswin_cl_loss_finalize", "cswin_cl_loss_bwd"):
        assert name in _lib.SIGNATURES and hasattr(h, name), name
    assert h.cswin_cl_loss_workspace(24, 12, 224 * 224) == 512 * (3 + 36) * 4
    assert h.cswin_cl_loss_workspace(1, 2, 1) == 9 * 4
    from cswin_unet_amd import ops
    from cswin_unet_amd._lib import CswinHipError
    assert "continual_loss" in ops.__all__
    with pytest.raises(CswinHipError):
        ops.continual_loss(torch.zeros(1, 12, 4, 4), torch.zeros(1, 4, 4, dtype=torch.long), torch.zeros(1, 9, 4, 4))
