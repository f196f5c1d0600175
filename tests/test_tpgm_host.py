"""Host side of TPGM (csrc/tpgm.hip, optim.FlatTPGM, continual.TPGM): the float64 restatement of the projection, of the gradient
its radii receive and of their Adam step, and the derived bounds that tests/test_gpu_tpgm*.py use -- checked here against torch
autograd and torch.optim.Adam on the CPU, against a recording of the reference's own tpgm.py (tests/golden/g10_tpgm.npz), against
an fp32 emulation of the kernels and against planted bugs.  No GPU."""
import math
import os

import numpy as np
import pytest
import torch

from oracle.determ import det_normal

from test_adamw_host import BETA1, BETA2, EPS, U, cdiv, sumsq_depth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g10_tpgm.npz")
GAMMA_MIN, NORM_EPS = 1e-2, 1e-8
EXCLUDED, HEAD = 1, 2                   # optim.TPGM_EXCLUDED / TPGM_HEAD (compared in test_init_rule_head_rule_and_tpgm_due)


# ------------------------------------------------------------------------------------------------
# float64 restatement (universal_train.py:391-615 for the forward rules, tpgm.py:47-56 for the gradient)
# ------------------------------------------------------------------------------------------------
def norms_ref(thetas, anchors, l1):
    """Per tensor sqrt(sum d^2), or sum |d| when l1, of d = theta - anchor."""
    out = []
    for p, a in zip(thetas, anchors):
        d = np.asarray(p, np.float64) - np.asarray(a, np.float64)
        out.append(float(np.abs(d).sum()) if l1 else float(np.sqrt((d * d).sum())))
    return np.array(out)


def cmax_ref(norms, flags):
    norms, head = np.asarray(norms, np.float64), (np.asarray(flags) & HEAD) != 0
    return np.where(head, np.maximum(10.0 * norms, 100.0), np.maximum(8.0 * norms, 80.0))


def ratios_ref(gamma, norms, flags, gamma_min=GAMMA_MIN):
    """(ratio, live, unclamped quotient): ratio = hardtanh(clamp(gamma, 1e-2, cmax) / (norm + 1e-8), 0, 1), exactly 1 for an excluded
    tensor; live: the gradient reaches gamma (torch's clamp passes at its bounds, its hardtanh does not; excluded: never)."""
    gamma, norms, flags = np.asarray(gamma, np.float64), np.asarray(norms, np.float64), np.asarray(flags)
    cmax = cmax_ref(norms, flags)
    q = np.clip(gamma, gamma_min, cmax) / (norms + NORM_EPS)
    excl = (flags & EXCLUDED) != 0
    live = (gamma >= gamma_min) & (gamma <= cmax) & (q > 0.0) & (q < 1.0) & ~excl
    return np.where(excl, 1.0, np.clip(q, 0.0, 1.0)), live, q


def project_ref(thetas, anchors, ratios):
    """anchor + ratio (theta - anchor) per tensor in float64; a ratio of exactly 1 returns theta itself."""
    return [np.asarray(p, np.float64) if r == 1.0 else np.asarray(a, np.float64) + r * (np.asarray(p, np.float64) - np.asarray(a, np.float64))
            for p, a, r in zip(thetas, anchors, ratios)]


def dots_ref(grads, thetas, anchors):
    """Per tensor (sum g d, sum |g d|)."""
    out = []
    for g, p, a in zip(grads, thetas, anchors):
        t = np.asarray(g, np.float64) * (np.asarray(p, np.float64) - np.asarray(a, np.float64))
        out.append((float(t.sum()), float(np.abs(t).sum())))
    return np.array(out).reshape(-1, 2)


def gamma_grad_ref(grads, thetas, anchors, gamma, flags, l1, grad_scale=1.0):
    """dL/dgamma_t = grad_scale (sum g~ d) / (norm_t + 1e-8) where live, else 0; grads is dL/dtheta~."""
    norms = norms_ref(thetas, anchors, l1)
    _, live, _ = ratios_ref(gamma, norms, flags)
    return np.where(live, grad_scale * dots_ref(grads, thetas, anchors)[:, 0] / (norms + NORM_EPS), 0.0)


def gamma_adam_ref(gamma, dgamma, m, v, step, lr, flags=None, coef=None):
    """clip_grad_norm_(gamma, 1.0) + one torch.optim.Adam(lr, betas (0.9, 0.999), eps 1e-8) step, step number `step` (1-based):
    (gamma, m, v, gradient norm, clip coefficient).  Excluded radii take no part.  coef: use this coefficient instead."""
    gamma, dgamma, m, v = (np.array(a, np.float64) for a in (gamma, dgamma, m, v))
    keep = np.ones(gamma.size, bool) if flags is None else (np.asarray(flags) & EXCLUDED) == 0
    with np.errstate(invalid="ignore", over="ignore"):
        gnorm = float(np.sqrt((dgamma[keep] ** 2).sum()))
        c = 1.0 / (gnorm + 1e-6)
    c = (1.0 if c > 1.0 else c) if coef is None else coef
    gq = dgamma * c
    m2 = BETA1 * m + (1 - BETA1) * gq
    v2 = BETA2 * v + (1 - BETA2) * gq * gq
    bc1, bc2 = 1 - BETA1 ** step, 1 - BETA2 ** step
    g2 = gamma - (lr / bc1) * m2 / (np.sqrt(v2) / math.sqrt(bc2) + EPS)
    return np.where(keep, g2, gamma), np.where(keep, m2, m), np.where(keep, v2, v), gnorm, c


# ------------------------------------------------------------------------------------------------
# bounds of the fp32 kernels, to first order in U = 2^-24, counted from csrc/tpgm.hip without relying on contraction (an fma
# where two roundings are counted only helps).  sqrt and the division are taken at two roundings (1 ulp), as in test_adamw_host.
# ------------------------------------------------------------------------------------------------
def stat_depth(numel, nchunks):
    """Additions a term passes through up to the per-tensor sum: flat_chunks.h's launch rule (test_adamw_host.sumsq_depth: a thread's
    trips, its four lanes, the tail, the 8 levels of the workgroup) and the tensor's chunks in chunk order."""
    return sumsq_depth(numel, nchunks)


def norm_bound(norm, numel, nchunks, l1):
    """d = fl(p - a) carries U.  l2: d^2 carries 2 + 1, the sum `depth` more and one spare: (depth + 4) U of the sum of squares,
    half of it and the square root's 2 for the norm.  l1: |d| carries 1, the sum depth, one spare."""
    depth = stat_depth(numel, nchunks)
    rel = (depth + 2) if l1 else (depth + 4) / 2 + 2
    return rel * U * np.abs(norm), rel


def dot_bound(abs_dot, numel, nchunks):
    """g * fl(d): 1 + 1, the sum depth, one spare -- against sum |g d|, not against the possibly cancelled dot."""
    return (stat_depth(numel, nchunks) + 3) * U * abs_dot


def ratio_bound(ratio, q, norm_rel, flags):
    """ratio = c / fl(norm + 1e-8): the norm's bound, the sum 1, the division 2, and 1 for c (gamma itself is exact; the clamp
    constants 1e-2, 8 norm and 10 norm are rounded).  0 where the quotient is saturated beyond this bound or the tensor excluded:
    there the kernel must give exactly 0 or 1."""
    rel = (norm_rel + 4) * U
    sat = (np.asarray(q) >= 1.0 + 2 * rel) | ((np.asarray(flags) & EXCLUDED) != 0)
    return np.where(sat, 0.0, rel * np.abs(ratio))


def dgamma_bound(abs_dot, norm, numel, nchunks, l1, grad_scale, live):
    """dgamma = fl(fl(gs * dot) / fl(norm + 1e-8)), gs = fl(grad_scale): the dot's bound, then 1 (gs) + 1 (product) + 1 (sum) + 2
    (division) and the norm's bound, all relative to A = gs sum |g d| / (norm + 1e-8) >= |dgamma|.  0 where the gradient is gated."""
    A = abs(grad_scale) * np.asarray(abs_dot) / (np.asarray(norm) + NORM_EPS)
    rel = np.array([stat_depth(n, c) + 3 + norm_bound(1.0, n, c, l1)[1] + 5 for n, c in zip(numel, nchunks)])
    return np.where(live, rel * U * A, 0.0)


def clip_bounds(dgamma, bdg, gnorm, coef):
    """G = sqrt(sum dgamma^2) added in tensor order by one thread: the inputs' errors give sum |dgamma| e / G, every square 1 and
    at most T additions give (T + 1) / 2, the square root 2.  coef = min(1, 1 / (G + 1e-6)): the sum 1, the division 2; 0 where
    it is clamped to exactly 1 on both sides (the caller decides)."""
    T = len(dgamma)
    bG = (float((np.abs(dgamma) * bdg).sum()) / gnorm if gnorm > 0 else float(np.sqrt((np.asarray(bdg) ** 2).sum()))) + ((T + 1) / 2 + 2) * U * gnorm
    return bG, (bG / (gnorm + 1e-6) + 3 * U) * coef


def adam_bounds(gamma, dgamma, bdg, m, v, step, lr, coef, bcoef, flags=None):
    """(bound gamma, bound m, bound v) of one step from the state (gamma, m, v), given the gradient dgamma +- bdg and the
    coefficient coef +- bcoef.  g' = fl(dgamma coef): e = bdg coef + |dgamma| bcoef + U |g'|.  The arithmetic of the step is
    adamw_elem's without decay (test_adamw_host.adamw_bound: 5U A_m, 8U A_v, U |gamma| + 22U delta); the gradient's own error is
    carried through the step by evaluating the float64 step at g' - e and g' + e (the step is smooth in g' and e is some 1e-6 of
    it, so the first order is the whole of it; it is doubled)."""
    gamma, dgamma, m, v = (np.asarray(a, np.float64) for a in (gamma, dgamma, m, v))
    gq = dgamma * coef
    e = np.asarray(bdg) * coef + np.abs(dgamma) * bcoef + U * np.abs(gq)
    Am = np.abs(BETA1 * m) + np.abs((1 - BETA1) * gq)
    Av = BETA2 * v + (1 - BETA2) * gq * gq
    bc1, bc2 = 1 - BETA1 ** step, 1 - BETA2 ** step
    delta = (lr / bc1) * Am / (np.sqrt(Av) / math.sqrt(bc2) + EPS)
    mid = gamma_adam_ref(gamma, gq, m, v, step, lr, coef=1.0)
    lo = gamma_adam_ref(gamma, gq - e, m, v, step, lr, coef=1.0)
    hi = gamma_adam_ref(gamma, gq + e, m, v, step, lr, coef=1.0)
    carried = [2.0 * np.maximum(np.abs(lo[k] - mid[k]), np.abs(hi[k] - mid[k])) for k in range(3)]
    bg, bm, bv = U * (np.abs(gamma) + 22.0 * delta) + carried[0], 5.0 * U * Am + carried[1], 8.0 * U * Av + carried[2]
    if flags is not None:
        keep = (np.asarray(flags) & EXCLUDED) == 0
        bg, bm, bv = (np.where(keep, b, 0.0) for b in (bg, bm, bv))
    return bg, bm, bv


def project_bound(theta, anchor, ratio, bratio):
    """out = fma(r, fl(theta - anchor), anchor): U |r d| for d, U |out| for the fma, and the ratio's own error |d| bratio; 0 where
    the ratio is exactly 1 (theta's bits)."""
    theta, anchor = np.asarray(theta, np.float64), np.asarray(anchor, np.float64)
    d = theta - anchor
    b = U * (np.abs(ratio * d) + np.abs(anchor + ratio * d)) + np.abs(d) * bratio
    return np.where(ratio == 1.0, 0.0, b)


def update_ref(thetas, anchors, grads, gamma, m, v, flags, l1, grad_scale, step, lr, nchunks=None, coef=None):
    """One projection update in float64 with every bound: a dict of (value, bound) pairs for norm, dgamma, gnorm, coef, gamma, m, v
    and the new ratio.  coef: hold the step to this coefficient (the device's), as test_gpu_adamw does."""
    numel = [np.asarray(p).size for p in thetas]
    nchunks = [cdiv(n, 16384) for n in numel] if nchunks is None else nchunks
    norms = norms_ref(thetas, anchors, l1)
    nb = np.array([norm_bound(x, n, c, l1) for x, n, c in zip(norms, numel, nchunks)])
    _, live, q = ratios_ref(gamma, norms, flags)
    dots = dots_ref(grads, thetas, anchors)
    dg = np.where(live, grad_scale * dots[:, 0] / (norms + NORM_EPS), 0.0)
    bdg = dgamma_bound(dots[:, 1], norms, numel, nchunks, l1, grad_scale, live)
    g2, m2, v2, gnorm, c = gamma_adam_ref(gamma, dg, m, v, step, lr, flags)
    bG, bc = clip_bounds(dg, bdg, gnorm, c)
    if coef is not None:
        g2, m2, v2, _, _ = gamma_adam_ref(gamma, dg, m, v, step, lr, flags, coef=coef)
        bg, bm, bv = adam_bounds(gamma, dg, bdg, m, v, step, lr, coef, 0.0, flags)
    else:
        bg, bm, bv = adam_bounds(gamma, dg, bdg, m, v, step, lr, c, bc, flags)
    r2, _, q2 = ratios_ref(g2, norms, flags)
    # the new ratio: its own arithmetic and, where it is not saturated, the new gamma's error over the norm
    br2 = ratio_bound(r2, q2, nb[:, 1], flags)
    br2 = np.where(br2 > 0, br2 + bg / (norms + NORM_EPS), 0.0)
    return dict(norm=(norms, nb[:, 0]), norm_rel=nb[:, 1], live=live, q=q, dgamma=(dg, bdg), gnorm=(gnorm, bG), coef=(c, bc), gamma=(g2, bg), m=(m2, bm),
                v=(v2, bv), ratio=(r2, br2), q_new=q2)


# ------------------------------------------------------------------------------------------------
# the kernels' arithmetic in numpy float32 (no contraction), in the kernels' own order of summation, with the planted bugs
# ------------------------------------------------------------------------------------------------
F = np.float32
WRONG = ("gradient_through_saturated_ratio", "clip_after_moments", "dot_with_projected_difference", "l1_for_l2")


def chunk_sum_fp32(terms):
    """One workgroup's sum of <= 16384 float32 terms: thread t takes the 4-element groups t, t + 256, ..., adds its four lanes as
    (0 + 1) + (2 + 3), thread t the tail element t, then the xor butterfly of each wave and (w0 + w1) + (w2 + w3)."""
    n = terms.size
    n4 = n // 4
    trips = max(1, cdiv(n4, 256))
    body = np.zeros(trips * 256 * 4, F)
    body[:n4 * 4] = terms[:n4 * 4]
    body = body.reshape(trips, 256, 4)
    acc = np.zeros((256, 4), F)
    for k in range(trips):
        acc = acc + body[k]
    s = (acc[:, 0] + acc[:, 1]) + (acc[:, 2] + acc[:, 3])
    tail = terms[n4 * 4:]
    s[:tail.size] = s[:tail.size] + tail
    s = s.reshape(4, 64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, np.arange(64) ^ o]
    return F((s[0, 0] + s[1, 0]) + (s[2, 0] + s[3, 0]))


def stats_fp32(thetas, anchors, grads, l1, ratios=None):
    """Per tensor (norm statistic, dot) as the two kernels form them: chunk sums, then the chunks in chunk order."""
    out = []
    for t, (p, a) in enumerate(zip(thetas, anchors)):
        d = np.asarray(p, F) - np.asarray(a, F)
        dd = d if ratios is None else F(ratios[t]) * d                   # the planted bug: the projected difference in the dot
        sn, sd = F(0), F(0)
        for c in range(0, d.size, 16384):
            x = d[c:c + 16384]
            sn = sn + chunk_sum_fp32(np.abs(x) if l1 else x * x)
            if grads is not None:
                sd = sd + chunk_sum_fp32(np.asarray(grads[t], F)[c:c + 16384] * dd[c:c + 16384])
        out.append((sn, sd))
    return out


def ratio_fp32(gamma, norm, flag):
    cmax = max(F(10) * norm, F(100)) if flag & HEAD else max(F(8) * norm, F(80))
    c = F(GAMMA_MIN) if gamma < F(GAMMA_MIN) else (cmax if gamma > cmax else gamma)
    r = c / (norm + F(NORM_EPS))
    live = bool(gamma >= F(GAMMA_MIN) and gamma <= cmax and r > 0 and r < 1)
    return (F(0) if r < 0 else (F(1) if r > 1 else r)), live, r


def update_fp32(thetas, anchors, grads, gamma, m, v, flags, l1, grad_scale, step, lr, wrong=None):
    """tpgm_chunk_stats + tpgm_finalize (update) in float32: (norm, gamma, m, v, ratio, [gnorm, coef])."""
    T = len(thetas)
    gamma, m, v = (np.array(a, F) for a in (gamma, m, v))
    use_l1 = (not l1) if wrong == "l1_for_l2" else l1
    proj = None
    if wrong == "dot_with_projected_difference":
        st = stats_fp32(thetas, anchors, None, use_l1)
        proj = [ratio_fp32(gamma[t], st[t][0] if use_l1 else np.sqrt(st[t][0]), flags[t])[0] for t in range(T)]
    st = stats_fp32(thetas, anchors, grads, use_l1, proj)
    norm, dg = np.zeros(T, F), np.zeros(T, F)
    for t in range(T):
        norm[t] = st[t][0] if use_l1 else np.sqrt(st[t][0])
        _, live, r = ratio_fp32(gamma[t], norm[t], flags[t])
        if wrong == "gradient_through_saturated_ratio":
            live = bool(gamma[t] >= F(GAMMA_MIN))
        if live and not flags[t] & EXCLUDED:
            dg[t] = (F(grad_scale) * st[t][1]) / (norm[t] + F(NORM_EPS))
    total = F(0)
    for t in range(T):
        total = total + dg[t] * dg[t]
    gnorm = np.sqrt(total)
    c = F(1) / (gnorm + F(1e-6))
    coef = F(1) if c > 1 else c
    b1, omb1, b2, omb2, eps = F(BETA1), F(1 - BETA1), F(BETA2), F(1 - BETA2), F(EPS)
    stepsz, isb2 = F(lr) / F(1 - BETA1 ** step), F(1.0 / math.sqrt(1 - BETA2 ** step))
    ratio = np.ones(T, F)
    for t in range(T):
        if flags[t] & EXCLUDED:
            continue
        gg = dg[t] if wrong == "clip_after_moments" else dg[t] * coef
        m[t] = b1 * m[t] + omb1 * gg
        v[t] = b2 * v[t] + omb2 * (gg * gg)
        quot = m[t] / (np.sqrt(v[t]) * isb2 + eps)
        if wrong == "clip_after_moments":
            quot = quot * coef
        gamma[t] = gamma[t] - stepsz * quot
        ratio[t] = ratio_fp32(gamma[t], norm[t], flags[t])[0]
    return norm, gamma, m, v, ratio, np.array([gnorm, coef], F)


# ------------------------------------------------------------------------------------------------
# inputs shared with the GPU tests
# ------------------------------------------------------------------------------------------------
RATIO_CASES = ("below", "one", "low", "high", "excluded", "head")


def tpgm_inputs(tag, numels, identical=False, spread=0.05):
    """Per-tensor float32 (theta, anchor, [g0, g1, g2]): anchor ~ N(0, 1), theta = anchor + N(0, spread^2) (theta == anchor when
    identical), gradients ~ N(0, 1) with a quarter each scaled by 1, 1e-2, 1e-4, 1e-6."""
    anchors = [det_normal(f"tpgm.{tag}.a{t}", (n,)) for t, n in enumerate(numels)]
    thetas = [a.copy() if identical else (a + det_normal(f"tpgm.{tag}.d{t}", (n,), spread)).astype(np.float32) for t, (a, n) in enumerate(zip(anchors, numels))]
    gs = []
    for k in range(3):
        g = [det_normal(f"tpgm.{tag}.g{k}.{t}", (n,)) for t, n in enumerate(numels)]
        pos = 0
        for x in g:
            x *= (10.0 ** (-2.0 * ((np.arange(pos, pos + x.size) + k) % 4))).astype(np.float32)
            pos += x.size
        gs.append(g)
    return thetas, anchors, gs


def case_setup(norms, l1=False):
    """(gamma, flags) that put tensor t in RATIO_CASES[t % 6], away from every decision by a margin the three steps of lr <= 0.05
    cannot cross: ratio below 1 (gamma = 0.5 norm or 0.3 norm), exactly 1 (gamma = 2 norm + 1), clamped low
    (gamma = 1e-3: c = 1e-2), clamped high (gamma past cmax), excluded, and a head tensor between 8 norm and 10 norm ... 100."""
    norms = np.asarray(norms, np.float64)
    gamma, flags = np.zeros(norms.size), np.zeros(norms.size, np.int32)
    for t, n in enumerate(norms):
        case = RATIO_CASES[t % 6]
        if case == "below":
            gamma[t] = (0.5 if t // 6 % 2 == 0 else 0.3) * n                 # live when 1e-2 <= gamma; not one ratio for all of them
        elif case == "one":
            gamma[t] = 2.0 * n + 1.0
        elif case == "low":
            gamma[t] = 1e-3
        elif case == "high":
            gamma[t] = max(8.0 * n, 80.0) + 7.0
        elif case == "excluded":
            gamma[t], flags[t] = 0.5 * n, EXCLUDED
        else:
            gamma[t], flags[t] = max(8.0 * n, 80.0) + 7.0, HEAD              # inside the head clamp, past the plain one
    return gamma.astype(np.float32), flags


# ------------------------------------------------------------------------------------------------
# the toy model of the autograd and golden tests: three tensors, one of them a head tensor by its name
# ------------------------------------------------------------------------------------------------
class Toy(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.fc1 = torch.nn.Linear(4, 3)
        self.output = torch.nn.Linear(3, 2, bias=False)

    def forward(self, x):
        return self.output(torch.tanh(self.fc1(x)))


TOY_NAMES = ("fc1.weight", "fc1.bias", "output.weight")
TOY_FLAGS = np.array([0, 0, HEAD], np.int32)


def toy_model(tag, dtype=torch.float64, delta_of=None, scale=0.3):
    """Toy with closed-form parameters; delta_of: another Toy, this one becomes it plus N(0, scale^2)."""
    net = Toy().to(dtype)
    with torch.no_grad():
        for n, p in net.named_parameters():
            val = torch.from_numpy(det_normal(f"tpgm.toy.{tag}.{n}", tuple(p.shape), scale if delta_of is not None else 1.0)).to(dtype)
            p.copy_(val if delta_of is None else dict(delta_of.named_parameters())[n].detach() + val)
    return net


def toy_loss(out, dy):
    return (out * dy).sum()


def autograd_gamma_grad(new, pre, gamma, flags, l1, x, dy):
    """(dL/dgamma, projected parameters, dL/dtheta~) by torch autograd through universal_train.py's forward rules (:460-478) with
    the graph kept as tpgm.py:47-56 keeps it."""
    threshold = torch.nn.Hardtanh(0, 1)
    gam = [torch.tensor(float(g), dtype=torch.float64, requires_grad=True) for g in gamma]
    proj = {}
    for (n, p), a, g, f in zip(new.named_parameters(), pre.parameters(), gam, flags):
        t = p.detach() - a.detach()
        norms = torch.sum(torch.abs(t)) if l1 else torch.norm(t)
        cmax = max(norms.item() * 10, 100.0) if f & HEAD else max(norms.item() * 8, 80.0)
        ratio = threshold(torch.clamp(g, min=1e-2, max=cmax) / (norms + 1e-8))
        proj[n] = t * ratio + a.detach()
    loss = toy_loss(torch.func.functional_call(new, proj, (x,)), dy)
    dgam = torch.autograd.grad(loss, gam, allow_unused=True)
    leaves = {n: v.detach().clone().requires_grad_() for n, v in proj.items()}
    gt = torch.autograd.grad(toy_loss(torch.func.functional_call(new, leaves, (x,)), dy), list(leaves.values()))
    return (np.array([0.0 if g is None else float(g) for g in dgam]), [v.detach().numpy() for v in proj.values()], [g.numpy() for g in gt])


# ------------------------------------------------------------------------------------------------
# tests
# ------------------------------------------------------------------------------------------------
# gamma as a multiple of the tensor's norm, or an absolute value: below 1e-2, above cmax, ratio > 1, strictly inside
TOY_CASES = {"inside": ("rel", 0.5, 0.25, 0.75), "below_min_above_cmax_over_one": ("abs", 1e-3, 500.0, 50.0),
             "over_one_inside_head_between_clamps": ("mixed", 3.0, 0.6, 90.0)}


@pytest.mark.parametrize("l1", [False, True], ids=["l2", "l1"])
@pytest.mark.parametrize("case", sorted(TOY_CASES))
def test_gamma_grad_ref_agrees_with_autograd(case, l1):
    pre = toy_model("anchor")
    new = toy_model("new", delta_of=pre)
    thetas = [p.detach().numpy() for p in new.parameters()]
    anchors = [p.detach().numpy() for p in pre.parameters()]
    norms = norms_ref(thetas, anchors, l1)
    kind, *vals = TOY_CASES[case]
    gamma = np.array(vals) * norms if kind == "rel" else np.array(vals)
    if kind == "mixed":
        gamma = np.array([vals[0] * norms[0], vals[1] * norms[1], vals[2]])
    x, dy = (torch.from_numpy(det_normal(f"tpgm.toy.{k}", s)).double() for k, s in (("x", (5, 4)), ("dy", (5, 2))))
    got, proj, gt = autograd_gamma_grad(new, pre, gamma, TOY_FLAGS, l1, x, dy)
    ratio, live, q = ratios_ref(gamma, norms, TOY_FLAGS)
    want = gamma_grad_ref(gt, thetas, anchors, gamma, TOY_FLAGS, l1)
    print(case, "norms", norms, "gamma", gamma, "q", q, "live", live, "autograd", got, "ref", want)
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    for a, b in zip(proj, project_ref(thetas, anchors, ratio)):
        assert np.abs(a - b).max() <= 1e-12
    if case == "inside":
        assert live.all() and (np.abs(want) > 1e-3).all()
    elif case == "below_min_above_cmax_over_one":
        # gamma < 1e-2: the ratio is 1e-2 / norm, inside (0, 1), and still no gradient; gamma > cmax; 1 < ratio < cmax / norm
        assert not live.any() and (want == 0).all() and 0 < q[0] < 1 and gamma[1] > cmax_ref(norms, TOY_FLAGS)[1] and q[2] > 1 and ratio[2] == 1
    else:
        assert list(live) == [False, True, False] and q[0] > 1 and 80 < gamma[2] < 100 and want[1] != 0


def test_gamma_adam_ref_agrees_with_torch_adam_after_clip_grad_norm():
    """Three steps, the clip active in the first two and not in the third, zero gradients included (Adam moves such a gamma by
    its momentum): 1e-12."""
    gamma0 = np.array([3.0, 0.7, 10.0, 4.5, 0.02])
    grads = [np.array([2.0, -1.5, 0.0, 0.3, 1e-4]), np.array([0.0, 4.0, 0.0, -0.2, 0.0]), np.array([0.1, 0.0, 0.0, -0.3, 0.2])]
    leaves = [torch.tensor([g], dtype=torch.float64, requires_grad=True) for g in gamma0]
    opt = torch.optim.Adam(leaves, lr=0.01)
    gamma, m, v = gamma0.copy(), np.zeros(5), np.zeros(5)
    coefs = []
    for k, g in enumerate(grads):
        for l, x in zip(leaves, g):
            l.grad = torch.tensor([x], dtype=torch.float64)
        total = float(torch.nn.utils.clip_grad_norm_(leaves, max_norm=1.0))
        opt.step()
        gamma, m, v, gnorm, c = gamma_adam_ref(gamma, g, m, v, k + 1, 0.01)
        coefs.append(c)
        assert abs(total - gnorm) <= 1e-12 * gnorm
        for got, want in ((np.array([float(l.detach()) for l in leaves]), gamma), (np.array([float(opt.state[l]["exp_avg"]) for l in leaves]), m),
                          (np.array([float(opt.state[l]["exp_avg_sq"]) for l in leaves]), v)):
            assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), k
    assert coefs[0] < 1 and coefs[1] < 1 and coefs[2] == 1.0
    assert gamma[2] == 10.0                                             # never a gradient, never a momentum: it stood still
    assert gamma[0] != gamma0[0] and abs(gamma[4] - gamma0[4]) > 1e-3   # a zero gradient at the second step still moved them
    kept = gamma_adam_ref(gamma0, grads[0], np.zeros(5), np.zeros(5), 1, 0.01, flags=np.array([0, EXCLUDED, 0, 0, 0]))
    assert kept[0][1] == gamma0[1] and kept[1][1] == 0 and kept[3] < np.linalg.norm(grads[0])


def test_restatement_against_the_recorded_tpgm_py():
    """tests/golden/g10_tpgm.npz: the reference's own tpgm.py (l2 mode, init=False, gamma preset inside (0, norm)) on the toy model
    in float32 -- its projected parameters and the gradients its constraints receive after one backward.  The restatement is fed
    the recorded inputs only; the tolerance is float32's: some 30 roundings of the largest magnitude involved."""
    z = np.load(GOLDEN)
    thetas, anchors = [z["new." + n] for n in TOY_NAMES], [z["anchor." + n] for n in TOY_NAMES]
    gamma = z["gamma"]
    norms = norms_ref(thetas, anchors, False)
    assert (gamma > GAMMA_MIN).all() and (gamma < norms).all()
    ratio, live, _ = ratios_ref(gamma, norms, TOY_FLAGS)
    assert live.all()
    proj = project_ref(thetas, anchors, ratio)
    for n, got in zip(TOY_NAMES, proj):
        want = z["projected." + n]
        assert np.abs(got - want).max() <= 30 * U * max(1.0, np.abs(want).max()), n
    new = Toy().double()
    leaves = {n: torch.from_numpy(p).requires_grad_() for n, p in zip(TOY_NAMES, proj)}
    out = torch.func.functional_call(new, leaves, (torch.from_numpy(z["x"]).double(),))
    assert np.abs(out.detach().numpy() - z["out"]).max() <= 100 * U * np.abs(z["out"]).max()
    gt = torch.autograd.grad(toy_loss(out, torch.from_numpy(z["dy"]).double()), list(leaves.values()))
    got = gamma_grad_ref([g.numpy() for g in gt], thetas, anchors, gamma, TOY_FLAGS, False)
    scale = dots_ref([g.numpy() for g in gt], thetas, anchors)[:, 1] / norms
    print("recorded", z["gamma_grad"], "restated", got, "sum |g d| / norm", scale)
    assert (np.abs(got - z["gamma_grad"]) <= 100 * U * scale).all() and (np.abs(got) > 1e-3).all()


def test_init_rule_head_rule_and_tpgm_due():
    from cswin_unet_amd.continual import tpgm_due
    from cswin_unet_amd.optim import TPGM_EXCLUDED, TPGM_HEAD, tpgm_init_gamma, tpgm_is_head
    assert (TPGM_EXCLUDED, TPGM_HEAD) == (EXCLUDED, HEAD)
    heads = ["output.weight", "cswin_unet.output.weight", "Segmentation_Head.0.bias", "final_conv.weight", "Classifier.bias", "stage1.0.attns.0.HEAD"]
    plain = ["stage1.0.qkv.weight", "norm_up.bias", "merge1.conv.weight", "upsample1.encoder.weight", "stage_up4.0.mlp.fc2.bias"]
    assert all(tpgm_is_head(n) for n in heads) and not any(tpgm_is_head(n) for n in plain)
    assert tpgm_init_gamma("stage1.0.qkv.weight", 1.0) == 3.0 and tpgm_init_gamma("stage1.0.qkv.weight", 1.5) == 3.0
    assert tpgm_init_gamma("stage1.0.qkv.weight", 2.25) == 4.5 and tpgm_init_gamma("stage1.0.qkv.weight", 0.0) == 3.0
    assert tpgm_init_gamma("output.weight", 1.0) == 10.0 and tpgm_init_gamma("output.weight", 2.0) == 10.0 and tpgm_init_gamma("output.weight", 3.0) == 15.0
    # universal_train.py:898-900 with its defaults start 10, frequency 5: epochs 14, 19, 24, ...
    assert [e for e in range(0, 30) if tpgm_due(e, 10, 5)] == [14, 19, 24, 29]
    assert [e for e in range(0, 6) if tpgm_due(e, 2, 1)] == [2, 3, 4, 5] and not tpgm_due(9, 10, 1) and tpgm_due(10, 10, 1)
    assert [e for e in range(0, 9) if tpgm_due(e, 0, 3)] == [2, 5, 8]


def test_ratios_ref_by_hand():
    norms = np.array([2.0, 2.0, 2.0, 2.0, 2.0, 20.0, 0.0, 2.0])
    gamma = np.array([1.0, 2.5, 1e-3, 90.0, 1.0, 170.0, 3.0, 16.0])
    flags = np.array([0, 0, 0, 0, EXCLUDED, HEAD, 0, 0])
    ratio, live, q = ratios_ref(gamma, norms, flags)
    assert np.allclose(ratio, [0.5, 1.0, 0.005, 1.0, 1.0, 1.0, 1.0, 1.0], rtol=1e-8, atol=0)
    assert list(live) == [True, False, False, False, False, False, False, False]
    assert abs(q[3] - 40.0) < 1e-6 and abs(q[5] - 8.5) < 1e-6 and q[6] == 3.0 / 1e-8 and ratio[4] == 1.0 and ratio[6] == 1.0
    assert list(cmax_ref(norms, flags)) == [80, 80, 80, 80, 80, 200, 80, 80]


def _host_case(l1, clip):
    """Ten tensors of 1027 and 16385 + 5 elements in the six ratio cases; gradients scaled so that the clip is live or not."""
    numels = (1027, 16389, 5, 1027, 9, 1027, 1027, 33, 1027, 1027)
    thetas, anchors, gs = tpgm_inputs("host", numels)
    norms = norms_ref(thetas, anchors, l1)
    gamma, flags = case_setup(norms)
    scale = (4000.0 if l1 else 40.0) if clip else 1.0                  # at scale 1 dgamma is some 0.25 per live tensor (l2), 0.005 (l1)
    gs = [[(g * np.float32(scale)).astype(np.float32) for g in step] for step in gs]
    return numels, thetas, anchors, gs, gamma, flags


def _three_updates(wrong, l1, clip, grad_scale=0.5, lr=0.05):
    """Largest |fp32 emulation - float64| / bound over three updates, each from the emulation's own state, for norm, gamma, m, v, the
    new ratio, the gradient norm and the coefficient; and whether the clip was live."""
    numels, thetas, anchors, gs, gamma, flags = _host_case(l1, clip)
    m, v = np.zeros(len(numels), np.float32), np.zeros(len(numels), np.float32)
    worst, clipped = {}, []
    for k in range(3):
        ref = update_ref(thetas, anchors, gs[k], gamma, m, v, flags, l1, grad_scale, k + 1, float(np.float32(lr)))
        norm, gamma, m, v, ratio, sc = update_fp32(thetas, anchors, gs[k], gamma, m, v, flags, l1, grad_scale, k + 1, lr, wrong=wrong)
        clipped.append(ref["coef"][0] < 1.0)
        for name, got in (("norm", norm), ("gamma", gamma), ("m", m), ("v", v), ("ratio", ratio), ("gnorm", sc[0]), ("coef", sc[1])):
            want, bound = ref[name]
            err, bound = np.abs(np.asarray(got, np.float64) - want), np.asarray(bound, np.float64)
            with np.errstate(divide="ignore", invalid="ignore"):
                rel = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
            worst[name] = max(worst.get(name, 0.0), float(np.max(rel)))
    return worst, clipped


@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
@pytest.mark.parametrize("l1", [False, True], ids=["l2", "l1"])
def test_the_bounds_hold_the_fp32_arithmetic(l1, clip):
    worst, clipped = _three_updates(None, l1, clip)
    print("fp32 emulation / bound:", worst, "clip live:", clipped)
    assert all(c == clip for c in clipped)
    assert all(w <= 1.0 for w in worst.values()), worst
    assert worst["norm"] >= 0.005 and worst["gamma"] >= 0.005, worst         # not slack by more than a factor 200


@pytest.mark.parametrize("wrong", WRONG)
def test_the_bounds_reject_the_planted_bugs(wrong):
    """Each bug, emulated in float32, leaves a bound by a factor of at least 4 within three updates with the clip live."""
    worst, clipped = _three_updates(wrong, False, True)
    print(f"{wrong}: emulation / bound: {worst}")
    assert all(clipped)
    assert max(worst["gamma"], worst["m"], worst["v"]) >= 4.0, (wrong, worst)


def test_case_setup_reaches_every_ratio_case():
    numels, thetas, anchors, _, gamma, flags = _host_case(False, True)
    norms = norms_ref(thetas, anchors, False)
    ratio, live, q = ratios_ref(gamma, norms, flags)
    by = {c: [t for t in range(len(numels)) if RATIO_CASES[t % 6] == c] for c in RATIO_CASES}
    assert all(live[t] and 0.25 < ratio[t] < 0.55 for t in by["below"]) and len({round(float(ratio[t]), 2) for t in by["below"]}) == 2
    assert all(not live[t] and ratio[t] == 1 and 1.5 < q[t] < 80 for t in by["one"])
    assert all(not live[t] and 0 < ratio[t] < 0.5 and gamma[t] < GAMMA_MIN for t in by["low"])
    assert all(not live[t] and ratio[t] == 1 and gamma[t] > cmax_ref(norms, flags)[t] for t in by["high"])
    assert all(not live[t] and ratio[t] == 1 and flags[t] == EXCLUDED and q[t] < 1 for t in by["excluded"])
    assert all(not live[t] and ratio[t] == 1 and flags[t] == HEAD and 80 < gamma[t] < 100 for t in by["head"])


def test_stat_depth_and_chunk_sum_transcribe_the_launch_rule():
    assert stat_depth(1, 1) == 12 and stat_depth(16384, 1) == 28 and stat_depth(3 * 16384 + 5, 4) == 31
    x = det_normal("tpgm.depth", (16384,)).astype(np.float32)
    for n in (1, 3, 4, 5, 1023, 1027, 16383, 16384):
        t = x[:n] * x[:n]
        s = float((t.astype(np.float64)).sum())
        assert abs(float(chunk_sum_fp32(t)) - s) <= stat_depth(n, 0) * U * s, n
    ones = np.ones(16384, np.float32)
    assert chunk_sum_fp32(ones) == 16384 and chunk_sum_fp32(ones[:1027]) == 1027 and chunk_sum_fp32(ones[:3]) == 3


def test_flat_tpgm_validates_before_any_device_work():
    from cswin_unet_amd.optim import FlatTPGM

    class Opt:
        params = [torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2))]
    with pytest.raises(ValueError, match="names"):
        FlatTPGM(Opt(), ["a"])
    with pytest.raises(KeyError, match="no trainable parameter"):
        FlatTPGM(Opt(), ["a", "b"], exclude=("c",))
