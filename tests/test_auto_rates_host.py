"""Host side of the per-step rates and of Adam on the flat buffers (csrc/adamw.hip: cswin_rate_finalize, cswin_adam_flat;
optim.FlatAdamW.set_auto_rates; continual.finetune_groups): the float64 references and the derived bounds that
tests/test_gpu_auto_rates.py and tests/test_gpu_auto_rates_step.py use, checked here against torch.optim.Adam on the CPU, against
planted bugs and against the reference's group membership.  No GPU."""
import json
import math
import os
import types

import numpy as np
import pytest
import torch

from test_adamw_host import BETA1, BETA2, EPS, LRS, U, adamw_bound, adamw_inputs, adamw_ref, sumsq_depth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUPLED, FRESH = 1, 2           # cswin_adam_flat's flags
FLAGS = (0, COUPLED, FRESH, COUPLED | FRESH)


# ------------------------------------------------------------------------------------------------
# float64 references
# ------------------------------------------------------------------------------------------------
def members_of(group_of, ngroups):
    """Group k's tensors in tensor order, from the per-tensor group index (-1: none)."""
    return [[t for t, k in enumerate(group_of) if k == g] for g in range(ngroups)]


def group_rates_ref(sumsq_g, sumsq_p, group_of, ngroups, statistic="grad", grad_scale=1.0, default=0.0):
    """(group_stat (G,), lr_mult (T,)) of finetune.py:135-140, 225-236 in float64 from the per-tensor sums of squares: a group's
    statistic is grad_scale * sqrt(sum of its tensors' sum g^2) -- the norm of its concatenated gradient -- and in the "ratio" mode
    that over sqrt(sum of its tensors' sum p^2) where this is > 1e-8, else 0 (universal_train.py:661-690); a tensor's multiplier is
    its group's statistic over the largest one (all 0 when that is <= 0, as continual.rgn_weights has it; a NaN statistic makes
    every grouped multiplier NaN), `default` for a tensor in no group."""
    sumsq_g, sumsq_p = np.asarray(sumsq_g, np.float64), np.asarray(sumsq_p, np.float64)
    stat = np.zeros(ngroups)
    with np.errstate(invalid="ignore", divide="ignore"):
        for k, mem in enumerate(members_of(group_of, ngroups)):
            stat[k] = grad_scale * math.sqrt(sumsq_g[mem].sum()) if not np.isnan(sumsq_g[mem].sum()) else np.nan
            if statistic == "ratio":
                pn = math.sqrt(sumsq_p[mem].sum())
                stat[k] = stat[k] / pn if pn > 1e-8 else 0.0
        top = np.nan if np.isnan(stat).any() else stat.max()
        rate = stat / top if top > 0 else np.full(ngroups, np.nan if np.isnan(top) else 0.0)
    return stat, np.array([default if k < 0 else rate[k] for k in group_of], np.float64)


def one_group_at_one(mult, group_of):
    """Exactly one group's multiplier is 1.0: the grouped tensors whose multiplier is exactly 1 are all the members of one group."""
    group_of = np.asarray(group_of)
    at_one = set(group_of[(np.asarray(mult) == 1.0) & (group_of >= 0)].tolist())
    return len(at_one) == 1 and bool((np.asarray(mult)[group_of == next(iter(at_one))] == 1.0).all())


def group_rates_bound(sumsq_g, sumsq_p, numels, nchunks, group_of, ngroups, statistic="grad", grad_scale=1.0):
    """(bound_stat (G,), bound_mult (T,)): what cswin_rate_finalize may differ by from group_rates_ref, to first order in U, counted
    from the kernel's operations (csrc/adamw.hip, rate_finalize_kernel):

      a tensor's sum of squares    test_adamw_host.sumsq_bound: (sumsq_depth + 2) U relative, every term positive
      a group's sum                its n_k tensors added in order, n_k more additions: (max_t depth_t + 2 + n_k) U =: r U
      sqrt (2) and * grad_scale    r / 2 + 3, what test_adamw_host.norm_bounds takes for the total norm
      ratio                        the second square root r_p / 2 + 2 and the division 2: (r_g + r_p) / 2 + 7
      top                          a maximum moves by no more than its arguments do: max_k bound_stat[k], absolute
      mult = stat_k / top          bound_stat[k] / top + mult * bound_top / top + 2 U mult (the division at two roundings)

    The group whose statistic IS the maximum gets exactly 1 on the device; the bound allows that."""
    stat, _ = group_rates_ref(sumsq_g, sumsq_p, group_of, ngroups, statistic, grad_scale)
    rel = np.zeros(ngroups)
    for k, mem in enumerate(members_of(group_of, ngroups)):
        r = max(sumsq_depth(numels[t], int(nchunks[t])) for t in mem) + 2 + len(mem)
        rel[k] = r / 2 + 3 if statistic == "grad" else r + 7
    bstat = rel * U * np.abs(stat)
    top = stat.max()
    btop = bstat.max()
    bmult = np.zeros(len(group_of))
    if top > 0:
        for t, k in enumerate(group_of):
            if k >= 0:
                mult = stat[k] / top
                bmult[t] = bstat[k] / top + mult * btop / top + 2 * U * mult
    return bstat, bmult


def adam_ref(p, g, m, v, step, lr, wd=1e-4, grad_scale=1.0, clip=1.0, mult=1.0, coupled=True, fresh=False):
    """One step in numpy float64, (p, m, v).  coupled: torch.optim.Adam, whose weight decay is grad.add(param, alpha=wd) and
    nothing else; not coupled: torch.optim.AdamW (test_adamw_host.adamw_ref).  fresh: the first step of an optimiser built for
    this step alone (finetune.py:237) -- zero moments, step 1 -- whatever m, v and step are; they come back unchanged."""
    p64, g64 = np.asarray(p, np.float64), np.asarray(g, np.float64)
    m_in, v_in, step_in = (np.zeros_like(p64), np.zeros_like(p64), 1) if fresh else (m, v, step)
    if coupled:
        out = adamw_ref(p64, g64 * (grad_scale * clip) + wd * p64, m_in, v_in, step_in, lr, wd=0.0, mult=mult)
    else:
        out = adamw_ref(p64, g64, m_in, v_in, step_in, lr, wd=wd, grad_scale=grad_scale, clip=clip, mult=mult)
    return (out[0], np.asarray(m, np.float64), np.asarray(v, np.float64)) if fresh else out


def adam_bound(p, g, m, v, step, lr, wd=1e-4, grad_scale=1.0, clip=1.0, mult=1.0, coupled=True, fresh=False):
    """(bound_p, bound_m, bound_v) of one step of cswin_adam_flat against adam_ref from the same state.  Not coupled: the operations
    are cswin_adamw_flat's, so the bound is test_adamw_host.adamw_bound (from zero moments at step 1 when fresh).  Coupled, the
    gradient that enters the moments is a difference-prone sum, so its error is carried as an absolute one through the same chain
    (adam_elem and adam_quotient, every operation at one rounding, sqrt and the divisions at two, no contraction relied on):

      g' = fma(wd, p, g * gsc)     e_g = 3U A_g, A_g = |g gsc| + |wd p|: gsc and its product 2U |g gsc|, the rounded wd U |wd p|, the
                                   fma U |g'|, and one more U |wd p| should the product be rounded on its own
      m  = fma(b1, m, omb1 g')     e_m = 3U A_m + omb1 e_g, A_m = |b1 m| + |omb1 g'|: the two rounded constants, the product, the fma
      v  = fma(b2, v, omb2 g'^2)   e_v = U b2 v + omb2 (3U g'^2 + 2 |g'| e_g + e_g^2) + U v
      s  = sqrt(v)                 e_s = min(e_v / (2 sqrt v), sqrt e_v) + 2U s   (|sqrt a - sqrt b| <= sqrt |a - b| where v is 0)
      dn = fma(s, isb2, eps)       e_dn = isb2' e_s + 3U dn  (isb2' = 1 / sqrt(bc2))
      q  = m / dn                  e_q = e_m / dn + A_m e_dn / dn^2 + 2U A_m / dn
      d  = st q, st = lr_t / bc1   e_d = st e_q + 5U st A_m / dn   (st carries 4 as in adamw_bound, the product 1)
      p  = p - d                   e_p = e_d + U (|p| + st A_m / dn)

    m and v are neither read nor written when fresh: their bounds are 0."""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    if fresh:
        m, v, step = np.zeros_like(p), np.zeros_like(p), 1
    if not coupled:
        bp, bm, bv = adamw_bound(p, g, m, v, step, lr, wd=wd, grad_scale=grad_scale, clip=clip, mult=mult)
    else:
        gs = g * (grad_scale * clip)
        gq = gs + wd * p
        eg = 3 * U * (np.abs(gs) + np.abs(wd * p))
        Am = np.abs(BETA1 * m) + np.abs((1 - BETA1) * gq)
        em = 3 * U * Am + (1 - BETA1) * eg
        Av = BETA2 * v + (1 - BETA2) * gq * gq
        ev = U * BETA2 * v + (1 - BETA2) * (3 * U * gq * gq + 2 * np.abs(gq) * eg + eg * eg) + U * Av
        s = np.sqrt(Av)
        with np.errstate(divide="ignore", invalid="ignore"):
            es = np.minimum(np.where(s > 0, ev / (2 * s), np.inf), np.sqrt(ev)) + 2 * U * s
        bc1, bc2 = 1 - BETA1 ** step, 1 - BETA2 ** step
        isb2 = 1 / math.sqrt(bc2)
        dn = s * isb2 + EPS
        edn = isb2 * es + 3 * U * dn
        eq = em / dn + Am * edn / dn ** 2 + 2 * U * Am / dn
        st = np.abs(lr * np.asarray(mult, np.float64)) / bc1
        ed = st * eq + 5 * U * st * Am / dn
        bp, bm, bv = ed + U * (np.abs(p) + st * Am / dn), em, ev
    return (bp, np.zeros_like(p), np.zeros_like(p)) if fresh else (bp, bm, bv)


# ------------------------------------------------------------------------------------------------
# the kernels' arithmetic in numpy float32, with the bugs the bounds must see
# ------------------------------------------------------------------------------------------------
def rates_fp32(sumsq_g, sumsq_p, group_of, ngroups, statistic, grad_scale, default, wrong=None):
    """rate_finalize_kernel's second half on float32 per-tensor sums: (group_stat, lr_mult)."""
    f = np.float32
    sumsq_g, sumsq_p = np.asarray(sumsq_g, f), np.asarray(sumsq_p, f)
    stat = np.zeros(ngroups, f)
    for k, mem in enumerate(members_of(group_of, ngroups)):
        sg, sp = f(0), f(0)
        for t in mem:
            sg, sp = f(sg + sumsq_g[t]), f(sp + sumsq_p[t])
        s = f(f(grad_scale) * np.sqrt(sg))
        if wrong == "sum_of_tensor_norms":
            s = f(0)
            for t in mem:
                s = f(s + f(grad_scale) * np.sqrt(sumsq_g[t]))
        if statistic == "ratio":
            pn = np.sqrt(sp)
            s = f(s / pn) if pn > f(1e-8) else f(0)
            if wrong == "ratio_per_tensor":
                s = f(0)
                for t in mem:
                    pt = np.sqrt(sumsq_p[t])
                    s = f(s + (f(grad_scale) * np.sqrt(sumsq_g[t]) / pt if pt > f(1e-8) else f(0)))
        stat[k] = s
    top = f(-np.inf)
    for s in stat:
        if top == top and not s <= top:
            top = s
    if wrong == "normalise_by_sum":
        top = stat.sum(dtype=f)
    with np.errstate(invalid="ignore"):
        rate = (stat / top).astype(f) if top > 0 else np.full(ngroups, f(0) if top == top else top, f)
    return stat, np.array([f(default) if k < 0 else rate[k] for k in group_of], f)


def adam_fp32(p, g, m, v, step, lr, wd, grad_scale, clip, mult, flags, wrong=None):
    """adam_flat_kernel's arithmetic (no contraction), the bias corrections formed as optim.FlatAdamW.apply forms them."""
    f = np.float32
    p, g, m, v = (np.asarray(a, f) for a in (p, g, m, v))
    coupled, fresh = bool(flags & COUPLED), bool(flags & FRESH)
    m_in, v_in = (np.zeros_like(p), np.zeros_like(p)) if fresh else (m, v)
    t = step if (not fresh or wrong == "step_t_corrections_when_fresh") else 1
    b1, omb1, b2, omb2, eps = f(BETA1), f(1 - BETA1), f(BETA2), f(1 - BETA2), f(EPS)
    bc1, isb2 = f(1 - BETA1 ** t), f(1.0 / math.sqrt(1 - BETA2 ** t))
    lr_t = f(lr) * np.asarray(mult, f)
    gq = g * (f(grad_scale) * f(clip))
    decoupled_decay = not coupled or wrong == "decoupled_decay_when_coupled"
    if not decoupled_decay:
        gq = f(wd) * p + gq
    mo = b1 * m_in + omb1 * gq
    vo = b2 * v_in + omb2 * (gq * gq)
    q = mo / (np.sqrt(vo) * isb2 + eps)
    decay = f(1) - lr_t * f(wd) if decoupled_decay else f(1)
    out = (p * decay - (lr_t / bc1) * q).astype(f)
    return (out, m, v) if fresh else (out, mo.astype(f), vo.astype(f))


ADAM_WRONG = (("decoupled_decay_when_coupled", COUPLED), ("decoupled_decay_when_coupled", COUPLED | FRESH),
              ("step_t_corrections_when_fresh", FRESH), ("step_t_corrections_when_fresh", COUPLED | FRESH))
RATES_WRONG = (("sum_of_tensor_norms", "grad"), ("normalise_by_sum", "grad"), ("normalise_by_sum", "ratio"), ("ratio_per_tensor", "ratio"))


def _adam_three_steps(flags, wrong, wd=1e-2):
    """Largest |fp32 emulation - adam_ref| / bound of p over three steps on a 1027-element tensor, each from the emulation's state."""
    ps, gs = adamw_inputs("auto.host", (1027,), norm=3.0)
    p, m, v = ps[0], np.zeros(1027, np.float32), np.zeros(1027, np.float32)
    worst = 0.0
    for k in range(3):
        lr = float(np.float32(LRS[k]))
        kw = dict(wd=wd, grad_scale=0.5, clip=0.75, mult=0.37)
        mode = dict(coupled=bool(flags & COUPLED), fresh=bool(flags & FRESH))
        ref = adam_ref(p, gs[k][0], m, v, k + 1, lr, **kw, **mode)
        bound = adam_bound(p, gs[k][0], m, v, k + 1, lr, **kw, **mode)
        p, m, v = adam_fp32(p, gs[k][0], m, v, k + 1, LRS[k], flags=flags, wrong=wrong, **kw)
        for got, want, b in zip((p, m, v), ref, bound):
            err = np.abs(got.astype(np.float64) - want)
            assert wrong or (err <= b).all(), (flags, k)
        worst = max(worst, float((np.abs(p.astype(np.float64) - ref[0]) / bound[0]).max()))
    return worst


def _rates_case(statistic):
    """Seven tensors in three interleaved groups and one in none; float32 per-tensor sums as a kernel would hand them over."""
    numels = (5, 1027, 9, 300, 16385, 4, 77, 12)
    group_of = [0, 1, 2, 0, 1, -1, 2, 0]
    ps, gs = adamw_inputs("auto.rates", numels)
    sg = np.array([float((a.astype(np.float64) ** 2).sum()) for a in gs[0]])
    sp = np.array([float((a.astype(np.float64) ** 2).sum()) for a in ps])
    return numels, group_of, sg, sp


# ------------------------------------------------------------------------------------------------
# tests
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fresh", [False, True], ids=["kept", "fresh"])
@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_adam_ref_agrees_with_torch_adam(wd, fresh):
    """adam_ref(coupled=True) against torch.optim.Adam(weight_decay, foreach=False) on CPU float64 tensors, three steps, one
    parameter group per tensor with a rate of its own; fresh: the optimiser is built anew for every step, as finetune.py:237
    does.  1e-12 relative."""
    numels, mults = (5, 1027, 9), (1.0, 0.37, 0.0)
    ps, gs = adamw_inputs("auto.torch", numels, norm=3.0)
    leaves = [torch.from_numpy(a).double().requires_grad_() for a in ps]
    build = lambda: torch.optim.Adam([{"params": [l], "lr": 1.0} for l in leaves], betas=(BETA1, BETA2), eps=EPS, weight_decay=wd, foreach=False)
    opt = build()
    state = [(a.astype(np.float64), np.zeros(a.size), np.zeros(a.size)) for a in ps]
    for k in range(3):
        if fresh:
            opt = build()
        for grp, mu in zip(opt.param_groups, mults):
            grp["lr"] = LRS[k] * mu
        for l, g in zip(leaves, gs[k]):
            l.grad = torch.from_numpy(g).double()
        opt.step()
        state = [adam_ref(p, g, m, v, k + 1, LRS[k], wd=wd, mult=mu, coupled=True, fresh=fresh) for (p, m, v), g, mu in zip(state, gs[k], mults)]
        for l, (p, m, v) in zip(leaves, state):
            assert np.abs(l.detach().numpy() - p).max() <= 1e-12 * np.abs(p).max(), k
            if not fresh:
                st = opt.state[l]
                assert np.abs(st["exp_avg"].numpy() - m).max() <= 1e-12 * np.abs(m).max() and np.abs(st["exp_avg_sq"].numpy() - v).max() <= 1e-12 * np.abs(v).max()
    assert np.array_equal(state[2][0], ps[2].astype(np.float64))          # rate 0: nothing moves, the coupled decay included
    if fresh:
        assert all((m == 0).all() and (v == 0).all() for _, m, v in state)


def test_adam_ref_uncoupled_is_adamw_ref():
    ps, gs = adamw_inputs("auto.same", (1027,), norm=3.0)
    m, v = np.abs(gs[1][0]) * 0.1, gs[2][0].astype(np.float64) ** 2
    a = adam_ref(ps[0], gs[0][0], m, v, 3, 0.01, wd=0.01, grad_scale=0.5, clip=0.7, mult=0.37, coupled=False)
    b = adamw_ref(ps[0], gs[0][0], m, v, 3, 0.01, wd=0.01, grad_scale=0.5, clip=0.7, mult=0.37)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("flags", FLAGS)
def test_the_adam_bound_holds_the_fp32_arithmetic(flags):
    """The kernel's arithmetic emulated in numpy float32 stays inside the bound in every mode, and the bound is not slack."""
    worst = _adam_three_steps(flags, None)
    print(f"flags {flags}: fp32 emulation / bound of p: {worst}")
    assert 0.02 <= worst <= 1.0, worst


@pytest.mark.parametrize("wrong,flags", ADAM_WRONG)
def test_the_adam_bound_rejects_the_wrong_variants(wrong, flags):
    """AdamW's decoupled decay where Adam's coupled one is asked for, and the step's own bias corrections where a fresh optimiser
    has those of step 1: each leaves the bound of p by a factor of at least 4 within three steps."""
    worst = _adam_three_steps(flags, wrong)
    print(f"{wrong}, flags {flags}: emulation / bound of p: {worst}")
    assert worst >= 4.0, (wrong, flags, worst)


@pytest.mark.parametrize("statistic", ["grad", "ratio"])
def test_the_rates_bound_holds_the_fp32_arithmetic(statistic):
    numels, group_of, sg, sp = _rates_case(statistic)
    nchunks = [-(-n // 16384) for n in numels]
    want_stat, want_mult = group_rates_ref(sg, sp, group_of, 3, statistic, 0.5, 0.25)
    bstat, bmult = group_rates_bound(sg, sp, numels, nchunks, group_of, 3, statistic, 0.5)
    stat, mult = rates_fp32(sg, sp, group_of, 3, statistic, 0.5, 0.25)
    assert (np.abs(stat - want_stat) <= bstat).all() and (np.abs(mult - want_mult) <= bmult).all()
    assert one_group_at_one(mult, group_of) and mult[5] == 0.25 and want_mult[5] == 0.25 and bmult[5] == 0.0
    assert want_mult.max() == 1.0 and (want_mult[np.array(group_of) >= 0] > 0).all()


@pytest.mark.parametrize("wrong,statistic", RATES_WRONG)
def test_the_rates_bound_rejects_the_wrong_variants(wrong, statistic):
    """The sum of the tensors' norms instead of the norm of the group's gradient, the sum instead of the maximum as the divisor,
    and the ratio formed per tensor and added up: each leaves the multipliers' bound by a factor of at least 4."""
    numels, group_of, sg, sp = _rates_case(statistic)
    nchunks = [-(-n // 16384) for n in numels]
    _, want_mult = group_rates_ref(sg, sp, group_of, 3, statistic, 0.5, 0.25)
    _, bmult = group_rates_bound(sg, sp, numels, nchunks, group_of, 3, statistic, 0.5)
    _, mult = rates_fp32(sg, sp, group_of, 3, statistic, 0.5, 0.25, wrong=wrong)
    grouped = np.array(group_of) >= 0
    worst = float((np.abs(mult - want_mult)[grouped] / bmult[grouped]).max())
    print(f"{wrong}, {statistic}: emulation / bound: {worst}")
    assert worst >= 4.0, (wrong, worst)


def test_group_rates_ref_edge_cases():
    """A zero gradient gives multipliers 0 (continual.rgn_weights' rule), a NaN gives NaN in every group, a group without parameter
    norm has ratio 0, and one group per tensor in the ratio mode is rgn_weights itself."""
    from cswin_unet_amd.continual import rgn_weights
    group_of = [0, 1, -1, 0]
    stat, mult = group_rates_ref(np.zeros(4), np.ones(4), group_of, 2, "grad", 1.0, 0.5)
    assert (stat == 0).all() and mult.tolist() == [0.0, 0.0, 0.5, 0.0]
    stat, mult = group_rates_ref([1.0, np.nan, 1.0, 1.0], np.ones(4), group_of, 2, "grad", 1.0, 0.5)
    assert np.isnan(mult[[0, 1, 3]]).all() and mult[2] == 0.5
    stat, mult = group_rates_ref([1.0, 4.0, 1.0, 1.0], [0.0, 4.0, 1.0, 0.0], group_of, 2, "ratio", 1.0, 0.5)
    assert stat.tolist() == [0.0, 1.0] and mult.tolist() == [0.0, 1.0, 0.5, 0.0]
    names = ["a.weight", "b.weight", "c.bias", "d.weight"]
    rs = np.random.RandomState(5)
    sg, sp = rs.rand(4) + 0.1, rs.rand(4) + 0.1
    _, mult = group_rates_ref(sg, sp, [0, 1, 2, 3], 4, "ratio")
    want = rgn_weights(names, [np.sqrt(np.stack([sg, sp], 1))])
    assert all(abs(mult[i] - want[n]) <= 1e-15 for i, n in enumerate(names))


def test_group_table_is_a_csr_list_in_tensor_order():
    from cswin_unet_amd.optim import group_table
    first, tensors, group_of, names = group_table(["b", None, "a", "b", "a", "b"], 6)
    assert names == ["b", "a"] and first.tolist() == [0, 3, 5] and tensors.tolist() == [0, 3, 5, 2, 4] and group_of.tolist() == [0, -1, 1, 0, 1, 0]
    assert all(a.dtype == np.int32 for a in (first, tensors, group_of))
    first, tensors, group_of, names = group_table(list(range(463)), 463, "ratio")
    assert first.tolist() == list(range(464)) and tensors.tolist() == list(range(463)) == group_of.tolist()


def test_finetune_groups_are_the_references():
    """continual.finetune_groups on the tiny config against the membership recorded from finetune.py's get_parameter_groups
    (tools/make_finetune_groups.py): the 22 groups in order, every one of the 463 parameters in exactly one of them."""
    from cswin_unet_amd.config import get_config
    from cswin_unet_amd.continual import FINETUNE_GRID, finetune_groups
    from cswin_unet_amd.networks.vision_transformer import CSwinUnet
    with open(os.path.join(ROOT, "tests", "golden", "g11_finetune_groups.json")) as f:
        want = json.load(f)["groups"]
    model = CSwinUnet(get_config(os.path.join(ROOT, "configs", "cswin_tiny_224_lite.yaml")), img_size=224, num_classes=9)
    got = finetune_groups(model)
    assert list(got) == list(want) and len(got) == 22
    assert got == want
    named = [n for v in got.values() for n in v]
    assert len(named) == 463 == len(set(named)) and set(named) == set(n for n, _ in model.named_parameters())
    core = finetune_groups(model.cswin_unet)                              # the core network: the same groups without the wrapper's prefix
    assert {g: ["cswin_unet." + n for n in v] for g, v in core.items()} == got
    assert FINETUNE_GRID == ((1e-3, 1e-4), (1e-4, 1e-4), (1e-5, 1e-4))


def test_options_are_validated_before_any_device_work():
    from cswin_unet_amd.optim import FlatAdamW, group_table
    from cswin_unet_amd.trainer import DataParallelTrainer, HipEngine, surgical_trainer, trainer_synapse
    net = torch.nn.Linear(4, 4)
    with pytest.raises(ValueError, match="statistic"):
        group_table([0, 1], 2, "rgn")
    with pytest.raises(ValueError, match="3 group entries for 2"):
        group_table([0, 1, 0], 2)
    with pytest.raises(ValueError, match="no tensor"):
        group_table([None, None], 2)
    with pytest.raises(ValueError, match="moments"):
        FlatAdamW([torch.nn.Parameter(torch.zeros(3))], lr=1e-3, moments="new")
    with pytest.raises(ValueError, match="moments"):
        HipEngine(net, 9, 0.05, 0.9, 1e-4, 0.4, 0.6, optimizer="adam", moments="new")
    with pytest.raises(ValueError, match="moments"):
        HipEngine(net, 9, 0.05, 0.9, 1e-4, 0.4, 0.6, optimizer="sgd", moments="fresh")
    with pytest.raises(ValueError, match="moments"):
        DataParallelTrainer(net, 9, optimizer="adamw", moments="new")
    with pytest.raises(RuntimeError, match="FlatAdamW"):                  # valid options: it gets as far as the CPU parameters
        HipEngine(net, 9, 0.05, 0.9, 1e-4, 0.2, 0.8, optimizer="adam", moments="fresh")
    sgd_engine = types.SimpleNamespace(opt=object(), param_names=["weight", "bias"])
    with pytest.raises(ValueError, match="set_auto_rates needs optimizer"):
        HipEngine.set_auto_rates(sgd_engine, "tensors")
    args = types.SimpleNamespace(optimizer="sgd", auto_rates="grad")
    with pytest.raises(ValueError, match="auto_rates needs optimizer"):
        trainer_synapse(args, net, "/nonexistent/never/created")
    for bad in (dict(auto_rates="rgn", optimizer="adam"), dict(moments="new", optimizer="adam"), dict(optimizer="adamax"),
                dict(subset_fraction=0.0), dict(lr_schedule="cosine")):
        with pytest.raises(ValueError, match=next(iter(bad))):
            trainer_synapse(types.SimpleNamespace(**bad), net, "/nonexistent/never/created")
    with pytest.raises(ValueError, match="auto_rates"):
        surgical_trainer(types.SimpleNamespace(base_lr=1e-3, auto_rates="rgn"), net, "/nonexistent/never/created")
    assert not os.path.exists("/nonexistent")


def test_engine_group_arguments_are_checked_by_name():
    """HipEngine.set_auto_rates turns {group: [names]} into one id per tensor: unknown names are a KeyError as in set_lr_weights, a
    name in two groups and an empty group a ValueError, and a tensor that is not named is in no group."""
    from cswin_unet_amd.trainer import HipEngine
    seen = {}
    opt = types.SimpleNamespace(set_auto_rates=lambda *a: seen.update(args=a))
    eng = types.SimpleNamespace(opt=opt, param_names=["a.weight", "a.bias", "b.weight", "c.weight"])
    HipEngine.set_auto_rates(eng, {"A": ["a.bias", "a.weight"], "C": ["c.weight"]}, "ratio", 0.5)
    assert seen["args"] == (["A", "A", None, "C"], "ratio", 0.5)
    HipEngine.set_auto_rates(eng, "tensors")
    assert seen["args"] == ([0, 1, 2, 3], "grad", 0.0)
    HipEngine.set_auto_rates(eng, None)
    assert seen["args"] == (None,)
    with pytest.raises(KeyError, match="z.weight"):
        HipEngine.set_auto_rates(eng, {"A": ["z.weight"]})
    with pytest.raises(ValueError, match="more than one"):
        HipEngine.set_auto_rates(eng, {"A": ["a.bias"], "B": ["a.bias"]})
    with pytest.raises(ValueError, match="no parameter"):
        HipEngine.set_auto_rates(eng, {"A": ["a.bias"], "B": []})
    with pytest.raises(ValueError, match="tensors"):
        HipEngine.set_auto_rates(eng, "layers")
