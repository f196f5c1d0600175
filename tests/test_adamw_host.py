"""Host side of the AdamW step (csrc/adamw.hip, optim.FlatAdamW, continual.rgn_weights): the float64 references and the derived
bounds that tests/test_gpu_adamw.py and tests/test_gpu_adamw_step.py use, checked here against torch on the CPU, against planted
bugs and against a literal transcription of the reference's RGN arithmetic.  No GPU."""
import math
from collections import defaultdict

import numpy as np
import pytest
import torch

from oracle.determ import det_normal

U = 2.0 ** -24                  # unit roundoff of fp32
CHUNK = 16384
LRS = (0.05, 0.02, 0.007)       # SGD_LRS of tests/test_gpu_step_tail.py
BETA1, BETA2, EPS = 0.9, 0.999, 1e-8


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------
# float64 references
# ------------------------------------------------------------------------------------------------
def clip_ref(grads, grad_scale, max_norm):
    """(per-tensor sum g^2, total_norm, clip_coef) of torch.nn.utils.clip_grad_norm_ applied to the tensors g * grad_scale."""
    sumsq = np.array([float((np.asarray(g, np.float64) ** 2).sum()) for g in grads])
    with np.errstate(invalid="ignore", over="ignore"):
        total = float(grad_scale * np.sqrt(sumsq.sum()))
        coef = max_norm / (total + 1e-6)
    return sumsq, total, (1.0 if coef > 1.0 else coef)


def adamw_ref(p, g, m, v, step, lr, beta1=BETA1, beta2=BETA2, eps=EPS, wd=0.01, grad_scale=1.0, clip=1.0, mult=1.0):
    """One torch.optim.AdamW step in numpy float64, element by element: (p, m, v) after step number `step` (1-based).  clip: the
    clipping coefficient (1: none); mult: the learning-rate multiplier, a scalar or an array that broadcasts against p."""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    gq = g * (grad_scale * clip)
    m = beta1 * m + (1 - beta1) * gq
    v = beta2 * v + (1 - beta2) * gq * gq
    bc1, bc2 = 1 - beta1 ** step, 1 - beta2 ** step
    lr_t = lr * np.asarray(mult, np.float64)
    p = p * (1 - lr_t * wd)
    p = p - (lr_t / bc1) * m / (np.sqrt(v) / math.sqrt(bc2) + eps)
    return p, m, v


def adamw_bound(p, g, m, v, step, lr, beta1=BETA1, beta2=BETA2, eps=EPS, wd=0.01, grad_scale=1.0, clip=1.0, mult=1.0):
    """(bound_p, bound_m, bound_v): what one step of the fp32 kernel may differ by from adamw_ref started from the same state, to
    first order in U = 2^-24, from the magnitudes involved.  Counted from adamw_elem and its kernel (csrc/adamw.hip), every
    operation at one rounding except sqrt and the division, taken at two (1 ulp), and without relying on contraction:

      g' = g * gsc, gsc = fl(grad_scale * clip_coef)                      2 roundings: |dg'| <= 2U |g'|
      m  = fma(b1, m, omb1 * g'): b1 and omb1 are rounded constants       U |b1 m| + (1 + 2 + 1) U |omb1 g'| + U |m|  <= 5U A_m,
                                                                          A_m = |b1 m_prev| + |(1 - b1) g'|  (>= |m|: cancellation is covered)
      v  = fma(b2, v, omb2 * (g' g')): g'^2 carries 2 * 2 + 1             U b2 v + (5 + 1 + 1) U omb2 g'^2 + U v  <= 8U v
      s  = sqrt(v)                                                        8/2 + 2 = 6
      dn = fma(s, inv_sqrt_bc2, eps): the two constants, one rounding     6 + 1 + 1 + 1 = 9 (both terms positive)
      st = lr_t / fl(bc1), lr_t = fl(lr * mult)                           1 + 1 + 2 = 4; the quotient m / dn 5 + 9 + 2 = 16;
      d  = st * (m / dn)                                                  4 + 16 + 1 = 21, relative to delta = st A_m / dn
      dc = 1 - lr_t * wd: wd a rounded constant                           (1 + 1 + 1) U |lr_t wd| + U; dc = 1 exactly when wd = 0
      p  = p * dc - d                                                     p * dc: (1 + 3 |lr_t wd|) U |p| + U |p|; the difference U (|p| + delta)

    so |dp| <= a U |p| + b U delta with a = 3 + 3 |lr_t wd| (1 when wd = 0) and b = 22; |dm| <= 5U A_m; |dv| <= 8U v."""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    gq = g * (grad_scale * clip)
    Am = np.abs(beta1 * m) + np.abs((1 - beta1) * gq)
    Av = beta2 * v + (1 - beta2) * gq * gq
    bc1, bc2 = 1 - beta1 ** step, 1 - beta2 ** step
    lr_t = np.abs(lr * np.asarray(mult, np.float64))
    delta = (lr_t / bc1) * Am / (np.sqrt(Av) / math.sqrt(bc2) + eps)
    a = (3.0 + 3.0 * lr_t * wd) if wd else 1.0
    return U * (a * np.abs(p) + 22.0 * delta), 5.0 * U * Am, 8.0 * U * Av


def sumsq_depth(numel, nchunks=0, ntensors=0):
    """Additions a term of a sum of squares passes through, a transcription of the launch rule (it MUST FOLLOW csrc/flat_chunks.h): a
    chunk is at most 16384 elements under one 256-thread workgroup, so a thread takes cdiv(n / 4, 256) trips of four elements,
    adds its four lanes in 2 levels and a tail element in 1, then the 8 levels of the workgroup tree (6 in the wave, 2 over the
    four waves); a tensor's `nchunks` partials are added in chunk order and the `ntensors` tensor sums in tensor order."""
    n = min(numel, CHUNK)
    return cdiv(n // 4, 256) + 2 + 1 + 8 + nchunks + ntensors


def sumsq_bound(sumsq, numel, nchunks=0, ntensors=0):
    """(reduction depth + 2) U relative: the square itself and one spare beside the depth (every term is positive)."""
    return (sumsq_depth(numel, nchunks, ntensors) + 2) * U * np.abs(sumsq)


def norm_bounds(total, coef, max_numel, max_chunks, ntensors):
    """Bounds of total_norm = grad_scale * sqrt(sum) (half the sum's relative bound, the sqrt at 2, the product 1) and of
    clip_coef = max_norm / (total_norm + 1e-6) (the sum 1, the division 2) -- 0 where the coefficient is clamped to exactly 1
    on both sides."""
    rel = (sumsq_depth(max_numel, max_chunks, ntensors) + 2) / 2 + 3
    return rel * U * abs(total), (rel + 3) * U * abs(coef)


# ------------------------------------------------------------------------------------------------
# layouts and inputs shared with the GPU tests
# ------------------------------------------------------------------------------------------------
LAYOUT = (1, 3, 4, 5, 1023, 1027, 16383, 16384, 16385, 3 * 16384 + 5)


def slots(numels):
    """(offsets, total) of optim's layout: 8-float slots."""
    offs, off = [], 0
    for n in numels:
        offs.append(off)
        off += (n + 7) // 8 * 8
    return offs, off


def adamw_inputs(tag, numels, norm=None):
    """Per-tensor float32 (p, [g0, g1, g2]) of a layout.  A quarter of the gradient elements each are scaled by 1, 1e-2, 1e-4 and
    1e-6, so that sqrt(v) comes near eps for some (where eps inside the square root would show).  norm: the three gradients are
    rescaled to this global norm."""
    ps = [det_normal(f"adamw.{tag}.p{t}", (n,)) for t, n in enumerate(numels)]
    gs = []
    for k in range(3):
        g = [det_normal(f"adamw.{tag}.g{k}.{t}", (n,)) for t, n in enumerate(numels)]
        pos = 0
        for a in g:
            a *= (10.0 ** (-2.0 * ((np.arange(pos, pos + a.size) + k) % 4))).astype(np.float32)
            pos += a.size
        if norm is not None:
            s = norm / math.sqrt(sum(float((a.astype(np.float64) ** 2).sum()) for a in g))
            g = [(a * s).astype(np.float32) for a in g]
        gs.append(g)
    return ps, gs


def flat(arrays, numels, fill=0.0):
    """The flat float32 buffer of per-tensor arrays, pad words = fill."""
    offs, total = slots(numels)
    out = np.full(total, fill, np.float32)
    for a, o in zip(arrays, offs):
        out[o:o + a.size] = a
    return out


def elem_mask(numels):
    """True at the elements of the flat buffer that belong to a tensor."""
    offs, total = slots(numels)
    mask = np.zeros(total, bool)
    for n, o in zip(numels, offs):
        mask[o:o + n] = True
    return mask


def per_elem(values, numels):
    """A per-tensor value spread over the flat buffer (pads: 1)."""
    offs, total = slots(numels)
    out = np.ones(total, np.float64)
    for x, n, o in zip(values, numels, offs):
        out[o:o + n] = x
    return out


# ------------------------------------------------------------------------------------------------
# the kernel's arithmetic in numpy float32, with the bugs the bound must see
# ------------------------------------------------------------------------------------------------
def adamw_fp32(p, g, m, v, step, lr, wd, grad_scale, clip, mult, wrong=None):
    f = np.float32
    p, g, m, v = (np.asarray(a, f) for a in (p, g, m, v))
    b1, omb1, b2, omb2, eps = f(BETA1), f(1 - BETA1), f(BETA2), f(1 - BETA2), f(EPS)
    bc1, bc2 = (f(1), 1.0) if wrong == "no_bias_correction" else (f(1 - BETA1 ** step), 1 - BETA2 ** step)
    isb2 = f(1.0 / math.sqrt(bc2))
    lr_t = f(lr) * np.asarray(mult, f)
    gsc = f(grad_scale) * (f(1) if wrong == "clip_after_moments" else f(clip))
    gq = g * gsc
    if wrong == "l2_in_gradient":
        gq = gq + f(wd) * p
    m = b1 * m + omb1 * gq
    v = b2 * v + omb2 * (gq * gq)
    if wrong == "eps_inside_sqrt":
        denom = np.sqrt(v * (isb2 * isb2) + eps)
    else:
        denom = np.sqrt(v) * isb2 + eps
    q = m / denom
    if wrong == "clip_after_moments":
        q = q * f(clip)
    decay = f(1) if wrong == "l2_in_gradient" else f(1) - lr_t * f(wd)
    return (p * decay - (lr_t / bc1) * q).astype(f), m.astype(f), v.astype(f)


WRONG = ("no_bias_correction", "l2_in_gradient", "eps_inside_sqrt", "clip_after_moments")


def _three_steps(wrong, norm):
    """Largest |fp32 emulation - adamw_ref| / bound over three steps on a 1027-element tensor, each step from the emulation's own
    state: for p, m and v."""
    numels = (1027,)
    ps, gs = adamw_inputs("host", numels, norm=norm)
    p, m, v = ps[0], np.zeros(1027, np.float32), np.zeros(1027, np.float32)
    worst = np.zeros(3)
    for k in range(3):
        g = gs[k][0]
        _, _, coef = clip_ref([g], 1.0, 1.0)
        kw = dict(wd=0.01, grad_scale=1.0, clip=float(np.float32(coef)), mult=1.0)
        ref = adamw_ref(p, g, m, v, k + 1, float(np.float32(LRS[k])), **kw)
        bound = adamw_bound(p, g, m, v, k + 1, float(np.float32(LRS[k])), **kw)
        p, m, v = adamw_fp32(p, g, m, v, k + 1, LRS[k], wrong=wrong, **kw)
        for j, (got, want, b) in enumerate(zip((p, m, v), ref, bound)):
            worst[j] = max(worst[j], float((np.abs(got.astype(np.float64) - want) / b).max()))
    return worst


# ------------------------------------------------------------------------------------------------
# tests
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_norm", [None, 1.0])
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_adamw_ref_agrees_with_torch_adamw_and_clip_grad_norm(wd, max_norm):
    """adamw_ref + clip_ref against torch.optim.AdamW(foreach=False) after clip_grad_norm_ on CPU float64 tensors, three steps
    with the rate changed between them and one parameter group per tensor for the multipliers: 1e-12 relative."""
    numels, mults, gs_scale = (5, 1027, 9), (1.0, 0.37, 0.0), 0.125
    ps, gs = adamw_inputs("torch", numels, norm=40.0 / gs_scale)
    leaves = [torch.from_numpy(a).double().requires_grad_() for a in ps]
    opt = torch.optim.AdamW([{"params": [l], "lr": 1.0} for l in leaves], lr=1.0, betas=(BETA1, BETA2), eps=EPS, weight_decay=wd, foreach=False)
    state = [(a.astype(np.float64), np.zeros(a.size), np.zeros(a.size)) for a in ps]
    for k in range(3):
        for grp, mu in zip(opt.param_groups, mults):
            grp["lr"] = LRS[k] * mu
        for l, g in zip(leaves, gs[k]):
            l.grad = torch.from_numpy(g).double() * gs_scale
        coef = 1.0
        if max_norm is not None:
            total = float(torch.nn.utils.clip_grad_norm_(leaves, max_norm))
            _, want_total, coef = clip_ref(gs[k], gs_scale, max_norm)
            assert abs(total - want_total) <= 1e-12 * total and abs(total - 40.0) < 1e-3 and coef < 0.03
        opt.step()
        state = [adamw_ref(p, g, m, v, k + 1, LRS[k], wd=wd, grad_scale=gs_scale, clip=coef, mult=mu)
                 for (p, m, v), g, mu in zip(state, gs[k], mults)]
        for l, (p, m, v) in zip(leaves, state):
            st = opt.state[l]
            for got, want in ((l.detach().numpy(), p), (st["exp_avg"].numpy(), m), (st["exp_avg_sq"].numpy(), v)):
                assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), k
    assert np.array_equal(state[2][0], ps[2].astype(np.float64))      # multiplier 0: neither the update nor the decay moves p


def test_clip_ref_follows_torch_on_non_finite_gradients():
    g = [np.array([1.0, np.inf, 2.0], np.float32), np.array([3.0], np.float32)]
    _, total, coef = clip_ref(g, 1.0, 1.0)
    assert total == np.inf and coef == 0.0
    leaves = [torch.zeros(a.size, dtype=torch.float64, requires_grad=True) for a in g]
    for l, a in zip(leaves, g):
        l.grad = torch.from_numpy(a).double()
    torch.nn.utils.clip_grad_norm_(leaves, 1.0)
    got = torch.cat([l.grad for l in leaves]).numpy()
    assert np.isnan(got[1]) and (got[[0, 2, 3]] == 0).all()
    want = np.concatenate(g).astype(np.float64) * coef
    assert np.isnan(want[1]) and (want[[0, 2, 3]] == 0).all()
    _, total, coef = clip_ref([np.array([np.nan, 1.0])], 1.0, 1.0)
    assert math.isnan(total) and math.isnan(coef)


@pytest.mark.parametrize("norm", [0.5, 40.0])
def test_the_bound_holds_the_fp32_arithmetic(norm):
    """The kernel's arithmetic emulated in numpy float32 (no contraction) stays inside the bound on both sides of the clip, and
    the bound is not slack: the emulation comes within a factor 50 of it."""
    worst = _three_steps(None, norm)
    print("fp32 emulation / bound (p, m, v):", worst)
    assert (worst <= 1.0).all() and (worst >= 0.02).all(), worst


@pytest.mark.parametrize("wrong", WRONG)
def test_the_bound_rejects_the_wrong_variants(wrong):
    """Each planted bug, emulated in float32, leaves the bound of p by a factor of at least 4 within three steps (at a gradient norm
    of 40, where the clip is live)."""
    worst = _three_steps(wrong, 40.0)
    print(f"{wrong}: emulation / bound (p, m, v): {worst}")
    assert worst[0] >= 4.0, (wrong, worst)


def test_sumsq_depth_transcribes_the_launch_rule():
    assert sumsq_depth(1) == 0 + 11 and sumsq_depth(3) == 11 and sumsq_depth(4) == 12 and sumsq_depth(1024) == 12 and sumsq_depth(1028) == 13
    assert sumsq_depth(16384) == 16 + 11 == sumsq_depth(10 ** 6)
    assert sumsq_depth(16385, nchunks=2) == 29 and sumsq_depth(16384, 4, 463) == 27 + 467
    x = det_normal("adamw.depth", (16384,)).astype(np.float64)
    s = float((x * x).sum())
    assert sumsq_bound(s, 16384) == 29 * U * s


def test_chunk_table_tiles_every_tensor():
    from cswin_unet_amd.optim import chunk_table
    numels = [1, 7, 9, 16384, 16385, 3 * 16384 + 5]
    offs, total = slots(numels)
    rows, first = chunk_table(numels, offs)
    assert rows.dtype.itemsize == 16 and rows.dtype.names == ("off", "n", "tensor") and first.dtype == np.int32
    assert first.tolist() == [0, 1, 2, 3, 4, 6, 10] and len(rows) == 10
    covered = np.zeros(total, int)
    for t, (n, o) in enumerate(zip(numels, offs)):
        mine = rows[first[t]:first[t + 1]]
        assert (mine["tensor"] == t).all() and len(mine) == cdiv(n, CHUNK)
        assert mine["off"][0] == o and (mine["off"][1:] == mine["off"][:-1] + mine["n"][:-1]).all()      # in order, no gap
        assert mine["off"][-1] + mine["n"][-1] == o + n and int(mine["n"].sum()) == n                    # ends with the tensor: no pad word
        for r in mine:
            covered[r["off"]:r["off"] + r["n"]] += 1
    assert (rows["n"] >= 1).all() and (rows["n"] <= CHUNK).all() and (rows["off"] % 4 == 0).all()
    assert (rows["tensor"][1:] >= rows["tensor"][:-1]).all()
    assert (covered == elem_mask(numels)).all()                       # every element once, every pad word never
    assert rows.view(np.int64).reshape(-1, 2)[5].tolist() == [int(rows["off"][5]), int(rows["n"][5]) | int(rows["tensor"][5]) << 32]
    with pytest.raises(ValueError):
        chunk_table([3, 3], [0, 4])


def _rgn_transcription(names, params, grads_per_batch):
    """universal_train.py:626-690 and :876-881 on numpy arrays, line for line."""
    layer_names = [n for n in names if "bn" not in n.lower() and "norm" not in n.lower()]
    metrics, average = defaultdict(list), defaultdict(float)
    for grads in grads_per_batch:
        _metrics = defaultdict(list)
        for name, param, grad in zip(names, params, grads):
            if name not in layer_names or grad is None:
                continue
            param_norm = float(np.linalg.norm(param))
            if param_norm > 1e-8:
                _metrics[name] = float(np.linalg.norm(grad)) / param_norm
            else:
                _metrics[name] = 0.0
        for k, v in _metrics.items():
            metrics[k].append(v)
    for k, v in metrics.items():
        if len(v) > 0:
            average[k] = np.array(v).mean(0)
    weights = dict(average)
    if weights:
        max_weight = max(weights.values()) if weights.values() else 1.0
        for k in weights:
            weights[k] = weights[k] / max_weight if max_weight > 0 else 0.0
    return weights


def test_rgn_weights_against_the_reference_arithmetic():
    from cswin_unet_amd.continual import rgn_weights
    names = ["stage1.0.qkv.weight", "stage1.0.norm1.weight", "stage1.0.mlp.fc1.bias", "output.weight", "merge1.BN.weight", "zero.weight"]
    rs = np.random.RandomState(3)
    params = [rs.standard_normal(n) for n in (12, 4, 6, 9, 4)] + [np.zeros(5)]
    batches = [[rs.standard_normal(p.size) * s for p in params] for s in (1.0, 0.1)] + [[np.zeros(p.size) for p in params]]     # the last batch: all zero
    norms = [[(np.linalg.norm(g), np.linalg.norm(p)) for g, p in zip(grads, params)] for grads in batches]
    got = rgn_weights(names, norms)
    want = _rgn_transcription(names, params, batches)
    assert set(got) == set(want) == {names[0], names[2], names[3], names[5]}
    assert all(abs(got[k] - want[k]) <= 1e-15 for k in want), (got, want)
    assert max(got.values()) == 1.0 and got["zero.weight"] == 0.0 and min(got.values()) >= 0.0
    zero = rgn_weights(names, [[(0.0, 1.0)] * 6])
    assert zero == _rgn_transcription(names, [np.ones(1)] * 6, [[np.zeros(1)] * 6]) and set(zero.values()) == {0.0}
    assert rgn_weights(names, torch.tensor(norms)) == got             # a (batches, T, 2) tensor's tolist() or the tensor itself
    with pytest.raises(ValueError):
        rgn_weights(names, [[(1.0, 1.0)] * 5])


def test_cosine_lr_is_cosine_annealing():
    from cswin_unet_amd.trainer import cosine_lr
    leaf = torch.zeros(1, requires_grad=True)
    opt = torch.optim.SGD([leaf], lr=1e-4)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=7)
    for epoch in range(8):
        assert abs(opt.param_groups[0]["lr"] - cosine_lr(1e-4, epoch, 7)) <= 1e-18, epoch
        opt.step()
        sched.step()
    assert cosine_lr(1e-4, 0, 7) == 1e-4 and abs(cosine_lr(1e-4, 7, 7)) < 1e-20


def test_flat_adamw_runs_on_a_hip_device_only():
    from cswin_unet_amd.optim import FlatAdamW, FlatSGD
    for cls in (FlatAdamW, FlatSGD):
        with pytest.raises(RuntimeError, match=cls.__name__):
            cls([torch.nn.Parameter(torch.zeros(3))], lr=1e-3)
        with pytest.raises(ValueError, match=cls.__name__):
            cls([], lr=1e-3)


def test_engine_options_are_validated_before_any_device_work():
    from cswin_unet_amd.trainer import DataParallelTrainer, HipEngine
    net = torch.nn.Linear(4, 4)
    with pytest.raises(ValueError, match="max_grad_norm"):
        HipEngine(net, 9, 0.05, 0.9, 1e-4, 0.4, 0.6, optimizer="sgd", max_grad_norm=1.0)
    with pytest.raises(ValueError, match="max_grad_norm"):
        DataParallelTrainer(net, 9, optimizer="sgd", max_grad_norm=1.0)
    with pytest.raises(ValueError, match="optimizer"):
        DataParallelTrainer(net, 9, optimizer="adam")
    with pytest.raises(ValueError, match="lr_schedule"):
        DataParallelTrainer(net, 9, lr_schedule="cosine")
    with pytest.raises(RuntimeError, match="FlatAdamW"):                # valid options: it gets as far as the CPU parameters
        DataParallelTrainer(net, 9, optimizer="adamw", max_grad_norm=1.0)
