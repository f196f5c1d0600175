"""The AdamW kernels (csrc/adamw.hip: cswin_chunk_sumsq, cswin_norm_finalize, cswin_adamw_flat) called directly on guarded flat
buffers, away from the model's layout: tensors on both sides of the 16-byte body, of a workgroup's 256 threads and of the
16384-element chunk, 1 to 463 tensors, both sides of the clip, every combination of the optional arguments, three consecutive
steps with the rate rewritten on the device.  References and bounds are test_adamw_host's (float64; the bounds are derived there
from the kernel's operations and shown to see the bugs they are for).  The pad words of the gradient buffer hold NaN, so a
kernel that reads one poisons the norm; those of p, m, v and the shadow hold sentinels that must survive bit for bit."""
import itertools
import math

import numpy as np
import pytest
import torch

from test_adamw_host import (BETA1, BETA2, EPS, LAYOUT, LRS, adamw_bound, adamw_inputs, adamw_ref, clip_ref, cdiv, elem_mask, flat,
                             norm_bounds, per_elem, slots, sumsq_bound)
from test_gpu_step_tail import (ERR_ALIGN, ERR_SHAPE, Guarded, GuardedAt, bits16, bits32, close, hip, put, release_inputs,  # noqa: F401
                                rne_bf16, settle)

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD_P, PAD_M, PAD_V = 7.0, -3.0, 5.0
MULTS = (0.0, 1.0, 0.37)
TENSOR_COUNTS = (1, 255, 256, 257, 463)          # the finalize kernel's second trip starts at 257; 463 is the model's count


def table(numels):
    """(device chunk table, device first_chunk, chunk count, chunks per tensor) of a layout."""
    from cswin_unet_amd.optim import chunk_table
    rows, first = chunk_table(numels, slots(numels)[0])
    return put(rows.view(np.int64).reshape(-1, 2)), put(first), len(rows), np.diff(first)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def state(numels, ps, shadow):
    """Guarded p, m, v (and shadow) of a layout: p from ps, m = v = 0, sentinels in the pad words."""
    total = slots(numels)[1]
    zeros = [np.zeros(n, np.float32) for n in numels]
    o = dict(p=Guarded((total,)), m=Guarded((total,)), v=Guarded((total,)))
    for name, arrays, pad in (("p", ps, PAD_P), ("m", zeros, PAD_M), ("v", zeros, PAD_V)):
        o[name].t.copy_(dev(flat(arrays, numels, fill=pad)))
    if shadow:
        o["shadow"] = Guarded((total,), torch.bfloat16)
        o["shadow"].t.copy_(o["p"].t.to(torch.bfloat16))
    return o


def grad_buffer(gs, numels):
    g = Guarded((slots(numels)[1],))
    g.t.copy_(dev(flat(gs, numels, fill=float("nan"))))
    return g


def norms(hip, g, p, tab, ntensors, grad_scale, max_norm, what):
    """chunk_sumsq + norm_finalize on guarded outputs: (partial, tensor_sumsq, scalars) as numpy, and the scalars' device tensor."""
    chunks, first, nchunks, _ = tab
    o = dict(partial=Guarded((nchunks, 2)), tensor_sumsq=Guarded((ntensors, 2)), scalars=Guarded((2,)))
    hip.call("cswin_chunk_sumsq", hip.ptr(g.t), None if p is None else hip.ptr(p), hip.ptr(chunks), nchunks, hip.ptr(o["partial"].t), hip.stream())
    hip.call("cswin_norm_finalize", hip.ptr(o["partial"].t), hip.ptr(first), ntensors, grad_scale, max_norm, hip.ptr(o["tensor_sumsq"].t),
             hip.ptr(o["scalars"].t), hip.stream())
    torch.cuda.synchronize()
    assert all(b.intact() for b in o.values()) and g.intact(), f"{what}: a guard word was overwritten"
    return o["partial"].t.cpu().numpy(), o["tensor_sumsq"].t.cpu().numpy(), o["scalars"].t.cpu().numpy(), o["scalars"]


def check_norms(gs, ps, numels, per_tensor_chunks, grad_scale, max_norm, sumsq, scalars, what):
    """tensor_sumsq and the two scalars against float64 within the derived bounds."""
    want, total, coef = clip_ref(gs, grad_scale, max_norm)
    bound = np.array([sumsq_bound(s, n, int(c)) for s, n, c in zip(want, numels, per_tensor_chunks)])
    close(sumsq[:, 0], want, bound, what + ".sumsq_g")
    if ps is not None:
        wantp = clip_ref(ps, 1.0, 1.0)[0]
        close(sumsq[:, 1], wantp, np.array([sumsq_bound(s, n, int(c)) for s, n, c in zip(wantp, numels, per_tensor_chunks)]), what + ".sumsq_p")
    btotal, bcoef = norm_bounds(total, coef, max(numels), int(max(per_tensor_chunks)), len(numels))
    close(scalars[:1], [total], [btotal], what + ".total_norm")
    if coef == 1.0 and max_norm / (total + btotal + 1e-6) > 1.0:
        assert scalars[1] == 1.0, (what, scalars)                       # clamped on both sides: exactly 1
    else:
        close(scalars[1:], [coef], [bcoef], what + ".clip_coef")
    return total, coef


def update(hip, o, g, tab, lr_dev, mult_dev, scalars, wd, grad_scale, step, what):
    chunks, _, nchunks, _ = tab
    hip.call("cswin_adamw_flat", hip.ptr(o["p"].t), hip.ptr(g.t), hip.ptr(o["m"].t), hip.ptr(o["v"].t), hip.ptr(chunks), nchunks, hip.ptr(lr_dev),
             hip.ptr(mult_dev), None if scalars is None else hip.ptr(scalars.t), BETA1, BETA2, EPS, wd, grad_scale, 1 - BETA1 ** step, 1 - BETA2 ** step,
             hip.ptr(o["shadow"].t) if "shadow" in o else None, hip.stream())
    settle(what, o)
    assert g.intact(), what


def three_steps(hip, numels, tag, clip, with_mult, shadow, wd, grad_scale, norm_targets=(40.0, 0.5, 40.0)):
    """Three steps on one layout, each compared with adamw_ref from the state the kernel had."""
    tab = table(numels)
    mask = elem_mask(numels)
    mults = np.array([MULTS[t % 3] for t in range(len(numels))], np.float32)
    mult_dev = put(mults) if with_mult else None
    mult_e = per_elem(mults.astype(np.float64), numels) if with_mult else 1.0
    frozen = (per_elem(mults.astype(np.float64), numels) == 0.0) & mask if with_mult else np.zeros_like(mask)
    lr_dev = put(np.array([LRS[0]], np.float32))
    o, pads = None, {}
    for k in range(3):
        ps, gs = adamw_inputs(tag, numels, norm=norm_targets[k] / grad_scale)
        if o is None:
            o = state(numels, ps, shadow)
            pads = {name: (bits16 if name == "shadow" else bits32)(b.t)[~mask].copy() for name, b in o.items()}
        if k:
            lr_dev.mul_(LRS[k] / LRS[k - 1])                             # rewritten on the device: the host passes no learning rate
        lr = float(lr_dev.cpu()[0])
        g = grad_buffer(gs[k], numels)
        what = f"adamw.{tag}.{'clip' if clip else 'noclip'}.{'mult' if with_mult else 'nomult'}.{'shadow' if shadow else 'noshadow'}.wd{wd}.gs{grad_scale}.step{k + 1}"
        coef, scalars = 1.0, None
        if clip:
            _, sumsq, sc, scalars = norms(hip, g, None, tab, len(numels), grad_scale, 1.0, what)
            check_norms(gs[k], None, numels, tab[3], grad_scale, 1.0, sumsq, sc, what)
            coef = float(sc[1])                                          # the update is held to the coefficient it was given
            assert (coef == 1.0) == (norm_targets[k] < 1.0), (what, sc)
        before = {name: b.t.clone() for name, b in o.items()}
        prev = [before[name].cpu().numpy().astype(np.float64) for name in ("p", "m", "v")]
        update(hip, o, g, tab, lr_dev, mult_dev, scalars, wd, grad_scale, k + 1, what)
        g64 = np.nan_to_num(g.t.cpu().numpy().astype(np.float64))       # the pad words: masked out below
        kw = dict(wd=wd, grad_scale=grad_scale, clip=coef, mult=mult_e)
        ref = adamw_ref(prev[0], g64, prev[1], prev[2], k + 1, lr, **kw)
        bound = adamw_bound(prev[0], g64, prev[1], prev[2], k + 1, lr, **kw)
        for name, want, b in zip(("p", "m", "v"), ref, bound):
            close(o[name].t.cpu().numpy()[mask], want[mask], b[mask], f"{what}.{name}")
        for name, b in o.items():                                        # no pad word of p, m, v or the shadow was written
            assert ((bits16 if name == "shadow" else bits32)(b.t)[~mask] == pads[name]).all(), f"{what}: a pad word of {name} changed"
        if shadow:
            assert torch.equal(o["shadow"].t, o["p"].t.to(torch.bfloat16)), what
            want16, nan = rne_bf16(bits32(o["p"].t))
            assert not nan.any() and (bits16(o["shadow"].t) == want16).all(), what
        if with_mult:
            assert frozen.any() and (bits32(o["p"].t)[frozen] == bits32(before["p"])[frozen]).all(), f"{what}: a frozen parameter moved"
            assert not shadow or (bits16(o["shadow"].t)[frozen] == bits16(before["shadow"])[frozen]).all(), f"{what}: a frozen shadow moved"
            assert (bits32(o["m"].t)[frozen] != bits32(before["m"])[frozen]).mean() > 0.99, f"{what}: the moments of a frozen tensor stood still"
            assert (bits32(o["v"].t)[frozen] != bits32(before["v"])[frozen]).mean() > 0.99, what
            live = mask & ~frozen
            assert not live.any() or (bits32(o["p"].t)[live] != bits32(before["p"])[live]).mean() > 0.99, what
    return o


@pytest.mark.parametrize("with_mult", [False, True], ids=["nomult", "mult"])
@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
def test_adamw_flat_three_steps_vs_float64(hip, clip, with_mult):
    """The ten-tensor layout: clip on / off x multipliers null / {0, 1, 0.37} x shadow on / off x weight decay {0, 0.01}, the
    gradient scale 1 with the first decay and 0.125 with the second; gradient norms 40, 0.5, 40 (times 1 / grad_scale)."""
    assert LAYOUT == (1, 3, 4, 5, 1023, 1027, 16383, 16384, 16385, 3 * 16384 + 5)
    for shadow, (wd, grad_scale) in itertools.product((False, True), ((0.0, 1.0), (0.01, 0.125))):
        three_steps(hip, LAYOUT, "layout", clip, with_mult, shadow, wd, grad_scale)


@pytest.mark.parametrize("ntensors", TENSOR_COUNTS)
def test_one_element_tensors(hip, ntensors):
    """T one-element tensors (eight-float slots, seven pad words each): the per-tensor sums are single squares, the finalize kernel
    takes a second trip from T = 257 on, and the update reads a multiplier per chunk."""
    numels = (1,) * ntensors
    three_steps(hip, numels, f"T{ntensors}", True, True, True, 0.01, 1.0)
    tab = table(numels)
    ps, gs = adamw_inputs(f"T{ntensors}", numels, norm=40.0)
    g = grad_buffer(gs[0], numels)
    p = put(flat(ps, numels, fill=float("nan")))
    partial, sumsq, sc, _ = norms(hip, g, p, tab, ntensors, 1.0, 1.0, f"adamw.T{ntensors}.norms")
    check_norms(gs[0], ps, numels, tab[3], 1.0, 1.0, sumsq, sc, f"adamw.T{ntensors}.norms")
    sq = np.concatenate(gs[0]).astype(np.float32) ** 2
    assert np.array_equal(sumsq[:, 0], sq) and np.array_equal(partial[:, 0], sq)      # one rounding and additions of zero


@pytest.mark.parametrize("grad_scale", [1.0, 0.125])
@pytest.mark.parametrize("target", [0.5, 40.0])
def test_norms_on_both_sides_of_the_clip(hip, target, grad_scale):
    """tensor_sumsq, total_norm and clip_coef of the ten-tensor layout against float64, with the parameters and without: then
    only the first column of partial is written."""
    numels = LAYOUT
    tab = table(numels)
    ps, gs = adamw_inputs("norms", numels, norm=target / grad_scale)
    g = grad_buffer(gs[0], numels)
    p = put(flat(ps, numels, fill=float("nan")))
    what = f"adamw.norms.n{target}.gs{grad_scale}"
    partial, sumsq, sc, _ = norms(hip, g, p, tab, len(numels), grad_scale, 1.0, what + ".with_p")
    total, coef = check_norms(gs[0], ps, numels, tab[3], grad_scale, 1.0, sumsq, sc, what + ".with_p")
    assert abs(total - target) < 1e-3 * target and (coef == 1.0) == (target < 1.0) and np.isfinite(partial).all()
    assert list(tab[3]) == [cdiv(n, 16384) for n in numels] and tab[2] == 14
    partial0, sumsq0, sc0, _ = norms(hip, g, None, tab, len(numels), grad_scale, 1.0, what + ".no_p")
    assert np.isnan(partial0[:, 1]).all() and np.array_equal(partial0[:, 0], partial[:, 0])
    assert np.array_equal(sumsq0[:, 0], sumsq[:, 0]) and np.array_equal(sc0, sc)
    check_norms(gs[0], None, numels, tab[3], grad_scale, 1.0, sumsq0, sc0, what + ".no_p")


def test_one_infinite_gradient_gives_torchs_outcome(hip):
    """One +inf: total_norm inf, clip_coef 0, that element's g' = inf * 0 = NaN (so its m, v and p), every other g' exactly 0 --
    m and v stay 0 at the first step and p only decays.  A NaN is reported, not repaired."""
    numels = (5, 1027, 9)
    tab = table(numels)
    mask = elem_mask(numels)
    ps, gs = adamw_inputs("inf", numels, norm=3.0)
    bad = slots(numels)[0][1] + 513
    gs[0][1][513] = np.inf
    g = grad_buffer(gs[0], numels)
    _, sumsq, sc, scalars = norms(hip, g, None, tab, 3, 1.0, 1.0, "adamw.inf")
    assert sc[0] == np.inf and sc[1] == 0.0 and sumsq[1, 0] == np.inf and np.isfinite(sumsq[[0, 2], 0]).all()
    o = state(numels, ps, True)
    p0 = o["p"].t.cpu().numpy().astype(np.float64)
    lr_dev = put(np.array([LRS[0]], np.float32))
    chunks, _, nchunks, _ = tab
    hip.call("cswin_adamw_flat", hip.ptr(o["p"].t), hip.ptr(g.t), hip.ptr(o["m"].t), hip.ptr(o["v"].t), hip.ptr(chunks), nchunks, hip.ptr(lr_dev),
             None, hip.ptr(scalars.t), BETA1, BETA2, EPS, 0.01, 1.0, 1 - BETA1, 1 - BETA2, hip.ptr(o["shadow"].t), hip.stream())
    torch.cuda.synchronize()
    assert all(b.intact() for b in o.values())
    p, m, v = (o[k].t.cpu().numpy() for k in ("p", "m", "v"))
    assert np.isnan(p[bad]) and np.isnan(m[bad]) and np.isnan(v[bad]) and bool(torch.isnan(o["shadow"].t[bad]))
    rest = mask.copy()
    rest[bad] = False
    assert (m[rest] == 0).all() and (v[rest] == 0).all() and np.isfinite(p[rest]).all()
    lr = float(lr_dev.cpu()[0])
    zeros = np.zeros_like(p0)
    want = adamw_ref(p0, zeros, zeros, zeros, 1, lr, wd=0.01)[0]
    close(p[rest], want[rest], adamw_bound(p0, zeros, zeros, zeros, 1, lr, wd=0.01)[0][rest], "adamw.inf.p")
    assert (p[~mask] == PAD_P).all()


def test_two_runs_give_the_same_bits(hip):
    """No float atomics: every sum has a fixed order."""
    runs = []
    for _ in range(2):
        numels = LAYOUT
        tab = table(numels)
        ps, gs = adamw_inputs("bits", numels, norm=40.0)
        g = grad_buffer(gs[0], numels)
        partial, sumsq, sc, scalars = norms(hip, g, put(flat(ps, numels)), tab, len(numels), 1.0, 1.0, "adamw.bits")
        o = state(numels, ps, True)
        update(hip, o, g, tab, put(np.array([LRS[0]], np.float32)), put(np.array([MULTS[t % 3] for t in range(len(numels))], np.float32)), scalars,
               0.01, 1.0, 1, "adamw.bits")
        runs.append([partial.view(np.uint32), sumsq.view(np.uint32), sc.view(np.uint32)] + [bits32(o[k].t) for k in ("p", "m", "v")] + [bits16(o["shadow"].t)])
    assert all(np.array_equal(a, b) for a, b in zip(*runs))


def test_refusals_touch_nothing(hip):
    """A null buffer, a pointer four bytes off a 16-byte boundary and nchunks = 0 return their error codes; nothing is launched."""
    numels = (9, 5)
    tab = table(numels)
    chunks, first, nchunks, _ = tab
    total = slots(numels)[1]
    names = ("p", "g", "m", "v")
    o = {n: Guarded((total,)) for n in names}
    o.update({n + "1": GuardedAt((total,), off=1) for n in names})
    o.update(shadow=Guarded((total,), torch.bfloat16), shadow1=GuardedAt((total,), torch.bfloat16, off=1), partial=Guarded((nchunks, 2)),
             tensor_sumsq=Guarded((2, 2)), scalars=Guarded((2,)))
    lr = put(np.array([0.1], np.float32))

    def adamw_args(n=nchunks, shadow="shadow", lr_dev=lr, table_=chunks, **swap):
        bufs = [None if swap.get(k, k) is None else hip.ptr(o[swap.get(k, k)].t) for k in names]
        return bufs + [hip.ptr(table_), n, hip.ptr(lr_dev), None, None, BETA1, BETA2, EPS, 0.01, 1.0, 0.1, 0.001, hip.ptr(o[shadow].t), hip.stream()]

    for k in names:
        hip.refused(ERR_SHAPE, f"adamw_flat {k} null", o, "cswin_adamw_flat", *adamw_args(**{k: None}))
        hip.refused(ERR_ALIGN, f"adamw_flat {k} 4 bytes off", o, "cswin_adamw_flat", *adamw_args(**{k: k + "1"}))
    hip.refused(ERR_ALIGN, "adamw_flat shadow 2 bytes off", o, "cswin_adamw_flat", *adamw_args(shadow="shadow1"))
    hip.refused(ERR_SHAPE, "adamw_flat nchunks 0", o, "cswin_adamw_flat", *adamw_args(n=0))
    hip.refused(ERR_SHAPE, "adamw_flat no table", o, "cswin_adamw_flat", *adamw_args(table_=None))
    hip.refused(ERR_SHAPE, "adamw_flat no rate", o, "cswin_adamw_flat", *adamw_args(lr_dev=None))
    sumsq = lambda g="g", p="p", n=nchunks, part="partial": (None if g is None else hip.ptr(o[g].t), None if p is None else hip.ptr(o[p].t), hip.ptr(chunks), n,
                                                             None if part is None else hip.ptr(o[part].t), hip.stream())
    hip.refused(ERR_SHAPE, "chunk_sumsq g null", o, "cswin_chunk_sumsq", *sumsq(g=None))
    hip.refused(ERR_SHAPE, "chunk_sumsq partial null", o, "cswin_chunk_sumsq", *sumsq(part=None))
    hip.refused(ERR_SHAPE, "chunk_sumsq nchunks 0", o, "cswin_chunk_sumsq", *sumsq(n=0))
    hip.refused(ERR_ALIGN, "chunk_sumsq g 4 bytes off", o, "cswin_chunk_sumsq", *sumsq(g="g1"))
    hip.refused(ERR_ALIGN, "chunk_sumsq p 4 bytes off", o, "cswin_chunk_sumsq", *sumsq(p="p1"))
    fin = lambda part="partial", n=2, ts="tensor_sumsq", sc="scalars": (None if part is None else hip.ptr(o[part].t), hip.ptr(first), n, 1.0, 1.0,
                                                                        None if ts is None else hip.ptr(o[ts].t), None if sc is None else hip.ptr(o[sc].t), hip.stream())
    hip.refused(ERR_SHAPE, "norm_finalize partial null", o, "cswin_norm_finalize", *fin(part=None))
    hip.refused(ERR_SHAPE, "norm_finalize tensor_sumsq null", o, "cswin_norm_finalize", *fin(ts=None))
    hip.refused(ERR_SHAPE, "norm_finalize scalars null", o, "cswin_norm_finalize", *fin(sc=None))
    hip.refused(ERR_SHAPE, "norm_finalize ntensors 0", o, "cswin_norm_finalize", *fin(n=0))
