"""The per-step rate and Adam kernels (csrc/adamw.hip: cswin_rate_finalize, cswin_adam_flat) called directly on guarded flat
buffers, away from the model's layout: the ten-tensor layout of test_adamw_host on both sides of the 16-byte body, of a workgroup's
256 threads and of the 16384-element chunk, 1 to 463 tiny tensors in 1 to 463 interleaved groups (the finalize kernel's second trip
over tensors and over groups starts at 257), both statistics, every flag combination of the update over three steps.  References
and bounds are test_auto_rates_host's (float64; the bounds are derived there from the kernels' operations and shown to see the
bugs they are for).  The pad words of the gradient buffer hold NaN, those of p, m, v and the shadow sentinels that must survive
bit for bit."""
import itertools

import numpy as np
import pytest
import torch

from test_adamw_host import BETA1, BETA2, EPS, LAYOUT, LRS, adamw_inputs, elem_mask, flat, per_elem, slots
from test_auto_rates_host import COUPLED, FLAGS, FRESH, adam_bound, adam_ref, group_rates_bound, group_rates_ref, one_group_at_one
from test_gpu_adamw import MULTS, TENSOR_COUNTS, check_norms, grad_buffer, norms, state, table
from test_gpu_step_tail import (ERR_ALIGN, ERR_SHAPE, Guarded, GuardedAt, bits16, bits32, close, hip, put, release_inputs,  # noqa: F401
                                rne_bf16, settle)

pytestmark = pytest.mark.gpu
GROUP_COUNTS = (1, 22, 256, 257)                 # and T itself: one group per tensor, the per-tensor mode
STATISTICS = ("grad", "ratio")
DEFAULT_MULT = 0.25


def tiny(ntensors):
    """1 to 9 elements per tensor: every slot has pad words, most sums have several terms."""
    return tuple(1 + t % 9 for t in range(ntensors))


def membership(ntensors, ngroups):
    """Tensor t is in group t % G, so a group's members are interleaved with the others'; past the first G tensors (which keep every
    group occupied) every fifth tensor is in no group."""
    return [-1 if t >= ngroups and t % 5 == 2 else t % ngroups for t in range(ntensors)]


def group_tables(group_of, ngroups):
    """The device CSR table of a membership, built by hand (optim.group_table is checked against the same rule on the host)."""
    mem = [[t for t, k in enumerate(group_of) if k == g] for g in range(ngroups)]
    first = np.cumsum([0] + [len(m) for m in mem]).astype(np.int32)
    return put(first), put(np.array([t for m in mem for t in m], np.int32)), put(np.array(group_of, np.int32))


RATE_CASES = [("layout", LAYOUT, g) for g in (1, 3, len(LAYOUT))] + \
             [(f"T{t}", tiny(t), g) for t in TENSOR_COUNTS for g in sorted(set(GROUP_COUNTS + (t,))) if g <= t]


def rates(hip, g, p, tab, numels, group_of, ngroups, statistic, grad_scale, max_norm, what, default=DEFAULT_MULT):
    """chunk_sumsq (with the parameters only in the ratio mode) + rate_finalize on guarded outputs; everything as numpy."""
    chunks, first, nchunks, _ = tab
    T = len(numels)
    gf, gt, go = group_tables(group_of, ngroups)
    o = dict(partial=Guarded((nchunks, 2)), tensor_sumsq=Guarded((T, 2)), scalars=Guarded((2,)), group_stat=Guarded((ngroups,)), lr_mult=Guarded((T,)))
    hip.call("cswin_chunk_sumsq", hip.ptr(g.t), hip.ptr(p) if statistic == "ratio" else None, hip.ptr(chunks), nchunks, hip.ptr(o["partial"].t), hip.stream())
    hip.call("cswin_rate_finalize", hip.ptr(o["partial"].t), hip.ptr(first), T, grad_scale, max_norm, hip.ptr(gf), hip.ptr(gt), hip.ptr(go), ngroups,
             STATISTICS.index(statistic), default, hip.ptr(o["tensor_sumsq"].t), hip.ptr(o["scalars"].t), hip.ptr(o["group_stat"].t),
             hip.ptr(o["lr_mult"].t), hip.stream())
    torch.cuda.synchronize()
    assert all(b.intact() for b in o.values()) and g.intact(), f"{what}: a guard word was overwritten"
    return {k: b.t.cpu().numpy() for k, b in o.items()}


def sums64(arrays):
    return np.array([float((a.astype(np.float64) ** 2).sum()) for a in arrays])


@pytest.mark.parametrize("tag,numels,ngroups", RATE_CASES, ids=[f"{c[0]}.G{c[2]}" for c in RATE_CASES])
def test_rate_finalize_vs_float64_and_norm_finalize(hip, tag, numels, ngroups):
    """Both statistics: tensor_sumsq and scalars are cswin_norm_finalize's bits on the same partial sums, group_stat and lr_mult
    stay inside the derived bounds, exactly one group's multiplier is 1, a tensor in no group has default_mult exactly, and a
    second run gives the same bits."""
    T = len(numels)
    tab = table(numels)
    group_of = membership(T, ngroups)
    assert set(group_of) - {-1} == set(range(ngroups)) and (ngroups == T or -1 in group_of or T <= ngroups + 2)
    ps, gs = adamw_inputs(f"rates.{tag}", numels, norm=40.0)
    g, p = grad_buffer(gs[0], numels), put(flat(ps, numels, fill=float("nan")))
    grouped = np.array(group_of) >= 0
    for statistic, grad_scale in zip(STATISTICS, (0.125, 1.0)):
        what = f"rates.{tag}.G{ngroups}.{statistic}"
        got = rates(hip, g, p, tab, numels, group_of, ngroups, statistic, grad_scale, 1.0, what)
        _, want_sumsq, want_sc, _ = norms(hip, g, p if statistic == "ratio" else None, tab, T, grad_scale, 1.0, what + ".norm_finalize")
        assert np.array_equal(got["tensor_sumsq"].view(np.uint32), want_sumsq.view(np.uint32)), what
        assert np.array_equal(got["scalars"].view(np.uint32), want_sc.view(np.uint32)), what
        assert np.isnan(got["tensor_sumsq"][:, 1]).all() == (statistic == "grad")          # the parameters are read in the ratio mode only
        check_norms(gs[0], ps if statistic == "ratio" else None, numels, tab[3], grad_scale, 1.0, got["tensor_sumsq"], got["scalars"], what)
        sg, sp = sums64(gs[0]), sums64(ps)
        want_stat, want_mult = group_rates_ref(sg, sp, group_of, ngroups, statistic, grad_scale, DEFAULT_MULT)
        bstat, bmult = group_rates_bound(sg, sp, numels, tab[3], group_of, ngroups, statistic, grad_scale)
        close(got["group_stat"], want_stat, bstat, what + ".group_stat")
        close(got["lr_mult"], want_mult, bmult, what + ".lr_mult")
        assert one_group_at_one(got["lr_mult"], group_of), what
        assert (got["lr_mult"][~grouped] == np.float32(DEFAULT_MULT)).all() and (got["lr_mult"][grouped] > 0).all(), what
        again = rates(hip, g, p, tab, numels, group_of, ngroups, statistic, grad_scale, 1.0, what + ".again")
        assert all(np.array_equal(got[k].view(np.uint32), again[k].view(np.uint32)) for k in got), what


@pytest.mark.parametrize("tag,numels,ngroups", [("layout", LAYOUT, 3), ("T463", tiny(463), 257)], ids=["layout.G3", "T463.G257"])
def test_rate_finalize_edge_cases(hip, tag, numels, ngroups):
    """A zero gradient: every grouped multiplier is 0.  One NaN gradient: NaN multipliers in every group, reported and not
    repaired, the tensors in no group untouched by it.  Ratio mode: a group whose parameters are all zero has statistic 0."""
    T = len(numels)
    tab = table(numels)
    group_of = membership(T, ngroups) if T > ngroups + 2 else [0, 1, 2, -1, 0, 1, 2, 0, 1, 2]
    grouped = np.array(group_of) >= 0
    assert (~grouped).any()
    ps, gs = adamw_inputs(f"rates.edge.{tag}", numels, norm=3.0)
    p = put(flat(ps, numels, fill=float("nan")))
    zero = grad_buffer([np.zeros(n, np.float32) for n in numels], numels)
    for statistic in STATISTICS:
        got = rates(hip, zero, p, tab, numels, group_of, ngroups, statistic, 1.0, 1.0, f"rates.zero.{tag}.{statistic}")
        assert (got["group_stat"] == 0).all() and (got["lr_mult"][grouped] == 0).all() and (got["lr_mult"][~grouped] == np.float32(DEFAULT_MULT)).all()
        assert got["scalars"][0] == 0 and got["scalars"][1] == 1
    bad_t = T // 2
    gs_nan = [a.copy() for a in gs[0]]
    gs_nan[bad_t][numels[bad_t] // 2] = np.nan
    g = grad_buffer(gs_nan, numels)
    for statistic in STATISTICS:
        got = rates(hip, g, p, tab, numels, group_of, ngroups, statistic, 1.0, 1.0, f"rates.nan.{tag}.{statistic}")
        assert np.isnan(got["lr_mult"][grouped]).all() and (got["lr_mult"][~grouped] == np.float32(DEFAULT_MULT)).all()
        assert np.isnan(got["scalars"]).all() and np.isnan(got["tensor_sumsq"][bad_t, 0])
        assert np.isnan(got["group_stat"]).sum() == 1 and np.isnan(got["group_stat"][group_of[bad_t]])
        assert np.isfinite(np.delete(got["tensor_sumsq"][:, 0], bad_t)).all()
    ps0 = [np.zeros_like(a) if group_of[t] == 1 else a for t, a in enumerate(ps)]
    g = grad_buffer(gs[0], numels)
    got = rates(hip, g, put(flat(ps0, numels, fill=float("nan"))), tab, numels, group_of, ngroups, "ratio", 1.0, 1.0, f"rates.p0.{tag}")
    want_stat, want_mult = group_rates_ref(sums64(gs[0]), sums64(ps0), group_of, ngroups, "ratio", 1.0, DEFAULT_MULT)
    assert got["group_stat"][1] == 0 and want_stat[1] == 0 and (got["lr_mult"][np.array(group_of) == 1] == 0).all()
    bstat, bmult = group_rates_bound(sums64(gs[0]), sums64(ps0), numels, tab[3], group_of, ngroups, "ratio", 1.0)
    close(got["lr_mult"], want_mult, bmult, f"rates.p0.{tag}.lr_mult")
    assert one_group_at_one(got["lr_mult"], group_of)


# ---- the update ---------------------------------------------------------------------------------------------------------------
def adam_update(hip, o, g, tab, lr_dev, mult_dev, scalars, wd, grad_scale, step, flags, what, null_moments=False, entry="cswin_adam_flat"):
    chunks, _, nchunks, _ = tab
    bc = (1 - BETA1, 1 - BETA2) if flags & FRESH else (1 - BETA1 ** step, 1 - BETA2 ** step)       # as optim.FlatAdamW.apply forms them
    m, v = (None, None) if null_moments else (hip.ptr(o["m"].t), hip.ptr(o["v"].t))
    head = [hip.ptr(o["p"].t), hip.ptr(g.t), m, v, hip.ptr(chunks), nchunks, hip.ptr(lr_dev), hip.ptr(mult_dev),
            None if scalars is None else hip.ptr(scalars.t), BETA1, BETA2, EPS, wd, grad_scale, *bc]
    tail = [hip.ptr(o["shadow"].t) if "shadow" in o else None, hip.stream()]
    hip.call(entry, *head, *([flags] if entry == "cswin_adam_flat" else []), *tail)
    settle(what, o)
    assert g.intact(), what


def clone_state(o):
    c = {}
    for name, b in o.items():
        c[name] = Guarded(tuple(b.t.shape), b.t.dtype)
        c[name].t.copy_(b.t)
    return c


def all_bits(b):
    return (bits16 if b.buf.dtype == torch.bfloat16 else bits32)(b.buf)


def adam_three_steps(hip, numels, tag, flags, clip, with_mult, shadow, wd, grad_scale, norm_targets=(40.0, 0.5, 40.0)):
    """Three steps on one layout, each compared with adam_ref from the state the kernel had."""
    coupled, fresh = bool(flags & COUPLED), bool(flags & FRESH)
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
            if fresh:                                                    # moments a fresh step must neither read nor write
                o["m"].t.copy_(torch.from_numpy(flat([np.full(n, 0.5, np.float32) for n in numels], numels, fill=-3.0)).to("cuda"))
                o["v"].t.copy_(torch.from_numpy(flat([np.full(n, 2.0, np.float32) for n in numels], numels, fill=5.0)).to("cuda"))
            pads = {name: (bits16 if name == "shadow" else bits32)(b.t)[~mask].copy() for name, b in o.items()}
        if k:
            lr_dev.mul_(LRS[k] / LRS[k - 1])
        lr = float(lr_dev.cpu()[0])
        g = grad_buffer(gs[k], numels)
        what = (f"adam.{tag}.flags{flags}.{'clip' if clip else 'noclip'}.{'mult' if with_mult else 'nomult'}."
                f"{'shadow' if shadow else 'noshadow'}.wd{wd}.gs{grad_scale}.step{k + 1}")
        coef, scalars = 1.0, None
        if clip:
            _, _, sc, scalars = norms(hip, g, None, tab, len(numels), grad_scale, 1.0, what)
            coef = float(sc[1])                                          # the update is held to the coefficient it was given
            assert (coef == 1.0) == (norm_targets[k] < 1.0), (what, sc)
        before = {name: b.t.clone() for name, b in o.items()}
        whole = {name: all_bits(b).copy() for name, b in o.items()}
        prev = [before[name].cpu().numpy().astype(np.float64) for name in ("p", "m", "v")]
        twin = clone_state(o) if flags == 0 or fresh else None
        adam_update(hip, o, g, tab, lr_dev, mult_dev, scalars, wd, grad_scale, k + 1, flags, what)
        if flags == 0:                                                   # both bits clear: cswin_adamw_flat, bit for bit
            adam_update(hip, twin, g, tab, lr_dev, mult_dev, scalars, wd, grad_scale, k + 1, 0, what + ".adamw_flat", entry="cswin_adamw_flat")
            assert all(np.array_equal(all_bits(o[n]), all_bits(twin[n])) for n in o), f"{what}: flags 0 is not cswin_adamw_flat"
        if fresh:                                                        # m and v are not looked at: null pointers do as well
            adam_update(hip, twin, g, tab, lr_dev, mult_dev, scalars, wd, grad_scale, k + 1, flags, what + ".null_moments", null_moments=True)
            assert all(np.array_equal(all_bits(o[n]), all_bits(twin[n])) for n in o), f"{what}: null moments give another result"
            assert np.array_equal(all_bits(o["m"]), whole["m"]) and np.array_equal(all_bits(o["v"]), whole["v"]), f"{what}: a fresh step touched m or v"
        g64 = np.nan_to_num(g.t.cpu().numpy().astype(np.float64))       # the pad words: masked out below
        kw = dict(wd=wd, grad_scale=grad_scale, clip=coef, mult=mult_e, coupled=coupled, fresh=fresh)
        ref = adam_ref(prev[0], g64, prev[1], prev[2], k + 1, lr, **kw)
        bound = adam_bound(prev[0], g64, prev[1], prev[2], k + 1, lr, **kw)
        for name, want, b in zip(("p", "m", "v"), ref, bound):
            close(o[name].t.cpu().numpy()[mask], want[mask], b[mask], f"{what}.{name}")
        for name, b in o.items():                                        # no pad word of p, m, v or the shadow was written
            assert ((bits16 if name == "shadow" else bits32)(b.t)[~mask] == pads[name]).all(), f"{what}: a pad word of {name} changed"
        if shadow:
            want16, nan = rne_bf16(bits32(o["p"].t))
            assert not nan.any() and (bits16(o["shadow"].t) == want16).all(), what
        if with_mult:
            assert frozen.any() and (bits32(o["p"].t)[frozen] == bits32(before["p"])[frozen]).all(), f"{what}: a frozen parameter moved"
            assert not shadow or (bits16(o["shadow"].t)[frozen] == bits16(before["shadow"])[frozen]).all(), f"{what}: a frozen shadow moved"
            if not fresh:
                assert (bits32(o["m"].t)[frozen] != bits32(before["m"])[frozen]).mean() > 0.99, f"{what}: the moments of a frozen tensor stood still"
            live = mask & ~frozen
            assert not live.any() or (bits32(o["p"].t)[live] != bits32(before["p"])[live]).mean() > 0.99, what


@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
@pytest.mark.parametrize("flags", FLAGS, ids=["adamw", "coupled", "fresh", "coupled.fresh"])
def test_adam_flat_three_steps_vs_float64(hip, flags, clip):
    """The ten-tensor layout: flags x clip on / off x multipliers null / {0, 1, 0.37} x shadow on / off, weight decay 1e-4 at
    gradient scale 1 without the shadow and 1e-2 at 0.125 with it; gradient norms 40, 0.5, 40 (times 1 / grad_scale)."""
    for with_mult, (shadow, wd, grad_scale) in itertools.product((False, True), ((False, 1e-4, 1.0), (True, 1e-2, 0.125))):
        adam_three_steps(hip, LAYOUT, "layout", flags, clip, with_mult, shadow, wd, grad_scale)


@pytest.mark.parametrize("ntensors", TENSOR_COUNTS)
def test_adam_flat_on_tiny_tensors(hip, ntensors):
    """T tensors of 1 to 9 elements, coupled with kept and with fresh moments: a multiplier per chunk, scalar tails everywhere."""
    for flags in (COUPLED, COUPLED | FRESH):
        adam_three_steps(hip, tiny(ntensors), f"T{ntensors}", flags, True, True, True, 1e-2, 1.0)


def test_rates_feed_the_update_on_the_device(hip):
    """The three launches of an auto-rate step in a row, nothing read in between: the update uses the multipliers and the clip
    coefficient that rate_finalize left in device memory."""
    numels = LAYOUT
    tab = table(numels)
    chunks, first, nchunks, _ = tab
    group_of = [0, 1, 2, -1, 0, 1, 2, 0, 1, 2]
    mask = elem_mask(numels)
    ps, gs = adamw_inputs("rates.chain", numels, norm=40.0)
    g = grad_buffer(gs[0], numels)
    o = state(numels, ps, True)
    prev = [o[n].t.cpu().numpy().astype(np.float64) for n in ("p", "m", "v")]
    gf, gt, go = group_tables(group_of, 3)
    r = dict(partial=Guarded((nchunks, 2)), tensor_sumsq=Guarded((10, 2)), scalars=Guarded((2,)), group_stat=Guarded((3,)), lr_mult=Guarded((10,)))
    lr_dev = put(np.array([LRS[0]], np.float32))
    hip.call("cswin_chunk_sumsq", hip.ptr(g.t), None, hip.ptr(chunks), nchunks, hip.ptr(r["partial"].t), hip.stream())
    hip.call("cswin_rate_finalize", hip.ptr(r["partial"].t), hip.ptr(first), 10, 1.0, 1.0, hip.ptr(gf), hip.ptr(gt), hip.ptr(go), 3, 0, 0.0,
             hip.ptr(r["tensor_sumsq"].t), hip.ptr(r["scalars"].t), hip.ptr(r["group_stat"].t), hip.ptr(r["lr_mult"].t), hip.stream())
    adam_update(hip, o, g, tab, lr_dev, r["lr_mult"].t, r["scalars"], 1e-2, 1.0, 1, COUPLED, "rates.chain")
    assert all(b.intact() for b in r.values())
    mult, coef = r["lr_mult"].t.cpu().numpy().astype(np.float64), float(r["scalars"].t.cpu()[1])
    assert mult[3] == 0.0 and coef < 0.03
    g64 = np.nan_to_num(g.t.cpu().numpy().astype(np.float64))
    kw = dict(wd=1e-2, clip=coef, mult=per_elem(mult, numels), coupled=True)
    ref, bound = adam_ref(*prev[:1], g64, *prev[1:], 1, float(lr_dev.cpu()[0]), **kw), adam_bound(*prev[:1], g64, *prev[1:], 1, float(lr_dev.cpu()[0]), **kw)
    for name, want, b in zip(("p", "m", "v"), ref, bound):
        close(o[name].t.cpu().numpy()[mask], want[mask], b[mask], f"rates.chain.{name}")
    frozen = (per_elem(mult, numels) == 0.0) & mask
    assert frozen.sum() == 5 and (o["p"].t.cpu().numpy()[frozen] == prev[0][frozen]).all()


def test_refusals_touch_nothing(hip):
    """Null required pointers, a pointer four bytes off a 16-byte boundary, nchunks = 0, ngroups = 0, flags and statistics that
    do not exist: the error codes come back and nothing is launched.  Fresh moments need no m and v."""
    numels = (9, 5)
    chunks, first, nchunks, _ = table(numels)
    total = slots(numels)[1]
    names = ("p", "g", "m", "v")
    o = {n: Guarded((total,)) for n in names}
    o.update({n + "1": GuardedAt((total,), off=1) for n in names})
    o.update(shadow=Guarded((total,), torch.bfloat16), shadow1=GuardedAt((total,), torch.bfloat16, off=1), partial=Guarded((nchunks, 2)),
             tensor_sumsq=Guarded((2, 2)), scalars=Guarded((2,)), group_stat=Guarded((1,)), lr_mult=Guarded((2,)))
    lr = put(np.array([0.1], np.float32))

    def adam_args(flags, n=nchunks, shadow="shadow", lr_dev=lr, table_=chunks, **swap):
        bufs = [None if swap.get(k, k) is None else hip.ptr(o[swap.get(k, k)].t) for k in names]
        return bufs + [hip.ptr(table_), n, hip.ptr(lr_dev), None, None, BETA1, BETA2, EPS, 0.01, 1.0, 0.1, 0.001, flags, hip.ptr(o[shadow].t), hip.stream()]

    for flags in FLAGS:
        for k in names if not flags & FRESH else ("p", "g"):
            hip.refused(ERR_SHAPE, f"adam_flat flags {flags} {k} null", o, "cswin_adam_flat", *adam_args(flags, **{k: None}))
            hip.refused(ERR_ALIGN, f"adam_flat flags {flags} {k} 4 bytes off", o, "cswin_adam_flat", *adam_args(flags, **{k: k + "1"}))
        hip.refused(ERR_ALIGN, f"adam_flat flags {flags} shadow 2 bytes off", o, "cswin_adam_flat", *adam_args(flags, shadow="shadow1"))
        hip.refused(ERR_SHAPE, f"adam_flat flags {flags} nchunks 0", o, "cswin_adam_flat", *adam_args(flags, n=0))
        hip.refused(ERR_SHAPE, f"adam_flat flags {flags} no table", o, "cswin_adam_flat", *adam_args(flags, table_=None))
        hip.refused(ERR_SHAPE, f"adam_flat flags {flags} no rate", o, "cswin_adam_flat", *adam_args(flags, lr_dev=None))
    for flags in (4, 7, -1):
        hip.refused(ERR_SHAPE, f"adam_flat flags {flags}", o, "cswin_adam_flat", *adam_args(flags))
    gf, gt, go = put(np.array([0, 2], np.int32)), put(np.array([0, 1], np.int32)), put(np.array([0, 0], np.int32))
    outs = ("tensor_sumsq", "scalars", "group_stat", "lr_mult")

    def rate_args(part="partial", n=2, ngroups=1, statistic=0, tables=(gf, gt, go), **swap):
        return ([None if part is None else hip.ptr(o[part].t), hip.ptr(first), n, 1.0, 1.0] + [hip.ptr(t) for t in tables] + [ngroups, statistic, 0.0]
                + [None if swap.get(k, k) is None else hip.ptr(o[k].t) for k in outs] + [hip.stream()])

    hip.refused(ERR_SHAPE, "rate_finalize partial null", o, "cswin_rate_finalize", *rate_args(part=None))
    for k in outs:
        hip.refused(ERR_SHAPE, f"rate_finalize {k} null", o, "cswin_rate_finalize", *rate_args(**{k: None}))
    for i in range(3):
        hip.refused(ERR_SHAPE, f"rate_finalize group table {i} null", o, "cswin_rate_finalize", *rate_args(tables=[None if j == i else t for j, t in enumerate((gf, gt, go))]))
    hip.refused(ERR_SHAPE, "rate_finalize ntensors 0", o, "cswin_rate_finalize", *rate_args(n=0))
    hip.refused(ERR_SHAPE, "rate_finalize ngroups 0", o, "cswin_rate_finalize", *rate_args(ngroups=0))
    hip.refused(ERR_SHAPE, "rate_finalize statistic 2", o, "cswin_rate_finalize", *rate_args(statistic=2))
