"""The TPGM kernels (csrc/tpgm.hip: cswin_tpgm_chunk_stats, cswin_tpgm_finalize, cswin_tpgm_project) called directly on guarded
flat buffers, away from the model's layout: tensors on both sides of the 16-byte body, of a workgroup's 256 threads and of the
16384-element chunk, 1 to 463 tensors, l2 and l1, with and without the gradient, every ratio case in one launch, the projection in
place and into another buffer with and without the bf16 shadow, three consecutive updates on both sides of the clip.  References
and bounds are test_tpgm_host's (float64; the bounds are derived there from the kernels' operations and shown to see the bugs they
are for).  The pad words of the anchor and of the gradient hold NaN, so a kernel that reads one poisons a norm or a dot; those of
every written flat buffer hold sentinels that must survive bit for bit."""
import numpy as np
import pytest
import torch

from test_adamw_host import LAYOUT, cdiv, elem_mask, flat, slots
from test_gpu_step_tail import (ERR_ALIGN, ERR_SHAPE, Guarded, GuardedAt, bits16, bits32, close, hip, put, release_inputs,  # noqa: F401
                                rne_bf16)
from test_tpgm_host import (EXCLUDED, HEAD, RATIO_CASES, case_setup, cmax_ref, norm_bound, norms_ref, project_bound, project_ref, ratio_bound,
                            ratios_ref, tpgm_inputs, update_ref)

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD_P, PAD_DST, PAD_SHADOW = 7.0, -5.0, -3.0
LR = 0.05
TENSOR_COUNTS = (1, 257, 463)            # the finalize kernel's second trip starts at 257; 463 is the model's count


def table(numels):
    """(device chunk table, device first_chunk, chunk count, chunks per tensor) of a layout."""
    from cswin_unet_amd.optim import chunk_table
    rows, first = chunk_table(numels, slots(numels)[0])
    return put(rows.view(np.int64).reshape(-1, 2)), put(first), len(rows), np.diff(first)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def flat_buffer(arrays, numels, pad):
    g = Guarded((slots(numels)[1],))
    g.t.copy_(dev(flat(arrays, numels, fill=pad)))
    return g


def flat64(arrays, numels):
    """test_adamw_host.flat in float64 (a reference or a bound must not be rounded to float32), pad words 0."""
    offs, total = slots(numels)
    out = np.zeros(total, np.float64)
    for a, o in zip(arrays, offs):
        out[o:o + np.asarray(a).size] = a
    return out


class State:
    """The guarded buffers of one layout: p (sentinel pads), anchor and g (NaN pads), the per-tensor arrays and the partials."""

    def __init__(self, numels, thetas, anchors, gamma, flags):
        self.numels, self.T = numels, len(numels)
        self.tab = table(numels)
        self.mask = elem_mask(numels)
        self.p = flat_buffer(thetas, numels, PAD_P)
        self.anchor = flat_buffer(anchors, numels, float("nan"))
        self.flags = put(np.asarray(flags, np.int32))
        self.o = dict(partial=Guarded((self.tab[2], 2)), gamma=Guarded((self.T,)), gm=Guarded((self.T,)), gv=Guarded((self.T,)), ratio=Guarded((self.T,)),
                      norm=Guarded((self.T,)), scalars=Guarded((2,)))
        self.o["gamma"].t.copy_(dev(np.asarray(gamma, np.float32)))
        self.o["gm"].t.zero_()
        self.o["gv"].t.zero_()

    def host(self, name):
        return self.o[name].t.cpu().numpy().copy()

    def stats(self, hip, g, l1, p=None):
        chunks, _, nchunks, _ = self.tab
        hip.call("cswin_tpgm_chunk_stats", hip.ptr(self.p.t if p is None else p), hip.ptr(self.anchor.t), None if g is None else hip.ptr(g.t), hip.ptr(chunks),
                 nchunks, int(l1), hip.ptr(self.o["partial"].t), hip.stream())

    def finalize(self, hip, l1, mode, grad_scale=1.0, step=1, with_moments=True):
        o = self.o
        hip.call("cswin_tpgm_finalize", hip.ptr(o["partial"].t), hip.ptr(self.tab[1]), self.T, int(l1), hip.ptr(self.flags), hip.ptr(o["gamma"].t),
                 hip.ptr(o["gm"].t) if with_moments else None, hip.ptr(o["gv"].t) if with_moments else None, float(grad_scale), LR, 1 - 0.9 ** step,
                 1 - 0.999 ** step, mode, hip.ptr(o["ratio"].t), hip.ptr(o["norm"].t), hip.ptr(o["scalars"].t) if with_moments else None, hip.stream())

    def settled(self, what, *more):
        torch.cuda.synchronize()
        for name, b in list(self.o.items()) + [("p", self.p), ("anchor", self.anchor)] + [(f"extra{i}", b) for i, b in enumerate(more)]:
            assert b.intact(), f"{what}: a guard word of {name} was overwritten"
        assert (bits32(self.p.t)[~self.mask] == np.float32(PAD_P).view(np.uint32)).all(), f"{what}: a pad word of p changed"


def setup(tag, numels, l1, identical=False, spread=0.05):
    thetas, anchors, gs = tpgm_inputs(tag, numels, identical=identical, spread=spread)
    gamma, flags = case_setup(norms_ref(thetas, anchors, l1))
    return thetas, anchors, gs, gamma, flags


def check_ratios(st, thetas, anchors, gamma, flags, l1, what):
    """norm[] and ratio[] of a mode-0 launch against float64; returns the float64 (ratio, live, q)."""
    norms = norms_ref(thetas, anchors, l1)
    nb = np.array([norm_bound(x, n, c, l1) for x, n, c in zip(norms, st.numels, st.tab[3])])
    close(st.host("norm"), norms, nb[:, 0], what + ".norm")
    ratio, live, q = ratios_ref(gamma, norms, flags)
    br = ratio_bound(ratio, q, nb[:, 1], flags)
    got = st.host("ratio")
    close(got, ratio, br, what + ".ratio")
    assert (got[br == 0] == ratio[br == 0]).all(), what                 # saturated or excluded: exactly 1
    return ratio, live, q


def cases_present(gamma, norms, flags):
    """Which of RATIO_CASES a launch holds, by their properties."""
    ratio, live, q = ratios_ref(gamma, norms, flags)
    cmax, excl, head = cmax_ref(norms, flags), (flags & EXCLUDED) != 0, (flags & HEAD) != 0
    return {"below": bool((live & (ratio < 1)).any()), "one": bool((~excl & (q > 1) & (gamma <= cmax) & (gamma >= 1e-2)).any()),
            "low": bool((~excl & (gamma < 1e-2)).any()), "high": bool((~excl & (gamma > cmax)).any()), "excluded": bool(excl.any()),
            "head": bool((head & (gamma > np.maximum(8 * norms, 80.0)) & (gamma <= cmax)).any())}


def three_updates(hip, numels, tag, l1, clip, grad_scale, spread=0.05):
    """Three updates on one layout, each compared with update_ref from the state the kernel had and held to the coefficient the
    kernel formed (which is checked by itself)."""
    thetas, anchors, gs, gamma, flags = setup(tag, numels, l1, spread=spread)
    st = State(numels, thetas, anchors, gamma, flags)
    assert all(cases_present(gamma.astype(np.float64), norms_ref(thetas, anchors, l1), flags).values()) or len(numels) < 6
    # <g, d / norm> is some 0.5 per live tensor in l2 and 0.005 in l1 (a large tensor): far above 1 with the clip, far below without
    scale = np.float32(((4000.0 if l1 else 40.0) if clip else 0.1) / grad_scale)
    for k in range(3):
        what = f"tpgm.{tag}.{'l1' if l1 else 'l2'}.{'clip' if clip else 'noclip'}.gs{grad_scale}.step{k + 1}"
        grads = [(g * scale).astype(np.float32) for g in gs[k]]
        g = flat_buffer(grads, numels, float("nan"))
        before = {n: st.host(n).astype(np.float64) for n in ("gamma", "gm", "gv")}
        st.stats(hip, g, l1)
        st.finalize(hip, l1, 1, grad_scale, k + 1)
        st.settled(what, g)
        sc = st.host("scalars")
        free = update_ref(thetas, anchors, grads, before["gamma"], before["gm"], before["gv"], flags, l1, grad_scale, k + 1, float(np.float32(LR)), st.tab[3])
        print(what, "gnorm, coef", sc, "float64", free["gnorm"][0], free["coef"][0], "live", int(free["live"].sum()))
        close(sc[:1], [free["gnorm"][0]], [free["gnorm"][1]], what + ".gnorm")
        (gnorm, bG), (coef, bcoef) = free["gnorm"], free["coef"]
        if coef == 1.0 and 1.0 / (gnorm + bG + 1e-6) > 1.0:
            assert sc[1] == 1.0, (what, sc)                              # clamped on both sides: exactly 1
        else:
            close(sc[1:], [coef], [bcoef], what + ".coef")
        assert len(numels) < 6 or (coef < 1.0) == clip, (what, coef)        # a single tensor's gradient may be one of the 1e-6 ones
        ref = update_ref(thetas, anchors, grads, before["gamma"], before["gm"], before["gv"], flags, l1, grad_scale, k + 1, float(np.float32(LR)), st.tab[3],
                         coef=float(sc[1]))
        for name, key in (("norm", "norm"), ("gamma", "gamma"), ("gm", "m"), ("gv", "v"), ("ratio", "ratio")):
            close(st.host(name), ref[key][0], ref[key][1], f"{what}.{name}")
        excl = (flags & EXCLUDED) != 0
        for name in ("gamma", "gm", "gv"):
            assert (st.host(name)[excl] == before[name][excl]).all(), f"{what}: an excluded {name} moved"
        assert (st.host("ratio")[excl] == 1.0).all(), what
        assert np.isfinite(st.host("partial")).all(), what
    return st


@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
@pytest.mark.parametrize("l1", [False, True], ids=["l2", "l1"])
def test_three_updates_vs_float64(hip, l1, clip):
    """The ten-tensor layout, every ratio case in each launch, gradient scales 1 and 0.5; the gradients are sized so that the norm
    of dL/dgamma lies above 1 (clip) or below it."""
    assert LAYOUT == (1, 3, 4, 5, 1023, 1027, 16383, 16384, 16385, 3 * 16384 + 5) and len(RATIO_CASES) == 6
    for grad_scale in (1.0, 0.5):
        st = three_updates(hip, LAYOUT, "layout", l1, clip, grad_scale)
        assert list(st.tab[3]) == [cdiv(n, 16384) for n in LAYOUT] and st.tab[2] == 14


@pytest.mark.parametrize("ntensors", TENSOR_COUNTS)
def test_one_element_tensors(hip, ntensors):
    """T one-element tensors (eight-float slots, seven pad words each): every per-tensor sum is one term, the finalize kernel takes a
    second trip from T = 257 on, and the gradient norm is added over all of them by one thread."""
    st = three_updates(hip, (1,) * ntensors, f"T{ntensors}", False, True, 1.0, spread=1.0)
    assert st.tab[2] == ntensors


@pytest.mark.parametrize("l1", [False, True], ids=["l2", "l1"])
def test_ratios_and_projection(hip, l1):
    """Mode 0 without a gradient (only the first column of partial is written; the moments and scalars are not needed), then the
    projection by the ratios the kernel wrote: in place and into another buffer, with and without the shadow.  Ratio-1 tensors
    keep src's bits: copied, or (in place) not stored at all, their shadow included."""
    numels = LAYOUT
    thetas, anchors, _, gamma, flags = setup("proj", numels, l1)
    st = State(numels, thetas, anchors, gamma, flags)
    what = f"tpgm.proj.{'l1' if l1 else 'l2'}"
    assert all(cases_present(gamma.astype(np.float64), norms_ref(thetas, anchors, l1), flags).values())
    st.stats(hip, None, l1)
    st.finalize(hip, l1, 0, with_moments=False)
    st.settled(what)
    partial = st.host("partial")
    assert np.isnan(partial[:, 1]).all() and np.isfinite(partial[:, 0]).all(), what
    assert np.array_equal(st.host("gamma"), gamma) and np.isnan(st.host("scalars")).all()
    check_ratios(st, thetas, anchors, gamma.astype(np.float64), flags, l1, what)
    r_dev = st.host("ratio")
    one = np.concatenate([np.full((n + 7) // 8 * 8, r == 1.0) for n, r in zip(numels, r_dev)]) & st.mask
    assert one.any() and (st.mask & ~one).any()
    want = flat64(project_ref(thetas, anchors, r_dev.astype(np.float64)), numels)
    bound = flat64([project_bound(p, a, float(r), 0.0) for p, a, r in zip(thetas, anchors, r_dev)], numels)
    src_bits = bits32(st.p.t).copy()
    chunks, _, nchunks, _ = st.tab
    total = slots(numels)[1]
    for shadow in (False, True):
        # into another buffer
        dst = Guarded((total,))
        dst.t.fill_(PAD_DST)
        sh = Guarded((total,), torch.bfloat16)
        sh.t.fill_(PAD_SHADOW)
        hip.call("cswin_tpgm_project", hip.ptr(st.p.t), hip.ptr(st.anchor.t), hip.ptr(dst.t), hip.ptr(st.o["ratio"].t), hip.ptr(chunks), nchunks,
                 hip.ptr(sh.t) if shadow else None, hip.stream())
        st.settled(f"{what}.copy.shadow{shadow}", dst, sh)
        got = dst.t.cpu().numpy()
        close(got[st.mask], want[st.mask], bound[st.mask], f"{what}.copy.shadow{shadow}")
        assert (got[~st.mask] == PAD_DST).all(), "a pad word of dst was written"
        assert (bits32(dst.t)[one] == src_bits[one]).all(), "a ratio-1 tensor was not copied bit for bit"
        assert (bits32(st.p.t) == src_bits).all(), "src was written"
        want16, nan = rne_bf16(bits32(dst.t))
        pad16 = bits16(torch.tensor([PAD_SHADOW], dtype=torch.bfloat16))[0]
        if shadow:
            assert not nan[st.mask].any() and (bits16(sh.t)[st.mask] == want16[st.mask]).all() and (bits16(sh.t)[~st.mask] == pad16).all()
        else:
            assert (bits16(sh.t) == pad16).all()
        # in place, on a copy of p with its sentinels
        inp = Guarded((total,))
        inp.t.copy_(st.p.t)
        sh = Guarded((total,), torch.bfloat16)
        sh.t.fill_(PAD_SHADOW)
        hip.call("cswin_tpgm_project", hip.ptr(inp.t), hip.ptr(st.anchor.t), hip.ptr(inp.t), hip.ptr(st.o["ratio"].t), hip.ptr(chunks), nchunks,
                 hip.ptr(sh.t) if shadow else None, hip.stream())
        st.settled(f"{what}.inplace.shadow{shadow}", inp, sh)
        assert (bits32(inp.t)[~(st.mask & ~one)] == src_bits[~(st.mask & ~one)]).all(), "in place: a ratio-1 tensor or a pad word changed"
        assert (bits32(inp.t)[st.mask & ~one] == bits32(dst.t)[st.mask & ~one]).all(), "in place and copied projections differ"
        moved = st.mask & ~one
        if shadow:
            assert (bits16(sh.t)[moved] == want16[moved]).all() and (bits16(sh.t)[~moved] == pad16).all(), "in place: the shadow of a kept tensor was stored"
        else:
            assert (bits16(sh.t) == pad16).all()


@pytest.mark.parametrize("l1", [False, True], ids=["l2", "l1"])
def test_identical_parameters(hip, l1):
    """p == anchor: every norm is exactly 0, every ratio exactly 1, the dot and with it every gradient 0, the clip coefficient 1, and
    no gamma moves (their moments are 0); the projection stores nothing in place."""
    numels = LAYOUT
    thetas, anchors, gs, _, _ = setup("same", numels, l1, identical=True)
    gamma = np.full(len(numels), 3.0, np.float32)
    flags = np.array([0, HEAD, EXCLUDED, 0, 0, HEAD, 0, 0, 0, 0], np.int32)
    st = State(numels, thetas, anchors, gamma, flags)
    g = flat_buffer(gs[0], numels, float("nan"))
    st.stats(hip, g, l1)
    st.finalize(hip, l1, 1, 1.0, 1)
    st.settled("tpgm.same", g)
    assert (st.host("norm") == 0).all() and (st.host("ratio") == 1).all() and (st.host("partial") == 0).all()
    assert np.array_equal(st.host("scalars"), np.array([0.0, 1.0], np.float32))
    assert np.array_equal(st.host("gamma"), gamma) and (st.host("gm") == 0).all() and (st.host("gv") == 0).all()
    before = bits32(st.p.t).copy()
    hip.call("cswin_tpgm_project", hip.ptr(st.p.t), hip.ptr(st.anchor.t), hip.ptr(st.p.t), hip.ptr(st.o["ratio"].t), hip.ptr(st.tab[0]), st.tab[2], None,
             hip.stream())
    st.settled("tpgm.same.project")
    assert (bits32(st.p.t) == before).all()


def test_two_runs_give_the_same_bits(hip):
    """No float atomics: every sum has a fixed order."""
    runs = []
    for _ in range(2):
        numels = LAYOUT
        thetas, anchors, gs, gamma, flags = setup("bits", numels, False)
        st = State(numels, thetas, anchors, gamma, flags)
        g = flat_buffer([(x * np.float32(40)).astype(np.float32) for x in gs[0]], numels, float("nan"))
        st.stats(hip, g, False)
        st.finalize(hip, False, 1, 0.5, 1)
        dst = Guarded((slots(numels)[1],))
        dst.t.fill_(PAD_DST)
        sh = Guarded((slots(numels)[1],), torch.bfloat16)
        sh.t.fill_(PAD_SHADOW)
        hip.call("cswin_tpgm_project", hip.ptr(st.p.t), hip.ptr(st.anchor.t), hip.ptr(dst.t), hip.ptr(st.o["ratio"].t), hip.ptr(st.tab[0]), st.tab[2],
                 hip.ptr(sh.t), hip.stream())
        st.settled("tpgm.bits", g, dst, sh)
        runs.append([bits32(st.o[n].t) for n in ("partial", "gamma", "gm", "gv", "ratio", "norm", "scalars")] + [bits32(dst.t), bits16(sh.t)])
    assert all(np.array_equal(a, b) for a, b in zip(*runs))


def test_refusals_touch_nothing(hip):
    """A null buffer, a pointer four bytes off a 16-byte boundary, no chunks, no tensors and an unknown mode return their error
    codes; nothing is launched."""
    numels = (9, 5)
    chunks, first, nchunks, _ = table(numels)
    total = slots(numels)[1]
    flags = put(np.zeros(2, np.int32))
    names = ("p", "anchor", "g", "dst")
    o = {n: Guarded((total,)) for n in names}
    o.update({n + "1": GuardedAt((total,), off=1) for n in names})
    o.update(shadow=Guarded((total,), torch.bfloat16), shadow1=GuardedAt((total,), torch.bfloat16, off=1), partial=Guarded((nchunks, 2)))
    o.update({n: Guarded((2,)) for n in ("gamma", "gm", "gv", "ratio", "norm", "scalars")})
    P = lambda k: None if k is None else hip.ptr(o[k].t)

    def stats(p="p", anchor="anchor", g="g", n=nchunks, part="partial", tab=chunks):
        return P(p), P(anchor), P(g), hip.ptr(tab), n, 0, P(part), hip.stream()

    for k in ("p", "anchor"):
        hip.refused(ERR_SHAPE, f"chunk_stats {k} null", o, "cswin_tpgm_chunk_stats", *stats(**{k: None}))
    for k in ("p", "anchor", "g"):
        hip.refused(ERR_ALIGN, f"chunk_stats {k} 4 bytes off", o, "cswin_tpgm_chunk_stats", *stats(**{k: k + "1"}))
    hip.refused(ERR_SHAPE, "chunk_stats partial null", o, "cswin_tpgm_chunk_stats", *stats(part=None))
    hip.refused(ERR_SHAPE, "chunk_stats nchunks 0", o, "cswin_tpgm_chunk_stats", *stats(n=0))
    hip.refused(ERR_SHAPE, "chunk_stats no table", o, "cswin_tpgm_chunk_stats", *stats(tab=None))

    def fin(part="partial", fc=first, T=2, fl=flags, gamma="gamma", gm="gm", gv="gv", mode=1, ratio="ratio", norm="norm", sc="scalars", bc1=0.1, bc2=0.001):
        return P(part), hip.ptr(fc), T, 0, hip.ptr(fl), P(gamma), P(gm), P(gv), 1.0, LR, bc1, bc2, mode, P(ratio), P(norm), P(sc), hip.stream()

    for k, kw in (("partial", dict(part=None)), ("first_chunk", dict(fc=None)), ("flags", dict(fl=None)), ("gamma", dict(gamma=None)), ("ratio", dict(ratio=None)),
                  ("norm", dict(norm=None)), ("gm", dict(gm=None)), ("gv", dict(gv=None)), ("scalars", dict(sc=None)), ("ntensors 0", dict(T=0)),
                  ("mode 2", dict(mode=2)), ("bc1 0", dict(bc1=0.0)), ("bc2 0", dict(bc2=0.0))):
        hip.refused(ERR_SHAPE, f"finalize {k}", o, "cswin_tpgm_finalize", *fin(**kw))

    def proj(src="p", anchor="anchor", dst="dst", ratio="ratio", n=nchunks, shadow="shadow", tab=chunks):
        return P(src), P(anchor), P(dst), P(ratio), hip.ptr(tab), n, P(shadow), hip.stream()

    for k in ("src", "anchor", "dst", "ratio"):
        hip.refused(ERR_SHAPE, f"project {k} null", o, "cswin_tpgm_project", *proj(**{k: None}))
    for k, v in (("src", "p1"), ("anchor", "anchor1"), ("dst", "dst1"), ("shadow", "shadow1")):
        hip.refused(ERR_ALIGN, f"project {k} off its boundary", o, "cswin_tpgm_project", *proj(**{k: v}))
    hip.refused(ERR_SHAPE, "project nchunks 0", o, "cswin_tpgm_project", *proj(n=0))
    hip.refused(ERR_SHAPE, "project no table", o, "cswin_tpgm_project", *proj(tab=None))


@pytest.mark.parametrize("kind", ["adamw", "sgd"])
def test_flat_tpgm_over_both_optimisers(monkeypatch, kind):
    """optim.FlatTPGM on small parameters: it walks the optimiser's own chunk table, FlatAdamW's or FlatSGD's; the initial radii
    follow the init rule; begin() ... end() restores bit for bit; an excluded tensor and one inside its ball are never stored;
    update() outside begin() and inside a stream capture is refused and leaves the step count alone."""
    from cswin_unet_amd.optim import FlatAdamW, FlatSGD, FlatTPGM, chunk_table
    numels = (5, 1027, 16385, 9)
    names = ["stage1.0.qkv.weight", "stage1.0.qkv.bias", "output.weight", "norm.weight"]
    thetas, anchors, gs = tpgm_inputs("object", numels, spread=1.0)
    params = [torch.nn.Parameter(dev(a)) for a in anchors]
    opt = FlatAdamW(params, lr=1e-3) if kind == "adamw" else FlatSGD(params, lr=1e-3)
    tp = FlatTPGM(opt, names, proj_lr=LR, exclude=("stage1.0.qkv.bias",))
    rows, first = chunk_table(list(numels), opt.offsets)
    assert tp.chunks is opt.chunks and tp.first_chunk is opt.first_chunk
    assert tp.nchunks == opt.nchunks == len(rows) and np.array_equal(tp.chunks.cpu().numpy(), rows.view(np.int64).reshape(-1, 2)) and \
        np.array_equal(tp.first_chunk.cpu().numpy(), first)
    assert tp.flags_host == [0, EXCLUDED, HEAD, 0]
    pn = norms_ref(anchors, [np.zeros(n) for n in numels], False)
    want = np.array([max(3.0, 2 * pn[0]), max(3.0, 2 * pn[1]), max(10.0, 5 * pn[2]), max(3.0, 2 * pn[3])])
    close(tp.gamma.cpu().numpy(), want, 1e-5 * want, "tpgm.object.gamma0")          # float32 norms of at most 16385 elements: some 30 roundings
    assert tuple(tp.ratio_stats()) == (1.0, 1.0, 1.0) and tp.ratio_stats().mean == 1.0
    with torch.no_grad():
        for p, v in zip(params, thetas):
            p.copy_(dev(v))
    norms = tp.tensor_norms().cpu().numpy()
    close(norms, norms_ref(thetas, anchors, False), 1e-5 * norms, "tpgm.object.norms")
    tp.set_constraints({"stage1.0.qkv.weight": 0.5 * float(norms[0]), "output.weight": 0.25 * float(norms[2])})      # the others keep their wide radii
    keep = bits32(opt.flat_param).copy()
    with pytest.raises(RuntimeError, match="outside begin"):
        tp.update(1.0)
    tp.begin()
    with pytest.raises(RuntimeError, match="already begun"):
        tp.begin()
    inside = bits32(opt.flat_param).copy()
    offs = opt.offsets
    moved = [bool((inside[o:o + n] != keep[o:o + n]).any()) for o, n in zip(offs, numels)]
    assert moved == [True, False, True, False]
    stats = tp.ratio_stats()
    assert abs(stats.min - 0.25) < 1e-6 and stats.max == 1.0 and abs(stats.mean - (0.5 + 0.25 + 1.0) / 3) < 1e-6     # the excluded tensor is left out
    for p, g in zip(params, gs[0]):
        p.grad = dev(g)
    opt.gather_grads()
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="capture"):
        tp.update(1.0)
    monkeypatch.undo()
    assert tp.step_count == 0
    g0 = tp.gamma.clone()
    tp.update(1.0)
    tp.reproject()
    assert tp.step_count == 1 and not torch.equal(tp.gamma[0], g0[0]) and not torch.equal(tp.gamma[2], g0[2]) and torch.equal(tp.gamma[[1, 3]], g0[[1, 3]])
    with pytest.raises(RuntimeError, match="between begin"):
        tp.apply()
    tp.end()
    tp.end()                                                            # a second end() is nothing
    assert (bits32(opt.flat_param) == keep).all()
    sd = tp.state_dict()
    assert sd["step"] == 1 and torch.equal(sd["gamma"], tp.gamma) and torch.equal(sd["anchor"], tp.flat_anchor)
    with pytest.raises(ValueError):
        tp.set_constraints([1.0, 2.0])
    with pytest.raises(KeyError):
        tp.set_constraints({"nothing": 1.0})


def test_flat_tpgm_keeps_the_bf16_shadow_in_the_bf16_mode():
    """In the bf16 matmul mode the projection writes the shadow the Linears read, and end() restores it bit for bit."""
    from cswin_unet_amd import _lib
    from cswin_unet_amd.optim import FlatSGD, FlatTPGM
    numels = (5, 1027, 16385)
    thetas, anchors, _ = tpgm_inputs("shadow", numels, spread=1.0)
    params = [torch.nn.Parameter(dev(a)) for a in anchors]
    opt = FlatSGD(params, lr=1e-3)
    tp = FlatTPGM(opt, ["a.weight", "b.weight", "c.weight"], proj_lr=LR)
    prev = _lib.set_precision(_lib.PREC_BF16)
    try:
        with torch.no_grad():
            for p, v in zip(params, thetas):
                p.copy_(dev(v))
        opt.refresh_shadow()
        norms = tp.tensor_norms().cpu().numpy()
        tp.set_constraints([0.5 * float(norms[0]), 1e3, 0.25 * float(norms[2])])
        keep, keep16 = bits32(opt.flat_param).copy(), bits16(opt.flat_param16).copy()
        tp.begin()
        assert (bits32(opt.flat_param) != keep).any() and torch.equal(opt.flat_param16, opt.flat_param.to(torch.bfloat16))
        o, n = opt.offsets[1], numels[1]
        assert (bits32(opt.flat_param)[o:o + n] == keep[o:o + n]).all() and (bits16(opt.flat_param16)[o:o + n] == keep16[o:o + n]).all()
        tp.end()
        assert (bits32(opt.flat_param) == keep).all() and (bits16(opt.flat_param16) == keep16).all()
        tp.apply()
        assert (bits32(opt.flat_param) != keep).any() and torch.equal(opt.flat_param16, opt.flat_param.to(torch.bfloat16))
    finally:
        _lib.set_precision(prev)
