"""The consolidation kernels (csrc/consolidate.hip: cswin_consolidate_chunks, cswin_consolidate_finalize, cswin_importance_accumulate,
cswin_flat_axpby) called directly on guarded flat buffers, away from the model's layout: tensors on both sides of the 16-byte body,
of a workgroup's 256 threads and of the 16384-element chunk, 1 to 463 tensors, the importance present and null, the gradient present
and null, penalty scales 1, 2 and 8, tensor weights 0 and 1 in one launch.  References and bounds are test_consolidate_host's
(float64; the bounds are derived there from the kernels' operations and shown to see the bugs they are for).  The pad words of every
flat buffer a kernel only reads hold NaN, so a kernel that reads one poisons a sum; those of every written flat buffer hold
sentinels that must survive bit for bit."""
import numpy as np
import pytest
import torch

from test_adamw_host import LAYOUT, cdiv, elem_mask, flat, slots
from test_consolidate_host import (accumulate_bound, axpby_bound, cons_inputs, dd_sum_bound, fd_sum_bound, grad_bound, importance_ref,
                                   mixed_weights, penalty_ref, scalar_bounds)
from test_gpu_step_tail import ERR_ALIGN, ERR_SHAPE, Guarded, GuardedAt, bits32, close, hip, put, release_inputs  # noqa: F401
from test_gpu_tpgm import TENSOR_COUNTS, dev, flat64, flat_buffer, table

pytestmark = pytest.mark.gpu
PAD_G, PAD_IMP = -5.0, 7.0
NAN = float("nan")
LAM = 0.37
LAYOUTS = {"layout": LAYOUT, **{f"T{n}": (1,) * n for n in TENSOR_COUNTS}}


class Case:
    """One layout's inputs, float64 reference (penalty scale 1) and device buffers; p, anchor and the importance have NaN pads."""

    def __init__(self, name, with_imp, tw=None):
        self.numels = numels = LAYOUTS[name]
        self.T = len(numels)
        self.thetas, self.anchors, imps, self.gs = cons_inputs(name, numels, spread=1.0 if numels[0] == 1 and self.T > 1 else 0.05)
        self.imps = imps if with_imp else None
        self.tw = mixed_weights(self.T) if tw is None else tw
        self.chunks, self.first, self.nchunks, self.per_tensor_chunks = table(numels)
        self.mask = elem_mask(numels)
        self.p = flat_buffer(self.thetas, numels, NAN)
        self.anchor = flat_buffer(self.anchors, numels, NAN)
        self.imp = flat_buffer(self.imps, numels, NAN) if with_imp else None
        self.tw_dev = put(self.tw)
        self.lam = put(np.array([LAM], np.float32))
        self.lam32 = float(np.float32(LAM))
        self.ref = penalty_ref(self.thetas, self.anchors, self.imps, self.lam32, self.tw)
        self.o = dict(partial=Guarded((self.nchunks, 2)), per_tensor=Guarded((self.T, 2)), scalars=Guarded((3,)))

    def run(self, hip, g, penalty_scale=1.0, lam=None, p=None):
        hip.call("cswin_consolidate_chunks", hip.ptr(self.p.t if p is None else p.t), hip.ptr(self.anchor.t), None if self.imp is None else hip.ptr(self.imp.t),
                 None if g is None else hip.ptr(g.t), hip.ptr(self.chunks), self.nchunks, hip.ptr(self.lam if lam is None else lam), hip.ptr(self.tw_dev),
                 float(penalty_scale), hip.ptr(self.o["partial"].t), hip.stream())
        hip.call("cswin_consolidate_finalize", hip.ptr(self.o["partial"].t), hip.ptr(self.first), self.T, hip.ptr(self.lam if lam is None else lam),
                 hip.ptr(self.tw_dev), hip.ptr(self.o["per_tensor"].t), hip.ptr(self.o["scalars"].t), hip.stream())

    def host(self, name):
        return self.o[name].t.cpu().numpy().copy()

    def settled(self, what, g=None, *more):
        torch.cuda.synchronize()
        bufs = list(self.o.items()) + [("p", self.p), ("anchor", self.anchor)] + ([("imp", self.imp)] if self.imp is not None else [])
        for name, b in bufs + ([("g", g)] if g is not None else []) + [(f"extra{i}", b) for i, b in enumerate(more)]:
            assert b.intact(), f"{what}: a guard word of {name} was overwritten"
        if g is not None:
            assert (bits32(g.t)[~self.mask] == np.float32(PAD_G).view(np.uint32)).all(), f"{what}: a pad word of g changed"

    def check_sums(self, what, lam_ratio=1.0):
        ref, nch = self.ref, self.per_tensor_chunks
        per = self.host("per_tensor")
        close(per[:, 0], ref["per_tensor"][:, 0], [fd_sum_bound(x, n, c) for x, n, c in zip(ref["abs_fd"], self.numels, nch)], what + ".sum_Fdd")
        close(per[:, 1], ref["per_tensor"][:, 1], [dd_sum_bound(x, n, c) for x, n, c in zip(ref["per_tensor"][:, 1], self.numels, nch)], what + ".sum_dd")
        want = np.array([ref["penalty"] * lam_ratio, ref["weighted"], ref["dist"]])
        close(self.host("scalars"), want, scalar_bounds(ref, self.numels, nch, self.tw) * np.array([lam_ratio, 1.0, 1.0]), what + ".scalars")
        assert np.isfinite(self.host("partial")).all(), what


def grad_buffer(case, k=0, minus_zero=False):
    grads = [g.copy() for g in case.gs[k]]
    if minus_zero:
        for g in grads:
            g[::3] = -0.0
    return grads, flat_buffer(grads, case.numels, PAD_G)


@pytest.mark.parametrize("with_imp", [True, False], ids=["importance", "l2sp"])
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_penalty_gradient_and_sums_vs_float64(hip, name, with_imp):
    """Every penalty scale with the gradient, then the statistics alone (a null gradient): the gradient within grad_bound of
    g + c F d, bit-identical where the tensor's weight is 0, the sums and the three scalars within their bounds."""
    assert LAYOUT == (1, 3, 4, 5, 1023, 1027, 16383, 16384, 16385, 3 * 16384 + 5) and TENSOR_COUNTS == (1, 257, 463)
    case = Case(name, with_imp)
    assert case.T == 1 or {0.0, 1.0} == set(case.tw.tolist())
    add1 = flat64(case.ref["grad"], case.numels)
    off = flat64([np.full(n, w == 0.0) for n, w in zip(case.numels, case.tw)], case.numels).astype(bool)
    for k, ps in enumerate((1.0, 2.0, 8.0)):
        what = f"consolidate.{name}.{'imp' if with_imp else 'l2sp'}.ps{ps:g}"
        grads, g = grad_buffer(case, k)
        before = bits32(g.t).copy()
        case.run(hip, g, ps)
        case.settled(what, g)
        g0 = flat64(grads, case.numels)
        got = g.t.cpu().numpy().astype(np.float64)
        close(got[case.mask], (g0 + ps * add1)[case.mask], grad_bound(ps * add1, g0)[case.mask], what + ".grad")
        assert (bits32(g.t)[off] == before[off]).all(), f"{what}: the gradient of a weight-0 tensor changed"
        assert case.T == 1 or (bits32(g.t)[case.mask & ~off] != before[case.mask & ~off]).any(), what
        case.check_sums(what)
    what = f"consolidate.{name}.{'imp' if with_imp else 'l2sp'}.report"
    for b in case.o.values():
        b.t.fill_(NAN)
    case.run(hip, None)
    case.settled(what)
    case.check_sums(what)


@pytest.mark.parametrize("with_imp", [True, False], ids=["importance", "l2sp"])
def test_a_zero_coefficient_leaves_the_gradients_bits_alone(hip, with_imp):
    """lambda = 0: the whole gradient keeps its bits, the planted -0.0 included (fma(0, t, -0.0) would be +0.0), and the sums are
    still formed.  lambda != 0: the same for the weight-0 tensors, while a -0.0 of a penalised tensor does move."""
    case = Case("layout", with_imp)
    grads, g = grad_buffer(case, 0, minus_zero=True)
    before = bits32(g.t).copy()
    assert (before[case.mask] == 0x80000000).sum() >= sum(cdiv(n, 3) for n in case.numels)
    zero = put(np.zeros(1, np.float32))
    case.run(hip, g, 2.0, lam=zero)
    case.settled("consolidate.lam0", g)
    assert (bits32(g.t) == before).all()
    sc = case.host("scalars")
    assert sc[0] == 0.0 and sc[1] > 0 and sc[2] > 0
    case.check_sums("consolidate.lam0", lam_ratio=0.0)
    case.run(hip, g, 2.0)
    case.settled("consolidate.lam", g)
    off = flat64([np.full(n, w == 0.0) for n, w in zip(case.numels, case.tw)], case.numels).astype(bool)
    after = bits32(g.t)
    assert (after[off] == before[off]).all() and (before[off] == 0x80000000).any()
    on = case.mask & ~off
    assert (after[on] != before[on]).mean() > 0.5


def test_lambda_scales_the_penalty_alone_and_two_runs_give_the_same_bits(hip):
    case = Case("layout", True)
    grads, g = grad_buffer(case, 1)
    case.run(hip, g, 2.0)
    case.settled("consolidate.first", g)
    first = {n: bits32(case.o[n].t).copy() for n in case.o}
    first_g = bits32(g.t).copy()
    _, g2 = grad_buffer(case, 1)
    for b in case.o.values():
        b.t.fill_(NAN)
    case.run(hip, g2, 2.0)
    case.settled("consolidate.second", g2)
    assert (bits32(g2.t) == first_g).all() and all((bits32(case.o[n].t) == first[n]).all() for n in case.o)
    double = put(np.array([2 * np.float32(LAM)], np.float32))
    sc1 = case.host("scalars")
    case.run(hip, None, 1.0, lam=double)
    case.settled("consolidate.doubled")
    sc2 = case.host("scalars")
    assert sc2[0] == 2 * sc1[0] and sc1[0] > 0
    assert (bits32(case.o["scalars"].t)[1:] == first["scalars"][1:]).all() and (bits32(case.o["per_tensor"].t) == first["per_tensor"]).all()


def test_an_inf_in_the_parameters_is_reported(hip):
    """An inf in one tensor: its sums, the penalty and the distance are not finite; every other tensor's sums keep their bits and
    no guard word changes."""
    case = Case("layout", True)
    case.run(hip, None)
    case.settled("consolidate.finite")
    clean = bits32(case.o["per_tensor"].t).copy()
    t_bad = 5
    assert case.tw[t_bad] == 1.0
    thetas = [p.copy() for p in case.thetas]
    thetas[t_bad][7] = np.inf
    assert case.imps[t_bad][7] > 0.0
    p_bad = flat_buffer(thetas, case.numels, NAN)
    grads, g = grad_buffer(case, 0)
    case.run(hip, g, 1.0, p=p_bad)
    case.settled("consolidate.inf", g, p_bad)
    per, sc = case.host("per_tensor"), case.host("scalars")
    assert not np.isfinite(per[t_bad]).any() and not np.isfinite(sc[0]) and not np.isfinite(sc[2])
    others = np.arange(case.T) != t_bad
    assert (bits32(case.o["per_tensor"].t).reshape(-1, 2)[others] == clean.reshape(-1, 2)[others]).all()


@pytest.mark.parametrize("statistic", [0, 1], ids=["squares", "abs"])
@pytest.mark.parametrize("grad_scale", [1.0, 0.125])
def test_importance_accumulate_three_batches_vs_float64(hip, statistic, grad_scale):
    numels = LAYOUT
    _, _, _, gs = cons_inputs("acc", numels)
    chunks, _, nchunks, _ = table(numels)
    mask = elem_mask(numels)
    imp = flat_buffer([np.zeros(n, np.float32) for n in numels], numels, PAD_IMP)
    what = f"importance_accumulate.{'abs' if statistic else 'squares'}.gs{grad_scale:g}"
    for k in range(3):
        g = flat_buffer(gs[k], numels, NAN)
        hip.call("cswin_importance_accumulate", hip.ptr(g.t), hip.ptr(imp.t), hip.ptr(chunks), nchunks, grad_scale, statistic, hip.stream())
        torch.cuda.synchronize()
        assert g.intact() and imp.intact(), what
        total = flat64([importance_ref([gs[j][t] for j in range(k + 1)], statistic, grad_scale, count=1) for t in range(len(numels))], numels)
        got = imp.t.cpu().numpy()
        assert (bits32(imp.t)[~mask] == np.float32(PAD_IMP).view(np.uint32)).all(), f"{what}: a pad word of the importance changed"
        close(got[mask], total[mask], accumulate_bound(total, k + 1, statistic)[mask], f"{what}.batch{k + 1}")
    assert (got[mask] >= 0).all() and got[mask].max() > 0


@pytest.mark.parametrize("with_src", [True, False], ids=["src", "scale_only"])
def test_flat_axpby_vs_float64(hip, with_src):
    numels = LAYOUT
    _, _, imps, gs = cons_inputs("axpby", numels)
    chunks, _, nchunks, _ = table(numels)
    mask = elem_mask(numels)
    dst = flat_buffer(imps, numels, PAD_IMP)
    src = flat_buffer(gs[0], numels, NAN) if with_src else None
    a, b = 0.9, 1.0 / 3.0
    hip.call("cswin_flat_axpby", hip.ptr(dst.t), None if src is None else hip.ptr(src.t), hip.ptr(chunks), nchunks, a, b, hip.stream())
    torch.cuda.synchronize()
    assert dst.intact() and (src is None or src.intact())
    assert (bits32(dst.t)[~mask] == np.float32(PAD_IMP).view(np.uint32)).all()
    d0, s0 = flat64(imps, numels), flat64(gs[0], numels) if with_src else None
    want = a * d0 + (b * s0 if with_src else 0.0)
    close(dst.t.cpu().numpy()[mask], want[mask], axpby_bound(a, d0, b, s0)[mask], f"flat_axpby.{'src' if with_src else 'scale'}")
    # the exact cases finish() relies on: decay 0 wipes a finite importance, a == 1 with b == 0 keeps it
    keep = bits32(dst.t).copy()
    hip.call("cswin_flat_axpby", hip.ptr(dst.t), None, hip.ptr(chunks), nchunks, 1.0, 0.0, hip.stream())
    assert (bits32(dst.t) == keep).all()
    hip.call("cswin_flat_axpby", hip.ptr(dst.t), None, hip.ptr(chunks), nchunks, 0.0, 0.0, hip.stream())
    assert (dst.t.cpu().numpy()[mask] == 0).all() and dst.intact()


def test_refused_calls_touch_nothing(hip):
    numels = (1027, 5)
    chunks, first, nchunks, _ = table(numels)
    total = slots(numels)[1]
    lam, tw = put(np.ones(1, np.float32)), put(np.ones(2, np.float32))
    names = ("p", "anchor", "imp", "g")
    o = {n: Guarded((total,)) for n in names}
    o.update({n + "1": GuardedAt((total,), off=1) for n in names})
    o.update(partial=Guarded((nchunks, 2)), per_tensor=Guarded((2, 2)), scalars=Guarded((3,)))
    P = lambda k: None if k is None else hip.ptr(o[k].t)

    def chunk(p="p", anchor="anchor", imp="imp", g="g", tab=chunks, n=nchunks, lm=lam, w=tw, part="partial"):
        return P(p), P(anchor), P(imp), P(g), hip.ptr(tab), n, hip.ptr(lm), hip.ptr(w), 1.0, P(part), hip.stream()

    for k in ("p", "anchor"):
        hip.refused(ERR_SHAPE, f"consolidate_chunks {k} null", o, "cswin_consolidate_chunks", *chunk(**{k: None}))
    for k in names:
        hip.refused(ERR_ALIGN, f"consolidate_chunks {k} 4 bytes off", o, "cswin_consolidate_chunks", *chunk(**{k: k + "1"}))
    for k, kw in (("partial null", dict(part=None)), ("nchunks 0", dict(n=0)), ("no table", dict(tab=None)), ("lam null", dict(lm=None)),
                  ("tensor_weight null", dict(w=None))):
        hip.refused(ERR_SHAPE, f"consolidate_chunks {k}", o, "cswin_consolidate_chunks", *chunk(**kw))

    def fin(part="partial", fc=first, T=2, lm=lam, w=tw, per="per_tensor", sc="scalars"):
        return P(part), hip.ptr(fc), T, hip.ptr(lm), hip.ptr(w), P(per), P(sc), hip.stream()

    for k, kw in (("partial", dict(part=None)), ("first_chunk", dict(fc=None)), ("lam", dict(lm=None)), ("tensor_weight", dict(w=None)),
                  ("per_tensor", dict(per=None)), ("scalars", dict(sc=None)), ("ntensors 0", dict(T=0))):
        hip.refused(ERR_SHAPE, f"consolidate_finalize {k}", o, "cswin_consolidate_finalize", *fin(**kw))

    def acc(g="g", imp="imp", tab=chunks, n=nchunks, stat=0):
        return P(g), P(imp), hip.ptr(tab), n, 1.0, stat, hip.stream()

    for k in ("g", "imp"):
        hip.refused(ERR_SHAPE, f"importance_accumulate {k} null", o, "cswin_importance_accumulate", *acc(**{k: None}))
        hip.refused(ERR_ALIGN, f"importance_accumulate {k} 4 bytes off", o, "cswin_importance_accumulate", *acc(**{k: k + "1"}))
    for k, kw in (("nchunks 0", dict(n=0)), ("no table", dict(tab=None)), ("statistic 2", dict(stat=2)), ("statistic -1", dict(stat=-1))):
        hip.refused(ERR_SHAPE, f"importance_accumulate {k}", o, "cswin_importance_accumulate", *acc(**kw))

    def axpby(dst="imp", src="g", tab=chunks, n=nchunks):
        return P(dst), P(src), hip.ptr(tab), n, 0.5, 0.5, hip.stream()

    hip.refused(ERR_SHAPE, "flat_axpby dst null", o, "cswin_flat_axpby", *axpby(dst=None))
    hip.refused(ERR_ALIGN, "flat_axpby dst 4 bytes off", o, "cswin_flat_axpby", *axpby(dst="imp1"))
    hip.refused(ERR_ALIGN, "flat_axpby src 4 bytes off", o, "cswin_flat_axpby", *axpby(src="g1"))
    hip.refused(ERR_SHAPE, "flat_axpby nchunks 0", o, "cswin_flat_axpby", *axpby(n=0))
    hip.refused(ERR_SHAPE, "flat_axpby no table", o, "cswin_flat_axpby", *axpby(tab=None))
