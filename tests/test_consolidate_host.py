"""Host side of the consolidation penalties (csrc/consolidate.hip, optim.FlatConsolidation, continual.Consolidation): the float64
restatement of the penalty, of its gradient and of the importance estimate, and the derived bounds that tests/test_gpu_consolidate*.py
use -- checked here against torch autograd and an explicit per-batch torch loop on the CPU, against an fp32 emulation of the
kernels and against planted bugs.  Also carry_consolidation_state and the option checks.  No GPU."""
import types

import numpy as np
import pytest
import torch

from oracle.determ import det_normal

from test_adamw_host import U, cdiv, sumsq_depth
from test_tpgm_host import chunk_sum_fp32, tpgm_inputs

STATISTICS = {"ewc": 0, "mas": 1}


# ------------------------------------------------------------------------------------------------
# float64 restatement
# ------------------------------------------------------------------------------------------------
def penalty_ref(thetas, anchors, imps, lam, tensor_weight, penalty_scale=1.0):
    """The penalty (lam / 2) sum_t w_t sum F d^2 in float64.  imps None: importance 1.  Returns a dict: penalty, weighted (sum_t w_t
    sum F d^2), dist (sqrt(sum d^2)), per_tensor (T, 2) of (sum F d^2, sum d^2), abs_fd (T,) of sum |F d d|, and grad, per tensor what the
    kernel adds to the flat gradient: lam w_t penalty_scale F d."""
    per, absfd, grad = [], [], []
    for t, (p, a) in enumerate(zip(thetas, anchors)):
        d = np.asarray(p, np.float64) - np.asarray(a, np.float64)
        f = np.ones_like(d) if imps is None else np.asarray(imps[t], np.float64)
        per.append((float((f * d * d).sum()), float((d * d).sum())))
        absfd.append(float(np.abs(f * d * d).sum()))
        grad.append(float(lam) * float(tensor_weight[t]) * float(penalty_scale) * f * d)
    per = np.array(per).reshape(-1, 2)
    weighted = float((np.asarray(tensor_weight, np.float64) * per[:, 0]).sum())
    return dict(penalty=0.5 * float(lam) * weighted, weighted=weighted, dist=float(np.sqrt(per[:, 1].sum())), per_tensor=per,
                abs_fd=np.array(absfd), grad=grad)


def importance_ref(grads_per_batch, statistic, grad_scale=1.0, count=None, decay=0.0, prev=None):
    """decay prev + (1 / count) sum over the batches of (grad_scale g)^2 (statistic 0) or |grad_scale g| (1), in float64; count
    defaults to the number of batches, prev to zeros."""
    acc = None
    for g in grads_per_batch:
        x = float(grad_scale) * np.asarray(g, np.float64)
        s = x * x if statistic == 0 else np.abs(x)
        acc = s if acc is None else acc + s
    count = len(grads_per_batch) if count is None else count
    return (0.0 if prev is None else decay * np.asarray(prev, np.float64)) + acc / count


# ------------------------------------------------------------------------------------------------
# bounds of the fp32 kernels, to first order in U = 2^-24, counted from csrc/consolidate.hip without relying on contraction (an fma
# where two roundings are counted only helps); sqrt at two roundings, as in test_adamw_host
# ------------------------------------------------------------------------------------------------
def grad_bound(added, g):
    """g' = fma(c, t, g), c = fl(fl(lam w) ps), t = fl(F fl(p - a)).  d carries 1, t 1 + 1 = 2; c: the two products and the rounded
    penalty_scale, 3; the product c t 3 + 2 + 1 = 6; the sum U (|g| + |c F d|): 7 U |c F d| + U |g|, and one spare on the first.
    added: the float64 c F d; g: the gradient before.  0 where c is exactly 0 (nothing is stored: the bits stay)."""
    added, g = np.abs(np.asarray(added, np.float64)), np.abs(np.asarray(g, np.float64))
    return np.where(added == 0.0, 0.0, U * (8.0 * added + g))


def fd_sum_bound(abs_fd, numel, nchunks):
    """sum t d over a tensor: t 2, d 1, the product 1, the sum `depth` (test_adamw_host.sumsq_depth: flat_chunks.h's launch rule and
    the tensor's chunks in chunk order), one spare -- against sum |t d|."""
    return (sumsq_depth(numel, nchunks) + 5) * U * np.abs(abs_fd)


def dd_sum_bound(dd, numel, nchunks):
    """sum d^2 over a tensor: d^2 carries 2 + 1, the sum depth, one spare (test_tpgm_host.norm_bound's count)."""
    return (sumsq_depth(numel, nchunks) + 4) * U * np.abs(dd)


def scalar_bounds(ref, numels, nchunks, tensor_weight):
    """Bounds of [penalty, weighted, dist].  weighted = sum_t fl(w_t S_t) in tensor order by one thread: the deepest tensor's bound,
    the product 1, T additions, against sum_t |w_t| sum |F d d|; the penalty one more product (lam / 2 is exact); dist = sqrt(sum
    of the tensors' sum d^2): half the relative bound of the sum and the square root's 2."""
    T = len(numels)
    deepest = max(sumsq_depth(n, c) for n, c in zip(numels, nchunks))
    A = float((np.abs(np.asarray(tensor_weight, np.float64)) * ref["abs_fd"]).sum())
    bw = (deepest + 5 + 1 + T) * U * A
    lam_half = abs(ref["penalty"] / ref["weighted"]) if ref["weighted"] else 0.0
    return np.array([lam_half * (bw + U * A), bw, ((deepest + 4 + T) / 2 + 2) * U * ref["dist"]])


def accumulate_bound(total, k, statistic):
    """imp after k accumulations from zero.  x = fl(fl(grad_scale) g) carries 2; x^2 2 * 2 + 1 = 5, |x| 2; every addition U of the
    running sum, which is non-negative and grows: k U of the final one; one spare.  total: the float64 sum."""
    return ((6 if statistic == 0 else 3) + k) * U * np.abs(total)


def axpby_bound(a, dst, b, src):
    """dst' = fma(fl(b), src, fl(fl(a) dst)): each product 2, the sum 1 of both, one spare: 4 U (|a dst| + |b src|)."""
    s = 0.0 if src is None else np.abs(b * np.asarray(src, np.float64))
    return 4.0 * U * (np.abs(a * np.asarray(dst, np.float64)) + s)


def estimate_bound(total, k, statistic, count, decay=0.0, prev=None):
    """The importance after k accumulations (grad_scale 1, no rounding of it: still counted) and finish(count, decay)."""
    prev = np.zeros_like(total) if prev is None else prev
    return accumulate_bound(total, k, statistic) / count + axpby_bound(decay, prev, 1.0 / count, total)


# ------------------------------------------------------------------------------------------------
# the kernels' arithmetic in numpy float32 (no contraction), in the kernels' own order of summation, with the planted bugs
# ------------------------------------------------------------------------------------------------
F = np.float32
WRONG_PENALTY = ("missing_half", "importance_twice", "sign_flipped", "penalty_scale_ignored", "tensor_weight_ignored")
WRONG_IMPORTANCE = ("abs_for_square", "mean_omitted")


def consolidate_fp32(thetas, anchors, imps, grads, lam, tensor_weight, penalty_scale, wrong=None):
    """cswin_consolidate_chunks + cswin_consolidate_finalize in float32: (new gradients, per_tensor, scalars)."""
    out, per = [], []
    for t, (p, a) in enumerate(zip(thetas, anchors)):
        d = (np.asarray(a, F) - np.asarray(p, F)) if wrong == "sign_flipped" else (np.asarray(p, F) - np.asarray(a, F))
        tt = d if imps is None else np.asarray(imps[t], F) * d
        if wrong == "importance_twice" and imps is not None:
            tt = np.asarray(imps[t], F) * tt
        w = F(1) if wrong == "tensor_weight_ignored" else F(tensor_weight[t])
        c = (F(lam) * w) * (F(1) if wrong == "penalty_scale_ignored" else F(penalty_scale))
        sfd, sdd = F(0), F(0)
        for o in range(0, d.size, 16384):
            sfd = sfd + chunk_sum_fp32(tt[o:o + 16384] * d[o:o + 16384])
            sdd = sdd + chunk_sum_fp32(d[o:o + 16384] * d[o:o + 16384])
        per.append((sfd, sdd))
        if grads is not None:
            g = np.asarray(grads[t], F)
            out.append(g.copy() if c == 0 else (c * tt + g).astype(F))
    weighted, dist = F(0), F(0)
    for t, (sfd, sdd) in enumerate(per):
        w = F(1) if wrong == "tensor_weight_ignored" else F(tensor_weight[t])
        weighted = weighted + w * sfd
        dist = dist + sdd
    half = F(lam) if wrong == "missing_half" else F(0.5) * F(lam)
    return out, np.array(per, F).reshape(-1, 2), np.array([half * weighted, weighted, np.sqrt(dist)], F)


def importance_fp32(grads_per_batch, statistic, grad_scale, count, decay=0.0, prev=None, wrong=None):
    """cswin_importance_accumulate per batch from zero, then cswin_flat_axpby(imp, scratch, decay, 1 / count), in float32."""
    stat = 1 if wrong == "abs_for_square" else statistic
    acc = np.zeros(np.asarray(grads_per_batch[0]).shape, F)
    for g in grads_per_batch:
        x = np.asarray(g, F) * F(grad_scale)
        acc = acc + (np.abs(x) if stat else x * x)
    b = F(1) if wrong == "mean_omitted" else F(1.0 / count)
    prev = np.zeros_like(acc) if prev is None else np.asarray(prev, F)
    return (F(decay) * prev + b * acc).astype(F)


# ------------------------------------------------------------------------------------------------
# inputs shared with the GPU tests
# ------------------------------------------------------------------------------------------------
def cons_inputs(tag, numels, spread=0.05):
    """Per-tensor float32 (theta, anchor, importance, [g0, g1, g2]): test_tpgm_host.tpgm_inputs and an importance N(0, 1)^2 >= 0
    (mean 1, a quarter of it below 0.1), an exact zero at every seventh element of the layout."""
    thetas, anchors, gs = tpgm_inputs("cons." + tag, numels, spread=spread)
    imps = []
    for t, n in enumerate(numels):
        f = det_normal(f"cons.{tag}.f{t}", (n,)).astype(np.float32) ** 2
        f[(np.arange(n) + t) % 7 == 3] = 0.0
        imps.append(f.astype(np.float32))
    return thetas, anchors, imps, gs


def mixed_weights(T):
    """w_t: 0 for every third tensor (at least one of each from T = 2 on), else 1."""
    return np.array([0.0 if t % 3 == 1 else 1.0 for t in range(T)], np.float32)


HOST_NUMELS = (1027, 16389, 5, 1027, 9, 33)


def _penalty_case(wrong, with_imp, penalty_scale, lam=0.37):
    """Largest |fp32 emulation - float64| / bound for the gradient, per_tensor and the three scalars."""
    thetas, anchors, imps, gs = cons_inputs("host", HOST_NUMELS)
    imps = imps if with_imp else None
    tw = mixed_weights(len(HOST_NUMELS))
    nchunks = [cdiv(n, 16384) for n in HOST_NUMELS]
    lam32 = float(np.float32(lam))
    ref = penalty_ref(thetas, anchors, imps, lam32, tw, penalty_scale)
    got_g, got_per, got_sc = consolidate_fp32(thetas, anchors, imps, gs[0], lam, tw, penalty_scale, wrong=wrong)
    worst = {}

    def rel(err, bound):
        with np.errstate(divide="ignore", invalid="ignore"):
            return float(np.max(np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))))
    worst["grad"] = max(rel(np.abs(g.astype(np.float64) - (g0.astype(np.float64) + add)), grad_bound(add, g0))
                        for g, g0, add in zip(got_g, gs[0], ref["grad"]))
    bfd = np.array([fd_sum_bound(x, n, c) for x, n, c in zip(ref["abs_fd"], HOST_NUMELS, nchunks)])
    bdd = np.array([dd_sum_bound(x, n, c) for x, n, c in zip(ref["per_tensor"][:, 1], HOST_NUMELS, nchunks)])
    worst["per_tensor"] = max(rel(np.abs(got_per[:, 0] - ref["per_tensor"][:, 0]), bfd), rel(np.abs(got_per[:, 1] - ref["per_tensor"][:, 1]), bdd))
    bs = scalar_bounds(ref, HOST_NUMELS, nchunks, tw)
    want = np.array([ref["penalty"], ref["weighted"], ref["dist"]])
    for k, name in enumerate(("penalty", "weighted", "dist")):
        worst[name] = rel(np.abs(np.float64(got_sc[k]) - want[k:k + 1]), bs[k:k + 1])
    return worst


# ------------------------------------------------------------------------------------------------
# tests
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_imp", [True, False], ids=["importance", "l2sp"])
def test_penalty_ref_agrees_with_autograd_of_the_written_out_penalty(with_imp):
    numels = (7, 12, 5)
    thetas, anchors, imps, _ = cons_inputs("auto", numels, spread=0.5)
    tw, lam, ps = np.array([1.0, 0.0, 1.0]), 0.7, 2.0
    leaves = [torch.from_numpy(p.astype(np.float64)).requires_grad_() for p in thetas]
    total = 0.0
    for t, (p, a) in enumerate(zip(leaves, anchors)):
        f = torch.from_numpy(imps[t].astype(np.float64)) if with_imp else 1.0
        total = total + tw[t] * (f * (p - torch.from_numpy(a.astype(np.float64))) ** 2).sum()
    penalty = (lam / 2) * total
    grads = torch.autograd.grad(penalty, leaves)
    ref = penalty_ref(thetas, anchors, imps if with_imp else None, lam, tw, ps)
    assert abs(float(penalty.detach()) - ref["penalty"]) <= 1e-12 * abs(ref["penalty"]) and ref["penalty"] > 0
    for g, want in zip(grads, ref["grad"]):
        assert np.abs(ps * g.numpy() - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    assert (ref["grad"][1] == 0).all() and np.abs(ref["grad"][0]).max() > 0
    d0 = thetas[0].astype(np.float64) - anchors[0].astype(np.float64)
    assert abs(ref["per_tensor"][0, 1] - (d0 * d0).sum()) <= 1e-12 and abs(ref["dist"] ** 2 - ref["per_tensor"][:, 1].sum()) <= 1e-12


@pytest.mark.parametrize("method", ["ewc", "mas"])
def test_importance_ref_agrees_with_an_explicit_per_batch_loop(method):
    """A small nn.Linear + cross entropy: per batch the gradient of the method's loss, F = (1 / n) sum g^2 (or |g|) by an explicit
    torch loop; then a second, online, estimation F <- decay F + F_new."""
    torch.manual_seed(0)
    net = torch.nn.Linear(5, 3).double()
    with torch.no_grad():
        for n, p in net.named_parameters():
            p.copy_(torch.from_numpy(det_normal(f"cons.lin.{n}", tuple(p.shape)).astype(np.float64)))
    batches = [(torch.from_numpy(det_normal(f"cons.lin.x{k}", (4, 5)).astype(np.float64)), torch.tensor([k % 3, 1, 2, 0])) for k in range(3)]

    def batch_grads(bs):
        out = []
        for x, y in bs:
            logits = net(x)
            loss = torch.nn.functional.cross_entropy(logits, y) if method == "ewc" else logits.square().sum() / logits.shape[0]
            out.append([g.numpy().copy() for g in torch.autograd.grad(loss, list(net.parameters()))])
        return out
    stat = STATISTICS[method]
    per_batch = batch_grads(batches)
    loop = [torch.zeros_like(p) for p in net.parameters()]
    for grads in per_batch:
        for acc, g in zip(loop, grads):
            acc += torch.from_numpy(g) ** 2 if method == "ewc" else torch.from_numpy(g).abs()
    loop = [(acc / len(batches)).numpy() for acc in loop]
    first = [importance_ref([b[i] for b in per_batch], stat) for i in range(2)]
    for a, b in zip(first, loop):
        assert np.abs(a - b).max() <= 1e-14 * max(1.0, np.abs(b).max()) and (a >= 0).all() and a.max() > 0
    # grad_scale and an explicit count: F of (0.5 g) over 6
    half = importance_ref([b[0] for b in per_batch], stat, grad_scale=0.5, count=6)
    assert np.abs(half - loop[0] * (0.25 if method == "ewc" else 0.5) / 2).max() <= 1e-14
    # online: two of the batches again, decay 0.9
    again = batch_grads(batches[:2])
    online = importance_ref([b[0] for b in again], stat, decay=0.9, prev=first[0])
    by_hand = 0.9 * loop[0] + sum((torch.from_numpy(b[0]) ** 2 if method == "ewc" else torch.from_numpy(b[0]).abs()).numpy() for b in again) / 2
    assert np.abs(online - by_hand).max() <= 1e-14 * max(1.0, np.abs(by_hand).max())


@pytest.mark.parametrize("penalty_scale", [1.0, 2.0, 8.0])
@pytest.mark.parametrize("with_imp", [True, False], ids=["importance", "l2sp"])
def test_the_bounds_hold_the_fp32_arithmetic(with_imp, penalty_scale):
    worst = _penalty_case(None, with_imp, penalty_scale)
    print("fp32 emulation / bound:", worst)
    assert all(w <= 1.0 for w in worst.values()), worst
    assert worst["grad"] >= 0.01 and worst["per_tensor"] >= 0.005, worst        # not slack by more than a factor 100 / 200


@pytest.mark.parametrize("wrong", WRONG_PENALTY)
def test_the_bounds_reject_the_planted_penalty_bugs(wrong):
    worst = _penalty_case(wrong, True, 2.0)
    print(f"{wrong}: emulation / bound: {worst}")
    seen = {"missing_half": ("penalty",), "importance_twice": ("grad", "per_tensor", "weighted"), "sign_flipped": ("grad",),
            "penalty_scale_ignored": ("grad",), "tensor_weight_ignored": ("grad", "weighted", "penalty")}[wrong]
    assert all(worst[k] > 1.0 for k in seen), (wrong, worst)


def _importance_case(wrong, statistic, grad_scale, decay):
    _, _, imps, gs = cons_inputs("imp", HOST_NUMELS)
    worst = 0.0
    for t in range(len(HOST_NUMELS)):
        batches = [g[t] for g in gs]
        prev = imps[t] if decay else None
        total = importance_ref(batches, statistic, float(np.float32(grad_scale)), count=1)
        want = importance_ref(batches, statistic, float(np.float32(grad_scale)), decay=decay, prev=prev)
        bound = estimate_bound(total, 3, statistic, 3, decay, prev)
        got = importance_fp32(batches, statistic, grad_scale, 3, decay, prev, wrong=wrong)
        err = np.abs(got.astype(np.float64) - want)
        with np.errstate(divide="ignore", invalid="ignore"):
            worst = max(worst, float(np.max(np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0)))))
    return worst


@pytest.mark.parametrize("decay", [0.0, 0.9])
@pytest.mark.parametrize("grad_scale", [1.0, 0.125])
@pytest.mark.parametrize("statistic", [0, 1], ids=["squares", "abs"])
def test_the_importance_bound_holds_the_fp32_arithmetic(statistic, grad_scale, decay):
    worst = _importance_case(None, statistic, grad_scale, decay)
    print("fp32 emulation / bound:", worst)
    assert 0.01 <= worst <= 1.0


@pytest.mark.parametrize("wrong", WRONG_IMPORTANCE)
def test_the_importance_bound_rejects_the_planted_bugs(wrong):
    worst = _importance_case(wrong, 0, 1.0, 0.0)
    print(f"{wrong}: emulation / bound: {worst}")
    assert worst > 1.0


def _state(method="ewc"):
    l2sp = method == "l2sp"
    names = {"a.weight": (4, 3), "a.bias": (4,), "output.weight": (9, 5, 1, 1), "scale": ()}
    tensors = {n: {"anchor": torch.from_numpy(np.asarray(det_normal(f"cons.carry.a.{n}", s or (1,))).reshape(s)),
                   "importance": None if l2sp else torch.from_numpy(np.asarray(det_normal(f"cons.carry.f.{n}", s or (1,))).reshape(s)).square()}
               for n, s in names.items()}
    return {"method": method, "weight": 3.0, "exclude": ["a.bias"], "tensors": tensors}


@pytest.mark.parametrize("method", ["ewc", "l2sp"])
def test_carry_consolidation_state_every_branch(method):
    from cswin_unet_amd.continual import carry_consolidation_state
    state = _state(method)
    cur = {"a.weight": torch.full((4, 3), 7.0), "a.bias": torch.full((4,), 7.0), "output.weight": torch.full((12, 5, 1, 1), 7.0),
           "scale": torch.tensor(7.0), "new.weight": torch.full((2, 2), 7.0)}
    out = carry_consolidation_state(state, cur)
    assert list(out["tensors"]) == list(cur) and out["method"] == method and out["weight"] == 3.0 and out["exclude"] == ["a.bias"]
    l2sp = method == "l2sp"
    for n in ("a.weight", "a.bias", "scale"):                            # same shape: copied
        assert torch.equal(out["tensors"][n]["anchor"], state["tensors"][n]["anchor"])
        assert out["tensors"][n]["importance"] is None if l2sp else torch.equal(out["tensors"][n]["importance"], state["tensors"][n]["importance"])
    grown = out["tensors"]["output.weight"]                               # leading rows carried, new rows: importance 0, anchor = current
    assert grown["anchor"].shape == (12, 5, 1, 1) and torch.equal(grown["anchor"][:9], state["tensors"]["output.weight"]["anchor"])
    assert (grown["anchor"][9:] == 7.0).all()
    fresh = out["tensors"]["new.weight"]                                  # absent: importance 0, anchor = current
    assert (fresh["anchor"] == 7.0).all()
    if l2sp:
        assert grown["importance"] is None and fresh["importance"] is None
    else:
        assert torch.equal(grown["importance"][:9], state["tensors"]["output.weight"]["importance"]) and (grown["importance"][9:] == 0).all()
        assert (fresh["importance"] == 0).all() and fresh["importance"].shape == (2, 2)
    assert (cur["output.weight"] == 7.0).all() and state["tensors"]["output.weight"]["anchor"].shape == (9, 5, 1, 1)      # inputs untouched
    for bad in ({"a.weight": torch.zeros(4, 4)}, {"a.weight": torch.zeros(3, 3)}, {"output.weight": torch.zeros(12, 6, 1, 1)},
                {"a.bias": torch.zeros(4, 1)}, {"scale": torch.zeros(2)}):
        with pytest.raises(ValueError, match=next(iter(bad)).replace(".", r"\.")):
            carry_consolidation_state(state, bad)


def test_options_are_validated_before_any_device_work():
    from cswin_unet_amd.continual import Consolidation
    from cswin_unet_amd.optim import FlatConsolidation
    from cswin_unet_amd.trainer import _step_options

    class Opt:
        params = [torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2))]
    for kw, match in ((dict(method="si"), "method"), (dict(weight=-1.0), "weight"), (dict(weight=float("nan")), "weight"),
                      (dict(weight=float("inf")), "weight"), (dict(weight="much"), "weight")):
        with pytest.raises(ValueError, match=match):
            FlatConsolidation(Opt(), ["a", "b"], **kw)
        with pytest.raises(ValueError, match=match):
            Consolidation(None, **kw)                                   # the trainer is not looked at
    with pytest.raises(ValueError, match="names"):
        FlatConsolidation(Opt(), ["a"])
    with pytest.raises(KeyError, match="no trainable parameter"):
        FlatConsolidation(Opt(), ["a", "b"], exclude=("c",))
    with pytest.raises(ValueError, match="state"):
        Consolidation(None, method="mas", state=_state("ewc"))
    # estimate: its checks come before the trainer (None here) or the batches are touched
    cons = Consolidation.__new__(Consolidation)
    cons.trainer = None
    for method, kw, match in (("l2sp", {}, "l2sp"), ("ewc", dict(decay=-0.1), "decay"), ("mas", dict(decay=1.5), "decay"),
                              ("ewc", dict(decay=float("nan")), "decay")):
        cons.flat = types.SimpleNamespace(method=method)
        with pytest.raises(ValueError, match=match):
            cons.estimate(iter(()), **kw)
    with pytest.raises(ValueError, match="decay"):
        cons.consolidate(iter(()), 2.0)
    # trainer_synapse's options
    ok = _step_options(types.SimpleNamespace())
    assert ok["consolidation"] is None and ok["consolidation_weight"] is None
    ok = _step_options(types.SimpleNamespace(consolidation=_state("mas"), consolidation_weight=5))
    assert ok["consolidation"]["method"] == "mas" and ok["consolidation_weight"] == 5.0
    assert _step_options(types.SimpleNamespace(consolidation="stage0_consolidation.pt"))["consolidation"] == "stage0_consolidation.pt"
    for bad, match in ((dict(consolidation=3), "consolidation"), (dict(consolidation={"method": "ewc"}), "consolidation"),
                       (dict(consolidation={"method": "si", "tensors": {}}), "method"),
                       (dict(consolidation=_state(), consolidation_weight=-2.0), "weight"),
                       (dict(consolidation=_state(), consolidation_weight=float("inf")), "weight"),
                       (dict(consolidation_weight=1.0), "consolidation_weight")):
        with pytest.raises(ValueError, match=match):
            _step_options(types.SimpleNamespace(**bad))


def test_flat_consolidation_runs_on_a_hip_device_only():
    from cswin_unet_amd.optim import FlatConsolidation

    class Opt:
        params = [torch.nn.Parameter(torch.zeros(3))]
    for method in ("ewc", "mas", "l2sp"):
        with pytest.raises(RuntimeError, match="FlatConsolidation"):
            FlatConsolidation(Opt(), ["w"], method=method)
