"""The DropPath-compacted launches of the Linear GEMM family at every tile configuration and sample geometry: cswin_linear_fwd_skip and
cswin_linear_bwd_data_skip (a sample ORDER: RowMap, gemm_mapped_kernel), cswin_linear_bwd_weight_batch_masked and
cswin_linear_bwd_tail_masked (sample MASKS: RowMask, KeptList), cswin_linear_bwd_tail_skip (both) and cswin_drop_path_order, called
directly through cswin_unet_amd._lib.

The tables, and which branch each row is there for, are in tests/droppath_cases.py; tests/test_droppath_host.py shows on the CPU that
its assertions (check_mapped, check_masked), which are the ones applied here, fail on a compaction that is subtly wrong.  Bounds: bit
equality with the entry point without an order / a mask wherever the kernels promise it, and test_gpu_parity's fp32 RTOL against
float64 (linear_ref of tests/test_gpu_gemm_shapes.py; the float64 product over the kept rows) -- no new number.  Every output is a
view into a NaN-filled buffer whose guard words must survive, every weight-gradient workspace is exactly as large as
cswin_linear_bwd_weight_workspace() says, the dropped samples' rows of A, gelu_pre, dy and x hold NaN (one read of them makes a
result non-finite), and every measured error goes to the suite's error log under a tag naming the case."""
import ctypes
import os

import numpy as np
import pytest
import torch

import droppath_cases as C
from oracle.determ import det_normal
from test_gpu_attn_shapes import Guarded, settle       # NaN guard bands round an output; their check after a launch
from test_gpu_gemm_shapes import TUNING_PREFIXES
from test_gpu_parity import RTOL                       # the suite's fp32 bound
from test_gpu_shapes import measure                    # max|got - ref| / rms(ref) in float64, printed and logged

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
sid = lambda s: "-".join(map(str, s))


def logged(got, ref, tag):
    return measure(torch.from_numpy(np.ascontiguousarray(got)), torch.from_numpy(np.ascontiguousarray(ref)), tag)


def T(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def vp(a):
    return ctypes.cast(a, ctypes.c_void_p)


@pytest.fixture(scope="module", autouse=True)
def default_launch_plan():
    """The tables name tile configurations, slabs and routes: they hold with no tuning variable set (read once per process)."""
    present = [v for v in os.environ if v.startswith(TUNING_PREFIXES)]
    if present:
        pytest.skip(f"{', '.join(present)} set: the launch plan these tests rely on does not hold")


# ------------------------------------------------------------------------------------------------
# forward and data gradient with a sample order
# ------------------------------------------------------------------------------------------------
class Mapped:
    """One Linear, forward or data gradient, on the device (droppath_cases.mapped_inputs)."""

    def __init__(self, form, shape):
        self.form, self.shape = form, shape
        self.inp = C.mapped_inputs(form, shape)
        i = self.inp
        self.ns, self.rps, self.M, self.cols, self.red = i["ns"], i["rps"], i["ns"] * i["rps"], i["cols"], i["red"]
        self.a, self.w, self.bias, self.residual, self.pre = T(i["a"]), T(i["w"]), T(i["bias"]), T(i["residual"]), T(i["pre"])
        self.what = f"droppath.{form[0]}.{form[1]}.{sid(shape)}"

    def run(self, keep=None, *, skip, poison=False, zero_a=False, order=None, what=""):
        """-> {y[, y_act]} or {dx} as float32 host arrays.  keep: per-sample flags (None: all); poison: NaN in the dropped samples'
        rows of A and gelu_pre; order: the order row to pass instead of order_of(keep)."""
        from cswin_unet_amd._lib import call, ptr, stream
        entry, f = self.form
        keep = np.ones(self.ns, bool) if keep is None else keep
        a = torch.zeros_like(self.a) if zero_a else self.a
        pre = self.pre
        if poison and not keep.all():
            rows = T(np.repeat(keep, self.rps))
            a = a.clone()
            a[~rows] = NAN
            if pre is not None:
                pre = pre.clone()
                pre[~rows] = NAN
        rs = T(C.row_scale_of(self.form, keep))
        order = T(C.order_of(keep) if order is None else np.asarray(order, np.int32))
        tail = (ptr(order), self.ns, stream()) if skip else (stream(),)
        sfx = "_skip" if skip else ""
        o = {("dx" if entry == "dgrad" else "y"): Guarded((self.M, self.cols))}
        if entry == "fwd":
            if f == "gelu":
                o["y_act"] = Guarded((self.M, self.cols))
            call("cswin_linear_fwd" + sfx, ptr(a), None, 0, ptr(self.w), ptr(self.bias), ptr(o["y"].t), ptr(o["y_act"].t) if f == "gelu" else None,
                 ptr(self.residual), ptr(rs), self.rps, self.M, self.cols, self.red, 0, 0, *tail)
        else:
            call("cswin_linear_bwd_data" + sfx, ptr(a), ptr(self.w), ptr(o["dx"].t), None, 0, ptr(pre), ptr(rs), self.rps, None, self.M, self.red,
                 self.cols, 0, 0, *tail)
        settle(f"{self.what} {what}", o)
        return {k: g.t.cpu().numpy() for k, g in o.items()}

    def check_patterns(self, patterns):
        """The unmapped launch against float64, the identity orders, then every keep pattern through droppath_cases.check_mapped."""
        form, what = self.form, self.what
        ref = C.mapped_reference(form, self.inp)
        plain = self.run(skip=False, what="unmapped")
        zero = self.run(skip=False, zero_a=True, what="zero A")
        for k in plain:
            err = logged(plain[k], ref[k], f"{what}.unmapped.{k}")
            assert np.isfinite(err) and err <= RTOL, (what, k, err)
        # every sample kept: the unmapped launch bit for bit, with a valid order and with anything behind a count of nsamples
        junk = np.concatenate([[self.ns], np.arange(self.ns)[::-1] * 7 - 5])            # negative and too large entries, never indexed through
        for name, order in (("all_kept", None), ("all_kept_junk_order", junk)):
            got = self.run(skip=True, order=order, what=name)
            for k in plain:
                assert np.array_equal(got[k], plain[k]), f"{what}.{name}: {k} is not the unmapped launch's"
        for name, keep in patterns:
            got = self.run(keep, skip=True, poison=True, what=name)
            C.check_mapped(f"{what}.{name}", form, got, plain, zero, ref, self.inp, keep, logged, RTOL)


@pytest.mark.parametrize("shape,config", C.MAPPED_SHAPES, ids=[sid(s) for s, _ in C.MAPPED_SHAPES])
def test_order_at_every_tile_configuration_form_and_keep_pattern(shape, config):
    """Kept rows: bit for bit the unmapped entry point's and within RTOL of float64.  Dropped rows: the bias (+0 without one), the
    zero-A launch's GELU(bias), the residual row, +0 for a data gradient.  Everything finite although the dropped samples' rows of A
    and gelu_pre hold NaN."""
    ns, rps = shape[:2]
    for form in C.FORMS:
        Mapped(form, shape).check_patterns(C.unique_patterns(ns, rps))


BOUND_FORMS = [("fwd", "plain"), ("fwd", "res_factors"), ("dgrad", "scaled")]


def test_order_at_the_accepted_side_of_the_quotient_bound():
    """(256, 4095): (M + 63) * rows_per_sample = 4 293 128 385 < 2^32, 16 MB per matrix at four columns.  All but one sample dropped,
    and only the last sample kept (the launch's first tile stands for physical rows from 1 044 225 on)."""
    ns, rps = C.BOUND["accepted"]
    only = lambda s: np.arange(ns) == s
    for form in BOUND_FORMS:
        Mapped(form, (ns, rps, 4, 4)).check_patterns([("all_but_one", only(ns // 2)), ("only_last", only(ns - 1))])


def test_past_the_quotient_bound_is_refused_and_touches_nothing():
    """(256, 4096): both skip entry points and the masked weight gradient answer CSWIN_ERR_UNSUPPORTED; no buffer is written."""
    from cswin_unet_amd._lib import CswinHipError, ReduceJob, WgradDesc, call, lib, ptr, stream
    ns, rps = C.BOUND["refused"]
    M, N, K = ns * rps, 4, 4
    x, w, bias = torch.zeros(M, K, device=DEV), torch.zeros(N, K, device=DEV), torch.zeros(N, device=DEV)
    order = T(C.order_of(np.arange(ns) != 3))
    y, dx = Guarded((M, N)), Guarded((M, K))
    with pytest.raises(CswinHipError, match=r"\(-5\).*below 2\^32"):
        call("cswin_linear_fwd_skip", ptr(x), None, 0, ptr(w), ptr(bias), ptr(y.t), None, None, None, rps, M, N, K, 0, 0, ptr(order), ns, stream())
    with pytest.raises(CswinHipError, match=r"\(-5\).*below 2\^32"):
        call("cswin_linear_bwd_data_skip", ptr(x), ptr(w), ptr(dx.t), None, 0, None, None, rps, None, M, N, K, 0, 0, ptr(order), ns, stream())
    nbytes = lib().cswin_linear_bwd_weight_workspace(M, N, K)
    o = dict(y=y, dx=dx, dw=Guarded((N, K)), dbias=Guarded((N,)), workspace=Guarded((nbytes // 4,)))
    wg, jobs = (WgradDesc * 1)(), (ReduceJob * 1)()
    d = wg[0]
    d.dy, d.x, d.dw, d.dbias, d.workspace, d.ws_bytes = x.data_ptr(), x.data_ptr(), o["dw"].t.data_ptr(), o["dbias"].t.data_ptr(), o["workspace"].t.data_ptr(), nbytes
    d.rows_per_sample, d.M, d.N, d.K = rps, M, N, K
    mask = torch.ones(ns, device=DEV)
    with pytest.raises(CswinHipError, match=r"\(-5\).*below 2\^32"):
        call("cswin_linear_bwd_weight_batch_masked", vp(wg), 1, vp(jobs), None, 0, (ctypes.c_void_p * 1)(mask.data_ptr()), (ctypes.c_int * 1)(ns), stream())
    settle("past the bound", o, untouched=True)


# ------------------------------------------------------------------------------------------------
# weight gradients with sample masks
# ------------------------------------------------------------------------------------------------
class Problem:
    """One weight gradient on the device.  keep: per-sample flags (None: no mask); the mask floats are 1.25 / 0, the row scale a
    factor per sample (0 for a dropped one).  The dropped samples' rows of dy and x hold NaN."""

    def __init__(self, tag, geometry, N, K, keep=None, scaled=False, bias=True):
        ns, rps = geometry
        self.tag, self.ns, self.rps, self.M, self.N, self.K, self.bias = tag, ns, rps, ns * rps, N, K, bias
        dy, x = C.masked_inputs(tag, ns, rps, N, K)
        self.keep = None if keep is None else np.asarray(keep, bool)
        kept = np.ones(ns, bool) if keep is None else self.keep
        scale = np.where(kept, C.sample_factors(ns), 0.0).astype(np.float32) if scaled else None
        self.dw_ref, self.db_ref = C.masked_reference(dy, x, kept, scale, rps)
        rows = np.repeat(kept, rps)
        dy, x = dy.copy(), x.copy()
        dy[~rows], x[~rows] = NAN, NAN
        self.dy, self.x, self.scale = T(dy), T(x), T(scale)
        self.mask = None if keep is None else T(np.where(kept, 1.25, 0.0).astype(np.float32))


def riders():
    """Two pending reductions (column sums of a few rows) for a tail call: (the job array, their Guarded outputs, their float64 sums)."""
    from cswin_unet_amd._lib import ReduceJob
    pend, outs, refs, keep = (ReduceJob * 2)(), [], [], []
    for i, (rows, n) in enumerate(((7, 300), (3, 132))):
        part = T(det_normal(f"droppath.rider.{i}", (rows, n)))
        out = Guarded((n,))
        pend[i].part, pend[i].out, pend[i].n_first, pend[i].n, pend[i].stride, pend[i].rows = part.data_ptr(), out.t.data_ptr(), n, n, n, rows
        outs.append(out)
        refs.append(part.double().sum(0).cpu().numpy())
        keep.append(part)
    return pend, outs, refs, keep


def launch(what, probs, *, masked, tail=None, order=None, pending=None, refused=None):
    """The problems through cswin_linear_bwd_weight_batch[_masked], or with tail = (dy, w) through cswin_linear_bwd_tail_masked /
    (order = (order row, samples)) cswin_linear_bwd_tail_skip; then their slab reductions.  masked = False: no mask is passed.
    -> ([(dw, dbias)], dx, the riders' outputs) as host arrays.  refused: the error the call must raise, touching nothing."""
    from cswin_unet_amd._lib import CswinHipError, ReduceJob, WgradDesc, call, lib, ptr, stream
    n = len(probs)
    wg, jobs, o = (WgradDesc * n)(), (ReduceJob * n)(), {}
    for i, p in enumerate(probs):
        nbytes = lib().cswin_linear_bwd_weight_workspace(p.M, p.N, p.K)
        o[f"dw{i}"], o[f"workspace{i}"] = Guarded((p.N, p.K)), Guarded((nbytes // 4,))
        if p.bias:
            o[f"dbias{i}"] = Guarded((p.N,))
        d = wg[i]
        d.dy, d.x, d.row_scale = p.dy.data_ptr(), p.x.data_ptr(), (p.scale.data_ptr() if p.scale is not None else None)
        d.dw, d.dbias = o[f"dw{i}"].t.data_ptr(), (o[f"dbias{i}"].t.data_ptr() if p.bias else None)
        d.workspace, d.ws_bytes, d.rows_per_sample, d.M, d.N, d.K = o[f"workspace{i}"].t.data_ptr(), nbytes, p.rps, p.M, p.N, p.K
    if masked:
        extra = ((ctypes.c_void_p * n)(*[p.mask.data_ptr() if p.mask is not None else None for p in probs]), (ctypes.c_int * n)(*[p.ns for p in probs]))
    else:
        extra = (None, None)
    pend = (vp(pending[0]), len(pending[0])) if pending else (None, 0)
    if pending:
        o.update({f"rider{k}": g for k, g in enumerate(pending[1])})
    if tail is not None:
        tdy, tw = tail
        o["dx"] = Guarded((tdy.shape[0], tw.shape[1]))
        args = (ptr(tdy), ptr(tw), ptr(o["dx"].t), tdy.shape[0], tdy.shape[1], tw.shape[1], vp(wg), n, vp(jobs), *pend, *extra)
        if order is not None:
            fn = lambda: call("cswin_linear_bwd_tail_skip", *args, ptr(order[0]), order[1], stream())
        else:
            fn = lambda: call("cswin_linear_bwd_tail_masked", *args, stream())
    else:
        name = "cswin_linear_bwd_weight_batch_masked" if masked else "cswin_linear_bwd_weight_batch"
        fn = lambda: call(name, vp(wg), n, vp(jobs), *pend, *(extra if masked else ()), stream())
    if refused:
        with pytest.raises(CswinHipError, match=refused):
            fn()
        settle(what, o, untouched=True)
        return None
    fn()
    call("cswin_rows_sum_multi", vp(jobs), n, stream())
    settle(what, {k: g for k, g in o.items() if not k.startswith("workspace")})
    for k, g in o.items():
        assert not k.startswith("workspace") or g.intact(), f"{what}: a guard word of {k} was overwritten"
    h = lambda k: o[k].t.cpu().numpy() if k in o else None
    return [(h(f"dw{i}"), h(f"dbias{i}")) for i in range(n)], h("dx"), [h(f"rider{k}") for k in range(len(pending[1]) if pending else 0)]


def same(a, b):
    return (a is None and b is None) or np.array_equal(a, b)


def check_problems(what, probs, outs):
    for i, (p, (dw, db)) in enumerate(zip(probs, outs)):
        C.check_masked(f"{what}.{i}", dw, db, p.dw_ref, p.db_ref if p.bias else None, logged, RTOL)


@pytest.mark.parametrize("problem,slabs", C.MASKED_PROBLEMS, ids=[f"{sid(p[0])}-{p[1]}-{p[2]}" for p, _ in C.MASKED_PROBLEMS])
def test_mask_at_every_geometry_and_keep_pattern(problem, slabs):
    """dw and dbias within RTOL of the float64 product over the kept rows and finite, with and without a row scale and dbias; every
    sample kept: the unmasked entry point's bits; every sample dropped: exact zeros; two runs: the same bits."""
    geometry, N, K = problem
    ns, rps = geometry
    tag = sid((ns, rps, N, K))
    for scaled in (False, True):
        for bias in (False, True):
            var = f"droppath.mask.{tag}.{int(scaled)}{int(bias)}"
            p = Problem(tag, geometry, N, K, keep=np.ones(ns, bool), scaled=scaled, bias=bias)
            (got,), _, _ = launch(var + ".all_kept", [p], masked=True)
            (want,), _, _ = launch(var + ".unmasked", [p], masked=False)
            check_problems(var + ".all_kept", [p], [got])
            assert np.array_equal(got[0], want[0]) and same(got[1], want[1]), f"{var}: every sample kept is not the unmasked launch bit for bit"
            for name, keep in C.unique_patterns(ns, rps):
                p = Problem(tag, geometry, N, K, keep=keep, scaled=scaled, bias=bias)
                (got,), _, _ = launch(f"{var}.{name}", [p], masked=True)
                check_problems(f"{var}.{name}", [p], [got])
                if not keep.any():
                    assert not got[0].any() and (got[1] is None or not got[1].any()), f"{var}.{name}: not exact zeros"
                if scaled and bias:
                    (again,), _, _ = launch(f"{var}.{name}.again", [p], masked=True)
                    assert np.array_equal(got[0], again[0]) and same(got[1], again[1]), f"{var}.{name}: two runs differ"


@pytest.mark.parametrize("k", range(len(C.MASKED_BATCHES)))
def test_mask_in_batches_of_four_with_mixed_sample_counts(k):
    probs = [Problem(f"b{k}.{i}", g, N, K, keep=None if name is None else C.keep_patterns(*g)[name], scaled=scaled, bias=bias)
             for i, (g, N, K, name, scaled, bias) in enumerate(C.MASKED_BATCHES[k])]
    outs, _, _ = launch(f"droppath.mask.batch{k}", probs, masked=True)
    check_problems(f"droppath.mask.batch{k}", probs, outs)
    again, _, _ = launch(f"droppath.mask.batch{k}.again", probs, masked=True)
    assert all(np.array_equal(a[0], b[0]) and same(a[1], b[1]) for a, b in zip(outs, again))


def test_mask_on_an_unaligned_problem_is_refused_and_nothing_is_enqueued():
    """N = 30 has no 16-B rows: CSWIN_ERR_ALIGN, never an unmasked run; outputs, workspaces and the pending reductions stay untouched."""
    keep = C.keep_patterns(65, 3)["every_other"]
    probs = [Problem("align.0", (65, 3), 36, 68, keep=keep), Problem("align.1", (65, 3), 30, 36, keep=keep)]
    pend = riders()
    launch("droppath.mask.unaligned", probs, masked=True, pending=pend, refused=r"\(-2\).*sample mask")
    launch("droppath.mask.unaligned.tail", probs, masked=True, pending=pend, tail=(probs[0].dy, T(np.zeros((36, 68), np.float32))),
           refused=r"\(-2\).*sample mask")
    check_problems("droppath.mask.aligned_alone", probs[:1], launch("droppath.mask.aligned_alone", probs[:1], masked=True)[0])


def test_mask_at_the_accepted_side_of_the_quotient_bound():
    """(256, 4095) under a mask: M * rows_per_sample = 4 292 870 400 < 2^32; only the last sample kept."""
    ns, rps = C.BOUND["accepted"]
    p = Problem("bound", (ns, rps), 4, 4, keep=np.arange(ns) == ns - 1, scaled=True)
    check_problems("droppath.mask.bound", [p], launch("droppath.mask.bound", [p], masked=True)[0])


# ------------------------------------------------------------------------------------------------
# the tail with an order on its data gradient
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(C.TAIL_CASES))
def test_tail_with_an_order(name):
    """cswin_linear_bwd_tail_skip on each of its routes (test_droppath_host.test_routes_of_the_tail_cases) against
    cswin_linear_bwd_tail_masked with the same masks: weight gradients and riders bit for bit, the data gradient's kept rows bit for
    bit, its dropped rows +0 although dy holds NaN there; the data gradient also against float64 and, on the separate route, against
    cswin_linear_bwd_data_skip at the same arguments."""
    from cswin_unet_amd._lib import call, ptr, stream
    case = C.TAIL_CASES[name]
    what = f"droppath.tail.{name}"
    probs = [Problem(f"tail.{name}.{i}", g, N, K, keep=None if pat is None else C.keep_patterns(*g)[pat], scaled=pat is not None)
             for i, (g, N, K, pat) in enumerate(case["problems"])]
    ns, rps, N, K = case["dgrad"]
    M = ns * rps
    keep = C.keep_patterns(ns, rps)["every_other"]
    rows = np.repeat(keep, rps)
    dy = det_normal(what + ".dy", (M, N))
    w = det_normal(what + ".w", (N, K), 1 / np.sqrt(N))
    dy0, dyp = dy.copy(), dy.copy()
    dy0[~rows], dyp[~rows] = 0.0, NAN            # the call without an order reads every row of dy; the one with an order must not
    tw, order = T(w), T(C.order_of(keep))
    masked = any(p.mask is not None for p in probs)

    pend0, pend1 = riders(), riders()
    outs0, dx0, rid0 = launch(what + ".masked", probs, masked=masked, tail=(T(dy0), tw), pending=pend0)
    outs1, dx1, rid1 = launch(what + ".skip", probs, masked=masked, tail=(T(dyp), tw), order=(order, ns), pending=pend1)
    check_problems(what, probs, outs1)
    for (a, b), (c, d) in zip(outs0, outs1):
        assert np.array_equal(a, c) and same(b, d), f"{what}: a weight gradient differs from the masked call's"
    for r0, r1, ref in zip(rid0, rid1, pend0[2]):
        assert np.array_equal(r0, r1), f"{what}: a riding reduction differs from the masked call's"
        # a column sum of at most 7 fp32 values: 6 roundings of at most 2^-24 of a partial sum each, partial sums within a few rms
        assert logged(r1, ref, what + ".rider") <= 1e-6
    assert np.isfinite(dx1).all() and np.array_equal(dx1[rows], dx0[rows]), f"{what}: the data gradient's kept rows differ"
    assert not dx1[~rows].any() and not np.signbit(dx1[~rows]).any(), f"{what}: a dropped row of dx is not +0"
    err = logged(dx1[rows], (dy.astype(np.float64) @ w.astype(np.float64))[rows], what + ".dx")
    assert np.isfinite(err) and err <= RTOL
    # every sample kept, with anything behind the count: the whole data gradient is the masked call's
    junk = T(np.concatenate([[ns], np.arange(ns)[::-1] * 7 - 5]).astype(np.int32))
    _, dx2, _ = launch(what + ".skip.all_kept", probs, masked=masked, tail=(T(dy0), tw), order=(junk, ns))
    assert np.array_equal(dx2, dx0)
    if name == "separate":
        alone = Guarded((M, K))
        call("cswin_linear_bwd_data_skip", ptr(T(dyp)), ptr(tw), ptr(alone.t), None, 0, None, None, rps, None, M, N, K, 0, 0, ptr(order), ns, stream())
        settle(what + ".data_skip", dict(dx=alone))
        assert np.array_equal(alone.t.cpu().numpy(), dx1), f"{what}: not cswin_linear_bwd_data_skip's data gradient"


# ------------------------------------------------------------------------------------------------
# cswin_drop_path_order
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [8, 65, 130, 256])
def test_drop_path_order_at_the_comparison_s_edges(B):
    """u == keep is dropped (the comparison is u < keep), one ulp below keep is kept, a NaN draw is dropped; the factors are torch's
    expression bit for bit and the order lists exactly the kept samples, on both sides of the 64-lane ballot."""
    from cswin_unet_amd import ops
    keep = np.array([0.8, 0.5, 0.95], np.float32)
    u = np.random.RandomState(B).uniform(0.0, 1.0, (3, B)).astype(np.float32)
    s = np.arange(B)
    u[0, s % 3 == 0] = keep[0]                                   # draws equal to keep: dropped
    u[1, s % 2 == 1] = np.nextafter(keep[1], np.float32(0))      # one ulp below keep: kept
    u[1, s % 5 == 0] = keep[1]
    u[2, s % 4 == 2] = NAN                                       # NaN: dropped
    u[2, B - 1] = np.nextafter(keep[2], np.float32(0))
    ud, kd = T(u), T(keep[:, None])
    scales, order = ops.drop_path_order(ud, kd)
    torch.cuda.synchronize()
    want = (ud < kd).to(torch.float32) / kd
    assert torch.equal(scales, want)
    kept = np.less(u, keep[:, None])                             # False for NaN
    assert not kept[0, s % 3 == 0].any() and kept[1, (s % 2 == 1) & (s % 5 != 0)].all() and not kept[1, s % 5 == 0].any()
    assert not kept[2, s % 4 == 2].any() and kept[2, B - 1] and (B - 1) % 4 != 2
    assert np.array_equal((scales != 0).cpu().numpy(), kept)
    assert order.dtype == torch.int32 and np.array_equal(order.cpu().numpy(), np.stack([C.order_of(r) for r in kept]))
