"""The DropPath compactions of the Linear GEMM family on the host (no GPU): the NumPy model of tests/droppath_cases.py -- sample order
-> logical row -> physical row, live / mixed / fill tiles, what a dropped row holds per form, the kept list by ballots, the device's
slab ranges -- against float64 linear_ref at every table row; the slab ranges against the host's split rule; the multiply-high
quotient up to the admitted bound; the routes of the tail cases from csrc/gemm_plan.h itself (tools/gemm_plan_check.cpp, as
tests/test_gemm_plan_host.py runs it); and the evidence that the assertions tests/test_gpu_droppath_shapes.py applies to the kernels
(droppath_cases.check_mapped / check_masked) fail on a compaction that is subtly wrong -- no broken kernel is run on a GPU for that.

Rows that catch each wrong variant (SENSITIVITY below): a mixed tile treated as a fill tile at (5, 52) "first" (208 kept rows = 3
tiles + 16 rows); the row scale of the logical sample at (256, 5) "rows64p1" with a factor per sample; the sample quotient one row
early at (65, 3) "every_other" (the kept samples are no run of neighbours there: in a run the early quotient lands on the same row);
a kept list whose second trip writes from index 0 at (130, 7) "all_but_64"; a slab without its last partial granule at (65, 3)
"neighbours" (189 kept rows); a dropped row's residual scaled at (24, 49) "every_other"."""
import numpy as np
import pytest

import droppath_cases as C
import test_gpu_gemm_shapes as G
from test_gemm_plan_host import plan_tool              # noqa: F401  (fixture: the header's plans through tools/gemm_plan_check.cpp)
from test_gpu_linear_skip import FORMS as SKIP_FORMS
from test_gpu_parity import RTOL

sid = lambda s: "-".join(map(str, s))


def model_runs(form, shape):
    """(inp, ref, plain, zero): the inputs, float64 linear_ref, the model's unmapped launch and its zero-A launch."""
    inp = C.mapped_inputs(form, shape)
    every = np.ones(inp["ns"], bool)
    plain = C.model_mapped(form, inp, C.order_of(every), C.row_scale_of(form, every))
    zinp = {k: v for k, v in inp.items() if not k.startswith("_")}
    zinp["a"] = np.zeros_like(inp["a"])
    zero = C.model_mapped(form, zinp, C.order_of(every), C.row_scale_of(form, every))
    return inp, C.mapped_reference(form, inp), plain, zero


def model_launch(form, inp, keep, wrong=None):
    rows = np.repeat(keep, inp["rps"])
    return C.model_mapped(form, inp, C.order_of(keep), C.row_scale_of(form, keep), wrong=wrong, poison=~rows)


# ------------------------------------------------------------------------------------------------
# reference agreement
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [s for s, _ in C.MAPPED_SHAPES], ids=sid)
def test_model_of_the_order_equals_linear_ref_on_kept_rows_and_states_the_dropped_ones(shape):
    """Every form and keep pattern: the model's unmapped launch is linear_ref to float64 rounding, its mapped launch passes the GPU
    test's assertions (kept rows equal, dropped rows the stated values, nothing read from a dropped sample), and an order whose
    count says "all kept" is the identity whatever follows the count."""
    ns, rps = shape[:2]
    for form in C.FORMS:
        inp, ref, plain, zero = model_runs(form, shape)
        for k in ref:
            assert C.rms_metric(plain[k], ref[k]) < 1e-12, (form, k)
        junk = np.concatenate([[ns], np.arange(ns)[::-1] * 7 - 5]).astype(np.int32)        # values outside [0, ns) behind the count
        ident = C.model_mapped(form, inp, junk, C.row_scale_of(form, np.ones(ns, bool)))
        assert all(np.array_equal(ident[k], plain[k]) for k in plain), form
        for name, keep in C.unique_patterns(ns, rps):
            got = model_launch(form, inp, keep)
            C.check_mapped(f"model.{sid(shape)}.{form[0]}.{form[1]}.{name}", form, got, plain, zero, ref, inp, keep, C.rms_metric, RTOL)


def masked_splits(M, N, K, n=1):
    return G.choose_split(M, N, K, 1024 // n)[0]


@pytest.mark.parametrize("problem", [p for p, _ in C.MASKED_PROBLEMS], ids=lambda p: f"{sid(p[0])}-{p[1]}-{p[2]}")
def test_model_of_the_mask_equals_the_float64_product_over_kept_rows(problem):
    (ns, rps), N, K = problem
    dy, x = C.masked_inputs(sid((ns, rps, N, K)), ns, rps, N, K)
    splits = masked_splits(ns * rps, N, K)
    patterns = C.unique_patterns(ns, rps) + [("all_kept", np.ones(ns, bool))]
    for name, keep in patterns:
        rows = np.repeat(keep, rps)
        dyp, xp = dy.copy(), x.copy()
        dyp[~rows], xp[~rows] = C.NAN, C.NAN
        assert np.array_equal(C.kept_list(keep), np.flatnonzero(keep)), name
        for scaled in (False, True):
            scale = np.where(keep, C.sample_factors(ns), 0.0) if scaled else None
            mask = np.where(keep, 1.25, 0.0)
            dw, db = C.model_masked(dyp, xp, mask, scale, rps, splits)
            C.check_masked(f"model.{name}.{int(scaled)}", dw, db, *C.masked_reference(dy, x, keep, scale, rps), C.rms_metric, 1e-12)
        # the device's slab ranges cover the kept rows exactly once
        R = int(keep.sum()) * rps
        r, ranges = C.slab_ranges(R, splits)
        assert r % 8 == 0 and np.array_equal(np.concatenate([np.arange(lo, hi) for lo, hi in ranges] or [[]]), np.arange(R)), name
        if keep.all():
            assert (len([1 for lo, hi in ranges if hi > lo]), r) == G.choose_split(ns * rps, N, K, 1024), name


# ------------------------------------------------------------------------------------------------
# slab ranges and the split rule
# ------------------------------------------------------------------------------------------------
def test_slab_ranges_cover_every_reduction_once():
    """splits slabs of ceil8(ceil(R / splits)) rows reach R for every (R, splits), and the slabs past R are empty, not negative."""
    R, S = np.meshgrid(np.arange(0, 3000), np.arange(1, 200), indexing="ij")
    r = -(-(-(-R // S)) // 8) * 8
    assert (S * r >= R).all() and (r % 8 == 0).all()
    for R, splits in ((0, 5), (1, 5), (16, 5), (195, 2), (903, 8), (6271, 49), (7, 3)):
        _, ranges = C.slab_ranges(R, splits)
        assert all(hi >= lo for lo, hi in ranges) and sum(hi - lo for lo, hi in ranges) == R and ranges[0][0] == 0
        assert all(a[1] == b[0] or b[1] == b[0] for a, b in zip(ranges, ranges[1:]))


def test_device_split_equals_the_hosts_with_every_sample_kept():
    """The kernel comment's claim: choose_split makes rows = ceil8(ceil(M / s)) from a count s and launches S = ceil(M / rows) slabs;
    the masked kernel recomputes ceil8(ceil(M / S)) from S.  They are equal for M = 1 .. 20000 at every admissible s (1 572 512
    cases): the masked launch then sums exactly the ranges the unmasked one does, which its bit equality rests on."""
    M = np.arange(1, 20001)
    smax = -(-M // 128)
    Ms = np.repeat(M, smax)
    s = np.concatenate([np.arange(1, k + 1) for k in smax])
    rows = -(-(-(-Ms // s)) // 8) * 8
    S = -(-Ms // rows)
    device = -(-(-(-Ms // S)) // 8) * 8
    assert len(Ms) == 1572512 and (device == rows).all()
    for M, N, K in [(ns * rps, N, K) for ((ns, rps), N, K), _ in C.MASKED_PROBLEMS]:          # and through the transcribed rule itself
        for target in (1024, 512, 341, 256, 768):
            S, rows = G.choose_split(M, N, K, target)
            assert C.slab_ranges(M, S)[0] == rows


# ------------------------------------------------------------------------------------------------
# the multiply-high quotient
# ------------------------------------------------------------------------------------------------
def test_multiply_high_quotient_is_exact_up_to_the_admitted_bound():
    """fdiv1 with fdiv_magic(rows_per_sample) equals n // rows_per_sample for EVERY dividend a launch of up to 256 samples can form
    (logical rows up to M + 63), at each rows_per_sample of the tables and at the extreme (256, 4095); (256, 4096) is outside."""
    for rps in sorted({g[1] for g in C.GEOMETRIES}) + [C.BOUND["accepted"][1]]:
        assert C.order_accepted(C.MAX_SAMPLES, rps) and C.mask_accepted(C.MAX_SAMPLES, rps)
        n = np.arange(C.MAX_SAMPLES * rps + 64, dtype=np.uint64)
        assert np.array_equal(C.fdiv1(n, C.fdiv_magic(rps)), n // np.uint64(rps)), rps
    assert C.fdiv_magic(1) == 0
    ns, rps = C.BOUND["accepted"]
    assert (ns * rps + 63) * rps == 4293128385 < 2 ** 32
    ns, rps = C.BOUND["refused"]
    assert not C.order_accepted(ns, rps) and not C.mask_accepted(ns, rps) and ns * rps * rps == 2 ** 32
    # past the bound the quotient does go wrong (not at 4096, a power of two: the bound is sufficient, not necessary)
    d = 4097
    m = C.fdiv_magic(d)
    n = next(k * d - 1 for k in range(1, 2 ** 21) if ((k * d - 1) * m) >> 32 != (k * d - 1) // d)
    assert n * d >= 2 ** 32


# ------------------------------------------------------------------------------------------------
# sensitivity
# ------------------------------------------------------------------------------------------------
# wrong variant -> the table row that catches it (shape or problem, form, keep pattern) and the assertion of check_mapped / check_masked
SENSITIVITY = [
    ("nlive_floor", (5, 52, 36, 36), ("fwd", "plain"), "first", "kept rows of y are not the unmapped"),
    ("scale_logical", (256, 5, 388, 36), ("fwd", "res_factors"), "rows64p1", "kept rows of y are not the unmapped"),
    ("quotient_early", (65, 3, 36, 100), ("dgrad", "plain"), "every_other", "not finite|kept rows of dx are not the unmapped"),
    ("residual_scaled", (24, 49, 516, 4), ("fwd", "res"), "every_other", "not its residual row"),
]
SENSITIVITY_MASKED = [
    ("second_trip_from_0", ((130, 7), 68, 100), "all_but_64"),
    ("drop_last_granule", ((65, 3), 36, 68), "neighbours"),
]


def pattern(ns, rps, name):
    return next(keep for names, keep in C.unique_patterns(ns, rps) if name in names.split("+"))


@pytest.mark.parametrize("wrong,shape,form,name,message", SENSITIVITY, ids=[s[0] for s in SENSITIVITY])
def test_assertions_catch_a_wrong_order(wrong, shape, form, name, message):
    assert (shape in [s for s, _ in C.MAPPED_SHAPES]) and form in C.FORMS
    inp, ref, plain, zero = model_runs(form, shape)
    keep = pattern(shape[0], shape[1], name)
    args = (form, plain, zero, ref, inp, keep, C.rms_metric, RTOL)
    C.check_mapped("right", form, model_launch(form, inp, keep), *args[1:])
    bad = model_launch(form, inp, keep, wrong=wrong)
    with pytest.raises(AssertionError, match=message):
        C.check_mapped("wrong", form, bad, *args[1:])
    # bit equality is what sees it: the same rows against float64 alone, at the suite's bound
    rows = np.repeat(keep, shape[1])
    k = "dx" if form[0] == "dgrad" else "y"
    if wrong != "residual_scaled" and np.isfinite(bad[k]).all():
        err = C.rms_metric(bad[k][rows], ref[k][rows])
        print(f"{wrong}: max|diff|/rms over the kept rows = {err:.3e}")
        assert err > 10 * RTOL


@pytest.mark.parametrize("wrong,problem,name", SENSITIVITY_MASKED, ids=[s[0] for s in SENSITIVITY_MASKED])
def test_assertions_catch_a_wrong_mask(wrong, problem, name):
    assert problem in [p for p, _ in C.MASKED_PROBLEMS]
    (ns, rps), N, K = problem
    dy, x = C.masked_inputs(sid((ns, rps, N, K)), ns, rps, N, K)
    keep = pattern(ns, rps, name)
    rows = np.repeat(keep, rps)
    dyp, xp = dy.copy(), x.copy()
    dyp[~rows], xp[~rows] = C.NAN, C.NAN
    mask, ref = np.where(keep, 1.25, 0.0), C.masked_reference(dy, x, keep, None, rps)
    splits = masked_splits(ns * rps, N, K)
    C.check_masked("right", *C.model_masked(dyp, xp, mask, None, rps, splits), *ref, C.rms_metric, RTOL)
    bad = C.model_masked(dyp, xp, mask, None, rps, splits, wrong=wrong)
    with pytest.raises(AssertionError):
        C.check_masked("wrong", *bad, *ref, C.rms_metric, RTOL)
    # ... and without the NaN rows the bound alone sees it
    dw, db = C.model_masked(dy, x, mask, None, rps, splits, wrong=wrong)
    errs = (C.rms_metric(dw, ref[0]), C.rms_metric(db, ref[1]))
    print(f"{wrong}: dw {errs[0]:.3e} dbias {errs[1]:.3e}")
    assert min(errs) > 10 * RTOL


# ------------------------------------------------------------------------------------------------
# routes and coverage
# ------------------------------------------------------------------------------------------------
def tail_request(case, order=1, njobs=2):
    probs = " ".join(f"{ns * rps} {N} {K} 0 {rps} {int(name is not None)} 1 1 -1" for (ns, rps), N, K, name in case["problems"])
    ns, rps, N, K = case["dgrad"]
    return f"batch {len(case['problems'])} 0 {probs} 1 {ns * rps} {N} {K} 1 1 {order} {njobs}"


def test_routes_of_the_tail_cases(plan_tool):
    """What gemm_plan.h's batch_route gives the launches of test_tail_with_an_order: the skip kernel with and without a mask, the
    masked kernel for the comparison call, and separate launches behind the mapped data gradient for a problem with N = 30."""
    for name, case in C.TAIL_CASES.items():
        plans, route = plan_tool([tail_request(case)])[0].split(" ; ")
        assert route == case["route"], name
        assert " V4 E4" in plans.split(" | ")[-1], name                   # the data gradient has 16-B accesses: it can take the order
    assert plan_tool([tail_request(C.TAIL_CASES["masks"], order=0)])[0].split(" ; ")[1] == C.TAIL_MASKED_ROUTE
    assert {c["route"].split()[0] for c in C.TAIL_CASES.values()} | {C.TAIL_MASKED_ROUTE.split()[0]} == {"tail_order", "tail_masked", "separate"}
    assert "dgrad_first" in C.TAIL_CASES["separate"]["route"]
    # the slabs of the masked problems, from the header
    for ((ns, rps), N, K), slabs in C.MASKED_PROBLEMS:
        got = plan_tool([f"batch 1 0 {ns * rps} {N} {K} 0 {rps} 1 1 1 -1 0 0 0 0 1 1 0 0"])[0]
        assert got.split(" ; ")[1] == "masked" and f" {slabs[0]}x{slabs[1]}(" in got, got


def test_case_tables_reach_every_configuration():
    shapes = [s for s, _ in C.MAPPED_SHAPES]
    # every tile configuration, for the forward and for the data gradient, with ragged column tiles and a ragged last k-step
    by_config = {}
    for (ns, rps, cols, red), config in C.MAPPED_SHAPES:
        M = ns * rps
        assert G.tiled_config(M, cols, red, 1, G.one_split(red), False, 0) == config
        for p in (G.gemm_plan("fwd", M, cols, red), G.gemm_plan("dgrad", M, red, cols)):
            assert p["tile"] + (p["bk"], p["kw"]) == config and (p["vec"], p["store"]) == (4, 4), (ns, rps, cols, red)
        assert cols % 4 == 0 and red % 4 == 0 and cols % 32 != 0 and red % 32 != 0
        assert C.order_accepted(ns, rps)
        by_config.setdefault(config, set()).add((ns, rps))
    assert set(by_config) == set(G.FP32_CONFIGS)
    for config, geos in by_config.items():
        assert len(geos) >= 3 and any(ns > 64 for ns, _ in geos), config
    # every form, every geometry and geometry class
    assert set(SKIP_FORMS) < set(C.FORMS) and {("fwd", "nobias"), ("fwd", "res_factors")} <= set(C.FORMS)
    assert {s[:2] for s in shapes} == set(C.GEOMETRIES)
    geos = C.GEOMETRIES
    assert any(ns == 1 for ns, _ in geos) and any(rps == 1 and ns > 1 for ns, rps in geos) and any(ns == C.MAX_SAMPLES for ns, _ in geos)
    assert any(rps >= 10 * C.BM for _, rps in geos) and any(64 < ns < 128 for ns, _ in geos) and any(128 < ns < 192 for ns, _ in geos)
    assert any(rps % 8 and rps < 8 and rps > 1 for _, rps in geos)           # sample borders inside every 8-row epilogue group
    # keep patterns: mixed tiles, fill tiles, kept rows on each side of a tile border, both sides of the 64-sample ballot
    classes, rems = set(), set()
    for ns, rps in geos:
        pats = C.keep_patterns(ns, rps)
        assert {"first", "last", "every"} <= set(pats) and not any(k.all() for k in pats.values())
        if ns > 64:
            assert {"only_63_64", "only_last", "all_but_64", "rows64", "rows64p1", "rows64m1"} <= set(pats), (ns, rps)
            both = [k for k in pats.values() if k[:64].any() and k[64:].any()]
            assert both and any(not k[:64].any() and k[64:].any() for k in pats.values())
        for k in pats.values():
            kept = int(k.sum()) * rps
            live, mixed, fill = C.tile_classes(kept, ns * rps)
            classes.add((live > 0, mixed, fill > 0))
            rems.add(kept % 64 if kept >= 63 else None)
    assert {(True, 1, True), (True, 0, True), (False, 0, True), (True, 1, False), (False, 1, True)} <= classes and {0, 1, 63} <= rems
    # masked problems: every geometry beyond 64 samples and (2, 3136), ragged 64-tiles, the host's slabs; batches mix sample counts
    assert {p[0] for p, _ in C.MASKED_PROBLEMS} == {g for g in geos if g[0] > 64} | {(2, 3136)}
    for ((ns, rps), N, K), slabs in C.MASKED_PROBLEMS:
        assert G.choose_split(ns * rps, N, K, 1024) == slabs and {N, K} <= {36, 68, 100} and C.mask_accepted(ns, rps)
    assert {n for (_, n, k), _ in C.MASKED_PROBLEMS} | {k for (_, n, k), _ in C.MASKED_PROBLEMS} == {36, 68, 100}
    for batch in C.MASKED_BATCHES:
        assert len(batch) == 4 and len({g for g, *_ in batch}) == 4 and any(p[3] is None for p in batch) and sum(p[3] is not None for p in batch) >= 2
        assert any(g[0] > 64 for g, *_ in batch) and any(g[0] <= 64 for g, *_ in batch)
        assert all(p[3] is None or p[3] in C.keep_patterns(*p[0]) for p in batch)
    # both sides of fdiv's bound
    assert C.order_accepted(*C.BOUND["accepted"]) and C.mask_accepted(*C.BOUND["accepted"])
    assert not C.order_accepted(*C.BOUND["refused"]) and not C.mask_accepted(*C.BOUND["refused"])
    # the tail: more than 64 samples, a ragged data gradient, masks of two kinds and a problem without; N = 30 for the separate route
    t = C.TAIL_CASES
    assert t["masks"]["dgrad"][0] > 64 and t["masks"]["dgrad"][3] in (36, 100)
    names = [p[3] for p in t["masks"]["problems"]]
    assert len(names) == 4 and None in names and len({n for n in names if n}) == 2
    assert all(p[3] is None for p in t["no_mask"]["problems"]) and len(t["no_mask"]["problems"]) == 4
    assert [p[1] for p in t["separate"]["problems"]] == [30] and t["separate"]["problems"][0][3] is None
    # every wrong variant of the model is named with the row that catches it
    assert {s[0] for s in SENSITIVITY} | {s[0] for s in SENSITIVITY_MASKED} == {
        "nlive_floor", "scale_logical", "quotient_early", "second_trip_from_0", "drop_last_granule", "residual_scaled"}
