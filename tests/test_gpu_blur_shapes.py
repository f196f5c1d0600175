"""cswin_gaussian_blur (csrc/blur.hip) called directly, at every tile plan and launch branch: the cases of
blur_cases.PLAN_CASES (one per plan signature that csrc/blur_plan.h can return, and the kernel branches beside them; the host
side of that claim is tests/test_blur_host.py), both load widths at the same shape, one NaN in a finite slice, the float32 value
classes a filter can mishandle, the limits of the entry point, repeated and captured launches, and the refusals.

Every call reads its input from a view into a NaN-filled buffer (a load outside the slices poisons the result) and writes into a
NaN-filled one: every element must have been written, the guard words of both must be intact and the input's bits unchanged.
The taps are utils.gaussian_taps_device's, and every call is followed by a synchronize.

Criterion: that of tests/test_gpu_blur.py (its own check is used): finite wherever scipy is, within one float32 ulp of scipy, at
most 1 element in 1e5 not bit-equal.  Every case here has fewer than 1e5 elements, so the cap means 0 -- which is what the numpy
emulation of the device's arithmetic gives on these very inputs (tests/test_blur_host.py).  The count of every case is printed.
Where the reference holds NaN, the position of a NaN is compared and not its payload."""
import ctypes

import numpy as np
import pytest
import torch

import blur_cases as B
from test_gpu_blur import _check_against_scipy
from test_gpu_step_tail import ERR_ALIGN, ERR_SHAPE, ERR_UNSUPPORTED, Guarded, GuardedAt, bits32, hip, put, release_inputs, settle  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 1.5e-20                     # prefill of an output that may hold NaN: no result here equals it
rid = lambda v: B.case_id(v) if isinstance(v, tuple) else f"r{v}"


def taps_of(r):
    from cswin_unet_amd.utils import gaussian_taps_device
    taps, radius = gaussian_taps_device(B.sigma_of(r), 4.0, torch.device(DEV))
    assert radius == r and taps.dtype == torch.float64 and taps.numel() == r + 1 and taps.data_ptr() % 16 == 0
    return taps


def blur(hip, x, r, what, xoff=0, yoff=0, taps=None, nan_ok=False, runs=1):
    """cswin_gaussian_blur of the numpy slices x (D, H, W) with x / y `xoff` / `yoff` float32 past a 16-byte boundary; the checks
    of the module docstring; the result as numpy.  nan_ok: the result may hold NaN, so the output starts as SENTINEL (the guards
    stay NaN) and it is the comparison with the reference that shows every element written."""
    D, H, W = x.shape
    gx, gy = GuardedAt(x.shape, off=xoff), GuardedAt(x.shape, off=yoff)
    gx.t.copy_(torch.from_numpy(np.array(x)))
    before = bits32(gx.buf)
    if nan_ok:
        gy.t.fill_(SENTINEL)
    taps = taps_of(r) if taps is None else taps
    torch.cuda.synchronize()
    for _ in range(runs):
        hip.call("cswin_gaussian_blur", hip.ptr(gx.t), hip.ptr(gy.t), hip.ptr(taps), r, D, H, W, hip.stream())
        torch.cuda.synchronize()
    assert gx.intact() and gy.intact(), f"{what}: a guard word was overwritten"
    assert nan_ok or gy.written(), f"{what}: output elements were never written"
    assert np.array_equal(bits32(gx.buf), before), f"{what}: the input was written to"
    return gy.t.cpu().numpy()


def check_special(got, want, what):
    """Bits equal scipy's, NaN where scipy has NaN (position, not payload); nothing is left of the prefill."""
    unequal = B.unequal_bits_or_nan(got, want)
    print(f"{what}: {unequal} of {got.size} elements not bit-equal; reference: {int(np.isnan(want).sum())} NaN, {int(np.isinf(want).sum())} inf")
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN in other places than scipy's"
    assert np.array_equal(np.isfinite(got), np.isfinite(want)), f"{what}: not finite where scipy is"
    assert unequal == 0


@pytest.mark.parametrize("case", B.PLAN_CASES, ids=B.plan_case_id)
def test_every_plan_and_branch_against_scipy(hip, case):
    shape, r, off = case
    x, want = B.plan_inputs(case)
    f = B.launch_facts(shape, r, B.plan_vec(case))
    what = f"{B.plan_case_id(case)} vec {f['vec']} TR {f['plan'].TR} CW {1 << f['plan'].cw_log2} budget {f['plan'].budget} grid {f['grid']}"
    _check_against_scipy(blur(hip, x, r, what, xoff=off), want, what)


# x 4 bytes off an 8-byte boundary at an even W: the 4-byte loads with 128- and 256-column chunks and two tiles
ALIGN_CASES = [((2, 18, 130), 4, 7), ((2, 15, 130), 0, 8)]


@pytest.mark.parametrize("shape,r,cwl", ALIGN_CASES, ids=lambda v: B.case_id(v) if isinstance(v, tuple) else f"{v}")
def test_pointer_offsets_give_the_aligned_bits(hip, shape, r, cwl):
    f1, f2 = B.launch_facts(shape, r, 1), B.launch_facts(shape, r, 2)
    assert f1["plan"].cw_log2 == cwl and f1["tiles"] >= 2 and f2["tiles"] >= 2        # what the case is here for
    x, want = B.slices(shape, B.sigma_of(r)), B.scipy_blur_case(shape, B.sigma_of(r))
    aligned = blur(hip, x, r, "aligned")
    _check_against_scipy(aligned, want, f"{shape} r {r} aligned")
    taps8 = put(taps_of(r), off=1)                                                     # float64: 8 mod 16
    assert taps8.data_ptr() % 16 == 8
    for what, kw in (("x 4 bytes off", dict(xoff=1)), ("x 12 bytes off", dict(xoff=3)), ("x at 8 mod 16", dict(xoff=2)),
                     ("y 4 bytes off", dict(yoff=1)), ("y at 8 mod 16", dict(yoff=2)), ("x and y 4 bytes off", dict(xoff=1, yoff=1)),
                     ("taps at 8 mod 16", dict(taps=taps8))):
        got = blur(hip, x, r, what, **kw)
        unequal = B.unequal_bits(got, aligned)
        print(f"{shape} r {r} {what}: {unequal} of {got.size} elements differ from the aligned run")
        assert unequal == 0, what


@pytest.mark.parametrize("r", B.NAN_RADII)
def test_one_nan_has_scipys_footprint(hip, r):
    for name, at in B.nan_positions(r):
        x = B.nan_input(r, at)
        want = B.scipy_blur_quiet(x, B.sigma_of(r))
        check_special(blur(hip, x, r, f"NaN at {name}", nan_ok=True), want, f"r {r} NaN at {name} {at}")


@pytest.mark.parametrize("r", B.SPECIAL_RADII)
@pytest.mark.parametrize("name", B.SPECIAL_NAMES)
def test_special_values_have_scipys_bits(hip, name, r):
    x = B.special_input(name)
    want = B.scipy_blur_quiet(x, B.sigma_of(r))
    for off in (0, 1):                                                                 # both load widths
        check_special(blur(hip, x, r, name, xoff=off, nan_ok=True), want, f"{name} r {r} x offset {off}")


LIMIT_CASES = [((2048, 1, 2), 4), ((1, 2048, 1), 4), ((1, 1, 2048), 4), ((1, 3, 2048), 32)]


@pytest.mark.parametrize("shape,r", LIMIT_CASES, ids=rid)
def test_the_limits_of_the_entry_point(hip, shape, r):
    x, want = B.slices(shape, B.sigma_of(r)), B.scipy_blur_case(shape, B.sigma_of(r))
    assert max(shape) == 2048 and x.size < 100000
    _check_against_scipy(blur(hip, x, r, f"{shape} r {r}"), want, f"{shape} r {r}")


# the template and the generic kernel, several tiles and chunks each
REPLAY_CASES = [((2, 18, 130), 4), ((2, 15, 66), 32)]


@pytest.mark.parametrize("shape,r", REPLAY_CASES, ids=rid)
def test_repeated_and_captured_launches_give_the_same_bits(hip, shape, r):
    x, want = B.slices(shape, B.sigma_of(r)), B.scipy_blur_case(shape, B.sigma_of(r))
    once = blur(hip, x, r, "once")
    _check_against_scipy(once, want, f"{shape} r {r}")
    assert B.unequal_bits(blur(hip, x, r, "twice", runs=2), once) == 0
    # one kernel, no branches: captured on a side stream, replayed twice
    D, H, W = shape
    gx, gy, taps = GuardedAt(shape), GuardedAt(shape), taps_of(r)
    gx.t.copy_(torch.from_numpy(np.array(x)))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        hip.call("cswin_gaussian_blur", hip.ptr(gx.t), hip.ptr(gy.t), hip.ptr(taps), r, D, H, W, hip.stream())
    torch.cuda.synchronize()
    for n in range(2):
        gy.t.fill_(float("nan"))
        graph.replay()
        settle(f"replay {n}", {"y": gy, "x": gx})
        assert B.unequal_bits(gy.t.cpu().numpy(), once) == 0, n
    del graph


def test_refusals_touch_nothing(hip):
    shape, r = (2, 8, 8), 4
    gx, gy, taps = GuardedAt(shape), GuardedAt(shape), taps_of(r)
    gx.t.copy_(torch.from_numpy(np.array(B.slices(shape, 1.0))))
    o = {"y": gy}
    P, st = hip.ptr, hip.stream()
    at = lambda t, nbytes: ctypes.c_void_p(t.data_ptr() + nbytes)

    def args(x=P(gx.t), y=P(gy.t), w=P(taps), radius=r, D=2, H=8, W=8):
        return (x, y, w, radius, D, H, W, st)
    name = "cswin_gaussian_blur"
    hip.refused(ERR_SHAPE, "x null", o, name, *args(x=None))
    hip.refused(ERR_SHAPE, "y null", o, name, *args(y=None))
    hip.refused(ERR_SHAPE, "taps null", o, name, *args(w=None))
    hip.refused(ERR_UNSUPPORTED, "x == y", o, name, *args(x=P(gy.t)))
    assert b"in place" in hip.lib().cswin_last_error()
    for dim in "DHW":
        for n in (0, 2049):
            hip.refused(ERR_SHAPE, f"{dim} = {n}", o, name, *args(**{dim: n}))
    for radius in (-1, 33):
        hip.refused(ERR_UNSUPPORTED, f"radius {radius}", o, name, *args(radius=radius))
    hip.refused(ERR_ALIGN, "x 2 bytes off", o, name, *args(x=at(gx.t, 2)))
    hip.refused(ERR_ALIGN, "y 2 bytes off", o, name, *args(y=at(gy.t, 2)))
    hip.refused(ERR_ALIGN, "taps 4 bytes off", o, name, *args(w=at(taps, 4)))
    assert b"gaussian_blur" in hip.lib().cswin_last_error()
    want = B.scipy_blur_case(shape, 1.0)                                               # and the same buffers then take a legal call
    hip.call(name, *args())
    settle("after the refusals", {"y": gy, "x": gx})
    assert B.unequal_bits(gy.t.cpu().numpy(), want) == 0
