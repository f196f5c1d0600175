"""The eb-criterion kernels (csrc/eb.hip: cswin_eb_tiles, cswin_eb_finalize) called directly on guarded buffers, away from the
model's layout: one-column tensors of 1 to 2048 rows (256 row phases, both sides of a full trip), column counts on both sides of
the 16- and 64-wide tiles and no multiple of 4, a tile of 2048 rows x 64 columns, and 257 tensors for the finalize kernel's second
trip.  Reference, bound and inputs are test_eb_host's (float64; the bound is derived there from the kernel's operations and shown
to see the bugs it is for).  The pad words of the gradient buffer hold NaN, so a kernel that reads one poisons its tensor."""
import math

import numpy as np
import pytest
import torch

from test_adamw_host import elem_mask, flat, slots
from test_eb_host import MANY, SHAPES, eb_bound, eb_fp32, eb_inputs, eb_ref
from test_gpu_step_tail import ERR_ALIGN, ERR_SHAPE, Guarded, GuardedAt, bits32, hip, put, release_inputs  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda"


def layout(shapes):
    """(device tile table, device first_tile, device numel, tile count, offsets, numels, tiles per tensor) of a list of shapes."""
    from cswin_unet_amd.optim import column_tiles
    numels = [math.prod(s) for s in shapes]
    offs, _ = slots(numels)
    rows, first = column_tiles(shapes, offs)
    return put(rows.view(np.int64).reshape(-1, 4)), put(first), put(np.array(numels, np.int32)), len(rows), offs, numels, np.diff(first)


def grad_buffer(gs, numels):
    g = Guarded((slots(numels)[1],))
    g.t.copy_(torch.from_numpy(flat([a.reshape(-1) for a in gs], numels, fill=float("nan"))).to(DEV))
    return g


def evidence(hip, gs, shapes, what):
    """Both launches on guarded outputs: (partial, evidence) as numpy.  The guard words and every word of the gradient buffer, its
    NaN pad words included, must come back bit for bit."""
    tiles, first, numel, ntiles, _, numels, _ = layout(shapes)
    g = grad_buffer(gs, numels)
    g0 = bits32(g.buf)
    o = dict(partial=Guarded((ntiles,)), evidence=Guarded((len(shapes),)))
    hip.call("cswin_eb_tiles", hip.ptr(g.t), hip.ptr(tiles), ntiles, hip.ptr(o["partial"].t), hip.stream())
    hip.call("cswin_eb_finalize", hip.ptr(o["partial"].t), hip.ptr(first), hip.ptr(numel), len(shapes), hip.ptr(o["evidence"].t), hip.stream())
    torch.cuda.synchronize()
    assert all(b.intact() for b in o.values()) and g.intact(), f"{what}: a guard word was overwritten"
    assert np.array_equal(bits32(g.buf), g0) and bool(torch.isnan(g.t[torch.from_numpy(~elem_mask(numels)).to(DEV)]).all()), f"{what}: the gradient buffer changed"
    return o["partial"].t.cpu().numpy(), o["evidence"].t.cpu().numpy()


def check(shapes, gs, got, what):
    """evidence against eb_ref within eb_bound per tensor, NaN exactly where the first dimension is 1; returns the float64 values."""
    refs, worst = [], 0.0
    for t, (s, g) in enumerate(zip(shapes, gs)):
        ref, bound = eb_ref(g, s), eb_bound(g, s)
        refs.append((ref, bound))
        if s[0] == 1:
            assert math.isnan(ref) and math.isnan(got[t]), (what, t, s, got[t])
            continue
        err = abs(float(got[t]) - ref)
        assert math.isfinite(got[t]) and math.isfinite(bound) and err <= bound, f"{what}: tensor {t} {s}: |{got[t]!r} - {ref!r}| = {err:.3e} > {bound:.3e}"
        worst = max(worst, err / bound if bound > 0 else 0.0)
    print(f"{what}: {len(shapes)} tensors, largest |error| / bound {worst:.4f}")
    return refs


@pytest.fixture(scope="module")
def runs(hip):
    """The twenty-tensor layout, twice, and the 257-tensor layout: computed once."""
    gs, many = eb_inputs("cases", SHAPES), eb_inputs("many", MANY)
    return dict(gs=gs, many=many, a=evidence(hip, gs, SHAPES, "eb.cases"), b=evidence(hip, gs, SHAPES, "eb.cases.again"),
                m=evidence(hip, many, MANY, "eb.many"))


def test_evidence_against_float64(runs):
    """Every tensor of the layout within its bound; NaN where shape[0] == 1 and nowhere else; tensors on both sides of the 0.95
    threshold by more than their bound, in float64 and in what the kernel returned."""
    partial, got = runs["a"]
    refs = check(SHAPES, runs["gs"], got, "eb.cases")
    assert [bool(np.isnan(v)) for v in got] == [s[0] == 1 for s in SHAPES] and np.isnan(got).sum() == 1
    below = [t for t, (r, b) in enumerate(refs) if r + b < 0.95]
    above = [t for t, (r, b) in enumerate(refs) if r - b > 0.95]
    assert len(below) >= 2 and len(above) >= 2, (below, above)
    assert all(got[t] < 0.95 for t in below) and all(got[t] >= 0.95 for t in above)
    same = sum(got[t].view(np.uint32) == eb_fp32(g, s)[0].view(np.uint32) for t, (s, g) in enumerate(zip(SHAPES, runs["gs"])) if s[0] > 1)
    print(f"eb.cases: {same} of {len(SHAPES) - 1} tensors have the bits of the float32 transcription (printed, not gated)")


def test_finalize_takes_a_second_trip(runs):
    """257 tensors of shape (2, 4): thread 0 of the one workgroup owns tensors 0 and 256."""
    partial, got = runs["m"]
    assert len(MANY) == 257 and partial.shape == (257,)
    check(MANY, runs["many"], got, "eb.many")
    assert np.array_equal(got.view(np.uint32), (partial / np.float32(8)).view(np.uint32))      # one tile per tensor: the partial over numel


def test_two_runs_give_the_same_bits(runs):
    """No float atomics: every sum has a fixed order."""
    for x, y in zip(runs["a"], runs["b"]):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


def test_refusals_touch_nothing(hip):
    """A null pointer, a count of 0, a gradient buffer four bytes off a 16-byte boundary and a table four bytes off an 8-byte one
    return their error codes; nothing is launched."""
    from cswin_unet_amd.optim import column_tiles
    shapes = [(9,), (5, 3)]
    tiles, first, numel, ntiles, _, numels, _ = layout(shapes)
    total = slots(numels)[1]
    rows, _ = column_tiles(shapes, slots(numels)[0])
    tiles_off = put(rows.view(np.int32), off=1)
    g, g_off = put(np.ones(total, np.float32)), put(np.ones(total, np.float32), off=1)
    o = dict(partial=Guarded((ntiles,)), evidence=Guarded((2,)))
    P = hip.ptr

    def tiles_args(g=g, tiles=tiles, n=ntiles, partial=o["partial"].t):
        return (P(g), P(tiles), n, P(partial), hip.stream())

    def fin_args(partial=o["partial"].t, first=first, numel=numel, n=2, ev=o["evidence"].t):
        return (P(partial), P(first), P(numel), n, P(ev), hip.stream())

    hip.refused(ERR_SHAPE, "eb_tiles g null", o, "cswin_eb_tiles", *tiles_args(g=None))
    hip.refused(ERR_SHAPE, "eb_tiles table null", o, "cswin_eb_tiles", *tiles_args(tiles=None))
    hip.refused(ERR_SHAPE, "eb_tiles partial null", o, "cswin_eb_tiles", *tiles_args(partial=None))
    hip.refused(ERR_SHAPE, "eb_tiles ntiles 0", o, "cswin_eb_tiles", *tiles_args(n=0))
    hip.refused(ERR_SHAPE, "eb_tiles ntiles -1", o, "cswin_eb_tiles", *tiles_args(n=-1))
    hip.refused(ERR_ALIGN, "eb_tiles g 4 bytes off", o, "cswin_eb_tiles", *tiles_args(g=g_off))
    hip.refused(ERR_ALIGN, "eb_tiles table 4 bytes off", o, "cswin_eb_tiles", *tiles_args(tiles=tiles_off))
    hip.refused(ERR_SHAPE, "eb_finalize partial null", o, "cswin_eb_finalize", *fin_args(partial=None))
    hip.refused(ERR_SHAPE, "eb_finalize first_tile null", o, "cswin_eb_finalize", *fin_args(first=None))
    hip.refused(ERR_SHAPE, "eb_finalize numel null", o, "cswin_eb_finalize", *fin_args(numel=None))
    hip.refused(ERR_SHAPE, "eb_finalize evidence null", o, "cswin_eb_finalize", *fin_args(ev=None))
    hip.refused(ERR_SHAPE, "eb_finalize ntensors 0", o, "cswin_eb_finalize", *fin_args(n=0))
    assert b"eb_" in hip.lib().cswin_last_error()
