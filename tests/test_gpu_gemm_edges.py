"""The two ends of the GEMM family's k-loop (cswin_unet_amd/csrc/gemm.hip, gemm_body; gemm_epilogue.h, epilogue_request / run_epilogue):
the epilogue's operands -- bias, row factors, residual / gelu_pre rows -- are requested in front of the last k-tile's MFMAs, and a
masked weight gradient's workgroup lists its kept samples in front of its first operand load.  Moving such loads changes no bit of
any result; these tests stand at the sizes where a moved load could go wrong.

Reductions.  The request point is in front of the ONLY tile when a workgroup has one k-tile, and a fill tile (no k-loop) requests in
front of its epilogue.  The two tile configurations with a 32-wide k-tile and one wave group, (64, 32, 32, 1) and (64, 64, 32, 1),
run at K = 4 and 32 (one k-tile) and K = 36 and 68 (a ragged last tile of 4).  The host gives two and four wave groups only to
reductions of 256 and 512 on (k_groups of tests/test_gpu_gemm_shapes.py's transcription), so (64, 32, 64, 2), (64, 64, 64, 2) and
(64, 64, 64, 4) run at the smallest reductions that select them, 256 and 512 -- four and eight 64-wide tiles, each wave group one
slice of every tile -- and at 260 and 516 (ragged last tile).  Every configuration is asserted with the transcription.
Geometries: 3 and 24 samples of 49 and 196 rows.  Forms: droppath_cases.FORMS, which holds every epilogue with auxiliary operands
(residual + row factor, GELU' + row factor, row factor alone, bias alone, bias + GELU) and the two without any (forward without a
bias, plain data gradient).  Keep patterns: every sample kept, the first / the last / all but one dropped, every sample dropped
(fill tiles only), with NaN in the dropped samples' rows of A and gelu_pre.

Edges.  M = 65, N = 36 (5 samples of 13 rows): the second row tile has one live row, the second column tile four live columns.
residual and gelu_pre are exact-size views with NaN in front of and behind them in the same allocation, and row_scale and bias
likewise, so a lane with m >= M or n >= N that loads and uses what lies beside its matrix makes the output non-finite.

Every comparison of a launch with an order against its twin without one is exact (np.array_equal), dropped rows are compared
exactly with the bias, GELU(bias), the residual row or +0, and the unmapped launch is held to float64 by the family's bound (RTOL
of tests/test_gpu_parity.py through tests/test_gpu_gemm_shapes.py), all in droppath_cases.check_mapped / Mapped.check_patterns.

Masks.  Weight gradients with sample masks at 1, 63, 64, 65 and 256 samples: kept samples on both sides of every 64-lane border
(63 | 64, 127 | 128, 191 | 192), slices that keep nothing in front of slices that do, every sample dropped.  The operands are small
integers and the factors 1.25 / 0.75, so every product and every partial sum is exact in fp32 and the result does not depend on the
summation order: the masked launch must equal (np.array_equal) the unmasked entry point's result on the compacted operands, and the
float64 sum of droppath_cases.model_masked over the NumPy model's kept list and slab ranges, rounded to fp32.  The list's order
itself (ascending, whatever slice a sample sits in) is droppath_cases.kept_list's, asserted beside it."""
import types

import numpy as np
import pytest
import torch

import droppath_cases as C
from oracle.determ import det_normal
from test_gpu_attn_shapes import Guarded, settle
from test_gpu_droppath_shapes import Mapped, T, default_launch_plan, launch, sid        # noqa: F401 (the fixture applies here too)
from test_gpu_gemm_shapes import choose_split, one_split, tiled_config

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
FENCE = 64                     # NaN floats in front of and behind a fenced operand (256 B: the view stays 16-B aligned)

# ((samples, rows per sample, output columns), reductions, the host's configuration)
EDGE_SHAPES = [
    ((3, 49, 96), (4, 32, 36, 68), (64, 32, 32, 1)),
    ((24, 196, 64), (4, 36), (64, 32, 32, 1)),
    ((3, 196, 1024), (4, 32, 36, 68), (64, 64, 32, 1)),
    ((24, 49, 512), (4, 68), (64, 64, 32, 1)),
    ((24, 49, 64), (256, 260), (64, 32, 64, 2)),
    ((3, 196, 1024), (256, 260), (64, 64, 64, 2)),
    ((24, 49, 512), (512, 516), (64, 64, 64, 4)),
]
EDGE_CASES = [(g + (red,), config) for g, reds, config in EDGE_SHAPES for red in reds]
PATTERNS = ("first", "last", "all_but_one", "every")


def patterns(ns, rps):
    p = C.keep_patterns(ns, rps)
    return [(name, p[name]) for name in PATTERNS]


def fenced(a):
    """Device copy of a float32 array as an exact-size view with FENCE NaN floats on both sides in the same allocation."""
    if a is None:
        return None
    a = np.ascontiguousarray(a, np.float32)
    buf = torch.full((a.size + 2 * FENCE,), NAN, device=DEV)
    buf[FENCE:FENCE + a.size] = torch.from_numpy(a.reshape(-1)).to(DEV)
    v = buf[FENCE:FENCE + a.size].view(a.shape)
    assert v.data_ptr() % 16 == 0
    return v


@pytest.mark.parametrize("shape,config", EDGE_CASES, ids=[sid(s) for s, _ in EDGE_CASES])
def test_request_point_at_one_tile_ragged_tiles_and_fill_tiles(shape, config):
    ns, rps, cols, red = shape
    assert tiled_config(ns * rps, cols, red, 1, one_split(red), False, 0) == config
    for form in C.FORMS:
        Mapped(form, shape).check_patterns(patterns(ns, rps))


class Fenced(Mapped):
    """Mapped whose bias, residual, gelu_pre and row factors are fenced views (the poisoned gelu_pre of a run with dropped samples too)."""

    def __init__(self, form, shape):
        super().__init__(form, shape)
        i = self.inp
        self.bias, self.residual, self.pre = fenced(i["bias"]), fenced(i["residual"]), fenced(i["pre"])

    def run(self, keep=None, *, skip, poison=False, zero_a=False, order=None, what=""):
        from cswin_unet_amd._lib import call, ptr, stream
        entry, f = self.form
        keep = np.ones(self.ns, bool) if keep is None else keep
        rows = np.repeat(keep, self.rps)
        a = np.zeros_like(self.inp["a"]) if zero_a else self.inp["a"].copy()
        pre = self.pre
        if poison and not keep.all():
            a[~rows] = NAN
            if pre is not None:
                p = self.inp["pre"].copy()
                p[~rows] = NAN
                pre = fenced(p)
        a = T(a)
        rs = fenced(C.row_scale_of(self.form, keep))
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


@pytest.mark.parametrize("red", [4, 36])
def test_edge_lanes_load_nothing_beside_their_matrices(red):
    shape = (5, 13, 36, red)                       # M = 65, N = 36
    assert tiled_config(65, 36, red, 1, one_split(red), False, 0) == (64, 32, 32, 1)
    for form in C.FORMS:
        Fenced(form, shape).check_patterns(patterns(5, 13))


# ------------------------------------------------------------------------------------------------
# masked weight gradients
# ------------------------------------------------------------------------------------------------
def only(ns, *kept):
    return np.isin(np.arange(ns), kept)


def masks_of(ns):
    """name -> kept flags for ns samples: see the module docstring."""
    m = {"all": np.ones(ns, bool), "none": np.zeros(ns, bool), "last": only(ns, ns - 1), "first_dropped": ~only(ns, 0),
         "every_other": np.arange(ns) % 2 == 1}
    if ns >= 63:
        m.update(only_62=only(ns, 62), all_but_62=~only(ns, 62))
    if ns >= 64:
        m.update(only_63=only(ns, 63), all_but_63=~only(ns, 63))
    if ns >= 65:
        m.update(only_63_64=only(ns, 63, 64), only_64=only(ns, 64), all_but_64=~only(ns, 64))
    if ns >= 256:
        m.update(borders=only(ns, 63, 64, 127, 128, 191, 192), only_128_on=np.arange(ns) >= 128, only_192=only(ns, 192),
                 all_but_borders=~only(ns, 64, 128, 192))
    seen = {}
    for name, keep in m.items():
        seen.setdefault(keep.tobytes(), (name, keep))
    return dict(seen.values())


def small_ints(tag, shape):
    return np.clip(np.rint(2.0 * det_normal(tag, shape)), -4, 4).astype(np.float32)


def problem(tag, ns, rps, N, K, keep, scaled, bias=True):
    """A weight gradient as test_gpu_droppath_shapes.launch takes it, with integer operands; keep = None: no mask.  NaN in the
    dropped samples' rows of both operands."""
    dy, x = small_ints(f"edges.{tag}.dy", (ns * rps, N)), small_ints(f"edges.{tag}.x", (ns * rps, K))
    kept = np.ones(ns, bool) if keep is None else np.asarray(keep, bool)
    scale = np.where(kept, np.where(np.arange(ns) % 3 == 0, 0.75, 1.25), 0.0).astype(np.float32) if scaled else None
    rows = np.repeat(kept, rps)
    pdy, px = dy.copy(), x.copy()
    pdy[~rows], px[~rows] = NAN, NAN
    return types.SimpleNamespace(tag=tag, ns=ns, rps=rps, M=ns * rps, N=N, K=K, bias=bias, dy=T(pdy), x=T(px), scale=T(scale),
                                 mask=None if keep is None else T(np.where(kept, 1.25, 0.0).astype(np.float32)),
                                 host=(dy, x, kept, scale))


def compacted(p):
    """The unmasked problem over the kept samples' rows alone (None: nothing is kept)."""
    dy, x, kept, scale = p.host
    if not kept.any():
        return None
    rows = np.repeat(kept, p.rps)
    nk = int(kept.sum())
    return types.SimpleNamespace(tag=p.tag + ".compacted", ns=nk, rps=p.rps, M=nk * p.rps, N=p.N, K=p.K, bias=p.bias, dy=T(dy[rows]), x=T(x[rows]),
                                 scale=None if scale is None else T(scale[kept]), mask=None, host=None)


def check_masked_problem(what, p, got, splits):
    dy, x, kept, scale = p.host
    dw, db = got
    assert np.array_equal(C.kept_list(kept), np.flatnonzero(kept)), what
    mdw, mdb = C.model_masked(dy, x, kept, scale, p.rps, splits)
    assert np.abs(mdw).max(initial=0.0) < 2 ** 22 and np.abs(mdb).max(initial=0.0) < 2 ** 22          # exact in fp32 at every partial sum
    assert np.array_equal(dw, mdw.astype(np.float32)) and np.array_equal(db, mdb.astype(np.float32)), f"{what}: not the model's sums"
    c = compacted(p)
    if c is None:
        assert not dw.any() and not db.any(), f"{what}: a reduction over no rows is not exact zeros"
        return
    (want,), _, _ = launch(what + ".compacted", [c], masked=False)
    assert np.array_equal(dw, want[0]) and np.array_equal(db, want[1]), f"{what}: not the unmasked launch of the compacted operands"


@pytest.mark.parametrize("ns", [1, 63, 64, 65, 256])
def test_masked_weight_gradient_lists_across_the_64_lane_borders(ns):
    rps, N, K = 3, 36, 68
    splits = choose_split(ns * rps, N, K, 1024)[0]          # a batch of one: the per-problem target 1024 / n
    for scaled in (False, True):
        for name, keep in masks_of(ns).items():
            what = f"edges.mask.{ns}.{int(scaled)}.{name}"
            p = problem(f"{ns}.{int(scaled)}", ns, rps, N, K, keep, scaled)
            (got,), _, _ = launch(what, [p], masked=True)
            check_masked_problem(what, p, got, splits)


def test_masked_batch_of_four_sample_counts():
    """63, 64, 65 and 256 samples in ONE launch: all but lane 62, lane 63 alone, both sides of the first border, of every border."""
    spec = [(63, "all_but_62", True), (64, "last", False), (65, "only_63_64", True), (256, "borders", True)]
    probs = [problem(f"batch.{ns}", ns, 3, 36, 68, masks_of(ns)[name], scaled) for ns, name, scaled in spec]
    outs, _, _ = launch("edges.mask.batch", probs, masked=True)
    for p, got in zip(probs, outs):
        check_masked_problem(f"edges.mask.batch.{p.ns}", p, got, choose_split(p.M, p.N, p.K, 1024 // len(probs))[0])
