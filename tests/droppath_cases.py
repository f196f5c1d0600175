"""Case tables and a NumPy model of the two DropPath compactions of the Linear GEMM family (cswin_unet_amd/csrc/gemm.hip, gemm_body and
run_epilogue): the SAMPLE ORDER of the forward / data-gradient Linears (RowMap, gemm_mapped_kernel, gemm_block_tail_skip_kernel) and the
SAMPLE MASK of the weight gradients (RowMask, KeptList, gemm_wgrad_batch_masked_kernel).  No GPU and no torch.cuda here:
tests/test_droppath_host.py holds the model to float64 and shows that the assertions below see a wrong compaction,
tests/test_gpu_droppath_shapes.py applies the same assertions to the kernels.

What each table row is there for
  GEOMETRIES (samples, rows per sample)
    (1, 7)     one sample: the only orders are "kept" (the identity) and "dropped" (no live tile at all)
    (7, 1)     rows_per_sample = 1: fdiv_magic is 0 and fdiv1 skips the division; a sample border between any two rows
    (5, 52)    the feature test's geometry: borders inside the 64-row tiles and inside the 8-row epilogue groups
    (24, 49)   the benchmark's batch at the stage-4 token count: 19 row tiles, borders at odd rows
    (65, 3)    one sample past the 64-lane ballot: the second trip of build_kept_list / drop_path_order_kernel holds one sample;
               three rows per sample put two or three borders into every 8-row epilogue group
    (130, 7)   three ballot trips, the last with two samples
    (256, 1)   the largest sample count (ord[] and KeptList are full), one row per sample
    (256, 5)   the largest sample count with borders inside every 8-row group
    (2, 3136)  the stage-1 token count: a sample spans 49 row tiles, 3136 = 49 * 64 so the kept rows end on a tile border
  keep_patterns: first / last / two neighbours dropped, all but one dropped, every sample dropped, every other sample dropped;
    rows64 / rows64p1 / rows64m1: the kept rows are k * 64 (no mixed tile), k * 64 + 1 (a mixed tile with one live row) and
    k * 64 - 1 (a mixed tile with one fill row); beyond 64 samples "only_63_64" (the kept list's second trip writes index 1 =
    n + popcount with n = 1), "only_last" (the first trip keeps nothing) and "all_but_64" (the second trip starts at n = 64)
  MAPPED_SHAPES: output columns and reductions that are multiples of 4 and of no tile size (ragged column tiles meet `n < N`, a ragged
    last k-step meets `j < r_end`), at each fp32 tile configuration of the host with at least three geometries, one of them beyond
    64 samples
  MASKED_PROBLEMS: every geometry beyond 64 samples and (2, 3136), with ragged 64-tiles (36, 68, 100): 2 slabs of 104 rows,
    8 of 120, 2 of 128, 10 of 128, 49 of 128
  MASKED_BATCHES: four problems of one launch with different sample counts, masks on some
  BOUND: both sides of fdiv's bound, (M + 63) * rows_per_sample < 2^32 for an order and M * rows_per_sample < 2^32 for a mask
  TAIL_CASES: the three routes of cswin_linear_bwd_tail_skip (gemm_plan.h, batch_route)"""
import math

import numpy as np
import torch

BM = 64                       # rows of a tile, at every tile configuration
MAX_SAMPLES = 256             # MASK_MAX_SAMPLES of gemm.hip, ops.MAX_MASK_SAMPLES
NAN = float("nan")

GEOMETRIES = [(1, 7), (7, 1), (5, 52), (24, 49), (65, 3), (130, 7), (256, 1), (256, 5), (2, 3136)]

# ((samples, rows per sample, output columns, reduction), the host's tile configuration (BM, BN, BK, KW)), forward and data gradient alike
MAPPED_SHAPES = [
    # 64x32 tiles (few workgroups), one wave group: a reduction of 36 is one ragged k-step of 32 + 4, 100 three full ones + 4
    ((1, 7, 36, 36), (64, 32, 32, 1)),
    ((5, 52, 36, 36), (64, 32, 32, 1)),
    ((65, 3, 36, 100), (64, 32, 32, 1)),
    ((256, 1, 68, 36), (64, 32, 32, 1)),
    # 64x32 tiles, two wave groups from a reduction of 256 on: 260 = four k-steps of 64 + 4, 516 = eight + 4
    ((7, 1, 36, 260), (64, 32, 64, 2)),
    ((5, 52, 68, 260), (64, 32, 64, 2)),
    ((65, 3, 36, 260), (64, 32, 64, 2)),
    ((256, 1, 36, 516), (64, 32, 64, 2)),
    # 64x64 tiles (more than 256 workgroups of 64x32): a reduction of 4 is one k-step with a single 16-B chunk
    ((24, 49, 516, 4), (64, 64, 32, 1)),
    ((256, 5, 388, 36), (64, 64, 32, 1)),
    ((2, 3136, 100, 36), (64, 64, 32, 1)),
    ((130, 7, 580, 100), (64, 64, 32, 1)),
    # 64x64 tiles, two wave groups (the tail's data gradient runs this tile too)
    ((24, 49, 516, 260), (64, 64, 64, 2)),
    ((256, 5, 388, 260), (64, 64, 64, 2)),
    ((130, 7, 580, 260), (64, 64, 64, 2)),
    ((2, 3136, 68, 260), (64, 64, 64, 2)),
    # 64x64 tiles, four wave groups: fewer than 320 workgroups and a reduction of 512 or more
    ((24, 49, 516, 516), (64, 64, 64, 4)),
    ((256, 5, 388, 516), (64, 64, 64, 4)),
    ((2, 3136, 100, 516), (64, 64, 64, 4)),
    ((130, 7, 580, 516), (64, 64, 64, 4)),
]
# the six forms of tests/test_gpu_linear_skip.py, the forward without a bias, and the residual form with a factor of its own per sample
FORMS = [("fwd", "plain"), ("fwd", "gelu"), ("fwd", "res"), ("dgrad", "plain"), ("dgrad", "scaled"), ("dgrad", "gelu"), ("fwd", "nobias"),
         ("fwd", "res_factors")]
FACTORS = (1.25, 0.5, 2.0, 0.75, 1.5, 3.0, 0.625)        # nonzero, no two of a period equal: sample s runs with FACTORS[s % 7]

# ((samples, rows per sample), N, K) of a weight gradient dw (N, K) = dy (M, N)^T x (M, K), and the slabs (count, rows) the host gives a batch of one
MASKED_PROBLEMS = [
    (((65, 3), 36, 68), (2, 104)),
    (((130, 7), 68, 100), (8, 120)),
    (((256, 1), 100, 36), (2, 128)),
    (((256, 5), 36, 36), (10, 128)),
    (((2, 3136), 68, 36), (49, 128)),
]
# batches of four: ((samples, rows per sample), N, K, pattern name or None = no mask, row scale, dbias)
MASKED_BATCHES = [
    [((65, 3), 36, 68, "every_other", True, True), ((130, 7), 68, 36, "all_but_64", False, True), ((256, 1), 100, 36, None, False, True),
     ((7, 1), 36, 36, "first", True, False)],
    [((256, 5), 36, 100, None, True, True), ((5, 52), 68, 68, "neighbours", True, True), ((256, 1), 36, 36, "only_63_64", False, False),
     ((24, 49), 100, 36, "every", True, True)],
]
# (samples, rows per sample): the accepted and the refused side of fdiv's bound
BOUND = dict(accepted=(256, 4095), refused=(256, 4096))
# cswin_linear_bwd_tail_skip: the weight-gradient problems ((samples, rows per sample), N, K, pattern or None), the data gradient's
# (samples, rows per sample, N, K) -- dx (M, K) = dy (M, N) w (N, K) under an order --, and the route gemm_plan.h gives with two riders
TAIL_CASES = dict(
    masks=dict(problems=[((130, 7), 36, 100, "every_other"), ((130, 7), 100, 36, "every_other"), ((65, 3), 68, 68, "only_63_64"),
                         ((130, 7), 36, 36, None)],
               dgrad=(130, 7, 68, 100), route="tail_order jobs_ride"),
    no_mask=dict(problems=[((130, 7), 36, 100, None), ((130, 7), 100, 36, None), ((65, 3), 68, 68, None), ((130, 7), 36, 36, None)],
                 dgrad=(130, 7, 68, 100), route="tail_order jobs_ride"),
    separate=dict(problems=[((130, 7), 30, 36, None)], dgrad=(130, 7, 68, 36), route="separate dgrad_first jobs_first"),
)
TAIL_MASKED_ROUTE = "tail_masked jobs_ride"       # what the comparison call of the first case (cswin_linear_bwd_tail_masked) takes


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------
# keep patterns and orders
# ------------------------------------------------------------------------------------------------
def order_of(keep):
    """The order row cswin_drop_path_order writes: the kept count, the kept samples ascending, the dropped ones ascending."""
    keep = np.asarray(keep, bool)
    idx = np.arange(len(keep))
    return np.concatenate([[int(keep.sum())], idx[keep], idx[~keep]]).astype(np.int32)


def keep_patterns(ns, rps):
    """name -> kept flags (ns bools), every pattern of the module docstring that the geometry allows.  Never all kept."""
    only = lambda *k: np.array([i in k for i in range(ns)])
    out = {"first": ~only(0), "last": ~only(ns - 1)}
    if ns >= 2:
        out["neighbours"] = ~only(1, 2) if ns > 3 else ~only(0, 1)
    out["all_but_one"] = only(ns // 2)
    out["every"] = np.zeros(ns, bool)
    out["every_other"] = np.arange(ns) % 2 == 0
    for name, rem, least in (("rows64", 0, 64), ("rows64p1", 1, 65), ("rows64m1", 63, 63)):
        nk = next((k for k in range(1, ns) if k * rps % BM == rem and k * rps >= least), None)
        if nk is not None:
            out[name] = np.arange(ns) >= ns - nk                # the LAST nk samples: no kept row stays where it was
    if ns > 64:
        out.update(only_63_64=only(63, 64), only_last=only(ns - 1), all_but_64=~only(64))
    return {k: v for k, v in out.items() if not v.all()}


def unique_patterns(ns, rps):
    """[(names joined by '+', kept flags)]: keep_patterns without repeats (a small geometry gives one pattern several names)."""
    seen = {}
    for name, keep in keep_patterns(ns, rps).items():
        seen.setdefault(keep.tobytes(), [[], keep])[0].append(name)
    return [("+".join(names), keep) for names, keep in seen.values()]


def sample_factors(ns):
    return np.array([FACTORS[s % len(FACTORS)] for s in range(ns)], np.float32)


def row_scale_of(form, keep):
    """The per-sample factors a form runs with (None: none): 0 for a dropped sample, as DropPath makes them."""
    entry, f = form
    keep = np.asarray(keep, bool)
    if f == "res_factors":
        return np.where(keep, sample_factors(len(keep)), 0.0).astype(np.float32)
    if f in ("res", "scaled") or form == ("dgrad", "gelu"):
        return np.where(keep, 1.25, 0.0).astype(np.float32)
    return None


# ------------------------------------------------------------------------------------------------
# fdiv (csrc/common.h) in Python integers
# ------------------------------------------------------------------------------------------------
def fdiv_magic(d):
    return 0 if d <= 1 else cdiv(2 ** 32, d)


def fdiv_exact(nmax, d):
    return d >= 1 and nmax >= 0 and (d == 1 or nmax * d < 2 ** 32)


def fdiv1(n, magic):
    """n / d as the kernels take it: one multiply-high, skipped for d = 1 (magic 0).  n: uint64 array."""
    n = np.asarray(n, np.uint64)
    return n if magic == 0 else (n * np.uint64(magic)) >> np.uint64(32)


def order_accepted(ns, rps):
    """samples_checked with the order's slack of 63 rows (the row tiles' last rows are divided before they are tested)."""
    return 1 <= ns <= MAX_SAMPLES and fdiv_exact(ns * rps + 63, rps)


def mask_accepted(ns, rps):
    return 1 <= ns <= MAX_SAMPLES and fdiv_exact(ns * rps, rps)


# ------------------------------------------------------------------------------------------------
# the sample order: logical row -> physical row, tiles, and what a launch leaves in every row
# ------------------------------------------------------------------------------------------------
def row_map(order, ns, rps, wrong=None):
    """(phys, smp, kept_rows, mapped): the physical row and the sample of every logical row m of a launch with this order, as
    gemm_body and run_epilogue compute them.  order[0] == ns: the identity, whatever the rest holds."""
    order = np.asarray(order, np.int64)
    nk = int(order[0])
    m = np.arange(ns * rps)
    if nk >= ns:
        return m, m // rps, ns * rps, False
    ord_ = np.clip(order[1:1 + ns], 0, ns - 1)
    magic = fdiv_magic(rps)
    j = fdiv1(m, magic).astype(np.int64)
    if wrong == "quotient_early":                      # the sample quotient one row early at a sample border
        j = np.minimum(fdiv1(m + 1, magic).astype(np.int64), ns - 1)
    phys = np.clip(ord_[j] * rps + (m - j * rps), 0, ns * rps - 1)
    return phys, ord_[j], max(nk, 0) * rps, True


def tile_classes(kept_rows, M):
    """(live, mixed, fill): the counts of row tiles with kept rows only, the tile (0 or 1) that holds the last kept row beside dropped
    ones, and the tiles without a kept row (no k-loop)."""
    tiles = cdiv(M, BM)
    live = cdiv(kept_rows, BM)
    mixed = int(kept_rows % BM != 0 and kept_rows < M)
    return live - mixed, mixed, tiles - live


def gelu(t):
    t = torch.from_numpy(np.ascontiguousarray(t, np.float64))
    return (0.5 * t * (1.0 + torch.erf(t / math.sqrt(2.0)))).numpy()


def gelu_grad(t):
    t = torch.from_numpy(np.ascontiguousarray(t, np.float64))
    return (0.5 * (1.0 + torch.erf(t / math.sqrt(2.0))) + t * torch.exp(-0.5 * t * t) / math.sqrt(2.0 * math.pi)).numpy()


def _row_products(form, inp):
    """The float64 product of every A row with the weight, and gelu'(gelu_pre), made once per problem: a row's figures do not depend
    on which other rows a launch computes, so every launch of the model takes the rows it computes from here."""
    if "_prod" not in inp:
        a, w = inp["a"].astype(np.float64), inp["w"].astype(np.float64)
        inp["_prod"] = a @ (w.T if form[0] == "fwd" else w)                  # fwd: w (cols, red); dgrad: w (red, cols)
        inp["_dgelu"] = gelu_grad(inp["pre"]) if inp.get("pre") is not None else None
    return inp["_prod"], inp["_dgelu"]


def model_mapped(form, inp, order, scale, wrong=None, poison=None):
    """What a launch of `form` with this order leaves in memory, in float64: {y[, y_act]} or {dx}.  inp: a (M, red), w, bias, residual,
    pre (absent ones None), ns, rps.  poison: the physical rows whose A and gelu_pre hold NaN; the model reads A and gelu_pre only
    where the kernel does, so NaN in a dropped sample's rows stays out.
    wrong: "nlive_floor" (the live tile count rounded down: the mixed tile becomes a fill tile), "scale_logical" (the row scale read
    at the logical sample), "quotient_early" (row_map), "residual_scaled" (a dropped row's residual scaled instead of copied)."""
    entry, f = form
    ns, rps = inp["ns"], inp["rps"]
    M = ns * rps
    phys, smp, kept_rows, mapped = row_map(order, ns, rps, wrong)
    m = np.arange(M)
    computed = kept_rows // BM * BM if (wrong == "nlive_floor" and mapped) else kept_rows
    prod, dgelu = _row_products(form, inp)
    bad = np.zeros(M, bool) if poison is None else np.asarray(poison, bool)
    live = m < computed
    acc = np.zeros_like(prod)
    acc[live] = np.where(bad[phys[live]][:, None], NAN, prod[phys[live]])  # fill tiles and a mixed tile's null rows: zero accumulators
    dropped = mapped & (m >= kept_rows)
    if scale is not None:
        scale = np.asarray(scale, np.float64)
        rs = (scale[m // rps] if (wrong == "scale_logical" or not mapped) else scale[smp])[:, None]
    out = {}
    if entry == "fwd":
        o = acc + (inp["bias"].astype(np.float64) if inp["bias"] is not None else 0.0)
        if f in ("res", "res_factors"):
            res = inp["residual"].astype(np.float64)[phys]
            o = o * rs
            o[dropped] = 0.0
            o = o + (res * np.where(dropped[:, None], rs, 1.0) if wrong == "residual_scaled" else res)
        key = "y"
        if f == "gelu":
            out["y_act"] = gelu(o)
    else:
        o = acc
        if f == "gelu":
            g = np.full_like(acc, 0.5)                                   # gelu_pre is not read for a dropped row: gelu'(0)
            g[~dropped] = np.where(bad[phys[~dropped]][:, None], NAN, dgelu[phys[~dropped]])
            o = o * g
        if scale is not None:
            o = o * rs
        key = "dx"
    out[key] = o
    full = {}
    for k, v in out.items():
        full[k] = np.full_like(v, NAN)
        full[k][phys] = v
    return full


def check_mapped(what, form, got, plain, zero, ref, inp, keep, metric, rtol):
    """The assertions of a mapped launch with dropped samples, on host arrays (float32 from the device, float64 from the model).
    got: the launch's outputs; plain: the unmapped launch's (every sample computed); zero: the zero-A launch's; ref: float64
    linear_ref; metric(got, ref, tag) -> max|got - ref| / rms(ref).  Kept rows: bit for bit plain's and within rtol of ref; dropped
    rows: the bias (+0 without one), GELU(bias) as the zero-A launch gives it, the residual row, +0 with a clear sign bit."""
    entry, f = form
    rows = np.repeat(np.asarray(keep, bool), inp["rps"])
    for k in got:
        assert np.isfinite(got[k]).all(), f"{what}: {k} is not finite (a dropped sample's rows were read, or a row was not written)"
        assert np.array_equal(got[k][rows], plain[k][rows]), f"{what}: the kept rows of {k} are not the unmapped launch's"
        if rows.any():
            err = metric(got[k][rows], ref[k][rows], f"{what}.{k}")
            assert np.isfinite(err) and err <= rtol, f"{what}: {k} max|diff|/rms = {err:.3e} > {rtol}"
    d = got["dx" if entry == "dgrad" else "y"][~rows]
    if entry == "dgrad":
        assert not d.any() and not np.signbit(d).any(), f"{what}: a dropped row of dx is not +0"
    elif f in ("res", "res_factors"):
        assert np.array_equal(d, inp["residual"][~rows].astype(d.dtype)), f"{what}: a dropped row is not its residual row"
    elif inp["bias"] is None:
        assert not d.any() and not np.signbit(d).any(), f"{what}: a dropped row is not +0"
    else:
        assert np.array_equal(d, np.broadcast_to(inp["bias"].astype(d.dtype), d.shape)), f"{what}: a dropped row is not the bias"
        if f == "gelu":
            assert np.array_equal(got["y_act"][~rows], zero["y_act"][~rows]), f"{what}: a dropped row of y_act is not GELU(bias)"


# ------------------------------------------------------------------------------------------------
# the sample mask: the kept list, the slab ranges, and the sums a launch makes
# ------------------------------------------------------------------------------------------------
def kept_list(mask, wrong=None):
    """build_kept_list: the kept samples ascending, listed in trips of 64 lanes (ballot + popcount).  Entries never written are 0.
    wrong = "second_trip_from_0": a trip writes from index 0 instead of behind the trips before it."""
    mask = np.asarray(mask)
    idx, n = np.zeros(MAX_SAMPLES, np.int64), 0
    for s0 in range(0, len(mask), 64):
        lanes = np.arange(s0, min(s0 + 64, len(mask)))
        k = mask[lanes] != 0
        at = (0 if wrong == "second_trip_from_0" else n) + np.cumsum(k) - k
        idx[at[k]] = lanes[k]
        n += int(k.sum())
    return idx[:n]


def slab_ranges(R, splits, wrong=None):
    """The device's ranges of the compacted reduction index: r_per_split = ceil8(ceil(R / splits)), slab s = [s r, min(R, (s + 1) r)).
    wrong = "drop_last_granule": a slab's last partial 8-row granule is left out."""
    r = cdiv(cdiv(R, splits), 8) * 8
    out = []
    for s in range(splits):
        lo, hi = s * r, min(R, (s + 1) * r)
        if wrong == "drop_last_granule" and hi > lo:
            hi = lo + (hi - lo) // 8 * 8
        out.append((lo, max(lo, hi)))
    return r, out


def model_masked(dy, x, mask, scale, rps, splits, wrong=None):
    """(dw, dbias) of a masked weight gradient in float64: the kept list, the slab ranges, the rows each slab reads, the slabs summed."""
    kept = kept_list(mask, "second_trip_from_0" if wrong == "second_trip_from_0" else None)
    R = len(kept) * rps
    _, ranges = slab_ranges(R, splits, "drop_last_granule" if wrong == "drop_last_granule" else None)
    dw, db = np.zeros((dy.shape[1], x.shape[1])), np.zeros(dy.shape[1])
    magic = fdiv_magic(rps)
    for lo, hi in ranges:
        c = np.arange(lo, hi)
        j = fdiv1(c, magic).astype(np.int64)
        row = kept[j] * rps + (c - j * rps)
        f = np.asarray(scale, np.float64)[kept[j]][:, None] if scale is not None else 1.0
        sdy = dy[row].astype(np.float64) * f
        dw += sdy.T @ x[row].astype(np.float64)
        db += sdy.sum(0)
    return dw, db


def check_masked(what, dw, db, dw_ref, db_ref, metric, rtol):
    """The assertions of a masked weight gradient against the float64 product over the kept rows (db None: no dbias)."""
    errs = {}
    for k, got, ref in (("dw", dw, dw_ref), ("dbias", db, db_ref)):
        if got is None:
            continue
        assert np.isfinite(got).all(), f"{what}: {k} is not finite (a dropped sample's rows were read)"
        if not ref.any():
            assert not got.any(), f"{what}: {k} of a reduction over no rows is not exact zeros"
        else:
            errs[k] = metric(got, ref, f"{what}.{k}")
    assert all(np.isfinite(e) and e <= rtol for e in errs.values()), (what, errs)


# ------------------------------------------------------------------------------------------------
# inputs and float64 references (CPU)
# ------------------------------------------------------------------------------------------------
def mapped_inputs(form, shape):
    """The operands of one Linear, forward or data gradient, as float32 arrays.  The weight is (cols, red) for the forward, which
    reads a = x (M, red) and writes (M, cols), and (red, cols) for the data gradient, which reads a = dy (M, red)."""
    from oracle.determ import det_normal
    entry, f = form
    ns, rps, cols, red = shape
    M = ns * rps
    tag = f"droppath.{entry}.{f}." + ".".join(map(str, shape))
    return dict(ns=ns, rps=rps, cols=cols, red=red, a=det_normal(tag + ".a", (M, red)),
                w=det_normal(tag + ".w", (cols, red) if entry == "fwd" else (red, cols), 1 / np.sqrt(red)),
                bias=det_normal(tag + ".b", (cols,)) if entry == "fwd" and f != "nobias" else None,
                residual=det_normal(tag + ".res", (M, cols)) if f in ("res", "res_factors") else None,
                pre=det_normal(tag + ".pre", (M, cols)) if form == ("dgrad", "gelu") else None)


def mapped_reference(form, inp):
    """float64 linear_ref (tests/test_gpu_gemm_shapes.py) of the form with EVERY sample kept, under the outputs' names of model_mapped:
    a kept sample's rows do not depend on which other samples are kept."""
    from test_gpu_gemm_shapes import linear_ref
    entry, f = form
    scale = row_scale_of(form, np.ones(inp["ns"], bool))
    if entry == "fwd":
        r = linear_ref(inp["a"], inp["w"], inp["bias"], residual=inp["residual"], row_scale=scale, rows_per_sample=inp["rps"])
        return {k: r[k].numpy() for k in (("y", "y_act") if f == "gelu" else ("y",))}
    M = inp["ns"] * inp["rps"]
    r = linear_ref(np.zeros((M, inp["cols"]), np.float32), inp["w"], None, inp["a"], row_scale=scale, rows_per_sample=inp["rps"],
                   gelu_pre=inp["pre"])
    return dict(dx=r["dpre" if f == "gelu" else "dx"].numpy())


def masked_inputs(tag, ns, rps, N, K):
    from oracle.determ import det_normal
    return det_normal(f"droppath.w.{tag}.dy", (ns * rps, N)), det_normal(f"droppath.w.{tag}.x", (ns * rps, K))


def masked_reference(dy, x, keep, scale, rps):
    """(dw, dbias): the float64 product over the kept samples' rows, scale = per-sample factors or None."""
    rows = np.repeat(np.asarray(keep, bool), rps)
    f = np.repeat(np.asarray(scale, np.float64), rps)[:, None] if scale is not None else 1.0
    sdy = (dy.astype(np.float64) * f)[rows]
    return sdy.T @ x.astype(np.float64)[rows], sdy.sum(0)


def rms_metric(got, ref, tag=None):
    """max|got - ref| / rms(ref) in float64: test_gpu_shapes.measure without its log."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(got - ref).max()) / (float(np.sqrt((ref ** 2).mean())) + 1e-30)
