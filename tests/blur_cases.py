"""Shared inputs, scipy references and the numpy emulation of the device blur (csrc/blur.hip behind ops.gaussian_blur) for
tests/test_blur_host.py (CPU) and tests/test_gpu_blur.py (GPU): the same seeded slices in both files, so what the emulation
shows on the CPU (0 elements unequal to scipy) is shown for the very inputs the device is measured on.  Inputs and references
are computed once per process and are read-only.

The emulation is the device's arithmetic stated in numpy: per axis, float64 products and sums in correlate1d's folded order
(acc = x[i] w[0], then acc += (x[i - k] + x[i + k]) w[-k] for k = r .. 1, multiply and add rounded separately), indices reflected
with period 2n, one rounding to float32 after each axis, axis 0 first.

For tests/test_gpu_blur_shapes.py, which calls the entry point itself: the kernel's tile plan transcribed (blur_plan, held to
csrc/blur_plan.h by tests/test_blur_host.py), what a launch meets (launch_facts), the case table PLAN_CASES, the special-value and
single-NaN inputs, and four wrong emulations (MUTATIONS) that the table's inputs must tell from scipy."""
import collections
import contextlib
import functools
import random

import numpy as np
from scipy.ndimage import gaussian_filter

# ((D, H, W), sigma) of the device tests
GPU_CASES = [
    ((1, 1, 1), 1),              # r = 4 on one sample: period 2
    ((2, 3, 5), 1),              # radius larger than both axes
    ((3, 2, 9), 1.7),            # r = 7 > H
    ((2, 9, 33), 0.5),           # r = 2, odd width
    ((6, 64, 48), 1),
    ((1, 65, 130), 3),           # r = 12, row-tile remainder
    ((1, 37, 600), 1),           # ten column chunks of 64 (the plan halves the chunk to 64 at r = 4 unless the slice is short), W % CW != 0
    ((1, 20, 1100), 1),
    ((2, 512, 512), 1),          # the real pair
    ((2, 17, 23), 0.1),          # r = 0
    ((1, 40, 40), 8),            # r = 32, the limit
    ((1, 5, 70), 8),
    ((3, 224, 300), 2),
    # beyond the issue's list: the widths and radii at which the kernel's tile plan moves to its larger LDS budgets
    ((1, 6, 1500), 1),           # no four-row tile in 24 KiB: 40 KiB
    ((1, 5, 1600), 8),           # r = 32 at this width: 64 KiB
    ((1, 3, 2048), 8),           # the widest slice at the largest radius
]


def case_id(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else f"sigma{v:g}"


@functools.lru_cache(maxsize=None)
def slices(shape, sigma):
    """Seeded (D, H, W) float32 slices of a case, mean 100 and deviation 400 (read-only)."""
    x = (np.random.default_rng(2000 + 7 * sum(shape) + int(100 * sigma)).standard_normal(shape) * 400 + 100).astype(np.float32)
    x.setflags(write=False)
    return x


def scipy_blur(x, sigma):
    """gaussian_filter of every slice on its own, in the slices' dtype."""
    return np.stack([gaussian_filter(s, sigma) for s in x])


@functools.lru_cache(maxsize=None)
def scipy_blur_case(shape, sigma):
    out = scipy_blur(slices(shape, sigma), sigma)
    assert out.shape == tuple(shape) and out.dtype == np.float32
    out.setflags(write=False)
    return out


def reflect_index(i, n):
    """scipy's mode "reflect" (d c b a | a b c d | d c b a) for integer arrays i of any range: period 2n."""
    m = np.mod(i, 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def mirror_index(i, n):
    """Mode "mirror" (d c b | a b c d | c b a), period 2n - 2: NOT scipy's default; the first of the MUTATIONS."""
    if n == 1:
        return np.zeros_like(i)
    m = np.mod(i, 2 * n - 2)
    return np.where(m < n, m, 2 * n - 2 - m)


def _fma(a, b, c):
    """a b + c with the product unrounded (Dekker's two-product, then the two roundoffs folded into the sum): what a contracted
    multiply-add gives, up to a double rounding that no test here depends on.  Finite operands only."""
    p = a * b
    split = lambda v: ((v * 134217729.0) - ((v * 134217729.0) - v), v - ((v * 134217729.0) - ((v * 134217729.0) - v)))
    (ah, al), (bh, bl) = split(a), split(b)
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl             # a b = p + e exactly
    s = p + c
    t = (p - (s - (s - p))) + (c - (s - p))                       # p + c = s + t exactly
    return s + (t + e)


def _pass(x, w, r, axis, reflect=reflect_index, fma=False, round32=True):
    """One correlate1d pass over `axis` of the array x (D, H, W): float64 in the folded order, rounded to float32.  The keywords
    are the MUTATIONS below; the defaults are the device's arithmetic."""
    n = x.shape[axis]
    x64 = x.astype(np.float64)
    i = np.arange(n)
    with np.errstate(all="ignore"):                                # the special values overflow and form inf - inf on purpose
        acc = x64 * w[r]
        for k in range(r, 0, -1):
            lo, hi = np.take(x64, reflect(i - k, n), axis=axis), np.take(x64, reflect(i + k, n), axis=axis)
            acc = _fma(lo + hi, w[r - k], acc) if fma else acc + (lo + hi) * w[r - k]
        return acc.astype(np.float32) if round32 else acc


# name -> an emulation that is wrong in one way a kernel can be wrong; tests/test_blur_host.py shows that the PLAN_CASES inputs
# tell each of them from scipy.  Nothing here touches device code.
MUTATIONS = {
    "mirror": lambda x, w, r: _pass(_pass(x, w, r, 1, reflect=mirror_index), w, r, 2, reflect=mirror_index),
    "fma": lambda x, w, r: _pass(_pass(x, w, r, 1, fma=True), w, r, 2, fma=True),
    "no_rounding_between_axes": lambda x, w, r: _pass(_pass(x, w, r, 1, round32=False), w, r, 2),
    "axes_swapped": lambda x, w, r: _pass(_pass(x, w, r, 2), w, r, 1),
}


def emulate(x, sigma, truncate=4.0, mutation=None):
    """numpy emulation of csrc/blur.hip on float32 slices (D, H, W), taps from utils.gaussian_taps; `mutation` names one of
    MUTATIONS instead."""
    from cswin_unet_amd.utils import gaussian_taps
    w, r = gaussian_taps(sigma, truncate)
    if mutation is not None:
        return MUTATIONS[mutation](x, w, r)
    return _pass(_pass(x, w, r, 1), w, r, 2)


def unequal_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape
    return int((a.view(np.uint32) != b.view(np.uint32)).sum())


def unequal_bits_or_nan(a, b):
    """unequal_bits where a NaN equals a NaN whatever its payload: the position of a NaN is compared, not its bits."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape
    na, nb = np.isnan(a), np.isnan(b)
    return int(((na != nb) | (~na & ~nb & (a.view(np.uint32) != b.view(np.uint32)))).sum())


# ---- the launch plan (a transcription of the host code: it MUST FOLLOW csrc/blur_plan.h and cswin_gaussian_blur) -----------------
BL_BUDGETS = (6144, 10240, 16384)          # floats: 24, 40, 64 KiB
BL_MAX_TR, BL_RB, BL_THREADS = 32, 4, 256
TR_SOURCES = ("rows", "cap", "slice")      # TR is rows() rounded down to row groups, the 32-row cap, or the slice's height

BlurPlan = collections.namedtuple("BlurPlan", "TR cw_log2 budget w_halvings row_halvings source")


def blur_plan(H, W, r, vec):
    """bl_plan(H, W, r, vec) for integers or integer arrays (broadcast): TR, cw_log2, the index of the LDS budget (-1 and TR 0
    where no budget holds a tile), how often the chunk was halved because W needs no wider one and how often because the tile was
    shorter than 4r rows, and the index into TR_SOURCES of where TR came from."""
    scalar = all(np.ndim(v) == 0 for v in (H, W, r, vec))
    H, W, r, vec = np.broadcast_arrays(*(np.asarray(v, np.int64) for v in (H, W, r, vec)))
    Hr = (H + BL_RB - 1) // BL_RB * BL_RB
    out = [np.zeros(H.shape, np.int64) for _ in range(6)]
    out[2] -= 1
    todo = np.ones(H.shape, bool)
    for b, budget in enumerate(BL_BUDGETS):
        def rows(cwl):
            num, den = budget - 2 * r * (1 << cwl), (1 << cwl) + W
            return np.sign(num) * (np.abs(num) // den)             # C's division truncates; the numerator can be negative
        cwl = np.where(vec == 2, 9, 8)
        wh, rh = np.zeros_like(cwl), np.zeros_like(cwl)
        live = np.ones(H.shape, bool)
        for _ in range(3):
            live &= (cwl > 6) & ((1 << (cwl - 1)) >= W)
            cwl, wh = cwl - live, wh + live
        live = np.ones(H.shape, bool)
        for _ in range(3):
            live &= (cwl > 6) & (rows(cwl) < 4 * r) & (rows(cwl) < Hr)
            cwl, rh = cwl - live, rh + live
        full = rows(cwl)
        TR = np.sign(full) * (np.abs(full) // BL_RB) * BL_RB
        ok = todo & (TR >= BL_RB)
        src = np.where(TR > BL_MAX_TR, 1, 0)
        TR = np.minimum(TR, BL_MAX_TR)
        src = np.where(TR > Hr, 2, src)
        TR = np.minimum(TR, Hr)
        for o, v in zip(out, (TR, cwl, b, wh, rh, src)):
            o[ok] = np.broadcast_to(v, H.shape)[ok]
        todo &= ~ok
    return BlurPlan(*(int(o) for o in out)) if scalar else BlurPlan(*out)


def plan_signature(p, vec):
    """What tells two plans apart as far as the kernel's code paths go (works on blur_plan's arrays as well)."""
    return (vec, p.budget, p.cw_log2, p.row_halvings > 0, p.source)


def launch_facts(shape, r, vec):
    """What the workgroups of cswin_gaussian_blur(x (D, H, W), radius r) meet, given the load width `vec` the entry point picks
    (2 for even W and an 8-byte aligned base, else 1).  Item counts are per pass of the kernel's strided loops over 256 threads,
    for the first and for the last tile of a slice."""
    D, H, W = shape
    assert vec == 1 or W % 2 == 0
    p = blur_plan(H, W, r, vec)
    TR, CW = p.TR, 1 << p.cw_log2
    tiles = -(-H // TR)
    last = H - (tiles - 1) * TR
    per_tile = lambda nrow: dict(stage=(nrow + 2 * r) * (CW // vec), column=-(-nrow // BL_RB) * CW, row=-(-nrow // BL_RB) * W)
    first_items, last_items = per_tile(min(TR, H)), per_tile(last)
    return dict(plan=p, signature=plan_signature(p, vec), vec=vec, grid=(tiles, D), tiles=tiles, last_rows=last, last_mod4=last % BL_RB,
                chunks=-(-W // CW), w_rem=W % CW, first_items=first_items, last_items=last_items,
                stage_under_256=last_items["stage"] < BL_THREADS, row_under_256=last_items["row"] < BL_THREADS,
                template=r == 4, lds_bytes=4 * (TR * W + (TR + 2 * r) * CW))


def sigma_of(r):
    """A sigma whose radius int(4 sigma + 0.5) at truncate = 4 is r."""
    return r / 4 if r else 0.1


def sigma_radius(sigma, truncate=4.0):
    """The radius of utils.gaussian_taps(sigma, truncate)."""
    return int(truncate * sigma + 0.5)


def plan_vec(case):
    shape, r, off = case
    return 2 if shape[2] % 2 == 0 and off % 2 == 0 else 1


# ((D, H, W), r, off) of tests/test_gpu_blur_shapes.py: x starts `off` float32 past a 16-byte boundary, so off = 1 takes the 4-byte
# loads at an even W.  One case per plan signature that the sweep of tests/test_blur_host.py reaches, behind at least one full tile
# wherever TR is not the slice's height, at the narrowest W and the fewest rows that have the signature; then the kernel branches
# that no signature asks for.  D = 2 throughout: the second slice has other data, so a wrong slice stride shows.
PLAN_CASES = [
    # 4-byte loads (odd W), 24 KiB: chunk 64 / 128 / 256, halved by the row rule or not, TR from rows(), the cap, the slice
    ((2, 29, 1), 32, 0), ((2, 34, 1), 0, 0), ((2, 1, 1), 0, 0),
    ((2, 15, 65), 32, 0), ((2, 36, 65), 6, 0), ((2, 2, 65), 21, 0),
    ((2, 25, 65), 3, 0), ((2, 3, 65), 0, 0),
    ((2, 18, 129), 4, 0), ((2, 4, 129), 9, 0),
    ((2, 15, 129), 0, 0), ((2, 1, 129), 0, 0),
    # 4-byte loads, 40 and 64 KiB
    ((2, 12, 449), 32, 0), ((2, 2, 449), 32, 0), ((2, 1, 545), 29, 0), ((2, 6, 1281), 0, 0),
    ((2, 7, 1473), 32, 0), ((2, 4, 1473), 32, 0),
    # 8-byte loads, 24 KiB: chunk 64 / 128 / 256 / 512
    ((2, 29, 2), 32, 0), ((2, 34, 2), 0, 0), ((2, 1, 2), 0, 0),
    ((2, 15, 66), 32, 0), ((2, 36, 66), 6, 0), ((2, 3, 66), 21, 0),
    ((2, 25, 66), 3, 0), ((2, 4, 66), 0, 0),
    ((2, 18, 130), 4, 0), ((2, 2, 130), 9, 0),
    ((2, 15, 130), 0, 0), ((2, 3, 130), 0, 0),
    ((2, 12, 258), 2, 0), ((2, 1, 258), 3, 0),
    ((2, 5, 258), 0, 0),
    # 8-byte loads, 40 and 64 KiB
    ((2, 10, 450), 32, 0), ((2, 4, 450), 32, 0), ((2, 3, 546), 29, 0), ((2, 8, 1794), 1, 0), ((2, 5, 1026), 0, 0),
    ((2, 6, 1474), 32, 0), ((2, 3, 1474), 32, 0),
    # the widest slice: 5 rows are two tiles of 4 at r = 32, 32 chunks of 64; and its 4-byte form one column narrower
    ((2, 5, 2048), 32, 0), ((2, 5, 2047), 32, 0),
    # 4-byte loads at an even W (the base 4 bytes off an 8-byte boundary): several chunks and tiles, the template and r = 32 at 64 KiB
    ((2, 18, 130), 4, 1), ((2, 6, 1474), 32, 1), ((2, 21, 300), 0, 1),
    # more than two tiles, W a multiple of the chunk, three full tiles and a remainder of 4k + 2 under the cap
    ((2, 13, 258), 0, 0), ((2, 21, 256), 2, 0), ((2, 70, 64), 4, 0), ((2, 37, 192), 4, 0),
    # one row (cancelling_row below, like 1 x 545 and 1 x 258 above): the template with both load widths
    ((2, 1, 600), 4, 0), ((2, 1, 601), 4, 0),
    # more than one reflection period on both axes (r >= 2H, r >= 2W), template and generic, both load widths
    ((2, 2, 2), 4, 0), ((2, 2, 1), 4, 0), ((2, 3, 2), 12, 0), ((2, 2, 3), 7, 0), ((2, 1, 2), 4, 0), ((2, 3, 3), 32, 0),
]


def plan_case_id(case):
    shape, r, off = case
    return "x".join(map(str, shape)) + f"-r{r}" + ("-off" if off else "")


def cancelling_row(W, r, seed):
    """A row of N(100, 400^2) in which every (r + 1)-th sample is the float32 nearest to minus its window's weighted sum over
    w[0]: the blur there is what the rounding of that one sample leaves, some 1e-7 of its terms, so the last bit of a float64
    product decides bits of the float32 result.  This is the input that tells a contracted multiply-add from scipy's two
    roundings (about one such sample in ten differs); on plain noise the two agree in all but one element in 2^28."""
    from cswin_unet_amd.utils import gaussian_taps
    w, _ = gaussian_taps(sigma_of(r))
    x = (np.random.default_rng(seed).standard_normal(W) * 400 + 100).astype(np.float32)
    k = np.arange(1, r + 1)
    for p in range(r, W - r, r + 1):
        x[p] = np.float32(-float(((x[p - k].astype(np.float64) + x[p + k]) * w[r - k]).sum()) / w[r])
    return x


def has_cancelling_rows(case):
    """The one-row cases wide enough for it: with H = 1 the column pass returns the row as it is."""
    (_, H, W), r, _ = case
    return H == 1 and r >= 1 and W > 2 * r + 1


@functools.lru_cache(maxsize=None)
def plan_inputs(case):
    """(x, scipy's blur of it) of a PLAN_CASES entry, read-only: the seeded slices of GPU_CASES at this shape, or cancelling_row
    for the one-row cases."""
    shape, r, _ = case
    if not has_cancelling_rows(case):
        return slices(shape, sigma_of(r)), scipy_blur_case(shape, sigma_of(r))
    x = np.stack([cancelling_row(shape[2], r, 3000 + 10 * r + d)[None] for d in range(shape[0])])
    want = scipy_blur(x, sigma_of(r))
    x.setflags(write=False)
    want.setflags(write=False)
    return x, want


# ---- special values --------------------------------------------------------------------------------------------------------------
SPECIAL_SHAPE = (2, 11, 600)               # at r = 4 and r = 2: a tile of 8 rows and one of 3, ten chunks of 64 columns
SPECIAL_RADII = (4, 2)                     # the template and the generic kernel
SPECIAL_NAMES = ("subnormal_inputs", "subnormal_results", "near_overflow", "signed_zeros", "inf_minus_inf")


@functools.lru_cache(maxsize=None)
def special_input(name):
    """Seeded SPECIAL_SHAPE float32 slices of one value class (read-only):
    subnormal_inputs   N(0, 1) x 1e-41: every element a float32 subnormal (or zero), and so is every result;
    subnormal_results  N(0, 1) x 3e-38: inputs either side of the smallest normal 1.18e-38, averages of them below it;
    near_overflow      N(0, 1) x 1e38: finite values up to the float32 maximum 3.4e38, +-inf where a draw passes it and at two set
                       places; every result within r of an infinity is infinite (the weights are positive and sum to one, so
                       windows of finite values stay finite);
    signed_zeros       +0.0 and -0.0 by a coin: a sum is -0.0 only where every term is;
    inf_minus_inf      N(100, 400^2) with +inf, -inf and NaN placed so that windows hold both infinities (NaN) and one (+-inf)."""
    rng = np.random.default_rng(4100 + SPECIAL_NAMES.index(name))
    z = rng.standard_normal(SPECIAL_SHAPE)
    with np.errstate(over="ignore"):
        if name == "subnormal_inputs":
            x = (z * 1e-41).astype(np.float32)
        elif name == "subnormal_results":
            x = (z * 3e-38).astype(np.float32)
        elif name == "near_overflow":
            x = (z * 1e38).astype(np.float32)
            x[0, 5, 30], x[1, 2, 61] = np.inf, -np.inf             # the draws alone hold an infinity only by chance
        elif name == "signed_zeros":
            x = np.where(z < 0, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
            x[1, :, 20:40] = -0.0                                  # a block larger than a window of r = 4: -0.0 results exist
        else:
            x = (z * 400 + 100).astype(np.float32)
            x[0, 2, 10], x[0, 3, 13] = np.inf, -np.inf             # within r = 2 of each other on both axes
            x[0, 9, 60], x[1, 0, 0], x[1, 10, 69] = np.nan, np.inf, -np.inf
            x[1, 5, 33] = np.nan
    x.setflags(write=False)
    return x


def scipy_blur_quiet(x, sigma):
    """scipy_blur with numpy's and scipy's warnings about the overflow and the invalid operation of the special values off."""
    import warnings
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        return scipy_blur(x, sigma)


# ---- one NaN in a finite slice ---------------------------------------------------------------------------------------------------
NAN_SHAPE = (2, 11, 600)                   # tiles of 8 + 3 rows at r = 2 and 4, of 4 + 4 + 3 at r = 12
NAN_RADII = (2, 4, 12)                     # r = 12 > H


def nan_positions(r):
    """(name, (d, i, j)) of the NaN: the corners, an edge, the interior, and the rows just outside and just inside the halo of the
    second tile of the plan of (NAN_SHAPE, r) where it has one."""
    D, H, W = NAN_SHAPE
    pos = [("corner00", (0, 0, 0)), ("corner0W", (0, 0, W - 1)), ("cornerH0", (1, H - 1, 0)), ("cornerHW", (1, H - 1, W - 1)),
           ("edge", (0, H // 2, 0)), ("interior", (1, H // 2, W // 2))]
    TR = blur_plan(H, W, r, 2).TR
    if TR < H and TR - r - 1 >= 0:
        pos += [("above_halo", (0, TR - r - 1, 33)), ("halo_top", (0, TR - r, 33))]
    return pos


def nan_input(r, at):
    x = slices(NAN_SHAPE, sigma_of(r)).copy()
    x[at] = np.nan
    return x


@contextlib.contextmanager
def scripted_draws(params):
    """random.random and np.random.randint answer so that RandomGenerator / RawSliceParams draw (kind, k, axis, angle) = params
    (kinds of datasets.AUG_*: 0 nothing, 1 rot90 + flip, 2 rotate)."""
    kind, k, axis, angle = params
    uniforms = {0: [0.25, 0.25], 1: [0.75], 2: [0.25, 0.75]}[kind]
    ints = {0: [], 1: [k, axis], 2: [angle]}[kind]
    real_random, real_randint = random.random, np.random.randint

    def fake_randint(lo, hi=None):
        v = ints.pop(0)
        assert lo <= v < hi
        return v
    random.random, np.random.randint = (lambda: uniforms.pop(0)), fake_randint
    try:
        yield
    finally:
        random.random, np.random.randint = real_random, real_randint
    assert not uniforms and not ints
