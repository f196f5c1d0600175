"""The kernels a run is judged by and trained on, away from the workload's shapes: cswin_resize_banded and cswin_argmax_zoom_back
(csrc/resize.hip), cswin_seg_metrics (csrc/metrics.hip), cswin_augment_gather and cswin_augment_labels (csrc/augment.hip) -- at
every instantiation of the resize (TR x VEC x F64), every y-pass tile of the metrics and both of its load paths, on the second
trip of every loop, past every device-side clamp and at the largest dimension the entry points accept.

The entry points are called through cswin_unet_amd._lib: only a direct call passes a pointer off its vector alignment, a
workspace of exactly the size the library asks for, a hand-made band or index table, or n != B samples.  References:
  resize    exact cases: hand-made bands of small integer weights on small integer inputs, every product and sum an integer
            below 2^24 in any order, so the device must be BIT-EQUAL to plain loops over start + t (resize_ref).  scipy cases:
            resize_cases.banded_product in float64 rounded once to float32, under the criterion of test_gpu_resize.py (at most
            1 float32 ulp, at most 1 element in 1e5 not bit-equal): the device sums the same float64 products in its own order
            and with fused multiply-adds, ~1e-15 relative before the one rounding.  On the chosen shapes the emulation itself is
            bit-equal to scipy.ndimage.zoom(order=3) (a host test).
  metrics   seg_metrics_cases.scipy_counts_hist, compared exactly; for the hand-placed inputs also a brute-force minimum over
            all seed / query pairs (brute_counts_hist), and a numpy restatement of the three bounded passes (edt_emulation) that
            exists to show what a walk stopped early or a skipped plane would do to the histogram.
  argmax    torch.argmax on the CPU gathered through the index vectors (0 where one is negative, indices past the end clamped to
            the last sample); an explicit first-wins / first-NaN-wins loop agrees on the rows of special values.
  augment   augment_cases.source_index / gather, extended to the clamps the header documents (aug_source_ref); checked against
            np.flip(np.rot90(...)) for every (k, axis).
Float outputs are views into NaN-filled buffers (Guarded), integer outputs views into buffers filled with the byte 0xA5
(GuardedInt): the bytes round a view must survive a call, every element of the view must have been written, and a refused call
writes nothing at all.  Every device call is followed by a synchronize so that a failing step ends its test before anything else
is enqueued.

The tests at the top need no GPU."""
import ctypes
import functools
import math
import zlib

import numpy as np
import pytest
import torch
from scipy.ndimage import zoom

import augment_cases as A
from resize_cases import banded_product
from seg_metrics_cases import blob_pair, nbins_of, scipy_counts_hist
from test_gpu_attn_shapes import GUARD, Guarded, settle  # NaN guard bands round a float output; their check after a launch

gpu = pytest.mark.gpu
DEV = "cuda"
ERR_SHAPE, ERR_ALIGN, ERR_WORKSPACE, ERR_UNSUPPORTED = -1, -2, -3, -5       # include/cswin_hip.h
NONE, ROT90_FLIP, ROTATE = A.NONE, A.ROT90_FLIP, A.ROTATE


def cdiv(a, b):
    return -(-a // b)


def rng_of(tag):
    return np.random.default_rng(zlib.crc32(tag.encode()))


# ------------------------------------------------------------------------------------------------
# launch rules (a transcription of the host code: it MUST FOLLOW csrc/resize.hip, csrc/metrics.hip and csrc/augment.hip)
# ------------------------------------------------------------------------------------------------
MAX_DIM = 2048                                           # per dimension, all five entry points
RZ_LDS_ELEMS = 8192                                      # TR * W doubles = 64 KiB
MAX_CLS = 255
G1_NONE = 0x7FFF
BC_VOX = 16                                              # voxels per thread of the border pass
AUG_TILE = 16


def resize_plan(W, x_byte_offset, f64):
    """(TR, VEC) of cswin_resize_banded; x_byte_offset: the input pointer's offset from a 16-byte boundary."""
    TR = 16 if W * 16 <= RZ_LDS_ELEMS else 8 if W * 8 <= RZ_LDS_ELEMS else 4
    VEC = 2 if W % 2 == 0 and x_byte_offset % (16 if f64 else 8) == 0 else 1
    return TR, VEC


def resize_grid(D, h, TR):
    return cdiv(h, TR), D


def resize_lds_bytes(W, TR):
    return TR * W * 8


def resize_trips(W, w, VEC):
    """Trips of the busiest thread through the H pass's column loop and the W pass's loop (256 threads)."""
    return cdiv(W, 256 * VEC), cdiv(w, 256)


def seg_plan(H, pred_off, label_off):
    """(TX, G, vec_ok) of cswin_seg_metrics; the offsets are the pointers' from a 16-byte boundary, in bytes."""
    TX = 64 if H <= 512 else 32 if H <= 1024 else 16
    return TX, 256 // TX, int(pred_off % 16 == 0 and label_off % 16 == 0)


def seg_grids(D, H, W, TX):
    """Grids of the border pass and of a class's x, y and z passes."""
    return dict(border=(cdiv(D * H * W, 256 * BC_VOX),), x=(cdiv(D * H, 4), 2), y=(cdiv(W, TX), D, 2), z=(cdiv(W, 64), cdiv(H, 4), 2 * D))


def up16(n):
    return (n + 15) & ~15


def seg_workspace(D, H, W, ncls):
    """cswin_seg_metrics_workspace: two border byte maps, g1 (uint16) and g2 (int32) for both directions, the boxes."""
    N = D * H * W
    return 2 * up16(N) + up16(2 * N * 2) + up16(2 * N * 4) + up16(ncls * 6 * 4)


def argmax_grid(B, H):
    return H, B


def augment_grid(n, Ho, Wo):
    return cdiv(Wo, AUG_TILE), cdiv(Ho, AUG_TILE), n


# ------------------------------------------------------------------------------------------------
# case tables
# ------------------------------------------------------------------------------------------------
# cswin_resize_banded with scipy's bands: (D, H, W) -> (h, w) and what the row is there for
RESIZE_SHAPES = [
    ((2, 9, 513), (5, 300)),          # TR = 8, odd W: VEC = 1; second trip of both loops
    ((2, 9, 514), (17, 257)),         # TR = 8, VEC = 2; h = 2 TR + 1
    ((1, 7, 1024), (9, 256)),         # TR = 8 at exactly 64 KiB of LDS
    ((2, 6, 1025), (4, 40)),          # TR = 4, VEC = 1; h = TR
    ((1, 5, 1026), (5, 33)),          # TR = 4, VEC = 2; h = TR + 1
    ((1, 5, 2048), (3, 2048)),        # TR = 4 at 64 KiB; h = TR - 1; w = 2048
    ((3, 520, 12), (300, 7)),         # tall and narrow: Th = 68 windows shared across a TR = 16 tile
]
# every shape in both dtypes on an aligned base; the even-W ones again one ELEMENT off (8 B of float64, 4 B of float32: VEC = 1)
RESIZE_CASES = [(s, o, dt, off) for s, o in RESIZE_SHAPES for dt in ("float32", "float64") for off in ((0, 1) if s[2] % 2 == 0 else (0,))]

# exact-integer cases: (tag, D, H, W, h, w, Th, Tw, element offset of the base).  One W per TR class at least; every case has
# starts below 0 and above n_in - T (the device clamps them) and, where there are three rows, an all-zero weight row.
EXACT_CASES = [
    ("tr16.t1", 2, 5, 12, 3, 7, 1, 1, 0),                # Th = Tw = 1
    ("tr16.full", 2, 6, 7, 5, 4, 6, 7, 0),               # Th = H, Tw = W: every start clamps to 0
    ("tr16.tiles", 2, 20, 30, 35, 9, 5, 7, 1),           # h = 2 TR + 3, base one element off
    ("tr8.t1", 1, 3, 600, 2, 5, 1, 1, 0),
    ("tr8.wide", 2, 9, 600, 9, 270, 3, 7, 0),            # h = TR + 1; second trip of both loops
    ("tr4.t1", 1, 2, 1100, 1, 1, 1, 1, 1),
    ("tr4.wide", 1, 7, 1100, 9, 300, 7, 5, 0),           # Th = H; h = 2 TR + 1
    ("ones", 1, 3, 5, 1, 1, 2, 3, 0),                    # D = h = w = 1
]

# cswin_seg_metrics: tag -> (shape, ncls, ndim, pred byte offset, label byte offset); seg_inputs builds the volumes
SEG_CASES = {
    "blob513": ((2, 513, 40), 4, 3, 0, 0),               # TX = 32
    "blob1025": ((1, 1025, 24), 4, 2, 0, 0),             # TX = 16, the 2-D border rule
    "blob1030": ((3, 1030, 70), 4, 3, 0, 0),             # TX = 16, W past one tile of 64
    "wide2048": ((1, 8, 2048), 3, 3, 0, 0),              # W = 2048: 32 chunks of the x pass; class 2 spans the row
    "deep2048": ((2048, 3, 5), 3, 3, 0, 0),              # D = 2048: class 2 walks 2047 planes
    "ncls255": ((3, 20, 30), 255, 3, 0, 0),
    "unaligned": ((5, 33, 71), 9, 3, 1, 8),              # vec_ok = 0; N % 16 != 0
    "unaligned513": ((2, 513, 40), 4, 3, 8, 0),          # vec_ok = 0 with TX = 32
    "h1": ((5, 1, 33), 3, 3, 0, 0),
    "w1": ((5, 33, 1), 3, 3, 0, 0),
    "voxel": ((1, 1, 1), 2, 3, 0, 0),                    # the single voxel in class 1 on both sides
    "corners": ((6, 40, 70), 3, 3, 0, 0),                # class 1: one voxel at opposite corners; both land in bin nbins - 1
    "line.ndim2": ((1, 600, 9), 2, 2, 0, 0),             # the same on a plane, TX = 32
    "line.ndim3": ((1, 600, 9), 2, 3, 0, 0),
    "zgap": ((24, 30, 30), 2, 3, 0, 0),                  # seedless planes and rows inside the box
    "plates": ((2, 1030, 8), 2, 3, 0, 0),                # two thin plates 500 rows apart: long y walks at TX = 16
}
FAR_APART = ("corners", "line.ndim2", "line.ndim3", "zgap", "plates")

# cswin_argmax_zoom_back: (h, w) -> (H, W); B = 3
ARGMAX_SHAPES = [((3, 2048), (5, 2048)), ((5, 7), (2048, 3)), ((33, 300), (17, 257))]
ARGMAX_NCLS = (1, 2, 255)
ARGMAX_B = 3

AUG_SHAPES = [(37, 53), (16, 16)]
AUG_LABEL_SIZES = {(37, 53): (21, 35), (16, 16): (9, 20)}         # (h, w): no multiple of 16
AUG_B = 3


# ------------------------------------------------------------------------------------------------
# resize: references and the comparison
# ------------------------------------------------------------------------------------------------
def resize_ref(x, wh, sh, ww, sw, wrong=None, TR=None):
    """float64 (D, h, w) of cswin_resize_banded from its definition: plain loops over start + t, the H pass first, starts
    clamped into [0, n_in - T] as the header documents.

    wrong (the sensitivity tests alone): "drop_tap" (the last tap of every window), "start" (every start one further),
    "tile_row" (the last output row of every tile of TR rows left out)."""
    D, H, W = x.shape
    (h, Th), (w, Tw) = wh.shape, ww.shape
    x = x.astype(np.float64)
    taps = lambda T: T - 1 if wrong == "drop_tap" else T
    shift = 1 if wrong == "start" else 0
    img = np.zeros((D, h, W))
    for i in range(h):
        s = min(max(int(sh[i]) + shift, 0), H - Th)
        for t in range(taps(Th)):
            img[:, i, :] += wh[i, t] * x[:, s + t, :]
    out = np.zeros((D, h, w))
    for j in range(w):
        s = min(max(int(sw[j]) + shift, 0), W - Tw)
        for t in range(taps(Tw)):
            out[:, :, j] += ww[j, t] * img[:, :, s + t]
    if wrong == "tile_row":
        out[:, TR - 1::TR, :] = 0.0
    return out


@functools.lru_cache(maxsize=None)
def exact_inputs(tag):
    """(x float64 (D, H, W) of integers in [-8, 8], wh, sh, ww, sw) of a row of EXACT_CASES: integer weights in [-3, 3] with a
    non-zero last tap, starts in [-3, n_in - T + 3] with the first below 0 and the last above n_in - T.  Read-only."""
    _, D, H, W, h, w, Th, Tw, _ = next(c for c in EXACT_CASES if c[0] == tag)
    rng = rng_of("eval.exact." + tag)
    x = rng.integers(-8, 9, (D, H, W)).astype(np.float64)

    def band(n_in, n_out, T):
        wgt = rng.integers(-3, 4, (n_out, T)).astype(np.float64)
        wgt[:, -1] = rng.choice([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0], n_out)
        start = rng.integers(-3, n_in - T + 4, n_out).astype(np.int32)
        start[0] = -2
        if n_out >= 2:
            start[-1] = n_in - T + 2
        if n_out >= 3:
            wgt[n_out // 2] = 0.0
        return wgt, start
    wh, sh = band(H, h, Th)
    ww, sw = band(W, w, Tw)
    for a in (x, wh, sh, ww, sw):
        a.setflags(write=False)
    return x, wh, sh, ww, sw


@functools.lru_cache(maxsize=None)
def wide_slices(shape, size, dtype):
    """Seeded standard-normal slices of a row of RESIZE_SHAPES (read-only)."""
    x = rng_of(f"eval.resize.{shape}.{size}").standard_normal(shape).astype(dtype)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def wide_ref(shape, size, dtype):
    """banded_product of wide_slices in float64, rounded once to float32 (read-only)."""
    y = banded_product(wide_slices(shape, size, dtype), size).astype(np.float32)
    y.setflags(write=False)
    return y


def bit_equal(got, want):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    return got.shape == want.shape and bool((got.view(np.uint32) == want.view(np.uint32)).all())


def ulp_figures(got, want):
    """(elements not bit-equal, largest difference in float32 ulps of want): the figures of test_gpu_resize's criterion."""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    unequal = int((got.view(np.uint32) != want.view(np.uint32)).sum())
    ulps = np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
    return unequal, float(ulps.max())


def within_one_ulp(got, want, tag=None):
    """test_gpu_resize.py's criterion: every element within 1 float32 ulp, at most 1 in 1e5 not bit-equal."""
    unequal, ulps = ulp_figures(got, want)
    if tag is not None:
        print(f"{tag}: {unequal} of {got.size} elements not bit-equal, max difference {ulps:.3g} ulp")
    return bool(np.isfinite(got).all()) and ulps <= 1.0 and unequal * 100000 <= got.size


# ------------------------------------------------------------------------------------------------
# metrics: inputs, the brute-force reference, a restatement of the three passes
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def seg_inputs(tag):
    """(pred, label) uint8 (D, H, W) of a row of SEG_CASES (read-only)."""
    shape = SEG_CASES[tag][0]
    far = tuple(n - 1 for n in shape)
    pred, label = np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)
    if tag.startswith("blob") or tag == "unaligned513":
        pred, label = blob_pair(shape, [1, 2, 3], 50 + shape[1])
    elif tag in ("wide2048", "deep2048"):
        pred, label = blob_pair(shape, [1], 61 + shape[0])
        pred[pred == 2], label[label == 2] = 0, 0
        pred[0, 0, 0], label[far] = 2, 2
    elif tag == "ncls255":
        pred, label = blob_pair(shape, [1, 128, 254], 62, rmin=0.15, rmax=0.3)
    elif tag == "unaligned":
        pred, label = blob_pair(shape, [1, 2, 3, 4, 5, 6, 7, 8], 63)
    elif tag in ("h1", "w1"):
        pred, label = blob_pair(shape, [1, 2], 64, rmin=0.15, rmax=0.3)
    elif tag == "voxel":
        pred[0, 0, 0], label[0, 0, 0] = 1, 1
    elif tag == "corners":
        pred, label = blob_pair(shape, [2], 65)
        pred[pred == 1], label[label == 1] = 0, 0
        pred[0, 0, 0], label[far] = 1, 1
    elif tag.startswith("line"):
        pred[0, 0, 0], label[far] = 1, 1
    elif tag == "zgap":
        label[1:4, 8:14, 9:16] = 1
        pred[20:23, 15:22, 12:18] = 1
    elif tag == "plates":
        pred[:, 10:12, 1:7] = 1
        label[:, 510:512, :] = 1
    else:
        raise KeyError(tag)
    pred, label = np.ascontiguousarray(pred), np.ascontiguousarray(label)
    pred.setflags(write=False)
    label.setflags(write=False)
    return pred, label


@functools.lru_cache(maxsize=None)
def seg_ref(tag):
    """scipy_counts_hist of a row of SEG_CASES (read-only)."""
    _, ncls, ndim, _, _ = SEG_CASES[tag]
    counts, hist = scipy_counts_hist(*seg_inputs(tag), ncls, ndim)
    counts.setflags(write=False)
    hist.setflags(write=False)
    return counts, hist


def plain_border(mask, ndim):
    """Set voxels of a (D, H, W) mask with a face neighbour that is unset or outside the array; ndim = 2: in-plane neighbours."""
    p = np.pad(mask, 1, constant_values=False)
    inner = p[1:-1, 1:-1, :-2] & p[1:-1, 1:-1, 2:] & p[1:-1, :-2, 1:-1] & p[1:-1, 2:, 1:-1]
    if ndim == 3:
        inner = inner & p[:-2, 1:-1, 1:-1] & p[2:, 1:-1, 1:-1]
    return mask & ~inner


def brute_counts_hist(pred, label, ncls, ndim):
    """counts / hist as the header defines them: borders from plain_border, every distance the minimum over ALL seed / query
    pairs of the integer squared distance."""
    counts, hist = np.zeros((ncls, 4), np.int64), np.zeros((ncls, nbins_of(pred.shape)), np.int32)
    for c in range(ncls):
        P, G = pred == c, label == c
        Pb, Gb = plain_border(P, ndim), plain_border(G, ndim)
        counts[c] = [P.sum(), G.sum(), (P & G).sum(), Pb.sum() + Gb.sum()]
        if c == 0 or not P.any() or not G.any():
            continue
        for q, s in ((Pb, Gb), (Gb, Pb)):
            q, s = np.argwhere(q).astype(np.int64), np.argwhere(s).astype(np.int64)
            for k in range(0, len(q), 256):
                d2 = ((q[k:k + 256, None, :] - s[None, :, :]) ** 2).sum(-1).min(1)
                np.add.at(hist[c], d2, 1)
    return counts, hist


def edt_emulation(seeds, queries, nbins, wrong=None):
    """Histogram row of one direction as csrc/metrics.hip forms it, inside the box of seeds and queries together: g1 = distance
    to the row's nearest seed (G1_NONE: none), the y and z minima as walks over growing |d| that stop once d^2 >= best.

    wrong (the sensitivity test alone): "y_early" (the y walk stops once (d + 1)^2 >= best: one step early), "skip_last_plane"
    (the z walk never visits the last plane of the box)."""
    idx = np.argwhere(seeds | queries)
    lo, hi = idx.min(0), idx.max(0) + 1
    box = tuple(slice(a, b) for a, b in zip(lo, hi))
    s, q = seeds[box], queries[box]
    Z, Y, X = s.shape
    far = np.int64(2) ** 40
    dist = np.abs(np.arange(X)[:, None] - np.arange(X)[None, :])
    g = np.where(s[:, :, None, :], dist[None, None], G1_NONE).min(-1).astype(np.int64)
    best = g * g
    for d in range(1, Y):
        live = ((d + 1) ** 2 if wrong == "y_early" else d * d) < best
        cand = np.full_like(best, far)
        cand[:, d:, :] = g[:, :-d, :] ** 2 + d * d
        cand[:, :-d, :] = np.minimum(cand[:, :-d, :], g[:, d:, :] ** 2 + d * d)
        best = np.where(live, np.minimum(best, cand), best)
    g2, last = best, Z - 1 if wrong == "skip_last_plane" else Z
    for d in range(1, Z):
        live = d * d < best
        cand = np.full_like(best, far)
        cand[d:] = g2[:-d] + d * d
        if last - d > 0:
            cand[:last - d] = np.minimum(cand[:last - d], g2[d:last] + d * d)
        best = np.where(live, np.minimum(best, cand), best)
    found = best[q]
    return np.bincount(found[found < nbins], minlength=nbins).astype(np.int32)


def emulated_hist(pred, label, ncls, ndim, wrong=None):
    hist = np.zeros((ncls, nbins_of(pred.shape)), np.int32)
    for c in range(1, ncls):
        P, G = pred == c, label == c
        if P.any() and G.any():
            Pb, Gb = plain_border(P, ndim), plain_border(G, ndim)
            hist[c] = edt_emulation(Gb, Pb, hist.shape[1], wrong) + edt_emulation(Pb, Gb, hist.shape[1], wrong)
    return hist


# ------------------------------------------------------------------------------------------------
# argmax: inputs and references
# ------------------------------------------------------------------------------------------------
def special_columns(ncls):
    """float32 (ncls, 7): +0 / -0 ties both ways, +inf twice, -inf everywhere, a NaN in class 0, a NaN only in the last class,
    all NaN."""
    c = np.arange(ncls)
    z = np.zeros(ncls, np.float32)
    pz, nz = np.where(c % 2 == 0, 0.0, -0.0).astype(np.float32), np.where(c % 2 == 0, -0.0, 0.0).astype(np.float32)
    two_inf, minf = z.copy(), np.full(ncls, -np.inf, np.float32)
    two_inf[[min(1, ncls - 1), ncls - 1]] = np.inf
    nan0, nan_last, nans = z.copy(), z.copy(), np.full(ncls, np.nan, np.float32)
    nan0[min(1, ncls - 1)] = np.inf
    nan0[0] = np.nan
    nan_last[0] = np.inf
    nan_last[-1] = np.nan
    return np.stack([pz, nz, two_inf, minf, nan0, nan_last, nans], axis=1)


def special_winners(ncls):
    """What torch.argmax's rule gives on special_columns, worked out by hand: the first of equals, the first NaN."""
    return [0, 0, min(1, ncls - 1), 0, 0, ncls - 1, 0]


@functools.lru_cache(maxsize=None)
def argmax_logits(ncls, h, w):
    """(B, ncls, h, w) float32: multiples of 0.25 (many ties); every third column holds one of special_columns (read-only)."""
    rng = rng_of(f"eval.argmax.{ncls}.{h}.{w}")
    x = (np.round(rng.standard_normal((ARGMAX_B, ncls, h, w)) * 4) / 4).astype(np.float32)
    sp = special_columns(ncls)
    for j in range(0, w, 3):
        x[:, :, :, j] = sp[None, :, None, (j // 3) % sp.shape[1]]
    x.setflags(write=False)
    return x


def index_vector(n_in, n_out, tag):
    """int32 (n_out) source indices, hand-made: random in range, then -1 in the middle (from 5 outputs on with -5 before it),
    n_in first and n_in + 7 last, and (from 8 outputs on) a repeated and a decreasing run."""
    v = rng_of("eval.index." + tag).integers(0, n_in, n_out).astype(np.int32)
    if n_out >= 8:
        v[3:6] = [n_in - 1, n_in - 1, 0]
    v[0], v[n_out - 1], v[n_out // 2] = n_in, n_in + 7, -1
    if n_out >= 5:
        v[n_out // 2 - 1] = -5
    return v


def argmax_first(col):
    """The rule as an explicit loop over the classes: a later class wins only if it is greater, or a NaN while the best is not."""
    best, arg = col[0], 0
    for c in range(1, len(col)):
        v = col[c]
        if not np.isnan(best) and (v > best or np.isnan(v)):
            best, arg = v, c
    return arg


def argmax_ref(logits, src_row, src_col, later=False):
    """uint8 (B, H, W): torch.argmax on the CPU gathered through the index vectors; 0 where an index is negative, indices past
    the end clamped to the last sample.  later (the sensitivity test alone): ties go to the later class."""
    B, ncls, h, w = logits.shape
    t = torch.from_numpy(np.array(logits))
    am = (ncls - 1 - torch.argmax(t.flip(1), 1) if later else torch.argmax(t, 1)).numpy()
    r, c = np.clip(src_row, 0, h - 1), np.clip(src_col, 0, w - 1)
    out = am[:, r][:, :, c]
    return np.where((src_row >= 0)[None, :, None] & (src_col >= 0)[None, None, :], out, 0).astype(np.uint8)


# ------------------------------------------------------------------------------------------------
# augment: the index rule with the documented clamps
# ------------------------------------------------------------------------------------------------
def aug_source_ref(H, W, kind, k, axis, amap, i, j, other_way=False):
    """Flat source index (negative: none) of pixel (i, j) of the transformed slice as include/cswin_hip.h defines T, for ANY
    (i, j) a caller may pass: k is taken mod 4, the map's entries and every derived row and column are clamped into the slice,
    a NULL map has no source anywhere.  For a sample listed with its own shape this is augment_cases.source_index (a host test).
    other_way (the sensitivity test alone): np.rot90 turned clockwise."""
    i, j = np.asarray(i, np.int64), np.asarray(j, np.int64)
    if kind == ROTATE:
        if amap is None:
            return np.full(np.broadcast(i, j).shape, -1, np.int64)
        p = np.minimum(i * W + j, H * W - 1)
        return np.minimum(np.asarray(amap, np.int64).ravel()[p], H * W - 1)
    r, c = i, j
    if kind == ROT90_FLIP:
        k = (-k if other_way else k) & 3
        Ht, Wt = (W, H) if k & 1 else (H, W)
        if axis == 0:
            i = Ht - 1 - i
        else:
            j = Wt - 1 - j
        r = (i, j, H - 1 - i, H - 1 - j)[k]
        c = (j, W - 1 - i, W - 1 - j, i)[k]
    r, c = np.clip(r, 0, H - 1), np.clip(c, 0, W - 1)
    return r * W + c


def aug_gather_ref(x, descs, Ho, Wo, other_way=False):
    """(n, Ho, Wo) of cswin_augment_gather: descs = [(kind, k, axis, src, map or None)], src clamped into the batch."""
    B, H, W = x.shape
    i, j = np.meshgrid(np.arange(Ho), np.arange(Wo), indexing="ij")
    return np.stack([A.gather(x[min(max(src, 0), B - 1)], aug_source_ref(H, W, kind, k, axis, amap, i, j, other_way))
                     for kind, k, axis, src, amap in descs])


def aug_labels_ref(lab, descs, rows, cols, rows_t, cols_t):
    """(n, h, w) int64 of cswin_augment_labels: the transposing samples (kind 1, odd k) read (rows_t, cols_t), a negative row or
    column index gives 0, one past the end of the transformed slice is clamped to its last sample."""
    B, H, W = lab.shape
    out = []
    for kind, k, axis, src, amap in descs:
        tr = kind == ROT90_FLIP and (k & 1)
        Ht, Wt = (W, H) if tr else (H, W)
        si, sj = np.meshgrid(rows_t if tr else rows, cols_t if tr else cols, indexing="ij")
        p = aug_source_ref(H, W, kind, k, axis, amap, np.minimum(si, Ht - 1), np.minimum(sj, Wt - 1))
        p = np.where((si >= 0) & (sj >= 0), p, -1)
        out.append(A.gather(lab[min(max(src, 0), B - 1)], p).astype(np.int64))
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def aug_batch(shape):
    """(x float32 (B, H, W), lab uint8 (B, H, W) of classes 0..8 and a few 255) of the augment tests (read-only)."""
    rng = rng_of(f"eval.aug.{shape}")
    x = rng.standard_normal((AUG_B,) + shape).astype(np.float32)
    lab = rng.integers(0, 9, (AUG_B,) + shape).astype(np.uint8)
    lab[rng.random(lab.shape) < 0.1] = 255
    x.setflags(write=False)
    lab.setflags(write=False)
    return x, lab


@functools.lru_cache(maxsize=None)
def bad_map(H, W):
    """utils.rotation_index(H, W, 19) with entries replaced by values at and past H * W and below -1 (read-only)."""
    from cswin_unet_amd.utils import rotation_index
    m = rotation_index(H, W, 19).copy()
    flat = m.reshape(-1)
    flat[5::7] = H * W + np.arange(len(flat[5::7]))
    flat[3::11] = -2 - np.arange(len(flat[3::11]))
    flat[0], flat[-1] = 2 ** 31 - 1, -2 ** 31
    m.setflags(write=False)
    return m


def aug_descs(shape, group):
    """The samples of one gather call on slices of `shape`.  group "straight": output (H, W); "turned": output (W, H); on a
    non-square shape each call also lists samples of the other group (their result is what the clamps make of it)."""
    from cswin_unet_amd.utils import rotation_index
    H, W = shape
    real, bad = rotation_index(H, W, 19), bad_map(H, W)
    even = [(ROT90_FLIP, k, axis, None) for k in (0, 2) for axis in (0, 1)]
    odd = [(ROT90_FLIP, k, axis, None) for k in (1, 3) for axis in (0, 1)] + [(ROT90_FLIP, 5, 0, None), (ROT90_FLIP, -1, 1, None)]
    other = [(NONE, 0, 0, None), (ROTATE, 0, 0, real), (ROTATE, 0, 0, rotation_index(H, W, -7)), (ROTATE, 0, 0, None), (ROTATE, 0, 0, bad)]
    if H == W:
        rows = other + even + odd
    elif group == "straight":
        rows = other + even + [(ROT90_FLIP, 1, 0, None), (ROT90_FLIP, 3, 1, None)]
    else:
        rows = odd + [(NONE, 0, 0, None), (ROT90_FLIP, 0, 0, None), (ROT90_FLIP, 2, 1, None), (ROTATE, 0, 0, real), (ROTATE, 0, 0, bad)]
    return [(kind, k, axis, s % AUG_B, amap) for s, (kind, k, axis, amap) in enumerate(rows)]


def label_indices(shape, size):
    """(src_row, src_col, src_row_t, src_col_t): utils.nearest_index of both shape groups, then negatives in the middle and
    entries at and past the end."""
    from cswin_unet_amd.utils import nearest_index
    (H, W), (h, w) = shape, size
    out = []
    for n_in, n_out in ((H, h), (W, w), (W, h), (H, w)):
        v = nearest_index(n_in, n_out).copy()
        v[n_out // 2], v[2] = -1, -3
        v[0], v[n_out - 2] = n_in, n_in + 4
        out.append(v)
    return out


# ------------------------------------------------------------------------------------------------
# host-only tests: the tables against the rules, the references against second formulations, what the comparisons can see
# ------------------------------------------------------------------------------------------------
def test_resize_tables_reach_every_instantiation_trip_and_clamp():
    reached = {resize_plan(s[2], off * np.dtype(dt).itemsize, dt == "float64") + (dt == "float64",) for s, _, dt, off in RESIZE_CASES}
    assert reached == {(TR, VEC, f64) for TR in (16, 8, 4) for VEC in (1, 2) for f64 in (False, True)}
    assert resize_plan(512, 0, False) == (16, 2) and resize_plan(513, 0, False) == (8, 1) and resize_plan(1024, 0, True) == (8, 2)
    assert resize_plan(1025, 0, False) == (4, 1) and resize_plan(2048, 0, False) == (4, 2) and resize_plan(2048, 8, False) == (4, 2)
    assert resize_plan(514, 8, True) == (8, 1) and resize_plan(514, 4, False) == (8, 1) and resize_plan(514, 16, True) == (8, 2)
    assert resize_lds_bytes(1024, 8) == resize_lds_bytes(2048, 4) == 65536 and all(resize_lds_bytes(s[2], resize_plan(s[2], 0, False)[0]) <= 65536 for s, _ in RESIZE_SHAPES)
    # both loops take a second trip somewhere, at VEC = 1 and at VEC = 2; h on both sides of a tile; every shape has more than one workgroup or slice
    assert resize_trips(513, 300, 1) == (3, 2) and resize_trips(514, 257, 2) == (2, 2) and resize_trips(2048, 2048, 2) == (4, 8)
    hs = {(resize_plan(s[2], 0, False)[0], o[0]) for s, o in RESIZE_SHAPES}
    assert {(8, 17), (4, 4), (4, 5), (4, 3), (16, 300)} <= hs
    assert resize_grid(2, 17, 8) == (3, 2) and resize_grid(3, 300, 16) == (19, 3)
    from cswin_unet_amd.utils import zoom_operator
    assert zoom_operator(520, 300)[0].shape[1] == 68
    # the exact cases: every TR class, T = 1, T = n_in, out-of-range starts on both sides, a zero row, all of D, h, w = 1
    assert {resize_plan(c[3], 0, False)[0] for c in EXACT_CASES} == {16, 8, 4}
    for TR in (16, 8, 4):
        assert any(resize_plan(c[3], 0, False)[0] == TR and c[6] == c[7] == 1 for c in EXACT_CASES)
    assert any(c[6] == c[2] and c[7] == c[3] for c in EXACT_CASES) and any(c[1] == c[4] == c[5] == 1 for c in EXACT_CASES)
    assert {c[8] for c in EXACT_CASES} == {0, 1}
    assert 7 * 3 * 7 * 3 * 8 < 2 ** 24                              # the largest magnitude any partial sum can reach
    for tag, D, H, W, h, w, Th, Tw, _ in EXACT_CASES:
        x, wh, sh, ww, sw = exact_inputs(tag)
        assert Th <= 7 and Tw <= 7 and np.abs(x).max() <= 8 and np.abs(wh).max() <= 3 and np.abs(ww).max() <= 3
        assert (x == np.rint(x)).all() and (wh == np.rint(wh)).all() and (ww == np.rint(ww)).all()
        assert sh[0] < 0 and sw[0] < 0 and (h < 2 or sh[-1] > H - Th) and (w < 2 or sw[-1] > W - Tw)
        assert (wh[:, -1] != 0).sum() >= h - 1 and (h < 3 or not wh[h // 2].any()) and (w < 3 or not ww[w // 2].any())


def test_seg_tables_reach_every_tile_both_load_paths_and_the_limits():
    plans = {tag: seg_plan(shape[1], po, lo) for tag, (shape, _, _, po, lo) in SEG_CASES.items()}
    assert {p[0] for p in plans.values()} == {64, 32, 16} and {p[2] for p in plans.values()} == {0, 1}
    assert {(p[0], p[1]) for p in plans.values()} == {(64, 4), (32, 8), (16, 16)}
    assert plans["blob513"][0] == 32 and plans["blob1025"][0] == 16 and plans["blob1030"][0] == 16 and plans["plates"][0] == 16
    assert plans["unaligned"] == (64, 4, 0) and plans["unaligned513"] == (32, 8, 0)
    assert seg_plan(512, 0, 0)[0] == 64 and seg_plan(1024, 0, 0)[0] == 32 and seg_plan(2048, 16, 32) == (16, 16, 1)
    assert all(p[0] * shape[1] * 2 <= 65536 for p, (shape, *_) in zip(plans.values(), SEG_CASES.values()))
    for tag, (shape, ncls, *_) in SEG_CASES.items():
        pred, label = seg_inputs(tag)
        assert pred.shape == label.shape == shape and max(pred.max(), label.max()) < ncls and (pred != label).any() == (tag != "voxel"), tag
    shapes = [c[0] for c in SEG_CASES.values()]
    assert any(s[0] == MAX_DIM for s in shapes) and any(s[2] == MAX_DIM for s in shapes) and any(s[1] == 1 for s in shapes) and any(s[2] == 1 for s in shapes)
    assert (1, 1, 1) in shapes and any(c[1] == MAX_CLS for c in SEG_CASES.values()) and {c[2] for c in SEG_CASES.values()} == {2, 3}
    assert math.prod(SEG_CASES["unaligned"][0]) % BC_VOX != 0
    assert seg_grids(3, 1030, 70, 16) == dict(border=(53,), x=(773, 2), y=(5, 3, 2), z=(2, 258, 6))
    assert seg_grids(2048, 3, 5, 64)["z"][2] == 4096 < 65536
    for shape, ncls, ndim, _, _ in SEG_CASES.values():
        assert nbins_of(shape) == (shape[0] - 1) ** 2 + (shape[1] - 1) ** 2 + (shape[2] - 1) ** 2 + 1
    assert 3 * (MAX_DIM - 1) ** 2 + G1_NONE ** 2 < 2 ** 31
    # the far-apart inputs do what they are there for
    for tag in ("corners", "line.ndim2", "line.ndim3"):
        counts, hist = seg_ref(tag)
        assert counts[1].tolist() == [1, 1, 0, 2] and hist[1, -1] == 2 and hist[1].sum() == 2, tag
    for tag in ("wide2048", "deep2048"):
        counts, hist = seg_ref(tag)
        assert counts[2].tolist() == [1, 1, 0, 2] and hist[2, -1] == 2 and counts[1, 2] > 0, tag
    pred, label = seg_inputs("zgap")
    assert not (pred.any(axis=(1, 2)) & label.any(axis=(1, 2))).any() and not (pred | label)[5:19].any()
    assert np.flatnonzero(seg_ref("plates")[1][1]).min() >= 498 ** 2
    assert seg_ref("voxel")[0][1].tolist() == [1, 1, 1, 2] and seg_ref("voxel")[1].tolist() == [[0], [2]]


def test_seg_workspace_formula_and_nbins_equal_the_library():
    """The size queries are host code: they answer without a device."""
    from cswin_unet_amd._lib import lib
    for tag, (shape, ncls, ndim, _, _) in SEG_CASES.items():
        assert lib().cswin_seg_metrics_workspace(*shape, ndim, ncls) == seg_workspace(*shape, ncls), tag
        assert lib().cswin_seg_metrics_nbins(*shape) == nbins_of(shape), tag
    assert lib().cswin_seg_metrics_workspace(MAX_DIM, 2, 2, 3, 2) == seg_workspace(MAX_DIM, 2, 2, 2)
    for bad in ((2, 8, 8, 2, 9), (1, 8, 8, 4, 9), (1, 8, 8, 3, 1), (1, 8, 8, 3, 256), (0, 8, 8, 3, 9), (1, 2049, 8, 3, 9)):
        assert lib().cswin_seg_metrics_workspace(*bad) == 0 and lib().cswin_last_error().decode().startswith("seg_metrics"), bad
    assert lib().cswin_seg_metrics_nbins(1, 8, 2049) == 0 and lib().cswin_seg_metrics_nbins(0, 8, 8) == 0


@pytest.mark.parametrize("tag", [c[0] for c in EXACT_CASES])
def test_resize_exact_reference_is_exact_and_order_free(tag):
    """The loops give integers that float32 holds, and a second formulation -- dense operators built from the clamped bands,
    multiplied with einsum in another order -- gives the same bits."""
    x, wh, sh, ww, sw = exact_inputs(tag)
    ref = resize_ref(x, wh, sh, ww, sw)
    assert (ref == np.rint(ref)).all() and np.abs(ref).max() < 2 ** 24 and (ref.astype(np.float32).astype(np.float64) == ref).all()

    def dense(wgt, start, n_in):
        R = np.zeros((len(start), n_in))
        for i, s in enumerate(np.clip(start, 0, n_in - wgt.shape[1])):
            R[i, s:s + wgt.shape[1]] = wgt[i]
        return R
    Rh, Rw = dense(wh, sh, x.shape[1]), dense(ww, sw, x.shape[2])
    assert bit_equal(np.einsum("dij,wj->diw", np.einsum("ih,dhj->dij", Rh, x), Rw), ref)
    assert bit_equal(np.einsum("ih,dhw->diw", Rh, np.einsum("dhj,wj->dhw", x, Rw)), ref)          # the W pass first


@pytest.mark.parametrize("shape,size", RESIZE_SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_resize_emulation_equals_scipy_zoom_and_the_loops(shape, size):
    """On these shapes the float64 emulation rounded to float32 is scipy.ndimage.zoom(order=3) bit for bit, for float32 and for
    float64 slices; the loops over start + t with the same bands agree with the einsum formulation."""
    from cswin_unet_amd.utils import zoom_operator
    for dtype in ("float32", "float64"):
        x = wide_slices(shape, size, dtype)
        want = np.stack([zoom(s, (size[0] / shape[1], size[1] / shape[2]), order=3) for s in x])
        assert want.shape == (shape[0],) + size and want.dtype == x.dtype
        unequal, ulps = ulp_figures(wide_ref(shape, size, dtype), want.astype(np.float32))
        print(f"{shape} -> {size} {dtype}: emulation vs scipy {unequal} unequal, {ulps:.3g} ulp")
        assert unequal == 0
    x = wide_slices(shape, size, "float32")
    loops = resize_ref(x, *zoom_operator(shape[1], size[0]), *zoom_operator(shape[2], size[1]))
    full = banded_product(x, size)
    assert np.abs(loops - full).max() <= 1e-13 * np.abs(full).max()
    assert within_one_ulp(loops.astype(np.float32), wide_ref(shape, size, "float32"))


def test_resize_comparisons_see_a_dropped_tap_a_shifted_start_and_a_missing_tile_row():
    """Bit-equality on the exact cases sees a dropped last tap at every case (its weight is non-zero by construction), a
    missing last row of a tile wherever the case has one, and a start off by one wherever a start can move.  On scipy's bands the
    last tap of a window is below 2^-64 by construction of zoom_operator, so a dropped tap is the exact cases' to find; the
    other two fail the 1-ulp criterion at every wide shape."""
    from cswin_unet_amd.utils import zoom_operator
    for tag, D, H, W, h, w, Th, Tw, _ in EXACT_CASES:
        x, wh, sh, ww, sw = exact_inputs(tag)
        ref = resize_ref(x, wh, sh, ww, sw)
        TR = resize_plan(W, 0, False)[0]
        assert not bit_equal(resize_ref(x, wh, sh, ww, sw, "drop_tap"), ref), tag
        if h >= TR:
            assert not bit_equal(resize_ref(x, wh, sh, ww, sw, "tile_row", TR), ref), tag
        if Th < H or Tw < W:
            legal = (np.clip(sh, 0, H - Th).astype(np.int32), np.clip(sw, 0, W - Tw).astype(np.int32))
            assert bit_equal(resize_ref(x, wh, legal[0], ww, legal[1]), ref), tag                 # the clamp is part of the reference
            assert not bit_equal(resize_ref(x, wh, legal[0], ww, legal[1], "start"), ref), tag    # and a start off by one is seen
    assert sum(c[4] >= resize_plan(c[3], 0, False)[0] for c in EXACT_CASES) >= 3
    for shape, size in RESIZE_SHAPES:
        x, ref = wide_slices(shape, size, "float32"), wide_ref(shape, size, "float32")
        bands = zoom_operator(shape[1], size[0]) + zoom_operator(shape[2], size[1])
        TR = resize_plan(shape[2], 0, False)[0]
        assert not within_one_ulp(resize_ref(x, *bands, "start").astype(np.float32), ref), (shape, "start")
        if size[0] >= TR:
            assert not within_one_ulp(resize_ref(x, *bands, "tile_row", TR).astype(np.float32), ref), (shape, "tile_row")
    assert {resize_plan(s[2], 0, False)[0] for s, o in RESIZE_SHAPES if o[0] >= resize_plan(s[2], 0, False)[0]} == {16, 8, 4}


@pytest.mark.parametrize("tag", FAR_APART + ("voxel", "h1", "w1", "ncls255"))
def test_seg_references_agree_scipy_brute_force_and_the_three_passes(tag):
    shape, ncls, ndim, _, _ = SEG_CASES[tag]
    pred, label = seg_inputs(tag)
    counts, hist = seg_ref(tag)
    bc, bh = brute_counts_hist(pred, label, ncls, ndim)
    assert np.array_equal(bc, counts) and np.array_equal(bh, hist)
    assert np.array_equal(emulated_hist(pred, label, ncls, ndim), hist)


def test_seg_comparison_sees_a_walk_stopped_early_and_a_skipped_plane():
    """Exact equality of the histogram sees a y walk that stops one step early (the blobs: many nearest seeds lie straight up a
    column, one row nearer than the row's own seed is far) and a z walk that leaves out the last plane of the box (the
    far-apart inputs whose far side lies in that plane)."""
    for tag, wrong in (("corners", "skip_last_plane"), ("deep.small", "skip_last_plane"), ("corners", "y_early"), ("h33", "y_early")):
        if tag == "deep.small":
            pred, label = blob_pair((9, 3, 5), [1], 61)
            pred, label, ncls = pred.copy(), label.copy(), 3
            pred[0, 0, 0], label[8, 2, 4] = 2, 2
        elif tag == "h33":
            pred, label, ncls = *blob_pair((5, 33, 71), [1, 2, 3], 63), 4
        else:
            pred, label, ncls = *seg_inputs(tag), SEG_CASES[tag][1]
        ref = scipy_counts_hist(pred, label, ncls, 3)[1]
        assert np.array_equal(emulated_hist(pred, label, ncls, 3), ref), tag
        bad = emulated_hist(pred, label, ncls, 3, wrong)
        print(f"{tag} {wrong}: {int(np.abs(bad.astype(np.int64) - ref).sum())} histogram counts moved")
        assert not np.array_equal(bad, ref), (tag, wrong)


def test_argmax_reference_and_the_rule_stated_as_a_loop():
    for ncls in (2, 3, 4, 255):
        sp = special_columns(ncls)
        assert [argmax_first(sp[:, k]) for k in range(sp.shape[1])] == special_winners(ncls), ncls
        assert torch.argmax(torch.from_numpy(sp), 0).tolist() == special_winners(ncls), ncls
    assert special_winners(1) == [0] * 7 and np.signbit(special_columns(4)[:, 0]).tolist() == [False, True, False, True]
    for (h, w), (H, W) in ARGMAX_SHAPES[1:]:
        x = argmax_logits(4 if h == 5 else 2, h, w)
        loop = np.array([[[argmax_first(x[b, :, i, j]) for j in range(w)] for i in range(h)] for b in range(ARGMAX_B)])
        ident = argmax_ref(x, np.arange(h, dtype=np.int32), np.arange(w, dtype=np.int32))
        assert np.array_equal(ident, loop)
        rows, cols = index_vector(h, H, "row"), index_vector(w, W, "col")
        want = np.array([[[0 if r < 0 or c < 0 else loop[b, min(r, h - 1), min(c, w - 1)] for c in cols] for r in rows] for b in range(ARGMAX_B)])
        assert np.array_equal(argmax_ref(x, rows, cols), want)
        assert ((x == np.where(np.isnan(x), -np.inf, x).max(axis=1, keepdims=True)).sum(axis=1) > 1).mean() > 0.05
        assert not np.array_equal(argmax_ref(x, rows, cols, later=True), want)                    # ties towards the later class are seen


def test_argmax_tables_hold_what_they_are_there_for():
    assert {s[0][1] for s in ARGMAX_SHAPES} >= {MAX_DIM} and {s[1][0] for s in ARGMAX_SHAPES} >= {MAX_DIM} and set(ARGMAX_NCLS) == {1, 2, MAX_CLS}
    assert argmax_grid(ARGMAX_B, 2048) == (2048, 3)
    for (h, w), (H, W) in ARGMAX_SHAPES:
        for n_in, n_out, name in ((h, H, "row"), (w, W, "col")):
            v = index_vector(n_in, n_out, name)
            assert (v[1:n_out - 1] < 0).any() and (n_out < 5 or (v < -1).any()) and (v == n_in).any() and v[n_out - 1] > n_in
            if n_out >= 8:
                assert (np.diff(v) == 0).any() and (np.diff(v) < 0).any()
    x = argmax_logits(255, 3, 2048)
    assert np.isnan(x).any() and np.isinf(x).any() and np.signbit(x[x == 0]).any()


def test_augment_reference_equals_flip_of_rot90_and_source_index():
    from cswin_unet_amd.utils import rotation_index
    for H, W in AUG_SHAPES:
        x = aug_batch((H, W))[0][0]
        for k in (0, 1, 2, 3, 5, -1, 6):
            for axis in (0, 1):
                want = np.flip(np.rot90(x, k), axis)
                i, j = np.meshgrid(np.arange(want.shape[0]), np.arange(want.shape[1]), indexing="ij")
                src = aug_source_ref(H, W, ROT90_FLIP, k, axis, None, i, j)
                assert np.array_equal(A.gather(x, src), want), (k, axis)
                assert np.array_equal(src, A.source_index(H, W, ROT90_FLIP, k & 3, axis, 0))
                turned = A.gather(x, aug_source_ref(H, W, ROT90_FLIP, k, axis, None, i, j, other_way=True))
                assert np.array_equal(turned, want) == (k % 2 == 0), (k, axis)                    # rot90 the other way is seen
        i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        assert np.array_equal(aug_source_ref(H, W, NONE, 0, 0, None, i, j), A.source_index(H, W, NONE, 0, 0, 0))
        assert np.array_equal(aug_source_ref(H, W, ROTATE, 0, 0, rotation_index(H, W, 19), i, j), A.source_index(H, W, ROTATE, 0, 0, 19))
        assert (aug_source_ref(H, W, ROTATE, 0, 0, None, i, j) == -1).all()
        # the clamps: whatever (i, j) and map, the result is a pixel of the slice or none
        far = np.meshgrid(np.arange(-3, 2 * max(H, W)), np.arange(-3, 2 * max(H, W)), indexing="ij")
        for kind, k, axis, amap in ((ROT90_FLIP, 1, 0, None), (ROT90_FLIP, 2, 1, None), (NONE, 0, 0, None)):
            assert aug_source_ref(H, W, kind, k, axis, amap, *far).min() >= 0 and aug_source_ref(H, W, kind, k, axis, amap, *far).max() < H * W
        bad = bad_map(H, W)
        assert (bad >= H * W).any() and (bad < -1).any() and aug_source_ref(H, W, ROTATE, 0, 0, bad, i, j).max() == H * W - 1
        got = A.gather(x, aug_source_ref(H, W, ROTATE, 0, 0, bad, i, j))
        assert (got[bad < 0] == 0).all() and (got[bad >= H * W] == x[-1, -1]).all()
    # a sample listed with the other group's shape: defined, and not what its own shape would give
    H, W = AUG_SHAPES[0]
    x = aug_batch((H, W))[0]
    mis = aug_gather_ref(x, [(ROT90_FLIP, 1, 0, 0, None)], H, W)[0]
    assert mis.shape == (H, W) and np.isin(mis, x[0]).all()
    assert not np.array_equal(aug_gather_ref(x, aug_descs((H, W), "turned"), W, H), aug_gather_ref(x, aug_descs((H, W), "turned"), W, H, other_way=True))


def test_augment_tables_hold_what_they_are_there_for():
    for shape in AUG_SHAPES:
        H, W = shape
        both = aug_descs(shape, "straight") + aug_descs(shape, "turned")
        assert {(k, axis) for kind, k, axis, _, _ in both if kind == ROT90_FLIP} >= {(k, axis) for k in range(4) for axis in (0, 1)} | {(5, 0), (-1, 1)}
        assert {kind for kind, *_ in both} == {NONE, ROT90_FLIP, ROTATE}
        assert any(kind == ROTATE and m is None for kind, _, _, _, m in both) and any(m is bad_map(H, W) for *_, m in both)
        if H != W:
            assert any(kind == ROT90_FLIP and k & 1 for kind, k, *_ in aug_descs(shape, "straight"))
            assert any(not (kind == ROT90_FLIP and k & 1) for kind, k, *_ in aug_descs(shape, "turned"))
        h, w = AUG_LABEL_SIZES[shape]
        assert h % 16 and w % 16 and augment_grid(5, h, w) == (cdiv(w, 16), cdiv(h, 16), 5)
        for v, n_in in zip(label_indices(shape, (h, w)), (H, W, W, H)):
            assert (v[1:-1] < 0).sum() >= 2 and (v >= n_in).sum() >= 2
        assert (aug_batch(shape)[1] == 255).any()


# ------------------------------------------------------------------------------------------------
# the entry points, called directly with guarded buffers
# ------------------------------------------------------------------------------------------------
GUARD_BYTES = GUARD * 4                                  # as many bytes as Guarded puts round a float32 view: 256
PATTERN = 0xA5


class GuardedInt:
    """Guarded for integer outputs, which cannot be NaN-filled: a byte buffer filled with 0xA5 with GUARD_BYTES before and after
    the view `.t` (`off` bytes past a 16-byte boundary; `.t` is None where that leaves the dtype misaligned and only `.addr`
    is of use).  An element that still holds the pattern counts as never written unless the reference holds that very value."""

    def __init__(self, shape, dtype, off=0):
        self.item = torch.empty((), dtype=dtype).element_size()
        self.nbytes = math.prod(shape) * self.item
        self.lo = GUARD_BYTES + off
        self.buf = torch.full((self.nbytes + 2 * GUARD_BYTES + 16,), PATTERN, dtype=torch.uint8, device=DEV)
        assert self.buf.data_ptr() % 16 == 0
        self.raw = self.buf[self.lo:self.lo + self.nbytes]
        self.addr = self.raw.data_ptr()
        self.t = self.raw.view(dtype).view(shape) if off % self.item == 0 else None
        self.sentinel = int.from_bytes(bytes([PATTERN]) * self.item, "little", signed=dtype != torch.uint8)

    def intact(self):
        return bool((self.buf[:self.lo] == PATTERN).all()) and bool((self.buf[self.lo + self.nbytes:] == PATTERN).all())

    def untouched(self):
        return bool((self.buf == PATTERN).all())

    def written(self, ref=None):
        left = self.t == self.sentinel
        if ref is not None:
            left = left & (torch.from_numpy(np.array(ref)).to(DEV).view(self.t.shape) != self.sentinel)
        return not bool(left.any())


def settle_int(what, bufs, refs=None):
    """settle for GuardedInt outputs; refs: name -> reference values, for outputs in which the pattern is a legal value."""
    torch.cuda.synchronize()
    for name, g in bufs.items():
        assert g.intact(), f"{what}: a guard byte of {name} was overwritten"
        assert name == "workspace" or g.written((refs or {}).get(name)), f"{what}: {name} has elements that were never written"


def put(a, off=0):
    """Device copy of a numpy array, `off` ELEMENTS past a 16-byte boundary.  The caller holds it until it has synchronized."""
    t = torch.from_numpy(np.array(a))
    buf = torch.zeros(t.numel() + 16, dtype=t.dtype, device=DEV)
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == off * t.element_size() % 16
    return v


def at(addr):
    return ctypes.c_void_p(addr)


@pytest.fixture(scope="module")
def hip():
    from cswin_unet_amd import _lib

    class Hip:
        call, ptr, stream, lib, Desc = staticmethod(_lib.call), staticmethod(_lib.ptr), staticmethod(_lib.stream), staticmethod(_lib.lib), _lib.AugmentDesc

        @staticmethod
        def refused(code, what, bufs, name, *args):
            got = getattr(_lib.lib(), name)(*args)
            msg = _lib.lib().cswin_last_error().decode()
            assert got == code, f"{what}: {name} returned {got} ({msg!r}), expected {code}"
            assert msg.startswith(name[len("cswin_"):].replace("_workspace", "")), f"{what}: message {msg!r}"
            torch.cuda.synchronize()
            for n, g in bufs.items():
                assert g.untouched(), f"refused {what}: {n} was written"
    return Hip


# ---- cswin_resize_banded ------------------------------------------------------------------------------------------------------
def run_resize(hip, x, wh, sh, ww, sw, off=0, what=""):
    D, H, W = x.shape
    (h, Th), (w, Tw) = wh.shape, ww.shape
    xd, whd, shd, wwd, swd = put(x, off), put(wh), put(sh), put(ww), put(sw)
    y = Guarded((D, h, w))
    hip.call("cswin_resize_banded", hip.ptr(xd), hip.ptr(y.t), hip.ptr(whd), hip.ptr(shd), Th, hip.ptr(wwd), hip.ptr(swd), Tw, D, H, W, h, w,
             int(x.dtype == np.float64), hip.stream())
    settle(what, dict(y=y))
    return y.t.cpu().numpy()


@gpu
@pytest.mark.parametrize("shape,size,dtype,off", RESIZE_CASES, ids=lambda v: v if isinstance(v, str) else str(v) if isinstance(v, int) else "x".join(map(str, v)))
def test_resize_wide_shapes_within_one_ulp_of_the_float64_product(hip, shape, size, dtype, off):
    from cswin_unet_amd.utils import zoom_operator
    x = wide_slices(shape, size, dtype)
    TR, VEC = resize_plan(shape[2], off * x.itemsize, dtype == "float64")
    tag = f"eval.resize.{shape}->{size}.{dtype}.off{off} <{TR}, {VEC}>"
    got = run_resize(hip, x, *zoom_operator(shape[1], size[0]), *zoom_operator(shape[2], size[1]), off=off, what=tag)
    assert within_one_ulp(got, wide_ref(shape, size, dtype), tag)


@gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("tag", [c[0] for c in EXACT_CASES])
def test_resize_exact_integer_cases_are_bit_equal(hip, tag, dtype):
    off = next(c for c in EXACT_CASES if c[0] == tag)[8]
    x, wh, sh, ww, sw = exact_inputs(tag)
    got = run_resize(hip, x.astype(dtype), wh, sh, ww, sw, off=off, what=f"eval.resize.exact.{tag}.{dtype}")
    ref = resize_ref(x, wh, sh, ww, sw).astype(np.float32)
    bad = np.argwhere(got.view(np.uint32) != ref.view(np.uint32))
    assert len(bad) == 0, (tag, len(bad), [(tuple(k), float(got[tuple(k)]), float(ref[tuple(k)])) for k in bad[:8]])


@gpu
def test_resize_refusals_touch_nothing(hip):
    D, H, W, h, w, Th, Tw = 2, 6, 10, 4, 5, 3, 2
    xd = put(np.ones((D, H, W), np.float32))
    whd, shd, wwd, swd = put(np.ones((h, Th))), put(np.zeros(h, np.int32)), put(np.ones((w, Tw))), put(np.zeros(w, np.int32))
    o = dict(y=Guarded((D, h, w)))

    def args(**kw):
        a = dict(x=hip.ptr(xd), y=hip.ptr(o["y"].t), wh=hip.ptr(whd), sh=hip.ptr(shd), Th=Th, ww=hip.ptr(wwd), sw=hip.ptr(swd), Tw=Tw, D=D, H=H, W=W, h=h, w=w, f64=0)
        a.update(kw)
        return tuple(a.values()) + (hip.stream(),)
    for dim in ("D", "H", "W", "h", "w"):
        hip.refused(ERR_SHAPE, f"{dim} = 0", o, "cswin_resize_banded", *args(**{dim: 0}))
        hip.refused(ERR_SHAPE, f"{dim} = 2049", o, "cswin_resize_banded", *args(**{dim: 2049}))
    hip.refused(ERR_SHAPE, "Th = 0", o, "cswin_resize_banded", *args(Th=0))
    hip.refused(ERR_SHAPE, "Th > H", o, "cswin_resize_banded", *args(Th=H + 1))
    hip.refused(ERR_SHAPE, "Tw = 0", o, "cswin_resize_banded", *args(Tw=0))
    hip.refused(ERR_SHAPE, "Tw > W", o, "cswin_resize_banded", *args(Tw=W + 1))
    hip.refused(ERR_UNSUPPORTED, "x_f64 = 2", o, "cswin_resize_banded", *args(f64=2))
    hip.refused(ERR_ALIGN, "wh 4 bytes off", o, "cswin_resize_banded", *args(wh=at(whd.data_ptr() + 4)))
    hip.refused(ERR_ALIGN, "float64 x 4 bytes off", o, "cswin_resize_banded", *args(x=at(xd.data_ptr() + 4), f64=1))
    for name in ("x", "y", "wh", "sh", "ww", "sw"):
        hip.refused(ERR_SHAPE, f"{name} = NULL", o, "cswin_resize_banded", *args(**{name: None}))


# ---- cswin_seg_metrics --------------------------------------------------------------------------------------------------------
def run_seg(hip, pred, label, ncls, ndim, pred_off=0, label_off=0, what=""):
    """One call with pattern-filled guarded counts / hist and a guarded workspace of exactly the size the library asks for;
    returns (counts int64 [ncls, 4], hist int32 [ncls, nbins]) on the CPU."""
    D, H, W = pred.shape
    nbins, nbytes = hip.lib().cswin_seg_metrics_nbins(D, H, W), hip.lib().cswin_seg_metrics_workspace(D, H, W, ndim, ncls)
    assert nbins == nbins_of(pred.shape) and nbytes == seg_workspace(D, H, W, ncls)
    pd, ld = put(pred.reshape(-1), pred_off), put(label.reshape(-1), label_off)
    assert seg_plan(H, pd.data_ptr(), ld.data_ptr()) == seg_plan(H, pred_off, label_off)
    o = dict(counts=GuardedInt((ncls, 4), torch.int64), hist=GuardedInt((ncls, nbins), torch.int32), workspace=GuardedInt((nbytes,), torch.uint8))
    assert not bool((o["counts"].t == 0).any()) and not bool((o["hist"].t == 0).any())          # nothing is zero before the call
    hip.call("cswin_seg_metrics", hip.ptr(pd), hip.ptr(ld), at(o["counts"].addr), at(o["hist"].addr), at(o["workspace"].addr), nbytes, D, H, W,
             ndim, ncls, hip.stream())
    settle_int(what, o)
    return o["counts"].t.cpu(), o["hist"].t.cpu()


def check_seg(counts, hist, wc, wh, what, rows=None):
    """Exact equality with the reference (on `rows`: all), hist[c].sum() = counts[c][3] where both sides are present and 0
    elsewhere, row 0 zero."""
    wc, wh = torch.from_numpy(np.asarray(wc)), torch.from_numpy(np.asarray(wh))
    rows = range(counts.shape[0]) if rows is None else rows
    for c in rows:
        assert torch.equal(counts[c], wc[c]), (what, c, counts[c].tolist(), wc[c].tolist())
        diff = (hist[c] != wh[c]).nonzero().reshape(-1)
        assert len(diff) == 0, (what, c, len(diff), [(int(s), int(hist[c, s]), int(wh[c, s])) for s in diff[:8]])
        both = c > 0 and counts[c, 0] > 0 and counts[c, 1] > 0
        assert int(hist[c].sum()) == (int(counts[c, 3]) if both else 0), (what, c)
    assert not bool(hist[0].any()), what


@gpu
@pytest.mark.parametrize("tag", sorted(SEG_CASES))
def test_seg_metrics_equal_scipy_at_every_tile_and_limit(hip, tag):
    shape, ncls, ndim, po, lo = SEG_CASES[tag]
    pred, label = seg_inputs(tag)
    counts, hist = run_seg(hip, pred, label, ncls, ndim, po, lo, what=f"eval.seg.{tag}")
    check_seg(counts, hist, *seg_ref(tag), tag)
    if tag in FAR_APART:
        assert int(counts[1, 0]) > 0 and int(counts[1, 1]) > 0 and int(hist[1].sum()) == int(counts[1, 3])


@gpu
def test_seg_metrics_two_calls_give_the_same_bits(hip):
    pred, label = seg_inputs("blob1030")
    a = run_seg(hip, pred, label, 4, 3, what="eval.seg.twice.a")
    b = run_seg(hip, pred, label, 4, 3, 8, 1, what="eval.seg.twice.b")                           # and the byte loads the same as the 16-B ones
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@gpu
def test_seg_metrics_ids_past_ncls_leave_the_legal_rows_right(hip):
    """Ids >= ncls are the caller's error.  What the kernel's comment promises: they are never counted, and to the legal classes
    they are "another class" -- rows 0 .. ncls - 1 are those of the same volumes measured with enough classes."""
    pred, label = blob_pair((5, 33, 71), [1, 2, 3, 4], 66)
    pred, label = pred.copy(), label.copy()
    pred[2, 16, 30:40], label[1, 3, 3] = 254, 255
    assert (pred >= 3).any() and (label >= 3).any()
    counts, hist = run_seg(hip, pred, label, 3, 3, what="eval.seg.illegal")
    wc, wh = scipy_counts_hist(pred, label, 256, 3)
    check_seg(counts, hist, wc[:3], wh[:3], "illegal ids")


@gpu
def test_seg_metrics_refusals_touch_nothing(hip):
    D, H, W, ncls = 2, 9, 11, 4
    nbins, nbytes = nbins_of((D, H, W)), seg_workspace(D, H, W, ncls)
    pd, ld = put(np.ones(D * H * W, np.uint8)), put(np.ones(D * H * W, np.uint8))
    o = dict(counts=GuardedInt((ncls, 4), torch.int64), hist=GuardedInt((ncls, nbins), torch.int32), workspace=GuardedInt((nbytes + 16,), torch.uint8))

    def args(**kw):
        a = dict(pred=hip.ptr(pd), label=hip.ptr(ld), counts=at(o["counts"].addr), hist=at(o["hist"].addr), ws=at(o["workspace"].addr), nbytes=nbytes,
                 D=D, H=H, W=W, ndim=3, ncls=ncls)
        a.update(kw)
        return tuple(a.values()) + (hip.stream(),)
    hip.refused(ERR_WORKSPACE, "workspace one byte short", o, "cswin_seg_metrics", *args(nbytes=nbytes - 1))
    hip.refused(ERR_WORKSPACE, "workspace NULL", o, "cswin_seg_metrics", *args(ws=None))
    hip.refused(ERR_ALIGN, "workspace 8 bytes off", o, "cswin_seg_metrics", *args(ws=at(o["workspace"].addr + 8)))
    hip.refused(ERR_ALIGN, "counts 4 bytes off", o, "cswin_seg_metrics", *args(counts=at(o["counts"].addr + 4)))
    hip.refused(ERR_ALIGN, "hist 2 bytes off", o, "cswin_seg_metrics", *args(hist=at(o["hist"].addr + 2)))
    hip.refused(ERR_SHAPE, "ndim 2 with D = 2", o, "cswin_seg_metrics", *args(ndim=2))
    hip.refused(ERR_SHAPE, "ndim 4", o, "cswin_seg_metrics", *args(ndim=4))
    hip.refused(ERR_SHAPE, "ncls 1", o, "cswin_seg_metrics", *args(ncls=1))
    hip.refused(ERR_SHAPE, "ncls 256", o, "cswin_seg_metrics", *args(ncls=256))
    hip.refused(ERR_SHAPE, "H = 2049", o, "cswin_seg_metrics", *args(H=2049))
    hip.refused(ERR_SHAPE, "W = 0", o, "cswin_seg_metrics", *args(W=0))
    hip.refused(ERR_SHAPE, "pred NULL", o, "cswin_seg_metrics", *args(pred=None))
    for bad in ((2, H, W, 2, ncls), (D, H, W, 4, ncls), (D, H, W, 3, 1), (D, H, W, 3, 256)):
        assert hip.lib().cswin_seg_metrics_workspace(*bad) == 0 and hip.lib().cswin_last_error().decode().startswith("seg_metrics")
    assert hip.lib().cswin_seg_metrics_nbins(D, 2049, W) == 0


# ---- cswin_argmax_zoom_back ---------------------------------------------------------------------------------------------------
def run_argmax(hip, logits, rows, cols, ref, what=""):
    B, ncls, h, w = logits.shape
    ld, rd, cd = put(logits), put(rows), put(cols)
    o = dict(out=GuardedInt((B, len(rows), len(cols)), torch.uint8))
    hip.call("cswin_argmax_zoom_back", hip.ptr(ld), at(o["out"].addr), hip.ptr(rd), hip.ptr(cd), B, ncls, h, w, len(rows), len(cols), hip.stream())
    settle_int(what, o, dict(out=ref))
    return o["out"].t.cpu().numpy()


@gpu
@pytest.mark.parametrize("ncls", ARGMAX_NCLS)
@pytest.mark.parametrize("hw,HW", ARGMAX_SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_argmax_zoom_back_with_hand_made_indices_and_special_values(hip, hw, HW, ncls):
    (h, w), (H, W) = hw, HW
    logits = argmax_logits(ncls, h, w)
    rows, cols = index_vector(h, H, "row"), index_vector(w, W, "col")
    ref = argmax_ref(logits, rows, cols)
    got = run_argmax(hip, logits, rows, cols, ref, what=f"eval.argmax.{hw}->{HW}.ncls{ncls}")
    bad = np.argwhere(got != ref)
    assert len(bad) == 0, (len(bad), [(tuple(k), int(got[tuple(k)]), int(ref[tuple(k)])) for k in bad[:8]])
    assert ncls > 1 or not got.any()


@gpu
def test_argmax_special_values_column_by_column(hip):
    """The seven special columns alone, through identity indices: the winners worked out by hand."""
    for ncls in (2, 3, 4, 255):
        sp = special_columns(ncls)
        logits = np.ascontiguousarray(np.broadcast_to(sp[None, :, None, :], (1, ncls, 2, sp.shape[1])))
        want = np.broadcast_to(np.array(special_winners(ncls), np.uint8), (1, 2, sp.shape[1]))
        got = run_argmax(hip, logits, np.arange(2, dtype=np.int32), np.arange(sp.shape[1], dtype=np.int32), want, what=f"eval.argmax.special.{ncls}")
        assert np.array_equal(got, want), (ncls, got[0, 0].tolist(), special_winners(ncls))


@gpu
def test_argmax_refusals_touch_nothing(hip):
    B, ncls, h, w, H, W = 2, 3, 4, 5, 6, 7
    ld, rd, cd = put(np.zeros((B, ncls, h, w), np.float32)), put(np.zeros(H, np.int32)), put(np.zeros(W, np.int32))
    o = dict(out=GuardedInt((B, H, W), torch.uint8))

    def args(**kw):
        a = dict(logits=hip.ptr(ld), out=at(o["out"].addr), rows=hip.ptr(rd), cols=hip.ptr(cd), B=B, ncls=ncls, h=h, w=w, H=H, W=W)
        a.update(kw)
        return tuple(a.values()) + (hip.stream(),)
    hip.refused(ERR_SHAPE, "ncls 0", o, "cswin_argmax_zoom_back", *args(ncls=0))
    hip.refused(ERR_SHAPE, "ncls 256", o, "cswin_argmax_zoom_back", *args(ncls=256))
    for dim in ("B", "h", "w", "H", "W"):
        hip.refused(ERR_SHAPE, f"{dim} = 2049", o, "cswin_argmax_zoom_back", *args(**{dim: 2049}))
        hip.refused(ERR_SHAPE, f"{dim} = 0", o, "cswin_argmax_zoom_back", *args(**{dim: 0}))
    hip.refused(ERR_SHAPE, "rows NULL", o, "cswin_argmax_zoom_back", *args(rows=None))
    hip.refused(ERR_ALIGN, "cols 2 bytes off", o, "cswin_argmax_zoom_back", *args(cols=at(cd.data_ptr() + 2)))


# ---- cswin_augment_gather / cswin_augment_labels ------------------------------------------------------------------------------
def aug_table(hip, descs):
    """(device table of cswin_augment_desc records, the device maps it points to) of [(kind, k, axis, src, map or None)]."""
    maps = {id(m): put(np.asarray(m, np.int32)) for *_, m in descs if m is not None}
    table = (hip.Desc * len(descs))()
    for d, (kind, k, axis, src, m) in zip(table, descs):
        d.kind, d.k, d.axis, d.src, d.map = kind, k, axis, src, None if m is None else maps[id(m)].data_ptr()
    assert ctypes.sizeof(table) == 24 * len(descs)
    return put(np.frombuffer(table, dtype=np.int64).copy()), maps


def run_gather(hip, x, descs, Ho, Wo, what=""):
    B, H, W = x.shape
    xd = put(x)
    table, maps = aug_table(hip, descs)
    o = dict(y=Guarded((len(descs), Ho, Wo)))
    hip.call("cswin_augment_gather", hip.ptr(xd), hip.ptr(o["y"].t), hip.ptr(table), len(descs), B, H, W, Ho, Wo, hip.stream())
    settle(what, o)
    return o["y"].t.cpu().numpy()


def run_labels(hip, lab, descs, idx, what=""):
    B, H, W = lab.shape
    h, w = len(idx[0]), len(idx[1])
    ld, idxd = put(lab), [put(v) for v in idx]
    table, maps = aug_table(hip, descs)
    o = dict(out=GuardedInt((len(descs), h, w), torch.int64))
    hip.call("cswin_augment_labels", hip.ptr(ld), at(o["out"].addr), hip.ptr(table), *[hip.ptr(v) for v in idxd], len(descs), B, H, W, h, w, hip.stream())
    settle_int(what, o)
    return o["out"].t.cpu().numpy()


def same_bits(got, ref, what):
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    bad = np.argwhere(got.view(np.uint32) != ref.view(np.uint32)) if got.dtype == np.float32 else np.argwhere(got != ref)
    assert got.shape == ref.shape and len(bad) == 0, (what, len(bad), [(tuple(k), got[tuple(k)].item(), ref[tuple(k)].item()) for k in bad[:8]])


@gpu
@pytest.mark.parametrize("shape", AUG_SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_augment_gather_every_transform_map_and_clamp(hip, shape):
    """Both calls of a shape: every (k, axis), k = 5 and -1, kind 0, real / NULL / out-of-range maps, and on the non-square
    shape the samples listed with the other group's output shape.  Values are copied: the bits must be the source's."""
    x = aug_batch(shape)[0]
    H, W = shape
    for group, (Ho, Wo) in (("straight", (H, W)), ("turned", (W, H))):
        descs = aug_descs(shape, group)
        got = run_gather(hip, x, descs, Ho, Wo, what=f"eval.gather.{shape}.{group}")
        same_bits(got, aug_gather_ref(x, descs, Ho, Wo), (shape, group))
        null = next(s for s, d in enumerate(descs) if d[0] == ROTATE and d[4] is None) if group == "straight" or H == W else None
        assert null is None or not got[null].any()


@gpu
def test_augment_src_indirection_with_more_samples_than_slices(hip):
    """n = 5 samples of B = 3 slices, src = (2, 0, 2, 7, -1): the last two are clamped to slices 2 and 0."""
    from cswin_unet_amd.utils import rotation_index
    for shape in AUG_SHAPES:
        x, lab = aug_batch(shape)
        H, W = shape
        kinds = [(NONE, 0, 0, None), (ROT90_FLIP, 2, 1, None), (ROTATE, 0, 0, rotation_index(H, W, -7)), (ROT90_FLIP, 0, 0, None), (NONE, 0, 0, None)]
        descs = [(kind, k, axis, src, m) for (kind, k, axis, m), src in zip(kinds, (2, 0, 2, 7, -1))]
        got = run_gather(hip, x, descs, H, W, what=f"eval.gather.src.{shape}")
        same_bits(got, aug_gather_ref(x, descs, H, W), shape)
        assert np.array_equal(got[0], x[2]) and np.array_equal(got[4], x[0]) and np.array_equal(got[3], x[2][::-1])
        idx = label_indices(shape, AUG_LABEL_SIZES[shape])
        same_bits(run_labels(hip, lab, descs, idx, what=f"eval.labels.src.{shape}"), aug_labels_ref(lab, descs, *idx), shape)


@gpu
@pytest.mark.parametrize("shape", AUG_SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_augment_labels_mixed_batch_with_hand_made_indices(hip, shape):
    """Transposing and non-transposing samples in one launch (both index pairs are read), every transform of the gather test,
    the value 255, (h, w) off the 16 x 16 tile, negative entries in the middle of the index vectors and entries past the end."""
    lab = aug_batch(shape)[1]
    descs = aug_descs(shape, "straight") + aug_descs(shape, "turned")
    descs = [d[:3] + (src,) + d[4:] for d, src in zip(descs, [0, 1, 2, 7, -1] * len(descs))]
    idx = label_indices(shape, AUG_LABEL_SIZES[shape])
    got = run_labels(hip, lab, descs, idx, what=f"eval.labels.{shape}")
    ref = aug_labels_ref(lab, descs, *idx)
    same_bits(got, ref, shape)
    assert (ref == 255).any() and (ref[:, len(idx[0]) // 2] == 0).all() and (ref[:, :, 2] == 0).all()
    tr = [s for s, d in enumerate(descs) if d[0] == ROT90_FLIP and d[1] & 1]
    assert tr and len(tr) < len(descs)


@gpu
def test_augment_refusals_touch_nothing(hip):
    B, H, W, h, w = 2, 6, 10, 5, 7
    xd, ld = put(np.ones((B, H, W), np.float32)), put(np.ones((B, H, W), np.uint8))
    table, _ = aug_table(hip, [(NONE, 0, 0, 0, None), (ROT90_FLIP, 2, 0, 1, None)])
    idx = [put(np.zeros(n, np.int32)) for n in (h, w, h, w)]
    o = dict(y=Guarded((2, H, W)), out=GuardedInt((2, h, w), torch.int64))

    def gargs(**kw):
        a = dict(x=hip.ptr(xd), y=hip.ptr(o["y"].t), table=hip.ptr(table), n=2, B=B, H=H, W=W, Ho=H, Wo=W)
        a.update(kw)
        return tuple(a.values()) + (hip.stream(),)

    def largs(**kw):
        a = dict(lab=hip.ptr(ld), out=at(o["out"].addr), table=hip.ptr(table), r=hip.ptr(idx[0]), c=hip.ptr(idx[1]), rt=hip.ptr(idx[2]), ct=hip.ptr(idx[3]),
                 n=2, B=B, H=H, W=W, h=h, w=w)
        a.update(kw)
        return tuple(a.values()) + (hip.stream(),)
    hip.refused(ERR_SHAPE, "output neither the shape nor its transpose", o, "cswin_augment_gather", *gargs(Ho=H, Wo=H))
    hip.refused(ERR_SHAPE, "output (W, W)", o, "cswin_augment_gather", *gargs(Ho=W, Wo=W))
    hip.refused(ERR_SHAPE, "n = 0", o, "cswin_augment_gather", *gargs(n=0))
    hip.refused(ERR_SHAPE, "H = 2049", o, "cswin_augment_gather", *gargs(H=2049, Ho=2049))
    hip.refused(ERR_SHAPE, "table NULL", o, "cswin_augment_gather", *gargs(table=None))
    hip.refused(ERR_ALIGN, "table 4 bytes off", o, "cswin_augment_gather", *gargs(table=at(table.data_ptr() + 4)))
    hip.refused(ERR_ALIGN, "table 4 bytes off", o, "cswin_augment_labels", *largs(table=at(table.data_ptr() + 4)))
    hip.refused(ERR_ALIGN, "label output 4 bytes off", o, "cswin_augment_labels", *largs(out=at(o["out"].addr + 4)))
    hip.refused(ERR_ALIGN, "src_col_t 2 bytes off", o, "cswin_augment_labels", *largs(ct=at(idx[3].data_ptr() + 2)))
    hip.refused(ERR_SHAPE, "w = 2049", o, "cswin_augment_labels", *largs(w=2049))
    hip.refused(ERR_SHAPE, "B = 0", o, "cswin_augment_labels", *largs(B=0))
    hip.refused(ERR_SHAPE, "src_row_t NULL", o, "cswin_augment_labels", *largs(rt=None))
