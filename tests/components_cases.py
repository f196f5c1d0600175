"""Shared by tests/test_components_host.py, tests/test_gpu_components.py and tests/test_gpu_components_shapes.py (not a test
module; the last one's case tables and the branch conditions they are checked against are in the lower half): the volumes the connected-
component kernels are tried on, the canonical labels and sizes built from scipy.ndimage.label, and the filter rule written out
component by component with scipy -- a second construction beside utils.filter_components_host, which the host test compares."""
import math

import numpy as np
from scipy.ndimage import label

from seg_metrics_cases import _ellipsoid


def canonical_labels(vol, ncls):
    """(labels int32, sizes int32) of vol's shape as include/cswin_hip.h defines them: labels = 0 for ids 0 and >= ncls, else
    1 + the smallest flat index of the voxel's face-connected component of its class; sizes = the component's voxel count at that
    smallest index, 0 elsewhere.  scipy's own numbering is never relied on: np.unique's first occurrence of a scipy label in
    C order is the component's smallest flat index."""
    vol = np.asarray(vol)
    labels, sizes = np.zeros(vol.size, np.int32), np.zeros(vol.size, np.int32)
    for c in range(1, ncls):
        lab, n = label(vol == c)
        if n == 0:
            continue
        flat = lab.ravel()
        ids, first, counts = np.unique(flat, return_index=True, return_counts=True)
        fg = ids > 0
        root = np.zeros(n + 1, np.int64)
        root[ids[fg]] = first[fg]
        on = flat > 0
        labels[on] = (root[flat[on]] + 1).astype(np.int32)
        sizes[first[fg]] = counts[fg]
    return labels.reshape(vol.shape), sizes.reshape(vol.shape)


def scipy_filter(vol, ncls, min_size, min_fraction):
    """The filter rule of the issue, one component at a time: min_size / min_fraction are sequences of ncls entries (entry 0
    unused).  A component of class c is kept iff its size >= max(min_size[c], ceil(min_fraction[c] * largest_c))."""
    vol = np.asarray(vol)
    out = vol.copy()
    for c in range(1, ncls):
        lab, n = label(vol == c)
        comps = [lab == k for k in range(1, n + 1)]
        if not comps:
            continue
        largest = max(int(m.sum()) for m in comps)
        thr = max(int(min_size[c]), math.ceil(float(min_fraction[c]) * float(largest)))
        for m in comps:
            if int(m.sum()) < thr:
                out[m] = 0
    return out


def rule_tables(rule, ncls):
    """(min_size, min_fraction) lists of a rule, written independently of utils.component_rule_tables."""
    if rule == "largest":
        return [0] * ncls, [0.0] + [1.0] * (ncls - 1)
    ms, mf = [0] * ncls, [0.0] * ncls
    for c, spec in rule.items():
        ms[c], mf[c] = spec.get("min_size", 0), spec.get("min_fraction", 0.0)
    return ms, mf


def noise(shape, ncls, density, seed):
    """Every voxel foreground with probability `density`, its class uniform in 1..ncls (ncls itself is out of range: background)."""
    rng = np.random.default_rng(seed)
    return np.where(rng.random(shape) < density, rng.integers(1, ncls + 1, shape), 0).astype(np.uint8)


def serpentine(shape):
    """One class-1 path: every second row of every second layer is full, consecutive full rows are joined by one voxel at
    alternating ends, consecutive full layers by one voxel at (z + 1, 0, 0).  One component with the deepest chains there are."""
    D, H, W = shape
    v = np.zeros(shape, np.uint8)
    for z in range(0, D, 2):
        v[z, 0::2, :] = 1
        for y in range(1, H, 2):
            v[z, y, W - 1 if (y // 2) % 2 == 0 else 0] = 1
        if z + 1 < D:
            v[z + 1, 0, 0] = 1
    return v


def checkerboard(shape):
    z, y, x = np.indices(shape)
    return (1 + ((x + y + z) & 1)).astype(np.uint8)


def organ_volume(shape=(12, 40, 36), seed=21, speck_fraction=0.02):
    """Nine-class volume in the style of seg_metrics_cases.blob_pair: one ellipsoid for each class 1..8, class 3 a second time
    as an exact copy shifted along x (two equal largest components, like paired organs), then single-voxel specks of random
    foreground classes on background voxels."""
    rng = np.random.default_rng(seed)
    vol = np.zeros(shape, np.uint8)
    dims = np.asarray(shape, np.float64)
    for cid in (1, 2, 4, 5, 6, 7, 8):
        _ellipsoid(vol, rng.uniform(0.15, 0.85, 3) * (dims - 1), np.maximum(rng.uniform(0.08, 0.2, 3) * dims, 1.0), cid)
    bg = np.flatnonzero(vol.ravel() == 0)
    pick = rng.choice(bg, max(8, int(speck_fraction * vol.size)), replace=False)
    vol.ravel()[pick] = rng.integers(1, 9, pick.size).astype(np.uint8)
    blob = np.zeros((5, 7, 6), np.uint8)
    _ellipsoid(blob, np.asarray([2.0, 3.0, 2.5]), np.asarray([2.0, 3.0, 2.5]), 3)
    for x0 in (2, 20):                                      # two copies, each inside a cleared box: nothing else touches them
        vol[0:7, 29:38, x0 - 1:x0 + 7] = 0
        vol[1:6, 30:37, x0:x0 + 6] = blob
    return vol


def speckled_two_class(shape=(6, 40, 48), seed=5):
    """(prediction-to-be, label): the label is one class-1 box; the prediction is the label plus 120 far specks of class 1 --
    more than 5 % of all border voxels, so that they decide the unfiltered HD95.  Filtering the prediction with "largest" gives
    the label back."""
    rng = np.random.default_rng(seed)
    lab = np.zeros(shape, np.uint8)
    lab[1:5, 8:20, 10:24] = 1
    pred = lab.copy()
    far = pred[:, 28:, 30:]          # a view: written through
    pick = rng.choice(far.size, 120, replace=False)
    z, y, x = np.unravel_index(pick, far.shape)
    far[z, y, x] = 1
    return pred, lab


# ------------------------------------------------------------------------------------------------
# the vectorised filter reference, percolating noise and the case tables of tests/test_gpu_components_shapes.py
# ------------------------------------------------------------------------------------------------
TILE = (4, 16, 64)                   # ops.COMPONENT_TILE (csrc/components_uf.h: CC_TZ, CC_TY, CC_TX); the host test compares
SEG = 16                             # CC_VOX: voxels per thread of the tile and seam passes
CF_VOX = 4                           # voxels per thread of the filter pass
PERCOLATION = {3: 0.3116, 2: 0.5927}          # site-percolation thresholds of the cubic and the square lattice


def percolating(shape, nfg, density, seed):
    """noise() with nfg foreground classes whose per-class density lies above the site-percolation threshold of the lattice
    (3-D, or 2-D for a single slice): each class then has one component that spans the volume, wound round ~10^4 .. 10^5
    small ones -- the load under which workgroups of the seam pass meet in the same union-find chains."""
    lattice = 2 if min(shape) == 1 else 3
    assert len(shape) == 3 and sorted(shape)[1] > 1 and density / nfg > PERCOLATION[lattice], (shape, nfg, density)
    return noise(shape, nfg, density, seed)


def filter_ref(vol, ncls, min_size, min_fraction):
    """The filter rule from canonical_labels, vectorised (scipy_filter builds one mask per component: fine for an organ volume,
    hopeless on 10^5 components).  A voxel's component size is sizes[label - 1]; the largest component of a class is a maximum
    over the roots; the threshold is formed in Python floats exactly as the rule states it."""
    vol = np.asarray(vol)
    labels, sizes = canonical_labels(vol, ncls)
    labels, sizes, flat = labels.ravel(), sizes.ravel(), vol.ravel()
    roots = np.flatnonzero(sizes)
    largest = np.zeros(ncls, np.int64)
    np.maximum.at(largest, flat[roots].astype(np.int64), sizes[roots].astype(np.int64))
    thr = np.zeros(256, np.float64)          # exact: every threshold that matters is an integer below 2^53 or beyond every size
    for c in range(1, ncls):
        thr[c] = max(int(min_size[c]), math.ceil(float(min_fraction[c]) * float(largest[c])))
    on = labels > 0
    drop = np.zeros(flat.size, bool)
    drop[on] = sizes[labels[on] - 1] < thr[flat[on]]
    return np.where(drop, 0, flat).astype(vol.dtype).reshape(vol.shape)


def tiles_of(shape):
    return math.prod(-(-n // t) for n, t in zip(shape, TILE))


def component_census(vol, ncls):
    """{class: (voxels of its largest component, tiles that component touches)}, the number of components, the number of tiles."""
    labels, sizes = canonical_labels(vol, ncls)
    z, y, x = np.indices(vol.shape, sparse=True)
    ny, nx = -(-vol.shape[1] // TILE[1]), -(-vol.shape[2] // TILE[2])
    tile = np.broadcast_to(((z // TILE[0]) * ny + y // TILE[1]) * nx + x // TILE[2], vol.shape)
    flat, big = np.asarray(vol).ravel(), {}
    roots = np.flatnonzero(sizes.ravel())
    for c in np.unique(flat[roots]).tolist():
        r = roots[flat[roots] == c]
        top = r[np.argmax(sizes.ravel()[r])]
        big[c] = (int(sizes.ravel()[top]), int(np.unique(tile[labels == top + 1]).size))
    return big, int(roots.size), tiles_of(vol.shape)


# name -> (builder, ncls).  The first two are the contended ones: every class has a spanning component among >= 10^4 others.
CONTENTION = {
    "noise3d": (lambda: percolating((33, 130, 515), 2, 0.72, 11), 3),          # ragged tiles on all three axes, 729 of them
    "slice": (lambda: percolating((1, 512, 1024), 1, 0.62, 11), 2),           # 512 tiles, seams in x and y only
    "solid": (lambda: np.ones((32, 128, 512), np.uint8), 2),                   # every tile's root hangs under voxel 0
    "serpentine": (lambda: serpentine((33, 130, 515)), 2),                     # one component, the deepest chain
}
PERCOLATING = ("noise3d", "slice")
CONTENTION_RULE = {1: {"min_fraction": 1.0}, 2: {"min_size": 50}}              # "largest" for class 1, a size for class 2


def ids_volume(shape, ids, seed):
    """Every voxel one of `ids`, uniformly."""
    return np.random.default_rng(seed).choice(np.asarray(ids, np.uint8), shape)


def seam_lanes(axis, a, b):
    """Two tiles along `axis` (0 = z, 1 = y, 2 = x), five lanes that cross the seam between them, background in between.  a, b
    are ids >= ncls.  Along the axis every lane holds four blocks, two on either side of the seam:
        1 a | b 1      two different illegal ids face each other; the class-1 blocks behind them must stay apart
        1 a | a 1      one illegal id on both sides: equal raw bytes, still no link
        0 1 | a 0      class 1 faces an illegal id, and the other way round
        0 a | 1 0
        2 1 | 1 2      the control: a legal link, one component across the seam
    Lanes are three voxels wide in the in-face axes, so the link rule's `previous voxel` sees illegal ids too."""
    lanes = [(1, a, b, 1), (1, a, a, 1), (0, 1, a, 0), (0, a, 1, 0), (2, 1, 1, 2)]
    t = TILE[axis]
    cross = [4 * len(lanes) + 1, 5]
    shape = cross[:axis] + [2 * t] + cross[axis:]
    v = np.zeros(shape, np.uint8)
    w = np.moveaxis(v, axis, 0)          # (along, lanes, depth): a view
    half = t // 2
    for k, lane in enumerate(lanes):
        for q, cid in enumerate(lane):
            lo = (0, half, t, t + half)[q]
            w[lo:lo + half, 4 * k + 1:4 * k + 4, 1:4] = cid
    return v


def placed(W, comps):
    """(1, 2 * len(comps), W): component k is a run of comps[k] = (id, size) voxels in row 2 * k, from a start that varies; the
    odd rows are background, so every run is one component of exactly that size."""
    v = np.zeros((1, 2 * len(comps), W), np.uint8)
    for k, (cid, size) in enumerate(comps):
        x0 = (3 * k) % (W - size + 1)
        v[0, 2 * k, x0:x0 + size] = cid
    return v


def word_gaps():
    """(1, 1, 48): four-voxel words, all-background ones between foreground ones (the vector path's early-out) and words that
    are part background."""
    words = [[1, 1, 1, 1], [0, 0, 0, 0], [1, 0, 0, 2], [0, 0, 0, 0], [0, 0, 0, 0], [2, 2, 2, 0], [0, 0, 0, 0], [0, 1, 1, 0], [0, 0, 0, 0],
             [3, 255, 0, 1], [0, 0, 0, 0], [1, 1, 2, 2]]
    return np.asarray(words, np.uint8).reshape(1, 1, -1)


# labelling: (shape, ids, ncls, density-free seed).  Two tiles along z and y, one to three along x.
LABEL_W = (16, 64, 66, 77, 130)
LABEL_SHAPE = lambda W: (5, 18, W)
LABEL_VOL_OFF = (0, 1, 4)            # bytes past a 16-byte boundary
LABEL_OUT_OFF = (0, 4)               # labels and sizes, bytes
LABEL_NCLS = 3                       # on noise with ids 1..3: id 3 is out of range
LINES = [(1, 1, 2048), (1, 2048, 1), (2048, 1, 1)]
LABEL_IDS = {"ncls2": ((6, 19, 70), (0, 1, 2, 255), 2), "ncls255": ((6, 19, 70), (0, 253, 254, 255), 255)}
SEAM_IDS = {"two": (3, 200), "one": (255, 255)}          # ncls = 3: the id `at` ncls, and ids beyond it


def label_volume(W):
    return noise(LABEL_SHAPE(W), 3, 0.8, 300 + W)


# filter: name -> (builder, ncls, rule as utils.component_rule_tables takes it)
MIX_IDS = (0, 0, 1, 1, 1, 2, 2, 3, 255)
MIX_RULE = {1: {"min_fraction": 0.5}, 2: {"min_size": 2}}
FILTER_N = {3: (1, 1, 3), 30: (2, 3, 5), 63: (1, 7, 9), 105: (3, 5, 7), 1025: (1, 25, 41)}
FILTER_CASES = {f"n{n}": ((lambda s=s, n=n: ids_volume(s, MIX_IDS, 700 + n)), 3, MIX_RULE) for n, s in FILTER_N.items()}
FILTER_CASES.update({
    "gaps": (word_gaps, 3, {1: {"min_size": 2}, 2: {"min_size": 3}}),
    "ncls255": (lambda: ids_volume((2, 9, 13), (0, 0, 253, 254, 254, 254, 255), 77), 255, {254: {"min_fraction": 0.5}, 253: {"min_size": 2}}),
    "huge": (lambda: ids_volume((2, 9, 13), (0, 1, 1, 2, 3), 78), 3, {1: {"min_size": 2 ** 40}}),
    "absent": (lambda: ids_volume((2, 9, 13), (0, 1, 3, 3), 79), 4, {1: {"min_size": 2}, 2: {"min_fraction": 1.0, "min_size": 5}}),
    # 0.1 * 30 rounds to 3.0 in float64 (threshold 3: the 3s stay, being equal to it); 0.07 * 100 to 7.000000000000001 (threshold 8)
    "ceil": (lambda: placed(32, [(1, 3), (1, 4), (1, 30), (2, 3), (1, 2), (1, 3), (1, 4)]), 3, {1: {"min_fraction": 0.1}}),
    "ceil_up": (lambda: placed(104, [(1, 7), (1, 8), (1, 100), (2, 7), (1, 7), (1, 6)]), 3, {1: {"min_fraction": 0.07}}),
    "tie": (lambda: placed(20, [(1, 7), (1, 12), (2, 5), (1, 12), (1, 11), (255, 4)]), 2, "largest"),
})
# (vol, out, labels) in bytes past a 16-byte boundary; out = None: in place
FILTER_ALIGN = [(0, 0, 0), (1, 0, 0), (0, 2, 0), (0, 0, 4), (0, None, 0), (1, None, 0)]


def label_branches(shape, vol_off):
    """The branch conditions of cc_tile_kernel / cc_seam_kernel / cc_load16 restated (they MUST FOLLOW csrc/components.hip), for
    a volume whose base lies vol_off bytes past a 16-byte boundary: the set of (condition, side) pairs that its threads take."""
    D, H, W = shape
    z, y, x0 = np.meshgrid(np.arange(D), np.arange(H), np.arange(0, W, SEG), indexing="ij")          # the threads with nvalid > 0
    lz, ly, seg = z % TILE[0], y % TILE[1], (x0 % TILE[2]) // SEG
    full = np.minimum(W - x0, SEG) == SEG
    v0 = (z * H + y) * W + x0
    fz, fy, fx = (lz == 0) & (z > 0), (ly == 0) & (y > 0), (seg == 0) & (x0 > 0)
    took = set()
    def see(name, cond, where=None):
        took.update((name, bool(b)) for b in np.unique(cond if where is None else cond[where]))
    see("nvalid == 16", full)
    see("tile load 16 B", (vol_off + v0) % 16 == 0, full)
    see("store int4", v0 % 4 == 0, full)
    for name, face, back in (("fy", fy, W), ("fz", fz, H * W)):
        see(name, face)
        see(name + " nvalid == 16", full, face)
        see(name + " own load 16 B", (vol_off + v0) % 16 == 0, face & full)
        see(name + " neighbour load 16 B", (vol_off + v0 - back) % 16 == 0, face & full)
    see("fx", fx)
    see("fz ly > 0", ly > 0, fz)
    see("fx ly > 0", ly > 0, fx)
    see("seam thread", fz | fy | fx)
    return took


def filter_branches(vol, ncls, vol_off, out_off, lab_off):
    """The same for cc_filter_kernel and its launch: vec_ok, the vector body against the tail, the early-out, and the ids on
    either side of ncls that each path meets.  out_off None: in place."""
    flat = np.asarray(vol).ravel()
    N = flat.size
    vec_ok = vol_off % 4 == 0 and (vol_off if out_off is None else out_off) % 4 == 0 and lab_off % 16 == 0
    took = {("vec_ok", vec_ok)}
    for v0 in range(0, N, CF_VOX):
        body = vec_ok and v0 + CF_VOX <= N
        if vec_ok:
            took.add(("v0 + 4 <= N", body))
        w = flat[v0:v0 + CF_VOX]
        if body:
            took.add(("w == 0", not w.any()))
        took.update((("vector" if body else "scalar") + " id < ncls", bool(i < ncls)) for i in w if i)
    return took


BOTH = (False, True)


class StubNet:
    """A `net` for predict_volume that ignores the image's values: slice k of the volume gets the one-hot logits of
    class_map[k] (D, H, W), handed out in call order.  No model, no parameters."""

    def __init__(self, class_map, ncls):
        import torch
        self.onehot = torch.nn.functional.one_hot(torch.from_numpy(np.asarray(class_map, np.int64)), ncls).permute(0, 3, 1, 2).float()
        self.pos = 0

    def eval(self):
        self.pos = 0
        return self

    def __call__(self, x):
        out = self.onehot[self.pos:self.pos + x.shape[0]].to(x.device).contiguous()
        self.pos += x.shape[0]
        return out
