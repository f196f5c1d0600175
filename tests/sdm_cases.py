"""Case table and label builders of the signed distance maps (csrc/sdm.hip) and of the boundary loss's tests: what
tests/test_sdm_host.py checks on the CPU and tests/test_gpu_sdm.py / test_gpu_boundary_loss.py run on the device.  Everything
here is deterministic, computed once and never written."""
import functools

import numpy as np

SDM_MAX_DIM = 2047                                       # csrc/sdm_plan.h
TX_STEPS = (128, 256)                                    # sdm_tx: 64 columns up to 128 rows, 32 up to 256, 16 above (16 KiB of LDS)
OOR = (-1, "ncls", 2 ** 32 + 1)                          # labels that are no class; 2^32 + 1 is class 1 to a kernel that truncates

HOST_SHAPES = ((1, 1), (1, 9), (9, 1), (7, 13), (16, 16))
HOST_KINDS = ("random", "absent", "full", "one_pixel", "oor")


def tx_of(H):
    return 64 if H <= 128 else (32 if H <= 256 else 16)


def random_labels(B, H, W, ncls, seed):
    return np.random.default_rng(seed).integers(0, ncls, size=(B, H, W)).astype(np.int64)


def coarse_labels(B, H, W, ncls, seed, cell=5):
    """Random labels in cells of `cell` pixels: regions a few pixels deep, so that inside distances pass 1."""
    rng = np.random.default_rng(seed)
    ch, cw = min(cell, H), min(cell, W)
    small = rng.integers(0, ncls, size=(B, -(-H // ch), -(-W // cw)))
    return np.kron(small, np.ones((ch, cw), np.int64))[:, :H, :W].astype(np.int64)


def blob_labels(B, H, W, ncls, seed):
    """Disc-and-rectangle "organs" on background 0: class c is a disc (odd c) or a rectangle (even c) of a random place and size,
    later classes drawn over earlier ones; samples differ."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:H, :W]
    lab = np.zeros((B, H, W), np.int64)
    for b in range(B):
        for c in range(1, ncls):
            cy, cx = rng.integers(0, H), rng.integers(0, W)
            ry, rx = rng.integers(1, max(2, H // 3)), rng.integers(1, max(2, W // 3))
            if c % 2:
                m = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
            else:
                m = (abs(yy - cy) <= ry) & (abs(xx - cx) <= rx)
            lab[b][m] = c
    return lab


def far_labels(B, H, W, ncls=None):
    """Background everywhere but one pixel of class 1 in a corner (another corner per sample): the farthest a distance gets,
    and the bounded column walk's worst case."""
    lab = np.zeros((B, H, W), np.int64)
    corners = ((0, 0), (H - 1, W - 1), (0, W - 1), (H - 1, 0))
    for b in range(B):
        lab[(b,) + corners[b % 4]] = 1
    return lab


def absent_full_labels(B, H, W, ncls, seed):
    """Sample 0: random labels in which class ncls - 1 never occurs; every other sample: that class alone."""
    lab = np.full((B, H, W), ncls - 1, np.int64)
    lab[0] = random_labels(1, H, W, ncls - 1, seed)[0]
    return lab


def with_oor(lab, ncls):
    """A copy with pixels of every out-of-range kind, spread over the samples (as many as the slice has room for)."""
    lab = np.array(lab)
    flat = lab.reshape(lab.shape[0], -1)
    n = flat.shape[1]
    for k, bad in enumerate(OOR):
        flat[k % lab.shape[0], (7 * k + 3) % n] = ncls if bad == "ncls" else bad
        flat[(k + 1) % lab.shape[0], (n - 1 - 5 * k) % n] = ncls if bad == "ncls" else bad
    return lab


def host_labels(kind, H, W, ncls=4, B=2):
    seed = 1000 + 17 * H + W
    if kind == "random":
        return random_labels(B, H, W, ncls, seed)
    if kind == "absent":
        return absent_full_labels(B, H, W, ncls, seed)[:1].repeat(B, 0)
    if kind == "full":
        return absent_full_labels(B, H, W, ncls, seed)
    if kind == "one_pixel":
        lab = random_labels(B, H, W, ncls - 1, seed)
        lab[0, H // 2, W // 2] = ncls - 1
        lab[1, H - 1, 0] = ncls - 1
        return lab
    assert kind == "oor"
    return with_oor(random_labels(B, H, W, ncls, seed), ncls)


def brute_d2(mask):
    """Squared distance of every pixel of a 2-D slice to the nearest pixel of `mask` (which has one), by the all-pairs minimum in
    integers."""
    ys, xs = np.nonzero(mask)
    yy, xx = np.mgrid[:mask.shape[0], :mask.shape[1]]
    d2 = (yy[..., None] - ys) ** 2 + (xx[..., None] - xs) ** 2
    return d2.min(-1)


def brute_maps(lab, ncls):
    """The definition, from the all-pairs minimum: +sqrt(d2 to the mask) outside, -(sqrt(d2 to the outside) - 1) inside, zeros for
    an empty or a full mask; the root and the difference in float64, then one rounding."""
    lab = np.asarray(lab)
    phi = np.zeros((lab.shape[0], ncls) + lab.shape[1:], np.float32)
    for b in range(lab.shape[0]):
        for c in range(ncls):
            m = lab[b] == c
            if not m.any() or m.all():
                continue
            out = np.sqrt(brute_d2(m).astype(np.float64))
            ins = np.sqrt(brute_d2(~m).astype(np.float64))
            phi[b, c] = np.where(m, -(ins - 1.0), out)
    return phi


# ---- device cases: (id, B, ncls, H, W, label kind) ----------------------------------------------------------------------------
GPU_CASES = [
    ("1x1", 1, 2, 1, 1, "random"),
    ("row70", 2, 3, 1, 70, "coarse"),                    # one row: the column pass has nothing to walk; two row chunks
    ("col70", 2, 3, 70, 1, "coarse"),                    # one column: every row is uniform, g1 is all NONE
    ("7x13", 3, 9, 7, 13, "random"),
    ("63x64", 2, 4, 63, 64, "coarse"),                   # a full row chunk, one full column tile
    ("64x65", 2, 4, 64, 65, "coarse"),                   # one pixel into the second chunk and tile
    ("65x129", 1, 5, 65, 129, "coarse"),                 # three chunks, three tiles, the last of one column
    ("h128", 1, 2, 128, 70, "coarse"),                   # TX = 64, its tallest slice; a second tile of 6 columns
    ("h129", 1, 2, 129, 70, "coarse"),                   # TX = 32: three tiles
    ("h256", 1, 2, 256, 70, "coarse"),
    ("h257", 1, 2, 257, 70, "coarse"),                   # TX = 16: five tiles
    ("h1025", 1, 2, 1025, 3, "coarse"),                  # a tall slice of coarse labels: walks that stop early
    ("h2047", 1, 2, 2047, 3, "far"),                     # the tallest slice, walked end to end
    ("w2047", 1, 2, 3, 2047, "far"),                     # the widest: 32 row chunks
    ("organs224", 2, 9, 224, 224, "blobs"),
    ("far224", 2, 9, 224, 224, "far"),                   # distances up to 223 sqrt 2 = 315.4
    ("absentfull224", 2, 9, 224, 224, "absent_full"),
    ("nc2", 2, 2, 7, 13, "random"),
    ("nc16", 2, 16, 7, 13, "random"),
    ("nc255", 2, 255, 7, 13, "random"),
    ("oor", 2, 4, 7, 13, "oor"),
    ("oor65x129", 1, 5, 65, 129, "oor_coarse"),
]


@functools.lru_cache(maxsize=None)
def gpu_labels(tag):
    _, B, ncls, H, W, kind = next(c for c in GPU_CASES if c[0] == tag)
    seed = 7000 + sum(map(ord, tag))
    lab = {"random": lambda: random_labels(B, H, W, ncls, seed), "coarse": lambda: coarse_labels(B, H, W, ncls, seed),
           "blobs": lambda: blob_labels(B, H, W, ncls, seed), "far": lambda: far_labels(B, H, W),
           "absent_full": lambda: absent_full_labels(B, H, W, ncls, seed),
           "oor": lambda: with_oor(random_labels(B, H, W, ncls, seed), ncls),
           "oor_coarse": lambda: with_oor(coarse_labels(B, H, W, ncls, seed), ncls)}[kind]()
    lab.setflags(write=False)
    return lab


@functools.lru_cache(maxsize=None)
def gpu_reference(tag):
    """utils.signed_distance_maps_host of the case's labels, computed once."""
    from cswin_unet_amd.utils import signed_distance_maps_host
    ncls = next(c for c in GPU_CASES if c[0] == tag)[2]
    phi = signed_distance_maps_host(gpu_labels(tag), ncls)
    phi.setflags(write=False)
    return phi
