"""Cases and references shared by the test-time-augmentation tests (tests/test_tta_host.py, tests/test_tta_plan_host.py,
tests/test_gpu_tta.py).  Everything here is numpy on the host: the views as the numpy expressions of the views' definition, the
float64 ensemble written from its definition (not through cswin_unet_amd.utils), and the seeded inputs.  References are cached
and returned read-only."""
import functools

import numpy as np
import torch
from scipy.ndimage import zoom

from oracle.determ import det_normal

CODES = tuple(range(8))
STRAIGHT = (0, 2, 4, 6)
NAMES = {"identity": 0, "transpose": 1, "flip_rows": 2, "flip_cols": 4, "rot90": 3, "rot180": 6, "rot270": 5, "anti_transpose": 7}
GAP = 1e-5                      # a reference top-two gap at or below it excuses a pixel's class
EXCUSED = 1e-3                  # at most this share of pixels may be excused


def view_np(x, c):
    """View c of the last two axes, as the definition writes it."""
    a = np.swapaxes(x, -1, -2) if c & 1 else x
    a = a[..., ::-1, :] if c & 2 else a
    return a[..., :, ::-1] if c & 4 else a


def inverse_code(c):
    """The code of the inverse view: the flips are their own inverses; under a transpose the two flips change places."""
    return c if not c & 1 else 1 | (2 if c & 4 else 0) | (4 if c & 2 else 0)


def back_np(a, c):
    """From view c's frame back to the source frame: a[..., i_c(r, s), j_c(r, s)] at (r, s)."""
    return view_np(a, inverse_code(c))


def ensemble_np(logits, views, classes=None):
    """P (B, nsel, h, w) float64 of logits (V, B, ncls, h', w'): the mean over the views of the float64 softmax over the listed
    channels, each in the source frame."""
    L = np.asarray(logits, np.float64)
    L = L if classes is None else L[:, :, list(classes)]
    P = 0.0
    with np.errstate(invalid="ignore", over="ignore"):
        for v, c in enumerate(views):
            e = np.exp(L[v] - L[v].max(axis=1, keepdims=True))
            P = P + back_np(e / e.sum(axis=1, keepdims=True), c)
        return np.ascontiguousarray(P / len(views))


def classes_of(P):
    """torch.argmax over the candidates: the first index wins, a NaN wins and the first NaN first."""
    return torch.argmax(torch.from_numpy(np.ascontiguousarray(P)), dim=1).numpy()


def top_two_gap(P):
    """Per pixel, the largest probability minus the second largest (NaN where a probability is NaN)."""
    if P.shape[1] == 1:
        return np.ones(P.shape[:1] + P.shape[2:])
    top = np.sort(P, axis=1)[:, -2:]
    return top[:, 1] - top[:, 0]


def zoom_back(cls, size):
    h, w = cls.shape[1:]
    if (h, w) == tuple(size):
        return cls.copy()
    return np.stack([zoom(c, (size[0] / h, size[1] / w), order=0) for c in cls])


# ---- view_batch: (B, h, w), the codes tried ----------------------------------------------------------------------------------
VIEW_SHAPES = [((1, 1, 1), CODES), ((3, 33, 33), CODES), ((2, 64, 64), CODES), ((2, 17, 40), STRAIGHT), ((1, 224, 224), CODES)]


# ---- geometry: votes ---------------------------------------------------------------------------------------------------------
VOTE, VOTE_NCLS = 20.0, 9


def fixed_class(B, h, w):
    b, r, s = np.meshgrid(np.arange(B), np.arange(h), np.arange(w), indexing="ij")
    return (3 * r + s + 5 * b + 1) % VOTE_NCLS


def vote_logits(views, B, h, w):
    """(V, B, 9, h', w') float32: 0 except, at view v's own image of source pixel (r, s), a vote of +20 for class
    (r + 2 s + v) % 9 and one for fixed_class(b, r, s).  The fixed class collects half of every view's probability (all of it
    where the two votes meet), any other class at most half of one view's (the eight v give eight different classes mod 9), so
    from two views on the fixed class wins with a gap of at least (1/2)(1 - 1/V); with one view the two tie exactly."""
    V = len(views)
    fixed = fixed_class(B, h, w)
    b, r, s = np.meshgrid(np.arange(B), np.arange(h), np.arange(w), indexing="ij")
    out = []
    for v, c in enumerate(views):
        src = np.zeros((B, VOTE_NCLS, h, w), np.float32)
        src[b, (r + 2 * s + v) % VOTE_NCLS, r, s] = VOTE
        src[b, fixed, r, s] = VOTE
        out.append(np.ascontiguousarray(view_np(src, c)))
    return np.stack(out) if len({o.shape for o in out}) == 1 else out


VOTE_VIEWS = [(c,) for c in CODES] + [STRAIGHT, CODES, (5, 0, 6)]
VOTE_SIZES = [((1, 1), None), ((33, 33), None), ((40, 40), None), ((17, 40), None), ((40, 40), (64, 48)), ((40, 40), (25, 30))]
VOTE_CLASSES = (4, 0, 8, 4, 2, 7, 1, 6, 0, 3, 5)          # every class, reordered, 4 and 0 twice


def vote_cases():
    """(views, (h, w), size or None, classes or None): every view list on every size it can have (a transposing view only on
    squares), and the reordering class list on the zoomed sizes."""
    out = []
    for views in VOTE_VIEWS:
        for hw, size in VOTE_SIZES:
            if hw[0] != hw[1] and any(c & 1 for c in views):
                continue
            out.append((views, hw, size, None))
            if size is not None and len(views) > 1:
                out.append((views, hw, size, VOTE_CLASSES))
    return out


# ---- probabilities and class maps on seeded normal logits ---------------------------------------------------------------------
# (tag, views, B, ncls, h = w, classes)
SUBSET14 = (0, 3, 4, 19, 6, 7, 8, 1, 10, 12, 13, 15, 16, 18)
PROB_CASES = [
    ("d4-9", CODES, 2, 9, 40, None),
    ("flips-16", STRAIGHT, 2, 16, 33, None),
    ("d4-17-general", CODES, 1, 17, 33, None),
    ("identity-9", (0,), 2, 9, 40, None),
    ("three-255", (3, 0, 6), 1, 255, 8, None),
    ("d4-14-of-20", CODES, 2, 20, 40, SUBSET14),
]


def prob_tolerance(nsel):
    """Absolute bound on a float32 ensemble probability against the float64 definition.  One view's probability carries at most
    about (nsel + 8) 2^-24 absolute error -- two expf roundings, nsel additions, a division, on values <= 1 -- and the mean over
    the views does not grow it: 1.5e-6 at nsel = 17, under 1e-5 by a factor of 6.  Past 17 candidates the same factor on the
    same expression."""
    return 1e-5 if nsel <= 17 else 6.0 * (nsel + 8) * 2.0 ** -24


@functools.lru_cache(maxsize=None)
def prob_case(tag):
    """(logits (V, B, ncls, h, w) float32, P float64, cls, gap) of a case, made once, read-only."""
    _, views, B, ncls, n, classes = next(c for c in PROB_CASES if c[0] == tag)
    logits = 3.0 * det_normal("tta.prob." + tag, (len(views), B, ncls, n, n))
    P = ensemble_np(logits, views, classes)
    res = (logits, P, classes_of(P), top_two_gap(P))
    for a in res:
        a.setflags(write=False)
    return res


def compare_classes(got, want, gap, tag):
    """got may differ from want only where gap <= GAP, and at most EXCUSED of the pixels lie there (the reference's own share is
    asserted first, so a bad input fails instead of hiding).  Returns the number of differing pixels."""
    near = gap <= GAP
    share = near.mean()
    differ = got != want
    print(f"{tag}: {int(near.sum())} of {near.size} pixels within {GAP} of a tie ({share:.2e}), {int(differ.sum())} differ")
    assert share <= EXCUSED, (tag, share)
    assert not (differ & ~near).any(), (tag, int((differ & ~near).sum()))
    return int(differ.sum())
