"""ops.argmax_zoom_back(logits, size, classes=...) / cswin_argmax_zoom_back_classes (csrc/resize.hip): the argmax over a list of
output channels, as a continual model is scored on one dataset's own classes, followed by scipy's order-0 zoom.  Every comparison
is exact, against scipy.ndimage.zoom(torch.argmax(logits[:, classes], 1), order=0) computed on the CPU.  Logits are multiples of
0.25, so ties inside the chosen channels are frequent (asserted).  Every device call is followed by a synchronize so that a
failing step ends its test before anything else is enqueued.

The direct calls of the C entry point use the guarded buffers of tests/test_gpu_eval_kernels.py (its helpers are copied here): a
refused call writes nothing at all, and a table with entries outside [0, ncls) is clamped on the device."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch
from scipy.ndimage import zoom

pytestmark = pytest.mark.gpu
DEV = "cuda"
ERR_SHAPE, ERR_ALIGN = -1, -2                             # include/cswin_hip.h
NCLS = 14

# (h, w) -> (H, W): up, down, identity, both strided loops more than once, and the pair whose last row and column scipy fills
# with its constant 0 instead of gathering
SHAPES = [((40, 56), (64, 48)), ((32, 40), (20, 24)), ((40, 56), (40, 56)), ((8, 300), (8, 300)), ((512, 512), (224, 224))]
CLASS_LISTS = {"kits23": [0, 9, 10, 11], "lits17": [0, 12, 13], "all": list(range(NCLS)), "single": [5], "unordered": [11, 0, 9],
               "repeat": [3, 3, 7]}


@functools.lru_cache(maxsize=None)
def logits_of(hw, ncls=NCLS, nan=False):
    """(B, ncls, h, w) float32 multiples of 0.25 (B = 1 at 512 x 512); read-only, shared by the tests."""
    h, w = hw
    B = 1 if h * w >= 2 ** 18 else 2
    rng = np.random.default_rng(ncls * 7919 + h * 31 + w + 17 * nan)
    x = (np.round(rng.standard_normal((B, ncls, h, w)) * 4) / 4).astype(np.float32)
    if nan:
        x[rng.random(x.shape) < 0.02] = np.nan
    x.setflags(write=False)
    return x


def reference(logits, classes, HW):
    """scipy's order-0 zoom of torch.argmax over the listed channels, on the CPU."""
    B, _, h, w = logits.shape
    am = torch.argmax(torch.from_numpy(np.array(logits))[:, list(classes)], 1).numpy()
    return np.stack([zoom(am[b], (HW[0] / h, HW[1] / w), order=0) for b in range(B)]).astype(np.uint8)


def tie_rate(logits, classes):
    sel = logits[:, list(classes)]
    with np.errstate(invalid="ignore"):
        return float(((sel == np.nanmax(sel, axis=1, keepdims=True)).sum(axis=1) > 1).mean())


def run(logits, classes, HW):
    from cswin_unet_amd import ops
    got = ops.argmax_zoom_back(torch.from_numpy(np.array(logits)).to(DEV), HW, classes=classes)
    torch.cuda.synchronize()
    assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == (logits.shape[0],) + tuple(HW)
    return got


@pytest.mark.parametrize("name", list(CLASS_LISTS))
@pytest.mark.parametrize("hw,HW", SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_subset_argmax_equals_torch_argmax_of_the_slice_and_scipy_order0(hw, HW, name):
    from cswin_unet_amd import ops
    classes, logits = CLASS_LISTS[name], logits_of(hw)
    if len(classes) > 1:
        assert tie_rate(logits, classes) > 0.02
    got = run(logits, classes, HW)
    want = reference(logits, classes, HW)
    bad = np.argwhere(got.cpu().numpy() != want)
    assert len(bad) == 0, (len(bad), [tuple(k) for k in bad[:8]])
    assert int(want.max()) < len(classes)
    if name == "single":
        assert not got.any()
    if name == "unordered":
        assert len(np.unique(want)) == 3                 # positions, not channel numbers
    if name == "repeat":
        assert not (want == 1).any() and (want == 2).any()          # the later position of a repeated class never wins
    if name == "all":
        plain = ops.argmax_zoom_back(torch.from_numpy(np.array(logits)).to(DEV), HW)
        torch.cuda.synchronize()
        assert torch.equal(got, plain)
    if HW == (224, 224):
        assert not want[:, -1, :].any() and not want[:, :, -1].any() and (name == "single" or want[:, :-1, :-1].any())


def test_subset_argmax_with_255_of_300_classes_in_descending_order():
    hw, HW, ncls = (40, 56), (64, 48), 300
    classes = list(range(299, 44, -1))
    assert len(classes) == 255
    logits = logits_of(hw, ncls)
    assert tie_rate(logits, classes) > 0.02
    got = run(logits, classes, HW).cpu().numpy()
    want = reference(logits, classes, HW)
    assert np.array_equal(got, want)
    assert want.max() > 200


def test_subset_argmax_a_nan_beats_every_number_and_the_first_nan_wins():
    hw, HW = (40, 56), (64, 48)
    logits = logits_of(hw, NCLS, True)
    for classes in (CLASS_LISTS["kits23"], CLASS_LISTS["unordered"], CLASS_LISTS["all"]):
        sel = logits[:, classes]
        assert np.isnan(sel).any(axis=1).mean() > 0.04 and (np.isnan(sel).sum(axis=1) > 1).any()
        assert np.array_equal(run(logits, classes, HW).cpu().numpy(), reference(logits, classes, HW)), classes


def test_wrapper_validates_the_class_list_on_the_host():
    from cswin_unet_amd import ops
    from cswin_unet_amd._lib import CswinHipError
    x = torch.zeros(1, NCLS, 4, 4, device=DEV)
    with pytest.raises(CswinHipError, match="entries"):
        ops.argmax_zoom_back(x, (8, 8), classes=[])
    with pytest.raises(CswinHipError, match="entries"):
        ops.argmax_zoom_back(x, (8, 8), classes=[0] * 256)
    with pytest.raises(CswinHipError, match=r"classes\[2\] = 14"):
        ops.argmax_zoom_back(x, (8, 8), classes=[0, 9, 14])
    with pytest.raises(CswinHipError, match=r"classes\[1\] = -1"):
        ops.argmax_zoom_back(x, (8, 8), classes=[0, -1])
    with pytest.raises(CswinHipError, match=r"classes\[0\]"):
        ops.argmax_zoom_back(x, (8, 8), classes=[1.5, 2])
    a = ops.argmax_zoom_back(x, (8, 8), classes=(0, 9))
    b = ops.argmax_zoom_back(x, (8, 8), classes=[0, 9])
    torch.cuda.synchronize()
    assert len([k for k in ops._class_tables if k[0] == (0, 9)]) == 1          # one upload per (list, device)
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------
# the entry point, called directly with guarded buffers (helpers of tests/test_gpu_eval_kernels.py)
# ------------------------------------------------------------------------------------------------
GUARD_BYTES = 256
PATTERN = 0xA5


class GuardedInt:
    """A byte buffer filled with 0xA5 with GUARD_BYTES before and after the view `.t`.  An element that still holds the pattern
    counts as never written unless the reference holds that very value."""

    def __init__(self, shape, dtype):
        self.item = torch.empty((), dtype=dtype).element_size()
        self.nbytes = math.prod(shape) * self.item
        self.lo = GUARD_BYTES
        self.buf = torch.full((self.nbytes + 2 * GUARD_BYTES + 16,), PATTERN, dtype=torch.uint8, device=DEV)
        assert self.buf.data_ptr() % 16 == 0
        self.raw = self.buf[self.lo:self.lo + self.nbytes]
        self.addr = self.raw.data_ptr()
        self.t = self.raw.view(dtype).view(shape)
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


def put(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def at(addr):
    return ctypes.c_void_p(addr)


def refused(code, what, bufs, name, *args):
    from cswin_unet_amd import _lib
    got = getattr(_lib.lib(), name)(*args)
    msg = _lib.lib().cswin_last_error().decode()
    assert got == code, f"{what}: {name} returned {got} ({msg!r}), expected {code}"
    assert msg.startswith(name[len("cswin_"):]), f"{what}: message {msg!r}"
    torch.cuda.synchronize()
    for n, g in bufs.items():
        assert g.untouched(), f"refused {what}: {n} was written"


def test_entry_point_refusals_touch_nothing():
    from cswin_unet_amd._lib import ptr, stream
    B, ncls, h, w, H, W = 2, 5, 4, 5, 6, 7
    ld, rd, cd = put(np.zeros((B, ncls, h, w), np.float32)), put(np.zeros(H, np.int32)), put(np.zeros(W, np.int32))
    td = put(np.zeros(260, np.int32))
    o = dict(out=GuardedInt((B, H, W), torch.uint8))

    def args(**kw):
        a = dict(logits=ptr(ld), out=at(o["out"].addr), rows=ptr(rd), cols=ptr(cd), classes=ptr(td), nsel=3, B=B, ncls=ncls, h=h, w=w,
                 H=H, W=W)
        a.update(kw)
        return tuple(a.values()) + (stream(),)
    name = "cswin_argmax_zoom_back_classes"
    refused(ERR_SHAPE, "nsel 0", o, name, *args(nsel=0))
    refused(ERR_SHAPE, "nsel 256", o, name, *args(nsel=256))
    refused(ERR_SHAPE, "ncls 0", o, name, *args(ncls=0))
    refused(ERR_SHAPE, "classes NULL", o, name, *args(classes=None))
    refused(ERR_SHAPE, "logits NULL", o, name, *args(logits=None))
    refused(ERR_ALIGN, "classes 2 bytes off", o, name, *args(classes=at(td.data_ptr() + 2)))
    refused(ERR_ALIGN, "rows 2 bytes off", o, name, *args(rows=at(rd.data_ptr() + 2)))
    for dim in ("B", "h", "w", "H", "W"):
        refused(ERR_SHAPE, f"{dim} = 2049", o, name, *args(**{dim: 2049}))
        refused(ERR_SHAPE, f"{dim} = 0", o, name, *args(**{dim: 0}))


def test_a_table_with_entries_outside_the_classes_is_clamped_on_the_device():
    """Entries -3 and ncls + 5 read channels 0 and ncls - 1.  The logits sit between planes of 1e30 (three before, six after, one
    batch): a read that was not clamped would stay inside the allocation, find 1e30 and win at its position."""
    from cswin_unet_amd._lib import call, ptr, stream
    ncls, h, w, H, W = 6, 12, 20, 12, 20
    x = logits_of((h, w), ncls)[:1]
    buf = torch.full((3 + ncls + 6, h, w), 1e30, dtype=torch.float32, device=DEV)
    buf[3:3 + ncls] = torch.from_numpy(np.array(x[0])).to(DEV)
    logits = buf[3:3 + ncls]
    rows, cols = put(np.arange(H, dtype=np.int32)), put(np.arange(W, dtype=np.int32))
    res = {}
    for tag, table in (("bad", [-3, 2, ncls + 5, 4]), ("clamped", [0, 2, ncls - 1, 4])):
        td = put(np.array(table, np.int32))
        o = dict(out=GuardedInt((1, H, W), torch.uint8))
        call("cswin_argmax_zoom_back_classes", ptr(logits), at(o["out"].addr), ptr(rows), ptr(cols), ptr(td), len(table), 1, ncls, h, w,
             H, W, stream())
        torch.cuda.synchronize()
        assert o["out"].intact()
        res[tag] = o["out"].t.cpu().numpy()
    want = reference(x, [0, 2, ncls - 1, 4], (H, W))
    assert o["out"].written(want)
    assert np.array_equal(res["clamped"], want)
    assert np.array_equal(res["bad"], want)
    assert len(np.unique(want)) == 4
