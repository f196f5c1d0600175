"""ops.class_counts / cswin_class_counts (csrc/label_stats.hip): the per-slice class histogram, compared with torch.equal against
torch.bincount per slice on the CPU, plus the identity that every row sums to the slice's element count (nothing is dropped: what
has no class is tallied in the last column).

The kernel has two ways to count a wave's labels of one step: one addition when they are all the same value, per-lane LDS atomics
otherwise.  Constant slices take the first alone (but for the few elements before the first and after the last 16-byte vector),
per-element random ids the second alone, seeded blobs both.  Shapes: fewer elements than one load per lane (3 x 7 x 5), several
trips of the loop, a 512 x 512 slice, and slices of 33 x 31 elements in a view that starts one element into its buffer, so that
every slice base is misaligned.  Every device call is followed by a synchronize."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from seg_metrics_cases import blob_pair

pytestmark = pytest.mark.gpu
DEV = "cuda"
ERR_SHAPE, ERR_ALIGN, ERR_UNSUPPORTED = -1, -2, -5       # include/cswin_hip.h

# (shape, dtype, view starts one element into its buffer)
CASES = [((3, 7, 5), "uint8", False), ((3, 7, 5), "int64", False), ((2, 64, 48), "uint8", False), ((2, 64, 48), "int64", False),
         ((1, 512, 512), "uint8", False), ((5, 33, 31), "uint8", True), ((5, 33, 31), "int64", True)]
CONTENTS = ["constant", "random", "blobs"]
NCLS = [1, 9, 256]


@functools.lru_cache(maxsize=None)
def raw_labels(shape, content):
    """uint8 (N, H, W), read-only and shared.  constant: slice n holds one id, 200 (out of range for ncls <= 9) among them."""
    N = shape[0]
    rng = np.random.default_rng(1000 * shape[1] + shape[2] + len(content))
    if content == "constant":
        ids = np.array([200, 0, 3, 255, 8])[:N]
        a = np.broadcast_to(ids[:, None, None], shape).astype(np.uint8)
    elif content == "random":
        a = rng.integers(0, 256, shape).astype(np.uint8)
        a[rng.random(shape) < 0.5] %= 12                # half of them small: ncls = 9 sees every class and some ids beyond
    else:
        a = blob_pair(shape, [1, 2, 3, 4, 5, 6, 7, 8], 77 + shape[2])[1]
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def reference(raw, ncls, table=None):
    """int64 (N, ncls + 1) by torch.bincount per slice on the CPU; raw: integer numpy (N, H, W), table: numpy or None."""
    cls = torch.from_numpy(np.asarray(raw).astype(np.int64))
    if table is not None:
        t = torch.from_numpy(np.asarray(table).astype(np.int64))
        inside = (cls >= 0) & (cls < len(t))
        cls = torch.where(inside, t[cls.clamp(0, len(t) - 1)], torch.full_like(cls, -1))
    cls = torch.where((cls >= 0) & (cls < ncls), cls, torch.full_like(cls, ncls))
    return torch.stack([torch.bincount(s.reshape(-1), minlength=ncls + 1) for s in cls])


def on_device(raw, dtype, offset):
    """The labels as a HIP tensor of `dtype`; offset: a view that starts one element into a larger buffer."""
    t = torch.from_numpy(np.asarray(raw).astype(dtype))
    if not offset:
        return t.to(DEV)
    buf = torch.zeros(t.numel() + 16, dtype=t.dtype, device=DEV)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == t.element_size() and v.is_contiguous()
    return v


def counts_of(labels, ncls, label_map=None):
    from cswin_unet_amd import ops
    got = ops.class_counts(labels, ncls, label_map)
    torch.cuda.synchronize()
    N = labels.shape[0] if labels.dim() == 3 else 1
    assert got.dtype == torch.int64 and got.is_cuda and tuple(got.shape) == (N, ncls + 1)
    return got.cpu()


@pytest.mark.parametrize("ncls", NCLS)
@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("shape,dtype,offset", CASES, ids=lambda v: v if isinstance(v, str) else str(v) if isinstance(v, bool) else "x".join(map(str, v)))
def test_class_counts_equal_bincount(shape, dtype, offset, content, ncls):
    raw = raw_labels(shape, content)
    got = counts_of(on_device(raw, dtype, offset), ncls)
    want = reference(raw, ncls)
    assert torch.equal(got, want), (got - want).abs().sum(1).tolist()
    assert (got.sum(1) == shape[1] * shape[2]).all()
    if content == "constant":
        assert ((got != 0).sum(1) == 1).all()
        if ncls <= 9:
            assert int(got[0, ncls]) == shape[1] * shape[2]          # the slice of id 200 has no class
    if content == "blobs" and ncls == 9 and shape[1] >= 64:
        assert ((got[:, :9] != 0).sum(1) >= 3).all()


def test_both_paths_are_what_the_contents_exercise():
    """CPU check of the inputs: in a constant slice every aligned 16-byte vector is one value; in the random ones almost none is;
    the blobs have both kinds inside the vectors one wave loads in a step (64 x 16 elements)."""
    for shape in ((2, 64, 48), (1, 512, 512)):
        for content, lo, hi in (("constant", 1.0, 1.0), ("random", 0.0, 0.001), ("blobs", 0.3, 0.999)):
            v = raw_labels(shape, content).reshape(shape[0], -1, 16)
            uniform = (v == v[..., :1]).all(-1)
            assert lo <= uniform.mean() <= hi, (shape, content, uniform.mean())
    steps = raw_labels((1, 512, 512), "blobs").reshape(-1, 1024)
    whole = (steps == steps[:, :1]).all(-1)
    assert whole.any() and not whole.all()


@pytest.mark.parametrize("dtype", ["uint8", "int64"])
def test_label_map_and_ids_without_a_class(dtype):
    from cswin_unet_amd.continual import new_label_map
    shape = (4, 64, 48)
    raw = blob_pair(shape, [1, 2, 3], 5)[1].astype(np.int64)
    rng = np.random.default_rng(9)
    stray = [4, 7, 255] if dtype == "uint8" else [4, 7, 255, 257, -1, -2 ** 40, 2 ** 32, 2 ** 32 + 3, 2 ** 63 - 1]
    where = rng.random(shape) < 0.05
    raw[where] = rng.choice(stray, int(where.sum()))
    raw[3] = stray[-1]                                            # a whole slice without a class
    table = new_label_map(9, 4)
    assert table.tolist() == [0, 9, 10, 11]
    got = counts_of(on_device(raw, dtype, False), 12, table.to(DEV))
    want = reference(raw, 12, table.numpy())
    assert torch.equal(got, want)
    assert (got.sum(1) == shape[1] * shape[2]).all()
    assert int(got[:, 12].sum()) == int(where.sum() + (~where[3]).sum()) and not got[:, 1:9].any() and (got[:, [9, 10, 11]].sum(0) > 0).all()
    # without the map the same ids are their own class; ids >= 2^32 and 257 must not alias classes 0, 3 and 1
    got_raw = counts_of(on_device(raw, dtype, False), 4)
    assert torch.equal(got_raw, reference(raw, 4))
    # a map may send an id outside [0, ncls) or below zero: no class
    odd = torch.tensor([0, 9, -4, 11, 2], dtype=torch.int32)
    got_odd = counts_of(on_device(raw, dtype, False), 10, odd.to(DEV))
    assert torch.equal(got_odd, reference(raw, 10, odd.numpy()))
    assert (got_odd.sum(1) == shape[1] * shape[2]).all()


def test_two_runs_give_the_same_counts_and_a_2d_slice_is_one_row():
    raw = raw_labels((1, 512, 512), "blobs")
    d = on_device(raw, "uint8", False)
    a, b = counts_of(d, 9), counts_of(d, 9)
    assert torch.equal(a, b)
    one = counts_of(d[0], 9)
    assert tuple(one.shape) == (1, 10) and torch.equal(one, a)


def test_wrapper_refusals():
    from cswin_unet_amd import ops
    from cswin_unet_amd._lib import CswinHipError
    lab = torch.zeros(2, 8, 8, dtype=torch.uint8, device=DEV)
    for bad in (lab.int(), lab.float(), lab.to(torch.int16)):
        with pytest.raises(CswinHipError, match="dtype"):
            ops.class_counts(bad, 9)
    with pytest.raises(CswinHipError):
        ops.class_counts(lab[0, 0], 9)
    with pytest.raises(CswinHipError):
        ops.class_counts(lab, 9, label_map=torch.zeros(4, dtype=torch.int64, device=DEV))
    with pytest.raises(CswinHipError):
        ops.class_counts(lab, 9, label_map=torch.zeros(4, dtype=torch.int32))
    for ncls in (0, 257):
        with pytest.raises(CswinHipError, match="ncls"):
            ops.class_counts(lab, ncls)


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

    def written(self):
        return not bool((self.t == self.sentinel).any())


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


def test_direct_call_writes_every_count_and_nothing_else():
    from cswin_unet_amd._lib import call, ptr, stream
    for ncls in (1, 9, 256):
        raw = raw_labels((5, 33, 31), "blobs")
        d = on_device(raw, "uint8", True)
        o = GuardedInt((5, ncls + 1), torch.int64)
        call("cswin_class_counts", ptr(d), 1, None, 0, at(o.addr), 5, 33 * 31, ncls, stream())
        torch.cuda.synchronize()
        assert o.intact() and o.written()
        assert torch.equal(o.t.cpu(), reference(raw, ncls))


def test_entry_point_refusals_touch_nothing():
    from cswin_unet_amd._lib import ptr, stream
    N, E, ncls = 3, 40, 9
    lab = torch.zeros(N * E + 2, dtype=torch.int64, device=DEV)
    table = torch.zeros(8, dtype=torch.int32, device=DEV)
    o = dict(counts=GuardedInt((N, 258), torch.int64))

    def args(**kw):
        a = dict(labels=ptr(lab), label_bytes=8, label_map=None, nmap=0, counts=at(o["counts"].addr), N=N, slice_elems=E, ncls=ncls)
        a.update(kw)
        return tuple(a.values()) + (stream(),)
    name = "cswin_class_counts"
    refused(ERR_SHAPE, "ncls 0", o, name, *args(ncls=0))
    refused(ERR_SHAPE, "ncls 257", o, name, *args(ncls=257))
    refused(ERR_UNSUPPORTED, "label_bytes 4", o, name, *args(label_bytes=4))
    refused(ERR_UNSUPPORTED, "label_bytes 0", o, name, *args(label_bytes=0))
    refused(ERR_SHAPE, "slice_elems 0", o, name, *args(slice_elems=0))
    refused(ERR_SHAPE, "slice_elems 2^31", o, name, *args(slice_elems=2 ** 31))
    refused(ERR_SHAPE, "N 0", o, name, *args(N=0))
    refused(ERR_SHAPE, "labels NULL", o, name, *args(labels=None))
    refused(ERR_SHAPE, "counts NULL", {}, name, *args(counts=None))
    refused(ERR_SHAPE, "a map of no entries", o, name, *args(label_map=ptr(table), nmap=0))
    refused(ERR_SHAPE, "entries of no map", o, name, *args(nmap=4))
    refused(ERR_ALIGN, "int64 labels 4 bytes off", o, name, *args(labels=at(lab.data_ptr() + 4)))
    refused(ERR_ALIGN, "counts 4 bytes off", o, name, *args(counts=at(o["counts"].addr + 4)))
    refused(ERR_ALIGN, "map 2 bytes off", o, name, *args(label_map=at(table.data_ptr() + 2), nmap=4))
