"""cswin_components_label and cswin_components_filter (csrc/components.hip) called directly, at every launch branch and under
contention.  tests/test_gpu_components.py goes through ops on volumes of at most 27 tiles whose irregular components have a few
hundred voxels; here

  contention  volumes of 512 and 729 tiles in which every class has a component that touches (nearly) every tile, wound round
              10^4 .. 10^5 small ones, a solid block and a serpentine of that size: the seam pass is the one launch of this
              project whose workgroups write memory that other workgroups of the same launch read, and only a load like this
              makes two of them meet in one union-find chain.  Labels and sizes must be those of scipy, and the same bits on a
              second run over the same buffers.
  branches    W on either side of the 16-voxel segment, of the 16-B load and of the int4 store; vol, labels and sizes off their
              vector alignment; sizes == NULL; dimensions of 2048; ids at and past ncls across a tile seam in x, y and z;
              ncls = 2 and ncls = 255; the filter's vector body, its tail, N < 4, its early-out, the scalar path, in place on
              either, thresholds past int32, equal to a size, and on either side of a float64 product that is not exact.
  refusals    what test_error_returns_before_any_launch lacks.

Only a direct call passes a pointer off its alignment or a workspace of exactly the size the library asks for.  Every output and the
workspace are views into buffers filled with the byte 0xA5 (GuardedInt of tests/test_gpu_eval_kernels.py): the bytes round a view
must survive a call, every element of the view must have been written, a refused call writes nothing.  Everything is an integer:
every comparison is torch.equal, no tolerance anywhere.  References: components_cases.canonical_labels (scipy.ndimage.label) and
components_cases.filter_ref, which tests/test_components_host.py holds against the two older filter references; that file also
asserts what the contention volumes are there for and that the case tables reach both sides of every branch.  Every device call
is followed by a synchronize so that a failing step ends its test before anything else is enqueued."""
import functools

import numpy as np
import pytest
import torch

import components_cases as C
from components_cases import canonical_labels, filter_ref, noise, rule_tables
from test_gpu_eval_kernels import ERR_ALIGN, ERR_SHAPE, ERR_UNSUPPORTED, GuardedInt, at, hip, put, settle_int  # noqa: F401

pytestmark = pytest.mark.gpu
TAB_BYTES = 256 * 4                  # the per-class table at the head of the workspace (CC_TAB ints)


def up16(n):
    return (n + 15) & ~15


def frozen(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays


@functools.lru_cache(maxsize=None)
def contention_ref(name):
    """(vol, labels, sizes) of a contention volume: built once, shared, read-only."""
    build, ncls = C.CONTENTION[name]
    vol = np.ascontiguousarray(build())
    return frozen(vol, *canonical_labels(vol, ncls))


# ---- cswin_components_label ---------------------------------------------------------------------------------------------------
def label_buffers(hip, shape, out_off=0, sizes=True):
    D, H, W = shape
    need = hip.lib().cswin_components_workspace(D, H, W)
    assert need == TAB_BYTES + 2 * up16(4 * D * H * W)
    o = dict(labels=GuardedInt(shape, torch.int32, out_off), workspace=GuardedInt((need,), torch.uint8))          # exactly `need` bytes
    if sizes:
        o["sizes"] = GuardedInt(shape, torch.int32, out_off)
    return o


def call_label(hip, vd, o, shape, ncls, what):
    D, H, W = shape
    hip.call("cswin_components_label", hip.ptr(vd), at(o["labels"].addr), at(o["sizes"].addr) if "sizes" in o else None,
             at(o["workspace"].addr), o["workspace"].nbytes, D, H, W, ncls, hip.stream())
    settle_int(what, o)
    return o["labels"].t.cpu(), (o["sizes"].t.cpu() if "sizes" in o else None)


def same(got, want, what):
    want = torch.from_numpy(np.array(want))
    bad = (got != want).nonzero()
    assert torch.equal(got, want), (what, bad.shape[0], [(k.tolist(), int(got[tuple(k)]), int(want[tuple(k)])) for k in bad[:8]])


def check_label(hip, vol, ncls, what, vol_off=0, out_off=0, ref=None):
    """One call on guarded buffers against canonical_labels, then one without sizes; returns the labels and sizes (CPU)."""
    vol = np.ascontiguousarray(vol)
    wl, ws = canonical_labels(vol, ncls) if ref is None else ref
    vd = put(vol.reshape(-1), vol_off)
    o = label_buffers(hip, vol.shape, out_off)
    assert vd.data_ptr() % 16 == vol_off and o["labels"].addr % 16 == out_off == o["sizes"].addr % 16 and o["workspace"].addr % 16 == 0
    labels, sizes = call_label(hip, vd, o, vol.shape, ncls, what)
    print(f"{what}: {int((ws > 0).sum())} components, largest {int(ws.max())}, {int((labels.numpy() != wl).sum())} label mismatches")
    same(labels, wl, what + " labels")
    same(sizes, ws, what + " sizes")
    assert int(sizes.sum()) == int((labels > 0).sum()) == int((vol != 0).sum() - (vol >= ncls).sum())
    bare = label_buffers(hip, vol.shape, out_off, sizes=False)
    only, _ = call_label(hip, vd, bare, vol.shape, ncls, what + " without sizes")
    assert torch.equal(only, labels), what + ": the call without sizes labels differently"
    return labels, sizes


@pytest.mark.parametrize("name", sorted(C.CONTENTION))
def test_contention_labels_equal_scipy_and_repeat_bit_for_bit(hip, name):
    vol, wl, ws = contention_ref(name)
    ncls = C.CONTENTION[name][1]
    vd = put(vol.reshape(-1))
    o = label_buffers(hip, vol.shape)
    labels, sizes = call_label(hip, vd, o, vol.shape, ncls, f"components.{name}")
    ncomp = int((ws > 0).sum())
    print(f"{name} {vol.shape}: {C.tiles_of(vol.shape)} tiles, {ncomp} components, largest {int(ws.max())}; "
          f"{int((labels.numpy() != wl).sum())} label and {int((sizes.numpy() != ws).sum())} size mismatches")
    same(labels, wl, name + " labels")
    same(sizes, ws, name + " sizes")
    assert int(sizes.sum()) == int((labels > 0).sum()) and int((sizes > 0).sum()) == ncomp
    again_l, again_s = call_label(hip, vd, o, vol.shape, ncls, f"components.{name} again")          # the same buffers, not cleared
    assert torch.equal(again_l, labels) and torch.equal(again_s, sizes)
    if name == "solid":
        assert bool((labels == 1).all()) and int(sizes.flatten()[0]) == vol.size
    if name == "serpentine":
        assert int(sizes.flatten()[0]) == int(vol.sum()) and ncomp == 1


@pytest.mark.parametrize("out_off", C.LABEL_OUT_OFF)
@pytest.mark.parametrize("vol_off", C.LABEL_VOL_OFF)
@pytest.mark.parametrize("W", C.LABEL_W)
def test_label_row_widths_and_alignments(hip, W, vol_off, out_off):
    vol = C.label_volume(W)
    assert (vol == C.LABEL_NCLS).any()                                       # an id out of range among the foreground
    check_label(hip, vol, C.LABEL_NCLS, f"components.W{W}.vol+{vol_off}.out+{out_off}", vol_off, out_off)


@pytest.mark.parametrize("fill", ["noise", "solid"])
@pytest.mark.parametrize("shape", C.LINES, ids=lambda s: "x".join(map(str, s)))
def test_label_dimension_of_2048(hip, shape, fill):
    vol = noise(shape, 2, 0.7, 7) if fill == "noise" else np.ones(shape, np.uint8)
    labels, sizes = check_label(hip, vol, 3, f"components.{shape}.{fill}")
    if fill == "solid":
        assert bool((labels == 1).all()) and int(sizes.flatten()[0]) == 2048


@pytest.mark.parametrize("ids", sorted(C.SEAM_IDS))
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_label_ids_past_ncls_join_nothing_across_a_seam(hip, axis, ids):
    vol = C.seam_lanes(axis, *C.SEAM_IDS[ids])
    labels, sizes = check_label(hip, vol, 3, f"components.seam.{'zyx'[axis]}.{ids}")
    assert not bool(labels[torch.from_numpy(np.array(vol >= 3))].any()) and int((sizes > 0).sum()) == 9


@pytest.mark.parametrize("name", sorted(C.LABEL_IDS))
def test_label_smallest_and_largest_ncls(hip, name):
    shape, ids, ncls = C.LABEL_IDS[name]
    vol = C.ids_volume(shape, ids, 41)
    labels, _ = check_label(hip, vol, ncls, f"components.{name}")
    legal = torch.from_numpy((vol > 0) & (vol < ncls))
    assert bool((labels[legal] > 0).all()) and not bool(labels[~legal].any()) and bool(legal.any()) and bool((~legal).any())


# ---- cswin_components_filter --------------------------------------------------------------------------------------------------
def tables(rule, ncls):
    ms, mf = rule_tables(rule, ncls)
    return np.asarray(ms, np.int64), np.asarray(mf, np.float64)


def check_filter(hip, vol, ncls, rule, what, vol_off=0, out_off=0, lab_off=0, want=None, then_in_place=False):
    """Labels and sizes from the label call (labels lab_off bytes past a 16-byte boundary), then the filter on guarded buffers
    against filter_ref; out_off None: in place.  then_in_place: a second call that writes over the input."""
    vol = np.ascontiguousarray(vol)
    D, H, W = vol.shape
    ms, mf = tables(rule, ncls)
    want = filter_ref(vol, ncls, ms, mf) if want is None else want
    src = GuardedInt(vol.shape, torch.uint8, vol_off)
    src.t.copy_(torch.from_numpy(np.array(vol)))
    o = dict(labels=GuardedInt(vol.shape, torch.int32, lab_off), sizes=GuardedInt(vol.shape, torch.int32),
             workspace=GuardedInt((hip.lib().cswin_components_workspace(D, H, W),), torch.uint8))
    labels, sizes = call_label(hip, src.t, o, vol.shape, ncls, what + " label")
    wl, ws = canonical_labels(vol, ncls)
    same(labels, wl, what + " labels")
    same(sizes, ws, what + " sizes")
    msd, mfd = put(ms), put(mf)
    dst = src if out_off is None else GuardedInt(vol.shape, torch.uint8, out_off)
    assert src.addr % 16 == vol_off and dst.addr % 16 == (vol_off if out_off is None else out_off) and o["labels"].addr % 16 == lab_off

    def call(into, tag):
        hip.call("cswin_components_filter", at(src.addr), at(o["labels"].addr), at(o["sizes"].addr), hip.ptr(msd), hip.ptr(mfd), at(into.addr),
                 at(o["workspace"].addr), o["workspace"].nbytes, D, H, W, ncls, hip.stream())
        settle_int(tag, dict(o, out=into, vol=src), refs=dict(out=want, vol=vol))
        same(into.t.cpu(), want, tag)
        assert torch.equal(o["labels"].t.cpu(), labels) and torch.equal(o["sizes"].t.cpu(), sizes), tag + ": labels or sizes were written"
    call(dst, what)
    if dst is not src:
        assert torch.equal(src.t.cpu(), torch.from_numpy(np.array(vol))), what + ": the input was written"
    if then_in_place:
        call(src, what + " in place")
    return want


def test_contention_filter_mixed_rule_then_in_place(hip):
    vol, _, _ = contention_ref("noise3d")
    want = check_filter(hip, vol, 3, C.CONTENTION_RULE, "components.filter.noise3d", then_in_place=True)
    dropped = want != vol
    print(f"noise3d filter: {int(dropped.sum())} voxels dropped, {int((vol == 1).sum() - (want == 1).sum())} of class 1")
    assert dropped[vol == 1].any() and dropped[vol == 2].any() and (want == 1).sum() == 602958


@pytest.mark.parametrize("align", C.FILTER_ALIGN, ids=lambda a: "vol+{}.out{}.labels+{}".format(a[0], "=vol" if a[1] is None else "+%d" % a[1], a[2]))
@pytest.mark.parametrize("name", sorted(C.FILTER_CASES))
def test_filter_sizes_alignments_ids_and_thresholds(hip, name, align):
    build, ncls, rule = C.FILTER_CASES[name]
    vol = build()
    want = check_filter(hip, vol, ncls, rule, f"components.filter.{name}.{align}", *align)
    assert np.array_equal(want[vol >= ncls], vol[vol >= ncls])              # and so are the device's: ids past ncls pass through


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_touch_nothing(hip):
    D, H, W, ncls = 3, 5, 7, 4
    N = D * H * W
    need = hip.lib().cswin_components_workspace(D, H, W)
    o = dict(vol=GuardedInt((N,), torch.uint8), labels=GuardedInt((N,), torch.int32), sizes=GuardedInt((N,), torch.int32),
             out=GuardedInt((N,), torch.uint8), workspace=GuardedInt((need + 16,), torch.uint8))
    ms, mf = put(np.zeros(ncls + 2, np.int64)), put(np.zeros(ncls + 2, np.float64))
    A = {k: g.addr for k, g in o.items()}

    def label(**kw):
        a = dict(vol=at(A["vol"]), labels=at(A["labels"]), sizes=at(A["sizes"]), ws=at(A["workspace"]), nbytes=need, D=D, H=H, W=W, ncls=ncls)
        a.update(kw)
        return tuple(a.values()) + (hip.stream(),)

    def filt(**kw):
        a = dict(vol=at(A["vol"]), labels=at(A["labels"]), sizes=at(A["sizes"]), ms=hip.ptr(ms), mf=hip.ptr(mf), out=at(A["out"]),
                 ws=at(A["workspace"]), nbytes=need, D=D, H=H, W=W, ncls=ncls)
        a.update(kw)
        return tuple(a.values()) + (hip.stream(),)
    for name, args in (("cswin_components_label", label), ("cswin_components_filter", filt)):
        hip.refused(ERR_ALIGN, "workspace 4 bytes off", o, name, *args(ws=at(A["workspace"] + 4)))
        hip.refused(ERR_ALIGN, "labels 2 bytes off", o, name, *args(labels=at(A["labels"] + 2)))
        hip.refused(ERR_ALIGN, "sizes 2 bytes off", o, name, *args(sizes=at(A["sizes"] + 2)))
        for dim in "DHW":
            hip.refused(ERR_SHAPE, f"{dim} = 2049", o, name, *args(**{dim: 2049}))
    hip.refused(ERR_ALIGN, "min_size 4 bytes off", o, "cswin_components_filter", *filt(ms=at(ms.data_ptr() + 4)))
    hip.refused(ERR_ALIGN, "min_fraction 4 bytes off", o, "cswin_components_filter", *filt(mf=at(mf.data_ptr() + 4)))
    hip.refused(ERR_UNSUPPORTED, "sizes is labels", o, "cswin_components_label", *label(sizes=at(A["labels"])))
    hip.refused(ERR_UNSUPPORTED, "sizes begins at labels' last element", o, "cswin_components_label", *label(sizes=at(A["labels"] + 4 * (N - 1))))
    hip.refused(ERR_UNSUPPORTED, "out is sizes", o, "cswin_components_filter", *filt(out=at(A["sizes"])))
    hip.refused(ERR_UNSUPPORTED, "out ends in sizes' first byte", o, "cswin_components_filter", *filt(out=at(A["sizes"] - N + 1)))
    hip.refused(ERR_UNSUPPORTED, "out at the workspace", o, "cswin_components_filter", *filt(out=at(A["workspace"])))
    hip.refused(ERR_UNSUPPORTED, "out at the last byte of the workspace's table", o, "cswin_components_filter", *filt(out=at(A["workspace"] + TAB_BYTES - 1)))
    hip.refused(ERR_UNSUPPORTED, "out is vol shifted by one byte", o, "cswin_components_filter", *filt(out=at(A["vol"] + 1)))
    hip.refused(ERR_UNSUPPORTED, "out is vol shifted back by one byte", o, "cswin_components_filter", *filt(out=at(A["vol"] - 1)))
