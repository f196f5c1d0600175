"""The two objectives' kernels (csrc/loss.hip and csrc/cl_loss.hip over csrc/loss_pixel.h) against the build before their common
pixel body was written once: that change moved no load, no store and no rounding, so every output must equal the recorded one bit
for bit, NaNs included (tests/golden/loss_parent.npz, written by `PYTHONPATH=. python tests/test_gpu_loss_parent.py record` on that
build).

Recorded for every row of LOSS_CASES and of CL_CASES: the per-block partials the sums kernel leaves in the workspace, sums, out,
coef and dlogits.  The rows hold every instantiation (B = 3, 7 x 13, every class count, both modes) and 1, 255, 257, 133 563 and
526 338 pixels: the smallest that reach the second workgroup and the second trip of the sums loop and of the backward loop.  Then,
on one 7 x 13 row per objective, the finalize and backward forms: class weights, w_ce = 0, w_focal = 0, kd_weight 0 and 1, a
grad_out of 0.37, no teacher (nold = 0), two ranks emulated on summed sums, an out-of-range label; and the two public ops (loss,
stats, the input gradient after (0.37 * loss).backward()).  An array of up to 4096 words is stored in full, a larger one as its
shape and the SHA-256 of its bytes.  Every buffer a kernel writes is filled with -5 first and the workspace is exactly as large
as the library says.  Only the C entry points, ops.ce_dice_loss / ops.continual_loss and the case tables and input makers of
test_gpu_step_tail / test_continual_host are used, so this file runs unchanged on either build."""
import hashlib
import os
import sys
import types

import numpy as np
import pytest
import torch

from test_continual_host import CL_CASES, case_of, cl_inputs
from test_gpu_step_tail import LOSS_CASES, bits32, hip, loss_inputs, put, release_inputs  # noqa: F401

gpu = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loss_parent.npz")
FULL_WORDS = 4096
BASE_ROW, CL_ROW = "nc5.logits", "nc12.old9"             # the 7 x 13 rows of the variants and the public ops
GOUT = 0.37


def filled(n):
    return torch.full((n,), -5.0, dtype=torch.float32, device=DEV)


def dev(a, dtype):
    return None if a is None else put(np.asarray(a, dtype))


def keep(out, name, t):
    a = bits32(t).reshape(-1).copy()
    if a.size <= FULL_WORDS:
        out[name] = a
    else:
        out[name + ".shape"] = np.array(t.shape, np.int64)
        out[name + ".sha256"] = np.frombuffer(hashlib.sha256(a.tobytes()).digest(), np.uint8).copy()


def run_base(hip, out, name, x, lab, probs=False, w_ce=0.4, w_dice=0.6, cw=None, gout=None, sums_in=None, n_pixels=None, world=1):
    """cswin_loss_sums -> _finalize -> _bwd with the scales ops.ce_dice_loss passes; returns the device sums."""
    P, st = hip.ptr, hip.stream
    B, ncls, HW = x.shape
    xd, ld, cwd = put(x), put(np.asarray(lab, np.int64)), dev(cw, np.float32)
    nbytes = hip.lib().cswin_loss_workspace(B, ncls, HW)
    ws, sums, res, coef, dl = filled(nbytes // 4), filled(1 + 3 * ncls), filled(3), filled(2 * ncls), filled(B * ncls * HW)
    hip.call("cswin_loss_sums", P(xd), P(ld), P(sums), P(ws), nbytes, B, ncls, HW, int(probs), st())
    fin = sums if sums_in is None else sums_in
    hip.call("cswin_loss_finalize", P(fin), P(res), P(coef), float(B * HW if n_pixels is None else n_pixels), ncls, w_ce, w_dice, P(cwd), st())
    hip.call("cswin_loss_bwd", P(xd), P(ld), P(coef), P(dev(None if gout is None else [gout], np.float32)), P(dl), w_ce / float(B * HW),
             w_dice / ncls * world, B, ncls, HW, int(probs), st())
    for k, t in (("partial", ws), ("sums", sums), ("out", res), ("coef", coef), ("dlogits", dl.view(B, ncls, HW))):
        keep(out, f"{name}:{k}", t)
    return sums


def run_cl(hip, out, name, x, lab, t, cw=None, lmap=None, T=3.0, alpha=1.0, gamma=4.0, w_focal=0.2, w_dice=0.8, kd_weight=0.5, gout=None,
           sums_in=None, n_pixels=None, batch=None, world=1):
    """cswin_cl_loss_sums -> _finalize -> _bwd with the scales ops.continual_loss passes; returns the device sums."""
    P, st = hip.ptr, hip.stream
    B, ncls, HW = x.shape
    nold = 0 if t is None else t.shape[1]
    xd, ld, td, cwd, md = put(x), put(np.asarray(lab, np.int64)), dev(t, np.float32), dev(cw, np.float32), dev(lmap, np.int32)
    n_map = 0 if lmap is None else len(lmap)
    nbytes = hip.lib().cswin_cl_loss_workspace(B, ncls, HW)
    ws, sums, res, coef, dl = filled(nbytes // 4), filled(3 + 3 * ncls), filled(5), filled(2 * ncls), filled(B * ncls * HW)
    hip.call("cswin_cl_loss_sums", P(xd), P(ld), P(md), n_map, P(td), P(cwd), P(sums), P(ws), nbytes, B, ncls, nold, HW, T, alpha, gamma, st())
    fin = sums if sums_in is None else sums_in
    hip.call("cswin_cl_loss_finalize", P(fin), P(res), P(coef), float(B * HW if n_pixels is None else n_pixels), float(B if batch is None else batch),
             ncls, w_focal, w_dice, kd_weight, T, st())
    hip.call("cswin_cl_loss_bwd", P(xd), P(ld), P(md), n_map, P(td), P(cwd), P(coef), P(dev(None if gout is None else [gout], np.float32)), P(dl),
             (1.0 - kd_weight) * w_focal / float(B * HW), (1.0 - kd_weight) * w_dice / ncls * world, kd_weight * T / B, B, ncls, nold, HW, T, alpha,
             gamma, st())
    for k, v in (("partial", ws), ("sums", sums), ("out", res), ("coef", coef), ("dlogits", dl.view(B, ncls, HW))):
        keep(out, f"{name}:{k}", v)
    return sums


def base_row(tag):
    def run(hip, out, name):
        x, lab = loss_inputs(tag)
        probs = next(c for c in LOSS_CASES if c[0] == tag)[4]
        run_base(hip, out, name, x, lab, probs, *((0.0, 1.0) if probs else (0.4, 0.6)))
    return run


def cl_args(tag):
    x, lab, t, cw, lmap = cl_inputs(tag)
    o = case_of(tag)[6]
    return (x, lab, t), dict(cw=cw, lmap=lmap, T=o["T"], alpha=o["alpha"], gamma=o["gamma"])


def cl_row(tag, **kw):
    def run(hip, out, name):
        a, k = cl_args(tag)
        run_cl(hip, out, name, *a, **{**k, **kw})
    return run


def base_variant(**kw):
    return lambda hip, out, name: run_base(hip, out, name, *loss_inputs(BASE_ROW), **kw)


def spoiled(lab):
    lab = np.array(lab)
    lab[0, 17], lab[2, 90] = -1, 2 ** 32 + 1
    return lab


def base_oor(hip, out, name):
    x, lab = loss_inputs(BASE_ROW)
    run_base(hip, out, name, x, spoiled(lab))


def cl_oor(hip, out, name):
    (x, lab, t), k = cl_args(CL_ROW)
    run_cl(hip, out, name, x, spoiled(lab), t, **k)


def cl_no_teacher(hip, out, name):
    (x, lab, _), k = cl_args(CL_ROW)
    run_cl(hip, out, name, x, lab, None, **k)


def base_two_ranks(hip, out, name):
    """The halves' sums added on the device, finalize on the global pixel count, the backward per half with world = 2."""
    x, lab = loss_inputs(BASE_ROW)
    halves = [(x[:1], lab[:1]), (x[1:], lab[1:])]
    total = sum(run_base(hip, {}, "", xh, lh) for xh, lh in halves)
    for r, (xh, lh) in enumerate(halves):
        run_base(hip, out, f"{name}:rank{r}", xh, lh, sums_in=total, n_pixels=lab.size, world=2)


def cl_two_ranks(hip, out, name):
    (x, lab, t), k = cl_args(CL_ROW)
    halves = [(x[:1], lab[:1], t[:1]), (x[1:], lab[1:], t[1:])]
    total = sum(run_cl(hip, {}, "", *h, **k) for h in halves)
    for r, h in enumerate(halves):
        run_cl(hip, out, f"{name}:rank{r}", *h, **k, sums_in=total, n_pixels=lab.size, batch=x.shape[0], world=2)


def public_base(hip, out, name):
    from cswin_unet_amd import ops
    x, lab = loss_inputs(BASE_ROW)
    xd = put(x.reshape(x.shape[0], x.shape[1], 7, 13)).requires_grad_()
    loss, stats = ops.ce_dice_loss(xd, put(lab.reshape(-1, 7, 13)))
    (GOUT * loss).backward()
    for k, t in (("loss", loss.reshape(1)), ("stats", stats), ("grad", xd.grad)):
        keep(out, f"{name}:{k}", t)


def public_cl(hip, out, name):
    from cswin_unet_amd import ops
    (x, lab, t), k = cl_args(CL_ROW)
    xd = put(x.reshape(x.shape[0], x.shape[1], 7, 13)).requires_grad_()
    loss, stats = ops.continual_loss(xd, put(lab.reshape(-1, 7, 13)), put(t.reshape(t.shape[0], t.shape[1], 7, 13)), temperature=k["T"],
                                     focal_gamma=k["gamma"], focal_alpha=k["alpha"], class_weight=dev(k["cw"], np.float32),
                                     label_map=dev(k["lmap"], np.int32))
    (GOUT * loss).backward()
    for n, v in (("loss", loss.reshape(1)), ("stats", stats), ("grad", xd.grad)):
        keep(out, f"{name}:{n}", v)


RECORDS = {f"base.{c[0]}": base_row(c[0]) for c in LOSS_CASES}
RECORDS.update({f"cl.{c[0]}": cl_row(c[0]) for c in CL_CASES})
RECORDS.update({
    "base.var.class_weight": base_variant(cw=[0.5, 2.0, 0.0, 1.25, 3.0]),
    "base.var.w_ce0": base_variant(w_ce=0.0, w_dice=1.0),
    "base.var.gout": base_variant(gout=GOUT),
    "base.var.two_ranks": base_two_ranks,
    "base.var.out_of_range": base_oor,
    "cl.var.w_focal0": cl_row(CL_ROW, w_focal=0.0),
    "cl.var.kd0": cl_row(CL_ROW, kd_weight=0.0),
    "cl.var.kd1": cl_row(CL_ROW, kd_weight=1.0),
    "cl.var.gout": cl_row(CL_ROW, gout=GOUT),
    "cl.var.no_teacher": cl_no_teacher,
    "cl.var.two_ranks": cl_two_ranks,
    "cl.var.out_of_range": cl_oor,
    "op.ce_dice_loss": public_base,
    "op.continual_loss": public_cl,
})


def recorded(hip, name):
    out = {}
    RECORDS[name](hip, out, name)
    torch.cuda.synchronize()
    return out


def test_golden_file_holds_every_record_and_nothing_else(golden):
    """No GPU needed: every record has its arrays, every array its record, the file keeps to its size."""
    files = golden("loss_parent").files
    assert all(any(k.startswith(name + ":") for k in files) for name in RECORDS)
    assert all(any(k.startswith(name + ":") for name in RECORDS) for k in files)
    assert os.path.getsize(GOLDEN) < 1_000_000


@gpu
@pytest.mark.parametrize("name", list(RECORDS))
def test_loss_bits_equal_the_build_before_the_shared_pixel_body(hip, golden, name):
    """Every recorded array of this record, word for word."""
    want, got = golden("loss_parent"), recorded(hip, name)
    assert sorted(got) == sorted(k for k in want.files if k.startswith(name + ":"))
    for key, a in got.items():
        ref = want[key]
        assert a.dtype == ref.dtype and a.shape == ref.shape, key
        if not np.array_equal(a, ref):
            k = int(np.flatnonzero(a != ref)[0])
            raise AssertionError(f"{key}: {int((a != ref).sum())} of {ref.size} words differ, the first at flat index {k}: "
                                 f"{int(a[k]):#x} for {int(ref[k]):#x}")


if __name__ == "__main__" and sys.argv[1:2] == ["record"]:
    from cswin_unet_amd import _lib
    dest = sys.argv[2] if len(sys.argv) > 2 else GOLDEN
    os.makedirs(os.path.dirname(dest), exist_ok=True)
    h, arrays = types.SimpleNamespace(call=_lib.call, ptr=_lib.ptr, stream=_lib.stream, lib=_lib.lib), {}
    for rec in RECORDS:
        arrays.update(recorded(h, rec))
    np.savez_compressed(dest, **arrays)
    print("wrote", dest, os.path.getsize(dest), "bytes,", len(arrays), "arrays")
