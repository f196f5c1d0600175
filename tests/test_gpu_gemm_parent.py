"""The tiled GEMM family (csrc/gemm.hip) against the build before its device half was tidied: one tile geometry, one operand
path, one batch dispatch.  That change merged no kernel and moved no load, no LDS image, no sum and no rounding, so every output
must equal the recorded one bit for bit (tests/golden/gemm_parent.npz, written by `PYTHONPATH=.:tests python
tests/test_gpu_gemm_parent.py record` on that build; the recorder runs every record twice and refuses to write when the two runs
differ).

Records, all through the C entry points with the case tables, input makers and guarded buffers of the existing shape tests:
  row.*     ROWS of test_gpu_gemm_shapes at precision 0: cswin_linear_fwd, cswin_linear_bwd_data and cswin_linear_bwd_weight in the
            plain and the row-scaled forms (with the row's misaligned operands), and at FORM_ROWS the concat, GELU, GELU-backward,
            split and add forms at both seams
  batch.*   BATCHES, BATCH_ODD and the TAIL launch with and without riding reductions
  tiled16.* TILED16 at precision 1; forward and data gradient also with x / dy, w and both stored as bf16 (io_bf16 1, 4, 5: with
            0 the four storage variants of the main loop; the data gradient's B image is the transposed-read one)
  conv*.*   TOKEN_CASES and STEM of test_gpu_conv_gather at precision 0, HEAD, TAP_MID and S2_EVEN also at precision 1:
            cswin_conv_tok_fwd, cswin_conv_tok_bwd_data (the generic transposed gather, or the stride-2 parity classes),
            cswin_conv_tok_bwd_weight, and for the "same" convolutions the data gradient as a forward convolution of dy
  mask.*    SMALL and MANY of test_gpu_wgrad_mask with each of DROPS, plain and with row_scale: the masked batch and the masked tail

An array of up to 4096 words is stored in full, a larger one as its shape and the SHA-256 of its bytes; words that several keys
share are stored once (pack).  This file runs unchanged on either build."""
import functools
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

from oracle.determ import det_normal

from test_gpu_attn_shapes import Guarded, bits, settle
from test_gpu_conv_gather import HEAD, S2_EVEN, STEM, TAP_MID, TOKEN_CASES
from test_gpu_gemm_shapes import (BATCHES, BATCH_ODD, FORM_ROWS, ROWS, TAIL, TILED16, batch_problems, gemm_inputs, lin, put, rid,  # noqa: F401
                                  row_scales, sample_rows, seams, tail_problems)
from test_gpu_shapes import cid, conv_inputs
from test_gpu_wgrad_mask import DROPS, MANY, SMALL, Problem, launch

gpu = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_parent.npz")
FULL_WORDS = 4096
DEV = "cuda"
MASK_SHAPES = {"small": SMALL, "many": MANY}
CONV_P1 = (HEAD, TAP_MID, S2_EVEN)

# name -> (kind, what it runs)
RECORDS = {f"row.{rid(r)}": ("row", r) for r in ROWS}
RECORDS.update({f"batch.{k}": ("batch", BATCHES[k][0]) for k in range(len(BATCHES))})
RECORDS.update({"batch.odd": ("batch", BATCH_ODD), "batch.tail": ("tail", False), "batch.tail_rider": ("tail", True)})
RECORDS.update({f"tiled16.{'x'.join(map(str, s))}.{e}": ("tiled16", (s, e)) for s, e, _ in TILED16})
RECORDS.update({f"conv0.{cid(c)}": ("conv", (c, 0)) for c in TOKEN_CASES + [STEM]})
RECORDS.update({f"conv1.{cid(c)}": ("conv", (c, 1)) for c in CONV_P1})
RECORDS.update({f"mask.{s}.{d}.{'row_scale' if sc else 'plain'}": ("mask", (s, d, sc)) for s in MASK_SHAPES for d in sorted(DROPS) for sc in (False, True)})


def keep(out, name, t):
    a = bits(t.contiguous()).reshape(-1).cpu().numpy().copy()
    if a.size <= FULL_WORDS:
        out[name] = a
    else:       # the shape as little-endian int64, then the digest
        out[name + ".sha256"] = np.frombuffer(np.array(t.shape, "<i8").tobytes() + hashlib.sha256(a.tobytes()).digest(), np.uint8).copy()


def pack(arrays):
    """What goes to the file: many records hold the same words (a form that only adds an output, the tail's weight gradients beside
    the batch's), so an array of more than 64 words that an earlier key already holds is stored as `<key>.same`, that key's name."""
    out, first = {}, {}
    for key, a in arrays.items():
        h = hashlib.sha256(a.tobytes()).digest() + str(a.dtype).encode()
        if a.size > 64 and h in first:
            out[key + ".same"] = np.frombuffer(first[h].encode(), np.uint8).copy()
        else:
            first.setdefault(h, key)
            out[key] = a
    return out


@functools.lru_cache(maxsize=None)
def unpack(path=GOLDEN):
    """key -> array of a packed file, read once per path."""
    npz = np.load(path)
    return {(k[:-5] if k.endswith(".same") else k): (npz[bytes(npz[k]).decode()] if k.endswith(".same") else npz[k]) for k in npz.files}


def keep_all(out, name, tensors):
    for k, t in tensors.items():
        if t is not None:
            keep(out, f"{name}:{k}", t)


def row_record(L, name, row):
    """The calls of test_gpu_gemm_shapes' three fp32 tests at this row."""
    shape, off = row
    M, N, K = shape
    i, rps, out = gemm_inputs(shape), sample_rows(M), {}
    rs = row_scales(M, rps)
    fwd = lambda form, *a, **kw: keep_all(out, f"{name}:fwd.{form}", L.fwd(shape, i["x"], i["w"], i["bias"], *a, what=f"{name} fwd {form}", **kw))
    dgrad = lambda form, **kw: keep_all(out, f"{name}:dgrad.{form}", L.dgrad(shape, i["dy"], i["w"], what=f"{name} dgrad {form}", **kw))
    dw = lambda form, **kw: keep_all(out, f"{name}:dw.{form}", L.dw(shape, i["dy"], i["x"], what=f"{name} dw {form}", **kw)[0])
    fwd("plain", off=off)
    fwd("res", residual=i["residual"], rs=rs, rps=rps, off=off)
    dgrad("plain", off=off)
    dgrad("scaled", rs=rs, rps=rps, off=off)
    dgrad("add", rs=rs, rps=rps, add=i["add"], off=off)
    dw("plain", off=off)
    dw("scaled", rs=rs, rps=rps, deferred=True, off=off)
    if row in FORM_ROWS:
        a, b = seams(K)
        fwd("gelu", act=True)
        fwd("concat", k_split=a)
        fwd("concat_res", k_split=b, residual=i["residual"], rs=rs, rps=rps)
        dgrad("gelu", pre=i["pre"], rs=rs, rps=rps)
        dgrad(f"split{a}", k_split=a)
        dgrad(f"split{b}", k_split=b)
        dw("nobias", dbias=False)
        dw("concat", k_split=a, deferred=True)
        dw("concat_scaled", k_split=b, rs=rs, rps=rps, dbias=False)
    return out


def keep_batch(out, name, res, dx=None, riders=None):
    for j, r in enumerate(res):
        keep_all(out, f"{name}:p{j}", dict(dw=r["dw"], dbias=r["dbias"]))
        out[f"{name}:p{j}.rows"] = np.array([r["rows"]], np.int64)
    if dx is not None:
        keep(out, f"{name}:dx", dx)
    for j, t in enumerate(riders or []):
        keep(out, f"{name}:rider{j}", t)


def batch_record(L, name, shapes):
    out = {}
    res, _, _ = L.batch(batch_problems(shapes)[0], what=name)
    keep_batch(out, name, res)
    return out


def tail_record(L, name, rider):
    M, C = TAIL["M"], TAIL["C"]
    out, pending = {}, None
    if rider:
        earlier = [(M, C, C), (M, 3 * C, C)]
        jobs, outs, alive = L.pending_jobs([dict(shape=s, dy=gemm_inputs(s)["dy"], x=gemm_inputs(s)["x"]) for s in earlier], what=name)
        pending = (jobs, outs)
    t = gemm_inputs((M, 3 * C, C))
    res, dx, riders = L.batch(batch_problems(tail_problems())[0], pending=pending, tail=dict(dy=t["dy"], w=t["w"]), what=name)
    keep_batch(out, name, res, dx, riders)
    return out


def tiled16_record(L, name, what):
    """precision 1 on unrounded inputs, so that the operand rounding is part of what is pinned."""
    shape, entry = what
    M = shape[0]
    i, rps, out = gemm_inputs(shape), sample_rows(M), {}
    rs = row_scales(M, rps)
    if entry == "fwd":
        for io in (0, 1, 4, 5):
            keep_all(out, f"{name}:plain.io{io}", L.fwd(shape, i["x"], i["w"], i["bias"], precision=1, io=io, what=f"{name} io{io}"))
        keep_all(out, f"{name}:gelu", L.fwd(shape, i["x"], i["w"], i["bias"], act=True, precision=1, what=f"{name} gelu"))
        keep_all(out, f"{name}:res", L.fwd(shape, i["x"], i["w"], i["bias"], residual=i["residual"], rs=rs, rps=rps, precision=1, what=f"{name} res"))
    elif entry == "dgrad":
        for io in (0, 1, 4, 5):
            keep_all(out, f"{name}:plain.io{io}", L.dgrad(shape, i["dy"], i["w"], precision=1, io=io, what=f"{name} io{io}"))
        keep_all(out, f"{name}:gelu", L.dgrad(shape, i["dy"], i["w"], pre=i["pre"], rs=rs, rps=rps, precision=1, what=f"{name} gelu"))
    else:
        keep_all(out, f"{name}:plain", L.dw(shape, i["dy"], i["x"], precision=1, deferred=True, what=f"{name} plain")[0])
        keep_all(out, f"{name}:scaled", L.dw(shape, i["dy"], i["x"], rs=row_scales(M, rps, True), rps=rps, precision=1, what=f"{name} scaled")[0])
    return out


def conv_record(L, name, what):
    """The three conv entry points on the case's seeded inputs; channels that are no multiple of 4 (the stem's 3) are zero padded
    on the host, in the tokens and in the weights."""
    from cswin_unet_amd._lib import call, lib, ptr, stream
    case, precision = what
    B, H, W, Cin, Cout, ks, stride, pad = case
    OH, OW = (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1
    x, w, b, dy = conv_inputs(case)
    cp = (Cin + 3) // 4 * 4
    x = np.concatenate([x, np.zeros(x.shape[:2] + (cp - Cin,), np.float32)], 2)
    w = np.concatenate([w, np.zeros((Cout, cp - Cin, ks, ks), np.float32)], 1)
    xd, wd, bd, dyd = put(x), put(w), put(b), put(dy)
    wp, wpt = torch.empty(Cout, ks * ks, cp, device=DEV), torch.empty(ks * ks, Cout, cp, device=DEV)
    call("cswin_conv_weight_permute", ptr(wd), ptr(wp), ptr(wpt), Cout, cp, ks, cp, stream())
    nbytes = lib().cswin_conv_tok_bwd_weight_workspace(B, H, W, cp, Cout, ks, stride, pad)
    o = dict(y=Guarded((B, OH * OW, Cout)), dx=Guarded((B, H * W, cp)), dw=Guarded((Cout, cp, ks, ks)), db=Guarded((Cout,)),
             workspace=Guarded((nbytes // 4,)))
    call("cswin_conv_tok_fwd", ptr(xd), ptr(wp), ptr(bd), ptr(o["y"].t), B, H, W, cp, Cout, ks, stride, pad, precision, stream())
    call("cswin_conv_tok_bwd_data", ptr(dyd), ptr(wpt), ptr(o["dx"].t), B, H, W, cp, Cout, ks, stride, pad, precision, stream())
    call("cswin_conv_tok_bwd_weight", ptr(dyd), ptr(xd), ptr(o["dw"].t), ptr(o["db"].t), ptr(o["workspace"].t), nbytes, B, H, W, cp, Cout, ks,
         stride, pad, 1, None, precision, stream())
    if stride == 1 and 2 * pad == ks - 1:
        wf = torch.empty(cp, ks * ks, Cout, device=DEV)
        call("cswin_conv_weight_flipT", ptr(wd), ptr(wf), Cout, cp, ks, stream())
        o["dx_same"] = Guarded((B, H * W, cp))
        call("cswin_conv_tok_fwd", ptr(dyd), ptr(wf), None, ptr(o["dx_same"].t), B, H, W, Cout, cp, ks, 1, pad, precision, stream())
    settle(name, o)
    out = {}
    keep_all(out, name, {k: g.t for k, g in o.items() if k != "workspace"})
    return out


def mask_record(L, name, what):
    """One masked batch launch and one masked tail launch (with a data gradient and a riding reduction) of the same problem.  The
    dropped samples' rows hold NaN in both operands."""
    from cswin_unet_amd._lib import ReduceJob
    s, drop, scaled = what
    shape = MASK_SHAPES[s]
    ns = shape["ns"]
    m = np.array([DROPS[drop][k % 5] for k in range(ns)], np.float32) * 1.25
    p = Problem(f"parent.{s}.{drop}", mask=m, scale=m * np.array([(1, 0.5, 2, 1, 3)[k % 5] for k in range(ns)], np.float32) if scaled else None, **shape)
    out = {}
    (dw, db), = launch([p], True)[0]
    keep_all(out, f"{name}:batch", dict(dw=dw, dbias=db))
    tdy = torch.from_numpy(det_normal(f"gparent.{s}.tail.dy", (p.M, p.N))).to(DEV)
    tw = torch.from_numpy(det_normal(f"gparent.{s}.tail.w", (p.N, 32), 1 / np.sqrt(32))).to(DEV)
    part = torch.from_numpy(det_normal("gparent.tail.part", (7, 300))).to(DEV)
    rider = torch.full((300,), float("nan"), device=DEV)
    pend = (ReduceJob * 1)()
    pend[0].part, pend[0].out, pend[0].n_first, pend[0].n, pend[0].stride, pend[0].rows = part.data_ptr(), rider.data_ptr(), 300, 300, 300, 7
    ((dw, db),), dx = launch([p], True, tail=(tdy, tw), pending=pend)
    keep_all(out, f"{name}:tail", dict(dw=dw, dbias=db, dx=dx, rider=rider))
    return out


KINDS = dict(row=row_record, batch=batch_record, tail=tail_record, tiled16=tiled16_record, conv=conv_record, mask=mask_record)


def recorded(L, name):
    kind, what = RECORDS[name]
    return KINDS[kind](L, name, what)


def test_golden_file_holds_every_record_and_nothing_else():
    """No GPU needed: every record has its arrays, every array its record, the file keeps to its size."""
    files = list(unpack())
    assert len(RECORDS) == len(ROWS) + len(BATCHES) + 3 + len(TILED16) + len(TOKEN_CASES) + 1 + len(CONV_P1) + 2 * len(DROPS) * 2
    arrays = lambda name: {k[len(name) + 1:].split(".sha256")[0] for k in files if k.startswith(name + ":")}
    for name, (kind, what) in RECORDS.items():
        mine = arrays(name)
        assert mine, name
        if kind == "row":
            forms = 7 + (9 if what in FORM_ROWS else 0)
            assert len({k.rsplit(":", 1)[0] for k in mine}) == forms, name
        elif kind == "mask":
            assert mine == {"batch:dw", "batch:dbias", "tail:dw", "tail:dbias", "tail:dx", "tail:rider"}, name
        elif kind == "conv":
            same = what[0][6] == 1 and 2 * what[0][7] == what[0][5] - 1
            assert mine == {"y", "dx", "dw", "db"} | ({"dx_same"} if same else set()), name
        elif kind in ("batch", "tail"):
            n = len(what) if kind == "batch" else 4
            assert {f"p{j}:dw" for j in range(n)} | {f"p{j}.rows" for j in range(n)} <= mine, name
            assert kind == "batch" or ("dx" in mine and ({"rider0", "rider1", "rider2", "rider3"} <= mine) == what), name
    assert all(any(k.startswith(name + ":") for name in RECORDS) for k in files)
    assert os.path.getsize(GOLDEN) < 1_000_000


def assert_same_bits(want, got, name):
    """got holds exactly the arrays that the golden file `want` has for record `name`, word for word."""
    assert sorted(got) == sorted(k for k in want if k.startswith(name + ":"))
    for key, a in got.items():
        ref = want[key]
        assert a.dtype == ref.dtype and a.shape == ref.shape, key
        if not np.array_equal(a, ref):
            k = int(np.flatnonzero(a != ref)[0])
            raise AssertionError(f"{key}: {int((a != ref).sum())} of {ref.size} words differ, the first at flat index {k}: "
                                 f"{int(a[k]):#x} for {int(ref[k]):#x}")


@gpu
@pytest.mark.parametrize("name", list(RECORDS))
def test_gemm_bits_equal_the_build_before_the_device_half_was_tidied(lin, name):
    """Every recorded array of this record, word for word."""
    assert_same_bits(unpack(), recorded(lin, name), name)


def record(names, recorded, dest):
    """The recorder (also test_gpu_bf16_parent's): every record twice on this build, nothing written when the two runs differ."""
    os.makedirs(os.path.dirname(dest), exist_ok=True)
    make = getattr(lin, "_get_wrapped_function", None)
    L = (make() if make else lin.__wrapped__)()
    arrays = {}
    for rec in names:
        first, second = recorded(L, rec), recorded(L, rec)
        assert sorted(first) == sorted(second), rec
        for key in first:
            if not np.array_equal(first[key], second[key]):
                sys.exit(f"{key}: two runs of the same build differ; nothing written")
        arrays.update(first)
        print(rec, len(first), "arrays", flush=True)
    np.savez_compressed(dest, **pack(arrays))
    print("wrote", dest, os.path.getsize(dest), "bytes,", len(arrays), "arrays")


if __name__ == "__main__" and sys.argv[1:2] == ["record"]:
    record(RECORDS, recorded, sys.argv[2] if len(sys.argv) > 2 else GOLDEN)
