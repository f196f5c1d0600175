"""The attention kernels (csrc/attn.hip) against the build before their tile steps, forward phases and staging helpers were
written once: that change merged no kernel and moved no load, no store and no rounding, so every output must equal the recorded
one bit for bit, NaNs included (tests/golden/attn_parent.npz, written by `PYTHONPATH=.:tests python tests/test_gpu_attn_parent.py
record` on that build; the recorder runs every record twice and refuses to write when the two runs differ).

One record per row of test_gpu_attn_shapes' tables: RUNS in mode 0, MODE_ROWS in modes 1, 3 and 7, DROP_ROWS in mode 0 with
p = 0.25 and a fixed seed.  Per record: y, y0 and lse of cswin_attn_fwd; then cswin_attn_bwd twice on the forward's outputs.  Once
with `deferred`: dqkv, the job fields it returns (the slab pointer as its offset into the workspace, out / out2 as the index of
the gradient they point to) and the LePE gradients after cswin_rows_sum_multi on those jobs, which is the path ops.py takes.  Once
without: dqkv and the LePE gradients of the immediate reduction must equal the first call's, word for word, and so the recorded
ones -- except the LePE gradients of jobs that qualify for the few-rows summation order (few_rows_job below, a transcription of
reduce_job_few_ok in csrc/common.h): the immediate reduction did not take that order before it went through the common job
table, and takes it since; those are compared with nothing.

Every output is a view into a NaN-filled guarded buffer and the workspace is exactly cswin_attn_bwd_workspace() bytes.  An array
of up to 4096 words is stored in full, a larger one as its shape and the SHA-256 of its bytes.  Only the C entry points and the
case tables, input makers and guarded buffers of test_gpu_attn_shapes are used, so this file runs unchanged on either build."""
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

from test_gpu_attn_shapes import (DROP_ROWS, MODE_ROWS, RUNS, attn, attn_inputs, attn_plan, bits, cid, run_id, settle)  # noqa: F401

gpu = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attn_parent.npz")
FULL_WORDS = 4096
DROP = (0.25, 20240607)
LW_SUB = 4                           # slab rows per window of the two-pass backward (csrc/attn.hip)
JOB_FIELDS = ("part_offset", "out", "out2", "n_first", "n", "stride", "rows", "conv_kk", "conv_cin")

# name -> (case, mode, factor on q and k, scale, dropout)
RECORDS = {f"m0.{run_id(r)}": (r[0], 0, r[1], r[2], (0.0, 0)) for r in RUNS}
RECORDS.update({f"m{m}.{cid(c)}": (c, m, 1, None, (0.0, 0)) for m in (1, 3, 7) for c in MODE_ROWS})
RECORDS.update({f"drop.{cid(c)}": (c, 0, 1, None, DROP) for c in DROP_ROWS})


def lepe_jobs(case):
    """(rows, n) of each branch's LePE slab reduction: B nWin slab_rows rows of [Cb 9 | Cb] columns."""
    B, reso, split, idx, C, heads = case
    plan, Cb = attn_plan(*case), C // len(idx)
    rows = B * (reso * reso // plan["N"]) * (LW_SUB if plan["bwd"][0] == "two_pass" else 1)
    return [(rows, 10 * Cb) for _ in idx]


def few_rows_job(rows, n):
    """reduce_job_few_ok for a job whose slabs and outputs are 16-byte aligned and whose columns are multiples of four."""
    return rows <= 16 and n >= 4096


def keep(out, name, t):
    a = bits(t.contiguous()).reshape(-1).cpu().numpy().copy()
    if a.size <= FULL_WORDS:
        out[name] = a
    else:
        out[name + ".shape"] = np.array(t.shape, np.int64)
        out[name + ".sha256"] = np.frombuffer(hashlib.sha256(a.tobytes()).digest(), np.uint8).copy()


def recorded(A, name):
    from cswin_unet_amd._lib import ReduceJob, call, ptr, stream
    from cswin_unet_amd.ops import _int_array, _job_ptr, _ptr_array
    case, mode, qk_mul, scale, drop = RECORDS[name]
    B, reso, split, idx, C, heads = case
    nb, out = len(idx), {}
    qkv, lw, lb, dy = A.dev(*attn_inputs(case, qk_mul), mode=mode)
    y, y0, lse = A.fwd(case, mode, qkv, lw, lb, scale, drop)
    for k, t in (("y", y), ("y0", y0), ("lse", lse)):
        keep(out, f"{name}:{k}", t)

    # the product path: the jobs come back in `deferred` and cswin_rows_sum_multi runs them
    o, nbytes = A.outputs_bwd(case, mode)
    jobs = (ReduceJob * nb)()
    grads = [o[f"dlepe_w{i}"].t for i in range(nb)], [o[f"dlepe_b{i}"].t for i in range(nb)]
    call("cswin_attn_bwd", ptr(qkv), _ptr_array(lw), _ptr_array(lb), ptr(lse), ptr(y0), ptr(dy), ptr(o["dqkv"].t), _ptr_array(grads[0]),
         _ptr_array(grads[1]), ptr(o["workspace"].t), nbytes, B, reso, C, nb, _int_array(heads), _int_array(idx), split, float(scale or 0.0),
         _job_ptr(jobs), drop[0], drop[1], None, mode, stream())
    torch.cuda.synchronize()
    assert all(g.untouched() for k, g in o.items() if k.startswith("dlepe")), "a deferred reduction wrote its outputs"
    fields = []
    for i, j in enumerate(jobs):
        assert (j.rows, j.n) == lepe_jobs(case)[i] and j.part % 16 == 0 and j.out % 16 == 0 and j.out2 % 16 == 0
        fields += [j.part - o["workspace"].t.data_ptr(), [t.data_ptr() for t in grads[0]].index(j.out), [t.data_ptr() for t in grads[1]].index(j.out2),
                   j.n_first, j.n, j.stride, j.rows, j.conv_kk, j.conv_cin]
    assert len(fields) == nb * len(JOB_FIELDS)
    out[f"{name}:jobs"] = np.array(fields, np.int64)
    call("cswin_rows_sum_multi", _job_ptr(jobs), nb, stream())
    settle(f"deferred attn_bwd {name}", o)
    for k, g in o.items():
        if k != "workspace":
            keep(out, f"{name}:{k}", g.t)

    # the immediate reduction
    now = A.bwd(case, mode, qkv, lw, lb, lse, y0, dy, scale, drop)
    few = [few_rows_job(*j) for j in lepe_jobs(case)]
    assert bool((bits(now["dqkv"]) == bits(o["dqkv"].t)).all()), "dqkv depends on whether the reduction is deferred"
    for k, t in now.items():
        if k != "dqkv" and not few[int(k[-1])]:
            assert bool((bits(t) == bits(o[k].t)).all()), f"{k}: the immediate reduction differs from cswin_rows_sum_multi on the same job"
    return out


def test_records_the_few_rows_order_can_touch():
    """No GPU needed.  rows <= 16 and 10 Cb >= 4096 columns: of all the tables' rows only the 768-channel single-branch one (two-pass
    backward, 3 x 1 x 4 = 12 slab rows of 7680 columns).  Its immediate LePE gradients are the only outputs compared with nothing."""
    touched = {RECORDS[name][0] for name in RECORDS if any(few_rows_job(*j) for j in lepe_jobs(RECORDS[name][0]))}
    assert touched == {(3, 11, 11, (-1,), 768, (96,))}
    assert lepe_jobs((3, 11, 11, (-1,), 768, (96,))) == [(12, 7680)]
    assert sorted(name for name in RECORDS if RECORDS[name][0] in touched) == sorted(f"m{m}.B3-r11-s11-i-1-C768-h96" for m in (0, 1, 3, 7))


def test_golden_file_holds_every_record_and_nothing_else(golden):
    """No GPU needed: every record has its arrays, every array its record, the file keeps to its size."""
    files = golden("attn_parent").files
    assert len(RECORDS) == len(RUNS) + 3 * len(MODE_ROWS) + len(DROP_ROWS)
    for name, (case, *_) in RECORDS.items():
        mine = {k[len(name) + 1:].split(".sha256")[0].split(".shape")[0] for k in files if k.startswith(name + ":")}
        want = {"y", "y0", "lse", "jobs", "dqkv"}
        for i in range(len(case[3])):
            want |= {f"dlepe_w{i}", f"dlepe_b{i}"}
        assert mine == want, name
    assert all(any(k.startswith(name + ":") for name in RECORDS) for k in files)
    assert os.path.getsize(GOLDEN) < 1_000_000


@gpu
@pytest.mark.parametrize("name", list(RECORDS))
def test_attention_bits_equal_the_build_before_the_shared_helpers(attn, golden, name):
    """Every recorded array of this record, word for word."""
    want, got = golden("attn_parent"), recorded(attn, name)
    assert sorted(got) == sorted(k for k in want.files if k.startswith(name + ":"))
    for key, a in got.items():
        ref = want[key]
        assert a.dtype == ref.dtype and a.shape == ref.shape, key
        if not np.array_equal(a, ref):
            k = int(np.flatnonzero(a != ref)[0])
            raise AssertionError(f"{key}: {int((a != ref).sum())} of {ref.size} words differ, the first at flat index {k}: "
                                 f"{int(a[k]):#x} for {int(ref[k]):#x}")


if __name__ == "__main__" and sys.argv[1:2] == ["record"]:
    dest = sys.argv[2] if len(sys.argv) > 2 else GOLDEN
    os.makedirs(os.path.dirname(dest), exist_ok=True)
    make = getattr(attn, "_get_wrapped_function", None)
    A = (make() if make else attn.__wrapped__)()
    arrays = {}
    for rec in RECORDS:
        first, second = recorded(A, rec), recorded(A, rec)
        assert sorted(first) == sorted(second), rec
        for key in first:
            if not np.array_equal(first[key], second[key]):
                sys.exit(f"{key}: two runs of the same build differ; nothing written")
        arrays.update(first)
        print(rec, len(first), "arrays", flush=True)
    np.savez_compressed(dest, **arrays)
    print("wrote", dest, os.path.getsize(dest), "bytes,", len(arrays), "arrays")
