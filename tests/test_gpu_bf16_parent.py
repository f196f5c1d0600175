"""The bf16 GEMM kernels (csrc/gemm16.hip, csrc/wgrad16.hip) against the build before their shared mechanisms moved into
csrc/bf16_tile.h: one LDS-DMA primitive, one transposed-read fragment, one patch put, one bf16 widening, one stamp writer.  That
change added, merged and removed no kernel and moved no load, no LDS image, no MFMA, no sum and no rounding, so every output must
equal the recorded one bit for bit (tests/golden/bf16_tile_parent.npz, written by `PYTHONPATH=.:tests python
tests/test_gpu_bf16_parent.py record` on that build; test_gpu_gemm_parent's recorder, which runs every record twice and refuses
to write when the two runs differ).

Records, all through the C entry points with the case tables, input makers and guarded buffers of test_gpu_gemm_shapes:
  gemm16.*  every row of GEMM16 whose plan is gemm16's, at io_bf16 5 and 7: the calls of fwd16_forms / dgrad16_forms on bf16-valued
            inputs (plain, the GELU pair, residual + row scale where the output is fp32; plain, GELU' with gelu_pre in fp32 and, io_bf16
            13 / 15, stored as bf16): 2 and 3 stages, a full and a half last step, ragged M, N % 64 == 8 and the 128 x 64 tile
  wgrad16.* every launch of WGRAD16: dw and dbias of every problem and the rows of its reduction job
  rider.*   the first register-path and the first LDS-DMA launch of WGRAD16 with two pending reductions riding in the grid: dw, dbias
            and what the riders wrote
The tiled family's transposed-read rows (tiled16.*) are in gemm_parent.npz and stay with test_gpu_gemm_parent.

Arrays are kept as that file keeps them (keep / pack / unpack).  This file runs unchanged on either build."""
import os
import sys

import pytest

from test_gpu_gemm_parent import assert_same_bits, keep_all, keep_batch, record, unpack
from test_gpu_gemm_shapes import GEMM16, WGRAD16, batch_problems, gemm_inputs, lin, row_scales, sample_rows  # noqa: F401

gpu = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bf16_tile_parent.npz")
G16_ROWS = [(s, e) for s, e, plan in GEMM16 if plan.startswith("gemm16")]
RIDERS = {"reg": next(k for k, w in enumerate(WGRAD16) if "reg" in w[3][0]), "dma": next(k for k, w in enumerate(WGRAD16) if "dma" in w[3][0])}
RIDER_SHAPES = [(300, 24, 24), (300, 72, 24)]      # the pending reductions: test_gpu_gemm_shapes' block tail has the same two

# name -> (kind, what it runs)
RECORDS = {f"gemm16.{'x'.join(map(str, s))}.{e}.io{io}": ("gemm16", (s, e, io)) for s, e in G16_ROWS for io in (5, 7)}
RECORDS.update({f"wgrad16.{k}": ("wgrad16", (k, False)) for k in range(len(WGRAD16))})
RECORDS.update({f"rider.{path}": ("wgrad16", (k, True)) for path, k in RIDERS.items()})


def gemm16_record(L, name, what):
    """The calls of fwd16_forms / dgrad16_forms at this row and storage."""
    shape, entry, io = what
    M = shape[0]
    i, rps, out = gemm_inputs(shape, True), sample_rows(M), {}
    rs = row_scales(M, rps)
    if entry == "fwd":
        keep_all(out, f"{name}:plain", L.fwd(shape, i["x"], i["w"], i["bias"], precision=1, io=io, what=f"{name} plain"))
        keep_all(out, f"{name}:gelu", L.fwd(shape, i["x"], i["w"], i["bias"], act=True, precision=1, io=io, what=f"{name} gelu"))
        if not io & 2:
            keep_all(out, f"{name}:res", L.fwd(shape, i["x"], i["w"], i["bias"], residual=i["residual"], rs=rs, rps=rps, precision=1, io=io,
                                               what=f"{name} res"))
    else:
        keep_all(out, f"{name}:plain", L.dgrad(shape, i["dy"], i["w"], precision=1, io=io, what=f"{name} plain"))
        for io_pre in (io, io | 8):
            form = "gelu16" if io_pre & 8 else "gelu"
            keep_all(out, f"{name}:{form}", L.dgrad(shape, i["dy"], i["w"], pre=i["pre"], rs=rs, rps=rps, precision=1, io=io_pre, what=f"{name} {form}"))
    return out


def wgrad16_record(L, name, what):
    k, riders = what
    shapes, ios, samples, _ = WGRAD16[k]
    out, pending = {}, None
    if riders:
        jobs, outs, alive = L.pending_jobs([dict(shape=s, dy=gemm_inputs(s)["dy"], x=gemm_inputs(s)["x"]) for s in RIDER_SHAPES], what=name)
        pending = (jobs, outs)
    res, _, ridden = L.batch(batch_problems(shapes, rounded=True, pow2=True, ios=ios, samples=samples)[0], precision=1, pending=pending, what=name)
    keep_batch(out, name, res, None, ridden)
    return out


KINDS = dict(gemm16=gemm16_record, wgrad16=wgrad16_record)


def recorded(L, name):
    kind, what = RECORDS[name]
    return KINDS[kind](L, name, what)


def test_golden_file_holds_every_record_and_nothing_else():
    """No GPU needed: every record has its arrays, every array its record, the file keeps to its size."""
    files = list(unpack(GOLDEN))
    assert len(G16_ROWS) == 12 and len(RECORDS) == 2 * len(G16_ROWS) + len(WGRAD16) + 2
    assert WGRAD16[RIDERS["reg"]][3] == ["wgrad16 reg 3x128(44)"] and WGRAD16[RIDERS["dma"]][3] == ["wgrad16 dma 3x128(64)"]
    arrays = lambda name: {k[len(name) + 1:].split(".sha256")[0] for k in files if k.startswith(name + ":")}
    for name, (kind, what) in RECORDS.items():
        mine = arrays(name)
        if kind == "gemm16":
            _, entry, io = what
            want = {"plain:y", "gelu:y", "gelu:y_act"} | ({"res:y"} if not io & 2 else set()) if entry == "fwd" else {"plain:dx", "gelu:dx", "gelu16:dx"}
            assert mine == want, name
        else:
            k, riders = what
            n = len(WGRAD16[k][0])
            want = {f"p{j}:dw" for j in range(n)} | {f"p{j}.rows" for j in range(n)} | {f"p{j}:dbias" for j in range(n if n == 1 else n - 1)}
            assert mine == want | ({f"rider{j}" for j in range(2 * len(RIDER_SHAPES))} if riders else set()), name
    assert all(any(k.startswith(name + ":") for name in RECORDS) for k in files)
    assert os.path.getsize(GOLDEN) < 1_000_000


@gpu
@pytest.mark.parametrize("name", list(RECORDS))
def test_bf16_bits_equal_the_build_before_bf16_tile_h(lin, name):
    """Every recorded array of this record, word for word."""
    assert_same_bits(unpack(GOLDEN), recorded(lin, name), name)


if __name__ == "__main__" and sys.argv[1:2] == ["record"]:
    record(RECORDS, recorded, sys.argv[2] if len(sys.argv) > 2 else GOLDEN)
