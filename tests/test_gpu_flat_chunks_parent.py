"""The flat optimisers' kernels (csrc/adamw.hip, tpgm.hip, sgd.hip over csrc/flat_chunks.h) against the build before the chunk
walk, the block sum, the finalize steps, the clip coefficient and the Adam moment update were written once: that change moved no
load, no store and no rounding, so every output must equal the recorded one bit for bit (tests/golden/flat_chunks_parent.npz,
written by `PYTHONPATH=. python tests/test_gpu_flat_chunks_parent.py record` on that build).

One layout reaches every branch of the walk and both trips of the finalize kernels: tensors of 1, 3, 4, 5, 1023, 1027 and 16385
elements (below the 16-byte body, tails of 1 and 3, both sides of a workgroup's 256 x 4 elements, a second chunk of one element)
and one-element tensors up to 257 in all.  Pad words hold NaN in the inputs the chunked kernels must not read and sentinels in
everything written; cswin_sgd_flat, which walks the pad words on purpose, gets finite ones.  Only the C entry points and the
helpers of test_gpu_step_tail / test_adamw_host / test_tpgm_host are used, so this file runs unchanged on either build."""
import os
import sys
import types

import numpy as np
import pytest
import torch

from test_adamw_host import BETA1, BETA2, EPS, LRS, adamw_inputs, flat, slots
from test_gpu_step_tail import bits16, bits32, hip, put, release_inputs  # noqa: F401
from test_tpgm_host import EXCLUDED, HEAD, RATIO_CASES, case_setup, norms_ref, tpgm_inputs

gpu = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "flat_chunks_parent.npz")
NUMELS = (1, 3, 4, 5, 1023, 1027, 16385) + (1,) * 250
T = len(NUMELS)
TOTAL = slots(NUMELS)[1]
MULTS = (0.0, 1.0, 0.37)                 # per tensor, in turn: an exact 0 freezes p and its shadow
GRAD_SCALE, NORM = 0.5, 40.0             # the gradients' global norm after grad_scale: the clip at max_norm 1 is live
TPGM_LR = 0.05


def flat_dev(arrays, pad, dtype=torch.float32):
    return torch.from_numpy(flat(arrays, NUMELS, fill=pad)).to(DEV).to(dtype)


def filled(shape, value, dtype=torch.float32):
    return torch.full(shape, value, dtype=dtype, device=DEV)


def recorded_arrays(hip):
    """name -> uint32 / uint16 bit patterns of every output of the recorded sequences, in the order they ran."""
    from cswin_unet_amd.optim import chunk_table
    P, st, out = hip.ptr, hip.stream, {}
    rows, first = chunk_table(list(NUMELS), slots(NUMELS)[0])
    assert len(rows) == T + 1 and TOTAL == 20480
    chunks, first, nchunks = put(rows.view(np.int64).reshape(-1, 2)), put(first), len(rows)

    def keep(name, t):
        out[name] = (bits16 if t.dtype == torch.bfloat16 else bits32)(t).copy()

    # ---- AdamW: norms with and without p, three clipped steps with multipliers and the shadow, one step with neither -----------
    ps, gs = adamw_inputs("flat_chunks", NUMELS, norm=NORM / GRAD_SCALE)
    p, m, v = flat_dev(ps, 7.0), filled((TOTAL,), 0.0), filled((TOTAL,), 0.0)
    mask = torch.from_numpy(flat([np.ones(n, np.float32) for n in NUMELS], NUMELS)).to(DEV) != 0
    m[~mask], v[~mask] = -3.0, 5.0
    shadow = filled((TOTAL,), -3.0, torch.bfloat16)
    g = [flat_dev(x, float("nan")) for x in gs]
    mult = put(np.array([MULTS[t % 3] for t in range(T)], np.float32))
    lr_dev = put(np.array([LRS[0]], np.float32))
    tensor_sumsq, scalars = filled((T, 2), -1.0), filled((2,), -1.0)

    def sumsq(gk, with_p, name=None):
        partial = filled((nchunks, 2), -1.0)
        hip.call("cswin_chunk_sumsq", P(gk), P(p) if with_p else None, P(chunks), nchunks, P(partial), st())
        hip.call("cswin_norm_finalize", P(partial), P(first), T, GRAD_SCALE, 1.0, P(tensor_sumsq), P(scalars), st())
        if name:
            keep(f"adamw.{name}.partial", partial)
            keep(f"adamw.{name}.tensor_sumsq", tensor_sumsq)
            keep(f"adamw.{name}.scalars", scalars)

    def adamw(gk, step, clipped):
        hip.call("cswin_adamw_flat", P(p), P(gk), P(m), P(v), P(chunks), nchunks, P(lr_dev), P(mult) if clipped else None,
                 P(scalars) if clipped else None, BETA1, BETA2, EPS, 0.01, GRAD_SCALE, 1 - BETA1 ** step, 1 - BETA2 ** step,
                 P(shadow) if clipped else None, st())

    sumsq(g[0], False, "sumsq_g")
    sumsq(g[0], True, "sumsq_gp")
    for k in range(3):
        lr_dev.fill_(LRS[k])
        sumsq(g[k], False)
        adamw(g[k], k + 1, True)
    for name, t in (("p", p), ("m", m), ("v", v), ("shadow", shadow), ("tensor_sumsq", tensor_sumsq), ("scalars", scalars)):
        keep(f"adamw.step3.{name}", t)
    assert float(scalars[0]) > 10.0 and float(scalars[1]) < 0.1                  # the clip was live
    adamw(g[0], 4, False)
    for name, t in (("p", p), ("m", m), ("v", v)):
        keep(f"adamw.step4_plain.{name}", t)

    # ---- TPGM: statistics in l2 / l1 with and without g, the ratios, two updates, the projection copied and in place -----------
    thetas, anchors, tg = tpgm_inputs("flat_chunks", NUMELS, spread=0.5)
    gamma0, flags_host = case_setup(norms_ref(thetas, anchors, False))
    assert len(RATIO_CASES) == 6 and (flags_host & EXCLUDED).any() and (flags_host & HEAD).any()
    theta, anchor = flat_dev(thetas, 7.0), flat_dev(anchors, float("nan"))
    flags, gamma = put(flags_host), put(gamma0)
    gm, gv, ratio, norm, tscalars = (filled((T,), 0.0), filled((T,), 0.0), filled((T,), -1.0), filled((T,), -1.0), filled((2,), -1.0))
    tgrad = [flat_dev([(x * np.float32(40)).astype(np.float32) for x in gk], float("nan")) for gk in tg]

    def stats(gk, l1, name=None):
        partial = filled((nchunks, 2), -1.0)
        hip.call("cswin_tpgm_chunk_stats", P(theta), P(anchor), P(gk), P(chunks), nchunks, int(l1), P(partial), st())
        if name:
            keep(f"tpgm.{name}.partial", partial)
        return partial

    def finalize(partial, l1, mode, step, name):
        hip.call("cswin_tpgm_finalize", P(partial), P(first), T, int(l1), P(flags), P(gamma), P(gm), P(gv), GRAD_SCALE, TPGM_LR, 1 - 0.9 ** step,
                 1 - 0.999 ** step, mode, P(ratio), P(norm), P(tscalars), st())
        for n, t in (("gamma", gamma), ("gm", gm), ("gv", gv), ("ratio", ratio), ("norm", norm), ("scalars", tscalars)):
            keep(f"tpgm.{name}.{n}", t)

    for l1 in (False, True):
        tag = "l1" if l1 else "l2"
        stats(tgrad[0], l1, f"stats_{tag}_g")
        finalize(stats(None, l1, f"stats_{tag}"), l1, 0, 1, f"ratios_{tag}")
    for k in range(2):
        finalize(stats(tgrad[k], False), False, 1, k + 1, f"update{k + 1}")
    assert float(tscalars[1]) < 1.0                                              # the radii's clip was live
    r = ratio.cpu().numpy()
    assert (r == 1.0).any() and ((r > 0.0) & (r < 1.0)).any()                    # kept and moved tensors in the projection
    dst, dshadow = filled((TOTAL,), -5.0), filled((TOTAL,), -3.0, torch.bfloat16)
    hip.call("cswin_tpgm_project", P(theta), P(anchor), P(dst), P(ratio), P(chunks), nchunks, P(dshadow), st())
    keep("tpgm.project.dst", dst)
    keep("tpgm.project.shadow", dshadow)
    hip.call("cswin_tpgm_project", P(theta), P(anchor), P(theta), P(ratio), P(chunks), nchunks, None, st())
    keep("tpgm.project.inplace", theta)

    # ---- SGD over the whole buffer, pad words and a tail of three included; the bf16 wire ---------------------------------------
    sp, sm, sshadow = flat_dev(ps, 7.0), filled((TOTAL,), 0.0), filled((TOTAL,), -3.0, torch.bfloat16)
    sg = [flat_dev(x, 0.25) for x in gs[:2]]
    for k in range(2):
        hip.call("cswin_sgd_flat", P(sp), P(sg[k]), P(sm), TOTAL - 1, P(lr_dev), 0.9, 1e-4, GRAD_SCALE, P(sshadow), st())
    for name, t in (("p", sp), ("m", sm), ("shadow", sshadow)):
        keep(f"sgd.step2.{name}", t)
    src = sg[0]
    for n in (5, 1027):
        wire, back = filled((n + 3,), -3.0, torch.bfloat16), filled((n + 3,), -5.0)
        hip.call("cswin_pack_bf16_scaled", P(src), P(wire), n, 1.0 / 3.0, st())
        hip.call("cswin_unpack_bf16", P(wire), P(back), n, st())
        keep(f"wire.n{n}.packed", wire)
        keep(f"wire.n{n}.unpacked", back)
    torch.cuda.synchronize()
    return out


@gpu
def test_flat_chunks_bits_equal_the_build_before_the_shared_walk(hip):
    """Every recorded array, element for element."""
    want = np.load(GOLDEN)
    got = recorded_arrays(hip)
    assert sorted(want.files) == sorted(got)
    for name, a in got.items():
        ref = want[name]
        assert a.dtype == ref.dtype and a.shape == ref.shape, name
        if not np.array_equal(a, ref):
            k = int(np.flatnonzero(a.reshape(-1) != ref.reshape(-1))[0])
            raise AssertionError(f"{name}: {int((a != ref).sum())} of {ref.size} elements differ, the first at flat index {k}: "
                                 f"{int(a.reshape(-1)[k]):#x} for {int(ref.reshape(-1)[k]):#x}")


if __name__ == "__main__" and sys.argv[1:2] == ["record"]:
    from cswin_unet_amd import _lib
    dest = sys.argv[2] if len(sys.argv) > 2 else GOLDEN
    os.makedirs(os.path.dirname(dest), exist_ok=True)
    np.savez_compressed(dest, **recorded_arrays(types.SimpleNamespace(call=_lib.call, ptr=_lib.ptr, stream=_lib.stream)))
    print("wrote", dest, os.path.getsize(dest), "bytes")
