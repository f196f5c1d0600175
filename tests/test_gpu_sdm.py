"""cswin_signed_distance_maps on the device, called directly with guarded buffers and an exact-size workspace, against
utils.signed_distance_maps_host bit for bit at every shape of tests/sdm_cases.py: both sides of the 64-pixel row chunk, of a
column tile and of every step of the column tile's width, the tallest and the widest slice, organs, the far pixel, absent and
full classes, the class-count limits and out-of-range labels.  Then: two runs give the same bits, and refused calls touch nothing."""
import numpy as np
import pytest
import torch

import sdm_cases as S
from test_gpu_attn_shapes import Guarded, settle

gpu = pytest.mark.gpu
DEV = "cuda"
ERR_SHAPE, ERR_WORKSPACE, ERR_UNSUPPORTED = -1, -3, -5        # include/cswin_hip.h


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def run_maps(lab, ncls, what):
    """The entry point on guarded buffers; returns the maps (numpy) and the guarded outputs."""
    from cswin_unet_amd._lib import call, lib, ptr, stream
    B, H, W = lab.shape
    ld = torch.from_numpy(np.array(lab)).to(DEV)
    nbytes = lib().cswin_sdm_workspace(B, ncls, H, W)
    assert nbytes == ((B * ncls * 4 + 255) // 256 * 256 + B * ncls * H * W * 2 + 15) // 16 * 16
    o = dict(phi=Guarded((B, ncls, H, W)), workspace=Guarded((nbytes // 4,)))
    call("cswin_signed_distance_maps", ptr(ld), ptr(o["phi"].t), ptr(o["workspace"].t), nbytes, B, ncls, H, W, stream())
    settle(what, o)
    return o["phi"].t.cpu().numpy(), o


@gpu
@pytest.mark.parametrize("case", S.GPU_CASES, ids=[c[0] for c in S.GPU_CASES])
def test_maps_equal_the_host_definition_bit_for_bit(case):
    tag, B, ncls, H, W, kind = case
    lab, want = S.gpu_labels(tag), S.gpu_reference(tag)
    got, _ = run_maps(lab, ncls, f"sdm.{tag}")
    differ = int((got != want).sum())
    print(f"sdm.{tag}: {differ} of {want.size} elements differ; |phi| up to {float(np.abs(want).max()):.3f}")
    assert np.array_equal(bits(got), bits(want))                          # the sign of a zero included
    if kind in ("oor", "oor_coarse"):
        assert ((lab < 0) | (lab >= ncls)).sum() >= 3


@gpu
def test_two_runs_give_equal_bits_and_ops_is_the_entry_point():
    from cswin_unet_amd import ops
    tag = "organs224"
    lab, ncls = S.gpu_labels(tag), 9
    a, _ = run_maps(lab, ncls, "sdm.rerun.a")
    b, _ = run_maps(lab, ncls, "sdm.rerun.b")
    assert np.array_equal(bits(a), bits(b))
    ld = torch.from_numpy(np.array(lab)).to(DEV)
    c = ops.signed_distance_maps(ld, ncls)
    assert c.dtype == torch.float32 and tuple(c.shape) == (2, ncls, 224, 224)
    assert np.array_equal(bits(c.cpu().numpy()), bits(a))
    assert np.array_equal(ops.signed_distance_maps(ld.int(), ncls).cpu().numpy(), a)      # other integer labels are widened
    with pytest.raises(Exception):
        ops.signed_distance_maps(ld.cpu(), ncls)
    with pytest.raises(ValueError):
        ops.signed_distance_maps(ld[0], ncls)
    with pytest.raises(ValueError):
        ops.signed_distance_maps(ld, 256)


@gpu
def test_refusals_touch_nothing():
    from cswin_unet_amd._lib import lib, ptr, stream
    h = lib()
    B, ncls, H, W = 2, 4, 7, 13
    ld = torch.from_numpy(np.array(S.gpu_labels("oor"))).to(DEV)
    nbytes = h.cswin_sdm_workspace(B, ncls, H, W)
    # buffers large enough for whatever a refused shape would have written first
    big = 1 << 19
    o = dict(phi=Guarded((2, 4, 2048, 13)), workspace=Guarded((big // 4,)))

    def refused(code, what, *args):
        got = h.cswin_signed_distance_maps(*args)
        assert got == code, f"{what}: returned {got}, expected {code}"
        settle("refused " + what, o, untouched=True)

    phi, ws = ptr(o["phi"].t), ptr(o["workspace"].t)
    refused(ERR_WORKSPACE, "one byte short", ptr(ld), phi, ws, nbytes - 1, B, ncls, H, W, stream())
    refused(ERR_WORKSPACE, "null workspace", ptr(ld), phi, None, nbytes, B, ncls, H, W, stream())
    refused(ERR_SHAPE, "null labels", None, phi, ws, nbytes, B, ncls, H, W, stream())
    refused(ERR_SHAPE, "null phi", ptr(ld), None, ws, nbytes, B, ncls, H, W, stream())
    refused(ERR_SHAPE, "B = 0", ptr(ld), phi, ws, nbytes, 0, ncls, H, W, stream())
    for hh, ww in ((0, W), (H, 0), (2048, W), (H, 2048), (-1, W)):
        refused(ERR_SHAPE, f"H={hh} W={ww}", ptr(ld), phi, ws, big, B, ncls, hh, ww, stream())
        assert h.cswin_sdm_workspace(B, ncls, hh, ww) == 0
    for n in (1, 0, 256, -2):
        refused(ERR_UNSUPPORTED, f"ncls={n}", ptr(ld), phi, ws, big, B, n, H, W, stream())
        assert h.cswin_sdm_workspace(B, n, H, W) == 0
    assert b"sdm_workspace" in h.cswin_last_error()
    # and the same buffers take the accepted call afterwards
    from cswin_unet_amd._lib import call
    good = Guarded((B, ncls, H, W))
    call("cswin_signed_distance_maps", ptr(ld), ptr(good.t), ws, nbytes, B, ncls, H, W, stream())
    torch.cuda.synchronize()
    assert good.intact() and np.array_equal(good.t.cpu().numpy(), S.gpu_reference("oor"))
