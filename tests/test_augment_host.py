"""Host side of the device augmentation (augment="hip"), without a GPU: the tables taken from scipy (utils.rotation_index), the
quarter-turn / flip index rule the kernels use (augment_cases.source_index), the RNG contract of datasets.RawSliceParams against
RandomGenerator, and the numpy emulation of the whole device pipeline against the reference's own outputs
(tests/golden/g9_augment.npz) under the criterion stated in tests/augment_cases.py."""
import random

import numpy as np
import pytest
import torch
from scipy import ndimage

import augment_cases as A

SHAPES = [(40, 56), (37, 53), (64, 64)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_rotation_index_gather_equals_scipy_rotate(shape):
    from cswin_unet_amd.utils import rotation_index
    H, W = shape
    rng = np.random.default_rng(H * 100 + W)
    img = rng.standard_normal(shape).astype(np.float32)
    lab = rng.integers(0, 256, size=shape).astype(np.uint8)
    holes = 0
    for angle in range(-20, 20):
        m = rotation_index(H, W, angle)
        assert m.dtype == np.int32 and m.shape == shape and m.min() >= -1 and m.max() < H * W and not m.flags.writeable
        assert rotation_index(H, W, angle) is m                                              # cached
        for x in (img, lab):
            want = ndimage.rotate(x, angle, order=0, reshape=False)
            got = A.gather(x, m)
            assert got.dtype == want.dtype and np.array_equal(got.view(np.uint8), want.view(np.uint8)), (shape, angle, x.dtype)
        holes = max(holes, int((m < 0).sum()))
    assert holes > 0                                                                         # scipy's constant occurs
    assert np.array_equal(rotation_index(H, W, 0), np.arange(H * W).reshape(H, W))


def test_rotation_index_bad_arguments_raise():
    from cswin_unet_amd.utils import rotation_index
    for bad in ((0, 8, 3), (8, 0, 3), (-1, 8, 3), (8, 2049, 3), (8, 8, 2.5)):
        with pytest.raises(ValueError):
            rotation_index(*bad)


@pytest.mark.parametrize("k,axis", [(k, a) for k in range(4) for a in range(2)])
def test_quarter_turn_and_flip_index_rule_equals_numpy(k, axis):
    H, W = 5, 7
    x = np.arange(H * W, dtype=np.float32).reshape(H, W) * 0.5 + 1
    want = np.flip(np.rot90(x, k), axis)
    src = A.source_index(H, W, A.ROT90_FLIP, k, axis, 0)
    assert src.shape == want.shape == ((W, H) if k % 2 else (H, W))
    assert np.array_equal(A.gather(x, src), want)
    assert sorted(src.ravel().tolist()) == list(range(H * W))                                # a permutation of the pixels


def test_raw_slice_params_consumes_both_rngs_like_random_generator():
    from cswin_unet_amd.datasets import RandomGenerator, RawSliceParams
    host, raw = RandomGenerator([224, 224]), RawSliceParams([224, 224])
    kinds = set()
    for i in range(A.G9_N):
        img, lab = A.g9_input(i)
        A.g9_seed(i)
        host({"image": img, "label": lab})
        after_host = (random.random(), int(np.random.randint(0, 1 << 30)))
        A.g9_seed(i)
        out = raw({"image": img.copy(), "label": lab})
        assert (random.random(), int(np.random.randint(0, 1 << 30))) == after_host, i
        assert out["image"].dtype == torch.float32 and np.array_equal(out["image"].numpy(), img)
        assert out["label"].dtype == torch.uint8 and np.array_equal(out["label"].numpy(), lab)
        assert out["params"].dtype == torch.int32 and out["params"].shape == (4,)
        kind, k, axis, angle = out["params"].tolist()
        # the branch and the values, drawn by hand in RandomGenerator's order
        A.g9_seed(i)
        if random.random() > 0.5:
            want = (A.ROT90_FLIP, np.random.randint(0, 4), np.random.randint(0, 2), 0)
        elif random.random() > 0.5:
            want = (A.ROTATE, 0, 0, np.random.randint(-20, 20))
        else:
            want = (A.NONE, 0, 0, 0)
        assert (kind, k, axis, angle) == want == A.g9_params(i), i
        kinds.add(kind)
    assert kinds == {A.NONE, A.ROT90_FLIP, A.ROTATE}


def test_emulated_device_pipeline_meets_the_criterion_on_the_reference_outputs():
    g = A.g9()
    for i in range(A.G9_N):
        img, lab = A.g9_input(i)
        got_img, got_lab = A.emulate(img, lab.astype(np.uint8), A.g9_params(i), (224, 224))
        assert np.array_equal(got_lab, g[f"lab{i}"].astype(np.int64)), i
        A.check_image(got_img, g[f"img{i}"][0], float(np.abs(img).max()), f"g9 sample {i} {A.g9_params(i)}")


def test_emulation_equals_the_host_functions_on_the_batch_cases():
    """The 14-sample batches of the GPU test through the emulation: the index rule, both shape groups and the fused label zoom."""
    for shape, size in A.BATCH_SHAPES:
        img, lab = A.batch14(shape, with_255=shape == (40, 56))
        assert (lab == 255).any() == (shape == (40, 56)) and len(np.unique(lab[lab < 255])) == 9
        want_img, want_lab = A.host_batch14(shape, size, shape == (40, 56))
        for b, p in enumerate(A.PARAMS14):
            got_img, got_lab = A.emulate(img[b], lab[b], p, size)
            assert np.array_equal(got_lab, want_lab[b]), (shape, p)
            A.check_image(got_img, want_img[b], float(np.abs(img[b]).max()), f"{shape} -> {size} {p}")


def test_raw_slice_params_refuses_what_the_device_path_does_not_take():
    from cswin_unet_amd.datasets import RawSliceParams
    raw = RawSliceParams([224, 224])
    img, lab = np.zeros((8, 8), np.float32), np.ones((8, 8), np.float32)
    assert raw({"image": img, "label": lab})["label"].dtype == torch.uint8
    for bad_img in (img.astype(np.float64), img.astype(np.int16)):
        with pytest.raises(ValueError, match='augment="host"'):
            raw({"image": bad_img, "label": lab})
    for bad_lab in (lab * 0.5, lab - 2, lab + 255):
        with pytest.raises(ValueError, match='augment="host"'):
            raw({"image": img, "label": bad_lab})


def test_collate_raw_slices_refuses_mixed_shapes():
    from cswin_unet_amd.datasets import RawSliceParams, collate_raw_slices
    raw = RawSliceParams([224, 224])
    a = raw({"image": np.zeros((8, 8), np.float32), "label": np.zeros((8, 8), np.float32)})
    b = raw({"image": np.zeros((8, 12), np.float32), "label": np.zeros((8, 12), np.float32)})
    batch = collate_raw_slices([a, dict(a)])
    assert batch["image"].shape == (2, 8, 8) and batch["label"].dtype == torch.uint8 and batch["params"].shape == (2, 4)
    with pytest.raises(ValueError, match=r"\(8, 8\).*\(8, 12\)"):
        collate_raw_slices([a, b])


def test_augment_batch_refuses_cpu_tensors():
    from cswin_unet_amd import ops
    from cswin_unet_amd._lib import CswinHipError
    with pytest.raises(CswinHipError):
        ops.augment_batch(torch.zeros(2, 8, 8), torch.zeros(2, 8, 8, dtype=torch.uint8), torch.zeros(2, 4, dtype=torch.int32), (4, 4))
