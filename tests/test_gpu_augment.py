"""Device augmentation of training batches (csrc/augment.hip and csrc/resize.hip behind ops.augment_batch, the "hip" mode of
trainer._Prefetcher and trainer_synapse) against the host path's own functions and the reference's outputs
(tests/golden/g9_augment.npz), on the inputs and under the criterion of tests/augment_cases.py: labels exactly, images within one
float32 ulp of scipy's (or 2**-50 * max|x|) with at most 1 in 1e5 of the elements at or above 2**-20 * max|x| not bit-equal.
Every device call is followed by a synchronize so that a failing step ends its test before anything else is enqueued."""
import logging
import random
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import augment_cases as A

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _augment(img, lab, params, size):
    from cswin_unet_amd import ops
    got_img, got_lab = ops.augment_batch(torch.from_numpy(img.copy()).to(DEV), torch.from_numpy(lab.copy()).to(DEV),
                                         torch.tensor(params, dtype=torch.int32), size)
    torch.cuda.synchronize()
    B = img.shape[0]
    assert got_img.dtype == torch.float32 and got_img.is_cuda and tuple(got_img.shape) == (B, 1) + tuple(size)
    assert got_lab.dtype == torch.int64 and got_lab.is_cuda and tuple(got_lab.shape) == (B,) + tuple(size)
    assert got_img.is_contiguous() and got_lab.is_contiguous()
    return got_img[:, 0].cpu().numpy(), got_lab.cpu().numpy()


@pytest.mark.parametrize("shape,size", A.BATCH_SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_augment_batch_equals_the_host_functions(shape, size):
    with_255 = shape == (40, 56)
    img, lab = A.batch14(shape, with_255)
    want_img, want_lab = A.host_batch14(shape, size, with_255)
    got_img, got_lab = _augment(img, lab, A.PARAMS14, size)
    assert (want_lab == 255).any() == with_255
    for b, p in enumerate(A.PARAMS14):
        assert np.array_equal(got_lab[b], want_lab[b]), (shape, p)
        A.check_image(got_img[b], want_img[b], float(np.abs(img[b]).max()), f"{shape} -> {size} {p}")


@pytest.mark.parametrize("side", [224, 512])
def test_augment_batch_equals_the_reference_outputs(side):
    """g9's inputs of one size as one batch (four at 224 x 224: no resize launch; eight at 512 x 512) against the fixture."""
    g = A.g9()
    ids = [i for i in range(A.G9_N) if A.g9_input(i)[0].shape == (side, side)]
    assert len(ids) == (4 if side == 224 else 8)
    img = np.stack([A.g9_input(i)[0] for i in ids])
    lab = np.stack([A.g9_input(i)[1] for i in ids]).astype(np.uint8)
    got_img, got_lab = _augment(img, lab, [A.g9_params(i) for i in ids], (224, 224))
    for b, i in enumerate(ids):
        assert np.array_equal(got_lab[b], g[f"lab{i}"].astype(np.int64)), i
        A.check_image(got_img[b], g[f"img{i}"][0], float(np.abs(img[b]).max()), f"g9 sample {i} {A.g9_params(i)}")


def _drain(train, lists, augment):
    from torch.utils.data import DataLoader
    from cswin_unet_amd.datasets import RandomGenerator, RawSliceParams, Synapse_dataset, collate_raw_slices
    from cswin_unet_amd.trainer import _Prefetcher
    hip = augment == "hip"
    ds = Synapse_dataset(train, lists, "train", transform=(RawSliceParams if hip else RandomGenerator)([224, 224]))
    loader = DataLoader(ds, batch_size=4, shuffle=False, num_workers=0, pin_memory=True, drop_last=True,
                        collate_fn=collate_raw_slices if hip else None)
    random.seed(7)
    np.random.seed(8)
    out = []
    for img, lab in _Prefetcher(loader, torch.device(DEV), augment, (224, 224)):
        torch.cuda.synchronize()
        assert img.dtype == torch.float32 and tuple(img.shape) == (4, 1, 224, 224)
        assert lab.dtype == torch.int64 and tuple(lab.shape) == (4, 224, 224)
        out.append((img.cpu().numpy(), lab.cpu().numpy()))
    return out


def test_prefetcher_hip_batches_equal_the_host_batches(tmp_path):
    from cswin_unet_amd.datasets import Synapse_dataset, write_synthetic_synapse
    from cswin_unet_amd.trainer import _Prefetcher
    train, _, lists = write_synthetic_synapse(str(tmp_path), size=256, n_slices=8, n_volumes=0)
    raw = Synapse_dataset(train, lists, "train")
    host, hip = _drain(train, lists, "host"), _drain(train, lists, "hip")
    assert len(host) == len(hip) == 2
    for n, ((himg, hlab), (dimg, dlab)) in enumerate(zip(host, hip)):
        assert np.array_equal(dlab, hlab), n
        for b in range(4):
            xmax = float(np.abs(raw[4 * n + b]["image"]).max())
            A.check_image(dimg[b, 0], himg[b, 0], xmax, f"batch {n} sample {b}")
    with pytest.raises(ValueError):
        _Prefetcher([], torch.device(DEV), "bogus")
    with pytest.raises(ValueError, match="output_size"):
        _Prefetcher([], torch.device(DEV), "hip")


def test_trainer_synapse_with_device_augmentation(tmp_path):
    """The settings of test_gpu_parity.test_trainer_synapse_on_synthetic_dataset with augment="hip"."""
    from cswin_unet_amd.config import get_config
    from cswin_unet_amd.datasets import write_synthetic_synapse
    from cswin_unet_amd.networks.vision_transformer import CSwinUnet
    from cswin_unet_amd.trainer import trainer_synapse
    train, _, lists = write_synthetic_synapse(str(tmp_path / "data"), n_slices=8, n_volumes=0, size=256)
    cfg = get_config(**{"MODEL.DROP_PATH_RATE": 0.0})
    torch.manual_seed(0)
    net = CSwinUnet(cfg, img_size=224, num_classes=9).to(DEV)
    args = SimpleNamespace(root_path=train, list_dir=lists, img_size=224, num_classes=9, batch_size=4, base_lr=0.05,
                           max_epochs=3, num_workers=0, seed=1234, augment="bogus")
    with pytest.raises(ValueError):
        trainer_synapse(args, net, str(tmp_path / "snap"))
    args.augment = "hip"
    records = []
    h = logging.Handler()
    h.emit = lambda r: records.append(r.getMessage())
    root = logging.getLogger()
    old_level = root.level
    root.setLevel(logging.INFO)
    root.addHandler(h)
    try:
        assert trainer_synapse(args, net, str(tmp_path / "snap")) == "Training Finished!"
    finally:
        root.removeHandler(h)
        root.setLevel(old_level)
    torch.cuda.synchronize()
    losses = [float(m.split("loss : ")[1].split(",")[0]) for m in records if m.startswith("iteration")]
    print("losses", losses)
    assert len(losses) == 6 and all(np.isfinite(losses)) and losses[-1] < losses[0]
    assert (tmp_path / "snap" / "epoch_2.pth").exists()


def test_bad_arguments_raise():
    from cswin_unet_amd import ops
    from cswin_unet_amd._lib import CswinHipError, call, ptr, stream
    img, lab = torch.zeros(2, 8, 8, device=DEV), torch.zeros(2, 8, 8, dtype=torch.uint8, device=DEV)
    par = torch.zeros(2, 4, dtype=torch.int32)
    for bad in ((img.cpu(), lab, par), (img, lab.cpu(), par), (img.double(), lab, par), (img, lab.long(), par),
                (img, lab[:1], par), (img[0], lab[0], par), (img, lab, par[:1]), (img, lab, par.float()),
                (torch.zeros(1, 2049, 8, device=DEV), torch.zeros(1, 2049, 8, dtype=torch.uint8, device=DEV), par[:1])):
        with pytest.raises(CswinHipError):
            ops.augment_batch(*bad, (4, 4))
    with pytest.raises(CswinHipError):
        ops.augment_batch(img, lab, par, (2049, 4))
    with pytest.raises(ValueError):
        ops.augment_batch(img, lab, torch.tensor([[3, 0, 0, 0], [0, 0, 0, 0]]), (4, 4))          # no such kind
    # the entry points themselves: a dimension above 2048, an output that is neither the slice's shape nor its transpose
    table, out, idx = torch.zeros(6, dtype=torch.int64, device=DEV), torch.zeros(2, 8, 8, device=DEV), torch.zeros(8, dtype=torch.int32, device=DEV)
    with pytest.raises(CswinHipError, match="1..2048"):
        call("cswin_augment_gather", ptr(img), ptr(out), ptr(table), 2, 2, 2049, 8, 2049, 8, stream())
    with pytest.raises(CswinHipError, match="transpose"):
        call("cswin_augment_gather", ptr(img), ptr(out), ptr(table), 2, 2, 8, 8, 8, 4, stream())
    with pytest.raises(CswinHipError, match="1..2048"):
        call("cswin_augment_labels", ptr(lab), ptr(out), ptr(table), ptr(idx), ptr(idx), ptr(idx), ptr(idx), 2, 2, 8, 8, 8, 2049, stream())
    with pytest.raises(CswinHipError, match="null"):
        call("cswin_augment_labels", ptr(lab), ptr(out), None, ptr(idx), ptr(idx), ptr(idx), ptr(idx), 2, 2, 8, 8, 8, 8, stream())
    torch.cuda.synchronize()


def test_strided_and_offset_views_equal_their_contiguous_copies():
    from cswin_unet_amd import ops
    shape, size = A.BATCH_SHAPES[1]
    img, lab = A.batch14(shape)
    par = torch.tensor(A.PARAMS14, dtype=torch.int32)
    dimg, dlab = torch.from_numpy(img.copy()).to(DEV), torch.from_numpy(lab.copy()).to(DEV)
    want = ops.augment_batch(dimg, dlab, par, size)
    torch.cuda.synchronize()
    flat_i, flat_l = torch.zeros(img.size + 1, device=DEV), torch.zeros(lab.size + 3, dtype=torch.uint8, device=DEV)
    flat_i[1:] = dimg.reshape(-1)                                                   # odd element offsets of the base pointers
    flat_l[3:] = dlab.reshape(-1)
    got = ops.augment_batch(flat_i[1:].view(*img.shape), flat_l[3:].view(*lab.shape), par, size)
    torch.cuda.synchronize()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    ti, tl = dimg.transpose(1, 2).contiguous().transpose(1, 2), dlab.transpose(1, 2).contiguous().transpose(1, 2)
    assert not ti.is_contiguous() and not tl.is_contiguous()
    got = ops.augment_batch(ti, tl, par, size)
    torch.cuda.synchronize()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
