"""Evaluating a continual model and scanning a stage's labels, end to end on the device: utils.predict_volume(class_indices=...)
with the resizes and the class-list argmax on the device against the host path, continual.evaluate_tasks on the device against the
host metrics, and continual.scan_labels feeding extreme_class_weights.  The network is the tiny configuration of
tests/test_gpu_resize.py with 14 classes and closed-form weights.  Every device call is followed by a synchronize."""
import numpy as np
import pytest
import torch

from oracle.determ import det_normal, fill_state_dict
from seg_metrics_cases import blob_pair

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = dict(rel=1e-12, abs=1e-12)
VOL = (5, 64, 48)
KITS23 = [0, 9, 10, 11]


class _OneChannel(torch.nn.Module):          # CSwinUnet.forward: 1 -> 3 channels (vision_transformer.py:40-41)
    def __init__(self, m):
        super().__init__()
        self.m = m

    def forward(self, x):
        return self.m(x.repeat(1, 3, 1, 1))


@pytest.fixture(scope="module")
def net():
    import cswin_unet_amd.networks.cswin_unet as N
    m = N.CSWinTransformer(img_size=224, num_classes=14, embed_dim=64, depth=[1, 2, 9, 1], split_size=[1, 2, 7, 7],
                           num_heads=[2, 4, 8, 16], mlp_ratio=4., qkv_bias=True, drop_path_rate=0.).to(DEV)
    return _OneChannel(fill_state_dict(m)).eval()


def test_predict_volume_over_a_class_list_hip_equals_host(net):
    from cswin_unet_amd.utils import predict_volume
    vol = det_normal("resize.vol", VOL)          # on this volume the device zoom is scipy's bit for bit (tests/test_gpu_resize.py)
    host = predict_volume(vol, net, (224, 224), batch_slices=2, class_indices=KITS23)
    hip = predict_volume(vol, net, (224, 224), batch_slices=2, resize="hip", class_indices=KITS23)
    torch.cuda.synchronize()
    assert hip.shape == host.shape == VOL and hip.dtype == np.uint8
    assert host.max() <= 3 and len(np.unique(host)) > 1
    assert np.array_equal(hip, host)
    full = predict_volume(vol, net, (224, 224), batch_slices=2, resize="hip")
    torch.cuda.synchronize()
    assert full.max() > 3                        # what the argmax over all 14 channels gives: ids no 4-class label volume holds


def _loader(seed, ids):
    vol = det_normal(f"continual_eval.vol{seed}", VOL)
    lab = blob_pair(VOL, ids, seed)[1]
    return [{"image": torch.from_numpy(vol)[None], "label": torch.from_numpy(lab.astype(np.int64))[None], "case_name": f"case{seed}"}]


def test_evaluate_tasks_on_the_device_equals_the_host_metrics(net):
    from cswin_unet_amd import continual as C
    loaders = {1: _loader(41, [1, 2, 3]), 2: _loader(42, [1, 2])}
    host = C.evaluate_tasks(net, loaders, C.REFERENCE_STAGE_CLASSES, (224, 224), metrics="host", resize="host", batch_slices=2)
    hip = C.evaluate_tasks(net, loaders, C.REFERENCE_STAGE_CLASSES, (224, 224), metrics="hip", resize="hip", batch_slices=2)
    torch.cuda.synchronize()
    assert set(hip) == set(host) == {1, 2}
    for task, nfg in ((1, 3), (2, 2)):
        (pv_h, cm_h, d_h, h_h), (pv_g, cm_g, d_g, h_g) = host[task], hip[task]
        assert len(pv_g) == len(pv_h) == 1 and len(pv_g[0]) == len(pv_h[0]) == nfg and cm_g.shape == (nfg, 2)
        for c, (g, w) in enumerate(zip(pv_g[0], pv_h[0]), start=1):
            print(f"task {task} class {c}: hip {g} host {w}")
            assert g[0] == w[0], (task, c, g, w)
            assert g[1] == pytest.approx(w[1], **TOL), (task, c, g, w)
        assert d_g == d_h and h_g == pytest.approx(h_h, **TOL)


def test_a_12_class_model_is_refused_for_task_2_before_any_kernel_runs():
    from cswin_unet_amd import continual as C

    class Twelve(torch.nn.Module):
        num_classes = 12

        def forward(self, x):
            raise AssertionError("the network must not run")

    def unread():
        raise AssertionError("the loader must not be read")
        yield

    with pytest.raises(ValueError, match="lits17"):
        C.evaluate_tasks(Twelve(), {1: unread(), 2: unread()}, C.REFERENCE_STAGE_CLASSES, (224, 224), metrics="hip", resize="hip")


def _reference_class_weights(counts, active):
    """universal_train.py:1019-1030 restated in numpy float64 on given counts."""
    counts = np.asarray(counts, np.float64)
    w = np.zeros(len(counts))
    for c in active:
        if counts[c] > 0:
            w[c] = 1.0 / np.sqrt(counts[c] + 1e-6)
    s = sum(w[c] for c in active)
    if s > 0:
        for c in active:
            w[c] = w[c] / s * len(active)
    w[0] = min(w[0], 0.5)
    return w


def test_scan_labels_feeds_the_class_weights_and_the_sampler():
    from cswin_unet_amd import continual as C
    lab = blob_pair((40, 64, 48), [1, 2, 3], 23)[1]                     # a kits23-like stage: raw ids 0..3
    small = blob_pair((2, 32, 40), [1, 2], 24)[1]
    # as a dataset hands them over: single float32 slices (the .npz slices), an int16 block, a uint8 block, another shape last
    entries = [lab[i].astype(np.float32) for i in range(7)] + [lab[7:30].astype(np.int16), lab[30:40], small]
    table = C.new_label_map(9, 4)
    counts = C.scan_labels(entries, 12, label_map=table, batch=16, device=DEV)
    torch.cuda.synchronize()
    assert counts.dtype == torch.int64 and not counts.is_cuda and tuple(counts.shape) == (42, 13)
    mapped = table.numpy()[lab.reshape(40, -1)]
    want = np.stack([np.bincount(m, minlength=13) for m in mapped])
    assert np.array_equal(counts[:40].numpy(), want)
    assert np.array_equal(counts[40:].numpy(), np.stack([np.bincount(table.numpy()[s.ravel()], minlength=13) for s in small]))
    assert (counts[:40].sum(1) == 64 * 48).all() and (counts[40:].sum(1) == 32 * 40).all() and not counts[:, 12].any()

    total = counts[:40].sum(0)[:12]
    active = [0, 9, 10, 11]
    assert all(int(total[c]) > 0 for c in active)
    got = C.extreme_class_weights(total, active)
    ref = _reference_class_weights(total.numpy(), active)
    # both are float64 arithmetic on the same integers, rounded once to float32 (half an ulp: 6e-8 relative)
    assert np.allclose(got.numpy(), ref, rtol=1e-6, atol=0) and float(got[1:9].abs().sum()) == 0 and float(got[9:].min()) > 0

    raw = C.scan_labels(entries[:-1], 4, batch=16, device=DEV)
    presence = raw[:, :4] > 0
    assert np.array_equal(presence.numpy(), np.stack([np.isin(np.arange(4), np.unique(s)) for s in lab]))
    ds = C.PositiveSampling(list(range(40)), presence, C.KITS23_RULE)
    assert ds.class_indices[3] == [i for i in range(40) if (lab[i] == 3).any()] and len(ds.class_indices[3]) not in (0, 40)
