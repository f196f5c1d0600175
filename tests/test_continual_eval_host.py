"""Host side of evaluating a continual model and of a stage's label statistics (cswin_unet_amd.continual, utils): the class lists
of universal_test.py, a checkpoint's task level, PositiveSampling's draw order against a restatement of the reference's rule,
scan_labels' refusals, and the class_indices argument of the volume loop on a stub network.  No GPU."""
import random

import numpy as np
import pytest
import torch

from cswin_unet_amd import continual as C
from cswin_unet_amd import ops
from cswin_unet_amd._lib import CswinHipError


def test_task_class_indices_are_the_reference_lists():
    assert C.REFERENCE_STAGE_CLASSES == (9, 4, 3) and C.REFERENCE_TASKS == {"synapse": 0, "kits23": 1, "lits17": 2}
    assert C.task_class_indices((9, 4, 3), 0) == [0, 1, 2, 3, 4, 5, 6, 7, 8]
    assert C.task_class_indices((9, 4, 3), 1) == [0, 9, 10, 11]
    assert C.task_class_indices((9, 4, 3), 2) == [0, 12, 13]
    # the general rule on another chain: offsets 5, 5 + (2 - 1) = 6
    assert C.task_class_indices((5, 2, 6), 0) == [0, 1, 2, 3, 4]
    assert C.task_class_indices((5, 2, 6), 1) == [0, 5]
    assert C.task_class_indices((5, 2, 6), 2) == [0, 6, 7, 8, 9, 10]
    for bad in (-1, 3):
        with pytest.raises(ValueError):
            C.task_class_indices((9, 4, 3), bad)


def test_task_level():
    assert [C.task_level(n, (9, 4, 3)) for n in (9, 12, 14)] == [1, 2, 3]
    with pytest.raises(ValueError, match="13"):
        C.task_level(13, (9, 4, 3))
    assert [C.task_level(n, (5, 2, 6)) for n in (5, 6, 11)] == [1, 2, 3]
    with pytest.raises(ValueError):
        C.task_level(10, (5, 2, 6))


def test_prefixes_and_checkpoint_class_count():
    w = torch.zeros(12, 64, 1, 1)
    plain = {"output.weight": w, "stage1.0.norm1.weight": torch.zeros(64)}
    for prefix in ("", "module.", "base_model.", "module.base_model.", "base_model.module."):
        sd = {prefix + k: v for k, v in plain.items()}
        stripped = C.strip_wrapper_prefixes(sd)
        assert set(stripped) == set(plain), prefix
        assert stripped["output.weight"] is w
        assert C.checkpoint_num_classes(sd) == 12, prefix
    wrapped = {"base_model.cswin_unet.output.weight": torch.zeros(14, 64, 1, 1), "base_model.cswin_unet.norm.bias": torch.zeros(3)}
    assert set(C.strip_wrapper_prefixes(wrapped)) == {"cswin_unet.output.weight", "cswin_unet.norm.bias"}
    assert C.checkpoint_num_classes(wrapped) == 14
    assert C.task_level(C.checkpoint_num_classes(wrapped), C.REFERENCE_STAGE_CLASSES) == 3
    # no output.weight: an error, not the reference's guess among every key that contains "output"
    with pytest.raises(KeyError):
        C.checkpoint_num_classes({"module.my_output_head.weight": torch.zeros(9, 64, 1, 1)})
    # a prefix in the middle of a key is no wrapper prefix
    assert set(C.strip_wrapper_prefixes({"stage1.module.weight": w})) == {"stage1.module.weight"}


class _Toy(torch.utils.data.Dataset):
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        assert 0 <= i < self.n
        return ("sample", i)


def _reference_draw(idx, n, rule, lists, positive_ratio):
    """PositiveSamplingDataset.__getitem__ (universal_train.py:220-241) for a rule given as a list: an if / elif chain whose
    conditions are `random.random() < p and lists[c]`, so every condition that is reached draws, whatever its list holds."""
    for p, c in rule:
        p = positive_ratio if p is None else p
        if random.random() < p and lists[c]:
            return random.choice(lists[c])
    return idx % n


@pytest.mark.parametrize("rule,ratio", [(C.KITS23_RULE, 0.8), (C.LITS17_RULE, 0.8), ([(0.9, 3), (0.9, 2), (None, 1)], 0.35)],
                         ids=["kits23", "lits17", "empty-first"])
def test_positive_sampling_has_the_reference_draw_order(rule, ratio):
    n = 23
    presence = np.zeros((n, 4), bool)
    presence[:, 0] = True
    presence[[2, 3, 5, 7, 11, 13], 1] = True
    presence[[5, 19], 2] = True
    if rule is C.KITS23_RULE:
        presence[[13], 3] = True                     # in "empty-first" class 3 stays empty: its draw happens and fails
    lists = {c: np.flatnonzero(presence[:, c]).tolist() for c in range(4)}
    ds = C.PositiveSampling(_Toy(n), presence, rule, positive_ratio=ratio)
    assert len(ds) == n
    assert ds.class_indices == {c: lists[c] for _, c in rule}
    order = [(7 * k) % (3 * n) for k in range(400)]              # indices beyond len: the fallback is idx % len
    random.seed(1234)
    got = [ds[i] for i in order]
    state_after = random.getstate()
    random.seed(1234)
    want = [("sample", _reference_draw(i, n, rule, lists, ratio)) for i in order]
    assert got == want
    assert random.getstate() == state_after                      # the same number of draws was consumed
    picked = {g[1] for g in got}
    assert len(picked) > 3 and any(g[1] == i % n for g, i in zip(got, order))
    if len(rule) == 3 and rule is not C.KITS23_RULE:
        # with the empty class's draw skipped, the stream shifts and the sequence changes: the order is visible
        random.seed(1234)
        skipping = [("sample", _reference_draw(i, n, rule[1:], lists, ratio)) for i in order]
        assert skipping != want


def test_positive_sampling_refuses_a_table_of_another_length():
    with pytest.raises(ValueError):
        C.PositiveSampling(_Toy(5), np.zeros((4, 4), bool), C.KITS23_RULE)
    with pytest.raises(ValueError):
        C.PositiveSampling(_Toy(5), np.zeros((5, 3), bool), C.KITS23_RULE)          # the rule names class 3


def test_scan_labels_refuses_bad_values_before_any_upload():
    ok = np.zeros((4, 6), np.float32)
    for bad, what in ((256, "256"), (-1, "-1"), (1.5, "1.5"), (np.nan, "nan")):
        a = ok.astype(np.float64 if isinstance(bad, float) else np.int64)
        a[2, 3] = bad
        with pytest.raises(ValueError, match="entry 1"):
            C.scan_labels([ok, a], 4, device="cpu")                # raised while entry 1 is read: nothing has been sent anywhere
    with pytest.raises(ValueError):
        C.scan_labels([np.zeros((2, 3, 4, 5), np.uint8)], 4, device="cpu")
    with pytest.raises(CswinHipError):
        C.scan_labels([ok], 4, device="cpu")                       # valid labels reach ops.class_counts, which has no CPU path


def test_new_ops_have_no_cpu_fallback():
    with pytest.raises(CswinHipError):
        ops.argmax_zoom_back(torch.zeros(1, 14, 4, 4), (8, 8), classes=[0, 9, 10, 11])
    with pytest.raises(CswinHipError):
        ops.class_counts(torch.zeros(2, 4, 4, dtype=torch.uint8), 9)
    with pytest.raises(CswinHipError):
        ops.class_counts(torch.zeros(2, 4, 4, dtype=torch.int64), 9, label_map=torch.zeros(3, dtype=torch.int32))
    assert "class_counts" in ops.__all__


class _Stub(torch.nn.Module):
    """14 fixed "logit" planes: channel c of pixel (i, j) is a hash of (c, i, j, the input's value there)."""
    num_classes = 14

    def forward(self, x):
        B, _, H, W = x.shape
        g = torch.Generator().manual_seed(5)
        base = torch.randn(14, H, W, generator=g)
        return base[None] * (1.0 + x) + torch.roll(base, 3, dims=0)[None]


def test_predict_volume_host_takes_the_argmax_over_the_listed_channels():
    from cswin_unet_amd.utils import predict_volume, test_single_volume
    net = _Stub()
    vol = np.random.default_rng(3).standard_normal((5, 16, 12)).astype(np.float32)
    x = torch.from_numpy(vol).unsqueeze(1)
    full = torch.argmax(net(x), 1).numpy()
    for idx in ([0, 9, 10, 11], [0, 12, 13], [11, 0, 9]):
        got = predict_volume(vol, net, (16, 12), batch_slices=2, device="cpu", class_indices=idx)
        assert got.shape == vol.shape
        assert np.array_equal(got, torch.argmax(net(x)[:, idx], 1).numpy()), idx
        assert got.max() < len(idx)
    assert np.array_equal(predict_volume(vol, net, (16, 12), batch_slices=2, device="cpu"), full)
    assert np.array_equal(predict_volume(vol, net, (16, 12), batch_slices=2, device="cpu", class_indices=list(range(14))), full)
    assert full.max() > 3                                                     # what a 4-class label volume cannot be scored against
    image, label = torch.from_numpy(vol)[None], torch.zeros((1,) + vol.shape, dtype=torch.int64)
    with pytest.raises(ValueError, match="class_indices"):
        test_single_volume(image, label, net, classes=4, patch_size=[16, 12], device="cpu", class_indices=[0, 12, 13])
    label[0, :, 4:9, 3:8] = 2
    m = test_single_volume(image, label, net, classes=4, patch_size=[16, 12], device="cpu", class_indices=[0, 9, 10, 11])
    assert len(m) == 3


def test_evaluate_tasks_refuses_an_unlearned_task_before_anything_runs():
    class Twelve(torch.nn.Module):
        num_classes = 12

        def forward(self, x):
            raise AssertionError("the network must not run")

    def loader():
        raise AssertionError("the loader must not be read")
        yield

    with pytest.raises(ValueError, match="lits17"):
        C.evaluate_tasks(Twelve(), {0: loader(), 2: loader()}, C.REFERENCE_STAGE_CLASSES, (16, 12), device="cpu")
    with pytest.raises(ValueError, match="task 2"):
        C.evaluate_tasks(Twelve(), {2: loader()}, (9, 4, 3, 2), (16, 12), device="cpu", num_classes=12)
