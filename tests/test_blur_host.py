"""Host side of the Gaussian-blurred data path (no GPU): utils.gaussian_taps against scipy's impulse response, the reflect
rule, the numpy emulation of csrc/blur.hip against scipy.ndimage.gaussian_filter on the inputs of tests/test_gpu_blur.py (bit
for bit: the precondition of the cap that test holds the device to), and blur_sigma through RandomGenerator, predict_volume,
test_single_volume and evaluate_volumes.  Then what tests/test_gpu_blur_shapes.py rests on: the Python transcription of the
kernel's tile plan against csrc/blur_plan.h itself (tools/blur_plan_check.cpp), the plan's invariants, the case table against
every plan signature and kernel branch, the emulation on the new cases and value classes, and four wrong emulations that the
table's inputs tell from scipy."""
import math
import os
import random
import shutil
import subprocess

import numpy as np
import pytest
import torch
from scipy.ndimage import gaussian_filter, gaussian_filter1d

import blur_cases as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sigma", [0.1, 0.5, 1, 1.7, 3, 8])
def test_gaussian_taps_are_scipys_impulse_response(sigma):
    from cswin_unet_amd.utils import gaussian_taps
    w, r = gaussian_taps(sigma)
    assert r == int(4.0 * sigma + 0.5) and w.shape == (2 * r + 1,) and w.dtype == np.float64
    assert np.array_equal(w, w[::-1])
    assert not w.flags.writeable and gaussian_taps(sigma)[0] is w
    impulse = np.zeros(4 * r + 3)
    impulse[2 * r + 1] = 1.0
    resp = gaussian_filter1d(impulse, sigma)
    assert np.array_equal(resp[r + 1:3 * r + 2], w)
    assert not resp[:r + 1].any() and not resp[3 * r + 2:].any()          # the window holds the whole response
    w2, r2 = gaussian_taps(sigma, truncate=2.0)
    assert r2 == int(2.0 * sigma + 0.5) and w2.shape == (2 * r2 + 1,)


@pytest.mark.parametrize("sigma", [0, -1, float("nan"), float("inf"), 9])
def test_gaussian_taps_refuse(sigma):
    from cswin_unet_amd.utils import gaussian_taps
    with pytest.raises(ValueError):
        gaussian_taps(sigma)


@pytest.mark.parametrize("n", [1, 2, 3, 7])
def test_reflect_rule_is_numpys_symmetric_padding(n):
    pad = 32
    want = np.pad(np.arange(n), pad, mode="symmetric")
    assert np.array_equal(B.reflect_index(np.arange(-pad, n + pad), n), want)


@pytest.mark.parametrize("shape,sigma", B.GPU_CASES, ids=B.case_id)
def test_emulation_is_bit_equal_to_scipy(shape, sigma):
    x = B.slices(shape, sigma)
    unequal = B.unequal_bits(B.emulate(x, sigma), B.scipy_blur_case(shape, sigma))
    print(f"{shape} sigma {sigma}: {unequal} of {x.size} elements not bit-equal")
    assert unequal == 0


# ---- what tests/test_gpu_blur_shapes.py rests on --------------------------------------------------------------------------------
SWEEP_H = (1, 3, 4, 5, 31, 32, 33, 2048)                    # the transcription sweep: W = 1..2048 x r = 0..32 x these x both widths
COVER_H = tuple(range(1, 45)) + (65, 100, 130, 2048)        # the signature sweep: the same W and r at these heights


def _grid(heights):
    """(H, W, r, vec) arrays of every legal combination of the sweep (vec = 2 needs an even W)."""
    h, w, r, vec = np.meshgrid(np.array(heights), np.arange(1, 2049), np.arange(33), np.array([1, 2]), indexing="ij")
    keep = (vec == 1) | (w % 2 == 0)
    return h[keep], w[keep], r[keep], vec[keep]


@pytest.fixture(scope="module")
def plan_tool(tmp_path_factory):
    """tools/blur_plan_check.cpp, compiled with the system C++ compiler: (H, W, r, vec) rows -> the header's plans."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("blur_plan") / "blur_plan_check")
    subprocess.run([cxx, "-O1", "-std=c++17", "-I", os.path.join(ROOT, "cswin_unet_amd", "csrc"),
                    os.path.join(ROOT, "tools", "blur_plan_check.cpp"), "-o", exe], check=True)

    def run(rows):
        text = "".join("%d %d %d %d\n" % tuple(row) for row in rows)
        out = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        got = np.array(out.stdout.split(), np.int64).reshape(-1, 4)
        assert len(got) == len(rows)
        return got
    return run


def _table_rows():
    rows = [(s[1], s[2], B.sigma_radius(sig), 2 if s[2] % 2 == 0 else 1) for s, sig in B.GPU_CASES]
    rows += [(s[1], s[2], B.sigma_radius(sig), 1) for s, sig in B.GPU_CASES]
    rows += [(s[1], s[2], r, B.plan_vec((s, r, off))) for s, r, off in B.PLAN_CASES]
    return rows


def test_plan_transcription_equals_the_header(plan_tool):
    h, w, r, vec = _grid(SWEEP_H)
    rows = np.concatenate([np.array(_table_rows()), np.stack([h, w, r, vec], 1)])
    got = plan_tool(rows)
    p = B.blur_plan(rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3])
    lds = 4 * (p.TR * rows[:, 1] + (p.TR + 2 * rows[:, 2]) * (1 << p.cw_log2))
    want = np.stack([p.TR, p.cw_log2, p.budget, lds], 1)
    bad = np.flatnonzero((got != want).any(1))
    print(f"{len(rows)} plans compared, {len(bad)} differ")
    assert len(bad) == 0, (rows[bad[0]], got[bad[0]], want[bad[0]])
    one = B.blur_plan(37, 600, 4, 2)                                      # the scalar form is the array form
    assert isinstance(one.TR, int) and (one.TR, one.cw_log2, one.budget, one.row_halvings, B.TR_SOURCES[one.source]) == (8, 6, 0, 3, "rows")


def test_plan_invariants_on_the_sweep():
    h, w, r, vec = _grid(SWEEP_H)
    p = B.blur_plan(h, w, r, vec)
    lds = 4 * (p.TR * w + (p.TR + 2 * r) * (1 << p.cw_log2))
    print(f"{len(h)} plans: TR {p.TR.min()}..{p.TR.max()}, chunk 2^{p.cw_log2.min()}..2^{p.cw_log2.max()}, largest LDS {lds.max()} bytes")
    assert (p.budget >= 0).all()                                          # a plan always exists
    assert (p.TR % 4 == 0).all() and p.TR.min() >= 4 and p.TR.max() <= 32
    assert lds.max() <= 65536
    assert (lds <= 4 * np.array(B.BL_BUDGETS)[p.budget]).all()            # and within the budget it was found in
    assert ((1 << p.cw_log2) <= 256 * vec).all() and (p.cw_log2 >= 6).all()
    assert ((p.TR + 2 * r) * (1 << p.cw_log2) * 4 + p.TR * w * 4 == lds).all()


def _signatures(h, w, r, vec):
    p = B.blur_plan(h, w, r, vec)
    fields = (vec, p.budget, p.cw_log2, (p.row_halvings > 0).astype(np.int64), p.source)      # every one of them in 0..15
    key = np.unique(sum(f << (4 * n) for n, f in enumerate(fields)))
    return {tuple(int(k >> (4 * n)) & 15 for n in range(5)) for k in key}


def test_plan_cases_reach_every_signature_of_the_sweep():
    reached = _signatures(*_grid(COVER_H))
    facts = [B.launch_facts(s, r, B.plan_vec((s, r, off))) for s, r, off in B.PLAN_CASES]
    have = {tuple(int(v) for v in f["signature"]) for f in facts}
    old = {tuple(int(v) for v in B.launch_facts(s, B.sigma_radius(sig), 2 if s[2] % 2 == 0 else 1)["signature"]) for s, sig in B.GPU_CASES}
    print(f"the sweep reaches {len(reached)} plan signatures, PLAN_CASES {len(have & reached)} of them, GPU_CASES {len(old & reached)}")
    print(f"PLAN_CASES: {len(B.PLAN_CASES)} cases, {sum(math.prod(s) for s, _, _ in B.PLAN_CASES)} elements")
    assert reached - have == set(), sorted(reached - have)
    assert have - reached == set()
    assert len(reached) >= 38
    assert {k[2] for k in have} == {6, 7, 8, 9} and {k[1] for k in have} == {0, 1, 2}
    assert all(math.prod(s) < 100000 for s, _, _ in B.PLAN_CASES)         # the 1-in-1e5 cap means 0 unequal on every case
    assert len({B.plan_case_id(c) for c in B.PLAN_CASES}) == len(B.PLAN_CASES)


def test_plan_cases_reach_every_kernel_branch():
    cases = [(s, r, B.launch_facts(s, r, B.plan_vec((s, r, off)))) for s, r, off in B.PLAN_CASES]
    assert all(s[0] == 2 for s, _, _ in cases)                            # the slice stride is checked everywhere
    for vec in (1, 2):
        mine = [(s, r, f) for s, r, f in cases if f["vec"] == vec]
        has = lambda cond: any(cond(s, r, f) for s, r, f in mine)
        for last in (1, 2, 3):                                            # a last tile of 1, 2, 3 rows behind a full one
            assert has(lambda s, r, f: f["tiles"] >= 2 and f["last_rows"] == last), (vec, last)
        assert has(lambda s, r, f: f["tiles"] >= 2 and f["last_mod4"] == 0), vec
        assert has(lambda s, r, f: f["tiles"] >= 2 and f["last_rows"] > 4 and f["last_mod4"]), vec      # 4k + m
        assert has(lambda s, r, f: f["tiles"] >= 3), vec
        assert has(lambda s, r, f: f["chunks"] == 1), vec
        assert has(lambda s, r, f: f["chunks"] >= 2 and f["w_rem"]), vec
        assert has(lambda s, r, f: f["stage_under_256"]), vec
        assert has(lambda s, r, f: f["row_under_256"]), vec
        assert has(lambda s, r, f: f["last_items"]["column"] < 256), vec
        assert has(lambda s, r, f: r == 0), vec
        assert has(lambda s, r, f: f["template"] and f["tiles"] >= 2 and f["chunks"] >= 2), vec
        assert has(lambda s, r, f: not f["template"] and r > 0 and f["tiles"] >= 2 and f["chunks"] >= 2), vec
        assert has(lambda s, r, f: s[1] in (1, 2, 3) and r >= 2 * s[1]), vec               # more than one reflection period in H
        assert has(lambda s, r, f: s[2] in (1, 2, 3) and r >= 2 * s[2]), vec               # and in W
        assert has(lambda s, r, f: f["template"] and s[1] in (1, 2, 3) and s[2] in (1, 2, 3) and r >= 2 * s[1] and r >= 2 * s[2]), vec
        assert has(lambda s, r, f: f["plan"].budget == 1 and f["chunks"] >= 2 and f["tiles"] >= 2), vec
        assert has(lambda s, r, f: f["plan"].budget == 2 and f["chunks"] >= 2 and f["tiles"] >= 2), vec
    assert any(f["chunks"] >= 2 and f["w_rem"] == 0 for _, _, f in cases)
    # the 4-byte loads at an even W: several chunks and tiles, the template, the 64 KiB budget
    odd = [(s, r, f) for s, r, f in cases if f["vec"] == 1 and s[2] % 2 == 0]
    assert any(f["template"] and f["tiles"] >= 2 and f["chunks"] >= 2 for _, _, f in odd)
    assert any(f["plan"].budget == 2 and f["tiles"] >= 2 for _, _, f in odd)
    assert (2, 5, 2048) in [s for s, _, _ in cases]                       # the widest slice


def test_launch_facts_of_a_case_worked_by_hand():
    """(1, 37, 600) at r = 4, 8-byte loads: the chunk is halved 512 -> 64 (rows() = 1, 4, 7, 8 against 4r = 16), TR = 8: five
    tiles, the last of 5 rows; ten chunks, the last of 24 columns; 16 x 32 stage items, 2 x 600 row-pass items."""
    f = B.launch_facts((1, 37, 600), 4, 2)
    assert (f["plan"].TR, f["plan"].cw_log2, f["plan"].w_halvings, f["plan"].row_halvings) == (8, 6, 0, 3)
    assert (f["tiles"], f["last_rows"], f["last_mod4"], f["chunks"], f["w_rem"]) == (5, 5, 1, 10, 24)
    assert f["first_items"] == dict(stage=16 * 32, column=2 * 64, row=2 * 600) and f["last_items"] == dict(stage=13 * 32, column=128, row=1200)
    assert f["template"] and f["lds_bytes"] == 4 * (8 * 600 + 16 * 64) and f["grid"] == (5, 1)
    assert all(B.launch_facts(s, B.sigma_radius(sig), 2 if s[2] % 2 == 0 else 1)["plan"].cw_log2 == 6 for s, sig in B.GPU_CASES)


@pytest.mark.parametrize("case", B.PLAN_CASES, ids=B.plan_case_id)
def test_emulation_is_bit_equal_to_scipy_on_the_plan_cases(case):
    x, want = B.plan_inputs(case)
    assert B.sigma_radius(B.sigma_of(case[1])) == case[1]
    unequal = B.unequal_bits(B.emulate(x, B.sigma_of(case[1])), want)
    print(f"{B.plan_case_id(case)}: {unequal} of {x.size} elements not bit-equal")
    assert unequal == 0 and np.isfinite(want).all()
    assert not np.array_equal(x[0], x[1])                                 # the two slices differ


@pytest.mark.parametrize("r", B.SPECIAL_RADII)
@pytest.mark.parametrize("name", B.SPECIAL_NAMES)
def test_emulation_is_bit_equal_to_scipy_on_the_special_values(name, r):
    x, tiny = B.special_input(name), np.float32(1.1754944e-38)
    want = B.scipy_blur_quiet(x, B.sigma_of(r))
    unequal = B.unequal_bits_or_nan(B.emulate(x, B.sigma_of(r)), want)
    sub = lambda a: int(((np.abs(a) < tiny) & (a != 0)).sum())
    print(f"{name} r {r}: {unequal} of {x.size} unequal; results: {sub(want)} subnormal, {int(np.isinf(want).sum())} inf, "
          f"{int(np.isnan(want).sum())} NaN, {int((np.signbit(want) & (want == 0)).sum())} -0.0")
    assert unequal == 0
    # the input is of the class its name says, so a device that treats the class otherwise has something to get wrong
    if name == "subnormal_inputs":
        assert (np.abs(x) < tiny).all() and sub(x) > x.size * 0.9 and sub(want) > x.size * 0.9
    elif name == "subnormal_results":
        assert sub(want) > 1000 and int((np.abs(want) >= tiny).sum()) > 1000 and sub(x) < sub(want)
    elif name == "near_overflow":
        assert np.isinf(want).sum() > np.isinf(x).sum() > 0 and not np.isnan(want).any()
        assert float(np.abs(want[np.isfinite(want)]).max()) > 1e37
    elif name == "signed_zeros":
        neg = np.signbit(want) & (want == 0)
        assert (want == 0).all() and 0 < neg.sum() < want.size and np.signbit(x).sum() > neg.sum()
    else:
        assert np.isnan(want).sum() > np.isnan(x).sum() and (want == np.inf).any() and (want == -np.inf).any()
        assert np.isfinite(want).sum() > want.size // 2


@pytest.mark.parametrize("r", B.NAN_RADII)
def test_emulation_has_scipys_nan_footprint(r):
    for name, at in B.nan_positions(r):
        x = B.nan_input(r, at)
        want = B.scipy_blur_quiet(x, B.sigma_of(r))
        n = int(np.isnan(want).sum())
        print(f"r {r} NaN at {name} {at}: {n} NaN results")
        assert B.unequal_bits_or_nan(B.emulate(x, B.sigma_of(r)), want) == 0
        assert 0 < n < want[at[0]].size or r >= 12                       # a window, not the slice (r = 12 > H covers every row)
        assert not np.isnan(want[1 - at[0]]).any()                       # the other slice is clean
    names = [n for n, _ in B.nan_positions(r)]
    assert ("above_halo" in names) == (r < 8)


@pytest.mark.parametrize("mutation", sorted(B.MUTATIONS))
def test_plan_case_inputs_see_a_mutated_emulation(mutation):
    """The inputs can tell a wrong kernel from scipy: each mutation differs from scipy on cases of the table."""
    seen = []
    for case in B.PLAN_CASES:
        x, want = B.plan_inputs(case)
        if B.unequal_bits(B.emulate(x, B.sigma_of(case[1]), mutation=mutation), want):
            seen.append(B.plan_case_id(case))
    print(f"{mutation}: differs from scipy on {len(seen)} of {len(B.PLAN_CASES)} cases")
    assert len(seen) >= 1
    if mutation == "fma":                                                 # the cancelling rows: both load widths of both kernels
        kernels = {(B.plan_vec(c), c[1] == 4) for c in B.PLAN_CASES if B.has_cancelling_rows(c) and B.plan_case_id(c) in seen}
        assert kernels == {(1, False), (1, True), (2, False), (2, True)}


def _sample(dtype=np.float32, shape=(48, 40)):
    rng = np.random.default_rng(31)
    img = rng.random(shape).astype(np.float32)
    if np.issubdtype(dtype, np.integer):
        img = np.rint(img * 1000).astype(dtype)
    lab = np.kron(rng.integers(0, 9, size=(shape[0] // 4, shape[1] // 4)), np.ones((4, 4), np.int64)).astype(np.float32)
    return img, lab


@pytest.mark.parametrize("seed", range(6))
def test_random_generator_blurs_before_its_transforms(seed):
    from cswin_unet_amd.datasets import RandomGenerator
    img, lab = _sample()

    def run(gen, image):
        random.seed(50 + seed)
        np.random.seed(60 + seed)
        out = gen({"image": image, "label": lab.copy()})
        return out, random.getstate(), np.random.get_state()

    got, rs, ns = run(RandomGenerator([32, 24], blur_sigma=1), img.copy())
    want, rs_w, ns_w = run(RandomGenerator([32, 24]), gaussian_filter(img, 1))
    plain, rs_p, ns_p = run(RandomGenerator([32, 24]), img.copy())
    assert torch.equal(got["image"], want["image"]) and torch.equal(got["label"], want["label"])
    assert not torch.equal(got["image"], plain["image"]) and torch.equal(got["label"], plain["label"])
    assert rs == rs_w == rs_p
    for a, b in ((ns, ns_w), (ns, ns_p)):
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def test_random_generator_draws_cover_every_branch():
    """The six seeds of the test above reach all three kinds."""
    from cswin_unet_amd.datasets import RawSliceParams
    img, lab = _sample()
    kinds = set()
    for seed in range(6):
        random.seed(50 + seed)
        np.random.seed(60 + seed)
        kinds.add(int(RawSliceParams([32, 24])({"image": img, "label": lab})["params"][0]))
    assert kinds == {0, 1, 2}


def test_random_generator_blurs_an_integer_image_as_float32():
    from cswin_unet_amd.datasets import RandomGenerator
    img, lab = _sample(np.int16)
    with B.scripted_draws((0, 0, 0, 0)):
        got = RandomGenerator([48, 40], blur_sigma=1)({"image": img, "label": lab})
    want = gaussian_filter(img.astype(np.float32), 1)
    assert got["image"].dtype == torch.float32 and np.array_equal(got["image"][0].numpy(), want)
    assert not np.array_equal(want, np.rint(want))                      # not scipy's rounded integer result


class StubNet(torch.nn.Module):
    """Class c where the pixel is nearest to the c-th of four levels: per-pixel, so a blur of the input moves the classes."""

    def forward(self, x):
        levels = torch.tensor([0.2, 0.4, 0.6, 0.8], dtype=x.dtype).view(1, 4, 1, 1)
        return -(x - levels) ** 2


def _volume(shape=(5, 40, 32)):
    vol = np.random.default_rng(77).random(shape).astype(np.float32)
    return vol


@pytest.mark.parametrize("patch", [(40, 32), (56, 48)], ids=["no_resize", "resize"])
def test_predict_volume_host_blurs_every_slice_with_scipy(patch):
    from cswin_unet_amd.utils import predict_volume
    vol, net = _volume(), StubNet()
    blurred = B.scipy_blur(vol, 1.0)
    got = predict_volume(vol, net, patch, batch_slices=2, device="cpu", blur_sigma=1.0)
    want = predict_volume(blurred, net, patch, batch_slices=2, device="cpu")
    plain = predict_volume(vol, net, patch, batch_slices=2, device="cpu")
    assert got.shape == vol.shape and np.array_equal(got, want)
    assert not np.array_equal(got, plain) and len(np.unique(got)) > 1
    assert np.array_equal(predict_volume(vol, net, patch, batch_slices=2, device="cpu", blur_sigma=None), plain)
    one = predict_volume(vol[0], net, patch, device="cpu", blur_sigma=1.0)
    assert np.array_equal(one, want[0])
    with pytest.raises(ValueError):
        predict_volume(vol, net, patch, device="cpu", blur_sigma=0)
    with pytest.raises(ValueError):
        predict_volume(vol, net, patch, device="cpu", blur_sigma=9)


def test_predict_volume_host_blurs_in_the_volumes_own_dtype():
    from cswin_unet_amd.utils import predict_volume
    vol, net = _volume().astype(np.float64), StubNet()
    got = predict_volume(vol, net, (40, 32), device="cpu", blur_sigma=1.0)
    assert np.array_equal(got, predict_volume(B.scipy_blur(vol, 1.0), net, (40, 32), device="cpu"))


def test_single_volume_and_evaluate_volumes_forward_blur_sigma(tmp_path):
    from cswin_unet_amd.utils import evaluate_volumes, test_single_volume
    vol, net = _volume(), StubNet()
    lab = (np.arange(vol.size).reshape(vol.shape) // 7 % 4).astype(np.int64)
    image, label = torch.from_numpy(vol)[None], torch.from_numpy(lab)[None]
    blurred = torch.from_numpy(B.scipy_blur(vol, 1.0))[None]
    kw = dict(classes=4, patch_size=[56, 48], device="cpu", metrics="host")
    got = test_single_volume(image, label, net, blur_sigma=1.0, test_save_path=str(tmp_path), case="c0", **kw)
    want = test_single_volume(blurred, label, net, **kw)
    plain = test_single_volume(image, label, net, **kw)
    assert got == want and got != plain
    assert np.array_equal(np.load(tmp_path / "c0_pred.npz")["image"], vol)          # the saved image is the one passed in
    loader = [{"image": image, "label": label, "case_name": "c0"}]
    ev = evaluate_volumes(loader, net, 4, (56, 48), metrics="host", device="cpu", blur_sigma=1.0)
    assert ev[0] == [want]
    assert evaluate_volumes(loader, net, 4, (56, 48), metrics="host", device="cpu")[0] == [plain]


@pytest.mark.parametrize("sigma", [0, -1.0, float("nan"), 9])
def test_trainer_synapse_refuses_a_bad_sigma_before_it_reads_anything(sigma, tmp_path):
    from types import SimpleNamespace
    from cswin_unet_amd.trainer import trainer_synapse
    snap = tmp_path / "snap"
    with pytest.raises(ValueError, match="gaussian_taps"):
        trainer_synapse(SimpleNamespace(blur_sigma=sigma, augment="hip"), None, str(snap))          # no dataset, no model
    assert not snap.exists()
