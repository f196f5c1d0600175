"""The launch policy of the attention kernels on the host (no GPU): the Python transcription in tests/test_gpu_attn_shapes.py
(attn_plan), from which that file's coverage claims and the job shapes of tests/test_gpu_attn_parent.py are computed, against
cswin_unet_amd/csrc/attn_plan.h itself -- the header the library launches from --, field by field through
tools/attn_plan_check.cpp: on every row of the case tables, on the models' attention shapes and on a sweep of window shapes
and unit counts around the thresholds of the split rules.  The figures beside the rows of CASES are held to the tool directly;
the comparison is shown to be able to fail (a tuning variable in the tool's environment moves named rows); and what the old
formulas left unchecked -- thread counts, LDS sizes against their reservation and the hardware's limit, the dS stride, the
workspace layout, the refusals -- is asserted on the tool's output over the same sweep."""
import glob
import os
import shutil
import subprocess

import pytest

import test_gpu_attn_shapes as A
from test_gpu_attn_parent import LW_SUB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HD, LDT = 32, 36                        # the padded head dim and the LDS row stride of the kernels' images (csrc/attn_plan.h)
LDS_PER_WORKGROUP = 160 * 1024          # MI355X: a single workgroup may declare all 160 KiB of a CU's LDS
LDS_PLAIN = 64 * 1024                   # above it a kernel needs the dynamic-LDS opt-in, i.e. a reservation
RESOS = tuple(range(1, 65)) + (96, 97, 113, 129, 193, 257)
IDXS = ((-1,), (0,), (1,), (0, 1))
BATCHES = (1, 2, 3, 8, 24)
THRESHOLDS = (256, 512, 768, 1024)      # of the split rules: nwg <= 256, nwg % 256, nwg < 1024
MAX_N = 288                             # 18 tiles of 16 tokens: the largest forward instantiation


@pytest.fixture(scope="module")
def plan_tool(tmp_path_factory):
    """tools/attn_plan_check.cpp, compiled with the system C++ compiler and no HIP include path: cases -> parsed plan lines."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("attn_plan") / "attn_plan_check")
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "cswin_unet_amd", "csrc"),
                    os.path.join(ROOT, "tools", "attn_plan_check.cpp"), "-o", exe], check=True)

    def run(cases, **tuning):
        env = {k: v for k, v in os.environ.items() if k not in A.TUNING_VARS}
        env.update(tuning)
        out = subprocess.run([exe], input="\n".join(request(c) for c in cases) + "\n", capture_output=True, text=True, env=env)
        assert out.returncode == 0, out.stderr
        lines = out.stdout.splitlines()
        assert len(lines) == len(cases)
        return [parse(line) for line in lines]
    return run


def request(case):
    B, reso, split, idx, C, heads = case
    return " ".join(map(str, (B, reso, C, len(idx), *heads, *idx, split)))


def parse(line):
    """A line of the tool: {"refused": name}, or its fields under the transcription's names and the header's."""
    if line.startswith("refused "):
        return dict(refused=line.split()[1])
    geo, fwd, bwd, ws = (part.split() for part in line.split(" | "))
    N, nt, nwg, hd, thin = map(int, geo)
    ws = list(map(int, ws))
    b = list(map(int, bwd[1:]))
    return dict(N=N, nt=nt, nwg=nwg, hd=hd, thin=bool(thin), fwd=(fwd[0], int(fwd[1]), int(fwd[2])), fwd_threads=int(fwd[3]), fwd_grid=int(fwd[4]),
                fwd_lds=int(fwd[5]), bwd=(bwd[0], b[0]), slab_rows=b[1], ds_stride=b[2], vs_floats=b[3], bwd_lds=b[4], lds_reserved=b[5],
                grids=b[6:], ws_bytes=ws[0], slab_off=ws[1:-1], delta_off=ws[-1])


def windows(reso, split, idx):
    """[(H_sp, W_sp)] per branch, written out here and not through the oracle."""
    return [(reso, reso) if i == -1 else (reso, split) if i == 0 else (split, reso) for i in idx]


def model_cases():
    """(B, reso, split, idx, C, heads) of every attention call of the models in configs/, at the benchmark's batch and at batch 1:
    read off the blocks of the constructed model, not retyped."""
    from cswin_unet_amd.config import get_config
    from cswin_unet_amd.networks.cswin_unet import CSWinBlock
    from cswin_unet_amd.networks.vision_transformer import CSwinUnet
    files = sorted(glob.glob(os.path.join(ROOT, "configs", "*.yaml")))
    assert len(files) >= 3
    out = []
    for f in files:
        model = CSwinUnet(get_config(f), num_classes=9)
        blocks = [m for m in model.modules() if isinstance(m, CSWinBlock)]
        assert len(blocks) >= 8                                       # four encoder and four decoder stages
        shapes = {(b.patches_resolution, b.split_size, tuple(m.idx for m in b.attns), b.dim, tuple(m.num_heads for m in b.attns)) for b in blocks}
        assert len(shapes) == 4, f
        out += [(B,) + s for s in sorted(shapes) for B in (24, 1)]
    return out


def table_cases():
    rows = A.ROWS + A.MODE_ROWS + A.DROP_ROWS + A.AUTOGRAD_ROWS
    return list(dict.fromkeys(rows + model_cases()))


def sweep_cases():
    """Every accepted shape of the sweep: reso in RESOS, every split dividing it with N <= 288, every idx, every batch; heads (equal
    in the branches, head dims 8 .. 32 in turn) such that nwg lies just under, on (where the units divide it) and just over each
    threshold of the split rules, and 1."""
    out, k = [], 0
    for reso in RESOS:
        for split in (s for s in range(1, reso + 1) if reso % s == 0):
            for idx in IDXS:
                shapes = windows(reso, split, idx)
                if shapes[0][0] * shapes[0][1] > MAX_N:
                    continue
                for B in BATCHES:
                    per_head = B * sum((reso // h) * (reso // w) for h, w in shapes)        # nwg = per_head * heads
                    hs = {1} | {T // per_head + d for T in THRESHOLDS for d in (0, 1)} | {(T - 1) // per_head for T in THRESHOLDS}
                    for h in sorted(h for h in hs if 1 <= h < 4096):
                        k += 1
                        out.append((B, reso, split, idx, len(idx) * h * (8, 16, 24, 32)[k % 4], (h,) * len(idx)))
    return out


@pytest.fixture(scope="module")
def swept(plan_tool):
    """(cases, the tool's plans) of the tables, the models and the sweep, made once; the landing of nwg around the thresholds is
    checked here so that every test on the sweep rests on it."""
    cases = list(dict.fromkeys(table_cases() + sweep_cases()))
    plans = plan_tool(cases)
    nwgs = {p["nwg"] for p in plans if "nwg" in p}
    for T in THRESHOLDS:
        assert {T - 1, T, T + 1} <= nwgs, T
    return cases, plans


FIELDS = ("N", "nt", "nwg", "hd", "thin", "fwd", "bwd")


def test_transcription_equals_the_header_field_by_field(swept):
    cases, plans = swept
    bad = []
    for case, got in zip(cases, plans):
        want = A.attn_plan(*case)
        if any(got.get(k) != want[k] for k in FIELDS):
            bad.append((case, {k: (got.get(k), want[k]) for k in FIELDS if got.get(k) != want[k]}))
    print(f"{len(cases)} plans compared on {len(FIELDS)} fields, {len(bad)} differ")
    assert len(cases) > 20000 and not bad, bad[:3]
    seen = {p["fwd"] for p in plans}, {p["bwd"] for p in plans}
    assert seen[0] == set(A.ALL_FWD) and seen[1] >= set(A.ALL_BWD)


def test_case_table_figures_are_the_headers(plan_tool):
    """The figures beside each row of CASES against the tool directly (not through the transcription); slab rows of the two-pass
    rows are test_gpu_attn_parent's LW_SUB, of the fused rows 1."""
    plans = plan_tool(A.ROWS)
    for (case, want), p in zip(A.CASES, plans):
        assert (p["N"], p["nt"], p["nwg"], p["fwd"], p["bwd"]) == want, A.cid(case)
        assert p["slab_rows"] == (LW_SUB if p["bwd"][0] == "two_pass" else 1), A.cid(case)


QS1_ROW = (8, 9, 9, (-1,), 256, (32,))          # fwd3<6, 1> by default: 256 units
QS2_ROW = (2, 9, 9, (-1,), 24, (3,))            # fwd3<6, 2> and bwd3<6> by default
NT4_ROW = (2, 8, 8, (-1,), 64, (2,))            # fwd3<4, 1>: below the split's smallest class


def test_the_comparison_can_fail(plan_tool):
    """With a tuning variable in the tool's environment alone the tool departs from the transcription (which holds the defaults)
    on named rows, so the comparison above does see a moved rule, and the tool reads the tuning structure the library reads."""
    rows = [QS1_ROW, QS2_ROW, NT4_ROW, A.ROWS[-1]]
    default = plan_tool(rows)
    assert [p["fwd"] for p in default] == [A.attn_plan(*c)["fwd"] for c in rows] == [("fwd3", 6, 1), ("fwd3", 6, 2), ("fwd3", 4, 1), ("fwd", 18, 2)]
    assert [p["bwd"] for p in default] == [("bwd3", 6), ("bwd3", 6), ("bwd3", 4), ("two_pass", 5)]
    split = plan_tool(rows, CSWIN_ATTN_FWD_QSPLIT="2")
    assert [p["fwd"] for p in split] == [("fwd3", 6, 2), ("fwd3", 6, 2), ("fwd3", 4, 1), ("fwd", 18, 2)]        # NT 4 has no split
    assert split[0]["fwd"] != A.attn_plan(*QS1_ROW)["fwd"] and (split[0]["fwd_grid"], split[0]["fwd_threads"]) == (512, 192)
    assert [p["bwd"] for p in split] == [p["bwd"] for p in default]
    whole = plan_tool(rows, CSWIN_ATTN_FWD_QSPLIT="1")
    assert [p["fwd"][2] for p in whole] == [1, 1, 1, 1] and whole[1]["fwd"] != A.attn_plan(*QS2_ROW)["fwd"]
    two = plan_tool(rows, CSWIN_ATTN_BWD_TWO_PASS="1")
    assert [p["bwd"] for p in two] == [("two_pass", 2), ("two_pass", 2), ("two_pass", 1), ("two_pass", 5)]
    assert two[1]["bwd"] != A.attn_plan(*QS2_ROW)["bwd"] and two[1]["slab_rows"] == LW_SUB and two[1]["ws_bytes"] > default[1]["ws_bytes"]
    assert [p["fwd"] for p in two] == [p["fwd"] for p in default]


def test_invariants_of_the_plans(swept):
    """Properties the launches and the kernels rely on, from the tool's output alone."""
    cases, plans = swept
    reserved = 0
    for case, p in zip(cases, plans):
        B, reso, split, idx, C, heads = case
        N, (family, NT, QS), (path, arg) = p["N"], p["fwd"], p["bwd"]
        tag = (case, p)
        assert N <= 16 * NT and p["nt"] == -(-N // 16), tag
        assert p["fwd_threads"] <= 1024 and p["fwd_threads"] % 64 == 0 and p["fwd_grid"] == QS * p["nwg"], tag
        assert p["fwd_threads"] // 64 == (-(-NT // 2) if QS == 2 else NT if family == "fwd3" else 8), tag      # a wave per query tile, or 8 that walk them
        assert p["fwd_lds"] == 4 * (2 * 16 * NT * LDT + 10 * HD) <= LDS_PER_WORKGROUP, tag
        assert p["ds_stride"] >= N and p["ds_stride"] % 8 == 4, tag
        if path == "bwd3":
            assert N <= 16 * arg and 64 * arg <= 1024 and p["grids"] == [p["nwg"]] and p["slab_rows"] == 1, tag
            assert p["vs_floats"] >= max(N * p["ds_stride"] + 16 * arg, (16 * arg + 1) * LDT) and p["vs_floats"] % 4 == 0, tag
            assert p["bwd_lds"] == 4 * (2 * 16 * arg * LDT + p["vs_floats"] + 2 * 16 * arg + (19 + arg) * HD), tag
            assert (p["lds_reserved"] > 0) == (p["bwd_lds"] > LDS_PLAIN), tag
            if p["lds_reserved"]:
                reserved += 1
                assert p["bwd_lds"] <= p["lds_reserved"] <= LDS_PER_WORKGROUP, tag
            assert p["bwd_lds"] <= LDS_PER_WORKGROUP, tag
        else:
            items = B * sum(heads) * reso * reso
            assert arg == -(-N // 64) and p["slab_rows"] == LW_SUB and p["bwd_lds"] == 0 == p["lds_reserved"], tag
            assert p["grids"] == [-(-items * 8 // 256), p["nwg"] * arg, p["nwg"] * arg, p["nwg"] * LW_SUB], tag
        # the workspace: the branches' slab regions in order, disjoint, ending where delta begins; delta to the end
        units = [B * (reso // h) * (reso // w) * heads[i] for i, (h, w) in enumerate(windows(reso, split, idx))]
        assert sum(units) == p["nwg"] and len(p["slab_off"]) == len(idx), tag
        end = 0
        for off, u in zip(p["slab_off"], units):
            assert off == end, tag
            end = off + u * p["slab_rows"] * 10 * HD
        assert end == p["delta_off"], tag
        assert p["ws_bytes"] == 4 * (p["nwg"] * 10 * HD * p["slab_rows"] + B * sum(heads) * reso * reso), tag
    print(f"{len(cases)} plans checked, {reserved} of them with an LDS reservation")
    assert reserved > 0


def predicted_refusal(case):
    """The refusal the rules give, branch by branch in the order the entry points make them; None: accepted."""
    B, reso, split, idx, C, heads = case
    if not (B > 0 and reso > 0 and C > 0 and len(idx) in (1, 2)):
        return "bad_arguments"
    Cb, hd0, N0 = C // len(idx), None, None
    for i, h, (H_sp, W_sp) in zip(idx, heads, windows(reso, split, idx)):
        if h <= 0 or Cb % h or Cb // h not in (8, 16, 24, 32) or hd0 not in (None, Cb // h):
            return "head_dim"
        hd0 = Cb // h
        if i not in (-1, 0, 1):
            return "error_mode"
        if H_sp <= 0 or W_sp <= 0 or reso % H_sp or reso % W_sp:
            return "divisibility"
        nWin = (reso // H_sp) * (reso // W_sp)
        if B * nWin * h >= 2 ** 20 or H_sp * W_sp >= 2 ** 12 or nWin >= 2 ** 12 or h >= 2 ** 12:
            return "index_range"
        if N0 not in (None, H_sp * W_sp):
            return "window_sizes"
        N0 = H_sp * W_sp
    return "window_tokens" if N0 > MAX_N else None


def test_refusals_are_the_ones_the_rules_predict(plan_tool, swept):
    """Nothing of the sweep above is refused; and over shapes that are not all acceptable -- splits that do not divide, windows
    past 288 and past 4095 tokens, head dims off the list or unequal, unknown modes, unequal windows, too many units, a batch of
    zero -- the tool names the refusal the rules give."""
    assert not any("refused" in p for p in swept[1])
    cases = [(0, 8, 8, (-1,), 32, (1,)), (1, 8, 0, (0,), 32, (1,)), (1, 8, 8, (-1,), 32, (0,)), (1, 8, 8, (-1,), 64, (4096,))]
    for reso in RESOS:
        for split in sorted({1, 2, 3, 5, 7, 12, reso}):
            for idx in IDXS + ((-1, 0), (0, -1), (2,), (0, 3)):
                for C, h in ((32, 1), (12, 1), (40, 1), (48, 3), (64, 1)):
                    cases.append((1, reso, split, idx, len(idx) * C, (h,) * len(idx)))
                cases.append((1, reso, split, idx, len(idx) * 32, (1, 2)[:len(idx)]))
                cases.append((3000, reso, split, idx, len(idx) * 128, (16,) * len(idx)))
    got = plan_tool(cases)
    want = [predicted_refusal(c) for c in cases]
    bad = [(c, g.get("refused"), w) for c, g, w in zip(cases, got, want) if g.get("refused") != w]
    kinds = {w for w in want}
    print(f"{len(cases)} requests, {sum(w is not None for w in want)} refused, {len(bad)} differ")
    assert not bad, bad[:3]
    assert kinds == {None, "bad_arguments", "head_dim", "error_mode", "divisibility", "index_range", "window_sizes", "window_tokens"}
