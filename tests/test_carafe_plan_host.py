"""The launch policy of the CARAFE kernels on the host (no GPU): the Python transcription in tests/test_gpu_carafe_shapes.py, from
which that file's coverage claims and its dbias bound are computed, against cswin_unet_amd/csrc/carafe_plan.h itself -- the header
the library launches from --, field by field through tools/carafe_plan_check.cpp: on every row of the case tables, on the models'
CARAFE calls and on a sweep of channel widths and maps around every clamp and around the fused kernel's tile.  The comparison is
shown to be able to fail (the tuning variable in the tool's environment moves the fused rows and no other); and what the
transcription does not say -- that a grid covers its items or sits at its clamp, that the workspace holds the partial sums of
whichever route is launched, the staging of the bias-in-e route, the fused kernel's threads and LDS, the refusals -- is asserted
on the tool's output over the same sweep."""
import glob
import os
import shutil
import subprocess

import pytest

import test_gpu_carafe_shapes as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TUNING_VAR = "CSWIN_CARAFE_GENERIC"
LDS_PLAIN = 64 * 1024                   # static LDS a kernel gets without the opt-in
THREADS = 256
CLASSES = 9                             # of the plane requests: any 0 < C <= Cz launches alike, the narrower of this and Cz is sent
CZS = tuple(range(4, 1044, 4))
# maps every (Cz, S) of the sweep gets: below the stencil, odd, B > 1, and H, W on both sides of multiples of the fused tile
MAPS = ((1, 1, 1), (2, 3, 5), (3, 7, 13), (1, 8, 8), (2, 8, 16), (1, 24, 24), (2, 7, 8), (2, 8, 9), (1, 9, 8), (3, 16, 15), (1, 17, 16),
        (24, 56, 56), (24, 7, 7), (1, 56, 56))
TILE_SIDES = (1, 7, 8, 9, 15, 16, 17, 24, 56)      # H and W of the dense map grid at the widths next to the fused one


@pytest.fixture(scope="module")
def plan_tool(tmp_path_factory):
    """tools/carafe_plan_check.cpp, compiled with the system C++ compiler and no HIP include path: request lines -> parsed lines."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("carafe_plan") / "carafe_plan_check")
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "cswin_unet_amd", "csrc"),
                    os.path.join(ROOT, "tools", "carafe_plan_check.cpp"), "-o", exe], check=True)

    def run(requests, **tuning):
        env = {k: v for k, v in os.environ.items() if k != TUNING_VAR}
        env.update(tuning)
        out = subprocess.run([exe], input="\n".join(requests) + "\n", capture_output=True, text=True, env=env)
        assert out.returncode == 0, out.stderr
        lines = out.stdout.splitlines()
        assert len(lines) == len(requests)
        return [parse(line) for line in lines]
    return run


BWD_FIELDS = ("lpr", "groups", "chunks", "grid_e", "grid_z", "colsum_lanes", "colsum_rgroups", "colsum_grid", "tiles_x", "tiles_y", "grid_fused",
              "part_rows", "ws_bytes")
FIELDS = {"tok": ("lpr", "groups", "grid"), "planes": ("ppb", "grid"), "colsum": ("lanes", "rgroups", "grid"),
          "limits": ("threads", "grid_clamp", "colsum_clamp", "colsum_rows", "bias_in_e_cz", "e_chunks", "e_stage_chunk_floats", "e_stage_bytes",
                     "fused_threads", "fused_tile", "fused_lds_bytes", "lds_plain")}


def parse(line):
    """A line of the tool: {"refused": name}, or its fields under the header's names."""
    tag, *rest = line.split()
    if tag == "refused":
        return dict(refused=rest[0])
    if tag == "bwd":
        return dict(zip(BWD_FIELDS, map(int, rest[1:])), route=rest[0])
    return dict(zip(FIELDS[tag], map(int, rest)))


def requests(case):
    """The forward in both forms and the backward of a (B, H, W, S, Cz)."""
    B, H, W, S, Cz = case
    return [f"tok {B} {H} {W} {Cz} {S}", f"planes {B} {H} {W} {Cz} {min(Cz, CLASSES)} {S}", f"bwd {B} {H} {W} {Cz} {S}"]


def model_cases():
    """(B, H, W, S, Cz) of every CARAFE call of the models in configs/, at the benchmark's batch and at batch 1: the map from the
    blocks that feed the module, S and Cz from the module, the head's Cz as CSWinTransformer.up_x4 pads its classes."""
    from cswin_unet_amd.config import get_config
    from cswin_unet_amd.networks.cswin_unet import CARAFE, CARAFE4
    from cswin_unet_amd.networks.vision_transformer import CSwinUnet
    files = sorted(glob.glob(os.path.join(ROOT, "configs", "*.yaml")))
    assert len(files) >= 3
    out = []
    for f in files:
        net = CSwinUnet(get_config(f), num_classes=CLASSES).cswin_unet
        ups = [(net.stage_up4, net.upsample4), (net.stage_up3, net.upsample3), (net.stage_up2, net.upsample2), (net.stage_up1, net.upsample1)]
        assert [type(up) for _, up in ups] == [CARAFE, CARAFE, CARAFE, CARAFE4]
        assert sum(isinstance(m, (CARAFE, CARAFE4)) for m in net.modules()) == len(ups)
        for blocks, up in ups:
            side = blocks[-1].patches_resolution
            ncls = net.output.out_channels
            Cz = max(16, 1 << (ncls - 1).bit_length()) if isinstance(up, CARAFE4) else up.out.out_channels
            out += [(B, side, side, up.up_factor, Cz) for B in (24, 1)]
    return out


def table_cases():
    rows = [(c.B, c.H, c.W, c.S, c.Cz) for c in T.SMALL + T.BIG + [d[0] for d in T.DELTAS]]
    return list(dict.fromkeys(rows + model_cases()))


def sweep_cases():
    """Every Cz = 4 .. 1040 and both S on MAPS, and on maps of one row whose pixel count puts items / groups and pixels / groups
    (8192 workgroups), pixels / pixels-per-workgroup of the plane forward (8192) and rows / (row groups x 64) of the column sums
    (512) one workgroup below, on and one above each clamp; at the widths round the fused one a dense grid of H and W."""
    out = []
    for Cz in CZS:
        g, rg = T.groups(Cz), THREADS // T.colsum_lanes(Cz)
        for S in (2, 4):
            S2 = S * S
            pixels = set()
            for d in (-1, 0, 1):
                pixels |= {T.cdiv((T.GRID_CLAMP + d) * g, S2), (T.GRID_CLAMP + d) * g // S2}           # items / groups
                pixels |= {(T.GRID_CLAMP + d) * g}                                                         # pixels / groups
                pixels |= {(T.GRID_CLAMP + d) * T.ppb(S)}                                                  # the plane forward
                pixels |= {T.cdiv((T.COLSUM_CLAMP + d) * rg * 64, S2), (T.COLSUM_CLAMP + d) * rg * 64 // S2}
            out += [(B, H, W, S, Cz) for B, H, W in MAPS] + [(1, 1, n, S, Cz) for n in sorted(pixels)]
            if Cz in (12, 16, 20):
                out += [(B, H, W, S, Cz) for B in (1, 3) for H in TILE_SIDES for W in TILE_SIDES]
    return out


@pytest.fixture(scope="module")
def swept(plan_tool):
    """(cases, [tok, planes, bwd] of each by default, the bwd of each with the tuning variable set, the limits line), made once;
    that the sweep does bracket every clamp is checked here so that every test on it rests on that."""
    cases = list(dict.fromkeys(table_cases() + sweep_cases()))
    lines = plan_tool([r for c in cases for r in requests(c)])
    plans = [lines[i:i + 3] for i in range(0, len(lines), 3)]
    generic = plan_tool([requests(c)[2] for c in cases], **{TUNING_VAR: "1"})
    limits = plan_tool(["limits"])[0]
    assert not any("refused" in p for three in plans for p in three) and not any("refused" in p for p in generic)
    wanted = {"items": set(), "pixels": set(), "planes": set(), "rows": set()}
    for (B, H, W, S, Cz), (tok, planes, bwd) in zip(cases, plans):
        wanted["items"].add(T.cdiv(B * H * W * S * S, tok["groups"]))
        wanted["pixels"].add(T.cdiv(B * H * W, tok["groups"]))
        wanted["planes"].add(T.cdiv(B * H * W, planes["ppb"]))
        if bwd["route"] == "colsum":
            wanted["rows"].add(T.cdiv(B * H * W * S * S, bwd["colsum_rgroups"] * limits["colsum_rows"]))
    for what, clamp in (("items", limits["grid_clamp"]), ("pixels", limits["grid_clamp"]), ("planes", limits["grid_clamp"]), ("rows", limits["colsum_clamp"])):
        assert {clamp - 1, clamp, clamp + 1} <= wanted[what], what
    return cases, plans, generic, limits


def transcribed(case):
    """The same fields from tests/test_gpu_carafe_shapes.py: (tok, planes, bwd)."""
    B, H, W, S, Cz = case
    plan = T.launch_plan(B, H, W, S, Cz)
    fused = T.fused_ok(H, W, Cz, S)
    route = "fused" if fused else "bias_in_e" if T.bias_in_e(Cz) else "colsum"
    assert ("fused" in plan, "colsum" in plan) == (route == "fused", route == "colsum")
    bwd = dict(route=route, lpr=T.lpr(Cz), groups=T.groups(Cz), chunks=T.chunk_pattern(Cz)[1], ws_bytes=T.workspace_bytes(B, H, W, Cz, S),
               grid_e=0, grid_z=0, colsum_lanes=0, colsum_rgroups=0, colsum_grid=0, tiles_x=0, tiles_y=0, grid_fused=0)
    if fused:
        bwd.update(tiles_x=W // T.TILE, tiles_y=H // T.TILE, grid_fused=plan["fused"][0], part_rows=plan["fused"][0])
    else:
        assert plan["bwd_e"] == plan["fwd"]
        bwd.update(grid_e=plan["bwd_e"][0], grid_z=plan["bwd_z"][0], part_rows=plan["bwd_e"][0])
        if route == "colsum":
            lanes = T.colsum_lanes(Cz)
            bwd.update(colsum_lanes=lanes, colsum_rgroups=THREADS // lanes, colsum_grid=plan["colsum"][0], part_rows=plan["colsum"][0])
            assert plan["colsum"][0] == T.colsum_blocks(B * H * W * S * S, Cz)
    return (dict(lpr=T.lpr(Cz), groups=T.groups(Cz), grid=plan["fwd"][0]), dict(ppb=T.ppb(S), grid=T.plane_plan(B, H, W, S)[0]), bwd)


def test_transcription_equals_the_header_field_by_field(swept):
    cases, plans, _, limits = swept
    assert (limits["grid_clamp"], limits["colsum_clamp"], limits["fused_tile"], limits["threads"]) == (T.GRID_CLAMP, T.COLSUM_CLAMP, T.TILE, THREADS)
    assert T.bias_in_e(limits["bias_in_e_cz"]) and not T.bias_in_e(limits["bias_in_e_cz"] + 4)
    bad = []
    for case, got in zip(cases, plans):
        for name, g, w in zip(("tok", "planes", "bwd"), got, transcribed(case)):
            if g != w:
                bad.append((case, name, {k: (g.get(k), w[k]) for k in w if g.get(k) != w[k]}))
    nfields = len(FIELDS["tok"]) + len(FIELDS["planes"]) + len(BWD_FIELDS) + 1
    print(f"{len(cases)} shapes compared on {nfields} fields, {len(bad)} differ")
    assert len(cases) > 10000 and not bad, bad[:3]
    assert {p[2]["route"] for p in plans} == {"fused", "bias_in_e", "colsum"}
    assert {p[0]["lpr"] for p in plans} == {1, 2, 4, 8, 16, 32, 64}


def test_column_sum_launch_of_every_width(plan_tool, swept):
    """colsum_partial_kernel's lanes, row groups and grid for every width of the sweep (the backward launches it above 512
    channels only), rows on both sides of the clamp."""
    limits = swept[3]
    reqs = []
    for C in CZS:
        per = THREADS // T.colsum_lanes(C) * limits["colsum_rows"]
        reqs += [(rows, C) for rows in (1, per - 1, per, per + 1, (T.COLSUM_CLAMP - 1) * per, T.COLSUM_CLAMP * per - 1, T.COLSUM_CLAMP * per,
                                        T.COLSUM_CLAMP * per + 1, (T.COLSUM_CLAMP + 1) * per, 77 * 2 ** 20)]
    got = plan_tool([f"colsum {rows} {C}" for rows, C in reqs])
    for (rows, C), g in zip(reqs, got):
        lanes = T.colsum_lanes(C)
        assert g == dict(lanes=lanes, rgroups=THREADS // lanes, grid=T.colsum_blocks(rows, C)), (rows, C, g)
        assert 1 <= g["lanes"] * g["rgroups"] <= THREADS and 1 <= g["grid"] <= limits["colsum_clamp"]
        assert g["grid"] == limits["colsum_clamp"] or g["grid"] * g["rgroups"] * limits["colsum_rows"] >= rows, (rows, C, g)
    assert {g["grid"] for g in got} >= {1, 2, T.COLSUM_CLAMP - 1, T.COLSUM_CLAMP}


def test_the_comparison_can_fail(swept):
    """With CSWIN_CARAFE_GENERIC in the tool's environment alone, exactly the fused rows leave the transcription (which holds the
    default) for the generic route of their width, and no other row moves: the comparison above does see a moved rule, and the
    tool reads the tuning structure the library reads."""
    cases, plans, generic, _ = swept
    moved = 0
    for case, (_, _, default), g in zip(cases, plans, generic):
        if default["route"] == "fused":
            moved += 1
            B, H, W, S, Cz = case
            assert g != default and g != transcribed(case)[2], case
            assert g["route"] == "bias_in_e" and g["grid_fused"] == 0 and g["part_rows"] == g["grid_e"] == T.grid_for(B * H * W * S * S, T.groups(Cz)), case
        else:
            assert g == default, case
    table = {(c.B, c.H, c.W, c.S, c.Cz) for c in T.FUSED + T.FUSED_PLANES}
    print(f"{moved} of {len(cases)} shapes are fused by default")
    assert moved >= len(table) and all(plans[cases.index(c)][2]["route"] == "fused" for c in table)


def test_invariants_of_the_plans(swept):
    """Properties the launches and the kernels rely on, from the tool's output alone."""
    cases, plans, generic, L = swept
    assert L["threads"] % 64 == 0 and L["fused_threads"] % 64 == 0 and L["fused_threads"] <= 1024 and L["threads"] <= 1024
    assert L["fused_threads"] >= 4 * L["fused_tile"] ** 2                                 # four lanes per interior pixel gather dz
    assert L["fused_lds_bytes"] <= LDS_PLAIN == L["lds_plain"] and L["e_stage_bytes"] <= LDS_PLAIN
    assert L["e_stage_bytes"] == L["e_chunks"] * L["e_stage_chunk_floats"] * 4
    routes = {"fused": 0, "bias_in_e": 0, "colsum": 0}

    def grid_ok(grid, per_workgroup, items, clamp):
        return 1 <= grid <= clamp and (grid == clamp or grid * per_workgroup >= items)

    for case, (tok, planes, bwd), gen in zip(cases, plans, generic):
        B, H, W, S, Cz = case
        tag = (case, tok, planes, bwd, gen)
        items, pixels = B * H * W * S * S, B * H * W
        assert tok["lpr"] * tok["groups"] == L["threads"] and tok["lpr"] <= 64 and tok["lpr"] & (tok["lpr"] - 1) == 0, tag
        assert tok["lpr"] <= Cz // 4 and (tok["lpr"] == 64 or 2 * tok["lpr"] > Cz // 4), tag
        assert grid_ok(tok["grid"], tok["groups"], items, L["grid_clamp"]), tag
        assert planes["ppb"] * S * S == L["threads"] and grid_ok(planes["grid"], planes["ppb"], pixels, L["grid_clamp"]), tag
        for p in (bwd, gen):
            routes[p["route"]] += 1
            assert (p["lpr"], p["groups"]) == (tok["lpr"], tok["groups"]) and p["chunks"] == T.cdiv(Cz // 4, p["lpr"]), tag
            # the workspace query does not see the flag and holds the partial sums of either setting, exactly those of the larger
            assert p["part_rows"] >= 1 and p["part_rows"] * Cz * 4 <= p["ws_bytes"], tag
            if p["route"] == "fused":
                assert (S, Cz) == (4, 16) and p["tiles_x"] * L["fused_tile"] == W and p["tiles_y"] * L["fused_tile"] == H, tag
                assert p["part_rows"] == p["grid_fused"] == B * p["tiles_x"] * p["tiles_y"], tag
                assert p["grid_e"] == p["grid_z"] == p["colsum_grid"] == 0, tag
                continue
            assert p["grid_fused"] == 0, tag
            assert p["grid_e"] == tok["grid"] and grid_ok(p["grid_z"], p["groups"], pixels, L["grid_clamp"]), tag
            if p["route"] == "bias_in_e":
                assert Cz <= L["bias_in_e_cz"] and p["part_rows"] == p["grid_e"] and p["colsum_grid"] == 0, tag
                assert p["chunks"] <= L["e_chunks"] and p["groups"] * 4 * p["lpr"] == L["e_stage_chunk_floats"], tag
            else:
                assert Cz > L["bias_in_e_cz"] and p["chunks"] > L["e_chunks"] and p["part_rows"] == p["colsum_grid"], tag
                assert p["colsum_lanes"] * p["colsum_rgroups"] <= L["threads"] and p["colsum_lanes"] == min(Cz, L["threads"]), tag
                assert grid_ok(p["colsum_grid"], p["colsum_rgroups"] * L["colsum_rows"], items, L["colsum_clamp"]), tag
        assert bwd["ws_bytes"] == gen["ws_bytes"] == max(bwd["part_rows"], gen["part_rows"]) * Cz * 4, tag
    print(f"{len(cases)} shapes checked with and without {TUNING_VAR}: {routes}")
    assert all(routes.values())


def predicted_refusal(tag, B, H, W, Cz, C, S):
    """The refusal the entry point's rules give, in the order it makes them; None: accepted."""
    fused = S == 4 and Cz == 16 and H % 8 == 0 and W % 8 == 0
    if tag == "bwd_planes":
        return "dimension" if min(B, H, W) <= 0 else "classes" if not 0 < C <= Cz else None if fused else "not_fused"
    if min(B, H, W) <= 0:
        return "dimension"
    if S not in (2, 4):
        return "scale"
    if Cz < 4 or Cz % 4:
        return "channels"
    return "classes" if tag == "planes" and not 0 < C <= Cz else None


def test_refusals_are_the_ones_the_entry_points_return_codes_for(plan_tool):
    """S outside {2, 4}, Cz no positive multiple of 4 and a non-positive dimension for every entry point, a class count outside
    (0, Cz] for the plane forms, anything but the fused shape for the plane backward -- the arguments
    test_gpu_carafe_shapes.test_carafe_refusals_touch_nothing and test_carafe_plane_backward_refusals_touch_nothing expect
    CSWIN_ERR_UNSUPPORTED for are among them -- and nothing else."""
    args = [(B, H, W, Cz, C, S) for B in (-1, 0, 2) for H in (0, 3, 8, 12) for W in (-8, 0, 5, 16) for Cz in (-4, 0, 2, 4, 6, 16, 32)
            for C in (0, 1, 9, 16, 20, 36) for S in (0, 1, 2, 3, 4, 8)]
    reqs = [(tag,) + a for a in args for tag in ("tok", "planes", "bwd", "bwd_planes")]
    line = lambda tag, B, H, W, Cz, C, S: f"{tag} {B} {H} {W} {Cz} {C} {S}" if "planes" in tag else f"{tag} {B} {H} {W} {Cz} {S}"
    got = plan_tool([line(*r) for r in reqs])
    want = [predicted_refusal(*r) for r in reqs]
    bad = [(r, g.get("refused"), w) for r, g, w in zip(reqs, got, want) if g.get("refused") != w]
    print(f"{len(reqs)} requests, {sum(w is not None for w in want)} refused, {len(bad)} differ")
    assert not bad, bad[:3]
    assert set(want) == {None, "dimension", "scale", "channels", "classes", "not_fused"}
    B, H, W, Cz, S = 2, 3, 5, 16, 4                        # the refusal tests' shape and what they change in it
    for kw in (dict(S=3), dict(Cz=6), dict(Cz=0), dict(B=0), dict(H=0)):
        a = dict(dict(B=B, H=H, W=W, Cz=Cz, S=S), **kw)
        got = plan_tool([line(tag, a["B"], a["H"], a["W"], a["Cz"], 9, a["S"]) for tag in ("tok", "planes", "bwd")])
        assert all("refused" in g for g in got), (kw, got)
    got = plan_tool([line("planes", B, H, W, Cz, C, S) for C in (0, Cz + 4)] +
                    [line("bwd_planes", *a) for a in ((2, 12, 16, 16, 9, 4), (2, 8, 16, 32, 9, 4), (2, 8, 16, 16, 9, 2), (2, 8, 16, 16, 0, 4),
                                                      (2, 8, 16, 16, 20, 4), (0, 8, 16, 16, 9, 4))])
    assert all("refused" in g for g in got), got
