"""The launch policy of the signed distance maps (csrc/sdm_plan.h) on the CPU, through tools/sdm_plan_check.cpp compiled with the
system compiler and no HIP include path: for every height the column tile and its LDS image stay within 64 KiB, the two grids
cover every row and every column exactly once, and what the entry point refuses has no plan."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import sdm_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, TX, TILES, ROW_BLOCKS, COL_BLOCKS, LDS, WS = range(7)


@pytest.fixture(scope="module")
def plan_tool(tmp_path_factory):
    """tools/sdm_plan_check.cpp: (B, ncls, H, W) rows -> the header's plans."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("sdm_plan") / "sdm_plan_check")
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "cswin_unet_amd", "csrc"),
                    os.path.join(ROOT, "tools", "sdm_plan_check.cpp"), "-o", exe], check=True)

    def run(rows):
        text = "".join("%d %d %d %d\n" % tuple(row) for row in rows)
        out = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        got = np.array(out.stdout.split(), np.int64).reshape(-1, 7)
        assert len(got) == len(rows)
        return got
    return run


def test_every_height_keeps_its_columns_in_64_kib(plan_tool):
    H = np.arange(1, S.SDM_MAX_DIM + 1)
    rows = np.stack([np.full_like(H, 3), np.full_like(H, 9), H, np.full_like(H, 224)], 1)
    got = plan_tool(rows)
    assert (got[:, OK] == 1).all()
    assert np.array_equal(got[:, TX], np.array([S.tx_of(h) for h in H]))
    assert np.array_equal(got[:, LDS], H * got[:, TX] * 2) and got[:, LDS].max() <= 65536
    assert got[:, LDS].max() > 65536 - 64                                  # and the budget is used: 2047 rows of 16 columns
    assert set(got[:, TX]) == {16, 32, 64} and (256 % got[:, TX] == 0).all()
    # the plan steps down where a wider tile would pass 16 KiB, and 16 columns are the floor
    for step in S.TX_STEPS:
        assert step * S.tx_of(step) * 2 <= 16384 < (step + 1) * S.tx_of(step) * 2
    assert np.array_equal(got[:, WS], ((3 * 9 * 4 + 255) // 256 * 256 + 3 * 9 * H * 224 * 2 + 15) // 16 * 16)


def test_every_height_has_grids_of_exactly_the_rows_and_columns(plan_tool):
    """For every H and a few batch sizes, class counts and widths: ceil(B H / 4) row workgroups, ceil(W / TX) column tiles per
    plane and B ncls of those; so the last row workgroup and the last tile of a plane are not empty and none is missing."""
    H = np.arange(1, S.SDM_MAX_DIM + 1)
    tx = np.array([S.tx_of(h) for h in H])
    for B, ncls in ((1, 2), (3, 9), (5, 255)):
        for W in (1, 15, 16, 17, 63, 64, 65, 224, 2047):
            got = plan_tool(np.stack([np.full_like(H, B), np.full_like(H, ncls), H, np.full_like(H, W)], 1))
            assert (got[:, OK] == 1).all() and np.array_equal(got[:, TX], tx)
            assert np.array_equal(got[:, ROW_BLOCKS], -(-(B * H) // 4))
            assert np.array_equal(got[:, TILES], -(-W // tx))
            assert np.array_equal(got[:, COL_BLOCKS], B * ncls * got[:, TILES])


def test_every_height_covers_every_cell_once(plan_tool):
    """The exact ownership check of the next test at every H, at one width that has a partial last tile for each TX."""
    B, ncls, W = 2, 3, 70
    H = np.arange(1, S.SDM_MAX_DIM + 1)
    got = plan_tool(np.stack([np.full_like(H, B), np.full_like(H, ncls), H, np.full_like(H, W)], 1))
    for h, g in zip(H, got):
        rows = np.arange(g[ROW_BLOCKS] * 4)
        assert (rows < B * h).sum() == B * h and (g[ROW_BLOCKS] - 1) * 4 < B * h
        k = np.arange(g[COL_BLOCKS])
        cols = (k % g[TILES])[:, None] * g[TX] + np.arange(g[TX])[None, :]
        cells = ((k // g[TILES])[:, None] * W + cols)[cols < W]
        assert np.array_equal(np.sort(cells), np.arange(B * ncls * W)) and (cols < W).any(1).all()


def test_grids_cover_every_row_and_column_once(plan_tool):
    shapes = [(B, ncls, H, W) for B in (1, 2, 5) for ncls in (2, 9) for H in (1, 3, 4, 5, 128, 129, 224, 257, 2047)
              for W in (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 224, 2047)]
    shapes += [c[1:5] for c in S.GPU_CASES]
    got = plan_tool(shapes)
    for (B, ncls, H, W), g in zip(shapes, got):
        assert g[OK] == 1
        # row pass: wave w of workgroup k owns row 4 k + w when it is below B * H
        rows = np.arange(g[ROW_BLOCKS] * 4)
        owned = rows[rows < B * H]
        assert len(owned) == B * H and (g[ROW_BLOCKS] - 1) * 4 < B * H
        # column pass: workgroup k owns columns [t TX, t TX + TX) below W of plane k // tiles, t = k % tiles
        k = np.arange(g[COL_BLOCKS])
        plane, t = k // g[TILES], k % g[TILES]
        cols = t[:, None] * g[TX] + np.arange(g[TX])[None, :]
        live = cols < W
        cells = (plane[:, None] * W + cols)[live]
        assert len(cells) == B * ncls * W and np.array_equal(np.sort(cells), np.arange(B * ncls * W))
        assert live.any(1).all()                                           # no workgroup without a column
        assert g[COL_BLOCKS] == B * ncls * g[TILES]


def test_refusals_have_no_plan(plan_tool):
    bad = [(0, 9, 7, 13), (-1, 9, 7, 13), (2, 1, 7, 13), (2, 0, 7, 13), (2, 256, 7, 13), (2, 9, 0, 13), (2, 9, 7, 0), (2, 9, 2048, 13),
           (2, 9, 7, 2048), (2, 9, -3, 13)]
    got = plan_tool(bad)
    assert not got.any()
    # at every height: a class count or a width outside the limits, and no batch
    H = np.arange(1, S.SDM_MAX_DIM + 1)
    for B, ncls, W in ((2, 1, 13), (2, 256, 13), (2, 9, 0), (2, 9, 2048), (0, 9, 13)):
        assert not plan_tool(np.stack([np.full_like(H, B), np.full_like(H, ncls), H, np.full_like(H, W)], 1)).any()
    for W in (1, 13, 2047):                                                # and every width at the heights just outside
        assert not plan_tool([(2, 9, 0, W), (2, 9, 2048, W), (2, 9, -1, W)]).any()
    edge = plan_tool([(1, 2, 1, 1), (1, 255, 2047, 2047), (2 ** 20, 255, 2047, 2047)])
    assert edge[0, OK] == 1 and edge[1, OK] == 1
    assert edge[2, OK] == 0                                                # more workgroups than one launch has
