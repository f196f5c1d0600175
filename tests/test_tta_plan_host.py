"""Views and launch policy of the test-time-augmentation kernels on the host (no GPU): cswin_unet_amd/csrc/tta_plan.h itself --
the header csrc/tta.hip maps pixels and launches with -- through tools/tta_plan_check.cpp, compiled with the system C++ compiler
and no HIP include path.  The index map against numpy for every code; the view list's packing and refusals; the grids, thread
counts and LDS size against what the kernels index and what the hardware gives a kernel without opt-in."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import tta_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE, LD, VIEW_TILE, REG_CLS, STAGE_CH, MAX_DIM = 16, 17, 32, 16, 8, 2048
LDS_PLAIN = 64 * 1024                   # above it a kernel needs the dynamic-LDS opt-in
OK, BAD_COUNT, BAD_CODE, NOT_SQUARE = range(4)


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("tta_plan") / "tta_plan_check")
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "cswin_unet_amd", "csrc"),
                    os.path.join(ROOT, "tools", "tta_plan_check.cpp"), "-o", exe], check=True)

    def run(requests):
        out = subprocess.run([exe], input="\n".join(requests) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        lines = out.stdout.splitlines()
        assert len(lines) == len(requests)
        return lines
    return run


def test_the_headers_index_map_is_numpys(tool):
    """apply the view with numpy to a slice of distinct values, and find every source pixel where the header says it is."""
    shapes = [(5, 5, T.CODES), (3, 7, T.STRAIGHT), (1, 1, T.CODES), (33, 33, T.CODES), (17, 40, T.STRAIGHT)]
    reqs = [(c, h, w) for h, w, codes in shapes for c in codes]
    for (c, h, w), line in zip(reqs, tool([f"pos {c} {h} {w}" for c, h, w in reqs])):
        ij = np.array(line.split(), np.int64).reshape(h, w, 2)
        x = np.arange(h * w).reshape(h, w)
        a = T.view_np(x, c)
        assert ij[..., 0].min() >= 0 and ij[..., 0].max() < a.shape[0] and ij[..., 1].min() >= 0 and ij[..., 1].max() < a.shape[1]
        assert np.array_equal(a[ij[..., 0], ij[..., 1]], x), (c, h, w)
        if h == w and c == 3:
            assert np.array_equal(np.rot90(x, 1)[ij[..., 0], ij[..., 1]], x)
        if h == w and c == 5:
            assert np.array_equal(np.rot90(x, 3)[ij[..., 0], ij[..., 1]], x)


def test_view_lists_are_packed_or_refused(tool):
    cases = [((40, 40), T.CODES), ((17, 40), T.STRAIGHT), ((1, 1), (7,)), ((8, 8), (5, 0, 6)), ((8, 8), (0, 0)),
             ((17, 40), (0, 2, 5)), ((17, 40), (1,)), ((8, 8), (0, 8)), ((8, 8), (-1,)), ((8, 9), (8, 1)), ((8, 8), ()),
             ((8, 8), tuple(range(8)) + (0,))]
    lines = tool([f"views {h} {w} {len(v)} " + " ".join(map(str, v)) for (h, w), v in cases])
    for ((h, w), views), line in zip(cases, lines):
        refusal, bad, packed, any_t = map(int, line.split())
        if not 1 <= len(views) <= 8:
            want = (BAD_COUNT, -1)
        else:
            want = (OK, -1)
            for k, c in enumerate(views):                               # the first offending entry, in list order
                if not 0 <= c <= 7:
                    want = (BAD_CODE, k)
                elif c & 1 and h != w:
                    want = (NOT_SQUARE, k)
                if want[0]:
                    break
        assert (refusal, bad) == want, ((h, w), views)
        if refusal == OK:
            assert [(packed >> (3 * v)) & 7 for v in range(len(views))] == list(views) and packed >> (3 * len(views)) == 0
            assert bool(any_t) == any(c & 1 for c in views)


def test_plans_cover_the_slice_and_fit_the_hardware(tool):
    dims = (1, 8, 31, 32, 33, 40, 64, 224, 225, 512, 2047, 2048)
    reqs = [(V, B, nsel, h, w) for V in (1, 4, 8) for B in (1, 3, 2048) for nsel in (1, 9, 16, 17, 255) for h in dims for w in dims]
    for (V, B, nsel, h, w), line in zip(reqs, tool(["plan %d %d %d %d %d" % r for r in reqs])):
        ens, view = (list(map(int, part.split())) for part in line.split(" | "))
        general, gx, gy, gz, threads, lds = ens
        assert general == (nsel > REG_CLS)
        assert (gx, gy, gz) == (-(-w // TILE), -(-h // TILE), B) and gx * TILE >= w > (gx - 1) * TILE and gy * TILE >= h > (gy - 1) * TILE
        assert 128 <= threads == TILE * TILE <= 1024 and gz <= 65535 and gx <= 65535 and gy <= 65535      # two waves make the lists
        # staged channels, the class tile (bytes), two int lists that can hold every output row / column, two counters
        assert lds == 4 * STAGE_CH * TILE * LD + TILE * LD + 2 * 4 * MAX_DIM + 8 <= LDS_PLAIN
        assert view == [-(-w // VIEW_TILE), -(-h // VIEW_TILE), V * B, 256] and V * B <= 65535
    # the padded strides.  view_batch: a column of the 32 x 33 tile (stride 33 floats) and a row (stride 1) each fall on 32
    # different banks.  The ensemble: a 32-lane group covers two tile rows, read as two columns of the staged tile (stride LD)
    # or written as two rows (stride 1): at most two lanes of a group meet on a bank.
    assert len({(k * (VIEW_TILE + 1)) % 32 for k in range(VIEW_TILE)}) == 32
    for ty in range(0, TILE, 32 // TILE):
        rows = range(ty, ty + 32 // TILE)
        read = [(tx * LD + r) % 32 for r in rows for tx in range(TILE)]
        write = [(r * LD + tx) % 32 for r in rows for tx in range(TILE)]
        assert max(read.count(b) for b in set(read)) <= 2 and max(write.count(b) for b in set(write)) <= 2
