"""The launch policy of the GEMM family on the host (no GPU): the Python transcription in tests/test_gpu_gemm_shapes.py (k_groups,
one_split, choose_split, tiled_config, gemm_plan, wgrad16_plan, batch_plan), from which that file's coverage claims and the
expectations of tests/test_gpu_linear_skip.py are computed, against cswin_unet_amd/csrc/gemm_plan.h itself -- the header the library
launches from --, line for line through tools/gemm_plan_check.cpp: on every row of the case tables, on the model's Linear shapes,
and on sweeps of sizes, alignments, seams, precisions, storage flags and batches.  Then the comparison is shown to be able to
fail: with a tuning variable in the tool's environment (read through the structure the library reads) it disagrees."""
import itertools
import os
import shutil
import subprocess

import pytest

import test_gpu_gemm_shapes as G
from test_gpu_linear_skip import SHAPES as SKIP_SHAPES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# sizes of the sweeps: every threshold of the rules has a neighbour on each side (4, 32, 64, the 256 / 512 reduction lengths of
# k_groups, the 320 / 640 workgroups, 768 and 1024 tiles) and the model's row counts.  N and K: the set without its three largest.
SIZES_M = (1, 3, 4, 8, 30, 32, 33, 63, 64, 65, 100, 127, 128, 129, 192, 256, 257, 260, 512, 513, 644, 768, 1024, 3136, 4704, 18816)
SIZES_NK = SIZES_M[:-3]
# batches: n-tuples of these (an N % 4 != 0 shape, W16_BLOCK's four, a ragged, a one-slab and a DMA-sized one)
BATCH_SHAPES = [(300, 30, 64)] + G.W16_BLOCK(1024) + [(300, 72, 64), (37, 8, 128), (2080, 128, 128)]
TAIL_NK = (96, 32)                     # the tail's data gradient: (M of problem 0, 96) x (96, 32)
BENCH_BATCH = 24                       # the benchmark's batch: the model's Linear shapes per stage as tools/block_linear_table.py lists them


@pytest.fixture(scope="module")
def plan_tool(tmp_path_factory):
    """tools/gemm_plan_check.cpp, compiled with the system C++ compiler: request lines -> the header's plan lines."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("gemm_plan") / "gemm_plan_check")
    subprocess.run([cxx, "-O1", "-std=c++17", "-I", os.path.join(ROOT, "cswin_unet_amd", "csrc"),
                    os.path.join(ROOT, "tools", "gemm_plan_check.cpp"), "-o", exe], check=True)

    def run(requests, **tuning):
        env = {k: v for k, v in os.environ.items() if not k.startswith(G.TUNING_PREFIXES)}
        env.update(tuning)
        out = subprocess.run([exe], input="\n".join(requests) + "\n", capture_output=True, text=True, env=env)
        assert out.returncode == 0, out.stderr
        lines = out.stdout.splitlines()
        assert len(lines) == len(requests)
        return lines
    return run


def line(p):
    """A plan of the transcription as the tool prints it: the kernel's name, then plan_str."""
    return G.plan_str(p) if p["kernel"] in ("gemm16", "wgrad16") else p["kernel"] + " " + G.plan_str(p)


def linear(entry, M, N, K, *, k_split=0, off=(), form="plain", precision=0, io=0):
    """(request, the transcription's line) of one Linear call; the alignment flags say what the entry point tells the header."""
    on = lambda *names: int(not any(n in off for n in names))
    want = line(G.gemm_plan(entry, M, N, K, k_split=k_split, off=off, form=form, precision=precision, io=io))
    if entry == "fwd":
        loads = on("x", "w") and (not k_split or on("x2"))
        outs = on("y", "bias") and (form != "gelu" or on("y_act")) and (form != "res" or on("residual"))
        return f"fwd {M} {N} {K} {k_split} {precision} {io} {int(loads)} {int(outs)}", want
    if entry == "dgrad":
        outs = on("dx") and (form != "gelu" or on("gelu_pre")) and (form != "add" or on("add")) and (form != "split" or on("dx2"))
        seam = k_split if form == "split" else 0
        return f"dgrad {M} {N} {K} {seam} {int(form == 'add')} {precision} {io} {on('dy', 'w')} {int(outs)}", want
    return f"dw {M} {N} {K} {k_split} {precision} {on('dy', 'x')} {on('x2')} {on('workspace')}", want      # the entry point has no io_bf16


def batch(problems, *, precision=0, ios=None, samples=None, off_workspace=(), tail=None, tail_off=()):
    n = len(problems)
    plans, dplan = G.batch_plan(problems, precision=precision, ios=ios, samples=samples, off_workspace=off_workspace, tail=tail, tail_off=tail_off)
    ios, samples = ios or [0] * n, samples or [None] * n
    req = f"batch {n} {precision} " + " ".join(f"{M} {N} {K} {ios[i]} {samples[i] or 0} 0 1 {int(i not in off_workspace)} -1"
                                               for i, (M, N, K) in enumerate(problems))
    tM, tN, tK = tail or (0, 0, 0)
    req += f" {int(tail is not None)} {tM} {tN} {tK} {int('dy' not in tail_off and 'w' not in tail_off)} {int('dx' not in tail_off)} 0 0"
    return req, " | ".join([line(p) for p in plans] + [line(dplan) if dplan else "-"])


def raw(Mo, No, R, splits, wgrad, precision):
    rps = G.one_split(R) if splits == 1 else G.cdiv(G.cdiv(R, splits), 8) * 8
    bm, bn, bk, kw = G.tiled_config(Mo, No, R, splits, rps, wgrad, precision)
    return f"tiled {Mo} {No} {R} {splits} {rps} {int(wgrad)} {precision}", f"{bm}x{bn}x{bk} KW{kw}"


def table_requests():
    """Every row of the case tables of test_gpu_gemm_shapes and test_gpu_linear_skip, and the model's Linear shapes."""
    out = []
    for (shape, off), _ in G.CASES:
        out += [linear(e, *shape, off=off) for e in ("fwd", "dgrad", "dw")]
    for shape, off in G.FORM_ROWS:
        a, b = G.seams(shape[2])
        out += [linear("fwd", *shape, off=off, form=f) for f in ("gelu", "res")]
        out += [linear("dgrad", *shape, off=off, form=f) for f in ("gelu", "add")]
        for seam in (a, b):
            out += [linear("fwd", *shape, k_split=seam), linear("dgrad", *shape, k_split=seam, form="split"), linear("dw", *shape, k_split=seam)]
    for problems, _ in G.BATCHES:
        out += [batch(problems), batch(problems, off_workspace=(1,)) if len(problems) > 1 else batch(problems, off_workspace=(0,))]
    M, C = G.TAIL["M"], G.TAIL["C"]
    out += [batch(G.BATCH_ODD), batch(G.tail_problems(), tail=(M, 3 * C, C)), batch(G.tail_problems(), tail=(M, 3 * C, C), tail_off=("dx",))]
    out += [linear(e, *shape, precision=1) for shape, e, _ in G.TILED16]
    out += [linear(e, *shape, precision=1, io=io) for shape, e, _ in G.GEMM16 for io in (5, 7)]
    out += [batch(problems, precision=1, ios=ios, samples=samples) for problems, ios, samples, _ in G.WGRAD16]
    for (ns, rps, cols, red), _ in SKIP_SHAPES:
        out += [linear("fwd", ns * rps, cols, red), linear("dgrad", ns * rps, red, cols), raw(ns * rps, cols, red, 1, False, 0)]
    for L, C in ((3136, 64), (784, 128), (196, 256), (49, 512)):
        M = BENCH_BATCH * L
        block = [(M, C, 4 * C), (M, 4 * C, C), (M, C, C), (M, 3 * C, C)]                  # fc2, fc1, proj, qkv
        for precision in (0, 1):
            out += [linear(e, *shape, precision=precision) for shape in block for e in ("fwd", "dgrad", "dw")]
            out += [batch(block, precision=precision), batch(block, precision=precision, tail=(M, 3 * C, C))]
        out += [linear(e, *shape, precision=1, io=5) for shape in block for e in ("fwd", "dgrad")]
        out += [batch(block, precision=1, ios=[3] * 4)]
    return out


def linear_sweep():
    """fwd, dgrad and dw over the size product: both precisions, all operands aligned and each named operand alone 4 bytes off,
    no seam and both seams(K), at precision 1 io 0 and 5.  The product is thinned to every other triple (the whole one takes the
    file past half a minute): each size still meets every size of another dimension with half the sizes of the third; raw_sweep
    below, which is what the tile choice rests on, keeps the whole product."""
    names = dict(fwd=("x", "w", "y", "bias"), dgrad=("dy", "w", "dx"), dw=("dy", "x", "workspace"))
    second = dict(fwd="x2", dgrad="dx2", dw="x2")
    for (i, M), (j, N), (k, K) in itertools.product(enumerate(SIZES_M), enumerate(SIZES_NK), enumerate(SIZES_NK)):
        if (i + j + k) % 2:
            continue
        for seam in (0,) + G.seams(K):
            if seam >= K:
                continue
            for entry in ("fwd", "dgrad", "dw"):
                offs = [()] + [(o,) for o in names[entry] + ((second[entry],) if seam else ())]
                form = "split" if entry == "dgrad" and seam else "plain"
                for off in offs:
                    yield linear(entry, M, N, K, k_split=seam, off=off, form=form)
                    yield linear(entry, M, N, K, k_split=seam, off=off, form=form, precision=1)
                    if entry != "dw":                                    # cswin_linear_bwd_weight has no io_bf16
                        yield linear(entry, M, N, K, k_split=seam, off=off, form=form, precision=1, io=5)


def batch_sweep():
    """Every n-tuple, n = 1..4, of BATCH_SHAPES: both precisions; no tail, an aligned tail and one with dx off; no workspace off
    and problem 0's; at precision 1 ios all 0 and all 3, with and without a row scale."""
    for n in range(1, 5):
        for problems in itertools.product(BATCH_SHAPES, repeat=n):
            tail = (problems[0][0],) + TAIL_NK
            aligned = all(N % 4 == 0 and K % 4 == 0 for _, N, K in problems)
            scale = [G.sample_rows(M) for M, _, _ in problems]
            for t, off_ws in itertools.product((dict(), dict(tail=tail), dict(tail=tail, tail_off=("dx",))), ((), (0,))):
                yield batch(problems, off_workspace=off_ws, **t)
                for io, samples in itertools.product((0, 3), (None, scale)):
                    if io == 0 or (aligned and not off_ws):               # bf16 storage on an unaligned problem is refused
                        yield batch(problems, precision=1, ios=[io] * n, samples=samples, off_workspace=off_ws, **t)


def raw_sweep():
    for Mo, No, R in itertools.product(SIZES_M, SIZES_NK, SIZES_NK):
        for splits, wgrad, precision in itertools.product((1, 3, 12), (False, True), (0, 1)):
            yield raw(Mo, No, R, splits, wgrad, precision)


@pytest.fixture(scope="module")
def swept():
    """(requests, the transcription's lines) of the tables and the three sweeps, made once."""
    pairs = table_requests() + list(linear_sweep()) + list(batch_sweep()) + list(raw_sweep())
    return [r for r, _ in pairs], [w for _, w in pairs]


def test_transcription_equals_the_header_line_for_line(plan_tool, swept):
    requests, want = swept
    got = plan_tool(requests)
    got = [g.split(" ; ")[0] for g in got]                   # a batch's route follows " ; ": the transcription does not name it
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    print(f"{len(requests)} requests compared, {len(bad)} differ")
    assert not bad, (requests[bad[0]], got[bad[0]], want[bad[0]])


def test_case_table_expectations_are_the_headers(plan_tool):
    """The strings the case tables of test_gpu_gemm_shapes hold, against the tool directly (not through the transcription)."""
    strip = lambda s: s.split(" ; ")[0].replace("tiled ", "").replace("batch ", "")
    for (shape, off), want in G.CASES:
        got = plan_tool([linear(e, *shape, off=off)[0] for e in ("fwd", "dgrad", "dw")])
        assert tuple(strip(g) for g in got) == want, (shape, off, got)
    for problems, want in G.BATCHES:
        got = strip(plan_tool([batch(problems)[0]])[0]).split(" | ")[:-1]
        assert [g.split()[-1] for g in got] == want, (problems, got)
    for problems, ios, samples, want in G.WGRAD16:
        got = strip(plan_tool([batch(problems, precision=1, ios=ios, samples=samples)[0]])[0]).split(" | ")[:-1]
        assert got == want, (problems, got)
    for shape, e, want in G.TILED16:
        assert strip(plan_tool([linear(e, *shape, precision=1)[0]])[0]) == want, (shape, e)
    for shape, e, want in G.GEMM16:
        assert strip(plan_tool([linear(e, *shape, precision=1, io=5)[0]])[0]) == want, (shape, e)
    for (ns, rps, cols, red), config in SKIP_SHAPES:
        assert plan_tool([raw(ns * rps, cols, red, 1, False, 0)[0]])[0] == "%dx%dx%d KW%d" % config


def test_routes_of_the_batch(plan_tool):
    """The route the tool prints after " ; " -- the kernel variant and what rides -- at the launches the GPU tests make."""
    M, C = G.TAIL["M"], G.TAIL["C"]
    route = lambda req: plan_tool([req])[0].split(" ; ")[1]
    with_jobs = lambda req, order=0: req.rsplit(" ", 2)[0] + f" {order} 2"
    masked = lambda req: req.replace(" 0 0 0 1 1 -1", " 0 37 1 1 1 -1", 1)                   # problem 0 with a row scale and a mask
    plain, tail = batch(G.tail_problems())[0], batch(G.tail_problems(), tail=(M, 3 * C, C))[0]
    assert route(plain) == "plain" and route(masked(plain)) == "masked"
    assert route(with_jobs(plain)) == "tail jobs_ride"                                      # pending reductions alone ride too
    assert route(tail) == "tail" and route(masked(tail)) == "tail_masked" and route(with_jobs(tail, 1)) == "tail_order jobs_ride"
    assert route(with_jobs(batch(G.tail_problems(), tail=(M, 3 * C, C), tail_off=("dx",))[0])) == "plain dgrad_first jobs_first"
    assert route(with_jobs(batch(G.BATCH_ODD, tail=(M, 3 * C, C))[0])) == "separate dgrad_first jobs_first"
    w16 = batch(G.W16_BLOCK(1024), precision=1, ios=[3] * 4, tail=(1024, 96, 32))[0]
    assert route(w16) == "wgrad16 dgrad_first" and route(with_jobs(w16)) == "wgrad16 dgrad_first jobs_ride"


@pytest.mark.parametrize("var,value", [("CSWIN_GEMM_PEN2", "1.0"), ("CSWIN_GEMM_SPLIT_WGS", "512"), ("CSWIN_W16_WGS", "512")])
def test_the_comparison_can_fail(plan_tool, swept, var, value):
    """With a tuning variable set the tool departs from the transcription (which holds the defaults): the comparison above sees a
    moved threshold, and the tool reads the tuning structure the library reads."""
    requests, want = swept
    got = [g.split(" ; ")[0] for g in plan_tool(requests, **{var: value})]
    differ = sum(g != w for g, w in zip(got, want))
    print(f"{var}={value}: {differ} of {len(requests)} requests differ")
    assert differ > 0
