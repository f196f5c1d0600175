"""Host side of the eb-criterion mode (csrc/eb.hip, optim.column_tiles, optim.FlatAdamW.tensor_evidence, continual.eb_weights): the
float64 reference and the derived bound that tests/test_gpu_eb.py and tests/test_gpu_eb_step.py use, checked here against torch on
the CPU, against a float32 transcription of the kernel's order and against planted bugs, on the cases the GPU test runs.  No GPU."""
import math

import numpy as np
import pytest
import torch

from cswin_unet_amd.continual import eb_metrics, eb_weights, surgical_lr_weights
from cswin_unet_amd.optim import column_tiles
from oracle.determ import det_normal

from test_adamw_host import U, cdiv, elem_mask, slots

EPS = 1e-8
COLS = 64                       # columns of a tile at the most (optim._EB_COLS)


# ------------------------------------------------------------------------------------------------
# the table's rule, restated
# ------------------------------------------------------------------------------------------------
def rows_cols(shape):
    """(d0, inner) of a tensor: rows along dimension 0, every other index a column; () counts as (1,)."""
    shape = tuple(shape) or (1,)
    return shape[0], math.prod(shape[1:])


def tiles_of(inner):
    """[(col0, ncols, width)] of a tensor's tiles: 64 columns each, the last one the rest; width the smallest power of two >= ncols."""
    out = []
    for col0 in range(0, inner, COLS):
        ncols = min(COLS, inner - col0)
        out.append((col0, ncols, 1 << (ncols - 1).bit_length()))
    return out


# ------------------------------------------------------------------------------------------------
# float64 reference and the bound
# ------------------------------------------------------------------------------------------------
def eb_ref(g, shape):
    """mean(g * g / (var(g, dim 0, unbiased) + 1e-8)) in float64, column by column; NaN when shape[0] == 1 (0 / 0)."""
    d0, inner = rows_cols(shape)
    g = np.asarray(g, np.float64).reshape(d0, inner)
    with np.errstate(invalid="ignore", divide="ignore"):
        m2 = ((g - g.mean(0)) ** 2).sum(0)
        var = m2 / (d0 - 1)
        return float(((g * g).sum(0) / (var + EPS)).sum() / g.size)


def eb_bound(g, shape):
    """What the kernel's float32 evidence may differ by from eb_ref, to first order in U = 2^-24 (the denominator exactly), from
    the magnitudes involved.  Counted from csrc/eb.hip, every operation at one rounding except the divisions, taken at two, and
    without relying on contraction.  Per column of n = d0 rows in a tile of width w: R = 256 / w row phases, a thread takes at
    most T = ceil(n / R) rows in row order, the R phase partials are added in phase order: a term passes D = T + R additions.
    With k = g_0 (the shift), d_i = g_i - k, S = sum d, Sabs = sum |d|, A = sum d^2, Q = sum g^2, B = S^2 / n, M2 = A - B:

      d^  = fl(g - k)                            |d^ - d| <= U |d|
      s1  = sum d^                               e1 = (D + 1) U Sabs
      s2  = sum d^ d^                            (D + 3) U A          (2 from d^, the square, the depth)
      q   = sum g g                              (D + 1) U Q
      b   = fl(fl(s1 s1) / n)                    2 |S| e1 / n + e1^2 / n + 3 U B     (the product 1, the division 2)
      m2  = fl(s2 - b)                           eM = (D + 3) U A + 2 |S| e1 / n + e1^2 / n + 3 U B + U M2
      var = fl(m2 / (n - 1)), clamped at 0       eV = eM / (n - 1) + 2 U var         (the clamp moves toward var >= 0)
      den = fl(var + 1e-8f)                      eD = eV + U 1e-8 + U (var + 1e-8)   (1e-8f is 1e-8 rounded)
      t   = fl(q / den)                          |t^ - t| <= t ((D + 3) U + eD / (den - eD)), infinite where eD >= den

    A >= B, so a column whose shift lies far from its mean in units of its spread has a large A / M2 and a wide bound: that is the
    cancellation the shifted form is left with, and the bound says so instead of hiding it.  The column terms of a tile meet in
    a 6-level butterfly, a tensor's tiles are added in tile order and the sum is divided by numel: (6 + tiles + 2) U of the sum of
    the terms (all are >= 0).  NaN for d0 == 1."""
    d0, inner = rows_cols(shape)
    g = np.asarray(g, np.float64).reshape(d0, inner)
    if d0 == 1:
        return float("nan")
    n = d0
    depth = np.empty(inner)
    for col0, ncols, width in tiles_of(inner):
        R = 256 // width
        depth[col0:col0 + ncols] = cdiv(n, R) + R
    d = g - g[0]
    S, Sabs, A, Q = d.sum(0), np.abs(d).sum(0), (d * d).sum(0), (g * g).sum(0)
    B = S * S / n
    M2 = ((g - g.mean(0)) ** 2).sum(0)
    var = M2 / (n - 1)
    e1 = (depth + 1) * U * Sabs
    eM = (depth + 3) * U * A + 2 * np.abs(S) * e1 / n + e1 * e1 / n + 3 * U * B + U * M2
    eV = eM / (n - 1) + 2 * U * var
    den = var + EPS
    eD = eV + U * EPS + U * den
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(eD < den, eD / (den - eD), np.inf)
        t = Q / den
        eT = np.where(t > 0, t * ((depth + 3) * U + rel), 0.0)
    return float((eT.sum() + (6 + len(tiles_of(inner)) + 2) * U * t.sum()) / g.size)


# ------------------------------------------------------------------------------------------------
# the kernel's order in numpy float32, and the bugs the bound must see
# ------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    """fl32(a * b + c): the product of two float32 is exact in float64."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def eb_fp32(g, shape, contract=True):
    """csrc/eb.hip's operations in its order in float32: (evidence, tile partials).  contract=False: separate multiply and add."""
    f = np.float32
    d0, inner = rows_cols(shape)
    g = np.asarray(g, f).reshape(d0, inner)
    partial = []
    with np.errstate(invalid="ignore", divide="ignore"):
        for col0, ncols, width in tiles_of(inner):
            R = 256 // width
            T = cdiv(d0, R)
            x = np.zeros((T * R, ncols), f)
            x[:d0] = g[:, col0:col0 + ncols]
            live = (np.arange(T * R) < d0).reshape(T, R, 1)
            x = x.reshape(T, R, ncols)                       # x[i, r] = row r + i R: phase r's i-th row
            k = g[0, col0:col0 + ncols]
            s1, s2, q = (np.zeros((R, ncols), f) for _ in range(3))
            for i in range(T):
                d = x[i] - k
                s1 = np.where(live[i], s1 + d, s1)
                s2 = np.where(live[i], _fma(d, d, s2) if contract else s2 + d * d, s2)
                q = np.where(live[i], _fma(x[i], x[i], q) if contract else q + x[i] * x[i], q)
            S1, S2, Q = (np.zeros(ncols, f) for _ in range(3))
            for r in range(R):                               # phase order
                S1, S2, Q = S1 + s1[r], S2 + s2[r], Q + q[r]
            var = (S2 - S1 * S1 / f(d0)) / f(d0 - 1)
            var = np.where(var < 0, f(0), var)
            lanes = np.zeros(64, f)
            lanes[:ncols] = Q / (var + f(EPS))
            for o in (32, 16, 8, 4, 2, 1):                   # the xor butterfly of wave 0
                lanes = lanes + lanes[np.arange(64) ^ o]
            partial.append(lanes[0])
        s = f(0)
        for p in partial:
            s = s + p
        return f(s / f(g.size)), np.array(partial, f)


WRONG = ("biased_variance", "no_eps", "last_axis", "whole_tensor", "per_column_count", "naive_variance")


def eb_wrong(g, shape, wrong):
    """The metric with one planted bug: in float64, except the naive variance, whose fault is float32's."""
    d0, inner = rows_cols(shape)
    shape = tuple(shape) or (1,)
    g32 = np.asarray(g, np.float32).reshape(shape)
    g = g32.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        if wrong == "biased_variance":
            var = g.var(0, keepdims=True)
        elif wrong == "last_axis":
            var = g.var(-1, ddof=1, keepdims=True)
        elif wrong == "whole_tensor":
            var = g.var(ddof=1)
        elif wrong == "naive_variance":
            n = np.float32(d0)
            s, q = g32.sum(0, keepdims=True, dtype=np.float32), (g32 * g32).sum(0, keepdims=True, dtype=np.float32)
            var = ((q - s * s / n) / np.float32(d0 - 1)).astype(np.float64)
        else:
            var = g.var(0, ddof=1, keepdims=True)
        terms = g * g / (var + (0.0 if wrong == "no_eps" else EPS))
        return float(terms.sum() / (inner if wrong == "per_column_count" else g.size))


# ------------------------------------------------------------------------------------------------
# the cases shared with the GPU test
# ------------------------------------------------------------------------------------------------
BIAS_ROWS = (1, 2, 3, 5, 9, 255, 256, 257, 2048)
SHAPES = [(n,) for n in BIAS_ROWS] + [(4, 3), (12, 9), (5, 15), (5, 16), (5, 17), (7, 63), (7, 64), (7, 65), (64, 3, 7, 7), (257, 129), (2048, 64)]
MANY = [(2, 4)] * 257           # the finalize kernel's second trip starts at tensor 256
KINDS = ("small", "offset", "equal", "zero", "large")
EQUAL = 3e-4                    # the all-equal column: every term is EQUAL^2 / 1e-8 = 9


def eb_inputs(tag, shapes):
    """Per-tensor float32 arrays.  Column j of tensor t is of kind KINDS[(2 t + j) % 5]: N(0, 1) 1e-4 (variance about the 1e-8 term),
    1 + 1e-3 N(0, 1) (the mean dwarfs the spread), all equal and not zero (variance 0, terms g^2 / 1e-8), all zero (terms 0, not
    NaN), N(0, 1) 1e3.  A tensor of five or more columns holds every kind; the one-column tensors take them in turn."""
    out = []
    for t, shape in enumerate(shapes):
        d0, inner = rows_cols(shape)
        z = det_normal(f"eb.{tag}.{t}", (d0, inner)).astype(np.float64)
        kind = (2 * t + np.arange(inner)) % 5
        a = np.select([kind == 0, kind == 1, kind == 2, kind == 3], [z * 1e-4, 1.0 + 1e-3 * z, np.full_like(z, EQUAL), np.zeros_like(z)], z * 1e3)
        out.append(a.astype(np.float32).reshape(tuple(shape) or ()))
    return out


@pytest.fixture(scope="module")
def cases():
    gs = eb_inputs("cases", SHAPES)
    return [(s, g, eb_ref(g, s), eb_bound(g, s)) for s, g in zip(SHAPES, gs)]


# ------------------------------------------------------------------------------------------------
# tests
# ------------------------------------------------------------------------------------------------
@pytest.mark.filterwarnings("ignore:var")
@pytest.mark.parametrize("shape", [(1,), (7,), (1, 5), (6, 5), (2, 3, 4), (5, 1, 3), (4, 2, 3, 3), (1, 2, 2, 2)])
def test_eb_ref_is_the_reference_expression(shape):
    """universal_train.py:669-672 on a CPU float64 tensor, NaN for a first dimension of 1 included."""
    g = det_normal(f"eb.torch.{shape}", shape)
    t = torch.from_numpy(g).double()
    want = float(((t * t) / (torch.var(t, dim=0, keepdim=True) + 1e-8)).mean())
    got = eb_ref(g, shape)
    if shape[0] == 1:
        assert math.isnan(want) and math.isnan(got) and math.isnan(eb_bound(g, shape))
    else:
        assert abs(got - want) <= 1e-12 * abs(want), (got, want)
    assert math.isnan(eb_ref(np.float32(3.0), ()))                      # a 0-dimensional tensor is (1,)


def test_the_cases_sit_on_both_sides_of_the_threshold(cases):
    """The float64 values of the GPU test's tensors: NaN exactly for d0 == 1, and tensors below and above 0.95 by more than their bound."""
    for shape, _, ref, bound in cases:
        assert math.isnan(ref) == (shape[0] == 1) and math.isnan(bound) == (shape[0] == 1), shape
    below = [s for s, _, r, b in cases if r + b < 0.95]
    above = [s for s, _, r, b in cases if r - b > 0.95]
    print("below 0.95:", below, "above:", above)
    assert len(below) >= 2 and len(above) >= 2
    for _, g, _, _ in cases:                                             # every kind of column is there as described
        a = g.reshape(g.shape[0], -1)
        if a.shape[1] >= 5:
            assert any((a[:, j] == 0).all() for j in range(5)) and any((a[:, j] == np.float32(EQUAL)).all() for j in range(5))


@pytest.mark.parametrize("contract", [True, False], ids=["fma", "mul_add"])
def test_the_bound_holds_the_fp32_transcription(cases, contract):
    """The kernel's order in numpy float32, with the fused multiply-adds and without, stays inside the bound on every case; the zero
    and d0 == 1 tensors come out exactly."""
    worst = 0.0
    for shape, g, ref, bound in cases:
        got, _ = eb_fp32(g, shape, contract)
        if shape[0] == 1:
            assert math.isnan(got), shape
            continue
        err = abs(float(got) - ref)
        print(f"{shape}: fp32 {float(got)!r} float64 {ref!r} |diff| {err:.3e} bound {bound:.3e}")
        assert math.isfinite(bound) and err <= bound, (shape, got, ref, bound)
        worst = max(worst, err / bound if bound > 0 else 0.0)
    print("largest error / bound:", worst)
    assert worst >= 1e-3                                                 # the bound is within three decades of what float32 does


# per bug: tensors of the cases that must see it (a one-column tensor cannot tell the first axis from the last, or a column from the tensor)
MUST_SEE = {
    "biased_variance": [(4, 3), (12, 9), (5, 16), (7, 65)],
    "no_eps": [(12, 9), (5, 17), (7, 64), (64, 3, 7, 7)],
    "last_axis": [(4, 3), (12, 9), (7, 63), (64, 3, 7, 7), (257, 129), (2048, 64)],
    "whole_tensor": [(4, 3), (12, 9), (7, 63), (64, 3, 7, 7), (257, 129), (2048, 64)],
    "per_column_count": [(2,), (2048,), (4, 3), (64, 3, 7, 7), (2048, 64)],
    "naive_variance": [(12, 9), (7, 65), (64, 3, 7, 7), (257, 129), (2048, 64)],
}


@pytest.mark.parametrize("wrong", WRONG)
def test_the_bound_rejects_the_wrong_variants(cases, wrong):
    """Each planted bug leaves the bound by a factor of at least 4 on the tensors meant to show it."""
    seen = {}
    for shape, g, ref, bound in cases:
        if shape[0] == 1:
            continue
        got = eb_wrong(g, shape, wrong)
        seen[shape] = abs(got - ref) / bound if bound > 0 and math.isfinite(got) else (0.0 if got == ref else math.inf)
    print(f"{wrong}: |wrong - float64| / bound:", {k: f"{v:.3g}" for k, v in seen.items()})
    assert set(MUST_SEE) == set(WRONG)
    for shape in MUST_SEE[wrong]:
        assert seen[shape] >= 4.0, (wrong, shape, seen[shape])


def _check_table(shapes):
    shapes = [tuple(s) for s in shapes]
    numels = [math.prod(s) for s in shapes]
    offs, total = slots(numels)
    rows, first = column_tiles(shapes, offs)
    assert rows.dtype.itemsize == 32 and rows.dtype.names == ("off", "d0", "inner", "col0", "ncols", "tensor", "width") and first.dtype == np.int32
    assert first[0] == 0 and first[-1] == len(rows) and len(first) == len(shapes) + 1 and (np.diff(first) >= 1).all()
    assert (rows["tensor"][1:] >= rows["tensor"][:-1]).all()
    covered = np.zeros(total, int)
    for t, (s, n, o) in enumerate(zip(shapes, numels, offs)):
        d0, inner = rows_cols(s)
        mine = rows[first[t]:first[t + 1]]
        assert (mine["tensor"] == t).all() and (mine["off"] == o).all() and (mine["d0"] == d0).all() and (mine["inner"] == inner).all()
        assert [(int(r["col0"]), int(r["ncols"]), int(r["width"])) for r in mine] == tiles_of(inner), s       # column order, the widths as specified
        assert d0 * inner == n
        for r in mine:
            idx = o + np.arange(d0)[:, None] * inner + r["col0"] + np.arange(r["ncols"])[None, :]
            covered[idx.reshape(-1)] += 1
    assert (covered == elem_mask(numels)).all()                          # every element once, every pad word never
    assert (rows["ncols"] >= 1).all() and (rows["ncols"] <= rows["width"]).all() and (rows["width"] <= 64).all()
    return rows, first


def test_column_tiles_cover_every_column_once():
    rows, first = _check_table([(), (1,), (5,), (3, 1), (2, 65)])
    assert first.tolist() == [0, 1, 2, 3, 4, 6]
    assert [tuple(int(v) for v in r) for r in rows] == [(0, 1, 1, 0, 1, 0, 1), (8, 1, 1, 0, 1, 1, 1), (16, 5, 1, 0, 1, 2, 1), (24, 3, 1, 0, 1, 3, 1),
                                                        (32, 2, 65, 0, 64, 4, 64), (32, 2, 65, 64, 1, 4, 1)]
    assert rows.view(np.int64).reshape(-1, 4)[4].tolist() == [32, 2 | 65 << 32, 0 | 64 << 32, 4 | 64 << 32]       # the library's 32-byte record
    assert tiles_of(1) == [(0, 1, 1)] and tiles_of(9) == [(0, 9, 16)] and tiles_of(147) == [(0, 64, 64), (64, 64, 64), (128, 19, 32)]
    _check_table(SHAPES)
    _check_table(MANY)
    with pytest.raises(ValueError):
        column_tiles([(3,), (3,)], [0, 4])
    with pytest.raises(ValueError):
        column_tiles([(0, 3)], [0])


def test_column_tiles_on_the_models_shapes():
    """The 463 tensors of the shipped model: the biases get width 1, the depthwise 3x3 kernels width 16, and the non-norm tensors
    have the first dimensions and column counts the kernel was laid out for."""
    from oracle.cswin_oracle import param_shapes
    shapes = param_shapes()
    assert len(shapes) == 463
    rows, first = _check_table(list(shapes.values()))
    keep = [tuple(s) for n, s in shapes.items() if "bn" not in n.lower() and "norm" not in n.lower()]
    assert len(keep) == 349
    assert {rows_cols(s)[1] for s in keep} == {1, 9, 64, 128, 144, 147, 256, 288, 512, 576, 1024, 1152, 2048, 2304}
    assert min(s[0] for s in keep) == 9 and max(s[0] for s in keep) == 2048
    assert sum(len(s) == 1 for s in keep) == 175 and sum(rows_cols(s)[1] == 9 for s in keep) == 50
    width = {int(r["inner"]): int(r["width"]) for r in rows if r["col0"] == 0}
    assert width[1] == 1 and width[9] == 16 and width[147] == 64 and width[64] == 64
    print(f"{len(rows)} tiles for {len(shapes)} tensors; largest tile {int((rows['d0'] * rows['ncols']).max()) * 4} bytes")


def test_eb_weights_threshold_and_mean():
    names = ["stage1.0.qkv.weight", "stage1.0.norm1.weight", "stage1.0.mlp.fc1.bias", "output.weight", "merge1.BN.weight", "nan.weight", "low.weight"]
    below, above = math.nextafter(0.95, 0.0), math.nextafter(0.95, 1.0)
    got = eb_weights(names, [[0.95, 7.0, below, above, 7.0, float("nan"), 0.0]])
    assert got == {names[0]: 1.0, names[2]: 0.0, names[3]: 1.0, names[5]: 0.0, names[6]: 0.0} and list(got) == [names[i] for i in (0, 2, 3, 5, 6)]
    assert all(type(v) is float for v in got.values())
    # the mean over two batches moves a value across the threshold, in both directions; np.array(v).mean(0) in float64 on the values given
    b0, b1 = [1.0, 0.0, 0.2, 0.96, 0.0, 1.0, 0.9], [0.8, 0.0, 1.8, 0.96, 0.0, float("nan"), 1.0]
    two = eb_weights(names, [b0, b1])
    assert eb_weights(names, [b0])[names[0]] == 1.0 and two[names[0]] == 0.0            # (1.0 + 0.8) / 2 = 0.9
    assert eb_weights(names, [b0])[names[2]] == 0.0 and two[names[2]] == 1.0            # (0.2 + 1.8) / 2 = 1.0
    assert two[names[3]] == 1.0 and two[names[5]] == 0.0 and two[names[6]] == 1.0       # a NaN in one batch: a NaN mean, weight 0
    means = eb_metrics(names, [b0, b1])
    for i in (0, 2, 3, 6):
        assert means[names[i]] == float(np.array([b0[i], b1[i]]).mean(0))
    assert math.isnan(means[names[5]]) and list(means) == list(two)
    assert eb_weights(names, torch.tensor([b0, b1], dtype=torch.float32)) == eb_weights(names, [np.float32(b0), np.float32(b1)])
    assert eb_weights(names, [[0.5] * 7], threshold=0.5) == {n: 1.0 for n in got}
    assert eb_weights(names, []) == {} and eb_metrics(names, []) == {}
    with pytest.raises(ValueError):
        eb_weights(names, [[1.0] * 6])


def test_surgical_method_is_validated_first():
    with pytest.raises(ValueError, match="method"):
        surgical_lr_weights(None, None, [], None, method="eb")
