"""The pyramid LK reference (tests/_lk_chain_ref.py) against the C oracle byte for byte, against float64 evaluations of
the same formulas within stated bounds, the decomposition identity of the chain, and the mutations of the contract it
must reject.  CPU only."""
import ast
import os
import time

import numpy as np
import pytest

import _f64_ref as F
import _lk_chain_ref as L
import _oracle as orc
from introtocomputervision_amd import synth
from test_f64_ref import check_lk

U = 2.0 ** -24
ETA = 2.0 ** -149


def same(a, b):
    """Bit for bit (NaN payloads aside: a NaN matches a NaN), the sign of zero included."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def image(kind, rows, cols, seed):
    rng = np.random.default_rng(seed)
    if kind == "textured":
        return synth.smooth_noise(seed, rows, cols)
    if kind == "random":  # full mantissas: every product and sum rounds
        return (rng.standard_normal((rows, cols)) * 37.3).astype(np.float32)
    if kind == "u8":
        return rng.integers(0, 256, (rows, cols)).astype(np.float32)
    if kind == "blocks":
        img = np.full((rows, cols), 7.0, np.float32)
        img[rows // 3: 2 * rows // 3 + 1, cols // 4: cols // 2 + 1] = 200.0
        return img
    if kind in ("big", "tiny"):
        return synth.smooth_noise(seed, rows, cols) * np.float32(2.0 ** (30 if kind == "big" else -30))
    if kind == "nonfinite":
        img = synth.smooth_noise(seed, rows, cols)
        for k, val in enumerate((np.nan, np.inf, -np.inf)):
            img[rng.integers(0, rows), rng.integers(0, cols)] = val
            img[(k * 5) % rows, 0] = val
        return img
    raise ValueError(kind)


KINDS = ["textured", "random", "u8", "blocks", "big", "tiny", "nonfinite"]
SHAPES = [(1, 1), (1, 9), (9, 1), (2, 3), (135, 241), (67, 121)]


def pair(kind, rows, cols, seed):
    a = image(kind, rows, cols, seed)
    b = np.roll(a, (1, 2), (0, 1)) if rows > 2 and cols > 2 else image(kind, rows, cols, seed + 1)
    return a, np.ascontiguousarray(b)


# The crafted coarse flows of the issue: dyadic values (ties of cvRound(v * 32)), signed zeros, integers, flows one pixel
# and far outside the image, and the values whose conversion is INT_MIN or saturates the 16-bit cell.
WILD = [0.0, -0.0, 3e9, -3e9, 2.0 ** 26, -2.0 ** 26, 2.0 ** 31 / 32, np.nan, np.inf, -np.inf, 1e30, -1e6]


def crafted_flow(kind, rows, cols, seed):
    rng = np.random.default_rng(seed)
    if kind == "dyadic":
        return (rng.integers(-1024, 1024, (rows, cols)) / 256.0).astype(np.float32)
    if kind == "zeros":
        return np.where(rng.random((rows, cols)) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    if kind == "integer":
        return rng.integers(-4, 5, (rows, cols)).astype(np.float32)
    if kind == "outside":  # one pixel past the image, and far past it
        return np.where(rng.random((rows, cols)) < 0.5, np.float32(cols + 1), np.float32(-1e5)).astype(np.float32)
    if kind == "wild":
        f = (rng.standard_normal((rows, cols)) * 1.5).astype(np.float32)
        idx = rng.choice(rows * cols, min(rows * cols, 3 * len(WILD)), replace=False)
        f.flat[idx] = np.resize(np.array(WILD, np.float32), idx.size)
        return f
    if kind == "smooth":
        return (rng.standard_normal((rows, cols)) * 1.5).astype(np.float32)
    raise ValueError(kind)


FLOWS = ["dyadic", "zeros", "integer", "outside", "wild", "smooth"]


# ----------------------------------------------------------------------------------------------- independence ----

def test_reference_imports_no_oracle():
    """The reference restates the contract: parsed imports, so the docstring may still name the oracle."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_lk_chain_ref.py")
    tree = ast.parse(open(path).read())
    names = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            names.update(a.name for a in node.names)
        elif isinstance(node, ast.ImportFrom):
            names.add(node.module or "")
            names.update(a.name for a in node.names)
        elif isinstance(node, ast.Call) and getattr(node.func, "id", None) == "__import__":
            names.add("__import__")
    assert names, "no imports parsed"
    for n in names:
        low = n.lower()
        assert "_oracle" not in low and "ctypes" not in low and "liboracle" not in low and n != "__import__", n
    assert names <= {"math", "numpy", "_edge_ref", "fmaf", "reflect101"}, names


# ---------------------------------------------------------------------------------------- tie to the oracle ------

@pytest.mark.parametrize("rows,cols", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_pyramid_operators_match_oracle(rows, cols, kind):
    img = image(kind, rows, cols, rows * 31 + cols)
    assert same(L.pyr_down(img), orc.pyr_down(img))
    assert same(L.pyr_up(img), orc.pyr_up(img))
    for dr, dc in ((45, 37), (2 * rows + 1, 2 * cols), (rows, 2 * cols + 1), (max(rows // 3, 1), cols), (1, 1), (3, 1)):
        assert same(L.resize_linear(img, dr, dc), orc.resize_linear(img, dr, dc)), (dr, dc)
    g = L.gaussian_pyramid(img, 3 if min(rows, cols) >= 4 else 1)
    assert all(same(a, b) for a, b in zip(g, orc.gaussian_pyramid(img, len(g))))


@pytest.mark.parametrize("rows,cols", SHAPES)
@pytest.mark.parametrize("flow", FLOWS)
def test_warp_matches_oracle(rows, cols, flow):
    img = image("nonfinite" if flow == "smooth" else "textured", rows, cols, rows + cols)
    du = crafted_flow(flow, rows, cols, 1)
    dv = crafted_flow(flow, rows, cols, 2)
    assert same(L.warp(img, du, dv), orc.lk_warp(img, du, dv))
    mx = (np.arange(cols, dtype=np.float32)[None, :] + du).astype(np.float32)
    my = (np.arange(rows, dtype=np.float32)[:, None] + dv).astype(np.float32)
    assert same(L.remap_linear(img, mx, my), orc.remap_linear(img, mx, my))


def test_cv_round_ties_and_int_min():
    v = np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 2.0 ** 31, -2.0 ** 31, 2.0 ** 31 - 128, np.nan, np.inf, -np.inf, 1e10],
                 np.float32)
    assert L.cv_round(v).tolist() == [0, 2, 2, 0, -2, -2, L.INT_MIN, L.INT_MIN, 2 ** 31 - 128, L.INT_MIN, L.INT_MIN,
                                      L.INT_MIN, L.INT_MIN]
    assert L.cv_round(v).tolist() == [orc.cv_round(float(x)) for x in v]


@pytest.mark.parametrize("rows,cols,wins", [(1, 1, [1, 3, 43]), (1, 9, [1, 3, 5]), (9, 1, [3, 7]), (2, 3, [1, 3, 5, 9]),
                                            (67, 121, [1, 3, 5, 7, 9, 11, 15, 21, 27, 43]), (135, 241, [15, 21])])
@pytest.mark.parametrize("kind", KINDS)
def test_lk_flow_matches_oracle(rows, cols, wins, kind):
    prev, nxt = pair(kind, rows, cols, rows * 3 + cols)
    for win in wins:
        u, v = L.lk_flow(prev, nxt, win)
        ou, ov = orc.lk_flow(prev, nxt, win)
        assert same(u, ou) and same(v, ov), (kind, win)


def oracle_step(prev, nxt, cu, cv, win):
    """OpticalFlow.cpp:137-162 for one level, composed of the oracle's single operators."""
    rows, cols = prev.shape
    if cu is None:
        du = np.zeros((rows, cols), np.float32)
        dv = np.zeros((rows, cols), np.float32)
    else:
        du = np.float32(2) * orc.pyr_up(cu)
        dv = np.float32(2) * orc.pyr_up(cv)
        if du.shape != (rows, cols):
            du = orc.resize_linear(du, rows, cols)
            dv = orc.resize_linear(dv, rows, cols)
    dx, dy = orc.lk_flow(prev, orc.lk_warp(nxt, du, dv), win)
    return du + dx, dv + dy


@pytest.mark.parametrize("rows,cols,frows,fcols", [(40, 60, 20, 30), (45, 37, 10, 10), (41, 61, 20, 30), (11, 15, 5, 7),
                                                   (3, 3, 1, 1), (64, 16, 32, 8), (37, 45, 30, 50)])
@pytest.mark.parametrize("flow", FLOWS)
def test_level_step_matches_oracle(rows, cols, frows, fcols, flow):
    """Crafted coarse flows of any size: a doubling one (COARSE), odd levels and arbitrary ratios (resize, FULL)."""
    prev, nxt = pair("textured", rows, cols, rows + 5 * cols)
    cu = crafted_flow(flow, frows, fcols, 3)
    cv = crafted_flow(flow, frows, fcols, 4)
    for win in (7, 15):
        got = L.level_step(prev, nxt, cu, cv, win)
        exp = oracle_step(prev, nxt, cu, cv, win)
        assert same(got[0], exp[0]) and same(got[1], exp[1]), win
    got = L.level_step(prev, nxt, None, None, 15)
    exp = oracle_step(prev, nxt, None, None, 15)
    assert same(got[0], exp[0]) and same(got[1], exp[1])


SMALL_PYR = [(1, 1, 1, 1), (1, 9, 3, 1), (9, 1, 3, 1), (2, 3, 3, 1), (2, 3, 5, 2), (135, 241, 15, 4), (135, 241, 21, 7),
             (67, 121, 7, 5), (67, 121, 43, 3), (67, 121, 11, 6)]
PYR_CASES = ([c + (k,) for c in SMALL_PYR for k in ("textured", "random", "u8", "nonfinite")] +
             [(270, 481, 15, 5, "textured"), (270, 481, 15, 5, "nonfinite"), (40, 32767, 5, 2, "textured"),
              (40, 32767, 3, 1, "textured")])


@pytest.mark.parametrize("rows,cols,win,levels,kind", PYR_CASES)
def test_lk_flow_pyr_matches_oracle(rows, cols, win, levels, kind):
    prev, nxt = pair(kind, rows, cols, rows + cols + levels)
    u, v = L.lk_flow_pyr(prev, nxt, win, levels)
    ou, ov = orc.lk_flow_pyr(prev, nxt, win, levels)
    assert same(u, ou) and same(v, ov)


@pytest.mark.parametrize("levels", [1, 2, 3, 4, 5])
def test_laplacian_pyramid_matches_oracle_ops(levels):
    img = image("textured", 135, 241, levels)
    lap = L.laplacian_pyramid(img, levels)
    g = orc.gaussian_pyramid(img, levels)
    assert len(lap) == levels and same(lap[-1], g[-1])
    for i in range(levels - 1):
        up = orc.pyr_up(g[i + 1])
        if up.shape != g[i].shape:
            up = orc.resize_linear(up, *g[i].shape)
        assert same(lap[i], g[i] - up), i


@pytest.mark.parametrize("cn", [1, 3, 4])
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_to_gray_matches_oracle(cn, dtype):
    rng = np.random.default_rng(cn)
    shape = (37, 53) if cn == 1 else (37, 53, cn)
    frame = rng.integers(0, 256, shape).astype(dtype) if dtype == np.uint8 else (rng.random(shape) * 300 - 20).astype(dtype)
    assert same(L.to_gray(frame), orc.to_gray(frame))


# ------------------------------------------------------------------------------- tie to the float64 references ---

def gamma(n):
    return n * U / (1 - n * U)


@pytest.mark.parametrize("kind", ["textured", "random", "u8", "blocks", "big", "tiny"])
@pytest.mark.parametrize("win", [3, 15, 43])
def test_lk_flow_inside_f64_bounds(kind, win):
    prev, nxt = pair(kind, 67, 121, win)
    check_lk(*L.lk_flow(prev, nxt, win), F.lk_flow(prev, nxt, win), f"chain ref lk {kind} win {win}")


def sep64(x, k, replicate=False):
    rows, cols = x.shape
    a = len(k) // 2
    t = sum(float(k[j]) * x[:, L._index(cols, j - a)] for j in range(len(k)))
    return sum(float(k[j]) * t[L._index(rows, j - a), :] for j in range(len(k)))


@pytest.mark.parametrize("kind", ["textured", "random", "big", "tiny"])
def test_pyr_up_within_gamma_of_float64(kind):
    """The blur's taps are exact dyadics: the float64 filter of the replicated image is exact, and any float32
    evaluation of two 5-term passes is within gamma_5 (2 + gamma_5) of F(|x|) (+ underflow)."""
    img = image(kind, 45, 37, 9)
    up = np.repeat(np.repeat(img.astype(np.float64), 2, 0), 2, 1)
    exact = sep64(up, L.G5)
    bound = (gamma(5) * (2 + gamma(5))) * sep64(np.abs(up), L.G5) + 36 * ETA
    err = np.abs(L.pyr_up(img).astype(np.float64) - exact)
    assert np.all(err <= bound), float(np.max(err - bound))


@pytest.mark.parametrize("src,dst", [((10, 10), (45, 37)), ((45, 37), (10, 10)), ((67, 121), (135, 241)), ((3, 1), (7, 5))])
def test_resize_within_gamma_of_float64(src, dst):
    """Half-pixel-centre bilinear interpolation in float64 with the same (float) sample positions: two blends of two
    terms, gamma_2 each, plus the float weights 1 - f (exact: f is a float in [0, 1) with ulp >= 2^-24... up to u)."""
    x = image("random", *src, 3).astype(np.float64)
    sy, fy = L._resize_axis(src[0], dst[0])
    sx, fx = L._resize_axis(src[1], dst[1])
    fx = np.where(sx < 0, 0.0, fx).astype(np.float64)
    sx = np.maximum(sx, 0)
    fx = np.where(sx + 1 >= src[1], 0.0, fx)
    sx = np.minimum(sx, src[1] - 1)
    fy = fy.astype(np.float64)
    h = x[:, sx] * (1 - fx) + x[:, np.minimum(sx + 1, src[1] - 1)] * fx
    y0, y1 = np.clip(sy, 0, src[0] - 1), np.clip(sy + 1, 0, src[0] - 1)
    exact = h[y0] * (1 - fy)[:, None] + h[y1] * fy[:, None]
    mag = np.abs(x).max()
    bound = (2 * gamma(2) + 4 * U) * mag + 4 * ETA
    err = np.abs(L.resize_linear(x.astype(np.float32), *dst).astype(np.float64) - exact)
    assert np.all(err <= bound), float(np.max(err - bound))


def test_remap_within_gamma_of_float64():
    """Bilinear interpolation on the 1/32 grid in float64: the map rounded to the grid (half to even) and taps outside
    read 0; the float blend of four exact-weight products is within gamma_4 sum |v w|."""
    rng = np.random.default_rng(5)
    img = image("random", 40, 50, 1).astype(np.float64)
    mx = (rng.random((40, 50)) * 56 - 3).astype(np.float32)
    my = (rng.random((40, 50)) * 46 - 3).astype(np.float32)
    X = np.rint(mx.astype(np.float64) * 32)
    Y = np.rint(my.astype(np.float64) * 32)
    x0, y0 = np.floor(X / 32).astype(int), np.floor(Y / 32).astype(int)
    fx, fy = X / 32 - x0, Y / 32 - y0
    exact = np.zeros(mx.shape)
    mass = np.zeros(mx.shape)
    for dy, wy in ((0, 1 - fy), (1, fy)):
        for dx, wx in ((0, 1 - fx), (1, fx)):
            yy, xx = y0 + dy, x0 + dx
            ok = (yy >= 0) & (yy < 40) & (xx >= 0) & (xx < 50)
            v = np.where(ok, img[np.clip(yy, 0, 39), np.clip(xx, 0, 49)], 0.0)
            exact += v * wy * wx
            mass += np.abs(v * wy * wx)
    err = np.abs(L.remap_linear(img.astype(np.float32), mx, my).astype(np.float64) - exact)
    assert np.all(err <= gamma(4) * mass + 4 * ETA)


# ------------------------------------------------------------------------------------ decomposition identity ---

@pytest.mark.parametrize("rows,cols,win,levels", [(135, 241, 15, 4), (67, 121, 7, 3), (64, 64, 21, 2), (41, 30, 3, 5)])
def test_decomposition_identity(rows, cols, win, levels):
    """lk_flow_pyr(P, N, w, L) == level_step(P, N, *lk_flow_pyr(pyrDown P, pyrDown N, w, L - 1), w)."""
    prev, nxt = pair("textured", rows, cols, levels)
    full = L.lk_flow_pyr(prev, nxt, win, levels)
    cu, cv = L.lk_flow_pyr(L.pyr_down(prev), L.pyr_down(nxt), win, levels - 1)
    step = L.level_step(prev, nxt, cu, cv, win)
    assert same(full[0], step[0]) and same(full[1], step[1])
    one = L.lk_flow_pyr(prev, nxt, win, 1)
    base = L.level_step(prev, nxt, None, None, win)
    assert same(one[0], base[0]) and same(one[1], base[1])


def test_speed_is_recorded():
    """The docstring's first timing (lk_flow at 256 x 512, window 15) stays in its range on one core."""
    prev, nxt = synth.lk_pair(3, 256, 512, 2, -1)
    t = time.perf_counter()
    L.lk_flow(prev, nxt, 15)
    assert time.perf_counter() - t < 10.0


# ---------------------------------------------------------------------------------------------- mutations ------
# Each mutation of the contract must change the result on the named input, where the reference is the oracle's.
# MUTATION_CASES[name] = (function of the mutation set -> result, oracle result).

def _pyr_case(mut, rows=67, cols=121, win=7, levels=3, kind="textured"):
    prev, nxt = pair(kind, rows, cols, 11)
    return L.lk_flow_pyr(prev, nxt, win, levels, mut)


def _pyr_oracle(rows=67, cols=121, win=7, levels=3, kind="textured"):
    prev, nxt = pair(kind, rows, cols, 11)
    return orc.lk_flow_pyr(prev, nxt, win, levels)


def _step_case(flow, frows, fcols, rows=40, cols=60):
    prev, nxt = pair("textured", rows, cols, 13)
    cu, cv = crafted_flow(flow, frows, fcols, 3), crafted_flow(flow, frows, fcols, 4)
    return (lambda mut: L.level_step(prev, nxt, cu, cv, 15, mut)), oracle_step(prev, nxt, cu, cv, 15)


def _warp_case(src_kind, du, dv, rows=20, cols=30):
    img = image(src_kind, rows, cols, 17)
    du = np.broadcast_to(np.float32(du), (rows, cols)).astype(np.float32)
    dv = np.broadcast_to(np.float32(dv), (rows, cols)).astype(np.float32)
    return (lambda mut: L.warp(img, du, dv, mut)), orc.lk_warp(img, du, dv)


def _inf_neighbour_warp():
    """An infinite pixel right of the sampled column: its weight is 0 on an integer map, 0 * inf = NaN."""
    img = image("textured", 20, 30, 1)
    img[:, 10] = np.inf
    du = np.zeros((20, 30), np.float32)
    dv = np.full((20, 30), 0.25, np.float32)
    return (lambda mut: L.warp(img, du, dv, mut)), orc.lk_warp(img, du, dv)


def _gray_case():
    rng = np.random.default_rng(2)
    frame = rng.integers(0, 256, (9, 11, 3)).astype(np.uint8)
    return (lambda mut: L.to_gray(frame, mut)), orc.to_gray(frame)


def _big_map_warp():
    """Map sum float(x) + du at x >= 4096 with du = 2^-6 + 2^-20: in float32 the sum rounds to x + 2^-6, whose
    v * 32 is a tie that goes to the even grid index; in double it is past the tie and rounds up."""
    img = image("textured", 4, 4200, 3)
    du = np.full((4, 4200), 2.0 ** -6 + 2.0 ** -20, np.float32)
    dv = np.zeros((4, 4200), np.float32)
    return (lambda mut: L.warp(img, du, dv, mut)), orc.lk_warp(img, du, dv)


def _resize_case():
    prev, nxt = pair("textured", 45, 37, 3)
    cu, cv = crafted_flow("smooth", 10, 10, 1), crafted_flow("smooth", 10, 10, 2)
    return (lambda mut: L.level_step(prev, nxt, cu, cv, 7, mut)), oracle_step(prev, nxt, cu, cv, 7)


def _pyr(**kw):
    return (lambda mut: _pyr_case(mut, **kw)), _pyr_oracle(**kw)


def _laplacian():
    img = image("textured", 67, 121, 4)
    g = orc.gaussian_pyramid(img, 3)
    exp = []
    for i in range(2):
        up = orc.pyr_up(g[i + 1])
        exp.append(g[i] - (orc.resize_linear(up, *g[i].shape) if up.shape != g[i].shape else up))
    return (lambda mut: L.laplacian_pyramid(img, 3, mut)[:2]), exp


MUTATION_CASES = {
    "pyrdown_blur": lambda: _pyr(),
    "pyrdown_even": lambda: _pyr(),
    "pyrup_zero_insert": _laplacian,
    "pyrup_replicate": _laplacian,
    "expand_no_x2": lambda: _step_case("smooth", 20, 30),
    "resize_skip": _resize_case,
    "resize_align_corners": _resize_case,
    "map_minus": lambda: _warp_case("textured", 1.25, -0.5),
    "round_floor": lambda: _warp_case("textured", 0.03, 0.0),
    "round_half_away": lambda: _warp_case("textured", 2.0 ** -6, 0.0),   # v * 32 = 0.5: a tie
    "map_double": _big_map_warp,
    "skip_zero_taps": _inf_neighbour_warp,
    "fused_blend": lambda: _warp_case("random", 0.40625, 0.71875),
    "remap_replicate": lambda: _warp_case("textured", 2.5, 1.5),
    "no_coarsest_warp": lambda: _pyr(kind="nonfinite", levels=1),  # a zero-flow warp is the identity on finite pixels
    "replace_du": lambda: _pyr(),
    "gray_bgr": _gray_case,
}


def _outputs(r):
    return list(r) if isinstance(r, (tuple, list)) else [r]


def test_every_mutation_has_a_case():
    assert set(MUTATION_CASES) == set(L.MUTATIONS)


@pytest.mark.parametrize("name", sorted(MUTATION_CASES))
def test_mutation_changes_the_result(name):
    fn, oracle = MUTATION_CASES[name]()
    ref = _outputs(fn(()))
    assert all(same(a, b) for a, b in zip(ref, _outputs(oracle))), "the unmutated reference is the oracle's"
    mutant = _outputs(fn((name,)))
    assert not all(same(a, b) for a, b in zip(mutant, ref)), f"{name} leaves the result unchanged"
