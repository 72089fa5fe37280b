"""The ps1 references (tests/_hough_ref.py, tests/_edge_ref.py) against the C oracle, byte for byte, and the
mutations of the contract they must reject.  CPU only."""
import math
import os
from fractions import Fraction

import numpy as np
import pytest

import _edge_ref as E
import _hough_ref as H
import _oracle as orc
from introtocomputervision_amd import config, synth

INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


def _random_mask(rows, cols, density, seed):
    return ((np.random.default_rng(seed).random((rows, cols)) < density) * 255).astype(np.uint8)


def _masks():
    """(id, mask): empty, full, random densities, drawn lines / circles, degenerate and large shapes."""
    yield "empty_40x50", np.zeros((40, 50), np.uint8)
    yield "full_37x41", np.full((37, 41), 255, np.uint8)
    yield "full_61x200", np.full((61, 200), 255, np.uint8)
    for shape in ((1, 300), (300, 1), (2, 2), (1, 1), (33, 65), (127, 31)):
        for d in (0.05, 0.5):
            yield f"rand{d}_{shape[0]}x{shape[1]}", _random_mask(*shape, d, shape[0] * 7 + shape[1])
    yield "rand0.2_97x131", _random_mask(97, 131, 0.2, 5)
    yield "drawn_480x640", synth.hough_mask(480, 640, n_lines=8, radii=(20, 40))[0]
    yield "drawn_1080x1920", synth.hough_mask(1080, 1920, n_lines=6, radii=(30,))[0]


MASKS = dict(_masks())


# ------------------------------------------------------------------ lines ------

@pytest.mark.parametrize("name", list(MASKS))
def test_lines_match_oracle(name):
    mask = MASKS[name]
    big = mask.size > 500_000
    for rho_bin, theta_bin in ([(1, 1), (7, 181)] if big else [(1, 1), (2, 7), (3, 1), (4, 181), (5, 7), (6, 1), (7, 1)]):
        exp = orc.hough_lines(mask, rho_bin, theta_bin)
        assert H.lines_dims(*mask.shape, rho_bin, theta_bin)[:2] == exp.shape == orc.hough_lines_dims(*mask.shape, rho_bin, theta_bin)
        assert np.array_equal(H.hough_lines(mask, rho_bin, theta_bin), exp), (rho_bin, theta_bin)


def test_line_bands_sum_to_the_whole():
    """A band (mask rows row0 .. row0 + n of a taller image) is the whole image's accumulator restricted to
    those rows' points; the bands of a partition sum to the whole."""
    mask = _random_mask(90, 70, 0.1, 11)
    for rho_bin, theta_bin in ((1, 1), (3, 7)):
        whole = H.hough_lines(mask, rho_bin, theta_bin)
        total = np.zeros_like(whole)
        for r0, r1 in ((0, 1), (1, 33), (33, 89), (89, 90)):
            band = H.hough_lines(mask[r0:r1], rho_bin, theta_bin, row0=r0, rows=90)
            only = np.zeros_like(mask)
            only[r0:r1] = mask[r0:r1]
            assert np.array_equal(band, orc.hough_lines(only, rho_bin, theta_bin)), (r0, r1)
            total += band
        assert np.array_equal(total, whole)


def test_trig_table_is_the_oracles():
    c, s = np.empty(360, np.float32), np.empty(360, np.float32)
    orc._sig("orc_hough_trig_table", None, [orc.vp, orc.vp])(orc._p(c), orc._p(s))
    hc, hs = H.trig(-90)
    assert np.array_equal(hc, c) and np.array_equal(hs, s)
    assert H.deg_to_rad(90) == np.float32(1.5707964) and float(H.deg_to_rad(90)) > math.pi / 2  # cos(90 deg) < 0


def test_dropped_votes_are_reached():
    """61 x 200, rho_bin 7: 2 maxDist / 7 = 60 exactly, and the far corner's rho 208 + 210 rounds to bin 60 =
    rhoBins -- votes the contract drops."""
    mask = np.full((61, 200), 255, np.uint8)
    under, over = H.dropped_line_votes(mask, 7, 1)
    assert under == 0 and over > 0
    acc = H.hough_lines(mask, 7, 1)
    assert acc.sum() == mask.size * 180 - over
    assert np.array_equal(acc, orc.hough_lines(mask, 7, 1))


# ------------------------------------------------------------------ circles ------

@pytest.mark.parametrize("name", [n for n in MASKS if MASKS[n].size <= 400_000])
def test_circles_match_oracle(name):
    mask = MASKS[name]
    diag = math.hypot(*mask.shape)
    for radius in (0, 1, 2, 30, int(diag) + 1, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1):
        exp = orc.hough_circles(mask, radius)
        got = H.hough_circles(mask, radius)
        assert np.array_equal(got, exp), radius
        if radius > diag:
            assert not got.any()  # every centre lies outside the image


def test_circles_at_1080p_and_bands():
    mask = MASKS["drawn_1080x1920"]
    assert np.array_equal(H.hough_circles(mask, 30), orc.hough_circles(mask, 30))
    mask = _random_mask(100, 80, 0.05, 3)
    for r0, r1 in ((0, 40), (40, 41), (41, 100)):
        only = np.zeros_like(mask)
        only[r0:r1] = mask[r0:r1]
        assert np.array_equal(H.hough_circles(mask[r0:r1], 9, row0=r0, rows=100), orc.hough_circles(only, 9))


def test_circle_tiles_are_loaded_beyond_one_chunk():
    """The dense masks the GPU tests use give one tile a row range of more than 2048 and 8192 points (chunks of the
    LDS point list) -- the fuzz never does."""
    dense = np.full((160, 300), 255, np.uint8)
    in_rows, listed = H.circle_tile_loads(dense, 30)
    assert in_rows > 8192 and listed > 2048
    # and the reference is still the oracle there
    sub = dense[:96, :160]
    assert np.array_equal(H.hough_circles(sub, 30), orc.hough_circles(sub, 30))


# ------------------------------------------------------------------ peaks ------

def _accumulators():
    rng = np.random.default_rng(17)
    yield "small_votes_300x400", rng.integers(-5, 50, (300, 400)).astype(np.int32)
    yield "int32_extremes_64x90", rng.choice(np.array([INT_MIN, INT_MIN + 1, -1, 0, 1, INT_MAX - 1, INT_MAX], np.int64),
                                             (64, 90)).astype(np.int32)
    yield "int32_random_50x70", rng.integers(INT_MIN, INT_MAX, (50, 70), endpoint=True).astype(np.int32)
    yield "negative_33x35", rng.integers(-1000, -990, (33, 35)).astype(np.int32)
    yield "row_1x5000", rng.integers(0, 9, (1, 5000)).astype(np.int32)
    yield "col_5000x1", rng.integers(0, 9, (5000, 1)).astype(np.int32)
    yield "one_1x1", np.array([[7]], np.int32)
    yield "ties_40x50", np.full((40, 50), 3, np.int32)
    yield "lines_acc", orc.hough_lines(MASKS["drawn_480x640"], 1, 1)


ACCS = dict(_accumulators())


@pytest.mark.parametrize("name", list(ACCS))
def test_peaks_match_oracle(name):
    acc = ACCS[name]
    for threshold in (INT_MIN, 0, 5, 300, INT_MAX):
        for num_peaks in (0, 1, 64, 65, 4096):
            exp = orc.hough_peaks(acc, num_peaks, threshold)
            assert np.array_equal(H.hough_peaks(acc, num_peaks, threshold), exp), (threshold, num_peaks)


def test_local_maximum_rule_is_up_left_as_written():
    """The exclusive bounds look at (y-1, x-1), (y-1, x) and (y, x-1) only; the last row skips (y, x-1) and the
    last column skips (y-1, x) -- so a larger neighbour below, to the right, or above a last-column cell is
    not looked at."""
    acc = np.zeros((4, 4), np.int32)
    acc[1, 1] = 5
    acc[2, 2] = 9          # below-right of (1, 1): not looked at
    acc[3, 0] = 4
    acc[2, 0] = 8          # above the last-row cell (3, 0): looked at
    acc[1, 3] = 6
    acc[0, 3] = 7          # above the last-column cell (1, 3): not looked at
    lm = H.local_maxima(acc)
    assert lm[1, 1] and not lm[3, 0] and lm[1, 3] and lm[0, 3]
    exp = orc.hough_peaks(acc, 16, 1)
    assert np.array_equal(H.hough_peaks(acc, 16, 1), exp)
    assert exp.tolist() == [[2, 2], [2, 0], [0, 3], [1, 3], [1, 1]]


# ------------------------------------------------------------------ edges ------

PS1_YAML = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "config", "ref", "ps1.yaml")


def ps1_edge_configs():
    """{section: (gaussian_size, sigma, low, high)} of every edge_detector_pN section of the reference's ps1.yaml."""
    cfg = config.load(PS1_YAML)
    out = {}
    for k in sorted(cfg):
        if k.startswith("edge_detector_"):
            p = config.edge_params(cfg, k)
            out[k] = (p["gaussian_size"], p["gaussian_sigma"], p["lower_threshold"], p["upper_threshold"])
    return out


def _scene(rows, cols, seed):
    rng = np.random.default_rng(seed)
    img = np.full((rows, cols), 60, np.int64)
    img[rows // 4: 3 * rows // 4, cols // 5: 4 * cols // 5] = 190
    yy, xx = np.mgrid[0:rows, 0:cols]
    img[(yy - rows // 2) ** 2 + (xx - cols // 2) ** 2 < (min(rows, cols) // 6) ** 2] = 20
    img += rng.integers(-12, 13, (rows, cols))
    return np.clip(img, 0, 255).astype(np.uint8)


def _oracle_edges(img, gs, sigma, lo, hi):
    import ctypes as C
    fn = orc._sig("orc_generate_edge", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_double,
                                                 C.c_double, C.c_double, C.c_void_p, C.c_size_t])
    img = np.ascontiguousarray(img, np.uint8)
    out = np.empty_like(img)
    assert fn(img.ctypes.data, img.shape[0], img.shape[1], img.shape[1], gs, sigma, lo, hi, out.ctypes.data,
              img.shape[1]) == 0
    return out


def _oracle_blur(img, n, sigma):
    import ctypes as C
    fn = orc._sig("orc_gauss_u8", None, [C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_double, C.c_void_p,
                                         C.c_size_t])
    img = np.ascontiguousarray(img, np.uint8)
    out = np.empty_like(img)
    fn(img.ctypes.data, img.shape[0], img.shape[1], img.shape[1], n, sigma, out.ctypes.data, img.shape[1])
    return out


def test_ps1_config_has_the_expected_edge_settings():
    cfg = ps1_edge_configs()
    assert len(cfg) == 7 and cfg["edge_detector_p3"] == (19, 4.0, 10, 50)


@pytest.mark.parametrize("shape", [(1, 70), (70, 1), (2, 2), (33, 35), (97, 131), (480, 640)])
def test_edges_match_oracle(shape):
    img = _scene(*shape, seed=shape[0]) if min(shape) > 8 else \
        np.random.default_rng(shape[1]).integers(0, 256, shape).astype(np.uint8)
    for key, (gs, sigma, lo, hi) in sorted(ps1_edge_configs().items()):
        exp = _oracle_edges(img, gs, sigma, lo, hi)
        assert np.array_equal(E.generate_edge(img, gs, sigma, lo, hi), exp), key


def test_edges_match_oracle_1080p_and_noise():
    img = _scene(1080, 1920, seed=3)
    assert np.array_equal(E.generate_edge(img, 5, 1.5, 30, 90), _oracle_edges(img, 5, 1.5, 30, 90))
    noise = np.random.default_rng(147).integers(0, 256, (70, 107)).astype(np.uint8)
    for gs, sigma, lo, hi in ((31, 2.125, 0, 102), (1, 0.0001, 100, 20), (3, 1.0, 0.5, 0.9)):
        assert np.array_equal(E.generate_edge(noise, gs, sigma, lo, hi), _oracle_edges(noise, gs, sigma, lo, hi))


def test_blur_and_taps_match_oracle():
    img = np.random.default_rng(0).integers(0, 256, (256, 256)).astype(np.uint8)
    for n in range(1, 32, 2):
        for sigma in (0.3, 1.0, 4.0):
            gk = np.empty(n, np.float32)
            orc._gk(n, sigma, orc._p(gk))
            assert np.array_equal(E.gaussian_taps(n, sigma), gk)
    for n, sigma in ((1, 0.0001), (3, 1.0), (13, 4.0), (19, 4.0), (31, 6.0)):
        assert np.array_equal(E.blur(img, n, sigma), _oracle_blur(img, n, sigma)), (n, sigma)


# ------------------------------------------------------------------ fmaf ------

def _round_f32(q):
    """A Fraction rounded to the nearest float32, ties to even."""
    f = np.float32(float(q))
    cands = [np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))]
    return min(cands, key=lambda c: (abs(Fraction(float(c)) - q), int(np.float32(c).view(np.uint32)) & 1))


def _adversarial_triples():
    """x * k + acc within 2^-46 ulp of a float32 midpoint (where rounding the float64 sum first goes wrong) and
    exact cancellations."""
    out = []
    for e in (-20, -3, 0, 1, 7, 30):
        for i in (1, 3, 100, 4095):
            for odd in (0, 1):
                acc = np.float32(2.0 ** e * (1 + odd * 2.0 ** -23))
                x = np.float32(1 + i * 2.0 ** -23)
                k = np.float32(2.0 ** (e - 24) * (1 - i * 2.0 ** -23))  # x k = ulp(acc) / 2 (1 - i^2 2^-46)
                for sx, sa in ((1, 1), (-1, -1), (-1, 1), (1, -1)):
                    out.append((np.float32(sx * x), k, np.float32(sa * acc)))
    rng = np.random.default_rng(9)
    for _ in range(200):  # cancellation: acc = -fl(x k), the result is the product's rounding error
        x, k = (np.float32(v) for v in rng.standard_normal(2) * 1000)
        out.append((x, k, np.float32(-(x * k))))
    return out


def test_fmaf_emulation_is_exact():
    rng = np.random.default_rng(1)
    n = 3000
    x = (rng.standard_normal(n) * 2.0 ** rng.integers(-30, 30, n)).astype(np.float32)
    k = (rng.standard_normal(n) * 2.0 ** rng.integers(-30, 30, n)).astype(np.float32)
    acc = (rng.standard_normal(n) * 2.0 ** rng.integers(-60, 60, n)).astype(np.float32)
    u8 = rng.integers(0, 256, n).astype(np.float32)  # the blur's own operand kinds
    taps = E.gaussian_taps(31, 6.0)[rng.integers(0, 31, n)]
    blur_acc = rng.random(n).astype(np.float32) * 255
    triples = list(zip(x, k, acc)) + list(zip(u8, taps, blur_acc)) + _adversarial_triples()
    tx, tk, ta = (np.array(v, np.float32) for v in zip(*triples))
    got = E.fmaf(tx, tk, ta)
    exp = np.array([_round_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))) for a, b, c in triples],
                   np.float32)
    assert np.array_equal(got, exp)
    # the adversarial cases are real: rounding the float64 sum first gets some of them wrong
    adv = _adversarial_triples()
    ax, ak, aa = (np.array(v, np.float32) for v in zip(*adv))
    naive = (ax.astype(np.float64) * ak + aa).astype(np.float32)
    assert (naive != E.fmaf(ax, ak, aa)).sum() > 10


# ------------------------------------------------------------------ mutations ------
# Each mutation of the contract must give a different answer on a case where the reference is the oracle's.

def _differs(mutant, reference):
    return mutant.shape != reference.shape or not np.array_equal(mutant, reference)


def test_mutation_numpy_round_for_roundf():
    mask = _random_mask(60, 80, 0.3, 1)
    ref = H.hough_lines(mask, 2, 1)
    assert np.array_equal(ref, orc.hough_lines(mask, 2, 1))
    assert _differs(H.hough_lines(mask, 2, 1, rounder=lambda v: np.round(np.asarray(v, np.float32))), ref)


def test_mutation_math_pi():
    """math.pi moves cos(+-79 deg), cos / sin(158 deg) and (199 deg) by one float each; at 1080p that flips votes."""
    mask = _random_mask(1080, 1920, 0.02, 1)
    ref = H.hough_lines(mask, 1, 1)
    assert np.array_equal(ref, orc.hough_lines(mask, 1, 1))
    assert _differs(H.hough_lines(mask, 1, 1, pi=math.pi), ref)


def test_mutation_fma_in_rho():
    mask = MASKS["drawn_480x640"]
    ref = H.hough_lines(mask, 1, 1)
    assert _differs(H.hough_lines(mask, 1, 1, fused=True), ref)


def test_mutation_clamp_instead_of_drop():
    mask = np.full((61, 200), 255, np.uint8)
    ref = H.hough_lines(mask, 7, 1)
    assert np.array_equal(ref, orc.hough_lines(mask, 7, 1))
    assert _differs(H.hough_lines(mask, 7, 1, clamp=True), ref)


def test_mutation_ge_in_peak_test():
    acc = ACCS["ties_40x50"].copy()
    acc[10, 10] = 9
    ref = H.hough_peaks(acc, 4096, 0)
    assert np.array_equal(ref, orc.hough_peaks(acc, 4096, 0))
    assert _differs(H.hough_peaks(acc, 4096, 0, strict=False), ref)


def test_mutation_inclusive_loop_bounds():
    acc = ACCS["small_votes_300x400"]
    ref = H.hough_peaks(acc, 4096, 0)
    assert _differs(H.hough_peaks(acc, 4096, 0, inclusive=True), ref)


def test_mutation_unstable_sort():
    acc = ACCS["ties_40x50"]
    ref = H.hough_peaks(acc, 64, 0)
    assert np.array_equal(ref, orc.hough_peaks(acc, 64, 0))
    assert _differs(H.hough_peaks(acc, 64, 0, stable=False), ref)


def test_mutation_a_ge_0():
    mask = np.zeros((20, 20), np.uint8)
    mask[5, 5] = 255  # radius 5: the votes at angle 0 and 90 land on a = 0 and b = 0
    ref = H.hough_circles(mask, 5)
    assert np.array_equal(ref, orc.hough_circles(mask, 5))
    assert _differs(H.hough_circles(mask, 5, a_ge0=True), ref)


def test_mutation_4_connectivity():
    img = _scene(97, 131, seed=2)
    ref = E.generate_edge(img, 3, 1.0, 10, 60)
    assert np.array_equal(ref, _oracle_edges(img, 3, 1.0, 10, 60))
    assert _differs(E.generate_edge(img, 3, 1.0, 10, 60, connectivity=4), ref)


def test_mutation_ge_thresholds():
    img = _scene(97, 131, seed=2)
    _, _, m = E.gradients(img)
    lo, hi = int(np.median(m[m > 0])), int(np.percentile(m, 95))  # thresholds that magnitudes hit exactly
    ref = E.generate_edge(img, 1, 0.0001, lo, hi)
    assert np.array_equal(ref, _oracle_edges(img, 1, 0.0001, lo, hi))
    assert _differs(E.generate_edge(img, 1, 0.0001, lo, hi, ge_thresholds=True), ref)


def test_mutation_symmetric_nms():
    img = np.full((20, 20), 50, np.uint8)
    img[:, 10:] = 150  # a step: the two columns beside it have equal magnitude
    ref = E.generate_edge(img, 1, 0.0001, 10, 20)
    assert np.array_equal(ref, _oracle_edges(img, 1, 0.0001, 10, 20))
    assert _differs(E.generate_edge(img, 1, 0.0001, 10, 20, symmetric=True), ref)


def test_mutation_unfused_blur():
    img = np.random.default_rng(0).integers(0, 256, (256, 256)).astype(np.uint8)
    ref = E.blur(img, 3, 1.0)
    assert np.array_equal(ref, _oracle_blur(img, 3, 1.0))
    assert _differs(E.blur(img, 3, 1.0, fused=False), ref)
