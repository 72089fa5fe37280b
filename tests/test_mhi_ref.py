"""tests/_mhi_ref.py pinned on the CPU: the structuring element, answers worked by hand, the lemma the bit-plane open
of mhi.hip relies on, properties of the open, every mutation on an input that tests/test_mhi_paths_gpu.py uses,
and -- in ONE test, the only place this file touches the oracle -- byte equality with oracle/oracle_ps7.c on that
module's whole case list.

`python tests/test_mhi_ref.py ties` repeats the searches the reference's docstring quotes."""
import os
import sys
import time

import numpy as np
import pytest

if __name__ == "__main__":  # run as a script: tests/ is on the path already, the repository root is not needed
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _mhi_cases as C
import _mhi_ref as M

HALF_WIDTHS = (0, 2, 3, 3, 3, 2, 0)


def block_mask(rows, cols, y0, x0, n):
    m = np.zeros((rows, cols), np.uint8)
    m[y0:y0 + n, x0:x0 + n] = 1
    return m


def random_masks():
    """Masks of several densities at the sizes where the reflection wraps more than once, and a few ordinary ones."""
    rng = np.random.default_rng(12)
    for shape in ((1, 9), (1, 1), (9, 1), (2, 2), (3, 4), (6, 7), (7, 6), (4, 30), (13, 11), (40, 37)):
        for p in (0.5, 0.8, 0.95):
            for _ in range(4):
                yield (rng.random(shape) < p).astype(np.uint8)


# ------------------------------------------------------------------------------------------- known answers

def test_ellipse_rows():
    se = M.ellipse()
    assert se.shape == (7, 7)
    for i, w in enumerate(HALF_WIDTHS):
        assert se[i].tolist() == [abs(j - 3) <= w for j in range(7)], i
    assert np.array_equal(se, se[::-1]) and np.array_equal(se, se[:, ::-1])
    # what the padding proof uses: the half-width does not grow with |dy|
    assert all(HALF_WIDTHS[3 + d] >= HALF_WIDTHS[3 + d + 1] for d in range(3))
    assert M.ellipse(mut=("se_rect",)).all()
    assert M.ellipse(mut=("se_rows_wide",)).sum(1).tolist() == [1, 7, 7, 7, 7, 7, 1]


def test_open_known_answers():
    # a 9 x 9 block: the erosion leaves its central 3 x 3 (the element's column of 7 and its rows of 7 must fit), the
    # dilation is the union of nine ellipses -- rows of half-width 1, 3, 4, 4, 4, 4, 4, 3, 1 about the centre column
    for rows, cols, y0, x0 in ((15, 15, 3, 3), (20, 31, 7, 19)):
        m = block_mask(rows, cols, y0, x0, 9)
        er = M.erode(m)
        assert np.array_equal(er, block_mask(rows, cols, y0 + 3, x0 + 3, 3))
        want = np.zeros_like(m)
        for i, w in enumerate((1, 3, 4, 4, 4, 4, 4, 3, 1)):
            want[y0 + i, x0 + 4 - w:x0 + 4 + w + 1] = 1
        assert np.array_equal(M.morph_open(m), want)
        assert want.sum() == 81 - 4 * (3 + 1)
    # a 6 x 6 block holds no column of 7
    assert not M.morph_open(block_mask(15, 15, 4, 4, 6)).any()
    # at the border the reflection completes the block: 6 rows against the top edge mirror to 11, 4 rows to 7, 3 to 5
    top = np.zeros((15, 15), np.uint8)
    top[0:4, 3:12] = 1
    assert M.erode(top).sum() == 3 and M.erode(top)[0, 6:9].all()
    top[3] = 0
    assert not M.morph_open(top).any()
    # all ones stay all ones, whatever the size
    for shape in ((1, 1), (1, 2), (1, 5), (5, 1), (2, 2), (3, 4), (6, 7), (7, 7), (20, 9)):
        assert M.morph_open(np.ones(shape, np.uint8)).all(), shape
        assert not M.morph_open(np.zeros(shape, np.uint8)).any()
    # ... but not with a zero-padded erosion
    assert not M.morph_open(np.ones((6, 7), np.uint8), mut=("erode_pad_zero",)).any()


def test_threshold_update_energy_known_answers():
    v = np.arange(256, dtype=np.uint8).reshape(8, 32)
    assert np.array_equal(M.threshold(v, 1.7), v >= 2) and np.array_equal(M.threshold(v, 2), v >= 2)
    assert np.array_equal(M.threshold(v, 255), v == 255) and not M.threshold(v, 256).any()
    assert M.threshold(v, 0).all() and M.threshold(v, -3).all()  # -val >= t: -0 >= 0, and everything for t < 0
    assert not M.threshold(v, float("nan")).any()
    assert np.array_equal(M.threshold(v, 0, mut=("thr_gt",)), v > 0)
    assert np.array_equal(M.threshold(v, 200, mut=("thr_neg_u8",)), (v >= 200) | ((v >= 1) & (v <= 56)))
    h = np.array([[0, 1, 2, 255, 7, 0]], np.uint8)
    m = np.array([[0, 0, 0, 0, 1, 2]], np.uint8)
    assert M.update(h, m, 25).tolist() == [[0, 0, 1, 254, 25, 0]]
    assert M.update(h, m, 300).tolist() == [[0, 0, 1, 254, 44, 0]]  # the uint8_t store of tau
    assert M.update(h, m, 256).tolist() == [[0, 0, 1, 254, 0, 0]]
    assert M.energy(h).tolist() == [[0, 1, 1, 1, 1, 0]]
    assert h.tolist() == [[0, 1, 2, 255, 7, 0]]  # a new array, the input untouched


def test_fast_fmaf_equals_the_twosum_emulation():
    from _edge_ref import fmaf as exact
    rng = np.random.default_rng(8)
    x = rng.integers(0, 256, 200000).astype(np.float32)
    k = rng.random(200000).astype(np.float32)
    acc = (rng.random(200000) * 255).astype(np.float32)
    assert np.array_equal(M.fmaf(x, k, acc).view(np.uint32), exact(x, k, acc).view(np.uint32))
    # a sum whose double is exactly a float midpoint while the exact sum is not: (1 + 2^-23) * (2^-24 - 2^-47) =
    # 2^-24 - 2^-70; added to 1 + 2^-23 (an odd mantissa) the double is the midpoint above it, which alone would tie
    # to even, 1 + 2^-22, where the exact sum lies below the midpoint.  Then the same on 1 (even: both ways give 1) and
    # a true tie, 1 * 2^-24 on 1 + 2^-23, which does go to even.
    u = 2.0 ** -23
    x2 = np.array([1 + u, 1 + u, 1], np.float32)
    k2 = np.array([2.0 ** -24 - 2.0 ** -47, 2.0 ** -24 - 2.0 ** -47, 2.0 ** -24], np.float32)
    a2 = np.array([1 + u, 1, 1 + u], np.float32)
    got = M.fmaf(x2, k2, a2)
    assert np.array_equal(got.view(np.uint32), exact(x2, k2, a2).view(np.uint32))
    s = x2.astype(np.float64) * k2.astype(np.float64) + a2.astype(np.float64)
    assert ((s.view(np.int64) & 0x1FFFFFFF) == 0x10000000).all()  # the slow path was taken
    assert got.astype(np.float64).tolist() == [1 + u, 1.0, 1 + 2 * u]
    assert s.astype(np.float32).astype(np.float64).tolist() == [1 + 2 * u, 1.0, 1 + 2 * u]  # what the shortcut alone gives
    taps = M.gaussian_taps(31, 10.0)
    img = rng.integers(0, 256, (40, 50)).astype(np.uint8)
    import _edge_ref as E
    assert np.array_equal(M.blur(img, (31, 31), 10.0), E.blur(img, 31, 10.0)) and len(taps) == 31


def test_blur_known_answers():
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (9, 11)).astype(np.uint8)
    assert np.array_equal(M.blur(img, (1, 1), 1.0), img)  # the 1-tap pass is the tap 1.0
    assert np.array_equal(M.blur(np.full((4, 5), 255, np.uint8), (31, 31), 10.0), np.full((4, 5), 255))
    assert np.array_equal(M.blur(np.full((1, 1), 77, np.uint8), (31, 1), 10.0), [[77]])
    # cv::Size(width, height): (5, 1) filters along x only
    rowwise = np.stack([M.blur(img[i:i + 1], (5, 1), 1.5)[0] for i in range(9)])
    assert np.array_equal(M.blur(img, (5, 1), 1.5), rowwise)
    assert np.array_equal(M.blur(img, (1, 5), 1.5), M.blur(img.T.copy(), (5, 1), 1.5).T)
    # an impulse of 255 spreads to round(255 * taps), reflected at the border
    imp = np.zeros((1, 7), np.uint8)
    imp[0, 0] = 255
    t = M.gaussian_taps(3, 1.0).astype(np.float64)
    assert M.blur(imp, (3, 1), 1.0)[0, :3].tolist() == [round(255 * t[1]), round(255 * t[0]), 0]
    assert M.subtract([[5, 9]], [[9, 5]]).tolist() == [[0, 4]]


# ------------------------------------------------------------------------------------------- the lemma, properties

def test_erosion_of_the_extension_is_the_extension_of_the_erosion():
    """What mhi_open7_bits_kernel relies on to pad the dilation without a second pass (reference docstring)."""
    n = 0
    for m in random_masks():
        assert np.array_equal(M.erode_of_extension(m), M.extension(M.erode(m), 3)), m.shape
        n += 1
    assert n == 120
    # with an element that is not symmetric the statement fails, so the check can fail: the centre row's right half
    # (offsets 0 .. 3) on a mask whose column 0 is empty.  With per-pass padding only column 0 erodes (no other pixel
    # reads column 0 or a mirror image of it), so the extension of the erosion is set at column -1; the erosion of the
    # extension reads columns -1 .. 2 there, column 0 among them.
    import scipy.ndimage as ndi
    se = np.zeros((7, 7), bool)
    se[3, 3:] = True
    m = np.ones((6, 9), np.uint8)
    m[:, 0] = 0
    inner = ndi.minimum_filter(M.extension(m, 3), footprint=se, mode="constant")[3:-3, 3:-3]
    outer = ndi.minimum_filter(M.extension(m, 6), footprint=se, mode="constant")[3:-3, 3:-3]
    assert inner[:, 0].sum() == 0 and inner[:, 1:].all()
    assert M.extension(inner, 3)[3, 2] == 1 and outer[3, 2] == 0


def test_reflected_padding_equals_ignoring_the_outside():
    """The docstring's proof, checked: padding the erosion with ones (the dilation with zeros) changes nothing."""
    import scipy.ndimage as ndi
    se = M.ellipse()
    for m in random_masks():
        assert np.array_equal(M.erode(m), ndi.minimum_filter(m, footprint=se, mode="constant", cval=1))
        assert np.array_equal(M.dilate(m), ndi.maximum_filter(m, footprint=se, mode="constant", cval=0))


def test_open_is_idempotent_and_contained_in_its_input():
    some = False
    for m in random_masks():
        o = M.morph_open(m)
        assert (o <= m).all() and np.array_equal(M.morph_open(o), o), m.shape
        assert set(np.unique(o)) <= {0, 1}
        some |= 0 < o.sum() < m.sum()
    assert some


# ------------------------------------------------------------------------------------------- the case list

def test_case_list_covers_what_it_claims():
    cs = C.cases()
    assert len({c.name for c in cs}) == len(cs)
    assert {(c.rows, c.cols) for c in cs} == set(C.SHAPES)
    rows, cols = {r for r, _ in C.SHAPES}, {c for _, c in C.SHAPES}
    assert {15, 16, 17, 51, 52, 53, 57, 58, 104, 105, 207, 208, 209, 213} <= rows
    assert {58, 63, 64, 65, 69, 70, 71, 128, 129, 133, 134, 200} <= cols
    assert {(1, 1), (1, 300), (300, 1), (2, 2), (3, 4), (5, 5), (6, 7)} <= set(C.SHAPES)
    for shape in C.SHAPES:
        mine = C.cases_of(*shape)
        assert {(31, 31), (31, 1), (1, 31)} <= {c.ksize for c in mine}
        assert [c.thresh for c in mine if c.kind == "step"] == list(C.THRESHOLDS)
    assert {c.ksize for c in cs} == {(1, 1), (3, 3), (5, 1), (1, 9), (7, 3), (31, 31), (31, 1), (1, 31)}
    for shape in ((53, 70), (105, 133), (52, 69)):
        f1, f2 = C.step_pair(*shape)
        assert set(np.unique(f2.astype(int) - f1.astype(int))) == set(C.STEP_DIFFS), shape
    # ragged masks: on every larger shape the noise cases give masks with both values, most of them
    for shape in C.SHAPES:
        if min(shape) >= 13:
            dens = [C.expected(c).mean() for c in C.cases_of(*shape) if c.kind == "noise"]
            assert sum(0.02 < d < 0.98 for d in dens) >= 4, (shape, dens)
    # the step pair shows every threshold: the masks of -3/0, 1, 1.7/2, 40, 255 and 256/NaN differ as they should
    by_t = {c.thresh: C.expected(c) for c in C.cases_of(105, 133) if c.kind == "step"}
    assert by_t[-3].all() and by_t[0].all() and not by_t[256].any() and not by_t[C.NAN].any()
    assert np.array_equal(by_t[1.7], by_t[2]) and by_t[255].any()
    sums = [int(by_t[t].sum()) for t in (0, 1, 2, 40, 255, 256)]
    assert sums == sorted(sums, reverse=True) and len(set(sums)) == 6


def test_reference_equals_oracle_on_the_case_list():
    """Keeps oracle/oracle_ps7.c honest (bench.py and smoke() still use it): byte equality on every case."""
    import _oracle as orc
    t0 = time.perf_counter()
    for c in C.cases():
        f1, f2 = C.frames(c)
        got = orc.mhi_frame_difference(f1, f2, c.thresh, c.ksize, c.sigma)
        assert np.array_equal(got, C.expected(c)), c.name
    for tup, x in M.TIE_TUPLES + M.FMA_TUPLES:
        f1, f2, t = M.tie_pair(tup, x)
        assert np.array_equal(orc.mhi_frame_difference(f1, f2, t, M.TIE_BLUR, M.TIE_SIGMA),
                              M.frame_difference(f1, f2, t, M.TIE_BLUR, M.TIE_SIGMA)), tup
    v = np.arange(768).astype(np.uint8).reshape(6, 128)
    for t in C.THRESHOLDS:
        assert np.array_equal(orc.mhi_threshold(v, t), M.threshold(v, t)), t
    assert np.array_equal(orc.mhi_energy(v), M.energy(v))
    hist, mask = C.update_inputs()
    for tau in C.TAUS:
        assert np.array_equal(orc.mhi_update(hist, mask, tau), M.update(hist, mask, tau)), tau
    print(f"\n{len(C.cases())} cases against the oracle: {time.perf_counter() - t0:.2f} s")


# ------------------------------------------------------------------------------------------- mutations

# mutation -> a case of the list on which the mask changes (the case tests/test_mhi_paths_gpu.py names when a kernel
# carries that mistake)
FD_MUTATION_CASES = {
    "blur_wh_swapped": "53x70-noise-b5x1-t40",
    "sub_reversed": "53x70-noise-b3x3-t1.7",
    "sub_abs": "53x70-step-b1x1-t1",
    "thr_gt": "53x70-step-b1x1-t1",
    "thr_truncated": "53x70-step-b1x1-t1.7",
    "thr_neg_u8": "53x70-step-b1x1-t255",
    "se_rect": "53x70-noise-b3x3-t1.7",
    "se_rows_wide": "53x70-noise-b3x3-t1.7",
    "erode_pad_zero": "6x7-step-b1x1-t0",
    "close_not_open": "53x70-noise-b3x3-t1.7",
    "erode_only": "53x70-step-b1x1-t1",
}


@pytest.mark.parametrize("mut", sorted(FD_MUTATION_CASES))
def test_frame_difference_mutation_changes_a_case(mut):
    c = C.case(FD_MUTATION_CASES[mut])
    f1, f2 = C.frames(c)
    got = M.frame_difference(f1, f2, c.thresh, c.ksize, c.sigma, mut=(mut,))
    assert not np.array_equal(got, C.expected(c)), (mut, c.name)


@pytest.mark.parametrize("mut,tuples", [("round_half_away", M.TIE_TUPLES), ("blur_unfused", M.FMA_TUPLES)])
def test_rounding_mutations_change_the_planted_rows(mut, tuples):
    t = M.gaussian_taps(5, M.TIE_SIGMA).astype(np.float64)
    holes = 0
    for tup, x in tuples:
        f1, f2, thr = M.tie_pair(tup, x)
        v = M.blur_float(f1, M.TIE_BLUR, M.TIE_SIGMA).astype(np.float64)[0]
        assert abs(v[10] - np.dot(t, tup)) < 1e-4  # the chain's result is the weighted sum, up to float rounding
        if mut == "round_half_away":
            assert v[10] == x + 0.5 and x % 2 == 0  # an exact tie above an even integer
            assert M.blur(f1, M.TIE_BLUR, M.TIE_SIGMA)[0, 10] == x
        else:
            assert abs(v[10] - (x + 0.5)) < 2e-5
        assert (np.rint(np.delete(v, 10)) <= x).all() and (np.abs(np.delete(v, 10) % 1 - 0.5) > 1e-3).all()
        want = M.frame_difference(f1, f2, thr, M.TIE_BLUR, M.TIE_SIGMA)
        got = M.frame_difference(f1, f2, thr, M.TIE_BLUR, M.TIE_SIGMA, mut=(mut,))
        assert sorted((int(want.sum()), int(got.sum()))) == [20, 21] and want[0, 10] != got[0, 10], tup
        holes += int(want.sum()) == 20
    assert holes == (0 if mut == "round_half_away" else 2)  # both directions of the unfused error are planted


def test_update_mutations_change_the_update_inputs():
    hist, mask = C.update_inputs()
    assert {0, 1, 2, 255} == set(np.unique(mask)) and {0, 1, 255} <= set(np.unique(hist))
    assert not np.array_equal(M.update(hist, mask, 25, mut=("update_mask_nonzero",)), M.update(hist, mask, 25))
    assert not np.array_equal(M.update(hist, mask, 300, mut=("update_tau_saturates",)), M.update(hist, mask, 300))
    assert np.array_equal(M.update(hist, mask, 255, mut=("update_tau_saturates",)), M.update(hist, mask, 255))
    assert not np.array_equal(M.update(hist, mask, 25, mut=("update_no_floor",)), M.update(hist, mask, 25))
    h = C.HISTORY
    args = (C.history_frames(), h["thresh"], h["ksize"], h["sigma"], h["tau"], h["save"])
    want = C.history_expected()
    assert np.array_equal(want[1], want[3]) and not np.array_equal(want[0], want[2])  # save = (5, 2, 7, 2)
    assert set(np.unique(want)) == {0, 1, 2, 3}  # set, decaying, and back on the floor
    assert (want[2] == 0).sum() > (want[0] == 0).sum()
    for mut in ("update_no_floor", "update_mask_nonzero", "sub_reversed", "thr_gt", "erode_only"):
        got = M.history_seq(*args, mut=(mut,))
        assert np.array_equal(got, want) == (mut in ("update_mask_nonzero", "thr_gt")), mut  # masks hold 0 and 1 here


def test_every_mutation_is_shown():
    shown = set(FD_MUTATION_CASES) | {"round_half_away", "blur_unfused", "update_mask_nonzero", "update_tau_saturates",
                                      "update_no_floor"}
    assert shown == set(M.MUTATIONS)
    with pytest.raises(ValueError):
        M.threshold(np.zeros((1, 1), np.uint8), 1, mut=("no_such_mutation",))


def test_print_reference_time_for_the_largest_case():
    f1, f2 = C.noise_pair(213, 200)
    t0 = time.perf_counter()
    M.frame_difference(f1, f2, 1.7, (31, 31), 10.0)
    print(f"\nreference frame_difference, 213 x 200, blur 31 x 31: {time.perf_counter() - t0:.3f} s")


# ------------------------------------------------------------------------------------------- the tie searches

def ties():
    for sigma in (0.8, 1.0, 1.5, 2.0, 10.0):
        print(f"3 x 1, sigma {sigma}: {len(M.find_ties3(sigma))} of 2^24 triples end on .5")
    found = np.concatenate([M.find_ties5(1 << 20, seed) for seed in range(16)])
    print(f"5 x 1, sigma {M.TIE_SIGMA}: {len(found)} of 2^24 random 5-tuples end on .5, "
          f"{int((found[:, 5] % 2 == 0).sum())} above an even integer")


if __name__ == "__main__":
    if sys.argv[1:] == ["ties"]:
        ties()
