"""tests/_ps3_driver_ref.py against what it restates (CPU): its closed form against the step-by-step walk of viz.line on
every segment with end points in [-6, 20]^2 on a 12 x 9 image, its far segments against a step-by-step walk in Python
integers that starts where the segment enters the image, and the cvRound rule."""
import numpy as np

import _ps3_driver_ref as R


def test_cv_round_halves_to_even_and_int_min_outside_int():
    for v, want in ((2.5, 2), (3.5, 4), (-0.5, 0), (-1.5, -2), (0.49999997, 0), (R.FAR, 2147483520), (2147483648.0, R.INT_MIN),
                    (-2147483648.0, R.INT_MIN), (-2147483904.0, R.INT_MIN), (R.NAN, R.INT_MIN), (R.INF, R.INT_MIN), (-R.INF, R.INT_MIN),
                    (3e9, R.INT_MIN), (16777217.0, 16777216)):
        assert R.cv_round(v) == want, v


def test_closed_form_equals_the_step_by_step_walk_on_every_small_segment():
    """All 27^4 segments at once: the walk of micv_viz::line, transcribed on arrays (x, y and err after every step), against
    start +- i and start +- minor_after(minor, major, i) at every step i <= major."""
    v = np.arange(-6, 21, dtype=np.int64)
    x1, y1, x2, y2 = (a.ravel() for a in np.meshgrid(v, v, v, v, indexing="ij"))
    swap = x1 > x2
    x1, x2, y1, y2 = np.where(swap, x2, x1), np.where(swap, x1, x2), np.where(swap, y2, y1), np.where(swap, y1, y2)
    dx, dys = x2 - x1, y2 - y1
    sy, dy = np.where(dys < 0, -1, 1), np.abs(dys)
    steep = dy > dx
    major, minor = np.where(steep, dy, dx), np.where(steep, dx, dy)
    err, x, y = major - 2 * minor, x1.copy(), y1.copy()
    for i in range(27):
        live = i <= major
        m = R.minor_after(minor, major, i)
        cx, cy = np.where(steep, x1 + m, x1 + i), np.where(steep, y1 + sy * i, y1 + sy * m)
        assert np.array_equal(cx[live], x[live]) and np.array_equal(cy[live], y[live]), i
        both = err < 0
        err = err + np.where(both, 2 * major - 2 * minor, -2 * minor)
        x = x + np.where(steep, both, 1)
        y = y + np.where(steep, sy, sy * both)
    # the last step is the far end
    assert np.array_equal(np.where(steep, x1 + R.minor_after(minor, major, major), x1 + major), x2)
    assert np.array_equal(np.where(steep, y1 + sy * major, y1 + sy * R.minor_after(minor, major, major)), y2)


def test_line_wide_equals_viz_line_on_a_12_by_9_image():
    """The restatement itself (in-image range and clip included) against the package's viz.line on every segment with end
    points in [-6, 20]^2: all 27^4 of them, each drawn by both into a cleared 12 x 9 picture."""
    from introtocomputervision_amd import viz
    v = range(-6, 21)
    got, want = np.zeros((9, 12, 1), np.uint8), np.zeros((9, 12), np.uint8)
    gflat, wflat = got.reshape(-1), want.reshape(-1)
    count = 0
    for a in v:
        for b in v:
            for c in v:
                for d in v:
                    got.fill(0)
                    want.fill(0)
                    R.line_wide(got, (a, b), (c, d), [7])
                    viz.line(want, (a, b), (c, d), 7)
                    assert gflat.tobytes() == wflat.tobytes(), (a, b, c, d)
                    count += 1
    assert count == 27 ** 4


def brute_force(img, p1, p2, cb):
    """The walk of micv_viz::line in Python integers, entered at the first step whose major coordinate is in the image:
    the minor advance there is the one integer m that puts err = major - 2 minor (i + 1) + 2 major m into the walk's
    range -2 minor <= err < 2 major - 2 minor, found by bisection; from there err is carried step by step."""
    rows, cols = img.shape[:2]
    if p1[0] > p2[0]:
        p1, p2 = p2, p1
    dx, dy = p2[0] - p1[0], p2[1] - p1[1]
    sy = -1 if dy < 0 else 1
    dy = abs(dy)
    steep = dy > dx
    major, minor = (dy, dx) if steep else (dx, dy)
    a, s, n = (p1[1], sy, rows) if steep else (p1[0], 1, cols)
    # the steps at which the major coordinate a + s i is 0 and n - 1
    ends = (-a * s, (n - 1 - a) * s)
    lo, hi = max(min(ends), 0), min(max(ends), major)
    if lo > hi:
        return
    i, m = lo, 0
    if major:
        err_of = lambda mm: major - 2 * minor * (i + 1) + 2 * major * mm
        l, h = 0, i + 1
        while l < h:  # the smallest m with err >= -2 minor
            mid = (l + h) // 2
            if err_of(mid) >= -2 * minor:
                h = mid
            else:
                l = mid + 1
        m = l
        assert -2 * minor <= err_of(m) < 2 * major - 2 * minor
    err = major - 2 * minor * (i + 1) + 2 * major * m
    while i <= hi:
        x, y = (p1[0] + m, p1[1] + sy * i) if steep else (p1[0] + i, p1[1] + sy * m)
        if 0 <= x < cols and 0 <= y < rows:
            img[y, x, :len(cb)] = cb
        both = err < 0
        err += 2 * major - 2 * minor if both else -2 * minor
        m += 1 if both else 0
        i += 1


def test_far_segments_equal_a_brute_force_walk_of_the_in_image_range():
    sl = R.segment_lists()
    crossing = 0
    for name in ("far_steep", "far_shallow", "far_extremes", "far_random", "nonfinite", "partly_outside", "halves"):
        for seg in sl[name]:
            p1, p2 = (R.cv_round(seg[0]), R.cv_round(seg[1])), (R.cv_round(seg[2]), R.cv_round(seg[3]))
            got, want = np.zeros((R.ROWS, R.COLS, 1), np.uint8), np.zeros((R.ROWS, R.COLS, 1), np.uint8)
            R.line_wide(got, p1, p2, [255])
            brute_force(want, p1, p2, [255])
            assert np.array_equal(got, want), (name, seg)
            crossing += bool(name.startswith("far") and got.any())
    assert crossing >= 30  # the far lists do pass through the picture


def test_the_named_far_segments_cross_the_whole_picture():
    sl = R.segment_lists()
    img = np.zeros((R.ROWS, R.COLS, 1), np.uint8)
    R.draw_segments(img, sl["far_steep"], (255.0,))
    assert img[:, :, 0].any(1).all() and set(np.nonzero(img[:, :, 0])[1]) <= {31, 32}  # one pixel per row, x = 31.5 +- 0.5
    img = np.zeros((R.ROWS, R.COLS, 1), np.uint8)
    R.draw_segments(img, sl["far_shallow"], (255.0,))
    assert img[:, :, 0].any(0).all() and set(np.nonzero(img[:, :, 0])[0]) <= {31, 32}


def test_a_vertical_epipolar_lines_end_points_leave_the_picture_untouched():
    buf, view = R.image(R.ROWS, R.COLS, 3, 5)
    before = buf.copy()
    R.draw_epipolar_lines(view, [[R.NAN, -R.INF, R.NAN, R.NAN, R.INF, 1.0], [R.NAN, R.INF, 1.0, R.NAN, R.INF, 1.0]], R.GREEN)
    assert np.array_equal(buf, before)


def test_case_table_is_what_the_gpu_tests_expect():
    names = [c[0] for c in R.cases()]
    assert len(set(names)) == len(names) and len(R.segment_lists()["random200"]) == 200
    assert R.case_tokens().count("\ncase ") == len(names)
