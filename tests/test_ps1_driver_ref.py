"""The arguments the ps1 driver kernels rest on, checked on the restatement (tests/_ps1_driver_ref.py) alone: the
closed-form line walk, the shape of the circle walk, the elliptic footprint, findParallelLines against the multimap it
restates, and the per-tile top-K selection of the radius-range search."""
import numpy as np
import pytest

import _ps1_driver_ref as R


def test_closed_form_line_walk_equals_the_serial_walk():
    """m(i) = (2 minor i + major - 1) div (2 major) for every minor <= major <= 300, shallow and steep, both signs."""
    for major in range(0, 301):
        i = np.arange(major + 1, dtype=np.int64)
        for minor in range(0, major + 1):
            walk = np.array(R.line_walk((0, 0), (major, minor)), np.int64)  # shallow: x is the major axis
            assert np.array_equal(walk[:, 0], i)
            assert np.array_equal(walk[:, 1], R.line_minor_steps(minor, major, i)), (minor, major)
    for major, minor in [(300, 299), (7, 3), (1, 1), (250, 1), (13, 0)]:
        i = np.arange(major + 1, dtype=np.int64)
        m = R.line_minor_steps(minor, major, i)
        down = np.array(R.line_walk((5, 9), (5 + major, 9 - minor)), np.int64)
        assert np.array_equal(down[:, 0], 5 + i) and np.array_equal(down[:, 1], 9 - m)
        if minor < major:  # steep: y is the major axis, walked from the left end point
            steep = np.array(R.line_walk((2, 1), (2 + minor, 1 + major)), np.int64)
            assert np.array_equal(steep[:, 1], 1 + i) and np.array_equal(steep[:, 0], 2 + m)
            if minor > 0:  # p1 right of p2: swapped, the walk starts at (2, 1 + major) and goes up
                back = np.array(R.line_walk((2 + minor, 1), (2, 1 + major)), np.int64)
                assert np.array_equal(back[:, 1], 1 + major - i) and np.array_equal(back[:, 0], 2 + m)
    assert R.line_walk((4, 4), (4, 4)) == [(4, 4)]  # major = 0: one pixel


def test_clipped_closed_form_draws_what_the_serial_walk_draws():
    """draw_lines by the closed form over the in-image steps == the serial walk with every pixel bounds-checked, for
    every theta column and rho rows at 0, mid and last, on a 31 x 47 image (end points up to ~100 diagonals outside)."""
    rows, cols = 31, 47
    img = np.zeros((rows, cols, 3), np.uint8)
    rb = 2 * int(np.ceil(np.hypot(rows, cols)))
    for row in (0, rb // 2, rb // 2 + 9, rb - 1):
        peaks = [(row, c) for c in range(180)]
        assert np.array_equal(R.draw_lines(img, peaks, 1, 1), R.draw_lines(img, peaks, 1, 1, serial=True)), row


def test_circle_walk_shape():
    for radius in range(0, 61):
        pts = set(R.circle_offsets(radius))
        for dx, dy in pts:  # the eight reflections
            assert {(dx, -dy), (-dx, dy), (-dx, -dy), (dy, dx), (dy, -dx), (-dy, dx), (-dy, -dx)} <= pts
            assert abs(np.hypot(dx, dy) - radius) < 1.0, (radius, dx, dy)
        # 8-connected: a walk over neighbours reaches every pixel
        start = next(iter(pts))
        seen, todo = {start}, [start]
        while todo:
            x, y = todo.pop()
            for nx in (x - 1, x, x + 1):
                for ny in (y - 1, y, y + 1):
                    if (nx, ny) in pts and (nx, ny) not in seen:
                        seen.add((nx, ny))
                        todo.append((nx, ny))
        assert seen == pts, radius
    assert set(R.circle_offsets(0)) == {(0, 0)}
    assert set(R.circle_offsets(1)) == {(1, 0), (-1, 0), (0, 1), (0, -1)}


def test_ellipse_half_widths():
    assert R.ellipse_half_widths(1) == (0,)
    assert R.ellipse_half_widths(3) == (0, 1, 0)
    assert R.ellipse_half_widths(5) == (0, 2, 2, 2, 0)
    assert R.ellipse_half_widths(7) == (0, 2, 3, 3, 3, 2, 0)


def test_erode_minimum_rule():
    """v = first tap, then v = (x < v) ? x : v: every compare with a NaN is false, so a NaN later tap never replaces and a
    NaN first tap stays; of -0 / +0 the earlier stays."""
    img = np.full((5, 5), 7, np.float32)
    img[2, 2] = np.nan  # a later tap of its neighbours, never the first (the first tap is (y - 2, x))
    out = R.erode(img, 5)
    assert out[2, 2] == 7 and not np.isnan(out[1:4, 1:4]).any()
    assert np.isnan(out[4, 2])  # (4, 2)'s first tap is (2, 2)
    z = np.zeros((1, 3), np.float32)
    z[0, 0] = -0.0
    out = R.erode(z, 3)  # taps of (0, 1) in raster order: border, -0, +0, +0, border
    assert np.signbit(out[0, 1]) and not np.signbit(out[0, 2])
    assert R.erode(np.array([[3, 9], [200, 4]], np.uint8), 1).tolist() == [[3, 9], [200, 4]]


def _multimap_parallel(peaks, delta_theta, delta_rho):
    """Solution.cpp:134-173 with a dict of lists for the multimap."""
    lines = {}
    for idx, (rho, theta) in enumerate(peaks):
        key = ((rho // delta_rho * delta_rho) << 32) | (theta // delta_theta * delta_theta)
        lines.setdefault(key, []).append(idx)
    out = []
    for key, idxs in lines.items():
        if len(idxs) > 1:
            out += [tuple(peaks[i]) for i in idxs]
    return out


def test_parallel_lines_against_the_multimap():
    rng = np.random.default_rng(7)
    for n, hi, dt, dr in [(0, 10, 4, 150), (1, 10, 4, 150), (12, 400, 4, 150), (40, 60, 1, 1), (200, 50, 3, 7), (64, 5, 9, 9)]:
        peaks = [tuple(int(v) for v in p) for p in rng.integers(0, hi, (n, 2))]
        got = R.parallel_lines(np.array(peaks, np.uint32).reshape(-1, 2), dt, dr)
        exp = _multimap_parallel(peaks, dt, dr)
        assert sorted(map(tuple, got.tolist())) == sorted(exp)
        keep = set(exp)
        assert [tuple(p) for p in got.tolist()] == [p for p in peaks if p in keep]  # input order (duplicates included)
    assert len(R.parallel_lines(np.array([[3, 3], [3, 3]], np.uint32), 1, 1)) == 2


def test_per_tile_top_k_gives_the_global_top_k():
    """Distinct keys (votes, index): the K largest of an accumulator are among the K largest of every 64 x 32 tile, so
    selecting from the union of the tiles' own top K loses nothing -- ties included."""
    rng = np.random.default_rng(11)
    for rows, cols, k, hi in [(70, 130, 5, 4), (33, 65, 64, 3), (96, 128, 10, 1000), (31, 63, 7, 2), (65, 129, 64, 1)]:
        acc = rng.integers(0, hi, (rows, cols)).astype(np.int64)
        idx = np.arange(rows * cols).reshape(rows, cols)

        def top(v, i, k=k):
            order = np.lexsort((i.ravel(), -v.ravel()))[:k]  # votes descending, index ascending
            return i.ravel()[order]

        union = np.concatenate([top(acc[y:y + 32, x:x + 64], idx[y:y + 32, x:x + 64])
                                for y in range(0, rows, 32) for x in range(0, cols, 64)])
        assert np.array_equal(top(acc, idx), top(acc.ravel()[union], union))


def test_f32_to_u8_rule():
    v = np.array([np.nan, np.inf, -np.inf, 255.5, 254.5, -0.5, 0.5, 1.5, 2.5, 300, -7, 3e9, -3e9, 2147483520.0], np.float32)
    assert R.to_u8(v).tolist() == [0, 0, 0, 255, 254, 0, 0, 2, 2, 255, 0, 0, 0, 255]
