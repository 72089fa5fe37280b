"""tests/_ps4_driver_ref.py against itself and against the restatements it builds on, on the CPU: the painter and the
owner formulation agree on every case of the GPU tests, the generator is _pf_ref's, the walks are _ps1_driver_ref's, and
the cases tell the contract from its near misses."""
import numpy as np
import pytest

import _pf_ref as PF
import _ps1_driver_ref as P1
import _ps4_driver_ref as R

KP = R.keypoint_cases()
LINES = R.line_cases()


def canvas_of(rows, cols, seed=3):
    return np.random.RandomState(seed).randint(0, 256, (rows, cols, 3)).astype(np.uint8)


def pair_canvas():
    a, b = R.pair_images()
    return R.hconcat(R.to_bgr(a), R.to_bgr(b))


# ------------------------------------------------------------------------------------ the two formulations ------

@pytest.mark.parametrize("name", list(KP))
def test_glyphs_painter_equals_owner(name):
    rows, cols, kp = KP[name]
    canvas = canvas_of(rows, cols + 9)
    for x0 in (0, 9):
        a, sa = R.draw_keypoints(canvas, x0, cols, None, kp, len(kp), 77)
        b, sb = R.draw_keypoints(canvas, x0, cols, None, kp, len(kp), 77, owner=True)
        assert np.array_equal(a, b) and sa == sb == R.rng_jump(77, 3 * len(kp))
        keep = np.ones(canvas.shape[1], bool)
        keep[x0:x0 + cols] = False
        assert np.array_equal(a[:, keep], canvas[:, keep])  # clipped to the window
    assert not np.array_equal(a, canvas)


@pytest.mark.parametrize("name", list(LINES))
def test_lines_painter_equals_owner(name):
    ka, kb, m, mask, xo = LINES[name]
    canvas = pair_canvas()
    a = R.draw_match_lines(canvas, ka, kb, m, len(m), mask, xo)
    assert np.array_equal(a, R.draw_match_lines(canvas, ka, kb, m, len(m), mask, xo, owner=True))


def test_long_lines_painter_equals_owner():
    rows, cols, a, b, m = R.long_line_case()
    canvas = canvas_of(rows, cols)
    got = R.draw_match_lines(canvas, a, b, m, 3)
    assert np.array_equal(got, R.draw_match_lines(canvas, a, b, m, 3, owner=True))
    assert [len(t[2]) for t in R.line_strokes(rows, cols, a, b, m, 3)] == [70, 199, 288]  # more than 64, more than 128 steps


def test_panels_painter_equals_owner():
    a, b = R.pair_images()
    _, _, kpa = KP["many"]
    kpb = R._many_keypoints(120, R.ROWS, R.CB, 8)
    ka, kb, m, mask, _ = LINES["n65_masked"]
    for glyphs in (True, False):
        p = R.match_panels(a, b, kpa, 300, kpb, 120, m, 65, mask, glyphs)
        q = R.match_panels(a, b, kpa, 300, kpb, 120, m, 65, mask, glyphs, owner=True)
        assert all(np.array_equal(x, y) for x, y in zip(p[:2], q[:2])) and p[2] == q[2]
        assert p[2] == (R.rng_jump(0, 3 * 420) if glyphs else 0)


# -------------------------------------------------------------------------------------- what it is built on ------

def test_rng_is_pf_refs_generator():
    for seed in (0, 1, 12345, 0xFFFFFFFF, 0x123456789ABCDEF0):
        g = PF.CvRng(seed)
        s = R.rng_start(seed)
        draws = []
        for _ in range(30):
            s = R.rng_step(s)
            draws.append(s & 0xFFFFFFFF)
            assert g.next() == draws[-1] and g.state == s
        col, after = R.colours(seed, 10, 255)
        assert after == s and np.array_equal(col[:, ::-1].ravel(), np.array(draws) % 255)
        for n in (0, 1, 29, 30):
            t = R.rng_start(seed)
            for _ in range(n):
                t = R.rng_step(t)
            assert R.rng_jump(seed, n) == t


def test_walks_are_ps1s():
    g = np.random.RandomState(1)
    for _ in range(200):
        p1, p2 = tuple(int(v) for v in g.randint(-20, 60, 2)), tuple(int(v) for v in g.randint(-20, 60, 2))
        xs, ys = R._walk_in(p1, p2, 37, 41)
        want = [(x, y) for x, y in P1.line_walk(p1, p2) if 0 <= x < 41 and 0 <= y < 37]
        assert list(zip(xs.tolist(), ys.tolist())) == want
        cx, cy = P1.line_pixels_in(p1, p2, 37, 41)
        assert sorted(zip(cx.tolist(), cy.tolist())) == sorted(want)
    for radius in (0, 1, 2, 3, 5, 8):
        xs, ys = R.glyph_pixels([50, 50, 2 * radius, -1], 101, 101)
        off = np.array(P1.circle_offsets(radius))
        assert np.array_equal(xs, 50 + off[:, 0]) and np.array_equal(ys, 50 + off[:, 1])
    # cvRound(size / 2) rounds the tie to even; the stroke ends at the rounded polynomial direction
    assert R.glyph_pixels([50, 50, 5, -1], 101, 101)[0].max() == 52 and R.glyph_pixels([50, 50, 7, -1], 101, 101)[0].max() == 54
    xs, ys = R.glyph_pixels([50, 50, 10, 90], 101, 101)
    assert (50, 55) in set(zip(xs.tolist(), ys.tolist())) and (50, 53) in set(zip(xs.tolist(), ys.tolist()))


def test_dots_follow_the_normalised_map():
    cases = R.dots_cases()
    gray, corners = cases["weak_beside_strong"]
    out = R.draw_dots(gray, corners)
    red = (out == R.RED).all(axis=2)
    assert red[2, 2] and red[5, 5] and red[9, 1] and not red[2, 3] and not red[7, 7] and red[7, 8] and red.sum() == 4  # 1 / 510 of the strongest: 1.96
    assert np.array_equal(out[~red], P1.gray2rgb(gray)[~red])
    gray, corners = cases["negative"]
    red = (R.draw_dots(gray, corners) == R.RED).all(axis=2)
    assert red.sum() == red.size - 1 and not red[4, 4]
    for name in ("all_equal", "all_zero"):
        gray, corners = cases[name]
        assert np.array_equal(R.draw_dots(gray, corners), P1.gray2rgb(gray))
    gray, corners = cases["nan"]
    red = (R.draw_dots(gray, corners) == R.RED).all(axis=2)
    assert red[3, 3] and not red[1, 1] and not red[6, 7] and not red[6, 6] and red.sum() == 1


# ---------------------------------------------------------------------------- near misses of the contract ------

def test_cases_reject_the_mutations():
    a, b = R.pair_images()
    canvas = pair_canvas()

    def lines(name, **kw):
        ka, kb, m, mask, xo = LINES[name]
        return R.draw_match_lines(canvas, ka, kb, m, len(m), mask, xo, **kw)

    def glyphs(name, **kw):
        rows, cols, kp = KP[name]
        return R.draw_keypoints(canvas_of(rows, cols + 9), 0, cols, None, kp, len(kp), 0, **kw)[0]
    for name in ("crossing", "crossing_reversed", "n300"):
        assert not np.array_equal(lines(name), lines(name, mut=("first_writer",))), name
    for name in ("same_pixel", "through_one_pixel", "through_one_pixel_reversed"):
        assert not np.array_equal(glyphs(name), glyphs(name, mut=("first_writer",))), name
    assert not np.array_equal(lines("n64"), lines("n64", mut=("mod256",)))
    assert not np.array_equal(lines("shapes"), lines("shapes", mut=("byte_order",)))
    assert not np.array_equal(glyphs("sizes"), glyphs("sizes", mut=("byte_order",)))
    assert not np.array_equal(glyphs("borders"), glyphs("borders", mut=("bleed",)))
    for name in ("n65_masked", "n300_masked", "out_of_range"):
        assert not np.array_equal(lines(name), lines(name, mut=("rank_is_index",))), name
    kpa, kpb = KP["many"][2], R._many_keypoints(120, R.ROWS, R.CB, 8)
    ka, kb, m, mask, _ = LINES["n65"]
    good = R.match_panels(a, b, kpa, 300, kpb, 120, m, 65)
    bad = R.match_panels(a, b, kpa, 300, kpb, 120, m, 65, mut=("glyphs_over_lines",))
    assert np.array_equal(good[0], bad[0]) and not np.array_equal(good[1], bad[1])
    for name in ("weak_beside_strong", "negative", "nan"):
        gray, corners = R.dots_cases()[name]
        assert not np.array_equal(R.draw_dots(gray, corners), R.draw_dots(gray, corners, mut=("dots_nonzero",))), name
