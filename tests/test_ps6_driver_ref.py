"""tests/_ps6_driver_ref.py, the numpy restatement of the ps6 driver's overlay (the dots of ParticleFilter::drawParticles
and the ring of micv_viz::rectangle): its two formulations agree on every case the GPU tests use, and each of five
deliberate mistakes changes at least one case in both.  The host loops themselves (the contract) are compared with it in
tests/test_ps6_driver_shim.py."""
import numpy as np
import pytest

import _ps6_driver_ref as R

CASES = R.cases()
EXPECTED = {c[0]: R.apply_case(c) for c in CASES}  # computed once, never written to


def test_the_two_formulations_agree_on_every_case():
    assert len({c[0] for c in CASES}) == len(CASES)
    for c in CASES:
        assert np.array_equal(EXPECTED[c[0]], R.apply_case(c, paint=R.paint_predicate)), c[0]
    for c in R.rect_cases():
        assert np.array_equal(R.apply_rect_case(c), R.apply_rect_case(c, R.paint_predicate)), c[0]


@pytest.mark.parametrize("mut", R.MUTATIONS)
def test_each_mistake_is_caught(mut):
    caught = [c[0] for c in CASES if not np.array_equal(EXPECTED[c[0]], R.apply_case(c, (mut,)))]
    assert caught, mut
    # the second formulation makes the same mistake the same way: a case that catches one catches the other
    for c in CASES:
        assert np.array_equal(R.apply_case(c, (mut,)), R.apply_case(c, (mut,), R.paint_predicate)), (mut, c[0])


def test_padding_and_bytes_beyond_the_colour_survive():
    for c in CASES:
        name, ch, pad = c[:3]
        buf = EXPECTED[name]
        assert np.all(buf[:, R.COLS * ch:] == R.SENTINEL), name
        if ch == 4 and name.endswith("c3") and "edge" not in name:  # a 3-value colour writes 0 into byte 3, never beyond
            assert buf.shape[1] == R.COLS * 4 + pad


def test_the_box_of_the_driver():
    # the reference's hand box, 73 x 87: halves 36.5 and 43.5, in float, each value through cvRound (halves to even)
    assert R.box_rect((540.0, 385.0), (73.0, 87.0)) == (504, 342, 73, 87)  # 503.5 -> 504, 341.5 -> 342
    assert R.box_rect((541.0, 386.0), (73.0, 87.0)) == (504, 342, 73, 87)  # 504.5 -> 504, 342.5 -> 342
    assert R.box_rect((R.NAN, 3.0), (9.0, 7.0)) == (R.INT_MIN, 0, 9, 7)    # 3 - 3.5 = -0.5 -> -0
    assert R.box_rect((R.INF, -R.INF), (3e9, -3e9)) == (R.INT_MIN,) * 4
    assert R.box_rect((20.0, 10.0), (0.5, 1.5)) == (20, 9, 0, 2)           # 19.75 -> 20, 9.25 -> 9, 0.5 -> 0, 1.5 -> 2
    assert R.cv_round(2.5) == 2 and R.cv_round(-2.5) == -2 and R.cv_round(3.5) == 4 and R.cv_round(2147483520.0) == 2147483520
    assert R.cv_round(2147483648.0) == R.INT_MIN and R.cv_round(-2147483648.0) == R.INT_MIN


def test_ring_wins_and_nothing_else_changes():
    c = next(c for c in CASES if c[0] == "box-inside")
    out = EXPECTED["box-inside"].reshape(R.ROWS, R.COLS, 3)
    clean = R.image(R.ROWS, R.COLS, 3, 0)[1]
    x, y, w, h = R.box_rect(*c[5])
    assert (x, y, w, h) == (16, 10, 21, 15)
    ring = np.zeros((R.ROWS, R.COLS), bool)
    ring[y, x:x + w] = ring[y + h - 1, x:x + w] = True
    ring[y:y + h, x] = ring[y:y + h, x + w - 1] = True
    assert np.all(out[ring] == [255, 0, 255])
    rest = out[~ring]
    assert np.all((rest == [0, 255, 0]).all(1) | (rest == clean[~ring]).all(1))
    assert ((rest == [0, 255, 0]).all(1)).sum() > 20
