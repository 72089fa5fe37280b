"""tests/_mhi_color_ref.py and tests/_mhi_color_cases.py pinned on the CPU: the grey step by hand and against the
oracle's 8-bit to_gray (the only place this file touches the oracle), every mutation on a named case that
tests/test_mhi_color_gpu.py runs, and masks that hold both values on every case of 15 x 58 or larger."""
import numpy as np
import pytest

import _mhi_color_cases as C
import _mhi_color_ref as R
import _mhi_ref as M

# mutation -> a case of test_mhi_color_gpu.py::test_frame_difference[53x70-*] whose mask it changes
SHOWN_BY = {
    "grey_before_subtract": "53x70x3-noise-b1x1-t40",
    "grey_before_blur": "53x70x3-noise-b3x3-t1.7",
    "grey_weights_bgr": "53x70x3-step-b1x1-t40",
    "grey_truncated": "53x70x3-step-b1x1-t1",
    "alpha_weighted": "53x70x4-step-b1x1-t1",
    "sub_abs": "53x70x3-step-b1x1-t2",
    "channel0_only": "53x70x3-step-b1x1-t1",
}


def test_grey_known_answers():
    px = lambda *v: int(R.grey(np.array([v], np.uint8))[0])
    assert px(1, 1, 0) == 1 and int(R.grey(np.array([[1, 1, 0]], np.uint8), mut=("grey_truncated",))[0]) == 0
    assert px(0, 0, 1) == 0 and px(0, 1, 0) == 1 and px(1, 0, 1) == 0
    assert px(255, 0, 0) == 76 and px(0, 255, 0) == 150 and px(0, 0, 255) == 29
    assert px(255, 255, 255) == 255 and sum(R.WEIGHTS) == 1 << 14
    assert px(255, 0, 0, 255) == 76  # alpha is not read
    assert int(R.grey(np.array([[255, 0, 0]], np.uint8), mut=("grey_weights_bgr",))[0]) == 29


@pytest.mark.parametrize("channels", C.CHANNELS)
def test_grey_agrees_with_the_oracle(channels):
    import _oracle as orc
    d = np.random.default_rng(5).integers(0, 256, (37, 53, channels)).astype(np.uint8)
    d[0, :4, :3] = ((1, 1, 0), (0, 0, 1), (255, 255, 255), (0, 0, 0))
    want = orc.to_gray(d)
    assert want.dtype == np.float32 and np.array_equal(want, R.grey(d).astype(np.float32))


def test_order_of_subtract_and_grey():
    """A channel whose difference saturates at 0 does not pull the others down."""
    b1 = np.array([[[100, 7, 100]]], np.uint8)
    b2 = np.array([[[103, 4, 100]]], np.uint8)
    assert int(R.grey_difference(b1, b2)[0, 0]) == 1
    assert int(R.grey_difference(b1, b2, mut=("grey_before_subtract",))[0, 0]) == 0  # 0.3 * 3 - 0.59 * 3 < 0
    assert int(R.grey_difference(b1, b2, mut=("sub_abs",))[0, 0]) == 3


def test_two_dimensional_frames_go_to_the_single_channel_reference():
    import _mhi_cases as C1
    c = C1.case("53x70-noise-b3x3-t1.7")
    f1, f2 = C1.frames(c)
    assert np.array_equal(R.frame_difference(f1, f2, c.thresh, c.ksize, c.sigma), C1.expected(c))
    # three equal channels: the weights sum to 1, so the mask is the single-channel one
    s1, s2 = (np.repeat(f[..., None], 3, -1) for f in (f1, f2))
    assert np.array_equal(R.frame_difference(s1, s2, c.thresh, c.ksize, c.sigma), C1.expected(c))
    h = C1.HISTORY
    got, diffs = R.history_seq(C1.history_frames(), h["thresh"], h["ksize"], h["sigma"], h["tau"], h["save"])
    assert np.array_equal(got, C1.history_expected()) and diffs.shape == (0, 53, 70)


def test_case_list_covers_what_the_issue_names():
    names = [c.name for c in C.cases()]
    assert len(set(names)) == len(names)
    for rows, cols in C.SHAPES:
        for ch in C.CHANNELS:
            cs = C.cases_of(rows, cols, ch)
            assert {c.ksize for c in cs if c.kind == "noise"} == {(1, 1), (3, 3), (7, 3), (31, 31)}
            assert all(c.thresh in C.THRESHOLDS or c.thresh != c.thresh for c in cs)
    f1, f2 = C.frames(C.case("53x70x4-step-b1x1-t1"))
    assert f1.shape == (53, 70, 4) and not np.array_equal(f1[..., 3], f2[..., 3])
    d = f2[..., :3].astype(int) - f1[..., :3]
    assert ((d[..., 0] > 0) & (d[..., 1] < 0)).any()
    assert (d.reshape(-1, 3) == (1, 1, 0)).all(1).any()


def test_large_cases_hold_both_values():
    bad = [c.name for c in C.cases() if C.large(c.rows, c.cols) and not (C.expected(c).any() and not C.expected(c).all())]
    assert not bad, bad
    assert all(set(np.unique(C.expected(c))) <= {0, 1} for c in C.cases())


@pytest.mark.parametrize("mut", sorted(SHOWN_BY))
def test_mutation_changes_a_named_case(mut):
    c = C.case(SHOWN_BY[mut])
    f1, f2 = C.frames(c)
    got = R.frame_difference(f1, f2, c.thresh, c.ksize, c.sigma, mut=(mut,))
    assert not np.array_equal(got, C.expected(c)), (mut, c.name)


def test_every_mutation_is_shown():
    assert set(SHOWN_BY) == R.COLOR_MUTATIONS | {"sub_abs"}
    with pytest.raises(ValueError):
        R.grey(np.zeros((1, 3), np.uint8), mut=("no_such",))


def test_sequence_and_batch_expectations():
    h = C.HISTORY
    hist, diffs = C.history_expected()
    assert hist.shape == (4, 53, 70) and diffs.shape == (4, 53, 70)
    assert np.array_equal(hist[1], hist[3]) and np.array_equal(diffs[2], diffs[3])
    assert set(np.unique(diffs)) == {0, 1} and not diffs[0].any()  # the block rests at update 8
    # the loop of single steps
    fr = C.history_frames()
    hh = np.zeros((53, 70), np.uint8)
    for j in range(1, 8):
        d = R.frame_difference(fr[j - 1], fr[j], h["thresh"], h["ksize"], h["sigma"])
        hh = M.update(hh, d, h["tau"])
        for i, s in enumerate(h["save"]):
            if s == j:
                assert np.array_equal(hist[i], hh)
    # every video of the batch ends with something in its history, and the two thresholds give different masks
    want = C.batch_expected()
    assert all(w.any() for w in want) and {b["tau"] for b in C.BATCH} == {1, 3, 300}
    assert {b["F"] for b in C.BATCH} >= {2, 9} and any(b["save"] == 1 for b in C.BATCH)
    assert any(b["save"] == b["F"] - 1 and b["F"] > 2 for b in C.BATCH)
    f = C.batch_videos()[3]
    assert not np.array_equal(R.frame_difference(f[0], f[1], 20, (3, 3), 1.0), R.frame_difference(f[0], f[1], 38, (3, 3), 1.0))
