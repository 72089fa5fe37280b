"""The exact integer references of disparitySSD (tests/_stereo_ref.py) against the C oracle, byte for byte, on small
8-bit-valued pairs: every radius the exact-sum kernels take and one past it, every CUDA-path flag set, degenerate and
ragged shapes, disparity ranges on either side of 0, across it and the whole int8 range.  No GPU."""
import numpy as np
import pytest

import _oracle as orc
import _stereo_ref as ref

SHAPES = [(1, 1), (1, 23), (19, 1), (6, 9), (13, 37)]  # 1 x 1, 1 x n, n x 1, cols < window (r >= 5), ragged
RANGES = [(-20, -3), (4, 30), (-9, 12), (-128, 127)]


def _pair(rng, rows, cols, kind, top=255):
    if kind == "noise":
        left = rng.integers(0, top + 1, (rows, cols))
        right = np.roll(left, -3, axis=1)
        right[::2] = rng.integers(0, top + 1, right[::2].shape)
    else:  # two levels: ties everywhere
        left = rng.integers(0, 2, (rows, cols)) * top
        right = rng.integers(0, 2, (rows, cols)) * top
    return left.astype(np.float32), right.astype(np.float32)


@pytest.mark.parametrize("rad", [0, 1, 2, 3, 4, 5, 6, 7, 12])
def test_exact_reference_equals_the_oracle(rad):
    rng = np.random.default_rng(100 + rad)
    # radius 12: (2r+1)^2 * 100^2 < 2^24 keeps the float contract's sums exact (at 255 they would round)
    top = 100 if rad > 7 else 255
    n = 0
    for i, (rows, cols) in enumerate(SHAPES):
        for j, (lo, hi) in enumerate(RANGES):
            left, right = _pair(rng, rows, cols, ("noise", "levels")[(i + j) % 2], top)
            for flags in range(4):
                if flags & ref.COLS_2R and rad == 0:
                    continue
                got = ref.ssd_cuda(left, right, rad, lo, hi, flags)
                assert np.array_equal(got, orc.disparity_ssd(left, right, rad, lo, hi, flags)), (rows, cols, lo, hi, flags)
                n += 1
            got = ref.ssd_serial(left, right, rad, lo, hi)
            assert np.array_equal(got, orc.disparity_ssd_serial(left, right, rad, lo, hi)), (rows, cols, lo, hi)
    assert n == len(SHAPES) * len(RANGES) * (2 if rad == 0 else 4)


def test_exact_reference_refuses_other_images():
    ok = np.zeros((4, 5), np.float32)
    for bad in (0.5, -1.0, 256.0, np.nan, np.inf):
        img = ok.copy()
        img[2, 3] = bad
        with pytest.raises(ValueError):
            ref.ssd_cuda(img, ok, 1, -2, 2)
        with pytest.raises(ValueError):
            ref.ssd_serial(ok, img, 1, -2, 2)
    assert np.array_equal(ref.ssd_cuda(-ok, ok, 1, -2, 2), np.full((4, 5), -2, np.int8))  # -0.0 is a legal 0
    with pytest.raises(ValueError):
        ref.ssd_cuda(ok, ok, 1, -2, 2, flags=4)  # SERIAL is ssd_serial


def test_exact_reference_is_fast_at_size():
    """1080 x 1920, 128 disparities: the size the GPU tests compare at (one core, a few seconds)."""
    import time
    rng = np.random.default_rng(7)
    left = rng.integers(0, 256, (1080, 1920)).astype(np.float32)
    right = np.roll(left, -9, axis=1)  # right(y, x) = left(y, x + 9): left(x) is right(x - 9), disparity -9
    t = time.perf_counter()
    got = ref.ssd_cuda(left, right, 5, -127, 0)
    assert time.perf_counter() - t < 20
    assert (got[:, 20:-20] == -9).all()  # (the clamped edges aside)
