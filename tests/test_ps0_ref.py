"""tests/_ps0_ref.py against independent computations (CPU): the statistics against fractions.Fraction sums, the arithmetic
chain against four separate array steps, the noise rule against an int16 computation, and swap o swap."""
from fractions import Fraction

import numpy as np

import _ps0_ref as R


def test_stats_against_fraction_sums():
    rng = np.random.default_rng(1)
    for img in (rng.integers(0, 256, (1, 1), dtype=np.uint8), rng.integers(0, 256, (37, 53), dtype=np.uint8), np.full((300, 300), 255, np.uint8),
                np.zeros((5, 5), np.uint8)):
        st = R.mean_stddev(img)
        vals = [int(v) for v in img.ravel()]
        n = len(vals)
        s, q = sum(vals), sum(v * v for v in vals)
        assert (st["sum"], st["sqsum"], st["min"], st["max"]) == (s, q, min(vals), max(vals))
        mean, var = Fraction(s, n), Fraction(q, n) - Fraction(s, n) ** 2
        assert abs(Fraction(float(st["mean"])) - mean) <= Fraction(float(np.spacing(st["mean"])))  # two roundings
        # the variance is a difference of two numbers near 255^2, each good to a few ulp of itself
        assert abs(Fraction(float(st["stddev"])) ** 2 - var) <= Fraction(float(8 * np.spacing(np.float64(q / n) + 1)))
    assert R.mean_stddev(np.full((4100, 4100), 255, np.uint8))["sum"] == 255 * 4100 * 4100 > 2 ** 31  # past int32
    assert R.mean_stddev(np.full((300, 300), 255, np.uint8))["sqsum"] == 65025 * 90000 > 2 ** 32


def test_arithmetic_chain_against_four_separate_steps():
    img = R.all_bytes()
    for mean, sd in R.ARITH_PARAMS:
        with np.errstate(all="ignore"):
            t = img.copy()
            t = R.sat_u8(R.cv_round(t.astype(np.float64) - np.float64(mean)))
            t = R.sat_u8(R.cv_round(t.astype(np.float32) * np.float32(1.0 / np.float64(sd) if sd else np.inf)))
            t = R.sat_u8(R.cv_round(t.astype(np.float32) * np.float32(10)))
            t = R.sat_u8(R.cv_round(t.astype(np.float64) + np.float64(mean)))
        assert np.array_equal(R.arithmetic(img, mean, sd), t), (mean, sd)
    assert (R.arithmetic(img, 127.3, 0.0) == 127).all()  # a = inf: t2 = 0 everywhere, then 0 + mean
    assert not R.arithmetic(img, R.NAN, 1.0).any()
    # t1 = 0 .. 155, t2 = round(t1 / 50) = 0 .. 3: the chain leaves four values, mean + 10 k
    assert list(np.unique(R.arithmetic(img, 100.0, 50.0))) == [100, 110, 120, 130]


def test_cv_round():
    got = R.cv_round(np.asarray([0.5, 1.5, 2.5, -0.5, -1.5, 2147483647.4, 2147483647.5, -2147483648.5, R.NAN, R.INF], np.float64))
    assert list(got) == [0, 2, 2, 0, -2, 2147483647, R.INT_MIN, -2147483648, R.INT_MIN, R.INT_MIN]


def test_noise_rule_against_int16():
    p = np.repeat(np.arange(256, dtype=np.uint8), len(R.SPECIAL_NOISE)).reshape(256, -1)
    z = np.tile(np.asarray(R.SPECIAL_NOISE, np.float32), (256, 1))
    n16 = np.zeros(z.shape, np.int16)
    for j, v in enumerate(R.SPECIAL_NOISE):
        v = np.float32(v)
        n16[:, j] = -128 if not np.isfinite(v) or abs(v) > 1e6 else int(np.clip(np.rint(v), -128, 127))
    s = np.clip(np.minimum(p.astype(np.int16), 127) + n16, -128, 127)
    assert np.array_equal(R.add_noise(p, z), np.maximum(s, 0).astype(np.uint8))
    assert R.add_noise(np.asarray([[200]], np.uint8), [[0.0]])[0, 0] == 127  # the reference's clip of the image


def test_swap_of_swap_is_the_identity_and_paste():
    _, img = R.image(9, 11, 3, 4, 2)
    assert np.array_equal(R.mix_channels(R.mix_channels(img, (2, 1, 0)), (2, 1, 0)), img)
    assert R.square(99, 200, 99, 200, 100) is None and R.square(100, 100, 100, 100, 100) == (0, 0, 0, 0)
    a, b = np.full((131, 259), 1, np.uint8), np.full((117, 140), 2, np.uint8)
    out = R.pixel_replacement(a, b)
    assert out.sum() == 2 * 117 * 140 - 100 * 100 and out[8, 20] == 1 and out[7, 20] == 2 and out[8, 19] == 2
