"""tests/_display_ref.py (the restatement the GPU tests of the "display" block compare against) checked on the CPU against
the two restatements that already exist -- viz.normalize_minmax_u8 and viz.jet_lut -- and against properties of the
contract; cv::randn against tests/_pf_ref.CvRng and the host entry point micv_cv_randn_f32_host (no device needed)."""
import numpy as np
import pytest

import _display_ref as dr
import _pf_ref as pf
from introtocomputervision_amd import viz

F32 = np.float32


def fields(seed, count):
    """Random f32 fields: magnitudes 1e-3 .. 1e4, range 1e-3 .. 1 of the magnitude."""
    rng = np.random.default_rng(seed)
    for _ in range(count):
        rows, cols = (int(v) for v in rng.integers(1, 40, 2))
        mag = 10.0 ** rng.uniform(-3, 4)
        span = mag * 10.0 ** rng.uniform(-3, 0)
        centre = rng.uniform(-1, 1) * (mag - span / 2)
        yield (centre + span * (rng.random((rows, cols)) - 0.5)).astype(F32), mag


def test_normalize_equals_viz_on_f32_fields():
    for img, _ in fields(0x5EED0D01, 400):
        assert np.array_equal(dr.normalize(img), viz.normalize_minmax_u8(img))


def test_normalize_equals_viz_with_nan_and_inf():
    rng = np.random.default_rng(0x5EED0D02)
    img = (rng.standard_normal((23, 31)) * 3).astype(F32)
    img[3, 4] = np.nan
    img[0, 0] = np.nan
    assert np.array_equal(dr.normalize(img), viz.normalize_minmax_u8(img))
    lo, hi = dr.minmax(img)
    clean = img[~np.isnan(img)]
    assert lo == clean.min() and hi == clean.max()  # NaNs do not move the range
    assert dr.normalize(img)[3, 4] == 0 and dr.normalize(img)[0, 0] == 0
    img[5, 5] = np.inf
    with np.errstate(all="ignore"):
        assert np.array_equal(dr.normalize(img), viz.normalize_minmax_u8(img))
    assert not dr.normalize(img).any()  # an infinite range: scale 0


def test_jet_table_equals_viz():
    assert np.array_equal(dr.jet_lut(), viz.jet_lut())
    v = np.arange(256, dtype=np.uint8).reshape(16, 16)
    assert np.array_equal(dr.jet(v), viz.apply_colormap_jet(v))
    lut = dr.jet_lut()
    assert tuple(lut[0]) == (128, 0, 0) and tuple(lut[255]) == (0, 0, 128)  # B, G, R


def test_constant_and_all_nan_images_give_zeros():
    assert not dr.normalize(np.full((5, 7), 3.25, F32)).any()
    assert not dr.normalize(np.full((5, 7), -7, np.int8)).any()
    assert not dr.normalize(np.full((5, 7), 200, np.uint8)).any()
    assert not dr.normalize(np.full((4, 4), np.nan, F32)).any()
    assert np.isnan(dr.minmax(np.full((4, 4), np.nan, F32))[0])
    z = np.zeros((3, 3), F32)
    z[1, 1] = -0.0
    assert not dr.normalize(z).any()


def test_output_spans_0_to_255():
    """On every f32 image whose range is at least 1e-3 of its largest magnitude, and on every int8 / uint8 image with two
    distinct values (with a range of a few ulps the float shift swallows the result: hence the condition)."""
    n = 0
    for img, _ in fields(0x5EED0D03, 2000):
        lo, hi = float(img.min()), float(img.max())
        if hi - lo < 1e-3 * max(abs(lo), abs(hi)) or img.size < 2:
            continue
        out = dr.normalize(img)
        assert out.min() == 0 and out.max() == 255, (lo, hi)
        n += 1
    assert n > 1000
    rng = np.random.default_rng(0x5EED0D04)
    for lo, hi in ((-95, 0), (0, 95), (-3, 0), (-128, 127), (-1, 0), (5, 6)):
        img = rng.integers(lo, hi + 1, (17, 19)).astype(np.int8)
        img[0, 0], img[0, 1] = lo, hi
        out = dr.normalize(img)
        assert out.min() == 0 and out.max() == 255 and out[0, 0] == 0 and out[0, 1] == 255
        assert np.array_equal(out, viz.normalize_minmax_u8(img.astype(F32)))  # (float)int8 is exact
    for lo, hi in ((0, 255), (7, 8), (100, 197)):
        img = rng.integers(lo, hi + 1, (9, 33)).astype(np.uint8)
        img[0, 0], img[0, 1] = lo, hi
        out = dr.normalize(img)
        assert out.min() == 0 and out.max() == 255
        assert np.array_equal(out, viz.normalize_minmax_u8(img.astype(F32)))


def test_invert_and_gain_noise():
    v = np.arange(256, dtype=np.uint8)
    assert np.array_equal(dr.invert(v), v[::-1])
    rng = np.random.default_rng(0x5EED0D05)
    a = rng.integers(0, 256, (6, 9)).astype(F32)
    n = (rng.standard_normal((6, 9)) * 10).astype(F32)
    assert dr.same(dr.gain_noise(a, 1.0, n), a + n)  # first + noise
    assert dr.same(dr.gain_noise(a, F32(1.1)), a * F32(1.1))  # left * contrastFactor
    assert dr.gain_noise(a, 1.1).dtype == F32


def test_randn_stands_on_cvrng():
    img, state = dr.randn(0xFFFFFFFF, 0.0, 10.0, 3, 4)
    rng = pf.CvRng()
    z = [rng.gaussian(1.0) for _ in range(12)]
    assert state == rng.state
    assert dr.same(img.ravel(), (np.array(z, np.float64).astype(F32) * F32(10)).astype(F32))
    assert dr.same(img.ravel()[:4], np.array([-1.6030947e-08, 1.5813506, -7.0092797, -4.2859597], F32))
    # one call of n samples equals two calls of n / 2, the state carried over
    h0, s0 = dr.randn(0xFFFFFFFF, 1.5, 2.0, 3, 2)
    h1, s1 = dr.randn(s0, 1.5, 2.0, 3, 2)
    full, s = dr.randn(0xFFFFFFFF, 1.5, 2.0, 6, 2)
    assert s == s1 and dr.same(full, np.concatenate([h0, h1]))


def test_randn_library_equals_restatement():
    from introtocomputervision_amd import display
    rng = display.RNG()
    a = display.randn((37, 41), 0.0, 10.0, rng)
    b = display.randn((37, 41), -2.5, 0.75, rng)  # continues the generator, as cv::theRNG() does
    ea, s = dr.randn(0xFFFFFFFF, 0.0, 10.0, 37, 41)
    eb, s = dr.randn(s, -2.5, 0.75, 37, 41)
    assert dr.same(a, ea) and dr.same(b, eb) and rng.state == s


def test_randn_moments():
    """100 000 draws from the default state: mean and standard deviation within 4 standard errors of 0 and 1."""
    from introtocomputervision_amd import display
    n = 100000
    z = display.randn((250, 400), 0.0, 1.0, display.RNG()).astype(np.float64).ravel()
    assert abs(z.mean()) < 4 / np.sqrt(n)
    assert abs(z.std() - 1) < 4 / np.sqrt(2 * n)
    assert np.sum(np.abs(z) > 3.442620) == 54  # the tail branch
