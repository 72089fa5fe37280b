"""numpy restatement of the "display" block of include/mi_cv.h, written from the contract, not from
the library: min-max normalisation to 8 bits for float32 / uint8 / int8 sources, the inversion, the JET table, the
gain / noise expression and cv::randn on a CV_32FC1 image.  Everything is exact: the GPU tests compare bit for bit."""
import numpy as np

import _pf_ref as pf

F32 = np.float32
DBL_EPSILON = float(np.finfo(np.float64).eps)


def minmax(src):
    """(lo, hi) as float32, NaNs skipped, +/-Inf taking part; (NaN, NaN) for an image without a non-NaN value."""
    v = np.asarray(src).astype(F32).ravel()
    v = v[~np.isnan(v)]
    if v.size == 0:
        return F32(np.nan), F32(np.nan)
    return F32(v.min()), F32(v.max())


def constants(lo, hi):
    """(a, b): scale = 255 * (hi - lo > DBL_EPSILON ? 1 / (hi - lo) : 0), shift = 0 - lo * scale in double; then float."""
    if np.isnan(lo):
        return F32(0), F32(0)
    with np.errstate(all="ignore"):
        lo, hi = np.float64(lo), np.float64(hi)
        d = hi - lo
        scale = np.float64(255.0) * (np.float64(1.0) / d if d > DBL_EPSILON else np.float64(0.0))
        shift = np.float64(0.0) - lo * scale
        return F32(scale), F32(shift)


def normalize(src):
    """cv::normalize(src, dst, 0, 255, NORM_MINMAX, CV_8U): t = (float)src * a + b, unfused; rint, clamp; 0 if not finite."""
    src = np.asarray(src)
    a, b = constants(*minmax(src))
    with np.errstate(all="ignore"):
        t = (src.astype(F32) * a).astype(F32) + b
        r = np.clip(np.rint(t), 0, 255)
    out = np.zeros(src.shape, np.uint8)
    ok = np.isfinite(t)
    out[ok] = r[ok].astype(np.uint8)
    return out


def invert(dst):
    return (255 - dst.astype(np.int32)).astype(np.uint8)


def jet_lut():
    """Entry i = (B, G, R) = cvRound(255 * clamp(1.5 - |4 x - k|, 0, 1)), k = 1, 2, 3, x = i / 255.0, in this order of
    operations in double; cvRound = ties to even."""
    lut = np.zeros((256, 3), np.uint8)
    for i in range(256):
        x = np.float64(i) / np.float64(255.0)
        for c, k in enumerate((1.0, 2.0, 3.0)):
            t = np.float64(1.5) - abs(np.float64(4.0) * x - np.float64(k))
            t = np.float64(0.0) if t < 0 else (np.float64(1.0) if t > 1 else t)
            lut[i, c] = int(np.rint(t * np.float64(255.0)))
    return lut


_LUT = None


def jet(dst):
    global _LUT
    if _LUT is None:
        _LUT = jet_lut()
    return _LUT[np.asarray(dst, np.uint8)]


def gain_noise(src, gain, noise=None):
    """src * gain + noise (or + 0.f) in float32, unfused."""
    with np.errstate(all="ignore"):
        t = (np.asarray(src, F32) * F32(gain)).astype(F32)
        return (t + (np.asarray(noise, F32) if noise is not None else F32(0))).astype(F32)


def randn(state, mean, sigma, rows, cols):
    """cv::randn on a rows x cols CV_32FC1 image from a cv::RNG in `state`: sample i (row-major) is the i-th ziggurat draw
    z, stored as z * sigma + mean in float32.  Returns (image, state afterwards)."""
    rng = pf.CvRng(state)
    z = np.array([rng.gaussian(1.0) for _ in range(rows * cols)], np.float64).astype(F32)  # the draws are floats
    img = ((z * F32(sigma)).astype(F32) + F32(mean)).astype(F32)
    return img.reshape(rows, cols), rng.state


def same(a, b):
    """Bit for bit; float32: NaNs by position, every other value by its bit pattern."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == F32:
        na, nb = np.isnan(a), np.isnan(b)
        return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32)))
    return bool(np.array_equal(a, b))
