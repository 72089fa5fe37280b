"""Exact numpy restatement of the "ps4: registration" contract (include/mi_cv.h): cv::invertAffineTransform,
cv::warpAffine (INTER_LINEAR / INTER_NEAREST, BORDER_CONSTANT 0, with and without WARP_INVERSE_MAP) and cv::addWeighted
on single-channel u8 and f32 images, and runProblem3's tail built from them.  Written from the rules, not from the
kernel: coordinates and the u8 blend are integer arithmetic, the f32 blend and addWeighted are np.float32 operations
one step at a time (IEEE, no FMA); doubles are np.float64."""
import numpy as np

WARP_INVERSE_MAP, WARP_NEAREST = 16, 1
INT_MIN = -(1 << 31)
_F64 = np.float64


def cv_round(v):
    """cvRound(double) as cvtsd2si: ties to even; NaN or a rounded value outside int32 -> INT_MIN.  int64 array."""
    v = np.asarray(v, _F64)
    with np.errstate(invalid="ignore"):
        r = np.rint(v)
        ok = (r >= -2147483648.0) & (r < 2147483648.0)
        return np.where(ok, np.where(ok, r, 0).astype(np.int64), INT_MIN)


def _wrap32(v):
    """int32 wrap-around of an int64 array."""
    return ((np.asarray(v, np.int64) + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def _invert64(m):
    """The double formulas on six doubles -> six doubles (np.float64 scalars, unfused)."""
    m0, m1, m2, m3, m4, m5 = (_F64(v) for v in m)
    with np.errstate(all="ignore"):
        D = m0 * m4 - m1 * m3
        D = _F64(1.0) / D if D != 0 else _F64(0.0)
        A11, A22, A12, A21 = m4 * D, m0 * D, -m1 * D, -m3 * D
        b1 = -A11 * m2 - A12 * m5
        b2 = -A21 * m2 - A22 * m5
    return [A11, A12, b1, A21, A22, b2]


def invert_affine(m):
    """cv::invertAffineTransform on 2x3 f32 (or [count, 2, 3]): each result rounded once to float."""
    m = np.asarray(m, np.float32)
    flat = m.reshape(-1, 6)
    with np.errstate(all="ignore"):
        out = np.array([[np.float32(v) for v in _invert64(r)] for r in flat], np.float32)
    return out.reshape(m.shape)


def _warp_matrix(m, inverse_map):
    M = [_F64(v) for v in np.asarray(m, np.float32).reshape(6)]
    if inverse_map:
        return M
    with np.errstate(all="ignore"):
        D = M[0] * M[4] - M[1] * M[3]
        D = _F64(1.0) / D if D != 0 else _F64(0.0)
        A11, A22 = M[4] * D, M[0] * D
        M[0] = A11
        M[1] = M[1] * -D
        M[3] = M[3] * -D
        M[4] = A22
        b1 = -M[0] * M[2] - M[1] * M[5]
        b2 = -M[3] * M[2] - M[4] * M[5]
        M[2], M[5] = b1, b2
    return M


def coords(m, drows, dcols, flags=0):
    """(X, Y) int64 arrays [drows, dcols] holding the int32 fixed-point coordinates after the shift
    (1/32 px for linear, whole pixels for nearest)."""
    M = _warp_matrix(m, bool(flags & WARP_INVERSE_MAP))
    nearest = bool(flags & WARP_NEAREST)
    delta, shift = (512, 10) if nearest else (16, 5)
    x = np.arange(dcols, dtype=_F64)
    y = np.arange(drows, dtype=_F64)
    with np.errstate(all="ignore"):
        adelta = cv_round(M[0] * x * _F64(1024))
        bdelta = cv_round(M[3] * x * _F64(1024))
        X0 = _wrap32(cv_round((M[1] * y + M[2]) * _F64(1024)) + delta)
        Y0 = _wrap32(cv_round((M[4] * y + M[5]) * _F64(1024)) + delta)
    X = _wrap32(X0[:, None] + adelta[None, :]) >> shift
    Y = _wrap32(Y0[:, None] + bdelta[None, :]) >> shift
    return X, Y


def _taps(src, sy, sx):
    """src[sy, sx] with 0 outside the image (never indexed there)."""
    rows, cols = src.shape
    ok = (sy >= 0) & (sy < rows) & (sx >= 0) & (sx < cols)
    v = src[np.where(ok, sy, 0), np.where(ok, sx, 0)]
    return np.where(ok, v, src.dtype.type(0))


def warp_affine(src, m, dsize=None, flags=0):
    """cv::warpAffine(src, dst, m, dsize, flags), BORDER_CONSTANT 0.  dsize = (width, height) as cv::Size; None = src's."""
    src = np.asarray(src)
    assert src.ndim == 2 and src.dtype in (np.uint8, np.float32)
    dcols, drows = (src.shape[1], src.shape[0]) if dsize is None else (int(dsize[0]), int(dsize[1]))
    X, Y = coords(m, drows, dcols, flags)
    if flags & WARP_NEAREST:
        return _taps(src, np.clip(Y, -32768, 32767), np.clip(X, -32768, 32767))
    sx, sy = np.clip(X >> 5, -32768, 32767), np.clip(Y >> 5, -32768, 32767)
    fx, fy = X & 31, Y & 31
    p00, p01 = _taps(src, sy, sx), _taps(src, sy, sx + 1)
    p10, p11 = _taps(src, sy + 1, sx), _taps(src, sy + 1, sx + 1)
    if src.dtype == np.uint8:
        w00, w01 = (32 - fx) * (32 - fy) * 32, fx * (32 - fy) * 32
        w10, w11 = (32 - fx) * fy * 32, fx * fy * 32
        s = w00 * p00.astype(np.int64) + w01 * p01.astype(np.int64) + w10 * p10.astype(np.int64) + w11 * p11.astype(np.int64)
        return ((s + 16384) >> 15).astype(np.uint8)
    f = np.float32
    ax1 = fx.astype(f) * f(0.03125)
    ay1 = fy.astype(f) * f(0.03125)
    ax0, ay0 = f(1) - ax1, f(1) - ay1
    with np.errstate(all="ignore"):
        r = p00 * (ay0 * ax0)
        r = r + p01 * (ay0 * ax1)
        r = r + p10 * (ay1 * ax0)
        r = r + p11 * (ay1 * ax1)
    return r.astype(f)


def add_weighted(a, alpha, b, beta, gamma=0.0):
    """cv::addWeighted(a, alpha, b, beta, gamma): float (a*alpha + b*beta) + gamma; u8 = cvRound, saturated."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and a.dtype in (np.uint8, np.float32)
    f = np.float32
    with np.errstate(all="ignore"):
        t = a.astype(f) * f(alpha) + b.astype(f) * f(beta)
        t = t + f(gamma)
    if a.dtype == np.float32:
        return t.astype(f)
    return np.clip(cv_round(t.astype(_F64)), 0, 255).astype(np.uint8)


def register_blend(a, b, m_a_to_b):
    """Solution.cpp:315-325: (reverseWarp, blended)."""
    warped = warp_affine(b, invert_affine(m_a_to_b), (a.shape[1], a.shape[0]), 0)
    return warped, add_weighted(a, 0.5, warped, 0.5, 0.0)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    """Equal bit for bit, NaNs compared by position (their payload is not part of the contract)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype != np.float32:
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb]))
