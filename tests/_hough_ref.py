"""Exact numpy reference of ps1's Hough chain, written from
ProblemSets/ps1_cpp/src/Hough.cu alone -- no oracle code.  Line numbers below are that file's.

Every quantity is either an integer count or a float32 value produced by the same IEEE operations
the source performs (float32 products and sums in numpy are exactly the device's, since the
library is built without contraction), so the accumulators and peak lists are compared with
np.array_equal.  The decisions of DESIGN.md §2 are applied where the source is not reproducible
or not defined:
  * __sincosf (:53, :86) is replaced by the correctly rounded double cos / sin of the float radian,
    cast to float (math.cos / math.sin: the C library's, as the library's host table uses);
  * votes outside the accumulator are dropped (the source writes out of bounds, :57);
  * float -> unsigned conversion of the circle centre saturates (negative and NaN -> 0, >= 2^32 ->
    2^32 - 1), which is what the device conversion does;
  * the circle accumulator is zeroed (the source forgets to, :318).
"""
import math

import numpy as np

PI = 3.14159265  # :20
MIN_THETA, MAX_THETA, THETA_WIDTH = -90, 90, 180  # Hough.h: the line loop runs theta = -90 .. 89


def deg_to_rad(theta):
    """degToRad (:22-24): float theta * double PI / 180.f, returned as float."""
    return np.float32(float(np.float32(theta)) * PI / float(np.float32(180.0)))


def trig(theta0, n=360, pi=PI):
    """float cos / sin of degToRad(theta0 + i), i < n, each the correctly rounded double of the
    float radian cast to float."""
    c = np.empty(n, np.float32)
    s = np.empty(n, np.float32)
    for i in range(n):
        rad = float(np.float32(float(np.float32(theta0 + i)) * pi / 180.0))
        c[i] = np.float32(math.cos(rad))
        s[i] = np.float32(math.sin(rad))
    return c, s


def roundf(v):
    """C roundf: half away from zero (numpy's round is half to even).  Exact for float32 input:
    floor(|v| + 0.5) in float64 has no rounding error for |v| < 2^52."""
    v = np.asarray(v, np.float32)
    a = np.floor(np.abs(v).astype(np.float64) + 0.5)
    return np.copysign(a, v).astype(np.float32)


def points(mask, row0=0):
    """Row-major (x, y) of the nonzero pixels (IsNonzero :182-186, thrust::copy_if :226-227).
    A band holds rows row0 .. row0 + mask.shape[0] - 1 of the image."""
    ys, xs = np.nonzero(np.asarray(mask) > 0)  # row-major
    return xs.astype(np.int64), ys.astype(np.int64) + row0


def lines_dims(rows, cols, rho_bin, theta_bin):
    """:258-262: maxDist = ceil(sqrt(rows^2 + cols^2)) (int arithmetic, double sqrt), bins by
    float ceil, at least 1."""
    max_dist = int(math.ceil(math.sqrt(rows * rows + cols * cols)))
    rb = max(1, int(math.ceil(np.float32(2 * max_dist) / np.float32(rho_bin))))
    tb = max(1, int(math.ceil(np.float32(THETA_WIDTH) / np.float32(theta_bin))))
    return rb, tb, max_dist


def lines_votes(mask, rho_bin=1, theta_bin=1, row0=0, rows=None, *, rounder=roundf, pi=PI, fused=False):
    """houghLinesAccumulateKernel (:35-59) for every point: (rhoBin, thetaBin) int64 arrays of shape
    [points, thetas] before the bounds test.  rounder / pi / fused exist for the mutation tests."""
    mask = np.asarray(mask)
    rows = mask.shape[0] if rows is None else rows
    _, _, diag = lines_dims(rows, mask.shape[1], rho_bin, theta_bin)
    xs, ys = points(mask, row0)
    thetas = np.arange(MIN_THETA, MAX_THETA, theta_bin)  # :51
    c, s = trig(MIN_THETA, 180, pi)
    c, s = c[thetas - MIN_THETA], s[thetas - MIN_THETA]
    fx, fy = xs.astype(np.float32)[:, None], ys.astype(np.float32)[:, None]
    if fused:  # one rounding for x*c + y*s (a contraction the contract forbids)
        t = (fx.astype(np.float64) * c + (fy * s).astype(np.float64)).astype(np.float32)
    else:
        t = fx * c + fy * s  # :54, float32 product, product, sum
    rho = rounder(t) + np.float32(diag)
    rho_b = rounder(rho / np.float32(rho_bin)).astype(np.int64)  # :55
    theta_b = np.broadcast_to((thetas - MIN_THETA) // theta_bin, rho_b.shape)  # :56, integer division
    return rho_b, theta_b


def hough_lines(mask, rho_bin=1, theta_bin=1, row0=0, rows=None, *, clamp=False, **mut):
    """cuda::houghLinesAccumulate (:251-290): int32 [rhoBins, thetaBins]; votes with rhoBin outside
    [0, rhoBins) are dropped (clamp=True: the mutation that clamps them instead)."""
    mask = np.asarray(mask)
    rows = mask.shape[0] if rows is None else rows
    rb, tb, _ = lines_dims(rows, mask.shape[1], rho_bin, theta_bin)
    r, t = lines_votes(mask, rho_bin, theta_bin, row0, rows, **mut)
    r, t = r.ravel(), t.ravel()
    if clamp:
        r = np.clip(r, 0, rb - 1)
    keep = (r >= 0) & (r < rb) & (t < tb)
    acc = np.bincount(r[keep] * tb + t[keep], minlength=rb * tb)
    return acc.reshape(rb, tb).astype(np.int32)


def dropped_line_votes(mask, rho_bin=1, theta_bin=1):
    """(votes with rhoBin < 0, votes with rhoBin >= rhoBins) -- the votes the contract drops."""
    rb, _, _ = lines_dims(mask.shape[0], mask.shape[1], rho_bin, theta_bin)
    r, _ = lines_votes(mask, rho_bin, theta_bin)
    return int((r < 0).sum()), int((r >= rb).sum())


def sat_u32(v):
    """float32 -> uint32, saturating (NaN and negatives -> 0, >= 2^32 -> 2^32 - 1), truncating."""
    v = np.asarray(v, np.float32).astype(np.float64)
    out = np.zeros(v.shape, np.int64)
    ok = v > 0
    out[ok] = np.minimum(np.trunc(v[ok]), 4294967295.0).astype(np.int64)
    return out


def circle_votes(mask, radius, row0=0, chunk=4096):
    """houghCirclesAccumulateKernel (:70-95): yields (a, b) int64 arrays [points, 360] per chunk of
    points; a = sat_u32(fl(x - fl(float(radius) * cos))), b likewise (:87-88)."""
    xs, ys = points(mask, row0)
    c, s = trig(0)
    r = np.float32(radius)  # size_t -> float, round to nearest
    rc, rs = r * c, r * s
    for i in range(0, len(xs), chunk):
        fx = xs[i:i + chunk].astype(np.float32)[:, None]
        fy = ys[i:i + chunk].astype(np.float32)[:, None]
        yield sat_u32(fx - rc), sat_u32(fy - rs)


def hough_circles(mask, radius, row0=0, rows=None, *, a_ge0=False):
    """cuda::houghCirclesAccumulate (:311-346): dense int32 [rows, cols], zeroed; a vote counts when
    0 < a < cols and 0 < b < rows (:91).  a_ge0: the mutation that admits a = 0 / b = 0."""
    mask = np.asarray(mask)
    rows = mask.shape[0] if rows is None else rows
    cols = mask.shape[1]
    acc = np.zeros(rows * cols, np.int64)
    lo = 0 if a_ge0 else 1
    for a, b in circle_votes(mask, radius, row0):
        keep = (a < cols) & (b < rows) & (a >= lo) & (b >= lo)
        acc += np.bincount((b[keep] * cols + a[keep]), minlength=rows * cols)
    return acc.reshape(rows, cols).astype(np.int32)


def local_maxima(acc, *, strict=True, inclusive=False):
    """findLocalMaximaKernel (:137-162): a cell is a "local maximum" unless some accumulator(y, x) >
    its own value for y in [max(0, ty - 1), min(rows - 1, ty + 1)) and x likewise -- exclusive upper
    bounds as written, so only the cells up / left (and the cell itself) are looked at, and the last
    row / column look at fewer.  strict=False (>= against the other cells) and inclusive=True (<=
    upper bounds) are mutations."""
    acc = np.asarray(acc, np.int64)
    rows, cols = acc.shape
    ty, tx = np.mgrid[0:rows, 0:cols]
    y_end = np.minimum(rows - 1, ty + 1) + (1 if inclusive else 0)
    x_end = np.minimum(cols - 1, tx + 1) + (1 if inclusive else 0)
    is_max = np.ones((rows, cols), bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy == 0 and dx == 0:
                continue  # v > v is never true
            y, x = ty + dy, tx + dx
            inside = (y >= 0) & (y < y_end) & (x >= 0) & (x < x_end)
            nb = acc[np.clip(y, 0, rows - 1), np.clip(x, 0, cols - 1)]
            beats = nb > acc if strict else nb >= acc
            is_max &= ~(inside & beats)
    return is_max


def hough_peaks(acc, num_peaks, threshold, *, stable=True, **mut):
    """cuda::findLocalMaxima (:366-415): local maxima with votes >= threshold (MaskAndThreshold
    :239-249, remove_if keeps row-major order), stable_sort by votes descending (:402), the first
    num_peaks, as (rho = row, theta = col) uint32 pairs (:410-414).  The source carries row / col in
    float fields (:99, :161): exact for every index below 2^24, which is as far as it is taken here.
    stable=False: the mutation that breaks ties by descending index."""
    acc = np.asarray(acc, np.int64)
    rows, cols = acc.shape
    assert rows < (1 << 24) and cols < (1 << 24)
    sel = local_maxima(acc, **mut) & (acc >= threshold)
    idx = np.flatnonzero(sel)
    v = acc.ravel()[idx]
    order = np.argsort(-v, kind="stable") if stable else np.lexsort((-idx, -v))
    idx = idx[order][:num_peaks]
    return np.stack([idx // cols, idx % cols], axis=1).astype(np.uint32).reshape(-1, 2)


# ---- the work split of hough.hip's tiled circle kernel (not part of the reference: the tests use it to
# show that their masks reach the kernel's chunk and packing limits) ----

CIRCLE_TA, CIRCLE_TB, CIRCLE_CHUNK = 64, 32, 2048


def circle_reach(radius, rows, cols):
    """Rows / columns beyond a tile whose points can vote into it, as micv_hough_circles_band_dev sets it."""
    return min(int(radius) + 1, rows + cols)


def circle_tile_loads(mask, radius, row0=0, rows=None):
    """Per 64 x 32 accumulator tile: the points of its row range [b0 - reach, b0 + 32 + reach) (what
    the kernel walks in chunks of 2048) and those that also pass its column filter
    [a0 - reach, a0 + 64 + reach).  Returns the two maxima over the tiles."""
    m = (np.asarray(mask) > 0).astype(np.int64)
    rows = m.shape[0] if rows is None else rows
    cols = m.shape[1]
    full = np.zeros((rows, cols), np.int64)
    full[row0:row0 + m.shape[0]] = m
    sat = np.zeros((rows + 1, cols + 1), np.int64)
    sat[1:, 1:] = full.cumsum(0).cumsum(1)
    reach = circle_reach(radius, rows, cols)
    b0 = np.arange(0, rows, CIRCLE_TB)[:, None]
    a0 = np.arange(0, cols, CIRCLE_TA)[None, :]
    y0, y1 = np.clip(b0 - reach, 0, rows), np.clip(b0 + CIRCLE_TB + reach, 0, rows)
    x0, x1 = np.clip(a0 - reach, 0, cols), np.clip(a0 + CIRCLE_TA + reach, 0, cols)
    in_rows = sat[y1, cols] - sat[y0, cols]
    listed = sat[y1, x1] - sat[y0, x1] - sat[y1, x0] + sat[y0, x0]
    return int(in_rows.max()), int(listed.max())
