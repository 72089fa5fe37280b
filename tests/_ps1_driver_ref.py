"""numpy restatement of what the ps1 driver (ProblemSets/ps1_cpp/src/main.cpp, Solution.cpp) does around the Hough
functions: the float blur and generateEdge on CV_32FC1, cv::erode with the elliptic footprint, findParallelLines,
GRAY2RGB, drawLinesParametric, drawCircles and the circle search over a radius range.  No library or oracle code; the
Hough and Canny parts come from _hough_ref / _edge_ref.

The OpenCV calls are not part of the reference tree; what is restated for them are the decisions DESIGN.md sections 2
and 3 record:
  * convertTo(CV_8U) = saturate_cast<uchar>(cvRound(v)), cvRound = cvtss2si: half to even; NaN, +-inf and everything
    outside int give INT_MIN, which saturates to 0;
  * cv::erode: BORDER_CONSTANT with FLT_MAX / 255, v = first tap, then v = (x < v) ? x : v in raster order;
  * cv::line, thickness 1, LINE_8: the walk of micv_viz::line (shim/micv_viz.hpp);
  * cv::circle, thickness 1: the midpoint walk of OpenCV 3.4's drawing.cpp.
"""
import math

import numpy as np

import _edge_ref as E
import _hough_ref as H

FLT_MAX = np.finfo(np.float32).max
PI_F = np.float32(3.14159265)  # Solution.cpp:17, a float


# ---- convertTo(CV_8U) --------------------------------------------------------------------------

def to_u8(v):
    v = np.asarray(v, np.float32)
    d = v.astype(np.float64)
    ok = np.isfinite(d) & (d >= -2147483648.0) & (d < 2147483648.0)
    r = np.where(ok, np.rint(np.where(ok, d, 0.0)), -2147483648.0)  # half to even
    return np.clip(r, 0, 255).astype(np.uint8)


# ---- blur / generateEdge on CV_32FC1 -------------------------------------------------------------

def blur_f32(img, n, sigma):
    """_edge_ref.blur on float pixels without its final rounding."""
    src = np.asarray(img, np.float32)
    rows, cols = src.shape
    taps = E.gaussian_taps(n, sigma)
    a = n // 2
    with np.errstate(invalid="ignore", over="ignore"):
        acc = np.zeros((rows, cols), np.float32)
        xi = np.arange(cols)
        for j in range(n):
            acc = E.fmaf(src[:, E.reflect101(xi - a + j, cols)], taps[j], acc)
        out = np.zeros((rows, cols), np.float32)
        yi = np.arange(rows)
        for j in range(n):
            out = E.fmaf(acc[E.reflect101(yi - a + j, rows), :], taps[j], out)
    return out


def generate_edge_f32(img, n, sigma, low, high):
    b = to_u8(blur_f32(img, n, sigma))
    weak, strong = E.suppress(b, low, high)
    return np.where(E.hysteresis(weak, strong), 255, 0).astype(np.uint8)


# ---- cv::erode, MORPH_ELLIPSE ---------------------------------------------------------------------

def ellipse_half_widths(k):
    """cv::getStructuringElement(MORPH_ELLIPSE, Size(k, k)): row i spans [c - hw, c + hw]."""
    r = c = k // 2
    inv_r2 = 1.0 / (r * r) if r else 0.0
    return tuple(int(np.rint(c * math.sqrt((r * r - (i - r) ** 2) * inv_r2))) for i in range(k))


def erode(img, k):
    img = np.asarray(img)
    border = FLT_MAX if img.dtype == np.float32 else img.dtype.type(255)
    r = k // 2
    rows, cols = img.shape
    p = np.full((rows + 2 * r, cols + 2 * r), border, img.dtype)
    p[r:r + rows, r:r + cols] = img
    v = None
    for i, hw in enumerate(ellipse_half_widths(k)):
        for dx in range(-hw, hw + 1):
            x = p[i:i + rows, r + dx:r + dx + cols]
            v = x.copy() if v is None else np.where(x < v, x, v)
    return v


# ---- findParallelLines -------------------------------------------------------------------------------

def parallel_lines(peaks, delta_theta, delta_rho):
    """The peaks whose (row / delta_rho, col / delta_theta) bin holds another peak, in input order."""
    p = np.asarray(peaks, np.uint32).reshape(-1, 2).astype(np.int64)
    key = (p[:, 0] // delta_rho * delta_rho) * (1 << 32) + p[:, 1] // delta_theta * delta_theta
    _, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
    return p[cnt[inv] > 1].astype(np.uint32).reshape(-1, 2)


# ---- overlays ---------------------------------------------------------------------------------------------

def gray2rgb(img):
    g = to_u8(img) if np.asarray(img).dtype == np.float32 else np.asarray(img, np.uint8)
    return np.repeat(g[:, :, None], 3, axis=2)


def line_walk(p1, p2):
    """micv_viz::line restated: the pixels (x, y) of the serial walk, in order."""
    (x1, y1), (x2, y2) = p1, p2
    if x1 > x2:
        x1, y1, x2, y2 = x2, y2, x1, y1
    dx, dy = x2 - x1, y2 - y1
    sy = -1 if dy < 0 else 1
    dy = abs(dy)
    steep = dy > dx
    major, minor = (dy, dx) if steep else (dx, dy)
    err, x, y = major - 2 * minor, x1, y1
    out = []
    for _ in range(major + 1):
        out.append((x, y))
        both = err < 0
        err += 2 * major - 2 * minor if both else -2 * minor
        if steep:
            y += sy
            x += 1 if both else 0
        else:
            x += 1
            y += sy if both else 0
    return out


def line_minor_steps(minor, major, i):
    """Minor-axis advance after i major steps of line_walk, in closed form."""
    if major == 0:
        return 0 * i
    return (2 * minor * i + major - 1) // (2 * major)


def line_pixels_in(p1, p2, rows, cols):
    """The pixels of line_walk(p1, p2) inside a rows x cols image, from the closed form over the steps whose major
    coordinate is inside (int64 arrays xs, ys)."""
    (x1, y1), (x2, y2) = p1, p2
    if x1 > x2:
        x1, y1, x2, y2 = x2, y2, x1, y1
    dx, dy = x2 - x1, y2 - y1
    sy = -1 if dy < 0 else 1
    dy = abs(dy)
    steep = dy > dx
    major, minor = (dy, dx) if steep else (dx, dy)
    if not steep:
        lo, hi = -x1, cols - 1 - x1
    elif sy > 0:
        lo, hi = -y1, rows - 1 - y1
    else:
        lo, hi = y1 - (rows - 1), y1
    lo, hi = max(lo, 0), min(hi, major)
    i = np.arange(lo, hi + 1, dtype=np.int64)
    m = line_minor_steps(minor, major, i)
    xs, ys = (x1 + m, y1 + sy * i) if steep else (x1 + i, y1 + sy * m)
    keep = (xs >= 0) & (xs < cols) & (ys >= 0) & (ys < rows)
    return xs[keep], ys[keep]


def _wrap_i32(v):
    return int(np.array([v & 0xFFFFFFFF], np.uint64).astype(np.uint32).view(np.int32)[0])


def row_col_to_rho_theta(row, col, rows, cols, rho_bin, theta_bin):
    """Solution.cpp:81-89."""
    diag = int(math.ceil(math.sqrt(rows * rows + cols * cols)))
    return _wrap_i32(int(row) * rho_bin - diag), _wrap_i32(int(col) * theta_bin - 90)


def line_endpoints(rho, theta, rows, cols):
    """drawLineParametric (Solution.cpp:91-114) up to cv::line: the two cv::Points."""
    f = np.float32
    theta_rad = f(theta) * PI_F / f(180.0)
    if theta_rad != 0:
        cs, sn = f(math.cos(float(theta_rad))), f(math.sin(float(theta_rad)))
        slope = (f(-1.0) * cs) / sn
        c = f(rho) / sn
        sx, ex = f(0), f(cols)
        sy_, ey = slope * sx + c, slope * ex + c
    else:
        cs = f(math.cos(float(theta_rad)))
        sy_, ey = f(0), f(rows)
        sx = ex = f(rho) / cs
    r = lambda v: int(np.rint(np.float64(v)))  # lrintf: half to even
    return (r(sx), r(sy_)), (r(ex), r(ey))


def draw_lines(img, peaks, rho_bin, theta_bin, color=(0, 255, 0), serial=False):
    """drawLinesParametric on the (row, col) peaks of findLocalMaxima, into a copy of img [rows, cols, 3].  Peaks with
    col * theta_bin >= 180 are not drawn (no such theta).  serial=True takes the pixels from line_walk itself."""
    out = np.array(img, np.uint8, copy=True)
    rows, cols = out.shape[:2]
    for row, col in np.asarray(peaks, np.int64).reshape(-1, 2):
        if col * theta_bin >= 180:
            continue
        rho, theta = row_col_to_rho_theta(row, col, rows, cols, rho_bin, theta_bin)
        p1, p2 = line_endpoints(rho, theta, rows, cols)
        if serial:
            for x, y in line_walk(p1, p2):
                if 0 <= x < cols and 0 <= y < rows:
                    out[y, x] = color
        else:
            xs, ys = line_pixels_in(p1, p2, rows, cols)
            out[ys, xs] = color
    return out


def circle_offsets(radius):
    """cv::circle, thickness 1: the (dx, dy) offsets of the midpoint walk, with repeats, in plot order."""
    out = []
    err, dx, dy, plus, minus = 0, radius, 0, 1, 2 * radius - 1
    while dx >= dy:
        out += [(dx, dy), (-dx, dy), (dx, -dy), (-dx, -dy), (dy, dx), (-dy, dx), (dy, -dx), (-dy, -dx)]
        dy += 1
        err += plus
        plus += 2
        mask = (1 if err <= 0 else 0) - 1
        err -= minus & mask
        dx += mask
        minus -= mask & 2
    return out


def draw_circles(img, peaks, counts, min_radius, color=(0, 255, 0)):
    """drawCircles for peaks [n_radii, K, 2] (row, col) and counts [n_radii]; radius = min_radius + index.  Centres
    beyond 65535 are not drawn (the library's limit); circles that cannot reach the image are skipped unwalked."""
    out = np.array(img, np.uint8, copy=True)
    rows, cols = out.shape[:2]
    peaks = np.asarray(peaks, np.int64)
    peaks = peaks.reshape(1, -1, 2) if peaks.ndim == 2 else peaks
    for ri in range(peaks.shape[0]):
        radius = min_radius + ri
        off = None
        for k in range(min(int(counts[ri]), peaks.shape[1])):
            cy, cx = int(peaks[ri, k, 0]), int(peaks[ri, k, 1])
            if cy > 65535 or cx > 65535:
                continue
            if radius - 1 > math.hypot(max(cx, cols - 1 - cx, 0), max(cy, rows - 1 - cy, 0)) + 1:
                continue  # farther than the farthest image pixel
            if off is None:
                off = np.array(circle_offsets(radius), np.int64)
            xs, ys = cx + off[:, 0], cy + off[:, 1]
            keep = (xs >= 0) & (xs < cols) & (ys >= 0) & (ys < rows)
            out[ys[keep], xs[keep]] = color
    return out


# ---- the radius range ------------------------------------------------------------------------------

def hough_circles_search(mask, min_radius, max_radius, num_peaks, threshold, accumulators=False):
    """Per radius: H.hough_peaks(H.hough_circles(mask, r), num_peaks, threshold)."""
    peaks, accs = [], []
    for r in range(min_radius, max_radius + 1):
        acc = H.hough_circles(mask, r)
        peaks.append(H.hough_peaks(acc, num_peaks, threshold))
        if accumulators:
            accs.append(acc)
    return (peaks, np.stack(accs) if accs else np.zeros((0,) + mask.shape, np.int32)) if accumulators else peaks


def pack_peaks(peak_lists, num_peaks):
    """Per-radius lists -> ([n_radii, num_peaks, 2] uint32 zero-padded, counts int64)."""
    out = np.zeros((len(peak_lists), num_peaks, 2), np.uint32)
    counts = np.zeros(len(peak_lists), np.int64)
    for i, p in enumerate(peak_lists):
        out[i, :len(p)] = p
        counts[i] = len(p)
    return out, counts


# ---- problems 7 and 8 (main.cpp:238-327) on a float image ---------------------------------------------

def problem7(img_f32, edge_cfg, circ_cfg):
    """edge_cfg = (gaussianSize, sigma, low, high); circ_cfg = (minRadius, maxRadius, numPeaks, threshold).
    Returns (edges, marked)."""
    eroded = erode(np.asarray(img_f32, np.float32), 5)
    edges = generate_edge_f32(eroded, *edge_cfg)
    r0, r1, k, thr = circ_cfg
    pk, cnt = pack_peaks(hough_circles_search(edges, r0, r1, k, thr), k)
    return edges, draw_circles(gray2rgb(img_f32), pk, cnt, r0)


def problem8(img_f32, edge_cfg, circ_cfg, line_cfg):
    """line_cfg = (rhoBinSize, thetaBinSize, numPeaks, threshold)."""
    edges, marked = problem7(img_f32, edge_cfg, circ_cfg)
    rb, tb, k, thr = line_cfg
    peaks = H.hough_peaks(H.hough_lines(edges, rb, tb), k, thr)
    return edges, draw_lines(marked, peaks, rb, tb)
