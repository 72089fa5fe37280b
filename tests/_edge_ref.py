"""numpy reference of ps1's edge front-end, sol::generateEdge (ps1_cpp/src/Solution.cpp:21-47: Gaussian
blur on CV_8U, then Canny with aperture 3 and the L1 norm).  No oracle code.

The blur and Canny internals are OpenCV's, which is not part of the reference; this module restates
the decisions DESIGN.md §2 and oracle/oracle.h record for them:
  * Gaussian taps (cv::getGaussianKernel, sigma > 0): exp(-(i - (n-1)/2)^2 / (2 sigma^2)) in double,
    cast to float, summed in double, scaled by 1 / sum in double, cast to float.
  * Blur: row pass then column pass, each tap acc = fmaf(x, k, acc) from +0 with the taps ascending,
    float intermediate, BORDER_REFLECT_101; round half to even, saturate to u8.
  * Canny: 3x3 Sobel with a replicated border, L1 magnitude; magnitudes outside the image are 0;
    direction by the integer tangent test (TG22 = 13573 = tan 22.5 deg in 15-bit fixed point) with
    `m > first neighbour && m >= second` along the horizontal and vertical directions and strict
    compares on both diagonal neighbours; weak = m > low, strong = m > high (floored thresholds,
    swapped if low > high).
  * Hysteresis: the pixels of every 8-connected component of (weak | strong) that holds a strong
    pixel -- computed by connected-component labelling, not by propagation.
"""
import math

import numpy as np
from scipy import ndimage


def gaussian_taps(n, sigma):
    k = [np.float32(math.exp(-0.5 / (sigma * sigma) * (i - (n - 1) * 0.5) ** 2)) for i in range(n)]
    inv = 1.0 / sum(float(t) for t in k)
    return np.array([np.float32(float(t) * inv) for t in k], np.float32)


def fmaf(x, k, acc):
    """Exact emulation of C fmaf on float32 arrays: the product of two floats is exact in float64,
    TwoSum gives the rounding error of the float64 sum, the sum is then rounded to odd (53 >= 24 + 2
    bits, so the final rounding to float32 is the single correct rounding)."""
    p = np.asarray(x, np.float32).astype(np.float64) * np.asarray(k, np.float32).astype(np.float64)
    a = np.asarray(acc, np.float32).astype(np.float64)
    p, a = np.broadcast_arrays(p, a)
    s = p + a
    z = s - p  # Knuth's TwoSum: s + e == p + a exactly
    e = (p - (s - z)) + (a - z)
    even = (s.view(np.int64) & 1) == 0
    fix = (e != 0) & even
    s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def reflect101(p, n):
    """cv::borderInterpolate(p, n, BORDER_REFLECT_101) on an index array."""
    p = np.asarray(p, np.int64)
    if n == 1:
        return np.zeros_like(p)
    period = 2 * n - 2
    p = np.abs(p) % period
    return np.where(p < n, p, period - p)


def blur(img, n, sigma, *, fused=True):
    """Gaussian blur on u8, row pass then column pass (fused=False: the unfused mutation)."""
    img = np.asarray(img, np.uint8)
    rows, cols = img.shape
    taps = gaussian_taps(n, sigma)
    a = n // 2
    mac = fmaf if fused else (lambda x, k, acc: np.float32(x) * np.float32(k) + np.float32(acc))
    src = img.astype(np.float32)
    acc = np.zeros((rows, cols), np.float32)
    xi = np.arange(cols)
    for j in range(n):
        acc = mac(src[:, reflect101(xi - a + j, cols)], taps[j], acc)
    out = np.zeros((rows, cols), np.float32)
    yi = np.arange(rows)
    for j in range(n):
        out = mac(acc[reflect101(yi - a + j, rows), :], taps[j], out)
    r = np.rint(out)  # half to even
    return np.clip(r, 0, 255).astype(np.uint8)


def gradients(img):
    """3x3 Sobel, replicated border: (gx, gy, L1 magnitude) int64."""
    p = np.pad(np.asarray(img, np.int64), 1, mode="edge")
    r0, r1, r2 = p[:-2], p[1:-1], p[2:]
    gx = (r0[:, 2:] + 2 * r1[:, 2:] + r2[:, 2:]) - (r0[:, :-2] + 2 * r1[:, :-2] + r2[:, :-2])
    gy = (r2[:, :-2] + 2 * r2[:, 1:-1] + r2[:, 2:]) - (r0[:, :-2] + 2 * r0[:, 1:-1] + r0[:, 2:])
    return gx, gy, np.abs(gx) + np.abs(gy)


def suppress(img, low, high, *, symmetric=False, ge_thresholds=False):
    """Non-maximum suppression and the double threshold: (weak, strong) bool planes.
    symmetric: the mutation with `>` on both sides; ge_thresholds: `>=` thresholds."""
    if low > high:
        low, high = high, low
    low, high = math.floor(low), math.floor(high)
    gx, gy, m = gradients(img)
    M = np.pad(m, 1)  # magnitudes outside the image count as 0
    c = M[1:-1, 1:-1]

    def at(dy, dx):
        return M[1 + dy:M.shape[0] - 1 + dy, 1 + dx:M.shape[1] - 1 + dx]

    ax, ay = np.abs(gx), np.abs(gy) << 15
    tg22x = ax * 13573
    tg67x = tg22x + (ax << 16)
    sgn = np.where((gx ^ gy) < 0, -1, 1)
    second = (lambda v, w: v > w) if symmetric else (lambda v, w: v >= w)
    horiz = (c > at(0, -1)) & second(c, at(0, 1))
    vert = (c > at(-1, 0)) & second(c, at(1, 0))
    diag_p = (c > at(-1, -1)) & (c > at(1, 1))   # sgn = +1: up-left and down-right
    diag_n = (c > at(-1, 1)) & (c > at(1, -1))   # sgn = -1: up-right and down-left
    is_max = np.where(ay < tg22x, horiz, np.where(ay > tg67x, vert, np.where(sgn > 0, diag_p, diag_n)))
    above = (lambda v, t: v >= t) if ge_thresholds else (lambda v, t: v > t)
    cand = above(c, low) & is_max
    strong = cand & above(c, high)
    return cand & ~strong, strong


def hysteresis(weak, strong, *, connectivity=8):
    """Every component of weak | strong (8-connected; 4 for the mutation) that holds a strong pixel."""
    structure = np.ones((3, 3), bool) if connectivity == 8 else ndimage.generate_binary_structure(2, 1)
    lab, n = ndimage.label(weak | strong, structure=structure)
    keep = np.zeros(n + 1, bool)
    keep[np.unique(lab[strong])] = True
    keep[0] = False
    return keep[lab]


def generate_edge(img, gauss_size, sigma, low, high, *, fused=True, connectivity=8, **nms):
    """sol::generateEdge: 255 / 0 edge mask.  A 1-tap Gaussian is the identity (its tap is 1.0)."""
    b = blur(img, gauss_size, sigma, fused=fused)
    weak, strong = suppress(b, low, high, **nms)
    return np.where(hysteresis(weak, strong, connectivity=connectivity), 255, 0).astype(np.uint8)
