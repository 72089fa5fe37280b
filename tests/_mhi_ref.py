"""numpy / scipy.ndimage reference of the ps7 motion-history path: mhi::frameDifference,
thresholdDifference, mhi::calcMotionHistory, mhi::energyFromHistory and mhiHelper's loop.  No oracle code and no
library code: written from

  * ps7_cpp/lib/MotionHistory.cpp:26-112 (frameDifference, calcMotionHistory, both energyFromHistory overloads),
  * ps7_cpp/lib/MotionHistory.cu:16-66 (AbsThreshold, motionHistoryKernel),
  * ps7_cpp/src/Solution.cpp:16-101 (mhiHelper's loop, for `history_seq`),
  * the declarations in include/mi_cv.h and the decisions about OpenCV in oracle/oracle.h and DESIGN.md section 2,

with `fmaf`, `reflect101` and `gaussian_taps` from tests/_edge_ref.py.

What the reference says and what it leaves open.  The reference sources say everything about
  * the order of the steps (MotionHistory.cpp:50-73): blur f1, blur f2, `subtract(f2Blur, f1Blur)`, threshold, MORPH_OPEN
    with `getStructuringElement(MORPH_ELLIPSE, Size(7, 7))`; `blurSize` is a cv::Size, so (width, height);
  * AbsThreshold (MotionHistory.cu:22-24): `val >= t || -val >= t` on a `uint8_t val` and a `double t`.  `-val`
    promotes to int, so it is the negative number (never 256 - val), and both comparisons are made in double: 1.7 keeps
    2 and drops 1; any t <= 0 keeps everything (val = 0 gives -0 >= t); a NaN keeps nothing;
  * motionHistoryKernel (MotionHistory.cu:63-65): `mask == 1 ? tau : max(h - 1, 0)` assigned to a `uint8_t`, so tau is
    stored modulo 256 (300 -> 44), a mask value of 2 or 255 is "no motion", and 0 stays 0;
  * energyFromHistory (MotionHistory.cpp:103-104): `pixel > 0 ? 1 : 0`.
Decisions of this repository, because the reference leaves them to OpenCV's CUDA modules (which are not in its tree):
  * the Gaussian filter's arithmetic: `getGaussianKernel` taps in double -> float, row pass (width taps along x) then
    column pass (height taps along y), every tap `acc = fmaf(x, k, acc)` from +0 with the taps ascending, a float
    intermediate, BORDER_REFLECT_101, then round half to even and saturate to u8.  A 1-tap pass has the single tap 1.0;
  * `cv::cuda::subtract` on CV_8U saturates: max(f2 - f1, 0);
  * `cv::cuda` morphology pads EVERY pass with BORDER_REFLECT_101: the erosion reads the reflected mask, the dilation
    reads the reflected eroded mask;
  * the structuring element: `cv::getStructuringElement`'s definition, restated in `ellipse` -- with r = height / 2 and
    c = width / 2, row i holds the columns c - dx .. c + dx, dx = round-half-even(c * sqrt((r^2 - dy^2) / r^2)),
    dy = i - r.  For 7 x 7 that is half-widths 0, 2, 3, 3, 3, 2, 0 (tests/test_mhi_ref.py).

Reflect-101 padding of the morphology equals ignoring the outside.  Let S be the element as a set of offsets (dy, dx)
and w(|dy|) its row half-width: S = {|dx| <= w(|dy|)} with w non-increasing (3, 3, 2, 0), so S is closed under shrinking
either |dy| or |dx|.  Take a pixel p = (y, x) of the image and a tap whose column x + dx lies outside, say x + dx < 0.
One reflection sends it to column -(x + dx) = x + dx' with dx' = -dx - 2x.  From 0 <= x < -dx follows dx < dx' <= -dx,
so |dx'| <= |dx|.  A reflection about the last column is the mirror image, and each further reflection of an index that
is still outside shrinks the distance to x again (the mirror lies between x and the index), so any number of
reflections ends at a column x + dx'' inside the image with |dx''| <= |dx|.  The same holds for rows.  Hence the
reflected tap reads pixel p + (dy'', dx'') with |dy''| <= |dy| and |dx''| <= |dx| <= w(|dy|) <= w(|dy''|): an offset
of S whose pixel lies inside the image, which the minimum (maximum) already covers.  So the set of values is that of
the element cut at the border, and a "neutral padding" (+inf for erode, 0 for dilate) mutation would be no mutation --
as "cut, not clamped" is none in tests/_ps4_feat_ref.py.  The padding mutation here is therefore `erode_pad_zero`.

The lemma mhi.hip's open kernel relies on: the mask extended by reflection is even about column 0 and about column
n - 1 (period 2n - 2; constant for n = 1); an erosion by an element symmetric in that axis commutes with both mirrors;
so the erosion of the extension has the same symmetries, i.e. it is the reflected extension of its own restriction to
the image, and that restriction is the erosion with reflect-101 padding.  `erode_of_extension` computes the left side
for tests/test_mhi_ref.py, which checks the statement down to 1 x N and 2 x 2 where the reflection wraps repeatedly.

`round_half_away` needs exact .5 ties in the float result of the blur, which random frames do not hold.  For the
3 x 1 blur there are none: `find_ties3` runs through all 2^24 u8 triples (a, b, c) for a sigma and finds no result on an
integer + .5 for sigma 0.8, 1, 1.5, 2 or 10 -- with symmetric taps the exact value is (a + c) t0 + b t1, some 1.3e5
distinct numbers and not 1.7e7, against a chance of about 2^-17 each.  The 5 x 1 blur has three independent sums: of
2^24 random 5-tuples at sigma 1.5, 204 end exactly on .5 (1.2e-5), 99 of them above an even integer, where half-to-even
and half-away differ.  TIE_TUPLES lists six of those whose neighbouring windows, in a row of zeros, stay at or below the
tie's integer; `tie_pair` plants one in a one-row image so that the tie decides one pixel of the mask
(tests/test_mhi_ref.py re-derives that each is an exact tie and that the mutation shows).

`blur_unfused` is as rare in random frames: the unfused chain differs from the fmaf chain by an ulp or two of the float,
which moves the u8 only when the result lies within 1e-5 of an integer + .5.  Of 2^24 random 5-tuples (5 x 1, sigma
1.5), 60 round differently; FMA_TUPLES lists six that `tie_pair` can plant the same way (x is the smaller of the two
roundings; for the last two the fmaf chain gives x + 1, so the reference itself has the hole).

Every function takes `mut`, a collection of mutation names (MUTATIONS); tests/test_mhi_ref.py shows that each one
changes a named result on an input that tests/test_mhi_paths_gpu.py uses.

Speed (numpy on one core of a server CPU, printed by tests/test_mhi_ref.py, never asserted): the 31 x 31 blur pair
and open at 213 x 200 take about 0.05 s.
"""
import math

import numpy as np
from scipy import ndimage

from _edge_ref import fmaf as _fmaf_twosum
from _edge_ref import gaussian_taps, reflect101

MUTATIONS = frozenset({
    "blur_wh_swapped", "blur_unfused", "round_half_away",
    "sub_reversed", "sub_abs",
    "thr_gt", "thr_truncated", "thr_neg_u8",
    "se_rect", "se_rows_wide", "erode_pad_zero", "close_not_open", "erode_only",
    "update_mask_nonzero", "update_tau_saturates", "update_no_floor"})

# (five pixels, x): the 5 x 1 blur with sigma 1.5 of the row [0.., a, b, c, d, e, 0..] is exactly x + .5 at c's column, x even
TIE_BLUR, TIE_SIGMA = (5, 1), 1.5
TIE_TUPLES = (((141, 47, 28, 152, 107), 84), ((248, 135, 236, 247, 87), 198), ((244, 55, 206, 60, 201), 140),
              ((11, 236, 196, 66, 244), 158), ((157, 209, 96, 126, 227), 152), ((138, 226, 89, 249, 7), 154))
FMA_TUPLES = (((172, 148, 185, 132, 61), 147), ((128, 217, 191, 75, 117), 153), ((89, 186, 51, 59, 205), 107),
              ((213, 164, 103, 132, 130), 140), ((155, 116, 154, 229, 235), 172), ((109, 244, 233, 132, 220), 195))


def _check(mut):
    bad = set(mut) - MUTATIONS
    if bad:
        raise ValueError(f"unknown mutations {sorted(bad)}")
    return frozenset(mut)


def fmaf(x, k, acc):
    """C fmaf on float32 arrays whose results are normal floats (here: within 0 .. 255).  The product of two floats is
    exact in double; s = the double nearest to product + acc.  Rounding s to float gives the correctly rounded fmaf
    unless s is exactly halfway between two floats: a float midpoint is itself a double, so the exact sum and s lie on
    the same side of every midpoint that s is not equal to.  Where some s is a midpoint (29 low mantissa bits of
    1 0000...), the exact TwoSum emulation of tests/_edge_ref.py decides; it is some five times slower, and
    tests/test_mhi_ref.py holds the two to the same bits."""
    s = np.asarray(x, np.float32).astype(np.float64) * np.asarray(k, np.float32).astype(np.float64) \
        + np.asarray(acc, np.float32).astype(np.float64)
    if ((s.view(np.int64) & 0x1FFFFFFF) == 0x10000000).any():
        return _fmaf_twosum(x, k, acc)
    return s.astype(np.float32)


def _wh(ksize):
    """cv::Size(width, height); a bare int is a square."""
    if isinstance(ksize, (tuple, list)):
        w, h = ksize
        return int(w), int(h)
    return int(ksize), int(ksize)


def ellipse(width=7, height=7, mut=()):
    """cv::getStructuringElement(MORPH_ELLIPSE, Size(width, height)) from its definition -> bool [height, width]."""
    mut = _check(mut)
    r, c = height // 2, width // 2
    inv_r2 = 1.0 / (r * r) if r else 0.0
    se = np.zeros((height, width), bool)
    for i in range(height):
        dy = i - r
        dx = round(c * math.sqrt((r * r - dy * dy) * inv_r2))  # cvRound: half to even
        se[i, max(c - dx, 0):min(c + dx + 1, width)] = True
    if "se_rect" in mut:
        se[...] = True
    if "se_rows_wide" in mut:  # rows 1 and 5 as wide as row 2
        se[1], se[height - 2] = se[2], se[2]
    return se


def blur_float(img, ksize, sigma, mut=()):
    """The separable Gaussian before rounding: float32 [..., rows, cols] (leading axes are a stack of images)."""
    mut = _check(mut)
    img = np.asarray(img, np.uint8)
    rows, cols = img.shape[-2:]
    w, h = _wh(ksize)
    if "blur_wh_swapped" in mut:
        w, h = h, w
    mac = (lambda x, k, acc: np.float32(x) * np.float32(k) + np.float32(acc)) if "blur_unfused" in mut else fmaf
    tx, ty = gaussian_taps(w, sigma), gaussian_taps(h, sigma)
    src = img.astype(np.float32)
    acc = np.zeros(img.shape, np.float32)
    xi = np.arange(cols)
    for j in range(w):
        acc = mac(src[..., reflect101(xi - w // 2 + j, cols)], tx[j], acc)
    out = np.zeros(img.shape, np.float32)
    yi = np.arange(rows)
    for j in range(h):
        out = mac(acc[..., reflect101(yi - h // 2 + j, rows), :], ty[j], out)
    return out


def blur(img, ksize, sigma, mut=()):
    """cv::cuda::createGaussianFilter(CV_8UC1, -1, ksize, sigma): u8 -> u8."""
    v = blur_float(img, ksize, sigma, mut).astype(np.float64)
    r = np.floor(v + 0.5) if "round_half_away" in mut else np.rint(v)  # (v >= 0; v + 0.5 is exact in double)
    return np.clip(r, 0, 255).astype(np.uint8)


def subtract(f2, f1, mut=()):
    """cv::cuda::subtract(f2, f1) on CV_8U."""
    mut = _check(mut)
    d = np.asarray(f2, np.uint8).astype(np.int64) - np.asarray(f1, np.uint8).astype(np.int64)
    if "sub_reversed" in mut:
        d = -d
    if "sub_abs" in mut:
        d = np.abs(d)
    return np.clip(d, 0, 255).astype(np.uint8)


def threshold(src, thresh, mut=()):
    """thresholdDifference / AbsThreshold<uint8_t> (MotionHistory.cu:17-48) -> {0, 1} uint8."""
    mut = _check(mut)
    val = np.asarray(src, np.uint8).astype(np.int64)
    t = float(thresh)
    if "thr_truncated" in mut and not math.isnan(t):
        t = float(int(t))
    neg = (256 - val) % 256 if "thr_neg_u8" in mut else -val
    cmp = np.greater if "thr_gt" in mut else np.greater_equal
    return (cmp(val.astype(np.float64), t) | cmp(neg.astype(np.float64), t)).astype(np.uint8)


def _extend(mask, pad, zero=False):
    rows, cols = mask.shape
    if zero:
        return np.pad(mask, pad)
    return mask[reflect101(np.arange(-pad, rows + pad), rows)][:, reflect101(np.arange(-pad, cols + pad), cols)]


def _morph(mask, se, dilate, pad_zero=False):
    """One pass of cv::cuda morphology: its own padded copy, the element anchored at its centre."""
    ry, rx = se.shape[0] // 2, se.shape[1] // 2
    ext = _extend(mask, max(ry, rx), pad_zero)
    f = ndimage.maximum_filter if dilate else ndimage.minimum_filter
    full = f(ext, footprint=se, mode="constant", cval=0)
    p = max(ry, rx)
    return full[p:p + mask.shape[0], p:p + mask.shape[1]]


def erode(mask, mut=()):
    mut = _check(mut)
    return _morph(np.asarray(mask, np.uint8), ellipse(mut=mut), False, "erode_pad_zero" in mut)


def dilate(mask, mut=()):
    return _morph(np.asarray(mask, np.uint8), ellipse(mut=_check(mut)), True)


def erode_of_extension(mask, mut=()):
    """The erosion of the mask's 6-pixel reflect-101 extension, where it is defined without any padding: the
    3-pixel extension's area ([rows + 6, cols + 6])."""
    ext = _extend(np.asarray(mask, np.uint8), 6)
    full = ndimage.minimum_filter(ext, footprint=ellipse(mut=_check(mut)), mode="constant", cval=0)
    return full[3:-3, 3:-3]


def extension(mask, pad):
    return _extend(np.asarray(mask, np.uint8), pad)


def morph_open(mask, mut=()):
    """MORPH_OPEN with the 7 x 7 ellipse: erode, then dilate."""
    mut = _check(mut)
    if "erode_only" in mut:
        return erode(mask, mut)
    if "close_not_open" in mut:
        return erode(dilate(mask, mut), mut)
    return dilate(erode(mask, mut), mut)


def difference_of_blurred(b1, b2, thresh, mut=()):
    """MotionHistory.cpp:56-73 on the two blurred frames: subtract, threshold, open."""
    mut = _check(mut)
    return morph_open(threshold(subtract(b2, b1, mut), thresh, mut), mut)


def frame_difference(f1, f2, thresh, ksize=3, sigma=1.0, mut=()):
    """mhi::frameDifference (MotionHistory.cpp:26-77) on single-channel u8 frames -> {0, 1} uint8."""
    mut = _check(mut)
    return difference_of_blurred(blur(f1, ksize, sigma, mut), blur(f2, ksize, sigma, mut), thresh, mut)


def update(history, mask, tau, mut=()):
    """mhi::calcMotionHistory -> motionHistoryKernel (MotionHistory.cu:52-66): a new array."""
    mut = _check(mut)
    h = np.asarray(history, np.uint8).astype(np.int64)
    m = np.asarray(mask, np.uint8)
    moving = (m != 0) if "update_mask_nonzero" in mut else (m == 1)
    t = min(int(tau), 255) if "update_tau_saturates" in mut else int(tau) & 0xFF
    decay = ((h - 1) & 0xFF) if "update_no_floor" in mut else np.maximum(h - 1, 0)
    return np.where(moving, t, decay).astype(np.uint8)


def energy(mhi):
    """mhi::energyFromHistory (MotionHistory.cpp:98-105)."""
    return (np.asarray(mhi, np.uint8) > 0).astype(np.uint8)


def history_seq(frames, thresh, ksize, sigma, tau, save, mut=()):
    """mhiHelper's loop (Solution.cpp:16-101): the history, from zero, after update j = frameDifference(frame j - 1,
    frame j) then calcMotionHistory, for every j in save (in save's order, repeats allowed)."""
    mut = _check(mut)
    frames = np.asarray(frames, np.uint8)
    blurred = blur(frames[:max(save) + 1], ksize, sigma, mut)  # every frame once: the blur of a frame is the same
    hist = np.zeros(frames.shape[1:], np.uint8)                # as f2 of one difference and as f1 of the next
    want = {}
    for f in range(1, max(save) + 1):
        hist = update(hist, difference_of_blurred(blurred[f - 1], blurred[f], thresh, mut), tau, mut)
        if f in save:
            want[f] = hist
    return np.stack([want[j] for j in save])


def tie_pair(tup, x, cols=21):
    """(f1, f2, thresh) of one row: f1 holds the tuple in zeros, f2 is 255, thresh = 255 - x, for TIE_BLUR and
    TIE_SIGMA.  A pixel is set where the blur of f1 is at most x.  For a TIE_TUPLES entry that blur is x + .5 at the
    tuple's centre (column cols // 2) and at most x elsewhere, so half-to-even gives an all-ones mask and half-away a
    hole at the centre, which the open keeps; for an FMA_TUPLES entry the centre rounds to x or x + 1 with the chain."""
    f1 = np.zeros((1, cols), np.uint8)
    f1[0, cols // 2 - 2:cols // 2 + 3] = tup
    return f1, np.full((1, cols), 255, np.uint8), 255 - x


def find_ties3(sigma=1.0):
    """Every u8 triple whose 3 x 1 blur is exactly an integer + .5 -> int array [n, 4]: a, b, c, floor(result)."""
    t = gaussian_taps(3, sigma)
    b, c = np.meshgrid(np.arange(256, dtype=np.float32), np.arange(256, dtype=np.float32), indexing="ij")
    out = []
    for a in range(256):
        v = fmaf(c, t[2], fmaf(b, t[1], fmaf(np.float32(a), t[0], np.float32(0)))).astype(np.float64)
        bi, ci = np.nonzero(v - np.floor(v) == 0.5)
        out += [(a, int(i), int(j), int(v[i, j])) for i, j in zip(bi, ci)]
    return np.array(out, np.int64).reshape(-1, 4)


def find_ties5(n, seed, sigma=TIE_SIGMA):
    """Of n random u8 5-tuples, those whose 5 x 1 blur is exactly an integer + .5 -> int array [m, 6]: the tuple and
    floor(result)."""
    t = gaussian_taps(5, sigma)
    q = np.random.default_rng(seed).integers(0, 256, (n, 5)).astype(np.float32)
    acc = np.zeros(n, np.float32)
    for k in range(5):
        acc = fmaf(q[:, k], t[k], acc)
    v = acc.astype(np.float64)
    i = np.nonzero(v - np.floor(v) == 0.5)[0]
    return np.concatenate([q[i], v[i, None]], axis=1).astype(np.int64)
