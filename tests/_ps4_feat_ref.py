"""numpy reference of the ps4 feature chain: Solution::harrisHelper's last step and Solution::siftHelper
(ps4_cpp/src/Solution.cpp:77-184) -- harris::refineCorners, sift::getKeypoints, the SIFT-style descriptor window,
knnMatch(k = 2) and the ratio test.  No oracle code and no library code: written from

  * ps4_cpp/lib/Harris.cpp:99-147 and Harris.cu:173-329 (refineCorners, both namespaces),
  * ps4_cpp/lib/Descriptors.cpp (PI at :5, getKeypoints at :27-47),
  * ps4_cpp/src/Solution.cpp:141-184 (the call sites: size 10, knnMatch(.., 2), `d0 < 0.75 * d1`),
  * DESIGN.md section 2 ("ps4 feature chain": the descriptor contract and the matcher's decisions),
  * the declarations in include/mi_cv.h,

with `fmaf` and `reflect101` from tests/_edge_ref.py.

How independent this is.  refineCorners, getKeypoints and the matcher are restated from the reference sources, which
say everything.  The descriptor is different: OpenCV's SIFT is not in the reference tree, its arithmetic is a decision
of this repository, and the DESIGN.md section that states it was written down together with this module, from the same
knowledge of the kernel.  So the descriptor's order of operations, its validity test, its angle reduction and its
variable names (calcSIFTDescriptor's) follow the contract step by step, as oracle_sift.c does; a step that the
contract itself gets wrong would be wrong here too.  What stands as an independent witness for the descriptor is
  * the polynomial coefficients, which are copied from nowhere: 1/n! (sine, cosine) and (ln 2)^n / n! (2^f) are
    computed here and rounded to float, beside cv::fastAtan2's four published constants;
  * numpy's vectorised evaluation of every sample of the square, which shares no control flow with the kernel (no
    blocks, no pruning, no atomics);
  * `descriptors_ideal`, the published algorithm in float64 with libm, to which the contract is held within one count;
  * the hand-worked answers and the rotation and shift properties of tests/test_ps4_feat_ref.py.

refineCorners.  `refine_corners_seq` is Harris.cpp:116-144 as written: raster scan, `double(R) >= threshold`, the
(2d+1)^2 window with CLAMPED coordinates in which the pixel itself is skipped, `R <= neighbour` rejecting (so a tie
kills both and a NaN neighbour rejects nothing), and `x += minDistance - 1` after a kept corner.  With minDistance 0
that statement is `x += -1` in front of the loop's `x++`: the reference never leaves its first corner.  The contract
(and this function) keeps every pixel that passes the threshold for d = 0 and goes on.  `refine_corners` is the
vectorised form without the skip; the two are equal because a strict maximum of a (2d+1)^2 window excludes any other
within d columns of its row (tests/test_ps4_feat_ref.py proves both statements).  A clamped window holds exactly the
pixels of the window cut at the border (a clamped coordinate pair is a pixel of the cut window, or the centre, which
is skipped), so "cut, not clamped" is no mutation at all; `nms_unclamped` therefore reads 0 outside the image, which is
what an unclamped read of a zero-padded plane gives.

Harris.cu differs from Harris.cpp in two ways.  (1) A thread owns NMS_COLS_PER_THREAD = 32 columns and its `idx +=
minDistance - 1` cannot leave them; since the skip never removes a corner this changes nothing.  (2) Its list comes
from `copy_if(.. > 0.f)` over the sparse map (:301-306), so with a threshold <= 0 kept corners whose value is <= 0
(or -0) are in the map and not in the list.  The library follows Harris.cpp: the list holds every kept pixel, in
row-major order, whatever its value; the map holds the values (a kept -0 is stored as -0, a kept 0 is
indistinguishable from "no corner" in the map alone).

Every function takes `mut`, a collection of mutation names (MUTATIONS); tests/test_ps4_feat_ref.py shows that each one
changes a named result.

Speed (numpy held to one core of a server CPU; `python tests/test_ps4_feat_ref.py speed` prints both; nothing
asserts them): descriptors of 300 size-10 keypoints (107 x 107 windows) on a 240 x 320 scene 1.1 s; knn2 of
64 x 3000 x 128: 1.2 s.  On the same core the 6147 small keypoints of tests/test_ps4_feat_paths_gpu.py take 12 s, its
300 sampled queries against 8192 train rows 30 s and its 4200 x 1100 job 32 s; an MI355X machine's host CPU with 16 threads
is several times faster (5 s and 10 s for the last two, that module's docstring).
"""
import math

import numpy as np

from _edge_ref import fmaf as _fmaf_finite
from _edge_ref import reflect101

F = np.float32
MUTATIONS = frozenset({
    "nms_ge", "nms_float_threshold", "nms_unclamped", "list_column_major",
    "kp_true_pi", "kp_xy_swapped",
    "desc_dy_sign", "desc_angle_sign", "desc_bin_width", "desc_no_wrap", "desc_no_clamp", "desc_round_half_away",
    "desc_border_inclusive", "desc_taylor_short",
    "knn_tie_high_index", "knn_reverse_dims", "ratio_le", "ratio_float"})

PI_REF = F(3.1415921636)  # Descriptors.cpp:5
# the one tolerance, atan2f within 1e-5 rad, carried through `* 180.f / PI`
ANGLE_TOL_DEG = float(F(1e-5)) * 180.0 / float(PI_REF)


def _check(mut):
    bad = set(mut) - MUTATIONS
    if bad:
        raise ValueError(f"unknown mutations {sorted(bad)}")
    return frozenset(mut)


def fmaf(x, k, acc):
    """C fmaf on float32 arrays (tests/_edge_ref.py), with IEEE results where an operand or the exact result is not
    finite (the emulation's error term is undefined there)."""
    with np.errstate(invalid="ignore", over="ignore"):
        r = _fmaf_finite(x, k, acc)
        plain = (np.asarray(x, F).astype(np.float64) * np.asarray(k, F).astype(np.float64)
                 + np.asarray(acc, F).astype(np.float64))
        return np.where(np.isfinite(plain), r, plain.astype(F)).astype(F)


def sobel3(img):
    """harris::getGradients with a 3x3 Sobel, scale 1 (separable filters): row pass then column
    pass, every tap `acc = fmaf(x, k, acc)` from +0, BORDER_REFLECT_101.  -> (gx, gy)."""
    img = np.asarray(img, F)
    rows, cols = img.shape
    xi, yi = np.arange(cols), np.arange(rows)

    def sep(krow, kcol):
        acc = np.zeros((rows, cols), F)
        for j in range(3):
            acc = fmaf(img[:, reflect101(xi - 1 + j, cols)], F(krow[j]), acc)
        out = np.zeros((rows, cols), F)
        for j in range(3):
            out = fmaf(acc[reflect101(yi - 1 + j, rows), :], F(kcol[j]), out)
        return out
    return sep((-1, 0, 1), (1, 2, 1)), sep((1, 2, 1), (-1, 0, 1))


# ------------------------------------------------------------------------------- refineCorners

def _passes(v, threshold, mut):
    if "nms_float_threshold" in mut:
        with np.errstate(over="ignore"):
            return bool(F(v) >= F(threshold))
    return bool(float(v) >= float(threshold))  # Harris.cpp:119: float against `const double`


def refine_corners_seq(R, threshold, min_distance, mut=()):
    """Harris.cpp:116-144 as written (see the module docstring for minDistance 0).  -> (sparse map, [(y, x)])."""
    mut = _check(mut)
    R = np.asarray(R, F)
    rows, cols = R.shape
    d = int(min_distance)
    corners = np.zeros((rows, cols), F)
    locs = []
    for y in range(rows):
        x = 0
        while x < cols:
            v = R[y, x]
            if _passes(v, threshold, mut):
                is_max = True
                for wy in range(-d, d + 1):
                    for wx in range(-d, d + 1):
                        if "nms_unclamped" in mut:
                            cy, cx = y + wy, x + wx
                            if cy == y and cx == x:
                                continue
                            nb = R[cy, cx] if 0 <= cy < rows and 0 <= cx < cols else F(0)
                        else:
                            cy, cx = min(max(0, y + wy), rows - 1), min(max(0, x + wx), cols - 1)
                            if cy == y and cx == x:
                                continue
                            nb = R[cy, cx]
                        if (v < nb) if "nms_ge" in mut else (v <= nb):
                            is_max = False
                            break
                    if not is_max:
                        break
                if is_max:
                    corners[y, x] = v
                    locs.append((y, x))
                    if d >= 1:
                        x += d - 1
            x += 1
    locs = np.array(locs, np.int32).reshape(-1, 2)
    if "list_column_major" in mut:
        locs = locs[np.lexsort((locs[:, 0], locs[:, 1]))]
    return corners, locs


def refine_corners(R, threshold, min_distance, mut=()):
    """The same result without the skip, one array operation per window offset."""
    mut = _check(mut)
    R = np.asarray(R, F)
    rows, cols = R.shape
    d = int(min_distance)
    if "nms_float_threshold" in mut:
        with np.errstate(over="ignore"):
            keep = R >= F(threshold)
    else:
        keep = R.astype(np.float64) >= float(threshold)
    yy, xx = np.arange(rows), np.arange(cols)
    if "nms_unclamped" in mut:
        P = np.zeros((rows + 2 * d, cols + 2 * d), F)
        P[d:d + rows, d:d + cols] = R
    for wy in range(-d, d + 1):
        for wx in range(-d, d + 1):
            if "nms_unclamped" in mut:
                if wy == 0 and wx == 0:
                    continue
                nb = P[d + wy:d + wy + rows, d + wx:d + wx + cols]
                other = True
            else:
                cy, cx = np.clip(yy + wy, 0, rows - 1), np.clip(xx + wx, 0, cols - 1)
                other = (cy != yy)[:, None] | (cx != xx)[None, :]
                nb = R[np.ix_(cy, cx)]
            rej = (R < nb) if "nms_ge" in mut else (R <= nb)
            keep &= ~(rej & other)
    corners = np.where(keep, R, F(0)).astype(F)
    ys, xs = np.nonzero(keep)
    locs = np.stack([ys, xs], 1).astype(np.int32)
    if "list_column_major" in mut:
        locs = locs[np.lexsort((locs[:, 0], locs[:, 1]))]
    return corners, locs


# ------------------------------------------------------------------------------- getKeypoints

def keypoints(gx, gy, locs, size, mut=()):
    """sift::getKeypoints, Descriptors.cpp:39-46 -> [n, 4] float32 (x, y, size, angle in degrees).  atan2 in float64,
    rounded to float (std::atan2(float, float)); `* 180.f / PI` are two float operations with the reference's PI."""
    mut = _check(mut)
    gx, gy = np.asarray(gx, F), np.asarray(gy, F)
    locs = np.asarray(locs, np.int64).reshape(-1, 2)
    ix, iy = gx[locs[:, 0], locs[:, 1]], gy[locs[:, 0], locs[:, 1]]
    a = np.arctan2(iy.astype(np.float64), ix.astype(np.float64)).astype(F)
    pi = F(math.pi) if "kp_true_pi" in mut else PI_REF
    with np.errstate(invalid="ignore"):
        ang = ((a * F(180)).astype(F) / pi).astype(F)
    kp = np.empty((len(locs), 4), F)
    kp[:, 0] = locs[:, 0 if "kp_xy_swapped" in mut else 1]  # cv::KeyPoint(corner.second, corner.first, ..)
    kp[:, 1] = locs[:, 1 if "kp_xy_swapped" in mut else 0]
    kp[:, 2] = F(size)
    kp[:, 3] = ang
    return kp


def angles_close(a, b):
    """Keypoint angles within the atan2f tolerance, compared on the circle (-180 and 180 are one direction)."""
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)) % 360.0
    return np.minimum(d, 360.0 - d) <= ANGLE_TOL_DEG


# ------------------------------------------------------------------------------- the descriptor window

SD, SN = 4, 8


def _coef(vals):
    return [F(v) for v in vals]


_SIN = _coef([(-1.0) ** k / math.factorial(2 * k + 1) for k in range(5, -1, -1)])   # y^11 .. y^1
_COS = _coef([(-1.0) ** k / math.factorial(2 * k) for k in range(6, -1, -1)])       # y^12 .. y^0
_EXP2 = _coef([math.log(2.0) ** n / math.factorial(n) for n in range(7, -1, -1)])   # f^7 .. f^0
_DEG = F(57.29577951308232)  # (float)(180 / CV_PI)
_AT = [F(F(c) * _DEG) for c in (0.9997878412794807, -0.3258083974640975, 0.1555786518463281, -0.04432655554792128)]


def _horner_fma(coefs, x):
    p = np.full(np.shape(x), coefs[0], F)
    for c in coefs[1:]:
        p = fmaf(p, x, c)
    return p


def sincos_deg(deg, mut=()):
    """sin and cos of a float angle in degrees: the turn fraction `t = deg / 360 - floor(..)`, quadrant `q = int(4 t)`,
    `y = (4 t - q) * (float)(pi / 2)`, Taylor polynomials in y^2 as fmaf chains (sine to y^11, times y; cosine to
    y^12), then the quadrant's signs and swap."""
    t = F(deg) / F(360)
    t = F(t - np.floor(t))
    x = F(t * F(4))
    q = int(x)
    f = F(x - F(q))
    q &= 3
    y = F(f * F(math.pi / 2))
    y2 = F(y * y)
    sy = F(_horner_fma(_SIN[1:] if "desc_taylor_short" in mut else _SIN, y2) * y)
    pc = F(_horner_fma(_COS, y2))
    return [(sy, pc), (pc, -sy), (-sy, -pc), (-pc, sy)][q]


def exp_neg(w):
    """exp(w) for w <= 0: 0 below -80; else `t = w * (float)log2(e)`, `k = rint(t)`, 2^k times the degree-7 Taylor
    polynomial of 2^f in `f = t - k` (an fmaf chain)."""
    w = np.asarray(w, F)
    with np.errstate(invalid="ignore", over="ignore"):
        t = (w * F(1.0 / math.log(2.0))).astype(F)
        k = np.rint(t)
        f = (t - k).astype(F)
        p = _horner_fma(_EXP2, f)
        kk = np.where(np.isfinite(k), k, 0).astype(np.int32)
        r = np.ldexp(p, kk).astype(F)
        return np.where(w < F(-80), F(0), r).astype(F)


def fast_atan2_deg(y, x):
    """cv::fastAtan2's polynomial in degrees, [0, 360): unfused float arithmetic."""
    y, x = np.asarray(y, F), np.asarray(x, F)
    with np.errstate(invalid="ignore", over="ignore"):
        ax, ay = np.abs(x), np.abs(y)
        flat = ax >= ay
        num, den = np.where(flat, ay, ax), np.where(flat, ax, ay)
        c = (num / (den + F(np.finfo(np.float64).eps)).astype(F)).astype(F)
        c2 = (c * c).astype(F)
        p = (_AT[3] * c2 + _AT[2]).astype(F)
        p = (p * c2 + _AT[1]).astype(F)
        p = (p * c2 + _AT[0]).astype(F)
        p = (p * c).astype(F)
        a = np.where(flat, p, (F(90) - p).astype(F))
        a = np.where(x < 0, (F(180) - a).astype(F), a)
        a = np.where(y < 0, (F(360) - a).astype(F), a)
        return a.astype(F)


def _geometry(kp, rows, cols, mut):
    x, y, size, angle = (F(v) for v in kp)
    valid = bool(size > 0 and np.isfinite(size) and np.isfinite(x) and np.isfinite(y) and np.isfinite(angle)
                 and abs(x) < F(1e9) and abs(y) < F(1e9))
    if not valid:
        return None
    px, py = int(np.rint(x)), int(np.rint(y))  # lrintf: half to even
    ori = F(angle) if "desc_angle_sign" in mut else F(F(360) - angle)
    ori = F(ori - F(F(360) * np.floor(F(ori / F(360)))))
    if not ori < F(360):
        ori = F(0)
    hw = F(F(3) * size) if "desc_bin_width" in mut else F(F(3) * F(size * F(0.5)))
    with np.errstate(over="ignore"):
        rf = F(F(F(hw * F(math.sqrt(2.0))) * F(SD + 1)) * F(0.5))
    diag = int(np.rint(math.sqrt(float(cols) * cols + float(rows) * rows)))
    radius = int(np.rint(rf)) if rf < F(diag) else diag
    radius = min(max(radius, 0), diag)
    s, c = sincos_deg(ori, mut)
    return px, py, ori, radius, F(c / hw), F(s / hw)


def _finish(hist, exps, mut):
    """hist [n, 4, 4, 8] int64 fixed point, exps [n] (the share unit is 2^(e - 40)) -> the 8-bit rows."""
    n = len(hist)
    d = np.ldexp(hist.reshape(n, 128).astype(F), (np.asarray(exps, np.int32) - 40)[:, None]).astype(F)
    with np.errstate(invalid="ignore", over="ignore"):
        nrm2 = np.zeros(n, F)
        for t in range(128):  # left to right, product and sum rounded separately
            nrm2 = (nrm2 + (d[:, t] * d[:, t]).astype(F)).astype(F)
        thr = (np.sqrt(nrm2).astype(F) * F(0.2)).astype(F)
        val = d if "desc_no_clamp" in mut else np.where(d < thr[:, None], d, thr[:, None]).astype(F)
        nrm2 = np.zeros(n, F)
        for t in range(128):
            nrm2 = (nrm2 + (val[:, t] * val[:, t]).astype(F)).astype(F)
        nrm = np.sqrt(nrm2).astype(F)
        eps = F(np.finfo(F).eps)
        scale = (F(512) / np.where(nrm > eps, nrm, eps)).astype(F)
        v = (val * scale[:, None]).astype(F)
        v = np.floor(v + F(0.5)) if "desc_round_half_away" in mut else np.rint(v)
        v = np.where(v < 0, F(0), np.where(v > 255, F(255), v))  # a NaN stays a NaN, as in `v < 0 ? 0 : v > 255 ? 255 : v`
    return v.astype(F)


def descriptors(gx, gy, kps, mut=()):
    """The descriptor contract of DESIGN.md section 2, exact to the bit.  Every sample of the (2 radius + 1)^2 square is
    tested; nothing is pruned.  -> [n, 128] float32 holding 8-bit values.  (Fields whose dx^2 + dy^2 overflows are
    outside the contract.)"""
    mut = _check(mut)
    gx, gy = np.asarray(gx, F), np.asarray(gy, F)
    rows, cols = gx.shape
    kps = np.asarray(kps, F).reshape(-1, 4)
    n = len(kps)
    hist = np.zeros((n, SD, SD, SN), np.int64)
    exps = np.zeros(n, np.int32)
    live = np.zeros(n, bool)
    lo, hi_r, hi_c = (0, rows - 1, cols - 1) if "desc_border_inclusive" in mut else (1, rows - 2, cols - 2)
    for k in range(n):
        g = _geometry(kps[k], rows, cols, mut)
        if g is None:
            continue
        px, py, ori, radius, cos_t, sin_t = g
        # the magnitude bound: 2 * max(|gx|, |gy|) over the bounding square inside the interior, NaN skipped
        r0, r1 = max(py - radius, lo), min(py + radius, hi_r)
        c0, c1 = max(px - radius, lo), min(px + radius, hi_c)
        if r0 > r1 or c0 > c1:
            continue
        blk = np.maximum(np.abs(gx[r0:r1 + 1, c0:c1 + 1]), np.abs(gy[r0:r1 + 1, c0:c1 + 1]))
        blk = blk[~np.isnan(blk)]
        bound = F(blk.max() * F(2)) if blk.size else F(0)
        if not (bound > 0 and np.isfinite(bound)):
            continue
        e = int(math.frexp(float(bound))[1])  # bound < 2^e
        exps[k], live[k] = e, True
        # every sample whose pixel lies inside the interior (the others fail the interior test whatever their bins)
        i = np.arange(r0 - py, r1 - py + 1, dtype=np.int64)[:, None]
        j = np.arange(c0 - px, c1 - px + 1, dtype=np.int64)[None, :]
        fi, fj = i.astype(F), j.astype(F)
        c_rot = ((fj * cos_t).astype(F) - (fi * sin_t).astype(F)).astype(F)
        r_rot = ((fj * sin_t).astype(F) + (fi * cos_t).astype(F)).astype(F)
        rbin = ((r_rot + F(SD // 2)).astype(F) - F(0.5)).astype(F)
        cbin = ((c_rot + F(SD // 2)).astype(F) - F(0.5)).astype(F)
        ok = (rbin > -1) & (rbin < SD) & (cbin > -1) & (cbin < SD)
        si, sj = np.nonzero(ok)
        if not len(si):
            continue
        rbin, cbin, c_rot, r_rot = rbin[si, sj], cbin[si, sj], c_rot[si, sj], r_rot[si, sj]
        dx = gx[r0 + si, c0 + sj]
        dy = gy[r0 + si, c0 + sj] if "desc_dy_sign" in mut else -gy[r0 + si, c0 + sj]
        with np.errstate(invalid="ignore", over="ignore"):
            w = (((c_rot * c_rot).astype(F) + (r_rot * r_rot).astype(F)).astype(F) * F(-1.0 / (SD * SD * 0.5))).astype(F)
            mag = (np.sqrt(((dx * dx).astype(F) + (dy * dy).astype(F)).astype(F)).astype(F) * exp_neg(w)).astype(F)
            obin = ((fast_atan2_deg(dy, dx) - ori).astype(F) * F(F(SN) / F(360))).astype(F)
            rf_, cf_, of_ = np.floor(rbin), np.floor(cbin), np.floor(obin)
            rb, cb, ob = (rbin - rf_).astype(F), (cbin - cf_).astype(F), (obin - of_).astype(F)
            ri, ci = rf_.astype(np.int64), cf_.astype(np.int64)
            oi = np.where(np.isnan(of_), 0, of_).astype(np.int64)
            if "desc_no_wrap" not in mut:
                oi = np.where(oi < 0, oi + SN, oi)
                oi = np.where(oi >= SN, oi - SN, oi)
                oi = np.clip(oi, 0, SN - 1)  # (only a NaN sample can still be outside)
            v_r1 = (mag * rb).astype(F); v_r0 = (mag - v_r1).astype(F)
            v_rc11 = (v_r1 * cb).astype(F); v_rc10 = (v_r1 - v_rc11).astype(F)
            v_rc01 = (v_r0 * cb).astype(F); v_rc00 = (v_r0 - v_rc01).astype(F)
            shares = []
            for (dr, dc, vrc) in ((0, 0, v_rc00), (0, 1, v_rc01), (1, 0, v_rc10), (1, 1, v_rc11)):
                hi_s = (vrc * ob).astype(F)
                shares.append((dr, dc, 0, (vrc - hi_s).astype(F)))
                shares.append((dr, dc, 1, hi_s))
            nan = np.isnan(mag)
            h = hist[k].reshape(-1).view(np.uint64)
            for dr, dc, do, v in shares:
                fx = np.rint(np.ldexp(np.where(nan, 0, v).astype(np.float64), 40 - e)).astype(np.int64)
                fx = np.where(nan, np.int64(-2 ** 63), fx)  # llrintf(NaN): every share of a NaN sample
                r_, c_, o_ = ri + dr, ci + dc, oi + do
                if "desc_no_wrap" not in mut:
                    o_ = np.where(o_ == SN, 0, o_)  # the orientation axis is circular
                inside = (r_ >= 0) & (r_ < SD) & (c_ >= 0) & (c_ < SD) & (o_ >= 0) & (o_ < SN)
                np.add.at(h, ((r_ * SD + c_) * SN + o_)[inside], fx[inside].view(np.uint64))  # wraps like int64
    out = np.zeros((n, 128), F)
    if live.any():
        out[live] = _finish(hist[live], exps[live], mut)
    return out


def descriptors_ideal(gx, gy, kps):
    """The same published algorithm in float64 with libm cos / sin / exp / atan2, a float64 histogram and no fixed
    point: the witness for the polynomials, the fixed point and the float arithmetic.  The integer decisions (the
    rounded position, the radius) are the contract's."""
    gx, gy = np.asarray(gx, np.float64), np.asarray(gy, np.float64)
    rows, cols = gx.shape
    kps = np.asarray(kps, F).reshape(-1, 4)
    out = np.zeros((len(kps), 128), F)
    for k, kp in enumerate(kps):
        g = _geometry(kp, rows, cols, frozenset())
        if g is None:
            continue
        px, py, _, radius, _, _ = g
        size, angle = float(kp[2]), float(kp[3])
        ori = (360.0 - angle) % 360.0
        hw = 1.5 * size
        ct, st = math.cos(math.radians(ori)) / hw, math.sin(math.radians(ori)) / hw
        i, j = np.mgrid[-radius:radius + 1, -radius:radius + 1]
        c_rot, r_rot = j * ct - i * st, j * st + i * ct
        rbin, cbin = r_rot + 1.5, c_rot + 1.5
        r, c = py + i, px + j
        ok = (rbin > -1) & (rbin < SD) & (cbin > -1) & (cbin < SD) & (r > 0) & (r < rows - 1) & (c > 0) & (c < cols - 1)
        if not ok.any():
            continue
        rbin, cbin, c_rot, r_rot, r, c = (a[ok] for a in (rbin, cbin, c_rot, r_rot, r, c))
        dx, dy = gx[r, c], -gy[r, c]
        mag = np.hypot(dx, dy) * np.exp(-(c_rot ** 2 + r_rot ** 2) / 8.0)
        obin = ((np.degrees(np.arctan2(dy, dx)) % 360.0) - ori) * (SN / 360.0)
        r0, c0, o0 = np.floor(rbin), np.floor(cbin), np.floor(obin)
        rb, cb, ob = rbin - r0, cbin - c0, obin - o0
        r0, c0, o0 = r0.astype(int), c0.astype(int), o0.astype(int)
        h = np.zeros((SD + 2, SD + 2, SN), np.float64)
        for dr in (0, 1):
            for dc in (0, 1):
                for do in (0, 1):
                    v = mag * (rb if dr else 1 - rb) * (cb if dc else 1 - cb) * (ob if do else 1 - ob)
                    np.add.at(h, (r0 + 1 + dr, c0 + 1 + dc, (o0 + do) % SN), v)
        d = h[1:SD + 1, 1:SD + 1].reshape(-1)
        nrm = math.sqrt((d * d).sum())
        if not nrm > 0:
            continue
        val = np.minimum(d, 0.2 * nrm)
        out[k] = np.clip(np.rint(val * (512.0 / max(math.sqrt((val * val).sum()), float(np.finfo(F).eps)))), 0, 255)
    return out


# ------------------------------------------------------------------------------- knnMatch(k = 2), the ratio test

def sq_distances(query, train, mut=()):
    """[nq, nt] float32: per pair `acc = fmaf(d, d, acc)` from +0 with `d = q[k] - t[k]` in float, k ascending."""
    q, t = np.asarray(query, F), np.asarray(train, F)
    acc = np.zeros((len(q), len(t)), F)
    dims = range(q.shape[1] - 1, -1, -1) if "knn_reverse_dims" in mut else range(q.shape[1])
    with np.errstate(invalid="ignore", over="ignore"):
        for k in dims:
            d = (q[:, k][:, None] - t[:, k][None, :]).astype(F)
            acc = fmaf(d, d, acc)
    return acc


def knn2(query, train, rows=None, mut=()):
    """cv::BFMatcher(NORM_L2)::knnMatch(query, train, 2) (Solution.cpp:179) -> (idx [n, 2] int32, dist [n, 2] float32):
    the two smallest squared distances by (distance, index), then sqrt in float.  A NaN distance is never selected:
    a query with fewer than two non-NaN distances has index -1 and distance +inf in the empty places.  +inf is an
    ordinary distance.  rows: the queries to compute (default all)."""
    mut = _check(mut)
    q, t = np.asarray(query, F), np.asarray(train, F)
    sel = np.arange(len(q)) if rows is None else np.asarray(rows, np.int64)
    idx = np.full((len(sel), 2), -1, np.int32)
    dist = np.full((len(sel), 2), np.inf, F)
    step = max(1, (1 << 21) // max(1, len(t)))
    for a in range(0, len(sel), step):
        d2 = sq_distances(q[sel[a:a + step]], t, mut)
        if "knn_tie_high_index" in mut:
            order = len(t) - 1 - np.argsort(d2[:, ::-1], axis=1, kind="stable")[:, :2]
        else:
            order = np.argsort(d2, axis=1, kind="stable")[:, :2]  # NaNs sort last, equal values by index
        dd = np.take_along_axis(d2, order, 1)
        real = ~np.isnan(dd)
        idx[a:a + step][real] = order[real]
        dist[a:a + step][real] = np.sqrt(dd[real]).astype(F)
    return idx, dist


def ratio_filter(idx2, dist2, ratio, cap=None, mut=()):
    """Solution.cpp:180-184: keep query q when `double(d0) < ratio * double(d1)`.  -> (matches [m, 2] int32 =
    (queryIdx, trainIdx), distances [m], count): the first `cap` kept queries in query order and the number kept."""
    mut = _check(mut)
    idx2, dist2 = np.asarray(idx2, np.int32), np.asarray(dist2, F)
    with np.errstate(invalid="ignore", over="ignore"):
        if "ratio_float" in mut:
            lhs, rhs = dist2[:, 0], (F(ratio) * dist2[:, 1]).astype(F)
        else:
            lhs, rhs = dist2[:, 0].astype(np.float64), float(ratio) * dist2[:, 1].astype(np.float64)
        keep = (lhs <= rhs) if "ratio_le" in mut else (lhs < rhs)
    qs = np.nonzero(keep)[0]
    count = len(qs)
    if cap is not None:
        qs = qs[:cap]
    return np.stack([qs, idx2[qs, 0]], 1).astype(np.int32), dist2[qs, 0].copy(), count
