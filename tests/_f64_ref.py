"""Float64 references of the three float pipelines, each with a per-pixel error bound (numpy + scipy only).

`lk_flow` (lk::calcOpticalFlow, one level), `harris_response` (harris::getCornerResponse) and `ncc_admissible`
(disparityNCorr) restate the reference directly -- ProblemSets/ps5_cpp/lib/OpticalFlow.cpp:12-104,
ProblemSets/ps4_cpp/lib/Harris.cpp:43-97 and Harris.cu:36-91, ProblemSets/ps2_cpp/lib/DisparityNCorr.cu:83-108 and
:16,212 -- and share no code with oracle/*.c or tests/_oracle.py.  Where the oracle checks a kernel bit for bit, these
check both against the operation itself: the value is computed in float64 with exact constants, and `bound` bounds
how far ANY evaluation that follows DESIGN.md §2 can be from it -- float32 storage of every named intermediate, any
summation order, with or without fused multiply-adds.  An output outside the bound is wrong whatever the oracle says.

Derivation (standard forward error analysis, u = 2^-24, gamma_n = n u / (1 - n u)):

* Sums.  Any evaluation of a sum of n rounded products sum k_i x_i (fused or not, any order) is within
  gamma_n sum |k_i x_i| of the exact sum.  A separable filter (row pass of nr taps, column pass of nc taps, float
  intermediate) whose float taps carry a relative error t and whose input carries an error field E is within
      c * F(|x| + E) + F(E),   c = (1 + t)(1 + gamma_nr)(1 + gamma_nc) - 1,
  of the exact filter F(x), where F(|x|) is the same separable operator on absolute values and absolute taps
  (nr, nc count nonzero taps: the Sobel derivative's zero tap adds an exact zero).
* Constants are error, not definition.  The exact taps are the Gaussian exp(-x^2 / 2 sigma^2) / sum, the Sobel
  taps times 1/9, alpha as given.  getGaussianKernel's float taps (float of exp, double sum, float of the quotient)
  are within TAP_REL = 3u (+ double rounding) of the exact taps; the float 1/9 folded into the Sobel smoothing taps within u; the float
  alpha within u; Harris' float weight g[wy] g[wx] within (1 + TAP_REL)^2 (1 + u) - 1.  The window sigma of LK is
  the reference's expression float(winSize) / 3.f, a float32 value by definition.
* Products and differences of inputs that carry errors ea, eb: |ab - a'b'| <= |a| eb + |b| ea + ea eb, plus u of the
  rounded result.  Underflow: every rounding may add ETA = 2^-149 absolute; each bound adds its count of roundings
  times ETA (invisible at ordinary magnitudes, decisive at 2^-40).
* LK.  Sobel 3x3 scaled 1/9 on both images (border reflect-101), Ix = (a + b) / 2 one rounding, It = next - prev
  one rounding, five products, GaussianBlur(win, sigma) reflect-101.  det is formed in double from the float sums
  (float x float products are exact in double; one rounding in the difference).  A pixel STRADDLES when the det
  interval contains 0.1: both (0, 0) and the solve are admissible there.  The 2x2 solve (in double, then rounded to
  float) is bounded componentwise (Bauer-Skeel): with dA, db the error bounds of A and b (plus 2^-50 |A|, |b| for
  the double arithmetic),  |dx| <= 2 |A^-1| (dA |x| + db)  whenever  eta = || |A^-1| dA ||_inf <= 1/2; summing the
  Neumann series instead of doubling, v + eta / (1 - eta) max(v) with v = |A^-1| (dA |x| + db) is used, which is
  never looser by more than the max and near v where eta is small.  Plus u |x| for the final float rounding.  Where that condition fails (ILLCOND) only finiteness is checkable.
* Harris.  The three window sums have n = win^2 terms, each a weight times a rounded product (and under harris::cpu
  one more rounding for the unfused multiply): c = (1 + w_rel)(1 + u)^2 (1 + gamma_n) - 1 on the clamped window sums
  of |g_x g_y| etc.  R = det - alpha tr^2 is then bounded through its operations; the bound scales with
  |mxx myy| + mxy^2 + alpha tr^2, not with |R|: that cancellation is what the check has to survive.  The same bound
  covers the default (float det, fmaf chain) and cpu_arithmetic=True (double det, unfused) arithmetic.  Where
  det or alpha tr^2 may pass 2^127 (gradients of images scaled by 2^30), float32 overflows and the bound is inf.
* NCC.  p, sum a^2, sum b^2 over a (2r+1) x wcols window of clamp-to-edge fetches, n = (2r+1) wcols terms:
  gamma_n (1 + u) times the window sum of |terms| (+ n ETA).  Under ROLLING (40-row strips, each row's column sums
  updated by one subtraction and one addition) row j of a strip has seen m = 2r + 1 + 2j column terms, every row
  from the strip's first window down to its own at most twice: gamma_(m + wcols) (1 + u) times twice that mass.
  The score p / sqrt(sum a^2 sum b^2) then carries the relative errors of the product (u), sqrt (u) and division
  (u) on top; it is taken as an interval.  A window whose exact sum a^2 or sum b^2 is 0 has p = 0 and scores NaN
  (never a candidate); a score whose denominator may leave float's normal range, or whose energies are not known to
  a quarter of their size, is unknown ([-inf, inf]).
* Safety.  Second-order terms dropped above and the float64 rounding of the references themselves are absorbed by
  one factor SAFETY = 2, applied once to each returned bound (and to the det and score error widths).

Non-finite inputs are out of scope (tests/test_contract_corners_gpu.py pins them against the oracle).
"""
import numpy as np
from scipy import ndimage

U = 2.0 ** -24
ETA = 2.0 ** -149
SAFETY = 2.0
TAP_REL = 3 * U + 2.0 ** -50  # float of exp, the double sum's weighted u, float of the quotient
TAU = 0.1  # OpticalFlow.cpp:82
COLS_2R, ROLLING = 1, 8  # MICV_STEREO_* flags that change the NCC arithmetic
STRIP = 40  # ROWS_PER_THREAD, DisparityNCorr.cu:17


def gamma(n):
    return n * U / (1 - n * U)


def gaussian_taps(n, sigma):
    """cv::getGaussianKernel(n, sigma) with exact arithmetic (sigma > 0)."""
    x = np.arange(n, dtype=np.float64) - (n - 1) / 2.0
    t = np.exp(-0.5 * x * x / (float(sigma) ** 2))
    return t / t.sum()


def _index(n, lo, hi, border):
    p = np.arange(lo, hi)
    if border == "clamp":
        return np.clip(p, 0, n - 1)
    if n == 1:  # reflect-101 (cv::borderInterpolate)
        return np.zeros_like(p)
    m = np.mod(p, 2 * n - 2)
    return np.where(m >= n, 2 * n - 2 - m, m)


def sep(x, krow, kcol, border):
    """Correlation with krow along x, then kcol along y (taps centred), float64."""
    rows, cols = x.shape
    ar, ac = len(krow) // 2, len(kcol) // 2
    xe = x[:, _index(cols, -ar, cols + ar, border)]
    t = ndimage.correlate1d(xe, np.asarray(krow, np.float64), axis=1, mode="constant")[:, ar:ar + cols]
    te = t[_index(rows, -ac, rows + ac, border)]
    return ndimage.correlate1d(te, np.asarray(kcol, np.float64), axis=0, mode="constant")[ac:ac + rows]


def _sep_err(xabs, err, krow, kcol, tap_rel, border):
    """Error bound of a float evaluation of sep() whose input is within err of exact (xabs = |exact input|)."""
    # a zero tap adds an exact zero: only nonzero taps round
    c = (1 + tap_rel) * (1 + gamma(np.count_nonzero(krow))) * (1 + gamma(np.count_nonzero(kcol))) - 1
    kr, kc = np.abs(krow), np.abs(kcol)
    fe = sep(err, kr, kc, border) if np.any(err) else 0.0
    return c * sep(xabs + err, kr, kc, border) + fe + (len(krow) + 1) * (len(kcol) + 1) * ETA


def _prod(a, ea, b, eb):
    """Bound on |fl(a' b') - a b| for |a' - a| <= ea, |b' - b| <= eb."""
    aa, ab = np.abs(a), np.abs(b)
    return aa * eb + ab * ea + ea * eb + U * (aa + ea) * (ab + eb) + ETA


def _f64(img, name):
    a = np.asarray(img, dtype=np.float32)
    if a.ndim != 2 or a.size == 0 or not np.all(np.isfinite(a)):
        raise ValueError(f"{name}: a non-empty finite 2-D float32 image is required")
    return a.astype(np.float64)


def lk_flow(prev, nxt, win):
    """lk::calcOpticalFlow, single level (OpticalFlow.cpp:41-104).

    Returns (value, bound, straddle, illcond): value and bound are float64 [2, rows, cols] (u, v).  value is the
    solve where a det >= 0.1 is possible and (0, 0) elsewhere; at STRADDLE pixels (0, 0) is admissible too.  bound is
    inf at ILLCOND pixels (solve possible, Bauer-Skeel condition fails) and 0 where only (0, 0) is possible."""
    p, n = _f64(prev, "prev"), _f64(nxt, "next")
    if p.shape != n.shape or win < 1 or win % 2 == 0:
        raise ValueError("same-size images and an odd window are required")
    # computeGradients (OpticalFlow.cpp:12-39): Sobel 3x3, scale 1/9 folded into the smoothing taps
    d1, s1 = np.array([-1.0, 0.0, 1.0]), np.array([1.0, 2.0, 1.0]) / 9.0
    grads = []
    for img in (p, n):
        ai = np.abs(img)
        zero = np.zeros_like(img)
        gx, gy = sep(img, d1, s1, "reflect101"), sep(img, s1, d1, "reflect101")
        grads.append((gx, _sep_err(ai, zero, d1, s1, U, "reflect101"),
                      gy, _sep_err(ai, zero, s1, d1, U, "reflect101")))
    (pgx, epgx, pgy, epgy), (ngx, engx, ngy, engy) = grads
    # :62-64  Ix = (nextIx + prevIx) / 2, It = next - prev
    ix = (ngx + pgx) / 2
    eix = (engx + epgx) / 2 + U * (np.abs(ngx) + np.abs(pgx) + engx + epgx) / 2 + ETA
    iy = (ngy + pgy) / 2
    eiy = (engy + epgy) / 2 + U * (np.abs(ngy) + np.abs(pgy) + engy + epgy) / 2 + ETA
    it = n - p
    eit = U * np.abs(it) + ETA
    # :66-77  five products, GaussianBlur(win, float(win) / 3.f), reflect-101
    sigma = float(np.float32(win) / np.float32(3))
    g = gaussian_taps(win, sigma)
    trel = (1 + TAP_REL) ** 2 - 1
    S, E = [], []
    for a, ea, b, eb in ((ix, eix, ix, eix), (ix, eix, iy, eiy), (iy, eiy, iy, eiy), (ix, eix, it, eit), (iy, eiy, it, eit)):
        S.append(sep(a * b, g, g, "reflect101"))
        E.append(_sep_err(np.abs(a * b), _prod(a, ea, b, eb), g, g, trel, "reflect101"))
    sxx, sxy, syy, sxt, syt = S
    exx, exy, eyy, ext, eyt = E
    # :82-98  det in double from the float sums; det < 0.1 -> (0, 0)
    det = sxx * syy - sxy * sxy
    edet = (np.abs(sxx) * eyy + np.abs(syy) * exx + exx * eyy + 2 * np.abs(sxy) * exy + exy * exy
            + 2.0 ** -52 * ((np.abs(sxx) + exx) * (np.abs(syy) + eyy) + (np.abs(sxy) + exy) ** 2))
    edet *= SAFETY
    may_zero = det - edet < TAU
    may_solve = det + edet >= TAU
    straddle = may_zero & may_solve
    # cv::solve (DECOMP_LU) of A x = b, b = -(Sxt, Syt); Bauer-Skeel componentwise bound
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        b0, b1 = -sxt, -syt
        i00, i01, i11 = syy / det, -sxy / det, sxx / det
        x0 = i00 * b0 + i01 * b1
        x1 = i01 * b0 + i11 * b1
        da00, da01, da11 = exx + 2.0 ** -50 * np.abs(sxx), exy + 2.0 ** -50 * np.abs(sxy), eyy + 2.0 ** -50 * np.abs(syy)
        db0, db1 = ext + 2.0 ** -50 * np.abs(b0), eyt + 2.0 ** -50 * np.abs(b1)
        a00, a01, a11 = np.abs(i00), np.abs(i01), np.abs(i11)
        norm = np.maximum(a00 * da00 + a01 * da01 + a00 * da01 + a01 * da11,
                          a01 * da00 + a11 * da01 + a01 * da01 + a11 * da11)
        r0 = da00 * np.abs(x0) + da01 * np.abs(x1) + db0
        r1 = da01 * np.abs(x0) + da11 * np.abs(x1) + db1
        v0, v1 = a00 * r0 + a01 * r1, a01 * r0 + a11 * r1
        # (I - |A^-1| dA)^-1 v <= v + eta / (1 - eta) max(v): at most 2 v's size where eta <= 1/2, near v where eta -> 0
        tail = norm / (1 - norm) * np.maximum(v0, v1)
        bx0, bx1 = v0 + tail, v1 + tail
        bx0 = SAFETY * (bx0 + U * (np.abs(x0) + bx0))
        bx1 = SAFETY * (bx1 + U * (np.abs(x1) + bx1))
        ok = (det > 0) & (norm <= 0.5) & np.isfinite(bx0) & np.isfinite(bx1)
    illcond = may_solve & ~ok
    value = np.zeros((2,) + p.shape)
    bound = np.zeros((2,) + p.shape)
    sel = may_solve & ok
    value[0][sel], value[1][sel] = x0[sel], x1[sel]
    bound[0][sel], bound[1][sel] = bx0[sel], bx1[sel]
    bound[0][illcond] = bound[1][illcond] = np.inf
    return value, bound, straddle, illcond


def harris_response(gx, gy, win, sigma, alpha):
    """harris::getCornerResponse (Harris.cpp:43-97 / Harris.cu:36-91): clamped window, weights g[wy] g[wx],
    R = det(M) - alpha tr(M)^2.  Returns (value, bound), float64 [rows, cols]; one bound for both arithmetics."""
    x, y = _f64(gx, "gx"), _f64(gy, "gy")
    if x.shape != y.shape or win < 1 or win % 2 == 0 or not sigma > 0:
        raise ValueError("same-size gradients, an odd window and sigma > 0 are required")
    g = gaussian_taps(win, sigma)
    nterm = win * win
    c = (1 + TAP_REL) ** 2 * (1 + U) * (1 + U) ** 2 * (1 + gamma(nterm)) - 1
    m, e = [], []
    for t in (x * x, x * y, y * y):
        m.append(sep(t, g, g, "clamp"))
        e.append(c * sep(np.abs(t), g, g, "clamp") + 2 * nterm * ETA)
    mxx, mxy, myy = m
    exx, exy, eyy = e
    al = float(alpha)
    tr = mxx + myy
    det = mxx * myy - mxy * mxy
    etr = exx + eyy + U * (np.abs(mxx) + np.abs(myy) + exx + eyy) + ETA
    scale = np.abs(mxx * myy) + mxy * mxy
    ed = (np.abs(myy) * exx + np.abs(mxx) * eyy + exx * eyy + 2 * np.abs(mxy) * exy + exy * exy
          + gamma(2) * (scale + (np.abs(mxx) + exx) * eyy + np.abs(myy) * exx + (2 * np.abs(mxy) + exy) * exy) + 2 * ETA)
    atr = np.abs(tr) + etr
    eq = al * (2 * np.abs(tr) * etr + etr * etr) + ((1 + U) ** 3 - 1) * al * atr * atr + 2 * ETA
    bound = SAFETY * (ed + eq + U * (np.abs(det) + al * tr * tr + ed + eq) + ETA)
    # float32 intermediates that may overflow: nothing is checkable there
    bound[~(SAFETY * (scale + al * atr * atr + ed + eq) < 2.0 ** 127)] = np.inf
    return det - al * tr * tr, bound


# ---------------------------------------------------------------------------------------------------- NCC ----

def _box(f, rad, wcols, y_lo=None):
    """Window sums of f (rows + 2 rad, cols + 2 rad + extra, rows clamp-extended): rows y - rad .. y + rad (or
    y_lo[y] .. y + rad, as extended-row indices), columns j .. j + wcols - 1 of f for every start j."""
    rows = f.shape[0] - 2 * rad
    cy = np.zeros((f.shape[0] + 1, f.shape[1]), f.dtype)
    np.cumsum(f, axis=0, out=cy[1:])
    cs = cy[2 * rad + 1:] - (cy[:rows] if y_lo is None else cy[y_lo])
    cx = np.zeros((rows, f.shape[1] + 1), f.dtype)
    np.cumsum(cs, axis=1, out=cx[:, 1:])
    return cx[:, wcols:] - cx[:, :f.shape[1] + 1 - wcols]


def _ncc_intervals(left, right, rad, dmin, dmax, flags, order):
    """Yields (d, lo, hi): an interval holding every contract evaluation of the score at d (lo = hi = -inf: never a
    candidate; lo = -inf, hi = inf: unknown)."""
    L, R = _f64(left, "left"), _f64(right, "right")
    if L.shape != R.shape or rad < 0 or dmin > dmax:
        raise ValueError("same-size images, rad >= 0 and dmin <= dmax are required")
    rows, cols = L.shape
    wcols = 2 * rad if flags & COLS_2R else 2 * rad + 1
    ry = np.clip(np.arange(-rad, rows + rad), 0, rows - 1)
    Le = L[ry][:, np.clip(np.arange(-rad, cols + rad), 0, cols - 1)]
    Re = R[ry][:, np.clip(np.arange(-rad + dmin, cols + rad + dmax), 0, cols - 1)]
    ncol = cols + 2 * rad
    if flags & ROLLING:
        j = np.arange(rows) % STRIP
        y_lo = np.arange(rows) - j
        n = (2 * rad + 1 + 2 * j + wcols)[:, None]
        mass_f = 2.0
    else:
        y_lo, n, mass_f = None, (2 * rad + 1) * wcols, 1.0
    rel = (1 + gamma(n)) * (1 + U) - 1
    eta = 2 * n * ETA
    AA = _box(Le * Le, rad, wcols)[:, :cols]
    BBall = _box(Re * Re, rad, wcols)
    ea = rel * mass_f * (_box(Le * Le, rad, wcols, y_lo)[:, :cols] if y_lo is not None else AA) + eta
    eball = rel * mass_f * (_box(Re * Re, rad, wcols, y_lo) if y_lo is not None else BBall) + eta
    nzA = _box((Le != 0).astype(np.int64), rad, wcols)[:, :cols]
    nzB = _box((Re != 0).astype(np.int64), rad, wcols)

    def side(E, e):
        """Energy-side factors, d-independent: bounds on sqrt of the computed energy (its part of the denominator,
        with the sqrt's and the product's rounding), and whether it is known well enough."""
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            r = SAFETY * e / E
            lo = np.sqrt(E * np.maximum(1 - r, 0) * (1 - U)) * (1 - U)
            hi = np.sqrt(E * (1 + r) * (1 + U)) * (1 + U)
            bad = ~(r <= 0.25) | ~(E * (1 + r) <= 2.0 ** 127)
        return lo, hi, bad

    alo, ahi, abad = side(AA, ea)
    blo, bhi, bbad = side(BBall, eball)
    zA, zB = nzA == 0, nzB == 0
    signed = L.min() < 0 or R.min() < 0
    ds = range(dmin, dmax + 1) if order > 0 else range(dmax, dmin - 1, -1)
    for d in ds:
        o = d - dmin
        pr = Le * Re[:, o:o + ncol]
        P = _box(pr, rad, wcols)[:, :cols]
        if y_lo is not None or signed:
            ep = SAFETY * (rel * mass_f * _box(np.abs(pr), rad, wcols, y_lo)[:, :cols] + eta)
        else:
            ep = SAFETY * (rel * P + eta)
        dlo = alo * blo[:, o:o + cols] * (1 - 2 * U)  # sqrt(fl(AA BB)), then the division's rounding
        dhi = ahi * bhi[:, o:o + cols] * (1 + 2 * U)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            plo, phi = P - ep, P + ep
            lo = plo / np.where(plo >= 0, dhi, dlo)
            hi = phi / np.where(phi >= 0, dlo, dhi)
            lo -= np.abs(lo) * 3 * U
            hi += np.abs(hi) * 3 * U
            # the product fl(AA BB) must stay normal: sqrt within [2^-63, 2^63.5)
            unknown = abad | bbad[:, o:o + cols] | ~(dlo >= 2.0 ** -62) | ~(dhi <= 2.0 ** 63)
        zero = zA | zB[:, o:o + cols]
        lo[zero | unknown] = -np.inf
        hi[unknown] = np.inf
        hi[zero] = -np.inf
        yield d, lo, hi


def ncc_admissible(left, right, rad, dmin, dmax, flags=0):
    """disparityNCorr's admissible outputs (DisparityNCorr.cu:83-108; best = 0, strict '>', :16,212).

    Returns a bool volume [dmax - dmin + 2, rows, cols]: plane 0 is the output -1, plane 1 + k is disparity dmin + k.
    d is admissible when its upper score beats every earlier d's lower score strictly, every later d's lower score
    non-strictly, and 0; -1 when no d has a lower score above 0.  Works per disparity on whole images (two passes)."""
    rows, cols = np.shape(left)
    nd = dmax - dmin + 1
    vol = np.zeros((nd + 1, rows, cols), bool)
    best_lo = np.zeros((rows, cols))  # running max of lo over earlier d, and the initial best = 0
    for d, lo, hi in _ncc_intervals(left, right, rad, dmin, dmax, flags, +1):
        vol[1 + d - dmin] = hi > best_lo
        best_lo = np.maximum(best_lo, lo)
    vol[0] = best_lo <= 0
    later = np.full((rows, cols), -np.inf)
    for d, lo, hi in _ncc_intervals(left, right, rad, dmin, dmax, flags, -1):
        vol[1 + d - dmin] &= hi >= later
        later = np.maximum(later, lo)
    return vol


def ncc_admits(vol, disp, dmin):
    """Per pixel: is disp (the int8 output) in the admissible set?  -1 is "no match" or the disparity -1."""
    disp = np.asarray(disp).astype(np.int64)
    k = disp - dmin + 1
    inside = (k >= 1) & (k < vol.shape[0])
    hit = inside & np.take_along_axis(vol, np.clip(k, 0, vol.shape[0] - 1)[None], 0)[0]
    return hit | ((disp == -1) & vol[0])
