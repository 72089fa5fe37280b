"""References of disparitySSD for float images that are NOT 8-bit-valued (numpy only; no oracle code, no ctypes).

Written from the contract alone -- csrc/stereo.hip's header, DESIGN.md section 2 ("Stereo"), include/mi_cv.h's
MICV_STEREO_* flags and the lines of ProblemSets/ps2_cpp/lib/DisparitySSD.cu / .cpp they cite -- as three independent
statements:

* `ssd_f32`: the ORDER-EXACT float32 restatement.  Every step is one numpy float32 operation on whole images, in the
  contract's association, so the bytes are the contract's whatever the image holds:
      term(y, xc, d)   = fl(fl(left(y, xc) - right(y, xc + d))^2)                both fetches clamp-to-edge
      colsum(y, xc, d) = ((term(y-r) + term(y-r+1)) + ...) + term(y+r)          top -> bottom   (DisparitySSD.cu:67-78)
      cost(y, x, d)    = ((colsum(x-r) + colsum(x-r+1)) + ...) + colsum(x-r+wcols-1)   left -> right       (:83-86)
  wcols = 2r + 1, or 2r under COLS_2R (:84).  d ascending, `cost < best` strict (:88), best starting at +inf or at 5e6
  under MIN_SSD_5E6 (:16,178), the output -1 where nothing beats it (:177).  A NaN cost never satisfies `<`.
  Under ROLLING the column sums are the kernel's own (:97-138): rows in strips of 40 (:17); a strip's first row is
  summed fresh, every further row is `(p - term that left the window) + term that entered`, two roundings.
* `ssd_serial_f32`: serial::disparitySSD (DisparitySSD.cpp:35-61).  Every term is rounded half away from zero
  (`round`, :51) into an integer sum, so the order of the additions is immaterial: int64 window sums.  For output x the
  positions searched are the padded columns max(0, x + r + minD) .. min(pcols - 1, x + r + maxD) (:42-43), i.e. the d
  with -r <= x + d <= cols - 1 + r; best starts at (99999999, 0) (:37-38), strict `<` (:54).  Finite images only.
* `ssd_admissible` / `ssd_admits`: the costs in float64 with a per-(d, pixel) interval that ANY float32 evaluation of
  the contract's terms falls in, whatever its association, and the set of disparities such an evaluation can return.

Bound of `ssd_admissible` (u = 2^-24, gamma_k = k u / (1 - k u), standard forward analysis):
  Every term is computed with three roundings -- the difference, and the square of the rounded difference is
  d^2 (1 + e1)^2 (1 + e2) -- so it is t (1 + theta_3) with t >= 0 the exact term.  Fresh sums: a term then passes
  through at most 2r column additions and wcols - 1 row additions; all terms are >= 0, so nothing cancels and the
  computed cost is C (1 + theta_k), k = 3 + 2r + wcols - 1, |theta_k| <= gamma_k: a RELATIVE bound on the exact cost C.
  ROLLING: the running sum of row j of a strip is the result of m = 2r + 1 + 2j additions and subtractions.  Written
  out, fl-sum = sum over the operations of (+-)term (1 + theta_m), so its distance from the exact window sum is at most
  gamma_m times the sum of |operands| -- every term from the strip's first window down to row j's, each at most twice
  (once added, once subtracted): twice the mass M of the column over rows y0 - r .. y + r.  (The rounding of a term
  itself cancels when the same value is subtracted again; what remains is inside gamma_3 M.)  With the row additions:
  |cost - C| <= gamma_(3 + m + wcols - 1) * 2 M, M the window sum over those rows, the same argument tests/_f64_ref.py
  makes for NCC.  A square that may underflow (0 < |difference| < 2^-62) adds ETA = 2^-149; where every term is exactly 0 the
  interval is the point 0.  Second-order terms and the float64 rounding of C
  itself are absorbed by the one factor SAFETY = 2 on the width.  A cost whose upper bound reaches 2^127 may overflow
  in float32: its upper end is +inf.

Mutants (`mutant=` keyword, for tests/test_stereo_f32_ref.py only): wrong readings of the contract that a test of the
kernels must be able to tell from the right one.
  "assoc_rev"    bottom -> top column sums and right -> left row sums (a legal evaluation, other rounding)
  "rows_first"   row sums over the window's columns first, then top -> bottom (legal, other rounding)
  "wcols+1", "wcols-1"   a window one column wider / narrower on the right
  "le"           `<=` for `<`: the last of equal costs wins
  "reflect101"   BORDER_REFLECT_101 instead of clamp-to-edge
  "fresh"        fresh column sums under ROLLING
  "half_even"    serial:: terms rounded half to even
  "inf_start"    best starts at +inf under MIN_SSD_5E6
  "skip_chunk2"  the first disparity of the second chunk of 64 (minD + 64) is never evaluated
"""
import numpy as np

from _f64_ref import ETA, SAFETY, gamma  # (u = 2^-24 enters through gamma)

COLS_2R, MIN_SSD_5E6, SERIAL, ROLLING = 1, 2, 4, 8  # MICV_STEREO_*
STRIP = 40  # ROWS_PER_THREAD, DisparitySSD.cu:17
MUTANTS = ("assoc_rev", "rows_first", "wcols+1", "wcols-1", "le", "reflect101", "fresh", "half_even", "inf_start",
           "skip_chunk2")
F32 = np.float32


def _index(n, lo, hi, reflect):
    p = np.arange(lo, hi)
    if not reflect:
        return np.clip(p, 0, n - 1)
    if n == 1:
        return np.zeros_like(p)
    m = np.mod(p, 2 * n - 2)
    return np.where(m >= n, 2 * n - 2 - m, m)


def _args(left, right, rad, lo, hi, dtype):
    L, R = np.asarray(left, dtype=F32), np.asarray(right, dtype=F32)
    if L.ndim != 2 or L.size == 0 or L.shape != R.shape:
        raise ValueError("two non-empty 2-D images of one size are required")
    if not 0 <= rad <= 31 or not -128 <= lo <= hi <= 127:
        raise ValueError("radius 0..31 and int8 disparities lo <= hi are required")
    return L.astype(dtype), R.astype(dtype)


def _extended(L, R, rad, lo, hi, ncol, reflect=False):
    """Left over rows -r .. rows-1+r and window columns -r .. -r+ncol-1; right over the same rows and the columns every
    shift lo..hi of those reaches.  Row y + r of either is image row y; right column (d - lo) + i pairs with left column i."""
    rows, cols = L.shape
    ry = _index(rows, -rad, rows + rad, reflect)
    return (L[ry][:, _index(cols, -rad, -rad + ncol, reflect)],
            R[ry][:, _index(cols, -rad + lo, -rad + ncol + hi, reflect)])


def _wcols(rad, flags, mutant):
    if flags & COLS_2R and rad < 1:
        raise ValueError("COLS_2R needs radius >= 1")
    w = 2 * rad if flags & COLS_2R else 2 * rad + 1
    return w + (mutant == "wcols+1") - (mutant == "wcols-1")


def _fresh(T, rows, cols, rad, wcols, mutant):
    """cost [rows, cols] of one disparity from its terms T [rows + 2r, >= cols + wcols - 1], float32, in order."""
    if wcols == 0:
        return np.zeros((rows, cols), F32)
    nr = 2 * rad + 1
    if mutant == "rows_first":
        ks = range(wcols)
        rs = T[:, 0:cols].copy()
        for k in ks[1:]:
            rs += T[:, k:k + cols]
        acc = rs[0:rows].copy()
        for k in range(1, nr):
            acc += rs[k:k + rows]
        return acc
    rk = list(range(nr))
    ck = list(range(wcols))
    if mutant == "assoc_rev":
        rk.reverse()
        ck.reverse()
    cs = T[rk[0]:rk[0] + rows].copy()
    for k in rk[1:]:
        cs += T[k:k + rows]
    acc = cs[:, ck[0]:ck[0] + cols].copy()
    for k in ck[1:]:
        acc += cs[:, k:k + cols]
    return acc


def _rolling(T, rows, cols, rad, wcols, mutant):
    """The same under ROLLING: column sums carried down strips of 40 rows, then the row sums."""
    ncol = T.shape[1]
    nstrip = -(-rows // STRIP)
    cs = np.empty((nstrip * STRIP, ncol), F32)
    y0 = np.arange(nstrip) * STRIP
    last = T.shape[0] - 1
    rk = list(range(2 * rad + 1))
    if mutant == "assoc_rev":
        rk.reverse()
    p = np.zeros((nstrip, ncol), F32)
    for k in rk:  # rows y0 - r .. y0 + r from 0 (0 + x is x: terms are never -0)
        p = p + T[y0 + k]
    cs[y0] = p
    for j in range(1, STRIP):
        y = y0 + j  # rows past the image compute garbage that is cut off below
        p = (p - T[np.minimum(y - 1, last)]) + T[np.minimum(y + 2 * rad, last)]
        cs[y] = p
    cs = cs[:rows]
    ck = list(range(wcols))
    if mutant == "assoc_rev":
        ck.reverse()
    if mutant == "rows_first":
        raise ValueError("rows_first has no meaning under ROLLING")
    if not ck:
        return np.zeros((rows, cols), F32)
    acc = cs[:, ck[0]:ck[0] + cols].copy()
    for k in ck[1:]:
        acc += cs[:, k:k + cols]
    return acc


def ssd_f32(left, right, rad, lo, hi, flags=0, mutant=None):
    """cuda::disparitySSD in float32, operation by operation (flags: COLS_2R, MIN_SSD_5E6, ROLLING) -> int8."""
    if flags & ~(COLS_2R | MIN_SSD_5E6 | ROLLING):
        raise ValueError(f"flags {flags}: SERIAL is ssd_serial_f32")
    if mutant not in (None,) + MUTANTS or mutant == "half_even":
        raise ValueError(f"mutant {mutant}")
    L, R = _args(left, right, rad, lo, hi, F32)
    rows, cols = L.shape
    wcols = _wcols(rad, flags, mutant)
    ncol = cols + max(wcols, 1) - 1
    Le, Re = _extended(L, R, rad, lo, hi, ncol, mutant == "reflect101")
    start = np.inf if not flags & MIN_SSD_5E6 or mutant == "inf_start" else 5000000.0
    best = np.full((rows, cols), start, F32)
    disp = np.full((rows, cols), -1, np.int8)
    rolling = flags & ROLLING and mutant != "fresh"
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for d in range(lo, hi + 1):
            if mutant == "skip_chunk2" and d == lo + 64:
                continue
            diff = Le - Re[:, d - lo:d - lo + ncol]
            T = diff * diff
            cost = (_rolling if rolling else _fresh)(T, rows, cols, rad, wcols, mutant)
            better = cost <= best if mutant == "le" else cost < best
            best[better] = cost[better]
            disp[better] = d
    return disp


def _box(f, rad, wcols, cols, y_lo=None):
    """Window sums (any exact or float64 dtype): rows y - r .. y + r (or from extended row y_lo[y]), columns x .. x +
    wcols - 1 of f, for x = 0 .. cols - 1."""
    rows = f.shape[0] - 2 * rad
    cy = np.zeros((f.shape[0] + 1, f.shape[1]), f.dtype)
    np.cumsum(f, axis=0, out=cy[1:])
    cs = cy[2 * rad + 1:] - (cy[:rows] if y_lo is None else cy[y_lo])
    cx = np.zeros((rows, f.shape[1] + 1), f.dtype)
    np.cumsum(cs, axis=1, out=cx[:, 1:])
    return cx[:, wcols:wcols + cols] - cx[:, :cols]


def ssd_serial_f32(left, right, rad, lo, hi, mutant=None):
    """serial::disparitySSD (MICV_STEREO_SERIAL) -> int8.  Finite images whose window sums fit an int."""
    if mutant not in (None, "half_even", "le", "reflect101", "skip_chunk2", "wcols+1", "wcols-1"):
        raise ValueError(f"mutant {mutant}")
    L, R = _args(left, right, rad, lo, hi, F32)
    if not (np.all(np.isfinite(L)) and np.all(np.isfinite(R))):
        raise ValueError("finite images are required")
    rows, cols = L.shape
    wcols = _wcols(rad, 0, mutant)
    ncol = cols + max(wcols, 1) - 1
    Le, Re = _extended(L, R, rad, lo, hi, ncol, mutant == "reflect101")
    x = np.arange(cols)[None, :]
    best = np.full((rows, cols), 99999999, np.int64)
    disp = np.zeros((rows, cols), np.int8)
    for d in range(lo, hi + 1):
        if mutant == "skip_chunk2" and d == lo + 64:
            continue
        diff = Le - Re[:, d - lo:d - lo + ncol]  # float32
        sq = (diff * diff).astype(np.float64)    # the float32 square, held exactly
        term = np.rint(sq) if mutant == "half_even" else np.floor(sq + 0.5)  # sq >= 0: half away from zero
        cost = _box(term.astype(np.int64), rad, wcols, cols)
        if cost.max(initial=0) >= 2 ** 31:
            raise ValueError("a window sum does not fit serial::'s int")
        better = ((cost <= best) if mutant == "le" else (cost < best)) & (x + d >= -rad) & (x + d <= cols - 1 + rad)
        best[better] = cost[better]
        disp[better] = d
    return disp


def _intervals(left, right, rad, lo, hi, flags, order):
    """Yields (d, c_lo, c_hi): float64 bounds of every contract evaluation of cost(d), d ascending or descending."""
    L, R = _args(left, right, rad, lo, hi, np.float64)
    if not (np.all(np.isfinite(L)) and np.all(np.isfinite(R))):
        raise ValueError("finite images are required")
    rows, cols = L.shape
    wcols = _wcols(rad, flags, None)
    ncol = cols + wcols - 1
    Le, Re = _extended(L, R, rad, lo, hi, ncol)
    if flags & ROLLING:
        j = np.arange(rows) % STRIP
        y_lo = np.arange(rows) - j  # extended row of image row y0 - r
        k = (3 + 2 * rad + 1 + 2 * j + wcols - 1)[:, None]
        mass_f = 2.0
    else:
        y_lo, k, mass_f = None, 3 + 2 * rad + wcols - 1, 1.0
    rel = gamma(k)
    for d in (range(lo, hi + 1) if order > 0 else range(hi, lo - 1, -1)):
        diff = Le - Re[:, d - lo:d - lo + ncol]
        T = diff * diff
        C = _box(T, rad, wcols, cols)
        M = C if y_lo is None else _box(T, rad, wcols, cols, y_lo)
        # a square underflows only when 0 < |diff| < 2^-62 (the difference of two floats never does; 0^2 is exact)
        tiny = ((diff != 0) & (np.abs(diff) < 2.0 ** -62)).astype(np.float64)
        w = SAFETY * (rel * mass_f * M + mass_f * ETA * _box(tiny, rad, wcols, cols, y_lo))
        c_hi = C + w
        c_hi[~(c_hi < 2.0 ** 127)] = np.inf  # float32 may overflow on the way
        yield d, C - w, c_hi


def ssd_admissible(left, right, rad, lo, hi, flags=0):
    """The outputs any float32 evaluation of cuda::disparitySSD's contract can give (finite images).

    Returns a bool volume [hi - lo + 2, rows, cols]: plane 0 is the output -1, plane 1 + k the disparity lo + k.
    d is admissible when its lower bound is below the start value and every earlier d's upper bound (strict `<`) and
    not above any later d's upper bound; -1 is admissible where no cost's UPPER bound is below the start value (every
    cost may have failed `cost < start`; with a start of +inf only where every cost may overflow)."""
    if flags & ~(COLS_2R | MIN_SSD_5E6 | ROLLING):
        raise ValueError(f"flags {flags}")
    rows, cols = np.shape(left)
    start = 5000000.0 if flags & MIN_SSD_5E6 else np.inf
    vol = np.zeros((hi - lo + 2, rows, cols), bool)
    best_hi = np.full((rows, cols), start)  # what an earlier d (or the start value) may have left as best
    for d, c_lo, c_hi in _intervals(left, right, rad, lo, hi, flags, +1):
        vol[1 + d - lo] = c_lo < best_hi
        best_hi = np.minimum(best_hi, c_hi)
    vol[0] = best_hi >= start
    later = np.full((rows, cols), np.inf)
    for d, c_lo, c_hi in _intervals(left, right, rad, lo, hi, flags, -1):
        vol[1 + d - lo] &= c_lo <= later
        later = np.minimum(later, c_hi)
    return vol


def ssd_admits(vol, got, lo):
    """Per pixel: is `got` (the int8 output) in the admissible set?  -1 is "no match" or the disparity -1."""
    got = np.asarray(got).astype(np.int64)
    k = got - lo + 1
    inside = (k >= 1) & (k < vol.shape[0])
    hit = inside & np.take_along_axis(vol, np.clip(k, 0, vol.shape[0] - 1)[None], 0)[0]
    return hit | ((got == -1) & vol[0])
