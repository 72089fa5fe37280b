"""The case table of disparitySSD's float kernels, shared by tests/test_stereo_f32_ref.py (CPU: the references against the
C oracle, the integer reference, the float64 bounds and the mutants) and tests/test_stereo_float_paths_gpu.py (the
kernels against the references).  One row = one call: path family, radius, flags, rows-per-wave option, the routes
that reach the kernel, shape, row pad, disparity range, image kind, seed.

Families (csrc/stereo_float.hpp, csrc/stereo.hip):
  tile            stereo_tile<R, ST_SSD, RPW>          R 1..10, full and COLS_2R windows, RPW 8 and 10
  serial_tile     stereo_tile<R, ST_SSD_SERIAL, RPW>   R 1..10
  generic         stereo_generic_kernel<ST_SSD>        r 0, 11, 15, 31, flags 0..3
  serial_generic  stereo_generic_kernel<ST_SSD_SERIAL> r 0, 11, 15, 31
  rolling         stereo_rolling_kernel<false>         r 0, 2, 7, 10, 11, 31, +- COLS_2R, +- MIN_SSD_5E6
Through the table rotate: disparity spans 0, 63, 64, 65, 128, 255 (the edges of the 64-disparity staging chunks) placed
below 0, above 0 or across it; rows around the 4 x RPW rows of a workgroup and the 40-row strip; columns around the
window and the 64 - 2r outputs of a wave (ROLLING: odd and even numbers of such segments, two waves per workgroup); a row
pad of 0 or 3 elements; image kinds.  Ranges lie next to 0, so that the planted disparity of the textured kinds and the
candidates around it are on the image.  Where a form's turn in the rotation is degenerate -- an image no wider than the
window, a handful of rows, a single disparity, or a clear match that answers one value nearly everywhere -- the form gets
a second, wide case (near ties for the cuda:: path), so that every form has an answer far from constant
(tests/test_stereo_f32_ref.py asserts it).  Nothing is larger than 131 x 260."""
from collections import namedtuple

import numpy as np

from test_f64_ref import image

COLS_2R, MIN_SSD_5E6, SERIAL, ROLLING = 1, 2, 4, 8

Case = namedtuple("Case", "id family rad flags rpw routes rows cols pad lo hi kind seed")

SPANS = (0, 63, 64, 65, 128, 255)
ROWS = (1, 7, 8, 9, 31, 32, 33, 39, 40, 41)
ROWS_ROLLING = ROWS + (81, 131)
FLOAT_KINDS = ("uniform", "normal", "neartie", "dyadic", "u8")      # cuda:: path tiles and generic
SERIAL_KINDS = ("uniform", "dyadic", "halfway", "neartie", "u8")    # ("normal": sums pass serial::'s int)
ROLLING_KINDS = ("uniform", "normal", "spikes", "neartie")
CLEAR_KINDS = ("uniform", "normal", "u8", "dyadic")  # a planted shift: one clear minimum at most pixels
FINITE_FLOAT_KINDS = ("uniform", "normal", "neartie", "dyadic", "spikes", "threshold", "threshold_below", "equal")


def exact_covers(rad, flags):
    """stereo_exact_covers(): the calls whose float tiles ride behind the exact-sum launch on a default context."""
    if flags & ROLLING or not 1 <= rad <= 7:
        return False
    if flags & SERIAL:
        return rad <= 5
    return not (flags & COLS_2R and rad < 2)


def cols_for(family, r, k):
    outw = 64 - 2 * r
    if family in ("generic", "serial_generic"):  # one thread per pixel, 64 columns per workgroup
        return (1, max(1, 2 * r), 2 * r + 1, 63, 64, 65, 129)[k % 7]
    if family == "rolling" and outw < 8:  # (r = 31: two outputs per wave; widths as for the generic kernel, 1..65 segments)
        return (1, 2 * r, 2 * r + 1, 63, 64, 65, 129, 130)[k % 8]
    if family == "rolling":  # 1, 2, 3 (a workgroup with one idle wave) and 4 segments of 64 - 2r outputs
        return (1, 2 * r + 1, max(1, outw - 1), outw, outw + 1, 2 * outw + 1, 4 * outw - 1, 3 * outw)[k % 8]
    return (1, 2 * r, 2 * r + 1, outw - 1, outw, outw + 1, 2 * outw + 1)[k % 7]


def _u8_top(rad):
    """The largest pixel value whose (2r+1)^2 window sums stay below 2^24: exact in float32 in any order."""
    return min(255, int(np.sqrt(2.0 ** 24 / (2 * rad + 1) ** 2)) - 1)


def _halfway_values():
    """float32 values v with fl(v * v) == k + 0.5 exactly, found by search around sqrt(k + 0.5): {k: v}."""
    out = {}
    for k in range(0, 200):
        t = np.float32(k + 0.5)
        v = np.float32(np.sqrt(np.float64(t)))
        for _ in range(4):
            v = np.nextafter(v, np.float32(0))
        for _ in range(9):
            if np.float32(v * v) == t:
                out[k] = v
                break
            v = np.nextafter(v, np.float32(np.inf))
    return out


HALFWAY = _halfway_values()
assert sum(k % 2 == 0 for k in HALFWAY) >= 4 and sum(k % 2 == 1 for k in HALFWAY) >= 4, sorted(HALFWAY)


def planted_shift(c):
    """The true disparity of the textured kinds: the one in range nearest -5 (inside the image for most pixels), but not
    the first of the range, which is also what a search that ignores d returns."""
    return min(max(-5, c.lo + min(2, c.hi - c.lo)), c.hi)


def match_on_image(c):
    """Columns [cols] at which the planted match of a textured pair (column x + shift) lies on the image.  Elsewhere the
    pair holds no true minimum: the best candidates fetch clamped edge columns, and those that lie wholly off the image
    cost the same."""
    x = np.arange(c.cols) + planted_shift(c)
    return (x >= 0) & (x <= c.cols - 1)


def _shifted(left, other, shift):
    """right(y, x) = left(y, x - shift), but for unrelated values at every seventh column of every third row: every
    window has a true minimum at d = shift whose cost is well above zero (1 term in 21), so that neither a candidate
    that lies off the image -- all of those cost the same -- nor rounding decides."""
    right = np.ascontiguousarray(np.roll(left, shift, axis=1))
    right[::3, ::7] = other[::3, ::7]
    return right


def make_pair(c):
    """(left, right), float32 [rows, cols], of a case."""
    rng = np.random.default_rng(c.seed)
    rows, cols, kind = c.rows, c.cols, c.kind
    shift = planted_shift(c)
    wcols = 2 * c.rad if c.flags & COLS_2R else 2 * c.rad + 1
    nrep = max(1.0, (2 * c.rad + 1) * wcols / 21.0)  # unrelated terms in a window of a textured pair
    gain = None
    if kind in ("uniform", "normal"):
        left = image(c.seed, rows, cols, kind)
        right = _shifted(left, image(c.seed + 1, rows, cols, kind), shift)
        gain = 5e6 / (nrep * (2 * 255.0 ** 2 / 12 if kind == "uniform" else 2e6))
    elif kind == "u8":
        top = _u8_top(c.rad)
        left = rng.integers(0, top + 1, (rows, cols)).astype(np.float32)
        right = _shifted(left, rng.integers(0, top + 1, (rows, cols)).astype(np.float32), shift)
        if c.flags & MIN_SSD_5E6:  # a dark half against a bright one
            right[:, cols // 2:] = top - right[:, cols // 2:]
    elif kind == "dyadic":  # multiples of 1/4 in 0..8: squares are multiples of 1/16, every sum exact
        left = (rng.integers(0, 33, (rows, cols)) / 4).astype(np.float32)
        right = _shifted(left, (rng.integers(0, 33, (rows, cols)) / 4).astype(np.float32), shift)
    elif kind == "neartie":
        # two unrelated images of period 8 in x, each pixel then moved by -2..2 ulp: cost(d) and cost(d + 8) are equal
        # but for the jitter, so candidates lie within a few ulp of each other and the order of the additions decides
        def periodic():
            base = np.tile((rng.random((rows, 8)) * 255).astype(np.float32), (1, cols // 8 + 1))[:, :cols]
            return (base * (1 + rng.integers(-2, 3, (rows, cols)) * 2.0 ** -23)).astype(np.float32)
        left, right = periodic(), periodic()
        gain = 5e6 / ((2 * c.rad + 1) * wcols * 2 * 255.0 ** 2 / 12)
    elif kind == "halfway":
        # serial::'s terms exactly k + 1/2, even and odd k: zero against planted values, top half in `right`, bottom
        # half in `left` (rows whose windows span the seam mix both)
        vals = np.array([0.0, 0.0, 1.0] + [HALFWAY[k] for k in sorted(HALFWAY)[:12]], np.float32)
        planted = vals[rng.integers(0, len(vals), (rows, cols))]
        top_half = (np.arange(rows) < max(1, rows // 2))[:, None]
        left = np.where(top_half, 0, planted).astype(np.float32)
        right = np.where(top_half, planted, 0).astype(np.float32)
    elif kind == "spikes":
        # a few pixels near 1e4 among 0..255 (a periodic pair, so that candidates lie close): while one is inside the
        # window the column sum is ~1e8 (ulp 8); a rolled sum keeps that rounding for the rest of its strip, a fresh
        # one does not
        def spiked():
            img = np.tile((rng.random((rows, 8)) * 255).astype(np.float32), (1, cols // 8 + 1))[:, :cols].copy()
            hit = rng.random((rows, cols)) < 0.004
            img[hit] = (1e4 * (1 + rng.random(int(hit.sum())))).astype(np.float32)
            return img
        left, right = spiked(), spiked()
    elif kind in ("threshold", "threshold_below"):  # r = 2, COLS_2R: 20 terms of 500^2 = exactly 5 000 000
        left = np.full((rows, cols), 500.0 if kind == "threshold" else 499.75, np.float32)
        right = np.zeros((rows, cols), np.float32)
    elif kind == "equal":  # every cost exactly 0: the first disparity, and only it (`<=` would take the last)
        left = np.full((rows, cols), 77.25, np.float32)
        right = left.copy()
    elif kind in ("nonfinite", "allnan"):
        left = image(c.seed, rows, cols, "uniform")
        right = _shifted(left, image(c.seed + 1, rows, cols, "uniform"), shift)
        if kind == "allnan":
            left[:] = np.nan
        else:
            left[rows // 3, cols // 4] = np.nan
            right[rows // 2, cols // 2] = np.inf
            left[(2 * rows) // 3, (3 * cols) // 4] = -np.inf
            right[rows - 1, 0] = -np.inf  # a clamped corner: reached by every window left of / below the image
    else:
        raise ValueError(kind)
    if gain is not None and c.flags & MIN_SSD_5E6:  # costs on either side of 5e6
        g = np.float32(np.sqrt(gain))
        left, right = left * g, right * g
    return np.ascontiguousarray(left, np.float32), np.ascontiguousarray(right, np.float32)


def _build():
    cases = []

    def place(i, span, rng):
        """[lo, lo + span] across 0, wholly below or wholly above it in turn, always next to 0: the planted shift
        (make_pair) and the candidates around it then lie inside all but the narrowest images."""
        where = i % 3
        if where == 1 and -4 - span >= -128:
            hi = -int(rng.integers(1, 3))
            return hi - span, hi
        if where == 2 and 4 + span <= 127:
            lo = int(rng.integers(1, 3))
            return lo, lo + span
        lo = -(span * int(rng.integers(1, 4)) // 4)
        if span >= 5:
            lo = min(lo, -5)
        lo = max(-128, min(lo, 127 - span))
        return lo, lo + span

    turns = {}  # family -> rotated cases so far: the rotations below do not depend on what other families hold

    def add(family, rad, flags, rpw, kind, rows=None, cols=None, lo=None, hi=None, routes=None, pad=None, wide=False):
        i = len(cases)
        rng = np.random.default_rng(77000 + i)
        rotated = lo is None and rows is None and cols is None
        n = turns.get(family, 0)
        if rotated and not wide:
            turns[family] = n + 1
        if lo is None:
            span = SPANS[(n + n // 6) % 6]  # (full and COLS_2R forms alternate: each meets every span)
            if wide:
                span = (63, 64, 65, 128)[n % 4]
                flags &= ~MIN_SSD_5E6  # (no template argument; with it the answer is little more than -1 or the shift)
                if kind in CLEAR_KINDS:
                    kind = "neartie"  # a clear match answers the shift nearly everywhere: let the search decide more
            lo, hi = place(n + wide, span, rng)
        if rows is None:
            table = ROWS_ROLLING if family == "rolling" else ROWS
            rows = (31, 32, 33, 39, 40, 41)[n % 6] if wide else table[(n * 7 + n // len(table)) % len(table)]
        if cols is None:
            cols = cols_for(family, rad, n * 4 + n // 7)
            if wide:
                cols = max(cols_for(family, rad, k) for k in (n % 3 + 3, 5))  # one of the three widest, never narrow
        if pad is None:
            pad = 3 * ((n + n // 2) % 2)
        if routes is None:
            routes = ("float",) + (("default",) if exact_covers(rad, flags) else ()) + (("host",) if i % 9 == 4 else ())
        cid = f"{i:03d}-{family}-r{rad}-f{flags}-rpw{rpw}-{kind}-{rows}x{cols}p{pad}-d{lo}_{hi}"
        cases.append(Case(cid, family, rad, flags, rpw, routes, rows, cols, pad, lo, hi, kind, 5000 + i))
        # a form whose turn in the rotation is degenerate (an image no wider than the window, a handful of pixels, a
        # single disparity) gets a second case on which the search has something to decide
        if rotated and not wide and (cols <= 2 * rad + 1 or rows < 16 or rows * cols < 400 or hi - lo < 8 or kind in CLEAR_KINDS):
            add(family, rad, flags, rpw, kind, wide=True)

    for rpw in (8, 10):
        for rad in range(1, 11):
            for w in (0, COLS_2R):
                i = len(cases)
                add("tile", rad, w | (MIN_SSD_5E6 if i % 3 == 1 else 0), rpw, FLOAT_KINDS[i % 5])
            add("serial_tile", rad, SERIAL, rpw, SERIAL_KINDS[len(cases) % 5])
    for k, rad in enumerate((0, 11, 15, 31)):
        for flags in range(4):
            if not (flags & COLS_2R and rad == 0):
                add("generic", rad, flags, 8, FLOAT_KINDS[len(cases) % 5])
        for n in (0, 3):  # (the table's own rotation would hand every one of these the same kind)
            add("serial_generic", rad, SERIAL, 8, SERIAL_KINDS[(k + n) % 5])
    for rad in (0, 2, 7, 10, 11, 31):
        for flags in range(4):
            if not (flags & COLS_2R and rad == 0):
                # (r = 0: a one-term cost lies far below a rolled sum's error bound -- no textured pair for the 5 % cap)
                add("rolling", rad, flags | ROLLING, 8, ROLLING_KINDS[len(cases) % 4 if rad else 2 + len(cases) % 2])
    # near ties for every radius group of every family: the order of the additions decides (the association mutants)
    for family, rad, flags, rpw in (("tile", 1, 0, 8), ("tile", 4, COLS_2R, 10), ("tile", 7, 0, 8), ("tile", 9, 0, 10),
                                    ("tile", 10, COLS_2R, 8), ("generic", 11, 0, 8), ("generic", 15, COLS_2R, 8),
                                    ("rolling", 2, ROLLING, 8), ("rolling", 10, ROLLING | COLS_2R, 8)):
        add(family, rad, flags, rpw, "neartie", rows=37, cols=150, lo=-20, hi=12)
    # uniform / normal pairs across a chunk edge at one size: the non-singleton share of the float64 sets is measured here
    for family, rad, flags, rpw, kind in (("tile", 1, 0, 8, "uniform"), ("tile", 4, 0, 10, "normal"), ("tile", 7, COLS_2R, 8, "uniform"),
                                          ("tile", 10, 0, 10, "normal"), ("generic", 11, 0, 8, "uniform"),
                                          ("rolling", 4, ROLLING, 8, "normal"), ("rolling", 11, ROLLING | COLS_2R, 8, "uniform")):
        add(family, rad, flags, rpw, kind, rows=37 if family != "rolling" else 81, cols=150, lo=-70, hi=3)
    # ROLLING's memory: spikes that leave the window stay in a rolled sum's rounding
    for rad, flags in ((2, ROLLING), (7, ROLLING | COLS_2R), (11, ROLLING), (31, ROLLING | MIN_SSD_5E6)):
        add("rolling", rad, flags, 8, "spikes", rows=81 if rad < 31 else 41, cols=131, lo=-12, hi=9)
    # serial::'s rounding: terms exactly halfway
    for family, rad, rpw in (("serial_tile", 2, 8), ("serial_tile", 6, 10), ("serial_tile", 10, 8), ("serial_generic", 11, 8),
                             ("serial_generic", 0, 8)):
        add(family, rad, SERIAL, rpw, "halfway", rows=33, cols=90, lo=-70, hi=20)
    # MIN_SSD_5E6 at a cost of exactly 5 000 000 (nothing found) and just below it (everything found)
    for family, flags in (("tile", 3), ("rolling", 3 | ROLLING)):
        for kind in ("threshold", "threshold_below"):
            add(family, 2, flags, 8, kind, rows=9, cols=70, lo=-5, hi=5, routes=("float", "default", "host"))
    # exact ties at cost 0
    for family, rad, flags, rpw in (("tile", 3, 0, 10), ("generic", 11, COLS_2R, 8), ("rolling", 2, ROLLING | MIN_SSD_5E6, 8)):
        add(family, rad, flags, rpw, "equal", rows=33, cols=70, lo=-70, hi=9)
    # NaN and infinities (cuda:: path only): a NaN cost never wins; an all-NaN image finds nothing
    for family, rad, flags, rpw in (("tile", 3, 0, 8), ("tile", 8, COLS_2R | MIN_SSD_5E6, 10), ("generic", 11, 0, 8),
                                    ("rolling", 2, ROLLING, 8)):
        for kind in ("nonfinite", "allnan"):
            add(family, rad, flags, rpw, kind, rows=41, cols=70, lo=-70, hi=9)
    return cases


CASES = _build()
FAMILIES = ("tile", "serial_tile", "generic", "serial_generic", "rolling")
