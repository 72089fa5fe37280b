"""The "ps3: driver" block of include/mi_cv.h restated in numpy and Python integers, from the rules stated there and in
DESIGN.md section 2 ("ps3 driver"); it shares nothing with csrc/ or oracle/.

  cv_round       Point2f -> Point: halves to even, INT_MIN for NaN, +-inf and values outside int;
  line_wide      micv_viz::line's walk in unbounded integers, visiting only the steps whose major coordinate is in the
                 image: step i sits at start +- i on the major axis and at start +- (2 minor i + major - 1) // (2 major)
                 on the minor one;
  draw_segments / draw_epipolar_lines   the two entry points on a numpy view.

CASES is shared by the GPU tests and by the sanitizer build of the host loop and of the kernel's lane."""
import numpy as np

INT_MIN = -(1 << 31)
NAN, INF = float("nan"), float("inf")
SENTINEL = 0xA5
GREEN = (0.0, 255.0, 0.0, 0.0)  # CV_RGB(0, 0xFF, 0), Solution.cpp:360
ROWS, COLS = 48, 64
FAR = 2147483520.0  # 2^31 - 128, the largest float below 2^31


def cv_round(v):
    v = np.float32(v)
    if not (v >= np.float32(-2147483648.0) and v < np.float32(2147483648.0)):
        return INT_MIN
    return int(np.rint(v))


def colour_bytes(color, cn):
    out = []
    for k in range(min(cn, 4)):
        v = np.rint(np.float64(color[k])) if k < len(color) else 0.0
        out.append(0 if not v > 0 else (255 if v > 255 else int(v)))
    return out


def walk_setup(p1, p2):
    """-> (start, steep, sy, major, minor) of micv_viz::line for two integer points."""
    if p1[0] > p2[0]:
        p1, p2 = p2, p1
    dx, dy = p2[0] - p1[0], p2[1] - p1[1]
    sy = -1 if dy < 0 else 1
    dy = abs(dy)
    steep = dy > dx
    major, minor = (dy, dx) if steep else (dx, dy)
    return p1, steep, sy, major, minor


def major_range(p1, steep, sy, major, rows, cols):
    """The steps i in 0 .. major whose major coordinate lies in the image -> (lo, hi), hi < lo when there is none."""
    a, s, n = (p1[1], sy, rows) if steep else (p1[0], 1, cols)
    lo, hi = (-a, n - 1 - a) if s > 0 else (a - (n - 1), a)
    return max(lo, 0), min(hi, major)


def minor_after(minor, major, i):
    """The minor coordinate's advance after i steps: (2 minor i + major - 1) // (2 major), 0 for a single point.  Plain
    arithmetic, so that it serves Python integers of any size and (small) numpy integer arrays alike."""
    d = 2 * major
    return (2 * minor * i + major - 1) // (d + (d == 0)) * (d != 0)


def line_wide(img, p1, p2, cb):
    rows, cols = img.shape[:2]
    p1, steep, sy, major, minor = walk_setup(p1, p2)
    lo, hi = major_range(p1, steep, sy, major, rows, cols)
    for i in range(lo, hi + 1):
        m = minor_after(minor, major, i)
        x, y = (p1[0] + m, p1[1] + sy * i) if steep else (p1[0] + i, p1[1] + sy * m)
        if 0 <= x < cols and 0 <= y < rows:
            img[y, x, :len(cb)] = cb


def draw_segments(view, segments, color):
    """In place on a rows x cols x ch view; segments [n, 4] float32."""
    cb = colour_bytes(color, view.shape[2])
    for x1, y1, x2, y2 in np.asarray(segments, np.float32).reshape(-1, 4):
        line_wide(view, (cv_round(x1), cv_round(y1)), (cv_round(x2), cv_round(y2)), cb)
    return view


def draw_epipolar_lines(view, endpoints, color):
    e = np.asarray(endpoints, np.float32).reshape(-1, 6)
    return draw_segments(view, e[:, [0, 1, 3, 4]], color)


# ---------------------------------------------------------------------------------------------------------- the cases
def image(rows, cols, ch, pad):
    """(buffer rows x (cols * ch + pad) with the padding at SENTINEL, the rows x cols x ch view into it)."""
    buf = np.full((rows, cols * ch + pad), SENTINEL, np.uint8)
    y, x, c = np.mgrid[0:rows, 0:cols, 0:ch]
    view = np.ndarray((rows, cols, ch), np.uint8, buffer=buf, strides=(buf.strides[0], ch, 1))
    view[...] = (x * 7 + y * 13 + c * 29 + 5) % 251
    return buf, view


def far_crossing(n, seed, rows=ROWS, cols=COLS):
    """Segments with both ends far outside (up to the edge of int) that pass through or near the image."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        px, py = rng.uniform(0, cols), rng.uniform(0, rows)
        ang = rng.uniform(0, 2 * np.pi)
        k1, k2 = 10.0 ** rng.uniform(3, 9.3, 2)
        out.append((px - np.cos(ang) * k1, py - np.sin(ang) * k1, px + np.cos(ang) * k2, py + np.sin(ang) * k2))
    return np.clip(np.asarray(out, np.float64), -2147483648.0, FAR)


def segment_lists(rows=ROWS, cols=COLS):
    r, c = float(rows), float(cols)
    lists = {
        "axis_diag": [(3, 5, 40, 5), (7, 2, 7, 30), (2, 2, 30, 30), (30, 2, 2, 30), (60, 40, 50, 30)],
        "slopes": [(1, 1, 60, 9), (1, 20, 60, 12), (5, 1, 12, 46), (20, 46, 13, 1), (2, 40, 61, 41), (33, 3, 34, 44)],
        "right_to_left": [(50, 10, 10, 20), (50, 30, 10, 12), (40, 45, 38, 2), (40, 2, 38, 45)],
        "zero_length": [(10, 10, 10, 10), (0, 0, 0, 0), (c - 1, r - 1, c - 1, r - 1), (-3, 4, -3, 4), (c, r, c, r)],
        "halves": [(2.5, 3.5, 20.5, 9.5), (0.5, 1.5, 1.5, 0.5), (-0.5, 10, 6.5, 14.5), (30.5, 40.5, 31.5, 20.5)],
        "partly_outside": [(-10, 5, 20, 30), (50, 40, 90, 60), (30, -20, 35, 70), (-5, -5, 70, 52), (-8, 52, 70, -6), (10, -1, 50, -1 + 3)],
        "wholly_outside": [(-20, -20, -3, -1), (70, 5, 90, 40), (5, 50, 60, 60), (-5, 10, -1, 40), (0, -9, 63, -1), (64, 0, 64, 47)],
        "nonfinite": [(NAN, 5, 20, 20), (5, NAN, 20, 20), (5, 5, INF, 20), (5, 5, 20, -INF), (NAN, NAN, NAN, NAN), (-INF, 10, INF, 10),
                      (3e9, 10, 20, 10), (10, -3e9, 10, 20), (-2147483648.0, 10, 20, 10), (10, -2147483648.0, 10, 20),
                      (-2147483648.0, -2147483648.0, FAR, FAR), (20, 20, 30, 30)],
        "far_steep": [(0, -FAR, 63, FAR)],
        "far_shallow": [(-FAR, 0, FAR, 63)],
        "far_extremes": [(-2147483648.0, -2147483648.0, FAR, FAR), (-2147483648.0, FAR, FAR, -2147483648.0), (-2147483648.0, 0, FAR, 47),
                         (31, -2147483648.0, 32, FAR), (FAR, -FAR, -FAR, FAR - 128 * 40), (-FAR, 24, FAR, 24), (32, FAR, 32, -FAR),
                         (-2000000000.0, -1234567936.0, 2100000000.0, 1296000000.0), (-65536, -65537, 65535 * 30000, 65536 * 30000),
                         (-16777216, -16777215, 16777216 + 60, 16777216 + 47)],
        "n0": [],
    }
    out = {k: np.asarray(v, np.float32).reshape(-1, 4) for k, v in lists.items()}
    out["far_random"] = far_crossing(40, 303).astype(np.float32)
    rng = np.random.default_rng(304)
    out["random200"] = np.stack([rng.uniform(-30, cols + 30, 200), rng.uniform(-30, rows + 30, 200),
                                 rng.uniform(-30, cols + 30, 200), rng.uniform(-30, rows + 30, 200)], 1).astype(np.float32)
    return out


def cases():
    """(name, ch, pad, segments, colour): every list on the dense 3-channel image; the six layouts on a mixed list."""
    out = []
    sl = segment_lists()
    for name, s in sl.items():
        out.append((f"seg-{name}", 3, 0, s, GREEN))
    mixed = np.concatenate([sl[k] for k in ("axis_diag", "slopes", "halves", "partly_outside", "nonfinite", "far_steep", "far_shallow")])
    col3, col4 = (10.4, 300.0, -5.0), (0.5, 1.5, 2.5, 200.0)
    for ch in (1, 3, 4):
        for pad in (0, 7):
            for cname, col in (("c3", col3), ("c4", col4)) if ch == 4 else (("c3", col3),):
                out.append((f"layout-{ch}ch-pad{pad}-{cname}", ch, pad, mixed, col))
                out.append((f"layout-{ch}ch-pad{pad}-{cname}-random", ch, pad, sl["random200"], col))
    return out


def apply_case(case):
    """The expected buffer (padding included) of a case."""
    _, ch, pad, segments, colour = case
    buf, view = image(ROWS, COLS, ch, pad)
    draw_segments(view, segments, colour)
    return buf


def case_tokens():
    """The cases as text for tools/probes/ps3_host_loops.cpp: `case name ch pad n c0 c1 c2 c3`, then n lines of four
    float32 bit patterns in hexadecimal (NaN and inf travel as they are)."""
    lines = [f"image {ROWS} {COLS}"]
    for name, ch, pad, segments, colour in cases():
        col = list(colour) + [0.0] * (4 - len(colour))
        lines.append(f"case {name} {ch} {pad} {len(segments)} " + " ".join(repr(float(v)) for v in col))
        for s in np.asarray(segments, np.float32).reshape(-1, 4):
            lines.append(" ".join(f"{int(w):08x}" for w in s.view(np.uint32)))
    return "\n".join(lines) + "\n"
