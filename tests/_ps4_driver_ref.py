"""numpy restatement of the "ps4: driver" block of include/mi_cv.h, written from the contract ("ps4 driver"),
not from the library: drawDots, hconcat, the keypoint glyphs and the match lines, each stroke with a colour of its own.

The overlay is stated twice.  `paint_serial` is the painter: strokes in order, every pixel of a stroke stored when it
is reached, later strokes over earlier ones.  `paint_owner` is the formulation a parallel kernel can run: every pixel
belongs to the stroke of the highest priority that touches it.  tests/test_ps4_driver_ref.py holds the two against
each other on every case of the GPU tests, and shows that the cases tell the contract from its near misses (`mut`)."""
import numpy as np

import _display_ref as D
import _pf_ref as PF
import _ps1_driver_ref as P1
import _ps4_feat_ref as FR

F32 = np.float32
RED = (0, 0, 255)
MULT = 4164903690
SEED = 12345  # cv::RNG rng(12345), Solution.cpp:194, :243


# ---- cv::RNG -----------------------------------------------------------------------------------------------------

def rng_start(state):
    return int(state) if int(state) else 0xFFFFFFFF


def rng_step(state):
    return ((state & 0xFFFFFFFF) * MULT + (state >> 32)) & 0xFFFFFFFFFFFFFFFF


def colours(state, n, modulus, mut=()):
    """n colours from `state` -> ([n, 3] uint8, state after 3 n draws).  The first draw is byte 2."""
    s = rng_start(state)
    out = np.zeros((n, 3), np.uint8)
    for j in range(n):
        d = []
        for _ in range(3):
            s = rng_step(s)
            d.append((s & 0xFFFFFFFF) % modulus)
        out[j] = d if "byte_order" in mut else d[::-1]
    return out, s


def rng_jump(state, n):
    """The state after n steps, in closed form: s_n = s_0 * A^n mod (A * 2^32 - 1) (0 stands for the modulus itself)."""
    m = MULT * (1 << 32) - 1
    s = rng_start(state)
    r = s * pow(MULT, n, m) % m
    return r if r or not n else m


# ---- scalar rounding ---------------------------------------------------------------------------------------------

def cv_round(v):
    """cvRound of a float32: half to even."""
    return int(np.rint(np.float64(F32(v))))


def coord_ok(v):
    v = F32(v)
    return bool(np.isfinite(v)) and abs(float(v)) < 1e9


# ---- dots, hconcat -----------------------------------------------------------------------------------------------

def draw_dots(gray, corners, mut=()):
    base = P1.gray2rgb(gray)
    corners = np.asarray(corners, F32)
    if "dots_nonzero" in mut:
        with np.errstate(invalid="ignore"):
            mask = corners != 0
    else:
        mask = D.normalize(corners) != 0
    out = base.copy()
    out[mask] = RED
    return out


def hconcat(a, b):
    return np.concatenate([a, b], axis=1)


def to_bgr(img):
    img = np.asarray(img, np.uint8)
    return np.repeat(img[:, :, None], 3, axis=2) if img.ndim == 2 else img.copy()


# ---- strokes: a stroke is (priority, colour, xs, ys) with the pixels in walk order ----------------------------

def _walk_in(p1, p2, rows, cols):
    """P1.line_walk's pixels inside the image, in order; a walk of more than 10^5 steps goes through the closed form."""
    if max(abs(p1[0] - p2[0]), abs(p1[1] - p2[1])) > 100000:
        return P1.line_pixels_in(p1, p2, rows, cols)
    px = [(x, y) for x, y in P1.line_walk(p1, p2) if 0 <= x < cols and 0 <= y < rows]
    a = np.array(px, np.int64).reshape(-1, 2)
    return a[:, 0], a[:, 1]


def glyph_pixels(kp, rows, cols):
    """The pixels of one keypoint's glyph inside a rows x cols window, in plot order."""
    x, y, size, angle = (F32(v) for v in kp)
    half = F32(size * F32(0.5))
    if not coord_ok(x) or not coord_ok(y) or not (half >= 0 and half <= 32767):
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    cx, cy, radius = cv_round(x), cv_round(y), cv_round(half)
    xs, ys = [], []
    if radius - 1 <= abs(cx) + abs(cy) + rows + cols:
        off = np.array(P1.circle_offsets(radius), np.int64)
        px, py = cx + off[:, 0], cy + off[:, 1]
        keep = (px >= 0) & (px < cols) & (py >= 0) & (py < rows)
        xs.append(px[keep])
        ys.append(py[keep])
    if angle != F32(-1) and coord_ok(angle):
        s, c = FR.sincos_deg(angle)
        ex, ey = cx + cv_round(F32(c) * F32(radius)), cy + cv_round(F32(s) * F32(radius))
        lx, ly = _walk_in((cx, cy), (ex, ey), rows, cols)
        xs.append(lx)
        ys.append(ly)
    if not xs:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(xs), np.concatenate(ys)


def paint_serial(img, strokes, mut=()):
    out = img.copy()
    if "first_writer" in mut:
        done = np.zeros(img.shape[:2], bool)
        for _, colour, xs, ys in strokes:
            for x, y in zip(xs, ys):
                if not done[y, x]:
                    out[y, x] = colour
                    done[y, x] = True
        return out
    for _, colour, xs, ys in strokes:
        for x, y in zip(xs, ys):
            out[y, x] = colour
    return out


def paint_owner(img, strokes):
    owner = np.zeros(img.shape[:2], np.int64)
    table = {}
    for prio, colour, xs, ys in strokes:
        table[prio + 1] = colour
        np.maximum.at(owner, (ys, xs), prio + 1)
    out = img.copy()
    for tag, colour in table.items():
        out[owner == tag] = colour
    return out


# ---- the entries -------------------------------------------------------------------------------------------------

def glyph_strokes(kp, n, cap, rows, cols, state, mut=()):
    n = max(0, min(int(n), int(cap)))
    col, state = colours(state, n, 256, mut)
    return [(j, col[j]) + glyph_pixels(kp[j], rows, cols) for j in range(n)], state


def draw_keypoints(canvas, x0, cols, src, kp, n, state, cap=None, owner=False, mut=()):
    """-> (canvas copy with the window drawn, state after).  src None keeps the window's content."""
    out = canvas.copy()
    rows = canvas.shape[0]
    kp = np.asarray(kp, F32).reshape(-1, 4)
    win = to_bgr(src) if src is not None else out[:, x0:x0 + cols].copy()
    wcols = canvas.shape[1] - x0 if "bleed" in mut else cols
    if "bleed" in mut:
        wide = out[:, x0:].copy()
        wide[:, :cols] = win
        win = wide
    strokes, state = glyph_strokes(kp, n, len(kp) if cap is None else cap, rows, wcols, state, mut)
    win = paint_owner(win, strokes) if owner else paint_serial(win, strokes, mut)
    out[:, x0:x0 + win.shape[1]] = win
    return out, state


def line_strokes(rows, cols, kp_a, kp_b, matches, n, mask=None, x_offset=0, seed=SEED, cap=None, mut=()):
    kp_a, kp_b = np.asarray(kp_a, F32).reshape(-1, 4), np.asarray(kp_b, F32).reshape(-1, 4)
    matches = np.asarray(matches, np.int64).reshape(-1, 2)
    n = max(0, min(int(n), len(matches) if cap is None else int(cap)))
    drawn = [i for i in range(n) if (mask is None or mask[i]) and 0 <= matches[i, 0] < len(kp_a) and 0 <= matches[i, 1] < len(kp_b)]
    ncol = n if "rank_is_index" in mut else len(drawn)
    col, _ = colours(seed, ncol, 256 if "mod256" in mut else 255, mut)
    strokes = []
    for r, i in enumerate(drawn):
        a, b = kp_a[matches[i, 0]], kp_b[matches[i, 1]]
        x1, y1, x2, y2 = a[0], a[1], F32(b[0] + F32(x_offset)), b[1]
        c = col[i if "rank_is_index" in mut else r]
        if all(coord_ok(v) for v in (x1, y1, x2, y2)):
            xs, ys = _walk_in((cv_round(x1), cv_round(y1)), (cv_round(x2), cv_round(y2)), rows, cols)
        else:
            xs = ys = np.zeros(0, np.int64)
        strokes.append((r, c, xs, ys))
    return strokes


def draw_match_lines(canvas, kp_a, kp_b, matches, n, mask=None, x_offset=0, seed=SEED, cap=None, owner=False, mut=()):
    strokes = line_strokes(canvas.shape[0], canvas.shape[1], kp_a, kp_b, matches, n, mask, x_offset, seed, cap, mut)
    return paint_owner(canvas, strokes) if owner else paint_serial(canvas, strokes, mut)


def match_panels(img_a, img_b, kp_a, n_a, kp_b, n_b, matches, n, mask=None, glyphs=True, seed=SEED, state=0, owner=False, mut=()):
    """-> (keypoint panel, match panel, state after)."""
    canvas = hconcat(to_bgr(img_a), to_bgr(img_b))
    ca, cb = img_a.shape[1], img_b.shape[1]
    if glyphs and "glyphs_over_lines" not in mut:
        canvas, state = draw_keypoints(canvas, 0, ca, None, kp_a, n_a, state, owner=owner, mut=mut)
        canvas, state = draw_keypoints(canvas, ca, cb, None, kp_b, n_b, state, owner=owner, mut=mut)
    lines = draw_match_lines(canvas, kp_a, kp_b, matches, n, mask, ca, seed, owner=owner, mut=mut)
    if glyphs and "glyphs_over_lines" in mut:
        canvas, state = draw_keypoints(canvas, 0, ca, None, kp_a, n_a, state, owner=owner)
        canvas, state = draw_keypoints(canvas, ca, cb, None, kp_b, n_b, state, owner=owner)
        lines, _ = draw_keypoints(lines, 0, ca, None, kp_a, n_a, 0, owner=owner)
        lines, _ = draw_keypoints(lines, ca, cb, None, kp_b, n_b, rng_jump(0, 3 * min(int(n_a), len(kp_a))), owner=owner)
    return canvas, lines, state


# ---- the cases the CPU and the GPU tests share -----------------------------------------------------------------------

ROWS, CA, CB = 37, 41, 29


def pair_images(rows=ROWS, ca=CA, cb=CB):
    yy, xx = np.mgrid[0:rows, 0:ca + cb]
    g = ((xx * 5 + yy * 3) % 200 + 20).astype(np.uint8)
    return np.ascontiguousarray(g[:, :ca]), np.ascontiguousarray(g[:, ca:])


def keypoint_cases():
    """name -> (rows, cols, kp [n, 4]) on one window."""
    r, c = ROWS, CA
    return {
        "borders": (r, c, [[0, 10, 10, 30], [c - 1, 12, 10, 200], [20, 0, 10, 90], [17, r - 1, 10, 271], [c - 1, r - 1, 10, 45]]),
        "sizes": (r, c, [[8, 8, 0, 10], [20, 8, 5, 100], [30, 20, 10, 250], [12, 25, 10, -1], [25, 28, 5, -1], [6, 30, 0, -1]]),
        "same_pixel": (r, c, [[20, 18, 10, 33], [20, 18, 10, 213], [20.4, 18.4, 5, 33]]),
        "through_one_pixel": (r, c, [[20, 18, 20, 0], [10, 18, 20, 0], [15, 13, 10, 90]]),
        "through_one_pixel_reversed": (r, c, [[15, 13, 10, 90], [10, 18, 20, 0], [20, 18, 20, 0]]),
        "odd_values": (r, c, [[np.nan, 5, 10, 0], [5, np.inf, 10, 0], [5, 5, np.nan, 0], [9, 9, 10, np.nan], [9, 20, -3, 0],
                              [2e9, 5, 10, 0], [30, 30, 10, 1e12], [15, 15, 70000, 0], [-40, 18, 100, 0], [20.5, 10.5, 7, 720.5]]),
        "one_row": (1, 23, [[3, 0, 6, 0], [10, 0, 4, 90], [22, 0, 10, 180]]),
        "one_col": (23, 1, [[0, 3, 6, 0], [0, 10, 4, 90], [0, 22, 10, 180]]),
        "many": (r, c, _many_keypoints(300, r, c, 7)),
    }


def _many_keypoints(n, rows, cols, seed):
    g = np.random.RandomState(seed)
    kp = np.zeros((n, 4), F32)
    kp[:, 0] = g.uniform(-3, cols + 3, n)
    kp[:, 1] = g.uniform(-3, rows + 3, n)
    kp[:, 2] = g.choice([0, 5, 10, 10, 10, 17], n)
    kp[:, 3] = np.where(g.rand(n) < 0.15, -1, g.uniform(0, 360, n))
    return kp


def line_cases():
    """name -> (kp_a, kp_b, matches, mask or None, x_offset) on the ROWS x (CA + CB) canvas."""
    def kps(pts):
        return [[x, y, 10, 0] for x, y in pts]
    out = {}
    a = kps([(2, 3), (40, 3), (5, 36), (5, 0), (20, 20), (20, 20), (0, 18), (33, 7)])
    b = kps([(25, 3), (3, 3), (5, 0), (5, 36), (-21, 20), (7, 20), (28, 18), (-8, 32)])
    out["shapes"] = (a, b, [[i, i] for i in range(8)], None, CA)  # horizontal x 2, vertical x 2, zero length, ..., diagonal 25
    out["crossing"] = (kps([(2, 2), (2, 34), (2, 18)]), kps([(27, 34), (27, 2), (27, 18)]), [[0, 0], [1, 1], [2, 2]], None, CA)
    out["crossing_reversed"] = (kps([(2, 18), (2, 34), (2, 2)]), kps([(27, 18), (27, 2), (27, 34)]), [[0, 0], [1, 1], [2, 2]], None, CA)
    out["out_of_range"] = (kps([(2, 2), (2, 30), (9, 9)]), kps([(20, 30), (20, 2)]),
                           [[0, 0], [3, 0], [1, 1], [0, 2], [-1, 0], [2, -1], [2, 1]], None, CA)
    out["odd_values"] = (kps([(np.nan, 2), (2, 30), (3e9, 1), (9, 9)]), kps([(20, 30), (20, np.inf), (4, 4)]),
                         [[0, 0], [1, 0], [1, 1], [2, 2], [3, 2]], None, CA)
    out["outside"] = (kps([(-500, -300), (-100, 18), (20, -5000)]), kps([(900, 700), (300, 18), (-21, 90000)]), [[0, 0], [1, 1], [2, 2]], None, CA)
    for n in (0, 1, 63, 64, 65, 300):
        g = np.random.RandomState(100 + n)
        ka = np.c_[g.uniform(0, CA, 40), g.uniform(0, ROWS, 40), np.full(40, 10.0), np.zeros(40)]
        kb = np.c_[g.uniform(0, CB, 50), g.uniform(0, ROWS, 50), np.full(50, 10.0), np.zeros(50)]
        m = np.c_[g.randint(0, 40, n), g.randint(0, 50, n)].reshape(-1, 2)
        out[f"n{n}"] = (ka, kb, m, None, CA)
        mask = (g.rand(n) < 0.6).astype(np.uint8)
        if n > 64:
            mask[[62, 63, 64]] = [1, 0, 1]
        if n > 200:
            mask[[126, 127, 128, 129, 191, 192]] = [0, 1, 1, 0, 1, 1]
        out[f"n{n}_masked"] = (ka, kb, m, mask, CA)
    return out


def long_line_case():
    """A canvas wide enough for strokes of more than 64 and more than 128 steps."""
    rows, cols = 9, 300
    a = [[1, 1, 10, 0], [2, 7, 10, 0], [290, 4, 10, 0]]
    b = [[70, 6, 10, 0], [200, 0, 10, 0], [3, 4, 10, 0]]
    return rows, cols, a, b, [[0, 0], [1, 1], [2, 2]]


def dots_cases():
    r, c = 11, 13
    g = np.random.RandomState(5)
    gray = g.uniform(-20, 300, (r, c)).astype(F32)
    gray[0, :4] = [np.nan, np.inf, -np.inf, 254.5]

    def sparse(entries, fill=0.0):
        m = np.full((r, c), fill, F32)
        for y, x, v in entries:
            m[y, x] = v
        return m
    return {
        "weak_beside_strong": (gray, sparse([(2, 2, 1000.0), (2, 3, 1.9), (5, 5, 2.0), (7, 7, 1.95), (7, 8, 1.97), (9, 1, 400.0)])),
        "negative": (gray, sparse([(2, 2, 10.0), (4, 4, -3.0), (8, 8, 1e-3)])),
        "all_equal": (gray, sparse([], 7.5)),
        "all_zero": (gray, sparse([])),
        "nan": (gray, sparse([(1, 1, np.nan), (3, 3, 5.0), (6, 6, 0.004), (6, 7, np.nan)])),
        "u8": (np.clip(np.nan_to_num(gray, nan=7.0), 0, 255).astype(np.uint8), sparse([(0, 0, 3.0), (10, 12, 9.0)])),
    }
