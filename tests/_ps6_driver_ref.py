"""The ps6 driver's overlay restated in numpy, twice: the dots of ParticleFilter::drawParticles (shim/micv_shim.hpp) and the
ring of micv_viz::rectangle (shim/micv_viz.hpp) around the driver's box (ps6_cpp/src/Solution.cpp:73-78).

  paint_loop       the painter: a loop over the particles (centre and four neighbours), then the four strokes of the ring
                   as micv_viz::line walks them, in Python integers;
  paint_predicate  per pixel: the ring's closed-form predicate decides first, then "some kept particle's centre lies
                   within Manhattan distance 1", from a count plane and its four shifts.

Both take `mut`, a set of deliberate mistakes (MUTATIONS); test_ps6_driver_ref.py checks that the two agree on every case
and that each mistake changes at least one.  CASES is shared with the GPU tests and with the sanitizer build of the host
loops."""
import numpy as np

INT_MIN = -(1 << 31)
NAN, INF = float("nan"), float("inf")
MUTATIONS = ("ring_first", "half_away", "margin_1", "br_not_reduced", "int_half")
SENTINEL = 0xA5
DOT, BOX = (0.0, 255.0, 0.0, 0.0), (255.0, 0.0, 255.0, 0.0)  # Solution.cpp:74, :78


def cv_round(v, away=False):
    """The project's cvRound of a float32: half to even; INT_MIN for NaN, +-inf and values outside int."""
    v = np.float32(v)
    if not (v >= np.float32(-2147483648.0) and v < np.float32(2147483648.0)):
        return INT_MIN
    if away:
        return int(np.sign(v) * np.floor(np.abs(np.float64(v)) + 0.5))
    return int(np.rint(v))


def box_rect(centre, size, mut=()):
    """cv::Rect(Point2f(c.x - w / 2, c.y - h / 2), Size2f(w, h)) -> (x, y, w, h); the arithmetic in float32."""
    away = "half_away" in mut
    w, h = np.float32(size[0]), np.float32(size[1])
    if "int_half" in mut:
        hw, hh = np.trunc(w / np.float32(2)), np.trunc(h / np.float32(2))
    else:
        hw, hh = w / np.float32(2), h / np.float32(2)
    with np.errstate(invalid="ignore", over="ignore"):
        x, y = np.float32(centre[0]) - hw, np.float32(centre[1]) - hh
    return cv_round(x, away), cv_round(y, away), cv_round(w, away), cv_round(h, away)


def colour_bytes(color, cn):
    out = []
    for k in range(min(cn, 4)):
        v = np.rint(np.float64(color[k])) if k < len(color) else 0.0
        out.append(0 if not v > 0 else (255 if v > 255 else int(v)))
    return out


def _kept_centres(particles, rows, cols, mut):
    """Integer centres of the particles that pass the margin test, in order."""
    m = np.float32(1.0 if "margin_1" in mut else 2.0)
    out = []
    for px, py in np.asarray(particles, np.float32).reshape(-1, 2):
        if not (px > -m and px < np.float32(cols) + m and py > -m and py < np.float32(rows) + m):
            continue
        if "half_away" in mut:
            out.append((cv_round(px, True), cv_round(py, True)))
        else:
            out.append((int(np.rint(px)), int(np.rint(py))))
    return out


def _line(img, p1, p2, cb):
    """micv_viz::line: cv::LineIterator's walk, left to right, every pixel bounds-checked."""
    rows, cols = img.shape[:2]
    if p1[0] > p2[0]:
        p1, p2 = p2, p1
    dx, dy = p2[0] - p1[0], p2[1] - p1[1]
    sy = -1 if dy < 0 else 1
    dy = abs(dy)
    steep = dy > dx
    major, minor = (dy, dx) if steep else (dx, dy)
    err, x, y = major - 2 * minor, p1[0], p1[1]
    for _ in range(major + 1):
        if 0 <= x < cols and 0 <= y < rows:
            img[y, x, :len(cb)] = cb
        both = err < 0
        err += 2 * major - 2 * minor if both else -2 * minor
        if steep:
            y += sy
            x += 1 if both else 0
        else:
            x += 1
            y += sy if both else 0


def _clip(a, b, n):
    """An axis-parallel stroke's extent cut to 0 .. n - 1 (the walk visits the same in-image pixels)."""
    lo, hi = max(min(a, b), 0), min(max(a, b), n - 1)
    return (lo, hi) if lo <= hi else None


def _ring_loop(img, rect, cb, mut):
    x, y, w, h = rect
    if w <= 0 or h <= 0:
        return
    rows, cols = img.shape[:2]
    red = 0 if "br_not_reduced" in mut else 1
    x1, y1 = x + w - red, y + h - red
    for (ax, ay), (bx, by) in (((x, y), (x1, y)), ((x1, y), (x1, y1)), ((x1, y1), (x, y1)), ((x, y1), (x, y))):
        if ay == by:
            c = _clip(ax, bx, cols)
            if c and 0 <= ay < rows:
                _line(img, (c[0], ay), (c[1], ay), cb)
        else:
            c = _clip(ay, by, rows)
            if c and 0 <= ax < cols:
                _line(img, (ax, c[0]), (ax, c[1]), cb)


def _as3(img):
    return img.reshape(img.shape[0], img.shape[1], -1)


def paint_loop(img, particles, dot, rect, box, mut=()):
    """The painter, on a copy.  img: rows x cols (x ch) uint8; rect None: no ring; particles None: no dots."""
    out = _as3(img.copy())
    rows, cols, ch = out.shape

    def dots():
        if particles is None:
            return
        cb = colour_bytes(dot, ch)
        for cx, cy in _kept_centres(particles, rows, cols, mut):
            for ox, oy in ((0, 0), (-1, 0), (1, 0), (0, -1), (0, 1)):
                x, y = cx + ox, cy + oy
                if 0 <= x < cols and 0 <= y < rows:
                    out[y, x, :len(cb)] = cb

    def ring():
        if rect is not None:
            _ring_loop(out, rect, colour_bytes(box, ch), mut)

    for step in ((ring, dots) if "ring_first" in mut else (dots, ring)):
        step()
    return out.reshape(img.shape)


def paint_predicate(img, particles, dot, rect, box, mut=()):
    """Per pixel: on the ring -> box; else within Manhattan distance 1 of a kept centre -> dot; else the image."""
    out = _as3(img.copy())
    rows, cols, ch = out.shape
    yy, xx = np.mgrid[0:rows, 0:cols]
    on_ring = np.zeros((rows, cols), bool)
    if rect is not None and rect[2] > 0 and rect[3] > 0:
        red = 0 if "br_not_reduced" in mut else 1
        x0, y0 = rect[0], rect[1]
        x1, y1 = x0 + rect[2] - red, y0 + rect[3] - red
        inside = (xx >= x0) & (xx <= x1) & (yy >= y0) & (yy <= y1)
        on_ring = inside & ((xx == x0) | (xx == x1) | (yy == y0) | (yy == y1))
    on_dot = np.zeros((rows, cols), bool)
    if particles is not None:
        plane = np.zeros((rows + 6, cols + 6), bool)  # centres lie in -2 .. n + 2
        for cx, cy in _kept_centres(particles, rows, cols, mut):
            plane[cy + 3, cx + 3] = True
        for oy, ox in ((0, 0), (0, -1), (0, 1), (-1, 0), (1, 0)):
            on_dot |= plane[3 + oy:3 + oy + rows, 3 + ox:3 + ox + cols]
    db, bb = colour_bytes(dot, ch), colour_bytes(box, ch)
    if "ring_first" in mut:
        on_ring &= ~on_dot
    else:
        on_dot &= ~on_ring
    out[on_dot, :len(db)] = db
    out[on_ring, :len(bb)] = bb
    return out.reshape(img.shape)


def overlay(img, particles, dot, centre, size, box, mut=(), paint=paint_loop):
    """The driver's painting of one frame: dots, then the box around the estimate."""
    return paint(img, particles, dot, box_rect(centre, size, mut), box, mut)


# ---------------------------------------------------------------------------------------------------------- the cases
ROWS, COLS = 37, 53


def image(rows, cols, ch, pad):
    """(buffer rows x (cols * ch + pad) with the padding at SENTINEL, the rows x cols x ch view into it)."""
    buf = np.full((rows, cols * ch + pad), SENTINEL, np.uint8)
    y, x, c = np.mgrid[0:rows, 0:cols, 0:ch]
    view = np.ndarray((rows, cols, ch), np.uint8, buffer=buf, strides=(buf.strides[0], ch, 1))
    view[...] = (x * 7 + y * 13 + c * 29 + 5) % 251
    return buf, view


def particle_lists(rows=ROWS, cols=COLS):
    r, c = float(rows), float(cols)
    ties = [-2.5, -1.5, -0.5, 0.5, 1.5, 2.5]
    eps = 1e-3
    lists = {
        "ties": [(a, b) for a in ties for b in ties] + [(c - 1 + t, r - 1 + t) for t in ties],
        "corners_edges": [(0, 0), (c - 1, 0), (0, r - 1), (c - 1, r - 1), (c / 2, 0), (c / 2, r - 1), (0, r / 2), (c - 1, r / 2),
                          (-1, -1), (c, r), (c + 1, r / 2), (c / 2, r + 1), (-1.75, 10), (10, -1.75)],
        "margin": [(-2 + eps, 5), (-2, 7), (-2 - eps, 9), (c + 2 - eps, 11), (c + 2, 13), (c + 2 + eps, 15),
                   (5, -2 + eps), (8, -2), (11, -2 - eps), (14, r + 2 - eps), (17, r + 2), (20, r + 2 + eps),
                   (-1.25, 20), (c + 1.25, 22), (24, -1.25), (27, r + 1.25), (-1.5, 30), (30, -1.5), (c + 1.5, 3), (33, r + 1.5)],
        "nonfinite": [(NAN, 5), (5, NAN), (INF, 5), (5, -INF), (-INF, INF), (1e30, 5), (5, -1e30), (NAN, NAN), (20, 20)],
        "one_pixel_300": [(25 + 0.4 * np.sin(i), 17 + 0.4 * np.cos(i)) for i in range(300)],
        "n0": [],
        "n1": [(12.5, 7.5)],
    }
    rng = np.random.default_rng(606)
    for n in (64, 65, 4096):
        lists[f"n{n}"] = np.stack([rng.uniform(-4, cols + 4, n), rng.uniform(-4, rows + 4, n)], 1)
    return {k: np.asarray(v, np.float32).reshape(-1, 2) for k, v in lists.items()}


def boxes(rows=ROWS, cols=COLS):
    """name -> (centre, (w, h)): the driver's float box."""
    r, c = float(rows), float(cols)
    return {
        "inside": ((26.0, 18.0), (21.0, 15.0)),
        "left": ((2.0, 18.0), (11.0, 9.0)), "right": ((c - 2, 18.0), (11.0, 9.0)),
        "top": ((26.0, 1.0), (11.0, 9.0)), "bottom": ((26.0, r - 1), (11.0, 9.0)),
        "tl": ((1.0, 1.0), (8.0, 8.0)), "tr": ((c - 1, 1.0), (8.0, 8.0)),
        "bl": ((1.0, r - 1), (8.0, 8.0)), "br": ((c - 1, r - 1), (8.0, 8.0)),
        "outside": ((-40.0, 18.0), (11.0, 9.0)), "outside_below": ((26.0, r + 30), (11.0, 9.0)),
        "around": ((c / 2, r / 2), (c + 20, r + 20)),
        "w1": ((20.0, 10.0), (1.4, 9.0)), "h1": ((20.0, 10.0), (9.0, 0.6)), "w1h1": ((20.0, 10.0), (1.0, 1.0)),
        "w0": ((20.0, 10.0), (0.5, 9.0)), "h0": ((20.0, 10.0), (9.0, 0.4)), "wneg": ((20.0, 10.0), (-3.0, 9.0)),
        "hneg": ((20.0, 10.0), (9.0, -7.0)),
        "tie_size": ((30.0, 20.0), (23.0, 27.0)),  # halves 11.5 and 13.5
        "tie_centre": ((20.5, 11.5), (10.0, 6.0)), "tie_both": ((22.5, 14.5), (9.0, 7.0)), "tie_w": ((20.0, 10.0), (6.5, 7.5)),
        "tie_neg": ((2.5, 1.5), (8.0, 6.0)),
        "hand": ((30.0, 20.0), (73.0, 87.0)),  # 36.5 and 43.5: the reference's hand box
        "nan_centre": ((NAN, 10.0), (9.0, 7.0)), "nan_y": ((10.0, NAN), (9.0, 7.0)), "inf_centre": ((INF, 10.0), (9.0, 7.0)),
        "nan_size": ((20.0, 10.0), (NAN, 7.0)), "huge_size": ((20.0, 10.0), (3e9, 7.0)), "huge_centre": ((3e9, 10.0), (9.0, 7.0)),
        "big": ((20.0, 10.0), (2e9, 2e9)),
    }


def through_dots(rows=ROWS, cols=COLS):
    """A particle list whose dots lie on, astride and beside the ring of the "inside" box (x 16 .. 36, y 10 .. 24)."""
    pts = [(16, 10), (36, 24), (26, 10), (26, 9), (26, 11), (15, 18), (17, 18), (16, 18), (36.5, 20), (30, 24.5), (20, 20), (37, 25)]
    return np.asarray(pts, np.float32)


def cases():
    """(name, ch, pad, particles or None, dot colour, (centre, size) or None, box colour).  Every list with no ring and
    with the inside box on the dense 3-channel image; every box with the through-dots; the six image layouts."""
    out = []
    pl, bx = particle_lists(), boxes()
    for name, p in pl.items():
        out.append((f"dots-{name}", 3, 0, p, DOT, None, BOX))
        out.append((f"dots-{name}-inside", 3, 0, p, DOT, bx["inside"], BOX))
    for name, b in bx.items():
        out.append((f"box-{name}", 3, 0, through_dots(), DOT, b, BOX))
        out.append((f"box-{name}-alone", 3, 0, None, DOT, b, BOX))
    col3, col4 = (10.4, 300.0, -5.0), (0.5, 1.5, 2.5, 200.0)
    for ch in (1, 3, 4):
        for pad in (0, 7):
            for cname, col in (("c3", col3), ("c4", col4)) if ch == 4 else (("c3", col3),):
                out.append((f"layout-{ch}ch-pad{pad}-{cname}", ch, pad, np.concatenate([pl["ties"], pl["corners_edges"], through_dots()]),
                            col, bx["tie_both"], tuple(reversed(col4)) if cname == "c4" else (7.0, 8.0, 9.0)))
                out.append((f"layout-{ch}ch-pad{pad}-{cname}-edge", ch, pad, pl["margin"], col, bx["br"], (255.0, 0.0, 255.0, 9.0)))
    return out


def apply_case(case, mut=(), paint=paint_loop):
    """The expected buffer (padding included) of a case."""
    _, ch, pad, particles, dot, box, box_colour = case
    buf, view = image(ROWS, COLS, ch, pad)
    rect = box_rect(box[0], box[1], mut) if box is not None else None
    view[...] = paint(view, particles, dot, rect, box_colour, mut)
    return buf


def rect_cases():
    """(name, ch, pad, (x, y, w, h), colour): cv::rectangle on integer rectangles, the extremes of int included."""
    big = (1 << 31) - 1
    return [
        ("rect-intmin", 3, 0, (INT_MIN, 5, 73, 9), BOX), ("rect-intmin-wide", 3, 7, (INT_MIN, INT_MIN, big, big), BOX),
        ("rect-span", 1, 0, (-5, -5, big, big), BOX), ("rect-intmax", 3, 0, (big, 3, 5, 5), BOX),
        ("rect-edge", 4, 7, (50, 30, big, big), (1.0, 2.0, 3.0, 4.0)), ("rect-neg-size", 3, 0, (3, 3, -1, 5), BOX),
        ("rect-zero", 3, 0, (3, 3, 5, 0), BOX), ("rect-1x1", 1, 7, (0, 0, 1, 1), BOX), ("rect-full", 3, 7, (0, 0, COLS, ROWS), BOX),
        ("rect-row", 3, 0, (2, ROWS - 1, 10, 1), BOX), ("rect-col", 4, 0, (COLS - 1, -3, 1, 12), BOX),
        ("rect-past", 3, 0, (-1, -1, COLS + 2, ROWS + 2), BOX), ("rect-inside", 1, 0, (7, 9, 20, 11), (200.0,)),
    ]


def apply_rect_case(case, paint=paint_loop):
    _, ch, pad, rect, colour = case
    buf, view = image(ROWS, COLS, ch, pad)
    view[...] = paint(view, None, DOT, rect, colour)
    return buf


def driver_case(rows=24, cols=40, nframes=3, n=70, seed=9):
    """Fixed estimates and particle lists for pfDriver's painting: (bbox (x, y, w, h), [(estimate, particles)])."""
    rng = np.random.default_rng(seed)
    ticks = []
    for t in range(nframes):
        c = (np.float32(10.5 + 7 * t), np.float32(8.25 + 5 * t))
        p = np.stack([rng.normal(c[0], 4, n), rng.normal(c[1], 4, n)], 1).astype(np.float32)
        ticks.append((c, p))
    return rows, cols, (3.0, 2.0, 9.0, 7.0), ticks


def driver_frames(rows, cols, nframes):
    y, x, c = np.mgrid[0:rows, 0:cols, 0:3]
    return [(((x * 7 + y * 13 + c * 29 + 5) % 251 + t) & 255).astype(np.uint8) for t in range(nframes)]


def _f(v):
    return float(np.float32(v)).hex()


def case_tokens():
    """The cases as the text tools/probes/ps6_host_loops.cpp reads (floats as C99 hex)."""
    lines = []
    for name, ch, pad, particles, dot, box, box_colour in cases():
        p = np.zeros((0, 2), np.float32) if particles is None else particles
        dotc = list(dot) + [0.0] * (4 - len(dot))
        boxc = list(box_colour) + [0.0] * (4 - len(box_colour))
        b = (box[0][0], box[0][1], box[1][0], box[1][1]) if box is not None else (0, 0, 0, 0)
        tok = ["overlay", name, ch, pad, 0 if particles is None else 1, len(p)] + [_f(v) for v in p.reshape(-1)]
        tok += [_f(v) for v in dotc] + [0 if box is None else 1] + [_f(v) for v in b] + [_f(v) for v in boxc]
        lines.append(" ".join(str(t) for t in tok))
    for name, ch, pad, rect, colour in rect_cases():
        col = list(colour) + [0.0] * (4 - len(colour))
        lines.append(" ".join(str(t) for t in ["rect", name, ch, pad, *rect] + [_f(v) for v in col]))
    rows, cols, bbox, ticks = driver_case()
    tok = ["driver", "driver", rows, cols, len(ticks), len(ticks[0][1])] + [_f(v) for v in bbox]
    for c, p in ticks:
        tok += [_f(c[0]), _f(c[1])] + [_f(v) for v in p.reshape(-1)]
    lines.append(" ".join(str(t) for t in tok))
    return "\n".join(lines) + "\n"


def scene(seed, rows, cols, ch, nframes, obj=(9, 7), start=None, step=(2, 1)):
    """Textured background and a textured object moving `step` pixels per frame, the kind tests/test_pf_gpu.py builds:
    (frames, the object's top-left (y, x) per frame, the object's texture)."""
    rng = np.random.default_rng(seed)
    bg = rng.integers(0, 256, (rows, cols, ch), dtype=np.uint8)
    bg = ((bg.astype(np.int32) + np.roll(bg, 1, 1)) // 2).astype(np.uint8)
    tex = rng.integers(0, 256, (obj[0], obj[1], ch), dtype=np.uint8)
    y, x = start if start is not None else (rows // 3, cols // 3)
    frames, pos = [], []
    for _ in range(nframes):
        f = bg.copy()
        yy, xx = min(max(y, 0), rows - obj[0]), min(max(x, 0), cols - obj[1])
        f[yy:yy + obj[0], xx:xx + obj[1]] = tex
        frames.append(f if ch == 3 else f[:, :, 0].copy())
        pos.append((yy, xx))
        y, x = y + step[1], x + step[0]
    return frames, pos, tex
