"""The frameDifference case list that tests/test_mhi_ref.py (reference against oracle, mutations) and
tests/test_mhi_paths_gpu.py (library against reference) share: a list, not a product.  Inputs and expected masks are
computed once per process and handed out read-only."""
import functools
from collections import namedtuple

import numpy as np

import _mhi_ref as ref

NAN = float("nan")
THRESHOLDS = (-3, 0, 1, 1.7, 2, 40, 255, 256, NAN)

# rows at the blur tile (16), one wave of the open (52 + 6-row aprons) and its workgroup of four (208); columns at the
# 64-bit word, at its 6-column aprons and at the `x0 + 70 <= cols` fast-path edge of the second word; images smaller
# than the structuring element and than the blur's half-width
SHAPES = ((15, 58), (16, 63), (17, 64), (51, 65), (52, 69), (53, 70), (57, 71), (58, 128), (104, 129), (105, 133),
          (207, 134), (208, 200), (209, 64), (213, 200), (13, 77),
          (1, 1), (1, 300), (300, 1), (2, 2), (3, 4), (5, 5), (6, 7))

# (ksize as (width, height), sigma, the noise pair's thresholds): thresholds at which the noise mask is ragged after
# the open (tests/test_mhi_ref.py asserts that every larger shape has masks holding both values)
BLURS = (((1, 1), 1.0, (1, 2)), ((3, 3), 1.0, (1.7, 40)), ((5, 1), 1.5, (2, 40)), ((1, 9), 1.2, (1, 40)),
         ((7, 3), 2.0, (1.7, 40)))
BLURS31 = (((31, 31), 10.0, (40, 1.7)), ((31, 1), 10.0, (40, 2)), ((1, 31), 10.0, (40, 1)))
STEP_DIFFS = (-3, -2, -1, 0, 1, 2, 3, 4, 5, 254, 255)

Case = namedtuple("Case", "name rows cols kind ksize sigma thresh")


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def noise_pair(rows, cols):
    """f2 - f1 = a diagonal ramp with a wiggle (-45 .. 45, what is left after a 31-tap blur) + 6 x 6 patches
    (-30 .. 60) + per-pixel noise (-12 .. 12): at every blur some regions pass a threshold and some do not, and the
    masks are ragged and alive at the borders."""
    rng = np.random.default_rng(rows * 7919 + cols)
    y, x = np.mgrid[0:rows, 0:cols]
    u = (y / max(rows - 1, 1) + x / max(cols - 1, 1)) / 2
    if (rows + cols) % 2:  # every other shape has its live corner at the top left
        u = 1 - u
    ramp = np.rint(90 * u - 45 + 8 * np.sin(y / 5.0) * np.cos(x / 7.0)).astype(np.int64)
    coarse = rng.integers(-30, 61, (rows // 6 + 1, cols // 6 + 1)).repeat(6, 0).repeat(6, 1)[:rows, :cols]
    f1 = rng.integers(50, 150, (rows, cols))
    f2 = f1 + ramp + coarse + rng.integers(-12, 13, (rows, cols))
    return _ro(f1.astype(np.uint8), np.clip(f2, 0, 255).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def step_pair(rows, cols):
    """Blocks of 9 x 9 (the last of a row or column runs to the border, so blocks touch every edge and corner) on
    which f2 - f1 is one of STEP_DIFFS: with the 1 x 1 blur the threshold inside the fused kernel decides whole blocks,
    and a 9 x 9 block survives the open."""
    nby, nbx = max(rows // 9, 1), max(cols // 9, 1)
    by = np.minimum(np.arange(rows) // 9, nby - 1)[:, None]
    bx = np.minimum(np.arange(cols) // 9, nbx - 1)[None, :]
    d = np.array(STEP_DIFFS)[(by * nbx + bx) * 4 % len(STEP_DIFFS)]  # (4 and 11 are coprime: every value in 11 blocks)
    f1 = np.where(d < 0, 7, np.where(d >= 254, 0, 100))
    return _ro(f1.astype(np.uint8), (f1 + d).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def moving_pair(rows, cols):
    """A bright block on a dim texture that moves right and down by a third of its size."""
    rng = np.random.default_rng(rows * 31 + cols)
    out = []
    s = max(min(rows, cols) // 2, 1)
    for k in range(2):
        f = rng.integers(90, 110, (rows, cols)).astype(np.uint8)
        y0, x0 = rows // 5 + k * (s // 3 + 1), cols // 6 + k * (s // 3 + 1)
        f[y0:y0 + s, x0:x0 + s] = 230
        out.append(f)
    return _ro(*out)


def frames(case):
    if case.kind == "same":
        f1, _ = noise_pair(case.rows, case.cols)
        return f1, f1
    return {"noise": noise_pair, "step": step_pair, "moving": moving_pair}[case.kind](case.rows, case.cols)


def _name(rows, cols, kind, ksize, thresh):
    return f"{rows}x{cols}-{kind}-b{ksize[0]}x{ksize[1]}-t{thresh}"


@functools.lru_cache(maxsize=None)
def cases():
    out = []

    def add(rows, cols, kind, ksize, sigma, thresh):
        out.append(Case(_name(rows, cols, kind, ksize, thresh), rows, cols, kind, ksize, sigma, thresh))

    for i, (rows, cols) in enumerate(SHAPES):
        for j in range(3):  # three of the five small blurs per shape, in rotation
            ksize, sigma, thr = BLURS[(i + j) % len(BLURS)]
            add(rows, cols, "noise", ksize, sigma, thr[(i + j) % 2])
        for j, (ksize, sigma, thr) in enumerate(BLURS31):  # the 31-tap passes on every shape, the tiny ones included
            add(rows, cols, "noise", ksize, sigma, thr[(i + j) % 2])
        for t in THRESHOLDS:
            add(rows, cols, "step", (1, 1), 1.0, t)
        for t in (THRESHOLDS[i % 3], THRESHOLDS[3 + i % 6]):
            add(rows, cols, "same", (3, 3), 1.0, t)
        add(rows, cols, "moving", (7, 3), 2.0, 10)
        ksize, sigma, _ = BLURS[i % len(BLURS)]
        add(rows, cols, "moving", ksize, sigma, THRESHOLDS[2 + i % 4])
    return tuple(out)


def cases_of(rows, cols):
    return [c for c in cases() if (c.rows, c.cols) == (rows, cols)]


def case(name):
    return next(c for c in cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def expected(case):
    f1, f2 = frames(case)
    return _ro(ref.frame_difference(f1, f2, case.thresh, case.ksize, case.sigma))[0]


# ---- calcMotionHistory and historySequence ----------------------------------------------------------------------
TAUS = (1, 2, 25, 255, 300)
UPDATE_SHAPE = (17, 70)  # more than one 4 x 64 block either way, ragged in both
HISTORY = dict(thresh=20, ksize=(3, 3), sigma=1.0, tau=3, save=(5, 2, 7, 2))  # unordered, with a repeat
HISTORY_SHAPE = (9, 53, 70)  # more frames than tau: what moved early decays to the floor


@functools.lru_cache(maxsize=None)
def update_inputs():
    """(history, mask): masks hold 0, 1, 2 and 255 (only 1 is motion), histories 0, 1, 255 and a few others."""
    rng = np.random.default_rng(70)
    mask = rng.choice(np.array([0, 1, 2, 255], np.uint8), UPDATE_SHAPE)
    hist = rng.choice(np.array([0, 1, 255, 0, 1, 255, 2, 44, 128, 254], np.uint8), UPDATE_SHAPE)
    return _ro(hist, mask)


@functools.lru_cache(maxsize=None)
def history_frames():
    """A bright block that moves for five frames and then rests, on a dim texture."""
    F, rows, cols = HISTORY_SHAPE
    rng = np.random.default_rng(9)
    out = rng.integers(90, 110, HISTORY_SHAPE).astype(np.uint8)
    for f in range(F):
        x0 = 4 + 9 * min(f, 5)
        out[f, 12:36, x0:x0 + 18] = 230
    return _ro(out)[0]


@functools.lru_cache(maxsize=None)
def history_expected():
    h = HISTORY
    return _ro(ref.history_seq(history_frames(), h["thresh"], h["ksize"], h["sigma"], h["tau"], h["save"]))[0]
