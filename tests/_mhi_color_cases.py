"""The colour frameDifference case list that tests/test_mhi_color_ref.py (mutations, the grey step against the oracle)
and tests/test_mhi_color_gpu.py (library against tests/_mhi_color_ref.py) share, after the pattern of
tests/_mhi_cases.py: a list, not a product; inputs and expected masks are computed once per process, read-only.

The pairs are built per channel from `noise_pair`, `step_pair`'s block layout and `moving_pair` so that one channel's
difference is negative where another's is positive: the subtraction saturates before the weighting, and a grey step
taken before the subtraction gives another mask.  Alpha is random and differs between the two frames."""
import functools
from collections import namedtuple

import numpy as np

import _mhi_cases as C1
import _mhi_color_ref as ref

THRESHOLDS = C1.THRESHOLDS
# the tile (16 rows, 64 columns), word, apron and workgroup edges of _mhi_cases.SHAPES, and images below the element's size
SHAPES = ((1, 1), (2, 2), (6, 7), (15, 58), (17, 64), (53, 70), (105, 133), (209, 64))
CHANNELS = (3, 4)
# (ksize as (width, height), sigma, the noise pair's two thresholds)
BLURS = (((1, 1), 1.0, (2, 40)), ((3, 3), 1.0, (1.7, 40)), ((7, 3), 2.0, (2, 40)), ((31, 31), 10.0, (2, 1.7)))
# per-channel differences of the step blocks.  (1, 1, 0): 4899 + 9617 + 8192 = 22708 -> 1 rounded, 14516 -> 0 truncated,
# and thresh 1 decides; (3, -3, 0): 1 after the saturation, 3 with an absolute difference; (255, 0, 0): 76, or 29 with
# the weights in BGR order; (0, 1, 0): 1, or 0 from channel 0 alone; (255, 255, 255): 255, the weights' sum
STEP_TRIPLES = ((1, 1, 0), (0, 0, 1), (3, -3, 0), (-2, 5, 1), (0, 1, 0), (255, 0, 0), (0, 0, 255), (2, 2, 2), (-1, -1, -1),
                (1, 0, 1), (255, 255, 255))
STEP_THRESHOLDS = (1, 1.7, 2, 40, 255)  # each leaves some blocks and drops others

Case = namedtuple("Case", "name rows cols channels kind ksize sigma thresh")


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _pack(f1, f2, channels, seed):
    """Lists of three [rows, cols] planes -> two interleaved u8 frames [rows, cols, channels] with random alpha."""
    rng = np.random.default_rng(seed)
    out = []
    for planes in (f1, f2):
        planes = [np.clip(p, 0, 255).astype(np.uint8) for p in planes]
        if channels == 4:
            planes.append(rng.integers(0, 256, planes[0].shape).astype(np.uint8))
        out.append(np.ascontiguousarray(np.stack(planes, -1)))
    return _ro(*out)


@functools.lru_cache(maxsize=None)
def noise_pair(rows, cols, channels):
    """Channel 0 is _mhi_cases.noise_pair with difference D.  On a 12 x 12 chequerboard channel 1 holds -2 D (even
    squares: positive exactly where channel 0 saturates at 0) or D - 30 (odd squares), channel 2 holds D - 15: on the
    odd squares all three are negative where D is, and the grey difference is 0 there."""
    a, b = C1.noise_pair(rows, cols)
    a, b = a.astype(np.int64), b.astype(np.int64)
    D = b - a
    y, x = np.mgrid[0:rows, 0:cols]
    even = (y // 12 + x // 12) % 2 == 0
    base1, base2 = a[::-1], a[:, ::-1]
    return _pack([a, base1, base2], [b, base1 + np.where(even, -2 * D, D - 30), base2 + D - 15], channels, rows * 131 + cols)


@functools.lru_cache(maxsize=None)
def step_pair(rows, cols, channels):
    """_mhi_cases.step_pair's 9 x 9 blocks with one of STEP_TRIPLES as the per-channel difference."""
    nby, nbx = max(rows // 9, 1), max(cols // 9, 1)
    by = np.minimum(np.arange(rows) // 9, nby - 1)[:, None]
    bx = np.minimum(np.arange(cols) // 9, nbx - 1)[None, :]
    d = np.array(STEP_TRIPLES)[(by * nbx + bx) * 4 % len(STEP_TRIPLES)]  # [rows, cols, 3]
    f1 = np.where(d < 0, 7, np.where(d >= 254, 0, 100))
    return _pack(list(np.moveaxis(f1, -1, 0)), list(np.moveaxis(f1 + d, -1, 0)), channels, rows * 137 + cols)


@functools.lru_cache(maxsize=None)
def moving_pair(rows, cols, channels):
    """_mhi_cases.moving_pair in channel 0, the same block moving BACK in channel 1, both at half brightness in 2."""
    a, b = C1.moving_pair(rows, cols)
    a, b = a.astype(np.int64), b.astype(np.int64)
    return _pack([a, b, a // 2], [b, a, b // 2], channels, rows * 139 + cols)


def frames(case):
    return {"noise": noise_pair, "step": step_pair, "moving": moving_pair}[case.kind](case.rows, case.cols, case.channels)


def large(rows, cols):
    return rows >= 15 and cols >= 58


@functools.lru_cache(maxsize=None)
def cases():
    out = []

    def add(rows, cols, ch, kind, ksize, sigma, thresh):
        out.append(Case(f"{rows}x{cols}x{ch}-{kind}-b{ksize[0]}x{ksize[1]}-t{thresh}", rows, cols, ch, kind, ksize, sigma, thresh))

    for i, (rows, cols) in enumerate(SHAPES):
        for ci, ch in enumerate(CHANNELS):
            for j, (ksize, sigma, thr) in enumerate(BLURS):  # every blur on every shape and channel count
                t = thr[(i + j + ci) % 2]
                # (what passes 40 on a 15- or 17-row image is too thin for the open: the lower threshold there)
                add(rows, cols, ch, "noise", ksize, sigma, thr[0] if t == 40 and min(rows, cols) < 36 else t)
            # the degenerate thresholds (everything, nothing, NaN) give constant masks: on the small shapes only; 255
            # needs the last triple, which an image of fewer than 11 blocks does not hold
            for t in (STEP_THRESHOLDS if large(rows, cols) else THRESHOLDS):
                if t == 255 and large(rows, cols) and (rows // 9) * (cols // 9) < len(STEP_TRIPLES):
                    continue
                add(rows, cols, ch, "step", (1, 1), 1.0, t)
            if min(rows, cols) >= 36:  # the strip the block uncovers is a sixth of that wide, and the open wants 7
                ksize, sigma, _ = BLURS[(i + ci) % 3]
                add(rows, cols, ch, "moving", ksize, sigma, (1.7, 2, 40)[(i + ci) % 3])
    return tuple(out)


def cases_of(rows, cols, channels):
    return [c for c in cases() if (c.rows, c.cols, c.channels) == (rows, cols, channels)]


def case(name):
    return next(c for c in cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def expected(case):
    f1, f2 = frames(case)
    return _ro(ref.frame_difference(f1, f2, case.thresh, case.ksize, case.sigma))[0]


# ---- the sequence and the batch ------------------------------------------------------------------------------------
HISTORY = dict(thresh=20, ksize=(3, 3), sigma=1.0, tau=3, save=(5, 2, 7, 2), save_diff=(8, 1, 5, 5))
HISTORY_SHAPE = (9, 53, 70, 3)


@functools.lru_cache(maxsize=None)
def history_frames(channels=3):
    """_mhi_cases.history_frames' block (moves for five frames, then rests) in channel 0; in channel 1 it is dark on a
    bright ground, so its differences have the other sign; channel 2 is texture only."""
    F, rows, cols, _ = HISTORY_SHAPE
    rng = np.random.default_rng(11)
    out = rng.integers(90, 110, (F, rows, cols, channels)).astype(np.uint8)
    if channels == 4:
        out[..., 3] = rng.integers(0, 256, (F, rows, cols))
    for f in range(F):
        x0 = 4 + 9 * min(f, 5)
        out[f, 12:36, x0:x0 + 18, 0] = 230
        out[f, 12:36, x0:x0 + 18, 1] = 20
    return _ro(out)[0]


@functools.lru_cache(maxsize=None)
def history_expected():
    h = HISTORY
    return _ro(*ref.history_seq(history_frames(), h["thresh"], h["ksize"], h["sigma"], h["tau"], h["save"], h["save_diff"]))


# 7 videos: frame counts 2 .. 9, taus 1, 3 and 300, two thresholds, save numbers including 1 and F - 1
BATCH = (dict(F=2, tau=1, thresh=20, save=1), dict(F=9, tau=300, thresh=20, save=8), dict(F=5, tau=3, thresh=38, save=1),
         dict(F=7, tau=3, thresh=38, save=4), dict(F=3, tau=300, thresh=20, save=2), dict(F=9, tau=1, thresh=20, save=3),
         dict(F=6, tau=3, thresh=38, save=5))
BATCH_BLUR = ((3, 3), 1.0)


@functools.lru_cache(maxsize=None)
def batch_videos(channels=3):
    """Video v is history_frames() from frame v % 3 on (so the videos differ), cut to its frame count."""
    fr = history_frames(channels)
    reps = np.concatenate([fr, fr[::-1]])
    return tuple(_ro(np.ascontiguousarray(reps[v % 3:v % 3 + b["F"]]))[0] for v, b in enumerate(BATCH))


@functools.lru_cache(maxsize=None)
def batch_expected(channels=3):
    ksize, sigma = BATCH_BLUR
    return _ro(np.stack([ref.history_seq(f, b["thresh"], ksize, sigma, b["tau"], (b["save"],))[0][0]
                         for f, b in zip(batch_videos(channels), BATCH)]))[0]
