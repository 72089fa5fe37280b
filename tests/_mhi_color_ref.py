"""numpy reference of mhi::frameDifference on colour frames and of mhiHelper's loop with both save lists, built on
tests/_mhi_ref.py (`blur`, `subtract`, `threshold`, `morph_open`, `update`) plus the grey step.  Written from

  * ps7_cpp/lib/MotionHistory.cpp:50-73: blur f1, blur f2 (CV_8UC3: every channel a plane of its own),
    `subtract(f2Blur, f1Blur)` per channel, `cvtColor(diff, diffGrey, COLOR_RGB2GRAY)`, threshold, open;
  * ps7_cpp/src/Solution.cpp:16-101 (mhiHelper: `vid >> frame` hands over BGR frames; saveDiffFrames, saveMHIFrames);
  * the contract in include/mi_cv.h (micv_mhi_frame_difference_c_dev).

The grey step is the 8-bit rule of cvtColor: g = (d0 * 4899 + d1 * 9617 + d2 * 1868 + 8192) >> 14 with channel 0 taking
the 0.299 weight as written (RGB2GRAY on BGR data), channel 3 ignored.  The weights sum to 16384, so g <= 255 without a
clamp.  The order matters: the subtraction saturates per channel BEFORE the weighting, so a channel that got darker
contributes 0 and does not cancel one that got brighter.

Every function takes `mut`; the colour mutations are COLOR_MUTATIONS, everything else goes on to tests/_mhi_ref.py
(`sub_abs` is one of those).  tests/test_mhi_color_ref.py shows each on a case that tests/test_mhi_color_gpu.py uses."""
import numpy as np

import _mhi_ref as M

WEIGHTS = (4899, 9617, 1868)
COLOR_MUTATIONS = frozenset({"grey_before_subtract", "grey_before_blur", "grey_weights_bgr", "grey_truncated",
                             "alpha_weighted", "channel0_only"})
MUTATIONS = COLOR_MUTATIONS | M.MUTATIONS


def _split(mut):
    mut = frozenset(mut)
    bad = mut - MUTATIONS
    if bad:
        raise ValueError(f"unknown mutations {sorted(bad)}")
    return mut & COLOR_MUTATIONS, mut - COLOR_MUTATIONS


def grey(d, mut=()):
    """cvtColor(COLOR_RGB2GRAY) on u8 [..., C], C = 3 or 4 -> u8 [...]."""
    cm, _ = _split(mut)
    d = np.asarray(d, np.uint8).astype(np.int64)
    if "channel0_only" in cm:
        return d[..., 0].astype(np.uint8)
    w = WEIGHTS[::-1] if "grey_weights_bgr" in cm else WEIGHTS
    acc = d[..., 0] * w[0] + d[..., 1] * w[1] + d[..., 2] * w[2]
    if "alpha_weighted" in cm and d.shape[-1] == 4:
        acc = acc + d[..., 3] * w[0]
    if "grey_truncated" not in cm:
        acc = acc + 8192
    return np.minimum(acc >> 14, 255).astype(np.uint8)


def _planes(f):
    """[..., rows, cols, C] -> [C, ..., rows, cols]"""
    return np.moveaxis(np.asarray(f, np.uint8), -1, 0)


def blur_planes(f, ksize, sigma, mut=()):
    """Every channel blurred as a plane of its own -> u8, the input's layout."""
    _, bm = _split(mut)
    return np.moveaxis(M.blur(_planes(f), ksize, sigma, bm), 0, -1)


def grey_difference(b1, b2, mut=()):
    """The u8 image the threshold sees, from the two blurred frames [..., C]."""
    cm, bm = _split(mut)
    if "grey_before_subtract" in cm:
        return M.subtract(grey(b2, mut), grey(b1, mut), bm)
    return grey(M.subtract(b2, b1, bm), mut)


def difference_of_blurred(b1, b2, thresh, mut=()):
    _, bm = _split(mut)
    return M.morph_open(M.threshold(grey_difference(b1, b2, mut), thresh, bm), bm)


def frame_difference(f1, f2, thresh, ksize=3, sigma=1.0, mut=()):
    """mhi::frameDifference on u8 frames [rows, cols, C], C = 3 or 4 (a 2-D frame goes to tests/_mhi_ref.py)."""
    cm, bm = _split(mut)
    f1, f2 = np.asarray(f1, np.uint8), np.asarray(f2, np.uint8)
    if f1.ndim == 2:
        return M.frame_difference(f1, f2, thresh, ksize, sigma, bm)
    if "grey_before_blur" in cm:
        return M.frame_difference(grey(f1, mut), grey(f2, mut), thresh, ksize, sigma, bm)
    return difference_of_blurred(blur_planes(f1, ksize, sigma, mut), blur_planes(f2, ksize, sigma, mut), thresh, mut)


def history_seq(frames, thresh, ksize, sigma, tau, save=(), save_diff=(), mut=()):
    """mhiHelper's loop on [F, rows, cols, C] (or [F, rows, cols]) frames -> (histories in save's order, masks in
    save_diff's order), each [n, rows, cols] u8; repeats allowed, either list may be empty."""
    _, bm = _split(mut)
    frames = np.asarray(frames, np.uint8)
    last = max(list(save) + list(save_diff))
    if frames.ndim == 3:
        blurred = M.blur(frames[:last + 1], ksize, sigma, bm)
        step = lambda a, b: M.difference_of_blurred(a, b, thresh, bm)
    else:
        blurred = blur_planes(frames[:last + 1], ksize, sigma, mut)
        step = lambda a, b: difference_of_blurred(a, b, thresh, mut)
    hist = np.zeros(frames.shape[1:3], np.uint8)
    hs, ds = {}, {}
    for f in range(1, last + 1):
        ds[f] = step(blurred[f - 1], blurred[f])
        hist = hs[f] = M.update(hist, ds[f], tau, bm)
    empty = np.zeros((0,) + frames.shape[1:3], np.uint8)
    return (np.stack([hs[j] for j in save]) if len(save) else empty,
            np.stack([ds[j] for j in save_diff]) if len(save_diff) else empty)
