"""Exact integer references of disparitySSD for 8-bit-valued image pairs (numpy only).

On images whose pixels are integers in 0..255 every term of the SSD is an integer, so the costs can be formed in
integer arithmetic without any rounding rule: the answer is exact whatever the order of the additions.  The float
contract (stereo.hip, the C oracle) gives the same costs as long as every partial sum stays below 2^24 -- always for
radius <= 7 ((2r+1)^2 * 255^2 < 2^24), for larger radii only when the pixel values are small enough.  serial::'s
costs are integer sums of rounded terms by definition, so there the two agree at any radius.

Both functions work per disparity on whole images (cumulative sums along y, then along x), which makes 1080 x 1920
with 128 disparities a matter of seconds -- where the scalar C oracle is slow.  tests/test_stereo_ref.py checks them
against the oracle byte for byte on small pairs; that ties the two references together.  These functions refuse images
that are not 8-bit-valued: there the float contract is restated, order-exact in float32 and with float64 bounds, by
tests/_stereo_f32_ref.py (tied to the oracle and to these functions by tests/test_stereo_f32_ref.py).
"""
import numpy as np

COLS_2R, MIN_SSD_5E6 = 1, 2  # MICV_STEREO_* (the CUDA-path flags)


def _u8(img, name):
    a = np.asarray(img)
    if a.ndim != 2 or a.size == 0:
        raise ValueError(f"{name}: a non-empty 2-D image is required")
    f = a.astype(np.float64)
    if not (np.all(np.isfinite(f)) and np.all(f == np.round(f)) and f.min() >= 0 and f.max() <= 255):
        raise ValueError(f"{name}: not an 8-bit-valued image (integers 0..255)")
    return f.astype(np.int32)


def _rows_clamped(img, rad):
    """img with rows -rad .. rows - 1 + rad, each clamped to the image (row y + rad of the result is image row y)."""
    ry = np.clip(np.arange(-rad, img.shape[0] + rad), 0, img.shape[0] - 1)
    return img[ry]


def _window_costs(left_p, right_w, rad, wcols, rows, cols, off):
    """Window sums of (left - right)^2 for one disparity.  left_p: rows + 2 rad rows, window columns -rad ..
    cols - 1 + rad.  right_w: the right image over the same rows, its column `off` = window column -rad shifted by d.
    Returns (rows, cols) int64: cost of the window whose columns are x - rad .. x - rad + wcols - 1."""
    n = cols + 2 * rad
    diff = left_p - right_w[:, off:off + n]
    sq = (diff * diff).astype(np.int64)
    cy = np.cumsum(sq, axis=0)
    cs = cy[2 * rad:].copy()  # column sums over rows y - rad .. y + rad
    cs[1:] -= cy[:rows - 1]
    cx = np.zeros((rows, n + 1), np.int64)
    np.cumsum(cs, axis=1, out=cx[:, 1:])
    return cx[:, wcols:wcols + cols] - cx[:, :cols]


def _search(left, right, rad, min_d, max_d, wcols):
    """Yields (d, cost) for d = min_d .. max_d with clamp-to-edge fetches on both images (rows and columns)."""
    L, R = _u8(left, "left"), _u8(right, "right")
    if L.shape != R.shape:
        raise ValueError("left and right differ in size")
    if rad < 0 or min_d > max_d:
        raise ValueError("bad radius or disparity range")
    rows, cols = L.shape
    lp = _rows_clamped(L, rad)[:, np.clip(np.arange(-rad, cols + rad), 0, cols - 1)]
    # right columns -rad + min_d .. cols - 1 + rad + max_d, clamped: every shift is a slice of it
    rw = _rows_clamped(R, rad)[:, np.clip(np.arange(-rad + min_d, cols + rad + max_d), 0, cols - 1)]
    for d in range(min_d, max_d + 1):
        yield d, _window_costs(lp, rw, rad, wcols, rows, cols, d - min_d)


def ssd_cuda(left, right, rad, min_d, max_d, flags=0):
    """cuda::disparitySSD's addressing (orc_disparity_ssd, flags 0..3): clamped fetch on both images, rows y - r ..
    y + r, window columns x - r .. x - r + wcols - 1 with wcols = 2r (COLS_2R) or 2r + 1; d ascending, strict '<'
    against the best so far, which starts at infinity (5e6 under MIN_SSD_5E6); -1 where nothing beats it."""
    if flags & ~(COLS_2R | MIN_SSD_5E6):
        raise ValueError(f"flags {flags}: only COLS_2R and MIN_SSD_5E6 have a CUDA-path meaning here")
    if (flags & COLS_2R) and rad < 1:
        raise ValueError("COLS_2R needs radius >= 1")
    if not (-128 <= min_d <= max_d <= 127):
        raise ValueError("disparities do not fit int8")
    wcols = 2 * rad if flags & COLS_2R else 2 * rad + 1
    shape = np.shape(left)
    best = np.full(shape, 5000000 if flags & MIN_SSD_5E6 else np.iinfo(np.int64).max, np.int64)
    disp = np.full(shape, -1, np.int8)
    for d, cost in _search(left, right, rad, min_d, max_d, wcols):
        better = cost < best
        best[better] = cost[better]
        disp[better] = d
    return disp


def ssd_serial(left, right, rad, min_d, max_d):
    """serial::disparitySSD's rules (orc_disparity_ssd_serial): replicate padding by r; for output x (padded column
    x + r) the search runs over padded positions max(0, x + r + min_d) .. min(pcol - 1, x + r + max_d), i.e. d such
    that x + d lies in -r .. cols - 1 + r; the (2r+1)^2 window at a position is fetched clamped; d ascending, strict
    '<' against 99999999; 0 where no position is searched (or none beats the start)."""
    rows, cols = np.shape(left)
    x = np.arange(cols)[None, :]
    best = np.full((rows, cols), 99999999, np.int64)
    disp = np.zeros((rows, cols), np.int8)
    for d, cost in _search(left, right, rad, min_d, max_d, 2 * rad + 1):
        better = (cost < best) & (x + d >= -rad) & (x + d <= cols - 1 + rad)
        best[better] = cost[better]
        disp[better] = d
    return disp
