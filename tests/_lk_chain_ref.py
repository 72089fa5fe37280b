"""Exact numpy reference of ps5's pyramid LK chain, lk::calcOpticalFlowPyr (no oracle code).

Written from the reference sources alone -- ProblemSets/ps5_cpp/lib/Pyramids.cu, Pyramids.cpp, OpticalFlow.cpp and
ps5_cpp/src/Solution.cpp:187-200 (the Laplacian pyramid) -- and the decisions DESIGN.md §2 records for what OpenCV 3.4.1
does inside its calls.  It shares no code with oracle/*.c or tests/_oracle.py; `fmaf` and `reflect101` come from
tests/_edge_ref.py, which is oracle-free too.  Every output is bit for bit what the contract specifies:

  * pyr_down: odd-index decimation of the UNBLURRED input, (rows/2) x (cols/2) (Pyramids.cu:31,53,65-66: the kernel is
    launched on d_src, not on d_blurred).
  * pyr_up: 2x2 replication (Pyramids.cu:86-91), then the separable [1,4,6,4,1]/16 filter (:19,126-127) as an fmaf
    chain from +0, row pass then column pass, float intermediate, BORDER_REFLECT_101.
  * to_gray (Pyramids.cpp:9-15): CV_8U (c0*4899 + c1*9617 + c2*1868 + 2^13) >> 14 with the alpha channel ignored, then
    float; CV_32F (c0*0.299f + c1*0.587f) + c2*0.114f unfused.  c0 carries the 0.299 weight (COLOR_RGB2GRAY).
  * resize_linear (cv::resize INTER_LINEAR, CV_32F; OpenCV 3.4.1 resizeGeneric_ with HResizeLinear / VResizeLinear):
    scale = 1 / (double(dsize) / ssize); f = float((d + 0.5) * scale - 0.5), s = floor(f), f -= s.  Columns: s < 0 gives
    (s, f) = (0, 0); from the first column whose s + 1 >= scols on (OpenCV's xmax) the row buffer is the single tap
    S[min(s, scols - 1)] * 1; every other column blends BOTH taps, S[s] * (1 - f) + S[s + 1] * f, a zero weight
    included ("x taps zero-weighted" -- on the left edge and at integer positions the second tap is
    multiplied by 0, so an infinite neighbour gives NaN and -0 + +0 gives +0; on the right edge the single tap keeps
    its sign and ignores nothing).  Rows: s and s + 1 clamped to the image, f NOT reset, row0 * (1 - f) + row1 * f.
    Horizontal then vertical, unfused float.
  * warp / remap_linear (lk::warp, OpticalFlow.cpp:106-120; cv::remap INTER_LINEAR, BORDER_CONSTANT 0): the map is
    float(x) + du in float32; X = cvRound(map * 32) with half to even, and INT_MIN for a NaN or a value outside the
    int32 range (the x86 conversion OpenCV 3.4.1 executes); cell saturate_cast<short>(X >> 5), fraction X & 31;
    weights (1 - k/32) products (exact); a tap outside the image reads 0; blend ((v0 w0 + v1 w1) + v2 w2) + v3 w3
    unfused with all four taps multiplied (0 * inf = NaN, as OpenCV's partial-border branch does).  A sample whose four
    taps are all outside is +0: OpenCV writes the border constant, the blend of four +0 taps with weights >= 0 is +0
    too, so the two readings agree.
  * lk_flow (OpticalFlow.cpp:41-104): Sobel 3x3 with the 1/9 scale folded into the smoothing taps
    (cv::cuda::createSobelFilter), (a + b) / 2.f as a * 0.5f + b * 0.5f with a = next's gradient (addWeighted),
    It = next - prev, five float products, GaussianBlur(win, float(win) / 3.f) as an fmaf chain (getGaussianKernel:
    exp(scale2x * x * x) in double, float taps summed in double, times 1 / sum, to float), det and Cramer in double,
    det < 0.1 -> (+0, +0), IEEE 1 / det otherwise (NaN det included).
  * level_step: one iteration of OpticalFlow.cpp:137-162 -- 2 * pyrUp of the coarse flow, cv::resize when either
    dimension differs, warp, lk_flow, du + dx.  At the coarsest level (coarse flow None) the flow is +0 and the
    warp still runs.
  * lk_flow_pyr: the level loop over level_step (`levels` replaces pyrDepth = 4); laplacian_pyramid: Solution.cpp:
    187-200 (pyrUp, resize only when the expansion is smaller, float difference, the coarsest level as is).

Every function takes `mut`, a collection of mutation names (MUTATIONS) that tests/test_lk_chain_ref.py uses to show
that a plausible misreading of the contract changes a result.

Speed (one core, numpy; tests/test_lk_chain_ref.py::test_speed_is_recorded reruns the first line): lk_flow at
256 x 512, window 15: 0.45 s; lk_flow_pyr 270 x 481, window 15, 4 levels: 0.85 s; 1080 x 1920, window 15, 5 levels:
12 s.  The five product fields are stacked and run through one vectorised fmaf per tap; the cost is the fmaf
emulation (a dozen float64 operations per element).
"""
import math

import numpy as np

from _edge_ref import fmaf, reflect101

INT_MIN = -2 ** 31
G5 = np.array([0.0625, 0.25, 0.375, 0.25, 0.0625], np.float32)  # Pyramids.cu:19
TAU = 0.1  # OpticalFlow.cpp:82

MUTATIONS = frozenset({
    "pyrdown_blur",        # pyrDown decimates the blurred image (as the source intends, not as it runs)
    "pyrdown_even",        # even-index decimation
    "pyrup_zero_insert",   # OpenCV's pyrUp: zero insertion, the same blur, x4
    "pyrup_replicate",     # BORDER_REPLICATE in pyrUp's blur
    "expand_no_x2",        # the expanded flow not doubled
    "resize_skip",         # crop / zero-pad instead of cv::resize
    "resize_align_corners",  # (d * (s - 1) / (d - 1)) sampling
    "map_minus",           # map = x - du
    "round_floor",         # floor(v * 32) instead of cvRound
    "round_half_away",     # cvRound with ties away from zero
    "map_double",          # map sum and scaling in double
    "skip_zero_taps",      # remap taps with weight 0 are left out
    "fused_blend",         # remap blend as an fmaf chain
    "remap_replicate",     # BORDER_REPLICATE in remap
    "no_coarsest_warp",    # the coarsest level is not warped
    "replace_du",          # du = dx instead of du + dx
    "gray_bgr",            # grey weights in BGR order
})


def _check(mut):
    bad = set(mut) - MUTATIONS
    if bad:
        raise ValueError(f"unknown mutations {sorted(bad)}")
    return frozenset(mut)


def _f32(a):
    return np.asarray(a, np.float32)


def gaussian_taps(n, sigma):
    """cv::getGaussianKernel(n, sigma, CV_32F), sigma > 0: exp(scale2x * x * x) in double, float taps, double sum."""
    scale2x = -0.5 / (sigma * sigma)
    t = []
    for i in range(n):
        x = i - (n - 1) * 0.5
        t.append(np.float32(math.exp(scale2x * x * x)))
    s = 0.0
    for v in t:
        s += float(v)
    s = 1.0 / s
    return np.array([np.float32(float(v) * s) for v in t], np.float32)


def _index(n, lo, replicate=False):
    p = np.arange(n) + lo
    return np.clip(p, 0, n - 1) if replicate else reflect101(p, n)


def sep_filter(src, krow, kcol, *, replicate=False):
    """Separable correlation on the last two axes: row pass then column pass, every tap acc = fmaf(x, k, acc) from +0,
    left -> right / top -> bottom, float intermediate, BORDER_REFLECT_101 (replicate: the mutation).  krow / kcol are
    lists of taps; a tap may be an array that broadcasts against the leading axes (one kernel per stacked field)."""
    src = _f32(src)
    rows, cols = src.shape[-2:]
    ar, ac = len(krow) // 2, len(kcol) // 2
    acc = np.zeros(src.shape, np.float32)
    for j, k in enumerate(krow):
        acc = fmaf(src[..., _index(cols, j - ar, replicate)], k, acc)
    out = np.zeros(src.shape, np.float32)
    for j, k in enumerate(kcol):
        out = fmaf(acc[..., _index(rows, j - ac, replicate), :], k, out)
    return out


# ----------------------------------------------------------------------------------------------- pyramids ------

def pyr_down(img, mut=()):
    """pyr::pyrDown as executed: dst(y, x) = src(2y + 1, 2x + 1)."""
    mut = _check(mut)
    img = _f32(img)
    rows, cols = img.shape[-2:]
    if "pyrdown_blur" in mut and rows and cols:
        img = sep_filter(img, list(G5), list(G5))
    o = 0 if "pyrdown_even" in mut else 1
    return np.ascontiguousarray(img[..., o::2, o::2][..., :rows // 2, :cols // 2])


def pyr_up(img, mut=()):
    """pyr::pyrUp: 2x2 replication, then the [1,4,6,4,1]/16 fmaf blur with reflect-101 (last two axes)."""
    mut = _check(mut)
    img = _f32(img)
    if "pyrup_zero_insert" in mut:
        up = np.zeros(img.shape[:-2] + (2 * img.shape[-2], 2 * img.shape[-1]), np.float32)
        up[..., ::2, ::2] = img
        return sep_filter(up, list(G5), list(G5)) * np.float32(4)
    up = np.repeat(np.repeat(img, 2, axis=-2), 2, axis=-1)
    return sep_filter(up, list(G5), list(G5), replicate="pyrup_replicate" in mut)


def gaussian_pyramid(img, levels, mut=()):
    """pyr::makeGaussianPyramid on a grey float image."""
    out = [_f32(img).copy()]
    for _ in range(1, levels):
        out.append(pyr_down(out[-1], mut))
    return out


def laplacian_pyramid(img, levels, mut=()):
    """sol::runProblem2's Laplacian pyramid (ps5 Solution.cpp:187-200)."""
    g = gaussian_pyramid(img, levels, mut)
    out = []
    for i in range(levels - 1):
        nxt = pyr_up(g[i + 1], mut)
        if nxt.shape[0] < g[i].shape[0] or nxt.shape[1] < g[i].shape[1]:
            nxt = resize_linear(nxt, *g[i].shape, mut=mut)
        out.append(g[i] - nxt)
    out.append(g[levels - 1])
    return out


def to_gray(frame, mut=()):
    """cvtColor(COLOR_RGB2GRAY) for 3 / 4 channels, then convertTo(CV_32F) (Pyramids.cpp:9-15)."""
    mut = _check(mut)
    a = np.asarray(frame)
    if a.ndim == 2:
        return a.astype(np.float32)
    order = (2, 1, 0) if "gray_bgr" in mut else (0, 1, 2)
    c0, c1, c2 = (a[..., i] for i in order)
    if a.dtype == np.uint8:
        y = (c0.astype(np.int64) * 4899 + c1.astype(np.int64) * 9617 + c2.astype(np.int64) * 1868 + (1 << 13)) >> 14
        return y.astype(np.float32)
    c0, c1, c2 = _f32(c0), _f32(c1), _f32(c2)
    return (c0 * np.float32(0.299) + c1 * np.float32(0.587)) + c2 * np.float32(0.114)


# ------------------------------------------------------------------------------------------------ resize -------

def _resize_axis(src_n, dst_n, align_corners=False):
    """Per destination index: source index s, weight f (float32) -- OpenCV's half-pixel form."""
    d = np.arange(dst_n, dtype=np.float64)
    if align_corners:
        f = (d * ((src_n - 1) / (dst_n - 1) if dst_n > 1 else d * 0.0)).astype(np.float32)
    else:
        scale = 1.0 / (float(dst_n) / src_n)
        f = ((d + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    return s, f


def resize_linear(src, drows, dcols, mut=()):
    """cv::resize(src, dst, Size(dcols, drows)), INTER_LINEAR, CV_32F (last two axes)."""
    mut = _check(mut)
    src = _f32(src)
    srows, scols = src.shape[-2:]
    if "resize_skip" in mut:
        out = np.zeros(src.shape[:-2] + (drows, dcols), np.float32)
        r, c = min(srows, drows), min(scols, dcols)
        out[..., :r, :c] = src[..., :r, :c]
        return out
    ac = "resize_align_corners" in mut
    sx, fx = _resize_axis(scols, dcols, ac)
    left = sx < 0
    fx = np.where(left, np.float32(0), fx)
    sx = np.where(left, 0, sx)
    single = sx + 1 >= scols
    single = np.cumsum(single) > 0  # from OpenCV's xmax on
    sx = np.minimum(sx, scols - 1)
    fx = np.where(single, np.float32(0), fx)
    a0 = (np.float32(1) - fx).astype(np.float32)
    s0 = src[..., sx]
    s1 = src[..., np.minimum(sx + 1, scols - 1)]
    with np.errstate(invalid="ignore", over="ignore"):
        h = np.where(single, s0 * np.float32(1), s0 * a0 + s1 * fx)
        sy, fy = _resize_axis(srows, drows, ac)
        y0 = np.clip(sy, 0, srows - 1)
        y1 = np.clip(sy + 1, 0, srows - 1)
        b0 = (np.float32(1) - fy).astype(np.float32)[:, None]
        b1 = fy[:, None]
        return (h[..., y0, :] * b0 + h[..., y1, :] * b1).astype(np.float32)


# ------------------------------------------------------------------------------------------------- remap -------

def cv_round(v, mut=()):
    """cvRound(float) as executed (x86 cvtss2si): half to even, INT_MIN for NaN or out of the int32 range -> int64."""
    mut = _check(mut)
    v = _f32(v).astype(np.float64)
    ok = (v > -2147483648.0) & (v < 2147483648.0)
    with np.errstate(invalid="ignore"):
        if "round_floor" in mut:
            r = np.floor(v)
        elif "round_half_away" in mut:
            r = np.sign(v) * np.floor(np.abs(v) + 0.5)
        else:
            r = np.rint(v)
        ok &= (r > -2147483649.0) & (r < 2147483648.0)
        return np.where(ok, np.nan_to_num(r), INT_MIN).astype(np.int64)


def remap_linear(src, mapx, mapy, mut=()):
    """cv::remap(src, dst, mapx, mapy, INTER_LINEAR), BORDER_CONSTANT 0, float maps."""
    mut = _check(mut)
    src = _f32(src)
    rows, cols = src.shape
    if "map_double" in mut:
        X = cv_round_double(mapx * 32.0, mut)
        Y = cv_round_double(mapy * 32.0, mut)
    else:
        X = cv_round(_f32(mapx) * np.float32(32), mut)
        Y = cv_round(_f32(mapy) * np.float32(32), mut)
    ix = np.clip(X >> 5, -32768, 32767)
    iy = np.clip(Y >> 5, -32768, 32767)
    kx = (X & 31).astype(np.float32) * np.float32(1.0 / 32)
    ky = (Y & 31).astype(np.float32) * np.float32(1.0 / 32)
    ax = (np.float32(1) - kx, kx)
    ay = (np.float32(1) - ky, ky)
    taps = []
    for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
        yy, xx = iy + dy, ix + dx
        w = ay[dy] * ax[dx]
        if "remap_replicate" in mut:
            v = src[np.clip(yy, 0, rows - 1), np.clip(xx, 0, cols - 1)]
        else:
            inside = (yy >= 0) & (yy < rows) & (xx >= 0) & (xx < cols)
            v = np.where(inside, src[np.clip(yy, 0, rows - 1), np.clip(xx, 0, cols - 1)], np.float32(0))
        taps.append((v, w))
    with np.errstate(invalid="ignore", over="ignore"):
        if "fused_blend" in mut:
            r = np.zeros(np.shape(X), np.float32)
            for v, w in taps:
                r = fmaf(v, w, r)
            return r
        terms = [np.where(w == 0, np.float32(0), v * w) if "skip_zero_taps" in mut else v * w for v, w in taps]
        r = terms[0]
        for t in terms[1:]:
            r = r + t
        return r.astype(np.float32)


def cv_round_double(v, mut=()):
    """The map_double mutation's conversion: the same rules on a float64 value."""
    v = np.asarray(v, np.float64)
    ok = (v > -2147483648.5) & (v < 2147483647.5)
    with np.errstate(invalid="ignore"):
        r = np.floor(v) if "round_floor" in mut else np.rint(v)
        return np.where(ok, np.nan_to_num(r), INT_MIN).astype(np.int64)


def warp(src, du, dv, mut=()):
    """lk::warp: remap at (float(x) + du, float(y) + dv), the sums in float32."""
    mut = _check(mut)
    src, du, dv = _f32(src), _f32(du), _f32(dv)
    rows, cols = src.shape
    xs = np.arange(cols, dtype=np.float32)[None, :]
    ys = np.arange(rows, dtype=np.float32)[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        if "map_double" in mut:
            mx = xs.astype(np.float64) + du.astype(np.float64)
            my = ys.astype(np.float64) + dv.astype(np.float64)
        elif "map_minus" in mut:
            mx, my = xs - du, ys - dv
        else:
            mx, my = xs + du, ys + dv
    return remap_linear(src, mx, my, mut)


# ------------------------------------------------------------------------------------------------ LK level -----

def sobel_scaled(imgs):
    """cv::cuda Sobel 3x3, scale 1/9 folded into the smoothing taps: (gx, gy) of a stack of images."""
    s = np.float32(1.0) / np.float32(9.0)
    smooth = [s * np.float32(1), s * np.float32(2), s * np.float32(1)]
    deriv = [np.float32(-1), np.float32(0), np.float32(1)]
    n = imgs.shape[0]
    both = np.concatenate([imgs, imgs])
    krow = [np.array([d] * n + [m] * n, np.float32)[:, None, None] for d, m in zip(deriv, smooth)]
    kcol = [np.array([m] * n + [d] * n, np.float32)[:, None, None] for d, m in zip(deriv, smooth)]
    g = sep_filter(both, krow, kcol)
    return g[:n], g[n:]


def lk_flow(prev, nxt, win, *, want_det=False):
    """lk::calcOpticalFlow for one level -> (u, v) float32 (and det(A) in double with want_det)."""
    prev, nxt = _f32(prev), _f32(nxt)
    if win < 1 or win % 2 == 0:
        raise ValueError("odd window expected")
    gx, gy = sobel_scaled(np.stack([prev, nxt]))
    half = np.float32(0.5)
    with np.errstate(invalid="ignore", over="ignore"):
        ix = gx[1] * half + gx[0] * half
        iy = gy[1] * half + gy[0] * half
        it = nxt - prev
        fields = np.stack([ix * ix, ix * iy, iy * iy, ix * it, iy * it])
    g = list(gaussian_taps(win, float(np.float32(win) / np.float32(3))))
    sxx, sxy, syy, sxt, syt = sep_filter(fields, g, g).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        a00, a01, a11 = sxx, sxy, syy
        b0 = (-sxt.astype(np.float32)).astype(np.float64)
        b1 = (-syt.astype(np.float32)).astype(np.float64)
        det = a00 * a11 - a01 * a01
        d = 1.0 / det
        solve = ~(det < TAU)
        u = np.where(solve, ((b0 * a11 - b1 * a01) * d), 0.0).astype(np.float32)
        v = np.where(solve, ((b1 * a00 - b0 * a01) * d), 0.0).astype(np.float32)
    return (u, v, det) if want_det else (u, v)


# ---------------------------------------------------------------------------------------------- the chain ------

def level_step(prev_k, next_k, coarse_u, coarse_v, win, mut=()):
    """One iteration of OpticalFlow.cpp:137-162 for a coarse flow of any size, or None at the coarsest level."""
    mut = _check(mut)
    prev_k, next_k = _f32(prev_k), _f32(next_k)
    rows, cols = prev_k.shape
    if coarse_u is None:
        du = np.zeros((rows, cols), np.float32)
        dv = np.zeros((rows, cols), np.float32)
        warped = next_k if "no_coarsest_warp" in mut else warp(next_k, du, dv, mut)
    else:
        e = pyr_up(np.stack([_f32(coarse_u), _f32(coarse_v)]), mut)
        if "expand_no_x2" not in mut:
            with np.errstate(over="ignore"):
                e = e * np.float32(2)
        if e.shape[-2:] != (rows, cols):
            e = resize_linear(e, rows, cols, mut)
        du, dv = e[0], e[1]
        warped = warp(next_k, du, dv, mut)
    dx, dy = lk_flow(prev_k, warped, win)
    if "replace_du" in mut:
        return dx, dy
    with np.errstate(invalid="ignore", over="ignore"):
        return du + dx, dv + dy


def lk_flow_pyr(prev, nxt, win, levels, mut=()):
    """lk::calcOpticalFlowPyr with `levels` pyramid levels (4 in the reference) on grey float images -> (u, v)."""
    pp = gaussian_pyramid(prev, levels, mut)
    nn = gaussian_pyramid(nxt, levels, mut)
    u = v = None
    for k in range(levels - 1, -1, -1):
        u, v = level_step(pp[k], nn[k], u, v, win, mut)
    return u, v
