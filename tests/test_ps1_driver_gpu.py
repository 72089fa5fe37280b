"""The ps1 driver on the device (hough.hip's radius-range circle search, ps1.hip) against the restatements
tests/_ps1_driver_ref.py, _hough_ref.py and _edge_ref.py, and against the library's own per-radius calls.  Equality is
exact everywhere."""
import functools

import numpy as np
import pytest

import _edge_ref as E
import _hough_ref as H
import _ps1_driver_ref as R

pytestmark = pytest.mark.gpu

INT_MIN = -2 ** 31


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def u32(t):
    return host(t).view(np.uint32)


def rand_mask(rows, cols, density, seed):
    return ((np.random.default_rng(seed).random((rows, cols)) < density) * 255).astype(np.uint8)


def _ps1():
    from introtocomputervision_amd import ps1
    return ps1


def _synth():
    from introtocomputervision_amd import synth
    return synth


# ------------------------------------------------------------------ the radius range ------

def check_range(mask, r0, r1, k, thr, exp=None, host_too=True, dmask=None):
    """counts and the peaks up to the count, device (lazy) form and host form, against the per-radius reference."""
    ps1 = _ps1()
    exp = R.hough_circles_search(mask, r0, r1, k, thr) if exp is None else exp
    peaks, counts = ps1.houghCirclesSearch(dev(mask) if dmask is None else dmask, r0, r1, k, thr, lazy=True)
    cnt, pk = host(counts), u32(peaks)
    assert pk.shape == (len(exp), k, 2)
    assert cnt.tolist() == [len(e) for e in exp]
    for i, e in enumerate(exp):
        assert np.array_equal(pk[i, :cnt[i]], e), (r0 + i)
    if host_too:
        got = ps1.houghCirclesSearch(mask, r0, r1, k, thr)
        assert len(got) == len(exp)
        for g, e in zip(got, exp):
            assert g.dtype == np.uint32 and np.array_equal(g, e)
    return exp


@functools.lru_cache(maxsize=None)
def _synth_case(thr):
    mask, _, _ = _synth().hough_mask(97, 150, n_lines=2, radii=(10, 14, 18))
    return mask, R.hough_circles_search(mask, 6, 22, 5, thr)


@pytest.mark.parametrize("thr,want_counts,tied_radii", [
    (90, [5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 4, 4, 3, 4, 0, 0], 12),
    (120, [4, 1, 1, 3, 3, 1, 0, 0, 4, 0, 0, 0, 4, 0, 0, 0, 0], 3)])
def test_range_on_the_synthetic_mask(thr, want_counts, tied_radii):
    mask, exp = _synth_case(thr)
    # the mix the case is chosen for: empty, partly filled and full lists, and ties among the kept peaks
    assert [len(e) for e in exp] == want_counts
    tied = 0
    for r, e in zip(range(6, 23), exp):
        v = H.hough_circles(mask, r)[e[:, 0], e[:, 1]]
        tied += len(np.unique(v)) < len(v)
    assert tied == tied_radii
    check_range(mask, 6, 22, 5, thr, exp)


SEAM_SHAPES = [(32, 64), (33, 65), (31, 63), (1, 300), (300, 1), (65, 129)]


@functools.lru_cache(maxsize=None)
def _seam_case(rows, cols):
    mask = rand_mask(rows, cols, 0.3, rows * 1000 + cols)
    return mask, R.hough_circles_search(mask, 0, 3, 64, 1), R.hough_circles_search(mask, 70, 70, 64, 1)


def test_seam_cases_hold_peaks_next_to_a_tile_seam():
    """Some reference peak lies in row 32 or column 64: its up or left neighbour belongs to another tile."""
    hit = False
    for rows, cols in SEAM_SHAPES:
        _, lo, hi = _seam_case(rows, cols)
        for e in lo + hi:
            hit = hit or bool(((e[:, 0] == 32) | (e[:, 1] == 64)).any())
    assert hit


@pytest.mark.parametrize("rows,cols", SEAM_SHAPES)
def test_range_tile_seams(rows, cols):
    mask, lo, hi = _seam_case(rows, cols)
    check_range(mask, 0, 3, 64, 1, lo)
    check_range(mask, 70, 70, 64, 1, hi, host_too=False)  # most votes dropped


def test_range_dense_mask():
    """40 x 70 of all 255: 2 800 points (more than the 2 048-point chunk), plateaus, more candidates per tile than K."""
    mask = np.full((40, 70), 255, np.uint8)
    exp = check_range(mask, 1, 5, 64, 0)
    assert all(len(e) == 64 for e in exp)


@pytest.mark.parametrize("thr", [0, INT_MIN])
def test_range_empty_mask(thr):
    mask = np.zeros((33, 65), np.uint8)
    exp = check_range(mask, 3, 5, 7, thr)
    first = np.stack([np.arange(7) // 65, np.arange(7) % 65], axis=1).astype(np.uint32)
    assert all(np.array_equal(e, first) for e in exp)  # every cell is a candidate: the first K indices


@functools.lru_cache(maxsize=None)
def _small_mask():
    return rand_mask(45, 83, 0.08, 5)


@pytest.mark.parametrize("k", [0, 1, 65])
def test_range_num_peaks(k):
    """0 peaks, 1 peak, and 65: past the fused form (the accumulators then go through the existing peak path)."""
    check_range(_small_mask(), 2, 6, k, 8)


def test_range_degenerate_ranges_and_pitch():
    import torch
    ps1 = _ps1()
    mask = _small_mask()
    # min_radius > max_radius: zero radii, nothing written
    peaks, counts = ps1.houghCirclesSearch(dev(mask), 5, 4, 3, 1, lazy=True)
    assert tuple(peaks.shape) == (0, 3, 2) and counts.numel() == 0
    assert ps1.houghCirclesSearch(mask, 5, 4, 3, 1) == []
    check_range(mask, 4, 4, 6, 8)  # a single radius
    wide = torch.zeros((45, 128), dtype=torch.uint8, device="cuda")
    wide[:, 83:] = 255  # a wrong pitch would read these
    wide[:, :83] = dev(mask)
    view = wide[:, :83]
    assert view.stride(0) == 128
    check_range(mask, 2, 6, 5, 8, host_too=False, dmask=view)
    hwide = np.full((45, 128), 255, np.uint8)
    hwide[:, :83] = mask
    got = ps1.houghCirclesSearch(hwide[:, :83], 2, 6, 5, 8)
    for g, e in zip(got, R.hough_circles_search(mask, 2, 6, 5, 8)):
        assert np.array_equal(g, e)


def test_range_accumulators_against_the_reference():
    mask = _small_mask()
    ps1 = _ps1()
    exp_pk, exp_acc = R.hough_circles_search(mask, 2, 6, 5, 8, accumulators=True)
    peaks, counts, acc = ps1.houghCirclesSearch(dev(mask), 2, 6, 5, 8, lazy=True, accumulators=True)
    assert np.array_equal(host(acc), exp_acc)
    cnt = host(counts)
    for i, e in enumerate(exp_pk):
        assert np.array_equal(u32(peaks)[i, :cnt[i]], e)
    got, hacc = ps1.houghCirclesSearch(mask, 2, 6, 70, 8, accumulators=True)  # the per-radius path with a caller's acc
    assert np.array_equal(hacc, exp_acc)
    for g, e in zip(got, R.hough_circles_search(mask, 2, 6, 70, 8)):
        assert np.array_equal(g, e)


def test_range_against_the_library_at_ps1_problem_5():
    """480 x 640, radii 20-50, K = 10, threshold 130: the accumulators equal houghCirclesAccumulate per radius bit for
    bit, and the peaks (with and without accumulators) equal findLocalMaxima on them."""
    from introtocomputervision_amd import hough
    ps1 = _ps1()
    mask, _, _ = _synth().hough_mask(480, 640)
    d = dev(mask)
    peaks, counts, acc = ps1.houghCirclesSearch(d, 20, 50, 10, 130, lazy=True, accumulators=True)
    peaks2, counts2 = ps1.houghCirclesSearch(d, 20, 50, 10, 130, lazy=True)
    cnt, pk, pk2 = host(counts), u32(peaks), u32(peaks2)
    assert np.array_equal(cnt, host(counts2))
    assert cnt.max() > 0
    for i, r in enumerate(range(20, 51)):
        a = hough.houghCirclesAccumulate(d, r)
        assert bool((a == acc[i]).all()), r
        p, c = hough.findLocalMaxima(a, 10, 130, lazy=True)
        n = int(host(c)[0])
        assert n == cnt[i], r
        assert np.array_equal(u32(p)[:n], pk[i, :n]) and np.array_equal(pk2[i, :n], pk[i, :n]), r


# ------------------------------------------------------------------ pre-processing ------

BLUR_CASES = [(1, 1, 31), (2, 3, 31), (5, 7, 31)] + [(r, c, n) for (r, c) in [(37, 70), (65, 129)] for n in (1, 3, 13, 19)]


@pytest.mark.parametrize("rows,cols,n", BLUR_CASES)
def test_gaussian_blur(rows, cols, n):
    ps1 = _ps1()
    rng = np.random.default_rng(rows * 100 + n)
    sigma = 0.3 * ((n - 1) * 0.5 - 1) + 0.8 if n > 1 else 0.7
    f = (rng.random((rows, cols), np.float32) * 300 - 20).astype(np.float32)
    exp = R.blur_f32(f, n, sigma)
    got = host(ps1.gaussianBlur(dev(f), n, sigma))
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), exp.view(np.uint32))
    assert np.array_equal(ps1.gaussianBlur(f, n, sigma).view(np.uint32), exp.view(np.uint32))
    b = rng.integers(0, 256, (rows, cols)).astype(np.uint8)
    expb = E.blur(b, n, sigma)
    assert np.array_equal(host(ps1.gaussianBlur(dev(b), n, sigma)), expb)
    assert np.array_equal(ps1.gaussianBlur(b, n, sigma), expb)


def test_generate_edge_f32_equals_u8_on_u8_images():
    """The existing 8-bit generateEdge as yardstick: test_canny's images and a random one."""
    from introtocomputervision_amd import hough
    from test_canny import _ramp_path_image, _serpentine, scene
    ps1 = _ps1()
    images = [(scene(120, 160), 5, 1.2, 40, 100), (scene(97, 131, seed=97), 1, 0.0001, 1, 3), (scene(33, 35, seed=33), 3, 1.0, 20, 60),
              (np.random.default_rng(3).integers(0, 256, (70, 107)).astype(np.uint8), 5, 2.1, 0, 30)]
    path = _serpentine(64, 140)
    images.append((_ramp_path_image(64, 140, path), 1, 0.0001, 30, 200))
    for img, gs, sigma, lo, hi in images:
        want = host(hough.generateEdge(dev(img), gs, sigma, lo, hi))
        f = img.astype(np.float32)
        assert np.array_equal(host(ps1.generateEdge(dev(f), gs, sigma, lo, hi)), want)
        assert np.array_equal(ps1.generateEdge(f, gs, sigma, lo, hi), want)
        assert np.array_equal(host(ps1.generateEdge(dev(img), gs, sigma, lo, hi)), want)  # uint8 dispatches to the existing entry
        assert want.any()


def test_generate_edge_f32_on_special_floats():
    from test_canny import scene
    ps1 = _ps1()
    f = scene(60, 90, seed=4).astype(np.float32) + np.float32(0.25)
    f[10, 10], f[11, 40], f[12, 70] = np.nan, np.inf, -np.inf
    f[30, 5:20], f[31, 5:20], f[32, 5:20] = 255.5, 254.5, -0.5
    f[50, 50] = 3e9
    for gs, sigma in [(1, 0.5), (3, 0.9)]:
        exp = R.generate_edge_f32(f, gs, sigma, 30, 90)
        assert np.array_equal(host(ps1.generateEdge(dev(f), gs, sigma, 30, 90)), exp)
        assert exp.any()
    # the conversion alone
    v = np.array([[np.nan, np.inf, -np.inf, 255.5, 254.5, -0.5, 0.5, 1.5, 2.5, 300, -7, 3e9, -3e9, 2147483520.0, -0.0]], np.float32)
    assert np.array_equal(host(ps1.gray2rgb(dev(v)))[:, :, 0], R.to_u8(v))


ERODE_SHAPES = [(1, 1), (2, 3), (5, 5), (37, 70), (65, 129)]


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.float32:
        nan = np.isnan(a) & np.isnan(b)
        return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | nan).all())
    return np.array_equal(a, b)


@pytest.mark.parametrize("rows,cols", ERODE_SHAPES)
def test_erode(rows, cols):
    ps1 = _ps1()
    rng = np.random.default_rng(rows * 7 + cols)
    rnd = (rng.random((rows, cols), np.float32) * 200 - 100).astype(np.float32)
    ints = rng.integers(0, 256, (rows, cols)).astype(np.float32)
    special = rnd.copy()
    flat = special.ravel()
    flat[rng.integers(0, flat.size, max(1, flat.size // 9))] = np.inf
    flat[rng.integers(0, flat.size, max(1, flat.size // 9))] = -np.inf
    flat[rng.integers(0, flat.size, max(1, flat.size // 9))] = np.nan  # first tap of some outputs, a later tap of others
    zeros = np.where(rng.random((rows, cols)) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    zeros_nan = zeros.copy()
    zeros_nan.ravel()[rng.integers(0, zeros.size, max(1, zeros.size // 7))] = np.nan
    bytes_ = rng.integers(0, 256, (rows, cols)).astype(np.uint8)
    for k in (1, 3, 5, 7):
        for img in (rnd, ints, special, zeros, zeros_nan, bytes_):
            exp = R.erode(img, k)
            assert _same_bits(host(ps1.erode(dev(img), k)), exp), (k, img.dtype)
        assert _same_bits(ps1.erode(special, k), R.erode(special, k))
        assert _same_bits(ps1.erode(bytes_, k), R.erode(bytes_, k))


def test_erode_rejects_other_sizes():
    from introtocomputervision_amd import _capi
    ps1 = _ps1()
    for k in (0, 2, 9, -1):
        with pytest.raises(_capi.MicvError):
            ps1.erode(dev(np.zeros((4, 4), np.float32)), k)


# ------------------------------------------------------------------ after the peaks ------

PARALLEL_CASES = {
    "no_group": ([(0, 0), (200, 0), (0, 50), (400, 100)], 4, 150),
    "one_group_of_2": ([(10, 3), (500, 90), (140, 1), (900, 40)], 4, 150),
    "two_groups": ([(10, 3), (500, 90), (140, 1), (901, 41), (905, 43), (2000, 7)], 4, 150),
    "all_one_key": ([(i, (7 * i) % 4) for i in range(149, -1, -1)], 4, 150),
    "delta_1": ([(5, 5), (5, 6), (5, 5), (6, 5), (5, 6)], 1, 1),
}


@pytest.mark.parametrize("name", sorted(PARALLEL_CASES))
def test_parallel_lines(name):
    ps1 = _ps1()
    pts, dt, dr = PARALLEL_CASES[name]
    p = np.array(pts, np.uint32).reshape(-1, 2)
    exp = R.parallel_lines(p, dt, dr)
    if name == "no_group":
        assert len(exp) == 0
    if name == "all_one_key":
        assert len(exp) == len(p)
    got = ps1.findParallelLines(dev(p.view(np.int32)), dt, dr)
    assert np.array_equal(u32(got), exp)
    assert np.array_equal(ps1.findParallelLines(p, dt, dr), exp)


def test_parallel_lines_4096_peaks_and_device_count():
    import torch
    ps1 = _ps1()
    rng = np.random.default_rng(9)
    p = rng.integers(0, 600, (4096, 2)).astype(np.uint32)
    exp = R.parallel_lines(p, 4, 150)
    assert 0 < len(exp) < 4096
    assert np.array_equal(u32(ps1.findParallelLines(dev(p.view(np.int32)), 4, 150)), exp)
    assert np.array_equal(ps1.findParallelLines(p, 4, 150), exp)
    # the count stays on the device: only the first 1000 rows are peaks
    cnt = torch.tensor([1000], dtype=torch.int64, device="cuda")
    out, ocnt = ps1.findParallelLines(dev(p.view(np.int32)), 4, 150, count=cnt, lazy=True)
    exp = R.parallel_lines(p[:1000], 4, 150)
    assert int(host(ocnt)[0]) == len(exp) and np.array_equal(u32(out)[:len(exp)], exp)


def test_parallel_lines_zero_delta_raises():
    from introtocomputervision_amd import _capi
    ps1 = _ps1()
    p = np.array([[1, 2], [1, 2]], np.uint32)
    for dt, dr in [(0, 150), (4, 0)]:
        with pytest.raises(_capi.MicvError):
            ps1.findParallelLines(dev(p.view(np.int32)), dt, dr)
        with pytest.raises(_capi.MicvError):
            ps1.findParallelLines(p, dt, dr)


def _backdrop(rows, cols):
    yy, xx = np.mgrid[0:rows, 0:cols]
    return np.stack([(yy * 3 + xx) % 251, (yy + 2 * xx) % 241, (yy * xx) % 239], axis=2).astype(np.uint8)


@pytest.mark.parametrize("rows,cols", [(61, 97), (480, 640)])
@pytest.mark.parametrize("theta_bin", [1, 3])
def test_draw_lines(rows, cols, theta_bin):
    """Every theta column, rho rows at 0, mid and last; six images per rho row (columns c = g mod 6) so that lines
    stay apart.  theta = 0, -90, +-1 and +-45 are among the columns of both bin sizes (90, 0, 89 / 91, 45 / 135 over
    the bin), and rho row 0 holds lines that miss the image."""
    ps1 = _ps1()
    rb, tb, _ = H.lines_dims(rows, cols, 1, theta_bin)
    thetas = {c * theta_bin - 90 for c in range(tb)}
    assert {0, -90, 45, -45} <= thetas and ({1, -1} <= thetas or theta_bin == 3)
    img = _backdrop(rows, cols)
    miss = R.draw_lines(img, [(0, 135 // theta_bin)], 1, theta_bin)
    assert np.array_equal(miss, img)  # x cos 45 + y sin 45 = -diag: no pixel
    for row in (0, rb // 2, rb - 1):
        for g in range(6):
            peaks = np.array([(row, c) for c in range(g, tb, 6)], np.uint32)
            exp = R.draw_lines(img, peaks, 1, theta_bin, (0, 255, 0))
            got = ps1.drawLinesParametric(dev(img), dev(peaks.view(np.int32)), 1, theta_bin)
            assert np.array_equal(host(got), exp), (row, g)
    peaks = np.array([(rb // 2 + 7, c) for c in range(0, tb, 5)] + [(rb // 2 - 30, 0)], np.uint32)
    exp = R.draw_lines(img, peaks, 1, theta_bin, (9, 8, 7))
    assert not np.array_equal(exp, img)
    assert np.array_equal(ps1.drawLinesParametric(img.copy(), peaks, 1, theta_bin, color=(9, 8, 7)), exp)


def test_draw_lines_rho_bin_device_count_and_bad_columns():
    import torch
    ps1 = _ps1()
    rows, cols = 61, 97
    img = _backdrop(rows, cols)
    rb, tb, _ = H.lines_dims(rows, cols, 2, 7)
    peaks = np.array([(rb // 2, 3), (rb // 2 + 5, 13), (rb // 2 + 2, 10), (rb // 2, 26), (rb // 2, 4000000000), (3, 20), (rb // 2 + 10, 16)], np.uint32)
    assert tb == 26  # column 26 and the huge one name no theta: not drawn
    exp = R.draw_lines(img, peaks, 2, 7)
    assert np.array_equal(host(ps1.drawLinesParametric(dev(img), dev(peaks.view(np.int32)), 2, 7)), exp)
    cnt = torch.tensor([2], dtype=torch.int64, device="cuda")
    exp2 = R.draw_lines(img, peaks[:2], 2, 7)
    assert not np.array_equal(exp, exp2)
    assert np.array_equal(host(ps1.drawLinesParametric(dev(img), dev(peaks.view(np.int32)), 2, 7, count=cnt)), exp2)


def test_draw_circles():
    """Centres inside, on each border, in each corner and outside; radius 0, 1, 20 and larger than the image; the
    [n_radii][K] layout with counts 0, partial and K."""
    ps1 = _ps1()
    rows, cols = 40, 60
    img = _backdrop(rows, cols)
    centres = [(20, 30), (0, 30), (39, 30), (20, 0), (20, 59), (0, 0), (0, 59), (39, 0), (39, 59), (45, 70), (300, 300),
               (100000, 5), (5, 4000000000), (60, 10)]
    k = len(centres)
    base = np.array(centres, np.uint32)
    for r0 in (0, 20, 200):
        peaks = np.stack([base, base[::-1], base])  # three radii: r0, r0 + 1, r0 + 2
        for counts in ([k, 5, 0], [0, 0, 0], [k, k, k], [1, k, 9]):
            cnt = np.array(counts, np.int64)
            exp = R.draw_circles(img, peaks, cnt, r0, (0, 255, 0))
            got = ps1.drawCircles(dev(img), dev(peaks.view(np.int32)), r0, counts=dev(cnt))
            assert np.array_equal(host(got), exp), (r0, counts)
        assert np.array_equal(ps1.drawCircles(img.copy(), peaks, r0, color=(1, 2, 3), counts=np.array([k, 5, 0])),
                              R.draw_circles(img, peaks, [k, 5, 0], r0, (1, 2, 3)))
    one = R.draw_circles(img, base[:1], [1], 20)
    assert not np.array_equal(one, img)
    assert np.array_equal(host(ps1.drawCircles(dev(img), dev(base[:1].view(np.int32)), 20)), one)  # [n, 2] form
    assert np.array_equal(R.draw_circles(img, base[:9], [9], 200), img)  # larger than the image: nothing inside


def test_gray2rgb():
    ps1 = _ps1()
    rng = np.random.default_rng(2)
    b = rng.integers(0, 256, (37, 70)).astype(np.uint8)
    f = (rng.random((37, 70), np.float32) * 400 - 70).astype(np.float32)
    f[3, 3], f[4, 4] = np.nan, np.inf
    for img in (b, f):
        exp = R.gray2rgb(img)
        got = ps1.gray2rgb(dev(img))
        assert tuple(got.shape) == (37, 70, 3) and np.array_equal(host(got), exp)
        assert np.array_equal(ps1.gray2rgb(img), exp)


# ------------------------------------------------------------------ the chains ------

def _chain_image():
    """120 x 160: dark discs and two dark bars on a bright, slightly noisy ground (float pixels, not integers)."""
    rng = np.random.default_rng(21)
    yy, xx = np.mgrid[0:120, 0:160]
    img = np.full((120, 160), 200.0)
    for cy, cx, r in [(40, 50, 12), (80, 110, 15), (30, 120, 10)]:
        img[np.hypot(yy - cy, xx - cx) <= r] = 40
    img[np.abs(0.6 * xx + 0.8 * yy - 110) < 2.0] = 60
    img[np.abs(xx - 20) < 1.5] = 50
    return (img + rng.random((120, 160)) * 6).astype(np.float32)


EDGE_CFG, CIRC_CFG, LINE_CFG = (5, 1.2, 40, 100), (8, 18, 3, 60), (1, 1, 4, 50)


@functools.lru_cache(maxsize=None)
def _chain_ref():
    img = _chain_image()
    return img, R.problem7(img, EDGE_CFG, CIRC_CFG), R.problem8(img, EDGE_CFG, CIRC_CFG, LINE_CFG)


def _device_problem7(d):
    ps1 = _ps1()
    edges = ps1.generateEdge(ps1.erode(d, 5), *EDGE_CFG)
    peaks, counts = ps1.houghCirclesSearch(edges, CIRC_CFG[0], CIRC_CFG[1], CIRC_CFG[2], CIRC_CFG[3], lazy=True)
    return edges, ps1.drawCircles(ps1.gray2rgb(d), peaks, CIRC_CFG[0], counts=counts), counts


def test_problem_7_chain():
    img, (edges, marked), _ = _chain_ref()
    assert edges.any() and not np.array_equal(marked, R.gray2rgb(img))  # circles were found and drawn
    d_edges, d_marked, counts = _device_problem7(dev(img))
    assert np.array_equal(host(d_edges), edges)
    assert int(host(counts).sum()) > 0
    assert np.array_equal(host(d_marked), marked)


def test_problem_8_chain():
    from introtocomputervision_amd import hough
    ps1 = _ps1()
    img, (_, marked7), (edges, marked) = _chain_ref()
    assert not np.array_equal(marked, marked7)  # lines were found and drawn
    d_edges, d_marked, _ = _device_problem7(dev(img))
    acc = hough.houghLinesAccumulate(d_edges, LINE_CFG[0], LINE_CFG[1])
    peaks, count = hough.findLocalMaxima(acc, LINE_CFG[2], LINE_CFG[3], lazy=True)
    ps1.drawLinesParametric(d_marked, peaks, LINE_CFG[0], LINE_CFG[1], count=count)
    assert np.array_equal(host(d_edges), edges)
    assert np.array_equal(host(d_marked), marked)
