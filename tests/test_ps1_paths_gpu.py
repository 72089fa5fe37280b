"""Every dispatch form of the ps1 chain (generateEdge -> houghLines / houghCircles -> findLocalMaxima, hough.hip and
canny.hip) against the exact references tests/_hough_ref.py and tests/_edge_ref.py, at the shapes where the kernels'
own structure has edges: the LDS-histogram / global-atomics line kernels, the circle kernel's 2048-point chunks,
tile seams and 15-bit packing, the four peak-selection forms under each list compaction, and the tile-by-tile
hysteresis."""
import math

import numpy as np
import pytest

import _edge_ref as E
import _hough_ref as H
import _oracle as orc
from test_canny import _ramp_path_image, _serpentine

pytestmark = pytest.mark.gpu

INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def rand_mask(rows, cols, density, seed):
    return ((np.random.default_rng(seed).random((rows, cols)) < density) * 255).astype(np.uint8)


@pytest.fixture(scope="module")
def ctxs():
    """One context per MICV_OPT_COMPACT_3PASS setting: -1 one-launch list always, 0 default (one launch up to 1 M
    elements), 1 count / scan / emit always."""
    from introtocomputervision_amd import _capi
    out = {}
    for v in (-1, 0, 1):
        c = _capi.Context(0)
        c.set_option(_capi.OPT_COMPACT_3PASS, v)
        out[v] = c
    yield out
    for c in out.values():
        c.close()


def _hough():
    from introtocomputervision_amd import hough
    return hough


# ------------------------------------------------------------------ lines ------

def _line_kernel(rows, cols, rho_bin):
    rb, _, _ = H.lines_dims(rows, cols, rho_bin, 1)
    return "lds" if rb * 4 <= 64 * 1024 else "global"


LINE_CASES = [  # (id, rows, cols, density, rho_bin, theta_bin)
    ("drawn_480x640", 480, 640, None, 1, 1),
    ("dropped_61x200_full", 61, 200, 1.0, 7, 1),
    ("theta7_97x131", 97, 131, 0.2, 2, 7),
    ("theta11_97x131", 97, 131, 0.2, 3, 11),
    ("theta181_33x65", 33, 65, 0.5, 1, 181),
    ("theta100_1x300", 1, 300, 0.5, 5, 100),
    ("tall_9000x40", 9000, 40, 0.01, 1, 1),
    ("wide_40x9000", 40, 9000, 0.01, 1, 1),
    ("tall_9000x40_rho2", 9000, 40, 0.01, 2, 7),
    ("bins16384_5792x5793", 5792, 5793, 0.0005, 1, 3),
    ("bins16386_5793x5793", 5793, 5793, 0.0005, 1, 3),
    ("bins16384_8192x1", 8192, 1, 0.3, 1, 1),
    ("bins16386_8193x1", 8193, 1, 0.3, 1, 1),
]


def _line_mask(rows, cols, density, seed=0):
    if density is None:
        from introtocomputervision_amd import synth
        return synth.hough_mask(rows, cols, n_lines=8, radii=(20, 40))[0]
    if density == 1.0:
        return np.full((rows, cols), 255, np.uint8)
    return rand_mask(rows, cols, density, rows * 31 + cols)


@pytest.mark.parametrize("case", LINE_CASES, ids=lambda c: f"{_line_kernel(c[1], c[2], c[4])}-{c[0]}")
def test_lines(ctxs, case):
    name, rows, cols, density, rho_bin, theta_bin = case
    hough = _hough()
    mask = _line_mask(rows, cols, density)
    exp = H.hough_lines(mask, rho_bin, theta_bin)
    got = host(hough.houghLinesAccumulate(dev(mask), rho_bin, theta_bin, ctx=ctxs[0]))
    assert got.shape == exp.shape and np.array_equal(got, exp)
    if name.startswith("dropped"):
        assert H.dropped_line_votes(mask, rho_bin, theta_bin)[1] > 0
    if rows * cols <= 200_000:  # the existing yardstick as well
        assert np.array_equal(got, orc.hough_lines(mask, rho_bin, theta_bin))
    if name == "drawn_480x640":  # the point list through the count / scan / emit launches
        assert np.array_equal(host(hough.houghLinesAccumulate(dev(mask), rho_bin, theta_bin, ctx=ctxs[1])), exp)


def _lines_band(ctx, band, row0, rows, rho_bin, theta_bin):
    import torch
    from introtocomputervision_amd import _buf as B
    from introtocomputervision_amd._capi import check, lib
    rb, tb, _ = H.lines_dims(rows, band.shape[1], rho_bin, theta_bin)
    acc = torch.full((rb, tb), -7, dtype=torch.int32, device=band.device)  # every cell must be written
    check(lib.micv_hough_lines_band_dev(ctx.handle, band.data_ptr(), band.shape[0], band.shape[1],
                                        B.stride_bytes(band), row0, rows, rho_bin, theta_bin, acc.data_ptr(),
                                        B.stream_of(band)))
    return host(acc)


def _circles_band(ctx, band, row0, rows, radius):
    import torch
    from introtocomputervision_amd import _buf as B
    from introtocomputervision_amd._capi import check, lib
    acc = torch.full((rows, band.shape[1]), -7, dtype=torch.int32, device=band.device)
    check(lib.micv_hough_circles_band_dev(ctx.handle, band.data_ptr(), band.shape[0], band.shape[1],
                                          B.stride_bytes(band), row0, rows, radius, acc.data_ptr(),
                                          B.stream_of(band)))
    return host(acc)


@pytest.mark.parametrize("kernel,rows,cols,rho_bin,theta_bin", [("lds", 480, 640, 1, 1), ("lds", 480, 640, 3, 7),
                                                                ("global", 9000, 40, 1, 2)])
def test_line_bands_and_pitched_masks(ctxs, kernel, rows, cols, rho_bin, theta_bin):
    """Row bands (the row-shard form) through both kernels, taken from a pitched buffer (row pitch != cols)."""
    import torch
    assert _line_kernel(rows, cols, rho_bin) == kernel
    mask = rand_mask(rows, cols, 0.02, rows)
    wide = torch.zeros((rows, cols + 37), dtype=torch.uint8, device="cuda")
    wide[:, 5:5 + cols] = dev(mask)
    view = wide[:, 5:5 + cols]
    hough = _hough()
    assert np.array_equal(host(hough.houghLinesAccumulate(view, rho_bin, theta_bin, ctx=ctxs[0])),
                          H.hough_lines(mask, rho_bin, theta_bin))
    total = None
    cuts = [0, 1, rows // 3, rows - 1, rows]
    for r0, r1 in zip(cuts, cuts[1:]):
        got = _lines_band(ctxs[0], view[r0:r1], r0, rows, rho_bin, theta_bin)
        assert np.array_equal(got, H.hough_lines(mask[r0:r1], rho_bin, theta_bin, row0=r0, rows=rows)), (r0, r1)
        total = got if total is None else total + got
    assert np.array_equal(total, H.hough_lines(mask, rho_bin, theta_bin))


# ------------------------------------------------------------------ circles ------

def _seam_mask():
    """Points on the circle kernel's tile seams: x = 63 / 64 (and 127 / 128), y = 31 / 32 (and 63 / 64)."""
    m = np.zeros((100, 200), np.uint8)
    for y in (0, 1, 31, 32, 63, 64, 99):
        for x in (0, 1, 63, 64, 127, 128, 199):
            m[y, x] = 255
    return m


CIRCLE_CASES = [  # (id, mask factory, radius)
    ("dense_160x300_r30", lambda: np.full((160, 300), 255, np.uint8), 30),
    ("dense_96x400_r5", lambda: np.full((96, 400), 255, np.uint8), 5),
    ("rand0.3_200x333_r17", lambda: rand_mask(200, 333, 0.3, 4), 17),
] + [(f"seams_r{r}", _seam_mask, r) for r in (0, 1, 32, 64, 65, 150, 223, 1000, 2 ** 31 - 1, 2 ** 32 - 1)] + [
    ("cols32767_r30", lambda: rand_mask(3, 32767, 0.01, 5), 30),
    ("cols32767_r40000", lambda: rand_mask(3, 32767, 0.002, 6), 40000),
    ("cols32767_r2^31-1", lambda: rand_mask(3, 32767, 0.002, 7), 2 ** 31 - 1),
    ("rows32767_r30", lambda: rand_mask(32767, 3, 0.05, 8), 30),
    ("rows32767_r2^32-1", lambda: rand_mask(32767, 3, 0.01, 9), 2 ** 32 - 1),
    ("one_pixel_r0", lambda: np.full((1, 1), 255, np.uint8), 0),
]


@pytest.mark.parametrize("case", CIRCLE_CASES, ids=lambda c: c[0])
def test_circles(ctxs, case):
    name, make, radius = case
    hough = _hough()
    mask = make()
    exp = H.hough_circles(mask, radius)
    got = host(hough.houghCirclesAccumulate(dev(mask), radius, ctx=ctxs[0]))
    assert np.array_equal(got, exp), int((got != exp).sum())
    if radius > math.hypot(*mask.shape):
        assert not exp.any()
    if name.startswith("dense_160x300"):
        in_rows, listed = H.circle_tile_loads(mask, radius)
        assert in_rows > 8192 and listed > 2048  # more than one 2048-point chunk, and more than four
    if name.startswith("rand0.3"):  # the point list through the count / scan / emit launches
        assert np.array_equal(host(hough.houghCirclesAccumulate(dev(mask), radius, ctx=ctxs[1])), exp)


@pytest.mark.parametrize("rows,cols,cuts,radius", [
    (32767, 3, [0, 16000, 32700, 32766, 32767], 30),   # y near 2^15 - 1 in the packed (y << 15 | x) entries
    (32767, 3, [0, 32767 - 64, 32767], 2 ** 31 - 1),
    (90, 130, [0, 1, 31, 32, 89, 90], 7),
])
def test_circle_bands(ctxs, rows, cols, cuts, radius):
    mask = rand_mask(rows, cols, 0.05, rows + radius % 1000)
    total = None
    view = dev(mask)
    for r0, r1 in zip(cuts, cuts[1:]):
        got = _circles_band(ctxs[0], view[r0:r1], r0, rows, radius)
        assert np.array_equal(got, H.hough_circles(mask[r0:r1], radius, row0=r0, rows=rows)), (r0, r1)
        total = got if total is None else total + got
    assert np.array_equal(total, H.hough_circles(mask, radius))


# ------------------------------------------------------------------ peaks ------

def _isolated_peaks(n, seed):
    """n isolated positive cells on a zero accumulator: with threshold 1 exactly n candidates, many ties."""
    acc = np.zeros((200, 200), np.int32)
    ys, xs = np.mgrid[1:200:3, 1:200:3]
    pos = np.stack([ys.ravel(), xs.ravel()], 1)[:n]
    assert len(pos) == n
    acc[pos[:, 0], pos[:, 1]] = np.random.default_rng(seed).integers(1, 40, n)
    return acc


def _accs():
    rng = np.random.default_rng(23)
    yield "cand4095", _isolated_peaks(4095, 1), 1
    yield "cand4096", _isolated_peaks(4096, 2), 1
    yield "cand4097", _isolated_peaks(4097, 3), 1
    yield "int32_extremes", rng.choice(np.array([INT_MIN, INT_MIN + 1, -1, 0, 1, INT_MAX - 1, INT_MAX], np.int64),
                                       (64, 90)).astype(np.int32), INT_MIN
    yield "int32_random", rng.integers(INT_MIN, INT_MAX, (70, 50), endpoint=True).astype(np.int32), 0
    yield "negative", rng.integers(-1000, -990, (33, 35)).astype(np.int32), -995
    yield "row_1x6000", rng.integers(0, 9, (1, 6000)).astype(np.int32), 3
    yield "col_6000x1", rng.integers(0, 9, (6000, 1)).astype(np.int32), 3
    yield "ties_const", np.full((40, 50), 3, np.int32), 3


ACCS = list(_accs())


def _peak_form(num_peaks, ncand):
    if num_peaks > 64:
        return "per_round"
    return "topk_wave" if ncand <= 4096 else "rescan"


def _candidates(acc, thr):
    return int((H.local_maxima(acc) & (acc >= thr)).sum())


PEAK_CASES = [pytest.param(name, acc, thr, k, id=f"{_peak_form(k, _candidates(acc, thr))}-{name}-k{k}")
              for name, acc, thr in ACCS for k in (0, 1, 64, 65, 4096)]


@pytest.mark.parametrize("opt", [-1, 0, 1], ids=lambda v: f"compact{v}")
@pytest.mark.parametrize("name,acc,thr,num_peaks", PEAK_CASES)
def test_peaks(ctxs, name, acc, thr, num_peaks, opt):
    """The selection form is named in the id: topk_wave (one launch, <= 4096 candidates), rescan (one launch, a full
    pass per round), per_round (a launch per round, num_peaks > 64); the list compaction by compact-1 / 0 / 1."""
    hough = _hough()
    if name.startswith("cand"):
        assert _candidates(acc, thr) == int(name[4:])
    exp = H.hough_peaks(acc, num_peaks, thr)
    got = host(hough.findLocalMaxima(dev(acc), num_peaks, thr, ctx=ctxs[opt])).astype(np.uint32)
    assert np.array_equal(got, exp)
    if opt == 0 and num_peaks in (64, 4096):
        assert np.array_equal(exp, orc.hough_peaks(acc, num_peaks, thr))


@pytest.mark.parametrize("opt", [-1, 0, 1], ids=lambda v: f"compact{v}")
@pytest.mark.parametrize("num_peaks", [64, 300])
def test_peaks_above_one_million_cells(ctxs, num_peaks, opt):
    """1100 x 1000 cells = 269 chunks of 4096: the default takes the three launches, -1 forces the one-launch
    chained scan beyond its 256-chunk reach."""
    hough = _hough()
    acc = np.random.default_rng(num_peaks).integers(0, 60, (1100, 1000)).astype(np.int32)
    exp = H.hough_peaks(acc, num_peaks, 30)
    assert len(exp) == num_peaks
    got = host(hough.findLocalMaxima(dev(acc), num_peaks, 30, ctx=ctxs[opt])).astype(np.uint32)
    assert np.array_equal(got, exp)


# ------------------------------------------------------------------ edges ------

def _scene(rows, cols, seed):
    rng = np.random.default_rng(seed)
    img = np.full((rows, cols), 60, np.int64)
    img[rows // 4: 3 * rows // 4, cols // 5: 4 * cols // 5] = 190
    yy, xx = np.mgrid[0:rows, 0:cols]
    img[(yy - rows // 2) ** 2 + (xx - cols // 2) ** 2 < (min(rows, cols) // 6) ** 2] = 20
    img += rng.integers(-12, 13, (rows, cols))
    return np.clip(img, 0, 255).astype(np.uint8)


def _edges(img, gs, sigma, lo, hi, ctx=None):
    return host(_hough().generateEdge(dev(img), gs, sigma, lo, hi, ctx=ctx))


@pytest.mark.parametrize("rows,cols,gs,sigma,lo,hi", [(33, 35, 3, 1.0, 20, 60), (480, 640, 5, 1.4, 20, 60),
                                                      (1080, 1920, 5, 1.5, 30, 90), (2160, 3840, 3, 1.0, 35, 130)])
def test_generate_edge_sizes(rows, cols, gs, sigma, lo, hi):
    img = _scene(rows, cols, rows)
    assert np.array_equal(_edges(img, gs, sigma, lo, hi), E.generate_edge(img, gs, sigma, lo, hi))


@pytest.mark.parametrize("gs", list(range(1, 20, 2)))
def test_generate_edge_gaussian_sizes(gs):
    img = _scene(97, 131, gs)
    sigma = 0.0001 if gs == 1 else gs / 3.0
    exp = E.generate_edge(img, gs, sigma, 10, 50)
    assert np.array_equal(_edges(img, gs, sigma, 10, 50), exp)


def tile_crossings(path, tw=64, th=62):
    """How often a pixel path moves from one 64 x 62 hysteresis tile to another."""
    tiles = [((y + 1) // th, x // tw) for y, x in path]  # a tile's first owned row is 62 k (lane 1 of 62 k - 1)
    return sum(a != b for a, b in zip(tiles, tiles[1:]))


def test_hysteresis_long_serpentine_seeded_at_the_far_end():
    """A weak serpentine that crosses the 64 x 62 hysteresis tiles hundreds of times, with its only strong pixel at
    the far end: the flood has to come back through every crossing, one relaunch round at least per tile visit."""
    rows, cols = 250, 300
    path = _serpentine(rows, cols, step=4)
    img = _ramp_path_image(rows, cols, path, strong_at=len(path) - 1)
    assert tile_crossings(path) > 100
    exp = E.generate_edge(img, 1, 0.0001, 10, 60)
    assert (exp > 0).sum() > len(path) // 2  # the chain is promoted, not just the seed
    assert np.array_equal(_edges(img, 1, 0.0001, 10, 60), exp)


def test_hysteresis_diagonal_touches_at_tile_corners():
    """Weak pixels that meet only diagonally, on a pixel checkerboard around the tile corners (x = 63 / 64,
    y = 61 / 62 and 123 / 124) and along a one-pixel diagonal through them, seeded far away."""
    rows, cols = 190, 200
    img = np.full((rows, cols), 100, np.int64)
    yy, xx = np.mgrid[0:rows, 0:cols]
    near = (np.abs(xx - 63.5) < 6) | (np.abs(yy - 61.5) < 6) | (np.abs(yy - 123.5) < 6)
    img[near & ((yy + xx) % 2 == 0)] = 112
    for i in range(0, 180):
        img[i + 5, min(cols - 1, i + 2)] = 121
    img[2:5, 0:3] = 250
    img = np.clip(img, 0, 255).astype(np.uint8)
    for lo, hi in ((5, 200), (20, 90), (1, 3)):
        exp = E.generate_edge(img, 1, 0.0001, lo, hi)
        assert np.array_equal(_edges(img, 1, 0.0001, lo, hi), exp), (lo, hi)


# ------------------------------------------------------------------ chain ------

def _ps1_sections():
    import os
    from introtocomputervision_amd import config
    cfg = config.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "config", "ref", "ps1.yaml"))
    out = []
    for p in range(2, 9):
        e = config.edge_params(cfg, f"edge_detector_p{p}")
        lines = [k for k in cfg if k.startswith("hough_") and k.endswith(f"_p{p}") and "circle" not in k]
        circles = [k for k in cfg if k.startswith("hough_circle") and k.endswith(f"_p{p}")]
        out.append((p, e, config.hough_params(cfg, lines[0]) if lines else None,
                    config.hough_circle_params(cfg, circles[0]) if circles else None))
    return out


@pytest.mark.parametrize("p,edge,lines,circles", [pytest.param(*s, id=f"ps1_p{s[0]}") for s in _ps1_sections()])
def test_ps1_chain(ctxs, p, edge, lines, circles):
    """edge -> lines / circles -> peaks with each ps1.yaml problem's settings, every stage against the references."""
    from introtocomputervision_amd import synth
    hough = _hough()
    mask0 = synth.hough_mask(240, 320, n_lines=5, radii=(20, 30, 40))[0]
    noise = np.random.default_rng(p).integers(-15, 16, mask0.shape)
    img = np.clip(np.where(mask0 > 0, 200, 70) + noise, 0, 255).astype(np.uint8)
    gs, sigma, lo, hi = edge["gaussian_size"], edge["gaussian_sigma"], edge["lower_threshold"], edge["upper_threshold"]
    edges_d = hough.generateEdge(dev(img), gs, sigma, lo, hi, ctx=ctxs[0])
    exp_edges = E.generate_edge(img, gs, sigma, lo, hi)
    assert np.array_equal(host(edges_d), exp_edges)
    if lines:
        acc = hough.houghLinesAccumulate(edges_d, lines["rho_bin_size"], lines["theta_bin_size"], ctx=ctxs[0])
        exp_acc = H.hough_lines(exp_edges, lines["rho_bin_size"], lines["theta_bin_size"])
        assert np.array_equal(host(acc), exp_acc)
        got = host(hough.findLocalMaxima(acc, lines["num_peaks"], lines["threshold"], ctx=ctxs[0])).astype(np.uint32)
        assert np.array_equal(got, H.hough_peaks(exp_acc, lines["num_peaks"], lines["threshold"]))
    if circles:
        for radius in (circles["min_radius"], circles["max_radius"]):
            acc = hough.houghCirclesAccumulate(edges_d, radius, ctx=ctxs[0])
            exp_acc = H.hough_circles(exp_edges, radius)
            assert np.array_equal(host(acc), exp_acc), radius
            got = host(hough.findLocalMaxima(acc, circles["num_peaks"], circles["threshold"], ctx=ctxs[0]))
            assert np.array_equal(got.astype(np.uint32), H.hough_peaks(exp_acc, circles["num_peaks"], circles["threshold"]))
