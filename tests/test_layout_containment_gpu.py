"""Layout containment of the core `_dev` entry points: every call writes its output views and nothing else, and gives
the same bytes whatever the alignment and pitch of its images.

One table row per entry point.  A row yields one or more cases (kernel sizes, flags, options); every case is run twice
through _capi.lib:
  A, packed    -- every plane dense and 256-byte aligned (the layout the Python wrappers allocate),
  B, embedded  -- every image argument placed by tests/_layout.py: one element past a 256-byte boundary, an odd row
                  padding (pitch no multiple of 16 bytes), batch images a non-16-byte gap apart, 64 KiB margins.
Both blocks are sentinel-filled, and after each call _layout.check asserts that no byte outside the output views
changed (row padding, gaps, margins, rows outside a band, every input) and that every output equals `expected` byte for
byte.  `expected` comes from the numpy reference modules of this directory where one covers the operation -- then A
must equal it too -- and from call A otherwise; each row says which.

A layout differs from the rules above only where include/mi_cv.h states a requirement; the row quotes the sentence."""
import ctypes as C

import numpy as np
import pytest

import _edge_ref as E
import _hough_ref as H
import _layout as Y
import _lk_chain_ref as L
import _ps1_driver_ref as P1
import _ps4_feat_ref as F4
import _stereo_ref as S8

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from introtocomputervision_amd import _capi  # noqa: E402
from _layout_table import (Case, run_case, rng_of, lk_frames, image_f32, image_u8, flow_field, edge_mask, gradients,  # noqa: E402
                           pointer_array, canvas, stereo_pair, f32, u8, i8, i32, i64, u32)

lib = _capi.lib
Plane = Y.Plane

SHAPES = [(35, 69), (18, 60)]     # columns = 1 mod 4, just over one 64-column tile and 32 rows; a multiple of 4, under one tile
PYR_SHAPES = SHAPES + [(50, 76)]  # levels 50x76, 25x38, 13x19


# ------------------------------------------------------------------------------------------- flow / pyramid ------

def row_lk_flow_pyr(rows, cols):
    """Expected: _lk_chain_ref.lk_flow_pyr.  Window 7 and 15 (fused level kernels), 9 (generic kernels); 3 levels."""
    prev, nxt = lk_frames(rows, cols, 1)
    for win in (7, 9, 15):
        def call(h, S, st, win=win):
            return lib.micv_lk_flow_pyr_dev(h, S.ptr("prev"), S.ptr("next"), rows, cols, S.pitch("prev"), win, 3, S.ptr("u"),
                                            S.ptr("v"), S.pitch("u"), st)
        eu, ev = L.lk_flow_pyr(prev, nxt, win, 3)
        yield Case(f"win {win}", lambda: [[Plane("prev", prev), Plane("next", nxt), Plane("u", shape=(rows, cols), dtype=f32),
                                           Plane("v", shape=(rows, cols), dtype=f32)]],
                   ["u", "v"], call, lambda A, eu=eu, ev=ev: {"u": eu, "v": ev})


def row_lk_flow(rows, cols):
    """Expected: _lk_chain_ref.lk_flow."""
    prev, nxt = lk_frames(rows, cols, 2)
    for win in (7, 9):
        def call(h, S, st, win=win):
            return lib.micv_lk_flow_dev(h, S.ptr("prev"), S.ptr("next"), rows, cols, S.pitch("prev"), win, S.ptr("u"), S.ptr("v"),
                                        S.pitch("u"), st)
        eu, ev = L.lk_flow(prev, nxt, win)
        yield Case(f"win {win}", lambda: [[Plane("prev", prev), Plane("next", nxt), Plane("u", shape=(rows, cols), dtype=f32),
                                           Plane("v", shape=(rows, cols), dtype=f32)]],
                   ["u", "v"], call, lambda A, eu=eu, ev=ev: {"u": eu, "v": ev})


def row_lk_warp(rows, cols):
    """Expected: _lk_chain_ref.warp."""
    src, du, dv = image_f32(rows, cols, 3), flow_field(rows, cols, 4), flow_field(rows, cols, 5)

    def call(h, S, st):
        return lib.micv_lk_warp_dev(h, S.ptr("src"), S.pitch("src"), S.ptr("du"), S.ptr("dv"), S.pitch("du"), rows, cols,
                                    S.ptr("dst"), S.pitch("dst"), st)
    exp = L.warp(src, du, dv)
    yield Case("warp", lambda: [[Plane("src", src), Plane("du", du), Plane("dv", dv), Plane("dst", shape=(rows, cols), dtype=f32)]],
               ["dst"], call, lambda A: {"dst": exp})


def level_flow_size(mode, rows, cols):
    if mode == "none":
        return 0, 0
    if mode == "coarse":  # an odd level takes a coarse flow one row / column too big (expanded, then resized)
        return (rows + 1) // 2, (cols + 1) // 2
    return max(rows // 3, 1), (cols + 5) // 2


def level_cases(rows, cols, batch):
    """Expected: _lk_chain_ref.level_step per pair.  A band strictly inside the image: the rows outside it stay sentinel.
    mi_cv.h: "flow_u/flow_v the coarser level's flow (flow_rows x flow_cols, dense pitch)" -- the coarse flow has no row
    padding; the pairs of a batch keep their gap ("its coarse flow at flow_u + i*flow_pair_stride": two rows and three
    floats in B, no multiple of 16 bytes); prev / next and u / v are pitched."""
    band = (rows // 4 + 1, rows - rows // 4 - 1)
    for win in (7, 15, 9):  # fused level kernels (15: the benchmark's), generic kernels
        for mode in ("none", "coarse", "full"):
            fr, fc = level_flow_size(mode, rows, cols)
            pairs = [lk_frames(rows, cols, 10 + i) for i in range(batch)]
            prev, nxt = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
            if fr:
                cu = np.stack([flow_field(fr, fc, 20 + i) for i in range(batch)])
                cv = np.stack([flow_field(fr, fc, 30 + i) for i in range(batch)])
            exp = [L.level_step(prev[i], nxt[i], cu[i] if fr else None, cv[i] if fr else None, win) for i in range(batch)]
            eu, ev = np.stack([e[0] for e in exp]), np.stack([e[1] for e in exp])

            def planes(prev=prev, nxt=nxt, fr=fr, cu=cu if fr else None, cv=cv if fr else None):
                one = (lambda a: a[0]) if batch == 1 else (lambda a: a)
                shape = (rows, cols) if batch == 1 else (batch, rows, cols)
                g = [Plane("prev", one(prev)), Plane("next", one(nxt)), Plane("u", shape=shape, dtype=f32, band=band),
                     Plane("v", shape=shape, dtype=f32, band=band)]
                if fr:
                    g += [Plane("fu", one(cu), dense=True), Plane("fv", one(cv), dense=True)]
                return [g]

            def call(h, S, st, win=win, fr=fr, fc=fc):
                fu, fv = (S.ptr("fu"), S.ptr("fv")) if fr else (None, None)
                if batch == 1:
                    return lib.micv_lk_level_dev(h, S.ptr("prev"), S.ptr("next"), rows, cols, S.pitch("prev"), win, fu, fv, fr, fc,
                                                 band[0], band[1], S.ptr("u"), S.ptr("v"), S.pitch("u"), st)
                return lib.micv_lk_level_batch_dev(h, S.ptr("prev"), S.ptr("next"), batch, S.dist("prev"), rows, cols, S.pitch("prev"),
                                                   win, fu, fv, fr, fc, S.dist("fu") if fr else 0, band[0], band[1], S.ptr("u"),
                                                   S.ptr("v"), S.dist("u"), S.pitch("u"), st)
            yield Case(f"win {win} {mode} band {band}", planes, ["u", "v"], call,
                       lambda A, eu=eu, ev=ev: {"u": eu if batch > 1 else eu[0], "v": ev if batch > 1 else ev[0]})


def row_lk_level(rows, cols):
    yield from level_cases(rows, cols, 1)


def row_lk_level_batch(rows, cols):
    yield from level_cases(rows, cols, 3)


def row_pyr_down(rows, cols):
    """Expected: _lk_chain_ref.pyr_down."""
    src = image_f32(rows, cols, 6)

    def call(h, S, st):
        return lib.micv_pyr_down_dev(h, S.ptr("src"), rows, cols, S.pitch("src"), S.ptr("dst"), S.pitch("dst"), st)
    yield Case("pyrDown", lambda: [[Plane("src", src), Plane("dst", shape=(rows // 2, cols // 2), dtype=f32)]], ["dst"], call,
               lambda A: {"dst": L.pyr_down(src)})


def row_pyr_up(rows, cols):
    """Expected: _lk_chain_ref.pyr_up.  The shape is the OUTPUT's where it is even (18 x 60 from 9 x 30); 35 x 69 cannot
    be a pyrUp output (dst is 2 rows x 2 cols), so the input has that shape and the output is 70 x 138."""
    srows, scols = (rows // 2, cols // 2) if rows % 2 == 0 and cols % 2 == 0 else (rows, cols)
    src = image_f32(srows, scols, 7)

    def call(h, S, st):
        return lib.micv_pyr_up_dev(h, S.ptr("src"), srows, scols, S.pitch("src"), S.ptr("dst"), S.pitch("dst"), st)
    yield Case("pyrUp", lambda: [[Plane("src", src), Plane("dst", shape=(2 * srows, 2 * scols), dtype=f32)]], ["dst"], call,
               lambda A: {"dst": L.pyr_up(src)})


def row_resize_linear(rows, cols):
    """Expected: _lk_chain_ref.resize_linear.  The two uses of the chain: one row / column more than the source, and the
    expanded flow of another ratio (more rows, fewer columns)."""
    for srows, scols in ((rows - 1, cols - 1), (2 * (rows // 3), 2 * ((cols + 5) // 2))):
        src = image_f32(srows, scols, 8)

        def call(h, S, st, srows=srows, scols=scols):
            return lib.micv_resize_linear_dev(h, S.ptr("src"), srows, scols, S.pitch("src"), S.ptr("dst"), rows, cols, S.pitch("dst"), st)
        yield Case(f"{srows}x{scols} -> {rows}x{cols}", lambda src=src: [[Plane("src", src), Plane("dst", shape=(rows, cols), dtype=f32)]],
                   ["dst"], call, lambda A, src=src: {"dst": L.resize_linear(src, rows, cols)})


def pyramid_cases(fn, reference, rows, cols):
    """mi_cv.h: "level l is (rows>>l) x (cols>>l), written densely (pitch = cols_l*4) at dst_levels[l]" -- the levels have
    no row padding; they keep the one-element base offset and the margins, and the source is pitched."""
    src = image_f32(rows, cols, 9)
    names = ["l0", "l1", "l2"]

    def planes():
        return [[Plane("src", src)] + [Plane(n, shape=(rows >> l, cols >> l), dtype=f32, dense=True) for l, n in enumerate(names)]]

    def call(h, S, st):
        return fn(h, S.ptr("src"), rows, cols, S.pitch("src"), 3, pointer_array([S.ptr(n) for n in names]), st)
    yield Case("3 levels", planes, names, call, lambda A: dict(zip(names, reference(src, 3))))


def row_gaussian_pyramid(rows, cols):
    """Expected: _lk_chain_ref.gaussian_pyramid."""
    yield from pyramid_cases(lib.micv_gaussian_pyramid_dev, L.gaussian_pyramid, rows, cols)


def row_laplacian_pyramid(rows, cols):
    """Expected: _lk_chain_ref.laplacian_pyramid."""
    yield from pyramid_cases(lib.micv_laplacian_pyramid_dev, L.laplacian_pyramid, rows, cols)


def row_gaussian_pyramid_batch(rows, cols):
    """Expected: _lk_chain_ref.gaussian_pyramid per image.  mi_cv.h: "level l of image i at dst_levels[l] + i*rows_l*cols_l
    floats, dense" -- levels without row padding and without a gap between the images (dense, tight); the source images
    are pitched and a gap apart.  Last case: row bands per level ("level l is written for rows [row_begin[l], row_end[l]) only") and
    "dst_levels[0] may be NULL = no level-0 copy": rows outside the bands stay sentinel."""
    batch = 3
    src = np.stack([image_f32(rows, cols, 40 + i) for i in range(batch)])
    names = ["l0", "l1", "l2"]
    exp = [np.stack([L.gaussian_pyramid(src[i], 3)[l] for i in range(batch)]) for l in range(3)]
    # without level 0 and without bands the packed call takes the 16-byte-per-lane build where cols % 4 == 0
    for tag, bands, used in (("all rows", None, names), ("all rows, no level 0", None, names[1:]),
                             ("row bands, no level 0", [(0, 0), ((rows >> 1) // 3, (rows >> 1) - 2), (1, (rows >> 2) - 1)], names[1:])):

        def planes(bands=bands, used=used):
            return [[Plane("src", src)] + [Plane(n, shape=(batch, rows >> int(n[1]), cols >> int(n[1])), dtype=f32, dense=True, tight=True,
                                                 band=bands[int(n[1])] if bands else None) for n in used]]

        def call(h, S, st, bands=bands, used=used):
            ptrs = [S.ptr(n) if n in used else None for n in names]
            rb = (C.c_int * 3)(*[b[0] for b in bands]) if bands else None
            re = (C.c_int * 3)(*[b[1] for b in bands]) if bands else None
            return lib.micv_gaussian_pyramid_batch_dev(h, S.ptr("src"), batch, S.dist("src"), rows, cols, S.pitch("src"), 3,
                                                       pointer_array(ptrs), rb, re, st)
        yield Case(tag, planes, used, call, lambda A, used=used: {n: exp[int(n[1])] for n in used})


def row_rgb8_to_gray(rows, cols):
    """Expected: _lk_chain_ref.to_gray."""
    rgb = rng_of(rows, cols, 50).integers(0, 256, (rows, cols, 3)).astype(u8)

    def call(h, S, st):
        return lib.micv_rgb8_to_gray_f32_dev(h, S.ptr("src"), rows, cols, S.pitch("src"), S.ptr("dst"), S.pitch("dst"), st)
    yield Case("rgb8", lambda: [[Plane("src", rgb.reshape(rows, cols * 3)), Plane("dst", shape=(rows, cols), dtype=f32)]], ["dst"], call,
               lambda A: {"dst": L.to_gray(rgb)})


def row_to_gray(rows, cols):
    """Expected: _lk_chain_ref.to_gray.  Every depth (MICV_DEPTH_8U, MICV_DEPTH_32F) and channel count (1, 3, 4) of the
    header."""
    for dtype, depth in ((u8, _capi.DEPTH_8U), (f32, _capi.DEPTH_32F)):
        for cn in (1, 3, 4):
            r = rng_of(rows, cols, 51 + cn)
            img = r.integers(0, 256, (rows, cols, cn)).astype(dtype)
            if dtype is f32:
                img = (img * f32(1.3) + r.standard_normal(img.shape).astype(f32)).astype(f32)
            frame = img[:, :, 0] if cn == 1 else img

            def call(h, S, st, cn=cn, depth=depth):
                return lib.micv_to_gray_f32_dev(h, S.ptr("src"), rows, cols, S.pitch("src"), cn, depth, S.ptr("dst"), S.pitch("dst"), st)
            yield Case(f"{np.dtype(dtype).name} x {cn}", lambda img=img, cn=cn: [[Plane("src", img.reshape(rows, cols * cn)),
                                                                                  Plane("dst", shape=(rows, cols), dtype=f32)]],
                       ["dst"], call, lambda A, frame=frame: {"dst": L.to_gray(frame)})


# ---------------------------------------------------------------------------------------- gradients / corners ----

def row_sobel(rows, cols):
    """Expected: _ps4_feat_ref.sobel3 for the 3 x 3 kernel (fused and under MICV_OPT_SOBEL_GENERIC); no reference module
    covers sizes 5, 7 (fused) and 9 (generic LDS row / column kernels): expected is the packed call."""
    src = image_f32(rows, cols, 60)
    for ksize, opts in ((3, {}), (5, {}), (7, {}), (9, {}), (3, {"SOBEL_GENERIC": 1})):
        def call(h, S, st, ksize=ksize):
            return lib.micv_sobel_dev(h, S.ptr("src"), rows, cols, S.pitch("src"), ksize, 1.0, S.ptr("gx"), S.ptr("gy"), S.pitch("gx"), st)
        ref = (lambda A: dict(zip(("gx", "gy"), F4.sobel3(src)))) if ksize == 3 else None
        yield Case(f"ksize {ksize} {opts}", lambda: [[Plane("src", src), Plane("gx", shape=(rows, cols), dtype=f32),
                                                       Plane("gy", shape=(rows, cols), dtype=f32)]], ["gx", "gy"], call, ref, opts)


def response_cases(rows, cols, ex):
    """No reference module of the list covers the response (tests/_f64_ref.py bounds it, it does not restate its bits):
    expected is the packed call.  Windows 3, 5, 7 (tiled kernels) and 9 (generic), each also under MICV_OPT_HARRIS_GENERIC;
    the _ex entry with harris::gpu and harris::cpu arithmetic."""
    gx, gy = gradients(rows, cols, 61)
    for win in (3, 5, 7, 9):
        for opts in ({}, {"HARRIS_GENERIC": 1}):
            for flags in ((0, 1) if ex else (None,)):
                def call(h, S, st, win=win, flags=flags):
                    a = (h, S.ptr("gx"), S.ptr("gy"), rows, cols, S.pitch("gx"), win, win / 3.0, 0.04)
                    b = (S.ptr("resp"), S.pitch("resp"), st)
                    return lib.micv_harris_response_ex_dev(*a, flags, *b) if ex else lib.micv_harris_response_dev(*a, *b)
                yield Case(f"win {win} {opts} flags {flags}", lambda: [[Plane("gx", gx), Plane("gy", gy),
                                                                        Plane("resp", shape=(rows, cols), dtype=f32)]],
                           ["resp"], call, None, opts)


def row_harris_response(rows, cols):
    yield from response_cases(rows, cols, False)


def row_harris_response_ex(rows, cols):
    yield from response_cases(rows, cols, True)


def row_harris_refine(rows, cols):
    """Expected: _ps4_feat_ref.refine_corners (map, list, count).  Both NMS forms (MICV_OPT_NMS_SCAN), a capacity above the
    count and one below it (mi_cv.h: "*count receives the number found (may exceed cap)"); list entries between the
    count and the capacity are not asserted, entry `cap` and beyond must stay sentinel."""
    R = rng_of(rows, cols, 62).standard_normal((rows, cols)).astype(f32)
    corners, locs = F4.refine_corners(R, 0.5, 2)
    assert len(locs) > 8
    for opts in ({}, {"NMS_SCAN": 1}):
        for cap in (rows * cols, 5):
            def call(h, S, st, cap=cap):
                return lib.micv_harris_refine_dev(h, S.ptr("resp"), rows, cols, S.pitch("resp"), 0.5, 2, S.ptr("corners"), S.pitch("corners"),
                                                  S.ptr("locs"), cap, S.ptr("count"), st)
            yield Case(f"{opts} cap {cap}", lambda cap=cap: [[Plane("resp", R), Plane("corners", shape=(rows, cols), dtype=f32),
                                                              Plane("locs", shape=(cap, 2), dtype=i32, dense=True),
                                                              Plane("count", shape=(1, 1), dtype=i64, dense=True)]],
                       ["corners", "locs", "count"], call,
                       lambda A, cap=cap: {"corners": corners, "locs": locs[:cap], "count": np.array([[len(locs)]], i64)}, opts)


def row_harris_corners(rows, cols):
    """Every optional plane requested.  Expected: gx, gy from _ps4_feat_ref.sobel3; the response from the packed call (no
    reference module restates it); map, list and count from _ps4_feat_ref.refine_corners on that response.  Window 5: the
    fused form (gradients inside the response kernel); window 9: the three launches of the separate entry points."""
    img = image_f32(rows, cols, 63)
    egx, egy = F4.sobel3(img)
    cap = rows * cols
    for win in (5, 9):
        def call(h, S, st, win=win):
            return lib.micv_harris_corners_dev(h, S.ptr("img"), rows, cols, S.pitch("img"), 3, win, win / 3.0, 0.04, 0, 1e6, 2,
                                               S.ptr("gx"), S.ptr("gy"), S.pitch("gx"), S.ptr("resp"), S.pitch("resp"), S.ptr("corners"),
                                               S.pitch("corners"), S.ptr("locs"), cap, S.ptr("count"), st)

        def ref(A):
            corners, locs = F4.refine_corners(A["resp"], 1e6, 2)
            return {"gx": egx, "gy": egy, "corners": corners, "locs": locs[:cap], "count": np.array([[len(locs)]], i64)}
        yield Case(f"win {win}", lambda: [[Plane("img", img)] + [Plane(n, shape=(rows, cols), dtype=f32) for n in ("gx", "gy", "resp", "corners")]
                                          + [Plane("locs", shape=(cap, 2), dtype=i32, dense=True), Plane("count", shape=(1, 1), dtype=i64, dense=True)]],
                   ["gx", "gy", "resp", "corners", "locs", "count"], call, ref)


def row_sift_angles(rows, cols):
    """atan2f-based: the packed call within the existing test's atol = 1e-5 rad (tests/test_ps124_gpu.py) of atan2 in
    float64 rounded to float (the arithmetic _ps4_feat_ref.keypoints gives the same step), and B byte-equal to A."""
    gx, gy = gradients(rows, cols, 64)
    exp = np.arctan2(gy.astype(np.float64), gx.astype(np.float64)).astype(f32)

    def call(h, S, st):
        return lib.micv_sift_angles_dev(h, S.ptr("gx"), S.ptr("gy"), rows, cols, S.pitch("gx"), S.ptr("ang"), S.pitch("ang"), st)
    yield Case("angles", lambda: [[Plane("gx", gx), Plane("gy", gy), Plane("ang", shape=(rows, cols), dtype=f32)]], ["ang"], call,
               lambda A: {"ang": exp}, approx={"ang": lambda got, ref: np.allclose(got, ref, rtol=0, atol=1e-5)})


# ------------------------------------------------------------------------------------------------- stereo --------

def row_disparity_ssd(rows, cols):
    """Expected: _stereo_ref.ssd_cuda / ssd_serial (8-bit-valued float images: ROLLING gives the fresh sums' result there).
    Flags 0, COLS_2R, SERIAL, ROLLING under MICV_OPT_STEREO_EXACT 0 (exact-sum kernels) and -1 (float kernels); radius 2."""
    left, right = stereo_pair(rows, cols, 70)
    rad, lo, hi = 2, -6, 3
    for exact in (0, -1):
        for flags in (0, _capi.STEREO_COLS_2R, _capi.STEREO_SERIAL, _capi.STEREO_ROLLING):
            def call(h, S, st, flags=flags):
                return lib.micv_disparity_ssd_dev(h, S.ptr("left"), S.ptr("right"), rows, cols, S.pitch("left"), rad, lo, hi, flags,
                                                  S.ptr("disp"), S.pitch("disp"), st)
            exp = S8.ssd_serial(left, right, rad, lo, hi) if flags == _capi.STEREO_SERIAL else S8.ssd_cuda(left, right, rad, lo, hi, flags & 3)
            yield Case(f"flags {flags} exact {exact}", lambda: [[Plane("left", left), Plane("right", right),
                                                                  Plane("disp", shape=(rows, cols), dtype=i8)]],
                       ["disp"], call, lambda A, exp=exp: {"disp": exp}, {"STEREO_EXACT": exact})


def row_disparity_ncorr(rows, cols):
    """No reference module of the list covers disparityNCorr (_stereo_ref / _stereo_f32_ref restate the SSD): expected is
    the packed call.  Radius 2 (tile form), flags 0, COLS_2R and ROLLING (strip-serial kernel)."""
    left, right = stereo_pair(rows, cols, 71)
    for flags in (0, _capi.STEREO_COLS_2R, _capi.STEREO_ROLLING):
        def call(h, S, st, flags=flags):
            return lib.micv_disparity_ncorr_dev(h, S.ptr("left"), S.ptr("right"), rows, cols, S.pitch("left"), 2, -6, 3, flags,
                                                S.ptr("disp"), S.pitch("disp"), st)
        yield Case(f"flags {flags}", lambda: [[Plane("left", left), Plane("right", right), Plane("disp", shape=(rows, cols), dtype=i8)]],
                   ["disp"], call)


# --------------------------------------------------------------------------------------------------- ps1 ---------

def filter_cases(fn, src, out_dtype, args, reference, tag):
    rows, cols = src.shape

    def call(h, S, st):
        return fn(h, S.ptr("src"), rows, cols, S.pitch("src"), *args, S.ptr("dst"), S.pitch("dst"), st)
    return Case(tag, lambda: [[Plane("src", src), Plane("dst", shape=(rows, cols), dtype=out_dtype)]], ["dst"], call,
                lambda A: {"dst": reference()})


def row_generate_edge(rows, cols):
    """Expected: _edge_ref.generate_edge.  Gaussian 3 and 5."""
    img = image_u8(rows, cols, 80)
    for gs in (3, 5):
        yield filter_cases(lib.micv_generate_edge_dev, img, u8, (gs, gs / 3.0, 20.0, 60.0),
                           lambda gs=gs: E.generate_edge(img, gs, gs / 3.0, 20.0, 60.0), f"gauss {gs}")


def row_generate_edge_f32(rows, cols):
    """Expected: _ps1_driver_ref.generate_edge_f32."""
    img = (image_u8(rows, cols, 81).astype(f32) * f32(1.01) + f32(0.25)).astype(f32)
    for gs in (3, 5):
        yield filter_cases(lib.micv_generate_edge_f32_dev, img, u8, (gs, gs / 3.0, 20.0, 60.0),
                           lambda gs=gs: P1.generate_edge_f32(img, gs, gs / 3.0, 20.0, 60.0), f"gauss {gs}")


def row_gaussian_blur_u8(rows, cols):
    """Expected: _edge_ref.blur."""
    img = image_u8(rows, cols, 82)
    for gs in (3, 5):
        yield filter_cases(lib.micv_gaussian_blur_u8_dev, img, u8, (gs, gs / 3.0), lambda gs=gs: E.blur(img, gs, gs / 3.0), f"gauss {gs}")


def row_gaussian_blur_f32(rows, cols):
    """Expected: _ps1_driver_ref.blur_f32."""
    img = image_f32(rows, cols, 83)
    for gs in (3, 5):
        yield filter_cases(lib.micv_gaussian_blur_f32_dev, img, f32, (gs, gs / 3.0), lambda gs=gs: P1.blur_f32(img, gs, gs / 3.0), f"gauss {gs}")


def row_erode_u8(rows, cols):
    """Expected: _ps1_driver_ref.erode.  Every footprint but the identity: 3, 5, 7."""
    img = image_u8(rows, cols, 84)
    for k in (3, 5, 7):
        yield filter_cases(lib.micv_erode_ellipse_u8_dev, img, u8, (k,), lambda k=k: P1.erode(img, k), f"ksize {k}")


def row_erode_f32(rows, cols):
    """Expected: _ps1_driver_ref.erode."""
    img = image_f32(rows, cols, 85)
    for k in (3, 5, 7):
        yield filter_cases(lib.micv_erode_ellipse_f32_dev, img, f32, (k,), lambda k=k: P1.erode(img, k), f"ksize {k}")


def row_gray_to_rgb8(rows, cols):
    """Expected: _ps1_driver_ref.gray2rgb.  Both source depths."""
    g8 = image_u8(rows, cols, 86)
    gf = (g8.astype(f32) * f32(1.2) - f32(20.5)).astype(f32)  # halves to round, values below 0 and above 255 to saturate
    for img, depth in ((g8, _capi.DEPTH_8U), (gf, _capi.DEPTH_32F)):
        def call(h, S, st, depth=depth):
            return lib.micv_gray_to_rgb8_dev(h, S.ptr("src"), depth, rows, cols, S.pitch("src"), S.ptr("dst"), S.pitch("dst"), st)
        yield Case(f"depth {depth}", lambda img=img: [[Plane("src", img), Plane("dst", shape=(rows, cols * 3), dtype=u8)]], ["dst"], call,
                   lambda A, img=img: {"dst": P1.gray2rgb(img).reshape(rows, cols * 3)})


def row_draw_lines(rows, cols):
    """Expected: _ps1_driver_ref.draw_lines.  The image is input and output; peaks and count (no pitch in the header)
    ride in the block as dense inputs.  Lines of every octant, one through a corner, one peak with theta >= 180 (not
    drawn), a count below max_peaks."""
    img = canvas(rows, cols, 87)
    _, _, diag = H.lines_dims(rows, cols, 1, 1)
    peaks = np.array([[diag + 10, 120], [diag + 20, 135], [diag + 5, 90], [diag + 12, 0], [diag - 8, 60], [diag, 45],
                      [diag + 3, 200], [diag + 15, 100]], u32)
    n = 7  # the last peak is beyond the count
    exp = P1.draw_lines(img.reshape(rows, cols, 3), peaks[:n], 1, 1, (0, 255, 0)).reshape(rows, cols * 3)
    assert (exp != img).any()
    color = (C.c_uint8 * 3)(0, 255, 0)

    def call(h, S, st):
        return lib.micv_draw_lines_parametric_dev(h, S.ptr("img"), rows, cols, S.pitch("img"), S.ptr("peaks"), S.ptr("count"), len(peaks),
                                                  1, 1, color, st)
    yield Case("lines", lambda: [[Plane("img", img), Plane("peaks", peaks, dense=True), Plane("count", np.array([[n]], i64), dense=True)]],
               ["img"], call, lambda A: {"img": exp})


def row_draw_circles(rows, cols):
    """Expected: _ps1_driver_ref.draw_circles.  Three radii, centres inside, on the border and outside the image."""
    img = canvas(rows, cols, 88)
    peaks = np.array([[[rows // 2, cols // 2], [0, 0], [rows - 1, cols - 1]],
                      [[rows // 3, cols // 4], [rows + 2, cols // 2], [5, 5]],
                      [[rows // 2, cols - 3], [2, cols // 3], [rows - 4, 7]]], u32)
    counts = np.array([3, 2, 3], i64)
    exp = P1.draw_circles(img.reshape(rows, cols, 3), peaks, counts, 4, (255, 0, 64)).reshape(rows, cols * 3)
    assert (exp != img).any()
    color = (C.c_uint8 * 3)(255, 0, 64)

    def call(h, S, st):
        return lib.micv_draw_circles_dev(h, S.ptr("img"), rows, cols, S.pitch("img"), S.ptr("peaks"), S.ptr("counts"), 3, 3, 4, color, st)
    yield Case("circles", lambda: [[Plane("img", img), Plane("peaks", peaks.reshape(9, 2), dense=True),
                                    Plane("counts", counts.reshape(3, 1), dense=True)]], ["img"], call, lambda A: {"img": exp})


def hough_cases(rows, cols, lines, banded):
    """mi_cv.h: "acc i32 [rho_bins x theta_bins] (dense, zeroed here)" / "acc i32 [rows x cols] (dense, zeroed here)" -- the
    accumulator has no row padding; it sits in a block of its own, so the margins on both sides of it are checked.  The mask
    is embedded; a band call gets the pointer to row `row0` of it."""
    mask = edge_mask(rows, cols, 90)
    row0, nb = (rows // 4, rows // 2) if banded else (0, rows)
    for par in ((1, 1), (2, 3)) if lines else (3, 6):
        if lines:
            rb, tb, _ = H.lines_dims(rows, cols, *par)
            exp = H.hough_lines(mask[row0:row0 + nb], par[0], par[1], row0=row0, rows=rows)
            shape = (rb, tb)
        else:
            exp = H.hough_circles(mask[row0:row0 + nb], par, row0=row0, rows=rows)
            shape = (rows, cols)
        assert exp.shape == shape and exp.any()

        def call(h, S, st, par=par):
            m = (S.ptr("mask", 0, row0), nb, cols, S.pitch("mask"), row0, rows) if banded else (S.ptr("mask"), rows, cols, S.pitch("mask"))
            tail = (*par, S.ptr("acc"), st) if lines else (par, S.ptr("acc"), st)
            name = "micv_hough_" + ("lines" if lines else "circles") + ("_band" if banded else "") + "_dev"
            return getattr(lib, name)(h, *m, *tail)
        yield Case(f"{par} rows {row0}..{row0 + nb}", lambda shape=shape: [[Plane("mask", mask)], [Plane("acc", shape=shape, dtype=i32, dense=True)]],
                   ["acc"], call, lambda A, exp=exp: {"acc": exp})


def row_hough_lines(rows, cols):
    """Expected: _hough_ref.hough_lines.  Bins (1, 1) and (2, 3)."""
    yield from hough_cases(rows, cols, True, False)


def row_hough_circles(rows, cols):
    """Expected: _hough_ref.hough_circles.  Radius 3 and 6."""
    yield from hough_cases(rows, cols, False, False)


def row_hough_lines_band(rows, cols):
    """Expected: _hough_ref.hough_lines(row0, rows) of the band's rows."""
    yield from hough_cases(rows, cols, True, True)


def row_hough_circles_band(rows, cols):
    """Expected: _hough_ref.hough_circles(row0, rows) of the band's rows."""
    yield from hough_cases(rows, cols, False, True)


# ------------------------------------------------------------------------------------------------ matching -------

def row_bf_knn2(rows, cols):
    """Expected: _ps4_feat_ref.knn2, indices and distance bytes.  dim % 4 == 0: in A the descriptor rows are 16-byte aligned
    (the vector form), in B the same rows start one float past a 256-byte boundary with an odd row padding (the scalar
    form): both must give the reference's bytes.  `rows`, `cols` are the query and train counts; dim 8 and 128 (SIFT),
    and 6 (no vector form).  idx2 / dist2 have no pitch in the header: dense lists."""
    nq, nt = cols, rows
    for dim in (8, 128, 6):
        r = rng_of(nq, nt, dim)
        q = r.integers(0, 256, (nq, dim)).astype(f32)
        t = r.integers(0, 256, (nt, dim)).astype(f32)
        t[3] = t[1]  # a tie, resolved by index
        q[2] = t[1]
        idx, dist = F4.knn2(q, t)

        def call(h, S, st, dim=dim):
            return lib.micv_bf_knn2_dev(h, S.ptr("q"), nq, S.pitch("q"), S.ptr("t"), nt, S.pitch("t"), dim, S.ptr("idx2"), S.ptr("dist2"), st)
        yield Case(f"dim {dim}", lambda q=q, t=t: [[Plane("q", q), Plane("t", t), Plane("idx2", shape=(nq, 2), dtype=i32, dense=True),
                                                    Plane("dist2", shape=(nq, 2), dtype=f32, dense=True)]],
                   ["idx2", "dist2"], call, lambda A, idx=idx, dist=dist: {"idx2": idx, "dist2": dist})


def row_bf_ratio_filter(rows, cols):
    """Expected: _ps4_feat_ref.ratio_filter.  No argument has a pitch: every list is dense, one element past a 256-byte
    boundary in B.  A capacity above the count and one below it."""
    nq = rows * 2 + 1
    r = rng_of(nq, cols, 95)
    q = r.integers(0, 64, (nq, 8)).astype(f32)
    t = r.integers(0, 64, (cols, 8)).astype(f32)
    idx, dist = F4.knn2(q, t)
    m, d, count = F4.ratio_filter(idx, dist, 0.8)
    assert count > 4
    for cap in (nq, 3):
        def call(h, S, st, cap=cap):
            return lib.micv_bf_ratio_filter_dev(h, S.ptr("idx2"), S.ptr("dist2"), nq, 0.8, S.ptr("matches"), S.ptr("distances"), cap,
                                                S.ptr("count"), st)
        yield Case(f"cap {cap}", lambda cap=cap: [[Plane("idx2", idx, dense=True), Plane("dist2", dist, dense=True),
                                                   Plane("matches", shape=(cap, 2), dtype=i32, dense=True),
                                                   Plane("distances", shape=(cap, 1), dtype=f32, dense=True),
                                                   Plane("count", shape=(1, 1), dtype=i64, dense=True)]],
                   ["matches", "distances", "count"], call,
                   lambda A, cap=cap: {"matches": m[:cap], "distances": d[:cap].reshape(-1, 1), "count": np.array([[count]], i64)})


# ------------------------------------------------------------------------------------------------- the table -----

TABLE = {
    "micv_lk_flow_pyr_dev": (row_lk_flow_pyr, PYR_SHAPES),
    "micv_lk_flow_dev": (row_lk_flow, SHAPES),
    "micv_lk_warp_dev": (row_lk_warp, SHAPES),
    "micv_lk_level_dev": (row_lk_level, SHAPES),
    "micv_lk_level_batch_dev": (row_lk_level_batch, SHAPES),
    "micv_pyr_down_dev": (row_pyr_down, SHAPES),
    "micv_pyr_up_dev": (row_pyr_up, SHAPES),
    "micv_resize_linear_dev": (row_resize_linear, SHAPES),
    "micv_gaussian_pyramid_dev": (row_gaussian_pyramid, PYR_SHAPES),
    "micv_gaussian_pyramid_batch_dev": (row_gaussian_pyramid_batch, PYR_SHAPES),
    "micv_laplacian_pyramid_dev": (row_laplacian_pyramid, PYR_SHAPES),
    "micv_rgb8_to_gray_f32_dev": (row_rgb8_to_gray, SHAPES),
    "micv_to_gray_f32_dev": (row_to_gray, SHAPES),
    "micv_sobel_dev": (row_sobel, SHAPES),
    "micv_harris_response_dev": (row_harris_response, SHAPES),
    "micv_harris_response_ex_dev": (row_harris_response_ex, SHAPES),
    "micv_harris_refine_dev": (row_harris_refine, SHAPES),
    "micv_harris_corners_dev": (row_harris_corners, SHAPES),
    "micv_sift_angles_dev": (row_sift_angles, SHAPES),
    "micv_disparity_ssd_dev": (row_disparity_ssd, SHAPES),
    "micv_disparity_ncorr_dev": (row_disparity_ncorr, SHAPES),
    "micv_generate_edge_dev": (row_generate_edge, SHAPES),
    "micv_generate_edge_f32_dev": (row_generate_edge_f32, SHAPES),
    "micv_gaussian_blur_u8_dev": (row_gaussian_blur_u8, SHAPES),
    "micv_gaussian_blur_f32_dev": (row_gaussian_blur_f32, SHAPES),
    "micv_erode_ellipse_u8_dev": (row_erode_u8, SHAPES),
    "micv_erode_ellipse_f32_dev": (row_erode_f32, SHAPES),
    "micv_gray_to_rgb8_dev": (row_gray_to_rgb8, SHAPES),
    "micv_draw_lines_parametric_dev": (row_draw_lines, SHAPES),
    "micv_draw_circles_dev": (row_draw_circles, SHAPES),
    "micv_hough_lines_dev": (row_hough_lines, SHAPES),
    "micv_hough_circles_dev": (row_hough_circles, SHAPES),
    "micv_hough_lines_band_dev": (row_hough_lines_band, SHAPES),
    "micv_hough_circles_band_dev": (row_hough_circles_band, SHAPES),
    "micv_bf_knn2_dev": (row_bf_knn2, SHAPES),
    "micv_bf_ratio_filter_dev": (row_bf_ratio_filter, SHAPES),
}

# Collection time: a misspelt row fails the whole module; tests/test_layout_containment_drivers_gpu.py accounts for every
# `_dev` entry point of _capi.SIGNATURES (this table, its own, or an exemption with a reason).
assert all(name in _capi.SIGNATURES for name in TABLE)

PARAMS = [pytest.param(name, shape, id=f"{name[5:]}-{shape[0]}x{shape[1]}") for name, (_, shapes) in TABLE.items() for shape in shapes]


@pytest.mark.parametrize("name,shape", PARAMS)
def test_containment(name, shape):
    cases = list(TABLE[name][0](*shape))
    assert cases, name
    for case in cases:
        case.tag = f"{name} {shape[0]}x{shape[1]} {case.tag}"
        run_case(case)
