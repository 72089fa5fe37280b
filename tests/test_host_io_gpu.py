"""The upload / download plumbing of the `_host` entry points, characterised without a reference: every entry is
called once with dense host arrays and once with every image operand in rows of a padded pitch (a different pad per
stride argument, the padding filled with 0xA5).  The two calls must return MICV_OK, leave every image operand and
every flat output byte-identical, and leave every padding byte untouched.  37x53 images take the 2-D copy when
pitched and the linear copy when dense; 1x70 images take the linear copy either way.  A second test alternates three
entries of different shapes on one context, the path on which device blocks come back from the context's cache."""
import ctypes as C

import numpy as np
import pytest

from _host_pitch import strided_host

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")  # before the library: the two share one HIP runtime, torch's

from introtocomputervision_amd import _capi, synth  # noqa: E402

U8, F32 = _capi.DEPTH_8U, _capi.DEPTH_32F
PADS = [3, 7, 1, 5, 11, 2]  # elements, one per stride argument
SHAPE, ROW = (37, 53), (1, 70)


@pytest.fixture(scope="module")
def ctx():
    c = _capi.Context()
    yield c
    c.close()


def tex(rows, cols, dtype=np.float32, seed=0x5EED0A10):
    t = synth.smooth_noise(seed, rows, cols, passes=1)
    return t.astype(np.uint8) if dtype == np.uint8 else (t * np.float32(0.37) - np.float32(11.5)).astype(np.float32)


class Operands:
    """Hands out the image operands of one call, dense or pitched, and keeps them for the comparison."""

    def __init__(self, pitched):
        self.pitched, self.kept = pitched, []

    def img(self, a, k):
        """(pointer, stride in bytes) of a copy of the 2-D array `a`; `k` picks the pad (one per stride argument)."""
        block, view = strided_host(np.ascontiguousarray(a), PADS[k] if self.pitched else 0)
        self.kept.append((block, view))
        return view.ctypes.data, view.strides[0]

    def images(self):
        for block, view in self.kept:
            pad = block[:, view.shape[1] * view.itemsize:]
            assert (pad == 0xA5).all(), "a padding byte was written"
        return [np.ascontiguousarray(v) for _, v in self.kept]


def lk_flow(L, h, o, shape):
    r, c = shape
    (p, s), (n, _) = o.img(tex(r, c), 0), o.img(tex(r, c, seed=0x5EED0A11), 0)
    (u, os_), (v, _) = o.img(np.zeros((r, c), np.float32), 1), o.img(np.zeros((r, c), np.float32), 1)
    return L.micv_lk_flow_host(h, p, n, r, c, s, 5, u, v, os_), []


def lk_warp(L, h, o, shape):
    r, c = shape
    src, ss = o.img(tex(r, c), 0)
    (du, fs), (dv, _) = o.img(tex(r, c, seed=1) * np.float32(0.05), 1), o.img(tex(r, c, seed=2) * np.float32(0.05), 1)
    dst, ds = o.img(np.zeros((r, c), np.float32), 2)
    return L.micv_lk_warp_host(h, src, ss, du, dv, fs, r, c, dst, ds), []


def pyr_down(L, h, o, shape):
    r, c = shape  # odd: the last row and column are dropped
    src, ss = o.img(tex(r, c), 0)
    dst, ds = o.img(np.zeros((r // 2, c // 2), np.float32), 1)
    return L.micv_pyr_down_host(h, src, r, c, ss, dst, ds), []


def sobel(L, h, o, shape):
    r, c = shape
    src, ss = o.img(tex(r, c), 0)
    (gx, gs), (gy, _) = o.img(np.zeros((r, c), np.float32), 1), o.img(np.zeros((r, c), np.float32), 1)
    return L.micv_sobel_host(h, src, r, c, ss, 3, 1.0, gx, gy, gs), []


def harris_refine(L, h, o, shape):
    r, c = shape
    resp, rs = o.img(tex(r, c), 0)
    corners, cs = o.img(np.zeros((r, c), np.float32), 1)
    cap = r * c  # every pixel fits
    locs, count = np.full((cap, 2), -7, np.int32), C.c_int64(-1)
    rc = L.micv_harris_refine_host(h, resp, r, c, rs, 1.0, 3, corners, cs, locs.ctypes.data, cap, C.byref(count))
    assert 0 < count.value <= cap, count.value  # the counted list is exercised
    return rc, [locs, np.int64(count.value)]


def disparity_ssd(L, h, o, shape):
    r, c = shape
    (le, s), (ri, _) = o.img(tex(r, c), 0), o.img(np.roll(tex(r, c), -3, axis=1), 0)
    disp, ds = o.img(np.full((r, c), 77, np.int8), 1)
    return L.micv_disparity_ssd_host(h, le, ri, r, c, s, 2, -6, 0, 0, disp, ds), []


def generate_edge(L, h, o, shape):
    r, c = shape
    src, ss = o.img(tex(r, c, np.uint8), 0)
    edges, es = o.img(np.zeros((r, c), np.uint8), 1)
    return L.micv_generate_edge_host(h, src, r, c, ss, 5, 1.4, 20.0, 60.0, edges, es), []


def gaussian_blur_f32(L, h, o, shape):
    r, c = shape
    src, ss = o.img(tex(r, c), 0)
    dst, ds = o.img(np.zeros((r, c), np.float32), 1)
    return L.micv_gaussian_blur_f32_host(h, src, r, c, ss, 5, 1.1, dst, ds), []


def gray_to_rgb8(L, h, o, shape):
    r, c = shape
    src, ss = o.img(tex(r, c), 0)
    dst, ds = o.img(np.zeros((r, 3 * c), np.uint8), 1)
    return L.micv_gray_to_rgb8_host(h, src, F32, r, c, ss, dst, ds), []


def mix_channels(L, h, o, shape):
    r, c = shape
    src, ss = o.img(tex(r, 3 * c, np.uint8), 0)
    dst, ds = o.img(np.zeros((r, 3 * c), np.uint8), 1)
    order = (C.c_int * 3)(2, 0, 1)
    return L.micv_mix_channels_u8_host(h, src, r, c, 3, ss, order, dst, 3, ds), []


def pixel_replacement(L, h, o, shape):
    r, c = shape
    r1, c1 = (r, c - 6) if r == 1 else (r - 4, c - 6)
    a, s1 = o.img(tex(r1, c1, np.uint8), 0)
    b, s2 = o.img(tex(r, c, np.uint8, seed=3), 1)
    dst, ds = o.img(np.zeros((r, c), np.uint8), 2)
    return L.micv_pixel_replacement_u8_host(h, a, r1, c1, s1, b, r, c, s2, 1, 1 if r == 1 else 11, dst, ds), []


def draw_segments(L, h, o, shape):
    r, c = shape
    img, s = o.img(tex(r, 3 * c, np.uint8), 0)  # in place
    seg = np.array([[2, 0, c - 3, r - 1], [c - 1, 0, 0, r - 1], [-9.5, r / 2, c + 9.5, r / 2]], np.float32)
    color = (C.c_double * 4)(10, 250, 30, 0)
    return L.micv_draw_segments_host(h, img, r, c, 3, s, seg.ctypes.data, len(seg), color), []


def draw_circles(L, h, o, shape):
    r, c = shape
    img, s = o.img(tex(r, 3 * c, np.uint8), 0)  # in place
    peaks = np.array([[[18, 26], [5, 40]], [[30, 10], [0, 0]]], np.uint32)  # [radius][peak] = (row, column)
    counts = np.array([2, 1], np.int64)
    color = (C.c_uint8 * 3)(0, 255, 90)
    return L.micv_draw_circles_host(h, img, r, c, s, peaks.ctypes.data, counts.ctypes.data, 2, 2, 6, color), []


def sift_descriptors(L, h, o, shape):
    r, c = shape
    (gx, gs), (gy, _) = o.img(tex(r, c), 0), o.img(tex(r, c, seed=4), 0)
    kp = np.array([[26, 18, 16, 30], [9.5, 7.25, 16, 200], [44, 30, 16, 0], [3, 33, 16, 359]], np.float32)  # x, y, size, angle
    desc, ds = o.img(np.zeros((len(kp), 128), np.float32), 1)  # a row per keypoint
    assert ds >= 512
    return L.micv_sift_descriptors_host(h, gx, gy, r, c, gs, kp.ctypes.data, len(kp), desc, ds), []


CASES = [(f, SHAPE) for f in (lk_flow, lk_warp, pyr_down, sobel, harris_refine, disparity_ssd, generate_edge, gaussian_blur_f32,
                              gray_to_rgb8, mix_channels, pixel_replacement, draw_segments, draw_circles, sift_descriptors)]
CASES += [(f, ROW) for f in (lk_warp, gaussian_blur_f32, gray_to_rgb8, mix_channels, pixel_replacement, draw_segments)]


def run(ctx, case, shape, pitched):
    o = Operands(pitched)
    rc, flat = case(_capi.lib, ctx.handle, o, shape)
    assert rc == _capi.OK, (case.__name__, shape, pitched, rc, _capi.last_error())
    return o.images() + [np.asarray(x) for x in flat]


def same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("case,shape", CASES, ids=[f"{f.__name__}-{s[0]}x{s[1]}" for f, s in CASES])
def test_pitched_equals_dense(ctx, case, shape):
    dense, pitched = run(ctx, case, shape, False), run(ctx, case, shape, True)
    assert same(dense, pitched), (case.__name__, shape)


def test_alternating_shapes_reuse_blocks(ctx):
    """Three entries of different shapes, alternately, thirty times on one context: every result equals the first."""
    rounds = [(mix_channels, SHAPE), (draw_segments, ROW), (sobel, (20, 31))]
    first = [run(ctx, f, s, True) for f, s in rounds]
    for i in range(30):
        f, s = rounds[i % 3]
        assert same(run(ctx, f, s, True), first[i % 3]), (i, f.__name__)
