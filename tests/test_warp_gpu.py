"""The "ps4: registration" entry points (micv_invert_affine, micv_warp_affine, micv_warp_affine_batch, micv_add_weighted,
micv_register_blend; `_dev` and `_host`) against the exact restatement tests/_warp_ref.py, bit for bit (NaNs by
position), with every output buffer pre-filled with a sentinel so that an unwritten or overwritten pixel shows."""
import ctypes as C

import numpy as np
import pytest

import _warp_ref as wr
from _host_pitch import strided_host
from introtocomputervision_amd import synth

pytestmark = pytest.mark.gpu

U8, F32 = 0, 5
INV, NEAREST = wr.WARP_INVERSE_MAP, wr.WARP_NEAREST
ALL_FLAGS = [0, INV, NEAREST, NEAREST | INV]


def lib():
    from introtocomputervision_amd._capi import lib as L
    return L


def handle():
    from introtocomputervision_amd.match import _host_ctx
    return _host_ctx().handle


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def depth_of(a):
    return U8 if a.dtype == np.uint8 else F32


def texture(rows, cols, dtype=np.uint8, seed=0x5EED0050):
    t = synth.smooth_noise(seed, rows, cols, passes=1)
    if dtype == np.uint8:
        return t.astype(np.uint8)
    return (t * np.float32(1.37) - np.float32(91.5)).astype(np.float32)


def rot(deg, scale=1.0, tx=0.0, ty=0.0):
    t = np.deg2rad(deg)
    a, b = scale * np.cos(t), scale * np.sin(t)
    return np.array([[a, -b, tx], [b, a, ty]], np.float32)


TRANSFORMS = {
    "identity": [[1, 0, 0], [0, 1, 0]],
    "shift_int": [[1, 0, 5], [0, 1, -3]],
    "shift_frac": [[1, 0, 2.37], [0, 1, -1.61]],
    "shift_half": [[1, 0, -0.5], [0, 1, 0.5]],
    "rot10": rot(10, 1.0, 4.0, -6.0),
    "rot90": [[0, -1, 20], [1, 0, 0]],
    "rot180": [[-1, 0, 30], [0, -1, 25]],
    "scale_half": [[0.5, 0, 0], [0, 0.5, 0]],
    "scale_3": [[3, 0, -7.5], [0, 3, 2.25]],
    "shear": [[1, 0.3, -4.2], [0.1, 1, 0.6]],
    "similarity": rot(-10, 1.1, 3.5, 8.25),
    "singular": [[1, 2, 3], [2, 4, 5]],
    "outside": [[1, 0, 10000], [0, 1, -10000]],
    "int_min": [[1e7, 0, 0], [0, 1e7, 0]],
    "int_min_shift": [[1, 0, 4e6], [0, 1, -3.5e6]],
    "wrap": [[3e6, 1e5, 7], [2.5e6, -4e6, 1]],
}


class Pitched:
    """A rows x cols image inside a wider sentinel-filled device block; .get() returns the image and checks the rest."""

    def __init__(self, rows, cols, dtype, pad, fill=None, sentinel=0xA5):
        import torch
        self.rows, self.cols, self.pad = rows, cols, pad
        self.dtype = np.dtype(dtype)
        self.sentinel = sentinel
        host = np.full((rows, (cols + pad) * self.dtype.itemsize), sentinel, np.uint8)
        if fill is not None:
            host.view(self.dtype)[:, :cols] = fill
        self.t = torch.from_numpy(host).cuda()
        self.stride = (cols + pad) * self.dtype.itemsize

    def ptr(self):
        return self.t.data_ptr()

    def get(self):
        host = self.t.cpu().numpy().view(self.dtype)
        rest = host[:, self.cols:].view(np.uint8)
        assert (rest == self.sentinel).all(), "wrote beyond the row"
        return np.ascontiguousarray(host[:, :self.cols])


def dev_matrix(m):
    import torch
    return torch.from_numpy(np.ascontiguousarray(m, np.float32)).cuda()


def warp_dev(src, m, flags, dsize=None, spad=0, dpad=0):
    import torch
    from introtocomputervision_amd._capi import check
    drows, dcols = (src.shape if dsize is None else (dsize[1], dsize[0]))
    s = Pitched(src.shape[0], src.shape[1], src.dtype, spad, fill=src)
    d = Pitched(drows, dcols, src.dtype, dpad)
    dm = dev_matrix(m)
    check(lib().micv_warp_affine_dev(handle(), s.ptr(), depth_of(src), src.shape[0], src.shape[1], s.stride, dm.data_ptr(),
                                     flags, d.ptr(), drows, dcols, d.stride, stream()))
    torch.cuda.synchronize()
    return d.get()


def warp_host(src, m, flags, dsize=None, spad=0, dpad=0):
    from introtocomputervision_amd._capi import check
    drows, dcols = (src.shape if dsize is None else (dsize[1], dsize[0]))
    _, sv = strided_host(src, spad)
    dblock, dv = strided_host(np.zeros((drows, dcols), src.dtype), dpad)
    dblock[...] = 0xA5
    mm = np.ascontiguousarray(m, np.float32)
    check(lib().micv_warp_affine_host(handle(), sv.ctypes.data, depth_of(src), src.shape[0], src.shape[1], sv.strides[0],
                                      mm.ctypes.data, flags, dv.ctypes.data, drows, dcols, dv.strides[0]))
    assert (dblock.view(src.dtype)[:, dcols:].view(np.uint8) == 0xA5).all()
    return np.ascontiguousarray(dv)


@pytest.mark.parametrize("name", sorted(TRANSFORMS))
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_transforms_all_modes(name, dtype):
    m = np.array(TRANSFORMS[name], np.float32)
    src = texture(45, 70, dtype)
    for flags in ALL_FLAGS:
        want = wr.warp_affine(src, m, None, flags)
        assert wr.same(warp_dev(src, m, flags), want), (name, flags, "dev")
    assert wr.same(warp_host(src, m, 0), wr.warp_affine(src, m, None, 0)), (name, "host")
    assert wr.same(warp_host(src, m, NEAREST | INV), wr.warp_affine(src, m, None, NEAREST | INV)), (name, "host")


SIZES = [  # (srows, scols), (dcols, drows) as cv::Size, source pad, destination pad (elements)
    ((1, 1), (1, 1), 0, 0), ((1, 37), (37, 1), 0, 0), ((41, 1), (1, 41), 0, 0), ((1, 1), (9, 5), 3, 1),
    ((33, 67), (67, 33), 0, 0), ((33, 67), (67, 33), 5, 3), ((24, 130), (130, 24), 1, 2), ((19, 258), (258, 19), 0, 6),
    ((30, 50), (131, 77), 0, 0), ((60, 90), (23, 17), 2, 1), ((17, 64), (64, 17), 0, 0), ((9, 129), (255, 10), 7, 5)]


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_sizes_and_strides(size, dtype):
    (srows, scols), dsize, spad, dpad = size
    src = texture(srows, scols, dtype)
    for m in (rot(10, 1.05, 1.5, -0.75), np.array([[1, 0, 0.4], [0, 1, 0.3]], np.float32)):
        for flags in ALL_FLAGS:
            want = wr.warp_affine(src, m, dsize, flags)
            assert wr.same(warp_dev(src, m, flags, dsize, spad, dpad), want), (size, flags, "dev")
            assert wr.same(warp_host(src, m, flags, dsize, spad, dpad), want), (size, flags, "host")


@pytest.mark.parametrize("rows,cols,dtype", [(1080, 1920, np.float32), (1080, 1920, np.uint8), (2160, 3840, np.uint8)])
def test_large_frames(rows, cols, dtype):
    src = texture(rows, cols, dtype)
    t = np.deg2rad(10.0)
    a, b = 1.1 * np.cos(t), 1.1 * np.sin(t)
    cx, cy = (cols - 1) / 2, (rows - 1) / 2
    m = np.array([[a, -b, cx - a * cx + b * cy], [b, a, cy - b * cx - a * cy]], np.float32)
    assert wr.same(warp_dev(src, m, 0), wr.warp_affine(src, m, None, 0))
    if rows == 1080:
        assert wr.same(warp_dev(src, m, NEAREST | INV), wr.warp_affine(src, m, None, NEAREST | INV))
        assert wr.same(warp_host(src, m, INV), wr.warp_affine(src, m, None, INV))


def special_image(rows=20, cols=28):
    """Finite texture with inf, -inf, NaN and -0 on and next to the border."""
    img = texture(rows, cols, np.float32)
    img[0, 0], img[0, 5], img[0, cols - 1] = np.inf, -np.inf, np.nan
    img[rows - 1, 0], img[rows - 1, 7], img[rows - 1, cols - 1] = np.nan, np.inf, -np.inf
    img[4, 0], img[9, cols - 1], img[1, 1] = np.inf, -np.inf, np.inf
    img[0, 10:14] = -0.0
    img[6:9, cols - 1] = -0.0
    img[12, 12] = np.nan
    return img


@pytest.mark.parametrize("m", [[[1, 0, 0], [0, 1, 0]], [[1, 0, 0.5], [0, 1, 0.25]], [[1, 0, -1.5], [0, 1, 2.75]],
                               [[1, 0, 3], [0, 1, -2]], rot(3, 1.0, 0.3, 0.2).tolist(), [[1, 0, 100], [0, 1, 0]]])
def test_f32_special_values_at_the_border(m):
    """Outside taps are 0.f and still multiplied: 0 * inf = NaN reaches the pixels whose cell straddles the border; a
    sample with all four taps outside is +0."""
    src = special_image()
    m = np.array(m, np.float32)
    for flags in ALL_FLAGS:
        want = wr.warp_affine(src, m, (34, 26), flags)
        got = warp_dev(src, m, flags, (34, 26))
        assert wr.same(got, want), flags
    far = warp_dev(src, np.array([[1, 0, 100], [0, 1, 0]], np.float32), 0)
    assert not far.view(np.uint32).any()


@pytest.mark.parametrize("k,l", [(0, 0), (5, -9), (-37, 64), (32, -32), (-1, 1), (100, 3), (-16, -16), (31, 33)])
def test_tie_to_lk_warp(k, l):
    """micv_warp_affine (f32, linear) by the translation (k/32, l/32) = micv_lk_warp with the constant flow
    (-k/32, -l/32): both coordinate walks give 32 x - k exactly, and the blend is restated from warp_sample."""
    import torch
    from introtocomputervision_amd import lk
    src = special_image(37, 53)
    m = np.array([[1, 0, k / 32.0], [0, 1, l / 32.0]], np.float32)
    got = warp_dev(src, m, 0)
    t = torch.from_numpy(src).cuda()
    du = torch.full_like(t, -k / 32.0)
    dv = torch.full_like(t, -l / 32.0)
    via_lk = lk.warp(t, du, dv).cpu().numpy()
    assert wr.same(got, via_lk)
    assert wr.same(got, wr.warp_affine(src, m, None, 0))


def test_invert_affine_both_paths():
    import torch
    from introtocomputervision_amd._capi import check
    rng = np.random.default_rng(7)
    ms = [np.array(v, np.float32) for v in TRANSFORMS.values()]
    ms += [np.array(v, np.float32) for v in ([[2, 0, 4], [0, 0.5, -8]], [[0, 2, 1], [-4, 0, 2]], [[0, 0, 7], [0, 0, -1]],
                                             [[1e-20, 0, 1], [0, 1e-20, 1]], [[1e30, 0, 1e30], [0, 1e30, -1e30]])]
    ms += [rng.normal(size=(2, 3)).astype(np.float32) * np.float32(10.0 ** rng.integers(-3, 4)) for _ in range(150)]
    m = np.stack(ms)
    want = wr.invert_affine(m)
    assert np.isfinite(want[:len(TRANSFORMS)]).all()
    host = np.full_like(m, 7)
    check(lib().micv_invert_affine_host(handle(), m.ctypes.data, len(m), host.ctypes.data))
    assert wr.same(host, want)
    dm = torch.from_numpy(m).cuda()
    out = torch.full((len(m) + 1, 2, 3), 7.0, device="cuda")
    check(lib().micv_invert_affine_dev(handle(), dm.data_ptr(), len(m), out.data_ptr(), stream()))
    torch.cuda.synchronize()
    assert wr.same(out[:-1].cpu().numpy(), want) and (out[-1] == 7).all()
    from introtocomputervision_amd import warp
    assert wr.same(warp.invertAffineTransform(m[4]), want[4]) and wr.same(warp.invertAffineTransform(dm).cpu().numpy(), want)


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("shared", [False, True])
def test_batch_equals_single_calls(dtype, shared):
    import torch
    from introtocomputervision_amd._capi import check
    count, rows, cols, drows, dcols = 64, 37, 70, 41, 68
    e = np.dtype(dtype).itemsize
    srcs = np.stack([texture(rows, cols, dtype, seed=0x5EED0060 + (0 if shared else i)) for i in range(count)])
    ms = np.stack([rot(-20 + 0.7 * i, 0.8 + 0.01 * i, 0.37 * i - 5, 3 - 0.21 * i) for i in range(count)])
    ms[5] = TRANSFORMS["singular"]
    ms[6] = TRANSFORMS["int_min"]
    # images a little apart, so a write beyond an image shows in the gap
    spitch = rows * cols * e + 64
    dpitch = drows * dcols * e + 48
    sblock = np.full((count, spitch), 0xA5, np.uint8)
    for i in range(count):
        sblock[i, :rows * cols * e] = srcs[i].reshape(-1).view(np.uint8)
    dsrc = torch.from_numpy(sblock).cuda()
    dm = torch.from_numpy(ms).cuda()
    for flags in (0, NEAREST | INV):
        for n in (64, 3, 1):
            dst = torch.full((count, dpitch), 0xA5, dtype=torch.uint8, device="cuda")
            check(lib().micv_warp_affine_batch_dev(handle(), dsrc.data_ptr(), 0 if shared else spitch, depth_of(srcs), rows, cols,
                                                   cols * e, dm.data_ptr(), n, flags, dst.data_ptr(), dpitch, drows, dcols,
                                                   dcols * e, stream()))
            torch.cuda.synchronize()
            got = dst.cpu().numpy()
            assert (got[:, drows * dcols * e:] == 0xA5).all() and (got[n:] == 0xA5).all()
            for i in range(n):
                src = srcs[0 if shared else i]
                img = got[i, :drows * dcols * e].view(dtype).reshape(drows, dcols)
                if flags == 0 or i < 8:
                    assert wr.same(img, warp_dev(src, ms[i], flags, (dcols, drows))), (i, flags, "single")
                if i in (0, 5, 6, 63):
                    assert wr.same(img, wr.warp_affine(src, ms[i], (dcols, drows), flags)), (i, flags, "ref")
    from introtocomputervision_amd import warp
    out = warp.warpAffineBatch(torch.from_numpy(srcs[0] if shared else srcs).cuda(), dm, (dcols, drows))
    assert wr.same(out[9].cpu().numpy(), wr.warp_affine(srcs[0 if shared else 9], ms[9], (dcols, drows), 0))


def add_weighted_dev(a, alpha, b, beta, gamma, pads=(0, 0, 0), in_place=False):
    import torch
    from introtocomputervision_amd._capi import check
    rows, cols = a.shape
    pa = Pitched(rows, cols, a.dtype, pads[0], fill=a)
    pb = Pitched(rows, cols, a.dtype, pads[1], fill=b)
    pd = pa if in_place else Pitched(rows, cols, a.dtype, pads[2])
    check(lib().micv_add_weighted_dev(handle(), pa.ptr(), pa.stride, alpha, pb.ptr(), pb.stride, beta, gamma, depth_of(a), rows,
                                      cols, pd.ptr(), pd.stride, stream()))
    torch.cuda.synchronize()
    return pd.get()


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_add_weighted(dtype):
    from introtocomputervision_amd._capi import check
    from introtocomputervision_amd import warp
    for rows, cols, pads in ((1, 1, (0, 0, 0)), (7, 131, (0, 0, 0)), (33, 67, (1, 2, 3)), (16, 64, (4, 0, 8))):
        a, b = texture(rows, cols, dtype, 0x5EED0071), texture(rows, cols, dtype, 0x5EED0072)
        if dtype == np.float32:
            a[0, 0], b[rows - 1, cols - 1] = np.inf, np.nan
            a[rows // 2, cols // 2] = b[rows // 2, cols // 2] = -0.0
        for alpha, beta, gamma in ((0.5, 0.5, 0.0), (0.3, 0.9, -7.25), (2.0, 1.5, 10.0), (-1.0, 1.0, 0.5), (1e10, 0.0, 0.0)):
            want = wr.add_weighted(a, alpha, b, beta, gamma)
            assert wr.same(add_weighted_dev(a, alpha, b, beta, gamma, pads), want), (rows, cols, alpha, beta, gamma)
            assert wr.same(add_weighted_dev(a, alpha, b, beta, gamma, pads, in_place=True), want)
            _, av = strided_host(a, pads[0])
            _, bv = strided_host(b, pads[1])
            dblock, dv = strided_host(np.zeros_like(a), pads[2])
            check(lib().micv_add_weighted_host(handle(), av.ctypes.data, av.strides[0], alpha, bv.ctypes.data, bv.strides[0], beta,
                                               gamma, depth_of(a), rows, cols, dv.ctypes.data, dv.strides[0]))
            assert wr.same(np.ascontiguousarray(dv), want) and (dblock.view(dtype)[:, cols:].view(np.uint8) == 0xA5).all()
        assert wr.same(warp.addWeighted(a, 0.5, b, 0.5), wr.add_weighted(a, 0.5, b, 0.5))


def test_half_half_on_u8_is_exact_in_any_order():
    """alpha = beta = 0.5, gamma = 0 on u8 (the reference's only case): every product and the sum are exact in float, so
    the result is round-half-even of (a + b) / 2 whatever the evaluation order."""
    a = np.arange(256, dtype=np.uint8).repeat(256).reshape(256, 256)
    b = np.ascontiguousarray(a.T)
    s = a.astype(np.int64) + b
    want = ((s >> 1) + ((s & 1) & ((s >> 1) & 1))).astype(np.uint8)
    assert np.array_equal(wr.add_weighted(a, 0.5, b, 0.5), want)
    assert np.array_equal(add_weighted_dev(a, 0.5, b, 0.5, 0.0), want)


def blend_dev(a, b, m, want_warped, pads=(0, 0, 0, 0)):
    import torch
    from introtocomputervision_amd._capi import check
    rows, cols = a.shape
    pa, pb = Pitched(rows, cols, a.dtype, pads[0], fill=a), Pitched(rows, cols, a.dtype, pads[1], fill=b)
    pw, po = Pitched(rows, cols, a.dtype, pads[2]), Pitched(rows, cols, a.dtype, pads[3])
    dm = dev_matrix(m)
    check(lib().micv_register_blend_dev(handle(), pa.ptr(), pa.stride, pb.ptr(), pb.stride, depth_of(a), rows, cols, dm.data_ptr(),
                                        pw.ptr() if want_warped else None, pw.stride, po.ptr(), po.stride, stream()))
    torch.cuda.synchronize()
    w = pw.get()
    if not want_warped:
        assert (w.view(np.uint8) == 0xA5).all()
    return (w if want_warped else None), po.get()


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_register_blend_equals_the_three_calls(dtype):
    from introtocomputervision_amd._capi import check
    from introtocomputervision_amd import warp
    for rows, cols, pads in ((1, 1, (0, 0, 0, 0)), (45, 70, (0, 0, 0, 0)), (33, 131, (1, 2, 3, 5)), (64, 128, (0, 4, 8, 0))):
        a = texture(rows, cols, dtype, 0x5EED0081)
        for name in ("similarity", "rot10", "shift_frac", "shear", "singular", "identity", "int_min"):
            m = np.array(TRANSFORMS[name], np.float32)
            b = wr.warp_affine(a, m)
            if dtype == np.float32 and rows > 1:
                b[0, 0], b[rows - 1, cols - 1], b[0, cols // 2] = np.inf, np.nan, -0.0
            # the three separate calls, on the device
            inv = np.full((2, 3), 7, np.float32)
            check(lib().micv_invert_affine_host(handle(), m.ctypes.data, 1, inv.ctypes.data))
            w3 = warp_dev(b, inv, 0)
            o3 = add_weighted_dev(a, 0.5, w3, 0.5, 0.0)
            want_w, want_o = wr.register_blend(a, b, m)
            assert wr.same(w3, want_w) and wr.same(o3, want_o), (name, "three calls against the restatement")
            w, o = blend_dev(a, b, m, True, pads)
            assert wr.same(w, w3) and wr.same(o, o3), (rows, cols, name, "fused, with warped")
            _, o = blend_dev(a, b, m, False, pads)
            assert wr.same(o, o3), (rows, cols, name, "fused, without warped")
            hw, ho = warp.registerBlend(a, b, m, return_warped=True)
            assert wr.same(hw, w3) and wr.same(ho, o3), (name, "host")
            assert wr.same(warp.registerBlend(a, b, m), o3)


def test_python_module_device_path():
    import torch
    from introtocomputervision_amd import warp
    src = texture(50, 80, np.uint8)
    m = np.array(TRANSFORMS["similarity"], np.float32)
    t = torch.from_numpy(src).cuda()
    dm = torch.from_numpy(m).cuda()
    for flags in ALL_FLAGS:
        assert wr.same(warp.warpAffine(t, dm, (90, 60), flags).cpu().numpy(), wr.warp_affine(src, m, (90, 60), flags))
        assert wr.same(warp.warpAffine(src, m, (90, 60), flags), wr.warp_affine(src, m, (90, 60), flags))
    assert wr.same(warp.warpAffine(t, m).cpu().numpy(), wr.warp_affine(src, m))
    # a view of a wider tensor, and a transform that is a view of a RANSAC-shaped [2, 2, 3] block
    wide = torch.from_numpy(texture(50, 96, np.uint8)).cuda()
    tr = torch.zeros((2, 2, 3), device="cuda")
    tr[0] = dm
    view = wide[:, 3:83]
    assert wr.same(warp.warpAffine(view, tr[0]).cpu().numpy(), wr.warp_affine(view.cpu().numpy(), m))
    b = torch.from_numpy(wr.warp_affine(src, m)).cuda()
    w, o = warp.registerBlend(t, b, tr[0], return_warped=True)
    want_w, want_o = wr.register_blend(src, b.cpu().numpy(), m)
    assert wr.same(w.cpu().numpy(), want_w) and wr.same(o.cpu().numpy(), want_o)
    assert wr.same(warp.addWeighted(t, 0.25, b, 0.75, 3).cpu().numpy(), wr.add_weighted(src, 0.25, b.cpu().numpy(), 0.75, 3))


def test_error_returns():
    import torch
    from introtocomputervision_amd._capi import EINVAL, OK, last_error
    L, h = lib(), handle()
    src = torch.zeros((40, 64), dtype=torch.uint8, device="cuda")
    dst = torch.full((40, 64), 0xA5, dtype=torch.uint8, device="cuda")
    m = dev_matrix(TRANSFORMS["rot10"])
    s, d, mp = src.data_ptr(), dst.data_ptr(), m.data_ptr()

    def warp(src=s, depth=U8, srows=40, scols=64, sstride=64, m=mp, flags=0, dst=d, drows=40, dcols=64, dstride=64):
        return L.micv_warp_affine_dev(h, src, depth, srows, scols, sstride, m, flags, dst, drows, dcols, dstride, None)

    bad = [dict(src=None), dict(m=None), dict(dst=None), dict(depth=1), dict(depth=F32, sstride=66), dict(flags=2), dict(flags=32),
           dict(flags=-1), dict(sstride=63), dict(dstride=63), dict(depth=F32, sstride=64, dstride=64), dict(srows=0), dict(scols=0),
           dict(drows=0), dict(dcols=-1), dict(srows=32768, sstride=64), dict(scols=32768, sstride=32768),
           dict(drows=32768), dict(dcols=32768, dstride=32768), dict(dst=s)]
    for kw in bad:
        assert warp(**kw) == EINVAL and last_error(), kw
    assert L.micv_warp_affine_dev(None, s, U8, 40, 64, 64, mp, 0, d, 40, 64, 64, None) == EINVAL

    def batch(count, spitch=40 * 64, dpitch=40 * 64, **kw):
        a = dict(src=s, depth=U8, srows=20, scols=64, sstride=64, m=mp, flags=0, dst=d, drows=20, dcols=64, dstride=64)
        a.update(kw)
        return L.micv_warp_affine_batch_dev(h, a["src"], spitch, a["depth"], a["srows"], a["scols"], a["sstride"], a["m"], count,
                                            a["flags"], a["dst"], dpitch, a["drows"], a["dcols"], a["dstride"], None)

    assert batch(-1) == EINVAL and last_error()
    assert batch(2, spitch=100) == EINVAL and batch(2, dpitch=100) == EINVAL and batch(2, flags=4) == EINVAL
    assert batch(1, scols=32768) == EINVAL and batch(1, src=None) == EINVAL
    assert batch(0) == OK and batch(0, spitch=0) == OK
    torch.cuda.synchronize()
    assert (dst == 0xA5).all()

    host = np.zeros((40, 64), np.uint8)
    out = np.zeros((40, 64), np.uint8)
    mh = np.array(TRANSFORMS["rot10"], np.float32)

    def warp_h(src=host.ctypes.data, depth=U8, srows=40, scols=64, sstride=64, m=mh.ctypes.data, flags=0, dst=out.ctypes.data,
               drows=40, dcols=64, dstride=64):
        return L.micv_warp_affine_host(h, src, depth, srows, scols, sstride, m, flags, dst, drows, dcols, dstride)

    for kw in (dict(src=None), dict(m=None), dict(dst=None), dict(depth=2), dict(flags=8), dict(sstride=10), dict(dstride=10),
               dict(srows=0), dict(dcols=0), dict(srows=32768), dict(dcols=32768, dstride=32768), dict(dst=host.ctypes.data)):
        assert warp_h(**kw) == EINVAL and last_error(), kw

    inv = torch.zeros(12, device="cuda")
    assert L.micv_invert_affine_dev(h, mp, -1, inv.data_ptr(), None) == EINVAL and last_error()
    assert L.micv_invert_affine_dev(h, None, 1, inv.data_ptr(), None) == EINVAL
    assert L.micv_invert_affine_dev(h, mp, 1, None, None) == EINVAL
    assert L.micv_invert_affine_dev(h, mp, 0, inv.data_ptr(), None) == OK
    assert L.micv_invert_affine_host(h, mh.ctypes.data, -1, mh.ctypes.data) == EINVAL
    assert L.micv_invert_affine_host(h, None, 1, mh.ctypes.data) == EINVAL
    assert L.micv_invert_affine_host(h, mh.ctypes.data, 0, None) == EINVAL
    assert L.micv_invert_affine_host(h, mh.ctypes.data, 0, mh.ctypes.data) == OK

    def addw(a=s, astride=64, b=s, bstride=64, depth=U8, rows=40, cols=64, dst=d, dstride=64):
        return L.micv_add_weighted_dev(h, a, astride, 0.5, b, bstride, 0.5, 0.0, depth, rows, cols, dst, dstride, None)

    for kw in (dict(a=None), dict(b=None), dict(dst=None), dict(depth=3), dict(astride=63), dict(bstride=1), dict(dstride=0),
               dict(rows=0), dict(cols=0), dict(rows=32768), dict(cols=32768, astride=32768, bstride=32768, dstride=32768),
               dict(depth=F32, astride=66, bstride=256, dstride=256)):
        assert addw(**kw) == EINVAL and last_error(), kw
    assert L.micv_add_weighted_host(h, None, 64, 0.5, host.ctypes.data, 64, 0.5, 0.0, U8, 40, 64, out.ctypes.data, 64) == EINVAL
    assert L.micv_add_weighted_host(h, host.ctypes.data, 64, 0.5, host.ctypes.data, 64, 0.5, 0.0, 7, 40, 64, out.ctypes.data, 64) == EINVAL
    assert L.micv_add_weighted_host(h, host.ctypes.data, 63, 0.5, host.ctypes.data, 64, 0.5, 0.0, U8, 40, 64, out.ctypes.data, 64) == EINVAL

    w = torch.zeros((40, 64), dtype=torch.uint8, device="cuda")
    wp = w.data_ptr()

    def blend(a=s, astride=64, b=wp, bstride=64, depth=U8, rows=40, cols=64, m=mp, warped=None, wstride=64, out=d, ostride=64):
        return L.micv_register_blend_dev(h, a, astride, b, bstride, depth, rows, cols, m, warped, wstride, out, ostride, None)

    for kw in (dict(a=None), dict(b=None), dict(m=None), dict(out=None), dict(depth=4), dict(astride=8), dict(bstride=8), dict(ostride=8),
               dict(warped=s, wstride=8), dict(rows=0), dict(cols=32768), dict(out=wp), dict(warped=wp), dict(warped=d)):
        assert blend(**kw) == EINVAL and last_error(), kw
    assert L.micv_register_blend_host(h, None, 64, host.ctypes.data, 64, U8, 40, 64, mh.ctypes.data, None, 0, out.ctypes.data, 64) == EINVAL
    assert L.micv_register_blend_host(h, host.ctypes.data, 64, host.ctypes.data, 64, U8, 40, 64, mh.ctypes.data, None, 0,
                                      out.ctypes.data, 8) == EINVAL
    assert L.micv_register_blend_host(h, host.ctypes.data, 64, host.ctypes.data, 64, 9, 40, 64, mh.ctypes.data, None, 0,
                                      out.ctypes.data, 64) == EINVAL
    torch.cuda.synchronize()
    assert (dst == 0xA5).all()


def chain_pair(rows=240, cols=320):
    """A textured image with distinct corners (a checkerboard multiplied into smooth noise: a plain checkerboard is
    periodic and matches ambiguously) and its warp by a small similarity."""
    tex = synth.smooth_noise(0x5EED0004, rows, cols)
    chk = synth.checkerboard(rows, cols, square=23)
    a = np.round(tex * (chk / 192.0)).astype(np.float32)
    S = rot(2.0, 1.02, -3.5, 4.25)
    return a, wr.warp_affine(a, S), S


def test_chain_on_one_stream_feeds_the_transform_on_the_device():
    """micv_harris_corners_dev -> keypoints -> descriptors -> micv_bf_knn2_dev -> ratio filter ->
    micv_ransac_solve_matches_dev -> micv_register_blend_dev on one stream, the last step reading `transforms` where
    RANSAC left it.  The only host reads before the final synchronise are Harris's own corner counts (the keypoint call
    takes n by value); nothing downstream of the matcher is read until the end."""
    import torch
    from introtocomputervision_amd import harris, match, ransac, warp
    from introtocomputervision_amd._capi import check
    a, b, S = chain_pair()
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    kps, descs = [], []
    for t in (ta, tb):
        r = harris.cornersFromImage(t, threshold=1e6)
        kp = harris.getKeypoints(r["gx"], r["gy"], r["locs"], 10)
        kps.append(kp)
        descs.append(harris.computeDescriptors(r["gx"], r["gy"], kp))
    idx, dist = match.knnMatch2(descs[0], descs[1])
    nq = idx.shape[0]
    mqt = torch.empty((nq, 2), dtype=torch.int32, device="cuda")
    md = torch.empty((nq,), dtype=torch.float32, device="cuda")
    cnt = torch.zeros((1,), dtype=torch.int64, device="cuda")
    check(lib().micv_bf_ratio_filter_dev(handle(), idx.data_ptr(), dist.data_ptr(), nq, 0.75, mqt.data_ptr(), md.data_ptr(), nq,
                                         cnt.data_ptr(), stream()))
    tr, mask, st = ransac.solve_matches(kps[0], kps[1], mqt, cnt, ransac.SIMILARITY, 6, 2000, 0.4, seed=42)
    warped, blended = warp.registerBlend(ta, tb, tr[0], return_warped=True)
    torch.cuda.synchronize()
    stats = st.cpu().numpy()
    T = tr.cpu().numpy()
    print("matches", int(cnt.item()), "stats", stats.tolist(), "transform", T[0].tolist())
    assert stats[0] > 0 and stats[2] > 0, "RANSAC reached no consensus: the test would pass on a zero transform"
    want_w, want_o = wr.register_blend(a, b, T[0])
    assert wr.same(warped.cpu().numpy(), want_w) and wr.same(blended.cpu().numpy(), want_o)
    # and the registration worked: away from the border the warped image is closer to `a` than `b` was
    inner = (slice(30, -30), slice(30, -30))
    wn = warped.cpu().numpy()
    assert np.abs(a - wn)[inner].mean() < np.abs(a - b)[inner].mean()
