"""ps0 of the reference (ProblemSets/ps0_cpp/main.cpp) on the device (csrc/ps0.hip): its five functions, the library calls
main makes between them, and main's whole solution as one call of three launches.  numpy arrays take the `_host` entry
points, torch CUDA tensors the `_dev` ones on the current stream, where nothing synchronises and mean and stddev are read
on the device.  include/mi_cv.h, "ps0", states the rules (parity with OpenCV unpinned)."""
import ctypes as C

import numpy as np

from . import _buf as B
from . import display, warp
from ._capi import check, lib
from .lk import _ctx_for
from .pf import _frame_view

STATS_DTYPE = np.dtype([("mean", "<f8"), ("stddev", "<f8"), ("sum", "<u8"), ("sqsum", "<u8"), ("min", "<i4"), ("max", "<i4")])
BLUE, GREEN, RED = 0, 1, 2  # main.cpp:14
NUM_CENTER_PIXELS = 100     # :26
NOISE_SIGMA = 5             # :163
PLANES = ("green", "red", "arithmetic", "translated", "difference", "noisyGreen", "noisyBlue")


def _call(name, ref, *args):
    h = _ctx_for(ref, None).handle
    if B.is_dev(ref):
        check(getattr(lib, name + "_dev")(h, *args, B.stream_of(ref)))
    else:
        check(getattr(lib, name + "_host")(h, *args))


def _plane(img, name):
    rows, cols, ch, stride = _frame_view(img, name)
    if ch != 1:
        raise ValueError(f"{name}: a single-channel image expected")
    return rows, cols, stride


def _new(ref, shape, dtype=np.uint8):
    return B.empty_like_shape(ref, shape, dtype)


def mixChannels(src, fromTo):
    """dst channel k = src channel fromTo[k]; one entry gives a [rows, cols] plane."""
    rows, cols, scn, sstride = _frame_view(src, "src")
    m = [int(v) for v in fromTo]
    dcn = len(m)
    dst = _new(src, (rows, cols) if dcn == 1 else (rows, cols, dcn))
    _call("micv_mix_channels_u8", src, B.ptr(src), rows, cols, scn, sstride, (C.c_int * max(dcn, 1))(*m), B.ptr(dst), dcn, cols * dcn)
    return dst


def swapRedBlue(inputImage):
    """swapRedBlue (main.cpp:17-23)."""
    return mixChannels(inputImage, (2, 1, 0))


def extractChannel(image, coi):
    """cv::extractChannel."""
    return mixChannels(image, (coi,))


def pixelReplacement(img1, img2, size=NUM_CENTER_PIXELS):
    """pixelReplacement (:25-42): img2 with img1's central size x size square in its centre."""
    r1, c1, ch, s1 = _frame_view(img1, "img1")
    r2, c2, ch2, s2 = _frame_view(img2, "img2")
    if ch != ch2 or B.is_dev(img1) != B.is_dev(img2):
        raise ValueError("img1 and img2: one kind and one number of channels expected")
    dst = _new(img2, tuple(img2.shape))
    _call("micv_pixel_replacement_u8", img2, B.ptr(img1), r1, c1, s1, B.ptr(img2), r2, c2, s2, ch, int(size), B.ptr(dst), c2 * ch)
    return dst


def meanStdDev(image):
    """cv::minMaxLoc + cv::meanStdDev (:135-138) -> the record: a STATS_DTYPE scalar for numpy, a 40-byte uint8 CUDA tensor
    (view it with statsFromDevice; its head is what doArithmeticOperations takes) for a CUDA tensor."""
    rows, cols, stride = _plane(image, "image")
    if B.is_dev(image):
        rec = _new(image, (STATS_DTYPE.itemsize,))
        _call("micv_mean_stddev_u8", image, B.ptr(image), rows, cols, stride, B.ptr(rec))
        return rec
    rec = np.zeros(1, STATS_DTYPE)
    _call("micv_mean_stddev_u8", image, B.ptr(image), rows, cols, stride, rec.ctypes.data)
    return rec[0]


def statsFromDevice(rec):
    return rec.cpu().numpy().view(STATS_DTYPE)[0]


def doArithmeticOperations(inputImage, mean, stdDev=None):
    """doArithmeticOperations (:47-56).  CUDA: `mean` may be the device record of meanStdDev (stdDev None), read on the
    device; two numbers are uploaded."""
    rows, cols, stride = _plane(inputImage, "inputImage")
    dst = _new(inputImage, (rows, cols))
    if B.is_dev(inputImage):
        if stdDev is None:
            ms = mean
        else:
            import torch
            ms = torch.tensor([float(mean), float(stdDev)], dtype=torch.float64, device=inputImage.device)
        _call("micv_ps0_arithmetic_u8", inputImage, B.ptr(inputImage), rows, cols, stride, B.ptr(ms), B.ptr(dst), cols)
    else:
        if stdDev is None:
            mean, stdDev = mean["mean"], mean["stddev"]
        _call("micv_ps0_arithmetic_u8", inputImage, B.ptr(inputImage), rows, cols, stride, float(mean), float(stdDev), B.ptr(dst), cols)
    return dst


def translateImg(image, xOffset, yOffset):
    """translateImg (:58-62): warp.warpAffine with [1 0 x; 0 1 y] and flags 0."""
    return warp.warpAffine(image, np.asarray([[1, 0, xOffset], [0, 1, yOffset]], np.float32))


def subtract(a, b):
    """`a -= b` on 8-bit images (:156-157) -> sat(a - b)."""
    rows, cols, sa = _plane(a, "a")
    rb, cb, sb = _plane(b, "b")
    if (rows, cols) != (rb, cb):
        raise ValueError("a and b differ in size")
    dst = _new(a, (rows, cols))
    _call("micv_subtract_sat_u8", a, B.ptr(a), sa, B.ptr(b), sb, rows, cols, B.ptr(dst), cols)
    return dst


def _noise_plane(noise, like, rows, cols):
    if B.is_dev(like):
        import torch
        if not B.is_dev(noise):
            noise = torch.from_numpy(np.ascontiguousarray(noise, np.float32)).to(like.device)
        noise = noise.contiguous()
        if noise.dtype != torch.float32 or tuple(noise.shape) != (rows, cols):
            raise ValueError("noise: a float32 plane of the image's size expected")
    else:
        noise = np.ascontiguousarray(noise, np.float32)
        if noise.shape != (rows, cols):
            raise ValueError("noise: a float32 plane of the image's size expected")
    return noise


def addGaussianNoise(image, mean=0.0, sigma=NOISE_SIGMA, noise=None, rng=None):
    """addGaussianNoise (:64-79).  noise: the float plane z * sigma + mean (None: drawn by display.randn from rng)."""
    rows, cols, stride = _plane(image, "image")
    if noise is None:
        noise = display.randn((rows, cols), mean, sigma, rng)
    noise = _noise_plane(noise, image, rows, cols)
    dst = _new(image, (rows, cols))
    _call("micv_add_noise_s8_u8", image, B.ptr(image), stride, B.ptr(noise), cols * 4, rows, cols, B.ptr(dst), cols)
    return dst


def run(image1, image2, noiseGreen=None, noiseBlue=None, size=NUM_CENTER_PIXELS, mean=0.0, sigma=NOISE_SIGMA, rng=None):
    """main.cpp:110-171 in three launches -> dict: swapped, green, red, replaced, arithmetic, translated, difference,
    noisyGreen, noisyBlue and stats (as meanStdDev returns it).  numpy images without noise planes: the `_host` entry draws
    green's plane, then blue's, from rng (default display.theRNG()), which comes back advanced."""
    r1, c1, ch1, s1 = _frame_view(image1, "image1")
    r2, c2, ch2, s2 = _frame_view(image2, "image2")
    if ch1 != 3 or ch2 != 3 or B.is_dev(image1) != B.is_dev(image2):
        raise ValueError("image1 and image2: two B, G, R images of one kind expected")
    dev = B.is_dev(image1)
    swapped, planes, replaced = _new(image1, (r1, c1, 3)), _new(image1, (7, r1, c1)), _new(image1, (r2, c2))
    head = (B.ptr(image1), r1, c1, s1, B.ptr(image2), r2, c2, s2, int(size))
    tail = (B.ptr(swapped), c1 * 3, B.ptr(planes), c1, r1 * c1, B.ptr(replaced), c2)
    if dev or noiseGreen is not None:
        if noiseGreen is None:
            noiseGreen = display.randn((r1, c1), mean, sigma, rng)
        if noiseBlue is None:
            noiseBlue = display.randn((r1, c1), mean, sigma, rng)
        ng, nb = _noise_plane(noiseGreen, image1, r1, c1), _noise_plane(noiseBlue, image1, r1, c1)
    if dev:
        rec = _new(image1, (STATS_DTYPE.itemsize,))
        _call("micv_ps0_run", image1, *head, B.ptr(ng), B.ptr(nb), c1 * 4, *tail, B.ptr(rec))
    elif noiseGreen is not None:
        # planes given on the host: the separate-plane form runs on uploaded copies
        import torch
        out = run(torch.from_numpy(np.ascontiguousarray(image1)).cuda(), torch.from_numpy(np.ascontiguousarray(image2)).cuda(), ng, nb, size)
        res = {k: v.cpu().numpy() for k, v in out.items() if k != "stats"}
        res["stats"] = statsFromDevice(out["stats"])
        return res
    else:
        rng = display.theRNG() if rng is None else rng
        st = C.c_uint64(rng.state)
        recs = np.zeros(1, STATS_DTYPE)
        check(lib.micv_ps0_run_host(_ctx_for(image1, None).handle, *head, C.byref(st), float(mean), float(sigma), *tail, recs.ctypes.data))
        rng.state = st.value
        rec = recs[0]
    out = {"swapped": swapped, "replaced": replaced, "stats": rec}
    out.update({name: planes[k] for k, name in enumerate(PLANES)})
    return out
