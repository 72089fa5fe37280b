"""Window stereo of the reference's ps2 (`cuda::` / `serial::` disparitySSD, disparityNCorr;
ProblemSets/ps2_cpp/include/DisparitySSD.h:18-43, DisparityNCorr.h:19-44)."""
import numpy as np

from . import _buf as B
from ._capi import (DISPARITY_NCC, DISPARITY_SSD, STEREO_COLS_2R, STEREO_MIN_SSD_5E6, STEREO_ROLLING, STEREO_SERIAL, check,
                    lib)
from .lk import _ctx_for

# window and threshold of DisparitySSD.cu, every row's column sums formed afresh (the fast kernel)
AS_WRITTEN_CUDA = STEREO_COLS_2R | STEREO_MIN_SSD_5E6
# + the kernel's rolling subtract / add column sums down 40-row strips (DisparitySSD.cu:97-138): differs
# from AS_WRITTEN_CUDA only on images that are not integer-valued
AS_WRITTEN_CUDA_ROLLING = AS_WRITTEN_CUDA | STEREO_ROLLING


def _run(dev_fn, host_fn, left, right, windowRad, minDisparity, maxDisparity, flags, ctx):
    B.check2d(left, np.float32, name="left")
    B.check2d(right, np.float32, name="right")
    if tuple(left.shape) != tuple(right.shape) or B.stride_bytes(left) != B.stride_bytes(right):
        raise ValueError("left and right differ in size / stride")
    rows, cols = left.shape
    disp = B.empty_like_shape(left, (rows, cols), np.int8)
    c = _ctx_for(left, ctx)
    if B.is_dev(left):
        check(dev_fn(c.handle, B.ptr(left), B.ptr(right), rows, cols, B.stride_bytes(left),
                     int(windowRad), int(minDisparity), int(maxDisparity), int(flags),
                     B.ptr(disp), cols, B.stream_of(left)))
    else:
        check(host_fn(c.handle, B.ptr(left), B.ptr(right), rows, cols, B.stride_bytes(left),
                      int(windowRad), int(minDisparity), int(maxDisparity), int(flags),
                      B.ptr(disp), cols))
    return disp


def disparitySSD(left, right, windowRad, minDisparity, maxDisparity, flags=0, ctx=None):
    """disparitySSD(left, right, windowRad, minDisparity, maxDisparity) -> int8 disparity.
    flags=0: (2r+1)^2 window, CUDA-path addressing; AS_WRITTEN_CUDA: DisparitySSD.cu as written;
    STEREO_SERIAL: DisparitySSD.cpp as written."""
    return _run(lib.micv_disparity_ssd_dev, lib.micv_disparity_ssd_host, left, right, windowRad,
                minDisparity, maxDisparity, flags, ctx)


def disparityNCorr(left, right, windowRad, minDisparity, maxDisparity, flags=0, ctx=None):
    """disparityNCorr, CUDA-path semantics (DisparityNCorr.cu:60-174)."""
    return _run(lib.micv_disparity_ncorr_dev, lib.micv_disparity_ncorr_host, left, right,
                windowRad, minDisparity, maxDisparity, flags, ctx)


SSD, NCC = DISPARITY_SSD, DISPARITY_NCC


def _pair_images(left, right):
    B.check2d(left, np.float32, name="left")
    B.check2d(right, np.float32, name="right")
    if B.is_dev(left) != B.is_dev(right) or tuple(left.shape) != tuple(right.shape) or \
            B.stride_bytes(left) != B.stride_bytes(right):
        raise ValueError("left and right differ in kind, size or stride")


def disparityPair(left, right, windowRad, disparityRange, metric=SSD, flags=0, ctx=None):
    """disparitySSDPair / disparityNCorrPair (ps2_cpp/src/main.cpp:21-78) -> (leftDisparity, rightDisparity), int8:
    the left image as reference over [-disparityRange, 0], the right one over [0, disparityRange]."""
    _pair_images(left, right)
    rows, cols = left.shape
    dl = B.empty_like_shape(left, (rows, cols), np.int8)
    dr = B.empty_like_shape(left, (rows, cols), np.int8)
    args = (_ctx_for(left, ctx).handle, B.ptr(left), B.ptr(right), rows, cols, B.stride_bytes(left), int(windowRad),
            int(disparityRange), int(metric), int(flags), B.ptr(dl), B.ptr(dr), cols)
    if B.is_dev(left):
        check(lib.micv_disparity_pair_dev(*args, B.stream_of(left)))
    else:
        check(lib.micv_disparity_pair_host(*args))
    return dl, dr


def disparityPairDisplay(left, right, windowRad, disparityRange, metric=SSD, flags=0, gain=1.0, noise=None, ctx=None):
    """One pair-and-display block of main.cpp's runProblem* after the grey conversion, as one call on one stream:
    left * gain + noise[0], right * gain + noise[1] (noise: a pair of float32 images, or None), the disparity pair, and
    the images the driver writes.  Returns (leftDisparity, rightDisparity, leftImage, leftImageInverted, rightImage):
    two int8 maps and three uint8 images (cv::normalize NORM_MINMAX to 0..255; `ones * 255 - leftImage`)."""
    _pair_images(left, right)
    rows, cols = left.shape
    nl = nr = None
    if noise is not None:
        nl, nr = noise
        _pair_images(nl, nr)
        if B.is_dev(nl) != B.is_dev(left) or tuple(nl.shape) != (rows, cols):
            raise ValueError("noise: need two images of left's kind and size")
    dl, dr = (B.empty_like_shape(left, (rows, cols), np.int8) for _ in range(2))
    il, ii, ir = (B.empty_like_shape(left, (rows, cols), np.uint8) for _ in range(3))
    args = (_ctx_for(left, ctx).handle, B.ptr(left), B.ptr(right), rows, cols, B.stride_bytes(left), float(gain),
            B.ptr(nl) if nl is not None else None, B.ptr(nr) if nl is not None else None,
            B.stride_bytes(nl) if nl is not None else 0, int(windowRad), int(disparityRange), int(metric), int(flags),
            B.ptr(dl), B.ptr(dr), cols, B.ptr(il), B.ptr(ii), B.ptr(ir), cols)
    if B.is_dev(left):
        changed = nl is not None or np.float32(gain) != np.float32(1)
        work = B.empty_like_shape(left, (2, rows, cols), np.float32) if changed else None
        check(lib.micv_disparity_pair_display_dev(*args, B.ptr(work) if changed else None, B.stream_of(left)))
    else:
        check(lib.micv_disparity_pair_display_host(*args))
    return dl, dr, il, ii, ir
