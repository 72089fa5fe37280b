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


def _pitch(a):
    """Row pitch in bytes of the last two dimensions of a uint8 array / tensor."""
    if a.shape[-2] == 1:
        return a.shape[-1]
    return a.stride(-2) if B.is_dev(a) else a.strides[-2]


def _run8(dev_fn, host_fn, left, right, windowRad, minDisparity, maxDisparity, flags, ctx):
    B.check2d(left, np.uint8, name="left")
    B.check2d(right, np.uint8, name="right")
    if B.is_dev(left) != B.is_dev(right) or tuple(left.shape) != tuple(right.shape):
        raise ValueError("left and right differ in kind or size")
    rows, cols = left.shape
    disp = B.empty_like_shape(left, (rows, cols), np.int8)
    args = (_ctx_for(left, ctx).handle, B.ptr(left), _pitch(left), B.ptr(right), _pitch(right), rows, cols, int(windowRad),
            int(minDisparity), int(maxDisparity), int(flags), B.ptr(disp), cols)
    if B.is_dev(left):
        check(dev_fn(*args, B.stream_of(left)))
    else:
        check(host_fn(*args))
    return disp


def _run8_batch(batch_fn, left, right, windowRad, minDisparity, maxDisparity, flags, ctx):
    for name, a in (("left", left), ("right", right)):
        if not B.is_dev(a) or not a.is_cuda or a.dim() != 3 or a.dtype != B.torch.uint8 or a.stride(2) != 1:
            raise ValueError(f"{name}: need a [batch, rows, cols] uint8 device tensor with unit column stride")
    if tuple(left.shape) != tuple(right.shape) or left.shape[0] < 1:
        raise ValueError("left and right differ in size, or the batch is empty")
    batch, rows, cols = left.shape
    disp = B.empty_like_shape(left, (batch, rows, cols), np.int8)
    check(batch_fn(
        _ctx_for(left, ctx).handle, B.ptr(left), left.stride(0) if batch > 1 else 0, _pitch(left), B.ptr(right),
        right.stride(0) if batch > 1 else 0, _pitch(right), batch, rows, cols, int(windowRad), int(minDisparity),
        int(maxDisparity), int(flags), B.ptr(disp), rows * cols, cols, B.stream_of(left)))
    return disp


def disparitySSD8(left, right, windowRad, minDisparity, maxDisparity, flags=0, ctx=None):
    """disparitySSD on the 8-bit images themselves (no convertTo(CV_32F)): uint8 numpy arrays take the `_host` entry, uint8
    torch device tensors the `_dev` one; each image with its own row stride, at any byte alignment.  -> int8 disparity,
    the bytes disparitySSD gives on the images converted to float32."""
    return _run8(lib.micv_disparity_ssd_u8_dev, lib.micv_disparity_ssd_u8_host, left, right, windowRad, minDisparity,
                 maxDisparity, flags, ctx)


def disparitySSD8Batch(left, right, windowRad, minDisparity, maxDisparity, flags=0, ctx=None):
    """disparitySSD8 on [batch, rows, cols] uint8 device tensors of any pair and row stride, as one pre-pass and one search
    launch over all pairs -> [batch, rows, cols] int8; element i holds the bytes of disparitySSD8(left[i], right[i], ...)."""
    return _run8_batch(lib.micv_disparity_ssd_u8_batch_dev, left, right, windowRad, minDisparity, maxDisparity, flags, ctx)


def disparityNCorr8(left, right, windowRad, minDisparity, maxDisparity, flags=0, ctx=None):
    """disparityNCorr on the 8-bit images themselves, as disparitySSD8 takes them: uint8 numpy arrays go to the `_host`
    entry, uint8 torch device tensors to the `_dev` one.  -> int8 disparity, the bytes disparityNCorr gives on the images
    converted to float32."""
    return _run8(lib.micv_disparity_ncorr_u8_dev, lib.micv_disparity_ncorr_u8_host, left, right, windowRad, minDisparity,
                 maxDisparity, flags, ctx)


def disparityNCorr8Batch(left, right, windowRad, minDisparity, maxDisparity, flags=0, ctx=None):
    """disparityNCorr8 on [batch, rows, cols] uint8 device tensors of any pair and row stride, the pair as a grid dimension
    of one energy launch and one search launch -> [batch, rows, cols] int8; element i holds the bytes of
    disparityNCorr8(left[i], right[i], ...)."""
    return _run8_batch(lib.micv_disparity_ncorr_u8_batch_dev, left, right, windowRad, minDisparity, maxDisparity, flags, ctx)


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
