"""The ps1 driver of the reference (ProblemSets/ps1_cpp/src/main.cpp, Solution.cpp) on the device, from the input
image to the marked image: blur, edges, erode, the circle search over a radius range, parallel lines and the overlays.
numpy arrays take the `_host` entry points, torch CUDA tensors the `_dev` ones; peak lists of device calls stay on
the device (int32 tensors holding the uint32 pairs) and the draw calls read them and their counts there."""
import ctypes as C

import numpy as np

from . import _buf as B
from . import hough as _hough
from ._capi import DEPTH_8U, DEPTH_32F, check, i64, lib
from .lk import _ctx_for

GREEN = (0, 255, 0)  # CV_RGB(0, 0xFF, 0), main.cpp:89


def _image(a, name="image"):
    """2-D uint8 or float32 image -> its numpy dtype."""
    if B.is_dev(a):
        import torch
        dt = {torch.uint8: np.uint8, torch.float32: np.float32}.get(a.dtype)
    else:
        dt = a.dtype.type if isinstance(a, np.ndarray) and a.dtype in (np.uint8, np.float32) else None
    if dt is None:
        raise ValueError(f"{name}: need uint8 or float32")
    B.check2d(a, dt, name=name)
    return dt


def _rgb(img, name="image"):
    """[rows, cols, 3] uint8 with interleaved channels -> (rows, cols, row pitch in bytes)."""
    if B.is_dev(img):
        import torch
        ok = img.is_cuda and img.dim() == 3 and img.shape[2] == 3 and img.dtype == torch.uint8 and img.stride(2) == 1 and img.stride(1) == 3
        pitch = img.stride(0) if ok and img.shape[0] > 1 else img.shape[1] * 3
    else:
        ok = isinstance(img, np.ndarray) and img.ndim == 3 and img.shape[2] == 3 and img.dtype == np.uint8 and img.strides[1:] == (3, 1)
        pitch = img.strides[0] if ok and img.shape[0] > 1 else img.shape[1] * 3
    if not ok:
        raise ValueError(f"{name}: need a [rows, cols, 3] uint8 image with interleaved channels")
    return img.shape[0], img.shape[1], pitch


def _color(color):
    c = (C.c_uint8 * 3)(*[int(v) for v in color])
    return c


def gaussianBlur(image, gaussianSize, gaussianSigma, ctx=None):
    """sol::gaussianBlur (Solution.cpp:49-61) on a uint8 or float32 image; the result has the input's type."""
    dt = _image(image)
    rows, cols = image.shape
    out = B.empty_like_shape(image, (rows, cols), dt)
    c = _ctx_for(image, ctx)
    sfx = "u8" if dt is np.uint8 else "f32"
    args = (c.handle, B.ptr(image), rows, cols, B.stride_bytes(image), int(gaussianSize), float(gaussianSigma), B.ptr(out),
            B.stride_bytes(out))
    if B.is_dev(image):
        check(getattr(lib, f"micv_gaussian_blur_{sfx}_dev")(*args, B.stream_of(image)))
    else:
        check(getattr(lib, f"micv_gaussian_blur_{sfx}_host")(*args))
    return out


def generateEdge(image, gaussianSize, gaussianSigma, lowerThreshold, upperThreshold, ctx=None, wait=True):
    """sol::generateEdge (Solution.cpp:21-47) -> 255 / 0 edge mask.  uint8 images go to hough.generateEdge; float32
    images (main.cpp:98, :107) are blurred in float and converted with saturate_cast<uchar>(cvRound(v)) first.
    wait=False (tensors only): the `_async` entries, the same bytes without a host wait."""
    if _image(image) is np.uint8:
        return _hough.generateEdge(image, gaussianSize, gaussianSigma, lowerThreshold, upperThreshold, ctx=ctx, wait=wait)
    rows, cols = image.shape
    edges = B.empty_like_shape(image, (rows, cols), np.uint8)
    c = _ctx_for(image, ctx)
    args = (c.handle, B.ptr(image), rows, cols, B.stride_bytes(image), int(gaussianSize), float(gaussianSigma),
            float(lowerThreshold), float(upperThreshold), B.ptr(edges), B.stride_bytes(edges))
    if B.is_dev(image):
        check((lib.micv_generate_edge_f32_dev if wait else lib.micv_generate_edge_f32_async)(*args, B.stream_of(image)))
    else:
        check(lib.micv_generate_edge_f32_host(*args))
    return edges


def erode(image, ksize=5, ctx=None):
    """cv::erode with cv::getStructuringElement(MORPH_ELLIPSE, Size(ksize, ksize)) (main.cpp:246-248); ksize odd, 1..7."""
    dt = _image(image)
    rows, cols = image.shape
    out = B.empty_like_shape(image, (rows, cols), dt)
    c = _ctx_for(image, ctx)
    sfx = "u8" if dt is np.uint8 else "f32"
    args = (c.handle, B.ptr(image), rows, cols, B.stride_bytes(image), int(ksize), B.ptr(out), B.stride_bytes(out))
    if B.is_dev(image):
        check(getattr(lib, f"micv_erode_ellipse_{sfx}_dev")(*args, B.stream_of(image)))
    else:
        check(getattr(lib, f"micv_erode_ellipse_{sfx}_host")(*args))
    return out


def houghCirclesSearch(edgeMask, minRadius, maxRadius, numPeaks, threshold, lazy=False, accumulators=False, ctx=None):
    """The radius loop of main.cpp:173-180 / :263-270 / :299-307 in one call: for every radius in [minRadius, maxRadius]
    the peaks findLocalMaxima(houghCirclesAccumulate(edgeMask, radius), numPeaks, threshold) gives.

    Returns a list with one [count, 2] (row, col) array per radius; with accumulators=True, (that list, the int32
    accumulators [n_radii, rows, cols]).  Device input with lazy=True: (peaks [n_radii, numPeaks, 2], counts [n_radii])
    as device tensors (and the accumulators), nothing read back and no host synchronisation; rows of `peaks` past a
    radius' count are unspecified."""
    B.check2d(edgeMask, np.uint8, name="edgeMask")
    rows, cols = edgeMask.shape
    k, r0, r1 = int(numPeaks), int(minRadius), int(maxRadius)
    if r0 < 0 or r1 < 0 or k < 0:
        raise ValueError("minRadius, maxRadius and numPeaks must not be negative")
    n = max(r1 - r0 + 1, 0)
    c = _ctx_for(edgeMask, ctx)
    dev = B.is_dev(edgeMask)
    acc = B.empty_like_shape(edgeMask, (n, rows, cols), np.int32) if accumulators else None
    if dev:
        import torch
        peaks = torch.empty((n, max(k, 1), 2), dtype=torch.int32, device=edgeMask.device)
        counts = torch.zeros((n,), dtype=torch.int64, device=edgeMask.device)
        check(lib.micv_hough_circles_range_peaks_dev(c.handle, B.ptr(edgeMask), rows, cols, B.stride_bytes(edgeMask), r0, r1, k,
                                                     int(threshold), peaks.data_ptr(), counts.data_ptr(),
                                                     acc.data_ptr() if accumulators and n else None, B.stream_of(edgeMask)))
        peaks = peaks[:, :k]
        if lazy:
            return (peaks, counts, acc) if accumulators else (peaks, counts)
        cnt = counts.cpu().numpy()
        out = [peaks[i, :int(cnt[i])] for i in range(n)]
    else:
        peaks = np.zeros((n, max(k, 1), 2), np.uint32)
        counts = np.zeros((n,), np.int64)
        check(lib.micv_hough_circles_range_peaks_host(c.handle, B.ptr(edgeMask), rows, cols, B.stride_bytes(edgeMask), r0, r1, k,
                                                      int(threshold), peaks.ctypes.data, counts.ctypes.data,
                                                      acc.ctypes.data if accumulators and n else None))
        if k != peaks.shape[1]:  # numPeaks = 0
            peaks = peaks[:, :0]
        out = [peaks[i, :int(counts[i])] for i in range(n)]
    return (out, acc) if accumulators else out


def rowColToRhoTheta(coordinates, rows, cols, rhoBinSize=1, thetaBinSize=1):
    """sol::rowColToRhoTheta (Solution.cpp:81-89) for [n, 2] (row, col) peaks of a rows x cols image -> [n, 2] int32
    (rho, theta).  Host arithmetic on a handful of integers (the driver logs them); drawLinesParametric does not need it."""
    import math
    rc = coordinates.cpu().numpy() if B.is_dev(coordinates) else np.asarray(coordinates)
    rc = rc.astype(np.int64).reshape(-1, 2) & 0xFFFFFFFF
    diag = int(math.ceil(math.sqrt(rows * rows + cols * cols)))
    rho = ((rc[:, 0] * int(rhoBinSize) - diag) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    theta = ((rc[:, 1] * int(thetaBinSize) - 90) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    return np.stack([rho, theta], axis=1)


def _peaks_and_count(peaks, count, name="peaks"):
    """[n, 2] peaks (+ optional count) -> (pointer holder, n, count: device int64 tensor or int)."""
    if B.is_dev(peaks):
        import torch
        if not (peaks.is_cuda and peaks.dim() == 2 and peaks.shape[1] == 2 and peaks.dtype == torch.int32 and peaks.is_contiguous()):
            raise ValueError(f"{name}: need a contiguous [n, 2] int32 CUDA tensor")
        n = peaks.shape[0]
        if count is None:
            count = torch.full((1,), n, dtype=torch.int64, device=peaks.device)
        elif not (B.is_dev(count) and count.is_cuda and count.dtype == torch.int64 and count.numel() >= 1):
            raise ValueError("count: need an int64 CUDA tensor")
        return peaks, n, count
    p = np.ascontiguousarray(peaks, np.uint32).reshape(-1, 2)
    n = p.shape[0] if count is None else min(int(count), p.shape[0])
    return p, n, n


def findParallelLines(rhoTheta, deltaTheta, deltaRho, count=None, lazy=False, ctx=None):
    """sol::findParallelLines (Solution.cpp:134-173): the (row, col) peaks whose (row / deltaRho, col / deltaTheta) bin
    holds at least one other peak, in INPUT order (the reference's order is that of an unordered_multimap's buckets).
    Device input: `count` is the device-side count of `rhoTheta` (default: all rows); lazy=True returns
    (peaks [n, 2], count) as device tensors without a host synchronisation."""
    p, n, cnt = _peaks_and_count(rhoTheta, count, "rhoTheta")
    if n > 4096:
        raise ValueError("findParallelLines: at most 4096 peaks")
    c = _ctx_for(rhoTheta, ctx)
    if B.is_dev(rhoTheta):
        import torch
        out = torch.empty((max(n, 1), 2), dtype=torch.int32, device=p.device)
        ocnt = torch.zeros((1,), dtype=torch.int64, device=p.device)
        check(lib.micv_parallel_lines_dev(c.handle, p.data_ptr(), cnt.data_ptr(), n, int(deltaRho), int(deltaTheta), out.data_ptr(),
                                          ocnt.data_ptr(), B.stream_of(p)))
        return (out[:n], ocnt) if lazy else out[:int(ocnt.item())]
    out = np.empty((max(n, 1), 2), np.uint32)
    ocnt = i64(0)
    check(lib.micv_parallel_lines_host(c.handle, p.ctypes.data, n, int(deltaRho), int(deltaTheta), out.ctypes.data, C.byref(ocnt)))
    return out[:ocnt.value]


def gray2rgb(image, ctx=None):
    """cv::cvtColor(CV_GRAY2RGB) to 8 bit: [rows, cols] uint8 or float32 -> [rows, cols, 3] uint8 (float32 through
    saturate_cast<uchar>(cvRound(v)))."""
    dt = _image(image)
    rows, cols = image.shape
    out = B.empty_like_shape(image, (rows, cols, 3), np.uint8)
    c = _ctx_for(image, ctx)
    args = (c.handle, B.ptr(image), DEPTH_8U if dt is np.uint8 else DEPTH_32F, rows, cols, B.stride_bytes(image), B.ptr(out), cols * 3)
    if B.is_dev(image):
        check(lib.micv_gray_to_rgb8_dev(*args, B.stream_of(image)))
    else:
        check(lib.micv_gray_to_rgb8_host(*args))
    return out


def drawLinesParametric(image, peaks, rhoBinSize=1, thetaBinSize=1, color=GREEN, count=None, ctx=None):
    """sol::rowColToRhoTheta + sol::drawLinesParametric (Solution.cpp:81-123) for [n, 2] (row, col) peaks of
    findLocalMaxima, drawn into `image` ([rows, cols, 3] uint8) in place; returns `image`.  Device input: `count` is the
    device-side count of `peaks` (default: all rows)."""
    rows, cols, pitch = _rgb(image)
    p, n, cnt = _peaks_and_count(peaks, count)
    if B.is_dev(image) != B.is_dev(peaks):
        raise ValueError("image and peaks must both be numpy arrays or both CUDA tensors")
    c = _ctx_for(image, ctx)
    if B.is_dev(image):
        check(lib.micv_draw_lines_parametric_dev(c.handle, image.data_ptr(), rows, cols, pitch, p.data_ptr(), cnt.data_ptr(), n,
                                                 int(rhoBinSize), int(thetaBinSize), _color(color), B.stream_of(image)))
    else:
        check(lib.micv_draw_lines_parametric_host(c.handle, image.ctypes.data, rows, cols, pitch, p.ctypes.data, n, int(rhoBinSize),
                                                  int(thetaBinSize), _color(color)))
    return image


def drawCircles(image, centers, radius, color=GREEN, counts=None, ctx=None):
    """sol::drawCircles (Solution.cpp:125-132), in place; returns `image`.  `centers` is either [n, 2] (row, col) peaks
    of one radius, or the [n_radii, numPeaks, 2] peaks of houghCirclesSearch with their `counts` [n_radii]; radius index
    i is drawn with radius + i."""
    rows, cols, pitch = _rgb(image)
    dev = B.is_dev(image)
    if dev != B.is_dev(centers):
        raise ValueError("image and centers must both be numpy arrays or both CUDA tensors")
    if dev:
        import torch
        if centers.dtype != torch.int32 or not centers.is_contiguous():
            centers = centers.contiguous()
            if centers.dtype != torch.int32:
                raise ValueError("centers: need an int32 tensor")
    else:
        centers = np.ascontiguousarray(centers, np.uint32)
    if centers.ndim == 2:
        centers = centers.reshape(1, -1, 2)
    if centers.ndim != 3 or centers.shape[2] != 2:
        raise ValueError("centers: need [n, 2] or [n_radii, numPeaks, 2]")
    nr, k = int(centers.shape[0]), int(centers.shape[1])
    if counts is None:
        counts = torch.full((nr,), k, dtype=torch.int64, device=centers.device) if dev else np.full((nr,), k, np.int64)
    elif dev:
        if not (B.is_dev(counts) and counts.dtype == torch.int64 and counts.numel() == nr and counts.is_contiguous()):
            raise ValueError("counts: need a contiguous int64 CUDA tensor with one entry per radius")
    else:
        counts = np.ascontiguousarray(counts, np.int64)
        if counts.size != nr:
            raise ValueError("counts: need one entry per radius")
    c = _ctx_for(image, ctx)
    args = (c.handle, B.ptr(image), rows, cols, pitch, B.ptr(centers), B.ptr(counts), nr, k, int(radius), _color(color))
    if dev:
        check(lib.micv_draw_circles_dev(*args, B.stream_of(image)))
    else:
        check(lib.micv_draw_circles_host(*args))
    return image
