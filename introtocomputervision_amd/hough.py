"""`cuda::` Hough functions of the reference's ps1 (ProblemSets/ps1_cpp/src/Hough.h:22-84)."""
import ctypes as C

import numpy as np

from . import _buf as B
from ._capi import check, i32, i64, lib
from .lk import _ctx_for


def linesAccumulatorShape(rows, cols, rhoBinSize=1, thetaBinSize=1):
    rb, tb = i32(), i32()
    check(lib.micv_hough_lines_dims(int(rows), int(cols), int(rhoBinSize), int(thetaBinSize),
                                    C.byref(rb), C.byref(tb)))
    return rb.value, tb.value


def houghLinesAccumulate(edgeMask, rhoBinSize=1, thetaBinSize=1, ctx=None):
    """cuda::houghLinesAccumulate (Hough.cu:251-309) -> int32 accumulator [rhoBins, thetaBins]."""
    B.check2d(edgeMask, np.uint8, name="edgeMask")
    rows, cols = edgeMask.shape
    rb, tb = linesAccumulatorShape(rows, cols, rhoBinSize, thetaBinSize)
    acc = B.empty_like_shape(edgeMask, (rb, tb), np.int32)
    c = _ctx_for(edgeMask, ctx)
    if B.is_dev(edgeMask):
        check(lib.micv_hough_lines_dev(c.handle, B.ptr(edgeMask), rows, cols,
                                       B.stride_bytes(edgeMask), int(rhoBinSize),
                                       int(thetaBinSize), B.ptr(acc), B.stream_of(edgeMask)))
    else:
        check(lib.micv_hough_lines_host(c.handle, B.ptr(edgeMask), rows, cols,
                                        B.stride_bytes(edgeMask), int(rhoBinSize),
                                        int(thetaBinSize), B.ptr(acc)))
    return acc


def houghCirclesAccumulate(edgeMask, radius, ctx=None):
    """cuda::houghCirclesAccumulate (Hough.cu:311-364) -> int32 accumulator [rows, cols]."""
    B.check2d(edgeMask, np.uint8, name="edgeMask")
    rows, cols = edgeMask.shape
    acc = B.empty_like_shape(edgeMask, (rows, cols), np.int32)
    c = _ctx_for(edgeMask, ctx)
    if B.is_dev(edgeMask):
        check(lib.micv_hough_circles_dev(c.handle, B.ptr(edgeMask), rows, cols,
                                         B.stride_bytes(edgeMask), int(radius), B.ptr(acc),
                                         B.stream_of(edgeMask)))
    else:
        check(lib.micv_hough_circles_host(c.handle, B.ptr(edgeMask), rows, cols,
                                          B.stride_bytes(edgeMask), int(radius), B.ptr(acc)))
    return acc


def findLocalMaxima(accumulator, numPeaks, threshold, ctx=None, lazy=False):
    """cuda::findLocalMaxima (Hough.cu:366-426) -> [n, 2] uint32 (row, col) pairs ordered by
    votes descending (stable).  Device input with lazy=True: returns (peaks[numPeaks, 2], count) as
    device tensors without reading the count back (no host synchronisation; rows >= count are
    unspecified) -- for pipelines that keep consuming on the device."""
    B.check2d(accumulator, np.int32, name="accumulator")
    if B.is_dev(accumulator) and not accumulator.is_contiguous():
        raise ValueError("accumulator must be contiguous")
    if not B.is_dev(accumulator) and not accumulator.flags.c_contiguous:
        raise ValueError("accumulator must be contiguous")
    rows, cols = accumulator.shape
    c = _ctx_for(accumulator, ctx)
    k = int(numPeaks)
    if B.is_dev(accumulator):
        import torch
        peaks = torch.empty((max(k, 1), 2), dtype=torch.int32, device=accumulator.device)
        cnt = torch.zeros((1,), dtype=torch.int64, device=accumulator.device) if lazy else B.pinned_count(accumulator)
        check(lib.micv_hough_peaks_dev(c.handle, B.ptr(accumulator), rows, cols, k, int(threshold),
                                       peaks.data_ptr(), cnt.data_ptr(), B.stream_of(accumulator)))
        if lazy:
            return peaks, cnt
        return peaks[:B.read_count(cnt, accumulator)]
    peaks = np.empty((max(k, 1), 2), np.uint32)
    cnt = i64(0)
    check(lib.micv_hough_peaks_host(c.handle, B.ptr(accumulator), rows, cols, k, int(threshold),
                                    peaks.ctypes.data, C.byref(cnt)))
    return peaks[:cnt.value]


def generateEdge(image, gaussianSize, gaussianSigma, lowerThreshold, upperThreshold, ctx=None, wait=True):
    """sol::generateEdge (ps1_cpp/src/Solution.cpp:21-47) on a 2-D uint8 CUDA tensor -> 255/0 edge
    mask (Gaussian blur + Canny, aperture 3).  wait=False (tensors only) takes micv_generate_edge_async: the same
    bytes from a fixed sequence of launches, enqueued on the current stream without a host wait."""
    if isinstance(image, np.ndarray):  # host-pointer entry point
        img = np.ascontiguousarray(image, np.uint8)
        if img.ndim != 2:
            raise ValueError("image: need a 2-D uint8 array")
        out = np.empty_like(img)
        from .match import _host_ctx
        check(lib.micv_generate_edge_host((ctx or _host_ctx()).handle, img.ctypes.data, img.shape[0], img.shape[1],
                                          img.strides[0], int(gaussianSize), float(gaussianSigma),
                                          float(lowerThreshold), float(upperThreshold), out.ctypes.data,
                                          out.strides[0]))
        return out
    import torch
    if not (B.is_dev(image) and image.is_cuda and image.dim() == 2 and image.dtype == torch.uint8
            and image.stride(1) == 1):
        raise ValueError("image: need a 2-D uint8 CUDA tensor with unit column stride")
    rows, cols = image.shape
    edges = torch.empty((rows, cols), dtype=torch.uint8, device=image.device)
    entry = lib.micv_generate_edge_dev if wait else lib.micv_generate_edge_async
    check(entry(_ctx_for(image, ctx).handle, image.data_ptr(), rows, cols,
                image.stride(0), int(gaussianSize), float(gaussianSigma),
                float(lowerThreshold), float(upperThreshold), edges.data_ptr(), cols,
                B.stream_of(image)))
    return edges


def generateEdgeBatch(images, gaussianSize, gaussianSigma, lowerThreshold, upperThreshold, ctx=None, scratch_mb=0):
    """sol::generateEdge on a batch of images of one size in one call, without a host wait: element i is
    generateEdge(images[i], ...).  A [batch, rows, cols] uint8 CUDA tensor with unit column stride (any row and image
    strides that do not make images overlap) goes to micv_generate_edge_batch_async and gives a tensor; a list of 2-D
    uint8 numpy arrays (views with pitches of their own are fine) goes to micv_generate_edge_batch_host and gives a
    [batch, rows, cols] array.  scratch_mb bounds the scratch of one piece of a device batch (0 = 64 MiB)."""
    gauss = (int(gaussianSize), float(gaussianSigma), float(lowerThreshold), float(upperThreshold))
    if B.is_dev(images):
        import torch
        if not (images.is_cuda and images.dim() == 3 and images.dtype == torch.uint8 and images.stride(2) == 1):
            raise ValueError("images: need a [batch, rows, cols] uint8 CUDA tensor with unit column stride")
        batch, rows, cols = images.shape
        edges = torch.empty((batch, rows, cols), dtype=torch.uint8, device=images.device)
        pitch = images.stride(1) if rows > 1 else cols
        check(lib.micv_generate_edge_batch_async(_ctx_for(images, ctx).handle, images.data_ptr(), batch,
                                                 images.stride(0) if batch > 1 else rows * pitch, rows, cols, pitch, *gauss,
                                                 edges.data_ptr(), rows * cols, cols, int(scratch_mb), B.stream_of(images)))
        return edges
    imgs = list(images)
    if not imgs or any(not isinstance(a, np.ndarray) or a.ndim != 2 or a.dtype != np.uint8 or a.shape != imgs[0].shape
                       or a.strides[1] != 1 for a in imgs):
        raise ValueError("images: need a uint8 CUDA tensor or a non-empty list of 2-D uint8 numpy arrays of one shape")
    rows, cols = imgs[0].shape
    out = np.empty((len(imgs), rows, cols), np.uint8)
    n = len(imgs)
    srcs = (C.c_void_p * n)(*[a.ctypes.data for a in imgs])
    strides = (C.c_size_t * n)(*[a.strides[0] if rows > 1 else cols for a in imgs])
    dsts = (C.c_void_p * n)(*[out[i].ctypes.data for i in range(n)])
    dstrides = (C.c_size_t * n)(*[cols] * n)
    from .match import _host_ctx
    check(lib.micv_generate_edge_batch_host((ctx or _host_ctx()).handle, srcs, strides, n, rows, cols, *gauss, dsts, dstrides))
    return out


def hysteresis(cand, strong, ctx=None):
    """The hysteresis stage on its own (micv_hysteresis_u8_*): two 2-D uint8 masks of one shape, non-zero = set -> 255
    where the pixel lies in an 8-connected component of cand | strong that holds a strong pixel, 0 elsewhere.  CUDA
    tensors are enqueued on the current stream without a host wait; numpy arrays take the host entry."""
    B.check2d(cand, np.uint8, name="cand")
    B.check2d(strong, np.uint8, name="strong")
    if B.is_dev(cand) != B.is_dev(strong) or tuple(cand.shape) != tuple(strong.shape):
        raise ValueError("cand and strong: need two masks of one shape, both tensors or both arrays")
    rows, cols = cand.shape
    edges = B.empty_like_shape(cand, (rows, cols), np.uint8)
    c = _ctx_for(cand, ctx)
    args = (c.handle, B.ptr(cand), B.stride_bytes(cand), B.ptr(strong), B.stride_bytes(strong), rows, cols, B.ptr(edges), cols)
    if B.is_dev(cand):
        check(lib.micv_hysteresis_u8_async(*args, B.stream_of(cand)))
    else:
        check(lib.micv_hysteresis_u8_host(*args))
    return edges
