"""`harris::` and `sift::` namespaces of the reference (ProblemSets/ps4_cpp/include/Harris.h,
Descriptors.h).  `harris.cpu.*` and `harris.gpu.*` of the reference share one implementation
here (their results are identical by specification)."""
import ctypes as C

import numpy as np

from . import _buf as B
from ._capi import check, i64, lib
from .lk import _ctx_for


def getGradients(img, kernelSize=3, scale=1.0, ctx=None):
    """harris::getGradients (Harris.cpp:14-41) -> (diffX, diffY).  scale = 1/9 gives the LK
    computeGradients (OpticalFlow.cpp:12-39)."""
    B.check2d(img, np.float32, name="in")
    rows, cols = img.shape
    gx = B.empty_like_shape(img, (rows, cols))
    gy = B.empty_like_shape(img, (rows, cols))
    c = _ctx_for(img, ctx)
    if B.is_dev(img):
        check(lib.micv_sobel_dev(c.handle, B.ptr(img), rows, cols, B.stride_bytes(img),
                                 int(kernelSize), float(scale), B.ptr(gx), B.ptr(gy),
                                 B.stride_bytes(gx), B.stream_of(img)))
    else:
        check(lib.micv_sobel_host(c.handle, B.ptr(img), rows, cols, B.stride_bytes(img),
                                  int(kernelSize), float(scale), B.ptr(gx), B.ptr(gy),
                                  B.stride_bytes(gx)))
    return gx, gy


HARRIS_CPU = 1  # mi_cv.h MICV_HARRIS_CPU


def getCornerResponse(gradX, gradY, windowSize, gaussianSigma, harrisScore, ctx=None, cpu_arithmetic=False):
    """harris::{cpu,gpu}::getCornerResponse (Harris.cpp:43-97 / Harris.cu:96-159) -> R.
    cpu_arithmetic: harris::cpu's arithmetic as written (Harris.cpp:78-92; MICV_HARRIS_CPU) instead of
    harris::gpu's (the default, as in the reference's configuration)."""
    B.check2d(gradX, np.float32, name="gradX")
    B.check2d(gradY, np.float32, name="gradY")
    if tuple(gradX.shape) != tuple(gradY.shape) or B.stride_bytes(gradX) != B.stride_bytes(gradY):
        raise ValueError("gradX and gradY differ in size / stride")
    rows, cols = gradX.shape
    resp = B.empty_like_shape(gradX, (rows, cols))
    c = _ctx_for(gradX, ctx)
    flags = HARRIS_CPU if cpu_arithmetic else 0
    if B.is_dev(gradX):
        check(lib.micv_harris_response_ex_dev(c.handle, B.ptr(gradX), B.ptr(gradY), rows, cols,
                                              B.stride_bytes(gradX), int(windowSize),
                                              float(gaussianSigma), float(harrisScore), flags, B.ptr(resp),
                                              B.stride_bytes(resp), B.stream_of(gradX)))
    else:
        check(lib.micv_harris_response_ex_host(c.handle, B.ptr(gradX), B.ptr(gradY), rows, cols,
                                               B.stride_bytes(gradX), int(windowSize),
                                               float(gaussianSigma), float(harrisScore), flags, B.ptr(resp),
                                               B.stride_bytes(resp)))
    return resp


def refineCorners(cornerResponse, threshold, minDistance, capacity=None, ctx=None, lazy=False):
    """harris::{cpu,gpu}::refineCorners (Harris.cpp:99-147 / Harris.cu:243-329) ->
    (corners, cornerLocs) with cornerLocs an [n, 2] int32 array of (y, x) in row-major order.
    Device input with lazy=True: returns (corners, locs[capacity, 2], count) without reading the
    count back (no host synchronisation)."""
    B.check2d(cornerResponse, np.float32, name="cornerResponse")
    rows, cols = cornerResponse.shape
    cap = int(capacity) if capacity is not None else rows * cols
    corners = B.empty_like_shape(cornerResponse, (rows, cols))
    c = _ctx_for(cornerResponse, ctx)
    if B.is_dev(cornerResponse):
        import torch
        locs = torch.empty((cap, 2), dtype=torch.int32, device=cornerResponse.device)
        # the count: a device word when the caller keeps it on the device, else a pinned host word the kernel writes
        cnt = torch.zeros((1,), dtype=torch.int64, device=cornerResponse.device) if lazy else B.pinned_count(cornerResponse)
        check(lib.micv_harris_refine_dev(c.handle, B.ptr(cornerResponse), rows, cols,
                                         B.stride_bytes(cornerResponse), float(threshold),
                                         int(minDistance), B.ptr(corners), B.stride_bytes(corners),
                                         locs.data_ptr(), cap, cnt.data_ptr(),
                                         B.stream_of(cornerResponse)))
        if lazy:
            return corners, locs, cnt
        n = min(B.read_count(cnt, cornerResponse), cap)
        return corners, locs[:n]
    locs = np.empty((cap, 2), np.int32)
    cnt = i64(0)
    check(lib.micv_harris_refine_host(c.handle, B.ptr(cornerResponse), rows, cols,
                                      B.stride_bytes(cornerResponse), float(threshold),
                                      int(minDistance), B.ptr(corners), B.stride_bytes(corners),
                                      locs.ctypes.data, cap, C.byref(cnt)))
    return corners, locs[:min(cnt.value, cap)]


def cornersFromImage(img, sobelSize=3, windowSize=5, gaussianSigma=1.5, harrisScore=0.04, threshold=5e8, minDistance=5,
                     capacity=None, ctx=None, cpu_arithmetic=False, want_gradients=True, want_response=False,
                     want_corners=False, lazy=False):
    """The ps4 caller's chain (harrisHelper, ps4_cpp/src/Solution.cpp:77-124: harris::getGradients -> getCornerResponse
    -> refineCorners) as ONE call (micv_harris_corners_dev / _host): with a 3x3 Sobel and windows 3 / 5 / 7 the gradients
    are formed inside the response kernel's tile.  Same bits as the three separate calls.
    Returns a dict: "locs" ([n, 2] int32 (y, x), row-major order), and as requested "gx", "gy", "response", "corners";
    device input with lazy=True: "locs" has `capacity` rows and "count" is a device word (no host synchronisation)."""
    B.check2d(img, np.float32, name="img")
    rows, cols = img.shape
    cap = int(capacity) if capacity is not None else rows * cols
    c = _ctx_for(img, ctx)
    flags = HARRIS_CPU if cpu_arithmetic else 0
    gx = B.empty_like_shape(img, (rows, cols)) if want_gradients else None
    gy = B.empty_like_shape(img, (rows, cols)) if want_gradients else None
    resp = B.empty_like_shape(img, (rows, cols)) if want_response else None
    corners = B.empty_like_shape(img, (rows, cols)) if want_corners else None
    rb = cols * 4

    def p(a):
        return B.ptr(a) if a is not None else None

    def sb(a):
        return B.stride_bytes(a) if a is not None else rb
    out = {}
    if B.is_dev(img):
        import torch
        locs = torch.empty((cap, 2), dtype=torch.int32, device=img.device)
        cnt = torch.zeros((1,), dtype=torch.int64, device=img.device) if lazy else B.pinned_count(img)
        check(lib.micv_harris_corners_dev(c.handle, B.ptr(img), rows, cols, B.stride_bytes(img), int(sobelSize), int(windowSize),
                                          float(gaussianSigma), float(harrisScore), flags, float(threshold), int(minDistance),
                                          p(gx), p(gy), sb(gx), p(resp), sb(resp), p(corners), sb(corners), locs.data_ptr(), cap,
                                          cnt.data_ptr(), B.stream_of(img)))
        if lazy:
            out["locs"], out["count"] = locs, cnt
        else:
            out["locs"] = locs[:min(B.read_count(cnt, img), cap)]
    else:
        locs = np.empty((cap, 2), np.int32)
        cnt = i64(0)
        check(lib.micv_harris_corners_host(c.handle, B.ptr(img), rows, cols, B.stride_bytes(img), int(sobelSize), int(windowSize),
                                           float(gaussianSigma), float(harrisScore), flags, float(threshold), int(minDistance),
                                           p(gx), p(gy), sb(gx), p(resp), sb(resp), p(corners), sb(corners), locs.ctypes.data, cap,
                                           C.byref(cnt)))
        out["locs"] = locs[:min(cnt.value, cap)]
    if want_gradients:
        out["gx"], out["gy"] = gx, gy
    if want_response:
        out["response"] = resp
    if want_corners:
        out["corners"] = corners
    return out


def _pitch8(a):
    """Row pitch in bytes of the last two dimensions of a uint8 array / tensor."""
    if a.shape[-2] == 1:
        return a.shape[-1]
    return a.stride(-2) if B.is_dev(a) else a.strides[-2]


def cornersFromImage8(img, sobelSize=3, windowSize=5, gaussianSigma=1.5, harrisScore=0.04, threshold=5e8, minDistance=5,
                      capacity=None, ctx=None, cpu_arithmetic=False, want_gradients=True, want_response=False,
                      want_corners=False, lazy=False, keypointSize=None):
    """cornersFromImage on the 8-bit image itself (no convertTo(CV_32F)): a uint8 numpy array takes the `_host` entry, a
    uint8 torch device tensor of any row stride the `_dev` one (micv_harris_corners_u8_*).  The same dict, with the bytes
    cornersFromImage gives on the image converted to float32; keypointSize adds "keypoints" ([n, 4] float32: x, y, size,
    angle_deg), the rows of getKeypoints at "locs" -- with or without the gradient planes."""
    B.check2d(img, np.uint8, name="img")
    rows, cols = img.shape
    cap = int(capacity) if capacity is not None else rows * cols
    c = _ctx_for(img, ctx)
    flags = HARRIS_CPU if cpu_arithmetic else 0
    gx = B.empty_like_shape(img, (rows, cols)) if want_gradients else None
    gy = B.empty_like_shape(img, (rows, cols)) if want_gradients else None
    resp = B.empty_like_shape(img, (rows, cols)) if want_response else None
    corners = B.empty_like_shape(img, (rows, cols)) if want_corners else None
    kp = B.empty_like_shape(img, (cap, 4)) if keypointSize is not None else None
    rb = cols * 4

    def p(a):
        return B.ptr(a) if a is not None else None

    args = (c.handle, B.ptr(img), rows, cols, _pitch8(img), int(sobelSize), int(windowSize), float(gaussianSigma), float(harrisScore),
            flags, float(threshold), int(minDistance), p(gx), p(gy), rb, p(resp), rb, p(corners), rb)
    ksize = float(keypointSize) if keypointSize is not None else 0.0
    out = {}
    if B.is_dev(img):
        import torch
        locs = torch.empty((cap, 2), dtype=torch.int32, device=img.device)
        cnt = torch.zeros((1,), dtype=torch.int64, device=img.device) if lazy else B.pinned_count(img)
        check(lib.micv_harris_corners_u8_dev(*args, locs.data_ptr(), cap, cnt.data_ptr(), ksize, p(kp), B.stream_of(img)))
        if lazy:
            out["locs"], out["count"] = locs, cnt
        else:
            n = min(B.read_count(cnt, img), cap)
            out["locs"] = locs[:n]
            kp = kp[:n] if kp is not None else None
    else:
        locs = np.empty((cap, 2), np.int32)
        cnt = i64(0)
        check(lib.micv_harris_corners_u8_host(*args, locs.ctypes.data, cap, C.byref(cnt), ksize, p(kp)))
        n = min(cnt.value, cap)
        out["locs"] = locs[:n]
        kp = kp[:n] if kp is not None else None
    if want_gradients:
        out["gx"], out["gy"] = gx, gy
    if want_response:
        out["response"] = resp
    if want_corners:
        out["corners"] = corners
    if kp is not None:
        out["keypoints"] = kp
    return out


def cornersFromImage8Batch(imgs, sobelSize=3, windowSize=5, gaussianSigma=1.5, harrisScore=0.04, threshold=5e8, minDistance=5,
                           capacity=None, ctx=None, cpu_arithmetic=False, want_gradients=True, want_response=False,
                           want_corners=False, keypointSize=None):
    """cornersFromImage8 on a [batch, rows, cols] uint8 device tensor of any batch and row stride, the image as a grid
    dimension of every launch (micv_harris_corners_u8_batch_dev).  Always lazy: "locs" is [batch, capacity, 2], "count"
    [batch] int64 on the device, "keypoints" [batch, capacity, 4], planes [batch, rows, cols]; element i holds the bytes
    of cornersFromImage8(imgs[i], ...).  capacity defaults to rows * cols."""
    if not B.is_dev(imgs) or not imgs.is_cuda or imgs.dim() != 3 or imgs.dtype != B.torch.uint8 or imgs.stride(2) != 1:
        raise ValueError("imgs: need a [batch, rows, cols] uint8 device tensor with unit column stride")
    if imgs.shape[0] < 1:
        raise ValueError("imgs: the batch is empty")
    import torch
    batch, rows, cols = imgs.shape
    cap = int(capacity) if capacity is not None else rows * cols
    c = _ctx_for(imgs, ctx)
    flags = HARRIS_CPU if cpu_arithmetic else 0

    def plane(want):
        return torch.empty((batch, rows, cols), dtype=torch.float32, device=imgs.device) if want else None

    def p(a):
        return a.data_ptr() if a is not None else None
    gx, gy, resp, corners = plane(want_gradients), plane(want_gradients), plane(want_response), plane(want_corners)
    locs = torch.empty((batch, cap, 2), dtype=torch.int32, device=imgs.device)
    cnt = torch.zeros((batch,), dtype=torch.int64, device=imgs.device)
    kp = torch.empty((batch, cap, 4), dtype=torch.float32, device=imgs.device) if keypointSize is not None else None
    rb, pb = cols * 4, rows * cols * 4
    check(lib.micv_harris_corners_u8_batch_dev(
        c.handle, imgs.data_ptr(), imgs.stride(0) if batch > 1 else 0, batch, rows, cols, _pitch8(imgs), int(sobelSize), int(windowSize),
        float(gaussianSigma), float(harrisScore), flags, float(threshold), int(minDistance), p(gx), p(gy), pb, rb, p(resp), pb, rb,
        p(corners), pb, rb, locs.data_ptr(), cap, cnt.data_ptr(), float(keypointSize) if keypointSize is not None else 0.0, p(kp),
        B.stream_of(imgs)))
    out = {"locs": locs, "count": cnt}
    if want_gradients:
        out["gx"], out["gy"] = gx, gy
    if want_response:
        out["response"] = resp
    if want_corners:
        out["corners"] = corners
    if kp is not None:
        out["keypoints"] = kp
    return out


# The reference's two namespaces, for code that spells them out.
class cpu:  # noqa: N801
    getCornerResponse = staticmethod(getCornerResponse)
    refineCorners = staticmethod(refineCorners)


gpu = cpu


def _check_grad_pair(gradX, gradY, *device_lists):
    """gradX / gradY go to the kernels with ONE shape and pitch: both must agree (and live on one device,
    together with any list the kernel indexes them by)."""
    B.check2d(gradX, np.float32, name="gradX")
    B.check2d(gradY, np.float32, name="gradY")
    if B.is_dev(gradX) != B.is_dev(gradY):
        raise ValueError("gradX and gradY: one is a device tensor, the other is not")
    if tuple(gradX.shape) != tuple(gradY.shape) or B.stride_bytes(gradX) != B.stride_bytes(gradY):
        raise ValueError("gradX and gradY differ in size / stride")
    if B.is_dev(gradX):
        if gradY.device != gradX.device:
            raise ValueError("gradX and gradY live on different devices")
        for name, t in device_lists:
            if not (B.is_dev(t) and t.is_cuda and t.device == gradX.device):
                raise ValueError(f"{name}: must be a CUDA tensor on gradX's device (numpy inputs take the host path)")


def getAnglesFromGradients(gradX, gradY, ctx=None):
    """sift::getAnglesFromGradients (Descriptors.cpp:7-25) -> angles (radians)."""
    _check_grad_pair(gradX, gradY)
    rows, cols = gradX.shape
    ang = B.empty_like_shape(gradX, (rows, cols))
    c = _ctx_for(gradX, ctx)
    if B.is_dev(gradX):
        check(lib.micv_sift_angles_dev(c.handle, B.ptr(gradX), B.ptr(gradY), rows, cols,
                                       B.stride_bytes(gradX), B.ptr(ang), B.stride_bytes(ang),
                                       B.stream_of(gradX)))
    else:
        check(lib.micv_sift_angles_host(c.handle, B.ptr(gradX), B.ptr(gradY), rows, cols,
                                        B.stride_bytes(gradX), B.ptr(ang), B.stride_bytes(ang)))
    return ang


def getKeypoints(gradX, gradY, cornerLocs, size, ctx=None):
    """sift::getKeypoints (Descriptors.cpp:27-47) -> [n, 4] float32 (x, y, size, angle_deg):
    the fields of the cv::KeyPoint the reference constructs."""
    _check_grad_pair(gradX, gradY, ("cornerLocs", cornerLocs)) if B.is_dev(gradX) else _check_grad_pair(gradX, gradY)
    rows, cols = gradX.shape
    c = _ctx_for(gradX, ctx)
    n = int(cornerLocs.shape[0])
    if B.is_dev(gradX):
        import torch
        locs = cornerLocs.to(torch.int32).contiguous()
        kp = torch.empty((n, 4), dtype=torch.float32, device=gradX.device)
        check(lib.micv_sift_keypoints_dev(c.handle, B.ptr(gradX), B.ptr(gradY), rows, cols,
                                          B.stride_bytes(gradX), locs.data_ptr(), n, float(size),
                                          kp.data_ptr(), B.stream_of(gradX)))
        return kp
    locs = np.ascontiguousarray(cornerLocs, dtype=np.int32)
    kp = np.empty((n, 4), np.float32)
    check(lib.micv_sift_keypoints_host(c.handle, B.ptr(gradX), B.ptr(gradY), rows, cols,
                                       B.stride_bytes(gradX), locs.ctypes.data, n, float(size),
                                       kp.ctypes.data))
    return kp


def computeDescriptors(gradX, gradY, keypoints, ctx=None):
    """The descriptor step of Solution::siftHelper (ps4_cpp/src/Solution.cpp:166-169,
    cv::xfeatures2d::SIFT::compute): [n, 4] keypoints (x, y, size, angle_deg) as getKeypoints returns
    them -> [n, 128] float32 descriptors (4 x 4 x 8 bins, 8-bit values).  Arithmetic: DESIGN.md §2."""
    _check_grad_pair(gradX, gradY, ("keypoints", keypoints)) if B.is_dev(gradX) else _check_grad_pair(gradX, gradY)
    rows, cols = gradX.shape
    c = _ctx_for(gradX, ctx)
    if B.is_dev(gradX):
        import torch
        kp = keypoints.to(torch.float32).contiguous().reshape(-1, 4)
        n = int(kp.shape[0])
        desc = torch.empty((n, 128), dtype=torch.float32, device=gradX.device)
        check(lib.micv_sift_descriptors_dev(c.handle, B.ptr(gradX), B.ptr(gradY), rows, cols,
                                            B.stride_bytes(gradX), kp.data_ptr(), n, desc.data_ptr(), 512,
                                            B.stream_of(gradX)))
        return desc
    kp = np.ascontiguousarray(keypoints, dtype=np.float32).reshape(-1, 4)
    n = kp.shape[0]
    desc = np.empty((n, 128), np.float32)
    check(lib.micv_sift_descriptors_host(c.handle, B.ptr(gradX), B.ptr(gradY), rows, cols,
                                         B.stride_bytes(gradX), kp.ctypes.data, n, desc.ctypes.data, 512))
    return desc


def computeDescriptors8(img, keypoints, count=None, ctx=None):
    """computeDescriptors on the 8-bit image itself (micv_sift_descriptors_u8_*): no float image and no gradient planes,
    the 3x3 Sobel pair of every sample is recomputed from the bytes.  A uint8 numpy array with [n, 4] keypoints takes the
    `_host` entry (count: an int or None); a uint8 CUDA tensor of any row stride with [cap, 4] CUDA keypoints the `_dev`
    one, count a 1-element int64 CUDA word (None: every row) that is read on the device.  -> [cap, 128] float32 with the
    bytes of computeDescriptors(*getGradients(img as float32, 3, 1.0), keypoints) in rows below min(count, cap); device rows
    past the count are not written (the tensor is zero-filled first)."""
    B.check2d(img, np.uint8, name="img")
    rows, cols = img.shape
    c = _ctx_for(img, ctx)
    if B.is_dev(img):
        import torch
        if not (B.is_dev(keypoints) and keypoints.is_cuda and keypoints.device == img.device):
            raise ValueError("keypoints: must be a CUDA tensor on img's device (numpy inputs take the host path)")
        kp = keypoints.to(torch.float32).contiguous().reshape(-1, 4)
        cap = int(kp.shape[0])
        if count is not None and not (B.is_dev(count) and count.is_cuda and count.device == img.device and count.dtype == torch.int64
                                      and count.numel() == 1):
            raise ValueError("count: a 1-element int64 CUDA tensor on img's device expected")
        desc = torch.zeros((cap, 128), dtype=torch.float32, device=img.device)
        check(lib.micv_sift_descriptors_u8_dev(c.handle, B.ptr(img), rows, cols, _pitch8(img), kp.data_ptr(), cap,
                                               count.data_ptr() if count is not None else None, desc.data_ptr(), 512, B.stream_of(img)))
        return desc
    kp = np.ascontiguousarray(keypoints, dtype=np.float32).reshape(-1, 4)
    n = kp.shape[0] if count is None else max(0, min(int(count), kp.shape[0]))
    desc = np.zeros((kp.shape[0], 128), np.float32)
    check(lib.micv_sift_descriptors_u8_host(c.handle, B.ptr(img), rows, cols, _pitch8(img), kp.ctypes.data, n, desc.ctypes.data, 512))
    return desc[:n]


def computeDescriptors8Batch(imgs, keypoints, count=None, ctx=None):
    """computeDescriptors8 on a [batch, rows, cols] uint8 device tensor of any batch and row stride with [batch, cap, 4]
    keypoints and a [batch] int64 device count (None: every row), one call (micv_sift_descriptors_u8_batch_dev): what
    cornersFromImage8Batch(keypointSize=...) returns goes straight in.  -> [batch, cap, 128] float32; element i holds the
    bytes of computeDescriptors8(imgs[i], keypoints[i], count[i:i+1])."""
    if not B.is_dev(imgs) or not imgs.is_cuda or imgs.dim() != 3 or imgs.dtype != B.torch.uint8 or imgs.stride(2) != 1:
        raise ValueError("imgs: need a [batch, rows, cols] uint8 device tensor with unit column stride")
    if imgs.shape[0] < 1:
        raise ValueError("imgs: the batch is empty")
    import torch
    batch, rows, cols = imgs.shape
    if not (B.is_dev(keypoints) and keypoints.is_cuda and keypoints.device == imgs.device and keypoints.dim() == 3
            and keypoints.shape[0] == batch and keypoints.shape[2] == 4):
        raise ValueError("keypoints: need a [batch, cap, 4] CUDA tensor on imgs' device")
    kp = keypoints.to(torch.float32).contiguous()
    cap = int(kp.shape[1])
    if count is not None and not (B.is_dev(count) and count.is_cuda and count.device == imgs.device and count.dtype == torch.int64
                                  and count.numel() == batch and count.is_contiguous()):
        raise ValueError("count: a contiguous [batch] int64 CUDA tensor on imgs' device expected")
    desc = torch.zeros((batch, cap, 128), dtype=torch.float32, device=imgs.device)
    check(lib.micv_sift_descriptors_u8_batch_dev(_ctx_for(imgs, ctx).handle, imgs.data_ptr(), imgs.stride(0) if batch > 1 else 0, batch, rows,
                                                 cols, _pitch8(imgs), kp.data_ptr(), cap, count.data_ptr() if count is not None else None,
                                                 desc.data_ptr(), cap * 512, 512, B.stream_of(imgs)))
    return desc
