"""The tail of Solution::runProblem3 of the reference's ps4 driver (ProblemSets/ps4_cpp/src/Solution.cpp:315-325,
344-354) on the HIP kernels of csrc/warp.hip: cv::invertAffineTransform, cv::warpAffine and the 0.5 / 0.5 blend
(cv::addWeighted), named as OpenCV names them.

Single-channel uint8 or float32 images.  numpy arrays take the `_host` entry points, torch CUDA tensors the `_dev`
ones on the current stream, without synchronising; with tensors the 2x3 transform may itself be a CUDA tensor -- a
view of `ransac.solve_matches`' transforms, say -- and is then read on the device."""
import numpy as np

from . import _buf as B
from ._capi import DEPTH_8U, DEPTH_32F, WARP_INVERSE_MAP, WARP_NEAREST, check, lib
from .lk import _ctx_for

INTER_NEAREST, INTER_LINEAR = WARP_NEAREST, 0  # cv::InterpolationFlags


def _depth(img, name):
    if B.is_dev(img):
        import torch
        if not img.is_cuda or img.dim() != 2 or (img.shape[1] > 1 and img.stride(1) != 1):
            raise ValueError(f"{name}: need a 2-D CUDA tensor with unit column stride")
        if img.dtype not in (torch.uint8, torch.float32):
            raise ValueError(f"{name}: dtype {img.dtype}, expected uint8 or float32")
        return DEPTH_8U if img.dtype == torch.uint8 else DEPTH_32F
    if not isinstance(img, np.ndarray) or img.ndim != 2 or img.dtype not in (np.uint8, np.float32):
        raise ValueError(f"{name}: need a 2-D numpy array of uint8 or float32")
    if img.shape[1] > 1 and img.strides[1] != img.itemsize:
        raise ValueError(f"{name}: need unit column stride")
    return DEPTH_8U if img.dtype == np.uint8 else DEPTH_32F


def _same(img, other, name):
    if B.is_dev(img) != B.is_dev(other) or tuple(img.shape) != tuple(other.shape) or img.dtype != other.dtype:
        raise ValueError(f"{name}: both images need the same kind, size and dtype")


def _transform(m, like, count=None):
    """The transform where the entry point for `like` reads it: a contiguous float32 [.., 2, 3] on the host for numpy
    images, on the device for tensors (a CUDA tensor is passed through, anything else is uploaded)."""
    shape = (2, 3) if count is None else (count, 2, 3)
    if B.is_dev(like):
        import torch
        if not isinstance(m, torch.Tensor):
            m = torch.from_numpy(np.ascontiguousarray(m, np.float32)).to(like.device)
        if not m.is_cuda or m.dtype != torch.float32 or tuple(m.shape) != shape or not m.is_contiguous():
            raise ValueError(f"M: need a contiguous float32 {shape} transform")
        return m
    if B.is_dev(m):
        raise ValueError("M: a CUDA transform needs CUDA images")
    m = np.ascontiguousarray(m, np.float32)
    if m.shape != shape:
        raise ValueError(f"M: need a {shape} transform")
    return m


def invertAffineTransform(m, ctx=None):
    """cv::invertAffineTransform on a 2x3 (or [count, 2, 3]) float32 transform."""
    dev = B.is_dev(m)
    if not dev:
        m = np.ascontiguousarray(m, np.float32)
    if tuple(m.shape[-2:]) != (2, 3) or len(m.shape) not in (2, 3):
        raise ValueError("M: need a 2x3 or [count, 2, 3] transform")
    count = 1 if len(m.shape) == 2 else int(m.shape[0])
    if dev:
        import torch
        if not (m.is_cuda and m.dtype == torch.float32 and m.is_contiguous()):
            raise ValueError("M: need a contiguous float32 CUDA tensor")
        out = torch.empty_like(m)
        check(lib.micv_invert_affine_dev(_ctx_for(m, ctx).handle, m.data_ptr(), count, out.data_ptr(), B.stream_of(m)))
    else:
        out = np.empty_like(m)
        check(lib.micv_invert_affine_host(_ctx_for(m, ctx).handle, m.ctypes.data, count, out.ctypes.data))
    return out


def warpAffine(src, m, dsize=None, flags=0, ctx=None):
    """cv::warpAffine(src, dst, M, dsize, flags) with BORDER_CONSTANT 0 -> dst.  dsize = (width, height) as cv::Size
    (None: src's size); flags: INTER_LINEAR (0) or INTER_NEAREST, optionally | WARP_INVERSE_MAP."""
    depth = _depth(src, "src")
    srows, scols = src.shape
    dcols, drows = (scols, srows) if dsize is None else (int(dsize[0]), int(dsize[1]))
    if drows < 1 or dcols < 1:
        raise ValueError("dsize: empty")
    m = _transform(m, src)
    dst = B.empty_like_shape(src, (drows, dcols), np.uint8 if depth == DEPTH_8U else np.float32)
    c = _ctx_for(src, ctx)
    args = (c.handle, B.ptr(src), depth, srows, scols, B.stride_bytes(src), B.ptr(m), int(flags), B.ptr(dst), drows,
            dcols, B.stride_bytes(dst))
    if B.is_dev(src):
        check(lib.micv_warp_affine_dev(*args, B.stream_of(src)))
    else:
        check(lib.micv_warp_affine_host(*args))
    return dst


def warpAffineBatch(src, ms, dsize=None, flags=0, ctx=None):
    """`count` warps in one launch (CUDA tensors only).  src [count, rows, cols]: image i by transform i -- a sequence
    registered to a key frame; src [rows, cols]: one shared source by `count` transforms.  ms: [count, 2, 3].
    Returns [count, drows, dcols]."""
    import torch
    if not B.is_dev(src) or src.dim() not in (2, 3) or not src.is_contiguous():
        raise ValueError("src: need a contiguous 2-D or 3-D CUDA tensor")
    count = int(ms.shape[0])
    shared = src.dim() == 2
    if not shared and src.shape[0] != count:
        raise ValueError("src and ms differ in count")
    img = src if shared else src[0]
    depth = _depth(img, "src")
    srows, scols = img.shape
    dcols, drows = (scols, srows) if dsize is None else (int(dsize[0]), int(dsize[1]))
    if drows < 1 or dcols < 1:
        raise ValueError("dsize: empty")
    m = _transform(ms, img, count)
    dst = torch.empty((count, drows, dcols), dtype=src.dtype, device=src.device)
    e = src.element_size()
    check(lib.micv_warp_affine_batch_dev(_ctx_for(src, ctx).handle, src.data_ptr(), 0 if shared else srows * scols * e, depth,
                                         srows, scols, scols * e, m.data_ptr(), count, int(flags), dst.data_ptr(),
                                         drows * dcols * e, drows, dcols, dcols * e, B.stream_of(src)))
    return dst


def addWeighted(a, alpha, b, beta, gamma=0, ctx=None):
    """cv::addWeighted(a, alpha, b, beta, gamma) -> dst; `a * 0.5 + b * 0.5` on cv::Mat's is addWeighted(a, .5, b, .5)."""
    depth = _depth(a, "a")
    _depth(b, "b")
    _same(a, b, "addWeighted")
    rows, cols = a.shape
    dst = B.empty_like_shape(a, (rows, cols), np.uint8 if depth == DEPTH_8U else np.float32)
    c = _ctx_for(a, ctx)
    args = (c.handle, B.ptr(a), B.stride_bytes(a), float(alpha), B.ptr(b), B.stride_bytes(b), float(beta), float(gamma),
            depth, rows, cols, B.ptr(dst), B.stride_bytes(dst))
    if B.is_dev(a):
        check(lib.micv_add_weighted_dev(*args, B.stream_of(a)))
    else:
        check(lib.micv_add_weighted_host(*args))
    return dst


def registerBlend(a, b, m, return_warped=False, ctx=None):
    """Solution.cpp:315-325 as one launch: `m` maps a's points onto b's (what ransacHelper returns); b is warped back
    onto a by the inverse and blended 0.5 / 0.5 with it.  Returns blended, or (warped, blended)."""
    depth = _depth(a, "a")
    _depth(b, "b")
    _same(a, b, "registerBlend")
    rows, cols = a.shape
    m = _transform(m, a)
    dt = np.uint8 if depth == DEPTH_8U else np.float32
    blended = B.empty_like_shape(a, (rows, cols), dt)
    warped = B.empty_like_shape(a, (rows, cols), dt) if return_warped else None
    c = _ctx_for(a, ctx)
    args = (c.handle, B.ptr(a), B.stride_bytes(a), B.ptr(b), B.stride_bytes(b), depth, rows, cols, B.ptr(m),
            B.ptr(warped) if return_warped else None, B.stride_bytes(blended), B.ptr(blended), B.stride_bytes(blended))
    if B.is_dev(a):
        check(lib.micv_register_blend_dev(*args, B.stream_of(a)))
    else:
        check(lib.micv_register_blend_host(*args))
    return (warped, blended) if return_warped else blended
