"""The display tail of the reference's drivers on the HIP kernels of csrc/display.hip: cv::normalize(x, x, 0, 255,
NORM_MINMAX, CV_8U), the inversion `ones * 255 - x`, cv::applyColorMap(COLORMAP_JET) (ps2 main.cpp:94-320, ps4
Solution.cpp:67,108, ps5 Solution.cpp:74-77), the gain / noise of ps2's driver (main.cpp:140-153, 191-193) and
cv::randn on the host.  The arithmetic is in include/mi_cv.h ("display").

numpy arrays take the `_host` entry points, torch CUDA tensors the `_dev` ones on the current stream, without
synchronising."""
import ctypes as C

import numpy as np

from . import _buf as B
from ._capi import DEPTH_8S, DEPTH_8U, DEPTH_32F, check, lib
from .lk import _ctx_for

_DEPTHS = {"float32": DEPTH_32F, "uint8": DEPTH_8U, "int8": DEPTH_8S}


def _image(a, name, ndims=(2,)):
    """(depth, element size, strides in bytes) of a 2-D image or a 3-D batch with unit column stride."""
    if B.is_dev(a):
        if not a.is_cuda or a.dim() not in ndims or (a.shape[-1] > 1 and a.stride(-1) != 1):
            raise ValueError(f"{name}: need a CUDA tensor of {' or '.join(map(str, ndims))} dimensions with unit column stride")
        dt, e = str(a.dtype).replace("torch.", ""), a.element_size()
        strides = [s * e for s in a.stride()]
    else:
        if not isinstance(a, np.ndarray) or a.ndim not in ndims or (a.shape[-1] > 1 and a.strides[-1] != a.itemsize):
            raise ValueError(f"{name}: need a numpy array of {' or '.join(map(str, ndims))} dimensions with unit column stride")
        dt, e, strides = a.dtype.name, a.itemsize, list(a.strides)
    if dt not in _DEPTHS:
        raise ValueError(f"{name}: dtype {dt}, expected float32, uint8 or int8")
    if 0 in a.shape:
        raise ValueError(f"{name}: empty")
    rows, cols = a.shape[-2], a.shape[-1]
    row = strides[-2] if rows > 1 else cols * e
    pitch = (strides[0] if a.shape[0] > 1 else max(row * rows, 1)) if len(a.shape) == 3 else 0
    if row < cols * e or (len(a.shape) == 3 and a.shape[0] > 1 and pitch < (rows - 1) * row + cols * e):
        raise ValueError(f"{name}: rows or images overlap")
    return _DEPTHS[dt], pitch, row


def normalizeMinMax(src, invert=False, jet=False, return_minmax=False, ctx=None):
    """cv::normalize(src, dst, 0, 255, NORM_MINMAX, CV_8U) of a float32 / uint8 / int8 image [rows, cols] or of a batch
    [n, rows, cols], each image by its own range, in two launches.  Returns dst; with invert, jet or return_minmax a
    tuple (dst, 255 - dst if invert, JET [.., rows, cols, 3] in B, G, R if jet, [.., 2] float32 (min, max) if
    return_minmax) -- all made in the same pass."""
    depth, pitch, sstride = _image(src, "src", (2, 3))
    batched = len(src.shape) == 3
    n = int(src.shape[0]) if batched else 1
    rows, cols = int(src.shape[-2]), int(src.shape[-1])
    lead = (n,) if batched else ()
    dst = B.empty_like_shape(src, lead + (rows, cols), np.uint8)
    inv = B.empty_like_shape(src, lead + (rows, cols), np.uint8) if invert else None
    col = B.empty_like_shape(src, lead + (rows, cols, 3), np.uint8) if jet else None
    mm = B.empty_like_shape(src, lead + (2,), np.float32) if return_minmax else None
    g, j = rows * cols, 3 * rows * cols
    args = (_ctx_for(src, ctx).handle, B.ptr(src), pitch, depth, n, rows, cols, sstride, B.ptr(dst), g, cols,
            B.ptr(inv) if invert else None, g, cols, B.ptr(col) if jet else None, j, 3 * cols, B.ptr(mm) if return_minmax else None)
    if B.is_dev(src):
        check(lib.micv_normalize_minmax_batch_dev(*args, B.stream_of(src)))
    else:
        check(lib.micv_normalize_minmax_batch_host(*args))
    out = (dst,) + ((inv,) if invert else ()) + ((col,) if jet else ()) + ((mm,) if return_minmax else ())
    return out[0] if len(out) == 1 else out


def applyColorMapJet(src, ctx=None):
    """cv::applyColorMap(src, dst, COLORMAP_JET): uint8 [rows, cols] -> uint8 [rows, cols, 3] (B, G, R)."""
    depth, _, sstride = _image(src, "src")
    if depth != DEPTH_8U:
        raise ValueError("src: uint8 expected")
    rows, cols = src.shape
    dst = B.empty_like_shape(src, (rows, cols, 3), np.uint8)
    args = (_ctx_for(src, ctx).handle, B.ptr(src), rows, cols, sstride, B.ptr(dst), 3 * cols)
    if B.is_dev(src):
        check(lib.micv_apply_colormap_jet_dev(*args, B.stream_of(src)))
    else:
        check(lib.micv_apply_colormap_jet_host(*args))
    return dst


def gainNoise(src, gain=1.0, noise=None, ctx=None):
    """src * gain + noise in float32, unfused: `first + noise` (main.cpp:148) with gain 1, `left * contrastFactor`
    (main.cpp:192) without noise."""
    B.check2d(src, np.float32, name="src")
    if noise is not None:
        B.check2d(noise, np.float32, name="noise")
        if B.is_dev(noise) != B.is_dev(src) or tuple(noise.shape) != tuple(src.shape):
            raise ValueError("noise: need src's kind and size")
    rows, cols = src.shape
    dst = B.empty_like_shape(src, (rows, cols), np.float32)
    args = (_ctx_for(src, ctx).handle, B.ptr(src), B.stride_bytes(src), float(gain), B.ptr(noise) if noise is not None else None,
            B.stride_bytes(noise) if noise is not None else 0, rows, cols, B.ptr(dst), cols * 4)
    if B.is_dev(src):
        check(lib.micv_gain_noise_f32_dev(*args, B.stream_of(src)))
    else:
        check(lib.micv_gain_noise_f32_host(*args))
    return dst


class RNG:
    """cv::RNG's state, carried from one randn to the next as cv::theRNG() carries it (initial state 0xffffffff)."""

    def __init__(self, state=0xFFFFFFFF):
        self.state = int(state) if state else 0xFFFFFFFF


_the_rng = RNG()


def theRNG():
    return _the_rng


def randn(shape, mean=0.0, sigma=1.0, rng=None):
    """cv::randn(dst, mean, sigma) on a CV_32FC1 image of `shape` = (rows, cols), drawn on the host from `rng` (default:
    theRNG()), which comes back advanced.  Returns a float32 numpy array."""
    rng = _the_rng if rng is None else rng
    rows, cols = int(shape[0]), int(shape[1])
    dst = np.empty((rows, cols), np.float32)
    st = C.c_uint64(rng.state)
    check(lib.micv_cv_randn_f32_host(C.byref(st), float(mean), float(sigma), rows, cols, dst.ctypes.data, cols * 4))
    rng.state = st.value
    return dst
