"""The ps5 driver of the reference (ProblemSets/ps5_cpp/src/Solution.cpp) around `lk` and `pyr`, on the device:
drawVelocityVectors (:13-37), savePyramid's montage (:86-99), warpHelper's warp-diff chain (:101-128) and one
denseLKWrapper (:40-84) as one call.  numpy arrays take the `_host` entry points, torch CUDA tensors the `_dev` ones on
the current stream; device results stay on the device and nothing synchronises.  The drawing and the montage equal the
host loops of `viz` / shim/micv_viz.hpp byte for byte (include/mi_cv.h, "ps5: driver")."""
import ctypes as C

import numpy as np

from . import _buf as B
from ._capi import DEPTH_8U, DEPTH_32F, LK_NAIVE, LK_PYRAMIDAL, check, i32, lib, sz, vp
from .lk import _ctx_for

GREEN = (0, 255, 0)  # cv::Scalar(0, 255, 0, 255), Solution.cpp:67


def _color(color):
    return (C.c_uint8 * 3)(*[int(v) for v in color][:3])


def _np_dtype(a):
    if B.is_dev(a):
        import torch
        return {torch.uint8: np.uint8, torch.float32: np.float32}.get(a.dtype)
    return a.dtype.type if isinstance(a, np.ndarray) and a.dtype in (np.uint8, np.float32) else None


def _strides_bytes(a):
    return [s * a.element_size() for s in a.stride()] if B.is_dev(a) else list(a.strides)


def _frame(a, name):
    """An 8-bit frame [rows, cols] or [rows, cols, cn] with dense pixels -> (rows, cols, channels, depth, row pitch)."""
    if not (B.is_dev(a) or isinstance(a, np.ndarray)) or len(a.shape) not in (2, 3) or 0 in a.shape:
        raise ValueError(f"{name}: need a [rows, cols] or [rows, cols, channels] image")
    if B.is_dev(a) and not a.is_cuda:
        raise ValueError(f"{name}: torch tensors must live on the GPU (numpy arrays take the host path)")
    dt = _np_dtype(a)
    if dt is None:
        raise ValueError(f"{name}: need uint8 or float32")
    cn = 1 if len(a.shape) == 2 else int(a.shape[2])
    es = np.dtype(dt).itemsize
    st = _strides_bytes(a)
    if (a.shape[1] > 1 and st[1] != cn * es) or (len(a.shape) == 3 and cn > 1 and st[2] != es):
        raise ValueError(f"{name}: need interleaved channels and dense pixels")
    rows, cols = int(a.shape[0]), int(a.shape[1])
    return rows, cols, cn, DEPTH_8U if dt is np.uint8 else DEPTH_32F, st[0] if rows > 1 else cols * cn * es


def _batched(a, dt, cn, name):
    """[rows, cols(, cn)] or [n, rows, cols(, cn)] of `dt` with dense pixels -> (n, rows, cols, image pitch, row pitch)."""
    want = 2 + (cn > 1)
    if not (B.is_dev(a) or isinstance(a, np.ndarray)) or len(a.shape) not in (want, want + 1) or 0 in a.shape:
        raise ValueError(f"{name}: need {want} or {want + 1} dimensions")
    if B.is_dev(a) and not a.is_cuda:
        raise ValueError(f"{name}: torch tensors must live on the GPU (numpy arrays take the host path)")
    if _np_dtype(a) is not dt or (cn > 1 and a.shape[-1] != cn):
        raise ValueError(f"{name}: need {np.dtype(dt).name}" + (f" with {cn} channels" if cn > 1 else ""))
    st, es = _strides_bytes(a), np.dtype(dt).itemsize
    lead = len(a.shape) - want
    rows, cols = int(a.shape[lead]), int(a.shape[lead + 1])
    if (cols > 1 and st[lead + 1] != cn * es) or (cn > 1 and st[-1] != es):
        raise ValueError(f"{name}: need interleaved channels and dense pixels")
    row = st[lead] if rows > 1 else cols * cn * es
    n = int(a.shape[0]) if lead else 1
    pitch = st[0] if lead and n > 1 else 0
    if row < cols * cn * es or (n > 1 and pitch < (rows - 1) * row + cols * cn * es):
        raise ValueError(f"{name}: rows or images overlap")
    return n, rows, cols, pitch, row


def toBGR8(frame, ctx=None):
    """prevImg.clone() + cv::cvtColor(GRAY2RGB) for a grey frame (Solution.cpp:66, :17-19): an 8-bit frame of 1 or 3
    channels -> a new [rows, cols, 3] uint8 image."""
    rows, cols, cn, depth, pitch = _frame(frame, "frame")
    out = B.empty_like_shape(frame, (rows, cols, 3), np.uint8)
    args = (_ctx_for(frame, ctx).handle, B.ptr(frame), depth, cn, rows, cols, pitch, B.ptr(out), cols * 3)
    if B.is_dev(frame):
        check(lib.micv_gray_or_bgr_to_bgr8_dev(*args, B.stream_of(frame)))
    else:
        check(lib.micv_gray_or_bgr_to_bgr8_host(*args))
    return out


def drawVelocityVectors(inputImg, u, v, color=GREEN, inplace=False, ctx=None):
    """drawVelocityVectors (Solution.cpp:13-37): the arrows (x, y) -> (x + u, y + v) on the lattice of strides
    max(1, rows // 30), max(1, cols // 30).  inputImg: an 8-bit frame [rows, cols] or [rows, cols, 3]; returns a new
    [rows, cols, 3] image and leaves the frame alone.  With inplace=True inputImg is a [rows, cols, 3] image or a batch
    [n, rows, cols, 3] (u, v then [n, rows, cols]) that is drawn on, in one launch, and returned; pitched images and
    fields are fine."""
    dev = B.is_dev(inputImg)
    if B.is_dev(u) != dev or B.is_dev(v) != dev:
        raise ValueError("inputImg, u and v must all be numpy arrays or all CUDA tensors")
    img = inputImg if inplace else toBGR8(inputImg, ctx=ctx)
    n, rows, cols, ipitch, istride = _batched(img, np.uint8, 3, "inputImg")
    nu, ur, uc, upitch, ustride = _batched(u, np.float32, 1, "u")
    nv, vr, vc, vpitch, vstride = _batched(v, np.float32, 1, "v")
    if (nu, ur, uc) != (n, rows, cols) or (nv, vr, vc) != (n, rows, cols):
        raise ValueError("drawVelocityVectors: image and flow fields of equal size expected")
    if dev and (u.device != img.device or v.device != img.device):
        raise ValueError("drawVelocityVectors: image and flow fields on one device expected")
    if ustride != vstride or upitch != vpitch:
        raise ValueError("u and v need the same strides")
    args = (_ctx_for(img, ctx).handle, B.ptr(img), ipitch, istride, B.ptr(u), B.ptr(v), upitch, ustride, n, rows, cols, _color(color))
    if dev:
        check(lib.micv_draw_velocity_vectors_dev(*args, B.stream_of(img)))
    else:
        check(lib.micv_draw_velocity_vectors_host(*args))
    return img


def pyramidMontage(pyramid, ctx=None):
    """savePyramid (Solution.cpp:86-99) without the file: the first four levels of `pyramid` (2-D, all float32 or all
    uint8, level 0 R x C) -> the [2R, 2C] uint8 montage; float32 levels are min-max normalised, each by its own range."""
    if len(pyramid) < 4:
        raise ValueError("pyramidMontage: four levels expected")
    lv = list(pyramid[:4])
    dt = _np_dtype(lv[0])
    if dt is None:
        raise ValueError("pyramidMontage: need float32 or uint8 levels")
    dev = B.is_dev(lv[0])
    for k, a in enumerate(lv):
        if B.is_dev(a) != dev:
            raise ValueError("pyramidMontage: levels must all be numpy arrays or all CUDA tensors")
        B.check2d(a, dt, name=f"level {k}")
        if 0 in a.shape:
            raise ValueError(f"level {k}: empty")
    R, Cc = int(lv[0].shape[0]), int(lv[0].shape[1])
    out = B.empty_like_shape(lv[0], (2 * R, 2 * Cc), np.uint8)
    args = (_ctx_for(lv[0], ctx).handle, (vp * 4)(*[B.ptr(a) for a in lv]), (i32 * 4)(*[int(a.shape[0]) for a in lv]),
            (i32 * 4)(*[int(a.shape[1]) for a in lv]), (sz * 4)(*[B.stride_bytes(a) for a in lv]),
            DEPTH_32F if dt is np.float32 else DEPTH_8U, B.ptr(out), 2 * Cc)
    if dev:
        check(lib.micv_pyramid_montage_dev(*args, B.stream_of(lv[0])))
    else:
        check(lib.micv_pyramid_montage_host(*args))
    return out


def warpDiff(prevImg, nextImg, du, dv, ctx=None):
    """warpHelper's difference (Solution.cpp:118-123): prevImg - lk.warp(nextImg, du, dv) in one kernel, bit for bit."""
    for a, name in ((prevImg, "prevImg"), (nextImg, "nextImg"), (du, "du"), (dv, "dv")):
        B.check2d(a, np.float32, name=name)
        if B.is_dev(a) != B.is_dev(prevImg):
            raise ValueError("warpDiff: arguments must all be numpy arrays or all CUDA tensors")
    if not (tuple(prevImg.shape) == tuple(nextImg.shape) == tuple(du.shape) == tuple(dv.shape)):
        raise ValueError("prevImg, nextImg, du, dv differ in size")
    if B.stride_bytes(du) != B.stride_bytes(dv):
        raise ValueError("du and dv need the same row stride")
    rows, cols = prevImg.shape
    diff = B.empty_like_shape(prevImg, (rows, cols))
    args = (_ctx_for(prevImg, ctx).handle, B.ptr(prevImg), B.stride_bytes(prevImg), B.ptr(nextImg), B.stride_bytes(nextImg), B.ptr(du),
            B.ptr(dv), B.stride_bytes(du), rows, cols, B.ptr(diff), cols * 4)
    if B.is_dev(prevImg):
        check(lib.micv_lk_warp_diff_dev(*args, B.stream_of(prevImg)))
    else:
        check(lib.micv_lk_warp_diff_host(*args))
    return diff


def warpDiffSequence(frames, winSize=21, level=0, levels=4, return_raw=False, return_flow=False, ctx=None):
    """warpHelper (Solution.cpp:101-128): for every consecutive pair of `frames` lk.calcOpticalFlow, the warp-diff with that
    flow and, for all pairs together, the min-max normalisation to 8 bit.

    Device: `frames` is a float32 CUDA tensor [n, rows, cols], one pyramid level of every frame (`level` / `levels` are
    not used).  Host: a sequence of n numpy frames of one format ([rows, cols] or [rows, cols, 3|4], uint8 or float32);
    the grey conversion and the Gaussian pyramid of `levels` levels run on the device and the chain takes level `level`.
    Returns the [n - 1, rows_l, cols_l] uint8 images; with return_raw / return_flow a tuple (images, float32
    differences if return_raw, u, v if return_flow)."""
    if B.is_dev(frames):
        n, rows, cols, pitch, stride = _batched(frames, np.float32, 1, "frames")
        if len(frames.shape) != 3:
            raise ValueError("frames: need [n, rows, cols]")
        np_ = max(n - 1, 1)
        d8 = B.empty_like_shape(frames, (np_, rows, cols), np.uint8)
        raw = B.empty_like_shape(frames, (np_, rows, cols)) if return_raw else None
        u = B.empty_like_shape(frames, (np_, rows, cols)) if return_flow else None
        v = B.empty_like_shape(frames, (np_, rows, cols)) if return_flow else None
        check(lib.micv_ps5_warp_diff_seq_dev(_ctx_for(frames, ctx).handle, B.ptr(frames), pitch if n > 1 else rows * stride, n, rows,
                                             cols, stride, int(winSize), B.ptr(d8), rows * cols, cols, B.ptr(raw) if return_raw else None,
                                             B.ptr(u) if return_flow else None, B.ptr(v) if return_flow else None, B.stream_of(frames)))
    else:
        fs = [np.ascontiguousarray(f) for f in frames]
        if not fs or any(f.shape != fs[0].shape or f.dtype != fs[0].dtype for f in fs) or fs[0].dtype not in (np.uint8, np.float32) \
                or fs[0].ndim not in (2, 3):
            raise ValueError("frames: equal-shape uint8 or float32 frames expected")
        a = fs[0]
        cn = 1 if a.ndim == 2 else a.shape[2]
        rows, cols = a.shape[:2]
        lr, lc = max(rows >> int(level), 1), max(cols >> int(level), 1)
        np_ = max(len(fs) - 1, 1)
        d8 = np.empty((np_, lr, lc), np.uint8)
        raw = np.empty((np_, lr, lc), np.float32) if return_raw else None
        u = np.empty((np_, lr, lc), np.float32) if return_flow else None
        v = np.empty((np_, lr, lc), np.float32) if return_flow else None
        fp = (vp * len(fs))(*[f.ctypes.data for f in fs])
        check(lib.micv_ps5_warp_diff_seq_host(_ctx_for(a, ctx).handle, fp, len(fs), rows, cols, cols * cn * a.dtype.itemsize, cn,
                                              DEPTH_8U if a.dtype == np.uint8 else DEPTH_32F, int(levels), int(level), int(winSize),
                                              d8.ctypes.data, raw.ctypes.data if return_raw else None,
                                              u.ctypes.data if return_flow else None, v.ctypes.data if return_flow else None))
    out = (d8,) + ((raw,) if return_raw else ()) + ((u, v) if return_flow else ())
    return out[0] if len(out) == 1 else out


def denseLKDisplay(prevImg, nextImg, mode="naive", winSize=21, levels=4, color=GREEN, colorMaps=True, ctx=None):
    """One denseLKWrapper (Solution.cpp:40-84) as one call on two 8-bit frames of 1 or 3 channels: grey conversion, the flow
    (`mode` "naive": lk.calcOpticalFlow; "pyramidal": lk.calcOpticalFlowPyr with `levels`), the arrows on a copy of prevImg
    and the JET maps of u and v.  Returns (u, v, arrows) or, with colorMaps, (u, v, arrows, uColorMap, vColorMap)."""
    modes = {"naive": LK_NAIVE, "pyramidal": LK_PYRAMIDAL, "hierarchical": LK_PYRAMIDAL, LK_NAIVE: LK_NAIVE, LK_PYRAMIDAL: LK_PYRAMIDAL}
    if mode not in modes:
        raise ValueError("mode: 'naive' or 'pyramidal'")
    dev = B.is_dev(prevImg)
    if B.is_dev(nextImg) != dev:
        raise ValueError("prevImg and nextImg must both be numpy arrays or both CUDA tensors")
    rows, cols, cn, depth, pitch = _frame(prevImg, "prevImg")
    if _frame(nextImg, "nextImg") != (rows, cols, cn, depth, pitch):
        raise ValueError("prevImg and nextImg differ in size, format or row stride")
    uv = B.empty_like_shape(prevImg, (2, rows, cols))  # one behind the other: the colour maps are then one batch of two
    arrows = B.empty_like_shape(prevImg, (rows, cols, 3), np.uint8)
    jet = B.empty_like_shape(prevImg, (2, rows, cols, 3), np.uint8) if colorMaps else None
    args = (_ctx_for(prevImg, ctx).handle, B.ptr(prevImg), B.ptr(nextImg), rows, cols, pitch, cn, depth, modes[mode], int(winSize),
            int(levels), _color(color), B.ptr(uv[0]), B.ptr(uv[1]), cols * 4, B.ptr(arrows), cols * 3,
            B.ptr(jet[0]) if colorMaps else None, B.ptr(jet[1]) if colorMaps else None, cols * 3)
    if dev:
        check(lib.micv_dense_lk_display_dev(*args, B.stream_of(prevImg)))
    else:
        check(lib.micv_dense_lk_display_host(*args))
    return (uv[0], uv[1], arrows) + ((jet[0], jet[1]) if colorMaps else ())


def denseLKDisplaySequence(frames, winSize=21, levels=4, color=GREEN, colorMaps=True, ctx=None):
    """denseLKWrapper in pyramidal mode over consecutive frames (Solution.cpp:254-285) as one call
    (micv_dense_lk_display_seq_async / _host): 8-bit frames of 1 or 3 channels, a CUDA tensor [F, rows, cols(, 3)] or a
    sequence of equal numpy frames.  Returns a dictionary of [F - 1, ...] arrays: "u", "v", "arrows" and, with colorMaps,
    "uColorMap", "vColorMap"; pair p holds the bytes of denseLKDisplay(frames[p], frames[p + 1], "pyramidal")."""
    dev = B.is_dev(frames)
    if dev:
        if len(frames.shape) not in (3, 4) or frames.shape[0] < 2:
            raise ValueError("frames: need [F, rows, cols] or [F, rows, cols, 3] with F >= 2")
        rows, cols, cn, depth, pitch = _frame(frames[0], "frames")
        nf = int(frames.shape[0])
        fpitch = frames.stride(0) * frames.element_size()
        if fpitch < (rows - 1) * pitch + cols * cn:
            raise ValueError("frames: frames overlap")
        first = frames
    else:
        fs = [np.ascontiguousarray(f) for f in frames]
        if len(fs) < 2 or any(f.shape != fs[0].shape or f.dtype != fs[0].dtype for f in fs):
            raise ValueError("frames: at least two equal-shape frames expected")
        rows, cols, cn, depth, pitch = _frame(fs[0], "frames")
        nf = len(fs)
        first = fs[0]
    n = nf - 1
    uv = B.empty_like_shape(first, (2, n, rows, cols))
    arrows = B.empty_like_shape(first, (n, rows, cols, 3), np.uint8)
    jet = B.empty_like_shape(first, (2, n, rows, cols, 3), np.uint8) if colorMaps else None
    h = _ctx_for(first, ctx).handle
    if dev:
        check(lib.micv_dense_lk_display_seq_async(h, B.ptr(frames), fpitch, nf, rows, cols, pitch, cn, depth, int(winSize), int(levels),
                                                  _color(color), B.ptr(uv[0]), B.ptr(uv[1]), rows * cols * 4, cols * 4, B.ptr(arrows),
                                                  rows * cols * 3, cols * 3, B.ptr(jet[0]) if colorMaps else None,
                                                  B.ptr(jet[1]) if colorMaps else None, rows * cols * 3, cols * 3, B.stream_of(frames)))
    else:
        def ptrs(a):
            return (vp * n)(*[a[p].ctypes.data for p in range(n)])
        check(lib.micv_dense_lk_display_seq_host(h, (vp * nf)(*[f.ctypes.data for f in fs]), nf, rows, cols, pitch, cn, depth, int(winSize),
                                                 int(levels), _color(color), ptrs(uv[0]), ptrs(uv[1]), cols * 4, ptrs(arrows), cols * 3,
                                                 ptrs(jet[0]) if colorMaps else None, ptrs(jet[1]) if colorMaps else None, cols * 3))
    out = {"u": uv[0], "v": uv[1], "arrows": arrows}
    if colorMaps:
        out["uColorMap"], out["vColorMap"] = jet[0], jet[1]
    return out


def runProblem4(yosemite, pupper, winSize=21, levels=4, color=GREEN, ctx=None):
    """sol::runProblem4 (Solution.cpp:248-290) without the files: the two frame sets (each three 8-bit frames, or any
    sequence denseLKDisplaySequence takes) from two calls.  Returns {"ps5-4-a-1", "ps5-4-a-2", "ps5-4-b-1", "ps5-4-b-2"} ->
    the arrow picture of pairs (0, 1) and (1, 2) of the first and of the second set, plus "flows": the two dictionaries."""
    a = denseLKDisplaySequence(yosemite, winSize, levels, color, True, ctx)
    b = denseLKDisplaySequence(pupper, winSize, levels, color, True, ctx)
    if len(a["arrows"]) < 2 or len(b["arrows"]) < 2:
        raise ValueError("runProblem4: three frames per set expected")
    return {"ps5-4-a-1": a["arrows"][0], "ps5-4-a-2": a["arrows"][1], "ps5-4-b-1": b["arrows"][0], "ps5-4-b-2": b["arrows"][1],
            "flows": (a, b)}
