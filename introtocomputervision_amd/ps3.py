"""The ps3 driver of the reference (ProblemSets/ps3_cpp/src/Solution.cpp:122-158 and :323-481) after the geometry of
`geometry.py`, on the device: drawEpipolarLines, and runProblem2 / runExtraCredit from the point sets to the two annotated
pictures (csrc/ps3.hip).  numpy arrays take the `_host` entry points, torch CUDA tensors the `_dev` ones on the current
stream, where nothing synchronises and the end points are read on the device.  The drawing equals the host loop of the
shim byte for byte (include/mi_cv.h, "ps3: driver"; parity with OpenCV's rasteriser unpinned)."""
import numpy as np

from . import _buf as B
from ._capi import GEOM_F64, check, lib
from .geometry import _rows, fundamental
from .lk import _ctx_for
from .pf import _frame_view
from .ps6 import _colour, _image

LINE_COLOR = (0.0, 255.0, 0.0, 0.0)  # CV_RGB(0, 0xFF, 0), Solution.cpp:360-361, :472-473


def _rows_f32(a, width, like, name):
    """An [n, width] float32 list on `like`'s side, contiguous -> (array, n)."""
    if B.is_dev(like):
        import torch
        if not (B.is_dev(a) and a.is_cuda and a.dtype == torch.float32 and a.is_contiguous() and a.device == like.device):
            raise ValueError(f"{name}: need a contiguous float32 CUDA tensor on the image's device")
        a = a.reshape(-1, width)
    else:
        a = np.ascontiguousarray(a, np.float32).reshape(-1, width)
    return a, int(a.shape[0])


def _draw(fn, img, rows_of, width, name, color, ctx):
    rows, cols, ch, stride = _image(img)
    p, n = _rows_f32(rows_of, width, img, name)
    args = (_ctx_for(img, ctx).handle, B.ptr(img), rows, cols, ch, stride, B.ptr(p) if n else None, n, _colour(color))
    if B.is_dev(img):
        check(getattr(lib, fn + "_dev")(*args, B.stream_of(img)))
    else:
        check(getattr(lib, fn + "_host")(*args))
    return img


def drawSegments(img, segments, color=LINE_COLOR, ctx=None):
    """cv::line(img, Point2f(x1, y1), Point2f(x2, y2), color) for every row of segments [n, 4] float32, in place: img
    [rows, cols] or [rows, cols, C] uint8 with C in (1, 3, 4) and any row stride.  Exact for every pair of int32 end
    points, however far outside the image.  Returns img."""
    return _draw("micv_draw_segments", img, segments, 4, "segments", color, ctx)


def drawEpipolarLines(img, endpoints, color=LINE_COLOR, ctx=None):
    """sol::drawEpipolarLines from the [n, 6] end points of geometry.fundamental.epipolarEndpoints (P_iL, P_iR), in
    place.  A vertical epipolar line has NaN / inf end points and leaves the image as it is.  Returns img."""
    return _draw("micv_draw_epipolar_lines", img, endpoints, 6, "endpoints", color, ctx)


def epipolarDisplay(fMat, ptsA, ptsB, picA, picB, color=LINE_COLOR, f64=False, inplace=False, endpoints=False, ctx=None):
    """Part c of runProblem2 (Solution.cpp:341-363) in one launch: the lines of image B's points into picA, the lines of
    image A's points into picB.  fMat 3 x 3, ptsA and ptsB 2 x n float32, the pictures uint8 with C in (1, 3, 4), of any
    two sizes.  inplace=False paints copies and leaves the pictures as they are.  -> (outA, outB), and with
    endpoints=True also the [2, n, 6] end points, the bits of geometry.fundamental.epipolarEndpoints for side 0, 1."""
    dev = B.is_dev(picA)
    if B.is_dev(picB) != dev or B.is_dev(ptsA) != dev or B.is_dev(ptsB) != dev:
        raise ValueError("epipolarDisplay: pictures and points on one side expected (numpy, or CUDA tensors)")
    a, b = _rows(ptsA, 2, "ptsA"), _rows(ptsB, 2, "ptsB")
    n = int(a.shape[0])
    if int(b.shape[0]) != n:
        raise ValueError("ptsA and ptsB differ in their number of points")
    view = _image if inplace else _frame_view  # a picture that is only read may be read-only
    ra, ca, ch, sa = view(picA, "picA")
    rb, cb, chb, sb = view(picB, "picB")
    if ch != chb or ch not in (1, 3, 4):
        raise ValueError("picA and picB: one number of channels, 1, 3 or 4, expected")
    if dev:
        import torch
        F = (fMat if B.is_dev(fMat) else torch.from_numpy(np.ascontiguousarray(fMat, np.float32))).to(picA.device).contiguous()
        if F.dtype != torch.float32 or F.numel() != 9 or a.device != picA.device or picB.device != picA.device:
            raise ValueError("epipolarDisplay: a 3 x 3 float32 fMat and one device expected")
    else:
        F = np.ascontiguousarray(fMat, np.float32)
        if F.size != 9:
            raise ValueError("fMat: need 3 x 3")
    outA, outB = (picA, picB) if inplace else (B.empty_like_shape(p, tuple(p.shape), np.uint8) for p in (picA, picB))
    osa, osb = _image(outA, "outA")[3], _image(outB, "outB")[3]
    ends = B.empty_like_shape(picA, (2, n, 6), np.float32) if endpoints else None
    args = (_ctx_for(picA, ctx).handle, B.ptr(F), B.ptr(a), B.ptr(b), n, B.ptr(picA), sa, ra, ca, B.ptr(picB), sb, rb, cb, ch,
            GEOM_F64 if f64 else 0, _colour(color), B.ptr(outA), osa, B.ptr(outB), osb, B.ptr(ends) if endpoints else None)
    if dev:
        check(lib.micv_ps3_epipolar_display_dev(*args, B.stream_of(picA)))
    else:
        check(lib.micv_ps3_epipolar_display_host(*args))
    return (outA, outB, ends) if endpoints else (outA, outB)


def runProblem2(ptsA, ptsB, picA, picB, color=LINE_COLOR, f64=False, ctx=None):
    """sol::runProblem2 (:323-368): ptsA, ptsB 2 x n float32, picA, picB the two pictures -> (F estimate 3 x 3, F of
    rank 2, ps3-2-c-1, ps3-2-c-2).  CUDA tensors: a chain of `_dev` calls on the current stream with no host read."""
    if B.is_dev(ptsA):
        # geometry.fundamental.solveLeastSquares reads its status word on the host; without an index list there is
        # nothing the word could report, so the entry is called directly and the word is left on the device
        import torch
        a, b = _rows(ptsA, 2, "ptsA"), _rows(ptsB, 2, "ptsB")
        if a.shape != b.shape:
            raise ValueError("ptsA and ptsB differ in their number of points")
        n = int(a.shape[0])
        est = torch.zeros((3, 3), dtype=torch.float32, device=a.device)
        st = torch.zeros(1, dtype=torch.int32, device=a.device)
        check(lib.micv_fundamental_ls_dev(_ctx_for(a, ctx).handle, a.data_ptr(), b.data_ptr(), n, None, 0, n, 1,
                                          GEOM_F64 if f64 else 0, est.data_ptr(), st.data_ptr(), B.stream_of(a)))
    else:
        est = fundamental.solveLeastSquares(ptsA, ptsB, f64=f64, ctx=ctx).reshape(3, 3)
    F = fundamental.rankReduce(est, f64=f64, ctx=ctx)
    return (est, F) + epipolarDisplay(F, ptsA, ptsB, picA, picB, color, f64=f64, ctx=ctx)


def runExtraCredit(ptsA, ptsB, picA, picB, color=LINE_COLOR, f64=False, ctx=None):
    """sol::runExtraCredit (:370-481) -> (T_a, T_b, F_Hat, F, ps3-2-e-1, ps3-2-e-2), the normalised chain of
    geometry.fundamental.normalized and the same drawing."""
    Ta, Tb, Fh, F = fundamental.normalized(ptsA, ptsB, f64=f64, ctx=ctx)
    return (Ta, Tb, Fh, F) + epipolarDisplay(F, ptsA, ptsB, picA, picB, color, f64=f64, ctx=ctx)
