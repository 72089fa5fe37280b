"""`mhi::` namespace of the reference's ps7 (ProblemSets/ps7_cpp/include/MotionHistory.h:8-28):
frame differencing and motion-history images, device tensors (uint8 CUDA; frames of 1, 3 or 4 channels)."""
from ._capi import check, lib
from .lk import _ctx_for
from .match import _host_ctx


def _chk(t, name):
    import torch
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dim() == 2 and t.dtype == torch.uint8
            and t.stride(1) == 1):
        raise ValueError(f"{name}: need a 2-D uint8 CUDA tensor with unit column stride")


def _stream(t):
    import torch
    return torch.cuda.current_stream(t.device).cuda_stream


def _blur_wh(blurSize):
    """cv::Size(width, height) as (w, h); a bare int means a square."""
    if isinstance(blurSize, (tuple, list)):
        w, h = blurSize
        return int(w), int(h)
    return int(blurSize), int(blurSize)


def _chk_frame(t, name):
    """A [rows, cols] or [rows, cols, C] (C = 1, 3, 4; interleaved) uint8 CUDA tensor -> (rows, cols, channels)."""
    import torch
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 and t.dim() in (2, 3)):
        raise ValueError(f"{name}: need a [rows, cols] or [rows, cols, C] uint8 CUDA tensor")
    ch = 1 if t.dim() == 2 else t.shape[2]
    if ch not in (1, 3, 4):
        raise ValueError(f"{name}: {ch} channels (1, 3 or 4)")
    if t.stride(-1) != 1 or (t.dim() == 3 and t.stride(1) != ch) or t.stride(0) < t.shape[1] * ch:
        raise ValueError(f"{name}: need interleaved samples with unit stride and rows that do not overlap")
    return t.shape[0], t.shape[1], ch


def frameDifference(f1, f2, thresh, blurSize=(3, 3), blurSigma=1.0, ctx=None):
    """mhi::frameDifference (MotionHistory.cpp:26-77) -> {0,1} uint8 mask [rows, cols].  blurSize is the
    reference's cv::Size as (width, height) (MotionHistory.h:14; default cv::Size(3, 3)).  Frames are
    [rows, cols] or, as a cv::VideoCapture hands them over, [rows, cols, 3 | 4] interleaved (mi_cv.h:
    micv_mhi_frame_difference_c_dev)."""
    import numpy as np
    bw, bh = _blur_wh(blurSize)
    if isinstance(f1, np.ndarray):  # host-pointer entry point
        a1 = np.ascontiguousarray(f1, np.uint8)
        a2 = np.ascontiguousarray(f2, np.uint8)
        if a1.ndim == 3 and a1.shape == a2.shape:
            if a1.shape[2] not in (1, 3, 4):
                raise ValueError(f"f1 / f2: {a1.shape[2]} channels (1, 3 or 4)")
            out = np.empty(a1.shape[:2], np.uint8)
            check(lib.micv_mhi_frame_difference_c_host((ctx or _host_ctx()).handle, a1.ctypes.data, a2.ctypes.data,
                                                       a1.shape[0], a1.shape[1], a1.shape[2], a1.strides[0],
                                                       float(thresh), bw, bh, float(blurSigma), out.ctypes.data,
                                                       out.strides[0]))
            return out
        if a1.ndim != 2 or a1.shape != a2.shape:
            raise ValueError("f1 / f2: need 2-D (or [rows, cols, C]) uint8 arrays of equal shape")
        out = np.empty_like(a1)
        check(lib.micv_mhi_frame_difference_host((ctx or _host_ctx()).handle, a1.ctypes.data, a2.ctypes.data,
                                                 a1.shape[0], a1.shape[1], a1.strides[0], float(thresh),
                                                 bw, bh, float(blurSigma), out.ctypes.data,
                                                 out.strides[0]))
        return out
    import torch
    if isinstance(f1, torch.Tensor) and f1.dim() == 3:
        rows, cols, ch = _chk_frame(f1, "f1")
        if _chk_frame(f2, "f2") != (rows, cols, ch) or f1.stride(0) != f2.stride(0):
            raise ValueError("f1 and f2 differ in size / stride")
        diff = torch.empty((rows, cols), dtype=torch.uint8, device=f1.device)
        check(lib.micv_mhi_frame_difference_c_dev(_ctx_for(f1, ctx).handle, f1.data_ptr(), f2.data_ptr(), rows, cols, ch,
                                                  f1.stride(0), float(thresh), bw, bh, float(blurSigma),
                                                  diff.data_ptr(), cols, _stream(f1)))
        return diff
    _chk(f1, "f1")
    _chk(f2, "f2")
    if tuple(f1.shape) != tuple(f2.shape) or f1.stride(0) != f2.stride(0):
        raise ValueError("f1 and f2 differ in size / stride")
    rows, cols = f1.shape
    diff = torch.empty((rows, cols), dtype=torch.uint8, device=f1.device)
    check(lib.micv_mhi_frame_difference_dev(_ctx_for(f1, ctx).handle, f1.data_ptr(), f2.data_ptr(), rows,
                                            cols, f1.stride(0), float(thresh), bw, bh,
                                            float(blurSigma), diff.data_ptr(), cols, _stream(f1)))
    return diff


def thresholdDifference(src, thresh, ctx=None):
    """thresholdDifference (MotionHistory.cu:27-48) -> {0,1} uint8."""
    import numpy as np
    if isinstance(src, np.ndarray):
        a1 = np.ascontiguousarray(src, np.uint8)
        out = np.empty_like(a1)
        check(lib.micv_mhi_threshold_host((ctx or _host_ctx()).handle, a1.ctypes.data, a1.shape[0], a1.shape[1],
                                          a1.strides[0], float(thresh), out.ctypes.data, out.strides[0]))
        return out
    import torch
    _chk(src, "src")
    rows, cols = src.shape
    dst = torch.empty((rows, cols), dtype=torch.uint8, device=src.device)
    check(lib.micv_mhi_threshold_dev(_ctx_for(src, ctx).handle, src.data_ptr(), rows, cols, src.stride(0),
                                     float(thresh), dst.data_ptr(), cols, _stream(src)))
    return dst


def calcMotionHistory(history, binaryMask, tau, ctx=None):
    """mhi::calcMotionHistory (MotionHistory.cpp:79-96): updates `history` in place."""
    import numpy as np
    if isinstance(history, np.ndarray):
        if history.dtype != np.uint8 or history.ndim != 2 or not history.flags.c_contiguous:
            raise ValueError("history: need a contiguous 2-D uint8 array (updated in place)")
        m = np.ascontiguousarray(binaryMask, np.uint8)
        if m.shape != history.shape:
            raise ValueError("history and binaryMask differ in size")
        check(lib.micv_mhi_update_host((ctx or _host_ctx()).handle, history.ctypes.data, history.strides[0],
                                       m.ctypes.data, m.strides[0], history.shape[0], history.shape[1], int(tau)))
        return history
    _chk(history, "history")
    _chk(binaryMask, "binaryMask")
    if tuple(history.shape) != tuple(binaryMask.shape):
        raise ValueError("history and binaryMask differ in size")
    rows, cols = history.shape
    check(lib.micv_mhi_update_dev(_ctx_for(history, ctx).handle, history.data_ptr(), history.stride(0),
                                  binaryMask.data_ptr(), binaryMask.stride(0), rows, cols, int(tau),
                                  _stream(history)))
    return history


def energyFromHistory(mhi, ctx=None):
    """mhi::energyFromHistory (MotionHistory.cpp:98-112): any nonzero history value -> 1.  A list of
    histories gives a list of energies (the vector overload, :107-112)."""
    import numpy as np
    if isinstance(mhi, (list, tuple)):
        return [energyFromHistory(m, ctx) for m in mhi]
    if isinstance(mhi, np.ndarray):
        a = np.ascontiguousarray(mhi, np.uint8)
        if a.ndim != 2:
            raise ValueError("mhi: need a 2-D uint8 array")
        out = np.empty_like(a)
        check(lib.micv_mhi_energy_host((ctx or _host_ctx()).handle, a.ctypes.data, a.shape[0], a.shape[1],
                                       a.strides[0], out.ctypes.data, out.strides[0]))
        return out
    import torch
    _chk(mhi, "mhi")
    rows, cols = mhi.shape
    mei = torch.empty((rows, cols), dtype=torch.uint8, device=mhi.device)
    check(lib.micv_mhi_energy_dev(_ctx_for(mhi, ctx).handle, mhi.data_ptr(), rows, cols, mhi.stride(0),
                                  mei.data_ptr(), cols, _stream(mhi)))
    return mei


def _chk_frames(frames, name="frames"):
    """[F, rows, cols] or [F, rows, cols, C] uint8 CUDA tensor -> (F, rows, cols, channels)."""
    import torch
    if not (isinstance(frames, torch.Tensor) and frames.is_cuda and frames.dim() in (3, 4) and frames.dtype == torch.uint8):
        raise ValueError(f"{name}: need a [F, rows, cols] or [F, rows, cols, C] uint8 CUDA tensor")
    ch = 1 if frames.dim() == 3 else frames.shape[3]
    if ch not in (1, 3, 4):
        raise ValueError(f"{name}: {ch} channels (1, 3 or 4)")
    F, rows, cols = frames.shape[:3]
    if frames.stride(-1) != 1 or (frames.dim() == 4 and frames.stride(2) != ch) or frames.stride(1) < cols * ch \
            or frames.stride(0) < rows * frames.stride(1):
        raise ValueError(f"{name}: need interleaved samples with unit stride, rows and frames that do not overlap")
    return F, rows, cols, ch


def historySequence(frames, thresh, blurSize, blurSigma, tau, saveFrames, ctx=None, saveDiffFrames=()):
    """mhiHelper's loop (ps7_cpp/src/Solution.cpp:16-101) over one video: frames is [F, rows, cols] or
    [F, rows, cols, C] uint8; the history after update number j (frameDifference(frame j-1, frame j), then
    calcMotionHistory) is returned for every j in saveFrames (1..F-1, mhiHelper's frameNum), stacked as
    [len(saveFrames), rows, cols] uint8.  With saveDiffFrames the result is the pair (histories, masks): the {0,1}
    mask of update j for every j in saveDiffFrames (mhiHelper's saveMHIFrames and saveDiffFrames)."""
    import numpy as np
    bw, bh = _blur_wh(blurSize)
    save = np.ascontiguousarray(np.asarray(saveFrames, dtype=np.int32).reshape(-1))
    sdiff = np.ascontiguousarray(np.asarray(saveDiffFrames, dtype=np.int32).reshape(-1))
    plain = sdiff.size == 0 and frames.ndim == 3
    if isinstance(frames, np.ndarray):
        if frames.ndim not in (3, 4) or frames.dtype != np.uint8:
            raise ValueError("frames: need a [F, rows, cols] or [F, rows, cols, C] uint8 array")
        ok = frames.strides[-1] == 1 and min(frames.strides) > 0 and (frames.ndim == 3 or frames.strides[2] == frames.shape[3])
        f = frames if ok else np.ascontiguousarray(frames)
        F, rows, cols = f.shape[:3]
        out = np.empty((save.size, rows, cols), np.uint8)
        if plain:
            check(lib.micv_mhi_history_seq_host((ctx or _host_ctx()).handle, f.ctypes.data, F, f.strides[0], f.strides[1],
                                                rows, cols, float(thresh), bw, bh, float(blurSigma), int(tau),
                                                save.ctypes.data, save.size, out.ctypes.data, out.strides[0],
                                                out.strides[1]))
            return out
        dout = np.empty((sdiff.size, rows, cols), np.uint8)
        check(lib.micv_mhi_history_seq_c_host((ctx or _host_ctx()).handle, f.ctypes.data, F, f.strides[0], f.strides[1], rows,
                                              cols, 1 if f.ndim == 3 else f.shape[3], float(thresh), bw, bh, float(blurSigma),
                                              int(tau), save.ctypes.data if save.size else None, save.size,
                                              out.ctypes.data if save.size else None, rows * cols, cols,
                                              sdiff.ctypes.data if sdiff.size else None, sdiff.size,
                                              dout.ctypes.data if sdiff.size else None, rows * cols, cols))
        return (out, dout) if sdiff.size else out
    import torch
    F, rows, cols, ch = _chk_frames(frames)
    out = torch.empty((save.size, rows, cols), dtype=torch.uint8, device=frames.device)
    if plain:
        check(lib.micv_mhi_history_seq_dev(_ctx_for(frames, ctx).handle, frames.data_ptr(), F, frames.stride(0),
                                           frames.stride(1), rows, cols, float(thresh), bw, bh, float(blurSigma), int(tau),
                                           save.ctypes.data, save.size, out.data_ptr(), rows * cols, cols,
                                           _stream(frames)))
        return out
    dout = torch.empty((sdiff.size, rows, cols), dtype=torch.uint8, device=frames.device)
    check(lib.micv_mhi_history_seq_c_dev(_ctx_for(frames, ctx).handle, frames.data_ptr(), F, frames.stride(0), frames.stride(1),
                                         rows, cols, ch, float(thresh), bw, bh, float(blurSigma), int(tau),
                                         save.ctypes.data if save.size else None, save.size,
                                         out.data_ptr() if save.size else None, rows * cols, cols,
                                         sdiff.ctypes.data if sdiff.size else None, sdiff.size,
                                         dout.data_ptr() if sdiff.size else None, rows * cols, cols, _stream(frames)))
    return (out, dout) if sdiff.size else out


def historyBatch(videos, thresh, blurSize, blurSigma, tau, saveFrame, ctx=None):
    """getAllMHIs' loop (Solution.cpp:113-146) in one call (micv_mhi_history_batch_dev): videos is a list of
    [F_v, rows, cols] or [F_v, rows, cols, C] uint8 CUDA tensors of one size, channel count and stride; thresh, tau and
    saveFrame are one value for all or one per video.  -> [V, rows, cols] uint8, the history after update saveFrame[v].
    No host synchronisation."""
    import ctypes
    import numpy as np
    import torch
    bw, bh = _blur_wh(blurSize)
    V = len(videos)
    shapes = {(_chk_frames(v, f"videos[{i}]")[1:], v.stride(0), v.stride(1), v.device) for i, v in enumerate(videos)}
    if len(shapes) > 1:
        raise ValueError("videos: differ in size, channels, stride or device")
    if V == 0:
        raise ValueError("videos: need at least one")
    per = lambda x, dt: np.ascontiguousarray(np.broadcast_to(np.asarray(x, dtype=dt).reshape(-1), (V,)))
    th, ta, sv = per(thresh, np.float64), per(tau, np.int32), per(saveFrame, np.int32)
    ptrs = (ctypes.c_void_p * V)(*[v.data_ptr() for v in videos])
    nfr = np.array([v.shape[0] for v in videos], np.int32)
    v0 = videos[0]
    _, rows, cols, ch = _chk_frames(v0)
    out = torch.empty((V, rows, cols), dtype=torch.uint8, device=v0.device)
    check(lib.micv_mhi_history_batch_dev(_ctx_for(v0, ctx).handle, ptrs, nfr.ctypes.data, v0.stride(0), v0.stride(1), V, rows,
                                         cols, ch, th.ctypes.data, ta.ctypes.data, sv.ctypes.data, bw, bh, float(blurSigma),
                                         out.data_ptr(), rows * cols, cols, _stream(v0)))
    return out
