"""The ps6 driver of the reference (ProblemSets/ps6_cpp/src/Solution.cpp:16-195) around `pf.ParticleFilter`, on the
device: the dot per particle of ParticleFilter::drawParticles, cv::rectangle around the estimate, pfDriver's loop body as
one call and the whole loop over a host sequence with the kept frames coming back annotated (csrc/ps6.hip).  numpy arrays
take the `_host` entry points, torch CUDA tensors the `_dev` ones on the current stream, where nothing synchronises and
the particles and the estimate are read on the device.  The drawing equals the host loops of the shim byte for byte
(include/mi_cv.h, "ps6: driver"; parity with OpenCV's rasteriser unpinned)."""
import ctypes as C

import numpy as np

from . import _buf as B
from ._capi import check, lib
from .lk import _ctx_for
from .pf import MEAN_SHIFT_LT, MEAN_SQ_ERR, STATE_DTYPE, ParticleFilter, _frame_view

DOT_COLOR = (0.0, 255.0, 0.0, 0.0)    # Solution.cpp:74
BOX_COLOR = (255.0, 0.0, 255.0, 0.0)  # Solution.cpp:78
HAND_BBOX, HAND_SIZE = (540.0, 385.0), (73.0, 87.0)  # Solution.cpp:144-145, :182-183
INT_MIN = -(1 << 31)
# the save sets of runProblem1 / 2 / 3 (Solution.cpp:120, :127, :151, :159, :177, :190)
SAVE_1A, SAVE_1E = (28, 84, 144), (14, 32, 46)
SAVE_2A, SAVE_2B = (15, 50, 150), (15, 50, 150)
SAVE_3A, SAVE_3B = (28, 84, 144), (15, 50, 140)


def _colour(color):
    c = [float(v) for v in color]
    if not 1 <= len(c) <= 4:
        raise ValueError("color: 1 to 4 values expected")
    return (C.c_double * 4)(*(c + [0.0] * (4 - len(c))))


def _image(img, name="img"):
    rows, cols, ch, stride = _frame_view(img, name)
    if ch not in (1, 3, 4):
        raise ValueError(f"{name}: 1, 3 or 4 channels expected")
    if not B.is_dev(img) and not img.flags.writeable:
        raise ValueError(f"{name}: a writable array expected")
    return rows, cols, ch, stride


def _xy(particles, like):
    """An [n, 2] float32 list on `like`'s side, contiguous -> (array, n)."""
    if B.is_dev(like):
        import torch
        if not (B.is_dev(particles) and particles.is_cuda and particles.dtype == torch.float32 and particles.is_contiguous()
                and particles.device == like.device):
            raise ValueError("particles: need a contiguous float32 CUDA tensor on the image's device")
        p = particles.reshape(-1, 2)
    else:
        p = np.ascontiguousarray(particles, np.float32).reshape(-1, 2)
    return p, int(p.shape[0])


def cvRound(v):
    """The project's cvRound of a float: halves to even; INT_MIN for NaN, +-inf and every value outside int."""
    v = np.float32(v)
    if not (v >= np.float32(-2147483648.0) and v < np.float32(2147483648.0)):
        return INT_MIN
    return int(np.rint(v))


def boxRect(centre, bboxSize):
    """cv::Rect(Point2f(c.x - w / 2, c.y - h / 2), Size2f(w, h)) as the driver builds it (:76-78) -> (x, y, w, h)."""
    w, h = np.float32(bboxSize[0]), np.float32(bboxSize[1])
    with np.errstate(invalid="ignore", over="ignore"):
        x, y = np.float32(centre[0]) - w / np.float32(2), np.float32(centre[1]) - h / np.float32(2)
    return cvRound(x), cvRound(y), cvRound(w), cvRound(h)


def drawParticles(img, particles, color=DOT_COLOR, ctx=None):
    """ParticleFilter::drawParticles on a particle list, in place: img [rows, cols] or [rows, cols, C] uint8 with C in
    (1, 3, 4) and any row stride, particles [n, 2] float32 (x, y).  Returns img."""
    rows, cols, ch, stride = _image(img)
    p, n = _xy(particles, img)
    args = (_ctx_for(img, ctx).handle, B.ptr(img), rows, cols, ch, stride, B.ptr(p) if n else None, n, _colour(color))
    if B.is_dev(img):
        check(lib.micv_draw_particles_dev(*args, B.stream_of(img)))
    else:
        check(lib.micv_draw_particles_host(*args))
    return img


def rectangle(img, rect, color=BOX_COLOR, ctx=None):
    """cv::rectangle(img, Rect(x, y, w, h), color) at its defaults, in place.  Returns img."""
    rows, cols, ch, stride = _image(img)
    x, y, w, h = (int(v) for v in rect)
    args = (_ctx_for(img, ctx).handle, B.ptr(img), rows, cols, ch, stride, x, y, w, h, _colour(color))
    if B.is_dev(img):
        check(lib.micv_draw_rectangle_dev(*args, B.stream_of(img)))
    else:
        check(lib.micv_draw_rectangle_host(*args))
    return img


def overlay(img, particles, centre, bboxSize, dotColor=DOT_COLOR, boxColor=BOX_COLOR, ctx=None):
    """The driver's painting of one frame in one launch, in place: the dots, then the box of `bboxSize` (floats) around
    `centre`.  Device: centre is a float32 CUDA tensor of (at least) 2 words, the estimate where a chain left it."""
    rows, cols, ch, stride = _image(img)
    p, n = _xy(particles, img)
    if B.is_dev(img):
        import torch
        if not (B.is_dev(centre) and centre.is_cuda and centre.dtype == torch.float32 and centre.numel() >= 2 and centre.is_contiguous()):
            raise ValueError("centre: need a contiguous float32 CUDA tensor of 2 words")
        c = centre
    else:
        c = np.ascontiguousarray(centre, np.float32).reshape(2)
    args = (_ctx_for(img, ctx).handle, B.ptr(img), rows, cols, ch, stride, B.ptr(p) if n else None, n, _colour(dotColor), B.ptr(c),
            float(bboxSize[0]), float(bboxSize[1]), _colour(boxColor))
    if B.is_dev(img):
        check(lib.micv_ps6_overlay_list_dev(*args, B.stream_of(img)))
    else:
        check(lib.micv_ps6_overlay_list_host(*args))
    return img


def overlayFilter(pf, frame, bboxSize, dotColor=DOT_COLOR, boxColor=BOX_COLOR):
    """The filter's current particles and the box around its current mean, into a CUDA frame in place
    (micv_ps6_overlay_dev): everything is read on the device."""
    if not B.is_dev(frame):
        raise ValueError("overlayFilter: a CUDA tensor expected (numpy frames: tickDisplay)")
    stride = pf._check_frame(frame)
    check(lib.micv_ps6_overlay_dev(pf._h, frame.data_ptr(), stride, _colour(dotColor), float(bboxSize[0]), float(bboxSize[1]),
                                   _colour(boxColor), B.stream_of(frame)))
    return frame


def tickDisplay(pf, frame, bboxSize, dotColor=DOT_COLOR, boxColor=BOX_COLOR, out=None):
    """One pass of pfDriver's loop body: pf.tick(frame), then the dots and the box into `out` (None: a new image;
    `frame` itself: in place).  -> (state, out): numpy frames give a STATE_DTYPE record (and set pf.last_status), CUDA
    tensors the 5-word device state of pf.tick; nothing synchronises there."""
    stride = pf._check_frame(frame)
    if out is None:
        out = B.empty_like_shape(frame, tuple(frame.shape), np.uint8)
    if B.is_dev(out) != B.is_dev(frame) or tuple(out.shape) != tuple(frame.shape):
        raise ValueError("out: an image of the frame's kind and shape expected")
    ostride = pf._check_frame(out)
    args = (pf._h, B.ptr(frame), stride, B.ptr(out), ostride, _colour(dotColor), float(bboxSize[0]), float(bboxSize[1]), _colour(boxColor))
    if B.is_dev(frame):
        import torch
        st = torch.empty(5, dtype=torch.int32, device=frame.device)
        check(lib.micv_ps6_tick_display_dev(*args, B.stream_of(frame), st.data_ptr()))
        return st, out
    if not out.flags.writeable:
        raise ValueError("out: a writable array expected")
    st = np.zeros(1, STATE_DTYPE)
    check(lib.micv_ps6_tick_display_host(*args, st.ctypes.data))
    pf.last_status = int(st[0]["status"])
    return st[0], out


def trackDisplay(pf, frames, bboxSize, saveFrames=(), allFrames=False, dotColor=DOT_COLOR, boxColor=BOX_COLOR):
    """pfDriver's loop over host frames as one call (micv_ps6_track_display_seq_host) -> (STATE_DTYPE array, {index:
    annotated frame}): the frames whose 0-based index is in saveFrames, or every frame with allFrames."""
    frames = [np.asarray(f) for f in frames]
    if not frames:
        raise ValueError("trackDisplay: no frames")
    strides = {pf._check_frame(f) for f in frames}
    if len(strides) != 1:
        raise ValueError("trackDisplay: every frame needs the same row stride")
    save = sorted({int(t) for t in saveFrames})
    keep = list(range(len(frames))) if allFrames else save
    outs = [np.empty(frames[0].shape, np.uint8) for _ in keep]
    ptrs = (C.c_void_p * len(frames))(*[f.ctypes.data for f in frames])
    optrs = (C.c_void_p * max(len(outs), 1))(*[o.ctypes.data for o in outs])
    sv = (C.c_int * max(len(save), 1))(*save)
    states = np.zeros(len(frames), STATE_DTYPE)
    rows, cols, ch, _ = _frame_view(frames[0])
    check(lib.micv_ps6_track_display_seq_host(pf._h, ptrs, len(frames), strides.pop(), _colour(dotColor), float(bboxSize[0]),
                                              float(bboxSize[1]), _colour(boxColor), sv, len(save), 1 if allFrames else 0, optrs,
                                              cols * ch, states.ctypes.data))
    return states, dict(zip(keep, outs))


def trackDisplayGroup(group, frames, bboxSizes, saveFrames, allFrames=False, dotColor=DOT_COLOR, boxColor=BOX_COLOR):
    """trackDisplay for a pf.FilterGroup over ONE sequence of host frames (micv_ps6_group_track_display_seq_host): every
    frame is uploaded once and ticked for all members in three launches; each member gets its own annotated pictures.
    bboxSizes: K (width, height) pairs; saveFrames: K collections of 0-based indices.
    -> (STATE_DTYPE array [nframes, K], [{index: annotated frame}] * K), member k's part equal to trackDisplay on it."""
    k = len(group)
    if len(bboxSizes) != k or len(saveFrames) != k:
        raise ValueError(f"trackDisplayGroup: {k} bounding-box sizes and {k} save sets expected")
    frames, ptrs, stride = group._host_frames(frames, "trackDisplayGroup")
    saves = [sorted({int(t) for t in s}) for s in saveFrames]
    keeps = [list(range(len(frames))) if allFrames else s for s in saves]
    outs = [[np.empty(frames[0].shape, np.uint8) for _ in keep] for keep in keeps]
    sv = [(C.c_int * max(len(s), 1))(*s) for s in saves]
    op = [(C.c_void_p * max(len(o), 1))(*[a.ctypes.data for a in o]) for o in outs]
    svp = (C.c_void_p * k)(*[C.addressof(a) for a in sv])
    opp = (C.c_void_p * k)(*[C.addressof(a) for a in op])
    nsave = (C.c_int * k)(*[len(s) for s in saves])
    wh = (C.c_float * (2 * k))(*[float(v) for b in bboxSizes for v in (b[0], b[1])])
    states = np.zeros((len(frames), k), STATE_DTYPE)
    rows, cols, ch, _ = _frame_view(frames[0])
    check(lib.micv_ps6_group_track_display_seq_host(group._h, ptrs, len(frames), stride, _colour(dotColor), wh, _colour(boxColor), svp,
                                                    nsave, 1 if allFrames else 0, opp, cols * ch, states.ctypes.data))
    return states, [dict(zip(keep, o)) for keep, o in zip(keeps, outs)]


def _driverFilter(f0, bbox, bboxSize, conf, simMode, **kw):
    """The filter pfDriver makes on its first frame (Solution.cpp:40-58)."""
    x, y, w, h = (cvRound(v) for v in (bbox[0], bbox[1], bboxSize[0], bboxSize[1]))
    if not (0 <= x and 0 <= y and w > 0 and h > 0 and x + w <= f0.shape[1] and y + h <= f0.shape[0]):
        raise ValueError("pfDriver: the bounding box does not lie in the frame")
    return ParticleFilter(f0[y:y + h, x:x + w].copy(), (f0.shape[1], f0.shape[0]), conf["num_particles"], simMode, conf["mse_sigma"],
                          conf["dynamics_sigma"], (float(bbox[0]), float(bbox[1])), **kw)


def pfDriver(frames, bbox, bboxSize, conf, simMode, saveFrames, allFrames=False, **kw):
    """pfDriver (Solution.cpp:16-107) over host frames: the model is frame 0 at cv::Rect(bbox, bboxSize) (each value
    through cvRound; a copy, not the reference's view into frame 0), the filter starts GAUSSIAN at the bbox with `conf`
    (config.pf_params: num_particles, mse_sigma, dynamics_sigma; alpha is the constructor's default 0.1, as the driver
    leaves it).  -> (STATE_DTYPE array, {index: annotated frame}); save indices past the sequence are never reached, as
    in the reference."""
    frames = [np.asarray(f) for f in frames]
    filt = _driverFilter(frames[0], bbox, bboxSize, conf, simMode, **kw)
    try:
        return trackDisplay(filt, frames, bboxSize, [t for t in saveFrames if 0 <= int(t) < len(frames)], allFrames)
    finally:
        filt.close()


def _bbox(bboxes, name):
    (x, y), (w, h) = bboxes[name]
    return (x, y), (w, h)


def runProblem1(frames_clean, frames_noisy, cfg, bboxes):
    """sol::runProblem1 (:109-132).  cfg: config.load(ps6.yaml); bboxes: {"pres_debate": ((x, y), (w, h)), "noisy_debate":
    ..} as config.load_bbox gives them.  -> {"ps6-1-a": (states, {index: frame}), "ps6-1-e": ..}."""
    from . import config
    a, e = _bbox(bboxes, "pres_debate"), _bbox(bboxes, "noisy_debate")
    return {"ps6-1-a": pfDriver(frames_clean, a[0], a[1], config.pf_params(cfg, "pfconf1"), MEAN_SQ_ERR, SAVE_1A),
            "ps6-1-e": pfDriver(frames_noisy, e[0], e[1], config.pf_params(cfg, "pfconf1_noisy"), MEAN_SQ_ERR, SAVE_1E)}


def runProblem2(frames_clean, frames_noisy, cfg, bboxes=None):
    """sol::runProblem2 (:134-164): Romney's hand, clean and noisy."""
    from . import config
    return {"ps6-2-a": pfDriver(frames_clean, HAND_BBOX, HAND_SIZE, config.pf_params(cfg, "pfconf2"), MEAN_SQ_ERR, SAVE_2A),
            "ps6-2-b": pfDriver(frames_noisy, HAND_BBOX, HAND_SIZE, config.pf_params(cfg, "pfconf2_noisy"), MEAN_SQ_ERR, SAVE_2B)}


def runProblem3(frames_clean, frames_noisy, cfg, bboxes):
    """sol::runProblem3 (:166-195): the histogram likelihood on the head and on the hand (both on the clean frames)."""
    from . import config
    a = _bbox(bboxes, "pres_debate")
    return {"ps6-3-a": pfDriver(frames_clean, a[0], a[1], config.pf_params(cfg, "pfconf3_head"), MEAN_SHIFT_LT, SAVE_3A),
            "ps6-3-b": pfDriver(frames_clean, HAND_BBOX, HAND_SIZE, config.pf_params(cfg, "pfconf3_hand"), MEAN_SHIFT_LT, SAVE_3B)}


def pfDriverGroup(frames, runs):
    """Several pfDriver runs over ONE sequence of host frames as one group: runs is a list of (bbox, bboxSize, conf, simMode,
    saveFrames).  -> [(STATE_DTYPE array, {index: annotated frame})] in the order of runs, each equal to pfDriver's."""
    from .pf import FilterGroup
    frames = [np.asarray(f) for f in frames]
    filters, group = [], None
    try:
        for bbox, size, conf, mode, _ in runs:
            filters.append(_driverFilter(frames[0], bbox, size, conf, mode))
        group = FilterGroup(filters)
        states, kept = trackDisplayGroup(group, frames, [r[1] for r in runs],
                                         [[t for t in r[4] if 0 <= int(t) < len(frames)] for r in runs])
        return [(np.ascontiguousarray(states[:, k]), kept[k]) for k in range(len(runs))]
    finally:
        if group is not None:
            group.close()
        for f in filters:
            f.close()


def runProblems(frames_clean, frames_noisy, cfg, bboxes):
    """runProblem1, 2 and 3 together: the six drivers as TWO groups, four filters on the clean frames and two on the noisy
    ones, so each video is uploaded once and each of its frames ticked for all its filters in three launches.  -> the union
    of the three dictionaries ("ps6-1-a" .. "ps6-3-b"), byte-equal to them.  The hand's box is bboxes["hand"] where given
    (((x, y), (w, h)) like the others), the reference's constants otherwise."""
    from . import config
    a, e = _bbox(bboxes, "pres_debate"), _bbox(bboxes, "noisy_debate")
    hand = _bbox(bboxes, "hand") if "hand" in bboxes else (HAND_BBOX, HAND_SIZE)
    conf = lambda name: config.pf_params(cfg, name)
    clean = pfDriverGroup(frames_clean, [(a[0], a[1], conf("pfconf1"), MEAN_SQ_ERR, SAVE_1A),
                                         (hand[0], hand[1], conf("pfconf2"), MEAN_SQ_ERR, SAVE_2A),
                                         (a[0], a[1], conf("pfconf3_head"), MEAN_SHIFT_LT, SAVE_3A),
                                         (hand[0], hand[1], conf("pfconf3_hand"), MEAN_SHIFT_LT, SAVE_3B)])
    noisy = pfDriverGroup(frames_noisy, [(e[0], e[1], conf("pfconf1_noisy"), MEAN_SQ_ERR, SAVE_1E),
                                         (hand[0], hand[1], conf("pfconf2_noisy"), MEAN_SQ_ERR, SAVE_2B)])
    return {"ps6-1-a": clean[0], "ps6-1-e": noisy[0], "ps6-2-a": clean[1], "ps6-2-b": noisy[1], "ps6-3-a": clean[2],
            "ps6-3-b": clean[3]}
