"""ParticleFilter of the reference's ps6 (ProblemSets/ps6_cpp/include/ParticleFilter.h, lib/ParticleFilter.cpp) on
the HIP kernels of csrc/pf.hip.  The arithmetic contract is include/mi_cv.h's "ps6: particle filter" block.

numpy frames take ``micv_pf_tick_host``, torch CUDA tensors ``micv_pf_tick_dev`` (asynchronous on the tensor's
current stream; the state then comes back as a device tensor).  `track(frames)` runs a whole host sequence through
``micv_pf_track_seq_host``."""
import ctypes as C

import numpy as np

from . import _buf as B
from ._capi import check, lib
from .lk import _ctx_for

MEAN_SQ_ERR, MEAN_SHIFT_LT = 0, 1  # ParticleFilter::SimilarityMode
MSE_SIGNED = 1
STATUS_NO_WEIGHT, STATUS_CLAMPED = 1, 2
MAX_PARTICLES = 4096
DEFAULT_SEED = 0xFFFFFFFF
STATE_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("x_var", "<f4"), ("y_var", "<f4"), ("status", "<u4")])


def _frame_view(frame, name="frame"):
    """(rows, cols, channels, stride) of an HxW or HxWxC u8 array / tensor with dense pixels."""
    if B.is_dev(frame):
        import torch
        if not frame.is_cuda or frame.dtype != torch.uint8:
            raise ValueError(f"{name}: need a uint8 CUDA tensor")
        if frame.dim() == 2:
            frame = frame.unsqueeze(-1)
        if frame.dim() != 3 or frame.stride(2) != 1 or frame.stride(1) != frame.shape[2]:
            raise ValueError(f"{name}: need H x W or H x W x C with dense pixels")
        return frame.shape[0], frame.shape[1], frame.shape[2], frame.stride(0)
    if not isinstance(frame, np.ndarray) or frame.dtype != np.uint8 or frame.ndim not in (2, 3):
        raise ValueError(f"{name}: need a 2-D or 3-D numpy array of uint8")
    ch = frame.shape[2] if frame.ndim == 3 else 1
    if frame.strides[1] != ch or (frame.ndim == 3 and frame.strides[2] != 1):
        raise ValueError(f"{name}: need dense pixels")
    return frame.shape[0], frame.shape[1], ch, frame.strides[0] if frame.shape[0] > 1 else frame.shape[1] * ch


class ParticleFilter:
    """ParticleFilter(model, imSize, numParticles, simMode, mseSigma, sampleSigma, initModelPos=(-1, -1), alpha=0.1).

    model: H x W (x 3) uint8 numpy array, copied.  imSize: (width, height) as cv::Size.  flags / seed: the library's
    extensions (MSE_SIGNED; the cv::RNG state every fresh generator starts from)."""

    def __init__(self, model, imSize, numParticles, simMode, mseSigma, sampleSigma, initModelPos=(-1.0, -1.0),
                 alpha=0.1, flags=0, seed=DEFAULT_SEED, ctx=None, device=0):
        model = np.ascontiguousarray(model)
        mrows, mcols, ch, _ = _frame_view(model, "model")
        self._ctx = ctx if ctx is not None else _ctx_for(model, None)
        self.width, self.height = int(imSize[0]), int(imSize[1])
        self.channels, self.n = ch, int(numParticles)
        self.model_shape = (mrows, mcols, ch)
        h = C.c_void_p()
        check(lib.micv_pf_create(self._ctx.handle, model.ctypes.data, mrows, mcols, mcols * ch, ch, self.height,
                                 self.width, self.n, int(simMode), float(mseSigma), float(sampleSigma),
                                 float(initModelPos[0]), float(initModelPos[1]), float(alpha), int(flags),
                                 int(seed), C.byref(h)))
        self._h = h

    def _check_frame(self, frame):
        rows, cols, ch, stride = _frame_view(frame)
        if (rows, cols, ch) != (self.height, self.width, self.channels):
            raise ValueError(f"frame is {rows} x {cols} x {ch}, the filter was made for "
                             f"{self.height} x {self.width} x {self.channels}")
        return stride

    def tick(self, frame):
        """One tick -> ((x, y), x_var, y_var) as the reference's tuple; `last_status` holds the status bits.
        A CUDA tensor frame returns the state as a 5-word device tensor instead (nothing synchronised)."""
        stride = self._check_frame(frame)
        if B.is_dev(frame):
            import torch
            st = torch.empty(5, dtype=torch.int32, device=frame.device)
            check(lib.micv_pf_tick_dev(self._h, frame.data_ptr(), stride, B.stream_of(frame), st.data_ptr()))
            return st
        st = np.zeros(1, STATE_DTYPE)
        check(lib.micv_pf_tick_host(self._h, frame.ctypes.data, stride, st.ctypes.data))
        s = st[0]
        self.last_status = int(s["status"])
        return (np.float32(s["x"]), np.float32(s["y"])), np.float32(s["x_var"]), np.float32(s["y_var"])

    @staticmethod
    def state_from_device(st):
        """The 5-word device state of tick(tensor) as a STATE_DTYPE record (synchronises)."""
        return st.cpu().numpy().view(STATE_DTYPE)[0]

    def getParticles(self, out=None):
        """n x 2 f32 particles; `out` a CUDA tensor copies on its current stream instead."""
        if out is not None:
            check(lib.micv_pf_particles_dev(self._h, out.data_ptr(), B.stream_of(out)))
            return out
        p = np.empty((self.n, 2), np.float32)
        check(lib.micv_pf_particles_host(self._h, p.ctypes.data))
        return p

    particles = getParticles

    def weights(self, out=None):
        if out is not None:
            check(lib.micv_pf_weights_dev(self._h, out.data_ptr(), B.stream_of(out)))
            return out
        w = np.empty(self.n, np.float32)
        check(lib.micv_pf_weights_host(self._h, w.ctypes.data))
        return w

    def model(self):
        """(model patch mrows x mcols x C u8, model histogram C x 32 f32)."""
        patch = np.empty(self.model_shape, np.uint8)
        hist = np.empty((self.channels, 32), np.float32)
        check(lib.micv_pf_model_host(self._h, patch.ctypes.data, hist.ctypes.data))
        return patch, hist

    def track(self, frames, with_particles=False):
        """Ticks over a sequence of host frames -> STATE_DTYPE array (and the n x 2 particles after each tick)."""
        frames = [np.asarray(f) for f in frames]
        if not frames:
            raise ValueError("track: no frames")
        strides = {self._check_frame(f) for f in frames}
        if len(strides) != 1:
            raise ValueError("track: every frame needs the same row stride")
        ptrs = (C.c_void_p * len(frames))(*[f.ctypes.data for f in frames])
        states = np.zeros(len(frames), STATE_DTYPE)
        parts = np.empty((len(frames), self.n, 2), np.float32) if with_particles else None
        check(lib.micv_pf_track_seq_host(self._h, ptrs, len(frames), strides.pop(), states.ctypes.data,
                                         parts.ctypes.data if parts is not None else None))
        return (states, parts) if with_particles else states

    def close(self):
        if getattr(self, "_h", None) and lib is not None:
            lib.micv_pf_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()


class FilterGroup:
    """Up to GROUP_MAX `ParticleFilter`s of one device and one frame size ticked together (micv_pf_group): three launches
    for the whole group, and afterwards every member is byte for byte where its own `tick` would have left it, so the
    members' accessors (getParticles, weights, model, ps6.overlayFilter) go on working and group ticks may be mixed
    with single ticks on one stream.  The group borrows the filters and keeps them alive; close the group first."""

    def __init__(self, filters):
        self.filters = list(filters)
        handles = (C.c_void_p * max(len(self.filters), 1))(*[f._h for f in self.filters])
        h = C.c_void_p()
        check(lib.micv_pf_group_create(handles, len(self.filters), C.byref(h)))
        self._h = h

    def __len__(self):
        return len(self.filters)

    def tick(self, frames):
        """One tick of every member -> [K, 5] int32 device tensor (row k: member k's state words; nothing synchronised).
        frames: one CUDA tensor for every member, or a list of K tensors, one each."""
        import torch
        frames = [frames] if B.is_dev(frames) else list(frames)
        if len(frames) not in (1, len(self.filters)):
            raise ValueError(f"tick: {len(frames)} frames for {len(self.filters)} filters, need 1 or {len(self.filters)}")
        if any(not B.is_dev(f) for f in frames):
            raise ValueError("tick: CUDA tensors expected (host frames: track)")
        strides = [self.filters[0]._check_frame(f) for f in frames]
        if len({(f.device, B.stream_of(f)) for f in frames}) != 1:
            raise ValueError("tick: every frame needs the same device and current stream")
        st = torch.empty((len(self.filters), 5), dtype=torch.int32, device=frames[0].device)
        ptrs = (C.c_void_p * len(frames))(*[f.data_ptr() for f in frames])
        check(lib.micv_pf_group_tick_dev(self._h, ptrs, (C.c_size_t * len(frames))(*strides), len(frames),
                                         B.stream_of(frames[0]), st.data_ptr()))
        return st

    @staticmethod
    def states_from_device(st):
        """The [K, 5] device states of tick as a STATE_DTYPE array of K records (synchronises)."""
        return st.cpu().numpy().view(STATE_DTYPE).reshape(-1)

    def _host_frames(self, frames, what):
        frames = [np.asarray(f) for f in frames]
        if not frames:
            raise ValueError(f"{what}: no frames")
        strides = {self.filters[0]._check_frame(f) for f in frames}
        if len(strides) != 1:
            raise ValueError(f"{what}: every frame needs the same row stride")
        return frames, (C.c_void_p * len(frames))(*[f.ctypes.data for f in frames]), strides.pop()

    def track(self, frames, with_particles=False):
        """Ticks of the whole group over one sequence of host frames, every frame uploaded once -> STATE_DTYPE array
        [nframes, K] (and a list of K arrays [nframes, n_k, 2]: each member's particles after each tick)."""
        frames, ptrs, stride = self._host_frames(frames, "track")
        states = np.zeros((len(frames), len(self.filters)), STATE_DTYPE)
        parts = [np.empty((len(frames), f.n, 2), np.float32) for f in self.filters] if with_particles else None
        pp = (C.c_void_p * len(self.filters))(*[p.ctypes.data for p in parts]) if with_particles else None
        check(lib.micv_pf_group_track_seq_host(self._h, ptrs, len(frames), stride, states.ctypes.data, pp))
        return (states, parts) if with_particles else states

    def close(self):
        if getattr(self, "_h", None) and lib is not None:
            lib.micv_pf_group_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()


def track(frames, model, numParticles, simMode, mseSigma, sampleSigma, initModelPos=(-1.0, -1.0), alpha=0.1,
          **kw):
    """A filter made for frames[0]'s size, run over every frame -> STATE_DTYPE array."""
    f0 = np.asarray(frames[0])
    pf = ParticleFilter(model, (f0.shape[1], f0.shape[0]), numParticles, simMode, mseSigma, sampleSigma,
                        initModelPos, alpha, **kw)
    try:
        return pf.track(frames)
    finally:
        pf.close()
