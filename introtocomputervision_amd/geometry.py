"""ps3 of the reference on the HIP kernels of csrc/geom.hip: `calib` (ps3_cpp/include/Calibration.h) and `fundamental`
(include/Fundamental.h) plus the driver's trial loop, epipolar end points and camera centre (src/Solution.cpp).

Points are 2 x n / 3 x n float32 as in the reference's cv::Mats; the C ABI (include/mi_cv.h, "ps3: geometry") takes
them as rows, [n][2] / [n][3], so this layer transposes.  numpy arrays take the `_host` entry points, CUDA tensors the
`_dev` ones and come back as CUDA tensors.  f64=True selects MICV_GEOM_F64: the same operations in double."""
import ctypes as C

import numpy as np

from . import _buf as B
from ._capi import GEOM_F64, check, lib
from .lk import _ctx_for
from .ransac import Generator


def _rows(p, dims, name):
    """dims x n (numpy or CUDA tensor) -> contiguous [n, dims] float32 of the same kind."""
    if B.is_dev(p):
        import torch
        if not (p.is_cuda and p.dtype == torch.float32 and p.dim() == 2 and p.shape[0] == dims):
            raise ValueError(f"{name}: need a {dims} x n float32 CUDA tensor")
        return p.t().contiguous()
    p = np.asarray(p)
    if p.ndim != 2 or p.shape[0] != dims:
        raise ValueError(f"{name}: need a {dims} x n array")
    return np.ascontiguousarray(p.T, np.float32)


def _handle(ref, ctx):
    if B.is_dev(ref):
        return _ctx_for(ref, ctx).handle
    from .match import _host_ctx
    return (ctx or _host_ctx()).handle


def _out(ref, shape, dtype=np.float32):
    return B.zeros_like_shape(ref, shape, dtype)


def _raise_bad(status):
    if int(status.cpu()[0]):
        raise ValueError("an index outside the point set")


def _solve(fn, a, b, indices, k, per, f64, ctx):
    """The shared shape of micv_calib_svd_* and micv_fundamental_ls_*."""
    n = int(a.shape[0])
    flags = GEOM_F64 if f64 else 0
    if indices is None:
        T, stride, ip = 1, 0, None
    else:
        T, stride = int(indices.shape[0]), int(indices.shape[1])
    out = _out(a, (T, per))
    if B.is_dev(a):
        import torch
        if indices is not None:
            indices = indices.to(device=a.device, dtype=torch.int32).contiguous()
            ip = indices.data_ptr()
        st = torch.zeros(1, dtype=torch.int32, device=a.device)
        check(getattr(lib, fn + "_dev")(_handle(a, ctx), a.data_ptr(), b.data_ptr(), n, ip, stride, k, T, flags,
                                        out.data_ptr(), st.data_ptr(), B.stream_of(a)))
        _raise_bad(st)
    else:
        if indices is not None:
            indices = np.ascontiguousarray(indices, np.int32)
            ip = indices.ctypes.data
        check(getattr(lib, fn + "_host")(_handle(a, ctx), a.ctypes.data, b.ctypes.data, n, ip, stride, k, T, flags,
                                         out.ctypes.data))
    return out


class TrialResult(tuple):
    """(residuals [iters, len(sizes)] float64 in the log's layout, best M [3, 4], its constraint size, the camera
    centre [3]) plus M [T, 3, 4], residual [T], indices, kcount and the arg-min records best_idx / best_res / best_M
    (one per size, then overall)."""

    def __new__(cls, residuals, M, size, center, **extra):
        r = super().__new__(cls, (residuals, M, size, center))
        r.__dict__.update(extra)
        return r


class calib:
    @staticmethod
    def solveLeastSquares(pts2d, pts3d, f64=False, ctx=None):
        """calib::solveLeastSquares -> the 12 x 1 solution (the last entry is the appended 1)."""
        p2, p3 = _rows(pts2d, 2, "pts2d"), _rows(pts3d, 3, "pts3d")
        n = int(p2.shape[0])
        if int(p3.shape[0]) != n:
            raise ValueError("pts2d and pts3d differ in their number of points")
        M, _, _ = calib._trials(p2, p3, None, n, 0, None, None, f64, ctx, best=False)
        return M.reshape(12, 1)

    @staticmethod
    def solveSVD(pts2d, pts3d, f64=False, ctx=None):
        """calib::solveSVD -> the 12 x 1 unit vector (sign as it falls)."""
        p2, p3 = _rows(pts2d, 2, "pts2d"), _rows(pts3d, 3, "pts3d")
        if int(p3.shape[0]) != int(p2.shape[0]):
            raise ValueError("pts2d and pts3d differ in their number of points")
        return _solve("micv_calib_svd", p2, p3, None, int(p2.shape[0]), 12, f64, ctx).reshape(12, 1)

    @staticmethod
    def solveSVDBatch(pts2d, pts3d, indices, f64=False, ctx=None):
        """calib::solveSVD of each index subset (indices [T, k]) -> [T, 12]."""
        p2, p3 = _rows(pts2d, 2, "pts2d"), _rows(pts3d, 3, "pts3d")
        return _solve("micv_calib_svd", p2, p3, indices, int(indices.shape[1]), 12, f64, ctx)

    @staticmethod
    def _trials(p2, p3, indices, k, j, kcount, group_sizes, f64, ctx, best=True):
        """micv_calib_ls_trials_* on row-layout points -> M [T, 12], residual [T], (best_idx, best_res, best_M)."""
        n = int(p2.shape[0])
        flags = GEOM_F64 if f64 else 0
        T = 1 if indices is None else int(indices.shape[0])
        stride = 0 if indices is None else int(indices.shape[1])
        G = len(group_sizes) if group_sizes is not None else 0
        gs = (C.c_int * G)(*[int(g) for g in group_sizes]) if G else None
        M, res = _out(p2, (T, 12)), _out(p2, (T,), np.float64)
        bi, br, bm = _out(p2, (G + 1,), np.int32), _out(p2, (G + 1,), np.float64), _out(p2, (G + 1, 12))
        dev = B.is_dev(p2)
        if dev:
            import torch
            conv = lambda a: None if a is None else a.to(device=p2.device, dtype=torch.int32).contiguous() \
                if B.is_dev(a) else torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(p2.device)
        else:
            conv = lambda a: None if a is None else np.ascontiguousarray(a, np.int32)
        indices, kcount = conv(indices), conv(kcount)
        ptr = lambda a: None if a is None else B.ptr(a)
        bp = (ptr(bi), ptr(br), ptr(bm)) if best else (None, None, None)
        if dev:
            st = torch.zeros(1, dtype=torch.int32, device=p2.device)
            check(lib.micv_calib_ls_trials_dev(_handle(p2, ctx), p2.data_ptr(), p3.data_ptr(), n, ptr(indices), stride,
                                               k, j, T, ptr(kcount), gs, G, flags, M.data_ptr(), res.data_ptr(), *bp,
                                               st.data_ptr(), B.stream_of(p2)))
            _raise_bad(st)
        else:
            check(lib.micv_calib_ls_trials_host(_handle(p2, ctx), p2.ctypes.data, p3.ctypes.data, n, ptr(indices),
                                                stride, k, j, T, ptr(kcount), gs, G, flags, M.ctypes.data,
                                                res.ctypes.data, *bp))
        return M, res, ((bi, br, bm) if best else None)

    @staticmethod
    def trialsBatch(pts2d, pts3d, indices, k, tests, kcount=None, group_sizes=None, f64=False, ctx=None):
        """Any number of trials in one launch: indices [T, >= k + tests] -> M [T, 12], residual [T] and the arg-min
        records (best_idx, best_res, best_M), one per group and one overall."""
        p2, p3 = _rows(pts2d, 2, "pts2d"), _rows(pts3d, 3, "pts3d")
        return calib._trials(p2, p3, indices, int(k), int(tests), kcount, group_sizes, f64, ctx)

    @staticmethod
    def trials(pts2d, pts3d, sizes=(8, 12, 16), iters=10, tests=4, seed=None, f64=False, gen=None, ctx=None):
        """The trial loop of the reference's problem 1b/1c (Solution.cpp:243-326) as one launch: for each constraint
        set size, `iters` trials on the first `size` entries of a fresh shuffle with the next `tests` entries as test
        points.  `seed`: the config's mersenne_seed words (None: a default-constructed engine), or pass a
        ransac.Generator as `gen`.  Returns a TrialResult."""
        p2, p3 = _rows(pts2d, 2, "pts2d"), _rows(pts3d, 3, "pts3d")
        n = int(p2.shape[0])
        sizes = [int(s) for s in sizes]
        kmax, T = max(sizes), len(sizes) * int(iters)
        if kmax + tests > n:
            raise ValueError(f"{kmax} constraints + {tests} test points from {n} points")
        g = gen or Generator(seed)
        perms = np.empty((T, n), np.int32)
        check(lib.micv_geom_trial_indices(g._h, n, T, perms.ctypes.data))
        idx = np.zeros((T, kmax + tests), np.int32)
        kc = np.repeat(np.asarray(sizes, np.int32), iters)
        for t in range(T):
            idx[t, :kc[t] + tests] = perms[t, :kc[t] + tests]
        M, res, (bi, br, bm) = calib._trials(p2, p3, idx, kmax, int(tests), kc, [iters] * len(sizes), f64, ctx)
        center = cameraCenter(bm[-1:], f64=f64, ctx=ctx)[0]
        win = int(bi[-1])
        return TrialResult(res.reshape(len(sizes), iters).T, bm[-1].reshape(3, 4), sizes[win // iters] if win >= 0 else None,
                           center, M_all=M.reshape(T, 3, 4), residual=res, indices=idx, kcount=kc, best_idx=bi,
                           best_res=br, best_M=bm)


class fundamental:
    @staticmethod
    def solveLeastSquares(pts2dA, pts2dB, f64=False, ctx=None):
        """fundamental::solveLeastSquares -> the 9 x 1 solution (reshape to 3 x 3 as the driver does)."""
        a, b = _rows(pts2dA, 2, "pts2dA"), _rows(pts2dB, 2, "pts2dB")
        if int(a.shape[0]) != int(b.shape[0]):
            raise ValueError("pts2dA and pts2dB differ in their number of points")
        return _solve("micv_fundamental_ls", a, b, None, int(a.shape[0]), 9, f64, ctx).reshape(9, 1)

    @staticmethod
    def solveLeastSquaresBatch(pts2dA, pts2dB, indices, f64=False, ctx=None):
        a, b = _rows(pts2dA, 2, "pts2dA"), _rows(pts2dB, 2, "pts2dB")
        return _solve("micv_fundamental_ls", a, b, indices, int(indices.shape[1]), 9, f64, ctx)

    @staticmethod
    def rankReduce(fMat, f64=False, ctx=None):
        """fundamental::rankReduce of a 3 x 3 matrix (or a batch [T, 3, 3])."""
        dev = B.is_dev(fMat)
        F = fMat.contiguous() if dev else np.ascontiguousarray(fMat, np.float32)
        if tuple(F.shape[-2:]) != (3, 3):
            raise ValueError("fMat: need 3 x 3")
        T = int(F.numel() if dev else F.size) // 9
        out = _out(F, tuple(F.shape))
        flags = GEOM_F64 if f64 else 0
        if dev:
            check(lib.micv_fundamental_rank_reduce_dev(_handle(F, ctx), F.data_ptr(), T, flags, out.data_ptr(),
                                                       B.stream_of(F)))
        else:
            check(lib.micv_fundamental_rank_reduce_host(_handle(F, ctx), F.ctypes.data, T, flags, out.ctypes.data))
        return out

    @staticmethod
    def normalized(pts2dA, pts2dB, f64=False, ctx=None):
        """The extra-credit chain (Solution.cpp:381-445) -> T_a, T_b, F_Hat, F (3 x 3 each)."""
        a, b = _rows(pts2dA, 2, "pts2dA"), _rows(pts2dB, 2, "pts2dB")
        n = int(a.shape[0])
        if int(b.shape[0]) != n:
            raise ValueError("pts2dA and pts2dB differ in their number of points")
        out = _out(a, (4, 3, 3))
        flags = GEOM_F64 if f64 else 0
        if B.is_dev(a):
            check(lib.micv_fundamental_normalized_dev(_handle(a, ctx), a.data_ptr(), b.data_ptr(), n, flags,
                                                      *[out[i].data_ptr() for i in range(4)], B.stream_of(a)))
        else:
            check(lib.micv_fundamental_normalized_host(_handle(a, ctx), a.ctypes.data, b.ctypes.data, n, flags,
                                                       *[out[i].ctypes.data for i in range(4)]))
        return out[0], out[1], out[2], out[3]

    @staticmethod
    def epipolarEndpoints(fMat, pts2d, side, rows, cols, f64=False, ctx=None):
        """The end points of the epipolar lines the driver draws: side 0 takes the points of image B and gives the
        lines in image A ((p^T F)^T), side 1 the points of image A and the lines in image B (F p), on a rows x cols
        image.  -> [n, 6] = P_iL, P_iR."""
        p = _rows(pts2d, 2, "pts2d")
        dev = B.is_dev(p)
        if dev:
            F = fMat.to(p.device).contiguous() if B.is_dev(fMat) else None
            if F is None:
                import torch
                F = torch.from_numpy(np.ascontiguousarray(fMat, np.float32)).to(p.device)
        else:
            F = np.ascontiguousarray(fMat, np.float32)
        n = int(p.shape[0])
        out = _out(p, (n, 6))
        flags = GEOM_F64 if f64 else 0
        if dev:
            check(lib.micv_epipolar_endpoints_dev(_handle(p, ctx), F.data_ptr(), p.data_ptr(), n, int(side), int(rows),
                                                  int(cols), flags, out.data_ptr(), B.stream_of(p)))
        else:
            check(lib.micv_epipolar_endpoints_host(_handle(p, ctx), F.ctypes.data, p.ctypes.data, n, int(side),
                                                   int(rows), int(cols), flags, out.ctypes.data))
        return out


def cameraCenter(M, f64=False, ctx=None):
    """-Q^-1 m4 of each 3 x 4 projection matrix (M [T, 12] or [T, 3, 4]) -> [T, 3]."""
    dev = B.is_dev(M)
    Mc = M.contiguous() if dev else np.ascontiguousarray(M, np.float32)
    T = int(Mc.numel() if dev else Mc.size) // 12
    out = _out(Mc, (T, 3))
    flags = GEOM_F64 if f64 else 0
    if dev:
        check(lib.micv_camera_center_dev(_handle(Mc, ctx), Mc.data_ptr(), T, flags, out.data_ptr(), B.stream_of(Mc)))
    else:
        check(lib.micv_camera_center_host(_handle(Mc, ctx), Mc.ctypes.data, T, flags, out.ctypes.data))
    return out


def trialIndices(gen, n, trials):
    """genUniqueRands' permutations on a ransac.Generator: [trials, n] int32; the engine advances."""
    out = np.empty((trials, n), np.int32)
    check(lib.micv_geom_trial_indices(gen._h, n, trials, out.ctypes.data))
    return out


def sampleIndices(seed, n, count, T, device="cuda", ctx=None):
    """The counter-based device sampler (not the reference's sequence): [T, count] int32 CUDA tensor."""
    import torch
    out = torch.empty((T, count), dtype=torch.int32, device=device)
    check(lib.micv_geom_sample_indices_dev(_handle(out, ctx), int(seed) & ((1 << 64) - 1), int(n), int(count), int(T),
                                           out.data_ptr(), B.stream_of(out)))
    return out
