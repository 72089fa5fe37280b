"""`moments::` namespace of the reference's ps7 (ProblemSets/ps7_cpp/include/Moments.h): central moments mu and
scale-invariant moments eta of single-channel images, on the device (csrc/moments.hip).  The arithmetic contract,
including the reference's as-written `x - yBar` and the optional fix, is in include/mi_cv.h ("ps7: central moments").

numpy arrays take the host-pointer entry point, CUDA tensors the device one (stream-ordered, no host sync)."""
from ._capi import MOMENTS_F32, MOMENTS_NORM_INF, MOMENTS_U8, MOMENTS_Y_FIXED, check, lib
from .lk import _ctx_for
from .match import _host_ctx

PS7_ORDERS = ((2, 0), (0, 2), (1, 2), (2, 1), (2, 2), (3, 0), (0, 3))  # Solution.cpp:248-249


def _flags(normInf, yFixed):
    return (MOMENTS_NORM_INF if normInf else 0) | (MOMENTS_Y_FIXED if yFixed else 0)


def _orders(orders):
    import numpy as np
    o = np.ascontiguousarray(np.asarray(orders, dtype=np.int32).reshape(-1, 2))
    if o.shape[0] == 0:
        raise ValueError("orders: need at least one (p, q)")
    return o


def centralMomentsBatch(imgs, orders=PS7_ORDERS, normInf=False, yFixed=False, ctx=None):
    """Moments of a batch: imgs is [B, rows, cols] uint8 or float32 (numpy, or a CUDA tensor whose rows have unit
    column stride).  Returns (mu [B, n], eta [B, n], raw [B, 3] = M00, M10, M01), all float32.
    normInf applies the driver's cv::normalize(.., 1.0, 0.0, NORM_INF, CV_32FC1) first (uint8 only)."""
    import numpy as np
    o = _orders(orders)
    n = o.shape[0]
    flags = _flags(normInf, yFixed)
    if isinstance(imgs, np.ndarray):
        a = imgs if imgs.ndim == 3 else imgs[None]
        if a.dtype not in (np.uint8, np.float32):
            raise ValueError("imgs: need uint8 or float32")
        if a.strides[2] != a.itemsize or a.strides[0] < 0 or a.strides[1] < 0:
            a = np.ascontiguousarray(a)
        typ = MOMENTS_F32 if a.dtype == np.float32 else MOMENTS_U8
        B, rows, cols = a.shape
        mu = np.empty((B, n), np.float32)
        eta = np.empty((B, n), np.float32)
        raw = np.empty((B, 3), np.float32)
        check(lib.micv_central_moments_host((ctx or _host_ctx()).handle, a.ctypes.data, B, a.strides[0], a.strides[1],
                                            rows, cols, typ, o.ctypes.data, n, flags, mu.ctypes.data, eta.ctypes.data,
                                            raw.ctypes.data))
        return mu, eta, raw
    import torch
    t = imgs if imgs.dim() == 3 else imgs.unsqueeze(0)
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype in (torch.uint8, torch.float32)
            and t.stride(2) == 1):
        raise ValueError("imgs: need a [B, rows, cols] uint8 / float32 CUDA tensor with unit column stride")
    typ = MOMENTS_F32 if t.dtype == torch.float32 else MOMENTS_U8
    B, rows, cols = t.shape
    es = t.element_size()
    mu, eta, raw = (torch.empty((B, n), dtype=torch.float32, device=t.device),
                    torch.empty((B, n), dtype=torch.float32, device=t.device),
                    torch.empty((B, 3), dtype=torch.float32, device=t.device))
    check(lib.micv_central_moments_dev(_ctx_for(t, ctx).handle, t.data_ptr(), B, t.stride(0) * es, t.stride(1) * es,
                                       rows, cols, typ, o.ctypes.data, n, flags, mu.data_ptr(), eta.data_ptr(),
                                       raw.data_ptr(), torch.cuda.current_stream(t.device).cuda_stream))
    return mu, eta, raw


def centralMoment(img, momentOrders=PS7_ORDERS, normInf=False, yFixed=False, ctx=None):
    """moments::centralMoment(img, momentOrders) (Moments.cpp:7-67) -> [(mu, eta), ...] as Python floats, one pair per
    order, like the reference's vector<pair<float, float>>."""
    mu, eta, _ = centralMomentsBatch(img, momentOrders, normInf, yFixed, ctx)
    mu = mu[0].tolist() if hasattr(mu, "tolist") else mu[0]
    eta = eta[0].tolist() if hasattr(eta, "tolist") else eta[0]
    return list(zip(mu, eta))
