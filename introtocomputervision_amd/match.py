"""Descriptor matching of the reference's ps4 driver (ProblemSets/ps4_cpp/src/Solution.cpp:172-184):
cv::BFMatcher::create()->knnMatch(d1, d2, raw, 2) followed by the 0.75 ratio test."""
from ._capi import check, lib
from .lk import _ctx_for

_HOST_CTX = []


def _host_ctx():
    if not _HOST_CTX:
        from ._capi import Context
        _HOST_CTX.append(Context(0))
    return _HOST_CTX[0]


def knnMatch2(query, train, ctx=None):
    """2 nearest train descriptors (L2) per query row -> (idx [nq, 2] int32, dist [nq, 2] float32).
    numpy arrays take the host-pointer entry point (upload, kernel, download), CUDA tensors the
    device one."""
    import numpy as np
    if isinstance(query, np.ndarray):
        from ._capi import Context
        q = np.ascontiguousarray(query, np.float32)
        t = np.ascontiguousarray(train, np.float32)
        if q.ndim != 2 or t.ndim != 2 or q.shape[1] != t.shape[1]:
            raise ValueError("query / train: need 2-D float32 arrays of equal width")
        idx = np.empty((q.shape[0], 2), np.int32)
        dist = np.empty((q.shape[0], 2), np.float32)
        c = ctx or _host_ctx()
        check(lib.micv_bf_knn2_host(c.handle, q.ctypes.data, q.shape[0], q.strides[0], t.ctypes.data,
                                    t.shape[0], t.strides[0], q.shape[1], idx.ctypes.data, dist.ctypes.data))
        return idx, dist
    import torch
    for t, n in ((query, "query"), (train, "train")):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dim() == 2 and t.dtype == torch.float32
                and t.stride(1) == 1):
            raise ValueError(f"{n}: need a 2-D float32 CUDA tensor with unit column stride")
    if query.shape[1] != train.shape[1]:
        raise ValueError("descriptor dimensions differ")
    nq, dim = query.shape
    idx = torch.empty((nq, 2), dtype=torch.int32, device=query.device)
    dist = torch.empty((nq, 2), dtype=torch.float32, device=query.device)
    check(lib.micv_bf_knn2_dev(_ctx_for(query, ctx).handle, query.data_ptr(), nq, query.stride(0) * 4,
                               train.data_ptr(), train.shape[0], train.stride(0) * 4, dim,
                               idx.data_ptr(), dist.data_ptr(),
                               torch.cuda.current_stream(query.device).cuda_stream))
    return idx, dist


def knnMatch2Counted(query, train, query_count, train_count, ctx=None):
    """knnMatch2 on CUDA tensors whose lengths are device words (micv_bf_knn2_counted_dev): query [nq_cap, dim] and train
    [nt_cap, dim] float32, query_count / train_count 1-element int64 CUDA tensors, clamped to [0, cap] on the device.
    -> (idx [nq_cap, 2], dist [nq_cap, 2]): rows below the query count as knnMatch2(query[:nq], train[:nt]), the rows
    past it {-1, -1} / {+inf, +inf}, which ratioTest never keeps.  Nothing is read back."""
    import torch
    for t, n in ((query, "query"), (train, "train")):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dim() == 2 and t.dtype == torch.float32
                and t.stride(1) == 1):
            raise ValueError(f"{n}: need a 2-D float32 CUDA tensor with unit column stride")
    if query.shape[1] != train.shape[1]:
        raise ValueError("descriptor dimensions differ")
    for t, n in ((query_count, "query_count"), (train_count, "train_count")):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int64 and t.numel() == 1 and t.device == query.device):
            raise ValueError(f"{n}: need a 1-element int64 CUDA tensor on query's device")
    nq, dim = query.shape
    idx = torch.empty((nq, 2), dtype=torch.int32, device=query.device)
    dist = torch.empty((nq, 2), dtype=torch.float32, device=query.device)
    check(lib.micv_bf_knn2_counted_dev(_ctx_for(query, ctx).handle, query.data_ptr(), nq, query.stride(0) * 4, query_count.data_ptr(),
                                       train.data_ptr(), train.shape[0], train.stride(0) * 4, train_count.data_ptr(), dim,
                                       idx.data_ptr(), dist.data_ptr(), torch.cuda.current_stream(query.device).cuda_stream))
    return idx, dist


def ratioTest(idx, dist, ratio=0.75, ctx=None):
    """Good matches: (matches [n, 2] int32 = (queryIdx, trainIdx), distances [n]) in query order."""
    import numpy as np
    if isinstance(idx, np.ndarray):
        import ctypes as C
        idx = np.ascontiguousarray(idx, np.int32)
        dist = np.ascontiguousarray(dist, np.float32)
        nq = idx.shape[0]
        matches = np.empty((nq, 2), np.int32)
        distances = np.empty((nq,), np.float32)
        cnt = C.c_int64(0)
        c = ctx or _host_ctx()
        check(lib.micv_bf_ratio_filter_host(c.handle, idx.ctypes.data, dist.ctypes.data, nq, float(ratio),
                                            matches.ctypes.data, distances.ctypes.data, nq, C.byref(cnt)))
        return matches[:cnt.value], distances[:cnt.value]
    import torch
    nq = idx.shape[0]
    matches = torch.empty((nq, 2), dtype=torch.int32, device=idx.device)
    distances = torch.empty((nq,), dtype=torch.float32, device=idx.device)
    cnt = torch.zeros((1,), dtype=torch.int64, device=idx.device)
    check(lib.micv_bf_ratio_filter_dev(_ctx_for(idx, ctx).handle, idx.data_ptr(), dist.data_ptr(), nq,
                                       float(ratio), matches.data_ptr(), distances.data_ptr(), nq,
                                       cnt.data_ptr(), torch.cuda.current_stream(idx.device).cuda_stream))
    n = int(cnt.item())
    return matches[:n], distances[:n]


def pairList(pairs, images, device):
    """The (query image, train image) list of matchPairs / ransac.solve_pairs as an [npairs, 2] int32 CUDA tensor.  A Python
    list is range-checked here (ValueError); a CUDA tensor goes through as it is -- the kernels treat an index outside
    [0, images) as two empty lists."""
    import torch
    if isinstance(pairs, torch.Tensor):
        if not (pairs.is_cuda and pairs.dtype == torch.int32 and pairs.dim() == 2 and pairs.shape[1] == 2 and pairs.is_contiguous()
                and pairs.device == device):
            raise ValueError("pairs: need a contiguous [npairs, 2] int32 CUDA tensor on the data's device")
        t = pairs
    else:
        rows = [(int(a), int(b)) for a, b in pairs]
        for a, b in rows:
            if not (0 <= a < images and 0 <= b < images):
                raise ValueError(f"pairs: ({a}, {b}) names an image outside 0 .. {images - 1}")
        t = torch.tensor(rows, dtype=torch.int32).reshape(-1, 2).to(device)
    if not 1 <= t.shape[0] <= 65535:
        raise ValueError("pairs: need 1 .. 65535 pairs")
    return t


def matchPairs(desc, count, pairs, ratio=0.75, capacity=None, want_knn=False, ctx=None):
    """knnMatch2Counted + the ratio test on a batch of pairs in two launches (micv_bf_match_pairs_dev).  desc [images, cap,
    dim] float32 CUDA (any image and row stride), count [images] int64 CUDA or None (every row), pairs a list of (query
    image, train image) or an [npairs, 2] int32 CUDA tensor (pairList).  -> (matches [npairs, capacity, 2] int32, distances
    [npairs, capacity], match_count [npairs] int64), with want_knn also (idx [npairs, cap, 2], dist [npairs, cap, 2]).
    Element p holds the bytes of the two single calls on pair p; match_count[p] is the total kept and may exceed
    `capacity` (default cap); rows at and past min(match_count[p], capacity) are not written.  Nothing is read back."""
    import torch
    if not (isinstance(desc, torch.Tensor) and desc.is_cuda and desc.dim() == 3 and desc.dtype == torch.float32 and desc.stride(2) == 1):
        raise ValueError("desc: need an [images, cap, dim] float32 CUDA tensor with unit column stride")
    images, cap, dim = desc.shape
    if images < 1 or cap < 1 or dim < 1:
        raise ValueError("desc: empty")
    if count is not None and not (isinstance(count, torch.Tensor) and count.is_cuda and count.dtype == torch.int64 and count.dim() == 1
                                  and count.shape[0] == images and count.is_contiguous() and count.device == desc.device):
        raise ValueError("count: need a contiguous [images] int64 CUDA tensor on desc's device")
    pt = pairList(pairs, images, desc.device)
    npairs = int(pt.shape[0])
    mcap = cap if capacity is None else int(capacity)
    dv = desc.device
    matches = torch.empty((npairs, mcap, 2), dtype=torch.int32, device=dv)
    distances = torch.empty((npairs, mcap), dtype=torch.float32, device=dv)
    mcount = torch.empty((npairs,), dtype=torch.int64, device=dv)
    idx = torch.empty((npairs, cap, 2), dtype=torch.int32, device=dv) if want_knn else None
    dist = torch.empty((npairs, cap, 2), dtype=torch.float32, device=dv) if want_knn else None
    check(lib.micv_bf_match_pairs_dev(_ctx_for(desc, ctx).handle, desc.data_ptr(), images, (desc.stride(0) if images > 1 else cap * desc.stride(1)) * 4,
                                      cap, (desc.stride(1) if cap > 1 else dim) * 4, count.data_ptr() if count is not None else None, dim,
                                      pt.data_ptr(), npairs, float(ratio), idx.data_ptr() if want_knn else None,
                                      dist.data_ptr() if want_knn else None, matches.data_ptr() if mcap else None,
                                      distances.data_ptr() if mcap else None, mcap, mcount.data_ptr(),
                                      torch.cuda.current_stream(dv).cuda_stream))
    return (matches, distances, mcount, idx, dist) if want_knn else (matches, distances, mcount)
