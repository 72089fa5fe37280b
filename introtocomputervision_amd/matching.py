"""`matching::` namespace of the reference's ps7 (ProblemSets/ps7_cpp/include/Matching.h): cv::ml::KNearest
classification and the leave-one-out / leave-one-person-out confusion matrices, on the device (csrc/knn.hip).

Not to be confused with `match.py`, which is ps4's descriptor matching (cv::BFMatcher knnMatch + ratio test).  The
k-NN contract (distance arithmetic, neighbour insertion, vote) is in include/mi_cv.h ("ps7: k-NN and confusion
matrices").  numpy arrays take the host-pointer entry points, CUDA tensors the device ones."""
from ._capi import KNN_F64_ACC, check, lib
from .lk import _ctx_for
from .match import _host_ctx


def _np_rows(a, name):
    import numpy as np
    a = np.asarray(a, dtype=np.float32)
    if a.ndim == 1:
        a = a[:, None]
    if a.ndim != 2:
        raise ValueError(f"{name}: need a 2-D float32 matrix")
    if a.strides[1] != 4 or a.strides[0] <= 0:
        a = np.ascontiguousarray(a)
    return a


def _cuda_rows(t, name):
    import torch
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32):
        raise ValueError(f"{name}: need a float32 CUDA tensor")
    if t.dim() == 1:
        t = t[:, None]
    if t.dim() != 2 or t.stride(1) != 1:
        raise ValueError(f"{name}: need a 2-D float32 CUDA tensor with unit column stride")
    return t


def _cuda_i32(t, n, name):
    import torch
    t = t.reshape(-1)
    if not (t.is_cuda and t.dtype == torch.int32 and t.numel() == n):
        raise ValueError(f"{name}: need {n} int32 values on the device")
    return t.contiguous()


def knnPredict(train, trainLabels, test, k=3, f64Acc=False, ctx=None):
    """KNearest::train(train, ROW_SAMPLE, trainLabels) + findNearest(test, k, results) -> int32 labels [ntest]."""
    import numpy as np
    flags = KNN_F64_ACC if f64Acc else 0
    if isinstance(train, np.ndarray):
        tr, te = _np_rows(train, "train"), _np_rows(test, "test")
        lab = np.ascontiguousarray(np.asarray(trainLabels).reshape(-1), np.int32)
        if tr.shape[1] != te.shape[1] or lab.size != tr.shape[0]:
            raise ValueError("train / test / labels: shapes disagree")
        pred = np.empty(te.shape[0], np.int32)
        check(lib.micv_knn_predict_host((ctx or _host_ctx()).handle, tr.ctypes.data, tr.shape[0], tr.strides[0],
                                        lab.ctypes.data, te.ctypes.data, te.shape[0], te.strides[0], tr.shape[1],
                                        int(k), flags, pred.ctypes.data))
        return pred
    import torch
    tr, te = _cuda_rows(train, "train"), _cuda_rows(test, "test")
    lab = _cuda_i32(trainLabels, tr.shape[0], "trainLabels")
    if tr.shape[1] != te.shape[1]:
        raise ValueError("train / test: widths differ")
    pred = torch.empty(te.shape[0], dtype=torch.int32, device=tr.device)
    check(lib.micv_knn_predict_dev(_ctx_for(tr, ctx).handle, tr.data_ptr(), tr.shape[0], tr.stride(0) * 4,
                                   lab.data_ptr(), te.data_ptr(), te.shape[0], te.stride(0) * 4, tr.shape[1], int(k),
                                   flags, pred.data_ptr(), torch.cuda.current_stream(tr.device).cuda_stream))
    return pred


def _confusion(features, labels, groups, numLabels, numGroups, k, f64Acc, ctx):
    import numpy as np
    flags = KNN_F64_ACC if f64Acc else 0
    nmat = numGroups + 1 if groups is not None else 1
    if isinstance(features, np.ndarray):
        f = _np_rows(features, "features")
        n = f.shape[0]
        lab = np.ascontiguousarray(np.asarray(labels).reshape(-1), np.int32)
        grp = None if groups is None else np.ascontiguousarray(np.asarray(groups).reshape(-1), np.int32)
        if lab.size != n or (grp is not None and grp.size != n):
            raise ValueError("features / labels / groups: row counts differ")
        mats = np.empty((nmat, numLabels, numLabels), np.float32)
        pred = np.empty(n, np.int32)
        left = np.zeros(1, np.int32)
        check(lib.micv_knn_confusion_host((ctx or _host_ctx()).handle, f.ctypes.data, n, f.strides[0], f.shape[1],
                                          lab.ctypes.data, None if grp is None else grp.ctypes.data, int(numLabels),
                                          int(numGroups), int(k), flags, mats.ctypes.data, pred.ctypes.data,
                                          left.ctypes.data))
        return mats, pred, left
    import torch
    f = _cuda_rows(features, "features")
    n = f.shape[0]
    lab = _cuda_i32(labels, n, "labels")
    grp = None if groups is None else _cuda_i32(groups, n, "groups")
    mats = torch.empty((nmat, numLabels, numLabels), dtype=torch.float32, device=f.device)
    pred = torch.empty(n, dtype=torch.int32, device=f.device)
    left = torch.empty(1, dtype=torch.int32, device=f.device)
    check(lib.micv_knn_confusion_dev(_ctx_for(f, ctx).handle, f.data_ptr(), n, f.stride(0) * 4, f.shape[1],
                                     lab.data_ptr(), None if grp is None else grp.data_ptr(), int(numLabels),
                                     int(numGroups), int(k), flags, mats.data_ptr(), pred.data_ptr(), left.data_ptr(),
                                     torch.cuda.current_stream(f.device).cuda_stream))
    return mats, pred, left


def naiveConfusionMatrix(features, labels, numLabels=3, k=3, f64Acc=False, ctx=None):
    """matching::naiveConfusionMatrix (Matching.cpp:33-74): leave-one-out -> (confusion [L, L], pred [n], left_out).
    left_out is a one-element int32 array (numpy in, numpy out; a CUDA tensor for CUDA input, so the device path
    needs no sync): the rows whose label or vote is outside 1..L, left out of the matrix (the reference asserts)."""
    mats, pred, left = _confusion(features, labels, None, numLabels, 0, k, f64Acc, ctx)
    return mats[0], pred, left


def confusionMatrix(features, labels, people, numPeople, numLabels=3, k=3, f64Acc=False, ctx=None):
    """matching::confusionMatrix (Matching.cpp:100-159): leave-one-person-out -> (confusions [numPeople + 1, L, L],
    pred [n], left_out); confusions[numPeople] is the average, as the reference appends it."""
    return _confusion(features, labels, people, numLabels, int(numPeople), k, f64Acc, ctx)
