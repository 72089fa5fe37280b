"""ps7 k-NN and confusion matrices on the device (csrc/knn.hip) against the exact restatement tests/_ps7_ref.py, bit
for bit: predictions, leave-one-out and leave-one-group-out matrices, ties, non-finite features, both accumulators."""
import numpy as np
import pytest

import _ps7_ref as ref

pytestmark = pytest.mark.gpu


def _m():
    from introtocomputervision_amd import matching
    return matching


def clusters(rng, n, d, L=3, spread=1.0):
    centres = rng.standard_normal((L, d)).astype(np.float32) * np.float32(3)
    lab = rng.integers(1, L + 1, n).astype(np.int32)
    f = centres[lab - 1] + rng.standard_normal((n, d)).astype(np.float32) * np.float32(spread)
    return f.astype(np.float32), lab


@pytest.mark.parametrize("d", [1, 3, 4, 7, 14, 64])
@pytest.mark.parametrize("k", [1, 3, 32])
@pytest.mark.parametrize("f64", [False, True])
def test_predict(d, k, f64):
    import torch
    rng = np.random.default_rng([d, k, int(f64)])
    tr, lab = clusters(rng, 500, d, L=5, spread=2.0)
    te, _ = clusters(rng, 300, d, L=5, spread=2.0)
    want = ref.knn_predict(tr, lab, te, k, f64)
    got = _m().knnPredict(tr, lab, te, k, f64)
    assert np.array_equal(got, want)
    gd = _m().knnPredict(torch.from_numpy(tr).cuda(), torch.from_numpy(lab).cuda(), torch.from_numpy(te).cuda(), k, f64)
    torch.cuda.synchronize()
    assert np.array_equal(gd.cpu().numpy(), want)


@pytest.mark.parametrize("n", [3, 27, 200])
@pytest.mark.parametrize("f64", [False, True])
def test_naive_confusion(n, f64):
    rng = np.random.default_rng([n, int(f64)])
    f, lab = clusters(rng, n, 7)
    emat, epred, eleft = ref.naive_confusion(f, lab, 3, 3, f64)
    mat, pred, left = _m().naiveConfusionMatrix(f, lab, 3, 3, f64)
    assert np.array_equal(pred, epred) and int(left[0]) == eleft
    assert np.array_equal(mat.view(np.uint32), emat.view(np.uint32))


def test_group_confusion_dev_and_host():
    import torch
    rng = np.random.default_rng(4)
    f, lab = clusters(rng, 27, 7)
    grp = np.tile(np.repeat(np.arange(1, 4, dtype=np.int32), 3), 3)
    emats, epred, eleft = ref.group_confusion(f, lab, grp, 3)
    mats, pred, left = _m().confusionMatrix(f, lab, grp, 3)
    assert np.array_equal(mats.view(np.uint32), emats.view(np.uint32)) and np.array_equal(pred, epred)
    dm, dp, dl = _m().confusionMatrix(torch.from_numpy(f).cuda(), torch.from_numpy(lab).cuda(),
                                      torch.from_numpy(grp).cuda(), 3)
    torch.cuda.synchronize()
    assert np.array_equal(dm.cpu().numpy().view(np.uint32), emats.view(np.uint32))
    assert np.array_equal(dp.cpu().numpy(), epred) and int(dl.cpu()[0]) == eleft == int(left[0])


def test_empty_group_and_labels_outside():
    rng = np.random.default_rng(8)
    f, lab = clusters(rng, 60, 5)
    grp = rng.integers(1, 4, 60).astype(np.int32)  # group 4 of 4 is empty
    grp[:3] = 9  # in no fold
    lab[10:14] = 7  # outside 1..L: left out when tested, and they vote 7 for their neighbours
    emats, epred, eleft = ref.group_confusion(f, lab, grp, 4)
    mats, pred, left = _m().confusionMatrix(f, lab, grp, 4)
    assert eleft > 0 and int(left[0]) == eleft
    assert np.array_equal(pred, epred) and np.array_equal(mats.view(np.uint32), emats.view(np.uint32))


def test_ties_and_nonfinite():
    f = np.array([[0.0], [1.0], [-1.0], [1.0], [2.0], [-2.0], [np.inf], [np.nan], [3.0]], np.float32)
    lab = np.array([1, 2, 3, 1, 2, 3, 1, 2, 3], np.int32)
    for k in (1, 3, 5):
        emat, epred, eleft = ref.naive_confusion(f, lab, 3, k)
        mat, pred, left = _m().naiveConfusionMatrix(f, lab, 3, k)
        assert np.array_equal(pred, epred) and int(left[0]) == eleft, (k, pred, epred)
        assert np.array_equal(mat.view(np.uint32), emat.view(np.uint32))


def test_large_leave_one_out():
    rng = np.random.default_rng(20000)
    f, lab = clusters(rng, 20000, 7, spread=2.5)
    emat, epred, eleft = ref.naive_confusion(f, lab, 3, 3)
    mat, pred, left = _m().naiveConfusionMatrix(f, lab, 3, 3)
    assert np.array_equal(pred, epred)
    assert np.array_equal(mat.view(np.uint32), emat.view(np.uint32))


def test_einval():
    import torch
    from introtocomputervision_amd._capi import EINVAL, Context, lib
    ctx = Context(0)
    f = torch.zeros((10, 4), dtype=torch.float32, device="cuda")
    lab = torch.ones(10, dtype=torch.int32, device="cuda")
    out = torch.empty(1000, dtype=torch.float32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream

    def conf(n=10, stride=16, dims=4, L=3, G=3, k=3, flags=0, groups=None, feats=f.data_ptr()):
        return lib.micv_knn_confusion_dev(ctx.handle, feats, n, stride, dims, lab.data_ptr(), groups, L, G, k, flags,
                                          out.data_ptr(), None, None, s)
    assert conf() == 0
    for kw in [dict(n=1), dict(dims=0), dict(dims=65, stride=260), dict(stride=15), dict(L=0), dict(L=17), dict(k=0),
               dict(k=33), dict(flags=2), dict(groups=lab.data_ptr(), G=0), dict(groups=lab.data_ptr(), G=33),
               dict(feats=None)]:
        assert conf(**kw) == EINVAL, kw

    def pred(ntrain=10, ntest=10, dims=4, k=3, flags=0):
        return lib.micv_knn_predict_dev(ctx.handle, f.data_ptr(), ntrain, 16, lab.data_ptr(), f.data_ptr(), ntest, 16,
                                        dims, k, flags, lab.data_ptr(), s)
    for kw in [dict(ntrain=0), dict(ntest=0), dict(dims=65), dict(k=33), dict(flags=8)]:
        assert pred(**kw) == EINVAL, kw
    torch.cuda.synchronize()
