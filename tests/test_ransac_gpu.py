"""micv_ransac_solve_{dev,host,matches_dev} against the exact restatement (tests/_ransac_ref.py), bit for
bit: both transforms, the inlier mask, iterations, best iteration and count.  Reference sampling
(the library's generator, pinned by tests/test_ransac_ref.py) and the device sampler both run."""
import ctypes as C

import numpy as np
import pytest

import _ransac_pin as pin
import _ransac_ref as rr

pytestmark = pytest.mark.gpu

LDS_MAX = 4096  # matches staged in LDS per workgroup (csrc/ransac.hip)


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def lib():
    from introtocomputervision_amd._capi import lib as L
    return L


def ctx():
    from introtocomputervision_amd.match import _host_ctx
    return _host_ctx()


def run_host(src, dst, samples, tt, th, iters, mr):
    from introtocomputervision_amd._capi import check
    n = len(src)
    tr = np.zeros((2, 2, 3), np.float32)
    mask = np.zeros(n, np.uint8)
    st = np.zeros(3, np.int32)
    s = np.ascontiguousarray(samples, np.int32)
    check(lib().micv_ransac_solve_host(ctx().handle, src.ctypes.data, dst.ctypes.data, n, s.ctypes.data, iters, tt, th,
                                       float(mr), tr.ctypes.data, mask.ctypes.data, st.ctypes.data))
    return tr, mask, st


def run_dev(src, dst, samples, tt, th, iters, mr):
    import torch
    from introtocomputervision_amd._capi import check
    n = len(src)
    ds, dd = torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda()
    sm = torch.from_numpy(np.ascontiguousarray(samples, np.int32)).cuda()
    tr = torch.full((2, 2, 3), 7.0, device="cuda")
    mask = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    st = torch.full((3,), -9, dtype=torch.int32, device="cuda")
    check(lib().micv_ransac_solve_dev(ctx().handle, ds.data_ptr(), dd.data_ptr(), n, sm.data_ptr(), iters, tt, th,
                                      float(mr), tr.data_ptr(), mask.data_ptr(), st.data_ptr(),
                                      torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return tr.cpu().numpy(), mask.cpu().numpy(), st.cpu().numpy()


def run_matches(src, dst, seed, tt, th, iters, mr, cap_extra=0):
    """The device-sampler form, on keypoint / match arrays laid out as the chain leaves them."""
    import torch
    from introtocomputervision_amd._capi import check
    n = len(src)
    cap = n + cap_extra
    kpa = torch.zeros((n, 4), device="cuda")
    kpb = torch.zeros((n, 4), device="cuda")
    kpa[:, :2] = torch.from_numpy(src).cuda()
    perm = np.random.default_rng(n).permutation(n)  # matches point into kp_b out of order
    kpb[torch.from_numpy(perm).cuda(), :2] = torch.from_numpy(dst).cuda()
    m = torch.full((cap, 2), -1, dtype=torch.int32, device="cuda")
    m[:n, 0] = torch.arange(n, dtype=torch.int32, device="cuda")
    m[:n, 1] = torch.from_numpy(perm.astype(np.int32)).cuda()
    cnt = torch.tensor([n], dtype=torch.int64, device="cuda")
    tr = torch.full((2, 2, 3), 7.0, device="cuda")
    mask = torch.full((cap,), 9, dtype=torch.uint8, device="cuda")
    st = torch.full((3,), -9, dtype=torch.int32, device="cuda")
    check(lib().micv_ransac_solve_matches_dev(ctx().handle, kpa.data_ptr(), n, kpb.data_ptr(), n, m.data_ptr(),
                                              cnt.data_ptr(), cap, seed, iters, tt, th, float(mr), tr.data_ptr(),
                                              mask.data_ptr(), st.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return tr.cpu().numpy(), mask.cpu().numpy(), st.cpu().numpy()


def expect(src, dst, samples, tt, th, iters, mr):
    r = rr.solve_samples(src, dst, samples, tt, th, iters, mr)
    return r


def same(got, r, n=None):
    tr, mask, st = got
    assert st.tolist() == [r["iterations"], r["best_iter"], r["best_count"]]
    assert np.array_equal(bits(tr[0]), bits(r["t_last"])), (tr[0], r["t_last"])
    assert np.array_equal(bits(tr[1]), bits(r["t_best"])), (tr[1], r["t_best"])
    n = len(r["mask"]) if n is None else n
    assert np.array_equal(mask[:n], r["mask"])
    assert not mask[n:].any()


def noisy_set(tt, n, seed, frac=0.6, noise=3):
    n_in = max(tt, int(n * frac))
    src, dst, _, _ = pin.synth(tt, n, n_in, seed)
    rng = np.random.default_rng(seed + 99)
    dst = (dst + rng.integers(-noise, noise + 1, dst.shape) + rng.choice([0, 0.5, 0.25], dst.shape)).astype(np.float32)
    return src, dst


def ref_samples(n, tt, iters, words=pin.PS4_SEED_WORDS):
    from introtocomputervision_amd import ransac
    return ransac.Generator(words).samples(n, tt, iters).astype(np.int64)


SIZES = [1, 2, 3, 63, 64, 65, 117, 4095, LDS_MAX - 1, LDS_MAX, LDS_MAX + 1]


@pytest.mark.parametrize("tt", [1, 2, 3])
@pytest.mark.parametrize("n", SIZES)
def test_sizes_both_samplers(tt, n):
    if n < tt:
        pytest.skip("n < k")
    src, dst = noisy_set(tt, n, 1000 + n + tt)
    iters = 300
    mr = 0.5
    s = ref_samples(n, tt, iters)
    r = expect(src, dst, s, tt, 6, iters, mr)
    same(run_dev(src, dst, s, tt, 6, iters, mr), r)
    same(run_host(src, dst, s, tt, 6, iters, mr), r)
    seed = 0xC0FFEE + n
    sd = rr.device_samples(seed, n, tt, iters)
    same(run_matches(src, dst, seed, tt, 6, iters, mr, cap_extra=5), expect(src, dst, sd, tt, 6, iters, mr), n)


@pytest.mark.parametrize("tt", [1, 2, 3])
def test_streamed_65536(tt):
    n, iters = 65536, 64
    src, dst = noisy_set(tt, n, 77 + tt, frac=0.3)
    s = ref_samples(n, tt, iters)
    same(run_dev(src, dst, s, tt, 10, iters, 0.9), expect(src, dst, s, tt, 10, iters, 0.9))
    sd = rr.device_samples(5, n, tt, iters)
    same(run_matches(src, dst, 5, tt, 10, iters, 0.9), expect(src, dst, sd, tt, 10, iters, 0.9))


@pytest.mark.parametrize("tt", [1, 2, 3])
@pytest.mark.parametrize("iters,mr", [(1, 0.9), (2000, 0.75), (2000, 1.0), (100000, 1.0)])
def test_max_iters(tt, iters, mr):
    n = 117 if tt == 1 else 78
    src, dst = noisy_set(tt, n, 31 + tt, frac=0.5)
    s = ref_samples(n, tt, iters)
    same(run_dev(src, dst, s, tt, 6, iters, mr), expect(src, dst, s, tt, 6, iters, mr))


@pytest.mark.parametrize("tt", [1, 2, 3])
@pytest.mark.parametrize("stop", [0, 30, 31, 32, 33, 63, 64, 65, 1999])
def test_stop_around_chunk_boundaries(tt, stop):
    """Samples of outliers until iteration `stop`, which samples inliers: the run stops exactly there."""
    n = 200
    src, dst, _, inl = pin.synth(tt, n, 120, 500 + tt)
    ins, outs = np.nonzero(inl)[0], np.nonzero(~inl)[0]
    rng = np.random.default_rng(stop)
    s = np.stack([rng.choice(outs, tt, replace=False) for _ in range(2000)])
    s[stop] = ins[:tt]
    s[stop + 1:] = ins[:tt] if stop + 1 < 2000 else s[stop + 1:]
    mr = (120 - tt) / n
    r = expect(src, dst, s, tt, 1, 2000, mr)
    assert r["iterations"] == stop + 1
    same(run_dev(src, dst, s, tt, 1, 2000, mr), r)


@pytest.mark.parametrize("th", [0, 1, 6, 10, 46340])
@pytest.mark.parametrize("tt", [1, 2, 3])
def test_thresholds(tt, th):
    n = 300
    src, dst = noisy_set(tt, n, 900 + th, noise=12)
    if th == 46340:  # distances around sqrt(2^31): the float sqrt rounding and int32 wrap-around
        dst = (dst + np.random.default_rng(3).integers(-46345, 46345, dst.shape)).astype(np.float32)
    s = ref_samples(n, tt, 500)
    same(run_dev(src, dst, s, tt, th, 500, 0.99), expect(src, dst, s, tt, th, 500, 0.99))


def test_degenerate_and_duplicate_samples():
    n = 50
    for tt in (2, 3):
        src, dst = noisy_set(tt, n, 4)
        src[5] = src[6]  # coincident points: singular similarity / affine
        src[7:10, 1] = src[7:10, 0]  # collinear
        s = np.array([[5, 6, 7][:tt], [7, 8, 9][:tt], [3, 3, 3][:tt], [1, 2, 4][:tt]] * 10)
        same(run_dev(src, dst, s, tt, 6, 40, 0.99), expect(src, dst, s, tt, 6, 40, 0.99))


def test_nonfinite_points():
    n = 70
    src, dst = noisy_set(2, n, 8)
    src[3] = [np.nan, 1]
    dst[4] = [np.inf, 2]
    src[5] = [1e10, -1e10]
    s = ref_samples(n, 2, 100)
    same(run_dev(src, dst, s, 2, 6, 100, 0.9), expect(src, dst, s, 2, 6, 100, 0.9))


def test_min_ratio_zero_and_bad_sample_index():
    src, dst = noisy_set(1, 10, 1)
    tr, mask, st = run_dev(src, dst, np.zeros((5, 1)), 1, 3, 5, 0.0)
    assert st.tolist() == [0, -1, 0] and not tr.any() and not mask.any()
    tr, mask, st = run_dev(src, dst, np.array([[0], [10], [1]]), 1, 3, 3, 0.5)
    assert st.tolist() == [-1, -1, 0] and not tr.any() and not mask.any()


def test_error_returns():
    from introtocomputervision_amd._capi import EINVAL, last_error
    import torch
    src, dst = noisy_set(3, 10, 1)
    ds, dd = torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda()
    sm = torch.zeros((4, 3), dtype=torch.int32, device="cuda")
    out = [torch.zeros(12, device="cuda"), torch.zeros(10, dtype=torch.uint8, device="cuda"),
           torch.zeros(3, dtype=torch.int32, device="cuda")]
    L, h = lib(), ctx().handle
    cases = [(2, 3, 4, 3, 0.5), (10, 0, 4, 3, 0.5), (10, 4, 4, 3, 0.5), (10, 3, 0, 3, 0.5), (10, 3, 4, -1, 0.5),
             (10, 3, 4, 3, float("nan"))]
    for n, tt, iters, th, mr in cases:
        rc = L.micv_ransac_solve_dev(h, ds.data_ptr(), dd.data_ptr(), n, sm.data_ptr(), iters, tt, th, mr,
                                     *[o.data_ptr() for o in out], None)
        assert rc == EINVAL and last_error(), (n, tt, iters, th, mr)
        rc = L.micv_ransac_solve_matches_dev(h, ds.data_ptr(), 10, dd.data_ptr(), 10, sm.data_ptr(),
                                             sm.data_ptr(), 10, 0, iters, tt, th, mr, *[o.data_ptr() for o in out],
                                             None)
        assert rc == EINVAL or (n, tt) == (2, 3), (n, tt, iters, th, mr)
    s = np.array([[0, 1, 10]], np.int32)
    tr, m, st = np.zeros(12, np.float32), np.zeros(10, np.uint8), np.zeros(3, np.int32)
    rc = L.micv_ransac_solve_host(h, src.ctypes.data, dst.ctypes.data, 10, s.ctypes.data, 1, 3, 3, 0.5,
                                  tr.ctypes.data, m.ctypes.data, st.ctypes.data)
    assert rc == EINVAL and "outside" in last_error()


def test_python_solve_as_written_both_paths():
    """ransac.solve on numpy and on CUDA tensors = the literal loop driven by the sampler pin,
    three solves in a row on one generator (runProblem3's order)."""
    import torch
    from introtocomputervision_amd import ransac
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        exe = pin.build_pin(d)
        sets = pin.ps4_problem3_sets()
        want = pin.run_problem3(exe, sets)
    for to_dev in (False, True):
        g = ransac.Generator(pin.PS4_SEED_WORDS)
        for (src, dst, _, _), (tt, th, mi, mr), (t, pos, ratio, its, _) in zip(sets, pin.PS4_RANSAC, want):
            a, b = (torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda()) if to_dev else (src, dst)
            res = ransac.solve(a, b, tt, th, mi, mr, gen=g)
            got_t = res[0].cpu().numpy() if to_dev else res[0]
            assert np.array_equal(bits(got_t), bits(t)) and res[1] == pos and res[2] == ratio
            assert res.iterations == its


def test_chain_on_device_matches_reference():
    """Harris -> keypoints -> descriptors -> knn2 -> ratio filter -> solve_matches_dev on one stream
    (after Harris's own corner count, no host synchronisation), against the restatement on the
    downloaded matches with the device sampler, and the synthetic translation recovered."""
    import torch
    from introtocomputervision_amd import harris, match, synth
    from introtocomputervision_amd._capi import check
    rows, cols, dx, dy = 240, 320, 7, -5
    base = synth.checkerboard(rows + 40, cols + 40, square=23, seed=0x5EED0001)
    a = np.ascontiguousarray(base[20:20 + rows, 20:20 + cols])
    b = np.ascontiguousarray(base[20 - dy:20 - dy + rows, 20 - dx:20 - dx + cols])
    kps, descs = [], []
    for img in (a, b):
        t = torch.from_numpy(img).cuda()
        r = harris.cornersFromImage(t, threshold=1e6)
        kp = harris.getKeypoints(r["gx"], r["gy"], r["locs"], 10)
        kps.append(kp)
        descs.append(harris.computeDescriptors(r["gx"], r["gy"], kp))
    idx, dist = match.knnMatch2(descs[0], descs[1])
    nq = idx.shape[0]
    mqt = torch.empty((nq, 2), dtype=torch.int32, device="cuda")
    md = torch.empty((nq,), dtype=torch.float32, device="cuda")
    cnt = torch.zeros((1,), dtype=torch.int64, device="cuda")
    check(lib().micv_bf_ratio_filter_dev(ctx().handle, idx.data_ptr(), dist.data_ptr(), nq, 0.75, mqt.data_ptr(),
                                         md.data_ptr(), nq, cnt.data_ptr(), torch.cuda.current_stream().cuda_stream))
    from introtocomputervision_amd import ransac
    tr, mask, st = ransac.solve_matches(kps[0], kps[1], mqt, cnt, ransac.TRANSLATION, 3, 2000, 0.2, seed=42)
    torch.cuda.synchronize()
    n = int(cnt.item())
    assert n >= 20
    m = mqt[:n].cpu().numpy()
    src = kps[0].cpu().numpy()[m[:, 0], :2]
    dst = kps[1].cpu().numpy()[m[:, 1], :2]
    r = rr.solve_samples(src, dst, rr.device_samples(42, n, 1, 2000), 1, 3, 2000, 0.2)
    same((tr.cpu().numpy(), mask.cpu().numpy(), st.cpu().numpy()), r)
    assert r["t_best"].tolist() == [[1, 0, dx], [0, 1, dy]]
