"""ps3 on the device (csrc/geom.hip) against the exact numpy restatement tests/_ps3_ref.py, bit for bit, in the float32
and the float64 mode; the device outputs against the reference's own log (tests/_ps3_pin.py); the float64 mode against
the true least-squares solution; and every MICV_EINVAL path."""
import json
import os

import numpy as np
import pytest

import _ps3_pin as pin
import _ps3_ref as R

pytestmark = pytest.mark.gpu
MODES = [False, True]


def _bits(a):
    """Bit pattern with every NaN made the same: NaN = NaN at the same positions, everything else bit for bit."""
    a = np.ascontiguousarray(a)
    if a.dtype.kind != "f":
        return a
    u = a.view(np.uint32 if a.dtype == np.float32 else np.uint64).copy()
    u[np.isnan(a)] = 0
    return u, np.isnan(a)


def same(got, want, what=""):
    got = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
    want = np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype.kind != "f":
        assert np.array_equal(got, want), what
        return
    (gu, gn), (wu, wn) = _bits(got), _bits(want)
    bad = np.nonzero((gu != wu) | (gn != wn))
    assert not len(bad[0]), f"{what}: {len(bad[0])} of {got.size} differ, first at {[int(b[0]) for b in bad]}: " \
                            f"{got[tuple(b[0] for b in bad)]!r} vs {want[tuple(b[0] for b in bad)]!r}"


def geo():
    from introtocomputervision_amd import geometry
    return geometry


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_trials(p2, p3, idx, k, j, kc=None, groups=None, f64=False, dev=True):
    g = geo()
    if dev:
        M, res, best = g.calib.trialsBatch(cuda(p2.T), cuda(p3.T), cuda(np.asarray(idx, np.int32)), k, j,
                                           kcount=None if kc is None else cuda(np.asarray(kc, np.int32)),
                                           group_sizes=groups, f64=f64)
    else:
        M, res, best = g.calib.trialsBatch(p2.T, p3.T, np.asarray(idx, np.int32), k, j, kcount=kc, group_sizes=groups,
                                           f64=f64)
    return M, res, best


def check_trials(p2, p3, idx, k, j, kc=None, groups=None, f64=False, dev=True, what=""):
    M, res, best = run_trials(p2, p3, idx, k, j, kc, groups, f64, dev)
    rM, rres, rbest = R.calib_ls_trials(p2, p3, idx, k, j, kcount=kc, group_sizes=groups, f64=f64)
    same(M, rM, what + " M")
    same(res, rres, what + " residual")
    for a, b, nm in zip(best, rbest, ("best_idx", "best_res", "best_M")):
        same(a, b, what + " " + nm)
    return M, res, best


def host_perms(n, trials, words=R.PS3_SEED_WORDS):
    from introtocomputervision_amd.ransac import Generator
    return geo().trialIndices(Generator(words), n, trials)


def subsets(seed, n, count, T):
    """T random index lists of `count` distinct points each (numpy's generator: any lists will do here)."""
    rng = np.random.default_rng(seed)
    return np.argsort(rng.random((T, n)), axis=1)[:, :count].astype(np.int32)


# ------------------------------------------------------------------ device = restatement

@pytest.mark.parametrize("f64", MODES)
@pytest.mark.parametrize("dev", [True, False])
def test_real_data_reference_trials(f64, dev):
    """The reference's 30 trials (8 / 12 / 16 constraints x 10, 4 test points, its seed) as one launch."""
    P = R.load_all()
    idx, kc, groups = R.reference_trials(host_perms(20, 30))
    check_trials(P["b"], P["p3"], idx, 16, 4, kc, groups, f64, dev, "ps3 1b")
    res = geo().calib.trials(cuda(P["b"].T) if dev else P["b"].T, cuda(P["p3"].T) if dev else P["p3"].T,
                             seed=R.PS3_SEED_WORDS, f64=f64)
    rM, rres, (bi, br, bm) = R.calib_ls_trials(P["b"], P["p3"], idx, 16, 4, kcount=kc, group_sizes=groups, f64=f64)
    same(res[0], rres.reshape(3, 10).T.copy(), "residual table")
    same(res[1].reshape(-1), bm[-1], "best M")
    assert res[2] == (8, 12, 16)[bi[-1] // 10]
    same(res[3], R.camera_center(bm[-1:], f64=f64)[0], "camera centre")


@pytest.mark.parametrize("f64", MODES)
@pytest.mark.parametrize("noise", [0.0, 0.5])
def test_synthetic_k_j_T(f64, noise):
    """k from the degenerate 0 .. 5 over 6 to 1024, j from 0 to 64, T across the wave and workgroup edges."""
    p2, p3 = R.synth_camera(11, 1100, noise)
    for k, j, T in ((0, 4, 5), (1, 4, 5), (3, 1, 9), (5, 4, 30), (6, 0, 1), (6, 4, 30), (7, 64, 63), (11, 5, 64),
                    (16, 4, 65), (100, 17, 30), (1024, 64, 6)):
        check_trials(p2, p3, subsets(k * 131 + j, len(p2), k + j, T), k, j, f64=f64, what=f"k {k} j {j} T {T}")
    p2, p3 = R.synth_camera(13, 3000, noise)  # more points than are staged in LDS
    check_trials(p2, p3, subsets(1, 3000, 20, 130), 16, 4, f64=f64, what="3000 points")
    p2, p3 = R.synth_camera(12, 40, noise)
    T = 10000
    idx = subsets(5, 40, 20, T)
    kc = np.random.default_rng(6).integers(6, 17, T).astype(np.int32)
    check_trials(p2, p3, idx, 16, 4, kc, [1, 4999, 0, 3000, 2000], f64, what="T 10000, groups of unequal size")


@pytest.mark.parametrize("f64", MODES)
def test_million_trials_device_sampler(f64):
    """10^6 trials drawn by the device sampler, every one of them compared."""
    import torch
    g = geo()
    P = R.load_all()
    T, k, j = 1_000_000, 8, 4
    idx = g.sampleIndices(0x1234ABCD5678, 20, k + j, T)
    ridx = R.sample_indices(0x1234ABCD5678, 20, k + j, T)
    same(idx, ridx, "device sampler")
    assert all(len(set(row)) == k + j for row in ridx[:2000].tolist())
    M, res, best = g.calib.trialsBatch(cuda(P["b"].T), cuda(P["p3"].T), idx, k, j, group_sizes=[T // 4, T - T // 4],
                                       f64=f64)
    torch.cuda.synchronize()
    rM, rres, rbest = R.calib_ls_trials(P["b"], P["p3"], ridx, k, j, group_sizes=[T // 4, T - T // 4], f64=f64)
    same(M, rM, "M")
    same(res, rres, "residual")
    for a, b in zip(best, rbest):
        same(a, b, "arg-min")
    # the sampler on another shape
    same(g.sampleIndices(7, 4096, 300, 50), R.sample_indices(7, 4096, 300, 50), "sampler 4096 / 300")


@pytest.mark.parametrize("f64", MODES)
def test_corners(f64):
    """Repeated indices, NaN / inf points, ties, chunk independence, determinism."""
    p2, p3 = R.synth_camera(3, 64, 0.3)
    idx = subsets(9, 64, 14, 200)
    idx[5, :10] = idx[5, 0]           # one point ten times: singular
    idx[6, 1] = idx[6, 0]             # a repeated point among enough others
    idx[7, 10:] = idx[7, 0]           # test points that are constraints
    check_trials(p2, p3, idx, 10, 4, f64=f64, what="repeated indices")
    q2, q3 = p2.copy(), p3.copy()
    q2[3, 0] = np.nan
    q3[8, 2] = np.inf
    q3[9, 1] = -np.inf
    q2[12, 1] = np.inf
    M, res, best = check_trials(q2, q3, idx, 10, 4, f64=f64, what="NaN / inf points")
    res = res.cpu().numpy()
    assert np.isnan(res).any() and np.isfinite(res).any()
    assert np.isfinite(res[int(best[0][-1])])  # a NaN never wins
    # ties: every trial twice, the copy first in one half and second in the other -> the first of a pair wins
    dup = np.concatenate([idx[:50], idx[:50], idx[100:150][::-1], idx[100:150]])
    M, res, best = check_trials(p2, p3, dup, 10, 4, groups=[100, 100], f64=f64, what="ties")
    bi = best[0].cpu().numpy()
    assert bi[0] < 50 and 100 <= bi[1] < 150
    # all NaN: nobody wins
    bad2 = np.full_like(p2, np.nan)
    M, res, best = check_trials(bad2, p3, idx[:70], 10, 4, groups=[3, 67], f64=f64, what="no winner")
    assert list(best[0].cpu().numpy()) == [-1, -1, -1] and float(best[1][-1]) == R.DBL_MAX
    # trial t of a batch = the same indices run alone or in another batch; two runs identical
    M, res, _ = run_trials(p2, p3, idx, 10, 4, f64=f64)
    M2, res2, _ = run_trials(p2, p3, idx, 10, 4, f64=f64)
    same(M2, M.cpu().numpy(), "second run")
    same(res2, res.cpu().numpy(), "second run")
    for t in (0, 63, 64, 199):
        M1, r1, _ = run_trials(p2, p3, idx[t:t + 1], 10, 4, f64=f64)
        same(M1[0], M[t].cpu().numpy(), "alone")
        same(r1[0], res[t].cpu().numpy(), "alone")
    Mh, rh, _ = run_trials(p2, p3, idx[37:140], 10, 4, f64=f64)
    same(Mh, M[37:140].cpu().numpy(), "another chunk")
    same(rh, res[37:140].cpu().numpy(), "another chunk")


@pytest.mark.parametrize("f64", MODES)
def test_svd_fundamental_and_small_pieces(f64):
    g = geo()
    P = R.load_all()
    p2, p3 = R.synth_camera(21, 1100, 0.4)
    for k, T in ((6, 30), (20, 65), (100, 7), (1024, 2), (3, 4)):
        idx = subsets(k, len(p2), k, T)
        same(g.calib.solveSVDBatch(cuda(p2.T), cuda(p3.T), cuda(idx), f64=f64), R.calib_svd(p2, p3, idx, f64=f64),
             f"svd k {k}")
    same(g.calib.solveSVD(P["a_norm"].T, P["p3_norm"].T, f64=f64).reshape(1, 12),
         R.calib_svd(P["a_norm"], P["p3_norm"], f64=f64), "1a svd (host entry)")
    q2 = p2.copy()
    q2[4, 0] = np.nan
    idx = subsets(2, 64, 8, 40)
    same(g.calib.solveSVDBatch(cuda(q2.T), cuda(p3.T), cuda(idx), f64=f64), R.calib_svd(q2, p3, idx, f64=f64),
         "svd with NaN points")
    rng = np.random.default_rng(4)
    pa = rng.uniform(0, 1000, (300, 2)).astype(np.float32)
    pb = (pa + rng.normal(0, 30, pa.shape)).astype(np.float32)
    for k, T in ((8, 64), (20, 33), (300, 3), (5, 9), (1, 2)):
        idx = subsets(k + 1, 300, k, T)
        same(g.fundamental.solveLeastSquaresBatch(cuda(pa.T), cuda(pb.T), cuda(idx), f64=f64),
             R.fundamental_ls(pa, pb, idx, f64=f64), f"fundamental k {k}")
    F = R.fundamental_ls(P["a"], P["b"], f64=f64)
    same(g.fundamental.solveLeastSquares(cuda(P["a"].T), cuda(P["b"].T), f64=f64).reshape(1, 9), F, "2a")
    mats = np.concatenate([F, rng.normal(0, 1, (70, 9)).astype(np.float32), np.zeros((1, 9), np.float32),
                           np.eye(3, dtype=np.float32).reshape(1, 9), np.full((1, 9), np.nan, np.float32)])
    same(g.fundamental.rankReduce(cuda(mats.reshape(-1, 3, 3)), f64=f64).reshape(-1, 9), R.rank_reduce(mats, f64=f64),
         "rank reduction")
    same(g.fundamental.rankReduce(F.reshape(3, 3), f64=f64).reshape(1, 9), R.rank_reduce(F, f64=f64), "2b (host)")
    for a, b in ((P["a"], P["b"]), (pa, pb), (pa[:9], pb[:9])):
        for dev in (True, False):
            got = g.fundamental.normalized(cuda(a.T) if dev else a.T, cuda(b.T) if dev else b.T, f64=f64)
            for x, y, nm in zip(got, R.fundamental_normalized(a, b, f64=f64), ("T_a", "T_b", "F_Hat", "F")):
                same(x.reshape(-1), y, nm)
    Fb = R.fundamental_normalized(P["a"], P["b"], f64=f64)[3]
    for side, pts in ((0, P["b"]), (1, P["a"]), (0, pa)):
        for dev in (True, False):
            same(g.fundamental.epipolarEndpoints(Fb.reshape(3, 3), cuda(pts.T) if dev else pts.T, side, 712, 1072,
                                                 f64=f64),
                 R.epipolar_endpoints(Fb, pts, side, 712, 1072, f64=f64), f"end points side {side}")
    Ms = np.concatenate([R.calib_ls_trials(p2, p3, subsets(1, 64, 12, 90), 12, 0, f64=f64, want_best=False)[0],
                         np.zeros((1, 12), np.float32)])
    same(g.cameraCenter(cuda(Ms), f64=f64), R.camera_center(Ms, f64=f64), "camera centre")
    same(g.cameraCenter(Ms[:3], f64=f64), R.camera_center(Ms[:3], f64=f64), "camera centre (host)")


# ------------------------------------------------------------------ the log, and the float64 mode

def device_outputs(f64, L, P):
    g = geo()
    an, p3n, a, b = P["a_norm"], P["p3_norm"], P["a"], P["b"]
    out = {}
    # 1a with its residual: the last point once more, as the test point
    p2x, p3x = np.vstack([an, an[-1:]]), np.vstack([p3n, p3n[-1:]])
    M, res, _ = g.calib.trialsBatch(cuda(p2x.T), cuda(p3x.T), cuda(np.arange(21, dtype=np.int32)[None]), 20, 1, f64=f64)
    out["M_ls"], out["res_ls"] = M[0].cpu().numpy(), [float(res[0])]
    same(g.calib.solveLeastSquares(cuda(an.T), cuda(p3n.T), f64=f64).reshape(-1), out["M_ls"], "1a, plain entry")
    out["M_svd"] = g.calib.solveSVD(cuda(an.T), cuda(p3n.T), f64=f64).cpu().numpy().reshape(-1)
    out["F_est"] = g.fundamental.solveLeastSquares(cuda(a.T), cuda(b.T), f64=f64).reshape(3, 3)
    out["F_rank2"] = g.fundamental.rankReduce(out["F_est"], f64=f64).cpu().numpy()
    out["F_est"] = out["F_est"].cpu().numpy()
    out["T_a"], out["T_b"], out["F_hat"], out["F_better"] = (
        t.cpu().numpy() for t in g.fundamental.normalized(cuda(a.T), cuda(b.T), f64=f64))
    out["center_from_log"] = g.cameraCenter(cuda(np.asarray(L["M_best"], np.float32).reshape(1, 12)), f64=f64).cpu().numpy()[0]
    out["endpoints_from_log"] = [
        g.fundamental.epipolarEndpoints(np.asarray(F, np.float32), cuda(pts.T), side, pin.ROWS, pin.COLS, f64=f64).cpu().numpy()
        for F, side, pts in ((L["F_rank2"], 0, b), (L["F_rank2"], 1, a), (L["F_better"], 0, b), (L["F_better"], 1, a))]
    return out


def f64_against_qr(P):
    """The float64 mode's 30 residuals against the true least-squares solution of each trial (QR on A)."""
    p2, p3 = P["b"], P["p3"]
    idx, kc, groups = R.reference_trials(host_perms(20, 30))
    _, res, _ = run_trials(p2, p3, idx, 16, 4, kc, groups, f64=True)
    res = res.cpu().numpy()
    worst, rows = 0.0, []
    for t in range(30):
        A = pin._calib_A(p2[idx[t, :kc[t]]], p3[idx[t, :kc[t]]], False)
        x = np.append(np.linalg.lstsq(A[:, :11], A[:, 11], rcond=None)[0], 1.0)
        r = np.mean([np.linalg.norm(pin.project64(x, p3[i])[:2] - p2[i].astype(np.float64)) for i in idx[t, kc[t]:kc[t] + 4]])
        S = A[:, :11].T @ A[:, :11]
        d = 1 / np.sqrt(np.diag(S))
        ks = np.linalg.cond(S * d[:, None] * d[None, :])
        bound = 8 * ks * 2.0 ** -53
        rel = abs(res[t] - r) / r
        rows.append((t, float(res[t]), float(r), float(rel), float(bound)))
        worst = max(worst, rel / bound)
    return res, rows, worst


def test_device_pinned_to_the_log_and_f64_usable():
    """The device outputs against the numbers the reference's binary printed (the criterion of tests/_ps3_pin.py, both
    modes), and the float64 mode against QR: relative residual difference <= 8 kappa_s 2^-53 per trial, kappa_s the
    condition number of A^T A after symmetric diagonal scaling.  In float64 all 30 residuals of problem 1b lie below
    10 pixels (0.5 .. 5.9 measured with numpy float64); the log's 2.45 .. 1764.8 and the float32 mode's equally wild
    values are float32 rounding noise of the 11 x 11 normal equations on un-normalised coordinates, not fit error."""
    L, P = R.parse_log(), R.load_all()
    report = {}
    for f64 in MODES:
        report["f64" if f64 else "f32"] = pin.check_pins(device_outputs(f64, L, P), L, P)
    res, rows, worst = f64_against_qr(P)
    for row in rows:
        print("trial %2d  f64 mode %.12g  QR %.12g  rel %.3g  bound %.3g" % row)
    report["f64_vs_qr_worst_ratio"] = worst
    report["f64_residual_range"] = [float(res.min()), float(res.max())]
    print(json.dumps(report))
    out = os.environ.get("MICV_PS3_PIN_OUT")
    if out:
        with open(out, "w") as f:
            json.dump(report, f, indent=1)
    assert worst <= 1.0, worst
    assert res.max() < 10.0


# ------------------------------------------------------------------ errors

def test_einval_paths_leave_outputs_untouched(ctx):
    """Every MICV_EINVAL path returns before anything is enqueued; outputs keep their fill."""
    import ctypes as C
    import torch
    from introtocomputervision_amd._capi import EINVAL, OK, lib
    P = R.load_all()
    p2, p3 = cuda(P["b"]), cuda(P["p3"])
    idx = cuda(subsets(1, 20, 12, 30))
    M = torch.full((30, 12), 7.0, device="cuda")
    res = torch.full((30,), 7.0, dtype=torch.float64, device="cuda")
    bi = torch.full((4,), 7, dtype=torch.int32, device="cuda")
    br = torch.full((4,), 7.0, dtype=torch.float64, device="cuda")
    bm = torch.full((4, 12), 7.0, device="cuda")
    st = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    gs = (C.c_int * 3)(10, 10, 10)

    def call(**kw):
        a = dict(ctx=ctx.handle, p2=p2.data_ptr(), p3=p3.data_ptr(), n=20, idx=idx.data_ptr(), stride=12, k=8, j=4,
                 T=30, kc=None, gs=gs, G=3, flags=0, M=M.data_ptr(), res=res.data_ptr(), bi=bi.data_ptr(),
                 br=br.data_ptr(), bm=bm.data_ptr(), st=st.data_ptr())
        a.update(kw)
        return lib.micv_calib_ls_trials_dev(a["ctx"], a["p2"], a["p3"], a["n"], a["idx"], a["stride"], a["k"], a["j"],
                                            a["T"], a["kc"], a["gs"], a["G"], a["flags"], a["M"], a["res"], a["bi"],
                                            a["br"], a["bm"], a["st"], None)

    bad_gs = (C.c_int * 3)(10, 10, 9)
    for kw in (dict(ctx=None), dict(p2=None), dict(p3=None), dict(M=None), dict(res=None), dict(st=None),
               dict(bi=None), dict(k=17, stride=21), dict(k=16, j=5, stride=21), dict(T=0), dict(T=-1), dict(gs=bad_gs),
               dict(G=0), dict(gs=None), dict(j=65), dict(stride=11), dict(flags=2), dict(idx=None), dict(n=0)):
        assert call(**kw) == EINVAL, kw
        assert lib.micv_last_error()
    torch.cuda.synchronize()
    for t in (M, res, bi, br, bm, st):
        assert bool((t == 7).all())
    assert call() == OK
    torch.cuda.synchronize()
    assert int(st[0]) == 0 and not bool((M == 7).any())
    # an index out of range: the host entry refuses it before anything is uploaded; outputs untouched
    g = geo()
    hidx = subsets(1, 20, 12, 30)
    hidx[17, 3] = 20
    hM = np.full((30, 12), 7, np.float32)
    hres = np.full(30, 7, np.float64)
    rc = lib.micv_calib_ls_trials_host(ctx.handle, P["b"].ctypes.data, P["p3"].ctypes.data, 20, hidx.ctypes.data, 12, 8,
                                       4, 30, None, None, 0, 0, hM.ctypes.data, hres.ctypes.data, None, None, None)
    assert rc == EINVAL and b"[17][3]" in lib.micv_last_error()
    assert (hM == 7).all() and (hres == 7).all()
    hidx[17, 3] = -1
    with pytest.raises(Exception):
        g.calib.solveSVDBatch(P["b"].T, P["p3"].T, hidx)
    with pytest.raises(Exception):
        g.fundamental.solveLeastSquaresBatch(P["a"].T, P["b"].T, hidx)
    # the device entry cannot see the list: it flags the call and gives that trial NaN, the others their values
    with pytest.raises(ValueError):
        g.calib.trialsBatch(cuda(P["b"].T), cuda(P["p3"].T), cuda(hidx), 8, 4)
    assert call(idx=cuda(hidx).data_ptr()) == OK
    torch.cuda.synchronize()
    assert int(st[0]) == 1 and bool(torch.isnan(M[17]).all()) and bool(torch.isnan(res[17]))
    hidx[17, 3] = 0
    rM, rres, _ = R.calib_ls_trials(P["b"], P["p3"], hidx, 8, 4)
    keep = np.arange(30) != 17
    same(M.cpu().numpy()[keep], rM[keep], "the other trials")
    # the other entries' argument checks
    o9 = torch.full((9,), 7.0, device="cuda")
    assert lib.micv_calib_svd_dev(ctx.handle, p2.data_ptr(), p3.data_ptr(), 20, None, 0, 1025, 1, 0, M.data_ptr(),
                                  st.data_ptr(), None) == EINVAL
    assert lib.micv_calib_svd_dev(ctx.handle, p2.data_ptr(), p3.data_ptr(), 20, None, 0, 20, 2, 0, M.data_ptr(),
                                  st.data_ptr(), None) == EINVAL
    assert lib.micv_fundamental_ls_dev(ctx.handle, p2.data_ptr(), p2.data_ptr(), 20, None, 0, 21, 1, 0, o9.data_ptr(),
                                       st.data_ptr(), None) == EINVAL
    assert lib.micv_fundamental_rank_reduce_dev(ctx.handle, o9.data_ptr(), 0, 0, o9.data_ptr(), None) == EINVAL
    assert lib.micv_fundamental_normalized_dev(ctx.handle, p2.data_ptr(), p2.data_ptr(), 0, 0, o9.data_ptr(),
                                               o9.data_ptr(), o9.data_ptr(), o9.data_ptr(), None) == EINVAL
    assert lib.micv_epipolar_endpoints_dev(ctx.handle, o9.data_ptr(), p2.data_ptr(), 20, 2, 10, 10, 0, M.data_ptr(),
                                           None) == EINVAL
    assert lib.micv_camera_center_dev(ctx.handle, None, 1, 0, o9.data_ptr(), None) == EINVAL
    assert lib.micv_geom_sample_indices_dev(ctx.handle, 1, 20, 21, 5, idx.data_ptr(), None) == EINVAL
    torch.cuda.synchronize()
    assert bool((o9 == 7).all())
