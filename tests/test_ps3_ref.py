"""CPU checks of ps3: the numpy restatement (tests/_ps3_ref.py) against the numbers the reference's own binary printed
(tests/golden/ps3/ps3.log, criterion in tests/_ps3_pin.py), the host-side trial sampler against a g++ pin of the
standard-library calls (tests/cpp/ps3_sampler_ref.cpp), and that mutations of the contract leave the yardstick."""
import os
import re
import subprocess

import numpy as np
import pytest

import _ps3_pin as pin
import _ps3_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ref_outputs(f64, L, P):
    an, p3n, a, b = P["a_norm"], P["p3_norm"], P["a"], P["b"]
    g = {}
    p2x, p3x = np.vstack([an, an[-1:]]), np.vstack([p3n, p3n[-1:]])  # the last point once more: 1a's test point
    M, res, _ = R.calib_ls_trials(p2x, p3x, np.arange(21)[None, :], 20, 1, f64=f64, want_best=False)
    g["M_ls"], g["res_ls"] = M[0], [res[0]]
    assert np.array_equal(R.calib_ls(an, p3n, f64=f64), M[0])
    g["M_svd"] = R.calib_svd(an, p3n, f64=f64)[0]
    g["proj_ls"] = R.project(g["M_ls"], p3n[-1], f64)
    g["proj_svd"] = R.project(g["M_svd"], p3n[-1], f64)
    assert R.point_residual(g["M_ls"], p3n[-1], an[-1], f64) == res[0] or f64
    g["res_svd"] = [R.point_residual(g["M_svd"], p3n[-1], an[-1], f64)]
    g["F_est"] = R.fundamental_ls(a, b, f64=f64)[0]
    g["F_rank2"] = R.rank_reduce(g["F_est"][None], f64=f64)[0]
    g["T_a"], g["T_b"], g["F_hat"], g["F_better"] = R.fundamental_normalized(a, b, f64=f64)
    g["center_from_log"] = R.camera_center(np.asarray(L["M_best"], np.float32).reshape(1, 12), f64=f64)[0]
    g["endpoints_from_log"] = [R.epipolar_endpoints(np.asarray(F, np.float32), pts, side, pin.ROWS, pin.COLS, f64=f64)
                               for F, side, pts in ((L["F_rank2"], 0, b), (L["F_rank2"], 1, a), (L["F_better"], 0, b),
                                                    (L["F_better"], 1, a))]
    return g


def test_fixture_shapes():
    P, L = R.load_all(), R.parse_log()
    assert [P[k].shape for k in ("a", "b", "a_norm", "p3", "p3_norm")] == [(20, 2), (20, 2), (20, 2), (20, 3), (20, 3)]
    assert L["residuals"].shape == (10, 3) and L["min_size"] == 8 and L["endpoints"].shape == (4, 20, 6)
    assert L["residuals"].min() == pytest.approx(L["min_residual"], rel=1e-5)
    assert np.allclose(L["pt3d"].reshape(-1)[:3], P["p3_norm"][-1], rtol=1e-5)


@pytest.mark.parametrize("f64", [False, True])
def test_restatement_pinned_to_the_log(f64):
    """Six matrices, T_a, T_b, 1a's projections and residuals, the camera centre from the logged M and the 80 epipolar
    lines from the logged F: e(result) <= 4 max(e(log), 1e-4) and the bounds of tests/_ps3_pin.py.  Measured for the
    float32 restatement: M 1.4e-5 (log 2.0e-5), SVD M 5.5e-6 (3.5e-5), F 2.7e-2 (1.46e-2), rank-2 F 2.7e-2 (1.45e-2),
    F_Hat 1.3e-3 (7.5e-4), "better" F 5.4e-2 (3.1e-2)."""
    L, P = R.parse_log(), R.load_all()
    rep = pin.check_pins(ref_outputs(f64, L, P), L, P)
    for k, v in rep.items():
        print(k, v)
    assert set(rep) >= {"M_ls", "M_svd", "F_est", "F_rank2", "F_hat", "F_better", "T_a", "T_b", "proj_ls", "proj_svd",
                        "res_ls", "res_svd", "center_from_log", "endpoints_from_log"}


def test_wrong_formulas_leave_the_yardstick():
    """The criterion is not vacuous: b = +1, a dropped column or a missing transpose land far outside it."""
    L, P = R.parse_log(), R.load_all()
    good = ref_outputs(False, L, P)
    for key, wrong in (("F_est", -good["F_est"] + 2 * np.eye(3, dtype=np.float32).reshape(9) * good["F_est"]),
                       ("F_better", good["F_better"].reshape(3, 3).T.reshape(9)),
                       ("M_ls", np.append(good["M_ls"][:10], [0, 1]).astype(np.float32)),
                       ("T_a", good["T_b"])):
        bad = dict(good)
        bad[key] = wrong
        with pytest.raises(AssertionError):
            pin.check_pins(bad, L, P)


def test_jacobi_converges_and_is_orthogonal():
    P = R.load_all()
    for f64 in (False, True):
        info = {}
        v = R.calib_svd(P["a_norm"], P["p3_norm"], f64=f64, info=info)[0]
        assert info["sweeps"] < R.MAX_SWEEPS and abs(float(np.linalg.norm(v.astype(np.float64))) - 1) < 1e-6
        F = R.fundamental_ls(P["a"], P["b"], f64=f64)
        r2 = R.rank_reduce(F, f64=f64, info=info)[0].astype(np.float64).reshape(3, 3)
        assert info["sweeps"] < R.MAX_SWEEPS
        s = np.linalg.svd(r2, compute_uv=False)
        assert s[2] <= (1e-6 if not f64 else 1e-7) * s[0]
    # NaN points: a NaN gamma never rotates, so the loop still ends within the cap
    bad = np.full((20, 2), np.nan, np.float32)
    R.calib_svd(bad, P["p3"], info=info)
    assert info["sweeps"] <= R.MAX_SWEEPS


def test_ldlt_solves_and_pivots():
    rng = np.random.default_rng(0)
    for N in (8, 11):
        B = rng.normal(size=(50, N, N))
        S = B @ B.transpose(0, 2, 1) + 0.1 * np.eye(N)
        S[:, np.arange(N), np.arange(N)] *= rng.uniform(1, 100, (50, N))  # make the pivot order matter
        S = (S + S.transpose(0, 2, 1)) / 2
        b = rng.normal(size=(50, N, 1))
        x = R.ldlt_solve(np.concatenate([S, b], axis=2).copy())
        assert np.allclose(x, np.linalg.solve(S, b)[:, :, 0], rtol=1e-8, atol=1e-10)
    # a zero pivot gives inf / NaN and does not raise
    with np.errstate(all="ignore"):
        x = R.ldlt_solve(np.zeros((1, 8, 9), np.float32))
    assert not np.isfinite(x).any()


def test_argmin_rules():
    res = np.array([np.nan, 3.0, 2.0, 2.0, np.inf, R.DBL_MAX, 1.0, np.nan])
    M = np.arange(8 * 12, dtype=np.float32).reshape(8, 12)
    bi, br, bm = R.argmin_records(res, M, [2, 2, 2, 2])
    assert list(bi) == [1, 2, -1, 6, 6] and br[2] == R.DBL_MAX and not bm[2].any() and np.array_equal(bm[4], M[6])


# ------------------------------------------------------------------ sampling

def build_pin(tmp):
    exe = os.path.join(str(tmp), "ps3_sampler_ref")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "ps3_sampler_ref.cpp"),
                    "-o", exe], check=True)
    return exe


def pin_run(exe, seed, runs):
    out = subprocess.run([exe, seed] + [str(v) for r in runs for v in r], check=True, capture_output=True,
                         text=True).stdout.split("\n")
    res = [[] for _ in runs]
    for line in out:
        if line:
            v = [int(x) for x in line.split()]
            res[v[0]].append(v[2:])
    return [np.asarray(r, np.int32).reshape(-1, n) for r, (n, _) in zip(res, runs)]


def test_trial_indices_equal_the_pin(tmp_path):
    """micv_geom_trial_indices word for word against the g++ pin: the ps3 seed (30 trials of 20) and three other
    seeds, n from 2 to 1000, and the generator left in the pin's state (one more draw)."""
    from introtocomputervision_amd import geometry
    from introtocomputervision_amd.ransac import Generator
    exe = build_pin(tmp_path)
    perms = pin_run(exe, R.PS3_SEED, [(20, 30)])
    assert perms[0][0].tolist() == [15, 3, 14, 10, 16, 0, 1, 6, 13, 5, 12, 7, 18, 8, 17, 11, 9, 2, 19, 4]
    # one engine through all the runs: each run starts in the state the one before left, and the last run (one more
    # draw) pins the state after everything else
    runs = [(20, 30), (2, 5), (3, 7), (17, 4), (64, 3), (255, 2), (1000, 3), (11, 1)]
    for seed in (R.PS3_SEED, "1", "deadbeef 2 3", "ffffffff 0 0 0 7 9 a b c"):
        want = pin_run(exe, seed, runs)
        g = Generator([int(w, 16) for w in seed.split()])
        for (n, trials), w in zip(runs, want):
            assert np.array_equal(geometry.trialIndices(g, n, trials), w), (seed, n)


def test_fresh_iota_differs_from_the_persistent_vector():
    """genUniqueRands starts every trial from 0 .. n-1; ransac::solve keeps shuffling one vector.  Same engine, same
    first permutation, different second one."""
    from introtocomputervision_amd import geometry
    from introtocomputervision_amd.ransac import Generator
    a = geometry.trialIndices(Generator(R.PS3_SEED_WORDS), 20, 2)
    g = Generator(R.PS3_SEED_WORDS)
    b = np.stack([g.permutation(20, 0), g.permutation(20, 1)])
    assert np.array_equal(a[0], b[0]) and not np.array_equal(a[1], b[1])
    assert np.array_equal(b[1], b[0][a[1]])  # the same second shuffle, applied to 0 .. 19 here and to b[0] there
    assert sorted(a[1].tolist()) == list(range(20))


def test_device_sampler_restatement_is_distinct_and_in_range():
    idx = R.sample_indices(99, 20, 20, 300)
    assert (np.sort(idx, axis=1) == np.arange(20)).all()
    idx = R.sample_indices(5, 4096, 320, 20)
    assert idx.min() >= 0 and idx.max() < 4096 and all(len(set(r)) == 320 for r in idx.tolist())


def test_python_layer_rejects_bad_shapes():
    from introtocomputervision_amd import geometry
    with pytest.raises(ValueError):
        geometry.calib.solveLeastSquares(np.zeros((3, 5), np.float32), np.zeros((3, 5), np.float32))
    with pytest.raises(ValueError):
        geometry.fundamental.solveLeastSquares(np.zeros((2, 5), np.float32), np.zeros((2, 6), np.float32))
    with pytest.raises(ValueError):
        geometry.calib.trials(np.zeros((2, 10), np.float32), np.zeros((3, 10), np.float32))


def test_geom_source_has_no_fused_multiply_add():
    """The contract says no FMA: the float kernels' ISA has no v_fma / v_mad on f32 / f64 outside the division and
    square-root expansions, which this check cannot separate -- so it checks the source and the build flag instead."""
    src = open(os.path.join(ROOT, "introtocomputervision_amd", "csrc", "geom.hip")).read()
    assert "fmaf(" not in src and "fma(" not in src.replace("fmaf(", "")
    assert "-ffp-contract=off" in open(os.path.join(ROOT, "introtocomputervision_amd", "csrc", "build.sh")).read()


def test_geom_kernels_use_no_scratch():
    """Nothing that pivoting permutes is indexed at run time in a per-thread array: every kernel of geom.hip compiles
    to 0 bytes of scratch and spills no vector register (tools/kernel_resources.py, the compiler's own report)."""
    import sys
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "geom"],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = [ln for ln in out.stdout.split("\n") if " scratch " in ln]
    assert len(rows) >= 18 and any("calib_ls_kernel<float>" in r for r in rows)
    for r in rows:
        assert re.search(r"spill\s+0 sgpr", r) and re.search(r"scratch\s+0 occ", r), r
