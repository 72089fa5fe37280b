"""The pins of ps3 against the reference's own log (tests/golden/ps3/ps3.log), shared by the CPU test of the numpy
restatement and the GPU test of the device outputs.  Every yardstick comes from the log and float64 only.

e(X) = max_i |X_i - X64_i| / |X64_i| is the worst element-wise relative distance from the float64 solution of the same
float32 inputs; a result passes when e(result) <= 4 * max(e(log), 1e-4): 1e-4 is twice the log's print precision (five
digits), 4 the margin between two draws from the same rounding-noise scale in different summation orders."""
import numpy as np

import _ps3_ref as R

ROWS, COLS = 712, 1072  # cols from the logged x = 1071 of every right end point; the height cancels in every end point
FLOOR, MARGIN = 1e-4, 4.0


def e(X, X64):
    X, X64 = np.asarray(X, np.float64).reshape(-1), np.asarray(X64, np.float64).reshape(-1)
    nz = X64 != 0
    assert np.all(X[~nz] == 0), "an entry that is exactly zero in float64 is not zero"
    return float(np.max(np.abs(X[nz] - X64[nz]) / np.abs(X64[nz])))


def _fix_sign(v):
    v = np.asarray(v, np.float64).reshape(-1)
    return v * np.sign(v[-1])


def _calib_A(p2, p3, svd):
    rows = []
    for (x, y), (X, Y, Z) in zip(p2.astype(np.float64), p3.astype(np.float64)):
        rows.append([X, Y, Z, 1, 0, 0, 0, 0, -x * X, -x * Y, -x * Z, -x if svd else x])
        rows.append([0, 0, 0, 0, X, Y, Z, 1, -y * X, -y * Y, -y * Z, -y if svd else y])
    return np.asarray(rows, np.float64)


def calib_ls64(p2, p3):
    A = _calib_A(p2, p3, False)
    x = np.linalg.lstsq(A[:, :11], A[:, 11], rcond=None)[0]
    return np.append(x, 1.0)


def calib_svd64(p2, p3):
    return np.linalg.svd(_calib_A(p2, p3, True))[2][-1]


def fund_ls64(pa, pb):
    a, b = pa.astype(np.float64), pb.astype(np.float64)
    u, v, up, vp = a[:, 0], a[:, 1], b[:, 0], b[:, 1]
    A = np.stack([u * up, v * up, up, u * vp, v * vp, vp, u, v], axis=1)
    return np.append(np.linalg.lstsq(A, -np.ones(len(A)), rcond=None)[0], 1.0).reshape(3, 3)


def rank2_64(F):
    U, s, Vt = np.linalg.svd(np.asarray(F, np.float64).reshape(3, 3))
    s[-1] = 0
    return U @ np.diag(s) @ Vt


def transform64(p):
    p = p.astype(np.float64)
    m = max(1.0, np.abs(p).max())
    return np.diag([1 / m, 1 / m, 1]) @ np.array([[1, 0, -p[:, 0].mean()], [0, 1, -p[:, 1].mean()], [0, 0, 1]])


def normalized64(pa, pb):
    Ta, Tb = transform64(pa), transform64(pb)
    ha = (Ta @ np.vstack([pa.astype(np.float64).T, np.ones(len(pa))])).T[:, :2]
    hb = (Tb @ np.vstack([pb.astype(np.float64).T, np.ones(len(pb))])).T[:, :2]
    fhat = rank2_64(fund_ls64(ha, hb))
    return Ta, Tb, fhat, Tb.T @ fhat @ Ta


def project64(M, X):
    h = np.asarray(M, np.float64).reshape(3, 4) @ np.append(np.asarray(X, np.float64), 1.0)
    return h / h[2]


def endpoint_y_and_bound(F, pts, side, cols):
    """float64 y of the left and right end points of each point's line and the first-order bound
    sum_ij |dy/dF_ij| |F_ij| 5e-5 of the five-digit rounding of F.  -> y [n, 2], bound [n, 2]."""
    F = np.asarray(F, np.float64).reshape(3, 3)
    ys, bs = [], []
    for x, y in pts.astype(np.float64):
        p = np.array([x, y, 1.0])
        l = F.T @ p if side == 0 else F @ p
        row_y, row_b = [], []
        for X in (0.0, float(cols - 1)):
            yy = -(l[2] + l[0] * X) / l[1]
            dl = np.array([-X / l[1], (l[2] + l[0] * X) / l[1] ** 2, -1.0 / l[1]])
            # l_c = sum_r p_r F[r][c] (side 0) or sum_c F[r][c] p_c (side 1)
            dF = np.outer(p, dl) if side == 0 else np.outer(dl, p)
            row_y.append(yy)
            row_b.append(float(np.sum(np.abs(dF) * np.abs(F)) * 5e-5))
        ys.append(row_y)
        bs.append(row_b)
    return np.asarray(ys), np.asarray(bs)


def check_pins(got, log, P):
    """got: the outputs under test (see the keys used below).  Asserts every pin, returns the measured figures."""
    an, p3n, a, b = P["a_norm"], P["p3_norm"], P["a"], P["b"]
    fest64 = fund_ls64(a, b)
    Ta64, Tb64, fhat64, fb64 = normalized64(a, b)
    six = {
        "M_ls": (calib_ls64(an, p3n), lambda v: np.asarray(v, np.float64).reshape(-1)),
        "M_svd": (_fix_sign(calib_svd64(an, p3n)), _fix_sign),
        "F_est": (fest64, None), "F_rank2": (rank2_64(fest64), None), "F_hat": (fhat64, None), "F_better": (fb64, None),
        "T_a": (Ta64, None), "T_b": (Tb64, None),
    }
    out = {}
    for name, (x64, fix) in six.items():
        fix = fix or (lambda v: np.asarray(v, np.float64).reshape(-1))
        e_log, e_got = e(fix(log[name]), x64), e(fix(got[name]), x64)
        out[name] = {"e_log": e_log, "e": e_got, "bound": MARGIN * max(e_log, FLOOR)}
    # the 1a projections of the last point and their residuals, where the outputs under test hold them
    last3, last2 = p3n[-1], an[-1].astype(np.float64)
    for tag, m64 in (("ls", six["M_ls"][0]), ("svd", six["M_svd"][0])):
        pr64 = project64(m64, last3)
        r64 = float(np.linalg.norm(pr64[:2] - last2))
        for key, x64, lg in (("proj_" + tag, pr64, log["proj_" + tag]), ("res_" + tag, [r64], [log["res_" + tag]])):
            if key in got:
                e_log, e_got = e(lg, x64), e(got[key], x64)
                out[key] = {"e_log": e_log, "e": e_got, "bound": MARGIN * max(e_log, FLOOR)}
    # the camera centre from the logged best M against the logged centre
    Mb = np.asarray(log["M_best"], np.float32).astype(np.float64).reshape(3, 4)
    condQ = float(np.linalg.cond(Mb[:, :3]))
    c_log = log["center"].reshape(-1)
    rel = float(np.linalg.norm(np.asarray(got["center_from_log"], np.float64).reshape(-1) - c_log) / np.linalg.norm(c_log))
    out["center_from_log"] = {"e": rel, "bound": condQ * 5e-5, "cond_Q": condQ}
    # the 80 lines: from the logged rank-2 F (blocks 0, 1) and "better" F (blocks 2, 3)
    worst = 0.0
    for blk, (Fl, side, pts) in enumerate(((log["F_rank2"], 0, b), (log["F_rank2"], 1, a), (log["F_better"], 0, b),
                                           (log["F_better"], 1, a))):
        Fl = np.asarray(Fl, np.float32)
        _, bound = endpoint_y_and_bound(Fl, pts, side, COLS)
        g = np.asarray(got["endpoints_from_log"][blk], np.float64)
        lg = log["endpoints"][blk]
        for col, bcol in ((1, 0), (4, 1)):
            tol = bound[:, bcol] + 5e-6 + np.abs(lg[:, col]) * 5e-8  # the log prints eight significant digits
            ratio = np.abs(g[:, col] - lg[:, col]) / tol
            worst = max(worst, float(ratio.max()))
        assert np.all(g[:, 0] == 0) and np.all(np.abs(g[:, 3] - lg[:, 3]) <= (COLS - 1) * 2.0 ** -21), "end point x"
        assert np.all(np.abs(g[:, [2, 5]] - 1) <= 2.0 ** -22), "end point w"
    out["endpoints_from_log"] = {"e": worst, "bound": 1.0}
    bad = {k: v for k, v in out.items() if not v["e"] <= v["bound"]}
    assert not bad, f"outside the log's yardstick: {bad}"
    return out
