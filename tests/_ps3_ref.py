"""Exact numpy restatement of the ps3 geometry contract of include/mi_cv.h ("ps3: geometry"): the normal-equation
solves with diagonal-pivoted LDL^T, the trial residual and its arg-min, the one-sided Jacobi, rank reduction, the
normalised chain, epipolar end points and the camera centre.  Written from the reference's ps3_cpp sources and the
header, not from the kernels.  Everything is vectorised over the T systems of a batch: numpy's float32 / float64
element-wise operations round each element exactly as one scalar operation does, so one array pass per scalar
operation of the contract keeps this an exact restatement, and a million trials can be checked in full.

`f64` selects R = float64 (MICV_GEOM_F64); otherwise R = float32.  Points are rows: pts2d [n, 2], pts3d [n, 3]."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ps3")
PS3_SEED = "16 38 c7 e4 6a a2 d8 cc 96 f6 fe f1 4b 7d a7 25"  # config/ps3.yaml `mersenne_seed`
PS3_SEED_WORDS = [int(w, 16) for w in PS3_SEED.split()]
DBL_MAX = np.finfo(np.float64).max
MAX_SWEEPS = 30


def _R(f64):
    return np.float64 if f64 else np.float32


# ------------------------------------------------------------------ fixtures

def load_points(name):
    """A point file of the reference (whitespace-separated rows) -> [n, dims] float32."""
    with open(os.path.join(GOLDEN, name)) as f:
        return np.asarray([[float(v) for v in line.split()] for line in f if line.strip()], np.float32)


def load_all():
    return {k: load_points(v) for k, v in (("a", "pts2d-pic_a.txt"), ("b", "pts2d-pic_b.txt"),
                                            ("a_norm", "pts2d-norm-pic_a.txt"), ("p3", "pts3d.txt"),
                                            ("p3_norm", "pts3d-norm.txt"))}


_NUM = r"[-+]?(?:\d+\.?\d*|\.\d+)(?:[eE][-+]?\d+)?"


def parse_log(path=None):
    """The numbers the reference's binary printed (tests/golden/ps3/ps3.log), as float64 arrays."""
    text = open(path or os.path.join(GOLDEN, "ps3.log")).read()

    def mat_after(label, rows, cols, start=0):
        i = text.index(label, start)
        j = text.index("]", i)
        body = text[text.index("[", i + len(label)) + 1:j]
        v = [float(x) for x in re.findall(_NUM, body)]
        assert len(v) == rows * cols, (label, v)
        return np.asarray(v, np.float64).reshape(rows, cols), j

    out = {}
    out["M_ls"], e = mat_after("Calibration parameters (using normal least squares):", 3, 4)
    out["pt3d"], e = mat_after("Projected 3D point", 1, 4, e)
    out["proj_ls"], e = mat_after("to 2D point", 1, 3, e)
    out["res_ls"] = float(re.search(r"Residual = (" + _NUM + ")", text[e:]).group(1))
    out["M_svd"], e = mat_after("Calibration parameters (using singular value decomposition):", 3, 4, e)
    _, e = mat_after("Projected 3D point", 1, 4, e)
    out["proj_svd"], e = mat_after("to 2D point", 1, 3, e)
    out["res_svd"] = float(re.search(r"Residual = (" + _NUM + ")", text[e:]).group(1))
    out["residuals"], e = mat_after("All computed residuals:", 10, 3, e)
    out["min_residual"] = float(re.search(r"Minimum residual: (" + _NUM + ")", text).group(1))
    out["min_size"] = int(re.search(r"Found with constraint size: (\d+)", text).group(1))
    out["M_best"], e = mat_after("Computed parameters:", 3, 4, e)
    out["center"], e = mat_after("Center of camera:", 3, 1, e)
    out["F_est"], e = mat_after("Fundamental matrix estimate:", 3, 3, e)
    out["F_rank2"], e = mat_after("Fundamental matrix with rank = 2", 3, 3, e)
    out["T_a"], e = mat_after("Transform matrix T_a:", 3, 3, e)
    out["T_b"], e = mat_after("Transform matrix T_b:", 3, 3, e)
    out["F_hat"], e = mat_after("Fundamental matrix F_Hat:", 3, 3, e)
    out["F_better"], e = mat_after("fundamental matrix F:", 3, 3, e)
    ends = re.findall(r"@pt(\d+): P_iL=\[([^\]]*)\], P_iR=\[([^\]]*)\]", text)
    assert len(ends) == 80
    arr = np.asarray([[float(x) for x in (l + "," + r).split(",")] for _, l, r in ends], np.float64)
    # four blocks of 20: problem 2 image A (lines of the points of B), image B; extra credit image A, image B
    out["endpoints"] = arr.reshape(4, 20, 6)
    return out


# ------------------------------------------------------------------ normal equations + LDL^T

def _calib_row(p2, p3, ids, row, svd, R):
    """[T, 12]: the x row (row 0) or y row (row 1) of each system's point `ids`; entry 11 is b (or -u for the SVD)."""
    X, Y, Z = (p3[ids, c].astype(R) for c in range(3))
    u = p2[ids, row].astype(R)
    one, zero = np.ones_like(X), np.zeros_like(X)
    lead = [X, Y, Z, one]
    cols = ([*lead, zero, zero, zero, zero] if row == 0 else [zero, zero, zero, zero, *lead])
    cols += [(-u) * X, (-u) * Y, (-u) * Z, (-u if svd else u)]
    return np.stack(cols, axis=1)


def _fund_row(pa, pb, ids, R):
    u, v, up, vp = pa[ids, 0].astype(R), pa[ids, 1].astype(R), pb[ids, 0].astype(R), pb[ids, 1].astype(R)
    return np.stack([u * up, v * up, up, u * vp, v * vp, vp, u, v, np.full_like(u, -1)], axis=1)


def ldlt_solve(S):
    """S [T, N, N + 1] (the last column is the right-hand side) -> x [T, N]; S is overwritten."""
    T, N = S.shape[0], S.shape[1]
    ar = np.arange(T)
    perm = np.zeros((T, N), np.int64)
    dg = np.arange(N)
    for p in range(N):
        diag = np.abs(S[:, dg, dg])
        q = np.full(T, p, np.int64)
        best = diag[:, p].copy()
        for i in range(p + 1, N):
            m = diag[:, i] > best
            best = np.where(m, diag[:, i], best)
            q = np.where(m, i, q)
        rp, rq = S[ar, p, :].copy(), S[ar, q, :].copy()
        S[ar, p, :] = rq
        S[ar, q, :] = rp
        cp, cq = S[ar, :, p].copy(), S[ar, :, q].copy()
        S[ar, :, p] = cq
        S[ar, :, q] = cp
        perm[:, p] = q
        d = S[:, p, p].copy()
        rowp = S[:, p, :].copy()
        l = rowp[:, :N] / d[:, None]
        m = N - 1 - p
        if m:
            i = np.arange(p + 1, N)[:, None]
            jj = np.arange(p + 1, N + 1)[None, :]
            hi = np.where(jj < N, np.maximum(i, jj), i)
            lo = np.where(jj < N, np.minimum(i, jj), N)
            S[:, p + 1:, p + 1:] = S[:, p + 1:, p + 1:] - l[:, hi] * rowp[:, lo]
            S[:, p + 1:, p] = l[:, p + 1:]
    x = np.zeros((T, N), S.dtype)
    for p in range(N - 1, -1, -1):
        s = S[:, p, N] / S[:, p, p]
        for i in range(p + 1, N):
            s = s - S[:, i, p] * x[:, i]
        x[:, p] = s
    for p in range(N - 1, -1, -1):
        q = perm[:, p]
        a, b = x[ar, p].copy(), x[ar, q].copy()
        x[ar, p] = b
        x[ar, q] = a
    return x


def _calib_solve(p2, p3, idx, R):
    T, k = idx.shape
    S = np.zeros((T, 11, 12), R)
    for i in range(k):
        for row in (0, 1):
            a = _calib_row(p2, p3, idx[:, i], row, False, R)
            S = S + a[:, :11, None] * a[:, None, :]
    x = ldlt_solve(S)
    return np.concatenate([x, np.ones((T, 1), R)], axis=1)


def _residual(M, p2, p3, tests, R):
    T, j = tests.shape
    s = np.zeros(T, np.float64)
    Md = M.astype(np.float64)
    for e in range(j):
        ids = tests[:, e]
        X, Y, Z = (p3[ids, c].astype(np.float64) for c in range(3))
        pr = []
        for r in range(3):
            v = Md[:, 4 * r] * X
            v = v + Md[:, 4 * r + 1] * Y
            v = v + Md[:, 4 * r + 2] * Z
            v = v + Md[:, 4 * r + 3] * 1.0
            pr.append(v.astype(R))
        rc = (1.0 / pr[2].astype(np.float64)).astype(R)
        d0 = (pr[0] * rc - p2[ids, 0].astype(R)).astype(np.float64)
        d1 = (pr[1] * rc - p2[ids, 1].astype(R)).astype(np.float64)
        s = s + np.sqrt(d0 * d0 + d1 * d1)
    return s / np.float64(j)


def project(M, X, f64=False):
    """project3D of one point with the contract's arithmetic: M [12] (R or float32), X [3] float32 -> [3] in R."""
    R = _R(f64)
    Md, Xd = np.asarray(M).astype(R).astype(np.float64), np.asarray(X, np.float32).astype(np.float64)
    pr = []
    for r in range(3):
        v = Md[4 * r] * Xd[0]
        v = v + Md[4 * r + 1] * Xd[1]
        v = v + Md[4 * r + 2] * Xd[2]
        v = v + Md[4 * r + 3] * 1.0
        pr.append(R(v))
    rc = R(1.0 / np.float64(pr[2]))
    return np.asarray([pr[0] * rc, pr[1] * rc, pr[2] * rc], R)


def point_residual(M, X, x, f64=False):
    """cv::norm(projection(0:2), x) of the contract for one point -> float64."""
    R = _R(f64)
    pr = project(M, X, f64)
    d0 = np.float64(R(pr[0] - R(x[0])))
    d1 = np.float64(R(pr[1] - R(x[1])))
    return float(np.sqrt(d0 * d0 + d1 * d1))


def argmin_records(residual, M, group_sizes=None):
    """G + 1 records (idx, residual, M[12]): per group, then overall; first strict minimum below DBL_MAX."""
    T = len(residual)
    bounds = [0]
    for g in (group_sizes or []):
        bounds.append(bounds[-1] + int(g))
    spans = list(zip(bounds[:-1], bounds[1:])) + [(0, T)]
    bi = np.full(len(spans), -1, np.int32)
    br = np.full(len(spans), DBL_MAX, np.float64)
    bm = np.zeros((len(spans), 12), np.float32)
    for n, (lo, hi) in enumerate(spans):
        r = residual[lo:hi]
        r = np.where(np.isnan(r), np.inf, r)
        if len(r) and r.min() < DBL_MAX:
            w = lo + int(np.argmin(r))
            bi[n], br[n], bm[n] = w, residual[w], M[w]
    return bi, br, bm


def calib_ls_trials(p2, p3, indices, k, j, kcount=None, group_sizes=None, f64=False, want_best=True):
    """-> M [T, 12] f32, residual [T] f64, (best_idx, best_res, best_M)."""
    R = _R(f64)
    n = len(p2)
    indices = np.asarray(indices, np.int64)
    T = indices.shape[0]
    kc = np.full(T, k, np.int64) if kcount is None else np.asarray(kcount, np.int64)
    M = np.full((T, 12), np.nan, np.float32)
    res = np.full(T, np.nan, np.float64)
    with np.errstate(all="ignore"):
        for kv in np.unique(kc):
            sel = np.nonzero(kc == kv)[0]
            if kv < 0 or kv > k:
                continue
            idx = indices[sel, :kv + j]
            ok = np.all((idx >= 0) & (idx < n), axis=1)
            sel, idx = sel[ok], idx[ok]
            if not len(sel):
                continue
            for c0 in range(0, len(sel), 1 << 16):  # in chunks: the temporaries of a million systems are large
                s, ix = sel[c0:c0 + (1 << 16)], idx[c0:c0 + (1 << 16)]
                Mr = _calib_solve(p2, p3, ix[:, :kv], R)
                M[s] = Mr.astype(np.float32)
                res[s] = _residual(Mr, p2, p3, ix[:, kv:kv + j], R)
    return M, res, (argmin_records(res, M, group_sizes) if want_best else None)


def calib_ls(p2, p3, f64=False):
    """calib::solveLeastSquares of all points -> [12] f32."""
    idx = np.arange(len(p2))[None, :]
    return calib_ls_trials(p2, p3, idx, len(p2), 0, f64=f64, want_best=False)[0][0]


def fundamental_ls(pa, pb, indices=None, f64=False, raw=False):
    """-> F [T, 9] f32 (raw: in R, unrounded)."""
    R = _R(f64)
    idx = np.arange(len(pa))[None, :] if indices is None else np.asarray(indices, np.int64)
    T, k = idx.shape
    out = np.full((T, 9), np.nan, R)
    ok = np.all((idx >= 0) & (idx < len(pa)), axis=1) if k else np.ones(T, bool)
    with np.errstate(all="ignore"):
        sub = idx[ok]
        S = np.zeros((len(sub), 8, 9), R)
        for i in range(k):
            a = _fund_row(pa, pb, sub[:, i], R)
            S = S + a[:, :8, None] * a[:, None, :]
        x = ldlt_solve(S)
        out[ok] = np.concatenate([x, np.ones((len(sub), 1), R)], axis=1)
    return out if raw else out.astype(np.float32)


# ------------------------------------------------------------------ one-sided Jacobi

def _colsum(prod):
    """[T, rows] -> [T]: 64 serial partials (partial l takes rows l, l + 64, ..) joined by the xor butterfly."""
    T, rows = prod.shape
    part = np.zeros((T, 64), prod.dtype)
    for m in range(0, rows, 64):
        blk = prod[:, m:m + 64]
        part[:, :blk.shape[1]] = part[:, :blk.shape[1]] + blk
    lanes = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        part = part + part[:, lanes ^ m]
    return part[:, 0]


def jacobi(A):
    """A [T, rows, NC] (overwritten) -> rotated A, V [T, NC, NC], column norms [T, NC], sweeps used."""
    R = A.dtype.type
    T, rows, NC = A.shape
    eps = R(1e-7) if R is np.float32 else R(1e-15)
    V = np.zeros((T, NC, NC), R)
    V[:, np.arange(NC), np.arange(NC)] = 1
    sweeps = 0
    with np.errstate(all="ignore"):
        for _ in range(MAX_SWEEPS):
            sweeps += 1
            any_rot = np.zeros(T, bool)
            for p in range(NC - 1):
                for q in range(p + 1, NC):
                    ap, aq = A[:, :, p].copy(), A[:, :, q].copy()
                    al, be, ga = _colsum(ap * ap), _colsum(aq * aq), _colsum(ap * aq)
                    rot = np.abs(ga) > eps * np.sqrt(al * be)
                    if not rot.any():
                        continue
                    any_rot |= rot
                    zeta = (be - al) / (R(2) * ga)
                    t = np.where(zeta >= 0, R(1), R(-1)) / (np.abs(zeta) + np.sqrt(R(1) + zeta * zeta))
                    c = R(1) / np.sqrt(R(1) + t * t)
                    s = c * t
                    c1, s1, r1 = c[:, None], s[:, None], rot[:, None]
                    A[:, :, p] = np.where(r1, c1 * ap - s1 * aq, ap)
                    A[:, :, q] = np.where(r1, s1 * ap + c1 * aq, aq)
                    vp, vq = V[:, :, p].copy(), V[:, :, q].copy()
                    V[:, :, p] = np.where(r1, c1 * vp - s1 * vq, vp)
                    V[:, :, q] = np.where(r1, s1 * vp + c1 * vq, vq)
            if not any_rot.any():
                break
        cn = np.stack([_colsum(A[:, :, c] * A[:, :, c]) for c in range(NC)], axis=1)
    return A, V, cn, sweeps


def _first_smallest(cn):
    m = np.zeros(len(cn), np.int64)
    ar = np.arange(len(cn))
    for c in range(1, cn.shape[1]):
        m = np.where(cn[:, c] < cn[ar, m], c, m)
    return m


def calib_svd(p2, p3, indices=None, f64=False, info=None):
    """calib::solveSVD -> [T, 12] f32."""
    R = _R(f64)
    idx = np.arange(len(p2))[None, :] if indices is None else np.asarray(indices, np.int64)
    T, k = idx.shape
    out = np.full((T, 12), np.nan, np.float32)
    ok = np.all((idx >= 0) & (idx < len(p2)), axis=1)
    sub = idx[ok]
    A = np.zeros((len(sub), 2 * k, 12), R)
    with np.errstate(all="ignore"):
        for i in range(k):
            for row in (0, 1):
                A[:, 2 * i + row, :] = _calib_row(p2, p3, sub[:, i], row, True, R)
    A, V, cn, sweeps = jacobi(A)
    if info is not None:
        info["sweeps"] = sweeps
    m = _first_smallest(cn)
    out[ok] = V[np.arange(len(sub)), :, m].astype(np.float32)
    return out


def rank_reduce(F, f64=False, raw=False, info=None):
    """fundamental::rankReduce of [T, 9] (float32, or R when chained) -> [T, 9]."""
    R = _R(f64)
    A = np.asarray(F).astype(R).reshape(-1, 3, 3).copy()
    A, V, cn, sweeps = jacobi(A)
    if info is not None:
        info["sweeps"] = sweeps
    m = _first_smallest(cn)
    T = len(A)
    A[np.arange(T), :, m] = 0
    out = np.zeros((T, 3, 3), R)
    with np.errstate(all="ignore"):
        for r in range(3):
            for c in range(3):
                s = np.zeros(T, R)
                for jn in range(3):
                    s = s + A[:, r, jn] * V[:, c, jn]
                out[:, r, c] = s
    out = out.reshape(T, 9)
    return out if raw else out.astype(np.float32)


# ------------------------------------------------------------------ the small pieces

def gemm3(A, B, R):
    A, B = np.asarray(A).reshape(3, 3), np.asarray(B).reshape(3, 3)
    C = np.zeros((3, 3), R)
    with np.errstate(all="ignore"):
        for r in range(3):
            for c in range(3):
                s = np.float64(A[r, 0]) * np.float64(B[0, c])
                s = s + np.float64(A[r, 1]) * np.float64(B[1, c])
                s = s + np.float64(A[r, 2]) * np.float64(B[2, c])
                C[r, c] = R(s)
    return C


def _norm_transform(p, R):
    n = len(p)
    mean = []
    with np.errstate(all="ignore"):
        for d in range(2):
            s = np.float64(0)
            i = 0
            while i + 4 <= n:
                s = s + np.float64(((R(p[i, d]) + R(p[i + 1, d])) + R(p[i + 2, d])) + R(p[i + 3, d]))
                i += 4
            while i < n:
                s = s + np.float64(R(p[i, d]))
                i += 1
            mean.append(R(s / np.float64(n)))
        mx = R(1)
        for v in np.abs(p.astype(R)).reshape(-1):
            if v > mx:
                mx = v
        sc = R(np.float64(1.0) / np.float64(mx))
    scale = np.array([[sc, 0, 0], [0, sc, 0], [0, 0, 1]], R)
    offset = np.array([[1, 0, -mean[0]], [0, 1, -mean[1]], [0, 0, 1]], R)
    return gemm3(scale, offset, R)


def _apply_T(Tm, p, R):
    out = np.zeros((len(p), 2), R)
    x, y = p[:, 0].astype(np.float64), p[:, 1].astype(np.float64)
    with np.errstate(all="ignore"):
        for d in range(2):
            s = np.float64(Tm[d, 0]) * x
            s = s + np.float64(Tm[d, 1]) * y
            s = s + np.float64(Tm[d, 2]) * 1.0
            out[:, d] = s.astype(R)
    return out


def fundamental_normalized(pa, pb, f64=False):
    """-> T_a, T_b, F_Hat, F, [9] f32 each."""
    R = _R(f64)
    Ta, Tb = _norm_transform(pa, R), _norm_transform(pb, R)
    na, nb = _apply_T(Ta, pa, R), _apply_T(Tb, pb, R)
    est = fundamental_ls(na, nb, f64=f64, raw=True)
    fhat = rank_reduce(est, f64=f64, raw=True)[0].reshape(3, 3)
    F = gemm3(gemm3(Tb.T, fhat, R), Ta, R)
    return tuple(m.astype(np.float32).reshape(9) for m in (Ta, Tb, fhat, F))


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def epipolar_endpoints(F, pts, side, rows, cols, f64=False):
    """-> [n, 6] f32: P_iL, P_iR of each point's epipolar line."""
    R = _R(f64)
    F = np.asarray(F, np.float32).reshape(3, 3).astype(np.float64)
    n = len(pts)
    x, y = pts[:, 0].astype(np.float64), pts[:, 1].astype(np.float64)
    one, zero = np.ones(n, R), np.zeros(n, R)
    rm1, cm1 = one * R(rows - 1), one * R(cols - 1)
    with np.errstate(all="ignore"):
        IL = _cross([zero, zero, one], [zero, rm1, one])
        IR = _cross([cm1, zero, one], [cm1, rm1, one])
        l = []
        for c in range(3):
            if side == 0:
                s = x * F[0, c]
                s = s + y * F[1, c]
                s = s + 1.0 * F[2, c]
            else:
                s = F[c, 0] * x
                s = s + F[c, 1] * y
                s = s + F[c, 2] * 1.0
            l.append(s.astype(R))
        PL, PR = _cross(l, IL), _cross(l, IR)
        rl = (1.0 / PL[2].astype(np.float64)).astype(R)
        rr = (1.0 / PR[2].astype(np.float64)).astype(R)
        out = np.stack([PL[0] * rl, PL[1] * rl, PL[2] * rl, PR[0] * rr, PR[1] * rr, PR[2] * rr], axis=1)
    return out.astype(np.float32)


def camera_center(M, f64=False):
    """M [T, 12] f32 -> [T, 3] f32."""
    R = _R(f64)
    M = np.asarray(M, np.float32).reshape(-1, 12)
    m = M.astype(np.float64)
    a, b, c, d, e, f, g, h, i = (m[:, n] for n in (0, 1, 2, 4, 5, 6, 8, 9, 10))
    with np.errstate(all="ignore"):
        det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g)
        nz = det != 0
        inv = 1.0 / det
        cof = [e * i - f * h, c * h - b * i, b * f - c * e, f * g - d * i, a * i - c * g, c * d - a * f,
               d * h - e * g, b * g - a * h, a * e - b * d]
        I = [np.where(nz, (v * inv).astype(R), R(0)).astype(R) for v in cof]
        out = np.zeros((len(M), 3), np.float32)
        for r in range(3):
            s = I[3 * r].astype(np.float64) * m[:, 3]
            s = s + I[3 * r + 1].astype(np.float64) * m[:, 7]
            s = s + I[3 * r + 2].astype(np.float64) * m[:, 11]
            out[:, r] = (-1.0 * s).astype(R).astype(np.float32)
    return out


# ------------------------------------------------------------------ sampling

def splitmix64(x):
    x = np.asarray(x, np.uint64)
    with np.errstate(over="ignore"):
        z = x + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def sample_indices(seed, n, count, T):
    """The counter-based device sampler of mi_cv.h -> [T, count] int32."""
    out = np.zeros((T, count), np.int32)
    t = np.arange(T, dtype=np.uint64) << np.uint64(32)
    for e in range(count):
        todo = np.arange(T)
        a = 0
        while len(todo):
            r = splitmix64(np.uint64(seed) ^ (t[todo] | np.uint64(e << 20) | np.uint64(a & 0xFFFFF)))
            idx = (((r >> np.uint64(32)) * np.uint64(n)) >> np.uint64(32)).astype(np.int32)
            dup = (out[todo, :e] == idx[:, None]).any(axis=1) if e else np.zeros(len(todo), bool)
            out[todo[~dup], e] = idx[~dup]
            todo = todo[dup]
            a += 1
    return out


def reference_trials(perms, sizes=(8, 12, 16), iters=10, tests=4):
    """The index lists of Solution.cpp's trial loop from its 30 permutations [30, n]: indices [T, max(sizes) + tests]
    (unused entries 0), kcount [T], group sizes."""
    T = len(sizes) * iters
    kmax = max(sizes)
    idx = np.zeros((T, kmax + tests), np.int32)
    kc = np.repeat(np.asarray(sizes, np.int32), iters)
    for t in range(T):
        idx[t, :kc[t] + tests] = perms[t][:kc[t] + tests]
    return idx, kc, [iters] * len(sizes)


def synth_camera(seed, n, noise=0.0):
    """n world points seen by a plausible camera -> pts2d [n, 2], pts3d [n, 3] float32."""
    rng = np.random.default_rng(seed)
    p3 = rng.uniform(-2.0, 2.0, (n, 3))
    K = np.array([[800.0, 0, 320], [0, 800.0, 240], [0, 0, 1]])
    ang = rng.uniform(-0.3, 0.3, 3)
    cx, sx, cy, sy, cz, sz = np.cos(ang[0]), np.sin(ang[0]), np.cos(ang[1]), np.sin(ang[1]), np.cos(ang[2]), np.sin(ang[2])
    Rm = (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
          @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))
    P = K @ np.hstack([Rm, np.array([[0.1], [-0.2], [8.0]])])
    h = (P @ np.vstack([p3.T, np.ones(n)])).T
    p2 = h[:, :2] / h[:, 2:3] + noise * rng.standard_normal((n, 2))
    return p2.astype(np.float32), p3.astype(np.float32)
