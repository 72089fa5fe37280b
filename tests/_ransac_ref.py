"""Exact numpy restatement of ransac::solve (ProblemSets/ps4_cpp/lib/RANSAC.cpp:27-152) with the
arithmetic DESIGN.md section 2 ("RANSAC") fixes.  Written from RANSAC.cpp and those decisions alone;
imports no library code.  Samples / permutations come from the caller, so either sampler drives it.

- hypotheses: translation in float32; similarity = hal::LU32f on the 4x4 float system (partial
  pivoting, first row of largest |a|, failure below 10 * FLT_EPSILON -> x = 0, no fma); affine =
  Pprime * P.inv() with the 3x3 closed-form inverse in double (rounded to float, zeros when
  det == 0) and a gemm that accumulates in double, k ascending from the first product, one rounding.
- point test: testB by the same gemm rule; both points through cvRound (half to even, INT_MIN for
  NaN / out of range); int32 wrap-around differences, squares, sum; float(sqrt(double(sum))) <=
  float(thresh); a negative sum is NaN, an outlier.
- consensus: positions idx >= k of the current permutation; ratio double(count) / double(N); best on
  strict '>'; stop when the best ratio reaches min_ratio or at max_iters; the returned transform is
  the LAST iteration's.
"""
import numpy as np

F32 = np.float32
INT_MIN = -(1 << 31)
LU_EPS = F32(F32(1.1920928955078125e-07) * F32(10))  # FLT_EPSILON * 10 in float
TRANSLATION, SIMILARITY, AFFINE = 1, 2, 3


def cv_round(v):
    """cvRound(float) as cvtss2si: round half to even; INT_MIN for NaN and out-of-range."""
    v = np.asarray(v, np.float32)
    ok = (v >= F32(-2147483648.0)) & (v < F32(2147483648.0))
    r = np.rint(np.where(ok, v, F32(0))).astype(np.int64)
    return np.where(ok, r, INT_MIN)


def wrap32(x):
    return ((np.asarray(x, np.int64) + (1 << 31)) % (1 << 32)) - (1 << 31)


def lu4_solve(A, b):
    """hal::LU32f on a batch: A (I, 4, 4) float32, b (I, 4) float32 -> x (I, 4); 0 where it fails."""
    A = np.array(A, np.float32)
    b = np.array(b, np.float32)
    m = A.shape[0]
    r = np.arange(m)
    fail = np.zeros(m, bool)
    with np.errstate(all="ignore"):
        for i in range(4):
            k = np.full(m, i)
            for j in range(i + 1, 4):
                k = np.where(np.abs(A[r, j, i]) > np.abs(A[r, k, i]), j, k)
            fail |= np.abs(A[r, k, i]) < LU_EPS
            ri, rk = A[r, i].copy(), A[r, k].copy()
            A[r, i], A[r, k] = rk, ri
            bi, bk = b[r, i].copy(), b[r, k].copy()
            b[r, i], b[r, k] = bk, bi
            d = F32(-1) / A[:, i, i]
            for j in range(i + 1, 4):
                alpha = A[:, j, i] * d
                for c in range(i + 1, 4):
                    A[:, j, c] = A[:, j, c] + alpha * A[:, i, c]
                b[:, j] = b[:, j] + alpha * b[:, i]
        for i in range(3, -1, -1):
            s = b[:, i].copy()
            for c in range(i + 1, 4):
                s = s - A[:, i, c] * b[:, c]
            b[:, i] = s / A[:, i, i]
    return np.where(fail[:, None], F32(0), b).astype(np.float32)


def inv3(P):
    """cv::invert of 3x3 CV_32F (closed form, double): P (I, 3, 3) float32 -> (I, 3, 3) float32."""
    p = np.asarray(P, np.float32).astype(np.float64)
    a = lambda i, j: p[:, i, j]  # noqa: E731
    d = (a(0, 0) * (a(1, 1) * a(2, 2) - a(1, 2) * a(2, 1)) - a(0, 1) * (a(1, 0) * a(2, 2) - a(1, 2) * a(2, 0))
         + a(0, 2) * (a(1, 0) * a(2, 1) - a(1, 1) * a(2, 0)))
    ok = d != 0.0
    with np.errstate(all="ignore"):
        d = 1.0 / np.where(ok, d, 1.0)
        cof = [[a(1, 1) * a(2, 2) - a(1, 2) * a(2, 1), a(0, 2) * a(2, 1) - a(0, 1) * a(2, 2),
                a(0, 1) * a(1, 2) - a(0, 2) * a(1, 1)],
               [a(1, 2) * a(2, 0) - a(1, 0) * a(2, 2), a(0, 0) * a(2, 2) - a(0, 2) * a(2, 0),
                a(0, 2) * a(1, 0) - a(0, 0) * a(1, 2)],
               [a(1, 0) * a(2, 1) - a(1, 1) * a(2, 0), a(0, 1) * a(2, 0) - a(0, 0) * a(2, 1),
                a(0, 0) * a(1, 1) - a(0, 1) * a(1, 0)]]
        out = np.stack([np.stack([(cof[i][j] * d).astype(np.float32) for j in range(3)], -1) for i in range(3)], -2)
    return np.where(ok[:, None, None], out, F32(0)).astype(np.float32)


def gemm_row(row, cols):
    """One output element per column: double accumulation, k ascending from the first product."""
    s = row[..., 0].astype(np.float64) * cols[..., 0, :].astype(np.float64)
    s = s + row[..., 1].astype(np.float64) * cols[..., 1, :].astype(np.float64)
    s = s + row[..., 2].astype(np.float64) * cols[..., 2, :].astype(np.float64)
    return s.astype(np.float32)


def hypotheses(ttype, q):
    """q (I, k, 4) float32 sample points (x, y, x', y') -> (I, 6) float32 row-major 2x3 transforms."""
    q = np.asarray(q, np.float32)
    m = q.shape[0]
    one, zero = np.ones(m, np.float32), np.zeros(m, np.float32)
    if ttype == TRANSLATION:
        return np.stack([one, zero, q[:, 0, 2] - q[:, 0, 0], zero, one, q[:, 0, 3] - q[:, 0, 1]], -1)
    if ttype == SIMILARITY:
        x1, y1, x2, y2 = q[:, 0, 0], q[:, 0, 1], q[:, 1, 0], q[:, 1, 1]
        A = np.stack([np.stack([x1, -y1, one, zero], -1), np.stack([y1, x1, zero, one], -1),
                      np.stack([x2, -y2, one, zero], -1), np.stack([y2, x2, zero, one], -1)], -2)
        b = np.stack([q[:, 0, 2], q[:, 0, 3], q[:, 1, 2], q[:, 1, 3]], -1)
        x = lu4_solve(A, b)
        return np.stack([x[:, 0], -x[:, 1], x[:, 2], x[:, 1], x[:, 0], x[:, 3]], -1)
    P = np.stack([q[:, :, 0], q[:, :, 1], np.ones((m, 3), np.float32)], -2)
    Pp = np.stack([q[:, :, 2], q[:, :, 3]], -2)
    I = inv3(P)
    return np.concatenate([gemm_row(Pp[:, 0, None, :], I), gemm_row(Pp[:, 1, None, :], I)], -1).reshape(m, 6)


def passes(t, src, dst, thresh, round_points=True):
    """Point test of every (hypothesis, point): t (I, 6), src / dst (N, 2) -> bool (I, N)."""
    t = np.asarray(t, np.float32).astype(np.float64)[:, :, None]
    x = np.asarray(src, np.float32)[:, 0].astype(np.float64)[None]
    y = np.asarray(src, np.float32)[:, 1].astype(np.float64)[None]
    bx = ((t[:, 0] * x + t[:, 1] * y) + t[:, 2]).astype(np.float32)
    by = ((t[:, 3] * x + t[:, 4] * y) + t[:, 5]).astype(np.float32)
    dst = np.asarray(dst, np.float32)
    with np.errstate(all="ignore"):
        if not round_points:  # mutation: Point2f distances
            d = np.sqrt((bx - dst[None, :, 0]) ** 2 + (by - dst[None, :, 1]) ** 2).astype(np.float32)
            return d <= F32(thresh)
        dx = wrap32(cv_round(bx) - cv_round(dst[None, :, 0]))
        dy = wrap32(cv_round(by) - cv_round(dst[None, :, 1]))
        s = wrap32(wrap32(dx * dx) + wrap32(dy * dy))
        dist = np.sqrt(np.where(s >= 0, s, -1).astype(np.float64)).astype(np.float32)  # NaN when negative
    return dist <= F32(thresh)


def counts_for_samples(src, dst, samples, ttype, thresh, block=1 << 22):
    """Inlier count of every iteration: points whose index is not in the iteration's sample."""
    src = np.asarray(src, np.float32).reshape(-1, 2)
    dst = np.asarray(dst, np.float32).reshape(-1, 2)
    samples = np.asarray(samples, np.int64).reshape(-1, ttype)
    n = src.shape[0]
    q = np.concatenate([src[samples], dst[samples]], -1)
    t = hypotheses(ttype, q)
    counts = np.empty(len(samples), np.int64)
    step = max(1, block // max(n, 1))
    for i0 in range(0, len(samples), step):
        ok = passes(t[i0:i0 + step], src, dst, thresh)
        rows = np.arange(ok.shape[0])[:, None]
        excl = np.zeros_like(ok)
        excl[rows, samples[i0:i0 + step]] = True
        counts[i0:i0 + step] = (ok & ~excl).sum(1)
    return t, counts


def solve_samples(src, dst, samples, ttype, thresh, max_iters, min_ratio):
    """The solve on explicit samples (iters x k): what micv_ransac_solve_* return.  dict of
    iterations, best_iter, best_count, t_last (2x3), t_best (2x3), mask (N,) uint8."""
    src = np.asarray(src, np.float32).reshape(-1, 2)
    dst = np.asarray(dst, np.float32).reshape(-1, 2)
    n = src.shape[0]
    samples = np.asarray(samples, np.int64).reshape(-1, ttype)[:max_iters]
    zero = np.zeros((2, 3), np.float32)
    if not (0.0 < min_ratio):
        return dict(iterations=0, best_iter=-1, best_count=0, t_last=zero, t_best=zero, mask=np.zeros(n, np.uint8))
    t, counts = counts_for_samples(src, dst, samples, ttype, thresh)
    hit = np.nonzero(counts.astype(np.float64) / float(n) >= min_ratio)[0]
    last = int(hit[0]) if len(hit) else max_iters - 1
    best = int(np.argmax(counts[:last + 1]))  # first maximum
    ok = passes(t[best:best + 1], src, dst, thresh)[0]
    ok[samples[best]] = False
    return dict(iterations=last + 1, best_iter=best, best_count=int(counts[best]), t_last=t[last].reshape(2, 3),
                t_best=t[best].reshape(2, 3), mask=ok.astype(np.uint8), counts=counts[:last + 1])


def solve_as_written(src, dst, ttype, thresh, max_iters, min_ratio, shuffle, mutations=()):
    """RANSAC.cpp's loop, statement by statement.  shuffle(list) permutes the persistent index
    list in place (std::shuffle with the shared engine).  Returns (transform 2x3 or None,
    consensusSet positions, ratio, iterations).  `mutations` switch in wrong readings of the source
    for the tests that must tell them apart: 'best_ge', 'count_sample', 'float_dist', 'reset_perm',
    'return_best', 'stop_strict'."""
    src = np.asarray(src, np.float32).reshape(-1, 2)
    dst = np.asarray(dst, np.float32).reshape(-1, 2)
    n, k = src.shape[0], ttype
    indices = list(range(n))
    consensus, ratio, iterations, transform, best_t = [], 0.0, 0, None, None
    while (ratio <= min_ratio if "stop_strict" in mutations else ratio < min_ratio) and iterations < max_iters:
        if "reset_perm" in mutations:
            indices = list(range(n))
        shuffle(indices)
        perm = np.asarray(indices, np.int64)
        q = np.concatenate([src[perm[:k]], dst[perm[:k]]], -1)[None]
        transform = hypotheses(ttype, q)[0]
        first = 0 if "count_sample" in mutations else k
        pos = np.arange(first, n)
        ok = passes(transform[None], src[perm[pos]], dst[perm[pos]], thresh,
                    round_points="float_dist" not in mutations)[0]
        cur = [int(p) for p in pos[ok]]
        cur_ratio = float(len(cur)) / float(n)
        if (cur_ratio >= ratio) if "best_ge" in mutations else (cur_ratio > ratio):
            ratio, consensus, best_t = cur_ratio, cur, transform
        iterations += 1
    out = best_t if "return_best" in mutations else transform
    return (None if out is None else out.reshape(2, 3)), consensus, ratio, iterations


def splitmix64(x):
    m = (1 << 64) - 1
    z = (x + 0x9E3779B97F4A7C15) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return z ^ (z >> 31)


def device_samples(seed, n, k, iters):
    """The counter-based sampler of micv_ransac_solve_matches_dev (include/mi_cv.h)."""
    out = np.empty((iters, k), np.int64)
    for i in range(iters):
        s = []
        for j in range(k):
            a = 0
            while True:
                r = splitmix64(seed ^ ((i << 32) | (j << 30) | a))
                idx = ((r >> 32) * n) >> 32
                if idx not in s:
                    break
                a += 1
            s.append(idx)
        out[i] = s
    return out
