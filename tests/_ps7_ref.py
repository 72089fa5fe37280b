"""Exact numpy restatement of ps7's second half as include/mi_cv.h states it: moments::centralMoment (Moments.cpp),
cv::ml::KNearest + matching::{naiveConfusionMatrix, confusionMatrix} (Matching.cpp) and mhiHelper's loop
(Solution.cpp:16-101, through tests/_mhi_ref.py, the oracle-free restatement of MotionHistory.cpp / .cu).  Every f32 step is a numpy float32 operation (IEEE,
no FMA); every sum is math.fsum (the exact sum rounded once to double) then float32."""
import math

import numpy as np

import _mhi_ref as mhi_ref

QNAN = np.uint32(0x7FC00000).view(np.float32)
FLT_MAX_BITS = 0x7F7FFFFF
PS7_ORDERS = ((2, 0), (0, 2), (1, 2), (2, 1), (2, 2), (3, 0), (0, 3))


def canon(a):
    """NaNs -> the canonical quiet NaN (mi_cv.h: output NaNs)."""
    a = np.array(a, dtype=np.float32, copy=True)
    a[np.isnan(a)] = QNAN
    return a


def bits(a):
    return np.ascontiguousarray(canon(a)).view(np.uint32)


# ---------------------------------------------------------------------------------------------------- moments ----

def exact_sum(terms):
    """S: flags first (NaN, or +Inf with -Inf -> NaN; +-Inf), else fsum (exact -> double) -> f32."""
    t = np.asarray(terms, dtype=np.float32).ravel()
    nan, pinf, ninf = bool(np.isnan(t).any()), bool((t == np.inf).any()), bool((t == -np.inf).any())
    if nan or (pinf and ninf):
        return QNAN
    if pinf:
        return np.float32(np.inf)
    if ninf:
        return np.float32(-np.inf)
    with np.errstate(over="ignore"):
        return np.float32(math.fsum(t.astype(np.float64).tolist()))


def ipow(d, p):
    """cv::pow on f32 with an integer power: 0 -> 1, 1 -> copy, else iPow_'s loop."""
    d = np.asarray(d, dtype=np.float32)
    if p == 0:
        return np.ones_like(d)
    if p == 1:
        return d.copy()
    with np.errstate(over="ignore", invalid="ignore"):
        a, b = np.ones_like(d), d.copy()
        while p > 1:
            if p & 1:
                a = a * b
            b = b * b
            p >>= 1
        return a * b


def pixel_values(img, norm_inf=False):
    img = np.asarray(img)
    if norm_inf:
        assert img.dtype == np.uint8
        m = int(img.max())
        s = np.float32(1.0 / m) if m > 0 else np.float32(0.0)  # normalize: 1.0 / max in double, 0 when max == 0
        return img.astype(np.float32) * s
    return img.astype(np.float32)


def eta_denominator(m00, pq):
    """pow(M00, 1 + (p+q)/2) by IEEE basic operations: left-to-right product, times sqrt(d) for a half."""
    d = np.float64(np.float32(m00))
    with np.errstate(all="ignore"):
        P = d
        for _ in range(1, 1 + pq // 2):
            P = P * d
        if pq & 1:
            P = P * np.sqrt(d)
    return P


def raw_moments(img, norm_inf=False):
    v = pixel_values(img, norm_inf)
    rows, cols = v.shape
    x = np.broadcast_to(np.arange(cols, dtype=np.float32)[None, :], v.shape)
    y = np.broadcast_to(np.arange(rows, dtype=np.float32)[:, None], v.shape)
    with np.errstate(all="ignore"):
        m00, m10, m01 = exact_sum(v), exact_sum(x * v), exact_sum(y * v)
    return v, x, y, m00, m10, m01


def central_moments(img, orders=PS7_ORDERS, norm_inf=False, y_fixed=False):
    """-> (mu [n], eta [n], raw [3]) float32, canonical NaNs."""
    v, x, y, m00, m10, m01 = raw_moments(img, norm_inf)
    with np.errstate(all="ignore"):
        xbar, ybar = np.float32(m10) / np.float32(m00), np.float32(m01) / np.float32(m00)
        dx = x - xbar
        dy = (y if y_fixed else x) - ybar  # Moments.cpp:59: cv::pow(xFull - yBar, q, yPow)
    mu, eta = [], []
    for p, q in orders:
        with np.errstate(all="ignore"):
            t = ipow(dy, q) * (ipow(dx, p) * v)
            u = exact_sum(t)
            e = np.float32(np.float64(u) / eta_denominator(m00, p + q))
        mu.append(u)
        eta.append(e)
    return canon(mu), canon(eta), canon([m00, m10, m01])


def opencv_order_sum(terms):
    """cv::sum's order as recalled (sum_ with a double accumulator): each group of four consecutive values of a row is
    added in f32, ((a + b) + c) + d, and that partial into a serial double; the rest of the row one by one.  This is
    the unpinned order the exact sum stands in for."""
    t = np.atleast_2d(np.asarray(terms, dtype=np.float32))
    acc = 0.0
    n4 = (t.shape[1] // 4) * 4
    with np.errstate(all="ignore"):
        part = ((t[:, 0:n4:4] + t[:, 1:n4:4]) + t[:, 2:n4:4]) + t[:, 3:n4:4]
    for r in range(t.shape[0]):
        for val in part[r].tolist():
            acc += val
        for val in t[r, n4:].tolist():
            acc += val
    return np.float32(acc)


# ------------------------------------------------------------------------------------------------------ k-NN ----

def knn_distances(test, train, f64=False):
    """[ntest, ntrain] f32 distances in knearest.cpp's order (mi_cv.h)."""
    test = np.asarray(test, np.float32)
    train = np.asarray(train, np.float32)
    d = test.shape[1]
    U, V = test[:, None, :], train[None, :, :]
    with np.errstate(all="ignore"):
        if f64:
            s = np.zeros((test.shape[0], train.shape[0]), np.float64)
            i = 0
            while i + 4 <= d:
                t = [(U[:, :, i + j] - V[:, :, i + j]).astype(np.float64) for j in range(4)]
                s = s + (((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]) + t[3] * t[3])
                i += 4
            for j in range(i, d):
                t0 = (U[:, :, j] - V[:, :, j]).astype(np.float64)
                s = s + t0 * t0
            return s.astype(np.float32)
        s = np.zeros((test.shape[0], train.shape[0]), np.float32)
        i = 0
        while i + 4 <= d:
            t = [U[:, :, i + j] - V[:, :, i + j] for j in range(4)]
            s = s + (((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]) + t[3] * t[3])
            i += 4
        for j in range(i, d):
            t0 = U[:, :, j] - V[:, :, j]
            s = s + t0 * t0
        return s


def vote(responses):
    """Bubble sort ascending, longest run, the first (smallest) on a tie; [] -> 0."""
    rp = sorted(int(r) for r in responses)
    if not rp:
        return 0
    result, prev, best = rp[0], 0, 0
    for j in range(1, len(rp) + 1):
        if j == len(rp) or rp[j] != rp[j - 1]:
            if best < j - prev:
                best, result = j - prev, rp[j - 1]
            prev = j
    return result


def knn_select(dist_row, labels, eligible, k):
    """The k slots after inserting every eligible row in order: the k smallest distance bits, earlier rows first on
    ties; bits >= FLT_MAX's (+Inf, NaN, FLT_MAX itself) never enter; k = min(k, eligible rows); empty slots vote 0."""
    b = np.asarray(dist_row, np.float32).view(np.int32).astype(np.int64)
    b = np.where(np.isnan(dist_row), 0x7FC00000, b)
    idx = np.nonzero(eligible)[0]
    ke = min(k, idx.size)
    cand = idx[b[idx] < FLT_MAX_BITS]
    order = cand[np.argsort(b[cand], kind="stable")][:ke]
    resp = [int(labels[j]) for j in order] + [0] * (ke - order.size)
    return resp


def knn_predict(train, labels, test, k=3, f64=False, block=256):
    train = np.asarray(train, np.float32)
    out = np.empty(len(test), np.int32)
    everyone = np.ones(train.shape[0], bool)
    for b0 in range(0, len(test), block):
        D = knn_distances(test[b0:b0 + block], train, f64)
        for r in range(D.shape[0]):
            out[b0 + r] = vote(knn_select(D[r], labels, everyone, k))
    return out


def knn_folds(features, labels, groups=None, num_groups=0, k=3, f64=False, block=256):
    """Each row's vote in its own fold (leave-one-out when groups is None); rows in no fold get 0."""
    f = np.asarray(features, np.float32)
    n = f.shape[0]
    labels = np.asarray(labels).ravel()
    pred = np.zeros(n, np.int32)
    g = None if groups is None else np.asarray(groups).ravel()
    for b0 in range(0, n, block):
        D = knn_distances(f[b0:b0 + block], f, f64)
        for r in range(D.shape[0]):
            i = b0 + r
            if g is None:
                elig = np.ones(n, bool)
                elig[i] = False
            else:
                if not 1 <= g[i] <= num_groups:
                    continue
                elig = g != g[i]
            pred[i] = vote(knn_select(D[r], labels, elig, k))
    return pred


def confusion_from(pred, labels, groups, num_labels, num_groups):
    """The matrices (Matching.cpp), f32 throughout, and the count of rows left out."""
    labels = np.asarray(labels).ravel()
    nm = num_groups if groups is not None else 1
    conf = np.zeros((nm, num_labels, num_labels), np.float32)
    cnt = np.zeros((nm, num_labels), np.float32)
    left = 0
    for i in range(len(labels)):
        g = 1 if groups is None else int(groups[i])
        if not 1 <= g <= nm:
            continue
        e, r = int(labels[i]), int(pred[i])
        if not (1 <= e <= num_labels and 1 <= r <= num_labels):
            left += 1
            continue
        conf[g - 1, e - 1, r - 1] += np.float32(1)
        cnt[g - 1, e - 1] += np.float32(1)
    with np.errstate(all="ignore"):
        c = cnt[:, :, None]
        mats = np.where(c != 0, conf / np.where(c != 0, c, 1), np.float32(0)).astype(np.float32)
    if groups is None:
        return mats, left
    avg = np.zeros((num_labels, num_labels), np.float32)
    for m in mats:
        avg = avg + m
    avg = avg * np.float32(1.0 / num_groups)
    return np.concatenate([mats, avg[None]]).astype(np.float32), left


def naive_confusion(features, labels, num_labels=3, k=3, f64=False):
    pred = knn_folds(features, labels, None, 0, k, f64)
    mats, left = confusion_from(pred, labels, None, num_labels, 0)
    return mats[0], pred, left


def group_confusion(features, labels, groups, num_groups, num_labels=3, k=3, f64=False):
    pred = knn_folds(features, labels, groups, num_groups, k, f64)
    mats, left = confusion_from(pred, labels, groups, num_labels, num_groups)
    return mats, pred, left


# ------------------------------------------------------------------------------------------------------- MHI ----

def history_seq(frames, thresh, blur, sigma, tau, save):
    """mhiHelper: the history after update j for every j in save."""
    return mhi_ref.history_seq(frames, thresh, blur, sigma, tau, list(save))


def mhi_energy(mhi):
    """mhi::energyFromHistory."""
    return mhi_ref.energy(mhi)


# --------------------------------------------------------------------------------------------- synthetic ps7 ----

def action_video(seed, action, nframes, rows=120, cols=160):
    """A textured background and a bright blob that moves by action: 1 left-right, 2 up-down, 3 grows."""
    rng = np.random.default_rng(seed)
    bg = rng.integers(20, 60, (rows, cols)).astype(np.float32)
    yy, xx = np.mgrid[0:rows, 0:cols].astype(np.float32)
    cy0, cx0 = rows * (0.4 + 0.2 * rng.random()), cols * (0.4 + 0.2 * rng.random())
    out = np.empty((nframes, rows, cols), np.uint8)
    for f in range(nframes):
        ph = f / max(nframes - 1, 1)
        cy, cx, r = cy0, cx0, rows * 0.12
        if action == 1:
            cx = cx0 + cols * 0.25 * math.sin(2 * math.pi * ph)
        elif action == 2:
            cy = cy0 + rows * 0.25 * math.sin(2 * math.pi * ph)
        else:
            r = rows * (0.08 + 0.12 * ph)
        blob = 200.0 * ((yy - cy) ** 2 + (xx - cx) ** 2 < r * r)
        out[f] = np.clip(bg + blob + rng.normal(0, 2, (rows, cols)), 0, 255).astype(np.uint8)
    return out
