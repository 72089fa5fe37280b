"""Inputs shared by tests/test_ps4_feat_ref.py (CPU, against the oracle) and tests/test_ps4_feat_paths_gpu.py (the
library against tests/_ps4_feat_ref.py): numpy only, no oracle and no library code.  Each builder plants what the
dispatch paths of harris.hip / sift.hip / match.hip can get wrong; the GPU tests assert that the planted thing is there."""
import numpy as np

F = np.float32

# ------------------------------------------------------------------------------------------------ NMS

SEAM_FIELD = (134, 200)
NMS_SIZES = [SEAM_FIELD, (40, 128), (35, 129), (34, 127), (5, 7), (1, 40), (40, 1), (70, 66)]
BETWEEN_FLOATS = 9.0 + 2.0 ** -30  # a double strictly between 9.0f and the next float
NMS_THRESHOLDS = [3.0, 0.0, -1.5, -np.inf, BETWEEN_FLOATS]

# Strict maxima of 9, pairwise more than 18 apart (so they survive every min_distance up to 18): both sides of the 16-row
# seam, of the 32-row seam, of the column seams at 64 and 128, and one whose neighbour beyond the seam is a NaN.
NMS_MAXIMA = [(15, 20), (16, 40), (31, 60), (32, 80), (52, 63), (72, 64), (15, 135), (40, 127), (60, 128), (115, 63)]
NMS_NAN_NEIGHBOUR = (115, 64)
# Tied pairs of 9s across the column seam and across each row seam: none of them is a corner for min_distance >= 1.
NMS_TIES = [((95, 63), (95, 64)), ((15, 105), (16, 105)), ((31, 165), (32, 165))]


def nms_field(rows, cols, seed, d=0):
    """Quantised responses 0..5 (exact ties everywhere), 2 % NaN, 1 % +inf, 1 % -inf, both zeros; 9s in the four image
    corners, at NMS_MAXIMA and at NMS_TIES (where they fit).  `d` is the min_distance the field is for: a +inf within d
    of a planted 9 would reject it, so those are replaced by 5 -- at every distance the planted maxima are corners
    and the rest of the field keeps its infinities."""
    rng = np.random.default_rng(seed)
    R = rng.integers(0, 6, (rows, cols)).astype(F)
    R[rng.random(R.shape) < 0.02] = np.nan
    R[rng.random(R.shape) < 0.01] = np.inf
    R[rng.random(R.shape) < 0.01] = -np.inf
    R[rng.random(R.shape) < 0.02] = -0.0
    planted = [(0, 0), (0, cols - 1), (rows - 1, 0), (rows - 1, cols - 1)] + NMS_MAXIMA + [p for t in NMS_TIES for p in t]
    for y, x in planted:
        if 0 <= y < rows and 0 <= x < cols:
            w = R[max(y - d, 0):y + d + 1, max(x - d, 0):x + d + 1]
            w[np.isposinf(w)] = 5
    for y, x in planted:
        if 0 <= y < rows and 0 <= x < cols:
            R[y, x] = 9
    if NMS_NAN_NEIGHBOUR[0] < rows and NMS_NAN_NEIGHBOUR[1] < cols:
        R[NMS_NAN_NEIGHBOUR] = np.nan
    return R


# ------------------------------------------------------------------------------------------------ descriptors

DESC_SIZES = [0.5, 4 / 3, 8 / 3, 4, 10, 12, 21.5, 40]  # hist_width = 3 * size / 2 is 2, 4, 6, 15, 18 for five of them


def special_keypoints(rows, cols):
    """Keypoints aimed at the places where the block pruning's argument is tight and at the geometry's edges."""
    kp = []
    cx, cy = cols // 2, rows // 2
    for a in range(-360, 721, 45):  # every multiple of 45 degrees, the floats beside it, above 360 and below -180
        for b in (np.nextafter(F(a), F(-1e9)), F(a), np.nextafter(F(a), F(1e9))):
            kp.append((cx, cy, 4, b))
    for s in DESC_SIZES:
        for a in (0, 45, 90, 30):
            kp.append((cx - 7, cy + 3, s, a))
    kp.append((cx, cy, 3 * max(rows, cols), 77))      # the radius is cut by the diagonal: the window covers the image
    kp.append((cx, cy, 1e6, 0))
    for x, y in ((0, 0), (cols - 1, 0), (0, rows - 1), (cols - 1, rows - 1), (-1, cy), (cols, cy), (cx, -1), (cx, rows),
                 (1, 1), (cols - 2, rows - 2), (-40, 10), (cx, rows + 30), (-1000, -1000)):
        kp.append((x, y, 8 / 3, 20))
        kp.append((x, y, 10, 90))
    for x, y in ((cx + 0.5, cy + 0.5), (cx + 1.5, cy - 0.5), (0.5, 0.5), (cols - 1.5, rows - 1.5), (-0.5, 2.5)):
        kp.append((x, y, 4, 45))                       # lrintf ties: half to even
    for bad in ((cx, cy, 0, 0), (cx, cy, -3, 10), (np.nan, cy, 10, 0), (cx, cy, 10, np.inf), (cx, cy, np.inf, 0),
                (cx, cy, np.nan, 1), (2e9, cy, 10, 0)):
        kp.append(bad)
    return np.array(kp, F)


def keypoint_list(rows, cols, n, seed):
    """special_keypoints, then random ones: positions up to 5 px outside, small sizes (the long lists stay cheap for
    numpy), angles in [-180, 540)."""
    head = special_keypoints(rows, cols)
    rng = np.random.default_rng(seed)
    m = max(n - len(head), 0)
    tail = np.stack([rng.uniform(-5, cols + 5, m), rng.uniform(-5, rows + 5, m), rng.choice([1.5, 8 / 3, 4, 6.5], m),
                     rng.uniform(-180, 540, m)], 1).astype(F)
    return np.concatenate([head, tail])[:n]


def poison(gx, gy):
    """NaN, +-inf and flat blocks in copies of the fields."""
    gx, gy = gx.copy(), gy.copy()
    rows, cols = gx.shape
    gx[rows // 4, cols // 4] = np.nan
    gy[rows // 2, cols // 2 + 9] = np.nan
    gy[rows // 2 + 20, cols // 3] = np.inf
    gx[rows // 5, 3 * cols // 4] = -np.inf
    gx[rows // 2 - 5:rows // 2 + 5, 30:60] = 0
    gy[rows // 2 - 5:rows // 2 + 5, 30:60] = 0
    return gx, gy


def magnitude_ramp(gx, gy):
    """The fields times 2^k, k stepping from -30 to 30 in vertical bands of 12 columns: windows that hold magnitudes far
    below the fixed point's unit beside ones at its top."""
    cols = gx.shape[1]
    k = (np.arange(cols) // 12 * 5) % 61 - 30
    s = np.ldexp(F(1), k).astype(F)
    return (gx * s).astype(F), (gy * s).astype(F)


# ------------------------------------------------------------------------------------------------ matching

kQT, kTT = 64, 128


def match_plan(nq, nt):
    """The launch shape the matcher documents (match.hip, micv_bf_knn2_dev): 64-query blocks, 128-row passes, the train
    set cut into slices of whole passes so that about 512 workgroups run -- 1024 once qblocks * passes >= 8192."""
    qblocks, passes = -(-nq // kQT), -(-nt // kTT)
    want = 1024 if qblocks * passes >= 8192 else 512
    slices = max(1, min(-(-want // qblocks), passes))
    slice_rows = -(-passes // slices) * kTT
    return {"qblocks": qblocks, "passes": passes, "want": want, "slice_rows": slice_rows, "slices": -(-nt // slice_rows)}


def match_sets(nq, nt, dim, seed):
    """Non-integer descriptors on both sides (the summation order decides the low bits), queries near a train row,
    every seventh one unrelated."""
    rng = np.random.default_rng(seed)
    t = (rng.normal(0, 40, (nt, dim)) + 100).astype(F)
    q = (t[rng.integers(0, nt, nq)] + rng.normal(0, 9, (nq, dim))).astype(F)
    q[::7] = (rng.normal(0, 40, (len(q[::7]), dim)) + 100).astype(F)
    return q, t


def plant_ties(q, t):
    """Groups of equal train rows (equal distances for every query) and, for each, a query equal to them:
      * rows 1, 9 (and 168): the ty groups 0 and 1 of the first pass (and ty 5 of the second);
      * rows 5, 131: one thread, two passes;
      * across a slice boundary, twice;
      * in slices of two and more passes, rows 17, 129 and rows 20, 130, 250: the thread of ty 0 carries rows 129 / 130
        of the second pass, and the fold of the ty groups pushes them BEFORE rows 17 / 20 of ty 2 -- the lower index
        arrives second, and only the tie-break by index puts it first.
    -> (groups, [(query row, [i0, i1] expected)])."""
    nq, nt = len(q), len(t)
    plan = match_plan(nq, nt)
    s = plan["slice_rows"]
    groups = []
    if nt > 9:
        groups.append([1, 9] + ([kTT + 40] if nt > kTT + 40 else []))
    if nt > kTT + 3:
        groups.append([5, kTT + 3])
    if plan["slices"] > 1:
        groups.append([s - 2, min(s + 1, nt - 1)])
        if nt > 2 * s:
            groups.append([s - 3, 2 * s])
    if s >= 2 * kTT and nt > 250:
        groups.append([17, kTT + 1])
        groups.append([20, kTT + 2, 250])
    if nt == 2:
        groups.append([0, 1])
    assert len({r for g in groups for r in g}) == sum(len(g) for g in groups)
    for g in groups:
        t[g[1:]] = t[g[0]]
    expect = []
    for k, g in enumerate(groups):
        if k < nq:
            q[k] = t[g[0]]
            expect.append((k, sorted(g)[:2]))
    return groups, expect


def poison_sets(q, t):
    q, t = q.copy(), t.copy()
    t[0, 0] = np.nan                              # a NaN distance for every query
    if len(t) > 3:
        t[3, -1] = np.inf                         # an infinite one
    if len(q) > 2:
        q[2, 0] = np.nan                          # a query with no distance at all
    if len(q) > 4:
        q[4, -1] = -np.inf
    return q, t
