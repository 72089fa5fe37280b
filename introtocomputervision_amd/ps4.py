"""The ps4 driver of the reference (ProblemSets/ps4_cpp/src/Solution.cpp) around `harris`, `match` and `ransac`, on the
device: drawDots (:59-69), cv::hconcat, cv::drawKeypoints with random colours (:147-158), the match lines (:190-207) and
the consensus lines (:240-250), harrisHelper's three pictures and siftHelper's / ransacHelper's panels as one call each.
numpy arrays take the `_host` entry points, torch CUDA tensors the `_dev` ones on the current stream; device results,
counts and the generator state stay on the device and nothing synchronises.  The drawing equals the host loops of
shim/micv_ps4.hpp byte for byte (include/mi_cv.h, "ps4: driver")."""
import ctypes as C

import numpy as np

from . import _buf as B
from ._capi import DEPTH_8U, DEPTH_32F, PS4_NO_GLYPHS, check, lib
from .lk import _ctx_for
from .ps5 import _batched, _frame

MATCH_SEED = 12345  # cv::RNG rng(12345), Solution.cpp:194, :243
SIFT_WINDOW_SIZE = 10  # Solution.cpp:138
MASK64 = (1 << 64) - 1


def _same_side(ref, *others):
    for a in others:
        if a is not None and B.is_dev(a) != B.is_dev(ref):
            raise ValueError("arguments must all be numpy arrays or all CUDA tensors")
        if a is not None and B.is_dev(a) and a.device != ref.device:
            raise ValueError("arguments must live on one device")


def _list(a, dt, width, name, like):
    """An [n, width] list of `dt`, contiguous -> (array, n)."""
    if B.is_dev(like):
        import torch
        want = getattr(torch, np.dtype(dt).name)
        if not (B.is_dev(a) and a.is_cuda and a.dtype == want and a.is_contiguous()):
            raise ValueError(f"{name}: need a contiguous {np.dtype(dt).name} CUDA tensor")
        a = a.reshape(-1, width) if width > 1 else a.reshape(-1)
    else:
        a = np.ascontiguousarray(a, dt).reshape((-1, width) if width > 1 else (-1,))
    return a, int(a.shape[0])


def _count_word(count, n, like, name):
    """Device side: the count as a 1-element int64 CUDA tensor (None: the list's length)."""
    import torch
    if count is None:
        return torch.full((1,), n, dtype=torch.int64, device=like.device)
    if not (B.is_dev(count) and count.is_cuda and count.dtype == torch.int64 and count.numel() == 1):
        raise ValueError(f"{name}: need a 1-element int64 CUDA tensor (the count the chain left on the device)")
    return count


def rngState(like, state=0):
    """The generator word of drawKeypoints / matchPanels: a 1-element uint64 array on `like`'s side (0 = cv::theRNG()'s
    start).  The calls advance it in place."""
    if B.is_dev(like):
        import torch
        v = int(state) & MASK64
        return torch.tensor([v - (1 << 64) if v >> 63 else v], dtype=torch.int64, device=like.device)
    return np.array([int(state) & MASK64], np.uint64)


def stateValue(state):
    """The word of rngState as a Python int (synchronises for a device word)."""
    return int(state.cpu().numpy().view(np.uint64)[0]) if B.is_dev(state) else int(state[0])


def _state_arg(state, like):
    if B.is_dev(like):
        import torch
        if not (B.is_dev(state) and state.is_cuda and state.dtype == torch.int64 and state.numel() == 1):
            raise ValueError("rng_state: need the 1-element CUDA word rngState() makes")
        return state.data_ptr()
    if not (isinstance(state, np.ndarray) and state.dtype == np.uint64 and state.size == 1):
        raise ValueError("rng_state: need the 1-element uint64 array rngState() makes")
    return state.ctypes.data_as(C.POINTER(C.c_uint64))


def drawDots(img, corners, ctx=None):
    """drawDots (Solution.cpp:59-69): the grey image (float32 or uint8) as [rows, cols, 3] uint8, (0, 0, 255) where the
    normalised corner map is non-zero."""
    rows, cols, cn, depth, pitch = _frame(img, "img")
    if cn != 1 or len(img.shape) != 2:
        raise ValueError("img: a grey image expected")
    B.check2d(corners, np.float32, name="corners")
    _same_side(img, corners)
    if tuple(corners.shape) != (rows, cols):
        raise ValueError("img and corners differ in size")
    out = B.empty_like_shape(img, (rows, cols, 3), np.uint8)
    args = (_ctx_for(img, ctx).handle, B.ptr(img), depth, rows, cols, pitch, B.ptr(corners), B.stride_bytes(corners), B.ptr(out), cols * 3)
    if B.is_dev(img):
        check(lib.micv_draw_dots_dev(*args, B.stream_of(img)))
    else:
        check(lib.micv_draw_dots_host(*args))
    return out


def hconcat(a, b, ctx=None):
    """cv::hconcat of two uint8 images of equal rows, both [rows, cols] or both [rows, cols, 3]; pitched views are fine."""
    ra, ca, cna, da, pa = _frame(a, "a")
    rb, cb, cnb, db, pb = _frame(b, "b")
    _same_side(a, b)
    if da != DEPTH_8U or db != DEPTH_8U or cna != cnb or cna not in (1, 3) or ra != rb or len(a.shape) != len(b.shape):
        raise ValueError("hconcat: two uint8 images of equal rows and 1 or 3 channels expected")
    out = B.empty_like_shape(a, (ra, ca + cb) + ((3,) if len(a.shape) == 3 else ()), np.uint8)
    args = (_ctx_for(a, ctx).handle, B.ptr(a), pa, ca, B.ptr(b), pb, cb, ra, cna, B.ptr(out), (ca + cb) * cna)
    if B.is_dev(a):
        check(lib.micv_hconcat_dev(*args, B.stream_of(a)))
    else:
        check(lib.micv_hconcat_host(*args))
    return out


def drawKeypoints(img, keypoints, count=None, rng_state=None, canvas=None, x0=0, cols=None, ctx=None):
    """cv::drawKeypoints(img, keypoints, out, Scalar::all(-1), DRAW_RICH_KEYPOINTS): img is an 8-bit grey or BGR image (or
    None: draw on what the canvas window holds), keypoints [n, 4] (x, y, size, angle) as harris.getKeypoints returns them.
    Device: `count` is the 1-element int64 CUDA word of the chain (None: every row).  `canvas` [rows, C, 3] with `x0`
    draws into the column window [x0, x0 + cols) of a wider image, clipped to it (cols: img's, or with img None the
    argument, by default the rest of the canvas); otherwise a new image is returned.
    `rng_state` (rngState()) continues a generator across calls and is advanced in place."""
    like = img if img is not None else canvas
    if like is None:
        raise ValueError("drawKeypoints: an image or a canvas expected")
    _same_side(like, img, canvas, keypoints if B.is_dev(like) else None)
    kp, n = _list(keypoints, np.float32, 4, "keypoints", like)
    if img is not None:
        rows, wcols, cn, depth, pitch = _frame(img, "img")
        if cols is not None and int(cols) != wcols:
            raise ValueError("cols: the window of an image is the image's width")
        cols = wcols
        if depth != DEPTH_8U or cn not in (1, 3):
            raise ValueError("img: uint8 with 1 or 3 channels expected")
    if canvas is None:
        canvas, x0 = B.empty_like_shape(img, (rows, cols, 3), np.uint8), 0
    _, crows, ccols, _, cstride = _batched(canvas, np.uint8, 3, "canvas")
    if len(canvas.shape) != 3:
        raise ValueError("canvas: need [rows, cols, 3]")
    if img is None:
        rows, cols, cn, pitch = crows, int(cols) if cols is not None else ccols - int(x0), 3, 0
    if crows != rows:
        raise ValueError("canvas and img differ in rows")
    state = rng_state if rng_state is not None else rngState(like)
    head = (_ctx_for(like, ctx).handle, B.ptr(img) if img is not None else None, cn, rows, cols, pitch, B.ptr(canvas), ccols, cstride, int(x0),
            B.ptr(kp) if n else None)
    if B.is_dev(like):
        check(lib.micv_draw_keypoints_dev(*head, _count_word(count, n, like, "count").data_ptr() if n else None, n,
                                          _state_arg(state, like), B.stream_of(like)))
    else:
        check(lib.micv_draw_keypoints_host(*head, n if count is None else max(0, min(int(count), n)), _state_arg(state, like)))
    return canvas


def drawMatchLines(canvas, kp_a, kp_b, matches, count=None, mask=None, x_offset=0, seed=MATCH_SEED, ctx=None):
    """The lines of siftHelper (:190-207) and, with `mask`, of ransacHelper (:240-250), on the [rows, cols, 3] uint8 canvas
    in place: match i from kp_a[q] to kp_b[t] + (x_offset, 0), the r-th drawn line with the r-th colour of cv::RNG(seed).
    Device: `count` is the ratio filter's 1-element int64 CUDA word (None: every row), `mask` a uint8 CUDA tensor with one
    entry per row of `matches` (the inlier mask of ransac.solve_matches goes straight in)."""
    _, rows, cols, _, stride = _batched(canvas, np.uint8, 3, "canvas")
    if len(canvas.shape) != 3:
        raise ValueError("canvas: need [rows, cols, 3]")
    _same_side(canvas, mask, *((kp_a, kp_b, matches) if B.is_dev(canvas) else ()))
    ka, na = _list(kp_a, np.float32, 4, "kp_a", canvas)
    kb, nb = _list(kp_b, np.float32, 4, "kp_b", canvas)
    m, n = _list(matches, np.int32, 2, "matches", canvas)
    if mask is not None:
        mask, nm = _list(mask, np.uint8, 1, "mask", canvas)
        if nm < n:
            raise ValueError("mask: one entry per match expected")
    head = (_ctx_for(canvas, ctx).handle, B.ptr(canvas), rows, cols, stride, B.ptr(ka) if na else None, na, B.ptr(kb) if nb else None, nb,
            B.ptr(m) if n else None)
    tail = (B.ptr(mask) if mask is not None and n else None, int(x_offset), int(seed) & MASK64)
    if B.is_dev(canvas):
        check(lib.micv_draw_match_lines_dev(*head, _count_word(count, n, canvas, "count").data_ptr(), n, *tail, B.stream_of(canvas)))
    else:
        check(lib.micv_draw_match_lines_host(*head, n if count is None else max(0, min(int(count), n)), *tail))
    return canvas


def harrisDisplay(img, sobelSize=3, windowSize=5, gaussianSigma=1.5, harrisScore=0.04, threshold=5e8, minDistance=5, capacity=None,
                  cpu_arithmetic=False, ctx=None):
    """harrisHelper (Solution.cpp:71-132) as one call on a float32 grey image.  Returns a dict: "gx", "gy", "response",
    "corners" (views of one [4, rows, cols] block), "locs" / "count" (device: `capacity` rows and a 1-element int64 CUDA
    word, nothing is read back; host: the list itself and an int), and the pictures "gradients" [rows, 2 cols],
    "response_u8" [rows, cols] and "dots" [rows, cols, 3]."""
    B.check2d(img, np.float32, name="img")
    rows, cols = (int(v) for v in img.shape)
    cap = int(capacity) if capacity is not None else rows * cols
    fields = B.empty_like_shape(img, (4, rows, cols))
    grad = B.empty_like_shape(img, (rows, 2 * cols), np.uint8)
    r8 = B.empty_like_shape(img, (rows, cols), np.uint8)
    dots = B.empty_like_shape(img, (rows, cols, 3), np.uint8)
    locs = B.zeros_like_shape(img, (max(cap, 1), 2), np.int32)
    cnt = B.zeros_like_shape(img, (1,), np.int64)
    args = (_ctx_for(img, ctx).handle, B.ptr(img), rows, cols, B.stride_bytes(img), int(sobelSize), int(windowSize), float(gaussianSigma),
            float(harrisScore), 1 if cpu_arithmetic else 0, float(threshold), int(minDistance), B.ptr(fields), B.ptr(locs), cap, B.ptr(cnt),
            B.ptr(grad), 2 * cols, B.ptr(r8), cols, B.ptr(dots), 3 * cols)
    if B.is_dev(img):
        check(lib.micv_ps4_harris_display_dev(*args, B.stream_of(img)))
        count = cnt
    else:
        check(lib.micv_ps4_harris_display_host(*args))
        count = int(cnt[0])
        locs = locs[:min(count, cap)]
    return {"gx": fields[0], "gy": fields[1], "response": fields[2], "corners": fields[3], "locs": locs[:cap], "count": count,
            "gradients": grad, "response_u8": r8, "dots": dots}


def matchPanels(img_a, img_b, kp_a, kp_b, matches, count_a=None, count_b=None, match_count=None, mask=None, glyphs=True,
                seed=MATCH_SEED, rng_state=None, want_keypoints=True, ctx=None):
    """The two pictures of siftHelper as one call on two grey uint8 images of equal rows: (keypoint panel, match panel).
    glyphs=False gives (None, ransacHelper's picture): the grey pair as BGR with the lines `mask` marks.  Counts as in
    drawKeypoints / drawMatchLines; rng_state continues across calls."""
    ra, ca, cna, da, pa = _frame(img_a, "img_a")
    rb, cb, cnb, db, pb = _frame(img_b, "img_b")
    if (cna, cnb, da, db) != (1, 1, DEPTH_8U, DEPTH_8U) or ra != rb:
        raise ValueError("matchPanels: two grey uint8 images of equal rows expected")
    dev = B.is_dev(img_a)
    _same_side(img_a, img_b, mask, *((kp_a, kp_b, matches) if dev else ()))
    ka, na = _list(kp_a, np.float32, 4, "kp_a", img_a)
    kb, nb = _list(kp_b, np.float32, 4, "kp_b", img_a)
    m, n = _list(matches, np.int32, 2, "matches", img_a)
    if mask is not None:
        mask, nm = _list(mask, np.uint8, 1, "mask", img_a)
        if nm < n:
            raise ValueError("mask: one entry per match expected")
    want_keypoints = want_keypoints and glyphs
    kpanel = B.empty_like_shape(img_a, (ra, ca + cb, 3), np.uint8) if want_keypoints else None
    mpanel = B.empty_like_shape(img_a, (ra, ca + cb, 3), np.uint8)
    state = rng_state if rng_state is not None else rngState(img_a)
    h = _ctx_for(img_a, ctx).handle
    head = (h, B.ptr(img_a), pa, ca, B.ptr(img_b), pb, cb, ra)
    tail = (B.ptr(mask) if mask is not None and n else None, 0 if glyphs else PS4_NO_GLYPHS, int(seed) & MASK64, _state_arg(state, img_a),
            B.ptr(kpanel) if want_keypoints else None, B.ptr(mpanel), (ca + cb) * 3)

    def p(a, k):
        return B.ptr(a) if k else None
    if dev:
        words = [_count_word(c, k, img_a, nm) for c, k, nm in ((count_a, na, "count_a"), (count_b, nb, "count_b"), (match_count, n, "match_count"))]
        check(lib.micv_ps4_match_panels_dev(*head, p(ka, na), words[0].data_ptr(), na, p(kb, nb), words[1].data_ptr(), nb, p(m, n),
                                            words[2].data_ptr(), n, *tail, B.stream_of(img_a)))
    else:
        def cl(c, k):
            return k if c is None else max(0, min(int(c), k))
        check(lib.micv_ps4_match_panels_host(*head, p(ka, na), cl(count_a, na), p(kb, nb), cl(count_b, nb), p(m, n), cl(match_count, n),
                                             *tail))
    return kpanel, mpanel


# ---- runProblem1 / 2 / 3 over the modules (device tensors in, device tensors out, no synchronisation) -------------

def _f32(img):
    import torch
    return img.to(torch.float32).contiguous() if B.is_dev(img) else np.ascontiguousarray(img, np.float32)


def runProblem1(img, params, capacity=4096, ctx=None):
    """harrisHelper on one 8-bit grey image with Config::Harris `params` (config.harris_params): harrisDisplay's dict."""
    return harrisDisplay(_f32(img), params["sobel_kernel_size"], params["window_size"], params["gaussian_sigma"], params["alpha"],
                         params["response_threshold"], params["min_distance"], capacity=capacity, ctx=ctx)


def runProblem2(img_a, img_b, params, capacity=4096, ratio=0.75, ctx=None):
    """harrisHelper on both images, then siftHelper: keypoints, descriptors, the 2-NN match and the ratio test, the
    keypoint panel and the match panel.  CUDA tensors only: every count stays a device word.  Returns a dict with the two
    harrisDisplay dicts ("a", "b"), "kp_a", "kp_b", "matches", "match_count", "keypoints_panel", "matches_panel"."""
    import torch
    from . import harris
    from .match import knnMatch2
    if not (B.is_dev(img_a) and B.is_dev(img_b)):
        raise ValueError("runProblem2: CUDA tensors expected (the host entry points serve the single steps)")
    out = {}
    kps, descs = [], []
    for key, img in (("a", img_a), ("b", img_b)):
        d = out[key] = runProblem1(img, params, capacity, ctx)
        kp = harris.getKeypoints(d["gx"], d["gy"], d["locs"], SIFT_WINDOW_SIZE, ctx=ctx)  # (rows past the count: pixel (0, 0))
        kps.append(kp)
        descs.append(harris.computeDescriptors(d["gx"], d["gy"], kp, ctx=ctx))
    # the train set is B's first `count` descriptors; rows past the count must never win: they are moved out of reach
    far = torch.arange(descs[1].shape[0], device=img_a.device).unsqueeze(1) >= out["b"]["count"]
    train = torch.where(far, torch.full_like(descs[1], float("inf")), descs[1])
    idx, dist = knnMatch2(descs[0], train, ctx=ctx)
    nq = idx.shape[0]
    dist = torch.where(torch.arange(nq, device=img_a.device).unsqueeze(1) >= out["a"]["count"], torch.full_like(dist, float("nan")), dist)
    matches = torch.zeros((nq, 2), dtype=torch.int32, device=img_a.device)
    distances = torch.empty((nq,), dtype=torch.float32, device=img_a.device)
    mcount = torch.zeros((1,), dtype=torch.int64, device=img_a.device)
    check(lib.micv_bf_ratio_filter_dev(_ctx_for(idx, ctx).handle, idx.data_ptr(), dist.data_ptr(), nq, float(ratio), matches.data_ptr(),
                                       distances.data_ptr(), nq, mcount.data_ptr(), B.stream_of(idx)))
    kpanel, mpanel = matchPanels(img_a, img_b, kps[0], kps[1], matches, out["a"]["count"], out["b"]["count"], mcount, ctx=ctx)
    out.update(kp_a=kps[0], kp_b=kps[1], matches=matches, match_count=mcount, keypoints_panel=kpanel, matches_panel=mpanel)
    return out


def _ransac_tail(out, img_a, img_b, whichTransform, ransacReprojThresh, maxIters, minConsensusRatio, seed, ctx):
    """ransacHelper and the registration tail on the dict of runProblem2 / runProblem2_8 (both runProblem3 forms end here)."""
    from . import ransac, warp
    tr, mask, st = ransac.solve_matches(out["kp_a"], out["kp_b"], out["matches"], out["match_count"], whichTransform,
                                        ransacReprojThresh, maxIters, minConsensusRatio, seed, ctx=ctx)
    _, panel = matchPanels(img_a, img_b, out["kp_a"], out["kp_b"], out["matches"], match_count=out["match_count"], mask=mask,
                           glyphs=False, ctx=ctx)
    blended = warp.registerBlend(img_a, img_b, tr[0], ctx=ctx) if ransac._type(whichTransform) != 1 else None
    out.update(transforms=tr, inlier_mask=mask, stats=st, consensus_panel=panel, blended=blended)
    return out


def runProblem2_8(img_a, img_b, params, capacity=4096, ratio=0.75, ctx=None):
    """runProblem2 on the two 8-bit pictures themselves, every list length a device word from the corners to the panels:
    harris.cornersFromImage8Batch with keypoints and without planes (two single calls when the pictures differ in size),
    harris.computeDescriptors8Batch, match.knnMatch2Counted, the ratio filter and the panels.  No float image, no gradient
    plane, no masking of rows past a count, nothing read back.  "a" / "b" are the corner dicts ("locs", "count",
    "keypoints"); "kp_a", "kp_b" (rows below the counts), "matches", "match_count" and the panels hold runProblem2's bytes."""
    import torch
    from . import harris
    from .match import knnMatch2Counted
    if not (B.is_dev(img_a) and B.is_dev(img_b)):
        raise ValueError("runProblem2_8: CUDA tensors expected (the host entry points serve the single steps)")
    for name, img in (("img_a", img_a), ("img_b", img_b)):
        if img.dtype != torch.uint8 or img.dim() != 2:
            raise ValueError(f"{name}: a [rows, cols] uint8 tensor expected")
    hp = dict(sobelSize=params["sobel_kernel_size"], windowSize=params["window_size"], gaussianSigma=params["gaussian_sigma"],
              harrisScore=params["alpha"], threshold=params["response_threshold"], minDistance=params["min_distance"], capacity=capacity,
              ctx=ctx, want_gradients=False, keypointSize=SIFT_WINDOW_SIZE)
    out = {}
    if tuple(img_a.shape) == tuple(img_b.shape):
        pair = torch.stack((img_a, img_b))
        d = harris.cornersFromImage8Batch(pair, **hp)
        desc = harris.computeDescriptors8Batch(pair, d["keypoints"], d["count"], ctx=ctx)
        for i, key in enumerate("ab"):
            out[key] = {"locs": d["locs"][i], "count": d["count"][i:i + 1], "keypoints": d["keypoints"][i]}
        descs = [desc[0], desc[1]]
    else:
        descs = []
        for key, img in (("a", img_a), ("b", img_b)):
            d = out[key] = harris.cornersFromImage8(img, lazy=True, **hp)
            descs.append(harris.computeDescriptors8(img, d["keypoints"], d["count"], ctx=ctx))
    kps = [out["a"]["keypoints"], out["b"]["keypoints"]]
    idx, dist = knnMatch2Counted(descs[0], descs[1], out["a"]["count"], out["b"]["count"], ctx=ctx)
    nq = idx.shape[0]
    matches = torch.zeros((nq, 2), dtype=torch.int32, device=img_a.device)
    distances = torch.empty((nq,), dtype=torch.float32, device=img_a.device)
    mcount = torch.zeros((1,), dtype=torch.int64, device=img_a.device)
    check(lib.micv_bf_ratio_filter_dev(_ctx_for(idx, ctx).handle, idx.data_ptr(), dist.data_ptr(), nq, float(ratio), matches.data_ptr(),
                                       distances.data_ptr(), nq, mcount.data_ptr(), B.stream_of(idx)))
    kpanel, mpanel = matchPanels(img_a, img_b, kps[0], kps[1], matches, out["a"]["count"], out["b"]["count"], mcount, ctx=ctx)
    out.update(kp_a=kps[0], kp_b=kps[1], matches=matches, match_count=mcount, keypoints_panel=kpanel, matches_panel=mpanel)
    return out


def runProblem3_8(img_a, img_b, params, whichTransform, ransacReprojThresh=3, maxIters=2000, minConsensusRatio=0.75, seed=0,
                  capacity=4096, ctx=None):
    """runProblem3 on runProblem2_8's chain: the same "transforms", "inlier_mask", "stats", "consensus_panel" and "blended"."""
    return _ransac_tail(runProblem2_8(img_a, img_b, params, capacity, ctx=ctx), img_a, img_b, whichTransform, ransacReprojThresh, maxIters,
                        minConsensusRatio, seed, ctx)


def runProblem3(img_a, img_b, params, whichTransform, ransacReprojThresh=3, maxIters=2000, minConsensusRatio=0.75, seed=0,
                capacity=4096, ctx=None):
    """runProblem2's chain, then ransacHelper on the device (ransac.solve_matches and the consensus lines of its inlier
    mask) and, for a similarity or affine transform, the registration tail (warp.registerBlend).  Adds "transforms",
    "inlier_mask", "stats", "consensus_panel" and "blended" (None for a translation) to runProblem2's dict."""
    return _ransac_tail(runProblem2(img_a, img_b, params, capacity, ctx=ctx), img_a, img_b, whichTransform, ransacReprojThresh, maxIters,
                        minConsensusRatio, seed, ctx)


def registerPairs8(imgs, pairs, params, whichTransform, ransacReprojThresh=3, maxIters=2000, minConsensusRatio=0.75, seed=0,
                   capacity=4096, ratio=0.75, ctx=None):
    """runProblem3_8's chain without its panels and its blend on a batch of pictures and a list of pairs of them, the number
    of launches independent of both: harris.cornersFromImage8Batch (keypoints, no planes), harris.computeDescriptors8Batch,
    match.matchPairs, ransac.solve_pairs and, for a similarity or affine type, warp.invertAffineTransform on row [0] of
    every pair and warp.warpAffineBatch of the pairs' second pictures.  imgs: [B, rows, cols] uint8 on the device; pairs: a
    list of (a, b), "chain" for (i, i + 1), "key" for (0, i), or an [npairs, 2] int32 CUDA tensor.  Returns the corner dict
    ("locs", "count", "keypoints") plus "pairs", "matches", "match_count", "transforms" [npairs, 2, 2, 3], "inlier_mask",
    "stats" and "warped" [npairs, rows, cols] (None for a translation).  Element p holds the bytes of runProblem3_8(imgs[a],
    imgs[b], ..., seed=ransac.pairSeed(seed, p)).  Nothing is read back."""
    import torch
    from . import harris, match, ransac, warp
    if not (B.is_dev(imgs) and imgs.is_cuda and imgs.dim() == 3 and imgs.dtype == torch.uint8):
        raise ValueError("imgs: a [B, rows, cols] uint8 CUDA tensor expected")
    nimg = int(imgs.shape[0])
    if isinstance(pairs, str):
        if pairs not in ("chain", "key") or nimg < 2:
            raise ValueError('pairs: "chain" or "key" on at least two pictures, a list, or an int32 CUDA tensor')
        pairs = [(i, i + 1) for i in range(nimg - 1)] if pairs == "chain" else [(0, i) for i in range(1, nimg)]
    pt = match.pairList(pairs, nimg, imgs.device)
    out = harris.cornersFromImage8Batch(imgs, sobelSize=params["sobel_kernel_size"], windowSize=params["window_size"],
                                        gaussianSigma=params["gaussian_sigma"], harrisScore=params["alpha"],
                                        threshold=params["response_threshold"], minDistance=params["min_distance"], capacity=capacity,
                                        ctx=ctx, want_gradients=False, keypointSize=SIFT_WINDOW_SIZE)
    desc = harris.computeDescriptors8Batch(imgs, out["keypoints"], out["count"], ctx=ctx)
    matches, _, mcount = match.matchPairs(desc, out["count"], pt, ratio=ratio, ctx=ctx)
    tr, mask, st = ransac.solve_pairs(out["keypoints"], pt, matches, mcount, whichTransform, ransacReprojThresh, maxIters,
                                      minConsensusRatio, seed, ctx=ctx)
    warped = None
    if ransac._type(whichTransform) != 1:
        inv = warp.invertAffineTransform(tr[:, 0].contiguous(), ctx=ctx)
        second = imgs.index_select(0, pt[:, 1].to(torch.int64).clamp(0, nimg - 1))  # (a device gather: nothing read back)
        warped = warp.warpAffineBatch(second, inv, ctx=ctx)
    out.update(pairs=pt, matches=matches, match_count=mcount, transforms=tr, inlier_mask=mask, stats=st, warped=warped)
    return out
