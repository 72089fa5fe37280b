"""ransac::seed / ransac::solve of the reference's ps4 library (ProblemSets/ps4_cpp/lib/RANSAC.cpp,
include/RANSAC.h:10-28) on the HIP kernels of csrc/ransac.hip.

The sampler is the reference's: one std::mt19937 shared by every solve, seeded once from the
config's ``mersenne_seed`` words, a persistent index vector shuffled once per iteration
(`Generator`, host side).  numpy points take ``micv_ransac_solve_host``, CUDA tensors
``micv_ransac_solve_dev``; either way the generator then advances by the iterations the solve ran,
as the reference's shared engine does.  `solve_matches` is the device-resident end of the ps4 chain
(its own counter-based sampler, not the reference's sequence)."""
import ctypes as C

import numpy as np

from ._capi import check, lib
from .lk import _ctx_for

TRANSLATION, SIMILARITY, AFFINE = 1, 2, 3
_TYPES = {"TRANSLATION": 1, "SIMILARITY": 2, "AFFINE": 3}


class Generator:
    """The reference's engine (std::seed_seq(words) -> std::mt19937; words None = default-constructed)."""

    def __init__(self, words=None):
        h = C.c_void_p()
        if words is None:
            check(lib.micv_ransac_rng_create(None, 0, C.byref(h)))
        else:
            w = np.ascontiguousarray(np.asarray(words, np.uint64).astype(np.uint32))
            check(lib.micv_ransac_rng_create(w.ctypes.data, len(w), C.byref(h)))
        self._h = h

    def samples(self, n, k, iters):
        """iters x k sample indices of the next solve over n points; the engine is not advanced."""
        out = np.empty((iters, k), np.int32)
        check(lib.micv_ransac_rng_samples(self._h, n, k, iters, out.ctypes.data))
        return out

    def permutation(self, n, it):
        """The index vector after iteration `it` (0-based) of the next solve; not advanced."""
        out = np.empty(n, np.int32)
        check(lib.micv_ransac_rng_permutation(self._h, n, it, out.ctypes.data))
        return out

    def advance(self, n, iterations):
        check(lib.micv_ransac_rng_advance(self._h, n, iterations))

    def __del__(self):
        if getattr(self, "_h", None) and lib is not None:
            lib.micv_ransac_rng_destroy(self._h)
            self._h = None


_RNG = [None]  # the file-static engine of RANSAC.cpp:12-13
_SEEDED = [False]


def seed(words):
    """ransac::seed: seeds the shared engine from std::seed_seq(words); later calls are ignored."""
    if not _SEEDED[0]:
        _RNG[0] = Generator(words)
        _SEEDED[0] = True


def generator():
    if _RNG[0] is None:
        _RNG[0] = Generator(None)  # `static std::mt19937 rng;` before any ransac::seed
    return _RNG[0]


class Result(tuple):
    """(transform, consensusSet, ratio) as ransac::solve returns them, plus the intended-semantics
    outputs: best_transform (the best iteration's 2x3), inlier_mask (over the original point
    indices), iterations, best_iter, best_count."""

    def __new__(cls, transform, consensus, ratio, **extra):
        r = super().__new__(cls, (transform, consensus, ratio))
        r.__dict__.update(extra)
        return r

    transform = property(lambda self: self[0])
    consensusSet = property(lambda self: self[1])
    ratio = property(lambda self: self[2])


def _type(t):
    t = _TYPES.get(t, t) if isinstance(t, str) else int(getattr(t, "value", t))
    if t not in (1, 2, 3):
        raise ValueError(f"whichTransform {t}: TRANSLATION (1), SIMILARITY (2) or AFFINE (3)")
    return t


def solve(srcPts, destPts, whichTransform, ransacReprojThresh=3, maxIters=2000, minConsensusRatio=0.75,
          gen=None, ctx=None):
    """ransac::solve.  srcPts / destPts: N x 2 float32 (numpy -> host entry point, CUDA tensor ->
    device entry point).  Returns a `Result`; the transform is the LAST iteration's, as written
    (an empty 0 x 3 array when no iteration ran), consensusSet the positions in the best
    iteration's permutation."""
    k = _type(whichTransform)
    g = gen or generator()
    dev = not isinstance(srcPts, np.ndarray)
    n = int(srcPts.shape[0])
    if srcPts.shape != (n, 2) or tuple(destPts.shape) != (n, 2):
        raise ValueError("srcPts / destPts: two N x 2 point arrays of equal N")
    if n < k:
        raise ValueError(f"{n} points, the transform needs {k}")
    iters = int(maxIters)
    if iters < 1:
        raise ValueError("maxIters < 1")
    samples = g.samples(n, k, iters)
    stats = np.zeros(3, np.int32)
    if not dev:
        from .match import _host_ctx
        src = np.ascontiguousarray(srcPts, np.float32)
        dst = np.ascontiguousarray(destPts, np.float32)
        tr = np.zeros((2, 2, 3), np.float32)
        mask = np.zeros(n, np.uint8)
        c = ctx or _host_ctx()
        check(lib.micv_ransac_solve_host(c.handle, src.ctypes.data, dst.ctypes.data, n, samples.ctypes.data, iters, k,
                                         int(ransacReprojThresh), float(minConsensusRatio), tr.ctypes.data,
                                         mask.ctypes.data, stats.ctypes.data))
    else:
        import torch
        for t, nm in ((srcPts, "srcPts"), (destPts, "destPts")):
            if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
                raise ValueError(f"{nm}: need a contiguous float32 CUDA tensor")
        dv = srcPts.device
        ds = torch.from_numpy(samples).to(dv)
        tr = torch.zeros((2, 2, 3), dtype=torch.float32, device=dv)
        mask = torch.zeros(n, dtype=torch.uint8, device=dv)
        st = torch.zeros(3, dtype=torch.int32, device=dv)
        check(lib.micv_ransac_solve_dev(_ctx_for(srcPts, ctx).handle, srcPts.data_ptr(), destPts.data_ptr(), n,
                                        ds.data_ptr(), iters, k, int(ransacReprojThresh), float(minConsensusRatio),
                                        tr.data_ptr(), mask.data_ptr(), st.data_ptr(),
                                        torch.cuda.current_stream(dv).cuda_stream))
        stats = st.cpu().numpy()
    iterations, best_iter, best_count = (int(v) for v in stats)
    if iterations < 0:
        raise RuntimeError("ransac: a sample index outside the point set")
    positions = []
    if best_count > 0:
        perm = g.permutation(n, best_iter)
        m = mask.cpu().numpy() if dev else mask
        inv = np.empty(n, np.int64)
        inv[perm] = np.arange(n)
        positions = sorted(int(p) for p in inv[np.nonzero(m)[0]])
    g.advance(n, iterations)
    transform = tr[0] if iterations > 0 else (tr.new_zeros((0, 3)) if dev else np.zeros((0, 3), np.float32))
    return Result(transform, positions, float(best_count) / float(n) if best_count else 0.0,
                  best_transform=tr[1], inlier_mask=mask, iterations=iterations, best_iter=best_iter,
                  best_count=best_count)


def solve_matches(kp_a, kp_b, matches, count, whichTransform, ransacReprojThresh=3, maxIters=2000,
                  minConsensusRatio=0.75, seed=0, ctx=None):
    """The device-resident chain end: kp_a / kp_b (n x 4 keypoints of micv_sift_keypoints), matches
    (cap x 2 int32) and count (1-element int64 CUDA tensor) as the ratio filter left them.  No host
    synchronisation: returns CUDA tensors (transforms [2, 2, 3] = as written / best, inlier mask [cap],
    stats [3] = iterations, best_iter, best_count)."""
    import torch
    k = _type(whichTransform)
    dv = kp_a.device
    cap = int(matches.shape[0])
    tr = torch.empty((2, 2, 3), dtype=torch.float32, device=dv)
    mask = torch.empty(max(cap, 1), dtype=torch.uint8, device=dv)
    st = torch.empty(3, dtype=torch.int32, device=dv)
    check(lib.micv_ransac_solve_matches_dev(_ctx_for(kp_a, ctx).handle, kp_a.data_ptr(), kp_a.shape[0],
                                            kp_b.data_ptr(), kp_b.shape[0], matches.data_ptr(), count.data_ptr(),
                                            cap, int(seed) & ((1 << 64) - 1), int(maxIters), k,
                                            int(ransacReprojThresh), float(minConsensusRatio), tr.data_ptr(),
                                            mask.data_ptr(), st.data_ptr(), torch.cuda.current_stream(dv).cuda_stream))
    return tr, mask[:cap], st


def pairSeed(seed, p):
    """The seed micv_ransac_solve_pairs_dev gives pair p: splitmix64(seed + p), the sum wrapping in 64 bits -- what
    solve_matches takes to reproduce element p of solve_pairs."""
    m = (1 << 64) - 1
    z = ((int(seed) + int(p)) + 0x9E3779B97F4A7C15) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return z ^ (z >> 31)


def solve_pairs(kp, pairs, matches, match_count, whichTransform, ransacReprojThresh=3, maxIters=2000, minConsensusRatio=0.75,
                seed=0, ctx=None):
    """solve_matches on a batch of pairs, four launches whatever their number (micv_ransac_solve_pairs_dev).  kp [images,
    kcap, 4] float32 CUDA keypoints, pairs as for match.matchPairs, matches [npairs, mcap, 2] and match_count [npairs] as
    matchPairs left them.  -> (transforms [npairs, 2, 2, 3], inlier mask [npairs, mcap], stats [npairs, 3]); element p holds
    the bytes of solve_matches(kp[a], kp[b], matches[p], match_count[p:p+1], ..., seed=pairSeed(seed, p)).  Nothing is read
    back."""
    import torch
    from .match import pairList
    k = _type(whichTransform)
    if not (isinstance(kp, torch.Tensor) and kp.is_cuda and kp.dim() == 3 and kp.shape[2] == 4 and kp.dtype == torch.float32
            and kp.stride(2) == 1 and (kp.shape[1] <= 1 or kp.stride(1) == 4)):
        raise ValueError("kp: need an [images, kcap, 4] float32 CUDA tensor with dense rows")
    images, kcap = int(kp.shape[0]), int(kp.shape[1])
    dv = kp.device
    pt = pairList(pairs, images, dv)
    npairs = int(pt.shape[0])
    if not (matches.is_cuda and matches.dtype == torch.int32 and matches.is_contiguous() and matches.dim() == 3
            and matches.shape[0] == npairs and matches.shape[2] == 2):
        raise ValueError("matches: need a contiguous [npairs, mcap, 2] int32 CUDA tensor")
    if not (match_count.is_cuda and match_count.dtype == torch.int64 and match_count.is_contiguous() and match_count.numel() == npairs):
        raise ValueError("match_count: need a contiguous [npairs] int64 CUDA tensor")
    mcap = int(matches.shape[1])
    tr = torch.empty((npairs, 2, 2, 3), dtype=torch.float32, device=dv)
    mask = torch.empty((npairs, max(mcap, 1)), dtype=torch.uint8, device=dv)
    st = torch.empty((npairs, 3), dtype=torch.int32, device=dv)
    check(lib.micv_ransac_solve_pairs_dev(_ctx_for(kp, ctx).handle, kp.data_ptr(), images, (kp.stride(0) if images > 1 else kcap * 4) * 4,
                                          kcap, pt.data_ptr(), npairs, matches.data_ptr(), match_count.data_ptr(), mcap,
                                          int(seed) & ((1 << 64) - 1), int(maxIters), k, int(ransacReprojThresh),
                                          float(minConsensusRatio), tr.data_ptr(), mask.data_ptr(), st.data_ptr(),
                                          torch.cuda.current_stream(dv).cuda_stream))
    return tr, mask[:, :mcap], st
