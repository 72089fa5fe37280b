#!/usr/bin/env python3
"""What the descriptor step and the corners -> keypoints -> descriptors -> match chain of ps4 cost from 8-bit pictures: the
parent commit's way against the u8 entries with device counts.

    python tools/sift_u8_profile.py [--out profiles/sift_u8] [--rounds 9] [--window-s 0.2]

Scenes: 480 x 640 and 1080 x 1920 pictures of 32 x 32 random blocks (a few hundred / two thousand corners, capacity 4096: a
sparse list, as config/ps4.yaml's pictures give), and 480 x 640 of 8 x 8 blocks (more corners than the capacity: the dense
list, where a device count saves nothing).  Per scene, per image:
  (a) descriptors alone, the parent's way: computeDescriptors over all `capacity` rows of the list, loop of n images
  (b) descriptors alone, the parent's way with the counts known: computeDescriptors over the first `count` rows
  (c) descriptors alone, u8: computeDescriptors8 (n = 1) / computeDescriptors8Batch with device counts, n = 1, 2, 8, 27
  (d) the chain on a pair, the parent's way: cornersFromImage8(want_gradients=True, keypoints) + computeDescriptors over
      `capacity` rows + torch.where + knnMatch2.  The keypoint rows past a count are set to ps4.runProblem2's (a size-10
      keypoint at pixel (0, 0)) with one torch.where, which the parent does not pay: left as the corner call leaves them
      (unwritten memory) they can hold any size, and one run of this tool measured 8.3 ms for this line at 480 x 640 that
      way -- windows as large as the picture, not a cost of the parent's chain
  (e) the chain, the parent's way reading the counts back and slicing
  (f) the chain, u8: cornersFromImage8Batch (keypoints, no planes) + computeDescriptors8Batch + knnMatch2Counted
(profiles/sift_u8/staged_experiment.jsonl keeps the (c) and (f) rows of an earlier run of this tool, five rounds, on two
builds side by side: "staged", a kernel that first copied each keypoint's window of up to 109 x 109 bytes to LDS, and
"direct", the kernel as it is.  The staged form lost in every row and was removed.)
Every figure is the median over `rounds` synchronised windows (host clock around the window), variants interleaved round by
round; min and max are the spread.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PS4 = dict(sobelSize=3, windowSize=5, gaussianSigma=1.5, harrisScore=0.04, threshold=5e8, minDistance=5)  # config/ps4.yaml
KP_SIZE = 10.0  # SIFT_WINDOW_SIZE, Solution.cpp:141
CAP = 4096      # ps4.runProblem2's capacity


def picture(seed, rows, cols, block):
    rng = np.random.default_rng(seed)
    py, px = (int(v) for v in rng.integers(0, block, 2))
    coarse = rng.integers(0, 256, (rows // block + 3, cols // block + 3), dtype=np.uint8)
    img = np.kron(coarse, np.ones((block, block), np.uint8))[py:py + rows, px:px + cols]
    return np.ascontiguousarray(img ^ rng.integers(0, 4, (rows, cols), dtype=np.uint8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sift_u8"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--window-s", type=float, default=0.2)
    ap.add_argument("--scenes", default="480x640/32,1080x1920/32,480x640/8")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("sift_u8_profile: no GPU (timings are only taken on one)")
    from introtocomputervision_amd import harris, match
    from introtocomputervision_amd._capi import Context
    ctx = Context(0)
    os.makedirs(a.out, exist_ok=True)
    lines = []
    for scene in a.scenes.split(","):
        size, block = scene.split("/")
        rows, cols = (int(v) for v in size.split("x"))
        dev8 = torch.from_numpy(np.stack([picture(100 + i, rows, cols, int(block)) for i in range(27)])).cuda()
        kw = dict(PS4, capacity=CAP, ctx=ctx)
        # what the corner chains leave behind: keypoints + counts (u8 batch), and the parent's planes for every image
        lists = harris.cornersFromImage8Batch(dev8, want_gradients=False, keypointSize=KP_SIZE, **kw)
        kp, cnt = lists["keypoints"], lists["count"]
        # rows past a count: what the parent's getKeypoints makes of them, a size-10 keypoint at pixel (0, 0)
        kp.masked_fill_(torch.arange(CAP, device="cuda")[None, :, None] >= cnt[:, None, None], 0.0)
        kp[:, :, 2] = KP_SIZE
        counts = [min(int(c), CAP) for c in cnt.cpu()]
        planes = [harris.getGradients(dev8[i].to(torch.float32), 3, 1.0, ctx=ctx) for i in range(27)]

        def parent_all(n):
            def run():
                for i in range(n):
                    harris.computeDescriptors(planes[i][0], planes[i][1], kp[i], ctx=ctx)
            return run, n

        def parent_sliced(n):
            def run():
                for i in range(n):
                    harris.computeDescriptors(planes[i][0], planes[i][1], kp[i, :counts[i]], ctx=ctx)
            return run, n

        def u8_batch(n):
            return (lambda: harris.computeDescriptors8Batch(dev8[:n], kp[:n], cnt[:n], ctx=ctx)), n

        rows_idx = torch.arange(CAP, device="cuda").unsqueeze(1)
        past = torch.tensor([0.0, 0.0, KP_SIZE, 0.0], device="cuda").expand(CAP, 4)

        def chain_parent(read_back):
            def run():
                ds, ks, cs = [], [], []
                for i in range(2):
                    o = harris.cornersFromImage8(dev8[i], want_gradients=True, lazy=True, keypointSize=KP_SIZE, **kw)
                    k = o["keypoints"]
                    if read_back:
                        k = k[:min(int(o["count"].item()), CAP)]
                    else:  # rows past the count are not written by the corner call: make them the parent's rows (see above)
                        k = torch.where(rows_idx >= o["count"], past, k)
                    ds.append(harris.computeDescriptors(o["gx"], o["gy"], k, ctx=ctx))
                    ks.append(k)
                    cs.append(o["count"])
                if read_back:
                    if ds[0].shape[0] and ds[1].shape[0] >= 2:
                        match.knnMatch2(ds[0], ds[1], ctx=ctx)
                    return
                far = torch.arange(CAP, device="cuda").unsqueeze(1) >= cs[1]
                train = torch.where(far, torch.full_like(ds[1], float("inf")), ds[1])
                idx, dist = match.knnMatch2(ds[0], train, ctx=ctx)
                torch.where(torch.arange(CAP, device="cuda").unsqueeze(1) >= cs[0], torch.full_like(dist, float("nan")), dist)
            return run, 2

        def chain_u8():
            def run():
                o = harris.cornersFromImage8Batch(dev8[:2], want_gradients=False, keypointSize=KP_SIZE, **kw)
                d = harris.computeDescriptors8Batch(dev8[:2], o["keypoints"], o["count"], ctx=ctx)
                match.knnMatch2Counted(d[0], d[1], o["count"][0:1], o["count"][1:2], ctx=ctx)
            return run, 2

        variants = {}
        for n in (1, 2, 8, 27):
            variants[f"(a) descriptors, parent: computeDescriptors over {CAP} rows, loop of {n}"] = parent_all(n)
            variants[f"(b) descriptors, parent with known counts: computeDescriptors over count rows, loop of {n}"] = parent_sliced(n)
            variants[f"(c) descriptors, u8 batch of {n}, device counts"] = u8_batch(n)
        variants["(c) descriptors, u8 single call, device count"] = ((lambda: harris.computeDescriptors8(dev8[0], kp[0], cnt[0:1], ctx=ctx)), 1)
        variants["(d) chain on a pair, parent: planes + all rows + torch.where + knnMatch2"] = chain_parent(False)
        variants["(e) chain on a pair, parent reading the counts back and slicing"] = chain_parent(True)
        variants["(f) chain on a pair, u8: batch corners + batch descriptors + counted matcher"] = chain_u8()

        # same descriptors either way, before anything is timed
        ref = harris.computeDescriptors(planes[0][0], planes[0][1], kp[0, :counts[0]], ctx=ctx)
        got = harris.computeDescriptors8Batch(dev8[:2], kp[:2], cnt[:2], ctx=ctx)[0, :counts[0]]
        assert torch.equal(ref, got), "the u8 descriptors differ from the f32 entry's"

        reps = {}
        for name, (fn, n) in variants.items():  # warm-up, and how many repetitions fill a window
            for _ in range(2):
                fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            k = 0
            while time.perf_counter() - t0 < 0.04:
                fn()
                k += 1
            torch.cuda.synchronize()
            reps[name] = max(2, int(a.window_s / ((time.perf_counter() - t0) / k)))
        times = {name: [] for name in variants}
        for _ in range(a.rounds):
            for name, (fn, n) in variants.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(reps[name]):
                    fn()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) / (reps[name] * n))
        for name, ts in times.items():
            ts = sorted(ts)
            rec = {"scene": scene, "capacity": CAP, "counts_of_images_0_1": counts[:2], "variant": name,
                   "us_per_image_median": round(1e6 * ts[len(ts) // 2], 2), "us_per_image_min": round(1e6 * ts[0], 2),
                   "us_per_image_max": round(1e6 * ts[-1], 2), "rounds": a.rounds, "repetitions_per_window": reps[name]}
            lines.append(rec)
            print(json.dumps(rec), flush=True)
    with open(os.path.join(a.out, "profile.jsonl"), "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
