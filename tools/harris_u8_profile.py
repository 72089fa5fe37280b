#!/usr/bin/env python3
"""What the ps4 corner chain costs per image from an 8-bit picture: the parent's way (convert to float32, then the f32
entry) against the u8 entries, single and batched, on the device and through the host entries.

    python tools/harris_u8_profile.py [--out profiles/harris_u8] [--rounds 9] [--window-s 0.25]

Per size (480 x 640 with config/ps4.yaml's parameters, and 1080 x 1920) it times, per image:
  (a) the parent's way: img.to(float32) + cornersFromImage(lazy=True), alone and in a loop of 4 and of 8 images
  (b) the single u8 call: cornersFromImage8(lazy=True)
  (c) the batch of 2, 4, 8 and 27: cornersFromImage8Batch
  (d) the host entries on numpy arrays: cornersFromImage8 against cornersFromImage on the converted array
  (e) (b) and (c) with keypoints and no planes, against cornersFromImage(want_gradients=True) + getKeypoints
Every figure is the median over `rounds` synchronised windows (each: as many repetitions as fill window-s, then one device
synchronise; host clock around the window), after a warm-up of every shape; min and max over the rounds are the spread.
The variants are interleaved round by round, so a drift of the machine hits all of them alike.  (a) runs the code paths of
the parent commit: the comparison is never against the new code itself.  Needs a GPU; there is no fallback."""
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
CAP = 1 << 15  # more than the corners of a 1080p picture of this kind (about 14 000)


def picture(seed, rows, cols):
    """8 x 8 blocks of random bytes at a random phase, two random low bits: a few corners per thousand pixels."""
    rng = np.random.default_rng(seed)
    py, px = (int(v) for v in rng.integers(0, 8, 2))
    coarse = rng.integers(0, 256, (rows // 8 + 3, cols // 8 + 3), dtype=np.uint8)
    img = np.kron(coarse, np.ones((8, 8), np.uint8))[py:py + rows, px:px + cols]
    return np.ascontiguousarray(img ^ rng.integers(0, 4, (rows, cols), dtype=np.uint8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "harris_u8"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--window-s", type=float, default=0.25)
    ap.add_argument("--sizes", default="480x640,1080x1920")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("harris_u8_profile: no GPU (timings are only taken on one)")
    from introtocomputervision_amd import harris
    from introtocomputervision_amd._capi import Context
    ctx = Context(0)
    os.makedirs(a.out, exist_ok=True)
    lines = []
    for size in a.sizes.split(","):
        rows, cols = (int(v) for v in size.split("x"))
        host8 = [picture(100 + i, rows, cols) for i in range(27)]
        dev8 = torch.from_numpy(np.stack(host8)).cuda()
        host32 = host8[0].astype(np.float32)
        lean = dict(PS4, capacity=CAP, ctx=ctx, want_gradients=False)
        full = dict(PS4, capacity=CAP, ctx=ctx, want_gradients=True)

        def parent_loop(n, kw):
            def run():
                for i in range(n):
                    harris.cornersFromImage(dev8[i].to(torch.float32), lazy=True, **kw)
            return run, n

        def u8_loop(n, kw):
            def run():
                for i in range(n):
                    harris.cornersFromImage8(dev8[i], lazy=True, **kw)
            return run, n

        def batch(n, kw):
            return (lambda: harris.cornersFromImage8Batch(dev8[:n], **kw)), n

        def parent_kp():
            o = harris.cornersFromImage(dev8[0].to(torch.float32), **full)
            harris.getKeypoints(o["gx"], o["gy"], o["locs"], KP_SIZE, ctx=ctx)

        variants = {}
        for tag, kw in (("lists only", lean), ("with gradient planes", full)):
            for n in (1, 4, 8):
                variants[f"(a) parent: to(float32) + cornersFromImage, loop of {n}, {tag}"] = parent_loop(n, kw)
            for n in (1, 4, 8):
                variants[f"(b) u8 single call, loop of {n}, {tag}"] = u8_loop(n, kw)
            for n in (2, 4, 8, 27):
                variants[f"(c) u8 batch of {n}, {tag}"] = batch(n, kw)
        kpkw = dict(lean, keypointSize=KP_SIZE)
        variants["(e) parent: cornersFromImage(want_gradients=True) + getKeypoints (reads the count)"] = (parent_kp, 1)
        variants["(e) u8 single call, keypoints, no planes"] = u8_loop(1, kpkw)
        for n in (2, 4, 8, 27):
            variants[f"(e) u8 batch of {n}, keypoints, no planes"] = batch(n, kpkw)
        hostkw = dict(PS4, capacity=CAP, ctx=ctx, want_gradients=False)
        variants["(d) host f32: cornersFromImage on the converted numpy array"] = ((lambda: harris.cornersFromImage(host32, **hostkw)), 1)
        variants["(d) host u8: cornersFromImage8 on the numpy array"] = ((lambda: harris.cornersFromImage8(host8[0], **hostkw)), 1)
        variants["(d) host f32 incl. the conversion: astype(float32) + cornersFromImage"] = (
            (lambda: harris.cornersFromImage(host8[0].astype(np.float32), **hostkw)), 1)

        # same corners either way, before anything is timed
        ref = harris.cornersFromImage(dev8[0].to(torch.float32), **lean)["locs"].cpu().numpy()
        got = harris.cornersFromImage8(dev8[0], **lean)["locs"].cpu().numpy()
        b = harris.cornersFromImage8Batch(dev8[:4], **lean)
        n0 = min(int(b["count"][0]), CAP)
        assert len(ref) < CAP, f"{len(ref)} corners: the lists are cut at {CAP}"
        assert np.array_equal(ref, got), "the u8 call's corners differ from the f32 entry's"
        assert n0 == len(ref) and np.array_equal(b["locs"][0, :n0].cpu().numpy(), ref), "the batch's corners differ from the f32 entry's"

        reps = {}
        for name, (fn, n) in variants.items():  # warm-up, and how many repetitions fill a window
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            k = 0
            while time.perf_counter() - t0 < 0.05:
                fn()
                k += 1
            torch.cuda.synchronize()
            per = (time.perf_counter() - t0) / k
            reps[name] = max(3, int(a.window_s / per))
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
            rec = {"size": size, "corners_in_image_0": len(ref), "variant": name, "us_per_image_median": round(1e6 * ts[len(ts) // 2], 2),
                   "us_per_image_min": round(1e6 * ts[0], 2), "us_per_image_max": round(1e6 * ts[-1], 2), "rounds": a.rounds,
                   "repetitions_per_window": reps[name]}
            lines.append(rec)
            print(json.dumps(rec))
    with open(os.path.join(a.out, "profile.jsonl"), "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
