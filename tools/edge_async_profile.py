#!/usr/bin/env python3
"""What sol::generateEdge costs with and without the host wait: the polled micv_generate_edge_dev against the union-find
entries of canny_uf.hip, per image.

    python tools/edge_async_profile.py [--out profiles/edge_async] [--rounds 9] [--calls 50] [--no-timing] [--no-resources]

Scenes: a rectangle-and-disc scene with noise at 480 x 640 and at 1080 x 1920 (Gaussian 5, sigma 1.4, thresholds 20 / 60: the
easy kind, where the polled loop converges in its first batch of rounds), and the 250 x 300 weak serpentine seeded at its
far end (Gaussian 1, thresholds 10 / 60: the kind that costs the polled loop a round per tile visit).  Per scene:
  polled        hough.generateEdge(wait=True): micv_generate_edge_dev, which stops the host in every call
  async         hough.generateEdge(wait=False): micv_generate_edge_async, enqueued only
  batch n       hough.generateEdgeBatch on n = 2, 8, 27 copies-with-different-noise of the scene, per image
  hysteresis    hough.hysteresis on the scene's candidate and strong masks: the stage alone (pack, union, mark, emit)
Every figure is the median over `rounds` windows of `calls` calls, host clock around a window that ends in a device
synchronise, the variants alternating round by round in one process on one build; min and max are the spread.  The
results are compared before anything is timed.  The timing needs a GPU; there is no fallback.

resources.txt in the same directory is the compiler's report for the kernels of canny_uf.hip (tools/kernel_resources.py:
registers, spills, scratch, occupancy, LDS); it needs the compiler and no GPU."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def scene(rows, cols, seed):
    rng = np.random.default_rng(seed)
    img = np.full((rows, cols), 60, np.int64)
    img[rows // 4: 3 * rows // 4, cols // 5: 4 * cols // 5] = 190
    yy, xx = np.mgrid[0:rows, 0:cols]
    img[(yy - rows // 2) ** 2 + (xx - cols // 2) ** 2 < (min(rows, cols) // 6) ** 2] = 20
    img += rng.integers(-12, 13, (rows, cols))
    return np.clip(img, 0, 255).astype(np.uint8)


def serpentine(rows, cols, seed, step=4, margin=3):
    """A dim one-pixel serpentine on a flat ground (weak edge pixels along it) with one bright blob at its far end (the
    only strong ones); the seed moves the ground by a grey level so that the images of a batch differ."""
    path, y, direction = [], margin, 1
    while y < rows - margin:
        xs = range(margin, cols - margin) if direction > 0 else range(cols - margin - 1, margin - 1, -1)
        path += [(y, x) for x in xs]
        path += [(yy, path[-1][1]) for yy in range(y + 1, min(y + step, rows - margin))]
        y += step
        direction = -direction
    img = np.full((rows, cols), 100 + seed % 3, np.int32)
    for (py, px) in path:
        img[py, px] = 118 + seed % 3
    y0, x0 = path[-1]
    img[max(0, y0 - 1):y0 + 2, max(0, x0 - 1):x0 + 2] = 250
    return img.astype(np.uint8)


SCENES = {  # name -> (maker, rows, cols, gaussian size, sigma, low, high)
    "scene 480x640": (scene, 480, 640, 5, 1.4, 20, 60),
    "scene 1080x1920": (scene, 1080, 1920, 5, 1.4, 20, 60),
    "serpentine 250x300": (serpentine, 250, 300, 1, 0.0001, 10, 60),
}


def resources(out):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "canny_uf"], capture_output=True, text=True)
    if r.returncode:
        raise SystemExit("edge_async_profile: the resource report failed:\n" + r.stderr)
    with open(os.path.join(out, "resources.txt"), "w") as f:
        f.write(r.stdout)
    print(r.stdout, end="")


def timing(a):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("edge_async_profile: no GPU (timings are only taken on one)")
    from introtocomputervision_amd import hough
    lines = []
    for name, (make, rows, cols, gs, sigma, lo, hi) in SCENES.items():
        imgs = torch.from_numpy(np.stack([make(rows, cols, i) for i in range(27)])).cuda()
        img = imgs[0]
        cand, strong = hough.generateEdge(img, gs, sigma, lo, lo), hough.generateEdge(img, gs, sigma, hi, hi)
        polled = hough.generateEdge(img, gs, sigma, lo, hi)
        # the same bytes every way, before anything is timed
        assert torch.equal(hough.generateEdge(img, gs, sigma, lo, hi, wait=False), polled), name
        assert torch.equal(hough.hysteresis(cand, strong), polled), name
        assert torch.equal(hough.generateEdgeBatch(imgs[:8], gs, sigma, lo, hi)[0], polled), name
        variants = {"polled": ((lambda: hough.generateEdge(img, gs, sigma, lo, hi)), 1),
                    "async": ((lambda: hough.generateEdge(img, gs, sigma, lo, hi, wait=False)), 1),
                    "hysteresis alone": ((lambda: hough.hysteresis(cand, strong)), 1)}
        for n in (2, 8, 27):
            variants[f"batch {n}"] = ((lambda n=n: hough.generateEdgeBatch(imgs[:n], gs, sigma, lo, hi)), n)
        for fn, _ in variants.values():  # warm-up: code objects, the arena
            fn()
            fn()
        torch.cuda.synchronize()
        times = {v: [] for v in variants}
        for _ in range(a.rounds):
            for v, (fn, n) in variants.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.calls):
                    fn()
                torch.cuda.synchronize()
                times[v].append((time.perf_counter() - t0) / (a.calls * n))
        for v, ts in times.items():
            ts = sorted(ts)
            rec = {"scene": name, "edge_pixels": int((polled != 0).sum()), "variant": v, "us_per_image_median": round(1e6 * ts[len(ts) // 2], 2),
                   "us_per_image_min": round(1e6 * ts[0], 2), "us_per_image_max": round(1e6 * ts[-1], 2), "rounds": a.rounds,
                   "calls_per_window": a.calls}
            lines.append(rec)
            print(json.dumps(rec), flush=True)
    with open(os.path.join(a.out, "profile.jsonl"), "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edge_async"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--no-timing", action="store_true")
    ap.add_argument("--no-resources", action="store_true")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    if not a.no_resources:
        resources(a.out)
    if not a.no_timing:
        timing(a)
    return 0


if __name__ == "__main__":
    sys.exit(main())
