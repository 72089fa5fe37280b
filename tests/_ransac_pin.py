"""Helpers shared by the RANSAC tests: the sampler pin (tests/cpp/ransac_sampler_ref.cpp, the
reference's literal seed_seq / mt19937 / std::shuffle calls, built with g++), synthetic point sets
with known transforms, and runProblem3's three solves driven by the pin."""
import os
import subprocess

import numpy as np

import _ransac_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PS4_SEED = "16 38 c7 e4 6a a2 d8 cc 96 f6 fe f1 4b 7d a7 25"  # config/ps4.yaml `mersenne_seed`
PS4_SEED_WORDS = [int(w, 16) for w in PS4_SEED.split()]
# config/ps4.yaml ransac_{trans,sim,affine}: (type, reprojection_threshold, max_iterations, consensus_ratio)
PS4_RANSAC = [(rr.TRANSLATION, 10, 2000, 0.2), (rr.SIMILARITY, 6, 2000, 0.6), (rr.AFFINE, 6, 2000, 0.6)]


def build_pin(tmp):
    exe = os.path.join(str(tmp), "ransac_sampler_ref")
    if not os.path.exists(exe):
        subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror",
                        os.path.join(ROOT, "tests", "cpp", "ransac_sampler_ref.cpp"), "-o", exe], check=True)
    return exe


def pin_perms(exe, seed, solves):
    """solves: [(n, iterations)] -> list (per solve) of int arrays [iterations, n]."""
    args = [exe, seed] + [str(v) for s in solves for v in s]
    out = subprocess.run(args, check=True, capture_output=True, text=True).stdout.split("\n")
    res = [[] for _ in solves]
    for line in out:
        if line:
            v = [int(x) for x in line.split()]
            res[v[0]].append(v[2:])
    return [np.asarray(r, np.int64).reshape(-1, n) for r, (n, _) in zip(res, solves)]


class ListShuffle:
    """std::shuffle with the shared engine, replayed from the pin's output: each call replaces the
    list with the next recorded vector (and checks the recording started from the same vector)."""

    def __init__(self, perms):
        self.perms, self.i = perms, 0

    def __call__(self, indices):
        indices[:] = [int(v) for v in self.perms[self.i]]
        self.i += 1


def synth(ttype, n, n_in, seed):
    """n point pairs, the first n_in (shuffled in) mapped exactly by a known transform with integer
    results; the rest random.  Returns src, dst (float32), the true 2x3, inlier flags."""
    rng = np.random.default_rng(seed)
    src = (rng.integers(0, 60, (n, 2)) * 5).astype(np.float64)
    if ttype == rr.TRANSLATION:
        T = np.array([[1, 0, -134], [0, 1, -78]], np.float64)
    elif ttype == rr.SIMILARITY:
        T = np.array([[0.6, -0.8, 38], [0.8, 0.6, -58]], np.float64)
    else:
        T = np.array([[2, 1, 39], [-1, 1, -65]], np.float64)
    dst = src @ T[:, :2].T + T[:, 2]
    inl = np.zeros(n, bool)
    inl[rng.permutation(n)[:n_in]] = True
    dst[~inl] = rng.integers(-300, 300, ((~inl).sum(), 2))
    return src.astype(np.float32), np.round(dst).astype(np.float32), T, inl


def ps4_problem3_sets():
    """Three synthetic match sets sized as the reference's log reports (117, 78, 78 matches)."""
    return [synth(rr.TRANSLATION, 117, 40, 1), synth(rr.SIMILARITY, 78, 56, 2), synth(rr.AFFINE, 78, 56, 3)]


def run_problem3(exe, sets, seed=PS4_SEED):
    """runProblem3's three solves in order, the engine shared, driven by the pin.  Returns per solve
    (transform, positions, ratio, iterations, perms of that solve)."""
    done, out = [], []
    for (src, dst, _, _), (tt, th, mi, mr) in zip(sets, PS4_RANSAC):
        perms = pin_perms(exe, seed, done + [(len(src), mi)])[-1]
        t, pos, ratio, its = rr.solve_as_written(src, dst, tt, th, mi, mr, ListShuffle(perms))
        out.append((t, pos, ratio, its, perms[:its]))
        done.append((len(src), its))
    return out
