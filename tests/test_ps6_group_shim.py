"""The group form of the ps6 driver through the C++ shim (micv_ps6::pfDriverGroupDevice, shim/micv_ps6.hpp):
tests/cpp/ps6_group_demo.cpp runs problems 1-3 as six single-filter library calls and as two calls on filter groups, and
fails unless every state and every written file is equal.  It compiles without a GPU; it runs on one."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ps6")
ROWS, COLS, NFRAMES = 120, 160, 30
# the reference's boxes (pres_debate.txt; Solution.cpp:144-145) at a quarter of the videos' size
HEAD, HAND = (80.2188, 43.7944, 25.8851, 32.2626), (135.0, 96.0, 18.0, 22.0)


def build_demo(tmp):
    exe = os.path.join(str(tmp), "ps6_group_demo")
    lib = os.path.join(ROOT, "introtocomputervision_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "ps6_group_demo.cpp"),
                    "-o", exe, "-L" + lib, "-lmicv", "-Wl,-rpath," + lib], check=True)
    return exe


def test_ps6_group_demo_compiles(tmp_path):
    build_demo(tmp_path)


def sequences():
    """A colour sequence with a textured 'head' starting at the head box and a textured 'hand' at the hand box, both
    moving, and a noisy copy."""
    rng = np.random.default_rng(607)
    bg = rng.integers(0, 256, (ROWS, COLS, 3), dtype=np.uint8)
    head = rng.integers(0, 256, (32, 26, 3), dtype=np.uint8)
    hand = rng.integers(0, 256, (22, 18, 3), dtype=np.uint8)
    clean, noisy = [], []
    for t in range(NFRAMES):
        f = bg.copy()
        y, x = 44 + t // 2, 80 + t
        f[y:y + 32, x:x + 26] = head
        y, x = 96 - t // 4, 135 - t // 2
        f[y:y + 22, x:x + 18] = hand
        clean.append(f)
        n = f.astype(np.int16) + rng.integers(-20, 21, f.shape, dtype=np.int16)
        noisy.append(np.clip(n, 0, 255).astype(np.uint8))
    return clean, noisy


@pytest.mark.gpu
def test_two_group_calls_write_the_files_of_six_single_calls(tmp_path):
    exe = build_demo(tmp_path)
    clean, noisy = sequences()
    for name, seq in (("clean", clean), ("noisy", noisy)):
        for t, f in enumerate(seq):
            f.tofile(str(tmp_path / f"{name}_{t}.u8"))
    for name in ("pres_debate.txt", "noisy_debate.txt"):
        (tmp_path / name).write_text(f"{HEAD[0]} {HEAD[1]}\n{HEAD[2]} {HEAD[3]}\n")
    os.mkdir(tmp_path / "single")
    os.mkdir(tmp_path / "group")
    run = subprocess.run([exe, os.path.join(GOLDEN, "ps6.yaml"), str(tmp_path / "pres_debate.txt"), str(tmp_path / "noisy_debate.txt"),
                          str(tmp_path), str(ROWS), str(COLS), str(NFRAMES), str(tmp_path)] + [str(v) for v in HAND],
                         capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "6 files compared, 0 differences" in run.stdout
    names = sorted(os.listdir(tmp_path / "single"))
    assert names == sorted(os.listdir(tmp_path / "group"))
    # the saved frames that a 30-frame sequence reaches
    want = {"ps6-1-a-f28.ppm", "ps6-1-e-f14.ppm", "ps6-2-a-f15.ppm", "ps6-2-b-f15.ppm", "ps6-3-a-f28.ppm", "ps6-3-b-f15.ppm"}
    assert set(names) == want, set(names) ^ want
    from introtocomputervision_amd import viz
    for n in names:
        assert open(tmp_path / "single" / n, "rb").read() == open(tmp_path / "group" / n, "rb").read(), n
        img = viz.imread(str(tmp_path / "group" / n))
        src = (noisy if n[:7] in ("ps6-1-e", "ps6-2-b") else clean)[int(n.rsplit("-f", 1)[1].split(".")[0])]
        changed = (img != src).any(2)
        assert (img[changed] == [255, 0, 255]).all(1).sum() > 20 and (img[changed] == [0, 255, 0]).all(1).sum() > 4, n  # a box and dots
