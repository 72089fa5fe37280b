"""shim/micv_ps7.hpp: tests/cpp/ps7_driver_demo.cpp runs problem 1 and problem 2's MHI stage of ps7 on the synthetic
colour videos of tests/_ps7_driver_cases.py both ways -- the reference's loops on the shim's mhi:: functions (CV_8UC3
frames that are ROIs of padded buffers) and the one-call forms -- and the files must be equal byte for byte, and equal
to the restatement's."""
import os
import subprocess

import numpy as np
import pytest

import _display_ref as D
import _mhi_color_ref as R
from _ps7_driver_cases import COLS, LONG, ROWS, expected_mhis, last_frame, videos, write_yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_demo(tmp):
    exe = os.path.join(str(tmp), "ps7_driver_demo")
    lib = os.path.join(ROOT, "introtocomputervision_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "ps7_driver_demo.cpp"),
                    "-o", exe, "-L" + lib, "-lmicv", "-Wl,-rpath," + lib], check=True)
    return exe


def test_ps7_driver_demo_compiles(tmp_path):
    build_demo(tmp_path)


def test_ps7_shim_signatures_still_compile_beside_the_driver_header(tmp_path):
    src = tmp_path / "both.cpp"
    src.write_text('#include "introtocomputervision_amd/shim/micv_ps7.hpp"\n#include "tests/cpp/ps7_shim_signatures.cpp"\n')
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-Wno-unused-function", "-I" + ROOT,
                        "-I" + os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def read_pgm(path):
    from introtocomputervision_amd import viz
    return viz.imread(str(path))


@pytest.mark.gpu
def test_device_forms_write_the_host_loops_files(tmp_path):
    exe = build_demo(tmp_path)
    for name, v in videos().items():
        v.tofile(str(tmp_path / f"{name}.u8"))
    os.mkdir(tmp_path / "host")
    os.mkdir(tmp_path / "dev")
    run = subprocess.run([exe, write_yaml(tmp_path), str(tmp_path), str(ROWS), str(COLS), str(tmp_path)],
                         capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "videos 27 mhis 27 different 0" in run.stdout
    names = sorted(os.listdir(tmp_path / "host"))
    assert names == sorted(os.listdir(tmp_path / "dev"))
    want = {"ps7-1-a-1.pgm", "ps7-1-b-1.pgm", "ps7-1-b-2.pgm", "ps7-1-b-3.pgm", "sets-diff-0.pgm", "sets-diff-1.pgm",
            "sets-mhi-0.pgm", "sets-mhi-1.pgm", "bgra.pgm"} | {f"mhi-{i:02d}-a{1 + i // 9}p{1 + i // 3 % 3}.pgm" for i in range(27)}
    assert set(names) == want, set(names) ^ want
    for n in names:
        assert open(tmp_path / "host" / n, "rb").read() == open(tmp_path / "dev" / n, "rb").read(), n
    # against the restatement
    mh = expected_mhis(3, 1)
    for i in range(27):
        assert np.array_equal(read_pgm(tmp_path / "dev" / f"mhi-{i:02d}-a{1 + i // 9}p{1 + i // 3 % 3}.pgm"), mh[i]), i
    args = (20, 3, 1, 3)
    hist, diff = R.history_seq(videos()[LONG], *args, (2, 7), (3, 9, 10))
    assert np.array_equal(read_pgm(tmp_path / "dev" / "ps7-1-a-1.pgm"), D.normalize(diff[2]))
    assert np.array_equal(read_pgm(tmp_path / "dev" / "sets-diff-0.pgm"), diff[0]) and diff[0].any()
    assert np.array_equal(read_pgm(tmp_path / "dev" / "sets-diff-1.pgm"), diff[1])
    assert np.array_equal(read_pgm(tmp_path / "dev" / "sets-mhi-0.pgm"), hist[0])
    assert np.array_equal(read_pgm(tmp_path / "dev" / "sets-mhi-1.pgm"), hist[1])
    v = videos()[LONG]
    assert np.array_equal(read_pgm(tmp_path / "dev" / "bgra.pgm"), R.frame_difference(v[3], v[4], 20, (3, 3), 1.0))
    b1 = R.history_seq(videos()["PS7A1P2T1"], *args, (last_frame(1, 2, 1),))[0][0]
    assert np.array_equal(read_pgm(tmp_path / "dev" / "ps7-1-b-1.pgm"), D.normalize(b1))
