"""The shim's corner chain on 8-bit Mats: micv_ps4::harrisCorners8 fills gradientX, gradientY, cornerResponse, corners and
cornerLocs of a FeaturesContainer from the CV_8UC1 picture the reference's driver loads -- whole and as an ROI with a
foreign step -- with one micv_harris_corners_u8_host call, and gives the bytes of the harris:: three-call path on the
converted picture.  tests/cpp/harris_u8_demo.cpp does the comparing."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shim_corner_chain_takes_8bit_mats(tmp_path):
    exe = str(tmp_path / "harris_u8_demo")
    lib = os.path.join(ROOT, "introtocomputervision_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-Wno-unused-function", os.path.join(ROOT, "tests", "cpp", "harris_u8_demo.cpp"),
                    "-o", exe, "-L" + lib, "-lmicv", "-Wl,-rpath," + lib], check=True)
    out = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr
