"""The shim on 8-bit Mats: cuda::disparitySSD, serial::disparitySSD and ps2::disparitySSDPair take the CV_8UC1 images the
reference's driver loads (ROI views included, steps that differ) and give the bytes of the same calls on the converted
pair; disparityNCorr refuses them with a message.  tests/cpp/stereo_u8_demo.cpp does the comparing."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shim_takes_8bit_mats(tmp_path):
    exe = str(tmp_path / "stereo_u8_demo")
    lib = os.path.join(ROOT, "introtocomputervision_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "stereo_u8_demo.cpp"),
                    "-o", exe, "-L" + lib, "-lmicv", "-Wl,-rpath," + lib], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr
