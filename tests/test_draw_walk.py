"""csrc/draw.hpp, the one rasteriser header of the overlay kernels, against the contract on the CPU: the line walk's clip with
its narrow and wide minor advance, the midpoint circle with its reach test and cvRound are built as a stand-alone program
(tools/probes/draw_walk_check.cpp) with the address and undefined-behaviour sanitizers; every lane runs one by one and the
pictures must equal those of micv_viz::line, micv_ps4::line / circle and micv_ps3::line_wide."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def test_draw_header_under_the_sanitizers_equals_the_contract(tmp_path):
    exe = str(tmp_path / "draw_walk_check")
    subprocess.run(SAN + ["-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "probes", "draw_walk_check.cpp"), "-o", exe],
                   check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stdout + run.stderr
    # every part ran: the exhaustive lattice (20 * 18 end points, squared), the long strokes, the int32 range, the circles
    for part in ("lattice: 129600 segments", "long: 1000 segments", "int32: ", "circles: 14760 and ", "cvRound: ", "draw_walk_check: ok"):
        assert part in run.stdout, run.stdout
