"""csrc/hyst_uf.hpp, the union-find core of the hysteresis without a host wait, on the CPU: tests/cpp/hyst_uf_host.cpp runs
its four phases over the crafted masks (word and row edges, serpentines, diagonals, checkerboards, random fields, the
degenerate ones), on one thread and on eight, against a plain flood -- built plain, and once more with the address and
undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "hyst_uf_host.cpp")
FLAVOURS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]}


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_union_find_core_equals_the_flood(tmp_path, flavour):
    exe = str(tmp_path / "hyst_uf_host")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-pthread"] + FLAVOURS[flavour] + [SRC, "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stdout + run.stderr
    assert "hyst_uf_host: ok, 894 runs" in run.stdout, run.stdout
