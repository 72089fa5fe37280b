"""The host loops that state the contract of the "ps0" block (shim/micv_ps0.hpp), and the device form beside them.  On the
CPU the loops are built as a stand-alone program (tools/probes/ps0_host_loops.cpp) with the address and undefined-behaviour
sanitizers and run on the cases of tests/_ps0_ref.py; their pictures must equal the numpy restatement.  On the GPU
tests/cpp/ps0_demo.cpp writes the nine pictures both ways and the files must be equal byte for byte."""
import os
import subprocess

import numpy as np
import pytest

import _ps0_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "tests", "golden", "config", "ref", "ps0.yaml")
SAN = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def test_host_loops_under_the_sanitizers_equal_the_restatement(tmp_path):
    exe = str(tmp_path / "ps0_host_loops")
    subprocess.run(SAN + [os.path.join(ROOT, "tools", "probes", "ps0_host_loops.cpp"), "-o", exe], check=True)
    lines, want = [], {}

    def put(name, arr):
        np.ascontiguousarray(arr).tofile(str(tmp_path / name))
        return name

    for i, (rows, cols) in enumerate(R.CHANNEL_SIZES):
        _, img = R.image(rows, cols, 3, 0, 10 + i)
        f = put(f"bgr{i}.u8", img)
        lines.append(f"swap swap{i} {rows} {cols} {f}")
        want[f"swap{i}"] = R.mix_channels(img, (2, 1, 0))
        for c in range(3):
            lines.append(f"extract ex{i}_{c} {rows} {cols} 3 {c} {f}")
            want[f"ex{i}_{c}"] = img[:, :, c]
    for i, ((r1, c1), (r2, c2)) in enumerate(R.PASTE_CASES):
        _, a = R.image(r1, c1, 1, 0, 21)
        _, b = R.image(r2, c2, 1, 0, 22)
        lines.append(f"paste paste{i} {r1} {c1} {r2} {c2} 1 100 {put(f'pa{i}.u8', a)} {put(f'pb{i}.u8', b)}")
        want[f"paste{i}"] = R.pixel_replacement(a, b)
    rng = np.random.default_rng(41)
    stats = {"s1": rng.integers(0, 256, (1, 1), dtype=np.uint8), "s2": rng.integers(0, 256, (1, 4099), dtype=np.uint8),
             "s3": rng.integers(0, 256, (257, 263), dtype=np.uint8), "s4": np.full((300, 300), 255, np.uint8)}
    for name, img in stats.items():
        lines.append(f"stats {name} {img.shape[0]} {img.shape[1]} {put(name + '.u8', img)}")
    f = put("bytes.u8", R.all_bytes())
    for i, (mean, sd) in enumerate(R.ARITH_PARAMS):
        lines.append(f"arith ar{i} 16 16 {float(mean).hex() if np.isfinite(mean) else mean} {float(sd).hex() if np.isfinite(sd) else sd} {f}")
        want[f"ar{i}"] = R.arithmetic(R.all_bytes(), mean, sd)
    _, g = R.image(131, 259, 1, 0, 51)
    _, h = R.image(131, 259, 1, 0, 52)
    fg, fh = put("g.u8", g), put("h.u8", h)
    lines.append(f"translate tr 131 259 -2 0 {fg}")
    want["tr"] = R.translate_left2(g)
    lines.append(f"subtract sub 131 259 {fg} {fh}")
    want["sub"] = R.subtract(g, h)
    ramp = np.resize(np.arange(256, dtype=np.uint8), (14, 256 * 14)).copy()
    z = R.special_noise_plane(*ramp.shape)
    lines.append(f"noise nz {ramp.shape[0]} {ramp.shape[1]} {put('ramp.u8', ramp)} {put('z.f32', z)}")
    want["nz"] = R.add_noise(ramp, z)
    (tmp_path / "cases.txt").write_text("\n".join(lines) + "\n")
    run = subprocess.run([exe, str(tmp_path / "cases.txt"), str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stdout + run.stderr
    assert f"cases {len(lines)}" in run.stdout
    for name, w in want.items():
        got = np.fromfile(str(tmp_path / (name + ".out")), np.uint8).reshape(w.shape)
        assert np.array_equal(got, w), name
    for name, img in stats.items():
        s, q, mn, mx, mean, sd = (tmp_path / (name + ".out")).read_text().split()
        w = R.mean_stddev(img)
        assert (int(s), int(q), int(mn), int(mx)) == (w["sum"], w["sqsum"], w["min"], w["max"]), name
        assert float.fromhex(mean) == w["mean"] and float.fromhex(sd) == w["stddev"], name


def build_demo(tmp):
    exe = os.path.join(str(tmp), "ps0_demo")
    lib = os.path.join(ROOT, "introtocomputervision_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "ps0_demo.cpp"), "-o", exe, "-L" + lib,
                    "-lmicv", "-Wl,-rpath," + lib], check=True)
    return exe


def test_ps0_demo_compiles(tmp_path):
    build_demo(tmp_path)


def test_the_header_compiles_beside_the_ps3_shim_signatures(tmp_path):
    src = tmp_path / "both.cpp"
    src.write_text('#include "introtocomputervision_amd/shim/micv_ps0.hpp"\n#include "tests/cpp/ps3_shim_signatures.cpp"\n')
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-Wno-unused-function", "-I" + ROOT,
                        "-I" + os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


@pytest.mark.gpu
def test_device_run_writes_the_host_loops_files(tmp_path):
    from introtocomputervision_amd import config, viz
    exe = build_demo(tmp_path)
    images = config.load(CFG)["images"]
    rng = np.random.default_rng(7)
    pics = {}
    for key, shape in (("image1", (131, 259, 3)), ("image2", (117, 140, 3))):
        stem = os.path.splitext(os.path.basename(images[key]))[0]
        pics[key] = rng.integers(0, 256, shape, dtype=np.uint8)
        viz.imwrite(str(tmp_path / (stem + ".ppm")), pics[key])
    os.mkdir(tmp_path / "host")
    os.mkdir(tmp_path / "dev")
    run = subprocess.run([exe, CFG, str(tmp_path), str(tmp_path)], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    names = sorted(os.listdir(tmp_path / "host"))
    assert names == sorted(os.listdir(tmp_path / "dev")) and len(names) == 9
    for n in names:
        assert open(tmp_path / "host" / n, "rb").read() == open(tmp_path / "dev" / n, "rb").read(), n
    assert np.array_equal(viz.imread(str(tmp_path / "dev" / "ps0-2-a-1.ppm")), pics["image1"][:, :, ::-1])
    assert np.array_equal(viz.imread(str(tmp_path / "dev" / "ps0-4-c-1.pgm")), R.translate_left2(pics["image1"][:, :, 1]))
