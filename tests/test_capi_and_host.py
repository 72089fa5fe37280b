"""CPU-side checks: libmicv.so loads and exports every symbol include/mi_cv.h declares (no
compute calls here), host-only entry points, the synthetic-input generator and the byte model."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_functions():
    src = open(os.path.join(ROOT, "include", "mi_cv.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(micv_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from introtocomputervision_amd import _capi
    names = header_functions()
    assert len(names) >= 50
    missing = [n for n in names if not hasattr(_capi.lib, n)]
    assert not missing, f"declared in include/mi_cv.h but not exported: {missing}"
    assert not _capi.MISSING
    undeclared = [n for n in names if n not in _capi.SIGNATURES]
    assert not undeclared, f"no ctypes signature for: {undeclared}"
    assert _capi.lib.micv_version().decode().startswith("micv")


def header_prototypes():
    """name -> (return kind, [argument kinds]) of every micv_* prototype in include/mi_cv.h."""
    src = open(os.path.join(ROOT, "include", "mi_cv.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"^\s*#.*$", "", src, flags=re.M)
    src = re.sub(r"\btypedef\b[^;]*;", "", src)
    pointer_types = {"micv_stream", "micv_kernel_log_fn"}
    scalar = {"size_t": "u64", "uint64_t": "u64", "int64_t": "i64", "int": "i32", "int32_t": "i32", "uint32_t": "u32",
              "unsigned": "u32", "unsigned int": "u32", "float": "f32", "double": "f64", "void": "void"}

    def kind(decl, named):
        if "*" in decl or "[" in decl:
            return "p"
        words = [w for w in decl.split() if w != "const"]
        if named and len(words) > 1 and words[-1] not in scalar and words[-1] not in pointer_types:
            words = words[:-1]  # the parameter's name
        t = " ".join(words)
        return "p" if t in pointer_types else scalar[t]

    protos = {}
    for ret, name, args in re.findall(r"([A-Za-z_][\w\s\*]*?)\b(micv_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", src):
        args = " ".join(args.split())
        kinds = [] if args in ("", "void") else [kind(a.strip(), True) for a in args.split(",")]
        assert name not in protos, f"{name} declared twice"
        protos[name] = (kind(" ".join(ret.split()), False), kinds)
    return protos


def ctypes_kind(t):
    import ctypes as C
    if t is None:
        return "void"
    if issubclass(t, (C._Pointer, C._CFuncPtr)):
        return "p"
    code = {"P": "p", "z": "p", "f": "f32", "d": "f64"}.get(t._type_)
    if code:
        return code
    assert t._type_ in "iIlLqQ", t
    return ("u" if t._type_ in "ILQ" else "i") + str(8 * C.sizeof(t))


def test_ctypes_signatures_match_the_header_kind_by_kind():
    """Every prototype of include/mi_cv.h against _capi.SIGNATURES: argument count, the kind of every argument
    (pointer / u64 / i64 / i32 / u32 / f32 / f64) and the kind of the return value.  A stride bound as 32 bits or a
    double bound as a float would pass the export check above and corrupt a call."""
    from introtocomputervision_amd import _capi
    protos = header_prototypes()
    assert sorted(protos) == header_functions(), sorted(set(header_functions()) ^ set(protos))
    assert len(protos) >= 250
    assert protos["micv_lk_level_batch_dev"][1][:5] == ["p", "p", "p", "i32", "u64"]
    assert protos["micv_set_kernel_log"] == ("i32", ["p", "p"]) and protos["micv_div_round_up"] == ("u64", ["u64", "u64"])
    assert protos["micv_ctx_destroy"][0] == "void" and protos["micv_version"] == ("p", [])
    wrong = []
    for name, (ret, kinds) in sorted(protos.items()):
        res, args = _capi.SIGNATURES[name]
        bound = (ctypes_kind(res), [ctypes_kind(a) for a in args])
        if bound != (ret, kinds):
            at = [i for i, (a, b) in enumerate(zip(bound[1], kinds)) if a != b]
            wrong.append(f"{name}: header {ret}({len(kinds)} args), bound {bound[0]}({len(args)} args), arguments {at} differ: "
                         f"{[(kinds[i], bound[1][i]) for i in at]}")
    assert not wrong, "\n".join(wrong)


def test_product_does_not_link_or_reference_the_oracle():
    import subprocess
    so = os.path.join(ROOT, "introtocomputervision_amd", "libmicv.so")
    deps = subprocess.run(["ldd", so], capture_output=True, text=True).stdout
    assert "oracle" not in deps and "torch" not in deps
    for dirpath, _, files in os.walk(os.path.join(ROOT, "introtocomputervision_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".h", ".sh")):
                text = open(os.path.join(dirpath, f), errors="ignore").read()
                assert "liboracle" not in text and "_oracle" not in text and "orc_" not in text, f


def test_host_only_entry_points():
    from introtocomputervision_amd import _capi, hough
    # common::divRoundUp (Utils.h:12-15): max(1, ceil(float(n)/float(d)))
    assert _capi.lib.micv_div_round_up(10, 3) == 4
    assert _capi.lib.micv_div_round_up(0, 16) == 1
    assert _capi.lib.micv_div_round_up(1920, 64) == 30
    assert hough.linesAccumulatorShape(1080, 1920, 1, 1) == (4406, 180)
    assert hough.linesAccumulatorShape(1080, 1920, 2, 7) == (2203, 26)
    with pytest.raises(_capi.MicvError):
        hough.linesAccumulatorShape(0, 10)


def test_errors_do_not_need_a_gpu():
    from introtocomputervision_amd import _capi
    import ctypes as C
    h = _capi.vp()
    rc = _capi.lib.micv_ctx_create(0, C.byref(h))
    if rc == 0:  # a GPU is present: nothing to check here
        _capi.lib.micv_ctx_destroy(h)
        return
    assert rc in (_capi.EHIP, _capi.EINVAL) and _capi.last_error()


def test_splitmix64_reference_values():
    from introtocomputervision_amd import synth
    # splitmix64(seed=0) first outputs: e220a8397b1dcdaf 6e789e6aa1b965f4 06c45d188009454f
    assert synth.splitmix64_u8(0, 3).tolist() == [0xE2, 0x6E, 0x06]
    a = synth.smooth_noise(0x5EED0005, 32, 48)
    assert a.dtype == np.float32 and np.array_equal(a, np.round(a)) and 0 <= a.min() and a.max() <= 255
    p, n = synth.lk_pair(0x5EED0005, 32, 48, 3, -2)
    assert np.array_equal(n[0, 3:], p[2, :-3])  # next(y, x) = prev(y + 2, x - 3)
    l, r, nd = synth.stereo_pair(1, 20, 64)
    assert np.array_equal(r[5, :30], l[5, -nd[5]:-nd[5] + 30])


def test_byte_model_matches_baseline_md():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert b.algorithmic_bytes_pair(1080, 1920, 5) == 55207680
    assert b.algorithmic_bytes_pair(1080, 1920, 4) == 54950400
    assert b.algorithmic_bytes_pair(2160, 3840, 5) == 220838400
    assert b.level0_kernel_bytes_pair(1080, 1920, 5) == 16 * 2073600 + 8 * 518400


def test_bench_dump_rows_are_fixed_and_fit_the_budget():
    """--dump-outputs keeps every row when they fit in 64 MB, else the same seeded sample of rows in every run."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert np.array_equal(b.dump_rows(1080, 1920 * 4, 2), np.arange(1080))
    rows = b.dump_rows(8 * 1080, 1920 * 4, 2)
    assert np.array_equal(rows, b.dump_rows(8 * 1080, 1920 * 4, 2))
    assert np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < 8 * 1080
    assert 2 * (len(rows) * 1920 * 4 + 128) <= 64 * 10**6 < 2 * ((len(rows) + 1) * 1920 * 4 + 128)
    assert b.parse_args(["--steps", "7", "--dump-outputs", "d"]).steps == 7
    with pytest.raises(SystemExit):
        b.parse_args(["--steps", "0"])


def test_bench_gpus_n_launches_n_ranks():
    """`python bench.py --gpus 2` run directly (no torchrun environment) must start 2 ranks itself:
    the launcher spawns torch.distributed.run as a child and relays rank 0's JSON line.  --dry-run
    over gloo: no kernels (there is no CPU fallback), only launcher / rendezvous / MAX / JSON."""
    import json
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo",
                        "--dry-run", "--steps", "3", "--warmup", "1"], capture_output=True, text=True,
                       env=env, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["ranks"] == 2 and len(d["config"]["per_rank_s"]) == 2
    assert d["steps"] == 3 and d["value"] is None and "dry run" in d["data"]
    # a failing child is reported, not swallowed (gloo without --dry-run is refused by every rank)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo",
                        "--steps", "1"], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode != 0 and not [l for l in p.stdout.splitlines() if l.startswith("{")]


def test_no_environment_knobs_in_the_default_build():
    """The shipped library reads no environment variables (options live in the context); the only
    getenv left is behind -DMICV_DIAG."""
    import subprocess
    so = os.path.join(ROOT, "introtocomputervision_amd", "libmicv.so")
    syms = subprocess.run(["nm", "-D", "--undefined-only", so], capture_output=True, text=True).stdout
    assert "getenv" not in syms
    blob = open(so, "rb").read()
    for knob in (b"MICV_LK_STOP", b"MICV_LK_GROUPS", b"MICV_FORCE_GENERIC", b"MICV_LK_NT"):
        assert knob not in blob, knob


def _schedule(rows, cols, batch, win, max_chain):
    import ctypes as C
    from introtocomputervision_amd import _capi
    n, tw, th = _capi.i64(), _capi.i32(), _capi.i32()
    _capi.check(_capi.lib.micv_lk_schedule_host(rows, cols, batch, win, max_chain, None, 0, C.byref(n),
                                                C.byref(tw), C.byref(th)))
    buf = np.zeros((n.value, 4), np.int32)
    _capi.check(_capi.lib.micv_lk_schedule_host(rows, cols, batch, win, max_chain, buf.ctypes.data, n.value,
                                                C.byref(n), C.byref(tw), C.byref(th)))
    return buf, tw.value, th.value


@pytest.mark.parametrize("win", [15, 11, 7])
def test_chain_schedule_covers_every_tile_exactly_once(win):
    """the schedule of the chain / streamed launches probed column tiles_x/2 for the
    interior rows; for cols 194..206 that column is not x-interior and the interior tiles of column 1
    were never scheduled.  Host-only check over the widths around every tile-count change."""
    shapes = [(200, 400), (400, 200), (200, 194), (200, 206), (270, 480), (135, 240), (540, 960), (1080, 1920),
              (33, 64), (64, 65), (300, 129), (97, 333)]
    shapes += [(200, c) for c in range(120, 330, 7)] + [(r, 200) for r in range(40, 300, 13)]
    for rows, cols in shapes:
        for batch in (1, 3):
            for max_chain in (1, 2, 4, 32):
                sched, tw, th = _schedule(rows, cols, batch, win, max_chain)
                assert len(sched) % 8 == 0
                tiles_x, tiles_y = -(-cols // tw), -(-rows // th)
                seen = np.zeros((batch, tiles_y, tiles_x), np.int32)
                for x, y, cnt, p in sched:
                    assert 0 <= cnt <= max_chain
                    if cnt == 0:
                        continue
                    assert 0 <= p < batch and 0 <= x < tiles_x and 0 <= y and y + cnt <= tiles_y, (rows, cols, x, y, cnt)
                    seen[p, y:y + cnt, x] += 1
                assert (seen == 1).all(), (win, rows, cols, batch, max_chain, np.argwhere(seen != 1)[:5])


def test_cmake_build_exports_the_same_abi(tmp_path):
    """The top-level CMakeLists.txt (HIP language, gfx950) is the integration entry point SURVEY.md section 7
    describes: configure + build it from scratch and check that its libmicv.so exports exactly the symbols
    include/mi_cv.h declares, and links neither torch nor the oracle."""
    import shutil
    import subprocess
    if not (shutil.which("cmake") and shutil.which("ninja") and os.path.exists("/opt/rocm/lib/llvm/bin/clang++")):
        pytest.skip("cmake / ninja / ROCm clang not available")
    b = str(tmp_path / "build")
    r = subprocess.run(["cmake", "-S", ROOT, "-B", b, "-G", "Ninja"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    r = subprocess.run(["cmake", "--build", b], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    so = os.path.join(b, "libmicv.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True).stdout
    exported = sorted(set(re.findall(r" T (micv_[a-z0-9_]+)$", syms, flags=re.M)))
    assert exported == header_functions()
    deps = subprocess.run(["ldd", so], capture_output=True, text=True).stdout
    assert "amdhip64" in deps and "torch" not in deps and "oracle" not in deps
    assert os.path.exists(os.path.join(b, "liboracle.so"))


def test_hand_placed_lds_loads_are_not_touched_before_their_wait():
    """The column pass of the LK level kernel reads LDS with inline-asm ds_read2st64_b32 (the compiler's own
    load merging costs a v_mov per value there).  hipcc does not count asm loads: a copy, spill or reuse of a
    destination register between the load and the asm `s_waitcnt lgkmcnt(0)` would read stale data, depending
    on timing.  tools/audit_asm_loads.py compiles lk_fused.hip and checks the ISA of every kernel; its
    detector is checked first on a doctored listing.  The same holds for stereo_exact.hip's asm s_load_dwordx8
    look-ahead (SGPRs, one column ahead, across the loop's back-edge): its control-flow walk is checked on doctored
    listings too -- a copy, a spill, a refill, an unwaited branch path, a back-edge, an s_endpgm.  The source must not
    reintroduce a switch that makes the kernels compute wrong sums on purpose (the removed MICV_SX_NOMASK)."""
    import importlib.util
    import subprocess
    import sys
    spec = importlib.util.spec_from_file_location("audit", os.path.join(ROOT, "tools", "audit_asm_loads.py"))
    audit = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(audit)
    good = """_Zk:
\t;;#ASMSTART
\tds_read2st64_b32 v[4:5], v9 offset0:1 offset1:5
\t;;#ASMEND
\tv_add_u32_e32 v1, v2, v3
\t;;#ASMSTART
\ts_waitcnt lgkmcnt(0)
\t;;#ASMEND
\tv_pk_fma_f32 v[6:7], v[4:5], s[0:1], v[6:7]
"""
    assert audit.audit(good) == ([], 1, 1)
    for bad_line in ("\tv_mov_b32_e32 v8, v5", "\tv_pk_fma_f32 v[6:7], v[4:5], s[0:1], v[6:7]", "\ts_barrier"):
        bad = good.replace("\tv_add_u32_e32 v1, v2, v3", bad_line)
        problems, loads, kernels = audit.audit(bad)
        assert len(problems) == 1 and loads == 1, bad_line

    # stereo_exact.hip's scalar look-ahead: one s_load_dwordx8 before the column loop, one per column, retired at the top of
    # the next column (across the back-edge) and once more behind the loop.  The walk follows the control-flow graph.
    sgood = """_Zs:
\ts_mov_b32 s2, 0
\t;;#ASMSTART
\ts_load_dwordx8 s[36:43], s[14:15], 0x1c0
\t;;#ASMEND
.LBB0_1:                                ; loop header
\tv_add_u32_e32 v1, v2, v3
\t;;#ASMSTART
\ts_waitcnt lgkmcnt(0)
\t;;#ASMEND
\ts_and_b32 s18, s39, 0xffffff
\tv_dot4_u32_u8 v4, s36, v5, v4
\t;;#ASMSTART
\ts_load_dwordx8 s[36:43], s[34:35], 0x1e0
\t;;#ASMEND
\tds_read_b32 v6, v7
\ts_add_i32 s2, s2, 1
\ts_cmp_lt_i32 s2, 4
\ts_cbranch_scc1 .LBB0_1
; %bb.2:
\t;;#ASMSTART
\ts_waitcnt lgkmcnt(0)
\t;;#ASMEND
\ts_endpgm
"""
    assert audit.audit_scalar(sgood) == ([], 2, {"_Zs": 2})
    assert audit.audit(sgood)[0] == []  # no hand-placed LDS load: nothing for the counted-window audit
    doctored = {
        "copy": ("\tds_read_b32 v6, v7", "\tds_read_b32 v6, v7\n\ts_mov_b32 s50, s37"),
        "spill": ("\tds_read_b32 v6, v7", "\tds_read_b32 v6, v7\n\tv_writelane_b32 v200, s38, 4"),
        "refill": ("\tds_read_b32 v6, v7", "\tds_read_b32 v6, v7\n\tv_readlane_b32 s40, v200, 4"),
        "branch": ("\ts_add_i32 s2, s2, 1", "\ts_cbranch_execz .LBB0_3\n\ts_add_i32 s2, s2, 1"),
        # the preheader waits, so only the back-edge reaches the header's use ahead of its wait (a linear scan sees the
        # use BEFORE the load in the text)
        "loop": ("\t;;#ASMEND\n.LBB0_1:", "\t;;#ASMEND\n\ts_waitcnt lgkmcnt(0)\n.LBB0_1:"),
        "endpgm": ("; %bb.2:\n\t;;#ASMSTART\n\ts_waitcnt lgkmcnt(0)\n\t;;#ASMEND\n", "; %bb.2:\n"),
    }
    for name, (old, new) in doctored.items():
        assert old in sgood, name
        bad = sgood.replace(old, new, 1)
        if name == "branch":
            bad += ".LBB0_3:\n\ts_and_b32 s18, s39, 0xff\n\ts_endpgm\n"
        if name == "loop":
            bad = bad.replace("\tv_add_u32_e32 v1, v2, v3", "\tv_add_u32_e32 v1, s36, v3")
        problems, loads, _ = audit.audit_scalar(bad)
        assert len(problems) == 1 and loads == 2, (name, problems)
        want = {"copy": "s_mov_b32 s50, s37", "spill": "v_writelane_b32", "refill": "v_readlane_b32",
                "branch": "s_and_b32 s18, s39, 0xff", "loop": "v_add_u32_e32 v1, s36, v3", "endpgm": "s_endpgm"}[name]
        assert want in problems[0][2], (name, problems)
    assert len(audit.REQUIRED_SCALAR) == 2 * (7 + 6 + 5)  # RPW 8 / 10 x (full r 1..7, COLS_2R r 2..7, serial r 1..5)
    for f in ("introtocomputervision_amd/csrc/stereo_exact.hip", "introtocomputervision_amd/csrc/build.sh", "CMakeLists.txt",
              "tools/audit_asm_loads.py"):
        assert "SX_NOMASK" not in open(os.path.join(ROOT, f)).read(), f
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "audit_asm_loads.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert ", 0 problems" in r.stdout and " 0 hand-placed" not in r.stdout
    assert " hand-placed scalar loads in 36 stereo search kernels" in r.stdout, r.stdout[-2000:]


def test_shim_functions_have_the_reference_headers_types():
    """tests/cpp/shim_signatures.cpp: one static_assert per shim function against the type the reference header declares
    (ps5 OpticalFlow.h / Pyramids.h, ps4 Harris.h / Descriptors.h, ps2 Disparity*.h, ps1 Hough.h, ps7 MotionHistory.h),
    plus calls that rely on the reference's default arguments.  Compile-only (VERDICT r4 Missing #3; the first run of it
    found lk::calcOpticalFlowPyr carrying a sixth parameter)."""
    import subprocess
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-Wno-unused-function", "-I" + ROOT,
                        "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "shim_signatures.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_comm_builds_without_the_rccl_header(tmp_path):
    """RCCL is dlopen'ed; comm.hip must not need <rccl/rccl.h> to BUILD: -DMICV_NO_RCCL_HEADER compiles the
    branch with the local declarations of the NCCL 2.x ABI subset (the header branch static_asserts that they agree)."""
    import subprocess
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "introtocomputervision_amd", "csrc", "comm.hip")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O1", "-std=c++17", "-fPIC", "-DMICV_NO_RCCL_HEADER",
                        "-c", src, "-o", str(tmp_path / "comm.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_level_kernel_name_needs_no_gpu_and_follows_the_options():
    """micv_lk_level_kernel_name is answered by the launch dispatch itself (nothing is launched).  No GPU here, so the
    context cannot be created: only the symbol and its argument checks are exercised on the CPU; the GPU suite
    compares names with what rocprofv3 reports (tests/test_lk_gpu.py)."""
    from introtocomputervision_amd import _capi
    assert hasattr(_capi.lib, "micv_lk_level_kernel_name")
    import ctypes as C
    buf = C.create_string_buffer(160)
    assert _capi.lib.micv_lk_level_kernel_name(None, 15, 1080, 1920, 8, buf, 160) == _capi.EINVAL


def test_hough_entry_points_refuse_what_they_cannot_index():
    """The limits the Hough entry points enforce, checked before the context is used (so no GPU is needed: the
    context argument only has to be non-null here).  Lines and circles: rows, cols <= 32767 (the circle kernel packs
    (y, x) into 15 bits each; the line accumulator is then at most 92 680 x 180 cells).  Peaks: fewer than 2^31
    accumulator cells (32-bit candidate indices) and num_peaks <= 4096.  Bands must lie inside the image."""
    import ctypes as C
    from introtocomputervision_amd import _capi, hough
    lib = _capi.lib
    fake = C.create_string_buffer(64)  # stands in for the context, the accumulator and the count
    p = C.addressof(fake)
    with pytest.raises(_capi.MicvError, match="bad argument"):
        hough.linesAccumulatorShape(32768, 10)
    assert hough.linesAccumulatorShape(32767, 32767, 1, 1) == (92680, 180)
    assert lib.micv_hough_circles_dev(p, p, 10, 32768, 32768, 5, p, None) == _capi.EINVAL
    assert "bad size 10x32768" in _capi.last_error()
    assert lib.micv_hough_circles_band_dev(p, p, 10, 20, 20, 95, 100, 5, p, None) == _capi.EINVAL
    assert "band [95, 105) outside the 100-row image" in _capi.last_error()
    assert lib.micv_hough_lines_band_dev(p, p, 10, 20, 20, -1, 100, 1, 1, p, None) == _capi.EINVAL
    assert "outside the 100-row image" in _capi.last_error()
    assert lib.micv_hough_peaks_dev(p, p, 65536, 32768, 10, 0, p, p, None) == _capi.EINVAL
    assert "bad size 65536x32768" in _capi.last_error()
    assert lib.micv_hough_peaks_dev(p, p, 10, 10, 4097, 0, p, p, None) == _capi.EINVAL
    assert "num_peaks 4097 > 4096" in _capi.last_error()
    assert lib.micv_hough_peaks_dev(p, p, 10, 10, 5, 0, None, p, None) == _capi.EINVAL
    assert "peaks_rc is null" in _capi.last_error()
