"""SIFT descriptors on 8-bit images and the counted matcher, the parts that need no GPU: the four entry points are declared in
include/mi_cv.h, exported by libmicv.so and bound in _capi.py with the argument kinds the header gives them; `_dev` without
its stream is `_host` apart from n standing in for cap and count; the null-context refusals; the Python entries refuse the
wrong dtype by name; micv_ps4::siftDescriptors8 compiles and links on an 8-bit ROI and calls the u8 entry."""
import os
import subprocess

import pytest

from test_harris_u8_api import declared_arguments, kind

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("micv_sift_descriptors_u8_dev", "micv_sift_descriptors_u8_host", "micv_sift_descriptors_u8_batch_dev", "micv_bf_knn2_counted_dev")


@pytest.mark.parametrize("name", NAMES)
def test_declared_exported_and_bound(name):
    from introtocomputervision_amd import _capi
    args = declared_arguments(name)
    assert hasattr(_capi.lib, name), f"{name} is not exported by libmicv.so"
    restype, argtypes = _capi.SIGNATURES[name]
    assert restype is _capi.i32 and len(argtypes) == len(args), (len(argtypes), args)
    for decl, ctype in zip(args, argtypes):
        assert ctype is kind(decl, _capi), (name, decl, ctype)
    assert args[-1].startswith("micv_stream") == name.endswith("_dev")
    assert args[1].startswith("const uint8_t *" if "sift" in name else "const float *")
    # no context: refused with a message before anything else is looked at
    zeros = [None if t is _capi.vp else 0 for t in argtypes]
    assert getattr(_capi.lib, name)(*zeros) == _capi.EINVAL and _capi.last_error()


def test_argument_orders():
    dev, host, batch, knn = (declared_arguments(n) for n in NAMES)
    # _dev without its stream is _host, apart from n standing in for cap and count
    assert [a for a in dev[:-1] if a not in ("int64_t cap", "const int64_t *count")] == [a for a in host if a != "int64_t n"]
    assert dev.index("int64_t cap") == host.index("int64_t n") and dev[dev.index("int64_t cap") + 1] == "const int64_t *count"
    # the f32 entry's list and output arguments in its order, the planes replaced by the bytes
    f32 = declared_arguments("micv_sift_descriptors_host")
    assert host[0] == f32[0] and host[1] == "const uint8_t *img" and host[2:4] == f32[3:5] and host[5:] == f32[6:]
    # the batch entry: those, plus the batch and one distance between images for the input and for the descriptors
    assert [a for a in batch if a not in dev] == ["size_t image_stride", "int batch", "size_t dimage_stride"]
    assert [a for a in batch if a in dev] == dev
    # the counted matcher: micv_bf_knn2_dev's arguments with caps for lengths and a device count after each stride
    plain = declared_arguments("micv_bf_knn2_dev")
    assert [a for a in knn if "count" not in a] == [a.replace("int nq", "int nq_cap").replace("int nt", "int nt_cap") for a in plain]
    assert knn[knn.index("size_t qstride") + 1] == "const int64_t *nq_count" and knn[knn.index("size_t tstride") + 1] == "const int64_t *nt_count"


def test_python_entry_points_refuse_the_wrong_dtype_by_name():
    import numpy as np
    from introtocomputervision_amd import harris, match, ps4
    f, kp = np.zeros((8, 8), np.float32), np.zeros((1, 4), np.float32)
    with pytest.raises(ValueError, match="uint8"):
        harris.computeDescriptors8(f, kp)
    with pytest.raises(ValueError, match="uint8"):
        harris.computeDescriptors8Batch(f[None], kp[None])
    with pytest.raises(ValueError, match="uint8"):
        harris.computeDescriptors8Batch(f.astype(np.uint8)[None], kp[None])  # a numpy batch: the entry is device-only
    with pytest.raises(ValueError, match="float32"):  # the float entries are unchanged: they refuse bytes
        harris.computeDescriptors(f.astype(np.uint8), f.astype(np.uint8), kp)
    with pytest.raises(ValueError, match="float32"):
        harris.getGradients(f.astype(np.uint8))
    with pytest.raises(ValueError, match="float32 CUDA"):
        match.knnMatch2Counted(f, f, None, None)
    for fn in (ps4.runProblem2_8, ps4.runProblem3_8):
        with pytest.raises(ValueError, match="CUDA"):
            fn(f.astype(np.uint8), f.astype(np.uint8), {}, *(("SIMILARITY",) if fn is ps4.runProblem3_8 else ()))


def test_shim_descriptors_compile_link_and_call_the_u8_entry(tmp_path):
    src = tmp_path / "sift_u8_calls.cpp"
    src.write_text('#include "introtocomputervision_amd/shim/micv_ps4.hpp"\n'
                   'void calls() {\n'
                   '    micv_shim::Mat big(20, 40, micv_shim::U8);\n'
                   '    micv_shim::Mat roi(16, 30, micv_shim::U8, big.ptr<uint8_t>(1) + 3, big.step);\n'
                   '    std::vector<micv_shim::KeyPoint> kps(1, micv_shim::KeyPoint(8.f, 8.f, 4.f, 30.f));\n'
                   '    micv_shim::Mat desc;\n'
                   '    micv_ps4::siftDescriptors8(roi, kps, desc);\n'
                   '}\n'
                   'int main(int argc, char **) {\n'
                   '    if (argc > 100) calls();\n'
                   '    return 0;\n'
                   '}\n')
    lib = os.path.join(ROOT, "introtocomputervision_amd")
    obj, exe = str(tmp_path / "sift_u8_calls.o"), str(tmp_path / "sift_u8_calls")
    for cmd in (["g++", "-std=c++17", "-O0", "-Wall", "-Werror", "-Wno-unused-function", "-I" + ROOT, "-c", str(src), "-o", obj],
                ["g++", obj, "-o", exe, "-L" + lib, "-lmicv", "-Wl,-rpath," + lib]):
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    syms = subprocess.run(["nm", "-u", obj], capture_output=True, text=True).stdout.split()
    assert "micv_sift_descriptors_u8_host" in syms, "micv_ps4::siftDescriptors8 does not call the u8 entry"
    assert "micv_sift_descriptors_host" not in syms, "the translation unit still reaches the f32 entry"
