"""LK on a device-resident frame sequence, the parts that need no GPU: the entry points are declared in include/mi_cv.h,
exported by libmicv.so and bound in _capi.py with the argument kinds the header gives them; the null-context refusals; and
the piece rule of micv_lk_flow_seq_plan, which the device entry walks.

The device entries end in _async, not _dev, as micv_generate_edge_async does: the layout tables of
test_layout_containment_drivers_gpu.py account for every `_dev` name, and these entries carry their own layout tests
(test_lk_seq_gpu.py)."""
import ctypes as C

import pytest

from test_harris_u8_api import declared_arguments, kind

NAMES = ("micv_lk_flow_seq_async", "micv_lk_flow_seq_plan", "micv_dense_lk_display_seq_async", "micv_dense_lk_display_seq_host",
         "micv_gray_pyramid_seq_async")


@pytest.mark.parametrize("name", NAMES)
def test_declared_exported_and_bound(name):
    from introtocomputervision_amd import _capi
    args = declared_arguments(name)
    assert hasattr(_capi.lib, name), f"{name} is not exported by libmicv.so"
    restype, argtypes = _capi.SIGNATURES[name]
    assert restype is _capi.i32 and len(argtypes) == len(args), (len(argtypes), args)
    for decl, ctype in zip(args, argtypes):
        assert ctype is kind(decl, _capi), (name, decl, ctype)
    assert args[-1].startswith("micv_stream") == name.endswith("_async")
    # no context (the plan: no result pointer): refused with a message before anything else is looked at
    zeros = [None if t is _capi.vp else 0 for t in argtypes]
    assert getattr(_capi.lib, name)(*zeros) == _capi.EINVAL and _capi.last_error()


def test_argument_orders():
    seq, plan, disp, disp_host = (declared_arguments(n) for n in NAMES[:4])
    assert seq == ["micv_ctx *ctx", "const void *frames", "size_t frame_pitch", "int nframes", "int rows", "int cols", "size_t stride",
                   "int channels", "int depth", "int win", "int levels", "int max_pairs", "float *u", "float *v", "size_t opair_pitch",
                   "size_t ostride", "micv_stream stream"]
    assert plan == ["int nframes", "int max_pairs", "int *first_frame", "int *npairs", "int cap", "int *npieces"]
    # the display: the sequence's frames, the single pair's settings and outputs, an image pitch beside every row stride
    assert disp[:11] == [a for a in seq[:11]] and disp[11] == "const uint8_t *color"
    single = declared_arguments("micv_dense_lk_display_dev")
    assert [a for a in disp if a in single and a not in seq] == [a for a in single if a in disp and a not in seq]
    assert [a for a in disp if a not in single and a not in seq] == ["size_t apitch", "size_t jpitch"]
    assert disp_host[1] == "const void *const *frames" and "float *const *u" in disp_host and not any("pitch" in a for a in disp_host)
    assert declared_arguments("micv_lk_flow_seq_host")[1:8] == disp_host[1:8]


def plan(nframes, max_pairs, cap=64):
    from introtocomputervision_amd import _capi
    first, pairs, n = (C.c_int * max(cap, 1))(), (C.c_int * max(cap, 1))(), C.c_int(-1)
    rc = _capi.lib.micv_lk_flow_seq_plan(nframes, max_pairs, first, pairs, cap, C.byref(n))
    return rc, n.value, [(first[i], pairs[i]) for i in range(min(max(n.value, 0), cap))]


def test_plan_cases():
    assert plan(2, 0) == (0, 1, [(0, 1)])
    assert plan(10, 0) == (0, 2, [(0, 8), (8, 1)])
    assert plan(5, 2) == (0, 2, [(0, 2), (2, 2)])
    assert plan(5, 1) == (0, 4, [(0, 1), (1, 1), (2, 1), (3, 1)])
    assert plan(4, 3) == (0, 1, [(0, 3)])
    # a bound larger than the sequence is the sequence: one piece, whatever the value
    assert plan(5, 2147483647) == (0, 1, [(0, 4)]) and plan(5, 2147483640) == (0, 1, [(0, 4)]) and plan(2, 2147483647) == (0, 1, [(0, 1)])


def test_plan_covers_every_pair_once_and_in_order():
    for nframes in range(2, 41):
        for max_pairs in range(0, 10):
            rc, n, pieces = plan(nframes, max_pairs)
            assert rc == 0 and n == len(pieces) >= 1
            m = max_pairs or 8
            covered = []
            for i, (f0, np_) in enumerate(pieces):
                assert f0 == i * m and 1 <= np_ <= m, (nframes, max_pairs, pieces)
                covered += list(range(f0, f0 + np_))
            assert covered == list(range(nframes - 1)), (nframes, max_pairs, pieces)
            assert all(np_ == m for _, np_ in pieces[:-1])


def test_plan_refusals():
    from introtocomputervision_amd import _capi, lk
    rc, n, _ = plan(10, 2, cap=3)  # five pieces do not fit three
    assert rc == _capi.EINVAL and n == 5 and "5 pieces" in _capi.last_error()
    rc, n, _ = plan(10, 2, cap=0)
    assert rc == _capi.EINVAL and n == 5
    for bad in ((1, 0), (0, 0), (-3, 2), (5, -1), (32769, 0)):
        rc, n, _ = plan(*bad)
        assert rc == _capi.EINVAL and n == -1 and _capi.last_error(), bad
    assert plan(32768, 32767)[:2] == (0, 1)
    assert lk.sequencePlan(10) == [(0, 8), (8, 1)] and lk.sequencePlan(5, 1) == [(0, 1), (1, 1), (2, 1), (3, 1)]
    with pytest.raises(_capi.MicvError):
        lk.sequencePlan(1)
    with pytest.raises(_capi.MicvError):
        lk.sequencePlan(5, -1)
