"""disparitySSD's float kernels path by path (csrc/stereo_float.hpp's stereo_tile, stereo_rolling_kernel and
stereo_generic_kernel in csrc/stereo.hip) against references that share nothing with the C oracle: every case of
tests/_stereo_float_cases.py runs on the device and must equal tests/_stereo_f32_ref.py's order-exact float32
restatement (`ssd_f32`, `ssd_serial_f32`) byte for byte; on finite float images the output must also lie in the
float64 admissible set (`ssd_admissible`), which no reading of the summation order can leave.

Routes: a context that never takes the exact-sum kernels (MICV_OPT_STEREO_EXACT = -1: the float launch), the default
context where stereo_exact_covers() holds (the float tiles ride as trailing workgroups of the exact-sum launch and
run because the pre-pass finds a pixel that is not 8-bit-valued), the host entry for some, and one sequence of float
and 8-bit pairs on a single default context (the fallback flag word and its epoch)."""
import numpy as np
import pytest

import _stereo_f32_ref as R
import _stereo_float_cases as T
import _stereo_ref as iref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

_CTX = {}


def ctx_for(key):
    """One context per option set for the whole module (creating contexts per case is slow)."""
    from introtocomputervision_amd import _capi
    if key not in _CTX:
        c = _capi.Context(0)
        for k, v in key:
            c.set_option(getattr(_capi, k), v)
        _CTX[key] = c
    return _CTX[key]


def dev(a, pad=0):
    """Device copy of a 2-D float array; pad > 0 gives it a row pitch of cols + pad elements."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    if pad == 0:
        return torch.from_numpy(a).cuda()
    wide = torch.full((a.shape[0], a.shape[1] + pad), 7.0, dtype=torch.float32, device="cuda")
    wide[:, :a.shape[1]] = torch.from_numpy(a).cuda()
    return wide[:, :a.shape[1]]


def same(got, exp, what):
    assert got.shape == exp.shape and got.dtype == exp.dtype == np.int8, what
    bad = got != exp
    if bad.any():
        idx = np.argwhere(bad)
        raise AssertionError(f"{what}: {len(idx)} of {exp.size} pixels differ, first {idx[:4].tolist()}: "
                             f"got {got[bad][:4].tolist()}, want {exp[bad][:4].tolist()}")


def admitted(vol, got, lo, what):
    ok = R.ssd_admits(vol, got, lo)
    if not ok.all():
        idx = np.argwhere(~ok)[:4]
        cells = [(tuple(i.tolist()), int(got[tuple(i)]), (np.nonzero(vol[:, i[0], i[1]])[0] + lo - 1).tolist()) for i in idx]
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.size} pixels outside the float64 admissible set, first "
                             f"(pixel, got, admissible; {lo - 1} = the output -1): {cells}")


def run(c, left, right, route):
    from introtocomputervision_amd import stereo
    key = (("OPT_STEREO_EXACT", -1 if route == "float" else 0), ("OPT_STEREO_ROWS", c.rpw))
    if route == "host":
        return np.asarray(stereo.disparitySSD(left, right, c.rad, c.lo, c.hi, c.flags, ctx=ctx_for(key)))
    return stereo.disparitySSD(dev(left, c.pad), dev(right, c.pad), c.rad, c.lo, c.hi, c.flags, ctx=ctx_for(key)).cpu().numpy()


@pytest.mark.parametrize("c", T.CASES, ids=[c.id for c in T.CASES])
def test_float_path(c):
    left, right = T.make_pair(c)
    if c.flags & T.SERIAL:
        exp = R.ssd_serial_f32(left, right, c.rad, c.lo, c.hi)
    else:
        exp = R.ssd_f32(left, right, c.rad, c.lo, c.hi, c.flags)
    vol = None
    if c.kind in T.FINITE_FLOAT_KINDS and not c.flags & T.SERIAL:
        vol = R.ssd_admissible(left, right, c.rad, c.lo, c.hi, c.flags)
    for route in c.routes:
        got = run(c, left, right, route)
        what = f"{route} route, {c.id}"
        same(got, exp, what)
        if vol is not None:
            admitted(vol, got, c.lo, what)


def test_float_and_8bit_pairs_alternate_on_one_context():
    """float pair, 8-bit pair, float pair of another size, 8-bit pair on ONE default context: the float tiles must run
    exactly when the pre-pass raised this call's epoch in the flag word, and leave at once otherwise."""
    from introtocomputervision_amd import _capi, stereo
    ctx = _capi.Context(0)
    try:
        rng = np.random.default_rng(404)
        for rad, flags in ((3, 0), (5, T.COLS_2R | T.MIN_SSD_5E6), (4, T.SERIAL)):
            steps = [("float", 33, 117), ("u8", 33, 117), ("float", 41, 59), ("u8", 41, 59), ("float", 41, 59)]
            for n, (kind, rows, cols) in enumerate(steps):
                if kind == "float":
                    left = (rng.random((rows, cols)) * 255).astype(np.float32)
                    other = (rng.random((rows, cols)) * 255).astype(np.float32)
                else:
                    left = rng.integers(0, 256, (rows, cols)).astype(np.float32)
                    other = rng.integers(0, 256, (rows, cols)).astype(np.float32)
                right = np.ascontiguousarray(np.roll(left, -7, axis=1))
                right[::3] = other[::3]
                if flags & T.MIN_SSD_5E6:
                    right[:, cols // 2:] = 255 - right[:, cols // 2:]
                lo, hi = -70, 9
                got = stereo.disparitySSD(dev(left), dev(right), rad, lo, hi, flags, ctx=ctx).cpu().numpy()
                what = f"step {n} ({kind} pair {rows}x{cols}) r={rad} flags={flags}"
                if flags & T.SERIAL:
                    same(got, R.ssd_serial_f32(left, right, rad, lo, hi), what)
                else:
                    same(got, R.ssd_f32(left, right, rad, lo, hi, flags), what)
                if kind == "u8":  # and the integer reference, which the exact-sum kernels answer to
                    exp = iref.ssd_serial(left, right, rad, lo, hi) if flags & T.SERIAL else iref.ssd_cuda(left, right, rad, lo, hi, flags)
                    same(got, exp, what + " (integer reference)")
    finally:
        ctx.close()
