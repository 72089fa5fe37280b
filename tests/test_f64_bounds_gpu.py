"""The float kernels against the float64 references with error bounds (tests/_f64_ref.py), not against the oracle:
lk::calcOpticalFlow in every dispatch form, harris::getCornerResponse in both arithmetics and both kernels, and
disparityNCorr across its templated and generic radii, row blockings, chunk boundaries, 8-bit and scaled images.
A kernel output outside the bound is wrong whatever the C oracle computes (tests/test_f64_ref.py ties the oracle to
the same bounds on the CPU)."""
import numpy as np
import pytest

import _f64_ref as F
from test_f64_ref import check_lk, harris_outside, image, report

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def dev(a, pad=0):
    """Device copy of a 2-D array; pad > 0 gives it a row pitch of cols + pad elements."""
    a = np.ascontiguousarray(a)
    if pad == 0:
        return torch.from_numpy(a).cuda()
    wide = torch.full((a.shape[0], a.shape[1] + pad), 7, dtype=torch.from_numpy(a).dtype, device="cuda")
    wide[:, :a.shape[1]] = torch.from_numpy(a).cuda()
    return wide[:, :a.shape[1]]


def host(t):
    return t.cpu().numpy()


def ctx_with(**opts):
    from introtocomputervision_amd import _capi
    c = _capi.Context(0)
    for k, v in opts.items():
        c.set_option(getattr(_capi, k), v)
    return c


_CTX = {}


def ctx_for(key):
    """One context per option set for the whole module (creating contexts per case is slow)."""
    if key not in _CTX:
        _CTX[key] = ctx_with(**dict(key))
    return _CTX[key]


def lk_pair(seed, rows, cols, kind="uniform"):
    prev = image(seed, rows, cols, kind)
    nxt = np.roll(prev, (1, -2), (0, 1))
    nxt[::3] = image(seed + 1, rows, cols, kind)[::3]
    return prev, nxt


def run_lk(prev, nxt, win, form, pad=0):
    from introtocomputervision_amd import lk
    key = (("OPT_LK_FORCE_GENERIC", form),) if form else ()
    u, v = lk.calcOpticalFlow(dev(prev, pad), dev(nxt, pad), winSize=win, ctx=ctx_for(key))
    return host(u), host(v)


# ------------------------------------------------------------------------------------------------------- LK ----

LK_WINS = [1, 3, 5, 7, 15, 21, 23, 43, 63]
SEAMS = [(31, 63), (32, 64), (33, 65), (63, 127), (64, 128), (65, 129), (127, 31), (128, 32), (129, 33), (1, 129), (97, 1)]


@pytest.mark.parametrize("form", [0, 1, 2, 3])
@pytest.mark.parametrize("win", LK_WINS)
def test_lk_forms_windows_seams(form, win):
    for i, (rows, cols) in enumerate(SEAMS):
        prev, nxt = lk_pair(rows * 131 + cols + win, rows, cols, ["uniform", "smooth", "normal", "flat"][i % 4])
        pad = [0, 1, 3, 64][i % 4]
        u, v = run_lk(prev, nxt, win, form, pad)
        check_lk(u, v, F.lk_flow(prev, nxt, win), f"lk form {form} win {win} {rows}x{cols} pad {pad}")


@pytest.mark.parametrize("win", [15, 43])
def test_lk_1080p(win):
    rows, cols = 1080, 1920
    prev = image(0xC0FFEE, rows, cols, "u8")
    nxt = np.roll(prev, (1, -2), (0, 1))
    ref = F.lk_flow(prev, nxt, win)
    u, v = run_lk(prev, nxt, win, 0)
    check_lk(u, v, ref, f"lk 1080p win {win}")
    print(f"lk 1080p win {win}: illcond {ref[3].mean():.2e} straddle {ref[2].mean():.2e} "
          f"median bound {np.median(np.maximum(*ref[1])[ref[1][0] > 0]):.2e}")


# --------------------------------------------------------------------------------------------------- Harris ----

def run_harris(gx, gy, win, sigma, form, xoff=0, cols=None, pad=0):
    from introtocomputervision_amd import harris
    key = (("OPT_HARRIS_GENERIC", 1),) if form == "generic" else ()
    cols = cols or gx.shape[1]
    dx, dy = dev(gx, pad), dev(gy, pad)
    R = harris.getCornerResponse(dx[:, xoff:xoff + cols], dy[:, xoff:xoff + cols], win, sigma, 0.04, ctx=ctx_for(key),
                                 cpu_arithmetic=form == "cpu")
    return host(R)


@pytest.mark.parametrize("form", ["default", "generic", "cpu"])
@pytest.mark.parametrize("win,sigma", [(3, 0.8), (5, 1.5), (7, 2.0), (9, 2.0), (11, 3.0), (63, 10.0)])
def test_harris_forms_and_tiles(form, win, sigma):
    rng = np.random.default_rng(win)
    bx = (rng.standard_normal((75, 456)) * 300).astype(np.float32)
    by = (rng.standard_normal((75, 456)) * 300).astype(np.float32)
    for xoff, cols in [(0, 448), (0, 331), (1, 330), (4, 330), (0, 1), (3, 64)]:
        gx, gy = bx[:, xoff:xoff + cols], by[:, xoff:xoff + cols]
        R = run_harris(bx, by, win, sigma, form, xoff, cols)
        ref = F.harris_response(gx, gy, win, sigma, 0.04)
        report(harris_outside(R, ref), R, ref[0], ref[1], f"harris {form} win {win} x {xoff}+{cols}")


def test_harris_4k_frame():
    """The C5 frame (3840 x 2160, test_ps124_gpu.test_c5_4k_harris_keypoints_lk) at the configured window."""
    from introtocomputervision_amd import harris, synth
    rows, cols = 2160, 3840
    tex = synth.smooth_noise(0x5EED0004, rows, cols)
    prev = np.round(tex * (synth.checkerboard(rows, cols, square=40) / 192.0)).astype(np.float32)
    gx, gy = harris.getGradients(dev(prev), 3)
    R = host(harris.getCornerResponse(gx, gy, 5, 1.5, 0.04))
    ref = F.harris_response(host(gx), host(gy), 5, 1.5, 0.04)
    report(harris_outside(R, ref), R, ref[0], ref[1], "harris 4k")


# ------------------------------------------------------------------------------------------------------ NCC ----

def run_ncc(left, right, rad, dmin, dmax, flags, rows_opt=None, pad=0):
    from introtocomputervision_amd import stereo
    key = (("OPT_STEREO_ROWS", rows_opt),) if rows_opt else ()
    return host(stereo.disparityNCorr(dev(left, pad), dev(right, pad), rad, dmin, dmax, flags, ctx=ctx_for(key)))


def check_ncc(left, right, rad, dmin, dmax, flags, got, what):
    vol = F.ncc_admissible(left, right, rad, dmin, dmax, flags)
    ok = F.ncc_admits(vol, got, dmin)
    if not ok.all():
        idx = np.argwhere(~ok)[:5]
        cells = [(tuple(i.tolist()), int(got[tuple(i)]),
                  (np.nonzero(vol[:, i[0], i[1]])[0] + dmin - 1).tolist()) for i in idx]
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.size} not admissible, first (pixel, got, admissible; "
                             f"{dmin - 1} = -1 output): {cells}")
    return vol


def ncc_pair(seed, rows, cols, kind, shift=-5):
    left = image(seed, rows, cols, kind)
    right = np.ascontiguousarray(np.roll(left, shift, 1))
    right[::3] = image(seed + 1, rows, cols, kind)[::3]
    return left, right


@pytest.mark.parametrize("rad", list(range(0, 12)) + [15])
@pytest.mark.parametrize("rows_opt", [8, 10])
def test_ncc_radii_rows_cols2r(rad, rows_opt):
    for flags in (0, F.COLS_2R) if rad else (0,):  # COLS_2R at radius 0 is refused (an empty window)
        for kind, (dmin, dmax) in (("uniform", (-12, 9)), ("u8", (-70, 3))):  # the second crosses a 64-wide chunk
            left, right = ncc_pair(rad * 7 + rows_opt, 37, 150, kind)
            got = run_ncc(left, right, rad, dmin, dmax, flags, rows_opt, pad=3 if flags else 0)
            check_ncc(left, right, rad, dmin, dmax, flags, got, f"ncc r {rad} rows {rows_opt} flags {flags} {kind}")


@pytest.mark.parametrize("rad", [0, 2, 7, 10, 11, 15])
def test_ncc_rolling(rad):
    """ROLLING: the strip-serial kernel (40-row strips, subtract-and-add column sums) on float images, where its
    rounding differs from fresh sums; 131 rows cross three strip seams."""
    for kind in ("uniform", "normal"):
        left, right = ncc_pair(rad * 3 + 1, 131, 150, kind, shift=-4)
        for flags in (F.ROLLING, F.ROLLING | F.COLS_2R) if rad else (F.ROLLING,):
            got = run_ncc(left, right, rad, -12, 9, flags, pad=3 if flags & F.COLS_2R else 0)
            check_ncc(left, right, rad, -12, 9, flags, got, f"ncc rolling r {rad} flags {flags} {kind}")


@pytest.mark.parametrize("scale", [2.0 ** -12, 2.0 ** 9, 2.0 ** 12])
def test_ncc_scaled_images_take_the_sqrtf_fallback(scale):
    """Pixels or window energies outside ncc_arith.hpp's checked range: the compiler's sqrtf / division."""
    for rad in (2, 7, 11):
        left, right = ncc_pair(rad, 45, 140, "uniform")
        left, right = left * np.float32(scale), right * np.float32(scale)
        got = run_ncc(left, right, rad, -20, 20, 0)
        check_ncc(left, right, rad, -20, 20, 0, got, f"ncc scaled {scale} r {rad}")


def test_ncc_reference_geometry():
    """The reference's pair geometry: 640 x 511, radius 7, disparities -96..0 (ps2 main.cpp)."""
    left, right = ncc_pair(7, 511, 640, "u8", shift=-30)
    for flags in (0, F.COLS_2R):
        check_ncc(left, right, 7, -96, 0, flags, run_ncc(left, right, 7, -96, 0, flags), f"ncc 640x511 flags {flags}")


def test_ncc_1080p_128_disparities():
    left, right = ncc_pair(0x1080, 1080, 1920, "u8", shift=-40)
    got = run_ncc(left, right, 3, -100, 27, 0)
    vol = check_ncc(left, right, 3, -100, 27, 0, got, "ncc 1080p")
    print(f"ncc 1080p r 3 d -100..27: non-singleton sets {(vol.sum(0) != 1).mean():.2e}")
