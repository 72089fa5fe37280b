"""Layout containment of the display, ps0, warp, motion-history, overlay, panel and ps5 driver `_dev` entry points: the
second table beside tests/test_layout_containment_gpu.py, in the same format (tests/_layout_table.py).

One row function per entry point; a row yields cases; every case runs in layout A (packed) and B (embedded: one
element past a 256-byte boundary, odd row padding, batch images a non-16-byte gap apart).  The rows of csrc/display.hip,
csrc/warp.hip and csrc/mhi.hip keep an alignment flag per plane and pick a vector or a scalar path from it, so they
also run the mixed layouts C (inputs as in A, outputs as in B) and D (inputs as in B, outputs as in A).  After every
call _layout.check asserts that no byte outside the output views changed and that every output view holds `expected`
byte for byte.  A canvas or a history that the call reads and then overwrites is a plane with data that is also an
output.

`expected` comes from the numpy reference modules of this directory, all bit-exact, so call A must equal it too.  Two
rows take their expected bytes from call A alone: micv_disparity_ncorr_u8_dev and micv_disparity_ncorr_u8_batch_dev --
no reference module restates disparityNCorr (the core table's micv_disparity_ncorr_dev row has the same reason; the C
oracle holds these entries to it in tests/test_stereo_ncc_u8_gpu.py).  One more plane does, for the like reason:
the Harris response R inside `fields` of micv_ps4_harris_display_dev; the references continue from it (the core table's
micv_harris_corners_dev row does the same).  The keypoint angle of micv_sift_keypoints_dev is atan2f-based: call A is
held to the reference within the existing tolerance, the other layouts to A by bytes, as the core table's
micv_sift_angles_dev row does.

A layout departs from the default placement only where include/mi_cv.h states a requirement; the row quotes it.  Records
and lists that the header types as structs, doubles or 64-bit words (micv_ps0_stats, colours, counts, the generator
word) are planes of 8-byte elements: the harness offsets a plane by one ELEMENT, which keeps a C object aligned as its
type demands.

The end of the module accounts for every `_dev` name of _capi.SIGNATURES: a row in the core table, a row here, or an
entry of EXEMPT with one of the reasons listed there."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

import _display_ref as D
import _hough_ref as H
import _layout as Y
import _lk_chain_ref as L
import _mhi_color_ref as MC
import _mhi_ref as M
import _pf_ref as PF
import _ps0_ref as P0
import _ps1_driver_ref as P1
import _ps3_driver_ref as P3
import _ps3_ref as G3
import _ps4_driver_ref as P4
import _ps4_feat_ref as F4
import _ps5_driver_ref as P5
import _ps6_driver_ref as P6
import _ps7_ref as P7
import _stereo_ref as S8
import _warp_ref as W

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from introtocomputervision_amd import _capi  # noqa: E402
from _layout_table import (Case, run_case, rng_of, lk_frames, image_f32, image_u8, flow_field, edge_mask, gradients,  # noqa: E402
                           pointer_array, canvas, stereo_pair, f32, u8, i8, i32, i64, u32)
import test_layout_containment_gpu as core  # noqa: E402  (its TABLE, for the accounting)

lib = _capi.lib
f64, u64 = np.float64, np.uint64
Plane = Y.Plane

SHAPES = [(35, 69), (18, 60)]     # columns = 1 mod 4, just over one 64-column tile and 32 rows; a multiple of 4, under one tile
PYR_SHAPES = SHAPES + [(50, 76)]  # levels 50x76, 25x38, 13x19
AB, ABCD = "AB", "ABCD"


def out(name, rows, cols, dtype=u8, **kw):
    return Plane(name, shape=(rows, cols), dtype=dtype, **kw)


def doubles(name, values):
    """A colour, a mean / stddev pair, thresholds: doubles in device memory, no pitch in the header -> a dense list."""
    return Plane(name, np.asarray(values, f64).reshape(1, -1), dense=True)


# ------------------------------------------------------------------------------------------------ display --------

def display_sources(rows, cols):
    """(depth, image) per source depth of the header: 32F with a NaN (skipped by the range), 8U, 8S."""
    f = image_f32(rows, cols, 101).copy()
    f[rows // 2, cols // 3] = np.nan
    b = image_u8(rows, cols, 102)
    return ((_capi.DEPTH_32F, f), (_capi.DEPTH_8U, b), (_capi.DEPTH_8S, (b.astype(np.int16) - 128).astype(i8)))


SUBSETS = [s for s in ((k & 1, k & 2, k & 4) for k in range(1, 8))]  # every non-empty subset of (u8, inverted, jet)


def normalize_expected(imgs, want_u8, want_inv, want_jet, want_mm):
    """_display_ref.normalize / invert / jet / minmax per image, stacked."""
    n = [D.normalize(i) for i in imgs]
    e = {}
    if want_u8:
        e["u8"] = np.stack(n)
    if want_inv:
        e["inv"] = np.stack([D.invert(x) for x in n])
    if want_jet:
        e["jet"] = np.stack([D.jet(x).reshape(x.shape[0], -1) for x in n])
    if want_mm:
        e["mm"] = np.array([D.minmax(i) for i in imgs], f32)
    return e


def normalize_cases(rows, cols, batch):
    """Expected: _display_ref.normalize, invert, jet, minmax.  mi_cv.h: "minmax_out (optional, DEVICE, 2 floats per
    image)" has no pitch: a dense list.  Every depth, every subset of the three outputs, minmax_out with every other one."""
    for depth, img in display_sources(rows, cols):
        # the images of a batch differ in range: each is normalised by its own
        imgs = [img] + [np.roll(img, 5 * k, axis=1) * f32(k + 1) if img.dtype == f32 else np.roll(img, 5 * k, axis=1) // img.dtype.type(k + 1)
                        for k in range(1, batch)]
        for k, (w8, wi, wj) in enumerate(SUBSETS):
            wm = k % 2 == 0
            exp = normalize_expected(imgs, w8, wi, wj, wm)
            exp = exp if batch > 1 else {n: (v[0] if n != "mm" else v) for n, v in exp.items()}
            lead = (batch,) if batch > 1 else ()

            def planes(imgs=imgs, w8=w8, wi=wi, wj=wj, wm=wm, lead=lead):
                g = [Plane("src", np.stack(imgs) if batch > 1 else imgs[0])]
                g += [Plane("u8", shape=lead + (rows, cols), dtype=u8)] if w8 else []
                g += [Plane("inv", shape=lead + (rows, cols), dtype=u8)] if wi else []
                g += [Plane("jet", shape=lead + (rows, cols * 3), dtype=u8)] if wj else []
                g += [Plane("mm", shape=(batch, 2), dtype=f32, dense=True)] if wm else []
                return [g]

            def call(h, S, st, depth=depth, w8=w8, wi=wi, wj=wj, wm=wm):
                def o(name, want):
                    if batch > 1:
                        return (S.ptr(name), S.dist(name), S.pitch(name)) if want else (None, 0, 0)
                    return (S.ptr(name), S.pitch(name)) if want else (None, 0)
                mm = S.ptr("mm") if wm else None
                if batch > 1:
                    return lib.micv_normalize_minmax_batch_dev(h, S.ptr("src"), S.dist("src"), depth, batch, rows, cols, S.pitch("src"),
                                                               *o("u8", w8), *o("inv", wi), *o("jet", wj), mm, st)
                return lib.micv_normalize_minmax_dev(h, S.ptr("src"), depth, rows, cols, S.pitch("src"), *o("u8", w8), *o("inv", wi),
                                                     *o("jet", wj), mm, st)
            yield Case(f"depth {depth} u8 {w8} inv {wi} jet {wj} minmax {wm}", planes, list(exp), call, lambda A, exp=exp: exp)


def row_normalize_minmax(rows, cols):
    yield from normalize_cases(rows, cols, 1)


def row_normalize_minmax_batch(rows, cols):
    yield from normalize_cases(rows, cols, 3)


def row_apply_colormap_jet(rows, cols):
    """Expected: _display_ref.jet."""
    src = image_u8(rows, cols, 103)

    def call(h, S, st):
        return lib.micv_apply_colormap_jet_dev(h, S.ptr("src"), rows, cols, S.pitch("src"), S.ptr("jet"), S.pitch("jet"), st)
    yield Case("jet", lambda: [[Plane("src", src), out("jet", rows, cols * 3)]], ["jet"], call,
               lambda A: {"jet": D.jet(src).reshape(rows, cols * 3)})


def row_gain_noise(rows, cols):
    """Expected: _display_ref.gain_noise.  With noise (gain 1), without (gain 1.7), and in place: "dst may alias src"."""
    src = image_f32(rows, cols, 104)
    noise = (rng_of(rows, cols, 105).standard_normal((rows, cols)) * 7).astype(f32)
    for tag, gain, nz, inplace in (("noise", 1.0, noise, False), ("gain", 1.7, None, False), ("in place", 0.6, noise, True)):
        dst = "src" if inplace else "dst"

        def planes(nz=nz, inplace=inplace):
            return [[Plane("src", src)] + ([Plane("noise", nz)] if nz is not None else []) + ([] if inplace else [out("dst", rows, cols, f32)])]

        def call(h, S, st, gain=gain, nz=nz, dst=dst):
            n = (S.ptr("noise"), S.pitch("noise")) if nz is not None else (None, 0)
            return lib.micv_gain_noise_f32_dev(h, S.ptr("src"), S.pitch("src"), gain, *n, rows, cols, S.ptr(dst), S.pitch(dst), st)
        yield Case(tag, planes, [dst], call, lambda A, gain=gain, nz=nz, dst=dst: {dst: D.gain_noise(src, gain, nz)})


def pair_expected(left, right, rad, rng):
    return S8.ssd_cuda(left, right, rad, -rng, 0, 0), S8.ssd_cuda(right, left, rad, 0, rng, 0)


def row_disparity_pair(rows, cols):
    """Expected: _stereo_ref.ssd_cuda both ways (MICV_DISPARITY_SSD; the NCC metric has no reference module and its single
    entry is a row of the core table).  One dstride serves both maps."""
    left, right = stereo_pair(rows, cols, 106)
    dl, dr = pair_expected(left, right, 2, 5)

    def call(h, S, st):
        return lib.micv_disparity_pair_dev(h, S.ptr("left"), S.ptr("right"), rows, cols, S.pitch("left"), 2, 5, _capi.DISPARITY_SSD, 0,
                                           S.ptr("dl"), S.ptr("dr"), S.pitch("dl"), st)
    yield Case("ssd", lambda: [[Plane("left", left), Plane("right", right), out("dl", rows, cols, i8), out("dr", rows, cols, i8)]],
               ["dl", "dr"], call, lambda A: {"dl": dl, "dr": dr})


def row_disparity_pair_display(rows, cols):
    """Expected: _display_ref.gain_noise, then _stereo_ref.ssd_cuda both ways, then _display_ref.normalize / invert.  The
    noise is integer-valued and keeps the sums in 0..255, where the exact reference applies.  mi_cv.h: "`work` (device,
    2 * rows * cols floats) holds left' and right'": a dense list, asserted too.  Second case: gain 1, no noise, no
    inverted image, no work."""
    left, right = stereo_pair(rows, cols, 107)
    left, right = np.clip(left, 4, 250), np.clip(right, 4, 250)
    r = rng_of(rows, cols, 108)
    nl, nr = r.integers(-3, 4, (rows, cols)).astype(f32), r.integers(-3, 4, (rows, cols)).astype(f32)
    for noisy in (True, False):
        l2, r2 = (D.gain_noise(left, 1.0, nl), D.gain_noise(right, 1.0, nr)) if noisy else (left, right)
        dl, dr = pair_expected(l2, r2, 2, 5)
        exp = {"dl": dl, "dr": dr, "il": D.normalize(dl), "ir": D.normalize(dr)}
        if noisy:
            exp.update({"inv": D.invert(exp["il"]), "work": np.concatenate([l2, r2])})

        def planes(noisy=noisy):
            g = [Plane("left", left), Plane("right", right), out("dl", rows, cols, i8), out("dr", rows, cols, i8), out("il", rows, cols),
                 out("ir", rows, cols)]
            if noisy:
                g += [Plane("nl", nl), Plane("nr", nr), out("inv", rows, cols), out("work", 2 * rows, cols, f32, dense=True)]
            return [g]

        def call(h, S, st, noisy=noisy):
            nz = (S.ptr("nl"), S.ptr("nr"), S.pitch("nl")) if noisy else (None, None, 0)
            return lib.micv_disparity_pair_display_dev(h, S.ptr("left"), S.ptr("right"), rows, cols, S.pitch("left"), 1.0, *nz, 2, 5,
                                                       _capi.DISPARITY_SSD, 0, S.ptr("dl"), S.ptr("dr"), S.pitch("dl"), S.ptr("il"),
                                                       S.ptr("inv") if noisy else None, S.ptr("ir"), S.pitch("il"),
                                                       S.ptr("work") if noisy else None, st)
        yield Case(f"noise {noisy}", planes, list(exp), call, lambda A, exp=exp: exp)


# -------------------------------------------------------------------------------------------------- ps0 ----------

def bytes_image(rows, cols, ch, seed):
    return rng_of(rows, cols, ch, seed).integers(0, 256, (rows, cols, ch)).astype(u8)


def row_mix_channels(rows, cols):
    """Expected: _ps0_ref.mix_channels.  1 to 4 source and destination channels."""
    for scn in (1, 2, 3, 4):
        src = bytes_image(rows, cols, scn, 110)
        for dcn in (1, 2, 3, 4):
            m = [(3 * k + dcn) % scn for k in range(dcn)]
            exp = P0.mix_channels(src, m).reshape(rows, cols * dcn)

            def call(h, S, st, scn=scn, dcn=dcn, m=m):
                return lib.micv_mix_channels_u8_dev(h, S.ptr("src"), rows, cols, scn, S.pitch("src"), (C.c_int * dcn)(*m), S.ptr("dst"), dcn,
                                                    S.pitch("dst"), st)
            yield Case(f"{scn} -> {dcn} {m}", lambda src=src, scn=scn, dcn=dcn: [[Plane("src", src.reshape(rows, cols * scn)),
                                                                                 out("dst", rows, cols * dcn)]],
                       ["dst"], call, lambda A, exp=exp: {"dst": exp})


def row_pixel_replacement(rows, cols):
    """Expected: _ps0_ref.pixel_replacement.  Images of two sizes, 1 and 3 channels, an odd and an even square."""
    r1, c1 = rows - 3, cols + 2
    for ch in (1, 3):
        a, b = bytes_image(r1, c1, ch, 111), bytes_image(rows, cols, ch, 112)
        for size in (9, 12):
            exp = P0.pixel_replacement(a, b, size).reshape(rows, cols * ch)

            def call(h, S, st, ch=ch, size=size):
                return lib.micv_pixel_replacement_u8_dev(h, S.ptr("a"), r1, c1, S.pitch("a"), S.ptr("b"), rows, cols, S.pitch("b"), ch, size,
                                                         S.ptr("dst"), S.pitch("dst"), st)
            yield Case(f"{ch} channels size {size}", lambda a=a, b=b, ch=ch: [[Plane("a", a.reshape(r1, c1 * ch)), Plane("b", b.reshape(rows, cols * ch)),
                                                                                out("dst", rows, cols * ch)]],
                       ["dst"], call, lambda A, exp=exp: {"dst": exp})


def stats_record(st):
    """micv_ps0_stats as five 8-byte words: double mean, stddev; uint64 sum, sqsum; int32 min, max."""
    return np.frombuffer(struct.pack("<ddQQii", st["mean"], st["stddev"], st["sum"], st["sqsum"], st["min"], st["max"]), i64).reshape(1, 5)


def row_mean_stddev(rows, cols):
    """Expected: _ps0_ref.mean_stddev, the whole record byte for byte."""
    src = image_u8(rows, cols, 113)

    def call(h, S, st):
        return lib.micv_mean_stddev_u8_dev(h, S.ptr("src"), rows, cols, S.pitch("src"), S.ptr("stats"), st)
    yield Case("stats", lambda: [[Plane("src", src), out("stats", 1, 5, i64, dense=True)]], ["stats"], call,
               lambda A: {"stats": stats_record(P0.mean_stddev(src))})


def row_ps0_arithmetic(rows, cols):
    """Expected: _ps0_ref.arithmetic.  mi_cv.h: "mean_stddev points at {mean, stddev} on the device": two doubles, a dense
    list.  The image's own statistics, and a zero stddev."""
    src = image_u8(rows, cols, 114)
    st0 = P0.mean_stddev(src)
    for mean, sd in ((st0["mean"], st0["stddev"]), (100.25, 0.0)):
        def call(h, S, st, mean=mean, sd=sd):
            return lib.micv_ps0_arithmetic_u8_dev(h, S.ptr("src"), rows, cols, S.pitch("src"), S.ptr("ms"), S.ptr("dst"), S.pitch("dst"), st)
        yield Case(f"mean {mean} stddev {sd}", lambda mean=mean, sd=sd: [[Plane("src", src), doubles("ms", [mean, sd]), out("dst", rows, cols)]],
                   ["dst"], call, lambda A, mean=mean, sd=sd: {"dst": P0.arithmetic(src, mean, sd)})


def row_subtract_sat(rows, cols):
    """Expected: _ps0_ref.subtract."""
    a, b = image_u8(rows, cols, 115), image_u8(rows, cols, 116)

    def call(h, S, st):
        return lib.micv_subtract_sat_u8_dev(h, S.ptr("a"), S.pitch("a"), S.ptr("b"), S.pitch("b"), rows, cols, S.ptr("dst"), S.pitch("dst"), st)
    yield Case("a - b", lambda: [[Plane("a", a), Plane("b", b), out("dst", rows, cols)]], ["dst"], call, lambda A: {"dst": P0.subtract(a, b)})


def noise_plane(rows, cols, seed):
    """sigma 40 draws with the special values of _ps0_ref in the first row (NaN, +-inf, halves, beyond int)."""
    z = (rng_of(rows, cols, seed).standard_normal((rows, cols)) * 40).astype(f32)
    z[0, :len(P0.SPECIAL_NOISE)] = np.asarray(P0.SPECIAL_NOISE, f32)
    return z


def row_add_noise(rows, cols):
    """Expected: _ps0_ref.add_noise.  The noise plane is f32, so its pitch is a multiple of 4 as the general rule says."""
    src, z = image_u8(rows, cols, 117), noise_plane(rows, cols, 118)

    def call(h, S, st):
        return lib.micv_add_noise_s8_u8_dev(h, S.ptr("src"), S.pitch("src"), S.ptr("z"), S.pitch("z"), rows, cols, S.ptr("dst"), S.pitch("dst"), st)
    yield Case("noise", lambda: [[Plane("src", src), Plane("z", z), out("dst", rows, cols)]], ["dst"], call, lambda A: {"dst": P0.add_noise(src, z)})


def row_ps0_run(rows, cols):
    """Expected: _ps0_ref.run.  mi_cv.h: "planes: seven rows1 x cols1 planes plane_pitch bytes apart, pstride bytes per
    row": a batch of seven images, pitched and a gap apart."""
    r2, c2 = rows - 4, cols - 7
    i1, i2 = bytes_image(rows, cols, 3, 119), bytes_image(r2, c2, 3, 120)
    ng, nb = noise_plane(rows, cols, 121), noise_plane(rows, cols, 122)
    size = 10
    w = P0.run(i1, i2, ng, nb, size)
    exp = {"swapped": w["swapped"].reshape(rows, cols * 3), "replaced": w["replaced"], "stats": stats_record(w["stats"]),
           "planes": np.stack([w[k] for k in ("green", "red", "arithmetic", "translated", "difference", "noisyGreen", "noisyBlue")])}

    def call(h, S, st):
        return lib.micv_ps0_run_dev(h, S.ptr("i1"), rows, cols, S.pitch("i1"), S.ptr("i2"), r2, c2, S.pitch("i2"), size, S.ptr("ng"), S.ptr("nb"),
                                    S.pitch("ng"), S.ptr("swapped"), S.pitch("swapped"), S.ptr("planes"), S.pitch("planes"), S.dist("planes"),
                                    S.ptr("replaced"), S.pitch("replaced"), S.ptr("stats"), st)
    yield Case("run", lambda: [[Plane("i1", i1.reshape(rows, cols * 3)), Plane("i2", i2.reshape(r2, c2 * 3)), Plane("ng", ng), Plane("nb", nb),
                                out("swapped", rows, cols * 3), Plane("planes", shape=(7, rows, cols), dtype=u8), out("replaced", r2, c2),
                                out("stats", 1, 5, i64, dense=True)]],
               list(exp), call, lambda A: exp)


# ------------------------------------------------------------------------------------------------- warp ----------

WARP_M = np.array([[1.04, 0.09, -2.3], [-0.08, 0.97, 1.6]], f32)
WARP_FLAGS = (0, _capi.WARP_NEAREST, _capi.WARP_INVERSE_MAP, _capi.WARP_INVERSE_MAP | _capi.WARP_NEAREST)


def warp_sources(rows, cols, seed):
    return ((_capi.DEPTH_8U, image_u8(rows, cols, seed)), (_capi.DEPTH_32F, image_f32(rows, cols, seed + 1)))


def row_warp_affine(rows, cols):
    """Expected: _warp_ref.warp_affine.  8U and 32F; linear and nearest; M as src -> dst (inverted inside) and as the
    inverse map; a source of another size than the destination.  The transform is six floats in device memory."""
    sr, sc = rows - 3, cols + 2
    for depth, src in warp_sources(sr, sc, 130):
        for flags in WARP_FLAGS:
            exp = W.warp_affine(src, WARP_M, (cols, rows), flags)

            def call(h, S, st, depth=depth, flags=flags):
                return lib.micv_warp_affine_dev(h, S.ptr("src"), depth, sr, sc, S.pitch("src"), S.ptr("m"), flags, S.ptr("dst"), rows, cols,
                                                S.pitch("dst"), st)
            yield Case(f"depth {depth} flags {flags}", lambda src=src: [[Plane("src", src), Plane("m", WARP_M.reshape(1, 6), dense=True),
                                                                         out("dst", rows, cols, src.dtype)]],
                       ["dst"], call, lambda A, exp=exp: {"dst": exp})


def row_warp_affine_batch(rows, cols):
    """Expected: _warp_ref.warp_affine per image.  Three images by three transforms, and one shared source:
    "src_pitch_bytes == 0 warps one shared source by `count` transforms"."""
    sr, sc, n = rows - 3, cols + 2, 3
    ms = np.stack([WARP_M, WARP_M * f32(0.9), np.array([[1, 0, -2], [0, 1, 0]], f32)])
    for depth, src0 in warp_sources(sr, sc, 132):
        srcs = np.stack([np.roll(src0, 3 * k, axis=1) for k in range(n)])
        for shared in (False, True):
            for flags in WARP_FLAGS:
                exp = np.stack([W.warp_affine(srcs[0 if shared else k], ms[k], (cols, rows), flags) for k in range(n)])

                def call(h, S, st, depth=depth, flags=flags, shared=shared):
                    return lib.micv_warp_affine_batch_dev(h, S.ptr("src"), 0 if shared else S.dist("src"), depth, sr, sc, S.pitch("src"), S.ptr("m"), n,
                                                          flags, S.ptr("dst"), S.dist("dst"), rows, cols, S.pitch("dst"), st)
                yield Case(f"depth {depth} flags {flags} shared {shared}",
                           lambda srcs=srcs, shared=shared: [[Plane("src", srcs[0] if shared else srcs), Plane("m", ms.reshape(n, 6), dense=True),
                                                              Plane("dst", shape=(n, rows, cols), dtype=srcs.dtype)]],
                           ["dst"], call, lambda A, exp=exp: {"dst": exp})


def row_add_weighted(rows, cols):
    """Expected: _warp_ref.add_weighted.  The blend of the reference (0.5, 0.5), a saturating difference, a float case with
    gamma, and in place: "dst may alias a or b"."""
    a8, b8 = image_u8(rows, cols, 134), image_u8(rows, cols, 135)
    af, bf = image_f32(rows, cols, 136), image_f32(rows, cols, 137)
    for tag, a, b, depth, al, be, ga, dst in (("u8 blend", a8, b8, _capi.DEPTH_8U, 0.5, 0.5, 0.0, "dst"), ("u8 a - b", a8, b8, _capi.DEPTH_8U, 1.0, -1.0, 0.0, "dst"),
                                              ("f32", af, bf, _capi.DEPTH_32F, 0.7, 0.3, 1.5, "dst"), ("u8 into a", a8, b8, _capi.DEPTH_8U, 0.5, 0.5, 3.0, "a"),
                                              ("f32 into b", af, bf, _capi.DEPTH_32F, 0.25, 0.5, 0.0, "b")):
        exp = W.add_weighted(a, al, b, be, ga)

        def call(h, S, st, depth=depth, al=al, be=be, ga=ga, dst=dst):
            return lib.micv_add_weighted_dev(h, S.ptr("a"), S.pitch("a"), al, S.ptr("b"), S.pitch("b"), be, ga, depth, rows, cols, S.ptr(dst),
                                             S.pitch(dst), st)
        yield Case(tag, lambda a=a, b=b, dst=dst: [[Plane("a", a), Plane("b", b)] + ([out("dst", rows, cols, a.dtype)] if dst == "dst" else [])],
                   [dst], call, lambda A, exp=exp, dst=dst: {dst: exp})


def row_register_blend(rows, cols):
    """Expected: _warp_ref.register_blend.  With and without `warped`, both depths."""
    for depth, b in warp_sources(rows, cols, 138):
        a = np.roll(b, 2, axis=1)
        ew, eb = W.register_blend(a, b, WARP_M)
        for want in (True, False):
            def call(h, S, st, depth=depth, want=want):
                w = (S.ptr("warped"), S.pitch("warped")) if want else (None, 0)
                return lib.micv_register_blend_dev(h, S.ptr("a"), S.pitch("a"), S.ptr("b"), S.pitch("b"), depth, rows, cols, S.ptr("m"), *w,
                                                   S.ptr("blended"), S.pitch("blended"), st)
            yield Case(f"depth {depth} warped {want}",
                       lambda a=a, b=b, want=want: [[Plane("a", a), Plane("b", b), Plane("m", WARP_M.reshape(1, 6), dense=True), out("blended", rows, cols, a.dtype)]
                                                    + ([out("warped", rows, cols, a.dtype)] if want else [])],
                       ["blended"] + (["warped"] if want else []), call,
                       lambda A, ew=ew, eb=eb, want=want: {"blended": eb, **({"warped": ew} if want else {})})


def row_invert_affine(rows, cols):
    """Expected: _warp_ref.invert_affine.  No image: `rows` transforms of six floats, dense lists, one singular."""
    n = rows
    m = (rng_of(rows, cols, 139).standard_normal((n, 6)) * 2).astype(f32)
    m[1] = (1, 2, 3, 2, 4, 5)  # determinant 0
    exp = W.invert_affine(m.reshape(n, 2, 3)).reshape(n, 6)

    def call(h, S, st):
        return lib.micv_invert_affine_dev(h, S.ptr("m"), n, S.ptr("inv"), st)
    yield Case("invert", lambda: [[Plane("m", m, dense=True), out("inv", n, 6, f32, dense=True)]], ["inv"], call, lambda A: {"inv": exp})


# -------------------------------------------------------------------------------------------------- mhi ----------

BLUR = (5, 3, 1.2)  # blur_w, blur_h, sigma: a non-square kernel
THRESH = 12.0


def video(rows, cols, ch, nframes, seed):
    """[F, rows, cols * ch] u8: a textured frame that moves two columns and a row per frame, with a little noise."""
    base = np.stack([image_u8(rows, cols, seed + c) for c in range(ch)], 2)
    r = rng_of(rows, cols, ch, seed)
    fr = [np.clip(np.roll(base, (f, 2 * f), axis=(0, 1)).astype(np.int64) + r.integers(-2, 3, base.shape), 0, 255).astype(u8) for f in range(nframes)]
    return np.stack(fr).reshape(nframes, rows, cols * ch)


def shaped(v, rows, cols, ch):
    return v.reshape(v.shape[0], rows, cols, ch) if ch > 1 else v


def row_mhi_frame_difference(rows, cols):
    """Expected: _mhi_ref.frame_difference."""
    v = video(rows, cols, 1, 2, 140)
    exp = M.frame_difference(v[0], v[1], THRESH, BLUR[:2], BLUR[2])
    assert exp.any()

    def call(h, S, st):
        return lib.micv_mhi_frame_difference_dev(h, S.ptr("f1"), S.ptr("f2"), rows, cols, S.pitch("f1"), THRESH, *BLUR, S.ptr("diff"), S.pitch("diff"), st)
    yield Case("difference", lambda: [[Plane("f1", v[0]), Plane("f2", v[1]), out("diff", rows, cols)]], ["diff"], call, lambda A: {"diff": exp})


def row_mhi_frame_difference_c(rows, cols):
    """Expected: _mhi_color_ref.frame_difference.  3 and 4 channels."""
    for ch in (3, 4):
        v = video(rows, cols, ch, 2, 141)
        f = shaped(v, rows, cols, ch)
        exp = MC.frame_difference(f[0], f[1], THRESH, BLUR[:2], BLUR[2])
        assert exp.any()

        def call(h, S, st, ch=ch):
            return lib.micv_mhi_frame_difference_c_dev(h, S.ptr("f1"), S.ptr("f2"), rows, cols, ch, S.pitch("f1"), THRESH, *BLUR, S.ptr("diff"),
                                                       S.pitch("diff"), st)
        yield Case(f"{ch} channels", lambda v=v: [[Plane("f1", v[0]), Plane("f2", v[1]), out("diff", rows, cols)]], ["diff"], call,
                   lambda A, exp=exp: {"diff": exp})


def row_mhi_threshold(rows, cols):
    """Expected: _mhi_ref.threshold.  A whole and a fractional threshold."""
    src = image_u8(rows, cols, 142)
    for t in (100.0, 17.5):
        def call(h, S, st, t=t):
            return lib.micv_mhi_threshold_dev(h, S.ptr("src"), rows, cols, S.pitch("src"), t, S.ptr("dst"), S.pitch("dst"), st)
        yield Case(f"thresh {t}", lambda: [[Plane("src", src), out("dst", rows, cols)]], ["dst"], call, lambda A, t=t: {"dst": M.threshold(src, t)})


def row_mhi_update(rows, cols):
    """Expected: _mhi_ref.update.  In place: the history is input and output.  A first update (history of zeros) and a
    later one (a history of every age, zeros included), tau 30 and 255."""
    r = rng_of(rows, cols, 143)
    mask = (r.random((rows, cols)) < 0.3).astype(u8)
    mask[0, :5] = 2  # not 1: decays
    for tag, hist, tau in (("first", np.zeros((rows, cols), u8), 30), ("later", r.integers(0, 40, (rows, cols)).astype(u8), 255)):
        exp = M.update(hist, mask, tau)

        def call(h, S, st, tau=tau):
            return lib.micv_mhi_update_dev(h, S.ptr("hist"), S.pitch("hist"), S.ptr("mask"), S.pitch("mask"), rows, cols, tau, st)
        yield Case(tag, lambda hist=hist: [[Plane("hist", hist), Plane("mask", mask)]], ["hist"], call, lambda A, exp=exp: {"hist": exp})


def row_mhi_energy(rows, cols):
    """Expected: _mhi_ref.energy."""
    src = np.where(rng_of(rows, cols, 144).random((rows, cols)) < 0.5, 0, image_u8(rows, cols, 144)).astype(u8)

    def call(h, S, st):
        return lib.micv_mhi_energy_dev(h, S.ptr("src"), rows, cols, S.pitch("src"), S.ptr("dst"), S.pitch("dst"), st)
    yield Case("energy", lambda: [[Plane("src", src), out("dst", rows, cols)]], ["dst"], call, lambda A: {"dst": M.energy(src)})


NFRAMES, TAU = 5, 3
SAVE = (1, 4, 2)


def row_mhi_history_seq(rows, cols):
    """Expected: _mhi_ref.history_seq.  Five frames a gap apart, saves out of order (1, 4, 2) into a batch of three outputs;
    tau 3 lets a pixel decay to zero inside the sequence."""
    v = video(rows, cols, 1, NFRAMES, 145)
    exp = M.history_seq(v, THRESH, BLUR[:2], BLUR[2], TAU, list(SAVE))
    assert exp.any()

    def call(h, S, st):
        return lib.micv_mhi_history_seq_dev(h, S.ptr("frames"), NFRAMES, S.dist("frames"), S.pitch("frames"), rows, cols, THRESH, *BLUR, TAU,
                                            (C.c_int * 3)(*SAVE), 3, S.ptr("out"), S.dist("out"), S.pitch("out"), st)
    yield Case("seq", lambda: [[Plane("frames", v), Plane("out", shape=(3, rows, cols), dtype=u8)]], ["out"], call, lambda A: {"out": exp})


def row_mhi_history_seq_c(rows, cols):
    """Expected: _mhi_color_ref.history_seq.  1, 3 and 4 channels; both lists, the history list alone and the difference
    list alone ("Either list may be empty (count 0, pointers NULL) but not both")."""
    for ch in (1, 3, 4):
        v = video(rows, cols, ch, NFRAMES, 146)
        for save, sd in ((SAVE, (3, 1)), (SAVE, ()), ((), (2, 4))):
            eh, ed = MC.history_seq(shaped(v, rows, cols, ch), THRESH, BLUR[:2], BLUR[2], TAU, save, sd)
            exp = {**({"out": eh} if save else {}), **({"diff": ed} if sd else {})}

            def call(h, S, st, ch=ch, save=save, sd=sd):
                o = ((C.c_int * len(save))(*save), len(save), S.ptr("out"), S.dist("out"), S.pitch("out")) if save else (None, 0, None, 0, 0)
                d = ((C.c_int * len(sd))(*sd), len(sd), S.ptr("diff"), S.dist("diff"), S.pitch("diff")) if sd else (None, 0, None, 0, 0)
                return lib.micv_mhi_history_seq_c_dev(h, S.ptr("frames"), NFRAMES, S.dist("frames"), S.pitch("frames"), rows, cols, ch, THRESH, *BLUR,
                                                      TAU, *o, *d, st)
            yield Case(f"{ch} channels save {save} diff {sd}",
                       lambda v=v, save=save, sd=sd: [[Plane("frames", v)] + ([Plane("out", shape=(len(save), rows, cols), dtype=u8)] if save else [])
                                                      + ([Plane("diff", shape=(len(sd), rows, cols), dtype=u8)] if sd else [])],
                       list(exp), call, lambda A, exp=exp: exp)


def row_mhi_history_batch(rows, cols):
    """Expected: _mhi_color_ref.history_seq per video with its one save number.  Three videos of different lengths,
    thresholds and tau; save numbers 1 (the step that does not read the history) and above 1 (the dword
    read-modify-write); 1 and 3 channels.  The videos share frame_pitch and stride: planes of one shape."""
    nf, th, tau, save = (5, 3, 4), (THRESH, 9.0, 20.0), (3, 200, 2), (4, 1, 3)
    for ch in (1, 3):
        vids = [video(rows, cols, ch, NFRAMES, 147 + 10 * k) for k in range(3)]
        exp = np.stack([MC.history_seq(shaped(vids[k], rows, cols, ch)[:nf[k]], th[k], BLUR[:2], BLUR[2], tau[k], (save[k],))[0][0] for k in range(3)])

        def call(h, S, st, ch=ch):
            return lib.micv_mhi_history_batch_dev(h, pointer_array([S.ptr(f"vid{k}") for k in range(3)]), (C.c_int * 3)(*nf), S.dist("vid0"), S.pitch("vid0"),
                                                  3, rows, cols, ch, (C.c_double * 3)(*th), (C.c_int * 3)(*tau), (C.c_int * 3)(*save), *BLUR, S.ptr("out"),
                                                  S.dist("out"), S.pitch("out"), st)
        yield Case(f"{ch} channels", lambda vids=vids: [[Plane(f"vid{k}", vids[k]) for k in range(3)] + [Plane("out", shape=(3, rows, cols), dtype=u8)]],
                   ["out"], call, lambda A, exp=exp: {"out": exp})


# ------------------------------------------------------------------------------------- overlays and panels -------
# A canvas the call reads and then overwrites is a plane with data that is also an output.  Strokes cross the image
# border and land on row 0, the last row, column 0 and the last column: one pixel too far is a changed padding byte.

DOT, BOX = (10.4, 300.0, -5.0, 77.0), (255.0, 0.0, 255.0, 9.0)


def colour(c):
    return (C.c_double * 4)(*c)


def picture(rows, cols, ch, seed):
    return rng_of(rows, cols, ch, seed).integers(0, 256, (rows, cols * ch)).astype(u8)


def border_points(rows, cols):
    """(x, y) on the four corners, the four edges, one pixel outside each, and a few inside."""
    r, c = rows - 1, cols - 1
    return [(0, 0), (c, 0), (0, r), (c, r), (c // 2, 0), (c // 2, r), (0, r // 2), (c, r // 2), (-1, 3), (c + 1, r - 3), (5, -1), (c - 5, r + 1),
            (c // 3, r // 3), (c - 0.5, r - 0.5), (0.5, 0.5), (-1.5, -1.5), (c + 1.5, r + 1.5)]


def row_draw_dots(rows, cols):
    """Expected: _ps4_driver_ref.draw_dots.  Both grey depths; corners on the four corners of the map."""
    g8 = image_u8(rows, cols, 150)
    gf = (g8.astype(f32) * f32(1.2) - f32(20.5)).astype(f32)
    corners = np.zeros((rows, cols), f32)
    for (y, x), v in zip(((0, 0), (0, cols - 1), (rows - 1, 0), (rows - 1, cols - 1), (rows // 2, cols // 2), (3, 5)), (900.0, 50.0, 7.0, 300.0, 1.0, 2.5)):
        corners[y, x] = v
    for gray, depth in ((g8, _capi.DEPTH_8U), (gf, _capi.DEPTH_32F)):
        exp = P4.draw_dots(gray, corners).reshape(rows, cols * 3)

        def call(h, S, st, depth=depth):
            return lib.micv_draw_dots_dev(h, S.ptr("gray"), depth, rows, cols, S.pitch("gray"), S.ptr("corners"), S.pitch("corners"), S.ptr("dst"),
                                          S.pitch("dst"), st)
        yield Case(f"depth {depth}", lambda gray=gray: [[Plane("gray", gray), Plane("corners", corners), out("dst", rows, cols * 3)]], ["dst"], call,
                   lambda A, exp=exp: {"dst": exp})


def keypoints(rows, cols, seed):
    """[n, 4] x, y, size, angle: glyphs on every border of a rows x cols window, inside, and outside."""
    kp = [[x, y, 10 + (k % 3) * 4, (k * 47) % 360 if k % 4 else -1] for k, (x, y) in enumerate(border_points(rows, cols))]
    r = rng_of(rows, cols, seed)
    more = np.c_[r.uniform(-3, cols + 3, 12), r.uniform(-3, rows + 3, 12), r.choice([0, 5, 10, 17], 12), r.uniform(0, 360, 12)]
    return np.concatenate([np.asarray(kp, f32), more.astype(f32)])


def row_draw_keypoints(rows, cols):
    """Expected: _ps4_driver_ref.draw_keypoints (canvas and generator word).  The canvas and *rng_state are read and
    written; count and kp_xysa are lists without a pitch.  A window inside the canvas ([3, cols - 4)), from a grey and a
    BGR source and without a source; a capacity below the count."""
    x0, wc = 3, cols - 7
    cv = canvas(rows, cols, 151)
    kp = keypoints(rows, wc, 152)
    state = 0x1234ABCD5
    for cn, cap in ((1, len(kp)), (3, len(kp)), (0, len(kp)), (3, 5)):
        src = None if cn == 0 else picture(rows, wc, cn, 153)
        ec, es = P4.draw_keypoints(cv.reshape(rows, cols, 3), x0, wc, None if src is None else (src if cn == 1 else src.reshape(rows, wc, 3)), kp,
                                   len(kp), state, cap)
        exp = {"canvas": ec.reshape(rows, cols * 3), "state": np.array([[es]], u64)}

        def call(h, S, st, cn=cn, cap=cap, src=src):
            s = (S.ptr("src"), cn, rows, wc, S.pitch("src")) if src is not None else (None, 3, rows, wc, 0)
            return lib.micv_draw_keypoints_dev(h, *s, S.ptr("canvas"), cols, S.pitch("canvas"), x0, S.ptr("kp"), S.ptr("count"), cap, S.ptr("state"), st)
        yield Case(f"source channels {cn} cap {cap}",
                   lambda src=src: [([Plane("src", src)] if src is not None else []) + [Plane("canvas", cv), Plane("kp", kp, dense=True),
                                                                                         Plane("count", np.array([[len(kp)]], i64), dense=True),
                                                                                         Plane("state", np.array([[state]], u64), dense=True)]],
                   ["canvas", "state"], call, lambda A, exp=exp: exp)


def row_draw_match_lines(rows, cols):
    """Expected: _ps4_driver_ref.draw_match_lines.  Lines between the border points of the two halves, some matches out of
    range, with and without a mask, a count below the capacity."""
    half = cols // 2
    ka = np.asarray([[x, y, 10, 0] for x, y in border_points(rows, half)], f32)
    kb = ka[::-1].copy()
    n = len(ka)
    matches = np.asarray([[i, (i * 5) % n] for i in range(n)] + [[n, 0], [0, -1]], i32)
    mask = (np.arange(len(matches)) % 3 != 1).astype(u8)
    cv = canvas(rows, cols, 154)
    for tag, mk, count in (("all", None, len(matches)), ("masked", mask, len(matches) - 3)):
        exp = P4.draw_match_lines(cv.reshape(rows, cols, 3), ka, kb, matches, count, mk, half, P4.SEED, len(matches)).reshape(rows, cols * 3)
        assert (exp != cv).any()

        def call(h, S, st, mk=mk):
            return lib.micv_draw_match_lines_dev(h, S.ptr("canvas"), rows, cols, S.pitch("canvas"), S.ptr("ka"), len(ka), S.ptr("kb"), len(kb), S.ptr("m"),
                                                 S.ptr("count"), len(matches), S.ptr("mask") if mk is not None else None, half, P4.SEED, st)
        yield Case(tag, lambda mk=mk, count=count: [[Plane("canvas", cv), Plane("ka", ka, dense=True), Plane("kb", kb, dense=True),
                                                     Plane("m", matches, dense=True), Plane("count", np.array([[count]], i64), dense=True)]
                                                    + ([Plane("mask", mk.reshape(-1, 1), dense=True)] if mk is not None else [])],
                   ["canvas"], call, lambda A, exp=exp: {"canvas": exp})


def segments(rows, cols):
    """[n, 4] x1, y1, x2, y2: the frame of the image, its diagonals, strokes that enter and leave, one far outside."""
    r, c = rows - 1, cols - 1
    s = [(0, 0, c, 0), (c, 0, c, r), (c, r, 0, r), (0, r, 0, 0), (0, 0, c, r), (0, r, c, 0), (-7, r // 2, c + 9, r // 3), (c // 2, -5, c // 3, r + 8),
         (-3, -2, 4, 6), (c + 3, r + 2, c - 4, r - 6), (c + 1, 0, c + 1, r), (0, r + 1, c, r + 1), (-1, 0, -1, r), (0, -1, c, -1),
         (-2.0e9, 5, 2.0e9, 9), (np.nan, 3, 5, 5), (c - 0.5, 0.5, 0.5, r - 0.5)]
    return np.asarray(s, f32)


def stroke_cases(fn, lists, reference, rows, cols, seed):
    """micv_draw_segments_dev / micv_draw_epipolar_lines_dev on 1, 3 and 4 channels."""
    for ch in (1, 3, 4):
        img = picture(rows, cols, ch, seed)
        exp = reference(img.reshape(rows, cols, ch).copy(), lists, DOT).reshape(rows, cols * ch)
        assert (exp != img).any()

        def call(h, S, st, ch=ch):
            return fn(h, S.ptr("img"), rows, cols, ch, S.pitch("img"), S.ptr("list"), len(lists), colour(DOT), st)
        yield Case(f"{ch} channels", lambda img=img: [[Plane("img", img), Plane("list", lists, dense=True)]], ["img"], call,
                   lambda A, exp=exp: {"img": exp})


def row_draw_segments(rows, cols):
    """Expected: _ps3_driver_ref.draw_segments."""
    yield from stroke_cases(lib.micv_draw_segments_dev, segments(rows, cols), P3.draw_segments, rows, cols, 155)


def row_draw_epipolar_lines(rows, cols):
    """Expected: _ps3_driver_ref.draw_epipolar_lines.  The [n][6] block: e[2] and e[5] are not read (NaN here)."""
    s = segments(rows, cols)
    e = np.full((len(s), 6), np.nan, f32)
    e[:, [0, 1, 3, 4]] = s
    yield from stroke_cases(lib.micv_draw_epipolar_lines_dev, e, P3.draw_epipolar_lines, rows, cols, 156)


def arrow_fields(rows, cols, seed):
    """(u, v): NaN (no arrow) but for some 60 lattice points, the border points among them, whose arrows point up to
    9 pixels away and so leave the image on every side."""
    r = rng_of(rows, cols, seed)
    u, v = np.full((rows, cols), np.nan, f32), np.full((rows, cols), np.nan, f32)
    ys, xs = P5.lattice(rows, cols)
    pts = [(int(x), int(y)) for x, y in border_points(rows, cols) if float(x).is_integer() and 0 <= x < cols and 0 <= y < rows]
    pts += [(int(r.integers(0, cols)), int(r.integers(0, rows))) for _ in range(50)]
    for x, y in pts:
        x, y = x - x % xs.step, y - y % ys.step
        u[y, x], v[y, x] = f32(r.uniform(-9, 9)), f32(r.uniform(-9, 9))
    return u, v


def velocity_cases(rows, cols, batch):
    green = (0, 255, 0)
    imgs = np.stack([canvas(rows, cols, 157 + k) for k in range(batch)])
    uv = [arrow_fields(rows, cols, 160 + k) for k in range(batch)]
    us, vs = np.stack([a[0] for a in uv]), np.stack([a[1] for a in uv])
    exp = np.stack([P5.draw_velocity_vectors(imgs[k].reshape(rows, cols, 3), us[k], vs[k], green)[0].reshape(rows, cols * 3) for k in range(batch)])
    assert (exp != imgs).any()
    one = (lambda a: a[0]) if batch == 1 else (lambda a: a)

    def call(h, S, st):
        return lib.micv_draw_velocity_vectors_dev(h, S.ptr("img"), S.dist("img"), S.pitch("img"), S.ptr("u"), S.ptr("v"), S.dist("u"), S.pitch("u"), batch,
                                                  rows, cols, (C.c_uint8 * 3)(*green), st)
    yield Case(f"batch {batch}", lambda: [[Plane("img", one(imgs)), Plane("u", one(us)), Plane("v", one(vs))]], ["img"], call, lambda A: {"img": one(exp)})


def row_draw_velocity_vectors(rows, cols):
    """Expected: _ps5_driver_ref.draw_velocity_vectors.  One image, and a batch of three: "image i at img + i*img_pitch",
    "field i (u + i*field_pitch bytes": images and fields a gap apart (the fields are f32, so field_pitch is a multiple of
    4 as the general rule gives it)."""
    yield from velocity_cases(rows, cols, 1)
    yield from velocity_cases(rows, cols, 3)


def particles(rows, cols, seed):
    r = rng_of(rows, cols, seed)
    more = np.c_[r.uniform(-4, cols + 4, 80), r.uniform(-4, rows + 4, 80)]
    return np.concatenate([np.asarray(border_points(rows, cols), f32), more.astype(f32), np.asarray([[np.nan, 4], [np.inf, 2]], f32)])


def row_draw_particles(rows, cols):
    """Expected: _ps6_driver_ref.paint_loop (dots only).  1, 3 and 4 channels."""
    p = particles(rows, cols, 165)
    for ch in (1, 3, 4):
        img = picture(rows, cols, ch, 166)
        exp = P6.paint_loop(img.reshape(rows, cols, ch), p, DOT, None, BOX).reshape(rows, cols * ch)

        def call(h, S, st, ch=ch):
            return lib.micv_draw_particles_dev(h, S.ptr("img"), rows, cols, ch, S.pitch("img"), S.ptr("xy"), len(p), colour(DOT), st)
        yield Case(f"{ch} channels", lambda img=img: [[Plane("img", img), Plane("xy", p, dense=True)]], ["img"], call, lambda A, exp=exp: {"img": exp})


def row_draw_rectangle(rows, cols):
    """Expected: _ps6_driver_ref.paint_loop (ring only).  The frame of the image itself, a ring that leaves through a
    corner, one around the image (nothing painted), one row high."""
    for ch in (1, 3, 4):
        img = picture(rows, cols, ch, 167)
        for rect in ((0, 0, cols, rows), (cols - 6, rows - 4, 20, 20), (-1, -1, cols + 2, rows + 2), (-3, rows - 1, 12, 1), (4, 3, 9, 7)):
            exp = P6.paint_loop(img.reshape(rows, cols, ch), None, DOT, rect, BOX).reshape(rows, cols * ch)

            def call(h, S, st, ch=ch, rect=rect):
                return lib.micv_draw_rectangle_dev(h, S.ptr("img"), rows, cols, ch, S.pitch("img"), *rect, colour(BOX), st)
            yield Case(f"{ch} channels rect {rect}", lambda img=img: [[Plane("img", img)]], ["img"], call, lambda A, exp=exp: {"img": exp})


def row_ps6_overlay_list(rows, cols):
    """Expected: _ps6_driver_ref.overlay.  The centre is two floats in device memory; a box through the last row and
    column, and one inside."""
    p = particles(rows, cols, 168)
    for ch in (1, 3, 4):
        img = picture(rows, cols, ch, 169)
        for centre, size in (((cols - 4.0, rows - 3.0), (9.0, 7.0)), ((cols / 2, rows / 2), (11.0, 9.0))):
            exp = P6.overlay(img.reshape(rows, cols, ch), p, DOT, centre, size, BOX).reshape(rows, cols * ch)

            def call(h, S, st, ch=ch, size=size):
                return lib.micv_ps6_overlay_list_dev(h, S.ptr("img"), rows, cols, ch, S.pitch("img"), S.ptr("xy"), len(p), colour(DOT), S.ptr("centre"),
                                                     size[0], size[1], colour(BOX), st)
            yield Case(f"{ch} channels centre {centre}",
                       lambda img=img, centre=centre: [[Plane("img", img), Plane("xy", p, dense=True), Plane("centre", np.asarray([centre], f32), dense=True)]],
                       ["img"], call, lambda A, exp=exp: {"img": exp})


def filter_scene(rows, cols, ch, seed):
    frames, pos, tex = P6.scene(seed, rows, cols, ch, 1)
    return frames[0], pos[0], (tex if ch == 3 else tex[:, :, 0])


def row_hconcat(rows, cols):
    """Expected: _ps4_driver_ref.hconcat.  1 and 3 bytes per pixel; two widths."""
    ca, cb = cols, cols // 2 + 1
    for bpp in (1, 3):
        a, b = picture(rows, ca, bpp, 171), picture(rows, cb, bpp, 172)

        def call(h, S, st, bpp=bpp):
            return lib.micv_hconcat_dev(h, S.ptr("a"), S.pitch("a"), ca, S.ptr("b"), S.pitch("b"), cb, rows, bpp, S.ptr("dst"), S.pitch("dst"), st)
        yield Case(f"bpp {bpp}", lambda a=a, b=b, bpp=bpp: [[Plane("a", a), Plane("b", b), out("dst", rows, (ca + cb) * bpp)]], ["dst"], call,
                   lambda A, a=a, b=b: {"dst": P4.hconcat(a, b)})


def row_gray_or_bgr_to_bgr8(rows, cols):
    """Expected: _ps4_driver_ref.to_bgr (a grey image replicated, a BGR image copied)."""
    for ch in (1, 3):
        src = picture(rows, cols, ch, 173)
        exp = P4.to_bgr(src if ch == 1 else src.reshape(rows, cols, 3)).reshape(rows, cols * 3)

        def call(h, S, st, ch=ch):
            return lib.micv_gray_or_bgr_to_bgr8_dev(h, S.ptr("src"), _capi.DEPTH_8U, ch, rows, cols, S.pitch("src"), S.ptr("dst"), S.pitch("dst"), st)
        yield Case(f"{ch} channels", lambda src=src: [[Plane("src", src), out("dst", rows, cols * 3)]], ["dst"], call, lambda A, exp=exp: {"dst": exp})


def row_pyramid_montage(rows, cols):
    """Expected: _ps5_driver_ref.pyramid_montage.  Four levels, each a pitched plane of its own with its own stride
    (level_strides); 32F (a constant level, NaNs, a negative level) and 8U."""
    sizes = [(rows, cols), (rows >> 1, cols >> 1), ((rows >> 2) + 1, cols >> 2), (max(rows >> 3, 1), (cols >> 3) + 1)]
    r = rng_of(rows, cols, 174)
    lf = [(r.standard_normal(s) * 50).astype(f32) for s in sizes]
    lf[1][:] = f32(3.25)
    lf[2].flat[::3] = np.nan
    lf[3] = -np.abs(lf[3]) - f32(1)
    l8 = [r.integers(0, 256, s).astype(u8) for s in sizes]
    names = ["l0", "l1", "l2", "l3"]
    for levels, depth in ((lf, _capi.DEPTH_32F), (l8, _capi.DEPTH_8U)):
        exp = P5.pyramid_montage(levels)

        def call(h, S, st, depth=depth):
            return lib.micv_pyramid_montage_dev(h, pointer_array([S.ptr(n) for n in names]), (C.c_int * 4)(*[s[0] for s in sizes]),
                                                (C.c_int * 4)(*[s[1] for s in sizes]), (C.c_size_t * 4)(*[S.pitch(n) for n in names]), depth, S.ptr("dst"),
                                                S.pitch("dst"), st)
        yield Case(f"depth {depth}", lambda levels=levels: [[Plane(n, l) for n, l in zip(names, levels)] + [out("dst", 2 * rows, 2 * cols)]], ["dst"], call,
                   lambda A, exp=exp: {"dst": exp})


# -------------------------------------------------------------------------------------------------- ps5 ----------

def row_lk_warp_diff(rows, cols):
    """Expected: _ps5_driver_ref.warp_diff."""
    prev, nxt = lk_frames(rows, cols, 180)
    du, dv = flow_field(rows, cols, 181), flow_field(rows, cols, 182)
    exp = P5.warp_diff(prev, nxt, du, dv)

    def call(h, S, st):
        return lib.micv_lk_warp_diff_dev(h, S.ptr("prev"), S.pitch("prev"), S.ptr("next"), S.pitch("next"), S.ptr("du"), S.ptr("dv"), S.pitch("du"), rows, cols,
                                         S.ptr("diff"), S.pitch("diff"), st)
    yield Case("warp diff", lambda: [[Plane("prev", prev), Plane("next", nxt), Plane("du", du), Plane("dv", dv), out("diff", rows, cols, f32)]], ["diff"], call,
               lambda A: {"diff": exp})


def frame_sequence(rows, cols, n, seed):
    a, b = lk_frames(rows, cols, seed)
    c, d = lk_frames(rows, cols, seed + 1)
    return np.stack([a, b, c, d][:n])


def row_ps5_warp_diff_seq(rows, cols):
    """Expected: _ps5_driver_ref.warp_diff_seq.  mi_cv.h: "diff_f32, u, v: optional (NULL = not wanted) dense outputs, pair p
    at + p*rows*cols floats": no row padding and no gap between the pairs; the frames ("frame t at frames + t*frame_pitch
    bytes") and the 8-bit images ("pair p at diff_u8 + p*u8_pitch") are pitched and a gap apart.  With and without the
    optional outputs; window 7 (fused) and 9."""
    frames = frame_sequence(rows, cols, 3, 183)
    for win, full in ((7, True), (9, False)):
        e8, ed, eu, ev = P5.warp_diff_seq(frames, win)
        exp = {"u8": e8, **({"diff": ed, "u": eu, "v": ev} if full else {})}

        def call(h, S, st, win=win, full=full):
            opt = (S.ptr("diff"), S.ptr("u"), S.ptr("v")) if full else (None, None, None)
            return lib.micv_ps5_warp_diff_seq_dev(h, S.ptr("frames"), S.dist("frames"), 3, rows, cols, S.pitch("frames"), win, S.ptr("u8"), S.dist("u8"),
                                                  S.pitch("u8"), *opt, st)
        yield Case(f"win {win} optional outputs {full}",
                   lambda full=full: [[Plane("frames", frames), Plane("u8", shape=(2, rows, cols), dtype=u8)]
                                      + ([Plane(n, shape=(2, rows, cols), dtype=f32, dense=True, tight=True) for n in ("diff", "u", "v")] if full else [])],
                   list(exp), call, lambda A, exp=exp: exp)


def frames_u8(rows, cols, ch, seed):
    """Two 8-bit frames of `ch` channels from the synthetic pair: [2, rows, cols * ch]."""
    prev, nxt = lk_frames(rows, cols, seed)
    lo, hi = min(prev.min(), nxt.min()), max(prev.max(), nxt.max())
    q = [np.clip(np.rint((f - lo) * (255.0 / (hi - lo))), 0, 255).astype(u8) for f in (prev, nxt)]
    if ch == 3:
        q = [np.stack([f, np.roll(f, 1, axis=1), f[::-1]], 2).reshape(rows, cols * 3) for f in q]
    return q


def row_dense_lk_display(rows, cols):
    """Expected: _lk_chain_ref.to_gray + lk_flow (naive) or lk_flow_pyr (pyramidal) for u and v, _ps5_driver_ref.
    draw_velocity_vectors on `prev` for the arrows, _display_ref.normalize + jet for the colour maps.  First case: grey
    frames, naive mode, u / v and the two JET maps as four separate planes; second: BGR frames, pyramidal mode, "v lies
    behind u and jet_v behind jet_u in memory": each pair is one batch plane of two; third: no colour maps."""
    green = (0, 255, 0)
    for ch, mode, levels, paired, maps in ((1, _capi.LK_NAIVE, 1, False, True), (3, _capi.LK_PYRAMIDAL, 2, True, True), (1, _capi.LK_NAIVE, 1, False, False)):
        prev, nxt = frames_u8(rows, cols, ch, 184)
        shape3 = (lambda f: f.reshape(rows, cols, 3) if ch == 3 else f)
        gp, gn = L.to_gray(shape3(prev)), L.to_gray(shape3(nxt))
        eu, ev = L.lk_flow(gp, gn, 7) if mode == _capi.LK_NAIVE else L.lk_flow_pyr(gp, gn, 7, levels)
        arrows = P5.draw_velocity_vectors(shape3(prev), eu, ev, green)[0].reshape(rows, cols * 3)
        ju, jv = (D.jet(D.normalize(f)).reshape(rows, cols * 3) for f in (eu, ev))
        if paired:
            exp = {"uv": np.stack([eu, ev]), "arrows": arrows, "jet": np.stack([ju, jv])}
        else:
            exp = {"u": eu, "v": ev, "arrows": arrows, **({"ju": ju, "jv": jv} if maps else {})}

        def planes(prev=prev, nxt=nxt, paired=paired, maps=maps):
            g = [Plane("prev", prev), Plane("next", nxt), out("arrows", rows, cols * 3)]
            if paired:
                return [g + [Plane("uv", shape=(2, rows, cols), dtype=f32), Plane("jet", shape=(2, rows, cols * 3), dtype=u8)]]
            return [g + [out("u", rows, cols, f32), out("v", rows, cols, f32)] + ([out("ju", rows, cols * 3), out("jv", rows, cols * 3)] if maps else [])]

        def call(h, S, st, ch=ch, mode=mode, levels=levels, paired=paired, maps=maps):
            if paired:
                o = (S.ptr("uv"), S.ptr("uv", 1), S.pitch("uv"), S.ptr("arrows"), S.pitch("arrows"), S.ptr("jet"), S.ptr("jet", 1), S.pitch("jet"))
            else:
                j = (S.ptr("ju"), S.ptr("jv"), S.pitch("ju")) if maps else (None, None, 0)
                o = (S.ptr("u"), S.ptr("v"), S.pitch("u"), S.ptr("arrows"), S.pitch("arrows"), *j)
            return lib.micv_dense_lk_display_dev(h, S.ptr("prev"), S.ptr("next"), rows, cols, S.pitch("prev"), ch, _capi.DEPTH_8U, mode, 7, levels,
                                                 (C.c_uint8 * 3)(*green), *o, st)
        yield Case(f"{ch} channels mode {mode} paired {paired} maps {maps}", planes, list(exp), call, lambda A, exp=exp: exp)


def row_flow_bound_check(rows, cols):
    """Expected: the header's sentence restated in numpy: bit 0 of *flag is set "when |v| > bound or v is not finite anywhere
    in rows [row_begin, row_end) of the `batch` fields".  *flag is zeroed by the caller, so it is read and written.  A
    value over the bound inside the band of the last field; the same value only outside the band; a NaN in the band; a
    field that keeps the bound (the row padding and the gaps hold sentinel bytes, which are far over it as floats)."""
    batch, band, bound = 3, (rows // 4, rows - rows // 4), 4.0
    base = (rng_of(rows, cols, 185).integers(-1000, 1000, (batch, rows, cols)) / 256.0).astype(f32)
    for tag, where, value in (("inside", (2, band[1] - 1, cols - 1), 4.5), ("outside", (2, band[1], cols - 1), 4.5), ("above", (0, band[0] - 1, 0), -9.0),
                              ("nan", (1, band[0], 0), np.nan), ("at the bound", (1, band[0], 3), 4.0), ("none", None, 0.0)):
        v = base.copy()
        if where:
            v[where] = value
        b = v[:, band[0]:band[1]]
        flag = int((~np.isfinite(b) | (np.abs(b) > f32(bound))).any())

        def call(h, S, st):
            return lib.micv_flow_bound_check_dev(h, S.ptr("v"), batch, S.dist("v"), rows, cols, S.pitch("v"), band[0], band[1], bound, S.ptr("flag"), st)
        yield Case(tag, lambda v=v: [[Plane("v", v), Plane("flag", np.zeros((1, 1), u32), dense=True)]], ["flag"], call,
                   lambda A, flag=flag: {"flag": np.array([[flag]], u32)})


# ------------------------------------------------------------------------------------------------ others ---------

def row_lk_flow_pyr_batch(rows, cols):
    """Expected: _lk_chain_ref.lk_flow_pyr per pair.  Three pairs a gap apart (the pairs are f32, so pair_stride and
    opair_stride are multiples of 4 as the general rule gives them); window 7 and 15 (fused), 9 (generic); 3 levels."""
    batch = 3
    pairs = [lk_frames(rows, cols, 190 + i) for i in range(batch)]
    prev, nxt = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    for win in (7, 9, 15):
        e = [L.lk_flow_pyr(prev[i], nxt[i], win, 3) for i in range(batch)]
        eu, ev = np.stack([x[0] for x in e]), np.stack([x[1] for x in e])

        def call(h, S, st, win=win):
            return lib.micv_lk_flow_pyr_batch_dev(h, S.ptr("prev"), S.ptr("next"), batch, S.dist("prev"), rows, cols, S.pitch("prev"), win, 3, S.ptr("u"),
                                                  S.ptr("v"), S.dist("u"), S.pitch("u"), st)
        yield Case(f"win {win}", lambda: [[Plane("prev", prev), Plane("next", nxt), Plane("u", shape=(batch, rows, cols), dtype=f32),
                                           Plane("v", shape=(batch, rows, cols), dtype=f32)]],
                   ["u", "v"], call, lambda A, eu=eu, ev=ev: {"u": eu, "v": ev})


def row_central_moments(rows, cols):
    """Expected: _ps7_ref.central_moments per image.  It reads images and writes lists: mu, eta [batch][n] and raw
    [batch][3] have no pitch.  u8, u8 under MICV_MOMENTS_NORM_INF, f32 (also with MICV_MOMENTS_Y_FIXED); an all-zero
    image in the batch (NaN centroids: the canonical NaN)."""
    batch = 3
    orders = [(2, 0), (0, 2), (1, 1), (3, 0), (2, 1), (0, 3), (2, 2)]
    flat = (C.c_int * (2 * len(orders)))(*[v for pq in orders for v in pq])
    i8s = np.stack([image_u8(rows, cols, 195), np.zeros((rows, cols), u8), image_u8(rows, cols, 196) // 3])
    ifs = np.stack([image_f32(rows, cols, 197), image_f32(rows, cols, 198) * f32(0.01), np.abs(image_f32(rows, cols, 199))])
    for tag, imgs, typ, flags in (("u8", i8s, _capi.MOMENTS_U8, 0), ("u8 norm inf", i8s, _capi.MOMENTS_U8, _capi.MOMENTS_NORM_INF),
                                  ("f32", ifs, _capi.MOMENTS_F32, 0), ("f32 y fixed", ifs, _capi.MOMENTS_F32, _capi.MOMENTS_Y_FIXED)):
        e = [P7.central_moments(im, orders, bool(flags & _capi.MOMENTS_NORM_INF), bool(flags & _capi.MOMENTS_Y_FIXED)) for im in imgs]
        exp = {"mu": np.stack([x[0] for x in e]), "eta": np.stack([x[1] for x in e]), "raw": np.stack([x[2] for x in e])}

        def call(h, S, st, typ=typ, flags=flags):
            return lib.micv_central_moments_dev(h, S.ptr("imgs"), batch, S.dist("imgs"), S.pitch("imgs"), rows, cols, typ, flat, len(orders), flags,
                                                S.ptr("mu"), S.ptr("eta"), S.ptr("raw"), st)
        yield Case(tag, lambda imgs=imgs: [[Plane("imgs", imgs), out("mu", batch, len(orders), f32, dense=True), out("eta", batch, len(orders), f32, dense=True),
                                            out("raw", batch, 3, f32, dense=True)]],
                   ["mu", "eta", "raw"], call, lambda A, exp=exp: exp)


def row_bf_knn2_counted(rows, cols):
    """Expected: _ps4_feat_ref.knn2 on the counted rows; mi_cv.h gives the rows past the query count index -1 and
    distance +inf.  The descriptor lists are pitched as in the core table's micv_bf_knn2_dev row; the count words are
    int64 in device memory.  Counts below, at and above the capacities."""
    nq_cap, nt_cap, dim = cols, rows, 8
    r = rng_of(rows, cols, 200)
    q, t = r.integers(0, 256, (nq_cap, dim)).astype(f32), r.integers(0, 256, (nt_cap, dim)).astype(f32)
    t[3], q[2] = t[1], t[1]
    for cq, ct in ((nq_cap - 5, nt_cap - 3), (nq_cap, nt_cap), (nq_cap + 4, nt_cap + 2)):
        nq, nt = min(cq, nq_cap), min(ct, nt_cap)
        idx, dist = np.full((nq_cap, 2), -1, i32), np.full((nq_cap, 2), np.inf, f32)
        idx[:nq], dist[:nq] = F4.knn2(q[:nq], t[:nt])

        def call(h, S, st):
            return lib.micv_bf_knn2_counted_dev(h, S.ptr("q"), nq_cap, S.pitch("q"), S.ptr("cq"), S.ptr("t"), nt_cap, S.pitch("t"), S.ptr("ct"), dim,
                                                S.ptr("idx2"), S.ptr("dist2"), st)
        yield Case(f"counts {cq} x {ct}", lambda cq=cq, ct=ct: [[Plane("q", q), Plane("t", t), Plane("cq", np.array([[cq]], i64), dense=True),
                                                                 Plane("ct", np.array([[ct]], i64), dense=True), out("idx2", nq_cap, 2, i32, dense=True),
                                                                 out("dist2", nq_cap, 2, f32, dense=True)]],
                   ["idx2", "dist2"], call, lambda A, idx=idx, dist=dist: {"idx2": idx, "dist2": dist})


def bytes_pair(rows, cols, seed):
    left, right = stereo_pair(rows, cols, seed)
    return left.astype(u8), right.astype(u8)


def stereo_u8_cases(rows, cols, metric, batch):
    """mi_cv.h: "the image pointer and pitch need NO alignment": the two byte images sit at odd addresses with DIFFERENT odd
    paddings (3 and 5 bytes, so lstride != rstride), in a batch a gap apart; the int8 map is pitched as well.  Radius 2,
    disparities -6 .. 3."""
    rad, lo, hi = 2, -6, 3
    pairs = [bytes_pair(rows, cols, 240 + k) for k in range(max(batch, 1))]
    lefts, rights = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    one = (lambda a: a) if batch else (lambda a: a[0])
    single, many = (lib.micv_disparity_ssd_u8_dev, lib.micv_disparity_ssd_u8_batch_dev) if metric == "ssd" else \
                   (lib.micv_disparity_ncorr_u8_dev, lib.micv_disparity_ncorr_u8_batch_dev)
    flag_list = (0, _capi.STEREO_COLS_2R, _capi.STEREO_SERIAL, _capi.STEREO_ROLLING) if metric == "ssd" else (0, _capi.STEREO_COLS_2R, _capi.STEREO_ROLLING)
    for flags in flag_list:
        ref = None
        if metric == "ssd":  # on bytes ROLLING gives the fresh sums' result
            e = np.stack([S8.ssd_serial(l, r, rad, lo, hi) if flags == _capi.STEREO_SERIAL else S8.ssd_cuda(l, r, rad, lo, hi, flags & 3)
                          for l, r in pairs])
            ref = (lambda A, e=e: {"disp": one(e)})

        def call(h, S, st, flags=flags):
            if batch:
                return many(h, S.ptr("left"), S.dist("left"), S.pitch("left"), S.ptr("right"), S.dist("right"), S.pitch("right"), batch, rows, cols,
                            rad, lo, hi, flags, S.ptr("disp"), S.dist("disp"), S.pitch("disp"), st)
            return single(h, S.ptr("left"), S.pitch("left"), S.ptr("right"), S.pitch("right"), rows, cols, rad, lo, hi, flags, S.ptr("disp"),
                          S.pitch("disp"), st)
        yield Case(f"flags {flags}", lambda: [[Plane("left", one(lefts), pad=3), Plane("right", one(rights), pad=5),
                                               Plane("disp", shape=((batch,) if batch else ()) + (rows, cols), dtype=i8)]], ["disp"], call, ref)


def row_disparity_ssd_u8(rows, cols):
    """Expected: _stereo_ref.ssd_cuda / ssd_serial.  Flags 0, COLS_2R, SERIAL, ROLLING."""
    yield from stereo_u8_cases(rows, cols, "ssd", 0)


def row_disparity_ssd_u8_batch(rows, cols):
    """Expected: _stereo_ref.ssd_cuda / ssd_serial per pair.  Three pairs."""
    yield from stereo_u8_cases(rows, cols, "ssd", 3)


def row_disparity_ncorr_u8(rows, cols):
    """No reference module covers disparityNCorr (as the core table's micv_disparity_ncorr_dev row says): expected is the
    packed call.  Flags 0, COLS_2R, ROLLING."""
    yield from stereo_u8_cases(rows, cols, "ncc", 0)


def row_disparity_ncorr_u8_batch(rows, cols):
    """Expected: the packed call, as for the single entry.  Three pairs."""
    yield from stereo_u8_cases(rows, cols, "ncc", 3)


def row_pf_group_tick(rows, cols):
    """Expected: _pf_ref.PF.tick per member (x, y, x_var, y_var as float bits, then the status word).  The frame is the
    image argument: one shared frame, embedded, for two members (mean-squared-error and histogram similarity);
    states_dev is a dense list of 5 words per member.  Filters and group are opaque handles, made afresh for every
    layout from the same seeds."""
    from introtocomputervision_amd import pf
    for ch in (3, 1):
        frame, pos, model = filter_scene(rows, cols, ch, 205)
        specs = [dict(model=model[:7, :5].copy(), n=64, mode=PF.MSE, mse=9.0, ss=2.5, init=(float(pos[1]), float(pos[0])), alpha=0.2, seed=12),
                 dict(model=model[:8, :6].copy(), n=65, mode=PF.HIST, mse=3.0, ss=4.0, init=(-1.0, -1.0), alpha=0.05, seed=13)]
        want = []
        for s in specs:
            t = PF.PF(s["model"], rows, cols, s["n"], s["mode"], s["mse"], s["ss"], s["init"], s["alpha"], 0, s["seed"]).tick(frame)
            want.append(np.concatenate([np.asarray(t[:4], f32).view(i32), np.asarray([t[4]], u32).view(i32)]))
        exp = np.concatenate(want).reshape(1, 10)

        def call(h, S, st, specs=specs):
            members = [pf.ParticleFilter(s["model"], (cols, rows), s["n"], s["mode"], s["mse"], s["ss"], s["init"], s["alpha"], seed=s["seed"]) for s in specs]
            group = pf.FilterGroup(members)
            rc = lib.micv_pf_group_tick_dev(group._h, pointer_array([S.ptr("frame")]), (C.c_size_t * 1)(S.pitch("frame")), 1, st, S.ptr("states"))
            torch.cuda.synchronize()
            group.close()
            for m in members:
                m.close()
            return rc
        yield Case(f"{ch} channels", lambda frame=frame, ch=ch: [[Plane("frame", frame.reshape(rows, cols * ch)), out("states", 1, 10, i32, dense=True)]],
                   ["states"], call, lambda A, exp=exp: {"states": exp})


def filter_case(rows, cols, ch, seed):
    """(frame, spec, reference filter after one tick of the frame, its state words): an MSE filter of 120 particles."""
    frame, pos, model = filter_scene(rows, cols, ch, seed)
    spec = dict(model=model, n=120, mode=PF.MSE, mse=10.0, ss=3.0, init=(float(pos[1]), float(pos[0])), alpha=0.15, seed=31)
    r = PF.PF(spec["model"], rows, cols, spec["n"], spec["mode"], spec["mse"], spec["ss"], spec["init"], spec["alpha"], 0, spec["seed"])
    t = r.tick(frame)
    words = np.concatenate([np.asarray(t[:4], f32).view(i32), np.asarray([t[4]], u32).view(i32)]).reshape(1, 5)
    return frame, spec, r, (t[0], t[1]), words


def make_filter(spec, rows, cols):
    from introtocomputervision_amd import pf
    return pf.ParticleFilter(spec["model"], (cols, rows), spec["n"], spec["mode"], spec["mse"], spec["ss"], spec["init"], spec["alpha"], seed=spec["seed"])


def row_pf_tick(rows, cols):
    """Expected: _pf_ref.PF.tick (the five state words).  The frame is embedded; the filter is an opaque handle, made
    afresh for every layout from the same seed."""
    for ch in (3, 1):
        frame, spec, _, _, words = filter_case(rows, cols, ch, 210)

        def call(h, S, st, spec=spec):
            g = make_filter(spec, rows, cols)
            rc = lib.micv_pf_tick_dev(g._h, S.ptr("frame"), S.pitch("frame"), st, S.ptr("state"))
            torch.cuda.synchronize()
            g.close()
            return rc
        yield Case(f"{ch} channels", lambda frame=frame, ch=ch: [[Plane("frame", frame.reshape(rows, cols * ch)), out("state", 1, 5, i32, dense=True)]],
                   ["state"], call, lambda A, words=words: {"state": words})


def row_ps6_tick_display(rows, cols):
    """Expected: _pf_ref.PF.tick for the state, the particles and the estimate, _ps6_driver_ref.overlay for the picture.
    Into a separate image (the frame stays an input) and in place: "out may be the frame itself (then ostride ==
    stride)"."""
    size = (9.0, 7.0)
    for ch in (3, 1):
        frame, spec, r, centre, words = filter_case(rows, cols, ch, 211)
        pic = P6.overlay(frame.reshape(rows, cols, ch), r.particles, DOT, centre, size, BOX).reshape(rows, cols * ch)
        assert (pic != frame.reshape(rows, cols * ch)).any()
        for dst in ("out", "frame"):
            def call(h, S, st, spec=spec, dst=dst):
                g = make_filter(spec, rows, cols)
                rc = lib.micv_ps6_tick_display_dev(g._h, S.ptr("frame"), S.pitch("frame"), S.ptr(dst), S.pitch(dst), colour(DOT), size[0], size[1],
                                                   colour(BOX), st, S.ptr("state"))
                torch.cuda.synchronize()
                g.close()
                return rc
            yield Case(f"{ch} channels into {dst}",
                       lambda frame=frame, ch=ch, dst=dst: [[Plane("frame", frame.reshape(rows, cols * ch)), out("state", 1, 5, i32, dense=True)]
                                                            + ([out("out", rows, cols * ch)] if dst == "out" else [])],
                       [dst, "state"], call, lambda A, pic=pic, words=words, dst=dst: {dst: pic, "state": words})


def row_ps6_overlay_filter(rows, cols):
    """Expected: _ps6_driver_ref.overlay with the particles and the estimate of _pf_ref.PF after one tick.  The filter is an
    opaque handle: every layout makes a fresh one from the same seed, ticks it on a packed copy of the frame and paints
    the frame under test in place."""
    size = (9.0, 7.0)
    for ch in (1, 3):
        frame, spec, r, centre, _ = filter_case(rows, cols, ch, 170)
        pic = P6.overlay(frame.reshape(rows, cols, ch), r.particles, DOT, centre, size, BOX).reshape(rows, cols * ch)

        def call(h, S, st, spec=spec, frame=frame):
            g = make_filter(spec, rows, cols)
            g.tick(frame)
            rc = lib.micv_ps6_overlay_dev(g._h, S.ptr("img"), S.pitch("img"), colour(DOT), size[0], size[1], colour(BOX), st)
            torch.cuda.synchronize()
            g.close()
            return rc
        yield Case(f"{ch} channels", lambda frame=frame, ch=ch: [[Plane("img", frame.reshape(rows, cols * ch))]], ["img"], call,
                   lambda A, pic=pic: {"img": pic})


def corner_list(rows, cols, seed, n=40):
    """[n, 2] (y, x) int32: the four corners of the image and random pixels."""
    r = rng_of(rows, cols, seed)
    locs = [(0, 0), (0, cols - 1), (rows - 1, 0), (rows - 1, cols - 1)] + [(int(r.integers(0, rows)), int(r.integers(0, cols))) for _ in range(n - 4)]
    return np.asarray(locs, i32)


def row_sift_keypoints(rows, cols):
    """Expected: _ps4_feat_ref.keypoints: x, y and size byte for byte; the angle is atan2f-based, so the packed call is held
    to the reference within _ps4_feat_ref.angles_close (the tolerance of tests/test_ps4_feat_paths_gpu.py) and B to A by
    bytes.  locs_yx and kp_xysa have no pitch: dense lists."""
    gx, gy = gradients(rows, cols, 212)
    locs = corner_list(rows, cols, 213)
    exp = F4.keypoints(gx, gy, locs, 10.0)

    def close(got, ref):
        return np.array_equal(got[:, :3].view(u32), ref[:, :3].view(u32)) and bool(F4.angles_close(got[:, 3], ref[:, 3]).all())

    def call(h, S, st):
        return lib.micv_sift_keypoints_dev(h, S.ptr("gx"), S.ptr("gy"), rows, cols, S.pitch("gx"), S.ptr("locs"), len(locs), 10.0, S.ptr("kp"), st)
    yield Case("keypoints", lambda: [[Plane("gx", gx), Plane("gy", gy), Plane("locs", locs, dense=True), out("kp", len(locs), 4, f32, dense=True)]],
               ["kp"], call, lambda A: {"kp": exp}, approx={"kp": close})


def row_sift_descriptors(rows, cols):
    """Expected: _ps4_feat_ref.descriptors.  Keypoints on the corners, inside, outside the picture and with a size of 0
    (all-zero rows); the descriptor rows are pitched ("desc: n rows of 128 floats, dstride bytes apart")."""
    gx, gy = gradients(rows, cols, 214)
    kp = keypoints(rows, cols, 215)
    kp[:, 2] = np.where(np.arange(len(kp)) % 7 == 3, 0, 4 + np.arange(len(kp)) % 3)
    kp[kp[:, 3] < 0, 3] = 0
    exp = F4.descriptors(gx, gy, kp)
    assert exp.any()

    def call(h, S, st):
        return lib.micv_sift_descriptors_dev(h, S.ptr("gx"), S.ptr("gy"), rows, cols, S.pitch("gx"), S.ptr("kp"), len(kp), S.ptr("desc"), S.pitch("desc"), st)
    yield Case("descriptors", lambda: [[Plane("gx", gx), Plane("gy", gy), Plane("kp", kp, dense=True), out("desc", len(kp), 128, f32)]], ["desc"], call,
               lambda A: {"desc": exp})


def row_ps4_match_panels(rows, cols):
    """Expected: _ps4_driver_ref.match_panels (both panels and the generator word).  With glyphs and both panels; with
    MICV_PS4_NO_GLYPHS, a mask and the match panel alone (*rng_state stays).  The two grey images differ in width."""
    ca, cb = cols // 2 + 3, cols - (cols // 2 + 3)
    ia, ib = picture(rows, ca, 1, 216), picture(rows, cb, 1, 217)
    ka, kb = keypoints(rows, ca, 218), keypoints(rows, cb, 219)
    n = min(len(ka), len(kb))
    matches = np.asarray([[i, (i * 5) % n] for i in range(n)] + [[len(ka), 0], [0, -1]], i32)
    mask = (np.arange(len(matches)) % 3 != 1).astype(u8)
    state = 0x9E3779B97F4A7C15
    for glyphs in (True, False):
        ek, em, es = P4.match_panels(ia, ib, ka, len(ka) - 2, kb, len(kb), matches, len(matches) - 1, None if glyphs else mask, glyphs, P4.SEED, state)
        exp = {"mp": em.reshape(rows, cols * 3), "state": np.array([[es]], u64), **({"kpp": ek.reshape(rows, cols * 3)} if glyphs else {})}

        def call(h, S, st, glyphs=glyphs):
            return lib.micv_ps4_match_panels_dev(h, S.ptr("ia"), S.pitch("ia"), ca, S.ptr("ib"), S.pitch("ib"), cb, rows, S.ptr("ka"), S.ptr("na"), len(ka),
                                                 S.ptr("kb"), S.ptr("nb"), len(kb), S.ptr("m"), S.ptr("nm"), len(matches), None if glyphs else S.ptr("mask"),
                                                 0 if glyphs else _capi.PS4_NO_GLYPHS, P4.SEED, S.ptr("state"), S.ptr("kpp") if glyphs else None, S.ptr("mp"),
                                                 S.pitch("mp"), st)

        def planes(glyphs=glyphs):
            word = (lambda name, v: Plane(name, np.array([[v]], i64), dense=True))
            g = [Plane("ia", ia), Plane("ib", ib), Plane("ka", ka, dense=True), Plane("kb", kb, dense=True), Plane("m", matches, dense=True),
                 word("na", len(ka) - 2), word("nb", len(kb)), word("nm", len(matches) - 1), Plane("state", np.array([[state]], u64), dense=True),
                 out("mp", rows, cols * 3)]
            return [g + ([out("kpp", rows, cols * 3)] if glyphs else [Plane("mask", mask.reshape(-1, 1), dense=True)])]
        yield Case(f"glyphs {glyphs}", planes, list(exp), call, lambda A, exp=exp: exp)


def row_ps3_epipolar_display(rows, cols):
    """Expected: _ps3_ref.epipolar_endpoints for both sides, then _ps3_driver_ref.draw_epipolar_lines on each picture.
    Two pictures of different sizes; into separate pictures with the end points ([2][n][6], a dense list), and in place
    without them: "out may be the picture itself (then ostride == stride)".  F and the points are lists."""
    r = rng_of(rows, cols, 230)
    F = r.normal(0, 1, (3, 3)).astype(f32)
    F[:2, :2] *= f32(1e-2)  # lines that cross the pictures at every slope
    rb, cb, n = rows - 5, cols - 9, 24
    pa = np.c_[r.uniform(0, cols, n), r.uniform(0, rows, n)].astype(f32)
    pb = np.c_[r.uniform(0, cb, n), r.uniform(0, rb, n)].astype(f32)
    for ch, inplace in ((3, False), (1, True), (4, False)):
        ia, ib = picture(rows, cols, ch, 231), picture(rb, cb, ch, 232)
        ea, eb = G3.epipolar_endpoints(F, pb, 0, rows, cols), G3.epipolar_endpoints(F, pa, 1, rb, cb)
        wa = P3.draw_epipolar_lines(ia.reshape(rows, cols, ch).copy(), ea, DOT).reshape(rows, cols * ch)
        wb = P3.draw_epipolar_lines(ib.reshape(rb, cb, ch).copy(), eb, DOT).reshape(rb, cb * ch)
        assert (wa != ia).any() and (wb != ib).any()
        oa, ob = ("ia", "ib") if inplace else ("oa", "ob")
        exp = {oa: wa, ob: wb, **({} if inplace else {"ends": np.concatenate([ea, eb])})}

        def call(h, S, st, ch=ch, inplace=inplace, oa=oa, ob=ob):
            return lib.micv_ps3_epipolar_display_dev(h, S.ptr("F"), S.ptr("pa"), S.ptr("pb"), n, S.ptr("ia"), S.pitch("ia"), rows, cols, S.ptr("ib"), S.pitch("ib"),
                                                     rb, cb, ch, 0, colour(DOT), S.ptr(oa), S.pitch(oa), S.ptr(ob), S.pitch(ob),
                                                     None if inplace else S.ptr("ends"), st)
        yield Case(f"{ch} channels in place {inplace}",
                   lambda ia=ia, ib=ib, ch=ch, inplace=inplace: [[Plane("F", F, dense=True), Plane("pa", pa, dense=True), Plane("pb", pb, dense=True),
                                                                  Plane("ia", ia), Plane("ib", ib)]
                                                                 + ([] if inplace else [out("oa", rows, cols * ch), out("ob", rb, cb * ch),
                                                                                        out("ends", 2 * n, 6, f32, dense=True)])],
                   list(exp), call, lambda A, exp=exp: exp)


def row_ps4_harris_display(rows, cols):
    """mi_cv.h: "its four fields in `fields` ([4][rows * cols] f32, dense: gx, gy, R, corners)": four planes without row
    padding, back to back.  Expected: gx, gy from _ps4_feat_ref.sobel3; R from the packed call (no reference module restates
    the response bit for bit, as the core table's micv_harris_corners_dev row says); everything after it from the
    references ON that R: corners, list and count from _ps4_feat_ref.refine_corners, grad_panel and resp_u8 from
    _display_ref.normalize, dots from _ps4_driver_ref.draw_dots.  Window 5 (the fused form) and 9 (three launches)."""
    img = image_f32(rows, cols, 233)
    egx, egy = F4.sobel3(img)
    cap = rows * cols
    for win in (5, 9):
        def call(h, S, st, win=win):
            return lib.micv_ps4_harris_display_dev(h, S.ptr("img"), rows, cols, S.pitch("img"), 3, win, win / 3.0, 0.04, 0, 1e6, 2, S.ptr("fields"), S.ptr("locs"),
                                                   cap, S.ptr("count"), S.ptr("grad"), S.pitch("grad"), S.ptr("resp8"), S.pitch("resp8"), S.ptr("dots"),
                                                   S.pitch("dots"), st)

        def ref(A):
            R = A["fields"][2]
            corners, locs = F4.refine_corners(R, 1e6, 2)
            return {"fields": np.stack([egx, egy, R, corners]), "locs": locs[:cap], "count": np.array([[len(locs)]], i64),
                    "grad": np.concatenate([D.normalize(egx), D.normalize(egy)], axis=1), "resp8": D.normalize(R),
                    "dots": P4.draw_dots(img, corners).reshape(rows, cols * 3)}
        yield Case(f"win {win}", lambda: [[Plane("img", img), Plane("fields", shape=(4, rows, cols), dtype=f32, dense=True, tight=True),
                                           out("locs", cap, 2, i32, dense=True), out("count", 1, 1, i64, dense=True), out("grad", rows, 2 * cols),
                                           out("resp8", rows, cols), out("dots", rows, cols * 3)]],
                   ["fields", "locs", "count", "grad", "resp8", "dots"], call, ref)


def row_hough_peaks(rows, cols):
    """Expected: _hough_ref.hough_peaks.  mi_cv.h gives the accumulator and the lists no pitch: dense.  Fewer peaks than
    candidates and more (the entries past *count are not asserted, the ones past num_peaks keep the sentinel)."""
    acc = rng_of(rows, cols, 220).integers(0, 40, (rows, cols)).astype(i32)
    acc[0, 0], acc[rows - 1, cols - 1], acc[0, cols - 1] = 90, 90, 70
    for num, thr in ((6, 30), (rows * cols, 38)):
        exp = H.hough_peaks(acc, num, thr)
        assert len(exp) == num or num == rows * cols

        def call(h, S, st, num=num, thr=thr):
            return lib.micv_hough_peaks_dev(h, S.ptr("acc"), rows, cols, num, thr, S.ptr("peaks"), S.ptr("count"), st)
        yield Case(f"num_peaks {num} threshold {thr}",
                   lambda num=num: [[Plane("acc", acc, dense=True)], [out("peaks", num, 2, u32, dense=True), out("count", 1, 1, i64, dense=True)]],
                   ["peaks", "count"], call, lambda A, exp=exp: {"peaks": exp, "count": np.array([[len(exp)]], i64)})


def row_hough_circles_range_peaks(rows, cols):
    """Expected: _ps1_driver_ref.hough_circles_search (peaks, counts and accumulators).  The mask is the image argument;
    peaks_rc, counts and acc have no pitch: dense, the radii back to back.  num_peaks 4 with a threshold every radius
    meets at least four times, so every row of peaks_rc is specified; with and without the accumulators."""
    mask = edge_mask(rows, cols, 221)
    r0, r1, num, thr = 3, 5, 4, 1
    peaks, accs = P1.hough_circles_search(mask, r0, r1, num, thr, True)
    packed, counts = P1.pack_peaks(peaks, num)
    assert (counts == num).all()
    nr = r1 - r0 + 1
    for want in (True, False):
        exp = {"peaks": packed.reshape(nr, num, 2), "counts": counts.reshape(nr, 1), **({"acc": accs.astype(i32)} if want else {})}

        def call(h, S, st, want=want):
            return lib.micv_hough_circles_range_peaks_dev(h, S.ptr("mask"), rows, cols, S.pitch("mask"), r0, r1, num, thr, S.ptr("peaks"), S.ptr("counts"),
                                                          S.ptr("acc") if want else None, st)
        yield Case(f"accumulators {want}",
                   lambda want=want: [[Plane("mask", mask)], [Plane("peaks", shape=(nr, num, 2), dtype=u32, dense=True, tight=True),
                                                              out("counts", nr, 1, i64, dense=True)]]
                   + ([[Plane("acc", shape=(nr, rows, cols), dtype=i32, dense=True, tight=True)]] if want else []),
                   list(exp), call, lambda A, exp=exp: exp)


def row_parallel_lines(rows, cols):
    """Expected: _ps1_driver_ref.parallel_lines.  Lists only (no pitch): peaks in bins of 5 x 3, a count below max_peaks;
    the entries of out_rc past *out_count are not asserted."""
    r = rng_of(rows, cols, 222)
    peaks = np.c_[r.integers(0, rows, cols), r.integers(0, 30, cols)].astype(u32)
    n = len(peaks) - 3
    exp = P1.parallel_lines(peaks[:n], 3, 5)
    assert 0 < len(exp) < n

    def call(h, S, st):
        return lib.micv_parallel_lines_dev(h, S.ptr("peaks"), S.ptr("count"), len(peaks), 5, 3, S.ptr("out"), S.ptr("ocount"), st)
    yield Case("parallel", lambda: [[Plane("peaks", peaks, dense=True), Plane("count", np.array([[n]], i64), dense=True),
                                     out("out", len(peaks), 2, u32, dense=True), out("ocount", 1, 1, i64, dense=True)]],
               ["out", "ocount"], call, lambda A: {"out": exp, "ocount": np.array([[len(exp)]], i64)})


# ------------------------------------------------------------------------------------------------- the table -----
# name -> (row function, shapes, layouts)

TABLE = {
    # display (csrc/display.hip)
    "micv_normalize_minmax_dev": (row_normalize_minmax, SHAPES, ABCD),
    "micv_normalize_minmax_batch_dev": (row_normalize_minmax_batch, SHAPES, ABCD),
    "micv_apply_colormap_jet_dev": (row_apply_colormap_jet, SHAPES, ABCD),
    "micv_gain_noise_f32_dev": (row_gain_noise, SHAPES, ABCD),
    "micv_disparity_pair_dev": (row_disparity_pair, SHAPES, ABCD),
    "micv_disparity_pair_display_dev": (row_disparity_pair_display, SHAPES, ABCD),
    # ps0 (csrc/ps0.hip)
    "micv_mix_channels_u8_dev": (row_mix_channels, SHAPES, AB),
    "micv_pixel_replacement_u8_dev": (row_pixel_replacement, SHAPES, AB),
    "micv_mean_stddev_u8_dev": (row_mean_stddev, SHAPES, AB),
    "micv_ps0_arithmetic_u8_dev": (row_ps0_arithmetic, SHAPES, AB),
    "micv_subtract_sat_u8_dev": (row_subtract_sat, SHAPES, AB),
    "micv_add_noise_s8_u8_dev": (row_add_noise, SHAPES, AB),
    "micv_ps0_run_dev": (row_ps0_run, SHAPES, AB),
    # warp (csrc/warp.hip)
    "micv_warp_affine_dev": (row_warp_affine, SHAPES, ABCD),
    "micv_warp_affine_batch_dev": (row_warp_affine_batch, SHAPES, ABCD),
    "micv_add_weighted_dev": (row_add_weighted, SHAPES, ABCD),
    "micv_register_blend_dev": (row_register_blend, SHAPES, ABCD),
    "micv_invert_affine_dev": (row_invert_affine, SHAPES, ABCD),
    # motion history (csrc/mhi.hip)
    "micv_mhi_frame_difference_dev": (row_mhi_frame_difference, SHAPES, ABCD),
    "micv_mhi_frame_difference_c_dev": (row_mhi_frame_difference_c, SHAPES, ABCD),
    "micv_mhi_threshold_dev": (row_mhi_threshold, SHAPES, ABCD),
    "micv_mhi_update_dev": (row_mhi_update, SHAPES, ABCD),
    "micv_mhi_energy_dev": (row_mhi_energy, SHAPES, ABCD),
    "micv_mhi_history_seq_dev": (row_mhi_history_seq, SHAPES, ABCD),
    "micv_mhi_history_seq_c_dev": (row_mhi_history_seq_c, SHAPES, ABCD),
    "micv_mhi_history_batch_dev": (row_mhi_history_batch, SHAPES, ABCD),
    # overlays and panels
    "micv_draw_dots_dev": (row_draw_dots, SHAPES, AB),
    "micv_draw_keypoints_dev": (row_draw_keypoints, SHAPES, AB),
    "micv_draw_match_lines_dev": (row_draw_match_lines, SHAPES, AB),
    "micv_draw_segments_dev": (row_draw_segments, SHAPES, AB),
    "micv_draw_epipolar_lines_dev": (row_draw_epipolar_lines, SHAPES, AB),
    "micv_draw_velocity_vectors_dev": (row_draw_velocity_vectors, SHAPES, AB),
    "micv_draw_particles_dev": (row_draw_particles, SHAPES, AB),
    "micv_draw_rectangle_dev": (row_draw_rectangle, SHAPES, AB),
    "micv_ps6_overlay_dev": (row_ps6_overlay_filter, SHAPES, AB),
    "micv_ps6_overlay_list_dev": (row_ps6_overlay_list, SHAPES, AB),
    "micv_hconcat_dev": (row_hconcat, SHAPES, AB),
    "micv_gray_or_bgr_to_bgr8_dev": (row_gray_or_bgr_to_bgr8, SHAPES, AB),
    "micv_pyramid_montage_dev": (row_pyramid_montage, PYR_SHAPES, AB),
    # ps5 (csrc/ps5.hip)
    "micv_lk_warp_diff_dev": (row_lk_warp_diff, SHAPES, AB),
    "micv_ps5_warp_diff_seq_dev": (row_ps5_warp_diff_seq, SHAPES, AB),
    "micv_dense_lk_display_dev": (row_dense_lk_display, SHAPES, AB),
    "micv_flow_bound_check_dev": (row_flow_bound_check, SHAPES, AB),
    # others
    "micv_lk_flow_pyr_batch_dev": (row_lk_flow_pyr_batch, PYR_SHAPES, AB),
    "micv_central_moments_dev": (row_central_moments, SHAPES, AB),
    # entries whose own tests keep an output or an input block at an aligned address, or never re-read the input block
    "micv_disparity_ssd_u8_dev": (row_disparity_ssd_u8, SHAPES, ABCD),
    "micv_disparity_ssd_u8_batch_dev": (row_disparity_ssd_u8_batch, SHAPES, ABCD),
    "micv_disparity_ncorr_u8_dev": (row_disparity_ncorr_u8, SHAPES, ABCD),
    "micv_disparity_ncorr_u8_batch_dev": (row_disparity_ncorr_u8_batch, SHAPES, ABCD),
    "micv_bf_knn2_counted_dev": (row_bf_knn2_counted, SHAPES, AB),
    "micv_pf_group_tick_dev": (row_pf_group_tick, SHAPES, AB),
    # one-call drivers and list entries of ps1, ps3, ps4 and ps6
    "micv_ps3_epipolar_display_dev": (row_ps3_epipolar_display, SHAPES, AB),
    "micv_ps4_harris_display_dev": (row_ps4_harris_display, SHAPES, AB),
    "micv_pf_tick_dev": (row_pf_tick, SHAPES, AB),
    "micv_ps6_tick_display_dev": (row_ps6_tick_display, SHAPES, AB),
    "micv_sift_keypoints_dev": (row_sift_keypoints, SHAPES, AB),
    "micv_sift_descriptors_dev": (row_sift_descriptors, SHAPES, AB),
    "micv_ps4_match_panels_dev": (row_ps4_match_panels, SHAPES, AB),
    "micv_hough_peaks_dev": (row_hough_peaks, SHAPES, AB),
    "micv_hough_circles_range_peaks_dev": (row_hough_circles_range_peaks, SHAPES, AB),
    "micv_parallel_lines_dev": (row_parallel_lines, SHAPES, AB),
}

# ---------------------------------------------------------------------------------------------- accounting -------
# Every `_dev` entry point has a row in one of the two tables or stands here with its reason.  The only reasons:
NO_IMAGE = "no image or pitch argument: it takes only lists, matrices or opaque handles"
MULTI_DEVICE = "more than one device"
DEFERRED = "deferred: no row yet"
OWN = "own layout test: "


def own(test):
    """`test` (tests/<file>::<function>) calls the entry itself with every image or list argument off alignment (one
    element past an aligned address), with a padded pitch where the argument has one, in a sentinel-checked block."""
    return f"{OWN}{test} places every image argument off alignment, with a padded pitch, in a sentinel-checked block"


EXEMPT = {
    **{n: NO_IMAGE for n in (
        "micv_calib_ls_trials_dev", "micv_calib_svd_dev", "micv_fundamental_ls_dev", "micv_fundamental_rank_reduce_dev",
        "micv_fundamental_normalized_dev", "micv_epipolar_endpoints_dev", "micv_camera_center_dev", "micv_geom_sample_indices_dev",
        "micv_knn_predict_dev", "micv_knn_confusion_dev", "micv_ransac_solve_dev", "micv_ransac_solve_matches_dev",
        "micv_pf_particles_dev", "micv_pf_weights_dev", "micv_allreduce_sum_i32_dev")},
    **{n: MULTI_DEVICE for n in ("micv_lk_flow_pyr_rowshard_dev", "micv_lk_flow_pyr_rowshard_virtual_dev", "micv_hough_lines_rowshard_dev")},
    # lists a kimage_stride apart, outputs back to back: every list of the call sits in a _layout block there
    "micv_ransac_solve_pairs_dev": own("tests/test_ransac_pairs_gpu.py::test_containment"),
    # run8 of that file: the byte image at offsets 0..3 with odd pitches, the planes 4-byte aligned only, every block re-read
    "micv_harris_corners_u8_dev": own("tests/test_harris_u8_gpu.py::test_every_fused_form"),
    "micv_harris_corners_u8_batch_dev": own("tests/test_harris_u8_gpu.py::test_batch_elements_are_the_single_calls"),
    # run8 of that file: image, keypoints, descriptors and counts in one _layout block
    "micv_sift_descriptors_u8_dev": own("tests/test_sift_u8_gpu.py::test_single_call_every_shape"),
    "micv_sift_descriptors_u8_batch_dev": own("tests/test_sift_u8_gpu.py::test_batch_equals_single_calls"),
    "micv_bf_match_pairs_dev": own("tests/test_match_pairs_gpu.py::test_containment"),
}
# DEFERRED is a reason only these may carry (none does: each has a row)
MAY_DEFER = {"micv_ps3_epipolar_display_dev", "micv_ps4_harris_display_dev", "micv_ps4_match_panels_dev", "micv_ps6_tick_display_dev",
             "micv_pf_tick_dev", "micv_hough_peaks_dev", "micv_hough_circles_range_peaks_dev", "micv_parallel_lines_dev", "micv_sift_keypoints_dev",
             "micv_sift_descriptors_dev"}


def account(signatures, tables, exempt):
    """Collection time: the `_dev` names of `signatures` are exactly the rows of `tables` plus `exempt`, no name twice; a
    test named as an entry's own layout test exists, in a file that calls that entry by name."""
    dev = {n for n in signatures if n.endswith("_dev")}
    sets = [set(t) for t in tables] + [set(exempt)]
    for i, a in enumerate(sets):
        for b in sets[i + 1:]:
            assert not a & b, f"listed twice: {sorted(a & b)}"
    listed = set().union(*sets)
    assert dev == listed, f"without a row or a reason: {sorted(dev - listed)}; no such entry point: {sorted(listed - dev)}"
    here = os.path.dirname(os.path.abspath(__file__))
    for name, reason in exempt.items():
        if reason.startswith(OWN):
            path, test = reason[len(OWN):].split(" ")[0].split("::")
            assert path.startswith("tests/"), reason
            with open(os.path.join(here, path[len("tests/"):])) as f:
                text = f.read()
            assert f"def {test}(" in text and f".{name}(" in text, f"{name}: {path}::{test} does not carry it"
        else:
            assert reason in (NO_IMAGE, MULTI_DEVICE, DEFERRED), (name, reason)
            assert reason != DEFERRED or name in MAY_DEFER, name
    return len(dev)


N_DEV = account(_capi.SIGNATURES, [core.TABLE, TABLE], EXEMPT)

PARAMS = [pytest.param(name, shape, id=f"{name[5:]}-{shape[0]}x{shape[1]}") for name, (_, shapes, _) in TABLE.items() for shape in shapes]


@pytest.mark.parametrize("name,shape", PARAMS)
def test_containment(name, shape):
    fn, _, layouts = TABLE[name]
    cases = list(fn(*shape))
    assert cases, name
    for case in cases:
        case.tag = f"{name} {shape[0]}x{shape[1]} {case.tag}"
        run_case(case, layouts)
