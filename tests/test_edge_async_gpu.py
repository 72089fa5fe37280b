"""generateEdge without a host wait (canny_uf.hip): the union-find hysteresis on crafted masks against
_edge_ref.hysteresis, the `_async` chains and the batch against the references and against the polled entries, the
layout of every new device-pointer entry through the _layout harness, the refusals, and one capture into a graph.
Every comparison is np.array_equal: the result is a set."""
import ctypes as C

import numpy as np
import pytest

import _edge_ref as E
import _layout as L
import _ps1_driver_ref as R
from test_canny import _ramp_path_image, _serpentine, scene
from test_ps1_paths_gpu import _scene

pytestmark = pytest.mark.gpu


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def _hough():
    from introtocomputervision_amd import hough
    return hough


def _ps1():
    from introtocomputervision_amd import ps1
    return ps1


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def ctx():
    from introtocomputervision_amd import _capi
    c = _capi.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------ the stage on crafted masks ------

SHAPES = [(1, 1), (1, 200), (200, 1)] + [(r, c) for r in (2, 63, 64) for c in (63, 64, 65, 129)]


def serpentine_mask(rows, cols):
    """A one-pixel path: every other row full, joined at alternating ends; its only strong pixel at the far end."""
    cand = np.zeros((rows, cols), np.uint8)
    cand[0::2] = 1
    for k, y in enumerate(range(1, rows - 1, 2)):
        cand[y, 0 if k % 2 else cols - 1] = 1
    last = (rows - 1) // 2 * 2
    strong = np.zeros_like(cand)
    strong[last, 0 if (last // 2) % 2 else cols - 1] = 255
    return cand, strong


def diagonal_masks(rows, cols):
    """Only diagonal contacts: both one-pixel diagonals (through x = 63 / 64 where the shape reaches them) over a pixel
    checkerboard around the columns where four words meet, seeded at one corner."""
    yy, xx = np.mgrid[0:rows, 0:cols]
    cand = ((yy == xx) | (yy == cols - 1 - xx)).astype(np.uint8)
    cand[(np.abs(xx % 64 - 31.5) > 26) & ((yy + xx) % 2 == 0)] = 7
    strong = np.zeros_like(cand)
    strong[0, 0] = 1
    return cand, strong


def random_masks(rows, cols, density, seed):
    rng = np.random.default_rng(seed)
    cand = (rng.random((rows, cols)) < density).astype(np.uint8) * 255
    strong = np.zeros_like(cand)
    strong[rng.integers(0, rows, 3), rng.integers(0, cols, 3)] = 1
    return cand, strong


def degenerate_masks(rows, cols):
    ones, zeros = np.ones((rows, cols), np.uint8), np.zeros((rows, cols), np.uint8)
    one = zeros.copy()
    one[rows - 1, cols - 1] = 9
    outside = ones.copy()  # the strong pixel is no candidate, and it still seeds the rest
    outside[rows // 2, cols // 2] = 0
    seed = zeros.copy()
    seed[rows // 2, cols // 2] = 1
    return {"all candidates, one strong": (ones, one, np.full((rows, cols), 255, np.uint8)),
            "no strong": (ones, zeros, zeros),
            "strong outside cand": (outside, seed, np.full((rows, cols), 255, np.uint8)),
            "nothing set": (zeros, zeros, zeros)}


def check_hysteresis(cand, strong, exp=None, label=""):
    ref = np.where(E.hysteresis(cand != 0, strong != 0), 255, 0).astype(np.uint8)
    if exp is not None:
        assert np.array_equal(ref, exp), label
    hough = _hough()
    dc, ds = dev(cand), dev(strong)
    for run in range(2):  # twice: the parent plane is not cleared between calls
        assert np.array_equal(host(hough.hysteresis(dc, ds)), ref), (label, run)
    return ref


@pytest.mark.parametrize("rows,cols", SHAPES, ids=lambda v: str(v))
def test_hysteresis_at_word_and_row_edges(rows, cols):
    check_hysteresis(*serpentine_mask(rows, cols), label="serpentine")
    check_hysteresis(*diagonal_masks(rows, cols), label="diagonals")
    check_hysteresis(*random_masks(rows, cols, 0.42, rows * 1000 + cols), label="random")
    for name, (cand, strong, exp) in degenerate_masks(rows, cols).items():
        check_hysteresis(cand, strong, exp, label=name)


def test_hysteresis_serpentine_65x129_seeded_at_the_far_end():
    cand, strong = serpentine_mask(65, 129)
    ref = check_hysteresis(cand, strong)
    assert np.array_equal(ref != 0, (cand | strong) != 0) and strong.sum() == 255  # one seed promotes the whole path


def test_hysteresis_diagonals_through_word_corners():
    cand, strong = diagonal_masks(130, 130)
    ref = check_hysteresis(cand, strong)
    assert ref[129, 129] == 255 and ref[63, 63] == 255 and ref[64, 64] == 255
    for name, (c, s, exp) in degenerate_masks(130, 200).items():
        check_hysteresis(c, s, exp, label=name)


@pytest.mark.parametrize("seed", range(4))
def test_hysteresis_random_near_critical(seed):
    """Density 0.42 on 130 x 200: the kept set is the winding near-critical kind, 43 - 80 % of the candidates (whole
    per cent: the four seeds give 43.5, 80.5, 79.6 and 63.7) and reaches from the first column or the one after it to
    the last, through every 64-column word.  Density 0.38 drops most, 0.46 keeps nearly all."""
    cand, strong = random_masks(130, 200, 0.42, seed)
    ref = check_hysteresis(cand, strong)
    kept = (ref != 0).sum() / ((cand | strong) != 0).sum()
    assert 43 <= int(100 * kept) <= 80 and (ref != 0).any(axis=0)[1:].all(), kept
    for density in (0.38, 0.46):
        check_hysteresis(*random_masks(130, 200, density, seed), label=density)


def test_hysteresis_host_entry_and_pitched_numpy_views():
    cand, strong = random_masks(70, 150, 0.42, 11)
    ref = np.where(E.hysteresis(cand != 0, strong != 0), 255, 0).astype(np.uint8)
    wide = np.zeros((70, 190), np.uint8)
    wide[:, 7:157] = cand
    assert np.array_equal(_hough().hysteresis(wide[:, 7:157], strong), ref)


# ------------------------------------------------------------------ the chains ------

def _async_and_polled(img, gs, sigma, lo, hi):
    mod = _hough() if img.dtype == np.uint8 else _ps1()
    d = dev(img)
    got = host(mod.generateEdge(d, gs, sigma, lo, hi, wait=False))
    return got, host(mod.generateEdge(d, gs, sigma, lo, hi))


CHAIN_CASES = [(33, 35, 3, 1.0, 20, 60)] + [(97, 131, gs, 0.0001 if gs == 1 else gs / 3.0, 10, 50) for gs in (1, 3, 5, 19)] + [
    (480, 640, 5, 1.4, 20, 60)]


@pytest.mark.parametrize("rows,cols,gs,sigma,lo,hi", CHAIN_CASES)
def test_generate_edge_async_on_scenes(rows, cols, gs, sigma, lo, hi):
    img = _scene(rows, cols, rows)
    exp = E.generate_edge(img, gs, sigma, lo, hi)
    got, polled = _async_and_polled(img, gs, sigma, lo, hi)
    assert np.array_equal(got, exp) and np.array_equal(polled, exp)
    f = img.astype(np.float32) + np.float32(0.25)
    expf = R.generate_edge_f32(f, gs, sigma, lo, hi)
    gotf, polledf = _async_and_polled(f, gs, sigma, lo, hi)
    assert np.array_equal(gotf, expf) and np.array_equal(polledf, expf)


def _serpentine_image():
    path = _serpentine(250, 300, step=4)
    return _ramp_path_image(250, 300, path, strong_at=len(path) - 1), path


def _corner_image():
    """The diagonal-contact image of test_ps1_paths_gpu.test_hysteresis_diagonal_touches_at_tile_corners."""
    rows, cols = 190, 200
    img = np.full((rows, cols), 100, np.int64)
    yy, xx = np.mgrid[0:rows, 0:cols]
    near = (np.abs(xx - 63.5) < 6) | (np.abs(yy - 61.5) < 6) | (np.abs(yy - 123.5) < 6)
    img[near & ((yy + xx) % 2 == 0)] = 112
    for i in range(0, 180):
        img[i + 5, min(cols - 1, i + 2)] = 121
    img[2:5, 0:3] = 250
    return np.clip(img, 0, 255).astype(np.uint8)


def test_generate_edge_async_serpentine_and_corners():
    img, path = _serpentine_image()
    exp = E.generate_edge(img, 1, 0.0001, 10, 60)
    assert (exp > 0).sum() > len(path) // 2
    got, polled = _async_and_polled(img, 1, 0.0001, 10, 60)
    assert np.array_equal(got, exp) and np.array_equal(polled, exp)
    img = _corner_image()
    for lo, hi in ((5, 200), (20, 90), (1, 3)):
        exp = E.generate_edge(img, 1, 0.0001, lo, hi)
        got, polled = _async_and_polled(img, 1, 0.0001, lo, hi)
        assert np.array_equal(got, exp) and np.array_equal(polled, exp), (lo, hi)


def test_generate_edge_async_dense_candidates_and_swapped_thresholds():
    """Uniform noise at 70 x 107, Gaussian 7, sigma 2.1, low threshold 0: the dense-candidate kind with winding chains."""
    img = np.random.default_rng(5).integers(0, 256, (70, 107)).astype(np.uint8)
    exp = E.generate_edge(img, 7, 2.1, 0, 40)
    got, polled = _async_and_polled(img, 7, 2.1, 0, 40)
    assert np.array_equal(got, exp) and np.array_equal(polled, exp) and 0 < (exp > 0).sum() < exp.size
    got, polled = _async_and_polled(img, 7, 2.1, 40, 0)  # the thresholds in swapped order
    assert np.array_equal(got, exp) and np.array_equal(polled, exp)
    f = img.astype(np.float32)
    gotf, polledf = _async_and_polled(f, 7, 2.1, 40, 0)
    assert np.array_equal(gotf, R.generate_edge_f32(f, 7, 2.1, 0, 40)) and np.array_equal(polledf, gotf)


def test_generate_edge_f32_async_on_special_floats():
    f = scene(60, 90, seed=4).astype(np.float32) + np.float32(0.25)
    f[10, 10], f[11, 40], f[12, 70] = np.nan, np.inf, -np.inf
    f[30, 5:20], f[31, 5:20], f[32, 5:20] = 255.5, 254.5, -0.5
    f[50, 50] = 3e9
    for gs, sigma in [(1, 0.5), (3, 0.9)]:
        exp = R.generate_edge_f32(f, gs, sigma, 30, 90)
        got, polled = _async_and_polled(f, gs, sigma, 30, 90)
        assert np.array_equal(got, exp) and np.array_equal(polled, exp) and exp.any()


# ------------------------------------------------------------------ the batch ------

BATCH_SETTINGS = (5, 1.4, 20, 60)


def _mixed_images(batch, rows=70, cols=107):
    """Scenes, noise, an image whose every candidate is strong beside one with no candidate at all."""
    rng = np.random.default_rng(batch)
    imgs = []
    for i in range(batch):
        kind = i % 4 if batch > 1 else 0
        if kind == 0:
            imgs.append(_scene(rows, cols, 10 * batch + i))
        elif kind == 1:  # sharp bars: every edge pixel is far above the high threshold
            img = np.zeros((rows, cols), np.uint8)
            img[:, (np.arange(cols) // 9) % 2 == 0] = 255
            imgs.append(img)
        elif kind == 2:
            imgs.append(np.full((rows, cols), 77, np.uint8))  # flat: no candidate
        else:
            imgs.append(rng.integers(0, 256, (rows, cols)).astype(np.uint8))
    return np.stack(imgs)


@pytest.fixture(scope="module")
def polled_singles():
    """Batch size -> (images, the polled single call on each): computed once, shared, never changed."""
    out = {}
    for batch in (1, 3, 9):
        imgs = _mixed_images(batch)
        ref = np.stack([host(_hough().generateEdge(dev(im), *BATCH_SETTINGS)) for im in imgs])
        ref.setflags(write=False)
        out[batch] = (imgs, ref)
    return out


@pytest.mark.parametrize("batch", [1, 3, 9])
def test_batch_equals_the_polled_single_calls(polled_singles, batch):
    imgs, ref = polled_singles[batch]
    hough = _hough()
    got = host(hough.generateEdgeBatch(dev(imgs), *BATCH_SETTINGS))
    assert np.array_equal(got, ref)
    for i, im in enumerate(imgs):
        assert np.array_equal(ref[i], E.generate_edge(im, *BATCH_SETTINGS)), i
    if batch > 1:  # nothing leaks between the all-strong image and the empty one beside it
        w, s = E.suppress(E.blur(imgs[1], 5, 1.4), 20, 60)
        assert s.any() and not w.any() and not got[2].any() and np.array_equal(got[1] != 0, s)
    # the host entry on a list, one element an ROI of a wider array
    wide = np.zeros((70, 140), np.uint8)
    wide[:, 20:127] = imgs[0]
    assert np.array_equal(hough.generateEdgeBatch([wide[:, 20:127]] + list(imgs[1:]), *BATCH_SETTINGS), ref)


def test_batch_with_padded_image_distance_and_pitch(polled_singles):
    import torch
    imgs, ref = polled_singles[3]
    big = torch.zeros((3, 70 + 5, 107 + 21), dtype=torch.uint8, device="cuda")
    view = big[:, 2:72, 3:110]
    view.copy_(dev(imgs))
    assert view.stride(0) > 70 * view.stride(1) and view.stride(1) > 107
    assert np.array_equal(host(_hough().generateEdgeBatch(view, *BATCH_SETTINGS)), ref)


def scratch_per_image(rows, cols):
    """canny_uf.hip's layout: the blur plane, the two bit planes and the parent plane, each rounded up to 256 bytes."""
    up = lambda b: -(-b // 256) * 256
    return up(rows * cols) + 2 * up(rows * -(-cols // 64) * 8) + up(rows * cols * 4)


def test_batch_in_pieces_under_a_scratch_bound():
    rows, cols, batch = 48, 200, 45
    assert scratch_per_image(rows, cols) == 9728 + 2 * 1536 + 38400
    piece = (1 << 20) // scratch_per_image(rows, cols)
    assert piece == 20 and -(-batch // piece) == 3  # 1 MiB holds 20 images: pieces of 20, 20 and 5
    rng = np.random.default_rng(45)
    imgs = np.stack([_scene(rows, cols, i) if i % 2 else rng.integers(0, 256, (rows, cols)).astype(np.uint8) for i in range(batch)])
    d = dev(imgs)
    whole = host(_hough().generateEdgeBatch(d, 3, 1.0, 20, 60))
    pieces = host(_hough().generateEdgeBatch(d, 3, 1.0, 20, 60, scratch_mb=1))
    assert np.array_equal(pieces, whole)
    for i in (0, 19, 20, 39, 40, 44):  # the first and the last image of every piece
        assert np.array_equal(whole[i], E.generate_edge(imgs[i], 3, 1.0, 20, 60)), i


# ------------------------------------------------------------------ layout ------

def test_layout_of_every_new_device_entry(ctx):
    """Each image one element off alignment, a padded pitch, a sentinel-checked block: nothing outside the output view
    changes, and the view holds the reference's bytes."""
    import torch
    from introtocomputervision_amd._capi import check, lib
    rows, cols, st = 70, 107, _stream()
    img = _scene(rows, cols, 3)
    gauss = (5, 1.4, 20.0, 60.0)

    S = L.slab([L.Plane("src", img), L.Plane("dst", shape=(rows, cols), dtype=np.uint8)])
    check(lib.micv_generate_edge_async(ctx.handle, S.ptr("src"), rows, cols, S.pitch("src"), *gauss, S.ptr("dst"), S.pitch("dst"), st))
    L.check(S, ["dst"], {"dst": E.generate_edge(img, *gauss)}, "micv_generate_edge_async")

    f = (img.astype(np.float32) * np.float32(1.01) + np.float32(0.25)).astype(np.float32)
    S = L.slab([L.Plane("src", f), L.Plane("dst", shape=(rows, cols), dtype=np.uint8)])
    check(lib.micv_generate_edge_f32_async(ctx.handle, S.ptr("src"), rows, cols, S.pitch("src"), *gauss, S.ptr("dst"), S.pitch("dst"), st))
    L.check(S, ["dst"], {"dst": R.generate_edge_f32(f, *gauss)}, "micv_generate_edge_f32_async")

    cand, strong = random_masks(rows, cols, 0.42, 2)
    S = L.slab([L.Plane("cand", cand), L.Plane("strong", strong, pad=5), L.Plane("dst", shape=(rows, cols), dtype=np.uint8, pad=7)])
    check(lib.micv_hysteresis_u8_async(ctx.handle, S.ptr("cand"), S.pitch("cand"), S.ptr("strong"), S.pitch("strong"), rows, cols,
                                       S.ptr("dst"), S.pitch("dst"), st))
    L.check(S, ["dst"], {"dst": np.where(E.hysteresis(cand != 0, strong != 0), 255, 0).astype(np.uint8)}, "micv_hysteresis_u8_async")

    imgs = _mixed_images(3)
    S = L.slab([L.Plane("src", imgs), L.Plane("dst", shape=imgs.shape, dtype=np.uint8)])
    check(lib.micv_generate_edge_batch_async(ctx.handle, S.ptr("src"), 3, S.dist("src"), rows, cols, S.pitch("src"), *gauss, S.ptr("dst"),
                                             S.dist("dst"), S.pitch("dst"), 0, st))
    L.check(S, ["dst"], {"dst": np.stack([E.generate_edge(im, *gauss) for im in imgs])}, "micv_generate_edge_batch_async")
    torch.cuda.synchronize()


# ------------------------------------------------------------------ refusals ------

def test_refusals_enqueue_nothing(ctx):
    from introtocomputervision_amd._capi import EINVAL, lib
    rows, cols, st = 20, 30, _stream()
    S = L.slab([L.Plane("src", np.zeros((2, rows, cols), np.uint8)), L.Plane("f32", np.zeros((rows, cols), np.float32)),
                L.Plane("dst", shape=(2, rows, cols), dtype=np.uint8)])
    h, src, f32, dst = ctx.handle, S.ptr("src"), S.ptr("f32"), S.ptr("dst")
    sp, fp, dp, sd, dd = S.pitch("src"), S.pitch("f32"), S.pitch("dst"), S.dist("src"), S.dist("dst")
    g = (3, 1.0, 20.0, 60.0)
    big = 65536  # a fake 65536 x 65536 image: 2^32 pixels, refused before anything is enqueued
    calls = {
        "edge null src": lambda: lib.micv_generate_edge_async(h, None, rows, cols, sp, *g, dst, dp, st),
        "edge null dst": lambda: lib.micv_generate_edge_async(h, src, rows, cols, sp, *g, None, dp, st),
        "edge pitch": lambda: lib.micv_generate_edge_async(h, src, rows, cols, cols - 1, *g, dst, dp, st),
        "edge out pitch": lambda: lib.micv_generate_edge_async(h, src, rows, cols, sp, *g, dst, cols - 1, st),
        "edge even gaussian": lambda: lib.micv_generate_edge_async(h, src, rows, cols, sp, 4, 1.0, 20.0, 60.0, dst, dp, st),
        "edge 2^32 pixels": lambda: lib.micv_generate_edge_async(h, src, big, big, big, *g, dst, big, st),
        "f32 null src": lambda: lib.micv_generate_edge_f32_async(h, None, rows, cols, fp, *g, dst, dp, st),
        "f32 pitch": lambda: lib.micv_generate_edge_f32_async(h, f32, rows, cols, cols * 4 - 4, *g, dst, dp, st),
        "f32 even gaussian": lambda: lib.micv_generate_edge_f32_async(h, f32, rows, cols, fp, 2, 1.0, 20.0, 60.0, dst, dp, st),
        "f32 2^32 pixels": lambda: lib.micv_generate_edge_f32_async(h, f32, big, big, big * 4, *g, dst, big, st),
        "hysteresis null strong": lambda: lib.micv_hysteresis_u8_async(h, src, sp, None, sp, rows, cols, dst, dp, st),
        "hysteresis pitch": lambda: lib.micv_hysteresis_u8_async(h, src, sp, src, cols - 1, rows, cols, dst, dp, st),
        "hysteresis 2^32 pixels": lambda: lib.micv_hysteresis_u8_async(h, src, big, src, big, big, big, dst, big, st),
        "batch null": lambda: lib.micv_generate_edge_batch_async(h, src, 2, sd, rows, cols, sp, *g, None, dd, dp, 0, st),
        "batch 0": lambda: lib.micv_generate_edge_batch_async(h, src, 0, sd, rows, cols, sp, *g, dst, dd, dp, 0, st),
        "batch -1": lambda: lib.micv_generate_edge_batch_async(h, src, -1, sd, rows, cols, sp, *g, dst, dd, dp, 0, st),
        "batch pitch": lambda: lib.micv_generate_edge_batch_async(h, src, 2, sd, rows, cols, cols - 1, *g, dst, dd, dp, 0, st),
        "batch even gaussian": lambda: lib.micv_generate_edge_batch_async(h, src, 2, sd, rows, cols, sp, 6, 1.0, 20.0, 60.0, dst, dd, dp, 0, st),
        "batch 2^32 pixels": lambda: lib.micv_generate_edge_batch_async(h, src, 2, big * big, big, big, big, *g, dst, big * big, big, 0, st),
        "batch overlapping outputs": lambda: lib.micv_generate_edge_batch_async(h, src, 2, sd, rows, cols, sp, *g, dst, dp, dp, 0, st),
    }
    for name, call in calls.items():
        assert call() == EINVAL, name
    L.check(S, [], {}, "refusals")  # the output sentinel, and everything else, is intact
    srcs, strides = (C.c_void_p * 1)(0), (C.c_size_t * 1)(cols)
    assert lib.micv_generate_edge_batch_host(h, srcs, strides, 1, rows, cols, *g, srcs, strides) == EINVAL
    assert lib.micv_generate_edge_batch_host(h, srcs, strides, 0, rows, cols, *g, srcs, strides) == EINVAL
    assert lib.micv_hysteresis_u8_host(h, None, cols, None, cols, rows, cols, None, cols) == EINVAL


# ------------------------------------------------------------------ capture ------

def test_generate_edge_async_in_a_captured_graph():
    """The one property the polled entry cannot have: the call sits in a captured stream.  A warm-up call of the same
    shape sizes the arena first; the graph is then replayed on two images written into its static input."""
    import torch
    hough = _hough()
    a, b = _scene(97, 131, 1), _scene(97, 131, 2)
    static_in = dev(a)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        hough.generateEdge(static_in, 5, 1.4, 20, 60, wait=False)  # warm-up on the capturing stream: its context, its arena
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        static_out = hough.generateEdge(static_in, 5, 1.4, 20, 60, wait=False)
    for img in (b, a):
        static_in.copy_(dev(img))
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(host(static_out), E.generate_edge(img, 5, 1.4, 20, 60))
