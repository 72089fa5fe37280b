"""The layout harness tests/_layout.py checks what it claims to: every planted fault is named with plane, row and
column.  CPU: the same Slab / check code on device="cpu" tensors, the "entry point" a few numpy stores."""
import numpy as np
import pytest

import _layout as Y


def make(band=None):
    rng = np.random.default_rng(7)
    src = rng.standard_normal((2, 9, 13)).astype(np.float32)
    planes = [Y.Plane("src", data=src),
              Y.Plane("mask", data=rng.integers(0, 256, (9, 13)).astype(np.uint8)),
              Y.Plane("dst", shape=(2, 9, 13), dtype=np.float32, band=band)]
    return Y.slab(planes, device="cpu"), src


def good_call(s, src, band=None):
    """dst = 2 * src, written through the slab's own pointers-in-bytes, rows of the band only."""
    host = s.buf.numpy()
    p = s.planes["dst"]
    r0, r1 = band if band else (0, p.rows)
    for i in range(p.nimg):
        Y.Slab._rows(host, p, i)[r0:r1] = (src[i, r0:r1] * 2).view(np.uint8).reshape(r1 - r0, -1)


def poke(s, name, image, row, col, value=None, nbytes=None):
    """A stray store at element (row, col) of image `image` of plane `name`; value None: the bytes flipped."""
    p = s.planes[name]
    off = p.base + image * p.dist + row * p.pitch + col * p.item
    host = s.buf.numpy()
    n = p.item if nbytes is None else nbytes
    host[off:off + n] = (host[off:off + n] ^ 0xFF) if value is None else value
    return off


def test_layout_rules():
    s, _ = make()
    for p in s.planes.values():
        assert p.base >= Y.MARGIN and s.nbytes - (p.base + p.nimg * p.dist) >= Y.MARGIN
        assert (p.base - p.item) % 256 == 0 and p.pitch == (p.cols + p.pad) * p.item
        assert p.pad % 2 == 1 and p.pitch % 16 != 0
        assert p.dist > p.rows * p.pitch and (p.dist - p.rows * p.pitch) % 16 != 0
    assert s.planes["src"].pitch % 16 != 0 and s.planes["mask"].base % 2 == 1
    # dense: no row padding, the images of a batch keep their gap; tight: the images back to back as well
    d = Y.slab([Y.Plane("flow", shape=(3, 9, 13), dtype=np.float32, dense=True),
                Y.Plane("level", shape=(3, 9, 13), dtype=np.float32, dense=True, tight=True)], device="cpu")
    flow, level = d.planes["flow"], d.planes["level"]
    assert flow.pitch == level.pitch == 13 * 4 and flow.base % 256 == level.base % 256 == 4
    assert flow.dist > 9 * flow.pitch and (flow.dist - 9 * flow.pitch) % 16 != 0 and flow.dist % 4 == 0
    assert level.dist == 9 * level.pitch
    host = d.buf.numpy()
    off = flow.base + 9 * flow.pitch  # the first byte behind image 0 of the dense plane is a gap, and is watched
    host[off] ^= 0xFF
    with pytest.raises(AssertionError, match=r"gap behind image plane 'flow' image 0 row 9 col 0 "):
        Y.check(d, ["flow"], {})
    t = Y.slab([Y.Plane("a", shape=(4, 8), dtype=np.float32)], packed=True, device="cpu")
    assert t.planes["a"].base % 256 == 0 and t.pitch("a") == 32 and t.dist("a") == 128
    # the pattern is not constant and not periodic in 256 bytes
    pat = Y.sentinel(np.arange(1 << 17))
    assert len(set(pat[:256].tolist())) == 256 and not np.array_equal(pat[:256], pat[256:512])


def test_per_plane_packed_override():
    """The mixed layouts of the driver table: one block, the inputs placed one way and the outputs the other.  The check
    works on either kind of plane: a clean call passes, a store into the embedded plane's row padding is named, and so
    is one behind the last row of the packed plane."""
    rng = np.random.default_rng(8)
    src = rng.integers(0, 256, (2, 9, 13)).astype(np.uint8)
    for src_packed, dst_packed, block in ((True, False, False), (False, True, False), (True, False, True), (False, True, True)):
        s = Y.slab([Y.Plane("src", data=src, packed=src_packed), Y.Plane("dst", shape=(2, 9, 13), dtype=np.uint8, packed=dst_packed)],
                   packed=block, device="cpu")
        for p, packed in ((s.planes["src"], src_packed), (s.planes["dst"], dst_packed)):
            if packed:
                assert p.base % 256 == 0 and p.pitch == 13 and p.dist == 9 * 13
            else:
                assert p.base % 256 == 1 and p.pitch == 13 + p.pad and p.pad % 2 == 1 and p.dist > 9 * p.pitch
            assert p.base >= Y.MARGIN and s.nbytes - (p.base + p.nimg * p.dist) >= Y.MARGIN
        assert np.array_equal(s.read("src"), src)
        host = s.buf.numpy()
        d = s.planes["dst"]
        for i in range(2):
            Y.Slab._rows(host, d, i)[:] = 255 - src[i]
        Y.check(s, ["dst"], {"dst": 255 - src})
        if dst_packed:
            poke(s, "dst", 1, 9, 0)
            with pytest.raises(AssertionError, match=r"margin behind plane 'dst' image 1 row 9 col 0 "):
                Y.check(s, ["dst"], {"dst": 255 - src})
        else:
            poke(s, "dst", 0, 4, 13)
            with pytest.raises(AssertionError, match=r"row padding of plane 'dst' image 0 row 4 col 13 "):
                Y.check(s, ["dst"], {"dst": 255 - src})
    # None follows the block
    s = Y.slab([Y.Plane("a", shape=(4, 8), dtype=np.float32)], packed=True, device="cpu")
    assert s.planes["a"].base % 256 == 0


def test_clean_call_passes():
    s, src = make()
    good_call(s, src)
    Y.check(s, ["dst"], {"dst": src * 2})
    assert np.array_equal(s.read("dst").view(np.uint32), (src * 2).view(np.uint32))
    s, src = make(band=(3, 6))
    good_call(s, src, (3, 6))
    Y.check(s, ["dst"], {"dst": src * 2})


def test_nan_compares_by_bytes():
    s, src = make()
    src = src.copy()
    src[0, 1, 1] = np.nan
    good_call(s, src)
    Y.check(s, ["dst"], {"dst": src * 2})
    other = (src * 2).copy()
    other.view(np.uint32)[0, 1, 1] ^= 1  # another NaN payload
    with pytest.raises(AssertionError, match=r"output plane 'dst' image 0 row 1 col 1 "):
        Y.check(s, ["dst"], {"dst": other})


def test_wrong_value_is_named():
    s, src = make()
    good_call(s, src)
    exp = src * 2
    exp[1, 8, 12] += 1
    with pytest.raises(AssertionError, match=r"output plane 'dst' image 1 row 8 col 12 "):
        Y.check(s, ["dst"], {"dst": exp})


def test_store_past_row_end():
    s, src = make()
    good_call(s, src)
    poke(s, "dst", 0, 4, 13, value=0)
    with pytest.raises(AssertionError, match=r"row padding of plane 'dst' image 0 row 4 col 13 "):
        Y.check(s, ["dst"], {"dst": src * 2})


def test_store_into_excluded_band_row():
    s, src = make(band=(3, 6))
    good_call(s, src, (3, 6))
    poke(s, "dst", 1, 6, 2, value=0)
    with pytest.raises(AssertionError, match=r"row outside the band of plane 'dst' image 1 row 6 col 2 "):
        Y.check(s, ["dst"], {"dst": src * 2})


def test_store_into_image_gap():
    s, src = make()
    good_call(s, src)
    poke(s, "dst", 0, 9, 0, value=0)  # the row behind the last row of image 0
    with pytest.raises(AssertionError, match=r"gap behind image plane 'dst' image 0 row 9 col 0 "):
        Y.check(s, ["dst"], {"dst": src * 2})


def test_changed_input_byte():
    s, src = make()
    good_call(s, src)
    poke(s, "mask", 0, 2, 5)
    with pytest.raises(AssertionError, match=r"view of plane 'mask' image 0 row 2 col 5 "):
        Y.check(s, ["dst"], {"dst": src * 2})
    s, src = make()
    good_call(s, src)
    poke(s, "src", 1, 0, 14)  # an input's padding counts too
    with pytest.raises(AssertionError, match=r"row padding of plane 'src' image 1 row 0 col 14 "):
        Y.check(s, ["dst"], {"dst": src * 2})


def test_store_into_margins():
    s, src = make()
    good_call(s, src)
    poke(s, "src", 0, -1, 3, value=0)  # before the first plane
    with pytest.raises(AssertionError, match=r"margin before plane 'src' image 0 row -1 col 3 "):
        Y.check(s, ["dst"], {"dst": src * 2})
    s, src = make()
    good_call(s, src)
    poke(s, "dst", 1, 11, 1, value=0)  # behind the last image of the last plane
    with pytest.raises(AssertionError, match=r"margin behind plane 'dst' image 1 row 11 col 1 "):
        Y.check(s, ["dst"], {"dst": src * 2})


def test_stray_store_of_a_nearby_sentinel_value():
    """A stray store that writes the sentinel byte of the NEXT position (what a constant fill would hide)."""
    s, src = make()
    good_call(s, src)
    p = s.planes["dst"]
    off = p.base + 2 * p.pitch + 13 * p.item
    host = s.buf.numpy()
    assert host[off] != host[off + 1]
    host[off] = host[off + 1]
    with pytest.raises(AssertionError, match=r"row padding of plane 'dst' image 0 row 2 col 13 "):
        Y.check(s, ["dst"], {"dst": src * 2})
    # and one that copies the sentinel bytes found 256 bytes further on
    s, src = make()
    good_call(s, src)
    host = s.buf.numpy()
    off = s.planes["dst"].base - 512
    host[off:off + 16] = host[off + 256:off + 272]
    with pytest.raises(AssertionError, match=r"plane '(mask|dst)'"):
        Y.check(s, ["dst"], {"dst": src * 2})


def test_list_rows_past_count_are_not_asserted_but_owned():
    s = Y.slab([Y.Plane("locs", shape=(8, 2), dtype=np.int32, dense=True)], device="cpu")
    host = s.buf.numpy()
    p = s.planes["locs"]
    Y.Slab._rows(host, p, 0)[:3] = np.arange(6, dtype=np.int32).reshape(3, 2).view(np.uint8)
    Y.Slab._rows(host, p, 0)[5] = 0  # an unspecified entry between count and capacity
    Y.check(s, ["locs"], {"locs": np.arange(6, dtype=np.int32).reshape(3, 2)})
    poke(s, "locs", 0, 8, 0, value=0)  # entry `capacity`: not the call's to write
    with pytest.raises(AssertionError, match=r"margin behind plane 'locs' image 0 row 8 col 0 "):
        Y.check(s, ["locs"], {"locs": np.arange(6, dtype=np.int32).reshape(3, 2)})
