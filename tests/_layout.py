"""Layout harness: image arguments embedded in one sentinel-filled block, and the check that an entry point
wrote its output views and nothing else.  torch and numpy only (the table test adds _capi); no oracle.

A `Slab` is ONE allocation of bytes.  Every byte starts as sentinel(offset), a pattern that depends on the position, so
that a stray store of zeros, NaN, a constant or a copy of a neighbouring row cannot reproduce it.  Each `Plane` is
placed in it
  - with a margin of MARGIN bytes (64 KiB) before the first and after the last plane and GUARD bytes between planes,
  - at ONE ELEMENT past a 256-byte boundary (f32: 4-byte but not 16-byte aligned; u8: an odd address),
  - with a row pitch of cols + pad elements, pad odd: 3, or the next odd number that keeps the pitch off a multiple
    of 16 bytes (13 f32 columns: pad 5),
  - images of a batch rows * pitch + gap bytes apart, the gap two rows and three elements: no multiple of 16 bytes.
Two departures, each for planes the header wants that way: `dense` drops the row padding only (pitch = cols elements;
the base offset, the margins and the gap between the images of a batch stay), `tight` drops the gap between images.
`packed=True` gives the layout the Python wrappers use instead (256-byte aligned, dense rows, dense images) inside the
same kind of block, so the same check applies to both calls of the table test.  A plane's own `packed` (True / False)
overrides the block's: the mixed layouts of the driver table place the inputs one way and the outputs the other in
ONE block, so that a kernel that keeps an alignment flag per plane meets an aligned source with an unaligned
destination and the reverse.

check(slab, outputs, expected) compares bytes as uint8 (NaN is not special) and names plane, image, row and column
of the first byte that is wrong."""
import numpy as np
import torch

MARGIN = 64 * 1024
GUARD = 4096


def sentinel(offsets):
    o = np.asarray(offsets, dtype=np.int64)
    return ((0xA5 ^ o ^ (o >> 8) ^ (o >> 16)) & 0xFF).astype(np.uint8)


class Plane:
    """One image argument: `data` ([rows, cols] or [nimg, rows, cols]; its bytes are the initial content) or
    shape = (rows, cols) / (nimg, rows, cols) + dtype for an output that starts as sentinel.  cols counts ELEMENTS
    (interleaved channels included).  band = (r0, r1): an output of which only rows [r0, r1) may be written.
    dense: the header wants this plane without row padding (pad = 0); tight: the header wants the images of the batch
    back to back (no gap).  Base offset and margins stay either way.  packed: None = as the block, True / False = this
    plane packed / embedded whatever the block is."""

    def __init__(self, name, data=None, shape=None, dtype=None, pad=3, band=None, dense=False, tight=False, packed=None):
        if data is not None:
            data = np.ascontiguousarray(data)
            shape, dtype = data.shape, data.dtype
        self.name, self.data, self.dtype = name, data, np.dtype(dtype)
        self.batched = len(shape) == 3
        self.nimg, self.rows, self.cols = (shape if self.batched else (1,) + tuple(shape))
        while not dense and (self.cols + pad) * self.dtype.itemsize % 16 == 0:
            pad += 2  # the smallest odd pad from `pad` up that keeps the pitch off a multiple of 16 bytes
        self.pad, self.band, self.dense, self.tight, self.packed = (0 if dense else pad), band, dense, tight, packed
        assert dense or pad % 2 == 1, "pad must be odd"
        # filled in by Slab
        self.base = self.pitch = self.dist = None

    @property
    def item(self):
        return self.dtype.itemsize


class Slab:
    def __init__(self, planes, packed=False, device="cuda"):
        self.planes = {p.name: p for p in planes}
        assert len(self.planes) == len(planes), "plane names must be unique"
        self.packed = packed
        off = MARGIN
        for p in planes:
            off = -(-off // 256) * 256
            if packed if p.packed is None else p.packed:
                p.base, p.pitch = off, p.cols * p.item
                p.dist = p.rows * p.pitch
            else:
                p.base = off + p.item
                p.pitch = (p.cols + p.pad) * p.item
                p.dist = p.rows * p.pitch if p.tight else p.rows * p.pitch + 2 * p.pitch + 3 * p.item
                assert p.tight or (p.dist - p.rows * p.pitch) % 16 != 0
                assert p.dense or p.item < 4 or p.pitch % 16 != 0, (p.name, p.pitch)
            off = p.base + p.nimg * p.dist + GUARD
        self.nbytes = off - GUARD + MARGIN
        host = sentinel(np.arange(self.nbytes))
        for p in planes:
            if p.data is not None:
                src = p.data.reshape(p.nimg, p.rows, p.cols).view(np.uint8)
                for i in range(p.nimg):
                    self._rows(host, p, i)[:, :] = src[i]
        self.orig = host
        self.buf = torch.from_numpy(host.copy()).to(device)
        if self.buf.is_cuda:
            assert self.buf.data_ptr() % 256 == 0

    # ---- geometry
    @staticmethod
    def _rows(host, p, i):
        """[rows, cols * item] uint8 view of image i of plane p in the host copy `host`."""
        start = p.base + i * p.dist
        a = np.lib.stride_tricks.as_strided(host[start:], shape=(p.rows, p.cols * p.item), strides=(p.pitch, 1))
        return a

    def ptr(self, name, image=0, row=0):
        p = self.planes[name]
        return self.buf.data_ptr() + p.base + image * p.dist + row * p.pitch

    def pitch(self, name):
        return self.planes[name].pitch

    def dist(self, name):
        return self.planes[name].dist

    def snapshot(self):
        return self.buf.cpu().numpy()

    def read(self, name, host=None):
        """The view of plane `name` as an array of its dtype, [rows, cols] or [nimg, rows, cols]."""
        p = self.planes[name]
        host = self.snapshot() if host is None else host
        a = np.stack([np.ascontiguousarray(self._rows(host, p, i)) for i in range(p.nimg)])
        a = a.view(p.dtype).reshape(p.nimg, p.rows, p.cols)
        return a if p.batched else a[0]

    def where(self, off):
        """(text, plane, image, row, col) of byte offset `off`: row / col in elements of the nearest plane; col >= cols
        is row padding, image >= nimg or row >= rows lies behind the plane, negative rows before it."""
        planes = list(self.planes.values())
        p = planes[0]
        for q in planes:
            if q.base <= off:
                p = q
        rel = off - p.base
        if rel < 0:
            row, col = rel // p.pitch, (rel % p.pitch) // p.item  # floor: row -1 is the pitch just before the plane
            img, kind = 0, "margin before"
        else:
            img = min(rel // p.dist, p.nimg - 1)
            r = rel - img * p.dist
            row, col = r // p.pitch, (r % p.pitch) // p.item
            if row >= p.rows:
                kind = "gap behind image" if img < p.nimg - 1 else "margin behind"
            elif col >= p.cols:
                kind = "row padding of"
            elif p.band and not p.band[0] <= row < p.band[1]:
                kind = "row outside the band of"
            else:
                kind = "view of"
        return f"{kind} plane {p.name!r} image {img} row {row} col {col} (byte {off})", p.name, img, row, col


def slab(planes, packed=False, device="cuda"):
    return Slab(planes, packed=packed, device=device)


def _as_bytes(a, p):
    a = np.ascontiguousarray(np.asarray(a, dtype=p.dtype))
    assert a.ndim == (3 if p.batched else 2), (p.name, a.shape)
    a = a if p.batched else a[None]
    return a.view(np.uint8).reshape(a.shape[0], a.shape[1], a.shape[2] * p.item)


def check(s, outputs, expected, label=""):
    """outputs: names of the planes the call may write.  expected[name]: the bytes of that view, an array of the
    plane's dtype and shape; with FEWER rows than the plane only those first rows are asserted (a list up to its
    returned count: the entries between count and capacity belong to the call but are not specified).
    Asserts (1) every byte outside the output views -- row padding, gaps, margins, rows outside a band, every input view
    and its padding -- is what it was before the call, (2) every output view equals expected."""
    got = s.snapshot()
    writable = np.zeros(s.nbytes, bool)
    for name in outputs:
        p = s.planes[name]
        r0, r1 = p.band if p.band else (0, p.rows)
        for i in range(p.nimg):
            Slab._rows(writable, p, i)[r0:r1, :] = True
    bad = np.flatnonzero((got != s.orig) & ~writable)
    if bad.size:
        off = int(bad[0])
        raise AssertionError(f"{label}: {bad.size} byte(s) outside the outputs changed, first in the {s.where(off)[0]}: "
                             f"0x{s.orig[off]:02x} -> 0x{got[off]:02x}")
    for name in outputs:
        if name not in expected:
            continue
        p = s.planes[name]
        exp = _as_bytes(expected[name], p)
        n = exp.shape[1]
        assert exp.shape[0] == p.nimg and n <= p.rows and exp.shape[2] == p.cols * p.item, (name, exp.shape)
        r0, r1 = p.band if p.band else (0, p.rows)
        for i in range(p.nimg):
            g = Slab._rows(got, p, i)[:n]
            ne = (g != exp[i])
            ne[:max(r0, 0)] = False
            ne[r1:] = False
            if ne.any():
                r, c = np.argwhere(ne)[0]
                ge = np.ascontiguousarray(g[r]).view(p.dtype)[c // p.item]
                ee = np.ascontiguousarray(exp[i, r]).view(p.dtype)[c // p.item]
                raise AssertionError(f"{label}: output plane {name!r} image {i} row {r} col {c // p.item} (byte {c % p.item}): "
                                     f"got {ge!r}, expected {ee!r}; {int(ne.sum())} byte(s) differ")
    return got
