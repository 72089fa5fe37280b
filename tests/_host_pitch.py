"""Host images with a padded pitch, shared by the tests of the `_host` entry points."""
import numpy as np


def strided_host(a, pad, sentinel=0xA5):
    """(block, view): `a` copied into rows that are `pad` elements wider, the padding filled with `sentinel` bytes."""
    block = np.full((a.shape[0], (a.shape[1] + pad) * a.itemsize), sentinel, np.uint8)
    view = block.view(a.dtype)[:, :a.shape[1]]
    view[...] = a
    return block, view
