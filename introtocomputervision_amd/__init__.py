"""MI355X-native per-pixel CV kernel path of tanmaniac/IntroToComputerVision.

The product is ``libmicv.so`` (hand-written HIP for gfx950 behind the C ABI declared in
``include/mi_cv.h``).  This package is the thin Python host side used by the tests and
``bench.py``: a ctypes binding plus modules named after the reference's namespaces
(``lk``, ``pyr``, ``harris``, ``sift``, ``stereo``, ``hough``, ``warp``, ``ps0``, ``ps1``, ``ps3``, ``ps4``, ``ps5``, ``ps6``, ``ps7``).  There is no CPU fallback:
importing ``_capi`` fails loudly when the library has not been built.
"""
__version__ = "0.1.0"

__all__ = ["warp", "ps0", "ps1", "ps3", "ps4", "ps5", "ps6", "ps7"]


def __getattr__(name):
    # `introtocomputervision_amd.warp` / `.ps1` / `.ps5` after a plain `import introtocomputervision_amd`: loaded on first use, so that
    # importing the package (or `synth`, which needs no library) does not load libmicv.so
    if name in __all__:
        import importlib
        return importlib.import_module("." + name, __name__)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
