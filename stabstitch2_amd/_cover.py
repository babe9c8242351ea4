"""ctypes binding of libstabstitch_cover.so (the C ABI declared in include/stabstitch_cover.h): coverage bitmaps of stitched frames
and the largest rectangle every frame covers.

The loader, the launch path and the rules are `_hip`'s: no CPU fallback, contiguous device tensors only, launches on the current
stream of the device that owns the pointers (`_hip.dptr` / `_hip.stream` supply both)."""
import ctypes
import os

from . import _hip as H

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'libstabstitch_cover.so')
HEADER, API, PREFIX = 'stabstitch_cover.h', 'SSC_API', 'ssc_'
MAX_VIEWS = 3
MAX_FRAMES = 65535
MAX_WIDTH = 8192
ERR_ARG = H.ERR_ARG

c_fp, c_i, c_f, c_ll, c_st = H.c_fp, H.c_i, H.c_f, H.c_ll, H.c_st

# name -> (restype, argtypes); mirrors include/stabstitch_cover.h one to one
SIGNATURES = {
    'ssc_version': (c_i, []),
    'ssc_bitmap_words': (c_ll, [c_i, c_i]),
    'ssc_coverage': (c_i, [c_fp] * 3 + [c_i] * 7 + [c_f, c_i, c_st]),
    'ssc_rect_workspace_bytes': (c_ll, [c_i, c_i]),
    'ssc_covered_rect': (c_i, [c_fp, c_i, c_i, c_i, c_fp, c_ll, c_fp, c_st]),
}

_lib = None


def lib():
    """The loaded library (loads on first use; raises if it has not been built)."""
    global _lib
    if _lib is None:
        _lib = H.load(LIB_PATH, SIGNATURES)
    return _lib


def call(name, *args):
    """`_hip.launch` on this library.  An argument the library refuses is a ValueError; a failed launch is a `_hip.HipError`."""
    H.check_side(H.launch(lib, name, args), name)
