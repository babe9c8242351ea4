"""ctypes binding of libstabstitch_blend.so (the C ABI declared in include/stabstitch_blend.h): MULTIBAND fusion.

The loader, the launch path and the rules are `_hip`'s: no CPU fallback, contiguous device tensors only, launches on the current
stream of the device that owns the pointers (`_hip.dptr` / `_hip.stream` supply both)."""
import os

from . import _hip as H

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'libstabstitch_blend.so')
HEADER, API, PREFIX = 'stabstitch_blend.h', 'SSB_API', 'ssb_'
MAX_VIEWS = 3
MAX_BANDS = 6
ERR_ARG = H.ERR_ARG

c_fp, c_i, c_ll, c_st = H.c_fp, H.c_i, H.c_ll, H.c_st

# name -> (restype, argtypes); mirrors include/stabstitch_blend.h one to one
SIGNATURES = {
    'ssb_version': (c_i, []),
    'ssb_multiband_workspace_floats': (c_ll, [c_i] * 5),
    'ssb_multiband_blend': (c_i, [c_fp, c_fp, c_fp, c_ll] + [c_i] * 5 + [c_st]),
    'ssb_multiband_blend_u8': (c_i, [c_fp, c_fp, c_fp, c_ll] + [c_i] * 5 + [c_st]),
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
