"""ctypes binding of libstabstitch_mbwarp.so (the C ABI declared in include/stabstitch_mbwarp.h): the direct warp of MULTIBAND fusion,
from the caller's frames to the planes the seam and the blend read, with optional exposure gains.

The loader, the launch path and the rules are `_hip`'s: no CPU fallback, contiguous device tensors only, launches on the current
stream of the device that owns the pointers (`_hip.dptr` / `_hip.stream` supply both)."""
import ctypes
import os

from . import _hip as H

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'libstabstitch_mbwarp.so')
HEADER, API, PREFIX = 'stabstitch_mbwarp.h', 'SSW_API', 'ssw_'
MAX_VIEWS = 3
MAX_ITEMS = 65535
ERR_ARG = H.ERR_ARG

c_fp, c_i, c_st = H.c_fp, H.c_i, H.c_st
c_pp = ctypes.c_void_p      # a host array of device pointers (`_hip.ptr_array`)

# name -> (restype, argtypes); mirrors include/stabstitch_mbwarp.h one to one
SIGNATURES = {
    'ssw_version': (c_i, []),
    'ssw_multiband_warp': (c_i, [c_pp] + [c_fp] * 4 + [c_i] * 7 + [c_st]),
    'ssw_multiband_warp_u8': (c_i, [c_pp] + [c_fp] * 4 + [c_i] * 7 + [c_st]),
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
