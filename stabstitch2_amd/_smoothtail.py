"""ctypes binding of libstabstitch_smoothtail.so (the C ABI declared in include/stabstitch_smoothtail.h): SmoothNet's Conv3d stack and
decoder for a stitched clip, restricted to the window frames the stitch reads.

The loader, the launch path and the rules are `_hip`'s: no CPU fallback, contiguous device tensors only, launches on the current
stream of the device that owns the pointers (`_hip.dptr` / `_hip.stream` supply both)."""
import os

from . import _hip as H

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'libstabstitch_smoothtail.so')
HEADER, API, PREFIX = 'stabstitch_smoothtail.h', 'SST_API', 'sst_'
MAX_WINDOWS = 2048
K_TILES = 180
ERR_ARG = H.ERR_ARG

c_fp, c_i, c_ll, c_st = H.c_fp, H.c_i, H.c_ll, H.c_st

# name -> (restype, argtypes); mirrors include/stabstitch_smoothtail.h one to one
SIGNATURES = {
    'sst_version': (c_i, []),
    'sst_compact_frames': (c_ll, [c_i, c_i]),
    'sst_conv3d_layer': (c_i, [c_fp, c_fp, c_fp, c_fp, c_fp, c_ll, c_i, c_i, c_i, c_i, c_st]),
    'sst_decode_scatter': (c_i, [c_fp, c_fp, c_fp, c_fp, c_i, c_i, c_st]),
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
