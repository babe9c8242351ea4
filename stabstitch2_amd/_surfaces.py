"""ctypes binding of libstabstitch_surfaces.so (the C ABI declared in include/stabstitch_surfaces.h): decoded NV12 surfaces, each with
its own planes and pitch, to packed BGR frames -- all surfaces of a call in one launch.

The loader, the launch path and the rules are `_hip`'s: no CPU fallback, launches on the current stream of the device that owns the
pointers (`_hip.stream` supplies it)."""
import ctypes
import os

from . import _hip as H

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'libstabstitch_surfaces.so')
HEADER, API, PREFIX = 'stabstitch_surfaces.h', 'SSF_API', 'ssf_'
MAX_SURFACES = 96
ERR_ARG = H.ERR_ARG

c_fp, c_i, c_ll, c_st = H.c_fp, H.c_i, H.c_ll, H.c_st
c_pp = ctypes.c_void_p      # a host array (of device pointers, or of ints)

# name -> (restype, argtypes); mirrors include/stabstitch_surfaces.h one to one
SIGNATURES = {
    'ssf_version': (c_i, []),
    'ssf_nv12_to_bgr': (c_i, [c_pp, c_pp, c_pp, c_i, c_i, c_i, c_fp, c_ll, c_st]),
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
