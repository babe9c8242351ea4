"""ctypes binding of libstabstitch_resample.so (the C ABI declared in include/stabstitch_resample.h): a rectangle of stitched frames
resampled with a prefilter to a fixed size, as fp32 planes, BGR bytes or NV12.

The loader, the launch path and the rules are `_hip`'s: no CPU fallback, device tensors only, launches on the current stream of the
device that owns the pointers (`_hip.dptr` / `_hip.stream` supply both)."""
import ctypes
import os

from . import _hip as H

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'libstabstitch_resample.so')
HEADER, API, PREFIX = 'stabstitch_resample.h', 'SSR_API', 'ssr_'
MAX_FRAMES = 65535
ASPECTS = {'stretch': 0, 'fill': 1}
ERR_ARG = H.ERR_ARG

c_fp, c_i, c_ll, c_st = H.c_fp, H.c_i, H.c_ll, H.c_st
_tail = [c_i] * 6 + [c_fp] + [c_i] * 4 + [c_st]        # n, Hc, Wc, Hout, Wout, aspect, rect_dev, y0, x0, h, w, stream

# name -> (restype, argtypes); mirrors include/stabstitch_resample.h one to one
SIGNATURES = {
    'ssr_version': (c_i, []),
    'ssr_source_window': (c_i, [ctypes.POINTER(c_i), c_i, c_i, c_i, c_i, c_i, ctypes.POINTER(ctypes.c_double)]),
    'ssr_resample_f32': (c_i, [c_fp, c_fp] + _tail),
    'ssr_resample_u8': (c_i, [c_fp, c_fp, c_ll] + _tail),
    'ssr_resample_u8_nv12': (c_i, [c_fp, c_fp, c_fp, c_i, c_ll] + _tail),
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
