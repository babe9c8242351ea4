"""ctypes binding of libstabstitch_mbwarp.so (the C ABI declared in include/stabstitch_mbwarp.h): the direct warp of MULTIBAND fusion,
from the caller's frames to the planes the seam and the blend read, with optional exposure gains.

A library of its own next to libstabstitch_hip.so, libstabstitch_blend.so and libstabstitch_seam.so, with the same rules: no CPU
fallback, contiguous device tensors only, launches on the current stream of the device that owns the pointers (`_hip.dptr` /
`_hip.stream` supply both)."""
import ctypes
import os

import torch

from . import _hip as H

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'libstabstitch_mbwarp.so')
MAX_VIEWS = 3
MAX_ITEMS = 65535
ERR_ARG = -1

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
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                'stabstitch2_amd: %s not found. Build it with `python -c "import __graft_entry__ as g; g.build()"` '
                'or stabstitch2_amd/csrc/build.sh (hipcc --offload-arch=gfx950). There is no CPU fallback.' % LIB_PATH)
        handle = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


def call(name, *args):
    """Launch on the GPU that owns the pointer arguments, on that device's current stream (as `_hip.call`).  An argument the library
    refuses is a ValueError; a failed launch is a `_hip.HipError`."""
    dev = None
    for a in args:
        d = getattr(a, 'dev', None)
        if d is not None:
            if dev is not None and d != dev:
                raise H.HipError('%s: tensors of one launch live on different GPUs (cuda:%d and cuda:%d)' % (name, dev, d))
            dev = d
    if dev is None:
        raise H.HipError('%s needs device tensors; there is no CPU path' % name)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    args = tuple(st if a is H._STREAM else a for a in args)
    with torch.cuda.device(dev):
        code = getattr(lib(), name)(*args)
    if code == ERR_ARG:
        raise ValueError('%s refused its arguments' % name)
    if code != 0:
        err = H.HipError('%s failed: launch error (%d)' % (name, code))
        err.code = code
        raise err
