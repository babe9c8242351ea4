"""ctypes binding of libstabstitch_surfaces.so (the C ABI declared in include/stabstitch_surfaces.h): decoded NV12 surfaces, each with
its own planes and pitch, to packed BGR frames -- all surfaces of a call in one launch.

A library of its own next to libstabstitch_hip.so, libstabstitch_blend.so, libstabstitch_seam.so and libstabstitch_mbwarp.so, with
the same rules: no CPU fallback, launches on the current stream of the device that owns the pointers (`_hip.stream` supplies it)."""
import ctypes
import os

import torch

from . import _hip as H

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'libstabstitch_surfaces.so')
MAX_SURFACES = 96
ERR_ARG = -1

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
