"""ctypes binding of libstabstitch_seam.so (the C ABI declared in include/stabstitch_seam.h): the dynamic-programming seam of MULTIBAND
fusion.

A library of its own next to libstabstitch_hip.so and libstabstitch_blend.so, with the same rules: no CPU fallback, contiguous device
tensors only, launches on the current stream of the device that owns the pointers (`_hip.dptr` / `_hip.stream` supply both)."""
import ctypes
import os

import torch

from . import _hip as H

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'libstabstitch_seam.so')
MAX_VIEWS = 3
CELLS = (1, 2, 4, 8, 16)
MU_MAX = 65535
PRIOR_MAX = 255.0
STATE_HEADER = 16
LDS_BYTES = 163840
TILE_W = 256
ERR_ARG = -1

c_fp, c_i, c_ll, c_st = H.c_fp, H.c_i, H.c_ll, H.c_st
c_f = ctypes.c_float

# name -> (restype, argtypes); mirrors include/stabstitch_seam.h one to one
SIGNATURES = {
    'ssm_version': (c_i, []),
    'ssm_seam_workspace_bytes': (c_ll, [c_i] * 5),
    'ssm_multiband_seam': (c_i, [c_fp] + [c_i] * 6 + [c_f, c_fp, c_ll, c_fp, c_ll, c_st]),
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


def grid(hc, wc, cell):
    """-> (hq, wq, wq4): the cell grid of a canvas and the padded row length of the cost planes."""
    hq, wq = -(-int(hc) // cell), -(-int(wc) // cell)
    return hq, wq, (wq + 3) & ~3


def lds_bytes(hc, wc, cell):
    """LDS of the dynamic program's workgroup on this grid (it must not exceed LDS_BYTES)."""
    hq, _, wq4 = grid(hc, wc, cell)
    return 4 * (16 + 2 * wq4 + 3 * hq) + hq * wq4 // 4


def layout(frames, views, hc, wc, cell):
    """The workspace as the header lays it out: {'cost', 'ext', 'seams', 'meta', 'rowf'} -> (offset in ints, shape), and 'ints' -> the
    total."""
    hq, _, wq4 = grid(hc, wc, cell)
    npairs = views * (views - 1) // 2
    gx = -(-int(wc) // TILE_W)
    nblk = gx * -(-int(hc) // max(4, cell))
    out, off = {}, 0
    for name, shape in (('cost', (frames, npairs, 3, hq, wq4)), ('ext', (frames, nblk, views, 2)), ('seams', (frames, views - 1, hq)),
                        ('meta', (frames, 8)), ('rowf', (frames, npairs, hq, gx))):
        out[name] = (off, shape)
        n = 1
        for s in shape:
            n *= s
        off += n
    out['ints'] = off
    return out


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
