"""ctypes binding of libstabstitch_seam.so (the C ABI declared in include/stabstitch_seam.h): the dynamic-programming seam of MULTIBAND
fusion.

The loader, the launch path and the rules are `_hip`'s: no CPU fallback, contiguous device tensors only, launches on the current
stream of the device that owns the pointers (`_hip.dptr` / `_hip.stream` supply both)."""
import os

from . import _hip as H

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'libstabstitch_seam.so')
HEADER, API, PREFIX = 'stabstitch_seam.h', 'SSM_API', 'ssm_'
MAX_VIEWS = 3
CELLS = (1, 2, 4, 8, 16)
MU_MAX = 65535
PRIOR_MAX = 255.0
STATE_HEADER = 16
LDS_BYTES = 163840
TILE_W = 256
ERR_ARG = H.ERR_ARG

c_fp, c_i, c_f, c_ll, c_st = H.c_fp, H.c_i, H.c_f, H.c_ll, H.c_st

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
        _lib = H.load(LIB_PATH, SIGNATURES)
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
    """`_hip.launch` on this library.  An argument the library refuses is a ValueError; a failed launch is a `_hip.HipError`."""
    H.check_side(H.launch(lib, name, args), name)
