"""CPU-only checks of the entry points behind the streaming stitchers' direct LINEAR render (ss_render_linear_frames(_u8): LINEAR
fusion of frames that each have their own canvas): the symbols exist on all three sides of the ABI, the workspace agrees with the
clip entry's where the two describe the same thing, and bad arguments are refused with SS_ERR_ARG before any device work (every
pointer below is host memory or NULL, so a launch would fault instead)."""
import ctypes
import os
import re

import pytest

from test_host_logic import built_lib  # noqa: F401  (fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
NAMES = ('ss_linear_frames_workspace_floats', 'ss_render_linear_frames', 'ss_render_linear_frames_u8')


def _ints(v):
    return (ctypes.c_int * len(v))(*v)


def test_linear_frames_symbols_exist_in_library_header_and_table(built_lib):
    from stabstitch2_amd import _hip
    hdr = open(os.path.join(ROOT, 'include', 'stabstitch_hip.h')).read()
    declared = set(re.findall(r'\bSS_API[^;]*?\b(ss_[a-z0-9_]+)\s*\(', hdr))
    for name in NAMES:
        assert hasattr(built_lib, name), name
        assert name in declared, name
        assert name in _hip.SIGNATURES, name


@pytest.mark.parametrize('views', [2, 3])
def test_linear_frames_workspace_equals_the_clip_workspace(built_lib, views):
    L = built_lib
    for hc, wc in ((740, 1882), (11, 11)):
        one = L.ss_linear_frames_workspace_floats(1, views, _ints([hc]), _ints([wc]))
        assert one > 0 and one == L.ss_linear_clip_workspace_floats(1, views, hc, wc), (hc, wc)
        for n in (2, 5, 32):
            assert L.ss_linear_frames_workspace_floats(n, views, _ints([hc] * n), _ints([wc] * n)) == \
                L.ss_linear_clip_workspace_floats(n, views, hc, wc), (n, hc, wc)
    # different sizes: the sum of the frames' own needs (each clip figure carries the one float of alignment slack)
    sizes = [(740, 1882), (11, 11), (97, 65)]
    rag = L.ss_linear_frames_workspace_floats(3, views, _ints([s[0] for s in sizes]), _ints([s[1] for s in sizes]))
    assert rag == sum(L.ss_linear_clip_workspace_floats(1, views, hc, wc) - 1 for hc, wc in sizes) + 1
    # what the render refuses needs no workspace
    assert L.ss_linear_frames_workspace_floats(0, views, _ints([11]), _ints([11])) == 0
    assert L.ss_linear_frames_workspace_floats(33, views, _ints([11] * 33), _ints([11] * 33)) == 0
    assert L.ss_linear_frames_workspace_floats(1, 4, _ints([11]), _ints([11])) == 0
    assert L.ss_linear_frames_workspace_floats(1, views, None, _ints([11])) == 0
    assert L.ss_linear_frames_workspace_floats(1, views, _ints([10]), _ints([11])) == 0
    assert L.ss_linear_frames_workspace_floats(1, views, _ints([11]), _ints([65536])) == 0


@pytest.mark.parametrize('u8', [False, True])
def test_linear_frames_refuses_bad_arguments(built_lib, u8):
    L = built_lib
    fn = L.ss_render_linear_frames_u8 if u8 else L.ss_render_linear_frames
    n = 33
    img = (ctypes.c_float * 64)()
    src, T, ws = (ctypes.c_float * 64)(), (ctypes.c_float * 64)(), (ctypes.c_double * 64)()      # (ws: 8-byte aligned)
    canvas = (ctypes.c_float * 64)()
    addr = lambda b: ctypes.cast(b, ctypes.c_void_p)
    views_base = (ctypes.c_void_p * 3)(*[addr(img).value] * 3)
    outs = (ctypes.c_void_p * n)(*[addr(canvas).value] * n)
    good = dict(views_base=views_base, src=addr(src), T=addr(T), out=outs, frames=2, views=2, h=48, w=64,
                hc=_ints([40] * n), wc=_ints([50] * n), mode=0, ws=addr(ws))

    def call(**kw):
        a = dict(good, **kw)
        return fn(a['views_base'], a['src'], a['T'], a['out'], a['frames'], a['views'], a['h'], a['w'], a['hc'], a['wc'], a['mode'],
                  a['ws'], None)

    for k in ('views_base', 'src', 'T', 'out', 'hc', 'wc', 'ws'):
        assert call(**{k: None}) == ERR_ARG, k
    assert call(views_base=(ctypes.c_void_p * 3)(addr(img).value, None, None)) == ERR_ARG          # a null view
    assert call(out=(ctypes.c_void_p * 2)(addr(canvas).value, None)) == ERR_ARG                    # a null frame
    assert call(frames=0) == ERR_ARG and call(frames=-1) == ERR_ARG and call(frames=33) == ERR_ARG
    assert call(views=4) == ERR_ARG and call(views=1) == ERR_ARG
    assert call(hc=_ints([40, 10])) == ERR_ARG and call(wc=_ints([10, 50])) == ERR_ARG
    assert call(wc=_ints([50, 65536])) == ERR_ARG and call(hc=_ints([65536, 40])) == ERR_ARG
    assert call(mode=2) == ERR_ARG and call(mode=-1) == ERR_ARG
    assert call(h=1) == ERR_ARG and call(w=0) == ERR_ARG
    assert all(v == 0.0 for v in canvas) and all(v == 0.0 for v in ws)                             # nothing was written
