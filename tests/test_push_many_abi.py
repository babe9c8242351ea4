"""CPU-only checks of the two entry points behind OnlineStitcher.push_many: bad arguments are refused with SS_ERR_ARG before any
device work (every pointer below is host memory or NULL, so a launch would fault instead)."""
import ctypes

import pytest

from test_host_logic import built_lib  # noqa: F401  (fixture)

ERR_ARG = -1


def _ptr(buf):
    return ctypes.cast(buf, ctypes.c_void_p)


def test_window_advance_refuses_bad_arguments(built_lib):
    L = built_lib
    ring, work, src = (ctypes.c_float * 4096)(), (ctypes.c_float * 8192)(), (ctypes.c_float * 4096)()
    offs = (ctypes.c_longlong * 4)(0, 126, 252, 378)
    state, ssrc = (ctypes.c_float * 512)(), (ctypes.c_float * 512)()

    def call(ring=_ptr(ring), work=_ptr(work), src=_ptr(src), off=_ptr(offs), rings=4, window=7, elems=126, k=8, state=None,
             state_src=None, blocks=0, block=0, stride=0, src_stride=0):
        return L.ss_window_advance(ring, work, src, off, rings, window, elems, k, state, state_src, blocks, block, stride,
                                   src_stride, None)

    assert call(ring=None) == ERR_ARG
    assert call(work=None) == ERR_ARG
    assert call(src=None) == ERR_ARG
    assert call(off=None) == ERR_ARG
    assert call(rings=0) == ERR_ARG and call(rings=9) == ERR_ARG
    assert call(window=1) == ERR_ARG
    assert call(elems=0) == ERR_ARG
    assert call(k=0) == ERR_ARG and call(k=33) == ERR_ARG
    assert call(window=17, elems=126) == ERR_ARG                                   # window * elems > 2048
    assert call(work=_ptr(ring)) == ERR_ARG                                        # work overlaps the rings
    assert call(off=_ptr((ctypes.c_longlong * 4)(0, -1, 0, 0))) == ERR_ARG         # negative source offset
    # state blocks: missing pointers, bad sizes, a destination block overlapping a source block
    assert call(blocks=2, block=126, stride=252, src_stride=126) == ERR_ARG
    assert call(state=_ptr(state), state_src=_ptr(ssrc), blocks=9, block=16, stride=16, src_stride=16) == ERR_ARG
    assert call(state=_ptr(state), state_src=_ptr(ssrc), blocks=2, block=0, stride=16, src_stride=16) == ERR_ARG
    assert call(state=_ptr(state), state_src=_ptr(ssrc), blocks=2, block=126, stride=100, src_stride=126) == ERR_ARG
    assert call(state=_ptr(state), state_src=_ptr(state), blocks=1, block=126) == ERR_ARG
    s1 = ctypes.c_void_p(ctypes.addressof(state) + 4 * 126)                        # state + block: dst block 1 == src block 0
    assert call(state=_ptr(state), state_src=s1, blocks=2, block=126, stride=126, src_stride=126) == ERR_ARG


def test_canvas_watch_frames_refuses_bad_arguments(built_lib):
    L = built_lib
    src, wi, wf = (ctypes.c_float * 2048)(), (ctypes.c_int * 4)(), (ctypes.c_float * 4)()
    good = dict(src=_ptr(src), frames=8, views=2, guard=0.02, wi=_ptr(wi), wf=_ptr(wf))

    def call(**kw):
        a = dict(good, **kw)
        return L.ss_canvas_watch_frames(a['src'], a['frames'], a['views'], a['guard'], a['wi'], a['wf'], None)

    assert call(src=None) == ERR_ARG
    assert call(wi=None) == ERR_ARG and call(wf=None) == ERR_ARG
    assert call(frames=0) == ERR_ARG and call(frames=-3) == ERR_ARG
    assert call(views=0) == ERR_ARG
    assert call(guard=-0.5) == ERR_ARG and call(guard=float('nan')) == ERR_ARG
    assert list(wi) == [0, 0, 0, 0]                                                # nothing was written


@pytest.mark.parametrize('name', ['ss_window_advance', 'ss_canvas_watch_frames'])
def test_new_entries_are_in_the_ctypes_table(name):
    from stabstitch2_amd import _hip
    assert name in _hip.SIGNATURES
