"""CPU-only checks of the entry point behind ThreeViewOnlineStitcher.push_many: bad arguments are refused with SS_ERR_ARG before any
device work (every pointer below is host memory or NULL, so a launch would fault instead)."""
import ctypes

from test_host_logic import built_lib  # noqa: F401  (fixture)

ERR_ARG = -1


def _ptr(buf):
    return ctypes.cast(buf, ctypes.c_void_p)


def test_cost_volume_chain_frames_refuses_bad_arguments(built_lib):
    L = built_lib
    x, out = (ctypes.c_float * 4096)(), (ctypes.c_float * 4096)()
    good = dict(x=_ptr(x), out=_ptr(out), views=3, k=8, h=45, w=60, c=128, r=3, out_cs=52)

    def call(**kw):
        a = dict(good, **kw)
        return L.ss_cost_volume_chain_frames(a['x'], a['out'], a['views'], a['k'], a['h'], a['w'], a['c'], a['r'], a['out_cs'], None)

    assert call(x=None) == ERR_ARG and call(out=None) == ERR_ARG
    assert call(views=1) == ERR_ARG and call(views=0) == ERR_ARG and call(views=-2) == ERR_ARG
    assert call(k=0) == ERR_ARG and call(k=-1) == ERR_ARG and call(k=33) == ERR_ARG
    assert call(h=0) == ERR_ARG and call(w=0) == ERR_ARG and call(c=0) == ERR_ARG
    assert call(c=126) == ERR_ARG and call(c=130) == ERR_ARG                         # c % 4
    assert call(out_cs=48) == ERR_ARG and call(r=5, out_cs=120) == ERR_ARG           # out_cs < (2r+1)^2
    assert call(r=4, out_cs=84) == ERR_ARG and call(r=0, out_cs=4) == ERR_ARG        # radii without a kernel
    # grid limits: more tiles x volumes than one launch addresses, more images than 32-bit indices, an image past 2^31 floats
    assert call(views=4096, k=32, h=1024, w=512, c=4) == ERR_ARG
    assert call(views=1 << 20, k=32, h=1, w=1) == ERR_ARG
    assert call(views=2, k=1, h=1 << 14, w=1 << 14, c=8) == ERR_ARG
    assert all(v == 0.0 for v in out)                                                # nothing was written


def test_cost_volume_chain_frames_is_in_the_ctypes_table():
    from stabstitch2_amd import _hip
    assert 'ss_cost_volume_chain_frames' in _hip.SIGNATURES
