"""The NV12 surface converter and the batched NV12 routes without a GPU: the fifth library's header, exports and ctypes table, the
kernels the built library carries, what it refuses, and the refusals of the Python layers that come before anything runs.  The
kernels and the routes themselves: tests/test_gpu_surfaces.py.
    python -m pytest tests/test_surfaces_abi.py"""
import ctypes
import os
import re
import sys

import pytest
import torch

import abi_surface as A
import sweep_inputs as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
KERNELS = ['sf_convert_kernel<0>', 'sf_convert_kernel<1>']


@pytest.fixture(scope='module')
def surf_lib():
    from stabstitch2_amd import _surfaces
    return A.built(_surfaces)


def test_header_exports_and_ctypes_table_agree(surf_lib):
    from stabstitch2_amd import _surfaces
    declared, defines = A.check(_surfaces)
    assert declared == ['ssf_nv12_to_bgr', 'ssf_version']
    assert defines['SSF_ERR_ARG'] == _surfaces.ERR_ARG == ERR_ARG and defines['SSF_MAX_SURFACES'] == _surfaces.MAX_SURFACES == 96
    assert surf_lib.ssf_version() == 1
    # (that the libraries before it do not know of it: test_native_binding.py, for every library)
    # the kernels use nv12.h's statement and do not restate its constants
    src = open(os.path.join(ROOT, 'stabstitch2_amd', 'csrc', 'surfaces.hip')).read()
    assert '#include "nv12.h"' in src and 'nv12_to_bgr(' in src
    for constant in ('1220542', '2116026', '409993', '852492', '1673527'):
        assert constant not in src, constant


def test_code_objects_hold_the_two_instantiations_without_scratch_spills_or_lds(surf_lib):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_resources as KR
    from stabstitch2_amd import _surfaces, _hip
    ks = KR.kernels(_surfaces.LIB_PATH)
    assert sorted(G.instantiation_key(n) for n in ks) == KERNELS, sorted(ks)
    main = {G.instantiation_key(n).split('<')[0] for n in KR.kernels(_hip.LIB_PATH)}
    for n, e in ks.items():
        assert not re.search(r'\b(mb|sm|mw)_[a-z]+_kernel', n), n        # the other libraries' launch witnesses claim that pattern
        assert G.instantiation_key(n).split('<')[0] not in main, n
        assert e['.private_segment_fixed_size'] == 0 and e['.vgpr_spill_count'] == 0 and e['.sgpr_spill_count'] == 0, (n, e)
        assert e['.group_segment_fixed_size'] == 0 and e['mfma_instructions'] == 0, (n, e)
        assert e.get('.agpr_count', 0) == 0 and e['.vgpr_count'] <= 64, (n, e)


def test_every_refusal_comes_before_a_launch(surf_lib):
    """Host pointers throughout: a call that got as far as a launch would fault."""
    buf = (ctypes.c_ubyte * 4096)()
    base = (ctypes.addressof(buf) + 15) & ~15
    fn = surf_lib.ssf_nv12_to_bgr

    def call(y=base, uv=base + 1024, pitch=16, n=1, h=4, w=8, out=base + 2048, stride=None, arrays=(True, True, True), ys=None, uvs=None,
             pitches=None):
        m = max(n, 1) if n <= 96 else 97
        ya = (ctypes.c_void_p * m)(*(ys if ys is not None else [y] * m))
        ua = (ctypes.c_void_p * m)(*(uvs if uvs is not None else [uv] * m))
        pa = (ctypes.c_int * m)(*(pitches if pitches is not None else [pitch] * m))
        return fn(ya if arrays[0] else None, ua if arrays[1] else None, pa if arrays[2] else None, n, h, w, out,
                  3 * h * w if stride is None else stride, None)

    for arrays in ((False, True, True), (True, False, True), (True, True, False)):
        assert call(arrays=arrays) == ERR_ARG                              # a null array
    assert call(out=None) == ERR_ARG
    assert call(y=None) == ERR_ARG and call(uv=None) == ERR_ARG            # a null entry
    assert call(n=3, ys=[base, None, base]) == ERR_ARG and call(n=3, uvs=[base + 1024, base + 1024, None]) == ERR_ARG
    for n in (0, -1, 97, 1 << 30):
        assert call(n=n) == ERR_ARG
    for bad in (0, -2, 3, 5):
        assert call(h=bad) == ERR_ARG and call(w=bad) == ERR_ARG
    assert call(pitch=17) == ERR_ARG and call(pitch=6) == ERR_ARG and call(pitch=0) == ERR_ARG and call(pitch=-16) == ERR_ARG
    assert call(n=2, pitches=[16, 6]) == ERR_ARG and call(n=2, pitches=[16, 9]) == ERR_ARG
    assert call(uv=base + 1025) == ERR_ARG and call(n=2, uvs=[base + 1024, base + 1027]) == ERR_ARG      # a UV plane off its 16-bit pairs
    assert call(stride=3 * 4 * 8 - 1) == ERR_ARG and call(stride=0) == ERR_ARG and call(stride=-96) == ERR_ARG
    assert call(h=65536, w=32768, pitch=32768, stride=1 << 40) == ERR_ARG          # h * w = 2^31
    assert call(h=46342, w=46342, pitch=46342, stride=1 << 40) == ERR_ARG          # the first even square past it


class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))


def _nets():
    return (_Net(), _Net(), _Net())


H, W = 180, 320


def _nv12(k=None, h=H, w=W):
    return torch.zeros(((k,) if k is not None else ()) + (h // 2 * 3, w), dtype=torch.uint8)


def test_ops_refuse_what_is_no_nv12_surface():
    from stabstitch2_amd import ops, _hip
    good = _nv12(2)
    surf, h, w, single = ops.nv12_surfaces(good)
    assert (len(surf), h, w, single) == (2, H, W, False) and ops.nv12_surfaces(good[0])[3] is True
    padded = torch.zeros((270, 384), dtype=torch.uint8)[:, :W]
    assert [s.stride(0) for s in ops.nv12_surfaces([good[0], padded])[0]] == [W, 384]      # a list: every surface its own pitch
    bad = [good.float(), _nv12(2, H, W + 1), torch.zeros((2, 271, W), dtype=torch.uint8), good[:, :, ::2], good[None],
           torch.zeros((270, 385), dtype=torch.uint8)[:, :W], [good[0], _nv12(None, H, W + 2)], [], [good[0], 'x'],
           torch.zeros((0, 270, W), dtype=torch.uint8)]
    for b in bad:
        with pytest.raises(ValueError, match='NV12'):
            ops.nv12_surfaces(b)
        with pytest.raises(ValueError, match='NV12'):
            ops.nv12_to_bgr(b)
    with pytest.raises(_hip.HipError, match='no CPU path'):              # a missing device is an error, not a fallback
        ops.nv12_to_bgr(good)


def test_the_streaming_entries_refuse_before_anything_runs(surf_lib):
    from stabstitch2_amd import online as O
    f = _nv12(4)
    two = O.OnlineStitcher(_nets(), H, W, viewport=(120, 200), grow='refit')
    odd = O.OnlineStitcher(_nets(), H, W, viewport=(121, 200), grow='refit')
    free = O.OnlineStitcher(_nets(), H, W)
    three = O.ThreeViewOnlineStitcher(_nets(), H, W, viewport=(120, 200), grow='refit')
    for st, v in ((two, 2), (three, 3), (free, 2), (odd, 2)):
        views = lambda x: (x,) * v                                      # noqa: E731
        with pytest.raises(ValueError, match="out must be 'bgr' or 'nv12'"):
            st.push_many_nv12(*views(f), out='yuv')
        for k in (0, 33):
            with pytest.raises(ValueError, match='NV12' if k == 0 else '1 to 32'):
                st.push_many_nv12(*views(_nv12(k)))
        with pytest.raises(ValueError, match='1 to 32'):
            st.push_many_nv12(*views([f[0]] * 33))
        with pytest.raises(ValueError, match='differ in length'):
            st.push_many_nv12(*(views(f)[:-1] + (f[:3],)))
        for bad in (_nv12(4, H, W + 2), _nv12(4, H + 2, W), torch.zeros((4, H, W, 3), dtype=torch.uint8), f.float(), f[0], [f[0], f[0][:, ::2]]):
            with pytest.raises(ValueError, match='NV12'):
                st.push_many_nv12(*(views(f)[:-1] + (bad,)))
        assert st.frames_in == 0 and st.static is None and st.batch_captures == 0
    for st in (free, odd):
        with pytest.raises(ValueError, match='even viewport'):
            st.push_many_nv12(f, f, out='nv12')
        assert st.frames_in == 0
    with pytest.raises(ValueError, match='meshes_only'):
        O.OnlineStitcher(_nets(), H, W, meshes_only=True).push_many_nv12(f, f)
    with pytest.raises(ValueError, match='even height and width'):
        O.OnlineStitcher(_nets(), 181, W).push_many_nv12(f, f)
    # the classes without it say so by name
    for cls, name in ((O.PipelinedOnlineStitcher, 'push_many_nv12'), (O.PipelinedThreeViewOnlineStitcher, 'push_many_nv12')):
        st = cls(_nets(), H, W)
        with pytest.raises(ValueError, match='%s has no %s' % (cls.__name__, name)):
            st.push_many_nv12(f, f, out='bgr')
        assert st.frames_in == 0
    pm = O.PipelinedMultiOnlineStitcher(_nets(), H, W, streams=2)
    with pytest.raises(ValueError, match='PipelinedMultiOnlineStitcher has no push_nv12'):
        pm.push_nv12(f[:2], f[:2])
    # MultiOnlineStitcher.push_nv12: S surfaces per view
    ms = O.MultiOnlineStitcher(_nets(), H, W, streams=2)
    with pytest.raises(ValueError, match="out must be"):
        ms.push_nv12(f[:2], f[:2], out='rgb')
    with pytest.raises(ValueError, match='2 NV12 surfaces per view'):
        ms.push_nv12(f[:3], f[:3])
    with pytest.raises(ValueError, match='differ in length'):
        ms.push_nv12(f[:2], f[:3])
    with pytest.raises(ValueError, match='NV12'):
        ms.push_nv12(f[:2], _nv12(2, H, W + 2))
    with pytest.raises(ValueError, match='even viewport'):
        ms.push_nv12(f[:2], f[:2], out='nv12')
    with pytest.raises(ValueError, match='meshes_only'):
        O.MultiOnlineStitcher(_nets(), H, W, streams=2, meshes_only=True).push_nv12(f[:2], f[:2])
    assert ms.frames_in == 0 and pm.frames_in == 0


def test_host_frame_stream_refuses_at_construction():
    from stabstitch2_amd import online as O
    two = O.OnlineStitcher(_nets(), H, W)
    for bad in ('yuv', 'NV12', None, 0):
        with pytest.raises(ValueError, match='frame_format'):
            O.HostFrameStream(two, frame_format=bad)
        with pytest.raises(ValueError, match="out must be"):
            O.HostFrameStream(two, out=bad)
    for bad in (0, -1, 33, 2.0, '4', True):
        with pytest.raises(ValueError, match='batch'):
            O.HostFrameStream(two, batch=bad)
    for st in (O.PipelinedOnlineStitcher(_nets(), H, W), O.PipelinedThreeViewOnlineStitcher(_nets(), H, W),
               O.MultiOnlineStitcher(_nets(), H, W, streams=2), O.PipelinedMultiOnlineStitcher(_nets(), H, W, streams=2)):
        for k in (2, 4, 32):
            with pytest.raises(ValueError, match='push_many_u8'):
                O.HostFrameStream(st, batch=k)
    with pytest.raises(ValueError, match='even viewport'):
        O.HostFrameStream(two, out='nv12')
    with pytest.raises(ValueError, match='even viewport'):
        O.HostFrameStream(O.OnlineStitcher(_nets(), H, W, viewport=(120, 201), grow='refit'), frame_format='nv12', out='nv12')
    with pytest.raises(ValueError, match='even height and width'):
        O.HostFrameStream(O.OnlineStitcher(_nets(), H, W + 1), frame_format='nv12')
