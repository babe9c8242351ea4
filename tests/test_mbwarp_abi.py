"""The direct MULTIBAND warp and the offline routes' exposure= keyword without a GPU: the fourth library's header, exports and ctypes
table, the kernels the built library carries, what it refuses, and the refusals of the Python layers that come before anything runs.
The kernels themselves: tests/test_gpu_mbwarp.py.
    python -m pytest tests/test_mbwarp_abi.py"""
import ctypes
import os
import re
import sys

import pytest
import torch

import abi_surface as A
import mbwarp_ref as WR
import sweep_inputs as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1


@pytest.fixture(scope='module')
def warp_lib():
    from stabstitch2_amd import _mbwarp
    return A.built(_mbwarp)


def test_header_exports_and_ctypes_table_agree(warp_lib):
    from stabstitch2_amd import _mbwarp
    declared, defines = A.check(_mbwarp)
    assert declared == ['ssw_multiband_warp', 'ssw_multiband_warp_u8', 'ssw_version']
    assert defines['SSW_ERR_ARG'] == _mbwarp.ERR_ARG == ERR_ARG and defines['SSW_MAX_VIEWS'] == _mbwarp.MAX_VIEWS == 3
    assert defines['SSW_MAX_ITEMS'] == _mbwarp.MAX_ITEMS == 65535
    from stabstitch2_amd import ops
    assert (defines['SSW_WARP_NORMAL'], defines['SSW_WARP_FAST']) == (ops.MODES['NORMAL'], ops.MODES['FAST'])
    assert warp_lib.ssw_version() == 1
    # the libraries before it do not know of it: not even the word (its prefix and header: test_native_binding.py, for every library)
    for other, text in A.headers_before(_mbwarp).items():
        assert not re.search(r'mbwarp', text), other


def test_code_objects_hold_the_reach_table_without_scratch_or_spills(warp_lib):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_resources as KR
    from stabstitch2_amd import _mbwarp
    ks = KR.kernels(_mbwarp.LIB_PATH)
    assert sorted(G.instantiation_key(n) for n in ks) == sorted(WR.reach()) and len(ks) == 4, sorted(ks)
    for n, e in ks.items():
        assert not re.search(r'\b(mb|sm)_[a-z]+_kernel', n), n           # the other libraries' launch witness claims that pattern
        assert e['.private_segment_fixed_size'] == 0 and e['.vgpr_spill_count'] == 0 and e['.sgpr_spill_count'] == 0, (n, e)
        assert e.get('.agpr_count', 0) == 0 and e['.vgpr_count'] <= 128, (n, e)                 # four waves per SIMD at the least
        assert e['.group_segment_fixed_size'] == 4 * 64 * 8, (n, e)     # the per-wave row table and nothing else
        assert e['mfma_instructions'] == 0
    # every instantiation has tests that exist
    for key, (kind, tests) in WR.reach().items():
        assert kind == 'exact' and tests
        for t in tests:
            mod, fn = t.split('::')
            assert re.search(r'^def %s\(' % fn, open(os.path.join(ROOT, mod.replace('.', os.sep) + '.py')).read(), re.M), t


def test_every_refusal_comes_before_a_launch(warp_lib):
    """Host pointers throughout: a call that got as far as a launch would fault."""
    buf = (ctypes.c_float * 4096)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    for fn in (warp_lib.ssw_multiband_warp, warp_lib.ssw_multiband_warp_u8):
        def call(imgs=(p, p, p), source=p, T=p, gains=None, out=p, n=1, v=2, h=8, w=8, hc=8, wc=8, mode=0):
            arr = None if imgs is None else (ctypes.c_void_p * 3)(*[None if i is None else i.value for i in imgs])
            return fn(arr, source, T, gains, out, n, v, h, w, hc, wc, mode, None)
        assert call(imgs=None) == ERR_ARG and call(source=None) == ERR_ARG and call(T=None) == ERR_ARG and call(out=None) == ERR_ARG
        assert call(imgs=(p, None, p)) == ERR_ARG and call(imgs=(None, p, p)) == ERR_ARG        # a view without frames
        assert call(imgs=(p, p, None), v=3) == ERR_ARG and call(imgs=(p, p, None), v=3, gains=p) == ERR_ARG
        for v in (-1, 0, 1, 4):
            assert call(v=v) == ERR_ARG
        for bad in (1, 0, -3):
            assert call(h=bad) == ERR_ARG and call(w=bad) == ERR_ARG and call(hc=bad) == ERR_ARG and call(wc=bad) == ERR_ARG
        for mode in (-1, 2, 16, 32):                                      # the renders' mode bits are not this library's
            assert call(mode=mode) == ERR_ARG
        for n in (0, -1):
            assert call(n=n) == ERR_ARG
        # the items ride in gridDim.z: n * V <= 65535
        assert call(n=32768, v=2) == ERR_ARG and call(n=21846, v=3) == ERR_ARG and call(n=65536, v=2, gains=p) == ERR_ARG
        assert call(n=1 << 30, v=3) == ERR_ARG                            # (no 32-bit wrap of n * V)


def test_the_python_layers_refuse_before_anything_runs(warp_lib):
    from stabstitch2_amd import ops, pipeline
    x = torch.zeros((1, 3, 8, 8))
    meshes = [torch.zeros((1, 1, 7, 9, 2))] * 2
    for bad in (0.1, 1, 'yes', (0.1, 10.0), dict(alpha=0.1)):
        with pytest.raises(ValueError, match='ExposureParams'):
            pipeline.render_frames([x, x], meshes, exposure=bad)
        with pytest.raises(ValueError, match='ExposureParams'):
            pipeline.run_two_view(x, x, x, x, None, exposure=bad)
        with pytest.raises(ValueError, match='ExposureParams'):
            pipeline.run_three_view(x, x, x, x, x, x, None, exposure=bad)
        with pytest.raises(ValueError, match='ExposureParams'):
            pipeline.render_frames_u8([x, x], meshes, exposure=bad)
        with pytest.raises(ValueError, match='ExposureParams'):
            pipeline.run_two_view_u8(x, x, None, device='cpu', exposure=bad)
        with pytest.raises(ValueError, match='ExposureParams'):
            pipeline.run_three_view_u8(x, x, x, None, device='cpu', exposure=bad)
    st = ops.exposure_state('cpu')
    with pytest.raises(ValueError, match='exposure_state'):
        pipeline.render_frames([x, x], meshes, exposure_state=st)
    with pytest.raises(ValueError, match='exposure_state'):
        pipeline.render_frames_u8([x, x], meshes, exposure_state=st)
    with pytest.raises(ValueError, match='exposure_state'):
        pipeline.three_view_render(x, x, x, meshes[0], meshes[0], meshes[0], exposure_state=st)
    assert pipeline.exposure_params(None) is None and pipeline.exposure_params(True) == ops.ExposureParams()
    p = ops.ExposureParams(alpha=0.5)
    assert pipeline.exposure_params(p) is p and pipeline.exposure_params(p, st) is p
    # gains of the wrong shape: render_multiband and multiband_warp say so
    src, T = torch.zeros((2, 63, 2)), torch.zeros((2, 2, 66))
    for bad in (torch.ones((3, 3)), torch.ones((2, 2, 3)), torch.ones((1, 2, 4)), torch.ones(6)):
        with pytest.raises(ValueError, match='gains'):
            ops.render_multiband([x, x], src, T, 16, 16, gains=bad)
        with pytest.raises(ValueError, match='gains'):
            ops.multiband_warp([x, x], src, T, 16, 16, gains=bad)
    clip = torch.zeros((2, 3, 8, 8))
    with pytest.raises(ValueError, match='gains'):
        ops.render_multiband([clip, clip], src[None].repeat(2, 1, 1, 1), T[None].repeat(2, 1, 1, 1), 16, 16, gains=torch.ones((2, 3)))
