"""SmoothNet's clip-only Conv3d stack without a GPU (libstabstitch_smoothtail.so): the library's header, exports and
ctypes table, the resources of its code objects, what it refuses, and when pipeline.smooth_stage takes it.  The kernels themselves:
tests/test_gpu_smoothtail.py.
    python -m pytest tests/test_smoothtail_abi.py"""
import ctypes
import os
import re
import sys

import pytest
import torch

import abi_surface as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1


@pytest.fixture(scope='module')
def tail_lib():
    from stabstitch2_amd import _smoothtail
    return A.built(_smoothtail)


def test_header_exports_and_ctypes_table_agree(tail_lib):
    from stabstitch2_amd import _hip, _smoothtail, smooth_network
    declared, defines = A.check(_smoothtail)
    assert declared == ['sst_compact_frames', 'sst_conv3d_layer', 'sst_decode_scatter', 'sst_version']
    assert defines['SST_ERR_ARG'] == _smoothtail.ERR_ARG == ERR_ARG
    assert defines['SST_MAX_WINDOWS'] == _smoothtail.MAX_WINDOWS == smooth_network.WINDOW_CHUNK
    assert defines['SST_K_TILES'] == _smoothtail.K_TILES == 5 * 3 * 3 * 128 // 32
    assert tail_lib.sst_version() == 1
    # a library of its own, outside the five: they keep their list, and none of their headers knows of it
    assert _hip.EXTRA_LIBRARIES == ('_smoothtail',) and '_smoothtail' not in _hip.LIBRARIES
    for m in A.modules():
        assert not re.search(r'sst_|SST_|smoothtail', A.header(m)), m.HEADER
        assert m.PREFIX != _smoothtail.PREFIX and m.API != _smoothtail.API
    # every declaration begins its line with the macro and carries the prefix
    names = re.findall(r'^SST_API\b[^;(]*?\b(\w+)\s*\(', A.header(_smoothtail), re.M)
    assert sorted(names) == declared
    assert _smoothtail.LIB_PATH.endswith('lib%s.so' % _smoothtail.HEADER[:-2])


def test_code_objects_have_no_scratch_and_no_spills(tail_lib):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_resources as KR
    from stabstitch2_amd import _smoothtail
    ks = KR.kernels(_smoothtail.LIB_PATH)
    assert len(ks) == 3 and sorted(re.search(r'(st_[a-z0-9_]+_kernel)', n).group(1) for n in ks) == \
        ['st_conv3d_kernel', 'st_decode_kernel', 'st_reduce_kernel'], sorted(ks)
    for n, e in ks.items():
        assert not re.search(r'\b(mb|sm|mw)_[a-z]+_kernel', n), n         # the other libraries' launch witnesses claim those patterns
        assert e['.private_segment_fixed_size'] == 0 and e['.vgpr_spill_count'] == 0 and e['.sgpr_spill_count'] == 0, (n, e)
    conv = next(e for n, e in ks.items() if 'st_conv3d_kernel' in n)
    assert conv['mfma_instructions'] == 16                               # one K tile of 32: 16 x v_mfma_f32_32x32x2_f32, one loop body
    assert conv['.vgpr_count'] + conv.get('.agpr_count', 0) <= 128       # four workgroups of 256 threads per CU by registers
    assert conv['.group_segment_fixed_size'] == 2 * 2 * 64 * 36 * 4      # two buffers of both operands, [64][32 + 4] floats each
    assert all(e['mfma_instructions'] == 0 for n, e in ks.items() if 'st_conv3d_kernel' not in n)


def test_every_refusal_comes_before_a_launch(tail_lib):
    """Host pointers throughout: a call that got as far as a launch would fault."""
    buf = (ctypes.c_float * 4096)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    big = 1 << 40

    def layer(x=p, w=p, b=p, out=p, ws=p, ws_floats=big, nw=2, first_in=0, first_out=2, seg=180):
        return tail_lib.sst_conv3d_layer(x, w, b, out, ws, ws_floats, nw, first_in, first_out, seg, None)
    assert layer(x=None) == ERR_ARG and layer(w=None) == ERR_ARG and layer(out=None) == ERR_ARG
    for nw in (0, -1, 2049, 1 << 30):
        assert layer(nw=nw) == ERR_ARG
    for fi, fo in ((2, 0), (4, 2), (6, 4), (1, 0)):                      # first_out < first_in
        assert layer(first_in=fi, first_out=fo) == ERR_ARG
    for fi, fo in ((1, 2), (2, 2), (3, 4), (5, 6), (6, 6), (1, 1)):      # the input lacks frame first_out - 2
        assert layer(first_in=fi, first_out=fo) == ERR_ARG
    for fi, fo in ((-1, 2), (0, 7), (0, -1), (7, 7)):
        assert layer(first_in=fi, first_out=fo) == ERR_ARG
    for seg in (0, -5, 181):
        assert layer(seg=seg) == ERR_ARG
    # a K cut needs its workspace: ceil(180 / seg) * frames_out * 63 * 128 floats
    need = 2 * (7 + 1 * 5) * 63 * 128
    assert layer(seg=90, ws=None) == ERR_ARG and layer(seg=90, ws_floats=need - 1) == ERR_ARG and layer(seg=90, ws_floats=0) == ERR_ARG

    def decode(hid=p, w=p, b=p, delta=p, nw=2, first=6):
        return tail_lib.sst_decode_scatter(hid, w, b, delta, nw, first, None)
    assert decode(hid=None) == ERR_ARG and decode(w=None) == ERR_ARG and decode(delta=None) == ERR_ARG
    for nw in (0, -1, 2049):
        assert decode(nw=nw) == ERR_ARG
    for first in (-1, 7):
        assert decode(first=first) == ERR_ARG
    assert tail_lib.sst_compact_frames(0, 0) == 0 and tail_lib.sst_compact_frames(3, 7) == 0
    assert [tail_lib.sst_compact_frames(26, f) for f in (0, 2, 4, 6)] == [182, 132, 82, 32]
    assert tail_lib.sst_compact_frames(1, 6) == 7 and tail_lib.sst_compact_frames(2048, 0) == 2048 * 7


def test_the_python_layer_refuses_and_chooses_before_anything_runs(tail_lib, monkeypatch):
    from stabstitch2_amd import _hip, ops
    x = torch.zeros((12, 63, 128))
    w = torch.zeros((128, 5, 3, 3, 128))
    with pytest.raises(ValueError, match='smooth_tail_layer'):
        ops.smooth_tail_layer(x, w, None, 3, 0, 2, 180)                  # 3 windows from frame 0 are 21 frames
    with pytest.raises(ValueError, match='smooth_tail_layer'):
        ops.smooth_tail_layer(torch.zeros((14, 63, 128)), w[:, :3], None, 2, 0, 2, 180)
    with pytest.raises(_hip.HipError):
        ops.smooth_tail_layer(torch.zeros((14, 63, 128)), w, None, 2, 0, 2, 180)      # CPU tensors: no CPU path
    with pytest.raises(ValueError, match='smooth_tail_decode'):
        ops.smooth_tail_decode(torch.zeros((8, 63, 128)), torch.zeros((4, 128)), None, torch.zeros((3, 7, 7, 9, 4)), 3)
    # when the stage takes the path
    monkeypatch.setattr(ops, 'SMOOTH_TAIL', True)
    assert ops.smooth_tail_usable(1, 7) and ops.smooth_tail_usable(26, 7) and ops.smooth_tail_usable(2048, 7)
    assert not ops.smooth_tail_usable(2049, 7) and not ops.smooth_tail_usable(0, 7)
    assert not ops.smooth_tail_usable(26, 5) and not ops.smooth_tail_usable(26, 9)
    with ops.deterministic():
        assert not ops.smooth_tail_usable(26, 7)
    monkeypatch.setattr(ops, 'SMOOTH_TAIL', False)
    assert not ops.smooth_tail_usable(26, 7)
    # the K cut is the conv engine's for the same windows (ss_conv_workspace_need): two partial sums for the 26 windows of a
    # 32-frame clip, none from 38 windows on (512 workgroups of 64 x 64 without a cut), 36 for a single window
    assert ops.smooth_tail_seg_tiles(26) == 90 and ops.smooth_tail_seg_tiles(37) == 90
    assert ops.smooth_tail_seg_tiles(38) == 180 and ops.smooth_tail_seg_tiles(2048) == 180
    assert ops.smooth_tail_seg_tiles(1) == 5 and ops.smooth_tail_seg_tiles(2) == 10 and ops.smooth_tail_seg_tiles(3) == 14
