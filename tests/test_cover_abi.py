"""Coverage and the largest covered rectangle without a GPU (libstabstitch_cover.so): the library's header, exports and
ctypes table, the resources of its code objects, what it refuses, the two reference searches of tests/cover_ref.py against each other,
and the refusals of `ops`, `pipeline` and `online`.  The kernels themselves: tests/test_gpu_cover.py.
    python -m pytest tests/test_cover_abi.py"""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

import abi_surface as A
import cover_ref as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1


@pytest.fixture(scope='module')
def cover_lib():
    from stabstitch2_amd import _cover
    return A.built(_cover)


def test_header_exports_and_ctypes_table_agree(cover_lib):
    from stabstitch2_amd import _hip, _cover
    declared, defines = A.check(_cover)
    assert declared == ['ssc_bitmap_words', 'ssc_coverage', 'ssc_covered_rect', 'ssc_rect_workspace_bytes', 'ssc_version']
    assert defines['SSC_ERR_ARG'] == _cover.ERR_ARG == ERR_ARG
    assert defines['SSC_MAX_VIEWS'] == _cover.MAX_VIEWS == 3
    assert defines['SSC_MAX_FRAMES'] == _cover.MAX_FRAMES == 65535
    assert defines['SSC_MAX_WIDTH'] == _cover.MAX_WIDTH >= 8192
    assert (defines['SSC_WARP_NORMAL'], defines['SSC_WARP_FAST']) == (0, 1)
    assert cover_lib.ssc_version() == 1
    # a library of its own in a tuple of its own: the two pinned tuples keep their contents, and no other header knows of it
    assert _hip.FEATURE_LIBRARIES == ('_cover',)
    assert '_cover' not in _hip.LIBRARIES and '_cover' not in _hip.EXTRA_LIBRARIES
    others = A.modules() + [__import__('stabstitch2_amd.' + n, fromlist=['x']) for n in _hip.EXTRA_LIBRARIES]
    assert len(others) == 6
    for m in others:
        # (the library's names in every spelling; the English verb occurs in three older comments: "covers", "must cover")
        assert not re.search(r'ssc_|SSC_|stabstitch_cover|_cover\b|cover\.hip|\bcv_', A.header(m)), m.HEADER
        assert re.findall(r'\w*cover\w*', A.header(m), re.I) in ([], ['covers'], ['cover', 'covers']), m.HEADER
        assert m.PREFIX != _cover.PREFIX and m.API != _cover.API
    names = re.findall(r'^SSC_API\b[^;(]*?\b(\w+)\s*\(', A.header(_cover), re.M)      # every declaration begins its line with the macro
    assert sorted(names) == declared
    assert _cover.LIB_PATH.endswith('lib%s.so' % _cover.HEADER[:-2])


def test_code_objects_have_no_scratch_and_no_spills(cover_lib):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_resources as KR
    from stabstitch2_amd import _cover
    ks = KR.kernels(_cover.LIB_PATH)
    src = open(os.path.join(ROOT, 'stabstitch2_amd', 'csrc', 'cover.hip')).read()
    defined = sorted(set(re.findall(r'__global__[^;{]*?\bvoid\s+(\w+)\s*\(', src)))
    assert defined == ['cv_coverage_kernel', 'cv_heights_kernel', 'cv_reduce_kernel', 'cv_rows_kernel']
    got = sorted(re.search(r'\b(cv_[a-z0-9_]+_kernel)', n).group(1) for n in ks)
    assert got == sorted(defined + ['cv_coverage_kernel']), sorted(ks)       # the coverage kernel in its two forms
    for n, e in ks.items():
        assert not re.search(r'\b(mb|sm|mw|st)_[a-z0-9_]+_kernel', n), n     # the other libraries' launch witnesses claim those patterns
        assert e['.private_segment_fixed_size'] == 0 and e['.vgpr_spill_count'] == 0 and e['.sgpr_spill_count'] == 0, (n, e)
    for n, e in ks.items():                                                  # no LDS beyond the row tables (the search: dynamic)
        if 'cv_coverage_kernel' in n:
            assert e['.group_segment_fixed_size'] == 4 * 64 * 8, (n, e)


def test_every_refusal_comes_before_a_launch(cover_lib):
    """Host pointers throughout: a call that got as far as a launch would fault."""
    from stabstitch2_amd import _cover
    buf = (ctypes.c_float * 4096)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    big = 1 << 40

    def cov(source=p, T=p, bitmap=p, frames=2, views=2, h=24, w=41, hc=43, wc=67, mode=0, min_mask=0.5, acc=0):
        return cover_lib.ssc_coverage(source, T, bitmap, frames, views, h, w, hc, wc, mode, min_mask, acc, None)
    assert cov(source=None) == ERR_ARG and cov(T=None) == ERR_ARG and cov(bitmap=None) == ERR_ARG
    for views in (-1, 0, 1, 4):
        assert cov(views=views) == ERR_ARG
    for k in ('h', 'w', 'hc', 'wc'):
        for v in (1, 0, -3):
            assert cov(**{k: v}) == ERR_ARG, (k, v)
    for mode in (-1, 2, 16, 32):
        assert cov(mode=mode) == ERR_ARG
    for frames in (0, -1):
        assert cov(frames=frames) == ERR_ARG and cov(frames=frames, acc=1) == ERR_ARG
    for mm in (0.0, -0.5, 1.0000001, 2.0, float('nan'), float('inf')):
        assert cov(min_mask=mm) == ERR_ARG and cov(min_mask=mm, acc=1) == ERR_ARG, mm
    assert cov(frames=65536) == ERR_ARG                                       # grid z
    assert cov(hc=8 * 65535 + 1) == ERR_ARG and cov(hc=8 * 65535 + 1, acc=1) == ERR_ARG      # grid y
    assert cov(wc=_cover.MAX_WIDTH + 1) == ERR_ARG

    def rect(bitmap=p, hc=43, wc=67, even=0, ws=p, ws_bytes=big, out=p):
        return cover_lib.ssc_covered_rect(bitmap, hc, wc, even, ws, ws_bytes, out, None)
    assert rect(bitmap=None) == ERR_ARG and rect(ws=None) == ERR_ARG and rect(out=None) == ERR_ARG
    for k in ('hc', 'wc'):
        for v in (1, 0, -3):
            assert rect(**{k: v}) == ERR_ARG
    assert rect(wc=_cover.MAX_WIDTH + 1) == ERR_ARG
    assert rect(hc=1 << 19, wc=8192) == ERR_ARG                              # 2^32 pixels: areas are 32-bit
    need = cover_lib.ssc_rect_workspace_bytes(43, 67)
    assert need >= 43 * 67 * 4 and rect(ws_bytes=need - 1) == ERR_ARG and rect(ws_bytes=0) == ERR_ARG
    # the size queries refuse what the launches refuse
    assert cover_lib.ssc_bitmap_words(43, 67) == 43 * 2 and cover_lib.ssc_bitmap_words(8, 64) == 8 and cover_lib.ssc_bitmap_words(9, 65) == 18
    assert cover_lib.ssc_bitmap_words(785, 1995) == 785 * 32
    for hc, wc in ((1, 67), (43, 1), (43, _cover.MAX_WIDTH + 1), (0, 0)):
        assert cover_lib.ssc_bitmap_words(hc, wc) == ERR_ARG and cover_lib.ssc_rect_workspace_bytes(hc, wc) == ERR_ARG
    assert cover_lib.ssc_rect_workspace_bytes(1 << 19, 8192) == ERR_ARG


def test_pack_and_unpack():
    rs = np.random.RandomState(3)
    for hc, wc in ((3, 9), (8, 64), (9, 65), (43, 67), (5, 130)):
        m = rs.rand(2, hc, wc) < 0.6
        b = C.pack(m)
        assert b.dtype == np.int64 and b.shape == (2, hc, C.words(wc))
        assert np.array_equal(C.unpack(b, wc), m) and not C.unpack(b, wc, pad=True)[..., wc:].any()
    one = np.zeros((2, 70), dtype=bool)
    one[1, 65] = True
    assert C.pack(one)[1, 1] == 2 and C.pack(one)[0].tolist() == [0, 0]
    top = np.zeros((2, 64), dtype=bool)
    top[0, 63] = True
    assert C.pack(top)[0, 0] == -2 ** 63                                     # bit 63: the sign bit of the int64 torch holds


def test_the_stack_reference_equals_brute_force():
    rs = np.random.RandomState(11)
    checked = 0
    for density in (0.3, 0.6, 0.8, 0.9, 0.98):
        for _ in range(50):
            hc, wc = rs.randint(2, 13), rs.randint(2, 71)
            m = rs.rand(hc, wc) < density
            for even in (False, True):
                assert C.rect(m, even) == C.rect_brute(m, even), (m, even)
            checked += 1
    assert checked == 250
    for m in (np.ones((12, 70), bool), np.zeros((12, 70), bool), C.staircase(12, 70), np.indices((12, 70)).sum(0) % 2 == 0):
        assert C.rect(m) == C.rect_brute(m)
    assert C.rect(np.zeros((4, 5), bool)) == (0, 0, 0, 0) and C.rect(np.ones((4, 5), bool)) == (0, 0, 4, 5)
    assert C.rect(np.ones((5, 5), bool), even=True) == (0, 0, 4, 4)
    for name, (m, want) in C.ties().items():
        assert C.rect(m) == C.rect_brute(m) == want, name


def test_ops_refuse_before_anything_runs(cover_lib):
    from stabstitch2_amd import _hip, ops
    src, Tk = torch.zeros((2, 2, 63, 2)), torch.zeros((2, 2, 2, 66))
    ok = dict(h=24, w=41, hc=43, wc=67)
    bad = [dict(source=torch.zeros((2, 4, 63, 2))), dict(source=torch.zeros((2, 2, 63, 3))), dict(T=torch.zeros((3, 2, 2, 66))),
           dict(source=src.double()), dict(mode='SLOW'), dict(min_mask=0.0), dict(min_mask=1.5), dict(min_mask='x'), dict(h=1), dict(w=0),
           dict(hc=1), dict(wc=8193), dict(hc=43.0), dict(source=None)]
    for b in bad:
        kw = dict(dict(source=src, T=Tk, **ok), **b)
        with pytest.raises(ValueError):
            ops.coverage(**kw)
    with pytest.raises(_hip.HipError):
        ops.coverage(src, Tk, **ok)                                          # CPU tensors: no CPU path
    for hc, wc in ((1, 67), (43, 8193), (43, 1)):
        with pytest.raises(ValueError):
            ops.coverage_state(hc, wc, 'cpu')
    with pytest.raises(ValueError, match='CoverageState'):
        ops.coverage_update(torch.zeros((43, 2), dtype=torch.int64), src, Tk, 24, 41)
    state = ops.CoverageState(torch.zeros((43, 2), dtype=torch.int64), torch.zeros(1 << 16, dtype=torch.uint8), 43, 67)
    with pytest.raises(ValueError, match='min_mask'):
        ops.coverage_update(state, src, Tk, 24, 41, min_mask=0.0)
    bm = torch.zeros((43, 2), dtype=torch.int64)
    with pytest.raises(ValueError, match='wc='):
        ops.covered_rect(bm)
    with pytest.raises(ValueError):
        ops.covered_rect(bm.int(), wc=67)
    with pytest.raises(ValueError, match='words'):
        ops.covered_rect(bm, wc=130)
    with pytest.raises(ValueError, match='stack'):
        ops.covered_rect(torch.zeros((3, 43, 2), dtype=torch.int64), wc=67)
    with pytest.raises(ValueError, match='ws'):
        ops.covered_rect(bm, wc=67, ws=torch.zeros(16, dtype=torch.uint8))
    with pytest.raises(ValueError):
        ops.covered_rect(state, wc=67)
    with pytest.raises(_hip.HipError):
        ops.covered_rect(bm, wc=67)


def test_pipeline_refuses_a_bad_crop_before_the_networks_run():
    from stabstitch2_amd import pipeline

    class Nets:                                  # touching a net would raise
        def __getitem__(self, i):
            raise AssertionError('the networks ran')

        def __iter__(self):
            raise AssertionError('the networks ran')
    x = torch.zeros((2, 3, 24, 41))
    u = torch.zeros((2, 24, 41, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match='min_mask'):
        pipeline.Crop(min_mask=0.0)
    with pytest.raises(ValueError, match='min_mask'):
        pipeline.Crop(min_mask=1.5)
    stale = pipeline.Crop()
    stale.rect = (0, 0, 4.0, 4)
    for crop in ('yes', True, (0, 0, 4, 4), stale):
        for call in (lambda: pipeline.run_two_view(x, x, x, x, Nets(), crop=crop),
                     lambda: pipeline.run_three_view(x, x, x, x, x, x, Nets(), crop=crop),
                     lambda: pipeline.run_two_view_u8(u, u, Nets(), device='cpu', crop=crop),
                     lambda: pipeline.run_three_view_u8(u, u, u, Nets(), device='cpu', crop=crop),
                     lambda: pipeline.render_frames([x, x], None, crop=crop),
                     lambda: pipeline.render_frames_u8([u, u], None, crop=crop),
                     lambda: pipeline.three_view_render(x, x, x, None, None, None, crop=crop)):
            with pytest.raises(ValueError, match='[Cc]rop'):
                call()
    c = pipeline.Crop(even=True, min_mask=1)
    assert (c.even, c.min_mask, c.rect, c.canvas) == (True, 1.0, None, None) and pipeline.check_crop(c) is c
    assert pipeline.check_crop(None) is None
    # crop=None is the default of every route, track_coverage=False of every stitcher
    for fn in (pipeline.render_frames, pipeline.render_frames_u8, pipeline.run_two_view, pipeline.run_three_view,
               pipeline.three_view_render, pipeline.run_two_view_u8, pipeline.run_three_view_u8):
        assert inspect.signature(fn).parameters['crop'].default is None, fn.__name__
    for fn in (pipeline.run_two_view_long, pipeline.run_three_view_long, pipeline.LongVideoStitcher.__init__,
               pipeline.HostClipRunner.__init__):
        assert 'crop' not in inspect.signature(fn).parameters, fn.__name__
    assert list(inspect.signature(pipeline.covered_rect).parameters) == ['meshes', 'img_h', 'img_w', 'warp_mode', 'prescaled', 'bbox',
                                                                          'size', 'even', 'min_mask']


class _FakeNet(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))


def test_the_stitchers_refuse_before_anything_runs(monkeypatch):
    from stabstitch2_amd import online
    nets = [_FakeNet(), _FakeNet(), _FakeNet()]
    for cls in (online.OnlineStitcher, online.ThreeViewOnlineStitcher, online.MultiOnlineStitcher, online.PipelinedOnlineStitcher,
                online.PipelinedMultiOnlineStitcher, online.PipelinedThreeViewOnlineStitcher):
        assert inspect.signature(cls.__init__).parameters['track_coverage'].default is False, cls.__name__
    for make in (lambda: online.MultiOnlineStitcher(nets, 180, 320, streams=2, track_coverage=True),
                 lambda: online.PipelinedOnlineStitcher(nets, 180, 320, track_coverage=True),
                 lambda: online.PipelinedMultiOnlineStitcher(nets, 180, 320, streams=2, track_coverage=True),
                 lambda: online.PipelinedThreeViewOnlineStitcher(nets, 180, 320, track_coverage=True)):
        with pytest.raises(ValueError, match='track_coverage'):
            make()
    with pytest.raises(ValueError, match='meshes_only'):
        online.OnlineStitcher(nets, 180, 320, meshes_only=True, track_coverage=True)
    with pytest.raises(ValueError, match='refit'):
        online.OnlineStitcher(nets, 180, 320, grow='refit', viewport=(204, 500), track_coverage=True)
    with pytest.raises(ValueError, match='refit'):
        online.ThreeViewOnlineStitcher(nets, 180, 320, grow='refit', viewport=(204, 660), track_coverage=True)
    # a captured step that renders inside its graph
    monkeypatch.setattr(online, 'DIRECT_RENDER', False)
    with pytest.raises(ValueError, match='graph'):
        online.OnlineStitcher(nets, 180, 320, track_coverage=True)
    with pytest.raises(ValueError, match='graph'):
        online.ThreeViewOnlineStitcher(nets, 180, 320, track_coverage=True)
    monkeypatch.setattr(online, 'DIRECT_RENDER', True)
    monkeypatch.setattr(online, 'DIRECT_LINEAR', False)
    with pytest.raises(ValueError, match='graph'):
        online.OnlineStitcher(nets, 180, 320, fusion_mode='LINEAR', track_coverage=True)
    # what is accepted: tracking off everywhere, on where the push renders or nothing is captured
    online.OnlineStitcher(nets, 180, 320, fusion_mode='LINEAR')
    st = online.OnlineStitcher(nets, 180, 320, fusion_mode='LINEAR', use_graph=False, track_coverage=True)
    assert st.track_coverage and st.coverage_frames == 0 and st.covered_rect() is None
    monkeypatch.setattr(online, 'DIRECT_LINEAR', True)
    st = online.OnlineStitcher(nets, 180, 320, grow='recapture', track_coverage=True)
    assert st.covered_rect() is None and st.covered_rect(even=True) is None
    plain = online.OnlineStitcher(nets, 180, 320)
    assert not plain.track_coverage and plain._cover is None
    with pytest.raises(ValueError, match='track_coverage'):
        plain.covered_rect()
