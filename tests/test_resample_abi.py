"""The fixed-size output of a rectangle without a GPU (libstabstitch_resample.so): the library's header, exports and
ctypes table, the tuples of `_hip`, the resources of its code objects, what it refuses, the window rule against tests/resample_ref.py,
that reference against torch's CPU float64 interpolate, the fp32 restatement against the gate, and the refusals of `ops`, `pipeline`
and `online`.  The kernel itself: tests/test_gpu_resample.py.
    python -m pytest tests/test_resample_abi.py"""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

import abi_surface as A
import resample_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
CASES = [(rect, size, aspect) for rect in R.RECTS for size in R.SIZES for aspect in R.ASPECTS]


@pytest.fixture(scope='module')
def rs_lib():
    from stabstitch2_amd import _resample
    return A.built(_resample)


@pytest.fixture(scope='module')
def frame():
    return np.random.default_rng(0).integers(0, 256, size=(3,) + R.FRAME).astype(np.float64)


def test_header_exports_and_ctypes_table_agree(rs_lib):
    from stabstitch2_amd import _hip, _resample
    declared, defines = A.check(_resample)
    assert declared == ['ssr_resample_f32', 'ssr_resample_u8', 'ssr_resample_u8_nv12', 'ssr_source_window', 'ssr_version']
    assert defines['SSR_ERR_ARG'] == _resample.ERR_ARG == ERR_ARG
    assert defines['SSR_MAX_FRAMES'] == _resample.MAX_FRAMES == 65535
    assert (defines['SSR_ASPECT_STRETCH'], defines['SSR_ASPECT_FILL']) == (_resample.ASPECTS['stretch'], _resample.ASPECTS['fill']) == (0, 1)
    assert rs_lib.ssr_version() == 1
    names = re.findall(r'^SSR_API\b[^;(]*?\b(\w+)\s*\(', A.header(_resample), re.M)      # every declaration begins its line with the macro
    assert sorted(names) == declared
    assert _resample.LIB_PATH.endswith('lib%s.so' % _resample.HEADER[:-2])


def test_the_tuples(rs_lib):
    """The three older tuples are what they were; the new library is a member of the open one (membership, not equality: the next
    library needs no edit here), and all_libraries() is the four joined, which the build walks."""
    from stabstitch2_amd import _hip, _resample
    assert _hip.LIBRARIES == ('_hip', '_blend', '_seam', '_mbwarp', '_surfaces')
    assert _hip.EXTRA_LIBRARIES == ('_smoothtail',)
    assert _hip.FEATURE_LIBRARIES == ('_cover',)
    assert '_resample' in _hip.LATER_LIBRARIES
    assert _hip.all_libraries() == _hip.LIBRARIES + _hip.EXTRA_LIBRARIES + _hip.FEATURE_LIBRARIES + _hip.LATER_LIBRARIES
    assert len(set(_hip.all_libraries())) == len(_hip.all_libraries())
    import __graft_entry__ as g
    assert 'all_libraries()' in inspect.getsource(g.build)
    build_sh = open(os.path.join(ROOT, 'stabstitch2_amd', 'csrc', 'build.sh')).read()
    assert re.search(r'for NAME in [a-z ]*\bresample\b', build_sh)
    # no older header knows of it
    older = [n for n in _hip.all_libraries() if n != '_resample']
    assert len(older) >= 7
    for name in older:
        m = __import__('stabstitch2_amd.' + name, fromlist=['x'])
        assert not re.search(r'ssr_|SSR_|stabstitch_resample|\brs_', A.header(m)), m.HEADER
        assert m.PREFIX != _resample.PREFIX and m.API != _resample.API


def test_code_objects_have_no_scratch_and_no_spills(rs_lib):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_resources as KR
    from stabstitch2_amd import _resample
    ks = KR.kernels(_resample.LIB_PATH)
    src = open(os.path.join(ROOT, 'stabstitch2_amd', 'csrc', 'resample.hip')).read()
    defined = sorted(set(re.findall(r'__global__[^;{]*?\bvoid\s+(\w+)\s*\(', src)))
    assert defined == ['rs_resample_kernel']
    got = sorted(re.search(r'\b(rs_[a-z0-9_]+_kernel)', n).group(1) for n in ks)
    assert got == ['rs_resample_kernel'] * 3, sorted(ks)                     # fp32, bytes, NV12
    for n, e in ks.items():
        assert not re.search(r'\b(mb|sm|mw|st|cv)_[a-z0-9_]+_kernel', n), n  # the other libraries' launch witnesses claim those patterns
        assert e['.private_segment_fixed_size'] == 0 and e['.vgpr_spill_count'] == 0 and e['.sgpr_spill_count'] == 0, (n, e)
        assert 0 < e['.group_segment_fixed_size'] <= 64 * 1024, (n, e)
    assert not re.search(r'atomic\w*\s*\(', src, re.I)                       # no atomic operation is called


def test_every_refusal_comes_before_a_launch(rs_lib):
    """Host pointers throughout: a call that got as far as a launch would fault."""
    buf = (ctypes.c_float * 4096)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    base = dict(n=2, Hc=43, Wc=67, Hout=16, Wout=24, aspect=1, rect_dev=None, y0=5, x0=7, h=30, w=50)

    def tail(kw):
        a = dict(base, **kw)
        return [a[k] for k in ('n', 'Hc', 'Wc', 'Hout', 'Wout', 'aspect', 'rect_dev', 'y0', 'x0', 'h', 'w')] + [None]

    def f32(src=p, out=p, **kw):
        return rs_lib.ssr_resample_f32(src, out, *tail(kw))

    def u8(src=p, out=p, stride=1 << 40, **kw):
        return rs_lib.ssr_resample_u8(src, out, stride, *tail(kw))

    def nv(src=p, y=p, uv=p, pitch=24, stride=1 << 40, **kw):
        return rs_lib.ssr_resample_u8_nv12(src, y, uv, pitch, stride, *tail(kw))
    common = [dict(src=None), dict(n=0), dict(n=-1), dict(n=65536), dict(aspect=2), dict(aspect=-1),
              dict(Hc=1 << 16, Wc=1 << 15), dict(Hout=1 << 16, Wout=1 << 15),        # 2^31 pixels in one frame
              dict(Hout=16 * 65535 + 2, Wout=2), dict(Hout=2, Wout=64 * 65535 + 2)]  # grid axes
    common += [dict({k: v}) for k in ('Hc', 'Wc', 'Hout', 'Wout') for v in (0, -2)]
    common += [dict({k: -1}) for k in ('y0', 'x0', 'h', 'w')]                        # a host rectangle with a negative member
    for fn in (f32, u8, nv):
        for kw in common:
            assert fn(**kw) == ERR_ARG, (fn.__name__, kw)
        for kw in common:                                                            # the same with a device rectangle named
            if not set(kw) & {'y0', 'x0', 'h', 'w'}:
                assert fn(rect_dev=p, **kw) == ERR_ARG, (fn.__name__, kw)
    assert f32(out=None) == ERR_ARG and u8(out=None) == ERR_ARG and nv(y=None) == ERR_ARG and nv(uv=None) == ERR_ARG
    assert u8(stride=3 * 16 * 24 - 1) == ERR_ARG and u8(stride=0) == ERR_ARG
    for kw in (dict(Hout=15), dict(Wout=23), dict(pitch=25), dict(pitch=22), dict(stride=24 * 24 - 2), dict(stride=(1 << 40) + 1),
               dict(uv=ctypes.c_void_p(p.value + 1))):
        assert nv(**kw) == ERR_ARG, kw
    # the window: refusals, and an empty rectangle is no refusal
    out = (ctypes.c_double * 4)()
    rect = (ctypes.c_int * 4)(5, 7, 30, 50)
    assert rs_lib.ssr_source_window(rect, 43, 67, 16, 24, 1, out) == 0
    assert rs_lib.ssr_source_window(None, 43, 67, 16, 24, 1, out) == ERR_ARG
    assert rs_lib.ssr_source_window(rect, 43, 67, 16, 24, 1, None) == ERR_ARG
    for args in ((0, 67, 16, 24, 1), (43, 67, 0, 24, 1), (43, 67, 16, 24, 2)):
        assert rs_lib.ssr_source_window(rect, *args, out) == ERR_ARG
    assert rs_lib.ssr_source_window((ctypes.c_int * 4)(5, -7, 30, 50), 43, 67, 16, 24, 1, out) == ERR_ARG


def test_source_window_equals_the_reference_bit_for_bit(rs_lib):
    from stabstitch2_amd import ops
    seen = set()
    for rect, size, aspect in CASES:
        want = R.window(rect, *R.FRAME, *size, aspect)
        got = ops.resample_window(rect, R.FRAME, size, aspect)
        assert [np.float64(v).tobytes() for v in got] == [np.float64(v).tobytes() for v in want], (rect, size, aspect, got, want)
        seen.add(want != tuple(float(v) for v in R.window(rect, *R.FRAME, *size, 'stretch')))
    assert seen == {False, True}                                             # 'fill' did cut some windows
    # 720p numbers: a fractional window
    assert ops.resample_window((39, 7, 704, 1980), (785, 1995), (720, 1280)) == R.window((39, 7, 704, 1980), 785, 1995, 720, 1280, 'fill')
    assert R.window((39, 7, 704, 1980), 785, 1995, 720, 1280, 'fill')[3] == 704 * 1280 / 720
    assert ops.resample_window((5, 7, 0, 9), R.FRAME, (4, 4)) == (0.0, 0.0, 0.0, 0.0)


def test_the_reference_equals_torch_interpolate(frame):
    """'stretch' is torch's CPU float64 interpolate(mode='bilinear', antialias=True) of the cropped frame."""
    x = torch.from_numpy(frame)[None]
    checked = 0
    for rect in R.RECTS:
        c = R.clip(rect, *R.FRAME)
        if c is None:
            continue
        ya, xa, yb, xb = c
        for size in R.SIZES:
            want = torch.nn.functional.interpolate(x[:, :, ya:yb, xa:xb], size=size, mode='bilinear', antialias=True, align_corners=False)
            got = R.resample(frame, size, rect, 'stretch')
            assert np.abs(got - want[0].numpy()).max() <= 1e-9, (rect, size)
            checked += 1
    assert checked == 7 * 8


def test_identity_is_exact_and_empty_is_black(frame):
    for aspect in R.ASPECTS:
        got = R.resample(frame, (30, 50), (5, 7, 30, 50), aspect)
        assert np.array_equal(got, frame[:, 5:35, 7:57])
        assert np.array_equal(R.resample_f32_sequential(frame, (30, 50), (5, 7, 30, 50), aspect), frame[:, 5:35, 7:57].astype(np.float32))
        assert not R.resample(frame, (4, 7), (5, 7, 0, 9), aspect).any()
    b, v = R.resample_u8(np.zeros((1, 4, 6, 3), np.uint8), (2, 2), (0, 0, 0, 0))
    nv = R.nv12(b)
    assert not b.any() and (nv[:, :2] == 16).all() and (nv[:, 2:] == 128).all()


def test_fmaf_restatement_is_exact():
    """Against exact rational arithmetic on values that sit on fp32 midpoints after the float64 sum."""
    from fractions import Fraction
    rng = np.random.default_rng(5)
    a = rng.random(2000).astype(np.float32)
    b = rng.integers(0, 256, 2000).astype(np.float32)
    c = (rng.random(2000) * 255).astype(np.float32)
    a[:4] = np.float32([2.0 ** -30, 2.0 ** -30, 1 + 2.0 ** -23, 2.0 ** -40])
    b[:4] = np.float32([1.0, -1.0, 1 + 2.0 ** -23, 3.0])
    c[:4] = np.float32([1 + 2.0 ** -24 * 0 + 2.0 ** -23, 1.0, 2.0 ** -24, 1 + 2.0 ** -23])
    got = R.fmaf(a, b, c)
    for i in range(len(a)):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo = np.nextafter(got[i], np.float32(-np.inf))
        hi = np.nextafter(got[i], np.float32(np.inf))
        err = abs(Fraction(float(got[i])) - exact)
        assert err <= abs(Fraction(float(lo)) - exact) and err <= abs(Fraction(float(hi)) - exact), i
        if err == abs(Fraction(float(lo)) - exact) or err == abs(Fraction(float(hi)) - exact):       # a true tie: to even
            assert int(np.float32(got[i]).view(np.uint32)) % 2 == 0 or err == 0, i


def test_the_fp32_restatement_stays_within_the_bound(frame):
    """Calibrates the gate on the CPU: the kernel's arithmetic, restated, against the float64 definition at every case."""
    worst = 0.0
    paths = set()
    for rect, size, aspect in CASES:
        ky, kx = R.tap_counts(rect, *R.FRAME, *size, aspect)
        ref = R.resample(frame, size, rect, aspect)
        seq = R.resample_f32_sequential(frame, size, rect, aspect)
        err = float(np.abs(seq.astype(np.float64) - ref).max())
        assert err <= R.bound(ky, kx), (rect, size, aspect, err, R.bound(ky, kx))
        worst = max(worst, err / R.bound(ky, kx))
        paths.add(R.staged(rect, *R.FRAME, *size, aspect))
    assert worst > 0.0
    assert True in paths and False in paths                                  # both of the kernel's paths occur among the cases
    assert R.staged((5, 7, 30, 50), *R.FRAME, 16, 24, 'fill') is True and R.staged((5, 7, 30, 50), *R.FRAME, 4, 7, 'fill') is False
    assert R.tap_counts((5, 7, 30, 50), *R.FRAME, 4, 7, 'stretch')[0] >= 15


def test_ops_refuse_before_anything_runs(rs_lib):
    from stabstitch2_amd import ops
    f = torch.zeros((2, 3, 43, 67))
    u = torch.zeros((2, 43, 67, 3), dtype=torch.uint8)
    bad = [dict(frames=f.double()), dict(frames=f[0, 0]), dict(frames=torch.zeros((2, 4, 43, 67))), dict(frames=u.permute(0, 3, 1, 2)),
           dict(frames=None), dict(size=(16,)), dict(size=(16, 0)), dict(size=(16.0, 24)), dict(size=16), dict(aspect='fit'),
           dict(aspect=1), dict(out_format='yuv'), dict(out_format='nv12'), dict(frames=u, out_format='nv12', size=(15, 24)),
           dict(frames=u, out_format='nv12', size=(16, 23)), dict(rect=(5, 7, 30)), dict(rect=(5, -7, 30, 50)), dict(rect=(5, 7, 30.0, 50)),
           dict(rect=torch.zeros(4, dtype=torch.int64)), dict(rect=torch.zeros(3, dtype=torch.int32)),
           dict(rect=torch.zeros(4, dtype=torch.int32, device='meta')),
           dict(out=torch.zeros((2, 3, 16, 25))), dict(out=torch.zeros((2, 3, 16, 24), dtype=torch.float64)),
           dict(out=torch.zeros((2, 3, 16, 48))[..., ::2]), dict(frames=u, out=torch.zeros((2, 16, 24, 3))),
           dict(frames=u, out=torch.zeros((2, 16, 24, 6), dtype=torch.uint8)[..., ::2]),
           dict(frames=u, out_format='nv12', out=torch.zeros((2, 24, 25), dtype=torch.uint8)[..., :24]),     # an odd pitch
           dict(frames=u, out_format='nv12', out=torch.zeros((2, 16, 24, 3), dtype=torch.uint8))]
    for b in bad:
        kw = dict(dict(frames=f, size=(16, 24)), **b)
        with pytest.raises(ValueError) as e:
            ops.resample(**kw)
        assert 'no CPU path' not in str(e.value), b                          # refused for what is wrong, before the device is looked at
    with pytest.raises(ValueError, match='no CPU path'):                     # a wrong device
        ops.resample(f, (16, 24))
    for kw in (dict(rect=(5, 7, 30)), dict(rect=torch.zeros(4, dtype=torch.int32)), dict(size=(0, 4)), dict(aspect='x'), dict(frame_hw=(43,))):
        with pytest.raises(ValueError):
            ops.resample_window(**dict(dict(rect=(5, 7, 30, 50), frame_hw=(43, 67), size=(16, 24)), **kw))
    assert list(inspect.signature(ops.resample).parameters) == ['frames', 'size', 'rect', 'aspect', 'out', 'out_format']
    assert inspect.signature(ops.resample).parameters['aspect'].default == 'fill'


def test_pipeline_refuses_a_bad_size_before_the_networks_run():
    from stabstitch2_amd import pipeline

    class Nets:                                  # touching a net would raise
        def __getitem__(self, i):
            raise AssertionError('the networks ran')

        def __iter__(self):
            raise AssertionError('the networks ran')
    for kw in (dict(size=(24,)), dict(size=(24, 0)), dict(size=(24.0, 64)), dict(size='720p'), dict(size=(24, 64), aspect='fit'), dict(aspect=None)):
        with pytest.raises(ValueError, match='Crop'):
            pipeline.Crop(**kw)
    c = pipeline.Crop(size=(24, 64))
    assert (c.size, c.aspect, c.rect, c.canvas, c.even, c.min_mask) == ((24, 64), 'fill', None, None, False, 0.5)
    assert pipeline.Crop(size=[24, 64], aspect='stretch').size == (24, 64) and pipeline.Crop().size is None
    assert list(inspect.signature(pipeline.Crop.__init__).parameters) == ['self', 'even', 'min_mask', 'size', 'aspect']
    x = torch.zeros((2, 3, 24, 41))
    u = torch.zeros((2, 24, 41, 3), dtype=torch.uint8)
    stale = pipeline.Crop(size=(24, 64))
    stale.size = (24, -1)                        # changed after it was built
    late = pipeline.Crop(size=(24, 64))
    late.aspect = 'fit'
    for crop in (stale, late):
        for call in (lambda: pipeline.run_two_view(x, x, x, x, Nets(), crop=crop),
                     lambda: pipeline.run_three_view(x, x, x, x, x, x, Nets(), crop=crop),
                     lambda: pipeline.run_two_view_u8(u, u, Nets(), device='cpu', crop=crop),
                     lambda: pipeline.run_three_view_u8(u, u, u, Nets(), device='cpu', crop=crop),
                     lambda: pipeline.render_frames([x, x], None, crop=crop),
                     lambda: pipeline.render_frames_u8([u, u], None, crop=crop),
                     lambda: pipeline.three_view_render(x, x, x, None, None, None, crop=crop)):
            with pytest.raises(ValueError, match='Crop'):
                call()


class _FakeNet(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))


def test_the_stitchers_refuse_before_anything_runs():
    from stabstitch2_amd import online
    nets = [_FakeNet(), _FakeNet(), _FakeNet()]
    frame = torch.zeros((3, 8, 8))
    for plain in (online.OnlineStitcher(nets, 180, 320), online.ThreeViewOnlineStitcher(nets, 180, 320)):
        with pytest.raises(ValueError, match='track_coverage'):
            plain.covered_rect_device()
        with pytest.raises(ValueError, match='track_coverage'):
            plain.to_size(frame, (4, 4))
    # the classes that refuse track_coverage keep refusing it
    for make in (lambda: online.MultiOnlineStitcher(nets, 180, 320, streams=2, track_coverage=True),
                 lambda: online.PipelinedOnlineStitcher(nets, 180, 320, track_coverage=True),
                 lambda: online.PipelinedMultiOnlineStitcher(nets, 180, 320, streams=2, track_coverage=True),
                 lambda: online.PipelinedThreeViewOnlineStitcher(nets, 180, 320, track_coverage=True)):
        with pytest.raises(ValueError, match='track_coverage'):
            make()
    for st in (online.OnlineStitcher(nets, 180, 320, track_coverage=True), online.ThreeViewOnlineStitcher(nets, 180, 320, track_coverage=True)):
        assert st.covered_rect_device() is None and st.covered_rect_device(even=True) is None
        for kw in (dict(size=(4,)), dict(size=(4, 0)), dict(aspect='fit')):
            with pytest.raises(ValueError, match='size|aspect'):
                st.to_size(**dict(dict(frames=frame, size=(4, 4)), **kw))
        with pytest.raises(ValueError, match='no canvas'):
            st.to_size(frame, (4, 4))
        st._cover, st.hc, st.wc = object(), 8, 8                             # a canvas, as far as the checks look
        for bad in (torch.zeros((3, 8, 9)), torch.zeros((8, 8)), torch.zeros((9, 8, 3), dtype=torch.uint8), None):
            with pytest.raises(ValueError, match='canvas'):
                st.to_size(bad, (4, 4))
        with pytest.raises(ValueError, match='rect'):
            st.to_size(frame, (4, 4), rect=(0, 0, 4, 4))
        with pytest.raises(ValueError, match='rect'):
            st.to_size(frame, (4, 4), rect=torch.zeros(4, dtype=torch.int64))
        st._cover = None
    assert list(inspect.signature(online.OnlineStitcher.to_size).parameters) == ['self', 'frames', 'size', 'aspect', 'rect', 'out', 'out_format']
