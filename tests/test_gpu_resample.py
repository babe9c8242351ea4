"""The fixed-size output of a rectangle on the GPU (libstabstitch_resample.so): the kernel in its three output forms
against tests/resample_ref.py -- the float64 definition through the gate `bound`, the sequential fp32 restatement bit for bit -- and
the layers above it (`Crop(size=)` of the offline routes, `to_size` of the streaming stitchers) against `ops.resample` of the same
frames."""
import functools
import gc
import re

import numpy as np
import pytest
import torch

import resample_ref as R
from test_gpu_mbwarp import _same
from test_gpu_parity import dev, hip_nets  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
T = torch.from_numpy
N = 3
HC, WC = R.FRAME
# named: a case every tile of which takes the staged path (weights and the horizontal pass in LDS), and one that takes the direct
# path (7 x down: 15 and more taps per axis)
STAGED_CASE = ((5, 7, 30, 50), (16, 24), 'fill')
DIRECT_CASE = ((5, 7, 30, 50), (4, 7), 'stretch')


@pytest.fixture(autouse=True)
def _no_garbage_inside_a_capture():
    """A stitcher that became cyclic garbage still owns HIP graphs: collect between the tests, where nothing captures."""
    gc.collect()
    yield
    gc.collect()


@functools.lru_cache(maxsize=None)
def _host_frames():
    u8 = np.random.default_rng(0).integers(0, 256, size=(N, HC, WC, 3)).astype(np.uint8)
    u8.setflags(write=False)
    return u8


@functools.lru_cache(maxsize=None)
def _reference(rect, size, aspect):
    """(float64 [N,3,Hout,Wout], the fp32 restatement, the bytes [N,Hout,Wout,3], bound) of a case, computed once."""
    planes = np.moveaxis(_host_frames(), -1, 1).astype(np.float64)
    ref = R.resample(planes, size, rect, aspect)
    seq = R.resample_f32_sequential(planes, size, rect, aspect)
    ky, kx = R.tap_counts(rect, HC, WC, size[0], size[1], aspect)
    return ref, seq, R.to_bytes(np.moveaxis(ref, 1, -1)), R.bound(ky, kx)


def _device_frames(dev):
    u8 = T(_host_frames().copy()).to(dev)
    return u8, u8.permute(0, 3, 1, 2).float().contiguous()


def _bytes_gate(got, ref64_hwc, want, bound, what):
    """Equal to the reference's bytes; a byte may differ, by 1, only where the float64 value lies within `bound` of k + 0.5, and at
    most 2 % of a case's bytes may use that."""
    got, want = got.astype(np.int64), want.astype(np.int64)
    diff = got != want
    if diff.any():
        frac = ref64_hwc - np.floor(ref64_hwc)
        assert (np.abs(frac[diff] - 0.5) <= bound).all(), (what, 'a byte differs away from a tie')
        assert np.abs(got - want).max() == 1, what
        assert diff.mean() <= 0.02, (what, float(diff.mean()))


@pytest.mark.parametrize('rect', R.RECTS, ids=lambda r: '%d_%d_%dx%d' % r)
def test_resample_against_the_reference(dev, rect):
    """Every size and both aspects of one rectangle, n = 3 and n = 1: fp32 within `bound` of float64 at every element and equal to the
    fp32 restatement bit for bit; bytes by the tie rule; the device rectangle == the host rectangle bit for bit."""
    from stabstitch2_amd import ops
    u8, f32 = _device_frames(dev)
    rdev = torch.tensor(rect, dtype=torch.int32, device=dev)
    empty = R.clip(rect, HC, WC) is None
    for size in R.SIZES:
        for aspect in R.ASPECTS:
            what = (rect, size, aspect)
            ref, seq, want8, bound = _reference(rect, size, aspect)
            got = ops.resample(f32, size, rect=rect, aspect=aspect)
            assert got.shape == (N, 3) + size and got.dtype == torch.float32
            g = got.cpu().numpy()
            err = float(np.abs(g.astype(np.float64) - ref).max())
            print('%s fp32 max|err| %.3e bound %.3e' % (what, err, bound))
            assert err <= bound, (what, err, bound)
            assert np.array_equal(g.view(np.int32), seq.view(np.int32)), (what, 'the fp32 restatement')
            _same(ops.resample(f32, size, rect=rdev, aspect=aspect), got, (what, 'device rect'))
            _same(ops.resample(f32[:1], size, rect=rdev, aspect=aspect), got[:1], (what, 'n = 1'))
            _same(ops.resample(f32[0], size, rect=rect, aspect=aspect), got[0], (what, 'one frame'))
            got8 = ops.resample(u8, size, rect=rect, aspect=aspect)
            assert got8.shape == (N,) + size + (3,) and got8.dtype == torch.uint8
            _bytes_gate(got8.cpu().numpy(), np.moveaxis(ref, 1, -1), want8, bound, what)
            assert torch.equal(ops.resample(u8, size, rect=rdev, aspect=aspect), got8), (what, 'device rect, bytes')
            assert torch.equal(ops.resample(u8[:1], size, rect=rect, aspect=aspect), got8[:1]), (what, 'n = 1, bytes')
            assert torch.equal(ops.resample(u8[0], size, rect=rdev, aspect=aspect), got8[0]), (what, 'one frame, bytes')
            if empty:
                assert not bool(got.any()) and not bool(got8.any()), what
            if size == (30, 50) and rect in ((5, 7, 30, 50), (13, 17, 30, 50)):
                y0, x0 = rect[:2]                                            # identity: bit for bit the crop
                _same(got, f32[:, :, y0:y0 + 30, x0:x0 + 50].contiguous(), (what, 'identity'))
                assert torch.equal(got8, u8[:, y0:y0 + 30, x0:x0 + 50]), (what, 'identity, bytes')
    if rect == (40, 60, 30, 50):                                             # the overhang is clipped in the kernel: == its clipped form
        for r in (rect, rdev):
            _same(ops.resample(f32, (16, 24), rect=r), ops.resample(f32, (16, 24), rect=(40, 60, 3, 7)), 'overhang')


def test_the_named_cases_take_both_paths():
    assert R.staged(STAGED_CASE[0], HC, WC, *STAGED_CASE[1], STAGED_CASE[2]) is True
    assert R.staged(DIRECT_CASE[0], HC, WC, *DIRECT_CASE[1], DIRECT_CASE[2]) is False
    assert max(R.tap_counts(DIRECT_CASE[0], HC, WC, *DIRECT_CASE[1], DIRECT_CASE[2])) >= 15
    assert STAGED_CASE[0] in R.RECTS and STAGED_CASE[1] in R.SIZES and DIRECT_CASE[1] in R.SIZES


def test_whole_frame_default_and_a_path_boundary(dev):
    """rect=None is the whole frame.  A 120 x 20 frame to 33 x 10 ('stretch': 3.6 x down the rows) has tiles on both sides of the
    staged path's row limit in ONE launch -- 16 output rows need 65 source rows, the last tile's single row needs 8 -- and equals the
    restatement like any other."""
    from stabstitch2_amd import ops
    u8, f32 = _device_frames(dev)
    _same(ops.resample(f32, (16, 24)), ops.resample(f32, (16, 24), rect=(0, 0, HC, WC)), 'rect=None')
    assert torch.equal(ops.resample(u8, (16, 24)), ops.resample(u8, (16, 24), rect=(0, 0, HC, WC)))
    tall = np.random.default_rng(1).integers(0, 256, size=(2, 3, 120, 20)).astype(np.float64)
    rect, size = (0, 0, 120, 20), (33, 10)
    assert R.staged(rect, 120, 20, *size, 'stretch') is None and R.staged(rect, 120, 20, *size, 'fill') is True
    x = T(tall.astype(np.float32)).to(dev)
    for aspect in R.ASPECTS:
        seq = R.resample_f32_sequential(tall, size, rect, aspect)
        ref = R.resample(tall, size, rect, aspect)
        got = ops.resample(x, size, rect=rect, aspect=aspect).cpu().numpy()
        assert np.abs(got - ref).max() <= R.bound(*R.tap_counts(rect, 120, 20, *size, aspect)), aspect
        assert np.array_equal(got.view(np.int32), seq.view(np.int32)), aspect


@pytest.mark.parametrize('size', [(30, 50), (16, 24), (2, 2), (16, 22)], ids=lambda s: '%dx%d' % s)
def test_nv12_and_strided_outputs_between_canaries(dev, size):
    """NV12 == ops.bgr_to_nv12(ops.resample(...)) byte for byte, into a surface with pitch > Wout; BGR into out= with a frame stride
    wider than a frame; nothing around either is written."""
    from stabstitch2_amd import ops
    u8, _ = _device_frames(dev)
    hout, wout = size
    canary = 0x5A
    for rect in (R.RECTS[0], R.RECTS[2], R.RECTS[6], R.RECTS[7], torch.tensor(R.RECTS[0], dtype=torch.int32, device=dev)):
        for aspect in R.ASPECTS:
            bgr = ops.resample(u8, size, rect=rect, aspect=aspect)
            want = ops.bgr_to_nv12(bgr)
            assert torch.equal(ops.resample(u8, size, rect=rect, aspect=aspect, out_format='nv12'), want)
            pitch, rows = wout + 6, hout // 2 * 3
            buf = torch.full((N, rows + 2, pitch), canary, device=dev, dtype=torch.uint8)
            surf = buf[:, 1:rows + 1, 2:2 + wout]
            res = ops.resample(u8, size, rect=rect, aspect=aspect, out=surf, out_format='nv12')
            assert res.data_ptr() == surf.data_ptr() and torch.equal(surf, want)
            keep = torch.ones_like(buf, dtype=torch.bool)
            keep[:, 1:rows + 1, 2:2 + wout] = False
            assert bool((buf[keep] == canary).all())
            if not torch.is_tensor(rect) and R.clip(rect, HC, WC) is None:
                assert bool((want[:, :hout] == 16).all()) and bool((want[:, hout:] == 128).all()) and not bool(bgr.any())
            frame = 3 * hout * wout
            for extra in (4, 7):                                             # dword stores where the stride allows, bytes where not
                flat = torch.full((N * (frame + extra) + 8,), canary, device=dev, dtype=torch.uint8)
                out = flat[4:4 + N * (frame + extra)].view(N, frame + extra)[:, :frame].view(N, hout, wout, 3)
                res = ops.resample(u8, size, rect=rect, aspect=aspect, out=out)
                assert res.data_ptr() == out.data_ptr() and torch.equal(out, bgr)
                gaps = flat[4:4 + N * (frame + extra)].view(N, frame + extra)[:, frame:]
                assert bool((gaps == canary).all()) and bool((flat[:4] == canary).all()) and bool((flat[-4:] == canary).all())
    one = ops.resample(u8[0], size, out_format='nv12')
    assert one.shape == (hout // 2 * 3, wout) and torch.equal(one, ops.bgr_to_nv12(ops.resample(u8[0], size)))
    for odd in ((31, 64), (32, 65), (69, 115), (4, 7)):
        with pytest.raises(ValueError, match='even'):
            ops.resample(u8, odd, out_format='nv12')
    with pytest.raises(ValueError, match='rect'):
        ops.resample(u8, size, rect=torch.tensor(R.RECTS[0], dtype=torch.int32))        # a rectangle on another device


# ================================================================================================ the offline routes
def _rs_names(names):
    return sorted(k for k in names if re.search(r'\brs_[a-z0-9_]+_kernel', k))


def _cv_names(names):
    return sorted(k for k in names if re.search(r'\bcv_[a-z]+_kernel', k))


@pytest.mark.parametrize('fusion', ['AVERAGE', 'MULTIBAND'])
def test_run_two_view_crop_to_size(dev, hip_nets, fusion):
    from stabstitch2_amd import ops, pipeline
    from test_gpu_linear_frames import _kernel_names
    from test_gpu_mbwarp import _clip, NFR
    c = _clip(dev)
    hr, lr, u8 = c['hr'], c['lr'], c['u8']
    size = (24, 64)
    kw = dict(fusion_mode=fusion, **(dict(bands=3) if fusion == 'MULTIBAND' else {}))
    full, hc, wc = pipeline.run_two_view(hr[0], hr[1], lr[0], lr[1], hip_nets, **kw)[:3]
    crop = pipeline.Crop(size=size)
    run = lambda cr: pipeline.run_two_view(hr[0], hr[1], lr[0], lr[1], hip_nets, crop=cr, **kw)       # noqa: E731
    got, h, w = run(crop)[:3]
    plain = pipeline.Crop()
    run(plain)
    assert (h, w) == size and got.shape == (NFR, 3) + size and crop.canvas == (hc, wc) and crop.rect == plain.rect
    assert crop.rect[2] * crop.rect[3] > 0
    _same(got, ops.resample(full, size, rect=crop.rect), 'ops.resample of the uncropped frames')
    _, names = _kernel_names(lambda: run(pipeline.Crop(size=size))[0])
    assert len(_rs_names(names)) == 1 and len(_cv_names(names)) == 4, (_rs_names(names), _cv_names(names))
    _, names = _kernel_names(lambda: run(pipeline.Crop())[0])
    assert not _rs_names(names) and len(_cv_names(names)) == 4
    res, names = _kernel_names(lambda: run(crop)[0])                          # the carried Crop: no coverage pass, one resample
    assert not _cv_names(names) and len(_rs_names(names)) == 1
    _same(res, got, 'a second call with the same Crop')
    stretched = pipeline.Crop(size=size, aspect='stretch')
    _same(run(stretched)[0], ops.resample(full, size, rect=crop.rect, aspect='stretch'), 'stretch')
    # uint8 in, uint8 out: the uint8 frames are what is resampled
    full8 = pipeline.run_two_view_u8(u8[0], u8[1], hip_nets, device=dev, **kw)[0]
    crop8 = pipeline.Crop(even=True, size=size)
    run8 = lambda cr: pipeline.run_two_view_u8(u8[0], u8[1], hip_nets, device=dev, crop=cr, **kw)      # noqa: E731
    got8, h8, w8 = run8(crop8)[:3]
    assert (h8, w8) == size and got8.dtype == torch.uint8 and got8.shape == (NFR,) + size + (3,)
    assert crop8.rect[2] % 2 == 0 and crop8.rect[3] % 2 == 0 and crop8.rect[2] * crop8.rect[3] > 0
    assert torch.equal(got8, ops.resample(full8, size, rect=crop8.rect))
    _, names = _kernel_names(lambda: run8(pipeline.Crop(size=size))[0])
    assert len(_rs_names(names)) == 1, _rs_names(names)
    _, names = _kernel_names(lambda: run8(pipeline.Crop())[0])
    assert not _rs_names(names)


def test_run_three_view_crop_to_size(dev, hip_nets):
    from stabstitch2_amd import ops, pipeline
    from test_gpu_mbwarp import _clip, NFR
    c = _clip(dev)
    hr, lr, u8 = c['hr'], c['lr'], c['u8']
    size = (24, 96)
    full, hc, wc = pipeline.run_three_view(hr[0], hr[1], hr[2], lr[0], lr[1], lr[2], hip_nets)[:3]
    crop = pipeline.Crop(size=size)
    got, h, w = pipeline.run_three_view(hr[0], hr[1], hr[2], lr[0], lr[1], lr[2], hip_nets, crop=crop)[:3]
    assert (h, w) == size and crop.canvas == (hc, wc) and crop.rect[2] * crop.rect[3] > 0 and got.shape == (NFR, 3) + size
    _same(got, ops.resample(full, size, rect=crop.rect), 'three views')
    full8 = pipeline.run_three_view_u8(u8[0], u8[1], u8[2], hip_nets, device=dev)[0]
    crop8 = pipeline.Crop(size=size)
    got8, h8, w8 = pipeline.run_three_view_u8(u8[0], u8[1], u8[2], hip_nets, device=dev, crop=crop8)[:3]
    assert (h8, w8) == size and torch.equal(got8, ops.resample(full8, size, rect=crop8.rect))


# ================================================================================================ the streaming stitchers
@pytest.mark.parametrize('views', [2, 3])
def test_to_size_of_the_streaming_stitchers(dev, hip_nets, views):
    """to_size(frame, size) == ops.resample(frame, size, rect=covered_rect()) after single pushes, push_many(4) and push_u8;
    covered_rect_device() == covered_rect(); the pushed frames do not depend on to_size being called; a held rectangle is used as
    held."""
    from stabstitch2_amd import ops, online
    from test_gpu_cover import _feed
    from test_gpu_multiband import _clip, SH, SW, PUSHES
    c = _clip(dev)
    cls = online.OnlineStitcher if views == 2 else online.ThreeViewOnlineStitcher
    size = (24, 64)
    st = cls(hip_nets, SH, SW, deterministic=True, track_coverage=True)
    assert st.covered_rect_device() is None
    frames, held = [], None
    for t in range(PUSHES):
        part = [c['hr'][v, t:t + 1] for v in range(views)] + [c['lr'][v, t:t + 1] for v in range(views)]
        out = st.push(*part)
        frames += out
        if out:
            rect = st.covered_rect()
            rd = st.covered_rect_device()
            assert rd.dtype == torch.int32 and rd.shape == (4,) and tuple(rd.cpu().tolist()) == rect
            assert tuple(st.covered_rect_device(even=True).cpu().tolist()) == st.covered_rect(even=True)
            held = rd if held is None else held
            _same(st.to_size(out[-1], size), ops.resample(out[-1], size, rect=rect), ('to_size', t))
    assert len(frames) == PUSHES and rect[2] * rect[3] > 0
    first = tuple(held.cpu().tolist())
    _same(st.to_size(frames[-1], size, rect=held, aspect='stretch'), ops.resample(frames[-1], size, rect=first, aspect='stretch'), 'held')
    if views == 3:
        return
    plain = _feed(cls(hip_nets, SH, SW, deterministic=True, track_coverage=True), c, views, ['p'] * PUSHES)
    for t in range(PUSHES):
        _same(frames[t], plain[t], ('a pushed frame with and without to_size', t))
    many = cls(hip_nets, SH, SW, deterministic=True, track_coverage=True)
    last = torch.stack(list(_feed(many, c, views, ['p'] * (PUSHES - 4) + [4])[-4:]))
    assert many.covered_rect() == rect
    got = many.to_size(last, size)
    assert got.shape == (4, 3) + size
    _same(got, ops.resample(last, size, rect=rect), 'push_many(4)')
    bytes_ = cls(hip_nets, SH, SW, deterministic=True, track_coverage=True)
    f8 = _feed(bytes_, c, views, ['p'] * PUSHES, u8=True)[-1]
    assert f8.dtype == torch.uint8 and bytes_.covered_rect() == rect
    got8 = bytes_.to_size(f8, size)
    assert torch.equal(got8, ops.resample(f8, size, rect=rect)) and got8.shape == size + (3,)
    assert torch.equal(bytes_.to_size(f8, size, out_format='nv12'), ops.bgr_to_nv12(got8))
    # every refusal
    with pytest.raises(ValueError, match='canvas'):
        st.to_size(frames[-1][:, :-1], size)
    with pytest.raises(ValueError, match='rect'):
        st.to_size(frames[-1], size, rect=rect)
    with pytest.raises(ValueError, match='size'):
        st.to_size(frames[-1], (24, 0))
    with pytest.raises(ValueError, match='aspect'):
        st.to_size(frames[-1], size, aspect='fit')
    with pytest.raises(ValueError, match='nv12'):
        st.to_size(frames[-1], size, out_format='nv12')
    off = cls(hip_nets, SH, SW, deterministic=True)
    with pytest.raises(ValueError, match='track_coverage'):
        off.to_size(frames[-1], size)
    with pytest.raises(ValueError, match='track_coverage'):
        off.covered_rect_device()
