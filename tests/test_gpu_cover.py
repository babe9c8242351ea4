"""Coverage bitmaps and the largest covered rectangle on the GPU (libstabstitch_cover.so): the coverage against the mask
planes the renders already write, the rectangle against tests/cover_ref.py, the offline routes' crop= against the slice of the same
call without it, and the streaming stitchers' track_coverage against a state advanced by hand.  Every comparison is exact."""
import gc
import re

import numpy as np
import pytest
import torch

import cover_ref as C
import mbwarp_ref as WR
from test_gpu_mbwarp import _case, _same
from test_gpu_parity import dev, hip_nets  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
T = torch.from_numpy

# 43 x 67: a second word of 3 bits, tile rows past the canvas; 3 x 9: waves that return whole; 8 x 64 and 9 x 65: a word boundary
# exactly at, and one past, the edge; 81 x 129: eleven tile rows, three words
CANVASES = [(43, 67), (3, 9), (8, 64), (9, 65), (81, 129)]


@pytest.fixture(autouse=True)
def _no_garbage_inside_a_capture():
    """A stitcher that became cyclic garbage still owns HIP graphs: collect between the tests, where nothing captures."""
    gc.collect()
    yield
    gc.collect()


def _unpack(bitmap, wc, pad=False):
    """int64 [..., hc, W64] on the device -> bool [..., hc, wc] (pad: all 64 W64 columns)."""
    bits = (bitmap[..., None] >> torch.arange(64, device=bitmap.device)) & 1
    out = bits.reshape(bitmap.shape[:-1] + (bitmap.shape[-1] * 64,)).bool()
    return out if pad else out[..., :wc]


def _rect(t):
    return tuple(int(v) for v in t.cpu().tolist())


# ================================================================================================ coverage == the mask planes
@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('views', [2, 3])
@pytest.mark.parametrize('canvas', CANVASES, ids=lambda c: '%dx%d' % c)
def test_coverage_equals_the_mask_planes(dev, canvas, views, n):
    """ops.coverage, unpacked == (multiband_warp's plane 4 >= min_mask).any(view), NORMAL and FAST, min_mask 0.5 and 1.0; pad bits
    zero.  Item 0's spline pushes part of its view off the canvas; on the canvases larger than the frame uncovered pixels occur, and
    under FAST mask values on both sides of 0.5 strictly inside (0, 1)."""
    from stabstitch2_amd import ops
    hc, wc = canvas
    h, w = WR.FRAME
    clips8, clips, sd, Tk = _case(dev, n, views, canvas)
    for mode in ('NORMAL', 'FAST'):
        mask = ops.multiband_warp(clips, sd, Tk, hc, wc, mode)[:, :, 4]                  # [n, V, hc, wc]
        for min_mask in (0.5, 1.0):
            got = ops.coverage(sd, Tk, h, w, hc, wc, mode, min_mask)
            assert got.shape == (n, hc, C.words(wc)) and got.dtype == torch.int64
            want = (mask >= min_mask).any(1)
            full = _unpack(got, wc, pad=True)
            assert torch.equal(full[..., :wc], want), (mode, min_mask)
            assert not bool(full[..., wc:].any()), (mode, min_mask, 'pad bits')
            assert np.array_equal(C.unpack(got.cpu().numpy(), wc), want.cpu().numpy())  # the reference's layout is the library's
        if hc > h:
            cov = (mask >= 0.5).any(1)
            assert bool(cov.any()) and bool((~cov).any()), mode
            if mode == 'FAST':
                assert bool(((mask > 0) & (mask < 0.5)).any()) and bool(((mask >= 0.5) & (mask < 1)).any())
    if n == 1:                                   # one frame without the frame axis
        _same(ops.coverage(sd[0], Tk[0], h, w, hc, wc), ops.coverage(sd, Tk, h, w, hc, wc), 'one frame')


def test_coverage_equals_the_mask_plane_of_tps_warp(dev):
    from stabstitch2_amd import ops
    n, views, (hc, wc) = 3, 2, CANVASES[0]
    h, w = WR.FRAME
    clips8, clips, sd, Tk = _case(dev, n, views, (hc, wc))
    U = torch.stack(clips, 1).reshape(n * views, 3, h, w).contiguous()
    for mode in ('NORMAL', 'FAST'):
        plane = ops.tps_warp(U, sd.view(n * views, 63, 2), Tk.view(n * views, 2, 66), hc, wc, mode, with_mask=True)[:, 3]
        want = (plane.view(n, views, hc, wc) >= 0.5).any(1)
        assert torch.equal(_unpack(ops.coverage(sd, Tk, h, w, hc, wc, mode), wc), want), mode


@pytest.mark.parametrize('canvas', [(43, 67), (9, 65)], ids=lambda c: '%dx%d' % c)
def test_coverage_between_canaries_and_accumulate(dev, canvas):
    """Both forms write their words and nothing around them; accumulate over 3 frames == the AND of the 3 per-frame bitmaps == three
    accumulate calls of one frame; a word that is zero stays zero."""
    from stabstitch2_amd import ops, _cover as CV, _hip as H
    n, views, (hc, wc) = 3, 3, canvas
    h, w = WR.FRAME
    _, _, sd, Tk = _case(dev, n, views, canvas)
    w64 = C.words(wc)
    pad, canary = 4 * w64 + 5, 0x5A5A5A5A5A5A5A5A
    for mode in ('NORMAL', 'FAST'):
        want = ops.coverage(sd, Tk, h, w, hc, wc, mode)
        size = n * hc * w64
        buf = torch.full((pad + size + pad,), canary, device=dev, dtype=torch.int64)
        CV.call('ssc_coverage', H.dptr(sd), H.dptr(Tk), H.dptr(buf[pad:pad + size], dtype=torch.int64), n, views, h, w, hc, wc,
                ops.MODES[mode], 0.5, 0, H.stream())
        assert bool((buf[:pad] == canary).all()) and bool((buf[pad + size:] == canary).all()), mode
        assert torch.equal(buf[pad:pad + size].view(n, hc, w64), want), mode
        both = want[0] & want[1] & want[2]
        size = hc * w64
        buf = torch.full((pad + size + pad,), canary, device=dev, dtype=torch.int64)
        fresh = ops.coverage_state(hc, wc, dev)
        assert bool(_unpack(fresh.bitmap, wc, pad=True)[:, :wc].all())
        assert not bool(_unpack(fresh.bitmap, wc, pad=True)[:, wc:].any())
        buf[pad:pad + size] = fresh.bitmap.reshape(-1)
        CV.call('ssc_coverage', H.dptr(sd), H.dptr(Tk), H.dptr(buf[pad:pad + size], dtype=torch.int64), n, views, h, w, hc, wc,
                ops.MODES[mode], 0.5, 1, H.stream())
        assert bool((buf[:pad] == canary).all()) and bool((buf[pad + size:] == canary).all()), mode
        assert torch.equal(buf[pad:pad + size].view(hc, w64), both), mode
        state = ops.coverage_update(fresh, sd, Tk, h, w, mode)
        assert state is fresh and torch.equal(state.bitmap, both), mode
        single = ops.coverage_state(hc, wc, dev)
        for f in range(n):
            ops.coverage_update(single, sd[f], Tk[f], h, w, mode)
        assert torch.equal(single.bitmap, both), mode
        zero = ops.CoverageState(torch.zeros_like(both), fresh.ws, hc, wc)
        assert not bool(ops.coverage_update(zero, sd, Tk, h, w, mode).bitmap.any())


# ================================================================================================ the rectangle == the reference
def _patterns(hc, wc):
    rs = np.random.RandomState(1000 * hc + wc)
    yy, xx = np.indices((hc, wc))
    out = {'ones': np.ones((hc, wc), bool), 'zeros': np.zeros((hc, wc), bool), 'checkerboard': (yy + xx) % 2 == 0,
           'staircase': C.staircase(hc, wc)}
    for d in (0.5, 0.9, 0.99):
        out['random%g' % d] = rs.rand(hc, wc) < d
    hole = np.ones((hc, wc), bool)
    hole[hc // 2, wc // 2] = False
    out['hole'] = hole
    ell = np.zeros((hc, wc), bool)
    ell[:, :max(1, wc // 3)] = True
    ell[hc - max(1, hc // 3):, :] = True
    out['L'] = ell
    return out


def test_rect_breaks_ties_as_the_reference_does(dev):
    """Two equal areas side by side, one above the other, and a 2 x 6 against a 3 x 4 from one corner."""
    from stabstitch2_amd import ops
    for name, (m, want) in C.ties().items():
        assert C.rect(m) == want
        assert _rect(ops.covered_rect(T(C.pack(m)).to(dev), wc=m.shape[1])) == want, name


@pytest.mark.parametrize('size', [(2, 2), (2, 64), (3, 9), (43, 67), (81, 129), (200, 300)], ids=lambda c: '%dx%d' % c)
def test_rect_equals_the_reference(dev, size):
    """ops.covered_rect on uploaded bitmaps == cover_ref.rect, component for component, even on and off, with the pad bits set to
    ones and the workspace between canaries."""
    from stabstitch2_amd import ops, _cover as CV
    hc, wc = size
    need = int(CV.lib().ssc_rect_workspace_bytes(hc, wc))
    padmask = T(C.pack(np.zeros((hc, wc), bool) | True) ^ np.int64(-1)).to(dev)          # ones exactly in the pad bits
    fence = 64
    cases = _patterns(hc, wc)
    for name, m in cases.items():
        want = C.rect(m)
        bm = T(C.pack(m)).to(dev) | padmask
        assert wc % 64 == 0 or bool(_unpack(bm, wc, pad=True)[:, wc:].all())
        for even in (False, True):
            buf = torch.full((fence + need + fence,), 0xA5, device=dev, dtype=torch.uint8)
            got = ops.covered_rect(bm, even, wc=wc, ws=buf[fence:fence + need])
            assert got.dtype == torch.int32 and got.shape == (4,) and got.is_cuda
            assert _rect(got) == C._even(want, even), (name, even, _rect(got), want)
            assert bool((buf[:fence] == 0xA5).all()) and bool((buf[fence + need:] == 0xA5).all()), name
        assert _rect(ops.covered_rect(bm[None], wc=wc)) == want, name
        state = ops.CoverageState(bm, torch.empty(need, device=dev, dtype=torch.uint8), hc, wc)
        assert _rect(ops.covered_rect(state)) == want, name


def _staircase_rect(hc, wc):
    """cover_ref.rect(staircase(hc, wc)) in closed form: the rectangles are (y0, 0, hc - y0, y0 * wc // hc)."""
    y0 = np.arange(hc)
    area = (hc - y0) * (y0 * wc // hc)
    best = int(np.argmax(area))                  # (the first maximum: the smallest y0)
    return (best, 0, hc - best, best * wc // hc)


@pytest.mark.parametrize('size', [(785, 1995), (2, 8192)], ids=lambda c: '%dx%d' % c)
def test_rect_finishes_on_a_whole_canvas(dev, size):
    """All ones and the staircase at 720p two-view size, and at the widest canvas the library takes (the largest tree)."""
    from stabstitch2_amd import ops
    hc, wc = size
    assert _staircase_rect(12, 70) == C.rect(C.staircase(12, 70)) and _staircase_rect(43, 67) == C.rect(C.staircase(43, 67))
    state = ops.coverage_state(hc, wc, dev)
    assert _rect(ops.covered_rect(state)) == (0, 0, hc, wc)
    assert _rect(ops.covered_rect(state, even=True)) == (0, 0, hc - (hc & 1), wc - (wc & 1))
    stairs = ops.CoverageState(T(C.pack(C.staircase(hc, wc))).to(dev), state.ws, hc, wc)
    assert _rect(ops.covered_rect(stairs)) == _staircase_rect(hc, wc)


# ================================================================================================ the offline routes
def _cv_names(names):
    return sorted(k for k in names if re.search(r'\bcv_[a-z]+_kernel', k))


@pytest.mark.parametrize('fusion', ['AVERAGE', 'MULTIBAND'])
def test_run_two_view_crop(dev, hip_nets, fusion):
    from stabstitch2_amd import ops, pipeline
    from test_gpu_linear_frames import _kernel_names
    from test_gpu_mbwarp import _clip, SH, SW, NFR
    c = _clip(dev)
    hr, lr, u8 = c['hr'], c['lr'], c['u8']
    kw = dict(fusion_mode=fusion, **(dict(bands=3) if fusion == 'MULTIBAND' else {}))
    full, hc, wc, m1, m2 = pipeline.run_two_view(hr[0], hr[1], lr[0], lr[1], hip_nets, **kw)
    crop = pipeline.Crop()
    got, h, w, _, _ = pipeline.run_two_view(hr[0], hr[1], lr[0], lr[1], hip_nets, crop=crop, **kw)
    y0, x0, rh, rw = crop.rect
    assert (h, w) == (rh, rw) and crop.canvas == (hc, wc) and got.shape == (NFR, 3, h, w) and h * w > 0
    assert all(type(v) is int for v in crop.rect)
    _same(got.contiguous(), full[:, :, y0:y0 + h, x0:x0 + w].contiguous(), 'the window of the same call without crop')
    # the rectangle is the reference's on the AND of the frames' coverage, and what pipeline.covered_rect says
    _, _, src, Tk = pipeline.render_plan([m1, m2], SH, SW)
    cov = C.unpack(ops.coverage(src, Tk, SH, SW, hc, wc).cpu().numpy(), wc).all(0)
    assert crop.rect == C.rect(cov)
    assert pipeline.covered_rect([m1, m2], SH, SW) == crop.rect
    assert pipeline.covered_rect([m1, m2], SH, SW, even=True) == C.rect(cov, even=True)
    # every pixel inside it is covered in every frame, by the mask planes; and the canvas has a border that is not
    mask = ops.multiband_warp([hr[0], hr[1]], src, Tk, hc, wc)[:, :, 4]
    assert bool((mask[:, :, y0:y0 + h, x0:x0 + w] >= 0.5).any(1).all()) and not bool((mask >= 0.5).any(1).all())
    # the first call's Crop again: no kernel of the library, the same window
    again = lambda: pipeline.run_two_view(hr[0], hr[1], lr[0], lr[1], hip_nets, crop=crop, **kw)[0]       # noqa: E731
    again()
    res, names = _kernel_names(again)
    assert not _cv_names(names) and crop.rect == (y0, x0, rh, rw), _cv_names(names)
    _same(res.contiguous(), got.contiguous(), 'a second call with the same Crop')
    _, names = _kernel_names(lambda: pipeline.run_two_view(hr[0], hr[1], lr[0], lr[1], hip_nets, crop=pipeline.Crop(), **kw)[0])
    assert len(_cv_names(names)) == 4 and sum('cv_coverage_kernel' in k for k in names) == 1, _cv_names(names)
    _, names = _kernel_names(lambda: pipeline.run_two_view(hr[0], hr[1], lr[0], lr[1], hip_nets, crop=None, **kw)[0])
    assert not _cv_names(names)
    with pytest.raises(ValueError, match='canvas'):
        bad = pipeline.Crop()
        bad.rect = (0, 0, hc + 1, 4)
        pipeline.render_frames([hr[0], hr[1]], [m1, m2], crop=bad, **kw)
    # uint8 in, uint8 out
    full8, hc8, wc8 = pipeline.run_two_view_u8(u8[0], u8[1], hip_nets, device=dev, **kw)[:3]
    crop8 = pipeline.Crop(even=True)
    got8, h8, w8 = pipeline.run_two_view_u8(u8[0], u8[1], hip_nets, device=dev, crop=crop8, **kw)[:3]
    a, b, rh8, rw8 = crop8.rect
    assert (h8, w8) == (rh8, rw8) and rh8 % 2 == 0 and rw8 % 2 == 0 and crop8.canvas == (hc8, wc8) and got8.dtype == torch.uint8
    assert torch.equal(got8, full8[:, a:a + h8, b:b + w8, :]) and got8.shape == (NFR, h8, w8, 3) and h8 * w8 > 0


def test_run_three_view_crop(dev, hip_nets):
    from stabstitch2_amd import ops, pipeline
    from test_gpu_mbwarp import _clip, SH, SW, NFR
    c = _clip(dev)
    hr, lr, u8 = c['hr'], c['lr'], c['u8']
    full, hc, wc, m1, mid, m3 = pipeline.run_three_view(hr[0], hr[1], hr[2], lr[0], lr[1], lr[2], hip_nets)
    crop = pipeline.Crop()
    got, h, w = pipeline.run_three_view(hr[0], hr[1], hr[2], lr[0], lr[1], lr[2], hip_nets, crop=crop)[:3]
    y0, x0, rh, rw = crop.rect
    assert (h, w) == (rh, rw) and crop.canvas == (hc, wc) and h * w > 0
    _same(got.contiguous(), full[:, :, y0:y0 + h, x0:x0 + w].contiguous(), 'three views')
    _, _, src, Tk = pipeline.render_plan([m1, mid, m3], SH, SW, prescaled=True)
    cov = C.unpack(ops.coverage(src, Tk, SH, SW, hc, wc).cpu().numpy(), wc).all(0)
    assert crop.rect == C.rect(cov) and pipeline.covered_rect([m1, mid, m3], SH, SW, prescaled=True) == crop.rect
    full8 = pipeline.run_three_view_u8(u8[0], u8[1], u8[2], hip_nets, device=dev)[0]
    crop8 = pipeline.Crop()
    got8, h8, w8 = pipeline.run_three_view_u8(u8[0], u8[1], u8[2], hip_nets, device=dev, crop=crop8)[:3]
    a, b, _, _ = crop8.rect
    assert torch.equal(got8, full8[:, a:a + h8, b:b + w8, :]) and got8.shape == (NFR, h8, w8, 3) and h8 * w8 > 0


# ================================================================================================ the streaming stitchers
class _Rendered:
    """(src, T, hc, wc) of every frame a stitcher renders, in order: copies taken where the fused renders are launched."""

    def __init__(self, monkeypatch):
        from stabstitch2_amd import ops
        self.frames = []
        for name in ('render_average', 'render_average_u8', 'render_average_clip', 'render_average_clip_u8'):
            monkeypatch.setattr(ops, name, self._wrap(getattr(ops, name)))

    def _wrap(self, real):
        def render(imgs, source, Tk, hc, wc, *a, **k):
            src = source if source.dim() == 4 else source[None]
            for f in range(src.shape[0]):
                self.frames.append((src[f].clone(), Tk.reshape(src.shape[0], -1, 2, 66)[f].clone(), hc, wc))
            return real(imgs, source, Tk, hc, wc, *a, **k)
        return render

    def state(self, ops, st, h, w, since=0):
        """The coverage of frames[since:] on st's canvas, advanced by hand."""
        state = ops.coverage_state(st.hc, st.wc, st.dev)
        for src, Tk, hc, wc in self.frames[since:]:
            assert (hc, wc) == (st.hc, st.wc)
            ops.coverage_update(state, src, Tk, h, w, st.warp_mode)
        return state


def _feed(st, c, views, schedule, u8=False):
    """schedule: 'p' = one push, an int k = push_many of k -> the frames handed out."""
    out, t = [], 0
    for s in schedule:
        k = 1 if s == 'p' else s
        if u8:
            out += st.push_u8(*[c['u8'][v, t] for v in range(views)]) if s == 'p' else st.push_many_u8(*[c['u8'][v, t:t + k] for v in range(views)])
        else:
            part = [c['hr'][v, t:t + k] for v in range(views)] + [c['lr'][v, t:t + k] for v in range(views)]
            out += st.push(*part) if s == 'p' else st.push_many(*part)
        t += k
    return out


def _check_state(ops, st, rec, h, w, frames, since=0):
    want = rec.state(ops, st, h, w, since)
    assert st.coverage_frames == frames == len(rec.frames) - since
    assert torch.equal(st._cover.bitmap, want.bitmap)
    rect = st.covered_rect()
    assert rect == _rect(ops.covered_rect(want)) == C.rect(C.unpack(want.bitmap.cpu().numpy(), st.wc))
    assert st.covered_rect(even=True) == _rect(ops.covered_rect(want, even=True))
    assert rect[2] * rect[3] > 0 and not bool(_unpack(want.bitmap, st.wc).all())      # a rectangle, and a border outside it
    return want


@pytest.mark.parametrize('views', [2, 3])
def test_track_coverage_follows_every_frame_handed_out(dev, hip_nets, monkeypatch, views):
    """The window fill and five steady pushes: the frames equal those of a stitcher without tracking, the state equals one advanced by
    hand from the (src, T) of every frame rendered; push_many(4) leaves the state of 4 pushes, push_u8 that of push, use_graph=False
    that of the captured step."""
    from stabstitch2_amd import ops, online
    from test_gpu_multiband import _clip, SH, SW, PUSHES
    c = _clip(dev)
    cls = online.OnlineStitcher if views == 2 else online.ThreeViewOnlineStitcher
    plain = _feed(cls(hip_nets, SH, SW, deterministic=True), c, views, ['p'] * PUSHES)
    rec = _Rendered(monkeypatch)
    st = cls(hip_nets, SH, SW, deterministic=True, track_coverage=True)
    assert st.covered_rect() is None and st.coverage_frames == 0
    got = _feed(st, c, views, ['p'] * PUSHES)
    assert len(got) == len(plain) == PUSHES
    for t in range(PUSHES):
        _same(got[t], plain[t], ('frame', t))
    want = _check_state(ops, st, rec, SH, SW, PUSHES)
    if views == 3:
        return
    many = cls(hip_nets, SH, SW, deterministic=True, track_coverage=True)
    _feed(many, c, views, ['p'] * (PUSHES - 4) + [4])
    assert many.coverage_frames == PUSHES and torch.equal(many._cover.bitmap, want.bitmap)
    bytes_ = cls(hip_nets, SH, SW, deterministic=True, track_coverage=True)
    _feed(bytes_, c, views, ['p'] * PUSHES, u8=True)
    assert bytes_.coverage_frames == PUSHES and torch.equal(bytes_._cover.bitmap, want.bitmap)
    eager = cls(hip_nets, SH, SW, deterministic=True, use_graph=False, track_coverage=True)
    _feed(eager, c, views, ['p'] * PUSHES)
    assert eager.coverage_frames == PUSHES and torch.equal(eager._cover.bitmap, want.bitmap)
    assert many.covered_rect() == bytes_.covered_rect() == eager.covered_rect() == st.covered_rect()


def test_a_recapture_growth_starts_a_fresh_state(dev, hip_nets, monkeypatch):
    """The drifting stream of test_streaming_canvas_overflow_is_detected_and_grown under grow='recapture': the state and the count
    stand for the frames handed out since the last growth, on the grown canvas."""
    from stabstitch2_amd import ops, online, synth
    from test_gpu_round5 import _push_drifting
    hr, lr = synth.make_clip(16, 360, 480, seed=0)
    hrd = [[f.to(dev) for f in v] for v in hr]
    lrd = [[f.to(dev) for f in v] for v in lr]
    rec = _Rendered(monkeypatch)
    st = online.OnlineStitcher(hip_nets, 360, 480, grow='recapture', track_coverage=True)
    sizes = []
    _push_drifting(st, hip_nets, hrd, lrd, 36, record=lambda t, s: (torch.cuda.synchronize(), sizes.append((s.hc, s.wc))))
    assert st.canvas_epoch >= 1 and len(rec.frames) == 36
    since = max(i for i in range(36) if rec.frames[i][2:] != rec.frames[i - 1][2:] and i > 0)
    assert 7 <= since < 36 and rec.frames[since][2:] == (st.hc, st.wc) != rec.frames[0][2:]
    _check_state(ops, st, rec, 360, 480, 36 - since, since)


def test_refusals(dev, hip_nets):
    from stabstitch2_amd import online
    SH, SW = 180, 320
    for make in (lambda: online.MultiOnlineStitcher(hip_nets, SH, SW, streams=2, track_coverage=True),
                 lambda: online.PipelinedOnlineStitcher(hip_nets, SH, SW, track_coverage=True),
                 lambda: online.PipelinedMultiOnlineStitcher(hip_nets, SH, SW, streams=2, track_coverage=True),
                 lambda: online.PipelinedThreeViewOnlineStitcher(hip_nets, SH, SW, track_coverage=True),
                 lambda: online.OnlineStitcher(hip_nets, SH, SW, meshes_only=True, track_coverage=True),
                 lambda: online.OnlineStitcher(hip_nets, SH, SW, grow='refit', viewport=(204, 500), track_coverage=True)):
        with pytest.raises(ValueError):
            make()
