"""The direct MULTIBAND warp on the GPU (libstabstitch_mbwarp.so) and exposure compensation on the offline routes: the
warp against ss_tps_warp_mask_nchw on the stacked planes, its gains against the fp32 product, canaries, the launches, render_multiband
and the pipeline's routes against their restatement in `ops` calls, and what the feature is for -- a darker camera pulled up before
the seam.  Every comparison is exact."""
import functools
import re

import numpy as np
import pytest
import torch

import exposure_ref as E
import mbwarp_ref as WR
import sweep_inputs as G
from stabstitch2_amd import synth
from test_gpu_parity import dev, hip_nets  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
T = torch.from_numpy
F = np.float32


def _same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape)
    if a.dtype == torch.float32:                 # bit for bit: -0 is not +0
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    assert torch.equal(a, b), what


@functools.lru_cache(maxsize=None)
def _host_case(n, views, canvas, seed=21):
    return WR.warp_inputs(n, views, canvas[0], canvas[1], seed=seed)


def _case(dev, n, views, canvas, seed=21):
    """-> (clips uint8 V x [n,h,w,3], clips fp32 V x [n,3,h,w] of the same values, source [n,V,63,2], T [n,V,2,66])"""
    from stabstitch2_amd import ops
    frames, src, tgt = _host_case(n, views, canvas, seed)
    clips8 = [T(np.ascontiguousarray(frames[:, v])).to(dev) for v in range(views)]
    clips = [c.permute(0, 3, 1, 2).float().contiguous() for c in clips8]
    sd = T(src).to(dev)
    Tk = ops.tps_solve(sd.view(n * views, 63, 2), T(tgt).to(dev)).view(n, views, 2, 66)
    return clips8, clips, sd, Tk


def _two_step(ops, imgs, sd, Tk, hc, wc, mode):
    n, v = sd.shape[:2]
    return ops.tps_warp(ops.multiband_stack(imgs), sd.view(n * v, 63, 2), Tk.view(n * v, 2, 66), hc, wc, mode, with_mask=True).view(n, v, 5, hc, wc)


# ================================================================================================ the warp
@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('views', [2, 3])
@pytest.mark.parametrize('canvas', WR.CANVASES, ids=lambda c: '%dx%d' % c)
def test_plain_warp_equals_stack_and_warp(dev, canvas, views, n):
    """multiband_warp(gains=None) == tps_warp(multiband_stack(imgs), .., with_mask=True) on all five planes, NORMAL and FAST, from
    fp32 planes and from uint8 frames.  Item 0's spline pushes part of its view off the canvas, and on the canvases larger than the
    frame part of the canvas lies outside every view: clamped taps (NORMAL) and skipped taps (FAST) both occur."""
    from stabstitch2_amd import ops
    hc, wc = canvas
    clips8, clips, sd, Tk = _case(dev, n, views, canvas)
    for mode in ('NORMAL', 'FAST'):
        want = _two_step(ops, clips, sd, Tk, hc, wc, mode)
        for name, imgs in (('fp32', clips), ('uint8', clips8)):
            got = ops.multiband_warp(imgs, sd, Tk, hc, wc, mode)
            assert got.shape == (n, views, 5, hc, wc)
            for p in range(5):
                _same(got[:, :, p], want[:, :, p], (mode, name, 'plane', p))
        _same(_two_step(ops, clips8, sd, Tk, hc, wc, mode), want, (mode, 'the two-step path from uint8'))
        if hc > WR.FRAME[0]:
            mask = want[:, :, 4]
            assert bool((mask < 0.5).any()) and bool((mask >= 0.5).any()), mode
            assert bool((mask[0, 0] >= 0.5).any()) and float(want[0, 0, 3].max()) > 1.0          # the shifted view is still on the canvas
    if n == 1:                                   # one frame without the frame axis
        got = ops.multiband_warp([c[0] for c in clips8], sd[0], Tk[0], hc, wc, 'NORMAL')
        _same(got, _two_step(ops, clips, sd, Tk, hc, wc, 'NORMAL')[0], 'one frame')


@pytest.mark.parametrize('views', [2, 3])
@pytest.mark.parametrize('u8', [False, True], ids=['fp32', 'uint8'])
def test_gains_scale_and_clamp_the_colour_planes(dev, u8, views):
    """Planes 0..2 == minimum(g * P_plain, 255) in fp32 on the device, planes 3 and 4 == P_plain; gains of exactly 1 reproduce
    P_plain (inputs in 0..255: the clamp never bites); three frames with three gain rows == three single-frame calls."""
    from stabstitch2_amd import ops
    n, (hc, wc) = 3, WR.CANVASES[0]
    clips8, clips, sd, Tk = _case(dev, n, views, (hc, wc))
    imgs = clips8 if u8 else clips
    g = T(WR.gains_case(n, views)).to(dev)
    assert float(g.min()) >= 0.5 and float(g.max()) == 2.0 and len({tuple(r) for r in g.view(-1, 3).tolist()}) == n * views
    for mode in ('NORMAL', 'FAST'):
        plain = ops.multiband_warp(imgs, sd, Tk, hc, wc, mode)
        got = ops.multiband_warp(imgs, sd, Tk, hc, wc, mode, gains=g)
        want = torch.minimum(g[:, :, :, None, None] * plain[:, :, :3], torch.tensor(255.0, device=dev))
        assert float((g[:, :, :, None, None] * plain[:, :, :3]).max()) > 255.0 and float(want.max()) == 255.0
        _same(got[:, :, :3], want, (mode, 'colour'))
        _same(got[:, :, 3:], plain[:, :, 3:], (mode, 'weight and mask'))
        _same(ops.multiband_warp(imgs, sd, Tk, hc, wc, mode, gains=torch.ones_like(g)), plain, (mode, 'unit gains'))
        for f in range(n):
            one = ops.multiband_warp([c[f] for c in imgs], sd[f], Tk[f], hc, wc, mode, gains=g[f])
            _same(one, got[f], (mode, 'frame', f))
            _same(ops.multiband_warp([c[f:f + 1] for c in imgs], sd[f:f + 1], Tk[f:f + 1], hc, wc, mode, gains=g[f:f + 1])[0], got[f],
                  (mode, 'clip of one', f))


@pytest.mark.parametrize('gains', [False, True], ids=['plain', 'gains'])
def test_canaries_and_a_nan_plane_in_front_of_the_frames(dev, gains):
    """P between canaries: nothing in front of it or behind it is written, all of it is.  Every view's frames sit behind (and in front
    of) a canvas-sized stretch of NaN: no tap reads it."""
    from stabstitch2_amd import ops, _mbwarp as W, _hip as H
    n, views, (hc, wc) = 2, 3, WR.CANVASES[0]
    h, w = WR.FRAME
    clips8, clips, sd, Tk = _case(dev, n, views, (hc, wc))
    g = T(WR.gains_case(n, views)).to(dev) if gains else None
    pad, size = hc * wc, n * views * 5 * hc * wc
    for mode in ('NORMAL', 'FAST'):
        want = ops.multiband_warp(clips, sd, Tk, hc, wc, mode, gains=g)
        fenced = []
        for c in clips:
            big = torch.full((pad + c.numel() + pad,), float('nan'), device=dev)
            big[pad:pad + c.numel()] = c.reshape(-1)
            fenced.append(big[pad:pad + c.numel()].view(n, 3, h, w))
        canary = 12345.678
        buf = torch.full((pad + size + pad,), canary, device=dev)
        buf[pad:pad + size] = float('nan')
        W.call('ssw_multiband_warp', H.ptr_array(fenced), H.dptr(sd), H.dptr(Tk), H.dptr(g, True), H.dptr(buf[pad:pad + size]), n, views, h, w,
               hc, wc, ops.MODES[mode], H.stream())
        assert bool((buf[:pad] == canary).all()) and bool((buf[pad + size:] == canary).all()), mode
        assert not bool(torch.isnan(buf).any()), mode
        _same(buf[pad:pad + size].view(n, views, 5, hc, wc), want, mode)
        # the uint8 entry: P between the same canaries
        buf[:] = canary
        W.call('ssw_multiband_warp_u8', H.ptr_array(clips8, dtype=torch.uint8), H.dptr(sd), H.dptr(Tk), H.dptr(g, True),
               H.dptr(buf[pad:pad + size]), n, views, h, w, hc, wc, ops.MODES[mode], H.stream())
        assert bool((buf[:pad] == canary).all()) and bool((buf[pad + size:] == canary).all()), mode
        _same(buf[pad:pad + size].view(n, views, 5, hc, wc), want, (mode, 'uint8'))


def test_launch_witness(dev):
    """The smallest calls under torch.profiler launch the four instantiations of mbwarp_ref.reach() and nothing else of the new
    library, one launch each; render_multiband(gains=None) launches nothing of it, render_multiband(gains=) exactly one.  Should the
    profiler report names without template arguments, base names are matched instead and the test says so in its output."""
    from stabstitch2_amd import ops
    from test_gpu_linear_frames import _kernel_names
    hc, wc = WR.CANVASES[1]
    clips8, clips, sd, Tk = _case(dev, 1, 2, (hc, wc))
    g = T(WR.gains_case(1, 2)).to(dev)
    ours = lambda names: [k for k in names if re.search(r'\bmw_[a-z]+_kernel', k)]        # noqa: E731
    launched = []
    for imgs in (clips, clips8):
        for gains in (None, g):
            fn = lambda: ops.multiband_warp(imgs, sd, Tk, hc, wc, 'NORMAL', gains=gains)      # noqa: E731
            fn()                                 # (once outside the profiler: module load)
            names = _kernel_names(fn)[1]
            assert len(names) == 1 and len(ours(names)) == 1, names
            launched += names
    if all('<' in k for k in launched):
        got = sorted(G.instantiation_key(k) for k in launched)
        print('\n[launch witness] matched by template arguments: %s' % got)
        assert got == sorted(WR.reach()), got
    else:
        print('\n[launch witness] the profiler reports no template arguments; matched by base name: %s' % launched)
        assert {re.search(r'\b(mw_[a-z]+_kernel)', k).group(1) for k in launched} == {k.split('<')[0] for k in WR.reach()}
    big = WR.CANVASES[0]
    clips8, clips, sd, Tk = _case(dev, 1, 2, big)
    for imgs in (clips, clips8):
        plain = lambda: ops.render_multiband(imgs, sd, Tk, big[0], big[1], 'NORMAL', 2)      # noqa: E731
        plain()
        names = _kernel_names(plain)[1]
        assert not ours(names) and any('tps_warp_kernel' in k for k in names), names
        with_gains = lambda: ops.render_multiband(imgs, sd, Tk, big[0], big[1], 'NORMAL', 2, gains=g)      # noqa: E731
        with_gains()
        names = _kernel_names(with_gains)[1]
        assert len(ours(names)) == 1 and not any('tps_warp_kernel' in k or 'ingest' in k for k in names), names


@pytest.mark.parametrize('views', [2, 3])
@pytest.mark.parametrize('u8', [False, True], ids=['fp32', 'uint8'])
def test_render_multiband_with_gains(dev, u8, views):
    """render_multiband(gains=g) == multiband_blend of the torch-built P (minimum(g * P_plain, 255) on the two-step path's planes),
    with the geometric seam and with the DP seam run on that P from an equal state; a clip of three and its frames one by one."""
    from stabstitch2_amd import ops
    n, (hc, wc), bands = 3, WR.CANVASES[2], 3
    clips8, clips, sd, Tk = _case(dev, n, views, (hc, wc))
    imgs = clips8 if u8 else clips
    g = T(WR.gains_case(n, views, seed=1)).to(dev)
    P = _two_step(ops, clips, sd, Tk, hc, wc, 'NORMAL')
    P[:, :, :3] = torch.minimum(g[:, :, :, None, None] * P[:, :, :3], torch.tensor(255.0, device=dev))
    want = ops.multiband_blend(P.clone(), bands, u8=u8)
    got = ops.render_multiband(imgs, sd, Tk, hc, wc, 'NORMAL', bands, gains=g)
    _same(got, want, 'geometric')
    assert not torch.equal(got, ops.render_multiband(imgs, sd, Tk, hc, wc, 'NORMAL', bands))
    cell = ops.seam_cell(hc, wc)
    s_ref, s_got, s_one = (ops.seam_state(views, hc, wc, cell, dev) for _ in range(3))
    want_dp = ops.multiband_blend(ops.multiband_seam(P.clone(), state=s_ref), bands, u8=u8)
    got_dp = ops.render_multiband(imgs, sd, Tk, hc, wc, 'NORMAL', bands, seam='dp', seam_state=s_got, gains=g)
    _same(got_dp, want_dp, 'dp')
    assert torch.equal(s_ref, s_got) and bool(s_got.any())
    for f in range(n):
        one = ops.render_multiband([c[f] for c in imgs], sd[f], Tk[f], hc, wc, 'NORMAL', bands, seam='dp', seam_state=s_one, gains=g[f])
        _same(one, got_dp[f], ('dp frame', f))
    assert torch.equal(s_one, s_got)


# ================================================================================================ the pipeline
SH, SW, NFR = 180, 320, 9                  # nine frames: MULTIBAND goes in a chunk of eight and one of one
SCALE = (0.8, 0.9, 1.1)                    # the last view's channels: a camera that disagrees on exposure
_runs = {}


def _clip(dev):
    if 'clip' not in _runs:
        from stabstitch2_amd import ops, pipeline
        hr, _ = synth.make_clip_device(NFR, SH, SW, seed=4, views=3, device=dev)
        hr = hr.clone()
        hr[1] = hr[1] * torch.tensor(SCALE, device=dev).view(1, 3, 1, 1)
        u8 = hr.permute(0, 1, 3, 4, 2).round().clamp(0, 255).to(torch.uint8).contiguous()
        loaded = [ops.ingest_u8(u8[v], pipeline.LR_H, pipeline.LR_W) for v in range(3)]
        _runs['clip'] = dict(u8=u8, hr=torch.stack([x[0] for x in loaded]), lr=torch.stack([x[1] for x in loaded]))
    return _runs['clip']


def _restated(dev, views, src, Tk, hc, wc, fusion, seam=None, frames=None, state=None, params=None):
    """The frames of a clip with exposure compensation as `ops` calls, frame by frame, one exposure state (and one seam state) run
    through them: exposure_update on the frame's footprint row, then the render with gains=."""
    from stabstitch2_amd import ops, pipeline
    n = src.shape[0]
    fp = ops.render_footprints(src, Tk, SH, SW, hc, wc)
    st = ops.exposure_state(dev) if state is None else state
    seam_state = ops.seam_state(len(views), hc, wc, ops.seam_cell(hc, wc), dev) if seam == 'dp' else None
    out, gains = [], []
    for i in (range(n) if frames is None else frames):
        g = ops.exposure_update([v[i:i + 1] for v in views], fp[i:i + 1], hc, wc, st, params, 'NORMAL')
        gains.append(g)
        imgs = [v[i] for v in views]
        if fusion in ('AVERAGE', 'FEATHER'):
            out.append(ops.render_average(imgs, src[i], Tk[i], hc, wc, 'NORMAL', footprint=fp[i] if pipeline.SKIP_OUTSIDE else None, gains=g,
                                          fusion=fusion))
        elif fusion == 'LINEAR':
            out.append(ops.render_linear_clip([v[i:i + 1] for v in views], src[i:i + 1], Tk[i:i + 1], hc, wc, 'NORMAL', gains=g)[0])
        else:
            kw = dict(seam='dp', seam_state=seam_state) if seam == 'dp' else {}
            out.append(ops.render_multiband(imgs, src[i], Tk[i], hc, wc, 'NORMAL', 3, gains=g, **kw))
    return torch.stack(out), torch.cat(gains), st


FUSIONS = [('AVERAGE', None), ('FEATHER', None), ('LINEAR', None), ('MULTIBAND', 'geometric'), ('MULTIBAND', 'dp')]


@pytest.mark.parametrize('fusion,seam', FUSIONS, ids=['%s-%s' % f if f[1] else f[0] for f in FUSIONS])
def test_run_two_view_with_exposure_equals_its_restatement(dev, hip_nets, fusion, seam):
    """run_two_view(exposure=True) == exposure_update + the ops render with gains= on the returned meshes, frame by frame; the list
    route and a clip rendered in two render_frames calls with one exposure_state= (and one seam_state=) equal the single call; the
    gains moved; exposure=None is the call without the keyword."""
    from stabstitch2_amd import ops, pipeline
    c = _clip(dev)
    hr, lr = c['hr'], c['lr']
    kw = dict(fusion_mode=fusion)
    if fusion == 'MULTIBAND':
        kw.update(bands=3, seam=seam)
    frames, hc, wc, m1, m2 = pipeline.run_two_view(hr[0], hr[1], lr[0], lr[1], hip_nets, exposure=True, **kw)
    _, _, src, Tk = pipeline.render_plan([m1, m2], SH, SW)
    want, gains, st = _restated(dev, [hr[0], hr[1]], src, Tk, hc, wc, fusion, seam)
    assert frames.shape == (NFR, 3, hc, wc)
    for i in range(NFR):
        _same(frames[i], want[i], (fusion, seam, 'frame', i))
    assert float((gains - 1).abs().max()) > 0.01
    plain = pipeline.run_two_view(hr[0], hr[1], lr[0], lr[1], hip_nets, **kw)[0]
    _same(pipeline.run_two_view(hr[0], hr[1], lr[0], lr[1], hip_nets, exposure=None, **kw)[0], plain, 'exposure=None')
    assert float((plain - frames).abs().max()) > 1.0
    # lists of separate frames
    lists = pipeline.render_frames([[hr[v][i] for i in range(NFR)] for v in range(2)], [m1, m2], exposure=True, **kw)[0]
    _same(lists, frames, 'lists')
    # two calls, one state
    es = ops.exposure_state(dev)
    more = dict(seam_state=ops.seam_state(2, hc, wc, ops.seam_cell(hc, wc), dev)) if seam == 'dp' else {}
    box = pipeline.canvas_bbox([m1, m2], SH, SW)
    parts = [pipeline.render_frames([hr[0][a:b], hr[1][a:b]], [m1[:, a:b].contiguous(), m2[:, a:b].contiguous()], bbox=box, size=(hc, wc),
                                    exposure=True, exposure_state=es, **kw, **more)[0] for a, b in ((0, 4), (4, NFR))]
    _same(torch.cat(parts), frames, 'two calls')
    assert torch.equal(es, st)
    # ExposureParams are passed on
    p = ops.ExposureParams(alpha=0.5, min_nodes=4)
    tuned = pipeline.render_frames([hr[0], hr[1]], [m1, m2], exposure=p, **kw)[0]
    _same(tuned[NFR - 1], _restated(dev, [hr[0], hr[1]], src, Tk, hc, wc, fusion, seam, params=p)[0][NFR - 1], 'params')


def test_linear_without_the_clip_render_goes_through_the_frames_render(dev, hip_nets, monkeypatch):
    """SS_LINEAR_CLIP=0: the per-frame chain has no gains, so a clip with exposure renders through ss_render_linear_frames_gains at
    n = 1 -- the same frames as the clip render, by other kernels."""
    from stabstitch2_amd import pipeline
    from test_gpu_linear_frames import _kernel_names
    c = _clip(dev)
    hr, lr = c['hr'], c['lr']
    run = lambda: pipeline.run_two_view(hr[0], hr[1], lr[0], lr[1], hip_nets, fusion_mode='LINEAR', exposure=True)[0]      # noqa: E731
    want, names = _kernel_names(run)
    assert any('lb_clip_warp_kernel' in k for k in names) and not any('lb_frames_warp_kernel' in k for k in names), names
    monkeypatch.setattr(pipeline, 'LINEAR_CLIP', False)
    got, names = _kernel_names(run)
    assert any('lb_frames_warp_kernel' in k for k in names) and not any('lb_clip_warp_kernel' in k for k in names), names
    _same(got, want, 'frames render')


@pytest.mark.parametrize('fusion', ['AVERAGE', 'LINEAR', 'MULTIBAND'])
def test_run_two_view_u8_with_exposure(dev, hip_nets, fusion):
    """run_two_view_u8(exposure=True) == canvas_to_u8 of the fp32 route on the converted frames."""
    from stabstitch2_amd import ops, pipeline
    c = _clip(dev)
    kw = dict(fusion_mode=fusion, **(dict(bands=3) if fusion == 'MULTIBAND' else {}))
    u8, hc, wc = pipeline.run_two_view_u8(c['u8'][0], c['u8'][1], hip_nets, device=dev, exposure=True, **kw)[:3]
    f32, hc2, wc2 = pipeline.run_two_view(c['hr'][0], c['hr'][1], c['lr'][0], c['lr'][1], hip_nets, exposure=True, **kw)[:3]
    assert (hc, wc) == (hc2, wc2) and u8.dtype == torch.uint8
    _same(u8, ops.canvas_to_u8(f32), fusion)
    assert not torch.equal(u8, pipeline.run_two_view_u8(c['u8'][0], c['u8'][1], hip_nets, device=dev, **kw)[0])


@pytest.mark.parametrize('fusion', ['AVERAGE', 'MULTIBAND'])
def test_run_three_view_with_exposure_equals_its_restatement(dev, hip_nets, fusion):
    from stabstitch2_amd import ops, pipeline
    c = _clip(dev)
    hr, lr = c['hr'], c['lr']
    kw = dict(fusion_mode=fusion, **(dict(bands=3) if fusion == 'MULTIBAND' else {}))
    frames, hc, wc, m1, mid, m3 = pipeline.run_three_view(hr[0], hr[1], hr[2], lr[0], lr[1], lr[2], hip_nets, exposure=True, **kw)
    _, _, src, Tk = pipeline.render_plan([m1, mid, m3], SH, SW, prescaled=True)
    want, gains, _ = _restated(dev, [hr[0], hr[1], hr[2]], src, Tk, hc, wc, fusion)
    for i in range(NFR):
        _same(frames[i], want[i], (fusion, 'frame', i))
    assert gains.shape == (NFR, 3, 3) and float((gains - 1).abs().max()) > 0.01
    u8 = pipeline.run_three_view_u8(c['u8'][0], c['u8'][1], c['u8'][2], hip_nets, device=dev, exposure=True, **kw)[0]
    _same(u8, ops.canvas_to_u8(frames), (fusion, 'uint8'))


# ================================================================================================ what it is for
def test_a_darker_camera_is_pulled_up_before_the_seam(dev):
    """Two views of one constant picture, view 0 at 120 and view 1 at 96, side by side with an overlap; MULTIBAND at bands = 0 is the
    hard seam composite.  Without exposure the two sides of the seam differ by 24.  With exposure=True the gains equal
    tests/exposure_ref.py's float64 statement (targets within 2 fp32 ulp of the float64 solve of the device's statistics, the smoothed
    gains bit for bit its fp32 walk), and the step is under half of the uncompensated one -- a condition, not a measurement: by the
    closed form of DESIGN.md 7c for means 120 and 96 under the defaults (lambda = 1e4) the gains are 0.9143 and 1.0685 and the step
    is 7.1, a ratio of 0.30.  At bands = 5 with the DP seam the same clip renders and stays within [0, 255]."""
    from stabstitch2_amd import ops, pipeline
    n, h, w = 3, 24, 41
    height, rects = 96.0, [(0.0, 160.0), (96.0, 256.0)]
    meshes = [T(m).to(dev) for m in WR.side_by_side_meshes(n, rects, height)]
    clips = [torch.full((n, 3, h, w), val, device=dev) for val in (120.0, 96.0)]
    kw = dict(fusion_mode='MULTIBAND', prescaled=True)
    plain, hc, wc = pipeline.render_frames(clips, meshes, bands=0, **kw)
    assert (hc, wc) == (96, 256)
    left, right = (slice(None), slice(None), slice(8, hc - 8), slice(100, 120)), (slice(None), slice(None), slice(8, hc - 8), slice(136, 156))
    assert float((plain[left] - 120).abs().max()) < 1e-3 and float((plain[right] - 96).abs().max()) < 1e-3
    step0 = float((plain[left].mean() - plain[right].mean()).abs())
    assert abs(step0 - 24.0) < 1e-3
    st = ops.exposure_state(dev)
    out = pipeline.render_frames(clips, meshes, bands=0, exposure=True, exposure_state=st, **kw)[0]
    # the gains, against the float64 statement
    _, _, src, Tk = pipeline.render_plan(meshes, h, w, prescaled=True)
    fp = ops.render_footprints(src, Tk, h, w, hc, wc)
    st2 = ops.exposure_state(dev)
    gains, diag = ops.exposure_update(clips, fp, hc, wc, st2, None, 'NORMAL', want_diag=True)
    assert torch.equal(st, st2)
    gains, diag = gains.cpu().numpy(), diag.cpu().numpy()
    s, started = np.ones((2, 3), F), False
    for f in range(n):
        d = diag[f]
        stats = {(0, 1): (int(d[0]), d[1:9:3].copy(), d[2:9:3].copy())}
        assert stats[(0, 1)][0] >= E.DEFAULTS['min_nodes']
        want, kept = E.targets(stats, 2)
        got_t = d[27:33].reshape(2, 3)
        ulps = np.max(np.abs(got_t.astype(F).astype(np.float64) - want.astype(F).astype(np.float64)) / np.spacing(np.abs(want.astype(F))))
        assert kept and bool(d[36]) and ulps <= 2.0, (f, got_t, want)
        s, started = E.smooth(s, started, got_t, kept, E.DEFAULTS['alpha'])
        assert np.array_equal(gains[f], s), (f, gains[f], s)
    assert np.abs(gains[:, 0] - 0.9143).max() < 2e-4 and np.abs(gains[:, 1] - 1.0685).max() < 2e-4, gains
    # the frames are those gains applied, and the step has shrunk
    _same(out, ops.render_multiband(clips, src, Tk, hc, wc, 'NORMAL', 0, gains=T(gains).to(dev)), 'the gains applied')
    step = float((out[left].mean() - out[right].mean()).abs())
    print('\n[capability] gains %s / %s, step %.3f -> %.3f (ratio %.3f)' % (gains[0, 0], gains[0, 1], step0, step, step / step0))
    assert step < 0.5 * step0, (step, step0)
    full = pipeline.render_frames(clips, meshes, bands=5, seam='dp', exposure=True, **kw)[0]
    assert full.shape == (n, 3, hc, wc) and bool(torch.isfinite(full).all()) and float(full.min()) >= 0.0 and float(full.max()) <= 255.0
