"""The offline clip path's route table (pipeline._render_clip): which entry points a render_frames / render_frames_u8
call launches, in order, for every fusion mode x {clip tensors, lists of frames} x {exposure off, on} -- literal lists written down
from the code before the routes were gathered in one place -- and the identities the table must keep: a clip equals its frames
rendered one by one through `ops` with one exposure state and one seam state run through them, lists equal clips, two calls with
the states carried over equal one.  Then the uint8-in / uint8-out callers: one ss_ingest_u8 per view, the bytes of the fp32 route.
Every comparison is exact."""
import functools

import numpy as np
import pytest
import torch

import mbwarp_ref as WR
from stabstitch2_amd import synth
from test_gpu_mbwarp import _same, SH, SW
from test_gpu_parity import dev, hip_nets  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
T = torch.from_numpy

N, BANDS, HEIGHT = 3, 2, 40.0
RECTS = [(0.0, 56.0), (24.0, 80.0), (48.0, 104.0)]        # neighbours overlap by 32 canvas pixels
GAIN = (1.0, 0.8, 1.15)                                  # cameras that disagree on exposure

# render_plan: the canvas box, the control points, the splines (per view, per view, once)
PLAN = {2: 'ss_mesh_bbox ss_mesh_bbox ss_mesh_normalize_views ss_mesh_normalize_views ss_tps_solve_shared_target',
        3: 'ss_mesh_bbox ss_mesh_bbox ss_mesh_bbox ss_mesh_normalize_views ss_mesh_normalize_views ss_mesh_normalize_views '
           'ss_tps_solve_shared_target'}
CHAIN = {2: 'ss_tps_warp_views ss_linear_blend ' * 3,
         3: 'ss_tps_warp_views ss_linear_blend ss_mask_union ss_linear_blend ' * 3}
# (mode, clip tensors | lists, exposure) -> what follows the plan; N = 3 frames, LINEAR_CLIP_FRAMES = MULTIBAND_FRAMES = 2: two chunks
ROUTES = {
    ('AVERAGE', 'clip', False): 'ss_render_footprints ss_render_average_clip',
    ('AVERAGE', 'clip', True): 'ss_render_footprints ss_exposure_update ss_render_average_clip_gains',
    ('AVERAGE', 'list', False): 'ss_render_footprints ss_render_average ss_render_average ss_render_average',
    ('AVERAGE', 'list', True): 'ss_render_footprints ' + 'ss_exposure_update ss_render_average_gains ' * 3,
    ('LINEAR', 'clip', False): 'ss_render_linear_clip ss_render_linear_clip',
    ('LINEAR', 'clip', True): 'ss_render_footprints ss_exposure_update ss_render_linear_clip_gains ss_render_linear_clip_gains',
    ('LINEAR', 'list', False): CHAIN[2],
    ('LINEAR', 'list', True): 'ss_render_footprints ' + 'ss_exposure_update ss_render_linear_frames_gains ' * 3,
    ('LINEAR-frames', 'clip', False): CHAIN[2],
    ('LINEAR-frames', 'clip', True): 'ss_render_footprints ss_exposure_update ' + 'ss_render_linear_frames_gains ' * 3,
    ('MULTIBAND', 'clip', False): 'ss_tps_warp_mask_nchw ssb_multiband_blend ' * 2,
    ('MULTIBAND', 'clip', True): 'ss_render_footprints ss_exposure_update ' + 'ssw_multiband_warp ssb_multiband_blend ' * 2,
    ('MULTIBAND', 'list', False): 'ss_tps_warp_mask_nchw ssb_multiband_blend ' * 3,
    ('MULTIBAND', 'list', True): 'ss_render_footprints ' + 'ss_exposure_update ssw_multiband_warp ssb_multiband_blend ' * 3,
    ('MULTIBAND-dp', 'clip', False): 'ss_tps_warp_mask_nchw ssm_multiband_seam ssb_multiband_blend ' * 2,
    ('MULTIBAND-dp', 'clip', True): 'ss_render_footprints ss_exposure_update ' + 'ssw_multiband_warp ssm_multiband_seam ssb_multiband_blend ' * 2,
    ('MULTIBAND-dp', 'list', False): 'ss_tps_warp_mask_nchw ssm_multiband_seam ssb_multiband_blend ' * 3,
    ('MULTIBAND-dp', 'list', True): 'ss_render_footprints ' + 'ss_exposure_update ssw_multiband_warp ssm_multiband_seam ssb_multiband_blend ' * 3,
}
for _form in ('clip', 'list'):
    for _on in (False, True):
        ROUTES[('FEATHER', _form, _on)] = ROUTES[('AVERAGE', _form, _on)]          # the same entry points, another bit of `mode`
        ROUTES[('LINEAR-frames', 'list', _on)] = ROUTES[('LINEAR', 'list', _on)]     # lists never take the clip render
        ROUTES[('OTHER', 'list', _on)] = ROUTES[('LINEAR', 'list', _on)]
# a fusion name that is none of the four renders as LINEAR, as the reference's `else` does: with gains through the clip render, without
# them through the per-frame chain even from clip tensors
ROUTES[('OTHER', 'clip', False)] = CHAIN[2]
ROUTES[('OTHER', 'clip', True)] = ROUTES[('LINEAR', 'clip', True)]
ROUTES_U8 = {
    ('AVERAGE', False): 'ss_render_footprints ss_render_average_clip_u8',
    ('AVERAGE', True): 'ss_render_footprints ss_exposure_update ss_render_average_clip_u8_gains',
    ('LINEAR', False): 'ss_render_linear_clip_u8 ss_render_linear_clip_u8',
    ('LINEAR', True): 'ss_render_footprints ss_exposure_update ss_render_linear_clip_u8_gains ss_render_linear_clip_u8_gains',
}
MODES = ['AVERAGE', 'FEATHER', 'LINEAR', 'LINEAR-frames', 'MULTIBAND', 'MULTIBAND-dp', 'OTHER']


class _Spy:
    """The entry-point names that go through _hip.launch (all six bindings do) while `record` runs a call."""

    def __init__(self, monkeypatch):
        from stabstitch2_amd import _hip
        self.names, real = None, _hip.launch

        def launch(lib, name, args, host_ok=False):
            if self.names is not None:
                self.names.append(name)
            return real(lib, name, args, host_ok)
        monkeypatch.setattr(_hip, 'launch', launch)

    def record(self, fn):
        self.names = []
        try:
            return fn(), self.names
        finally:
            self.names = None


@pytest.fixture
def spy(monkeypatch):
    from stabstitch2_amd import pipeline
    monkeypatch.setattr(pipeline, 'MULTIBAND_FRAMES', 2)      # N = 3: every chunk loop crosses a boundary and ends on a short chunk
    monkeypatch.setattr(pipeline, 'LINEAR_CLIP_FRAMES', 2)
    return _Spy(monkeypatch)


@functools.lru_cache(maxsize=None)
def _host(views):
    """N frames of `views` views of WR.FRAME, every frame and view different, view k's colours scaled by GAIN[k]; meshes that put the
    views side by side on overlapping rectangles, each frame's moved a little further right."""
    h, w = WR.FRAME
    rs = np.random.RandomState(77)
    base = rs.randint(24, 200, (N, h, w, 3)).astype(np.float64)
    frames = [np.clip(np.rint(base * GAIN[k] + rs.randint(-6, 7, base.shape)), 0, 255).astype(np.uint8) for k in range(views)]
    meshes = []
    for k, m in enumerate(WR.side_by_side_meshes(N, RECTS[:views], HEIGHT)):
        m = m.copy()
        for i in range(N):
            m[0, i, :, :, 0] += np.float32(1.5 * i * (k + 1))
        meshes.append(m)
    return frames, meshes


def _inputs(dev, views):
    """-> (uint8 clips V x [N,h,w,3], fp32 clips V x [N,3,h,w] of the same values, meshes V x [1,N,7,9,2] in canvas pixels)"""
    frames, meshes = _host(views)
    clips8 = [T(f).to(dev) for f in frames]
    return clips8, [c.permute(0, 3, 1, 2).float().contiguous() for c in clips8], [T(m).to(dev) for m in meshes]


def _mode_kw(mode, monkeypatch):
    from stabstitch2_amd import pipeline
    if mode == 'LINEAR-frames':
        monkeypatch.setattr(pipeline, 'LINEAR_CLIP', False)
    fusion = mode.split('-')[0]
    kw = dict(fusion_mode=fusion, prescaled=True)
    if fusion == 'MULTIBAND':
        kw.update(bands=BANDS, seam='dp' if mode.endswith('dp') else 'geometric')
    return fusion, kw


def _frame_by_frame(dev, views, src, Tk, hc, wc, fusion, dp, params):
    """The clip as `ops` calls, frame by frame, one exposure state and one seam state run through the frames: exposure_update on the
    frame's footprint row, then the one-frame render with gains=.  -> (frames, exposure state, seam state | None)"""
    from stabstitch2_amd import ops, pipeline
    h, w = WR.FRAME
    u8 = views[0].dtype == torch.uint8
    fused = ops.fused_render(fusion)
    fp = ops.render_footprints(src, Tk, h, w, hc, wc) if (params is not None or (pipeline.SKIP_OUTSIDE and fused)) else None
    st = ops.exposure_state(dev)
    ss = ops.seam_state(len(views), hc, wc, ops.seam_cell(hc, wc), dev) if dp else None
    out = []
    for i in range(N):
        one = [c[i:i + 1] for c in views]
        g = None if params is None else ops.exposure_update(one, fp[i:i + 1], hc, wc, st, params, 'NORMAL')
        if fused:
            render = ops.render_average_u8 if u8 else ops.render_average
            out.append(render([c[i] for c in views], src[i], Tk[i], hc, wc, 'NORMAL', footprint=fp[i] if pipeline.SKIP_OUTSIDE else None,
                              gains=g, fusion=fusion))
        elif fusion != 'MULTIBAND':
            out.append(ops.render_linear_clip(one, src[i:i + 1], Tk[i:i + 1], hc, wc, 'NORMAL', gains=g)[0])
        else:
            kw = dict(seam='dp', seam_state=ss) if dp else {}
            out.append(ops.render_multiband([c[i] for c in views], src[i], Tk[i], hc, wc, 'NORMAL', BANDS, gains=g, **kw))
    return torch.stack(out), st, ss


def _split(render, clips, meshes, box, size, dp, params, dev):
    """The clip in two calls, frames [0, 1) and [1, N), the states carried over -> (frames, exposure state, seam state | None)"""
    from stabstitch2_amd import ops
    es = ops.exposure_state(dev) if params is not None else None
    ss = ops.seam_state(len(clips), size[0], size[1], ops.seam_cell(*size), dev) if dp else None
    more = dict(exposure=params, exposure_state=es) if params is not None else {}
    if dp:
        more['seam_state'] = ss
    parts = [render([c[a:b] for c in clips], [m[:, a:b].contiguous() for m in meshes], bbox=box, size=size, **more)[0]
             for a, b in ((0, 1), (1, N))]
    return torch.cat(parts), es, ss


def _check_cell(dev, spy, views, mode, exposure, monkeypatch):
    from stabstitch2_amd import ops, pipeline
    fusion, kw = _mode_kw(mode, monkeypatch)
    dp = mode.endswith('dp')
    params = ops.ExposureParams(alpha=0.5, min_nodes=2) if exposure else None
    _, clips, meshes = _inputs(dev, views)
    h, w = WR.FRAME
    hc, wc, src, Tk = pipeline.render_plan(meshes, h, w, prescaled=True)          # (also builds the cached rigid mesh outside the records)
    more = dict(exposure=params) if exposure else {}
    assert views == 2 or (mode, exposure) == ('LINEAR-frames', False)          # three views: the chain, from clips and from lists
    (got, hc2, wc2), names = spy.record(lambda: pipeline.render_frames(clips, meshes, **kw, **more))
    assert (hc2, wc2) == (hc, wc) and got.shape == (N, 3, hc, wc)
    want = (PLAN[views] + ' ' + (CHAIN[3] if views == 3 else ROUTES[(mode, 'clip', exposure)])).split()
    assert names == want, (mode, 'clip', exposure, names)
    lists = [[c[i] for i in range(N)] for c in clips]
    (got_l, _, _), names = spy.record(lambda: pipeline.render_frames(lists, meshes, **kw, **more))
    want = (PLAN[views] + ' ' + (CHAIN[3] if views == 3 else ROUTES[(mode, 'list', exposure)])).split()
    assert names == want, (mode, 'list', exposure, names)
    ref, st, ss = _frame_by_frame(dev, clips, src, Tk, hc, wc, fusion, dp, params)
    _same(got, ref, (mode, 'clip == frame by frame'))
    _same(got_l, got, (mode, 'lists == clip'))
    box = pipeline.canvas_bbox(meshes, h, w, prescaled=True)
    two, es, ss2 = _split(lambda c, m, **k: pipeline.render_frames(c, m, **kw, **k), clips, meshes, box, (hc, wc), dp, params, dev)
    _same(two, got, (mode, 'two calls == one'))
    if exposure:
        assert torch.equal(es, st) and float((es[:9] - 1).abs().max()) > 0.01      # the gains moved
        assert float((got - pipeline.render_frames(clips, meshes, **kw)[0]).abs().max()) > 1.0
    if dp:
        assert torch.equal(ss2, ss) and bool(ss.any())


@pytest.mark.parametrize('exposure', [False, True], ids=['plain', 'exposure'])
@pytest.mark.parametrize('mode', MODES)
def test_render_frames_routes(dev, spy, monkeypatch, mode, exposure):
    """Two views: the launches of the clip route and of the list route are the table's; clip == frame by frame through `ops` == lists
    == two calls with the states carried over, bit for bit; the exposure state and the seam state end where the restatement's do."""
    _check_cell(dev, spy, 2, mode, exposure, monkeypatch)


def test_linear_frame_chain_with_three_views(dev, spy, monkeypatch):
    """Three views where the route differs: the per-frame chain unites the first two masks and blends a second time."""
    _check_cell(dev, spy, 3, 'LINEAR-frames', False, monkeypatch)


@pytest.mark.parametrize('exposure', [False, True], ids=['plain', 'exposure'])
@pytest.mark.parametrize('fusion', ['AVERAGE', 'LINEAR'])
def test_render_frames_u8_routes(dev, spy, monkeypatch, fusion, exposure):
    """render_frames_u8: the table's launches (LINEAR takes the clip render whatever LINEAR_CLIP says); == the one-frame uint8 renders
    of `ops` with one exposure state == canvas_to_u8 of render_frames == two calls with the state carried over."""
    from stabstitch2_amd import ops, pipeline
    params = ops.ExposureParams(alpha=0.5, min_nodes=2) if exposure else None
    clips8, clips, meshes = _inputs(dev, 2)
    h, w = WR.FRAME
    hc, wc, src, Tk = pipeline.render_plan(meshes, h, w, prescaled=True)
    kw = dict(fusion_mode=fusion, prescaled=True)
    more = dict(exposure=params) if exposure else {}
    (got, hc2, wc2), names = spy.record(lambda: pipeline.render_frames_u8(clips8, meshes, **kw, **more))
    assert (hc2, wc2) == (hc, wc) and got.shape == (N, hc, wc, 3) and got.dtype == torch.uint8
    assert names == (PLAN[2] + ' ' + ROUTES_U8[(fusion, exposure)]).split(), (fusion, exposure, names)
    ref, st, _ = _frame_by_frame(dev, clips8, src, Tk, hc, wc, fusion, False, params)
    _same(got, ref, (fusion, 'uint8 clip == frame by frame'))
    _same(got, ops.canvas_to_u8(pipeline.render_frames(clips, meshes, **kw, **more)[0]), (fusion, 'uint8 == canvas_to_u8 of fp32'))
    box = pipeline.canvas_bbox(meshes, h, w, prescaled=True)
    two, es, _ = _split(lambda c, m, **k: pipeline.render_frames_u8(c, m, **kw, **k), clips8, meshes, box, (hc, wc), False, params, dev)
    _same(two, got, (fusion, 'two calls == one'))
    if exposure:
        assert torch.equal(es, st) and float((es[:9] - 1).abs().max()) > 0.01
    if fusion == 'LINEAR':
        monkeypatch.setattr(pipeline, 'LINEAR_CLIP', False)
        (again, _, _), names2 = spy.record(lambda: pipeline.render_frames_u8(clips8, meshes, **kw, **more))
        assert names2 == names
        _same(again, got, 'LINEAR_CLIP off')


def test_render_frames_u8_still_refuses_multiband(dev):
    from stabstitch2_amd import pipeline
    clips8, _, meshes = _inputs(dev, 2)
    with pytest.raises(ValueError, match="fusion must be 'AVERAGE' or 'FEATHER', got 'MULTIBAND'"):
        pipeline.render_frames_u8(clips8, meshes, fusion_mode='MULTIBAND', prescaled=True)


# ================================================================================================ uint8 in, uint8 out
_runs = {}


def _video(dev):
    """The smallest clip the networks take: WINDOW frames of three views at test_gpu_mbwarp's size, as decoded uint8 frames and as
    what ONE ingest per view makes of them."""
    if 'video' not in _runs:
        from stabstitch2_amd import ops, pipeline
        hr, _ = synth.make_clip_device(pipeline.WINDOW, SH, SW, seed=4, views=3, device=dev)
        u8 = hr.permute(0, 1, 3, 4, 2).round().clamp(0, 255).to(torch.uint8).contiguous()
        loaded = [ops.ingest_u8(u8[v], pipeline.LR_H, pipeline.LR_W) for v in range(3)]
        _runs['video'] = u8, [x[0] for x in loaded], [x[1] for x in loaded]
    return _runs['video']


def _fusion_kw(fusion):
    return dict(fusion_mode=fusion, **(dict(bands=3) if fusion == 'MULTIBAND' else {}))


@pytest.mark.parametrize('fusion', ['AVERAGE', 'MULTIBAND'])
@pytest.mark.parametrize('views', [2, 3])
def test_u8_runs_ingest_once_per_view(dev, hip_nets, spy, fusion, views):
    """run_two_view_u8 / run_three_view_u8, fused uint8 render (AVERAGE) and fp32 route + canvas_to_u8 (MULTIBAND): ONE ss_ingest_u8
    per view -- never one for the hr planes and one for the lr frames -- and the bytes of canvas_to_u8 of the fp32 run."""
    from stabstitch2_amd import ops, pipeline
    u8, hr, lr = _video(dev)
    assert pipeline._u8_fused(fusion) == (fusion == 'AVERAGE')
    kw = _fusion_kw(fusion)
    if views == 2:
        res, names = spy.record(lambda: pipeline.run_two_view_u8(u8[0], u8[1], hip_nets, device=dev, **kw))
        f32 = pipeline.run_two_view(hr[0], hr[1], lr[0], lr[1], hip_nets, **kw)
    else:
        res, names = spy.record(lambda: pipeline.run_three_view_u8(u8[0], u8[1], u8[2], hip_nets, device=dev, **kw))
        f32 = pipeline.run_three_view(hr[0], hr[1], hr[2], lr[0], lr[1], lr[2], hip_nets, **kw)
    assert names.count('ss_ingest_u8') == views, [k for k in names if 'ingest' in k]
    assert names.count('ss_canvas_to_u8') == (0 if fusion == 'AVERAGE' else 1)
    assert res[1:3] == f32[1:3] and res[0].dtype == torch.uint8
    _same(res[0], ops.canvas_to_u8(f32[0]), (fusion, views))


@pytest.mark.parametrize('fused', [True, False], ids=['u8-fused', 'fp32-route'])
def test_host_clip_runner_ingests_once_per_view(dev, hip_nets, spy, monkeypatch, fused):
    """Two clips through HostClipRunner.run under both settings of U8_FUSED: one ss_ingest_u8 per view and clip, the same bytes."""
    from stabstitch2_amd import ops, pipeline
    monkeypatch.setattr(pipeline, 'U8_FUSED', fused)
    u8, hr, lr = _video(dev)
    pairs = [(0, 1), (1, 2)]
    host = [tuple(u8[k].cpu() for k in p) for p in pairs]
    runner = pipeline.HostClipRunner(hip_nets, device=dev)
    out, names = spy.record(lambda: [(v.clone(), hc, wc) for v, hc, wc in runner.run(iter(host))])
    torch.cuda.synchronize(dev)
    assert len(out) == 2 and names.count('ss_ingest_u8') == 4, [k for k in names if 'ingest' in k]
    assert names.count('ss_canvas_to_u8') == (0 if fused else 2)
    assert names.count('ss_render_average_clip_u8') == (2 if fused else 0)
    for (a, b), (video, hc, wc) in zip(pairs, out):
        f32 = pipeline.run_two_view(hr[a], hr[b], lr[a], lr[b], hip_nets)
        assert (hc, wc) == f32[1:3]
        _same(video.to(dev), ops.canvas_to_u8(f32[0]), ('clip', a, b, fused))
