"""MULTIBAND fusion on the GPU (libstabstitch_blend.so): the library against the float64 statement of
tests/multiband_ref.py inside its derived bound E(B) at every pixel (canvases down to one pixel, several frames per call, tied weights,
NaN under the mask), the launches of the blend and seam libraries, the identities between the entry points and the routes bit for
bit, and the streaming stitchers under fusion_mode='MULTIBAND' against the ops render of their own splines and against each other.
    python -m pytest tests -m gpu"""
import functools
import gc

import numpy as np
import pytest
import torch

import multiband_ref as MR
import nv12_ref as N
import sweep_inputs as G
from stabstitch2_amd import synth
from test_gpu_parity import dev, hip_nets  # noqa: F401  (fixtures)
from test_multiband_abi import bands_of, clamp_case

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
T = torch.from_numpy


@functools.lru_cache(maxsize=None)
def _warp_inputs(size, views, seed=11):
    h, w, hc, wc = size
    U, src, tgt = G.warp_case(views, h, w, hc, wc, seed=seed)
    return np.ascontiguousarray(U[:, :3]), src, tgt


def _warped(dev, size, views):
    """P of a real warp by the library's own ss_tps_warp_mask_nchw -> (P on the device, its copy on the host)."""
    from stabstitch2_amd import ops
    h, w, hc, wc = size
    U3, src, tgt = _warp_inputs(size, views)
    sd = T(src).to(dev)
    U = ops.multiband_stack([T(u).to(dev) for u in U3])
    P = ops.tps_warp(U, sd, ops.tps_solve(sd, T(tgt).to(dev)), hc, wc, 'NORMAL', with_mask=True)
    return P, P.cpu().numpy()


def _check(dev, name, P, Ph, bands):
    from stabstitch2_amd import ops
    v = Ph.shape[0]
    got = ops.multiband_blend(P, bands).cpu().numpy().astype(np.float64)
    ref = MR.blend(Ph, bands)
    err = float(np.abs(got - ref).max())
    if G.VERBOSE:
        print('  [multiband] %s %s V%d B%d: worst |diff| %.2e = %.4f of the bound' % (Ph.shape[-2:], name, v, bands, err, err / MR.bound(bands, v)))
    assert err <= MR.bound(bands, v), (name, v, bands, err, MR.bound(bands, v))
    return got


# ================================================================================================ the library against float64
@pytest.mark.parametrize('views', [2, 3])
@pytest.mark.parametrize('size', MR.CASES, ids=lambda s: '%dx%d_to_%dx%d' % s)
def test_blend_of_real_warps_against_fp64(dev, size, views):
    """Every pixel (the decisions are exact on the input, nothing is left out) at 0, 1, 3 and the most bands the canvas allows."""
    P, Ph = _warped(dev, size, views)
    assert np.array_equal(Ph[:, 3].max((1, 2)) > 1.0, [True] * views)          # the weight plane came through the warp
    assert ((Ph[:, 4] >= 0.5).sum(0) >= 2).mean() >= 0.1                        # the views overlap
    hc, wc = size[2:]
    outs = {b: _check(dev, 'warp', P, Ph, b) for b in bands_of(hc, wc)}
    assert np.abs(outs[3] - outs[0]).max() > 1.0                                # the bands do something


@pytest.mark.parametrize('views', [2, 3])
@pytest.mark.parametrize('kind', MR.MADE_UP)
@pytest.mark.parametrize('size', MR.CASES, ids=lambda s: '%dx%d_to_%dx%d' % s)
def test_blend_of_made_up_masks_against_fp64(dev, size, kind, views):
    """A hole, an empty view, disjoint views; noise colours; mask values on both sides of 0.5."""
    hc, wc = size[2:]
    Ph = MR.made_up(kind, views, hc, wc)
    P = T(Ph).to(dev)
    for b in bands_of(hc, wc):
        got = _check(dev, kind, P, Ph, b)
        union = (Ph[:, 4] >= 0.5).any(0)
        assert (got[:, ~union] == 0).all() and (~union).any()


@pytest.mark.parametrize('size', [MR.CASES[2], MR.CASES[5]], ids=lambda s: '%dx%d_to_%dx%d' % s)
def test_blend_clamps_both_ways(dev, size):
    hc, wc = size[2:]
    Ph = clamp_case(hc, wc)
    raw = MR.blend(Ph, 3, raw=True)[1]
    assert raw.min() < -20 and raw.max() > 275
    got = _check(dev, 'clamp', T(Ph).to(dev), Ph, 3)
    assert got.min() == 0.0 and got.max() == 255.0 and (got == 0).sum() > 50 and (got == 255).sum() > 50


@pytest.mark.parametrize('views', [2, 3])
@pytest.mark.parametrize('size', MR.SMALL, ids=lambda s: '%dx%d' % s)
def test_blend_of_small_canvases_against_fp64(dev, size, views):
    """mb_plan accepts hc, wc >= 1: one pixel, one row, one column, 3 -> 2, a 2 x 2 top level, at every band count the canvas allows.
    fp32 inside the bound and between canaries, uint8 = the cast of the fp32 output (numpy's and ops.canvas_to_u8's), one band more
    refused.  The fp32 numpy evaluation of the statement stays under 0.02 of the bound on these inputs: a wrong tap is not inside it."""
    from stabstitch2_amd import ops
    from test_gpu_rest_sweeps import canaried, canaries_intact
    hc, wc = size
    Ph = MR.small_case(views, hc, wc)
    P = T(Ph).to(dev)
    valid = Ph[:, 4] >= 0.5
    assert len(np.unique(Ph[:, 3])) == Ph[:, 3].size                            # no ties
    if hc >= 2 and wc >= 2:
        assert valid.any() and not valid.all()                                  # a valid and an invalid pixel
    top = MR.max_bands(hc, wc)
    worst = 0.0
    for b in range(top + 1):
        ref = MR.blend(Ph, b)
        buf, mid = canaried(3 * hc * wc, dev)
        got = ops.multiband_blend(P, b, out=mid.view(3, hc, wc))
        canaries_intact(buf, 3 * hc * wc, 'multiband_blend %s B%d' % (size, b))
        err = float(np.abs(got.cpu().numpy().astype(np.float64) - ref).max())
        worst = max(worst, err / MR.bound(b, views))
        assert err <= MR.bound(b, views), (size, views, b, err, MR.bound(b, views))
        buf8, mid8 = canaried(hc * wc * 3, dev, dtype=torch.uint8, value=0xAB)
        got8 = ops.multiband_blend(P, b, out=mid8.view(hc, wc, 3), u8=True)
        canaries_intact(buf8, hc * wc * 3, 'multiband_blend u8 %s B%d' % (size, b), value=0xAB)
        assert np.array_equal(got8.cpu().numpy(), G.astype_u8(got.cpu().numpy()).transpose(1, 2, 0)), (size, views, b)
        _same(got8, ops.canvas_to_u8(got.clone()[None])[0], ('u8', size, views, b))
    print('\n[multiband claim] %d x %d V%d, bands 0..%d: worst |diff| = %.4f of the bound; %d of %d mask values valid'
          % (hc, wc, views, top, worst, int(valid.sum()), valid.size))
    if top < MR.MAX_BANDS:
        with pytest.raises(ValueError):
            ops.multiband_blend(P, top + 1)


@pytest.mark.parametrize('views', [2, 3])
@pytest.mark.parametrize('size', [MR.CASES[5], MR.CASES[1]], ids=lambda s: '%dx%d_to_%dx%d' % s)
def test_several_frames_in_one_call_against_fp64(dev, size, views):
    """Three different frames in one call (frames ride in gridDim.z, at their own offsets of P, the workspace and the output): each
    against the float64 statement of its own P, fp32 and the uint8 cast, at 0 bands and at the most."""
    from stabstitch2_amd import ops
    h, w, hc, wc = size
    n = 3
    U, src, tgt = G.warp_case(n * views, h, w, hc, wc, seed=12)
    sd = T(src).to(dev)
    clips = [T(np.ascontiguousarray(U[v::views, :3])).to(dev) for v in range(views)]
    P = ops.tps_warp(ops.multiband_stack(clips), sd, ops.tps_solve(sd, T(tgt).to(dev)), hc, wc, 'NORMAL', with_mask=True).view(n, views, 5, hc, wc)
    Ph = P.cpu().numpy()
    assert not np.array_equal(Ph[0], Ph[1]) and not np.array_equal(Ph[1], Ph[2]) and not np.array_equal(Ph[0], Ph[2])
    for b in (0, MR.max_bands(hc, wc)):
        got = ops.multiband_blend(P, b)
        got8 = ops.multiband_blend(P, b, u8=True).cpu().numpy()
        assert got.shape == (n, 3, hc, wc)
        for f in range(n):
            err = float(np.abs(got[f].cpu().numpy().astype(np.float64) - MR.blend(Ph[f], b)).max())
            assert err <= MR.bound(b, views), (f, views, b, err, MR.bound(b, views))
            assert np.array_equal(got8[f], G.astype_u8(got[f].cpu().numpy()).transpose(1, 2, 0)), (f, views, b)


@pytest.mark.parametrize('views', [2, 3])
@pytest.mark.parametrize('size', [MR.CASES[5], MR.CASES[1]], ids=lambda s: '%dx%d_to_%dx%d' % s)
def test_tied_weights_go_to_the_lowest_view(dev, size, views):
    """The 'hole' masks with the weight planes equal in all views on the left half of the canvas: the statement's first of equal maxima
    and the kernel's strict `>` from view 0 upwards name the same owner; noise colours, so another owner is grey levels away."""
    hc, wc = size[2:]
    Ph, ties = MR.tied(MR.made_up('hole', views, hc, wc))
    assert ties[:, :wc // 2].sum() > 100 and not ties[:, wc // 2:].any()        # tied, doubly valid pixels exist
    other = Ph.copy()                                                           # (the same pixels given to the highest tied view instead)
    other[:, 3, :, :wc // 2] += np.arange(views, dtype=np.float32)[:, None, None]
    assert np.abs(MR.blend(other, 0) - MR.blend(Ph, 0)).max() > 1.0
    P = T(Ph).to(dev)
    for b in bands_of(hc, wc):
        _check(dev, 'tied', P, Ph, b)


@pytest.mark.parametrize('views', [2, 3])
def test_invalid_pixels_carry_nothing(dev, views):
    """P of a real warp with planes 0..3 of every pixel below the 0.5 mask set to NaN: the output has the bits of the unmodified P's,
    fp32 and uint8 -- the decisions read the mask first, and no arithmetic touches what an invalid view holds."""
    from stabstitch2_amd import ops
    size = MR.CASES[1]
    hc, wc = size[2:]
    P, Ph = _warped(dev, size, views)
    invalid = P[:, 4] < 0.5
    Q = P.clone()
    Q[:, :4] = torch.where(invalid[:, None], torch.full_like(Q[:, :4], float('nan')), Q[:, :4])
    assert int(invalid.sum()) > 100 and int(torch.isnan(Q).sum()) == 4 * int(invalid.sum()) and not bool(torch.isnan(Q[:, 4]).any())
    assert bool((~invalid).sum(0).eq(0).any())                                  # pixels outside the union too
    for b in bands_of(hc, wc):
        want = ops.multiband_blend(P, b)
        _same(ops.multiband_blend(Q, b), want, ('fp32', views, b))
        _same(ops.multiband_blend(Q, b, u8=True), ops.multiband_blend(P, b, u8=True), ('u8', views, b))
        assert not bool(torch.isnan(want).any())


# ================================================================================================ identities, bit for bit
def _same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b), what


@pytest.mark.parametrize('views', [2, 3])
@pytest.mark.parametrize('size', [MR.CASES[1], MR.CASES[5]], ids=lambda s: '%dx%d_to_%dx%d' % s)
def test_entry_points_agree_bit_for_bit(dev, size, views):
    """Three frames in one call == three calls; uint8 == canvas_to_u8 of fp32; render_multiband == stack, warp, blend -- from fp32
    planes and from uint8 frames; a workspace handed in and reused == a fresh one."""
    from stabstitch2_amd import ops
    h, w, hc, wc = size
    n = 3
    U, src, tgt = G.warp_case(n * views, h, w, hc, wc, seed=12)
    u8 = np.clip(np.rint(U[:, :3]), 0, 255).astype(np.uint8)
    sd = T(src).to(dev)
    src_c, T_c = sd.view(n, views, 63, 2), ops.tps_solve(sd, T(tgt).to(dev)).view(n, views, 2, 66)
    frames = T(np.ascontiguousarray(u8.transpose(0, 2, 3, 1))).to(dev).view(n, views, h, w, 3)
    clips_u8 = [frames[:, v].contiguous() for v in range(views)]
    clips = [ops.ingest_u8(c)[0] for c in clips_u8]
    bands = MR.max_bands(hc, wc)
    P = ops.tps_warp(ops.multiband_stack(clips), sd, T_c.view(n * views, 2, 66), hc, wc, 'NORMAL', with_mask=True).view(n, views, 5, hc, wc)
    together = ops.multiband_blend(P, bands)
    ws = ops.multiband_workspace(1, views, hc, wc, bands, dev)
    ws.fill_(float('nan'))
    for f in range(n):
        _same(ops.multiband_blend(P[f], bands, ws=ws), together[f], ('frames', f))
    together8 = ops.multiband_blend(P, bands, u8=True)
    _same(together8, ops.canvas_to_u8(together), 'u8')
    assert together8.shape == (n, hc, wc, 3) and int(together8.max()) > 200
    _same(ops.render_multiband(clips, src_c, T_c, hc, wc, 'NORMAL', bands), together, 'render clip')
    _same(ops.render_multiband(clips_u8, src_c, T_c, hc, wc, 'NORMAL', bands), together8, 'render clip u8')
    for f in range(n):
        _same(ops.render_multiband([c[f] for c in clips], src_c[f], T_c[f], hc, wc, 'NORMAL', bands), together[f], ('render', f))
        _same(ops.render_multiband([c[f] for c in clips_u8], src_c[f], T_c[f], hc, wc, 'NORMAL', bands), together8[f], ('render u8', f))
    if bands < MR.MAX_BANDS:
        with pytest.raises(ValueError, match='3 pixels'):
            ops.render_multiband(clips, src_c, T_c, hc, wc, 'NORMAL', bands + 1)
    with pytest.raises(ValueError):
        ops.multiband_blend(P[:, :, :4].contiguous(), bands)


@pytest.mark.parametrize('views', [2, 3])
def test_render_frames_routes_agree(dev, views):
    """pipeline.render_frames with fusion_mode='MULTIBAND': the clip route (10 frames: a chunk of 8 and one of 2), the list route and
    ops.render_multiband frame by frame give the same frames; and they are not LINEAR's."""
    from stabstitch2_amd import ops, pipeline
    from stabstitch2_amd.spatial_network import get_rigid_mesh
    n, h, w = 10, 72, 96
    g = torch.Generator().manual_seed(5 + views)
    rigid = get_rigid_mesh(1, 360, 480, device='cpu')[0]
    meshes = []
    for v in range(views):
        m = rigid[None].repeat(n, 1, 1, 1) + (torch.rand((n, 7, 9, 2), generator=g) - 0.5) * 30.0
        m[..., 0] += v * 150.0
        meshes.append(m[None].contiguous().to(dev))
    clips = [(torch.rand((n, 3, h, w), generator=g) * 255).to(dev) for _ in range(views)]
    out, hc, wc = pipeline.render_frames(clips, meshes, fusion_mode='MULTIBAND', bands=3)
    assert pipeline.MULTIBAND_FRAMES == 8 and out.shape == (n, 3, hc, wc)
    lists, hc2, wc2 = pipeline.render_frames([[c[i] for i in range(n)] for c in clips], meshes, fusion_mode='MULTIBAND', bands=3)
    _same(lists, out, 'lists')
    _, _, src, Tk = pipeline.render_plan(meshes, h, w)
    for i in (0, 7, 8, 9):
        _same(ops.render_multiband([c[i] for c in clips], src[i], Tk[i], hc, wc, 'NORMAL', 3), out[i], ('frame', i))
    default, _, _ = pipeline.render_frames(clips, meshes, fusion_mode='MULTIBAND')
    _same(default[0], ops.render_multiband([c[0] for c in clips], src[0], Tk[0], hc, wc, 'NORMAL', 5), 'default bands')
    linear, _, _ = pipeline.render_frames(clips, meshes, fusion_mode='LINEAR')
    assert float((linear - out).abs().max()) > 1.0
    with pytest.raises(ValueError, match='bands'):
        pipeline.render_frames(clips, meshes, fusion_mode='LINEAR', bands=3)
    with pytest.raises(ValueError, match='bands'):
        pipeline.render_frames(clips, meshes, fusion_mode='MULTIBAND', bands=7)


# ================================================================================================ the stitchers
SH, SW, PUSHES = 180, 320, 12              # 7 window-fill pushes + 5 steady-state ones
VIEWPORTS = {2: (204, 500), 3: (204, 660)}
_runs = {}


@pytest.fixture(autouse=True)
def _no_garbage_inside_a_capture():
    """A stitcher that became cyclic garbage still owns HIP graphs; the collector must not meet it while another stitcher's graph
    is being captured: collect between the tests, where nothing captures."""
    gc.collect()
    yield
    gc.collect()


def _clip(dev):
    if 'clip' not in _runs:
        from stabstitch2_amd import ops, pipeline
        hr, _ = synth.make_clip_device(PUSHES, SH, SW, seed=4, views=3, device=dev)
        raw = hr.permute(0, 1, 3, 4, 2).round().clamp(0, 255).to(torch.uint8).cpu().numpy()
        nv = [[N.bgr_to_nv12(raw[v, t]) for t in range(PUSHES)] for v in range(3)]      # as a decoder delivers it, and its conversion
        u8 = torch.stack([torch.stack([T(N.nv12_to_bgr(f)) for f in per]) for per in nv]).to(dev)
        loaded = [ops.ingest_u8(u8[v], pipeline.LR_H, pipeline.LR_W) for v in range(3)]
        _runs['clip'] = dict(nv=nv, u8=u8, hr=torch.stack([x[0] for x in loaded]), lr=torch.stack([x[1] for x in loaded]))
    return _runs['clip']


def _push_all(st, dev, views, u8=False, n=PUSHES):
    c = _clip(dev)
    out = []
    for t in range(n):
        if u8:
            out += st.push_u8(*[c['u8'][v, t] for v in range(views)])
        else:
            out += st.push(*([c['hr'][v, t:t + 1] for v in range(views)] + [c['lr'][v, t:t + 1] for v in range(views)]))
    return out


def _make(nets, views, **kw):
    from stabstitch2_amd import online
    kw.setdefault('fusion_mode', 'MULTIBAND')
    return (online.OnlineStitcher if views == 2 else online.ThreeViewOnlineStitcher)(nets, SH, SW, **kw)


def _reference(dev, nets, views):
    """PUSHES deterministic pushes through the MULTIBAND stitcher of `views` views (captured graph, the push renders), once."""
    key = ('ref', views)
    if key not in _runs:
        st = _make(nets, views, deterministic=True)
        frames = _push_all(st, dev, views)
        assert len(frames) == PUSHES and st._direct() and st.graph is not None and not st._fused and st.bands == 5
        _runs[key] = frames
    return _runs[key]


def _same_lists(a, b, what):
    assert len(a) == len(b), (what, len(a), len(b))
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and x.dtype == y.dtype and torch.equal(x, y), (what, i)


@pytest.mark.parametrize('views', [2, 3])
def test_stream_frames_are_the_multiband_render_of_their_own_splines(dev, hip_nets, views, monkeypatch):
    """Every frame a MULTIBAND stitcher hands out (the window's seven, then five behind the captured graph) ==
    ops.render_multiband on the stitcher's own solved splines of that frame, with bands=3 handed through."""
    from stabstitch2_amd import online, ops
    c = _clip(dev)
    Cls = online.OnlineStitcher if views == 2 else online.ThreeViewOnlineStitcher
    st = _make(hip_nets, views, bands=3)
    solved = []
    inner = online._Stitcher._render_solved

    def spy(self, imgs, src, Tk, *a, **kw):      # (on the class: a spy stored on the stitcher would tie it into a reference cycle)
        solved.append((src.clone(), Tk.clone()))
        return inner(self, imgs, src, Tk, *a, **kw)
    monkeypatch.setattr(Cls, '_render_solved', spy)
    emitted = 0
    for t in range(PUSHES):
        solved.clear()
        got = st.push(*([c['hr'][v, t:t + 1] for v in range(views)] + [c['lr'][v, t:t + 1] for v in range(views)]))
        if not got:
            continue
        if len(got) == 7:
            assert len(solved) == 7
            splines, frames_t = list(solved), range(7)
        else:
            splines, frames_t = [st._deferred[:2]], [t]
        for (src, Tk), ft, frame in zip(splines, frames_t, got):
            want = ops.render_multiband([c['hr'][v, ft] for v in range(views)], src, Tk, st.hc, st.wc, 'NORMAL', 3)
            assert frame.shape == (3, st.hc, st.wc) and torch.equal(frame, want), (views, t, ft, float((frame - want).abs().max()))
            emitted += 1
    assert emitted == PUSHES and st.graph is not None and st._direct()


@pytest.mark.parametrize('views', [2, 3])
def test_multiband_stream_is_not_the_linear_stream(dev, hip_nets, views):
    """No class renders MULTIBAND as LINEAR any more: the same input, frames that differ by grey levels on the overlap."""
    ref = _reference(dev, hip_nets, views)
    lin = _push_all(_make(hip_nets, views, fusion_mode='LINEAR', deterministic=True), dev, views)
    assert len(lin) == len(ref)
    for a, b in zip(ref, lin):
        assert a.shape == b.shape and float((a - b).abs().max()) > 1.0


@pytest.mark.parametrize('views', [2, 3])
def test_push_u8_and_push_many_equal_the_pushes(dev, hip_nets, views):
    """push_u8 == canvas_to_u8 of push; push_many / push_many_u8 at k = 4 (three calls, the window fills inside the second) == twelve
    pushes, under deterministic=True; and a stitcher without a graph gives the same frames."""
    from stabstitch2_amd import ops
    c = _clip(dev)
    ref = _reference(dev, hip_nets, views)
    ref8 = [ops.canvas_to_u8(f[None])[0] for f in ref]
    st = _make(hip_nets, views, deterministic=True)
    _same_lists(_push_all(st, dev, views, u8=True), ref8, 'push_u8')
    assert st._u8_steady()
    for u8 in (False, True):
        many = _make(hip_nets, views, deterministic=True)
        got = []
        for t in range(0, PUSHES, 4):
            if u8:
                got += many.push_many_u8(*[c['u8'][v, t:t + 4] for v in range(views)])
            else:
                got += many.push_many(*([c['hr'][v, t:t + 4] for v in range(views)] + [c['lr'][v, t:t + 4] for v in range(views)]))
        _same_lists(got, ref8 if u8 else ref, 'push_many u8=%s' % u8)
        assert many.batch_captures >= 1
    eager = _make(hip_nets, views, deterministic=True, use_graph=False)
    _same_lists(_push_all(eager, dev, views, n=9), ref[:9], 'use_graph=False')
    assert not eager._direct()


def test_viewport_fixes_the_frame_size(dev, hip_nets):
    """viewport= with grow='refit': every frame has the viewport's size and is the render of its splines at that size (push_u8)."""
    from stabstitch2_amd import ops
    c = _clip(dev)
    hc, wc = VIEWPORTS[2]
    st = _make(hip_nets, 2, viewport=(hc, wc), grow='refit')
    frames = _push_all(st, dev, 2, u8=True, n=9)
    assert len(frames) == 9 and all(f.shape == (hc, wc, 3) and f.dtype == torch.uint8 for f in frames) and (st.hc, st.wc) == (hc, wc)
    src, Tk = st._deferred[:2]
    _same(frames[-1], ops.render_multiband([c['u8'][v, 8] for v in range(2)], src, Tk, hc, wc, 'NORMAL', 5), 'viewport')
    assert int(frames[-1].max()) > 100


@pytest.mark.parametrize('views', [2, 3])
def test_push_nv12_equals_push_u8_of_the_converted_frames(dev, hip_nets, views):
    """push_nv12 goes ingest -> push -> the sinks: out='bgr' hands out push_u8's frames of the converted input, out='nv12' their
    numpy BGR -> NV12; the window fill and two steady-state pushes, under a viewport (even sizes)."""
    c = _clip(dev)
    n = 9
    ref_st = _make(hip_nets, views, viewport=VIEWPORTS[views])
    ref = [ref_st.push_u8(*[c['u8'][v, t] for v in range(views)]) for t in range(n)]
    assert [len(r) for r in ref] == [0] * 6 + [7, 1, 1]
    hc, wc = VIEWPORTS[views]
    outs = ['bgr'] * 7 + ['nv12', 'bgr']
    st = _make(hip_nets, views, viewport=VIEWPORTS[views])
    got = [st.push_nv12(*[T(c['nv'][v][t]).to(dev) for v in range(views)], out=outs[t]) for t in range(n)]
    assert [len(g) for g in got] == [len(r) for r in ref]
    for t, (g, r) in enumerate(zip(got, ref)):
        for a, b in zip(g, r):
            if outs[t] == 'bgr':
                assert a.shape == (hc, wc, 3) and torch.equal(a, b), t
            else:
                assert a.shape == (hc // 2 * 3, wc) and np.array_equal(a.cpu().numpy(), N.bgr_to_nv12(b.cpu().numpy())), t


def test_recapture_growth_renders_on_the_grown_canvas(dev, hip_nets):
    """A canvas cropped on its right side under grow='recapture': it grows, the graph is captured again, and every steady-state frame
    is the MULTIBAND render of its splines on the canvas of its push."""
    from stabstitch2_amd import ops
    c = _clip(dev)
    probe = _make(hip_nets, 2)
    _push_all(probe, dev, 2, n=7)
    bb = [float(x) for x in probe.bbox.cpu()]
    crop = [bb[0], bb[1] - 0.10 * (bb[1] - bb[0]), bb[2], bb[3]]
    st = _make(hip_nets, 2, canvas=crop, grow='recapture')
    first, checked = None, 0
    for t in range(PUSHES):
        got = st.push(c['hr'][0, t:t + 1], c['hr'][1, t:t + 1], c['lr'][0, t:t + 1], c['lr'][1, t:t + 1])
        torch.cuda.synchronize()                     # (the growth check reads the watcher one push later: make it land)
        if got and first is None:
            first = (st.hc, st.wc)
        if len(got) == 1:
            src, Tk = st._deferred[:2]
            _same(got[0], ops.render_multiband([c['hr'][v, t] for v in range(2)], src, Tk, st.hc, st.wc, 'NORMAL', 5), ('grown', t))
            checked += 1
    assert checked == PUSHES - 7 and st.canvas_epoch >= 1 and (st.hc, st.wc) != first, (st.canvas_epoch, first, st.hc, st.wc)


def test_refusals(dev, hip_nets):
    from stabstitch2_amd import online
    with pytest.raises(ValueError, match='exposure'):
        online.OnlineStitcher(hip_nets, SH, SW, fusion_mode='MULTIBAND', exposure=True)
    with pytest.raises(ValueError, match='bands'):
        online.OnlineStitcher(hip_nets, SH, SW, fusion_mode='MULTIBAND', bands=7)
    with pytest.raises(ValueError, match='bands'):
        online.OnlineStitcher(hip_nets, SH, SW, fusion_mode='LINEAR', bands=3)
    with pytest.raises(ValueError, match='bands'):
        online.ThreeViewOnlineStitcher(hip_nets, SH, SW, fusion_mode='FEATHER', bands=3)
    for make in (lambda: online.MultiOnlineStitcher(hip_nets, SH, SW, streams=2, fusion_mode='MULTIBAND'),
                 lambda: online.PipelinedOnlineStitcher(hip_nets, SH, SW, fusion_mode='MULTIBAND'),
                 lambda: online.PipelinedMultiOnlineStitcher(hip_nets, SH, SW, streams=2, fusion_mode='MULTIBAND'),
                 lambda: online.PipelinedThreeViewOnlineStitcher(hip_nets, SH, SW, fusion_mode='MULTIBAND')):
        with pytest.raises(ValueError, match='MULTIBAND'):
            make()


# ================================================================================================ the launches of the two libraries
def test_every_instantiation_of_the_blend_and_seam_libraries_is_launched(dev):
    """The smallest calls under torch.profiler -- a 5 x 5 canvas, V = 2 and 3, bands 0, 1 and 2 (a level written from a coarser one
    needs two), fp32 and uint8, and one seam call each -- launch every instantiation that sweep_inputs.blend_reach and seam_reach
    list, and nothing else of the two libraries.  Should the profiler report names without template arguments, base names are matched
    instead and the test says so in its output."""
    import re
    from stabstitch2_amd import ops
    from test_gpu_linear_frames import _kernel_names
    launched = []
    for v in (2, 3):
        P = T(MR.small_case(v, 5, 5)).to(dev)
        calls = [lambda b=b, u8=u8: ops.multiband_blend(P, b, u8=u8) for b in (0, 1, 2) for u8 in (False, True)]
        calls.append(lambda: ops.multiband_seam(P.clone(), 1, 0, 8.0))
        for fn in calls:
            fn()                                     # (once outside the profiler: module load)
            launched += _kernel_names(fn)[1]
    ours = sorted({k for k in launched if re.search(r'\b(mb|sm)_[a-z]+_kernel', k)})
    wanted = set(G.blend_reach()) | set(G.seam_reach())
    assert len(wanted) == 21
    if all('<' in k for k in ours if 'mb_reduce_kernel' not in k):
        got = {G.instantiation_key(k) for k in ours}
        print('\n[launch witness] matched by template arguments: %s' % sorted(got))
        assert got == wanted, (sorted(wanted - got), sorted(got - wanted))
    else:
        got = {re.search(r'\b((?:mb|sm)_[a-z]+_kernel)', k).group(1) for k in ours}
        print('\n[launch witness] the profiler reports no template arguments; matched by base name: %s' % ours)
        assert got == {k.split('<')[0] for k in wanted}, (got, ours)
