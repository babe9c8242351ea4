"""Fixed-size streaming output on the GPU: `viewport=(Hout, Wout)` and the device-side canvas refit `grow='refit'` (online.py).

The refit kernels are held bit for bit to the numpy fp32 restatement of tests/test_canvas_fit_abi.py (and the watcher's rows to
ref64.canvas_watch); the stitchers are held to the plain stitchers (a viewport of the natural size changes nothing), to a render
rebuilt by hand from the box each push read (the refit under drift), and to one another (eager, captured, two pushes in flight).
HR frames are 360 x 480 throughout."""
import contextlib

import numpy as np
import pytest
import torch

import ref64 as R
from stabstitch2_amd import synth
from test_canvas_fit_abi import F, fit_aspect, fit_update
from test_gpu_parity import dev, hip_nets, clip16  # noqa: F401  (fixtures)
from test_gpu_rest_sweeps import same_bits
from test_gpu_round5 import _push_drifting

pytestmark = pytest.mark.gpu

H, W = 360, 480
VIEWPORT = (300, 520)
N_DRIFT = 44


# ------------------------------------------------------------------------------------------------ 1. kernels against the restatement
def _kernel_case(streams, views, seed):
    """Control points of `streams` streams normalised on their canvases, stream s in case s % 9: 0 inside the guard, 1-4 beyond one
    side, 5 beyond two sides, 6 a NaN point among points that stay inside, 7 far beyond zoom_limit, 8 beyond an edge by a hair (the
    0.5-px refusal at margin 0) -- so that only some streams of a launch grow; each stream on a box of its own."""
    rs = np.random.RandomState(seed)
    src = rs.uniform(-0.9, 0.9, (streams, views, 63, 2)).astype(F)
    box = np.zeros((streams, 4), F)
    for s in range(streams):
        c = s % 9
        v, k = rs.randint(views), rs.randint(63)
        if c == 1:
            src[s, v, k, 0] = -1.21
        elif c == 2:
            src[s, v, k, 0] = 1.07
        elif c == 3:
            src[s, v, k, 1] = -1.13
        elif c == 4:
            src[s, v, k, 1] = 1.3
        elif c == 5:
            src[s, v, k, 0] = 1.17
            src[s, (v + 1) % views, k, 1] = -1.09
        elif c == 6:
            src[s, v, k, 0] = np.nan
        elif c == 7:
            src[s, v, k, 0] = -4.5
        elif c == 8:
            src[s, v, k, 0] = 1.0004
        box[s] = (-64 - 3 * s, 576 + 2 * s, -60 - s, 420 + 5 * s)
    return src, box


def _expect(src, wi, wf, box, epoch, ext0, guard, margin, zoom, hout, wout, frames=False):
    """The rows after one launch: the documented watcher (ref64.canvas_watch), then the restated refit -- per stream, or (frames) the
    frames of ONE stream one after the other and a single refit behind the last."""
    wi, wf, box, epoch = wi.copy(), wf.copy(), box.copy(), epoch.copy()
    if frames:
        for f in range(src.shape[0]):
            R.canvas_watch(src[f].reshape(1, -1, 2), guard, wi, wf)
    else:
        R.canvas_watch(src.reshape(src.shape[0], -1, 2), guard, wi, wf)
    for s in range(box.shape[0]):
        box[s], epoch[s], wf[s] = fit_update(box[s], epoch[s], ext0[s], wf[s], guard, margin, zoom, wout, hout)
    return wi, wf, box, epoch


def _fit_on(dev, box, ext0_np, hout, wout, margin, zoom, epoch0):
    from stabstitch2_amd import ops
    n = box.shape[0]
    return ops.CanvasFit(torch.from_numpy(box.copy()).to(dev), torch.full((n,), epoch0, dtype=torch.int32, device=dev),
                         torch.from_numpy(ext0_np.copy()).to(dev), margin, zoom, hout, wout)


def _rows(dev, n, seen=3):
    """Watcher rows that have seen frames before (extents well inside)."""
    wi = np.tile(np.array([seen, 0, -1, 0], np.int32), (n, 1))
    wf = np.tile(np.array([-0.5, 0.5, -0.4, 0.4], F), (n, 1))
    return wi, wf


@pytest.mark.parametrize('views', [2, 3])
@pytest.mark.parametrize('streams', [1, 3, 33])
def test_fit_kernels_equal_the_restatement_bit_for_bit(dev, streams, views):
    """ss_canvas_watch_fit, ss_canvas_watch_frames_fit (1, 2 and 8 frames) and ss_render_footprints_watch_fit on 1, 3 and 33 streams of
    2 and 3 views, a wide and a tall viewport, margin 0.03 and 0 (the 0.5-px refusal): box, epoch, watch_f and watch_i equal the
    numpy restatement exactly (the boxes set at the viewport's aspect, as ss_box_fit_aspect leaves them: against another aspect the
    letterbox alone would pass the zoom limit), ext0 and the control points are left alone, and the footprints are those of the
    entry without the fit (lattice, hulls and class counts bit for bit; the tile lists as sets: their order inside a class is not
    specified).  The entries without the fit, given the same inputs, leave the rows the documented watcher leaves, and no box."""
    from stabstitch2_amd import ops
    from stabstitch2_amd.spatial_network import get_rigid_mesh, get_norm_mesh
    guard, zoom = 0.0283, 2.0
    nrigid = get_norm_mesh(get_rigid_mesh(1, H, W, device=dev), H, W).contiguous()
    for (hout, wout), margin in (((96, 330), 0.03), ((330, 96), 0.03), ((96, 330), 0.0)):
        src, box = _kernel_case(streams, views, 100 * streams + views)
        if streams == 1:
            src, box = _kernel_case(9, views, 7)[0][5:6], _kernel_case(9, views, 7)[1][5:6]      # (one stream: the two-sided case)
        box = np.array([fit_aspect(b, wout, hout) for b in box], F)      # canvases as they are set: at the viewport's aspect
        ext0 = np.stack((box[:, 1] - box[:, 0], box[:, 3] - box[:, 2]), 1).astype(F)
        wi0, wf0 = _rows(dev, streams)
        epoch0 = np.full((streams,), 2, np.int32)
        want = _expect(src, wi0, wf0, box, epoch0, ext0, guard, margin, zoom, hout, wout)
        assert 0 < int((want[3] != epoch0).sum()) < max(streams, 2)                          # some streams grow, not all
        srcd = torch.from_numpy(src).to(dev)
        # --- ss_canvas_watch_fit
        fit = _fit_on(dev, box, ext0, hout, wout, margin, zoom, 2)
        wi, wf = torch.from_numpy(wi0.copy()).to(dev), torch.from_numpy(wf0.copy()).to(dev)
        ops.canvas_watch(srcd, wi, wf, guard, fit=fit)
        for got, exp, name in ((wi, want[0], 'watch_i'), (wf, want[1], 'watch_f'), (fit.box, want[2], 'box'), (fit.epoch, want[3], 'epoch'),
                               (fit.ext0, ext0, 'ext0'), (srcd, src, 'src')):
            same_bits(got, exp, 'canvas_watch_fit %s (%d streams, %d views, %dx%d, margin %g)' % (name, streams, views, hout, wout, margin))
        # --- the entry without the fit: the documented watcher alone
        wi, wf = torch.from_numpy(wi0.copy()).to(dev), torch.from_numpy(wf0.copy()).to(dev)
        ops.canvas_watch(srcd, wi, wf, guard)
        pi, pf = wi0.copy(), wf0.copy()
        R.canvas_watch(src.reshape(streams, -1, 2), guard, pi, pf)
        same_bits(wi, pi, 'canvas_watch watch_i')
        same_bits(wf, pf, 'canvas_watch watch_f')
        # --- ss_render_footprints_watch_fit: the viewport is the canvas size
        T = ops.tps_solve_shared(srcd.reshape(-1, 63, 2), nrigid).reshape(streams, views, 2, 66)
        fit = _fit_on(dev, box, ext0, hout, wout, margin, zoom, 2)
        wi, wf = torch.from_numpy(wi0.copy()).to(dev), torch.from_numpy(wf0.copy()).to(dev)
        fp = ops.render_footprints(srcd, T, H, W, hout, wout, watch=(guard, wi, wf), fit=fit)
        for got, exp, name in ((wi, want[0], 'watch_i'), (wf, want[1], 'watch_f'), (fit.box, want[2], 'box'), (fit.epoch, want[3], 'epoch'),
                               (fit.ext0, ext0, 'ext0'), (srcd, src, 'src')):
            same_bits(got, exp, 'render_footprints_watch_fit %s (%d streams, %d views, %dx%d, margin %g)'
                      % (name, streams, views, hout, wout, margin))
        wi, wf = torch.from_numpy(wi0.copy()).to(dev), torch.from_numpy(wf0.copy()).to(dev)
        fp0 = ops.render_footprints(srcd, T, H, W, hout, wout, watch=(guard, wi, wf))
        same_bits(wi, pi, 'render_footprints_watch watch_i')
        same_bits(wf, pf, 'render_footprints_watch watch_f')
        ny, nx = -(-hout // 8) + 1, 2 * (-(-wout // 64)) + 1
        head, nt = views * ny * nx * 2 + 4 * views + 4, (ny - 1) * ((nx - 1) // 2)
        a, b = fp.cpu().numpy().view(np.uint32), fp0.cpu().numpy().view(np.uint32)
        assert a.shape == b.shape == (streams, head + 4 * nt)
        assert (a[:, :head] == b[:, :head]).all(), 'lattice / hulls / class counts'
        for s in range(streams):
            for c in range(4):
                cnt = int(a[s, head - 4 + c])
                assert cnt <= nt
                assert sorted(a[s, head + c * nt:head + c * nt + cnt]) == sorted(b[s, head + c * nt:head + c * nt + cnt]), (s, c)
    # --- ss_canvas_watch_frames_fit: k frames of ONE stream, one refit behind the last
    for k in (1, 2, 8):
        for case, margin, (hout, wout) in ((5, 0.03, (96, 330)), (0, 0.03, (330, 96)), (8, 0.0, (96, 330)), (7, 0.03, (96, 330)),
                                           (6, 0.03, (96, 330)), (2, 0.03, (330, 96))):
            src, box = _kernel_case(9 * k, views, 31 * k + views)
            src = np.ascontiguousarray(src[case::9][:k])            # k frames, all of this case ...
            src[:k - 1] = np.clip(np.nan_to_num(src[:k - 1]), -0.9, 0.9)      # ... or rather: only the LAST frame leaves the canvas
            box = np.array([fit_aspect(b, wout, hout) for b in box[case:case + 1]], F)
            ext0 = np.stack((box[:, 1] - box[:, 0], box[:, 3] - box[:, 2]), 1).astype(F)
            wi0, wf0 = _rows(dev, 1, seen=11)
            want = _expect(src, wi0, wf0, box, np.array([0], np.int32), ext0, guard, margin, zoom, hout, wout, frames=True)
            assert int(want[3][0]) == (1 if case in (5, 2) else 0), (case, want)
            fit = _fit_on(dev, box, ext0, hout, wout, margin, zoom, 0)
            wi, wf = torch.from_numpy(wi0.copy()).to(dev), torch.from_numpy(wf0.copy()).to(dev)
            srcd = torch.from_numpy(src).to(dev)
            ops.canvas_watch_frames(srcd, wi, wf, guard, fit=fit)
            for got, exp, name in ((wi, want[0], 'watch_i'), (wf, want[1], 'watch_f'), (fit.box, want[2], 'box'),
                                   (fit.epoch, want[3], 'epoch'), (fit.ext0, ext0, 'ext0'), (srcd, src, 'src')):
                same_bits(got, exp, 'canvas_watch_frames_fit %s (%d frames, %d views, case %d)' % (name, k, views, case))
            wi, wf = torch.from_numpy(wi0.copy()).to(dev), torch.from_numpy(wf0.copy()).to(dev)
            ops.canvas_watch_frames(srcd, wi, wf, guard)
            pi, pf = wi0.copy(), wf0.copy()
            for f in range(k):
                R.canvas_watch(src[f].reshape(1, -1, 2), guard, pi, pf)
            same_bits(wi, pi, 'canvas_watch_frames watch_i')
            same_bits(wf, pf, 'canvas_watch_frames watch_f')


def test_box_fit_aspect_equals_the_restatement(dev):
    from stabstitch2_amd import ops
    rs = np.random.RandomState(5)
    boxes = np.stack([np.array([x, x + w, y, y + h], F) for x, y, w, h in zip(rs.uniform(-500, 100, 40), rs.uniform(-400, 80, 40),
                                                                               rs.uniform(40, 3000, 40), rs.uniform(40, 2000, 40))])
    boxes[0] = (-64, 576, -60, 420)
    for hout, wout in ((480, 640), (11, 65535), (300, 520), (2000, 33)):
        d = torch.from_numpy(boxes.copy()).to(dev)
        e = torch.zeros((40, 2), device=dev)
        ops.box_fit_aspect(d, hout, wout, e)
        want = np.array([fit_aspect(b, wout, hout) for b in boxes], F)
        same_bits(d, want, 'box_fit_aspect %dx%d' % (hout, wout))
        same_bits(e, np.stack((want[:, 1] - want[:, 0], want[:, 3] - want[:, 2]), 1).astype(F), 'ext0')
    assert tuple(fit_aspect(boxes[0], 640, 480)) == tuple(boxes[0])


# ------------------------------------------------------------------------------------------------ shared clips
@pytest.fixture(scope='module')
def clipd(dev, clip16):
    hr, lr = clip16
    return [[f.to(dev) for f in v] for v in hr], [[f.to(dev) for f in v] for v in lr]


def _u8(hr):
    """a decoded frame [H,W,3] uint8 from an fp32 HR frame [1,3,H,W]"""
    return hr[0].permute(1, 2, 0).clamp(0, 255).to(torch.uint8).contiguous()


# ------------------------------------------------------------------------------------------------ 2. neutral when nothing grows
CANVAS = (-64.0, 576.0, -60.0, 420.0)          # 640 x 480: natural size 480 x 640, and 640 * 480 == 480 * 640 -- the fit is a no-op
INSIDE_SHIFT = -24.0                           # LR px between the views at which the stream stays inside CANVAS, see _view_shift


@contextlib.contextmanager
def _view_shift(nets, px):
    """The stream that stays inside CANVAS.  The synthetic SpatialNet sets view 2 off against view 1 by -216 LR px: the two meshes of
    the 360 x 480 clip then span x = -112 .. 592 and leave the 640-wide box on both sides in every frame.  With the offset at `px` =
    -24 (the stage-1 head bias, edited in place as _push_drifting does and put back afterwards) they span x = -17 .. 496 and y =
    -6 .. 365 over the 16 frames (CPU oracle): 47 px from the nearest edge, and the watcher's guard is 9 px there (margin 0.03)."""
    bias = nets[0]._prepared()['r1']['fc'][2][1]
    bias[0::2] = px
    try:
        yield
    finally:
        bias[0::2] = -216.0


def _mixed_pushes(st, hrd, lrd, views=2):
    """9 x push, 2 x push_u8, push_many(k = 3) -> every frame, in order (uint8 ones as they are)."""
    out = []
    fr = lambda t: [hrd[v][t % 16] for v in range(views)] + [lrd[v][t % 16] for v in range(views)]
    for t in range(9):
        out += st.push(*fr(t))
    for t in range(9, 11):
        out += st.push_u8(*[_u8(f) for f in fr(t)[:views]])
    many = [torch.cat([fr(t)[i] for t in range(11, 14)], 0) for i in range(2 * views)]
    out += st.push_many(*many)
    return out


@pytest.mark.parametrize('warp,fusion', [('NORMAL', 'AVERAGE'), ('FAST', 'LINEAR')])
def test_viewport_of_the_natural_size_changes_nothing(dev, hip_nets, clipd, warp, fusion):
    """OnlineStitcher on the 640 x 480 box, and the same with viewport=(480, 640) under grow='never' and grow='refit', on a clip that
    stays inside: every frame of push, push_u8 and push_many (k = 3) bit-identical."""
    from stabstitch2_amd.online import OnlineStitcher
    hrd, lrd = clipd
    mk = lambda **kw: OnlineStitcher(hip_nets, H, W, canvas=CANVAS, warp_mode=warp, fusion_mode=fusion, **kw)
    plain = mk()
    with _view_shift(hip_nets, INSIDE_SHIFT):
        ref = _mixed_pushes(plain, hrd, lrd)
    assert (plain.hc, plain.wc) == (480, 640) and len(ref) == 14
    rep = plain.overflow_report()
    assert rep['clipped_frames'] == 0 and rep['near_frames'] == 0, rep          # the stream does stay inside
    for grow in ('never', 'refit'):
        st = mk(viewport=(480, 640), grow=grow)
        assert (st.hc, st.wc) == (480, 640)
        with _view_shift(hip_nets, INSIDE_SHIFT):
            got = _mixed_pushes(st, hrd, lrd)
        rep = st.overflow_report()
        assert rep['canvas_epoch'] == 0 and rep['clipped_frames'] == 0 and rep['box'] == CANVAS, rep
        assert len(got) == len(ref)
        for t, (a, b) in enumerate(zip(got, ref)):
            assert a.dtype == b.dtype and torch.equal(a, b), (grow, t)


def test_viewport_of_the_natural_size_changes_nothing_three_views_and_multi(dev, hip_nets, clipd):
    from stabstitch2_amd.online import MultiOnlineStitcher, ThreeViewOnlineStitcher
    hrd, lrd = clipd
    # two streams (the clip at two phases), one viewport for both
    batch = lambda t: [torch.cat([v[(t + s) % 16] for s in range(2)], 0) for v in (hrd[0], hrd[1], lrd[0], lrd[1])]
    outs = {}
    for key, kw in (('plain', {}), ('never', dict(viewport=(480, 640))), ('refit', dict(viewport=(480, 640), grow='refit'))):
        st = MultiOnlineStitcher(hip_nets, H, W, streams=2, canvases=[CANVAS, CANVAS], **kw)
        got = [[], []]
        with _view_shift(hip_nets, INSIDE_SHIFT):
            for t in range(11):
                for s, fr in enumerate(st.push(*batch(t))):
                    got[s] += fr
        assert st.canvas_sizes == [(480, 640)] * 2 and st.canvas_epoch == [0, 0] and st.clipped_frames == [0, 0]
        assert st.canvas_box == [CANVAS, CANVAS]
        outs[key] = got
    for key in ('never', 'refit'):
        for s in range(2):
            assert len(outs[key][s]) == len(outs['plain'][s]) == 11
            assert all(torch.equal(a, b) for a, b in zip(outs[key][s], outs['plain'][s])), (key, s)
    # three views on a 1440 x 720 output box, viewport 720 x 1440
    hr3, lr3 = synth.make_clip(16, H, W, seed=4, views=3)
    hrd3 = [[f.to(dev) for f in v] for v in hr3]
    lrd3 = [[f.to(dev) for f in v] for v in lr3]
    # (the three meshes span x = -2 .. 931 and y = -3 .. 370 in first-canvas px on this clip (CPU oracle), the guard is 20 px: well inside)
    box3 = (-240.0, 1200.0, -180.0, 540.0)
    ref = None
    for kw in ({}, dict(viewport=(720, 1440)), dict(viewport=(720, 1440), grow='refit')):
        st = ThreeViewOnlineStitcher(hip_nets, H, W, canvas=box3, **kw)
        got = _mixed_pushes(st, hrd3, lrd3, views=3)
        rep = st.overflow_report()
        assert (st.hc, st.wc) == (720, 1440) and rep['canvas_epoch'] == 0 and rep['clipped_frames'] == 0 and rep['box'] == box3, rep
        if ref is None:
            ref = got
            continue
        assert len(got) == len(ref) == 14
        for t, (a, b) in enumerate(zip(got, ref)):
            assert a.dtype == b.dtype and torch.equal(a, b), (kw, t)


# ------------------------------------------------------------------------------------------------ 3. constant size, aspect fit
def test_viewport_fixes_the_frame_size_from_construction(dev, hip_nets, clipd):
    """viewport=(300, 520), no canvas: hc / wc before the first push, every one of the 7 + n frames of that shape (fp32 and uint8), and a
    canvas box that contains the un-fitted one (the first window's box grown by the margin: what the plain stitcher fixes) on every
    side, at the viewport's aspect."""
    from stabstitch2_amd.online import OnlineStitcher
    hrd, lrd = clipd
    st = OnlineStitcher(hip_nets, H, W, viewport=VIEWPORT)
    assert (st.hc, st.wc) == VIEWPORT and st.canvas_box is None
    plain = OnlineStitcher(hip_nets, H, W)
    frames = []
    for t in range(10):
        frames += st.push(hrd[0][t], hrd[1][t], lrd[0][t], lrd[1][t])
        plain.push(hrd[0][t], hrd[1][t], lrd[0][t], lrd[1][t])
    frames += st.push_u8(_u8(hrd[0][10]), _u8(hrd[1][10]))
    assert len(frames) == 11
    assert all(tuple(f.shape) == (3,) + VIEWPORT and f.dtype == torch.float32 for f in frames[:10])
    assert tuple(frames[10].shape) == VIEWPORT + (3,) and frames[10].dtype == torch.uint8
    assert (st.hc, st.wc) == VIEWPORT
    box, un = st.canvas_box, plain.canvas_box
    assert box[0] <= un[0] and box[1] >= un[1] and box[2] <= un[2] and box[3] >= un[3], (box, un)
    assert box == tuple(float(v) for v in st.bbox.cpu()) == st.overflow_report()['box']
    a, b = F(F(box[1]) - F(box[0])) * F(VIEWPORT[0]), F(F(box[3]) - F(box[2])) * F(VIEWPORT[1])
    assert abs(float(a) - float(b)) <= 4 * float(np.spacing(max(a, b))), (box, a, b)
    assert all(bool(torch.isfinite(f).all()) for f in frames[:10]) and float(frames[9].abs().max()) > 1.0


# ------------------------------------------------------------------------------------------------ 4. refit under drift, eager
@pytest.fixture(scope='module')
def drift_eager(dev, hip_nets, clipd):
    """44 pushes of the drifting stream through the eager viewport stitcher under grow='refit', ops.stream_splines spied on: per
    frame the LR meshes and the box the launch read; the epoch after every push."""
    from stabstitch2_amd import ops
    from stabstitch2_amd.online import OnlineStitcher
    hrd, lrd = clipd
    seen, epochs = [], []
    real = ops.stream_splines

    def spy(meshes, stride, bboxes, *a, **k):
        seen.append(([m.clone() for m in meshes], bboxes.clone()))
        return real(meshes, stride, bboxes, *a, **k)
    st = OnlineStitcher(hip_nets, H, W, viewport=VIEWPORT, grow='refit', use_graph=False)
    ops.stream_splines = spy
    try:
        outs = _push_drifting(st, hip_nets, hrd, lrd, N_DRIFT, record=lambda t, s: epochs.append(s.canvas_epoch))
    finally:
        ops.stream_splines = real
    return dict(st=st, frames=[f for o in outs for f in o], seen=seen, epochs=epochs, report=st.overflow_report())


def test_refit_under_drift_eager(dev, hip_nets, clipd, drift_eager):
    """The views drift apart by 10 % of the width from frame 20 on.  grow='recapture' keeps every frame inside on this drift although it
    acts a push LATER, and a refitted box is never smaller than a recaptured one: nothing may be cropped.  The canvas grows (not
    before the drift starts), every box contains the one before, and frame t is, bit for bit, ops.stream_splines +
    ops.render_footprints + ops.render_average at the viewport's size on the box its push read."""
    from stabstitch2_amd import ops
    hrd, lrd = clipd
    d = drift_eager
    st, rep = d['st'], d['report']
    print('\n[refit, eager] report %s epochs %s' % (rep, d['epochs']))
    assert rep['frames_seen'] == N_DRIFT and len(d['frames']) == N_DRIFT == len(d['seen'])
    assert rep['clipped_frames'] == 0, rep
    assert st.canvas_epoch >= 1 and st.canvas_epoch == rep['canvas_epoch'] == d['epochs'][-1]
    assert all(e == 0 for e in d['epochs'][:20]), d['epochs']
    boxes = [b.cpu().numpy() for _, b in d['seen']] + [np.array(st.canvas_box, F)]
    for prev, cur in zip(boxes, boxes[1:]):
        assert cur[0] <= prev[0] and cur[1] >= prev[1] and cur[2] <= prev[2] and cur[3] >= prev[3], (prev, cur)
    assert len({tuple(b) for b in boxes}) == st.canvas_epoch + 1
    assert (st.hc, st.wc) == VIEWPORT
    for t, ((meshes, box), frame) in enumerate(zip(d['seen'], d['frames'])):
        src, T = ops.stream_splines(meshes, 126, box, st.nrigid, H, W)
        fp = ops.render_footprints(src, T, H, W, VIEWPORT[0], VIEWPORT[1])[0]
        ref = ops.render_average([hrd[0][t % 16], hrd[1][t % 16]], src[0], T[0], VIEWPORT[0], VIEWPORT[1], 'NORMAL', footprint=fp)
        assert tuple(frame.shape) == (3,) + VIEWPORT and torch.equal(frame, ref), t


# ------------------------------------------------------------------------------------------------ 5. the same under the graph
def test_refit_under_drift_captured(dev, hip_nets, clipd, drift_eager):
    """use_graph=True: frames and epochs equal the eager run's bit for bit; the graph object of the last push is the one captured
    before the first growth, with as many nodes as a grow='never' viewport stitcher's; push_many (k = 4) captures nothing across a
    growth."""
    from stabstitch2_amd.online import OnlineStitcher
    hrd, lrd = clipd
    d = drift_eager
    st = OnlineStitcher(hip_nets, H, W, viewport=VIEWPORT, grow='refit')
    epochs, graphs = [], []
    outs = _push_drifting(st, hip_nets, hrd, lrd, N_DRIFT, record=lambda t, s: (epochs.append(s.canvas_epoch), graphs.append(s.graph)))
    frames = [f for o in outs for f in o]
    assert epochs == d['epochs'] and st.canvas_box == d['st'].canvas_box
    assert len(frames) == N_DRIFT and all(torch.equal(a, b) for a, b in zip(frames, d['frames']))
    assert st.overflow_report() == d['report']
    first_growth = next(t for t, e in enumerate(epochs) if e > 0)
    assert graphs[first_growth - 1] is not None and graphs[-1] is graphs[first_growth - 1] and (st.hc, st.wc) == VIEWPORT
    never = OnlineStitcher(hip_nets, H, W, viewport=VIEWPORT)
    for t in range(9):
        never.push(hrd[0][t], hrd[1][t], lrd[0][t], lrd[1][t])
    assert st.graph_nodes == never.graph_nodes
    # push_many, k = 4: the drift advances from call to call
    sm = OnlineStitcher(hip_nets, H, W, viewport=VIEWPORT, grow='refit')
    bias = hip_nets[0]._prepared()['r1']['fc'][2][1]
    captures, many = [], []
    try:
        for c in range(11):
            bias[0::2] = -216.0 - 6.0 * min(max(4 * c - 20 + 1, 0), 12)
            idx = [(4 * c + j) % 16 for j in range(4)]
            many += sm.push_many(*[torch.cat([v[i] for i in idx], 0) for v in (hrd[0], hrd[1], lrd[0], lrd[1])])
            captures.append(sm.batch_captures)
    finally:
        bias[0::2] = -216.0
    assert len(many) == 44 and all(tuple(f.shape) == (3,) + VIEWPORT for f in many)
    assert sm.canvas_epoch >= 1 and captures[2] >= 1 and captures[-1] == captures[2], (sm.canvas_epoch, captures)


# ------------------------------------------------------------------------------------------------ 6. two pushes in flight
def test_refit_with_two_pushes_in_flight(dev, hip_nets, clipd, drift_eager):
    """PipelinedOnlineStitcher against the plain stitcher on the drifting stream, and PipelinedThreeViewOnlineStitcher against
    ThreeViewOnlineStitcher with the outer views sliding outwards (the output box grows at least once): the frames, one push late
    and closed with flush(), bit for bit; equal epochs and boxes; nothing cropped."""
    from stabstitch2_amd.online import (PipelinedOnlineStitcher, ThreeViewOnlineStitcher, PipelinedThreeViewOnlineStitcher)
    hrd, lrd = clipd
    d = drift_eager
    pipe = PipelinedOnlineStitcher(hip_nets, H, W, viewport=VIEWPORT, grow='refit')
    assert (pipe.hc, pipe.wc) == VIEWPORT
    outs = _push_drifting(pipe, hip_nets, hrd, lrd, N_DRIFT)
    frames = [f for o in outs for f in o] + pipe.flush()
    torch.cuda.synchronize()
    assert len(frames) == N_DRIFT and all(torch.equal(a, b) for a, b in zip(frames, d['frames']))
    assert pipe.canvas_epoch == d['epochs'][-1] >= 1 and pipe.canvas_box == d['st'].canvas_box
    assert pipe.clipped_frames == 0 and pipe.overflow_report() == d['report']
    # three views, 360 x 480 each; the drift of _push_drifting (the bias both pairs 1-2 and 2-3 are set off by walks from -216 by -6 LR
    # px per frame for 12 frames from frame 20) slides the OUTER views outwards by 72 LR px each against the middle one.  The viewport
    # is narrower than the natural box (about 986 x 394): the letterbox adds height, the width keeps the margin's 28 px a side.
    hr3, lr3 = synth.make_clip(16, H, W, seed=4, views=3)
    hrd3 = [[f.to(dev) for f in v] for v in hr3]
    lrd3 = [[f.to(dev) for f in v] for v in lr3]
    bias = hip_nets[0]._prepared()['r1']['fc'][2][1]

    def run(st):
        out = []
        try:
            for t in range(40):
                i = t % 16
                bias[0::2] = -216.0 - 6.0 * min(max(t - 19, 0), 12)
                out += st.push(hrd3[0][i], hrd3[1][i], hrd3[2][i], lrd3[0][i], lrd3[1][i], lrd3[2][i])
        finally:
            bias[0::2] = -216.0
        return out
    vp3 = (400, 900)
    plain = ThreeViewOnlineStitcher(hip_nets, H, W, viewport=vp3, grow='refit')
    ref = run(plain)
    pipe3 = PipelinedThreeViewOnlineStitcher(hip_nets, H, W, viewport=vp3, grow='refit')
    got = run(pipe3) + pipe3.flush()
    torch.cuda.synchronize()
    print('\n[refit, three views] %s' % (plain.overflow_report(),))
    assert len(got) == len(ref) == 40 and all(tuple(f.shape) == (3,) + vp3 for f in got)
    assert all(torch.equal(a, b) for a, b in zip(got, ref))
    assert pipe3.canvas_epoch == plain.canvas_epoch >= 1 and pipe3.canvas_box == plain.canvas_box
    assert pipe3.overflow_report() == plain.overflow_report()
    assert plain.clipped_frames == 0 and pipe3.clipped_frames == 0
    assert tuple(float(v) for v in pipe3.first_canvas.cpu()) == tuple(float(v) for v in plain.first_canvas.cpu())


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_viewport_and_refit_refusals(dev, hip_nets):
    from stabstitch2_amd import online as O
    classes = [(O.OnlineStitcher, {}), (O.MultiOnlineStitcher, dict(streams=2)), (O.ThreeViewOnlineStitcher, {}),
               (O.PipelinedOnlineStitcher, {}), (O.PipelinedMultiOnlineStitcher, dict(streams=2)),
               (O.PipelinedThreeViewOnlineStitcher, {})]
    for cls, kw in classes:
        with pytest.raises(ValueError, match='viewport'):
            cls(hip_nets, H, W, grow='refit', **kw)
        with pytest.raises(ValueError, match='viewport'):
            cls(hip_nets, H, W, viewport=(10, 640), **kw)
        with pytest.raises(ValueError, match='viewport'):
            cls(hip_nets, H, W, viewport=(480, 65536), **kw)
        with pytest.raises(ValueError, match='grow'):
            cls(hip_nets, H, W, grow='recapture', viewport=(480, 640), **kw)
        with pytest.raises(ValueError, match='zoom_limit'):
            cls(hip_nets, H, W, grow='refit', viewport=(480, 640), zoom_limit=-1.0, **kw)
        st = cls(hip_nets, H, W, grow='refit', viewport=(480, 640), **kw)
        assert (st.hc, st.wc) == (480, 640) and st.grow == 'refit'
