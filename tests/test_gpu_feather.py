"""FEATHER fusion on the GPU (SS_FUSE_FEATHER): the fused render's FEATHER instantiations against the float64 statement
of tests/feather_ref.py inside its derived bound, the identities between the entry points bit for bit, and the streaming stitchers
under fusion_mode='FEATHER' against the ops render of their own splines and against each other.
    python -m pytest tests -m gpu"""
import functools
import gc

import numpy as np
import pytest
import torch

import feather_ref as FR
import nv12_ref as N
import sweep_inputs as G
from stabstitch2_amd import synth
from test_gpu_parity import dev, hip_nets  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
T = torch.from_numpy
# frame h, w, canvas hc, wc: the tile-edge canvases of the AVERAGE sweep (test_gpu_kernel_sweeps.WARP_CASES), and a small frame on a
# canvas of two partial tile columns
CASES = [(72, 96, 80, 120), (72, 96, 81, 129), (72, 96, 85, 191), (72, 96, 84, 128), (72, 96, 87, 65), (36, 48, 43, 67)]
GAINS = np.array([[0.7, 1.0, 1.3], [1.2, 0.9, 1.1], [0.8, 1.25, 1.0]], np.float32)


@functools.lru_cache(maxsize=None)
def _inputs(size, views, seed):
    h, w, hc, wc = size
    U, src, tgt = G.warp_case(views, h, w, hc, wc, seed=seed)
    return np.ascontiguousarray(U[:, :3]), src, tgt


def _device(dev, U, src, tgt):
    from stabstitch2_amd import ops
    sd = T(src).to(dev)
    return [T(np.ascontiguousarray(u)).to(dev) for u in U], sd, ops.tps_solve(sd, T(tgt).to(dev))


# ================================================================================================ the kernels against float64
@pytest.mark.parametrize('mode', ['NORMAL', 'FAST'])
@pytest.mark.parametrize('seed', [11, 12])
@pytest.mark.parametrize('views', [2, 3])
@pytest.mark.parametrize('size', CASES, ids=lambda s: '%dx%d_to_%dx%d' % s)
def test_feather_render_against_fp64(dev, size, views, seed, mode):
    """ss_render_average with SS_FUSE_FEATHER through the kernel's own ss_tps_solve, every pixel of full and partial 64 x 8 tiles,
    against feather_ref.feather64 inside feather_ref.bound (the dense-warp sweep's intensity gate for the samples, its coordinate
    gate for the weights, 8 ulp of 255 for the fuse; the fp32 restatement stays inside half of it: test_feather_abi).  Left out:
    pixels where a view is within 1e-4 of its border or 0 < den < 1e-3 -- at most 1 % of the canvas, or the case fails."""
    from stabstitch2_amd import ops
    h, w, hc, wc = size
    U, src, tgt = _inputs(size, views, seed)
    ref = FR.feather64(U, src, tgt, hc, wc, mode)
    planes, sd, Tk = _device(dev, U, src, tgt)
    got = ops.render_average(planes, sd, Tk, hc, wc, mode, fusion='FEATHER')
    ratio, share = FR.worst(got, ref, U, mode)
    if G.VERBOSE:
        print('  [feather] %s V%d seed %d %-6s worst |diff|/bound %.3f, left out %.3f %%' % (size, views, seed, mode, ratio, 100 * share))
    assert ratio <= 1.0, (ratio, share)
    reached = (ref['w'] > 0).sum(0)
    assert (reached >= 2).mean() >= 0.15                             # the views do overlap
    # not AVERAGE under another name: on the overlap the two formulas differ by grey levels
    avg = ops.render_average(planes, sd, Tk, hc, wc, mode)
    assert float((avg - got).abs().max()) > 1.0


@pytest.mark.parametrize('mode', ['NORMAL', 'FAST'])
@pytest.mark.parametrize('views', [2, 3])
def test_feather_render_with_gains_against_fp64(dev, views, mode):
    """The gain forms: every sample enters as min(g c, 255), gains distinct per view and channel, against the float64 statement."""
    from stabstitch2_amd import ops
    size = CASES[1]
    h, w, hc, wc = size
    U, src, tgt = _inputs(size, views, 11)
    ref = FR.feather64(U, src, tgt, hc, wc, mode, gains=GAINS[:views])
    assert (GAINS[:views, :, None, None] * ref['c'] > 255.0).mean() > 0.01        # the clamp is at work
    planes, sd, Tk = _device(dev, U, src, tgt)
    got = ops.render_average(planes, sd, Tk, hc, wc, mode, gains=T(GAINS[:views]).to(dev), fusion='FEATHER')
    ratio, share = FR.worst(got, ref, U, mode, gains=GAINS[:views])
    assert ratio <= 1.0, (ratio, share)
    plain = FR.feather64(U, src, tgt, hc, wc, mode)
    assert np.abs(plain['out'] - ref['out']).max() > 10.0


# ================================================================================================ identities, bit for bit
def _same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b), what


@pytest.mark.parametrize('mode', ['NORMAL', 'FAST'])
@pytest.mark.parametrize('views', [2, 3])
@pytest.mark.parametrize('size', [CASES[2], CASES[5]], ids=lambda s: '%dx%d_to_%dx%d' % s)
def test_feather_entry_points_agree_bit_for_bit(dev, size, views, mode):
    """Two frames on byte-exact planes: the clip forms == the single-frame forms; the uint8 forms == canvas_to_u8 of the fp32 form;
    gains of 1 == no gains; a footprint (with tiles that views do not reach) == no footprint, in every form."""
    from stabstitch2_amd import ops
    h, w, hc, wc = size
    U, src, tgt = G.warp_case(2 * views, h, w, hc, wc, seed=11)
    u8 = np.clip(np.rint(U[:, :3]), 0, 255).astype(np.uint8)
    sd = T(src).to(dev)
    Tk = ops.tps_solve(sd, T(tgt).to(dev))
    frames_u8 = [T(np.ascontiguousarray(u8[i].transpose(1, 2, 0))).to(dev) for i in range(2 * views)]
    planes = [ops.ingest_u8(f[None])[0][0] for f in frames_u8]
    src_c, T_c = sd.view(2, views, 63, 2), Tk.view(2, views, 2, 66)
    fps = ops.render_footprints(src_c, T_c, h, w, hc, wc)
    ones = torch.ones((2, views, 3), device=dev)
    kw = dict(fusion='FEATHER')
    want = []
    for f in range(2):
        sl = slice(f * views, (f + 1) * views)
        one = ops.render_average(planes[sl], sd[sl], Tk[sl], hc, wc, mode, **kw)
        want.append(one)
        one8 = ops.canvas_to_u8(one[None])[0]
        _same(ops.render_average_u8(frames_u8[sl], sd[sl], Tk[sl], hc, wc, mode, **kw), one8, ('u8', f))
        _same(ops.render_average(planes[sl], sd[sl], Tk[sl], hc, wc, mode, footprint=fps[f], **kw), one, ('footprint', f))
        _same(ops.render_average_u8(frames_u8[sl], sd[sl], Tk[sl], hc, wc, mode, footprint=fps[f], **kw), one8, ('u8 footprint', f))
        _same(ops.render_average(planes[sl], sd[sl], Tk[sl], hc, wc, mode, gains=ones[f], **kw), one, ('gains 1', f))
        _same(ops.render_average_u8(frames_u8[sl], sd[sl], Tk[sl], hc, wc, mode, gains=ones[f], footprint=fps[f], **kw), one8,
              ('u8 gains 1 footprint', f))
    want = torch.stack(want)
    want8 = ops.canvas_to_u8(want)
    clip = [torch.stack([planes[f * views + v] for f in range(2)]) for v in range(views)]
    clip8 = [torch.stack([frames_u8[f * views + v] for f in range(2)]) for v in range(views)]
    for fp in (None, fps):
        _same(ops.render_average_clip(clip, src_c, T_c, hc, wc, mode, footprint=fp, **kw), want, 'clip')
        _same(ops.render_average_clip_u8(clip8, src_c, T_c, hc, wc, mode, footprint=fp, **kw), want8, 'clip u8')
        _same(ops.render_average_clip(clip, src_c, T_c, hc, wc, mode, footprint=fp, gains=ones, **kw), want, 'clip gains 1')
        _same(ops.render_average_clip_u8(clip8, src_c, T_c, hc, wc, mode, footprint=fp, gains=ones, **kw), want8, 'clip u8 gains 1')
    # where the float64 coordinates put a view far outside a whole tile (0.4 of its half extent), the footprint has skipped something
    import ref64 as R
    xn, yn = R.tps_dense_coords(src[:views], R.tps_solve(src[:views], tgt[:views]), hc, wc)
    r = FR.border_distance(xn, yn)
    far = sum(bool((r[:, by:by + 8, bx:bx + 64].reshape(views, -1).max(1) < -0.4).any())
              for by in range(0, hc, 8) for bx in range(0, wc, 64))
    ny, nx = (hc + 7) // 8 + 1, 2 * ((wc + 63) // 64) + 1
    at = views * ny * nx * 2 + 4 * views                            # the class counters: tiles reached by 3, 2, 1, 0 views
    cls = fps[0].view(torch.int32)[at:at + 4].tolist()
    assert sum(cls) == ((hc + 7) // 8) * ((wc + 63) // 64) and sum(cls[4 - views:]) >= far, (cls, far)
    assert int((want8.view(-1, 3).sum(1) > 0).sum()) > 100


PAD = 14
# NV12 cases: frame (h, w), canvas (hc, wc) even, its box (wmin, wmax, hmin, hmax) in HR px -- partial tiles, canvases wider than the
# views; the last one is the smallest frame the NV12 routes take
NV12_CASES = [((12, 16), (18, 70), (-4.0, 66.0, -3.0, 15.0)), ((24, 36), (40, 130), (-10.0, 120.0, -8.0, 32.0)),
              ((2, 2), (6, 66), (-1.0, 4.0, -0.5, 2.5))]


def _nv12_frames(dev, seed, h, w, pad):
    """One random NV12 frame -> (the device surface [h*3/2, w] with row pitch w + pad, its conversion uint8 [h,w,3] on the device)."""
    dense = N.random_nv12(np.random.default_rng(seed), h, w)
    padding = np.random.default_rng(seed + 1).integers(0, 256, (h // 2 * 3, pad), dtype=np.uint8)
    return T(np.concatenate((dense, padding), 1)).to(dev)[:, :w], T(N.nv12_to_bgr(dense)).to(dev)


@pytest.mark.parametrize('mode', ['NORMAL', 'FAST'])
@pytest.mark.parametrize('views', [2, 3])
def test_feather_nv12_equals_the_u8_render_and_its_nv12(dev, views, mode):
    """NV12 in == ops.render_average_u8 on the nv12_ref-converted frames; NV12 out == nv12_ref.bgr_to_nv12 of that frame; dense and
    padded pitches on both sides, with and without a footprint, down to a 2 x 2 frame; the padding is not written."""
    from stabstitch2_amd import ops
    from stabstitch2_amd.spatial_network import get_rigid_mesh, get_norm_mesh
    for (h, w), (hc, wc), box in NV12_CASES:
        g = torch.Generator().manual_seed(31 + views + h)
        rigid = get_rigid_mesh(1, 360, 480, device='cpu')[0]
        meshes = []
        for v in range(views):
            m = rigid.clone() + (torch.rand((7, 9, 2), generator=g) - 0.5) * 40.0
            m[..., 0] += v * 6.0 * 480.0 / max(w, 16)
            meshes.append(m[None].contiguous().to(dev))
        nrigid = get_norm_mesh(get_rigid_mesh(1, h, w, device=dev), h, w).contiguous()
        src, Tk = ops.stream_splines(meshes, 126, torch.tensor([box], dtype=torch.float32, device=dev), nrigid, h, w)
        fp = ops.render_footprints(src, Tk, h, w, hc, wc)[0]
        ny, nx = (hc + 7) // 8 + 1, 2 * ((wc + 63) // 64) + 1
        if w >= 12:                              # (canvases far wider than the views: tiles that no view reaches)
            assert int(fp.view(torch.int32)[views * ny * nx * 2 + 4 * views + 3]) > 0, (h, w)
        ref = None
        for pad in (0, PAD):
            per = [_nv12_frames(dev, 500 + 10 * v + h, h, w, pad) for v in range(views)]
            nv, bgr = [p[0] for p in per], [p[1] for p in per]
            r = ops.render_average_u8(bgr, src[0], Tk[0], hc, wc, mode, fusion='FEATHER')
            assert ref is None or torch.equal(r, ref)
            ref = r
            for f in (None, fp):
                _same(ops.render_average_nv12(nv, src[0], Tk[0], hc, wc, mode, footprint=f, fusion='FEATHER'), ref, (h, w, pad, 'bgr'))
                buf = torch.full((hc // 2 * 3, wc + pad), 0xAB, dtype=torch.uint8, device=dev)
                res = ops.render_average_nv12(nv, src[0], Tk[0], hc, wc, mode, footprint=f, out_format='nv12', out=buf[:, :wc],
                                              fusion='FEATHER')
                assert np.array_equal(res.cpu().numpy(), N.bgr_to_nv12(ref.cpu().numpy())), (h, w, pad, 'nv12')
                assert bool((buf[:, wc:] == 0xAB).all())
        px = ref.view(-1, 3).sum(1)
        assert int((px == 0).sum()) > 0 and int((px > 0).sum()) > 30, (h, w)
        avg = ops.render_average_u8(bgr, src[0], Tk[0], hc, wc, mode)
        assert not torch.equal(avg, ref)


# ================================================================================================ the stitchers
SH, SW, PUSHES = 180, 320, 12              # the exposure tests' size; 7 window-fill pushes + 5 steady-state ones
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
    """The seeded three-view clip as a decoder delivers it -> dict(nv: NV12 frames numpy [3][PUSHES]; u8 [3,N,SH,SW,3]: their
    conversion; hr [3,N,3,SH,SW], lr [3,N,3,360,480]: ingest_u8's planes of those bytes) -- every route sees the same frames."""
    if 'clip' not in _runs:
        from stabstitch2_amd import ops, pipeline
        hr, _ = synth.make_clip_device(PUSHES, SH, SW, seed=4, views=3, device=dev)
        raw = hr.permute(0, 1, 3, 4, 2).round().clamp(0, 255).to(torch.uint8).cpu().numpy()
        nv = [[N.bgr_to_nv12(raw[v, t]) for t in range(PUSHES)] for v in range(3)]
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
    kw.setdefault('fusion_mode', 'FEATHER')
    return (online.OnlineStitcher if views == 2 else online.ThreeViewOnlineStitcher)(nets, SH, SW, **kw)


def _reference(dev, nets, views):
    """PUSHES deterministic pushes through the FEATHER stitcher of `views` views (captured graph, direct render), once."""
    key = ('ref', views)
    if key not in _runs:
        st = _make(nets, views, deterministic=True)
        frames = _push_all(st, dev, views)
        assert len(frames) == PUSHES and st._direct() and st.graph is not None and st._fused
        _runs[key] = (frames, st.graph_nodes, (st.hc, st.wc))
    return _runs[key]


def _same_lists(a, b, what):
    assert len(a) == len(b), (what, len(a), len(b))
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and x.dtype == y.dtype and torch.equal(x, y), (what, i)


@pytest.mark.parametrize('warp', ['NORMAL', 'FAST'])
@pytest.mark.parametrize('views', [2, 3])
def test_stream_frames_are_the_feather_render_of_their_own_splines(dev, hip_nets, views, warp, monkeypatch):
    """Every frame a FEATHER stitcher hands out (the window's seven, then five through the captured graph and the direct render) ==
    ops.render_average(fusion='FEATHER') on the stitcher's own solved splines and footprint of that frame, and is not AVERAGE's
    frame."""
    from stabstitch2_amd import online, ops, pipeline
    c = _clip(dev)
    Cls = online.OnlineStitcher if views == 2 else online.ThreeViewOnlineStitcher
    st = _make(hip_nets, views, warp_mode=warp)
    solved = []
    inner = online._Stitcher._render_solved

    def spy(self, imgs, src, Tk, *a, **kw):      # (on the class: a spy stored on the stitcher would tie it into a reference cycle)
        solved.append((src.clone(), Tk.clone()))
        return inner(self, imgs, src, Tk, *a, **kw)
    monkeypatch.setattr(Cls, '_render_solved', spy)
    emitted, differs = 0, False
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
            imgs = [c['hr'][v, ft:ft + 1] for v in range(views)]
            fp = ops.render_footprints(src[None], Tk[None], SH, SW, st.hc, st.wc)[0] if pipeline.SKIP_OUTSIDE else None
            want = ops.render_average(imgs, src, Tk, st.hc, st.wc, warp, footprint=fp, fusion='FEATHER')
            assert torch.equal(frame, want), (views, warp, t, ft, float((frame - want).abs().max()))
            differs |= float((ops.render_average(imgs, src, Tk, st.hc, st.wc, warp, footprint=fp) - frame).abs().max()) > 1.0
            emitted += 1
    assert emitted == PUSHES and st.graph is not None and st._direct() and differs


@pytest.mark.parametrize('views', [2, 3])
def test_push_u8_and_push_many_equal_the_pushes(dev, hip_nets, views):
    """push_u8 == canvas_to_u8 of push in the uint8 steady state; push_many / push_many_u8 at k = 4 (three calls, the window fills
    inside the second) == twelve pushes, under deterministic=True."""
    from stabstitch2_amd import ops
    c = _clip(dev)
    ref, nodes, _ = _reference(dev, hip_nets, views)
    ref8 = [ops.canvas_to_u8(f[None])[0] for f in ref]
    st = _make(hip_nets, views, deterministic=True)
    _same_lists(_push_all(st, dev, views, u8=True), ref8, 'push_u8')
    assert st._u8_steady() and st.graph_nodes == nodes
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


@pytest.mark.parametrize('views', [2, 3])
def test_push_nv12_equals_push_u8_of_the_converted_frames(dev, hip_nets, views):
    """Under a viewport, on a dense and on a padded surface: out='bgr' hands out push_u8's frames of the converted input, out='nv12'
    their numpy BGR -> NV12 (the render writes NV12 itself), the format changing between pushes; a graph of push_u8's size."""
    c = _clip(dev)
    n = 9
    ref_st = _make(hip_nets, views, viewport=VIEWPORTS[views])
    ref = [ref_st.push_u8(*[c['u8'][v, t] for v in range(views)]) for t in range(n)]
    assert [len(r) for r in ref] == [0] * 6 + [7, 1, 1] and ref_st.graph_nodes
    hc, wc = VIEWPORTS[views]
    for pad, fill in ((0, 'bgr'), (PAD, 'nv12')):
        other = 'nv12' if fill == 'bgr' else 'bgr'
        outs = [fill] * 7 + [other, fill]
        surf = [[T(np.concatenate((f, np.full((f.shape[0], pad), 0x5A, np.uint8)), 1)).to(dev)[:, :SW] for f in per[:n]]
                for per in c['nv'][:views]]
        st = _make(hip_nets, views, viewport=VIEWPORTS[views])
        got = [st.push_nv12(*[surf[v][t] for v in range(views)], out=outs[t]) for t in range(n)]
        assert [len(g) for g in got] == [len(r) for r in ref] and st.graph_nodes == ref_st.graph_nodes
        for t, (g, r) in enumerate(zip(got, ref)):
            for a, b in zip(g, r):
                if outs[t] == 'bgr':
                    assert a.shape == (hc, wc, 3) and torch.equal(a, b), (pad, t)
                else:
                    assert a.shape == (hc // 2 * 3, wc) and np.array_equal(a.cpu().numpy(), N.bgr_to_nv12(b.cpu().numpy())), (pad, t)


def test_pipelined_stitchers_equal_the_plain_ones_one_push_late(dev, hip_nets):
    """... and the plain FEATHER stitchers' graphs have as many nodes as the AVERAGE stitchers': the same launches."""
    from stabstitch2_amd import online
    for views, Pipe in ((2, online.PipelinedOnlineStitcher), (3, online.PipelinedThreeViewOnlineStitcher)):
        plain = _make(hip_nets, views)
        ref = _push_all(plain, dev, views)
        avg = _make(hip_nets, views, fusion_mode='AVERAGE')
        _push_all(avg, dev, views, n=9)
        assert plain.graph_nodes and avg.graph_nodes == plain.graph_nodes, (avg.graph_nodes, plain.graph_nodes)
        pipe = Pipe(hip_nets, SH, SW, fusion_mode='FEATHER')
        c = _clip(dev)
        got, counts = [], []
        for t in range(PUSHES):
            r = pipe.push(*([c['hr'][v, t:t + 1] for v in range(views)] + [c['lr'][v, t:t + 1] for v in range(views)]))
            counts.append(len(r))
            got += r
        got += pipe.flush()
        torch.cuda.synchronize()
        assert counts == [0] * 6 + [7, 0] + [1] * (PUSHES - 8) and pipe._fused and (pipe.hc, pipe.wc) == (plain.hc, plain.wc)
        _same_lists(got, ref, 'pipelined, %d views' % views)


def test_multi_stream_equals_the_single_streams(dev, hip_nets):
    """Two batched streams (the pair and its mirror) under deterministic=True == two OnlineStitchers, on their own canvases and on
    one shared canvas size (the clip-style render); the pipelined batch == the plain one, one push late."""
    from stabstitch2_amd import online
    c = _clip(dev)

    def batch(t):
        a, b = c['hr'][0, t:t + 1], c['hr'][1, t:t + 1]
        la, lb = c['lr'][0, t:t + 1], c['lr'][1, t:t + 1]
        return torch.cat((a, b)), torch.cat((b, a)), torch.cat((la, lb)), torch.cat((lb, la))
    for canvases in (None, [(-40.0, 400.0, -20.0, 200.0)] * 2):
        multi = online.MultiOnlineStitcher(hip_nets, SH, SW, streams=2, canvases=canvases, fusion_mode='FEATHER', deterministic=True)
        pipe = online.PipelinedMultiOnlineStitcher(hip_nets, SH, SW, streams=2, canvases=canvases, fusion_mode='FEATHER',
                                                   deterministic=True)
        single = [online.OnlineStitcher(hip_nets, SH, SW, canvas=None if canvases is None else canvases[s], fusion_mode='FEATHER',
                                        deterministic=True) for s in range(2)]
        got, late, want = [[], []], [[], []], [[], []]
        for t in range(PUSHES):
            x = batch(t)
            for s, fr in enumerate(multi.push(*x)):
                got[s] += fr
            for s, fr in enumerate(pipe.push(*x)):
                late[s] += fr
            for s in range(2):
                want[s] += single[s].push(*[v[s:s + 1] for v in x])
        for s, fr in enumerate(pipe.flush()):
            late[s] += fr
        torch.cuda.synchronize()
        assert multi._fused and multi.canvas_sizes == [(x.hc, x.wc) for x in single] == pipe.canvas_sizes
        for s in range(2):
            assert len(want[s]) == PUSHES
            _same_lists(got[s], want[s], ('multi', canvases is not None, s))
            _same_lists(late[s], want[s], ('pipelined multi', canvases is not None, s))


def test_exposure_stream_is_the_estimator_and_the_gain_render(dev, hip_nets, monkeypatch):
    """exposure=True under FEATHER: every frame == the stitcher's own splines and footprint -> ops.exposure_update on a state of the
    test's own -> ops.render_average(gains=, fusion='FEATHER'); the final gain state equals the test's."""
    from stabstitch2_amd import online, ops, pipeline
    c = _clip(dev)
    hr, lr = c['hr'].clone(), c['lr']
    hr[1] = (hr[1] * torch.tensor((0.8, 0.9, 1.1), device=dev).view(1, 3, 1, 1)).clamp(0, 255)      # a second camera exposed otherwise
    st = online.OnlineStitcher(hip_nets, SH, SW, fusion_mode='FEATHER', exposure=True)
    solved = []
    inner = online.OnlineStitcher._render_solved

    def spy(self, imgs, src, Tk, *a, **kw):
        solved.append((src.clone(), Tk.clone()))
        return inner(self, imgs, src, Tk, *a, **kw)
    monkeypatch.setattr(online.OnlineStitcher, '_render_solved', spy)
    mine = ops.exposure_state(dev)
    emitted = 0
    for t in range(PUSHES):
        solved.clear()
        got = st.push(hr[0, t:t + 1], hr[1, t:t + 1], lr[0, t:t + 1], lr[1, t:t + 1])
        if not got:
            continue
        splines, frames_t = (list(solved), range(7)) if len(got) == 7 else ([st._deferred[:2]], [t])
        for (src, Tk), ft, frame in zip(splines, frames_t, got):
            imgs = [hr[0, ft:ft + 1], hr[1, ft:ft + 1]]
            fp = ops.render_footprints(src[None], Tk[None], SH, SW, st.hc, st.wc)
            gains = ops.exposure_update(imgs, fp, st.hc, st.wc, mine, st.exposure, 'NORMAL')
            want = ops.render_average(imgs, src, Tk, st.hc, st.wc, 'NORMAL', footprint=fp[0] if pipeline.SKIP_OUTSIDE else None,
                                      gains=gains, fusion='FEATHER')
            assert torch.equal(frame, want), (t, ft, float((frame - want).abs().max()))
            emitted += 1
    assert emitted == PUSHES and st.graph is not None and st._direct()
    assert torch.equal(st._exp_state, mine) and int(mine.view(torch.int32)[9]) == 1
    assert float((st.exposure_gains - 1.0).abs().max()) > 0.02           # the gains are not the identity


def test_offline_paths_take_the_fused_render(dev, hip_nets):
    """pipeline.render_frames / render_frames_u8 under FEATHER: one clip launch with footprints == the per-frame ops renders; the
    uint8 path is the fused one; run_two_view_u8 == canvas_to_u8 of run_two_view."""
    from stabstitch2_amd import ops, pipeline
    c = _clip(dev)
    n = 7
    assert pipeline._u8_fused('FEATHER')
    f32, hc, wc, m1, m2 = pipeline.run_two_view(c['hr'][0, :n], c['hr'][1, :n], c['lr'][0, :n], c['lr'][1, :n], hip_nets,
                                                fusion_mode='FEATHER')
    avg = pipeline.run_two_view(c['hr'][0, :n], c['hr'][1, :n], c['lr'][0, :n], c['lr'][1, :n], hip_nets)[0]
    assert avg.shape == f32.shape and float((avg - f32).abs().max()) > 1.0
    hcp, wcp, src, Tk = pipeline.render_plan([m1, m2], SH, SW, False, None, None)
    assert (hcp, wcp) == (hc, wc)
    for i in (0, n - 1):
        want = ops.render_average([c['hr'][0, i], c['hr'][1, i]], src[i], Tk[i], hc, wc, fusion='FEATHER')
        assert torch.equal(f32[i], want), i
    u8, hc8, wc8 = pipeline.run_two_view_u8(c['u8'][0, :n], c['u8'][1, :n], hip_nets, fusion_mode='FEATHER')[:3]
    assert (hc8, wc8) == (hc, wc) and torch.equal(u8, ops.canvas_to_u8(f32))
