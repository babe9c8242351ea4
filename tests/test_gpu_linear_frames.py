"""The streaming stitchers' direct LINEAR render: ss_render_linear_frames(_u8) -- LINEAR fusion of frames that each have their own
canvas, three launches (four with three views) whatever the number of frames -- against the clip kernel bit for bit, and the
stitchers that use it (online.DIRECT_LINEAR) against the in-graph per-frame chain they replace.
    python -m pytest tests -m gpu"""
import pytest
import torch

from stabstitch2_amd import synth
from test_gpu_parity import dev, hip_nets  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


# ------------------------------------------------------------------ 1. the kernels against the clip kernels
H, W = 48, 64                              # HR frames
SHIFT = 32.0                               # HR px between neighbouring views: they overlap by half a frame
# frame -> (canvas box (wmin, wmax, hmin, hmax) in HR px, vertical stretch of the meshes, HR px between neighbouring views)
FRAMES = [
    ((30.0, 41.5, 10.0, 21.5), 1.0, SHIFT),        # 11 x 11, the minimum; over the seam of views 1 and 2
    ((20.0, 70.0, 0.0, 40.0), 1.0, SHIFT),         # wc = 50 < 64: a single partial column tile
    ((0.0, 129.0, 2.0, 47.5), 1.0, SHIFT),         # wc = 129 = 64 * 2 + 1, hc = 45: no multiple of 8
    ((10.0, 90.0, 0.0, 120.0), 2.5, SHIFT),        # hc = 120 > the 96-row strip: a strip seam inside the (stretched) overlap
    ((0.0, 150.0, 0.0, 48.0), 1.0, 80.0),          # the views lie 80 px apart: no overlap at all (no candidates, empty range)
    ((0.0, 28.0, 5.0, 45.0), 1.0, SHIFT),          # the second (and third) view misses the canvas entirely
]
SIZES = [(int(b[3] - b[2]), int(b[1] - b[0])) for b, _, _ in FRAMES]
PERM = [3, 5, 0, 4, 1, 2]
_kernel_cache = {}


def _kernel_case(dev, views):
    """-> (fp32 frames per view [6,3,H,W], their uint8 rounding [6,H,W,3], src [6,V,63,2], T [6,V,2,66]); seeded, once per V."""
    if views not in _kernel_cache:
        from stabstitch2_amd import ops
        from stabstitch2_amd.spatial_network import get_rigid_mesh, get_norm_mesh
        g = torch.Generator().manual_seed(1234 + views)
        n = len(FRAMES)
        hr = (torch.rand((views, n, 3, H, W), generator=g) * 255.0).to(dev)
        u8 = hr.permute(0, 1, 3, 4, 2).round().clamp(0, 255).to(torch.uint8).contiguous()
        rigid = get_rigid_mesh(1, 360, 480, device='cpu')[0]                              # [7,9,2] LR px
        meshes = []
        for v in range(views):
            per = []
            for _, stretch, shift in FRAMES:
                m = rigid.clone() + (torch.rand((7, 9, 2), generator=g) - 0.5) * 16.0     # +- 8 LR px = +- 1 HR px
                m[..., 1] *= stretch
                m[..., 0] += v * shift * 480.0 / W
                per.append(m)
            meshes.append(torch.stack(per, 0).contiguous().to(dev))                     # [6,7,9,2]
        boxes = torch.tensor([b for b, _, _ in FRAMES], dtype=torch.float32, device=dev)
        nrigid = get_norm_mesh(get_rigid_mesh(1, H, W, device=dev), H, W).contiguous()
        src, T = ops.stream_splines(meshes, 126, boxes, nrigid, H, W)
        _kernel_cache[views] = ([hr[v].contiguous() for v in range(views)], [u8[v].contiguous() for v in range(views)], src, T)
    return _kernel_cache[views]


def _clip_reference(dev, views, mode, u8):
    """Every frame through ops.render_linear_clip on its own, on its own canvas; once per case, never written again."""
    key = ('ref', views, mode, u8)
    if key not in _kernel_cache:
        from stabstitch2_amd import ops
        f32, f8, src, T = _kernel_case(dev, views)
        imgs = f8 if u8 else f32
        _kernel_cache[key] = [ops.render_linear_clip([x[i:i + 1] for x in imgs], src[i:i + 1], T[i:i + 1], hc, wc, mode)[0]
                              for i, (hc, wc) in enumerate(SIZES)]
    return _kernel_cache[key]


@pytest.mark.parametrize('u8', [False, True], ids=['fp32', 'uint8'])
@pytest.mark.parametrize('mode', ['NORMAL', 'FAST'])
@pytest.mark.parametrize('views', [2, 3])
def test_linear_frames_equal_the_clip_kernel(dev, views, mode, u8):
    """ONE call over six frames on six canvases (the minimum 11 x 11, a single partial column tile, wc = 64 k + 1, hc no multiple of
    8, hc above the strip height, views that do not overlap, a second view off the canvas) equals ops.render_linear_clip called on
    each frame alone, bit for bit: at the default strip height and at 17 rows per strip (seams all over the small canvases), and
    with the frames in another order (a frame's result does not depend on its position in the call)."""
    from stabstitch2_amd import ops, _hip
    assert SIZES == [(11, 11), (40, 50), (45, 129), (120, 80), (48, 150), (40, 28)]
    f32, f8, src, T = _kernel_case(dev, views)
    imgs = f8 if u8 else f32
    ref = _clip_reference(dev, views, mode, u8)
    # (the cases are what they claim, in the blender's own terms: a pixel is covered where a mask rounds to 1, it is an overlap
    # pixel where round(m1 m2) != 0 -- the NORMAL sampler leaves residues outside the image that do not round to 1)
    if not u8 and mode == 'NORMAL':
        for i, (hc, wc) in enumerate(SIZES):
            wv = ops.tps_warp_views([x[i] for x in f32], src[i], T[i], hc, wc, mode)
            cover = [int((wv[k, 3].round() != 0).sum()) for k in range(views)]
            both = int(((wv[0, 3] * wv[1, 3]).round() != 0).sum())
            assert cover[0] > 0, (i, cover)
            if i == 4:
                assert both == 0 and cover[1] > 0, (i, both, cover)
            elif i == 5:
                assert sum(cover[1:]) == 0, (i, cover)
            else:
                assert both > 0, (i, both, cover)
    try:
        for rows in (0, 17):
            _hip.lib().ss_linear_clip_set_rows(rows)
            got = ops.render_linear_frames(imgs, src, T, SIZES, mode)
            assert len(got) == len(SIZES)
            for i, (g, r) in enumerate(zip(got, ref)):
                assert g.shape == r.shape and g.dtype == r.dtype and torch.equal(g, r), (rows, i, SIZES[i])
            perm = torch.tensor(PERM, device=dev)
            got = ops.render_linear_frames([x[perm].contiguous() for x in imgs], src[perm].contiguous(), T[perm].contiguous(),
                                           [SIZES[j] for j in PERM], mode)
            for k, j in enumerate(PERM):
                assert torch.equal(got[k], ref[j]), (rows, 'permuted', k, j)
    finally:
        _hip.lib().ss_linear_clip_set_rows(0)
    # a single frame, into a tensor and a workspace of the caller's
    i = 2
    out = [torch.zeros_like(ref[i])]
    ws = ops.linear_frames_workspace([SIZES[i]], views, dev)
    res = ops.render_linear_frames([x[i:i + 1] for x in imgs], src[i:i + 1], T[i:i + 1], [SIZES[i]], mode, outs=out, ws=ws)
    assert res[0] is out[0] and torch.equal(out[0], ref[i])


# ------------------------------------------------------------------ the stitchers
SH, SW, PUSHES = 180, 320, 12              # HR size; 7 window-fill pushes + 5 steady-state ones
_clips = {}


def _clip(dev):
    """Seeded synthetic clip, three views: (hr [3,N,3,SH,SW], lr [3,N,3,360,480]) on the device, N = PUSHES + 2 (stream s of a
    MultiOnlineStitcher starts s frames in)."""
    if 'c' not in _clips:
        _clips['c'] = synth.make_clip_device(PUSHES + 2, SH, SW, seed=4, views=3, device=dev)
    return _clips['c']


def _args(dev, kind):
    hr, lr = _clip(dev)
    if kind == 'single':
        return lambda t: (hr[0, t:t + 1], hr[1, t:t + 1], lr[0, t:t + 1], lr[1, t:t + 1])
    if kind == 'three':
        return lambda t: tuple(hr[v, t:t + 1] for v in range(3)) + tuple(lr[v, t:t + 1] for v in range(3))
    # three streams: the pair (1, 2) from frame 0, the pair (2, 3) from frame 1, the pair (2, 1) from frame 2
    pairs = ((0, 1, 0), (1, 2, 1), (1, 0, 2))
    return lambda t: (torch.stack([hr[a, t + o] for a, _, o in pairs]), torch.stack([hr[b, t + o] for _, b, o in pairs]),
                      torch.stack([lr[a, t + o] for a, _, o in pairs]), torch.stack([lr[b, t + o] for _, b, o in pairs]))


def _build(nets, kind, warp, direct, monkeypatch, **kw):
    from stabstitch2_amd import online
    monkeypatch.setattr(online, 'DIRECT_LINEAR', bool(direct))
    if kind == 'single':
        return online.OnlineStitcher(nets, SH, SW, warp_mode=warp, fusion_mode='LINEAR', **kw)
    if kind == 'three':
        return online.ThreeViewOnlineStitcher(nets, SH, SW, warp_mode=warp, fusion_mode='LINEAR', **kw)
    return online.MultiOnlineStitcher(nets, SH, SW, streams=3, warp_mode=warp, fusion_mode='LINEAR', **kw)


def _flat(res):
    """A push's frames as one flat list (MultiOnlineStitcher: stream by stream)."""
    return [f for per in res for f in per] if res and isinstance(res[0], list) else list(res)


def _kernel_names(fn):
    from torch.profiler import profile, ProfilerActivity
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        res = fn()
        torch.cuda.synchronize()
    return res, [e.name for e in prof.events() if e.device_type.name == 'CUDA' and 'Memcpy' not in e.name and 'Memset' not in e.name]


def test_multi_stream_linear_push_launch_count(dev, hip_nets, monkeypatch):
    """A steady-state LINEAR push of three streams on three canvases of different sizes renders with exactly three lb_* launches
    (not three per stream) and none of the per-frame chain's kernels."""
    canvases = [(-10.0, 470.0, -8.0, 190.0), (-20.0, 480.0, -5.0, 188.0), (0.0, 455.0, -12.0, 195.0)]
    st = _build(hip_nets, 'multi', 'NORMAL', True, monkeypatch, canvases=canvases)
    args = _args(dev, 'multi')
    for t in range(9):
        st.push(*args(t))
    assert st._direct() and st.static is not None and st.graph is not None
    sizes = st.canvas_sizes
    assert sizes == [(198, 480), (193, 500), (207, 455)] and len(set(sizes)) == 3, sizes
    res, names = _kernel_names(lambda: st.push(*args(9)))
    assert [tuple(f[0].shape) for f in res] == [(3,) + s for s in sizes]
    lb = [k for k in names if 'lb_' in k]
    assert len(lb) == 3, names
    assert not [k for k in names if 'lb_blur' in k or 'tps_warp_views' in k], names


@pytest.mark.parametrize('warp', ['NORMAL', 'FAST'])
@pytest.mark.parametrize('kind', ['single', 'multi', 'three'])
def test_direct_linear_stitchers_equal_in_graph(dev, hip_nets, monkeypatch, kind, warp):
    """7 + 5 pushes: the stitcher with the direct LINEAR render (the graph ends with the splines, the push renders the caller's
    frames through ops.render_linear_frames) returns the frames of the stitcher that keeps the per-frame chain in its graph, bit
    for bit; it holds no static canvas, and its graph is shorter."""
    from stabstitch2_amd import online
    inside = _build(hip_nets, kind, warp, False, monkeypatch)
    direct = _build(hip_nets, kind, warp, True, monkeypatch)
    args = _args(dev, kind)
    emitted = 0
    for t in range(PUSHES):
        a, b = _flat(inside.push(*args(t))), _flat(direct.push(*args(t)))
        assert len(a) == len(b), (t, len(a), len(b))
        for i, (x, y) in enumerate(zip(a, b)):
            assert x.shape == y.shape and torch.equal(x, y), (kind, warp, t, i, float((x - y).abs().max()))
        emitted += len(b)
    n = 3 if kind == 'multi' else 1
    assert emitted == n * PUSHES
    assert direct._direct() and not inside._direct()
    assert direct.static['out'] is None and inside.static['out'] is not None
    assert inside.graph_nodes is not None and direct.graph_nodes is not None
    print('\n[graph nodes, %s %s LINEAR] in-graph %d, direct %d' % (kind, warp, inside.graph_nodes, direct.graph_nodes))
    assert direct.graph_nodes < inside.graph_nodes, (inside.graph_nodes, direct.graph_nodes)
    monkeypatch.setattr(online, 'DIRECT_LINEAR', True)
    assert not online.PipelinedOnlineStitcher(hip_nets, SH, SW, fusion_mode='LINEAR')._direct()


@pytest.mark.parametrize('kind', ['single', 'multi', 'three'])
def test_push_u8_linear_takes_the_uint8_route(dev, hip_nets, monkeypatch, kind):
    """push_u8 with LINEAR fusion: byte for byte ops.ingest_u8 -> push -> ops.canvas_to_u8, window fill and steady state; in the
    steady state the blend kernel writes the video frame itself (no canvas_to_u8 launch)."""
    from stabstitch2_amd import ops, pipeline
    hr, _ = _clip(dev)
    u8 = hr.permute(0, 1, 3, 4, 2).round().clamp(0, 255).to(torch.uint8).contiguous()          # [3,N,SH,SW,3]
    if kind == 'single':
        frames = lambda t: (u8[0, t], u8[1, t])
    elif kind == 'three':
        frames = lambda t: (u8[0, t], u8[1, t], u8[2, t])
    else:
        frames = lambda t: (torch.stack((u8[0, t], u8[1, t + 1], u8[1, t + 2])), torch.stack((u8[1, t], u8[2, t + 1], u8[0, t + 2])))
    a = _build(hip_nets, kind, 'NORMAL', True, monkeypatch)
    b = _build(hip_nets, kind, 'NORMAL', True, monkeypatch)
    for t in range(PUSHES):
        fr = frames(t)

        def push():
            return a.push_u8(*fr)
        got, names = _kernel_names(push) if t == PUSHES - 1 else (push(), None)
        got = _flat(got)
        if kind == 'multi':
            loaded = [ops.ingest_u8(f, pipeline.LR_H, pipeline.LR_W) for f in fr]
            ref = b.push(*[x[0] for x in loaded], *[x[1] for x in loaded])
        else:
            loaded = [ops.ingest_u8(f[None], pipeline.LR_H, pipeline.LR_W) for f in fr]
            ref = b.push(*[x[0] for x in loaded], *[x[1] for x in loaded])
        ref = [ops.canvas_to_u8(f[None])[0] for f in _flat(ref)]
        assert len(got) == len(ref) and (len(got) > 0) == (t >= 6), (t, len(got), len(ref))
        for i, (x, y) in enumerate(zip(got, ref)):
            assert x.dtype == torch.uint8 and x.shape == y.shape and torch.equal(x, y), (kind, t, i)
        if names is not None:
            assert a._u8_steady()
            assert not [k for k in names if 'canvas_u8' in k or 'canvas_to_u8' in k], names
            assert [k for k in names if 'lb_frames' in k], names


def test_direct_linear_follows_canvas_growth(dev, hip_nets, monkeypatch):
    """grow='recapture' with LINEAR fusion on the drifting stream of test_stream_canvas_growth_vs_oracle (cropped canvas): the
    canvas grows, the direct render's workspace and frames follow the new size, and every frame equals the in-graph stitcher's."""
    from test_gpu_stream_oracle import _oracle_bbox, _pair_args
    from stabstitch2_amd import online
    n, h, w = 24, 360, 640
    seq = ('c640', 0, False, n)
    bb = _oracle_bbox(seq)
    cw, ch = bb[1] - bb[0], bb[3] - bb[2]
    crop = [bb[0], bb[1] - 0.08 * cw, bb[2] + 0.05 * ch, bb[3]]
    sts = []
    for direct in (False, True):
        monkeypatch.setattr(online, 'DIRECT_LINEAR', direct)
        sts.append(online.OnlineStitcher(hip_nets, h, w, canvas=crop, fusion_mode='LINEAR', grow='recapture'))
    inside, direct = sts
    assert direct._direct() and not inside._direct()
    args = _pair_args(seq, dev)
    first = None
    for t in range(n):
        a, b = inside.push(*args(t)), direct.push(*args(t))
        torch.cuda.synchronize()                  # (the growth check reads the watcher one push later: make it land)
        if first is None and b:
            first = (direct.hc, direct.wc)
        assert len(a) == len(b), t
        assert (inside.hc, inside.wc, inside.canvas_epoch) == (direct.hc, direct.wc, direct.canvas_epoch), t
        for x, y in zip(a, b):
            assert tuple(y.shape) == (3, direct.hc, direct.wc), (t, tuple(y.shape), direct.hc, direct.wc)
            assert torch.equal(x, y), (t, float((x - y).abs().max()))
    assert direct.canvas_epoch >= 1
    assert (direct.hc, direct.wc) != first and direct.hc >= first[0] and direct.wc >= first[1], (first, direct.hc, direct.wc)
