"""NV12 in and out on the GPU ("Frame formats"): every NV12 route of the library -- ingest, sink, the fused AVERAGE render,
the LINEAR frames render, push_nv12 of the streaming stitchers -- equals, byte for byte, the three-step chain it replaces: convert the
NV12 frame to packed BGR with tests/nv12_ref.py, run the packed-BGR route, convert the uint8 video frame to NV12 with nv12_ref.  The
frames hold random bytes over the full range in all three channels (luma below 16 and saturating chroma occur), and every case
runs on a dense frame (pitch = W) and on a padded surface (pitch = W + 14, other random bytes in the padding).
    python -m pytest tests -m gpu"""
import numpy as np
import pytest
import torch

import nv12_ref as N
from stabstitch2_amd import synth
from test_gpu_parity import dev, hip_nets  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

PAD = 14
_cache = {}


def _surface(dev, arr, w):
    """numpy uint8 [..., rows, pitch] -> the device tensor's leading w columns: an NV12 frame (batch) with row stride `pitch`."""
    return torch.from_numpy(arr).to(dev)[..., :w]


def _frames(dev, seed, n, h, w, pad):
    """n random NV12 frames of one view -> (device NV12 batch [n,h*3/2,w] with pitch w + pad, their conversion uint8 [n,h,w,3])."""
    rng = np.random.default_rng(seed)
    dense = np.stack([N.random_nv12(rng, h, w) for _ in range(n)], 0)
    padding = np.random.default_rng(seed + 1).integers(0, 256, (n, h // 2 * 3, pad), dtype=np.uint8)
    bgr = np.stack([N.nv12_to_bgr(f) for f in dense], 0)
    return _surface(dev, np.concatenate((dense, padding), 2), w), torch.from_numpy(bgr).to(dev)


def _padded_out(dev, rows, w, pad, n=None):
    """An output surface filled with 0xAB -> (the whole buffer, the [.., rows, w] view the kernels write)."""
    buf = torch.full(((rows, w + pad) if n is None else (n, rows, w + pad)), 0xAB, dtype=torch.uint8, device=dev)
    return buf, buf[..., :w]


# ------------------------------------------------------------------ ingest and sink
@pytest.mark.parametrize('pad', [0, PAD], ids=['dense', 'padded'])
@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('size,lr', [((12, 16), (12, 16)), ((12, 16), (6, 8)), ((14, 18), (5, 7))], ids=['same', 'half', 'general'])
def test_ingest_nv12_equals_ingest_u8_of_the_converted_frames(dev, size, lr, n, pad):
    from stabstitch2_amd import ops
    (h, w), (lh, lw) = size, lr
    nv, bgr = _frames(dev, 100 + h + n, n, h, w, pad)
    assert int(nv[:, :h].min()) < 16 and int(nv[:, h:].max()) > 240            # luma below black, chroma beyond the range
    hr_ref, lr_ref = ops.ingest_u8(bgr, lh, lw)
    hr, lrs = ops.ingest_nv12(nv, lh, lw)
    assert hr.shape == hr_ref.shape and torch.equal(hr, hr_ref)
    assert lrs.shape == lr_ref.shape and torch.equal(lrs, lr_ref)
    none, lr_only = ops.ingest_nv12(nv, lh, lw, want_hr=False)
    assert none is None and torch.equal(lr_only, lr_ref)
    hr1, lr1 = ops.ingest_nv12(nv[n - 1], lh, lw)                                # one frame [h*3/2, w]
    assert torch.equal(hr1, hr_ref[n - 1:]) and torch.equal(lr1, lr_ref[n - 1:])


@pytest.mark.parametrize('pad', [0, PAD], ids=['dense', 'padded'])
@pytest.mark.parametrize('size', [(2, 2), (18, 70), (6, 258)])
def test_bgr_to_nv12_equals_numpy(dev, size, pad):
    from stabstitch2_amd import ops
    h, w = size
    rng = np.random.default_rng(7 + w)
    bgr = rng.integers(0, 256, (2, h, w, 3), dtype=np.uint8)
    ref = np.stack([N.bgr_to_nv12(f) for f in bgr], 0)
    buf, out = _padded_out(dev, h // 2 * 3, w, pad, n=2)
    res = ops.bgr_to_nv12(torch.from_numpy(bgr).to(dev), out=out)
    assert np.array_equal(res.cpu().numpy(), ref)
    assert bool((buf[..., w:] == 0xAB).all())                                    # the padding is not written
    assert np.array_equal(ops.bgr_to_nv12(torch.from_numpy(bgr[1]).to(dev)).cpu().numpy(), ref[1])


# ------------------------------------------------------------------ the renders
# frame size -> canvas boxes (wmin, wmax, hmin, hmax) in HR px: canvases (18, 70) and (40, 130) -- no multiples of the 64 x 8 tile,
# more than one tile each way, far wider than the views: most samples fall outside the frames, the last tile column lies beyond
# every view's mesh
BOXES = {(18, 70): (-4.0, 66.0, -3.0, 15.0), (40, 130): (-10.0, 120.0, -8.0, 32.0)}
SHIFT = 6.0                                # HR px between neighbouring views


def _splines(dev, views, h, w, boxes):
    """Seeded meshes of `views` views on len(boxes) canvases -> (src [n,V,63,2], T [n,V,2,66])."""
    key = ('splines', views, h, w, tuple(boxes))
    if key not in _cache:
        from stabstitch2_amd import ops
        from stabstitch2_amd.spatial_network import get_rigid_mesh, get_norm_mesh
        g = torch.Generator().manual_seed(77 + views + h)
        rigid = get_rigid_mesh(1, 360, 480, device='cpu')[0]                              # [7,9,2] LR px
        meshes = []
        for v in range(views):
            per = []
            for _ in boxes:
                m = rigid.clone() + (torch.rand((7, 9, 2), generator=g) - 0.5) * 40.0
                m[..., 0] += v * SHIFT * 480.0 / w
                per.append(m)
            meshes.append(torch.stack(per, 0).contiguous().to(dev))
        bx = torch.tensor(list(boxes), dtype=torch.float32, device=dev)
        nrigid = get_norm_mesh(get_rigid_mesh(1, h, w, device=dev), h, w).contiguous()
        _cache[key] = ops.stream_splines(meshes, 126, bx, nrigid, h, w)
    return _cache[key]


def _unreached_tiles(fp, views, hc, wc):
    """Tiles of a footprint row that no view reaches: the fourth class counter (csrc/render.hip, render_order_kernel)."""
    ny, nx = (hc + 7) // 8 + 1, 2 * ((wc + 63) // 64) + 1
    return int(fp.view(torch.int32)[views * ny * nx * 2 + 4 * views + 3])


@pytest.mark.parametrize('footprint', [False, True], ids=['everywhere', 'footprint'])
@pytest.mark.parametrize('mode', ['NORMAL', 'FAST'])
@pytest.mark.parametrize('views', [2, 3])
def test_render_average_nv12_equals_the_u8_render_and_its_nv12(dev, views, mode, footprint):
    """out_format 'bgr' against ops.render_average_u8 on the converted frames, 'nv12' against numpy BGR -> NV12 of that; frames
    (12, 16) and (24, 36) on canvases (18, 70) and (40, 130), dense and padded surfaces on both sides."""
    from stabstitch2_amd import ops
    canvases = list(BOXES)
    for h, w in ((12, 16), (24, 36)):
        src, T = _splines(dev, views, h, w, tuple(BOXES[c] for c in canvases))
        for i, (hc, wc) in enumerate(canvases):
            fp = None
            if footprint:
                fp = ops.render_footprints(src[i:i + 1], T[i:i + 1], h, w, hc, wc)[0]
                assert _unreached_tiles(fp, views, hc, wc) > 0, (h, w, hc, wc)
            ref = None
            for pad in (0, PAD):
                per_view = [_frames(dev, 500 + 10 * v + h, 1, h, w, pad) for v in range(views)]
                nv, bgr = [p[0][0] for p in per_view], [p[1][0] for p in per_view]
                r = ops.render_average_u8(bgr, src[i], T[i], hc, wc, mode, footprint=fp)
                assert ref is None or torch.equal(r, ref)                        # (the padding holds other bytes, the frames do not)
                ref = r
                got = ops.render_average_nv12(nv, src[i], T[i], hc, wc, mode, footprint=fp)
                assert got.shape == ref.shape and torch.equal(got, ref), (h, w, hc, wc, pad, 'bgr')
                buf, out = _padded_out(dev, hc // 2 * 3, wc, pad)
                res = ops.render_average_nv12(nv, src[i], T[i], hc, wc, mode, footprint=fp, out_format='nv12', out=out)
                assert np.array_equal(res.cpu().numpy(), N.bgr_to_nv12(ref.cpu().numpy())), (h, w, hc, wc, pad, 'nv12')
                assert bool((buf[:, wc:] == 0xAB).all())
            # the case is what it claims: samples inside the frames (a picture) and outside them (black)
            px = ref.view(-1, 3).sum(1)
            assert int((px == 0).sum()) > hc * wc // 4 and int((px > 0).sum()) > 50, (h, w, hc, wc)


@pytest.mark.parametrize('mode', ['NORMAL', 'FAST'])
@pytest.mark.parametrize('views', [2, 3])
def test_render_linear_frames_nv12_equals_the_u8_render(dev, views, mode):
    """Two frames on different canvases in one call against ops.render_linear_frames on the converted frames."""
    from stabstitch2_amd import ops
    h, w = 24, 36
    sizes = [(40, 130), (18, 70)]
    src, T = _splines(dev, views, h, w, tuple(BOXES[c] for c in sizes))
    for pad in (0, PAD):
        per_view = [_frames(dev, 900 + v, 2, h, w, pad) for v in range(views)]
        ref = ops.render_linear_frames([p[1] for p in per_view], src, T, sizes, mode)
        got = ops.render_linear_frames_nv12([p[0] for p in per_view], src, T, sizes, mode)
        for g, r, s in zip(got, ref, sizes):
            assert g.shape == r.shape and g.dtype == torch.uint8 and torch.equal(g, r), (pad, s)
            assert int((r.view(-1, 3).sum(1) > 0).sum()) > 50


# ------------------------------------------------------------------ the stitchers
SH, SW, PUSHES = 180, 320, 9               # HR size; the window fill (7 pushes), the capture, one replay ... two of them
VIEWPORTS = {2: (204, 500), 3: (204, 660)}


def _clip(dev):
    """Seeded synthetic clip, three views, as a decoder would deliver it and as the reference side sees it:
    -> (NV12 frames numpy [3][PUSHES] of [SH*3/2, SW], their conversion to packed BGR on the device [3][PUSHES] of [SH,SW,3])."""
    if 'clip' not in _cache:
        hr, _ = synth.make_clip_device(PUSHES, SH, SW, seed=4, views=3, device=dev)
        u8 = hr.permute(0, 1, 3, 4, 2).round().clamp(0, 255).to(torch.uint8).cpu().numpy()
        nv = [[N.bgr_to_nv12(u8[v, t]) for t in range(PUSHES)] for v in range(3)]
        bgr = [[torch.from_numpy(N.nv12_to_bgr(f)).to(dev) for f in per] for per in nv]
        _cache['clip'] = (nv, bgr)
    return _cache['clip']


def _stream(st, push, frames, outs=None):
    """PUSHES pushes -> (frames handed out per push, graph nodes)."""
    got = []
    for t in range(PUSHES):
        args = [f[t] for f in frames]
        got.append(push(*args) if outs is None else push(*args, out=outs[t]))
    return got, st.graph_nodes


@pytest.mark.parametrize('cls,warp,fusion', [('two', 'NORMAL', 'AVERAGE'), ('two', 'FAST', 'LINEAR'), ('three', 'NORMAL', 'AVERAGE')])
def test_push_nv12_equals_push_u8_of_the_converted_frames(dev, hip_nets, cls, warp, fusion):
    """Nine pushes -- the window fill, the graph capture, a replay -- on a dense and on a padded surface: out='bgr' hands out
    push_u8's frames of the converted input byte for byte, out='nv12' their numpy BGR -> NV12, with push_u8's cadence and a graph
    of push_u8's size.  The format changes between pushes (dense: BGR for the fill, then NV12, BGR; padded: NV12 for the fill, then
    BGR, NV12): every phase is seen in both formats, and the graph captured under one replays under the other."""
    from stabstitch2_amd import online
    views = 2 if cls == 'two' else 3
    Cls = online.OnlineStitcher if cls == 'two' else online.ThreeViewOnlineStitcher
    mk = lambda: Cls(hip_nets, SH, SW, warp_mode=warp, fusion_mode=fusion, viewport=VIEWPORTS[views])
    nv, bgr = _clip(dev)
    ref_st = mk()
    ref, ref_nodes = _stream(ref_st, ref_st.push_u8, bgr[:views])
    assert [len(r) for r in ref] == [0] * 6 + [7, 1, 1] and ref_nodes
    hc, wc = VIEWPORTS[views]
    for pad, fill in ((0, 'bgr'), (PAD, 'nv12')):
        other = 'nv12' if fill == 'bgr' else 'bgr'
        outs = [fill] * 7 + [other, fill]
        surfaces = [[_surface(dev, np.concatenate((f, np.full((f.shape[0], pad), 0x5A, np.uint8)), 1), SW) for f in per]
                    for per in nv[:views]]
        st = mk()
        got, nodes = _stream(st, st.push_nv12, surfaces, outs)
        assert [len(g) for g in got] == [len(r) for r in ref]
        assert nodes == ref_nodes, (nodes, ref_nodes)
        for t, (g, r) in enumerate(zip(got, ref)):
            for a, b in zip(g, r):
                if outs[t] == 'bgr':
                    assert a.shape == (hc, wc, 3) and torch.equal(a, b), (pad, t)
                else:
                    assert a.shape == (hc // 2 * 3, wc) and a.dtype == torch.uint8
                    assert np.array_equal(a.cpu().numpy(), N.bgr_to_nv12(b.cpu().numpy())), (pad, t)


def test_push_nv12_refusals(dev, hip_nets):
    from stabstitch2_amd import online
    good = torch.zeros((SH // 2 * 3, SW), dtype=torch.uint8, device=dev)
    plain = online.OnlineStitcher(hip_nets, SH, SW)
    odd = online.OnlineStitcher(hip_nets, SH, SW, viewport=(205, 500))
    three = online.ThreeViewOnlineStitcher(hip_nets, SH, SW, viewport=(204, 661))
    for st, n in ((plain, 2), (odd, 2), (three, 3)):
        with pytest.raises(ValueError, match='even viewport'):
            st.push_nv12(*[good] * n, out='nv12')
    even = online.OnlineStitcher(hip_nets, SH, SW, viewport=VIEWPORTS[2])
    for bad in (torch.zeros((SH, SW, 3), dtype=torch.uint8, device=dev),                         # a BGR frame
                torch.zeros((SH // 2 * 3, SW + 2), dtype=torch.uint8, device=dev),               # another width
                torch.zeros((SH // 2 * 3, SW), dtype=torch.float32, device=dev),
                torch.zeros((SW, SH // 2 * 3), dtype=torch.uint8, device=dev).t()):              # columns that are not dense
        with pytest.raises(ValueError, match='NV12'):
            even.push_nv12(good, bad)
    with pytest.raises(ValueError, match="'bgr' or 'nv12'"):
        even.push_nv12(good, good, out='rgb')
    with pytest.raises(ValueError, match='even height and width'):
        online.OnlineStitcher(hip_nets, SH + 1, SW).push_nv12(good, good)
    for Pipe, n, name in ((online.PipelinedOnlineStitcher, 2, 'OnlineStitcher.push_nv12'),
                          (online.PipelinedThreeViewOnlineStitcher, 3, 'ThreeViewOnlineStitcher.push_nv12')):
        with pytest.raises(ValueError, match=name):
            Pipe(hip_nets, SH, SW, viewport=VIEWPORTS[n]).push_nv12(*[good] * n)
    assert all(s.frames_in == 0 for s in (plain, odd, three, even))              # refused before any state changed
