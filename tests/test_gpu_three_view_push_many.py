"""ThreeViewOnlineStitcher.push_many / push_many_u8: k frame triples of ONE stream per call.  The chain-frames cost-volume launch
against ss_cost_volume on gathered pairs; the strided splines against contiguous copies; the batched stream against single pushes
bit for bit (deterministic kernel policy) with window fill, odd / repeated k and interleaved pushes, in both render modes, eager and
graph-captured, on its own and on a cropped canvas; uint8 in and out; the middle view's single trunk pass; against the CPU oracle
at 720p under the default kernel policy; canvas growth; graph reuse, recapture and eviction; refused inputs.
    python -m pytest tests -m gpu"""
import numpy as np
import pytest
import torch

from stabstitch2_amd import ops, synth
from test_gpu_parity import dev, hip_nets, close_boxes  # noqa: F401  (fixtures / helpers)
from test_gpu_stream_oracle import _equal
from test_gpu_push_many import _fresh_nets, _clip as _pair_clip

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

E = 126


# ------------------------------------------------------------------ 1. kernels
@pytest.mark.parametrize('k', [1, 3, 8, 32])
def test_cost_volume_chain_frames_equals_gathered_pairs(dev, k):
    """ss_cost_volume_chain_frames == ss_cost_volume on the gathered contiguous pairs (F[s + h][j], F[s + h][j + 1]), bit for bit,
    for a chain of three views and of two (one pair: OnlineStitcher's batched step) on TemporalNet's feature geometry; a NaN guard
    behind `out` stays untouched.  Two views: also equal to ss_cost_volume_shifted(n = 2 k, split = k, shift = 1) over the same
    features, the launch that step made before."""
    g = torch.Generator().manual_seed(100 + k)
    for views in (3, 2):
        S = views - 1
        F = torch.randn((views, k + 1, 45, 60, 128), generator=g).to(dev)
        shape = (2, S, k, 45, 60, 52)
        n = int(np.prod(shape))
        buf = torch.full((n + 4096,), float('nan'), device=dev)
        got = ops.cost_volume_chain_frames(F, 3, out=buf[:n].view(shape))
        x1 = torch.stack([F[s + h, j] for h in range(2) for s in range(S) for j in range(k)], 0).contiguous()
        x2 = torch.stack([F[s + h, j + 1] for h in range(2) for s in range(S) for j in range(k)], 0).contiguous()
        ref = ops.cost_volume(x1, x2, 3)
        torch.cuda.synchronize()
        assert torch.equal(got.reshape(ref.shape), ref), (views, k)
        assert bool(torch.isnan(buf[n:]).all()), 'wrote past out'
        if views == 2:
            Ff = F.view((2 * (k + 1),) + tuple(F.shape[2:]))
            old = ops.cost_volume(Ff[:-1], Ff[1:], 3, n=2 * k, split=k, shift=1)
            torch.cuda.synchronize()
            assert torch.equal(got.reshape(old.shape), old), ('split / shift', k)


def test_three_view_splines_frame_stride(dev):
    """ops.three_view_splines(frames=k, frame_stride=7 * 126) on the window-last meshes of SmoothNet windows == the same launch on
    contiguous copies, bit for bit."""
    from stabstitch2_amd.spatial_network import get_rigid_mesh, get_norm_mesh
    k, nw = 5, 11
    g = torch.Generator().manual_seed(5)
    rig = get_rigid_mesh(1, 360, 480, device='cpu').reshape(1, 1, 7, 9, 2)
    m1 = (rig + torch.randn((nw, 7, 7, 9, 2), generator=g) * 3.0).contiguous().to(dev)
    m2 = (rig + torch.randn((nw, 7, 7, 9, 2), generator=g) * 3.0).contiguous().to(dev)
    first = torch.tensor([-60.0, 1000.0, -40.0, 420.0], device=dev)
    box = torch.tensor([-90.0, 1100.0, -50.0, 430.0], device=dev)
    nrig = get_norm_mesh(get_rigid_mesh(1, 360, 640, device=dev), 360, 640).contiguous()
    c = nw - k                                          # pair (2, 3)'s frames start c windows further
    a = ops.three_view_splines(m1[0, -1], m2[0, -1], m1[c, -1], m2[c, -1], first, box, nrig, 360, 640, frames=k, frame_stride=7 * E)
    cp = lambda m, s: m[s:s + k, -1].contiguous()
    b = ops.three_view_splines(cp(m1, 0), cp(m2, 0), cp(m1, c), cp(m2, c), first, box, nrig, 360, 640)
    torch.cuda.synchronize()
    for x, y in zip(a[0], b[0]):
        assert torch.equal(x, y)
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert bool(torch.isfinite(a[2]).all())


# ------------------------------------------------------------------ 2. batched stream == single pushes, bit for bit
_clips = {}


def _clip(n, h, w, seed):
    """-> [hr1, hr2, hr3, lr1, lr2, lr3] device tensors [n,...] of a three-view clip."""
    key = (n, h, w, seed)
    if key not in _clips:
        hr, lr = synth.make_clip_device(n, h, w, seed=seed, views=3, device='cpu')
        _clips[key] = [hr[v] for v in range(3)] + [lr[v] for v in range(3)]
    return _clips[key]


def _u8(frames):
    return [f.permute(0, 2, 3, 1).round().clamp(0, 255).to(torch.uint8).contiguous() for f in frames[:3]]


# calls: an int k = push_many of k frame triples, 'p' = one plain push.  The window fill ends inside the second call (whose steady
# part is a batch of 6), odd k, k = 1, a repeated k (6) whose graph is replayed, pushes in between.
SCHEDULE = [5, 8, 'p', 3, 1, 'p', 8, 6]


def _feed(st, schedule, frames, u8=False):
    """-> every frame the calls return, in order."""
    out, t = [], 0
    for c in schedule:
        n = 1 if c == 'p' else c
        part = [f[t:t + n] for f in frames]
        if c == 'p':
            out += st.push_u8(*[p[0] for p in part]) if u8 else st.push(*part)
        else:
            out += st.push_many_u8(*part) if u8 else st.push_many(*part)
        t += n
    torch.cuda.synchronize()
    return out


def _singles(st, n, frames, u8=False, t0=0):
    out = []
    for t in range(t0, t0 + n):
        out += st.push_u8(*[f[t] for f in frames]) if u8 else st.push(*[f[t:t + 1] for f in frames])
    torch.cuda.synchronize()
    return out


def _same_stream(a, b, what):
    assert (a.hc, a.wc) == (b.hc, b.wc) and a.frames_in == b.frames_in, what
    ra, rb = a.overflow_report(), b.overflow_report()
    assert ra == rb, (what, ra, rb)
    return ra


_canvases = {}


def _cropped_canvas(nets, frames, h, w, seed):
    """The output canvas a three-view stream fixes for itself after its first window, right edge 8 % of its width in and top 5 % of
    its height down."""
    if (h, w, seed) not in _canvases:
        from stabstitch2_amd.online import ThreeViewOnlineStitcher
        st = ThreeViewOnlineStitcher(nets, h, w, use_graph=False, deterministic=True)
        for t in range(7):
            st.push(*[f[t:t + 1] for f in frames])
        bb = st.bbox.cpu().tolist()
        cw, ch = bb[1] - bb[0], bb[3] - bb[2]
        _canvases[(h, w, seed)] = [bb[0], bb[1] - 0.08 * cw, bb[2] + 0.05 * ch, bb[3]]
    return _canvases[(h, w, seed)]


@pytest.mark.parametrize('canvas', ['own', 'cropped'])
@pytest.mark.parametrize('use_graph', [True, False], ids=['graph', 'eager'])
@pytest.mark.parametrize('warp,fusion', [('NORMAL', 'AVERAGE'), ('FAST', 'LINEAR')])
def test_three_view_push_many_equals_single_pushes(dev, hip_nets, warp, fusion, use_graph, canvas):
    """deterministic=True, 180x320, 33 triples through SCHEDULE against a stitcher fed the same triples one push at a time: every
    frame bit for bit, the canvas size, frames_in and overflow_report(), the captured batch sizes.  The cropped canvas
    (grow='never') clips frames."""
    from stabstitch2_amd.online import ThreeViewOnlineStitcher
    h, w = 180, 320
    n = sum(1 if c == 'p' else c for c in SCHEDULE)
    frames = [t.to(dev) for t in _clip(n, h, w, 31)]
    cv = None if canvas == 'own' else _cropped_canvas(hip_nets, frames, h, w, 31)
    mk = lambda: ThreeViewOnlineStitcher(hip_nets, h, w, canvas=cv, warp_mode=warp, fusion_mode=fusion, use_graph=use_graph,
                                         deterministic=True)
    ref_st, st = mk(), mk()
    ref = _singles(ref_st, n, frames)
    got = _feed(st, SCHEDULE, frames)
    assert len(got) == n == len(ref)                # (nothing for the first 6 triples, 7 frames at the 7th, then one per triple)
    _equal(got, ref, 'three-view push_many vs push %s/%s graph=%s %s' % (warp, fusion, use_graph, canvas))
    rep = _same_stream(st, ref_st, canvas)
    assert rep['frames_seen'] == n
    if canvas == 'cropped':
        assert rep['clipped_frames'] > 0, rep
    if use_graph:
        assert sorted(st.graph_nodes_batch) == [1, 3, 6, 8] and st.batch_captures == 4
    else:
        assert st.batch_captures == 0 and sorted(st._batch) == [1, 3, 6, 8]


@pytest.mark.parametrize('fusion', ['AVERAGE', 'LINEAR'])
def test_three_view_push_many_u8_equals_push_u8(dev, hip_nets, fusion):
    """push_many_u8 == push_u8 byte for byte at the odd geometry 251x377 (deterministic kernel policy), through SCHEDULE."""
    from stabstitch2_amd.online import ThreeViewOnlineStitcher
    h, w = 251, 377
    n = sum(1 if c == 'p' else c for c in SCHEDULE)
    u8 = [f.to(dev) for f in _u8(_clip(n, h, w, 11))]
    mk = lambda: ThreeViewOnlineStitcher(hip_nets, h, w, fusion_mode=fusion, deterministic=True)
    ref_st, st = mk(), mk()
    ref = _singles(ref_st, n, u8, u8=True)
    got = _feed(st, SCHEDULE, u8, u8=True)
    assert len(got) == n and all(f.dtype == torch.uint8 and f.shape[-1] == 3 for f in got)
    _equal(got, ref, 'three-view push_many_u8 vs push_u8 %s' % fusion)
    _same_stream(st, ref_st, 'u8 ' + fusion)


@pytest.mark.parametrize('use_graph', [True, False], ids=['graph', 'eager'])
@pytest.mark.parametrize('views', [2, 3], ids=['two-view', 'three-view'])
def test_batched_step_leaves_the_state_of_single_pushes(dev, hip_nets, views, use_graph):
    """The k-frame step both classes share (_PairStep._batch_meshes) against single pushes, deterministic=True, 180x320: 7 plain
    pushes, then push_many of k = 1 (one new row: the in-place views degenerate), k = 2 (the smallest k with a shifted pair inside
    the batch) and k = 8 > WINDOW (every ring row comes from the work rows); a reference stitcher takes the same 18 frames one push
    at a time.  Every returned frame and overflow_report(), then prev_feat, ring and the previous motions pair_s[:, 0] (three
    views: the chains') bit for bit.  pair_s[:, 1], the `new` slot, is not compared: a single push writes it before it reads it and
    leaves it equal to slot 0, a batched step does not write it (it holds what the last single push left), and nothing reads it
    before the next write."""
    from stabstitch2_amd.online import OnlineStitcher, ThreeViewOnlineStitcher, WINDOW
    h, w, ks = 180, 320, (1, 2, 8)
    assert ks[-1] > WINDOW
    n = 7 + sum(ks)
    if views == 2:
        hr, lr = _pair_clip(n, h, w, 31)
        frames = [t.to(dev) for t in (hr[0], hr[1], lr[0], lr[1])]
    else:
        frames = [t.to(dev) for t in _clip(n, h, w, 31)]
    cls = OnlineStitcher if views == 2 else ThreeViewOnlineStitcher
    mk = lambda: cls(hip_nets, h, w, use_graph=use_graph, deterministic=True)
    ref_st, st = mk(), mk()
    ref = _singles(ref_st, n, frames)
    got, t = _singles(st, 7, frames), 7
    for k in ks:
        got += st.push_many(*[f[t:t + k] for f in frames])
        t += k
    torch.cuda.synchronize()
    assert len(got) == n == len(ref)
    _equal(got, ref, '%d-view batched step vs single pushes, graph=%s' % (views, use_graph))
    rep = _same_stream(st, ref_st, 'batched step')
    assert rep['frames_seen'] == n
    a, b = (st.static, ref_st.static) if views == 2 else (st.chains.static, ref_st.chains.static)
    for name in ('prev_feat', 'ring'):
        assert torch.equal(a[name], b[name]), name
    assert torch.equal(a['pair_s'][:, 0], b['pair_s'][:, 0]), 'pair_s[:, 0]'


def test_three_view_push_many_passes_each_view_once(dev, hip_nets):
    """The batched step sends the three views' k frames through the twin trunks ONCE: one stem launch over 3 k images (not 4 k), as
    the single push's chain mode does for one triple."""
    from stabstitch2_amd.online import ThreeViewOnlineStitcher
    h, w, k = 180, 320, 5
    frames = [t.to(dev) for t in _clip(7 + k, h, w, 4)]
    st = ThreeViewOnlineStitcher(hip_nets, h, w, use_graph=False)
    st.push_many(*[f[:7] for f in frames])
    stems = []
    real = ops.H.call

    def spy(name, *a):
        if name == 'ss_stem_pool':
            stems.append(a[4])                   # images of the launch
        return real(name, *a)
    ops.H.call = spy
    try:
        got = st.push_many(*[f[7:] for f in frames])
    finally:
        ops.H.call = real
    torch.cuda.synchronize()
    assert len(got) == k and stems == [3 * k], stems


# ------------------------------------------------------------------ 3. against the oracle at 720p, default kernel policy
_o720 = {}


def _oracle_720():
    """The CPU oracle's three-view run on synth.make_clip(16, 720, 1280, seed=7, views=3), once: the two boxes (first canvas, output
    canvas), the composed meshes and the frames of both fusions with their box statistics."""
    if not _o720:
        import cases
        from oracle import pipeline as P
        from test_gpu_parity import _oracle_nets
        n, h, w, k = 16, 720, 1280, 16
        hr, lr = synth.make_clip(n, h, w, seed=7, views=3)
        nets = _oracle_nets()
        a12 = P.estimate_meshes(nets, lr[0], lr[1])
        a23 = P.estimate_meshes(nets, lr[1], lr[2])
        s = lambda m: P._scale_to_hr(m, h, w)
        w12_1, w12_2, w23_1, w23_2 = s(a12['smooth_mesh1']), s(a12['smooth_mesh2']), s(a23['smooth_mesh1']), s(a23['smooth_mesh2'])
        off = (w12_2 - w23_1).reshape(1, n, -1, 2).mean(dim=2).unsqueeze(2).unsqueeze(2)
        _o720['first'] = [float(v) for v in P._bbox([w12_1, w12_2, w23_1 + off, w23_2 + off])]
        om1, omid, om3 = P.three_view_compose(a12['smooth_mesh1'], a12['smooth_mesh2'], a23['smooth_mesh1'], a23['smooth_mesh2'], h, w)
        box = [float(v) for v in P._bbox([om1, omid, om3])]
        _o720['box'], _o720['xmid'] = box, float(omid[..., 0].max())
        _o720['frames'] = [torch.cat(v, 0) for v in hr] + [torch.cat(v, 0) for v in lr]
        for fusion in ('AVERAGE', 'LINEAR'):
            ofr, owc, ohc = P.three_view_render(hr[0], hr[1], hr[2], om1, omid, om3, 'NORMAL', fusion)
            ref = np.stack([cases.box_down(f.numpy().transpose(1, 2, 0), k) for f in ofr])
            rng = np.stack([cases.box_iqr(f.numpy().transpose(1, 2, 0), k) for f in ofr])
            _o720[fusion] = (ref, rng, int(ohc), int(owc))
    return _o720


@pytest.mark.parametrize('fusion', ['AVERAGE', 'LINEAR'])
def test_three_view_push_many_720p_vs_oracle(dev, hip_nets, fusion):
    """720x1280, 16 triples (synth seed 7) on the oracle's two boxes, in batches that reach a steady k = 4 ([4] * 4) and k = 8
    ([8, 8]): canvas size equal to the oracle's, nothing clipped, every frame within the gates of test_three_view_stream_vs_oracle_720p
    (AVERAGE: views-1-2 region p99 < 0.05 and max < 3.0 grey levels, clean-box median < 0.02; LINEAR: close_boxes 0.3, cover 0.5),
    and within 1e-3 grey levels (median) of single pushes (the networks' kernels are chosen per launch size).  The AVERAGE gate's
    cover share on these 16 frames, computed with the oracle alone on the CPU: ok.mean() = 0.627 (> 0.3, the existing test's
    condition)."""
    import cases
    from stabstitch2_amd.online import ThreeViewOnlineStitcher
    n, h, w, kb = 16, 720, 1280, 16
    o = _oracle_720()
    ref, rng, ohc, owc = o[fusion]
    frames = [t.to(dev) for t in o['frames']]
    mk = lambda: ThreeViewOnlineStitcher(hip_nets, h, w, canvas=o['box'], first_canvas=o['first'], fusion_mode=fusion)
    single = _singles(mk(), n, frames)
    for sched in ([4] * 4, [8, 8]):
        st = mk()
        got = _feed(st, sched, frames)
        assert len(got) == n and (st.hc, st.wc) == (ohc, owc)
        rep = st.overflow_report()
        assert rep['frames_seen'] == n and rep['clipped_frames'] == 0, rep
        g = np.stack([cases.box_down(f.permute(1, 2, 0).cpu().numpy(), kb) for f in got])
        if fusion == 'AVERAGE':
            xlim = int((o['xmid'] - o['box'][0]) // kb) - 1
            ok = cases.smooth_boxes(rng, kb)
            ok[:, :, xlim:] = False
            assert ok.mean() > 0.3, ok.mean()
            dd = np.abs(g - ref)[ok]
            print('\n[3-view push_many %s vs oracle, AVERAGE] p99 %.3e max %.3e' % (sched, np.quantile(dd, 0.99), dd.max()))
            assert np.quantile(dd, 0.99) < 0.05 and dd.max() < 3.0, (sched, float(np.quantile(dd, 0.99)), float(dd.max()))
            clean = cases.smooth_boxes(rng, kb)
            assert np.median(np.abs(g - ref)[clean]) < 0.02
        else:
            close_boxes(g, ref, rng, 0.3, 'three-view LINEAR push_many %s vs oracle' % sched, k=kb, cover=0.5)
        med = max(float((a - b).abs().median()) for a, b in zip(got, single))
        print('[3-view push_many %s vs single pushes, %s] worst frame median %.2e' % (sched, fusion, med))
        assert med < 1e-3, (sched, med)


# ------------------------------------------------------------------ 4. canvas growth
def test_three_view_push_many_canvas_growth(dev, hip_nets):
    """grow='recapture' from an output canvas cropped from the stream's own first-window box, batches of 4 (deterministic policy):
    the canvas grows, fewer frames are clipped than with grow='never' on the same triples, the final canvas holds every composed
    mesh, and every frame of the calls after the last growth equals single pushes on the final canvas."""
    from stabstitch2_amd.online import ThreeViewOnlineStitcher
    n, h, w, k = 24, 180, 320, 4
    frames = [t.to(dev) for t in _clip(n, h, w, 9)]
    crop = _cropped_canvas(hip_nets, frames, h, w, 9)

    def run(grow):
        st = ThreeViewOnlineStitcher(hip_nets, h, w, canvas=crop, grow=grow, deterministic=True)
        outs, epochs = [], []
        for c in range(n // k):
            outs.append(st.push_many(*[f[c * k:(c + 1) * k] for f in frames]))
            torch.cuda.synchronize()             # (the growth check reads the watcher one call later: make it land)
            epochs.append(st.canvas_epoch)
        return st, outs, epochs
    never, _, _ = run('never')
    st, outs, epochs = run('recapture')
    rn, rg = never.overflow_report(), st.overflow_report()
    assert rn['frames_seen'] == rg['frames_seen'] == n
    assert st.canvas_epoch >= 1, epochs
    assert rg['clipped_frames'] < rn['clipped_frames'], (rg, rn)
    last = max(c for c in range(len(epochs)) if epochs[c] != (epochs[c - 1] if c else 0))
    assert last >= 2, epochs                     # (the first call that can see the watcher's copy is the third)
    final = st.bbox.cpu().tolist()
    # single pushes on the final canvas (same first canvas): their composed meshes are the stream's (they do not depend on the
    # output canvas), recorded per frame -- eagerly, so that every push passes through _render
    ref_st = ThreeViewOnlineStitcher(hip_nets, h, w, canvas=final, first_canvas=st.first_canvas.cpu().tolist(), use_graph=False,
                                     deterministic=True)
    meshes = []
    real = ref_st._render

    def rec(imgs, m, out=None, splines=None):
        meshes.append(torch.cat([x.reshape(-1, 2) for x in m], 0).cpu())
        return real(imgs, m, out, splines)
    ref_st._render = rec
    ref = _singles(ref_st, n, frames)
    assert len(meshes) == n
    m = torch.cat(meshes, 0)
    tol = 0.05
    assert float(m[:, 0].min()) >= final[0] - tol and float(m[:, 0].max()) <= final[1] + tol, (final, crop)
    assert float(m[:, 1].min()) >= final[2] - tol and float(m[:, 1].max()) <= final[3] + tol, (final, crop)
    assert (st.hc, st.wc) == (ref_st.hc, ref_st.wc)
    assert all(len(outs[c]) == k for c in range(last, len(outs)))
    got = [f for c in range(last, len(outs)) for f in outs[c]]
    _equal(got, ref[last * k:], 'three-view push_many after its last growth')


# ------------------------------------------------------------------ 5. graphs
def test_three_view_push_many_graphs_reuse_recapture_evict(dev):
    """A repeated k replays its graph; reloading a net's weights recaptures and the frames follow the new weights (equal to single
    pushes that saw the same reload); a fifth batch size drops the least recently used one."""
    from stabstitch2_amd.online import ThreeViewOnlineStitcher, BATCH_GRAPHS
    nets = _fresh_nets(dev)
    h, w = 180, 320
    n = 7 + 4 + 2 * 4 + 4 + 1 + 2 + 3 + 5 + 2 + 1
    frames = [t.to(dev) for t in _clip(n, h, w, 5)]
    st = ThreeViewOnlineStitcher(nets, h, w, deterministic=True)
    ref_st = ThreeViewOnlineStitcher(nets, h, w, deterministic=True)
    t = 0

    def many(k):
        nonlocal t
        a = st.push_many(*[f[t:t + k] for f in frames])
        b = _singles(ref_st, k, frames, t0=t)
        t += k
        torch.cuda.synchronize()
        return a, b

    many(7)                                              # window fill only: nothing captured
    assert st.batch_captures == 0
    a, b = many(4)
    _equal(a, b, 'first k=4')
    assert st.batch_captures == 1 and list(st._batch) == [4]
    for _ in range(2):
        a, b = many(4)
        _equal(a, b, 'repeated k=4')
    assert st.batch_captures == 1
    # reload TemporalNet's weights: both stitchers recapture, the batched frames follow
    sd = synth.synthetic_state_dict(nets[1])
    sd['feature_extractor_stage1.0.weight'] = sd['feature_extractor_stage1.0.weight'] * 1.5
    nets[1].load_state_dict(sd, strict=True)
    a, b = many(4)
    _equal(a, b, 'k=4 after a reload')
    assert st.batch_captures == 2
    # LRU of BATCH_GRAPHS sizes
    assert BATCH_GRAPHS == 4
    for k in (1, 2, 3):
        many(k)
    assert list(st._batch) == [4, 1, 2, 3] and st.batch_captures == 5
    many(5)                                              # evicts 4
    assert list(st._batch) == [1, 2, 3, 5] and st.batch_captures == 6
    many(2)                                              # still held: replayed
    assert list(st._batch) == [1, 3, 5, 2] and st.batch_captures == 6
    a, b = many(1)
    _equal(a, b, 'k=1 after the LRU shuffle')
    assert st.batch_captures == 6 and t == n
    assert all(isinstance(st.graph_nodes_batch[k], (int, type(None))) for k in (1, 2, 3, 4, 5))


# ------------------------------------------------------------------ 6. refusals
def test_three_view_push_many_refusals_leave_the_stream_unchanged(dev, hip_nets, monkeypatch):
    """Every invalid push_many / push_many_u8 raises ValueError before any state changes: the calls that follow give the frames of a
    stitcher that never saw the bad input (window fill and steady state).  The pipelined class refuses both."""
    from stabstitch2_amd import layers as L
    from stabstitch2_amd.online import ThreeViewOnlineStitcher, PipelinedThreeViewOnlineStitcher
    h, w = 180, 320
    n = 16
    f = [t.to(dev) for t in _clip(n, h, w, 7)]
    u8 = [x.to(dev) for x in _u8(_clip(n, h, w, 7))]

    def bad_calls(st, t):
        h1, h2, h3, l1, l2, l3 = [x[t:t + 3] for x in f]
        u = [x[t:t + 3] for x in u8]
        cases = [
            lambda: st.push_many(h1, h2[:2], h3, l1, l2, l3),                        # leading dimensions disagree
            lambda: st.push_many(h1, h2, h3, l1, l2, l3[:2]),
            lambda: st.push_many(h1[:0], h2[:0], h3[:0], l1[:0], l2[:0], l3[:0]),     # k = 0
            lambda: st.push_many(*[x.repeat(11, 1, 1, 1) for x in (h1, h2, h3, l1, l2, l3)]),    # k = 33
            lambda: st.push_many(h1[:, :, :-1], h2[:, :, :-1], h3[:, :, :-1], l1, l2, l3),      # wrong frame size
            lambda: st.push_many(h1, h2, h3.transpose(2, 3), l1, l2, l3),           # transposed
            lambda: st.push_many(h1[0], h2[0], h3[0], l1[0], l2[0], l3[0]),         # wrong rank
            lambda: st.push_many(h1, h2.double(), h3, l1, l2, l3),                  # wrong dtype
            lambda: st.push_many(h1, h2, h3, l1, l2, l3[:, :, :-8]),                # wrong LR size
            lambda: st.push_many(u[0], u[1], u[2], l1, l2, l3),
            lambda: st.push_many_u8(u[0], u[1], u[2][:2]),
            lambda: st.push_many_u8(u[0].float(), u[1].float(), u[2].float()),
            lambda: st.push_many_u8(u[0][0], u[1][0], u[2][0]),                     # rank 3: [H,W,3] is one frame
            lambda: st.push_many_u8(u[0][:, :-1], u[1][:, :-1], u[2][:, :-1]),
            lambda: st.push_many_u8(u[0][:0], u[1][:0], u[2][:0]),
        ]
        for i, c in enumerate(cases):
            with pytest.raises(ValueError):
                c()
            assert st.frames_in == t, i
        monkeypatch.setattr(L, 'QUAD', False)
        with pytest.raises(ValueError):
            st.push_many(h1, h2, h3, l1, l2, l3)
        with pytest.raises(ValueError):
            st.push_many_u8(*u)
        monkeypatch.setattr(L, 'QUAD', True)
        assert st.frames_in == t

    a, b = ThreeViewOnlineStitcher(hip_nets, h, w), ThreeViewOnlineStitcher(hip_nets, h, w)
    got, ref = [], []
    for t0, k in ((0, 4), (4, 5), (9, 4), (13, 3)):
        bad_calls(a, t0)
        got += a.push_many(*[x[t0:t0 + k] for x in f])
        ref += b.push_many(*[x[t0:t0 + k] for x in f])
    torch.cuda.synchronize()
    _equal(got, ref, 'after refused calls')
    assert a.overflow_report() == b.overflow_report()
    pipe = PipelinedThreeViewOnlineStitcher(hip_nets, h, w)
    with pytest.raises(ValueError):
        pipe.push_many(*[x[:3] for x in f])
    with pytest.raises(ValueError):
        pipe.push_many_u8(*[x[:3] for x in u8])
    assert pipe.frames_in == 0
