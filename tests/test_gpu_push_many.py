"""OnlineStitcher.push_many / push_many_u8: k frame pairs of ONE stream per call.  The two kernels behind the batched step against
the launches they replace; the batched stream against single pushes bit for bit (deterministic kernel policy) with window fill,
odd / repeated k and interleaved pushes, in both render modes, eager and graph-captured, on its own and on a cropped canvas; uint8
in and out; against the CPU oracle at 720p under the default kernel policy; canvas growth; graph reuse, recapture and eviction;
refused inputs.
    python -m pytest tests -m gpu"""
import pytest
import torch

from stabstitch2_amd import ops, synth
from test_gpu_parity import dev, hip_nets  # noqa: F401  (fixtures)
from test_gpu_stream_oracle import _seq, _oracle, _oracle_bbox, _hr_meshes, _vs_oracle, _pair_args, _run, _equal, _forget

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

E = 126


# ------------------------------------------------------------------ 1. kernels
@pytest.mark.parametrize('k', [1, 3, 8, 32])
def test_window_advance_equals_k_window_pushes(dev, k):
    """ss_window_advance == k calls of ss_window_push, bit for bit: the rings, the state blocks, and the work rows (window j of the
    batch = the ring after push j + 1)."""
    g = torch.Generator().manual_seed(k)
    W, R = 7, 4
    ring0 = torch.randn((R, W, E), generator=g).to(dev)
    src = torch.randn((2, 2 * (k + 1), E), generator=g).to(dev)         # the step's tsmotion rows [smesh | tsmotion][2 (k + 1)]
    n1 = k + 1
    offs = [(0 * n1 + 1) * E, (1 * n1 + 1) * E, (2 * n1 + 1) * E, (3 * n1 + 1) * E]
    # ss_window_push's state move (block b at b * 2E <- the block E further) against the same move as a copy from state + E
    state0 = torch.randn((2, 2, E), generator=g).to(dev)
    ring, state, windows = ring0.clone(), state0.clone(), []
    for j in range(k):
        ops.window_push(ring, src, [o + j * E for o in offs], state=state, blocks=2, block=E, stride=2 * E, delta=E)
        windows.append(ring.clone())
    ring2, state2 = ring0.clone(), state0.clone()
    work = torch.full((R, W - 1 + k, E), float('nan'), device=dev)
    ops.window_advance(ring2, work, src, offs, k, state=state2, state_src=state2.view(-1)[E:], blocks=2, block=E, stride=2 * E,
                       src_stride=2 * E)
    torch.cuda.synchronize()
    assert torch.equal(ring2, ring) and torch.equal(state2, state)
    for j in range(k):
        assert torch.equal(work[:, j:j + W], windows[j]), j
    # the push_many layout: pair_s[:, 0] <- the newest of [view][k + 1] motion rows
    sw = torch.randn((2, k + 1, E), generator=g).to(dev)
    ps = torch.randn((2, 2, E), generator=g).to(dev)
    keep = ps[:, 1].clone()
    ops.window_advance(ring0.clone(), work, src, offs, k, state=ps, state_src=sw.view(-1)[k * E:], blocks=2, block=E,
                       stride=2 * E, src_stride=(k + 1) * E)
    torch.cuda.synchronize()
    assert torch.equal(ps[:, 0], sw[:, k]) and torch.equal(ps[:, 1], keep)


def _watch_points(k, seed, nan_at=None, out_from=None):
    """[k,2,63,2] canvas-normalised control points: inside, a few frames near an edge, frames from `out_from` on outside."""
    g = torch.Generator().manual_seed(seed)
    src = torch.rand((k, 2, 63, 2), generator=g) * 1.8 - 0.9
    src[1::3, 0, 5, 0] = 0.99                                   # near the right edge (within a guard of 0.02)
    if out_from is not None:
        src[out_from::2, 1, 7, 1] = -1.05                       # outside, every other frame from out_from
    if nan_at is not None:
        src[nan_at, 0, 11, 0] = float('nan')
    return src


@pytest.mark.parametrize('guard', [0.0, 0.02])
def test_canvas_watch_frames_equals_sequential_watch(dev, guard):
    """ss_canvas_watch_frames == k sequential ss_canvas_watch calls on one row: on a row that has seen frames before, a batch whose
    first clip lies in its middle, a NaN point, near-edge frames."""
    for k, nan_at, out_from in ((9, None, 4), (5, 2, None), (1, None, None), (32, 7, 20)):
        src = _watch_points(k, k, nan_at, out_from).to(dev)
        wi, wf = ops.canvas_watch_state(1, dev)
        wi2, wf2 = ops.canvas_watch_state(1, dev)
        pre = _watch_points(3, 100).to(dev)                     # three frames already seen on this row
        for t in range(3):
            ops.canvas_watch(pre[t:t + 1].contiguous(), wi, wf, guard)
            ops.canvas_watch(pre[t:t + 1].contiguous(), wi2, wf2, guard)
        for t in range(k):
            ops.canvas_watch(src[t:t + 1].contiguous(), wi, wf, guard)
        ops.canvas_watch_frames(src, wi2, wf2, guard)
        torch.cuda.synchronize()
        assert torch.equal(wi2, wi) and torch.equal(wf2, wf), (k, wi2.tolist(), wi.tolist())
        row = wi[0].tolist()
        assert row[0] == 3 + k
        if out_from is not None:
            assert row[2] == 3 + (min(out_from, nan_at) if nan_at is not None else out_from)
        elif nan_at is not None:
            assert row[1] == 1 and row[2] == 3 + nan_at
        else:
            assert row[1] == 0 and row[2] == -1


def test_stream_splines_frames_broadcast_one_canvas(dev):
    """ops.stream_splines(frames=k) on ONE canvas == the same launch with the canvas repeated per frame."""
    from stabstitch2_amd.spatial_network import get_rigid_mesh, get_norm_mesh
    k = 5
    rig = get_rigid_mesh(1, 360, 480, device='cpu').reshape(1, 1, 1, 7, 9, 2)
    m = (rig + torch.randn((2, k, 7, 7, 9, 2), generator=torch.Generator().manual_seed(3)) * 4.0).contiguous().to(dev)
    box = torch.tensor([-40.0, 700.0, -30.0, 400.0], device=dev)
    nrig = get_norm_mesh(get_rigid_mesh(1, 360, 640, device=dev), 360, 640).contiguous()
    a = ops.stream_splines([m[0, 0, -1], m[1, 0, -1]], 7 * E, box, nrig, 360, 640, frames=k)
    b = ops.stream_splines([m[0, 0, -1], m[1, 0, -1]], 7 * E, box[None].repeat(k, 1).contiguous(), nrig, 360, 640)
    torch.cuda.synchronize()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ------------------------------------------------------------------ 2. batched stream == single pushes, bit for bit
_clips = {}


def _clip(n, h, w, seed):
    key = (n, h, w, seed)
    if key not in _clips:
        hr, lr = synth.make_clip_device(n, h, w, seed=seed, device='cpu')
        _clips[key] = (hr, lr)
    return _clips[key]


# calls: an int k = push_many of k frame pairs, 'p' = one plain push.  The window fill ends inside the second call (whose steady
# part is a batch of 6), odd k, k = 1, a repeated k (6) whose graph is replayed, pushes in between.
SCHEDULE = [5, 8, 'p', 3, 1, 'p', 8, 6]


def _feed(st, schedule, frames, u8=False):
    """-> every frame the calls return, in order."""
    out, t = [], 0
    for c in schedule:
        n = 1 if c == 'p' else c
        part = [f[t:t + n] for f in frames]
        if c == 'p':
            out += st.push_u8(part[0][0], part[1][0]) if u8 else st.push(*part)
        else:
            out += st.push_many_u8(*part) if u8 else st.push_many(*part)
        t += n
    torch.cuda.synchronize()
    return out


def _singles(st, n, frames, u8=False):
    out = []
    for t in range(n):
        out += st.push_u8(frames[0][t], frames[1][t]) if u8 else st.push(*[f[t:t + 1] for f in frames])
    torch.cuda.synchronize()
    return out


def _same_stream(a, b, what):
    assert (a.hc, a.wc) == (b.hc, b.wc) and a.frames_in == b.frames_in, what
    ra, rb = a.overflow_report(), b.overflow_report()
    assert ra == rb, (what, ra, rb)
    return ra


_canvases = {}


def _cropped_canvas(nets, dev, frames, h, w):
    """The canvas a stream fixes for itself after its first window, right edge 8 % of its width in and top 5 % of its height down."""
    if (h, w) not in _canvases:
        from stabstitch2_amd.online import OnlineStitcher
        st = OnlineStitcher(nets, h, w, use_graph=False)
        for t in range(7):
            st.push(*[f[t:t + 1] for f in frames])
        bb = st.bbox.cpu().tolist()
        cw, ch = bb[1] - bb[0], bb[3] - bb[2]
        _canvases[(h, w)] = [bb[0], bb[1] - 0.08 * cw, bb[2] + 0.05 * ch, bb[3]]
    return _canvases[(h, w)]


@pytest.mark.parametrize('canvas', ['own', 'cropped'])
@pytest.mark.parametrize('use_graph', [True, False], ids=['graph', 'eager'])
@pytest.mark.parametrize('warp,fusion', [('NORMAL', 'AVERAGE'), ('FAST', 'LINEAR')])
def test_push_many_equals_single_pushes(dev, hip_nets, warp, fusion, use_graph, canvas):
    """deterministic=True, 360x640, 33 frames through SCHEDULE against a stitcher fed the same frames one push at a time: every
    frame bit for bit, the canvas size, frames_in and overflow_report().  The cropped canvas (grow='never') clips some frames."""
    from stabstitch2_amd.online import OnlineStitcher
    h, w = 360, 640
    n = sum(1 if c == 'p' else c for c in SCHEDULE)
    hr, lr = _clip(n, h, w, 31)
    frames = [t.to(dev) for t in (hr[0], hr[1], lr[0], lr[1])]
    cv = None if canvas == 'own' else _cropped_canvas(hip_nets, dev, frames, h, w)
    mk = lambda: OnlineStitcher(hip_nets, h, w, canvas=cv, warp_mode=warp, fusion_mode=fusion, use_graph=use_graph,
                                deterministic=True)
    ref_st, st = mk(), mk()
    ref = _singles(ref_st, n, frames)
    got = _feed(st, SCHEDULE, frames)
    assert len(got) == n == len(ref)                # (nothing for the first 6 frames, 7 at the 7th, then one per frame)
    _equal(got, ref, 'push_many vs push %s/%s graph=%s %s' % (warp, fusion, use_graph, canvas))
    rep = _same_stream(st, ref_st, canvas)
    assert rep['frames_seen'] == n
    if canvas == 'cropped':
        assert rep['clipped_frames'] > 0, rep
    if use_graph:
        assert sorted(st.graph_nodes_batch) == [1, 3, 6, 8] and st.batch_captures == 4


@pytest.mark.parametrize('fusion', ['AVERAGE', 'LINEAR'])
def test_push_many_u8_equals_push_u8(dev, hip_nets, fusion):
    """push_many_u8 == push_u8 byte for byte at the odd geometry 251x377 (deterministic kernel policy), through SCHEDULE."""
    from stabstitch2_amd.online import OnlineStitcher
    h, w = 251, 377
    n = sum(1 if c == 'p' else c for c in SCHEDULE)
    hr, _ = _clip(n, h, w, 11)
    u8 = [hr[v].permute(0, 2, 3, 1).round().clamp(0, 255).to(torch.uint8).contiguous().to(dev) for v in range(2)]
    mk = lambda: OnlineStitcher(hip_nets, h, w, fusion_mode=fusion, deterministic=True)
    ref_st, st = mk(), mk()
    ref = _singles(ref_st, n, u8, u8=True)
    got = _feed(st, SCHEDULE, u8, u8=True)
    assert all(f.dtype == torch.uint8 and f.shape[-1] == 3 for f in got)
    _equal(got, ref, 'push_many_u8 vs push_u8 %s' % fusion)
    _same_stream(st, ref_st, 'u8 ' + fusion)


# ------------------------------------------------------------------ 4. against the oracle, default kernel policy
@pytest.mark.parametrize('warp,fusion', [('NORMAL', 'AVERAGE'), ('FAST', 'LINEAR')])
def test_push_many_720p_vs_oracle(dev, hip_nets, warp, fusion):
    """720x1280, 16 frames on the oracle's canvas in batches of 4 and of 8: every frame within the oracle gates, nothing clipped,
    and within 1e-3 grey levels (median) of single pushes (the networks' kernels are chosen per launch size)."""
    from stabstitch2_amd.online import OnlineStitcher
    n, h, w = 16, 720, 1280
    seq = ('c720', 0, False, n)
    ref, ohc, owc = _oracle(seq, warp, fusion)
    canvas = _oracle_bbox(seq)
    frames = [t.to(dev) for t in _seq(seq)]
    single = _run(OnlineStitcher(hip_nets, h, w, canvas=canvas, warp_mode=warp, fusion_mode=fusion), n, _pair_args(seq, dev))
    for k in (4, 8):
        st = OnlineStitcher(hip_nets, h, w, canvas=canvas, warp_mode=warp, fusion_mode=fusion)
        got = _feed(st, [k] * (n // k), frames)
        assert (st.hc, st.wc) == (ohc, owc)
        rep = st.overflow_report()
        assert rep['frames_seen'] == n and rep['clipped_frames'] == 0, rep
        _vs_oracle(got, ref, fusion, '720p push_many k=%d %s/%s' % (k, warp, fusion))
        med = max(float((a - b).abs().median()) for a, b in zip(got, single))
        assert med < 1e-3, (k, med)
    _forget('c720')


# ------------------------------------------------------------------ 5. canvas growth
def test_push_many_canvas_growth_vs_oracle(dev, hip_nets):
    """grow='recapture' from the cropped canvas of test_stream_canvas_growth_vs_oracle, batches of 4: the canvas grows, the final
    canvas holds every oracle mesh, and every frame of the calls after the last growth equals the oracle on the final canvas."""
    from stabstitch2_amd.online import OnlineStitcher
    n, h, w, k = 24, 360, 640, 4
    seq = ('c640', 0, False, n)
    bb = _oracle_bbox(seq)
    cw, ch = bb[1] - bb[0], bb[3] - bb[2]
    crop = [bb[0], bb[1] - 0.08 * cw, bb[2] + 0.05 * ch, bb[3]]
    st = OnlineStitcher(hip_nets, h, w, canvas=crop, grow='recapture')
    frames = [t.to(dev) for t in _seq(seq)]
    outs, epochs = [], []
    for c in range(n // k):
        outs.append(st.push_many(*[f[c * k:(c + 1) * k] for f in frames]))
        torch.cuda.synchronize()                 # (the growth check reads the watcher one call later: make it land)
        epochs.append(st.canvas_epoch)
    assert st.canvas_epoch >= 1, epochs
    last = max(c for c in range(len(epochs)) if epochs[c] != (epochs[c - 1] if c else 0))
    assert last >= 2, epochs                     # (the first call that can see the watcher's copy is the third)
    final = st.bbox.cpu().tolist()
    m = torch.cat([x[0].reshape(n, -1, 2) for x in _hr_meshes(seq)], 1)
    tol = 0.05
    assert float(m[..., 0].min()) >= final[0] - tol and float(m[..., 0].max()) <= final[1] + tol, (final, bb)
    assert float(m[..., 1].min()) >= final[2] - tol and float(m[..., 1].max()) <= final[3] + tol, (final, bb)
    ref, ohc, owc = _oracle(seq, 'NORMAL', 'AVERAGE', final)
    assert (st.hc, st.wc) == (ohc, owc)
    assert all(len(outs[c]) == k for c in range(last, len(outs)))
    got = [f for c in range(last, len(outs)) for f in outs[c]]
    _vs_oracle(got, ref[last * k:], 'AVERAGE', 'push_many after its last growth')


# ------------------------------------------------------------------ 6. graphs
def _fresh_nets(dev):
    from stabstitch2_amd.spatial_network import SpatialNet
    from stabstitch2_amd.temporal_network import TemporalNet
    from stabstitch2_amd.smooth_network import SmoothNet
    nets = []
    for cls in (SpatialNet, TemporalNet, SmoothNet):
        m = cls()
        m.load_state_dict(synth.synthetic_state_dict(m), strict=True)
        nets.append(m.to(dev))
    return nets


def test_push_many_graphs_reuse_recapture_evict(dev):
    """A repeated k replays its graph; reloading a net's weights recaptures and the frames follow the new weights (equal to single
    pushes that saw the same reload); a fifth batch size drops the least recently used one."""
    from stabstitch2_amd.online import OnlineStitcher, BATCH_GRAPHS
    nets = _fresh_nets(dev)
    h, w = 360, 480
    n = 7 + 4 + 2 * 4 + 4 + 1 + 2 + 3 + 5 + 2 + 1
    hr, lr = _clip(n, h, w, 5)
    frames = [t.to(dev) for t in (hr[0], hr[1], lr[0], lr[1])]
    st = OnlineStitcher(nets, h, w, deterministic=True)
    ref_st = OnlineStitcher(nets, h, w, deterministic=True)
    t = 0

    def many(k):
        nonlocal t
        a = st.push_many(*[f[t:t + k] for f in frames])
        b = _singles(ref_st, k, [f[t:t + k] for f in frames])
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


# ------------------------------------------------------------------ 7. refusals
def test_push_many_refusals_leave_the_stream_unchanged(dev, hip_nets, monkeypatch):
    """Every invalid push_many / push_many_u8 raises ValueError before any state changes: the calls that follow give the frames of a
    stitcher that never saw the bad input (window fill and steady state)."""
    from stabstitch2_amd import layers as L
    from stabstitch2_amd.online import OnlineStitcher, PipelinedOnlineStitcher
    h, w = 360, 480
    n = 16
    hr, lr = _clip(n, h, w, 7)
    f = [t.to(dev) for t in (hr[0], hr[1], lr[0], lr[1])]
    u8 = [hr[v].permute(0, 2, 3, 1).round().clamp(0, 255).to(torch.uint8).contiguous().to(dev) for v in range(2)]

    def bad_calls(st, t):
        sl = lambda k: [x[t:t + k] for x in f]
        h1, h2, l1, l2 = sl(3)
        cases = [
            lambda: st.push_many(h1, h2[:2], l1, l2),                                  # leading dimensions disagree
            lambda: st.push_many(h1, h2, l1, l2[:2]),
            lambda: st.push_many(h1[:0], h2[:0], l1[:0], l2[:0]),                     # k = 0
            lambda: st.push_many(*[x.repeat(11, 1, 1, 1) for x in (h1, h2, l1, l2)]),    # k = 33
            lambda: st.push_many(h1[:, :, :-1], h2[:, :, :-1], l1, l2),               # wrong frame size
            lambda: st.push_many(h1.transpose(2, 3), h2.transpose(2, 3), l1, l2),     # transposed
            lambda: st.push_many(h1[0], h2[0], l1[0], l2[0]),                         # wrong rank
            lambda: st.push_many(h1.double(), h2.double(), l1, l2),                   # wrong dtype
            lambda: st.push_many(u8[0][t:t + 3], u8[1][t:t + 3], l1, l2),
            lambda: st.push_many_u8(u8[0][t:t + 3], u8[1][t:t + 2]),
            lambda: st.push_many_u8(u8[0][t:t + 3].float(), u8[1][t:t + 3].float()),
            lambda: st.push_many_u8(u8[0][t], u8[1][t]),                              # rank 3: [H,W,3] is one frame
            lambda: st.push_many_u8(u8[0][t:t + 3, :-1], u8[1][t:t + 3, :-1]),
            lambda: st.push_many_u8(u8[0][:0], u8[1][:0]),
        ]
        for i, c in enumerate(cases):
            with pytest.raises(ValueError):
                c()
            assert st.frames_in == t, i
        monkeypatch.setattr(L, 'QUAD', False)
        with pytest.raises(ValueError):
            st.push_many(h1, h2, l1, l2)
        with pytest.raises(ValueError):
            st.push_many_u8(u8[0][t:t + 3], u8[1][t:t + 3])
        monkeypatch.setattr(L, 'QUAD', True)
        assert st.frames_in == t

    a, b = OnlineStitcher(hip_nets, h, w), OnlineStitcher(hip_nets, h, w)
    got, ref = [], []
    for t0, k in ((0, 4), (4, 5), (9, 4), (13, 3)):
        bad_calls(a, t0)
        got += a.push_many(*[x[t0:t0 + k] for x in f])
        ref += b.push_many(*[x[t0:t0 + k] for x in f])
    torch.cuda.synchronize()
    _equal(got, ref, 'after refused calls')
    assert a.overflow_report() == b.overflow_report()
    mo = OnlineStitcher(hip_nets, h, w, meshes_only=True)
    with pytest.raises(ValueError):
        mo.push_many(*[x[:3] for x in f])
    with pytest.raises(ValueError):
        mo.push_many_u8(u8[0][:3], u8[1][:3])
    assert mo.frames_in == 0
    pipe = PipelinedOnlineStitcher(hip_nets, h, w)
    with pytest.raises(ValueError):
        pipe.push_many(*[x[:3] for x in f])
    with pytest.raises(ValueError):
        pipe.push_many_u8(u8[0][:3], u8[1][:3])
    assert pipe.frames_in == 0
