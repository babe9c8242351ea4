"""The two-view streaming stitchers against the CPU ORACLE directly (not only against another part of this repository): smoothed
meshes over a long stream, every frame at 720p in all four warp / fusion modes, the stream's own canvas, a cropped canvas and its
growth, batched streams, decoded uint8 in and out at an odd geometry; and the frame-size check every push makes.
Oracle results are computed once per (clip, mode, canvas) and every stitcher class is compared with that one result.
    python -m pytest tests -m gpu"""
import numpy as np
import pytest
import torch

from oracle import pipeline as P, frame_io as FIO
from stabstitch2_amd import synth
from test_gpu_parity import dev, hip_nets, close, close_boxes, _oracle_nets  # noqa: F401  (fixtures / helpers)

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

# per-frame gates of test_two_view_720p_default_kernel_mix_vs_oracle: (median, p99.9) of |frame - oracle| in grey levels
GATES = {'AVERAGE': (5e-3, 0.1), 'LINEAR': (2e-2, 0.5)}
MESH_TOL = 5e-3                        # LR px: the offline oracle tests' mesh tolerance
# clip name -> (frames, H, W, seed)
CLIPS = {'c480': (42, 360, 480, 21), 'c720': (16, 720, 1280, 8), 'c640': (26, 360, 640, 9), 'u8': (11, 251, 377, 11)}

_cache = {'nets': None, 'clips': {}, 'meshes': {}, 'frames': {}}


def _onets():
    if _cache['nets'] is None:
        _cache['nets'] = _oracle_nets()
    return _cache['nets']


def _clip(name):
    """-> (hr [2,N,3,H,W], lr [2,N,3,360,480], u8 [2,N,H,W,3] | None) CPU tensors.  'u8': decoded uint8 frames (as _u8_clip in
    test_gpu_round3.py), HR / LR through the oracle's frame loader (oracle.frame_io.load_frame)."""
    c = _cache['clips']
    if name not in c:
        n, h, w, seed = CLIPS[name]
        hr, lr = synth.make_clip_device(n, h, w, seed=seed, device='cpu')
        u8 = None
        if name == 'u8':
            u8 = hr.permute(0, 1, 3, 4, 2).round().clamp(0, 255).to(torch.uint8).contiguous()
            loaded = [[FIO.load_frame(u8[v, t].numpy()) for t in range(n)] for v in range(2)]
            hr = torch.stack([torch.stack([torch.from_numpy(a) for a, _ in lv]) for lv in loaded])
            lr = torch.stack([torch.stack([torch.from_numpy(b) for _, b in lv]) for lv in loaded])
        c[name] = (hr, lr, u8)
    return c[name]


def _seq(seq):
    """seq = (clip, start, swap, n): the clip from frame `start`, n frames, views swapped or not -> (hr1, hr2, lr1, lr2) [n,...]."""
    name, start, swap, n = seq
    hr, lr, _ = _clip(name)
    a, b = (1, 0) if swap else (0, 1)
    assert start + n <= hr.shape[1]
    s = slice(start, start + n)
    return hr[a, s], hr[b, s], lr[a, s], lr[b, s]


def _u8_seq(seq):
    name, start, swap, n = seq
    u8 = _clip(name)[2]
    a, b = (1, 0) if swap else (0, 1)
    return u8[a, start:start + n], u8[b, start:start + n]


def _lists(t):
    return [t[i:i + 1] for i in range(t.shape[0])]


def _meshes(seq):
    """Oracle smoothed meshes (m1, m2) [1,n,7,9,2] (LR px) of a sequence.  Mesh i depends on frames 0 .. max(i, 6) only, so a
    longer run of the same clip / start / swap serves a shorter one."""
    name, start, swap, n = seq
    for (k, m) in _cache['meshes'].items():
        if k[:3] == seq[:3] and k[3] >= n:
            return m[0][:, :n], m[1][:, :n]
    _, _, l1, l2 = _seq(seq)
    acc = P.estimate_meshes(_onets(), _lists(l1), _lists(l2))
    _cache['meshes'][seq] = (acc['smooth_mesh1'], acc['smooth_mesh2'])
    return _cache['meshes'][seq]


def _hr_meshes(seq):
    h, w = CLIPS[seq[0]][1:3]
    return [P._scale_to_hr(m, h, w) for m in _meshes(seq)]


def _oracle_bbox(seq):
    """The oracle's canvas (bbox over all frames, HR px) as (wmin, wmax, hmin, hmax) floats."""
    return [float(v) for v in P._bbox(_hr_meshes(seq))]


def _oracle(seq, warp, fusion, canvas=None):
    """-> (frames [n] HWC fp32 ndarrays, Hc, Wc) of P.get_stable_sqe on `canvas` (None: the oracle's own bbox); once per key."""
    key = (seq, warp, fusion, None if canvas is None else tuple(float(v) for v in canvas))
    if key not in _cache['frames']:
        h1, h2, _, _ = _seq(seq)
        m1, m2 = _meshes(seq)
        fr, wc, hc = P.get_stable_sqe(_lists(h1), _lists(h2), m1, m2, warp, fusion, canvas=canvas)
        _cache['frames'][key] = (fr, int(hc), int(wc))
    return _cache['frames'][key]


def _forget(name):
    for k in [k for k in _cache['frames'] if k[0][0] == name]:
        del _cache['frames'][k]


def _vs_oracle(got, ref, fusion, what):
    """Every frame [3,Hc,Wc] (device) against the oracle's HWC frame at the gates of `fusion`; prints the worst values."""
    med_tol, tail_tol = GATES[fusion]
    assert len(got) == len(ref), (what, len(got), len(ref))
    worst = [0.0, 0.0]
    for i, (g, r) in enumerate(zip(got, ref)):
        g = g.permute(1, 2, 0).cpu().numpy()
        assert g.shape == r.shape, (what, i, g.shape, r.shape)
        assert np.isfinite(g).all(), (what, i)
        d = np.abs(g - r)
        med, tail = float(np.median(d)), float(np.quantile(d, 0.999))
        assert med < med_tol and tail < tail_tol, (what, i, med, tail)
        worst = [max(worst[0], med), max(worst[1], tail)]
    print('\n[%s vs oracle] %d frames, worst median %.2e, worst p99.9 %.2e' % (what, len(got), worst[0], worst[1]))


def _equal(a, b, what):
    """Nested lists of device tensors, bit for bit."""
    if torch.is_tensor(a):
        assert torch.is_tensor(b) and a.shape == b.shape and torch.equal(a, b), what
        return
    assert len(a) == len(b), (what, len(a), len(b))
    for x, y in zip(a, b):
        _equal(x, y, what)


def _run(st, n, args, flush=False):
    """n pushes of args(t) -> the frames in order (a pipelined stitcher: the frames handed out late and by flush())."""
    out = []
    for t in range(n):
        out += st.push(*args(t))
    if flush:
        out += st.flush()
    torch.cuda.synchronize()
    return out


def _run_multi(st, n, args, flush=False):
    S = st.S
    out = [[] for _ in range(S)]
    for t in range(n):
        for s, fr in enumerate(st.push(*args(t))):
            out[s] += fr
    if flush:
        for s, fr in enumerate(st.flush()):
            out[s] += fr
    torch.cuda.synchronize()
    return out


def _pair_args(seq, dev):
    h1, h2, l1, l2 = [t.to(dev) for t in _seq(seq)]
    return lambda t: (h1[t:t + 1], h2[t:t + 1], l1[t:t + 1], l2[t:t + 1])


def _batch_args(seqs, dev):
    """Pushes of S streams, stream s = seqs[s] -> args(t) = (hr1, hr2, lr1, lr2) [S,...]."""
    parts = [[t.to(dev) for t in _seq(q)] for q in seqs]
    return lambda t: tuple(torch.stack([p[k][t] for p in parts], 0) for k in range(4))


# ------------------------------------------------------------------ 1. smoothed meshes over a long stream
def test_stream_meshes_vs_oracle_over_40_frames(dev, hip_nets):
    """meshes_only streams fed 40 pairs of a clip that does not repeat: past the first window the 7-frame ring shifts 33 times
    (first-tsmotion zeroing, cached TemporalNet features, the previous spatial motions move with it).  Every smoothed mesh the
    stream returns against P.estimate_meshes on the same sequence: OnlineStitcher eager and graph-captured, and a batch of three
    streams (stream s starts s frames into the clip, stream 2 with its views swapped)."""
    from stabstitch2_amd.online import OnlineStitcher, MultiOnlineStitcher
    n, S = 40, 3
    seqs = [('c480', s, s == 2, n) for s in range(S)]
    ref = [_meshes(q) for q in seqs]
    for use_graph in (True, False):
        st = OnlineStitcher(hip_nets, 360, 480, use_graph=use_graph, meshes_only=True)
        args = _pair_args(seqs[0], dev)
        got = [st.push(None, None, *args(t)[2:]) for t in range(n)]
        assert [g is None for g in got] == [True] * 6 + [False] * (n - 6)
        for v in range(2):
            m = torch.cat([g[v] for g in got[6:]], 0)[None]                       # [1,n,7,9,2]
            close(m, ref[0][v], MESH_TOL, 'stream smooth_mesh%d (use_graph=%s) vs oracle' % (v + 1, use_graph))
    ms = MultiOnlineStitcher(hip_nets, 360, 480, streams=S, meshes_only=True)
    args = _batch_args(seqs, dev)
    got = [ms.push(None, None, *args(t)[2:]) for t in range(n)]
    assert [g is None for g in got] == [True] * 6 + [False] * (n - 6)
    for v in range(2):
        m = torch.cat([g[v] for g in got[6:]], 1)                                 # [S,n,7,9,2]
        for s in range(S):
            close(m[s:s + 1], ref[s][v], MESH_TOL, 'batched stream %d smooth_mesh%d vs oracle' % (s, v + 1))


# ------------------------------------------------------------------ 2. 720p, all four modes, on the oracle's canvas
@pytest.mark.parametrize('warp,fusion', [('NORMAL', 'AVERAGE'), ('NORMAL', 'LINEAR'), ('FAST', 'AVERAGE'), ('FAST', 'LINEAR')])
def test_two_view_stream_720p_vs_oracle(dev, hip_nets, warp, fusion):
    """OnlineStitcher and PipelinedOnlineStitcher (+ flush) at 720x1280, 16 pushes (window fill, graph capture, 8 replays and
    more), given the oracle's canvas: canvas size equal, nothing clipped, EVERY frame against P.get_stable_sqe at the gates of the
    offline 720p test; the pipelined frames equal the plain ones bit for bit in every mode."""
    from stabstitch2_amd.online import OnlineStitcher, PipelinedOnlineStitcher
    n, h, w = 16, 720, 1280
    seq = ('c720', 0, False, n)
    ref, ohc, owc = _oracle(seq, warp, fusion)
    canvas = _oracle_bbox(seq)
    args = _pair_args(seq, dev)
    plain = OnlineStitcher(hip_nets, h, w, canvas=canvas, warp_mode=warp, fusion_mode=fusion)
    got = _run(plain, n, args)
    pipe = PipelinedOnlineStitcher(hip_nets, h, w, canvas=canvas, warp_mode=warp, fusion_mode=fusion)
    gotp = _run(pipe, n, args, flush=True)
    for st in (plain, pipe):
        assert (st.hc, st.wc) == (ohc, owc), ((st.hc, st.wc), (ohc, owc))
        rep = st.overflow_report()
        assert rep['frames_seen'] == n and rep['clipped_frames'] == 0, rep
    _vs_oracle(got, ref, fusion, '720p stream %s/%s' % (warp, fusion))
    _equal(gotp, got, 'pipelined vs plain stream %s/%s' % (warp, fusion))
    _forget('c720')


# ------------------------------------------------------------------ 3. own canvas, cropping, growth
def _crop_expectation(seq, canvas, band=0.05):
    """Frames whose ORACLE mesh leaves `canvas` -> (clearly out, ambiguous) frame indices.  The watcher (canvas_watch_update in
    csrc/common.h) calls a frame clipped when a control point of either view lies beyond the canvas by more than its slack of
    2.5e-4 canvas half-widths; a point within `band` HR px of that line is ambiguous (HIP and oracle meshes differ by < 1e-2 px)."""
    m = torch.cat([x[0].reshape(x.shape[1], -1, 2) for x in _hr_meshes(seq)], 1).double()    # [n, 126, 2] both views
    wmin, wmax, hmin, hmax = canvas
    sw, sh = 2.5e-4 * (wmax - wmin) / 2.0, 2.5e-4 * (hmax - hmin) / 2.0
    x, y = m[..., 0], m[..., 1]
    e = torch.stack((wmin - x.min(1).values - sw, x.max(1).values - wmax - sw,
                     hmin - y.min(1).values - sh, y.max(1).values - hmax - sh), 1).max(1).values
    clear = [i for i in range(len(e)) if float(e[i]) > band]
    amb = [i for i in range(len(e)) if abs(float(e[i])) <= band]
    return clear, amb


def _check_clipping(rep, n, clear, amb, what):
    assert rep['frames_seen'] == n, (what, rep)
    assert len(clear) <= rep['clipped_frames'] <= len(clear) + len(amb), (what, rep, clear, amb)
    first = rep['first_clipped_frame']
    if rep['clipped_frames'] == 0:
        assert first == -1, (what, rep)
    else:
        assert first in clear + amb and (not clear or first <= min(clear)), (what, rep, clear, amb)


def test_stream_own_canvas_vs_oracle(dev, hip_nets):
    """A stream that fixes its own canvas (the first window's bbox plus the margin): every frame against the oracle rendered on
    `st.bbox`, canvas size equal."""
    from stabstitch2_amd.online import OnlineStitcher
    n, h, w = 24, 360, 640
    seq = ('c640', 0, False, n)
    st = OnlineStitcher(hip_nets, h, w)
    got = _run(st, n, _pair_args(seq, dev))
    canvas = st.bbox.cpu().tolist()
    ref, ohc, owc = _oracle(seq, 'NORMAL', 'AVERAGE', canvas)
    assert (st.hc, st.wc) == (ohc, owc)
    _vs_oracle(got, ref, 'AVERAGE', 'stream on its own canvas')


def test_stream_cropped_canvas_vs_oracle(dev, hip_nets):
    """A canvas smaller than the oracle's (right edge 8 % of the width in, top 5 % of the height down): every frame against the
    oracle rendered on the same cropped canvas, and the watcher's count / first clipped frame against the frames whose oracle mesh
    leaves it -- for OnlineStitcher and PipelinedOnlineStitcher.  A second crop through the median of the frames' right extents
    clips some frames and not others."""
    from stabstitch2_amd.online import OnlineStitcher, PipelinedOnlineStitcher
    n, h, w = 24, 360, 640
    seq = ('c640', 0, False, n)
    bb = _oracle_bbox(seq)
    cw, ch = bb[1] - bb[0], bb[3] - bb[2]
    crop = [bb[0], bb[1] - 0.08 * cw, bb[2] + 0.05 * ch, bb[3]]
    xmax = torch.stack([m[0, :, :, :, 0].reshape(n, -1).max(1).values for m in _hr_meshes(seq)], 0).max(0).values
    half = [bb[0], float(xmax.median()), bb[2], bb[3]]
    ref, ohc, owc = _oracle(seq, 'NORMAL', 'AVERAGE', crop)
    args = _pair_args(seq, dev)
    clear, amb = _crop_expectation(seq, crop)
    hclear, hamb = _crop_expectation(seq, half)
    assert clear and 0 < len(hclear) and len(hclear) + len(hamb) < n, (clear, hclear, hamb)
    base = None
    for cls in (OnlineStitcher, PipelinedOnlineStitcher):
        pipelined = cls is PipelinedOnlineStitcher
        st = cls(hip_nets, h, w, canvas=crop)
        got = _run(st, n, args, flush=pipelined)
        assert (st.hc, st.wc) == (ohc, owc)
        _check_clipping(st.overflow_report(), n, clear, amb, cls.__name__ + ' crop')
        if base is None:
            _vs_oracle(got, ref, 'AVERAGE', 'stream on a cropped canvas')
            base = got
        else:
            _equal(got, base, 'pipelined vs plain on a cropped canvas')
        sh = cls(hip_nets, h, w, canvas=half)
        _run(sh, n, args, flush=pipelined)
        _check_clipping(sh.overflow_report(), n, hclear, hamb, cls.__name__ + ' median crop')


def test_stream_canvas_growth_vs_oracle(dev, hip_nets):
    """grow='recapture' from the cropped canvas: the final canvas holds every oracle mesh, and every frame from the last growth on
    (the growth re-fixes the canvas at the start of a push, before its render) equals the oracle rendered on the final canvas."""
    from stabstitch2_amd.online import OnlineStitcher
    n, h, w = 24, 360, 640
    seq = ('c640', 0, False, n)
    bb = _oracle_bbox(seq)
    cw, ch = bb[1] - bb[0], bb[3] - bb[2]
    crop = [bb[0], bb[1] - 0.08 * cw, bb[2] + 0.05 * ch, bb[3]]
    st = OnlineStitcher(hip_nets, h, w, canvas=crop, grow='recapture')
    args = _pair_args(seq, dev)
    outs, epochs = [], []
    for t in range(n):
        outs.append(st.push(*args(t)))
        torch.cuda.synchronize()                  # (the growth check reads the watcher one push later: make it land)
        epochs.append(st.canvas_epoch)
    assert st.canvas_epoch >= 1, epochs
    last = max(t for t in range(n) if epochs[t] != (epochs[t - 1] if t else 0))
    assert last < n - 4, epochs
    final = st.bbox.cpu().tolist()
    m = torch.cat([x[0].reshape(n, -1, 2) for x in _hr_meshes(seq)], 1)
    tol = 0.05
    assert float(m[..., 0].min()) >= final[0] - tol and float(m[..., 0].max()) <= final[1] + tol, (final, bb)
    assert float(m[..., 1].min()) >= final[2] - tol and float(m[..., 1].max()) <= final[3] + tol, (final, bb)
    ref, ohc, owc = _oracle(seq, 'NORMAL', 'AVERAGE', final)
    assert (st.hc, st.wc) == (ohc, owc)
    assert all(len(outs[t]) == 1 for t in range(last, n))
    _vs_oracle([outs[t][0] for t in range(last, n)], ref[last:], 'AVERAGE', 'stream after its last growth')


# ------------------------------------------------------------------ 4. batched streams
@pytest.mark.parametrize('warp,fusion', [('NORMAL', 'AVERAGE'), ('FAST', 'LINEAR')])
def test_multi_stream_vs_oracle(dev, hip_nets, warp, fusion):
    """MultiOnlineStitcher and PipelinedMultiOnlineStitcher, S = 3 streams at 360x640 (stream s starts s frames into the clip,
    stream 2 with its views swapped), 12 pushes, three canvas setups: the streams' own canvases, the oracle's per-stream boxes (of
    different sizes: a render per stream), and boxes of ONE size (the clip-style render).  Every stream's frames against the
    oracle's run of its own sequence on the same canvas; the pipelined frames equal the plain ones bit for bit."""
    from stabstitch2_amd.online import MultiOnlineStitcher, PipelinedMultiOnlineStitcher
    S, n, h, w = 3, 12, 360, 640
    seqs = [('c640', s, s == 2, n) for s in range(S)]
    boxes = [_oracle_bbox(q) for q in seqs]
    sw = int(np.ceil(max(b[1] - b[0] for b in boxes))) + 1
    sh = int(np.ceil(max(b[3] - b[2] for b in boxes))) + 1
    shared = [[float(np.floor(b[0])), float(np.floor(b[0]) + sw), float(np.floor(b[2])), float(np.floor(b[2]) + sh)] for b in boxes]
    args = _batch_args(seqs, dev)
    for name, canvases in (('own', None), ('oracle boxes', boxes), ('one size', shared)):
        plain = MultiOnlineStitcher(hip_nets, h, w, streams=S, canvases=canvases, warp_mode=warp, fusion_mode=fusion)
        got = _run_multi(plain, n, args)
        pipe = PipelinedMultiOnlineStitcher(hip_nets, h, w, streams=S, canvases=canvases, warp_mode=warp, fusion_mode=fusion)
        gotp = _run_multi(pipe, n, args, flush=True)
        if name == 'oracle boxes':
            assert len(set(plain.canvas_sizes)) > 1 and not plain.static['one_size'], plain.canvas_sizes
        if name == 'one size':
            assert set(plain.canvas_sizes) == {(sh, sw)} and plain.static['one_size'], plain.canvas_sizes
        assert pipe.canvas_sizes == plain.canvas_sizes
        for s in range(S):
            canvas = plain.single[s].bbox.cpu().tolist()
            ref, ohc, owc = _oracle(seqs[s], warp, fusion, canvas)
            assert plain.canvas_sizes[s] == (ohc, owc), (name, s, plain.canvas_sizes, (ohc, owc))
            _vs_oracle(got[s], ref, fusion, 'batched stream %d (%s, %s/%s)' % (s, name, warp, fusion))
        _equal(gotp, got, 'pipelined vs plain batch (%s, %s/%s)' % (name, warp, fusion))


# ------------------------------------------------------------------ 5. decoded uint8 in, uint8 video out, odd geometry
def _oracle_video(seq, warp, canvas):
    """The reference's loop on the oracle: load_frame per frame (done in _clip), meshes, get_stable_sqe on `canvas`,
    `.astype(np.uint8)` per frame (to_video_frame)."""
    fr, hc, wc = _oracle(seq, warp, 'AVERAGE', canvas)
    return [FIO.to_video_frame(np.transpose(f, (2, 0, 1))) for f in fr], hc, wc


def _vs_oracle_u8(got, ref, what):
    """uint8 [Hc,Wc,3] video frames against the oracle's.  The fp32 gate of test_two_view_odd_geometry_vs_oracle (p99.9 < 0.25
    grey levels) bounds the bytes: truncation turns a float difference d into a one-byte flip with probability ~d, so a small
    share of bytes differ by one; a difference of 2 or more needs |d| > 1, beyond the fp32 p99.9 -- under 0.1 % of the bytes."""
    assert len(got) == len(ref), (what, len(got), len(ref))
    worst = [0.0, 0.0]
    for i, (g, r) in enumerate(zip(got, ref)):
        g = g.cpu().numpy() if torch.is_tensor(g) else np.asarray(g)
        assert g.dtype == np.uint8 and g.shape == r.shape, (what, i, g.dtype, g.shape, r.shape)
        d = np.abs(g.astype(np.int16) - r.astype(np.int16))
        f1, f2 = float((d > 0).mean()), float((d >= 2).mean())
        assert f1 < 0.03 and f2 < 1e-3, (what, i, f1, f2)
        worst = [max(worst[0], f1), max(worst[1], f2)]
    print('\n[%s vs oracle] %d frames, worst share of bytes differing %.2e, by 2 or more %.2e' % (what, len(got), worst[0], worst[1]))


@pytest.mark.parametrize('warp', ['NORMAL', 'FAST'])
def test_u8_streams_odd_geometry_vs_oracle(dev, hip_nets, warp):
    """Decoded uint8 [251,377,3] frames (non-integer resize ratios in both axes, partial render tiles) through HostFrameStream over
    OnlineStitcher and over PipelinedOnlineStitcher, and through MultiOnlineStitcher.push_u8 with S = 2 (stream 1 a frame later,
    views swapped): every uint8 video frame against the oracle's loop on the stitcher's own canvas."""
    from stabstitch2_amd.online import OnlineStitcher, PipelinedOnlineStitcher, MultiOnlineStitcher, HostFrameStream
    n, h, w = 10, 251, 377
    seqs = [('u8', 0, False, n), ('u8', 1, True, n)]
    a1, a2 = _u8_seq(seqs[0])
    source = [(a1[t].pin_memory(), a2[t].pin_memory()) for t in range(n)]
    base = None
    for cls in (OnlineStitcher, PipelinedOnlineStitcher):
        st = cls(hip_nets, h, w, warp_mode=warp)
        got = [f.clone() for f in HostFrameStream(st).run(source)]
        torch.cuda.synchronize()
        ref, hc, wc = _oracle_video(seqs[0], warp, st.bbox.cpu().tolist())
        assert (st.hc, st.wc) == (hc, wc)
        if base is None:
            _vs_oracle_u8(got, ref, 'HostFrameStream %s' % warp)
            base = got
        else:
            _equal(got, base, 'pipelined vs plain HostFrameStream')
    u = [[x.to(dev) for x in _u8_seq(q)] for q in seqs]
    ms = MultiOnlineStitcher(hip_nets, h, w, streams=2, warp_mode=warp)
    got = [[] for _ in range(2)]
    for t in range(n):
        for s, fr in enumerate(ms.push_u8(torch.stack([u[0][0][t], u[1][0][t]]), torch.stack([u[0][1][t], u[1][1][t]]))):
            got[s] += fr
    torch.cuda.synchronize()
    for s in range(2):
        ref, hc, wc = _oracle_video(seqs[s], warp, ms.single[s].bbox.cpu().tolist())
        assert ms.canvas_sizes[s] == (hc, wc)
        _vs_oracle_u8(got[s], ref, 'MultiOnlineStitcher.push_u8 stream %d %s' % (s, warp))


# ------------------------------------------------------------------ 6. frame-size check on every push
def _stitchers(nets, h, w):
    """(name, make, views per push, streams per push (0: an unbatched stitcher)) for the six stream classes."""
    from stabstitch2_amd import online as O
    return [('OnlineStitcher', lambda: O.OnlineStitcher(nets, h, w), 2, 0),
            ('PipelinedOnlineStitcher', lambda: O.PipelinedOnlineStitcher(nets, h, w), 2, 0),
            ('MultiOnlineStitcher', lambda: O.MultiOnlineStitcher(nets, h, w, streams=2), 2, 2),
            ('PipelinedMultiOnlineStitcher', lambda: O.PipelinedMultiOnlineStitcher(nets, h, w, streams=2), 2, 2),
            ('ThreeViewOnlineStitcher', lambda: O.ThreeViewOnlineStitcher(nets, h, w), 3, 0),
            ('PipelinedThreeViewOnlineStitcher', lambda: O.PipelinedThreeViewOnlineStitcher(nets, h, w), 3, 0)]


def _wrong(t, shape):
    return torch.zeros(shape, dtype=t.dtype, device=t.device)


@pytest.mark.parametrize('u8', [False, True], ids=['push', 'push_u8'])
def test_push_rejects_frames_of_the_wrong_size(dev, hip_nets, u8):
    """Every push (push, push_u8) of all six stream classes refuses, with ValueError and before any state changes, a frame of
    another size, a transposed one of the same element count and a bad LR shape -- during the window fill (push 3) and in the
    steady state (push 10).  The pushes that follow give frames equal bit for bit to a stitcher that never saw the bad ones, with
    the same overflow report."""
    n, h, w = 12, 180, 320
    hr, lr = synth.make_clip_device(n + 1, h, w, seed=6, views=3, device=dev)
    frames = hr.permute(0, 1, 3, 4, 2).round().clamp(0, 255).to(torch.uint8).contiguous()
    for name, make, views, S in _stitchers(hip_nets, h, w):
        def good(t):
            if u8:
                if S:
                    return tuple(frames[v, t:t + S] for v in range(views))
                return tuple(frames[v, t] for v in range(views))
            k = S or 1
            return tuple(hr[v, t:t + k] for v in range(views)) + tuple(lr[v, t:t + k] for v in range(views))

        def bad(t):
            g = list(good(t))
            lead = (S,) if S else ((1,) if not u8 else ())
            out = []
            # another size, a transposed frame of the same element count: in every view (the views agree with each other), and in
            # the last view only
            for shp in (((h + 4, w, 3), (w, h, 3)) if u8 else ((3, h + 4, w), (3, w, h))):
                out.append([_wrong(x, lead + shp) for x in g[:views]] + g[views:])
                out.append(g[:views - 1] + [_wrong(g[views - 1], lead + shp)] + g[views:])
            if not u8:
                out.append(g[:views] + [_wrong(g[views], lead + (3, 480, 360))] + g[views + 1:])    # LR transposed
                out.append(g[:views] + [_wrong(g[views], lead + (3, 360, 481))] + g[views + 1:])
            return out
        a, b = make(), make()
        pa = a.push_u8 if u8 else a.push
        pb = b.push_u8 if u8 else b.push
        for t in range(n):
            if t in (2, 9):
                for x in bad(t):
                    with pytest.raises(ValueError):
                        pa(*x)
            _equal(pa(*good(t)), pb(*good(t)), '%s push %d after a refused push' % (name, t))
        if hasattr(a, 'flush'):
            fl = (lambda s: s.flush_u8()) if u8 else (lambda s: s.flush())
            _equal(fl(a), fl(b), name + ' flush')
        torch.cuda.synchronize()
        assert a.overflow_report() == b.overflow_report(), name
        assert a.frames_in == b.frames_in == n, name


def test_host_frame_stream_rejects_frames_of_the_wrong_size(dev, hip_nets):
    """HostFrameStream.run raises ValueError when its source yields a pair of the wrong size (checked before the upload), first
    pair or later."""
    from stabstitch2_amd.online import OnlineStitcher, HostFrameStream
    h, w = 180, 320
    hr, _ = synth.make_clip_device(6, h, w, seed=6, device='cpu')
    u8 = hr.permute(0, 1, 3, 4, 2).round().clamp(0, 255).to(torch.uint8).contiguous()
    good = [(u8[0, t], u8[1, t]) for t in range(6)]
    wrong = (torch.zeros((w, h, 3), dtype=torch.uint8), torch.zeros((w, h, 3), dtype=torch.uint8))
    for src in (good[:3] + [wrong] + good[3:], [wrong] + good):
        with pytest.raises(ValueError):
            list(HostFrameStream(OnlineStitcher(hip_nets, h, w)).run(src))
    torch.cuda.synchronize()
