"""Round-6 GPU tests: the streaming push's fused normalisation + watcher, meshes_only streams past their first window, the
three-view stream against the oracle.
    python -m pytest tests -m gpu"""
import os

import numpy as np
import pytest
import torch

from stabstitch2_amd import synth
from test_gpu_parity import dev, hip_nets, close, close_boxes, clip16  # noqa: F401  (fixtures / helpers)

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stream_normalize_watch_equals_the_separate_launches(dev):
    """ss_stream_normalize_watch (one launch per push) == ss_mesh_normalize_views(_boxes) per view + ss_canvas_watch, bit for bit:
    control points and watcher state, one canvas and a canvas per stream, two and three views; a NaN control point counts as
    outside the canvas (fminf / fmaxf dropped it); a guard below the rounding slack makes `near` coincide with `out`."""
    from stabstitch2_amd import ops
    g = torch.Generator(device='cpu').manual_seed(11)
    for S, V, boxes in ((1, 2, False), (1, 3, False), (5, 2, True)):
        rigid = torch.stack(torch.meshgrid(torch.linspace(0, 360, 7), torch.linspace(0, 480, 9), indexing='ij'), -1).flip(-1)
        meshes = [(rigid[None, None] + 9 * torch.randn((S, 7, 7, 9, 2), generator=g)).to(dev).contiguous() for _ in range(V)]
        newest = [m[0, -1] for m in meshes]                       # stream 0's newest mesh; stream s is 7 * 126 floats further
        if boxes:
            bb = torch.tensor([[-20.0 - s, 1300.0 + 3 * s, -15.0, 745.0 + s] for s in range(S)], device=dev)
        else:
            bb = torch.tensor([-20.0, 1300.0, -15.0, 745.0], device=dev)
        for guard in (0.0, 0.02):
            wi0, wf0 = ops.canvas_watch_state(S, dev)
            wi1, wf1 = ops.canvas_watch_state(S, dev)
            for _ in range(3):                                     # the watcher accumulates over pushes
                if boxes:
                    ref = ops.mesh_normalize_views_boxes(newest, 7 * 126, bb, 720, 1280)
                else:
                    ref = ops.mesh_normalize_views([m[0, -1:] for m in meshes], bb, 720, 1280)
                ops.canvas_watch(ref, wi0, wf0, guard)
                got = ops.stream_normalize_watch(newest, 7 * 126, bb, 720, 1280, guard, wi1, wf1)
                assert torch.equal(got, ref)
                assert torch.equal(wi0, wi1) and torch.equal(wf0, wf1)
            assert int(wi1[0, 0]) == 3
    # a NaN control point: outside (both kernels), whatever the other points say
    m = [rigid[None].to(dev).contiguous(), rigid[None].to(dev).clone().contiguous()]
    m[1][0, 3, 4, 1] = float('nan')
    bb = torch.tensor([-10.0, 1290.0, -10.0, 730.0], device=dev)
    wi, wf = ops.canvas_watch_state(1, dev)
    src = ops.stream_normalize_watch(m, 126, bb, 720, 1280, 0.0, wi, wf)
    assert wi[0].tolist() == [1, 1, 0, 1]
    wi2, wf2 = ops.canvas_watch_state(1, dev)
    ops.canvas_watch(src, wi2, wf2, 0.0)
    assert wi2[0].tolist() == [1, 1, 0, 1]
    # a mesh that touches the edge of its own bbox (margin 0): inside, and with guard 0 not `near` either
    m = [rigid[None].to(dev).contiguous(), rigid[None].to(dev).contiguous()]
    bb = torch.tensor([0.0, 1280.0, 0.0, 720.0], device=dev)
    wi, wf = ops.canvas_watch_state(1, dev)
    ops.stream_normalize_watch(m, 126, bb, 720, 1280, 0.0, wi, wf)
    assert wi[0].tolist() == [1, 0, -1, 0]
    wi, wf = ops.canvas_watch_state(1, dev)
    ops.stream_normalize_watch(m, 126, bb, 720, 1280, 0.01, wi, wf)
    assert wi[0].tolist() == [1, 0, -1, 1]


@pytest.mark.parametrize('use_graph', [True, False])
def test_meshes_only_streams_past_the_first_window(dev, hip_nets, clip16, use_graph):
    """`push` of a meshes_only stitcher crashed after the first window (st['out'] / watch_i are None in that
    mode).  12 pairs through OnlineStitcher and MultiOnlineStitcher(streams=2) with meshes_only=True: None for six pushes, 7 meshes
    on the 7th, then one per push -- equal to the offline clip's smoothed meshes (same sliding windows) within the kernel-choice
    tolerance, graph and eager alike."""
    from stabstitch2_amd import pipeline
    from stabstitch2_amd.online import OnlineStitcher, MultiOnlineStitcher
    hr, lr = clip16
    n = 12
    d = lambda frames: torch.cat([f.to(dev) for f in frames[:n]], 0)
    H1, H2, L1, L2 = d(hr[0]), d(hr[1]), d(lr[0]), d(lr[1])
    _, _, _, m1, m2 = pipeline.run_two_view(H1, H2, L1, L2, hip_nets)            # [1,n,7,9,2]
    st = OnlineStitcher(hip_nets, 360, 480, use_graph=use_graph, meshes_only=True)
    got1, got2 = [], []
    for t in range(n):
        r = st.push(H1[t:t + 1], H2[t:t + 1], L1[t:t + 1], L2[t:t + 1])
        if t < 6:
            assert r is None
            continue
        assert r[0].shape[0] == (7 if t == 6 else 1) and tuple(r[0].shape[1:]) == (7, 9, 2)
        got1.append(r[0].clone()); got2.append(r[1].clone())
    g1, g2 = torch.cat(got1, 0), torch.cat(got2, 0)
    assert g1.shape[0] == n
    assert float((g1 - m1[0]).abs().max()) < 2e-3 and float((g2 - m2[0]).abs().max()) < 2e-3
    assert st.overflow_report()['frames_seen'] == 0                # no canvas, nothing watched
    ms = MultiOnlineStitcher(hip_nets, 360, 480, streams=2, use_graph=use_graph, meshes_only=True)
    got = []
    for t in range(n):
        r = ms.push(torch.cat((H1[t:t + 1], H2[t:t + 1])), torch.cat((H2[t:t + 1], H1[t:t + 1])),
                    torch.cat((L1[t:t + 1], L2[t:t + 1])), torch.cat((L2[t:t + 1], L1[t:t + 1])))
        if t < 6:
            assert r is None
            continue
        assert tuple(r[0].shape) == (2, 7 if t == 6 else 1, 7, 9, 2)
        got.append(r[0][0].clone())                                # stream 0 = the pair above, view 1
    assert float((torch.cat(got, 0) - m1[0]).abs().max()) < 2e-3
    assert [rep['frames_seen'] for rep in ms.overflow_report()] == [0, 0]


def test_deterministic_policy_makes_a_frame_independent_of_its_batch(dev, hip_nets, monkeypatch):
    """the kernel-choice pin as an API (`deterministic=True` on pipeline.run_two_view / OnlineStitcher /
    MultiOnlineStitcher, `with ops.deterministic():` below them).  Under it every layer's kernel follows its geometry alone (no
    launch-size thresholds, no split-K, FC on one kernel), so the SAME 32 frames give the SAME bits as one resident clip, as
    passes of 16 pairs through the networks, as a stream of single pairs on the clip's canvas, and as one of two batched streams.
    (Under the default policy these differ by ~1e-5 px / ~1e-3 grey levels: asserted too, so the test cannot pass vacuously.)"""
    from stabstitch2_amd import pipeline, ops
    from stabstitch2_amd.online import OnlineStitcher, MultiOnlineStitcher
    n = 32
    hr, lr = synth.make_clip_device(n, 360, 480, seed=3, device=dev)
    fa, hc, wc, m1a, m2a = pipeline.run_two_view(hr[0], hr[1], lr[0], lr[1], hip_nets, deterministic=True)
    monkeypatch.setattr(pipeline, 'SPATIAL_CHUNK', 16)
    fb, hcb, wcb, m1b, m2b = pipeline.run_two_view(hr[0], hr[1], lr[0], lr[1], hip_nets, deterministic=True)
    monkeypatch.setattr(pipeline, 'SPATIAL_CHUNK', 32)
    assert (hc, wc) == (hcb, wcb) and torch.equal(m1a, m1b) and torch.equal(m2a, m2b) and torch.equal(fa, fb)
    bbox = ops.mesh_bbox([m1a, m2a], 360, 480).cpu().tolist()
    st = OnlineStitcher(hip_nets, 360, 480, canvas=bbox, deterministic=True)
    frames = []
    for t in range(n):
        frames += st.push(hr[0][t:t + 1], hr[1][t:t + 1], lr[0][t:t + 1], lr[1][t:t + 1])
    assert (st.hc, st.wc) == (hc, wc) and len(frames) == n
    fs = torch.stack(frames, 0)
    assert torch.equal(fs, fa), float((fs - fa).abs().max())
    # two batched streams (this pair and its mirror): stream 0 equals the single stream bit for bit
    ms = MultiOnlineStitcher(hip_nets, 360, 480, streams=2, canvases=[bbox, bbox], deterministic=True)
    got = []
    for t in range(12):
        r = ms.push(torch.cat((hr[0][t:t + 1], hr[1][t:t + 1])), torch.cat((hr[1][t:t + 1], hr[0][t:t + 1])),
                    torch.cat((lr[0][t:t + 1], lr[1][t:t + 1])), torch.cat((lr[1][t:t + 1], lr[0][t:t + 1])))
        got += r[0]
    assert torch.equal(torch.stack(got, 0), fa[:12])
    # the default policy: close, not equal
    fd = pipeline.run_two_view(hr[0], hr[1], lr[0], lr[1], hip_nets)[0]
    sd = OnlineStitcher(hip_nets, 360, 480, canvas=bbox)
    fsd = []
    for t in range(n):
        fsd += sd.push(hr[0][t:t + 1], hr[1][t:t + 1], lr[0][t:t + 1], lr[1][t:t + 1])
    fsd = torch.stack(fsd, 0)
    assert not torch.equal(fsd, fd) and float((fsd - fd).abs().median()) < 1e-3
    assert float((fa - fd).abs().median()) < 1e-3                  # and the two policies agree to the usual tolerance


def test_three_view_stream_vs_oracle_720p(dev, hip_nets):
    """`ThreeViewOnlineStitcher` at 720p against the ORACLE's three-view path (oracle/pipeline.py: two full
    2-view passes, composition, three-image render) on the same 10 triples, with the two boxes the oracle's offline run takes over
    all frames (the composition's first canvas, the output canvas) handed to the stream: canvas size equal, frames within the
    gates of test_run_three_view_vs_oracle (AVERAGE: views-1-2 region sharply, whole canvas through the median; LINEAR: whole
    canvas).  The middle view passes the trunks once per push (chain mode): the launches of a push are counted."""
    import cases
    from oracle import pipeline as P
    from test_gpu_parity import _oracle_nets
    from stabstitch2_amd import ops
    from stabstitch2_amd.online import ThreeViewOnlineStitcher
    n, h, w = 10, 720, 1280
    hr, lr = synth.make_clip(n, h, w, seed=7, views=3)
    nets = _oracle_nets()
    a12 = P.estimate_meshes(nets, lr[0], lr[1])
    a23 = P.estimate_meshes(nets, lr[1], lr[2])
    # the oracle's boxes: first canvas = bbox of the aligned HR meshes, output canvas = bbox of the composed ones
    s = lambda m: P._scale_to_hr(m, h, w)
    w12_1, w12_2, w23_1, w23_2 = s(a12['smooth_mesh1']), s(a12['smooth_mesh2']), s(a23['smooth_mesh1']), s(a23['smooth_mesh2'])
    off = (w12_2 - w23_1).reshape(1, n, -1, 2).mean(dim=2).unsqueeze(2).unsqueeze(2)
    first = [float(v) for v in P._bbox([w12_1, w12_2, w23_1 + off, w23_2 + off])]
    om1, omid, om3 = P.three_view_compose(a12['smooth_mesh1'], a12['smooth_mesh2'], a23['smooth_mesh1'], a23['smooth_mesh2'], h, w)
    box = [float(v) for v in P._bbox([om1, omid, om3])]
    hrd = [[f.to(dev) for f in v] for v in hr]
    lrd = [[f.to(dev) for f in v] for v in lr]
    k = 16
    for fusion in ('AVERAGE', 'LINEAR'):
        ofr, owc, ohc = P.three_view_render(hr[0], hr[1], hr[2], om1, omid, om3, 'NORMAL', fusion)
        st = ThreeViewOnlineStitcher(hip_nets, h, w, canvas=box, first_canvas=first, fusion_mode=fusion)
        frames = []
        for t in range(n):
            frames += st.push(hrd[0][t], hrd[1][t], hrd[2][t], lrd[0][t], lrd[1][t], lrd[2][t])
        assert len(frames) == n and (st.hc, st.wc) == (int(ohc), int(owc))
        assert st.overflow_report()['frames_seen'] == n and st.clipped_frames == 0
        got = np.stack([cases.box_down(f.permute(1, 2, 0).cpu().numpy(), k) for f in frames])
        ref = np.stack([cases.box_down(f.numpy().transpose(1, 2, 0), k) for f in ofr])
        rng = np.stack([cases.box_iqr(f.numpy().transpose(1, 2, 0), k) for f in ofr])
        if fusion == 'AVERAGE':
            xlim = int(float(omid[..., 0].max() - box[0]) // k) - 1
            ok = cases.smooth_boxes(rng, k)
            ok[:, :, xlim:] = False
            assert ok.mean() > 0.3, ok.mean()
            dd = np.abs(got - ref)[ok]
            print('\n[3-view stream vs oracle, AVERAGE] p99 %.3e max %.3e' % (np.quantile(dd, 0.99), dd.max()))
            assert np.quantile(dd, 0.99) < 0.05 and dd.max() < 3.0, (float(np.quantile(dd, 0.99)), float(dd.max()))
            clean = cases.smooth_boxes(rng, k)
            assert np.median(np.abs(got - ref)[clean]) < 0.02
        else:
            close_boxes(got, ref, rng, 0.3, 'three-view LINEAR stream vs oracle', k=k, cover=0.5)


def test_three_view_stream_shares_the_middle_view_and_grows_its_canvas(dev, hip_nets):
    """(a) chain mode: a steady-state push sends THREE images through the twin trunks (one stem launch over 3 frames x 2 banks),
    and its meshes equal the unshared batch of two pairs (four image passes) within the kernel-choice tolerance;
    (b) grow='recapture': a triple stream whose outer views drift apart grows its output canvas before anything is cropped, where
    grow='never' counts cropped frames."""
    from stabstitch2_amd import ops
    from stabstitch2_amd.online import ThreeViewOnlineStitcher, MultiOnlineStitcher
    n, h, w = 16, 180, 320
    hr, lr = synth.make_clip(n, h, w, seed=4, views=3)
    hrd = [[f.to(dev) for f in v] for v in hr]
    lrd = [[f.to(dev) for f in v] for v in lr]
    stems = []
    real = ops.H.call

    def spy(name, *a):
        if name == 'ss_stem_pool':
            stems.append(a[4])                   # images of the launch
        return real(name, *a)
    res = {}
    for chain in (True, False):
        ms = MultiOnlineStitcher(hip_nets, h, w, streams=2, use_graph=False, meshes_only=True, chain=chain)
        got = []
        for t in range(n):
            if t == 10:
                ops.H.call = spy
            try:
                r = ms.push(None, None, torch.cat((lrd[0][t], lrd[1][t])), torch.cat((lrd[1][t], lrd[2][t])))
            finally:
                ops.H.call = real
            if r is not None:
                got.append(torch.stack((r[0][:, -1], r[1][:, -1]), 0).clone())
        res[chain] = torch.stack(got, 0)
        assert stems == ([3] if chain else [4]), stems
        del stems[:]
    assert float((res[True] - res[False]).abs().max()) < 1e-3
    # (b) drifting outer views
    def run(grow):
        st = ThreeViewOnlineStitcher(hip_nets, h, w, grow=grow, use_graph=True)
        out = []
        for t in range(40):
            i = t % n
            dx = 0 if t < 14 else int(min(t - 14, 16) * 1.5)          # views 1 and 3 slide outwards by up to 24 px (7.5 % of the width)
            h1 = torch.roll(hrd[0][i], -dx, -1); h3 = torch.roll(hrd[2][i], dx, -1)
            l1 = torch.roll(lrd[0][i], -int(dx * 480 / w), -1); l3 = torch.roll(lrd[2][i], int(dx * 480 / w), -1)
            out += st.push(h1, hrd[1][i], h3, l1, lrd[1][i], l3)
        torch.cuda.synchronize()
        return st, out
    never, _ = run('never')
    rep = never.overflow_report()
    grown, frames = run('recapture')
    repg = grown.overflow_report()
    assert rep['frames_seen'] == repg['frames_seen'] == 40
    if rep['clipped_frames'] > 0:                # (the synthetic regressors follow the drift: when they do, growth must prevent the cropping)
        assert repg['clipped_frames'] < rep['clipped_frames'] and grown.canvas_epoch >= 1 and grown.wc > never.wc
    assert all(bool(torch.isfinite(f).all()) for f in frames)


def test_render_eps_fold_is_opt_in_and_within_the_gates(dev, golden, hip_nets, clip16, monkeypatch):
    """VERDICT r5 item 7, measured instead of declined: SS_RENDER_EPS_FOLD=1 (SS_WARP_EPS_FOLD on the fused AVERAGE renders: the
    reference's + 1e-6 folded into the row table, a log(a) instead of d2 log(d2 + 1e-6)) is OFF by default; switched on, the fused
    render still passes the reference's gates -- G7 (fused AVERAGE frame), G9 (16-frame pipeline: canvas, box medians, PSNR / SSIM)
    and G13 (uint8 bytes vs the reference's writer) -- and its deviation from the default render is reported."""
    import test_gpu_parity as TP
    import test_gpu_round3 as T3
    from stabstitch2_amd import ops, pipeline
    assert ops.RENDER_EPS_FOLD is False and ops._avg_mode('NORMAL') == 0
    hr, lr = synth.make_clip_device(8, 720, 1280, seed=0, device=dev)
    f0, hc, wc, m1, m2 = pipeline.run_two_view(hr[0], hr[1], lr[0], lr[1], hip_nets)
    monkeypatch.setattr(ops, 'RENDER_EPS_FOLD', True)
    assert ops._avg_mode('NORMAL') == 16 and ops._avg_mode('FAST') == 17
    f1 = pipeline.run_two_view(hr[0], hr[1], lr[0], lr[1], hip_nets)[0]
    d = (f1 - f0).abs()
    print('\n[eps fold vs default, 720p AVERAGE] median %.2e  p99.9 %.2e  max %.2e grey levels'
          % (float(d.median()), float(torch.quantile(d.flatten()[::97], 0.999)), float(d.max())))
    assert float(d.median()) < 2e-3 and float(torch.quantile(d.flatten()[::97], 0.999)) < 0.2
    TP.test_tps_dense_warp_and_fusion(dev, golden)                  # G6 / G7: the fused AVERAGE frame under the switch
    TP.test_pipeline_vs_reference(dev, golden, hip_nets, clip16)    # G9
    T3.test_u8_pipeline_bytes_vs_reference(dev, golden, hip_nets)   # G13: the reference writer's bytes


def test_pipelined_stream_equals_the_plain_stream(dev, hip_nets, clip16):
    """PipelinedOnlineStitcher (two pushes in flight: push t + 1's trunks / stage-1 heads on a second HIP stream beside push t's
    regressor heads, smoothing and render; one HIP graph per half and buffer parity) delivers, one push late and after `flush()`,
    exactly OnlineStitcher's frames -- bit for bit, with the same overflow bookkeeping."""
    from stabstitch2_amd.online import OnlineStitcher, PipelinedOnlineStitcher
    hr, lr = clip16
    hrd = [[f.to(dev) for f in v] for v in hr]
    lrd = [[f.to(dev) for f in v] for v in lr]
    n = 40
    plain = OnlineStitcher(hip_nets, 360, 480)
    ref = []
    for t in range(n):
        i = t % 16
        ref += plain.push(hrd[0][i], hrd[1][i], lrd[0][i], lrd[1][i])
    pipe = PipelinedOnlineStitcher(hip_nets, 360, 480)
    got, counts = [], []
    for t in range(n):
        i = t % 16
        r = pipe.push(hrd[0][i], hrd[1][i], lrd[0][i], lrd[1][i])
        counts.append(len(r))
        got += r
    got += pipe.flush()
    assert counts == [0] * 6 + [7, 0] + [1] * (n - 8) and pipe.flush() == []
    assert len(got) == len(ref) == n and (pipe.hc, pipe.wc) == (plain.hc, plain.wc)
    torch.cuda.synchronize()
    for a, b in zip(got, ref):
        assert torch.equal(a, b)
    assert pipe.overflow_report() == plain.overflow_report()
    assert pipe.graph_nodes is None or pipe.graph_nodes >= 60


def test_pipelined_multi_stream_equals_the_plain_batch(dev, hip_nets, clip16):
    """PipelinedMultiOnlineStitcher (S live pairs per push, two pushes in flight) against MultiOnlineStitcher: every stream's
    frames bit for bit, one push late; per-stream canvases of different sizes and the one-size clip-style render."""
    from stabstitch2_amd.online import MultiOnlineStitcher, PipelinedMultiOnlineStitcher
    hr, lr = clip16
    H1 = torch.cat([f.to(dev) for f in hr[0]], 0); H2 = torch.cat([f.to(dev) for f in hr[1]], 0)
    L1 = torch.cat([f.to(dev) for f in lr[0]], 0); L2 = torch.cat([f.to(dev) for f in lr[1]], 0)
    S, n = 3, 20

    def batch(t):      # stream s shows the clip s frames ahead (stream 2 with the views swapped: another canvas size)
        idx = [(t + s) % 16 for s in range(S)]
        a, b, c, d = H1[idx].clone(), H2[idx].clone(), L1[idx].clone(), L2[idx].clone()
        a[2], b[2] = H2[idx[2]], H1[idx[2]]
        c[2], d[2] = L2[idx[2]], L1[idx[2]]
        return a, b, c, d
    for canvases in (None, [(-20.0, 700.0, -15.0, 375.0)] * S):
        plain = MultiOnlineStitcher(hip_nets, 360, 480, streams=S, canvases=canvases)
        pipe = PipelinedMultiOnlineStitcher(hip_nets, 360, 480, streams=S, canvases=canvases)
        ref = [[] for _ in range(S)]
        got = [[] for _ in range(S)]
        for t in range(n):
            for s, fr in enumerate(plain.push(*batch(t))):
                ref[s] += fr
            for s, fr in enumerate(pipe.push(*batch(t))):
                got[s] += fr
        for s, fr in enumerate(pipe.flush()):
            got[s] += fr
        torch.cuda.synchronize()
        assert pipe.canvas_sizes == plain.canvas_sizes
        for s in range(S):
            assert len(got[s]) == len(ref[s]) == n
            for a, b in zip(got[s], ref[s]):
                assert torch.equal(a, b)
        assert pipe.overflow_report() == plain.overflow_report()


def test_pipelined_three_view_stream_equals_the_plain_one(dev, hip_nets):
    """PipelinedThreeViewOnlineStitcher against ThreeViewOnlineStitcher: the same frames bit for bit, one push late."""
    from stabstitch2_amd.online import ThreeViewOnlineStitcher, PipelinedThreeViewOnlineStitcher
    n, h, w = 16, 180, 320
    hr, lr = synth.make_clip(n, h, w, seed=4, views=3)
    hrd = [[f.to(dev) for f in v] for v in hr]
    lrd = [[f.to(dev) for f in v] for v in lr]
    for fusion in ('AVERAGE', 'LINEAR'):
        plain = ThreeViewOnlineStitcher(hip_nets, h, w, fusion_mode=fusion)
        pipe = PipelinedThreeViewOnlineStitcher(hip_nets, h, w, fusion_mode=fusion)
        ref, got = [], []
        for t in range(24):
            i = t % n
            ref += plain.push(hrd[0][i], hrd[1][i], hrd[2][i], lrd[0][i], lrd[1][i], lrd[2][i])
            got += pipe.push(hrd[0][i], hrd[1][i], hrd[2][i], lrd[0][i], lrd[1][i], lrd[2][i])
        got += pipe.flush()
        torch.cuda.synchronize()
        assert len(got) == len(ref) == 24 and (pipe.hc, pipe.wc) == (plain.hc, plain.wc)
        for a, b in zip(got, ref):
            assert torch.equal(a, b)
        assert pipe.overflow_report() == plain.overflow_report()


def test_pipelined_stitcher_measures_its_stream_pair(dev, hip_nets):
    """Which hardware queue a HIP stream lands on depends on every stream the process made before, and an unlucky pair turns the
    pipelined push 1.5 - 4x slower (LAB_NOTES R6.5).  _TwoInFlight._pick_streams tries PIPE_STREAM_CANDIDATES streams pairwise on
    the captured halves and keeps the fastest pair: stitchers built after 0 .. 5 further streams exist all run at the same rate, and
    the probe leaves the stream state untouched (frames equal to the plain stitcher's are checked by the tests above)."""
    import time
    from stabstitch2_amd import online
    from stabstitch2_amd.online import PipelinedThreeViewOnlineStitcher
    n, h, w = 16, 360, 640
    hr, lr = synth.make_clip_device(n, h, w, seed=2, views=3, device=dev)
    rates, dummies = [], []
    for k in range(6):
        st = PipelinedThreeViewOnlineStitcher(hip_nets, h, w)
        push = lambda i: st.push(hr[0][i:i + 1], hr[1][i:i + 1], hr[2][i:i + 1], lr[0][i:i + 1], lr[1][i:i + 1], lr[2][i:i + 1])
        for t in range(12):
            push(t % n)
        torch.cuda.synchronize()
        c = online.PIPE_STREAM_CANDIDATES
        assert len(st.stream_probe_ms) == c * (c - 1) // 2
        t0 = time.perf_counter()
        for t in range(60):
            push(t % n)
        torch.cuda.synchronize()
        rates.append((time.perf_counter() - t0) / 60 * 1e3)
        s = torch.cuda.Stream(dev)
        with torch.cuda.stream(s):
            torch.zeros(1, device=dev)
        dummies.append(s)
    assert max(rates) < 1.25 * min(rates), rates


def test_three_view_splines_equal_the_seven_launches(dev):
    """ss_three_view_splines (align -> normalise -> solve -> points -> finish on the first canvas, then normalise on the output
    canvas + solve onto the rigid mesh, 3 workgroups per frame) against the seven launches it replaces: meshes, control points
    and coefficients bit for bit; the watcher inside ss_render_footprints_watch against stream_normalize_watch's."""
    from stabstitch2_amd import ops, pipeline
    from stabstitch2_amd.spatial_network import get_rigid_mesh, get_norm_mesh
    h, w = 720, 1280
    g = torch.Generator().manual_seed(5)
    rigid_lr = get_rigid_mesh(1, 360, 480, device='cpu').reshape(1, 7, 9, 2)
    nrigid = get_norm_mesh(get_rigid_mesh(1, h, w, device=dev), h, w).contiguous()
    for k, amp in ((1, 6.0), (3, 25.0)):
        ms = [(rigid_lr + amp * torch.randn((k, 7, 9, 2), generator=g) + off).to(dev).contiguous()
              for off in (torch.tensor([0.0, 0.0]), torch.tensor([300.0, 4.0]), torch.tensor([-8.0, 3.0]), torch.tensor([290.0, -5.0]))]
        first = torch.tensor([-40.0, 2900.0, -60.0, 800.0], device=dev)
        outb = torch.tensor([-90.0, 3000.0, -100.0, 850.0], device=dev) if amp < 10 else torch.tensor([0.0, 2400.0, 0.0, 700.0], device=dev)
        sh = lambda m: m.reshape(1, k, 7, 9, 2)
        ref = pipeline.three_view_compose(sh(ms[0]), sh(ms[1]), sh(ms[2]), sh(ms[3]), h, w, first_canvas=first)
        wi0, wf0 = ops.canvas_watch_state(k, dev)
        src_ref = ops.stream_normalize_watch([m.contiguous() for m in ref], 126, outb.expand(k, 4).contiguous(), 0.0, 0.0, 0.01, wi0, wf0)
        T_ref = ops.tps_solve_shared(src_ref.reshape(k * 3, 63, 2), nrigid).reshape(k, 3, 2, 66)
        meshes, src, T = ops.three_view_splines(ms[0], ms[1], ms[2], ms[3], first, outb, nrigid, h, w)
        torch.cuda.synchronize()
        for a, b in zip(meshes, ref):
            assert torch.equal(a, b)
        assert torch.equal(src, src_ref) and torch.equal(T, T_ref)
        wi1, wf1 = ops.canvas_watch_state(k, dev)
        ops.render_footprints(src, T, h, w, 760, 2900, watch=(0.01, wi1, wf1))
        torch.cuda.synchronize()
        assert torch.equal(wi1, wi0) and torch.equal(wf1, wf0)
        if amp > 10:
            assert int(wi0[:, 1].sum()) > 0            # the second box is too small on purpose: the watcher has something to say


def test_stream_splines_equal_normalise_plus_solve(dev):
    """ss_stream_splines (control points + splines of every view and stream in one launch) == stream_normalize_watch +
    tps_solve_shared bit for bit, one canvas for all streams and a canvas per stream, LR-scale and canvas-pixel meshes; the watcher
    through render_footprints(watch=...) per stream slice equals stream_normalize_watch's."""
    from stabstitch2_amd import ops
    from stabstitch2_amd.spatial_network import get_rigid_mesh, get_norm_mesh
    h, w = 720, 1280
    g = torch.Generator().manual_seed(12)
    nrigid = get_norm_mesh(get_rigid_mesh(1, h, w, device=dev), h, w).contiguous()
    rigid_lr = get_rigid_mesh(1, 360, 480, device='cpu').reshape(1, 7, 9, 2)
    S = 3
    for views in (2, 3):
        meshes = [(rigid_lr + 8.0 * torch.randn((S, 7, 9, 2), generator=g) + torch.tensor([150.0 * v, 2.0 * v])).to(dev).contiguous()
                  for v in range(views)]
        for boxes in (torch.tensor([-30.0, 2700.0, -40.0, 780.0], device=dev),
                      torch.tensor([[-30.0, 2700.0, -40.0, 780.0], [0.0, 2000.0, 0.0, 700.0], [-100.0, 3000.0, -90.0, 900.0]], device=dev)):
            wi0, wf0 = ops.canvas_watch_state(S if boxes.dim() == 2 else 1, dev)
            if boxes.dim() == 1:
                continue_streams = 1
                ms = [m[:1].contiguous() for m in meshes]
            else:
                ms = meshes
            ref = ops.stream_normalize_watch(ms, 126, boxes, h, w, 0.02, wi0, wf0)
            T_ref = ops.tps_solve_shared(ref.reshape(-1, 63, 2), nrigid).reshape(ref.shape[0], views, 2, 66)
            src, T = ops.stream_splines(ms, 126, boxes, nrigid, h, w)
            torch.cuda.synchronize()
            assert torch.equal(src, ref) and torch.equal(T, T_ref)
            wi1, wf1 = ops.canvas_watch_state(src.shape[0], dev)
            for s_ in range(src.shape[0]):
                ops.render_footprints(src[s_:s_ + 1], T[s_:s_ + 1], h, w, 800, 2800, watch=(0.02, wi1[s_:s_ + 1], wf1[s_:s_ + 1]))
            torch.cuda.synchronize()
            assert torch.equal(wi1, wi0) and torch.equal(wf1, wf0)


def test_chain_pairs_share_their_launches(dev):
    """A chain of pairs (view 1, view 2), (view 2, view 3) reads views [0:2] and [1:3] of one trunk output: the feature normalisation
    of ss_ccl and the homography warp take them as ONE launch (overlapping inputs) -- results equal to separate tensors."""
    from stabstitch2_amd import ops
    g = torch.Generator().manual_seed(9)
    f = torch.randn((3, 23, 30, 256), generator=g).to(dev)
    a, b = f[0:2], f[1:3]
    flow_o, _ = ops.ccl(a, b, 10.0, True, False)
    flow_s, _ = ops.ccl(a.clone(), b.clone(), 10.0, True, False)
    assert torch.equal(flow_o, flow_s)
    x = torch.randn((3, 45, 60, 128), generator=g).to(dev)
    th = (torch.eye(3).reshape(1, 9).repeat(4, 1) + 0.05 * torch.randn((4, 9), generator=g)).to(dev).contiguous()
    w1, w2 = ops.homo_warp_pair(x[0:2], x[1:3], th[0:2], th[2:4], 45, 60)
    r1, r2 = ops.homo_warp_nhwc(x[0:2].clone(), th[0:2].clone(), 45, 60), ops.homo_warp_nhwc(x[1:3].clone(), th[2:4].clone(), 45, 60)
    torch.cuda.synchronize()
    assert torch.equal(w1, r1) and torch.equal(w2, r2)
    assert w2.data_ptr() == w1.data_ptr() + w1.numel() * 4          # one launch: one output tensor
    # temporal cost volumes of a chain of S pairs from the S + 1 views stored once == the volumes of the concatenated layout
    for S in (1, 2, 4):
        prev = torch.randn((S + 1, 45, 60, 128), generator=g).to(dev)
        cur = torch.randn((S + 1, 45, 60, 128), generator=g).to(dev)
        got = ops.cost_volume(prev, cur, 3, chain=S)
        ref = ops.cost_volume(torch.cat((prev[:S], prev[1:]), 0), torch.cat((cur[:S], cur[1:]), 0), 3)
        torch.cuda.synchronize()
        assert got.shape == ref.shape and torch.equal(got, ref)


def test_three_view_stream_fused_splines_are_frame_neutral(dev, hip_nets, monkeypatch):
    """ThreeViewOnlineStitcher with the fused composition launch (default) against the seven separate launches: frames, overflow
    report and canvases identical, graph nodes fewer."""
    from stabstitch2_amd import online
    from stabstitch2_amd.online import ThreeViewOnlineStitcher
    n, h, w = 16, 180, 320
    hr, lr = synth.make_clip(n, h, w, seed=6, views=3)
    hrd = [[f.to(dev) for f in v] for v in hr]
    lrd = [[f.to(dev) for f in v] for v in lr]
    res = {}
    for fused in (True, False):
        monkeypatch.setattr(online, 'FUSED_SPLINES', fused)
        for fusion in ('AVERAGE', 'LINEAR'):
            st = ThreeViewOnlineStitcher(hip_nets, h, w, fusion_mode=fusion, margin=0.0)      # margin 0: the watcher has work
            frames = []
            for t in range(22):
                i = t % n
                frames += st.push(hrd[0][i], hrd[1][i], hrd[2][i], lrd[0][i], lrd[1][i], lrd[2][i])
            torch.cuda.synchronize()
            res[(fused, fusion)] = (frames, st.overflow_report(), (st.hc, st.wc), st.graph_nodes)
    for fusion in ('AVERAGE', 'LINEAR'):
        a, b = res[(True, fusion)], res[(False, fusion)]
        assert len(a[0]) == len(b[0]) and a[2] == b[2] and a[1] == b[1]
        for x, y in zip(a[0], b[0]):
            assert torch.equal(x, y)
        if a[3] is not None and b[3] is not None:
            assert a[3] <= b[3] - 5


def test_direct_render_is_frame_neutral(dev, hip_nets, clip16, monkeypatch):
    """DIRECT_RENDER (default): the steady-state graph ends with splines and footprints, the AVERAGE render is launched by the push on
    the caller's own HR frames into a fresh tensor (no copies of the frames into static buffers, no clone of a static canvas).  Frames
    equal those of the render-inside-the-graph form bit for bit -- plain and pipelined, two and three views; a returned frame is
    not overwritten by later pushes."""
    from stabstitch2_amd import online
    from stabstitch2_amd.online import OnlineStitcher, PipelinedOnlineStitcher, ThreeViewOnlineStitcher, PipelinedThreeViewOnlineStitcher
    hr, lr = clip16
    hr = [[f.to(dev) for f in v] for v in hr]
    lr = [[f.to(dev) for f in v] for v in lr]
    n = len(hr[0])
    out = {}
    for direct in (True, False):
        monkeypatch.setattr(online, 'DIRECT_RENDER', direct)
        for cls in (OnlineStitcher, PipelinedOnlineStitcher):
            st = cls(hip_nets, hr[0][0].shape[-2], hr[0][0].shape[-1])
            frames = []
            for t in range(20):
                i = t % n
                frames += st.push(hr[0][i], hr[1][i], lr[0][i], lr[1][i])
            if hasattr(st, 'flush'):
                frames += st.flush()
            torch.cuda.synchronize()
            out[(direct, cls.__name__)] = [f.clone() for f in frames]
            if direct and cls is OnlineStitcher:
                assert st._direct() and frames[-1].data_ptr() != frames[-2].data_ptr()
                assert st.static['hr1'] is None and st.static['hr2'] is None          # no static HR buffers for a render outside the graph
    for name in ('OnlineStitcher', 'PipelinedOnlineStitcher'):
        a, b = out[(True, name)], out[(False, name)]
        assert len(a) == len(b) == 20
        for x, y in zip(a, b):
            assert torch.equal(x, y)
    h, w = 180, 320
    hr3, lr3 = synth.make_clip(12, h, w, seed=8, views=3)
    hr3 = [[f.to(dev) for f in v] for v in hr3]
    lr3 = [[f.to(dev) for f in v] for v in lr3]
    out3 = {}
    for direct in (True, False):
        monkeypatch.setattr(online, 'DIRECT_RENDER', direct)
        for cls in (ThreeViewOnlineStitcher, PipelinedThreeViewOnlineStitcher):
            st = cls(hip_nets, h, w)
            frames = []
            for t in range(16):
                i = t % 12
                frames += st.push(hr3[0][i], hr3[1][i], hr3[2][i], lr3[0][i], lr3[1][i], lr3[2][i])
            if hasattr(st, 'flush'):
                frames += st.flush()
            torch.cuda.synchronize()
            out3[(direct, cls.__name__)] = frames
    for name in ('ThreeViewOnlineStitcher', 'PipelinedThreeViewOnlineStitcher'):
        a, b = out3[(True, name)], out3[(False, name)]
        assert len(a) == len(b) == 16
        for x, y in zip(a, b):
            assert torch.equal(x, y)


def test_push_u8_streams_decoded_frames_byte_for_byte(dev, hip_nets):
    """push_u8: decoded uint8 frames in, uint8 video frames out.  Steady state: the cv2-exact resize writes the graph's LR inputs, the
    render samples the uint8 frames and writes the uint8 frame (no fp32 planes, no fp32 canvas).  Equal, byte for byte, to
    ingest_u8 -> push -> canvas_to_u8 on a second stitcher -- two views, three views, and a pipelined stitcher (fallback route)."""
    from stabstitch2_amd import ops
    from stabstitch2_amd.online import OnlineStitcher, ThreeViewOnlineStitcher, PipelinedOnlineStitcher
    n, h, w = 12, 360, 640
    hr, _ = synth.make_clip(n, h, w, seed=13, views=3)
    u8 = [[f.reshape(3, h, w).clamp(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous().to(dev) for f in v] for v in hr]     # [H,W,3]
    def reference(cls, views):
        st = cls(hip_nets, h, w)
        out = []
        for t in range(18):
            i = t % n
            hrf, lrf = ops.ingest_u8(torch.stack([u8[v][i] for v in range(views)], 0), 360, 480)
            args = [hrf[v:v + 1] for v in range(views)] + [lrf[v:v + 1] for v in range(views)]
            out += [ops.canvas_to_u8(f.reshape((1,) + tuple(f.shape[-3:])))[0] for f in st.push(*args)]
        if hasattr(st, 'flush'):
            out += [ops.canvas_to_u8(f.reshape((1,) + tuple(f.shape[-3:])))[0] for f in st.flush()]
        return out
    for cls, views in ((OnlineStitcher, 2), (ThreeViewOnlineStitcher, 3), (PipelinedOnlineStitcher, 2)):
        st = cls(hip_nets, h, w)
        got = []
        for t in range(18):
            i = t % n
            got += st.push_u8(*[u8[v][i] for v in range(views)])
        if hasattr(st, 'flush_u8'):
            got += st.flush_u8()
        ref = reference(cls, views)
        torch.cuda.synchronize()
        assert len(got) == len(ref) == 18
        for a, b in zip(got, ref):
            assert a.dtype == torch.uint8 and tuple(a.shape) == (st.hc, st.wc, 3) and torch.equal(a, b)


def test_multi_stream_push_u8(dev, hip_nets):
    """MultiOnlineStitcher.push_u8 (S streams of decoded uint8 frames per push): byte for byte ingest_u8 -> push -> canvas_to_u8 of a
    second MultiOnlineStitcher, window fill and steady state; canvases per stream (one uint8 render per stream) and canvases of one size
    (one clip-style uint8 render launch)."""
    from stabstitch2_amd import ops
    from stabstitch2_amd.online import MultiOnlineStitcher
    n, h, w, S = 10, 360, 640, 3
    hr, _ = synth.make_clip(n + S, h, w, seed=15, views=2)
    u8 = [torch.stack([f.reshape(3, h, w).clamp(0, 255).to(torch.uint8).permute(1, 2, 0) for f in v], 0).contiguous().to(dev) for v in hr]   # [n+S,H,W,3]
    for canvases in (None, [(-30.0, 1000.0, -20.0, 400.0)] * S):
        a = MultiOnlineStitcher(hip_nets, h, w, streams=S, canvases=canvases)
        b = MultiOnlineStitcher(hip_nets, h, w, streams=S, canvases=canvases)
        for t in range(16):
            i = t % n
            f1, f2 = u8[0][i:i + S].contiguous(), u8[1][i:i + S].contiguous()          # stream s sees frame i + s
            got = a.push_u8(f1, f2)
            hr1, lr1 = ops.ingest_u8(f1, 360, 480)
            hr2, lr2 = ops.ingest_u8(f2, 360, 480)
            ref = [[ops.canvas_to_u8(x.reshape((1,) + tuple(x.shape[-3:])))[0] for x in per] for per in b.push(hr1, hr2, lr1, lr2)]
            torch.cuda.synchronize()
            assert [len(p_) for p_ in got] == [len(p_) for p_ in ref]
            for ga, rb in zip(got, ref):
                for x, y in zip(ga, rb):
                    assert x.dtype == torch.uint8 and torch.equal(x, y)


def test_host_frame_stream_equals_push_u8(dev, hip_nets):
    """HostFrameStream: uint8 frames in host memory (pinned tensors and plain numpy arrays) -> uint8 frames in pinned host memory,
    uploads / downloads of neighbouring pushes on their own streams: every frame, in order, byte for byte what push_u8 returns on the
    device; yielded tensors stay valid for `depth` further frames."""
    from stabstitch2_amd.online import OnlineStitcher, ThreeViewOnlineStitcher, HostFrameStream
    n, h, w = 10, 360, 640
    hr, _ = synth.make_clip(n, h, w, seed=14, views=3)
    host = [[f.reshape(3, h, w).clamp(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous() for f in v] for v in hr]
    from stabstitch2_amd.online import PipelinedOnlineStitcher
    for cls, views, pinned in ((OnlineStitcher, 2, True), (ThreeViewOnlineStitcher, 3, False), (PipelinedOnlineStitcher, 2, True)):
        seq = [tuple((host[v][t % n].pin_memory() if pinned else host[v][t % n].numpy()) for v in range(views)) for t in range(25)]
        ref_st = (OnlineStitcher if views == 2 else ThreeViewOnlineStitcher)(hip_nets, h, w)       # (the plain stitcher is the reference)
        ref = []
        for fr in seq:
            ref += [f.cpu() for f in ref_st.push_u8(*[(x if torch.is_tensor(x) else torch.from_numpy(x)).to(dev) for x in fr])]
        runner = HostFrameStream(cls(hip_nets, h, w), depth=3)
        got, held = [], []
        for f in runner.run(iter(seq)):
            assert f.is_pinned() and f.dtype == torch.uint8
            held.append(f)
            got.append(f.clone())
            if len(held) > 3:                      # a frame yielded `depth` frames ago is still intact
                assert torch.equal(held[-4], got[-4])
        assert len(got) == len(ref) == 25
        for a, b in zip(got, ref):
            assert torch.equal(a, b)


def test_tps_solve_round6_kernel_against_round4(dev, request):
    """tps_solve_kernel of round 6 (four waves, lane = row, one barrier per column, pivot search under the previous update) against
    the round-4 kernel kept in the tuning build (`ss_tps_solve_r4`): same pivot rule and factors, the update an fma instead of
    mul + sub -- T agrees to 1e-6 of max |T| (bit for bit on ordinary meshes), on clip-like, strongly deformed and near-degenerate
    control points (two pairs of points 1e-4 / 1e-5 apart: |T| ~ 1e7), with per-system and shared targets; residual of the fp64
    system on the deformed set."""
    import ctypes
    import importlib.util
    from stabstitch2_amd import _hip, ops
    spec = importlib.util.spec_from_file_location('_tuning', os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), 'tools', '_tuning.py'))
    tuning = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tuning)
    product = _hip.lib()
    request.addfinalizer(lambda: setattr(_hip, '_lib', product))
    lib = tuning.lib()
    _hip._lib = product
    lib.ss_tps_solve_r4.restype = ctypes.c_int
    lib.ss_tps_solve_r4.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int, ctypes.c_void_p]
    g = torch.Generator().manual_seed(11)
    ys, xs = torch.meshgrid(torch.linspace(-1, 1, 7), torch.linspace(-1, 1, 9), indexing='ij')
    rigid = torch.stack([xs, ys], -1).reshape(1, 63, 2)
    n = 48
    sets = {'clip': rigid + 0.05 * torch.randn((n, 63, 2), generator=g), 'deformed': rigid + 0.4 * torch.randn((n, 63, 2), generator=g)}
    deg = rigid.repeat(n, 1, 1).clone()
    deg[:, 1] = deg[:, 0] + 1e-4 * torch.randn((n, 2), generator=g)
    deg[:, 40] = deg[:, 41] + 1e-5
    sets['degenerate'] = deg
    for name, src in sets.items():
        src = src.to(dev).contiguous()
        tgt = (rigid.repeat(n, 1, 1) + 0.02 * torch.randn((n, 63, 2), generator=g)).to(dev).contiguous()
        new = ops.tps_solve(src, tgt)
        old = torch.empty_like(new)
        rc = lib.ss_tps_solve_r4(src.data_ptr(), tgt.data_ptr(), old.data_ptr(), n, torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        torch.cuda.synchronize()
        assert torch.isfinite(new).all(), name
        assert float((new - old).abs().max()) <= 1e-6 * float(old.abs().max()), name
        if name != 'degenerate':
            assert torch.equal(new, old), name
    # residual: A [a; w] = [Y; 0] in fp64 with the kernel's own fp32 entries
    src = sets['deformed'][:4].double()
    tgt = rigid.repeat(4, 1, 1).double()
    T = ops.tps_solve(src.float().to(dev).contiguous(), tgt.float().to(dev).contiguous()).double().cpu()     # [4,2,66]
    for i in range(4):
        s32 = src[i].float()
        d2 = ((s32[:, None, :] - s32[None, :, :]) ** 2).sum(-1)
        K = (d2 * torch.log((d2 + torch.tensor(1e-6, dtype=torch.float32)).double()).float()).double()
        P = torch.cat([torch.ones(63, 1, dtype=torch.float64), s32.double()], 1)
        A = torch.zeros((66, 66), dtype=torch.float64)
        A[:63, :3] = P
        A[:63, 3:] = K
        A[63:, 3:] = P.t()
        Y = torch.zeros((66, 2), dtype=torch.float64)
        Y[:63] = tgt[i]
        ref = torch.linalg.solve(A, Y)
        assert float((T[i].t() - ref).abs().max()) <= 2e-5 * max(1.0, float(ref.abs().max()))


@pytest.mark.parametrize('shape', [(64, 64, 90, 120, 24), (128, 128, 45, 60, 40), (256, 256, 23, 30, 48), (16, 64, 45, 60, 40),
                                   (64, 64, 37, 61, 33)])
def test_wino43_persistent_workgroups_are_output_neutral(dev, shape):
    """conv_wino43p_kernel walking SEVERAL tile blocks per workgroup (one workgroup per CU, the next block's rows requested in front
    of the epilogue) against the same kernel launched with one workgroup per block (`ss_wino43_set_persistent(0)`): bit-identical,
    both block geometries (8 x 60, 16 x 32), with / without residual, the single-chunk (cin = 16) instantiation, a ragged map; and
    within the engine's usual gate of fp64 direct convolution."""
    from stabstitch2_amd import ops, _hip as H
    cin, cout, h, w, n = shape
    g = torch.Generator(device='cpu').manual_seed(cin + 7 * h)
    x = torch.randn((n, h, w, cin), generator=g).to(dev)
    wgt = (torch.randn((cout, 1, 3, 3, cin), generator=g) / np.sqrt(9 * cin)).to(dev)
    bias = torch.randn((cout,), generator=g).to(dev)
    res = torch.randn((n, h, w, cout), generator=g).to(dev)
    try:
        for r in (None, res):
            H.lib().ss_wino43_set_persistent(0)
            a = ops.conv_winograd43(x, wgt, bias, r, True)
            H.lib().ss_wino43_set_persistent(1)
            b = ops.conv_winograd43(x, wgt, bias, r, True)
            c = ops.conv_winograd43(x, wgt, bias, r, True)
            torch.cuda.synchronize()
            assert torch.equal(a, b) and torch.equal(b, c)
            want = torch.nn.functional.conv2d(x[:4].double().permute(0, 3, 1, 2), wgt[:, 0].double().permute(0, 3, 1, 2), bias.double(), padding=1)
            if r is not None:
                want = want + r[:4].double().permute(0, 3, 1, 2)
            want = want.clamp_min(0).permute(0, 2, 3, 1)
            assert float((b[:4].double() - want).abs().max()) < 3e-4
    finally:
        H.lib().ss_wino43_set_persistent(1)
        ops._w43_persist_set[0] = None
