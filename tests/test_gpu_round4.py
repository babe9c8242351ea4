"""Round-4 GPU tests: LINEAR fusion as a clip-level path, batch-of-streams streaming, fused regressor tail, host placement.
    python -m pytest tests -m gpu"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cases
from stabstitch2_amd import synth
from test_gpu_parity import dev, hip_nets, close, clip16  # noqa: F401  (fixtures / helpers)

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _meshes(hip_nets, lr, views, h, w):
    from stabstitch2_amd import pipeline
    if views == 2:
        acc = pipeline.estimate_meshes(hip_nets, lr[0], lr[1])
        return [acc['smooth_mesh1'], acc['smooth_mesh2']], False
    a12 = pipeline.estimate_meshes(hip_nets, lr[0], lr[1])
    a23 = pipeline.estimate_meshes(hip_nets, lr[1], lr[2])
    return list(pipeline.three_view_compose(a12['smooth_mesh1'], a12['smooth_mesh2'], a23['smooth_mesh1'],
                                            a23['smooth_mesh2'], h, w)), True


# ------------------------------------------------------------------ LINEAR fusion, whole clip
@pytest.mark.parametrize('views', [2, 3])
@pytest.mark.parametrize('size', [(360, 480), (251, 377)])
def test_linear_clip_equals_per_frame_chain(dev, hip_nets, views, size):
    """ops.render_linear_clip (3 launches per clip, 4 with three views) is bit-identical to the per-frame chain
    tps_warp_views + linear_blend (+ mask_union + linear_blend): frames, mask1 of every pass, both warp modes, fp32 planes
    and uint8 frames in / video frames out.  The odd size has partial tiles in both blend-kernel directions."""
    from stabstitch2_amd import ops, pipeline
    h, w = size
    n = 7
    hr, lr = synth.make_clip_device(n, h, w, seed=3, views=views, device=dev)
    meshes, pres = _meshes(hip_nets, lr, views, h, w)
    hc, wc, src, T = pipeline.render_plan(meshes, h, w, pres)
    clips = [hr[v].contiguous() for v in range(views)]
    u8 = [c.permute(0, 2, 3, 1).round().clamp(0, 255).to(torch.uint8).contiguous() for c in clips]
    for mode in ('NORMAL', 'FAST'):
        got, mk = ops.render_linear_clip(clips, src, T, hc, wc, mode, want_masks=True)
        got8 = ops.render_linear_clip(u8, src, T, hc, wc, mode)
        for i in range(n):
            wv = ops.tps_warp_views([c[i] for c in clips], src[i], T[i], hc, wc, mode)
            f = ops.linear_blend(wv[0, 0:3], wv[1, 0:3], wv[0, 3], wv[1, 3])
            m = ops.linear_blend(None, None, wv[0, 3], wv[1, 3], True)
            assert torch.equal(mk[i, 0], m), (mode, i, float((mk[i, 0] - m).abs().max()))
            if views == 3:
                un = ops.mask_union(wv[0, 3], wv[1, 3])
                m2 = ops.linear_blend(None, None, un, wv[2, 3], True)
                assert torch.equal(mk[i, 1], m2), (mode, i, float((mk[i, 1] - m2).abs().max()))
                f = ops.linear_blend(f, wv[2, 0:3], un, wv[2, 3])
            assert torch.equal(got[i], f), (mode, i, float((got[i] - f).abs().max()))
            # uint8 frames are exact in fp32 -> the uint8 route equals the quantised fp32 route's `.astype(uint8)`
            wq = ops.tps_warp_views([c[i].permute(2, 0, 1).float().contiguous() for c in u8], src[i], T[i], hc, wc, mode)
            fq = ops.linear_blend(wq[0, 0:3], wq[1, 0:3], wq[0, 3], wq[1, 3])
            if views == 3:
                fq = ops.linear_blend(fq, wq[2, 0:3], ops.mask_union(wq[0, 3], wq[1, 3]), wq[2, 3])
            assert torch.equal(got8[i], ops.canvas_to_u8(fq[None])[0]), (mode, i)
    # the blend kernel's other forms (64 x 64 tiles; rolling strips of another height): same bits
    from stabstitch2_amd import _hip
    base, bmk = ops.render_linear_clip(clips, src, T, hc, wc, 'NORMAL', want_masks=True)
    try:
        for rows in (-1, 17):
            _hip.lib().ss_linear_clip_set_rows(rows)
            alt, amk = ops.render_linear_clip(clips, src, T, hc, wc, 'NORMAL', want_masks=True)
            assert torch.equal(alt, base) and torch.equal(amk, bmk), rows
    finally:
        _hip.lib().ss_linear_clip_set_rows(0)
    # pipeline level: tensors take the clip launches, lists of frames the per-frame chain
    a, _, _ = pipeline.render_frames(clips, meshes, 'NORMAL', 'LINEAR', prescaled=pres)
    b, _, _ = pipeline.render_frames([[c[i:i + 1] for i in range(n)] for c in clips], meshes, 'NORMAL', 'LINEAR', prescaled=pres)
    assert torch.equal(a, b)


def test_linear_clip_launch_count(dev, hip_nets):
    """A 2-view LINEAR clip is rendered by THREE kernel launches (<= 5 per clip instead of 8 per frame)."""
    from stabstitch2_amd import _hip, pipeline
    n, h, w = 8, 360, 480
    hr, lr = synth.make_clip_device(n, h, w, seed=1, device=dev)
    acc = pipeline.estimate_meshes(hip_nets, lr[0], lr[1])
    ms = [acc['smooth_mesh1'], acc['smooth_mesh2']]
    pipeline.render_frames([hr[0], hr[1]], ms, 'NORMAL', 'LINEAR')
    torch.cuda.synchronize()
    from torch.profiler import profile, ProfilerActivity
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        pipeline.render_frames([hr[0], hr[1]], ms, 'NORMAL', 'LINEAR')
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type.name == 'CUDA' and 'Memcpy' not in e.name and 'Memset' not in e.name]
    lb = [k for k in names if 'lb_clip' in k]
    assert len(lb) == 3, names
    assert not [k for k in names if 'lb_blur' in k or 'tps_warp_views' in k], names


def test_linear_u8_pipeline_matches_float_pipeline(dev, hip_nets):
    """run_two_view_u8(..., 'LINEAR'): the uint8 clip route (warp from the decoded frames, blend writes the video frame) gives
    the bytes of the fp32 route ingest -> render_frames -> to_video_frames."""
    from stabstitch2_amd import pipeline
    n, h, w = 9, 360, 480
    hr, _ = synth.make_clip_device(n, h, w, seed=5, device=dev)
    u8 = [hr[v].permute(0, 2, 3, 1).round().clamp(0, 255).to(torch.uint8).contiguous() for v in range(2)]
    a, hc, wc, m1, m2 = pipeline.run_two_view_u8(u8[0], u8[1], hip_nets, fusion_mode='LINEAR', device=dev)
    hr1, lr1 = pipeline.load_frames_u8(u8[0], device=dev)
    hr2, lr2 = pipeline.load_frames_u8(u8[1], device=dev)
    fr, hc2, wc2, _, _ = pipeline.run_two_view(hr1, hr2, lr1, lr2, hip_nets, 'NORMAL', 'LINEAR')
    assert (hc, wc) == (hc2, wc2)
    assert torch.equal(a, pipeline.to_video_frames(fr))


# ------------------------------------------------------------------ advisor items of round 3
def test_tps_solve_relaxed_pivot_on_near_degenerate_points(dev):
    """the TPS elimination picks its pivot by a 25-bit key of the fp64 magnitude (relaxed partial pivoting).  On
    near-coincident and near-collinear control points the solution must still be as good as an fp64 LAPACK solve of the
    same system: compared through the residual of the 66 x 66 system (the solutions themselves are ill-conditioned)."""
    from stabstitch2_amd import ops
    rs = np.random.RandomState(7)
    base = np.stack(np.meshgrid(np.linspace(-1, 1, 9), np.linspace(-1, 1, 7)), -1).reshape(63, 2)
    sets = []
    a = base.copy(); a[10] = a[11] + 1e-4; a[40] = a[41] + np.array([0.0, 2e-4]); sets.append(a)          # near-coincident pairs
    b = base.copy(); b[:, 1] = 0.3 * b[:, 0] + 1e-3 * rs.randn(63); sets.append(b)                         # near-collinear
    c = base + 0.02 * rs.randn(63, 2); sets.append(c)                                                      # well-posed control
    src = torch.from_numpy(np.stack(sets).astype(np.float32)).to(dev)
    tgt = torch.from_numpy((np.stack(sets) + 0.05 * rs.randn(3, 63, 2)).astype(np.float32)).to(dev)
    T = ops.tps_solve(src, tgt).cpu().numpy().astype(np.float64)          # [3,2,66], coefficient order [a0, ax, ay, w_1..w_63]
    for i in range(3):
        s = src[i].cpu().numpy()
        dx = (s[:, None, 0] - s[None, :, 0]).astype(np.float32)
        dy = (s[:, None, 1] - s[None, :, 1]).astype(np.float32)
        d2 = (dx * dx + dy * dy).astype(np.float32)
        R = (d2 * np.log((d2 + np.float32(1e-6)).astype(np.float64)).astype(np.float32)).astype(np.float64)
        P = np.concatenate((np.ones((63, 1)), s.astype(np.float64)), 1)
        W = np.zeros((66, 66))
        W[:63, :3], W[:63, 3:], W[63:, 3:] = P, R, P.T
        rhs = np.concatenate((tgt[i].cpu().numpy().astype(np.float64), np.zeros((3, 2))), 0)
        ref = np.linalg.solve(W, rhs).astype(np.float32).astype(np.float64)            # fp64 solve, rounded like the kernel's output
        res_ref = np.abs(W @ ref - rhs).max()
        res_gpu = np.abs(W @ T[i].T - rhs).max()
        scale = np.abs(W).max() * max(np.abs(ref).max(), 1.0)
        assert res_gpu <= 10 * res_ref + 1e-6 * scale, (i, res_gpu, res_ref)


def test_window_push_rejects_overlapping_state_blocks(dev):
    """ss_window_push moves its state blocks without ordering between them -- overlapping source / destination
    ranges are an argument error at the C ABI, not a silent race."""
    import ctypes
    from stabstitch2_amd import _hip as H
    ring = torch.zeros((1, 7, 126), device=dev)
    src = torch.zeros(126, device=dev)
    state = torch.zeros(1024, device=dev)
    offs = (ctypes.c_longlong * 1)(0)
    args = lambda blocks, block, stride, delta: (H.dptr(ring), H.dptr(src), ctypes.cast(offs, ctypes.c_void_p), 1, 7, 126,
                                                 H.dptr(state), blocks, block, stride, delta, H.stream())
    H.call('ss_window_push', *args(2, 126, 252, 126))                         # stride = delta + block: fine
    with pytest.raises(H.HipError):
        H.call('ss_window_push', *args(2, 126, 200, 126))                     # block 1's destination inside block 0's source
    with pytest.raises(H.HipError):
        H.call('ss_window_push', *args(1, 126, 0, 100))                       # delta < block


def test_stem_pool_in_several_launches(dev, monkeypatch):
    """batches beyond one launch's 32-bit input offsets are split by ops.stem_pool -- same result."""
    from stabstitch2_amd import ops
    n, h, w = 5, 72, 96
    x = torch.randn(n, 3, h, w, device=dev)
    wgt = torch.zeros(128, 7, 24, device=dev)
    wgt[:, :, :21] = torch.randn(128, 7, 21, device=dev) * 0.1
    bias = torch.randn(128, device=dev)
    buf = ops.stem_input([x])
    want = ops.stem_pool(buf, wgt, bias)
    monkeypatch.setattr(ops, 'STEM_POOL_MAX_BYTES', 2 * h * (w + 8) * 12 + 1)          # two frames per launch
    got = ops.stem_pool(buf, wgt, bias)
    assert torch.equal(got, want)


# ------------------------------------------------------------------ multi-GPU readiness on one GPU
def test_bench_two_ranks_share_one_gpu():
    """`bench.py --gpus 2 --backend gloo --share-device` self-launches two ranks that BOTH drive cuda:0 with
    the real kernels: rank -> clip seed, per-rank timing, the result gather and the N > 1 JSON line on hardware, short of RCCL
    itself (which refuses two ranks on one device; its one-rank all_gather is test_rccl_one_rank_all_gather)."""
    import json
    env = dict(os.environ)
    env['HSA_ENABLE_IPC_MODE_LEGACY'] = '0'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--backend', 'gloo', '--share-device',
                        '--steps', '2', '--warmup', '1', '--frames', '8', '--no-cpu-baseline', '--no-other-configs'],
                       capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d['n_gpus'] == 2 and d['ranks'] == 2 and d['backend'] == 'gloo' and d['share_device'] is True
    assert d['clip_seeds'] == [0, 1] and d['per_rank_device'] == [0, 0]
    assert len(d['per_rank_seconds']) == 2 and all(s > 0 for s in d['per_rank_seconds'])
    assert len(d['per_rank_numa_node']) == 2 and 'placement' in d['host']
    # whole-job value = frames of both ranks / slowest rank
    assert abs(d['value'] - 2 * 8 * 2 / max(d['per_rank_seconds'])) < 1e-2 * d['value']
    assert d['scaling'] == 'weak' and 'x 2 GPUs = configs[3]' in d['config']['workload']


# ------------------------------------------------------------------ batch-of-streams streaming mode
def _stream_inputs(S, n, h, w, dev, seeds):
    hrs, lrs = [], []
    for sd in seeds:
        hr, lr = synth.make_clip_device(n, h, w, seed=sd, device=dev)
        hrs.append(hr)
        lrs.append(lr)
    # [view][stream][frame] -> per push t: [S,3,H,W]
    hr = [torch.stack([hrs[s][v] for s in range(S)], 0) for v in range(2)]          # [S,n,3,H,W]
    lr = [torch.stack([lrs[s][v] for s in range(S)], 0) for v in range(2)]
    return hr, lr


def test_multi_stream_matches_single_streams(dev, hip_nets):
    """MultiOnlineStitcher(streams=4) against four OnlineStitchers fed the same frames: the first window is the single-stream
    code (bit-identical); in the steady state the networks see the four pairs as one batch, and the conv engine picks its
    kernel (Winograd / implicit GEMM / split-K) by launch size -- another summation order, motions ~1e-5 px apart -- so the
    frames are compared with a tolerance far below the path's parity gates.  Graph replay == eager, bit for bit."""
    from stabstitch2_amd.online import MultiOnlineStitcher, OnlineStitcher
    S, n, h, w = 4, 12, 360, 480
    hr, lr = _stream_inputs(S, n, h, w, dev, seeds=[0, 1, 2, 3])
    multi = MultiOnlineStitcher(hip_nets, h, w, streams=S)
    eager = MultiOnlineStitcher(hip_nets, h, w, streams=S, use_graph=False)
    single = [OnlineStitcher(hip_nets, h, w) for _ in range(S)]
    worst = 0.0
    for t in range(n):
        args = (hr[0][:, t].contiguous(), hr[1][:, t].contiguous(), lr[0][:, t].contiguous(), lr[1][:, t].contiguous())
        got = multi.push(*args)
        ge = eager.push(*args)
        for s in range(S):
            want = single[s].push(args[0][s:s + 1], args[1][s:s + 1], args[2][s:s + 1], args[3][s:s + 1])
            assert len(got[s]) == len(want) == len(ge[s])
            for a, b, c in zip(got[s], want, ge[s]):
                assert a.shape == b.shape
                assert torch.equal(a, c), 'graph replay differs from eager'
                if t < 7:
                    assert torch.equal(a, b)
                else:
                    # (the reference's clamped sampler steps from full intensity to 0 across the last image row / column, A6: a
                    # coordinate 1e-5 px apart can flip single edge pixels by a whole grey value -- counted, not bounded)
                    d = (a - b).abs()
                    worst = max(worst, float(d.median()))
                    flips = float((d > 5e-2).float().mean())
                    assert flips < 1e-4 and float(d.mean()) < 2e-3, (t, s, flips, float(d.mean()))
    assert multi.canvas_sizes == [(x.hc, x.wc) for x in single]
    if os.environ.get('SS_VERBOSE'):
        print('multi vs single streams: worst median |diff| %.2e grey levels' % worst)


def test_multi_stream_streams_are_independent(dev, hip_nets):
    """Within a batch a stream's frames do not depend on its neighbours: duplicates of one stream give identical bytes, and
    swapping the other streams changes nothing."""
    from stabstitch2_amd.online import MultiOnlineStitcher
    n, h, w = 10, 360, 480
    hr, lr = _stream_inputs(3, n, h, w, dev, seeds=[5, 6, 5])
    perm = [1, 0, 2]
    a = MultiOnlineStitcher(hip_nets, h, w, streams=3)
    b = MultiOnlineStitcher(hip_nets, h, w, streams=3)
    for t in range(n):
        x = [hr[0][:, t].contiguous(), hr[1][:, t].contiguous(), lr[0][:, t].contiguous(), lr[1][:, t].contiguous()]
        ga = a.push(*x)
        gb = b.push(*[v[perm].contiguous() for v in x])
        for fa, fc in zip(ga[0], ga[2]):
            assert torch.equal(fa, fc)
        for s in range(3):
            for fa, fb in zip(ga[perm[s]], gb[s]):
                assert torch.equal(fa, fb)


# ------------------------------------------------------------------ three-view LINEAR chain pinned on the reference's blender
def test_three_view_linear_blender_internals_vs_reference(dev, golden, hip_nets):
    """G12 (extended in round 4): what the reference's linear_blender sees and decides in its chained three-view calls
    (test_online_tra_threeview.py:489-502) -- warped masks, nonzero counts, centroids, mask1 -- recorded from the reference
    itself, against the product's clip-level LINEAR path.  This pins WHERE the three-view LINEAR frames may move: the masks
    agree to rounding; the centroids (means over nonzero() pixels, which count the clamped sampler's +-1e-3 residues outside
    the image: machine-dependent) agree to a fraction of a pixel; mask1 follows."""
    from stabstitch2_amd import ops, pipeline
    g = golden('g12_threeview_full')
    n = g['mesh1'].shape[1]
    hr, lr = synth.make_clip(n, 180, 320, seed=4, views=3)
    hrd = [torch.cat(v, 0).to(dev) for v in hr]
    lrd = [torch.cat(v, 0).to(dev) for v in lr]
    a12 = pipeline.estimate_meshes(hip_nets, lrd[0], lrd[1], keep_spatial_cache2=True)
    a23 = pipeline.estimate_meshes(hip_nets, lrd[1], lrd[2], tmotion1=a12['tmotion2'], spatial_cache1=a12.get('spatial_cache2'))
    ms = pipeline.three_view_compose(a12['smooth_mesh1'], a12['smooth_mesh2'], a23['smooth_mesh1'], a23['smooth_mesh2'], 180, 320)
    hc, wc, src, T = pipeline.render_plan(list(ms), 180, 320, True)
    assert [hc, wc] == list(g['canvas_linear'])
    _, mk = ops.render_linear_clip([x.contiguous() for x in hrd], src, T, hc, wc, 'NORMAL', want_masks=True)
    box = lambda t: cases.box_down(t.cpu().numpy()[..., None], 4)[..., 0]
    worst = dict(count=0.0, center=0.0, mask=0.0, mask1=0.0)
    for i in range(n):
        wv = ops.tps_warp_views([x[i] for x in hrd], src[i], T[i], hc, wc, 'NORMAL')
        m = [wv[k, 3] for k in range(3)]
        chain = ((m[0], m[1]), (ops.mask_union(m[0], m[1]), m[2]))
        for p, (rm, tm) in enumerate(chain):
            for k, mm in enumerate((rm, tm)):
                nz = torch.nonzero(mm)
                cnt, ctr = nz.shape[0], nz.float().mean(0).cpu().numpy()
                worst['count'] = max(worst['count'], abs(cnt - g['lin_count'][i, p, k]) / g['lin_count'][i, p, k])
                worst['center'] = max(worst['center'], float(np.abs(ctr - g['lin_center'][i, p, 2 * k:2 * k + 2]).max()))
                # (box MEDIANS of a 0 / 1 plane flip by 0.5 in the boxes the image border runs through: quantile, not max)
                worst['mask'] = max(worst['mask'], float(np.quantile(np.abs(box(mm) - g['lin_ref_m' if k == 0 else 'lin_tgt_m'][i, p]), 0.99)))
            d = np.abs(box(mk[i, p]) - g['lin_mask1'][i, p])
            worst['mask1'] = max(worst['mask1'], float(np.quantile(d, 0.999)))
    if os.environ.get('SS_VERBOSE'):
        print('  three-view LINEAR internals vs reference:', worst)
    # observed on MI355X: mask 0 (99 % of the boxes), count 2.8e-3, centre 0.87 px, mask1 4.4e-3
    assert worst['mask'] < 1e-3, worst          # box medians of the warped ones-masks, 99 % of the boxes
    assert worst['count'] < 0.01, worst         # nonzero() counts include the residues outside the image: machine-dependent
    assert worst['center'] < 1.5, worst         # centroids [px]: 0.3 % of the count x the canvas span
    assert worst['mask1'] < 1e-2, worst         # the blend weight (0..1), 99.9 % of the boxes: x the local contrast = the frames' gap


# ------------------------------------------------------------------ the 2x2 max-pool inside the split-K reduction
@pytest.mark.parametrize('shape', [(2, 11, 15, 128, 128), (3, 5, 7, 128, 256), (1, 23, 30, 64, 64), (2, 10, 14, 64, 128)])
def test_conv_pool2_in_splitk_reduce(dev, shape):
    """ops.conv(..., pool2=True) on small maps that run split-K: the reduction kernel takes MaxPool2d(2, 2) itself
    (ss_conv_pool2_nhwc) -- bit-identical to conv + ReLU followed by the max-pool launch, single and grouped."""
    from stabstitch2_amd import ops
    n, h, w, cin, cout = shape
    torch.manual_seed(3)
    x = torch.randn(n, h, w, cin, device=dev)
    wgt = torch.randn(cout, 1, 3, 3, cin, device=dev) * 0.05
    old = ops.WINOGRAD
    ops.WINOGRAD = False                 # force the implicit-GEMM path (the Winograd kernel has its own fused pool)
    try:
        assert ops.pool2_in_reduce(x, wgt)
        got = ops.conv(x, wgt, None, stride=1, pad=(0, 1, 1), relu=True, pool2=True)
        want = ops.maxpool(ops.conv(x, wgt, None, stride=1, pad=(0, 1, 1), relu=True), 2, 2, 0)
        assert torch.equal(got, want)
        xg = torch.randn(2, n, h, w, cin, device=dev)
        wg = torch.randn(2, cout, 1, 3, 3, cin, device=dev) * 0.05
        bg = torch.randn(2, cout, device=dev)
        gotg = ops.conv_grouped(xg, wg, bg, None, stride=1, pad=(0, 1, 1), relu=True, pool2=True)
        y = ops.conv_grouped(xg, wg, bg, None, stride=1, pad=(0, 1, 1), relu=True)
        wantg = ops.maxpool(y.view(2 * n, h, w, cout), 2, 2, 0).view(2, n, h // 2, w // 2, cout)
        assert torch.equal(gotg, wantg)
    finally:
        ops.WINOGRAD = old


# ------------------------------------------------------------------ four heads in shared launches, stream overlap, host runner
def test_quad_regressor_matches_separate_heads(dev, hip_nets):
    """layers.run_regressor_quad (SpatialNet's ref / tgt heads + TemporalNet's head on two views as 4-group launches) against the
    separate heads: same arithmetic per image, the conv engine's kernel choice follows the launch size -> motions within 1e-4 px
    (the parity gate of the networks' outputs); chunked and single-chunk feeding, and the opt-in stream overlap bit for bit."""
    from stabstitch2_amd import pipeline, layers
    n = 20
    _, lr = synth.make_clip_device(n, 360, 480, seed=7, device=dev)
    old = layers.QUAD
    try:
        layers.QUAD = False
        ref = pipeline.joint_stage(hip_nets[0], hip_nets[1], lr[0], lr[1], chunk=8)
        layers.QUAD = True
        got = pipeline.joint_stage(hip_nets[0], hip_nets[1], lr[0], lr[1], chunk=8)
        one = pipeline.joint_stage(hip_nets[0], hip_nets[1], lr[0], lr[1], chunk=32)
        pipeline.QUAD_OVERLAP = True
        ovl = pipeline.joint_stage(hip_nets[0], hip_nets[1], lr[0], lr[1], chunk=8)
    finally:
        layers.QUAD = old
        pipeline.QUAD_OVERLAP = False
    for name, a, b, c, d in zip(('smotion1', 'smotion2', 'tmotion1', 'tmotion2'), ref, got, one, ovl):
        close(b, a, 1e-4, 'quad vs separate heads: ' + name)
        close(c, a, 1e-4, 'quad, one chunk vs separate heads: ' + name)
        assert torch.equal(d, b), name                         # the second stream changes the schedule, not the arithmetic
    assert float(got[2][0].abs().max()) == 0.0 and float(got[3][0].abs().max()) == 0.0      # frame 0: zero temporal motion


def test_host_clip_runner_equals_resident(dev, hip_nets):
    """HostClipRunner (pinned host uint8 in -> pinned host uint8 out through the staging rings, three streams) delivers the
    bytes of run_two_view_u8 on the resident clip, clip after clip, AVERAGE and LINEAR; clips of different lengths reuse the
    rings (a shorter clip takes slices)."""
    from stabstitch2_amd import pipeline
    h, w = 360, 480
    clips = []
    for sd, n in ((0, 12), (1, 12), (2, 9), (3, 12), (4, 12)):
        hr, _ = synth.make_clip_device(n, h, w, seed=sd, device=dev)
        clips.append([hr[v].permute(0, 2, 3, 1).round().clamp(0, 255).to(torch.uint8).contiguous().cpu().pin_memory() for v in range(2)])
    for fusion in ('AVERAGE', 'LINEAR'):
        runner = pipeline.HostClipRunner(hip_nets, dev, fusion_mode=fusion)
        got = [(v.clone(), hc, wc) for v, hc, wc in runner.run((c[0], c[1]) for c in clips)]
        assert len(got) == len(clips)
        for c, (v, hc, wc) in zip(clips, got):
            want, whc, wwc, _, _ = pipeline.run_two_view_u8(c[0].to(dev), c[1].to(dev), hip_nets, fusion_mode=fusion, device=dev)
            assert (hc, wc) == (whc, wwc) and torch.equal(v, want.cpu()), fusion


@pytest.mark.parametrize('warp_mode,fusion_mode', [('FAST', 'LINEAR')])
def test_multi_stream_other_modes(dev, hip_nets, warp_mode, fusion_mode):
    """MultiOnlineStitcher with warp FAST / fusion LINEAR: graph replay equals eager, streams with equal inputs give equal bytes."""
    from stabstitch2_amd.online import MultiOnlineStitcher
    n, h, w = 9, 360, 480
    hr, lr = _stream_inputs(2, n, h, w, dev, seeds=[8, 8])
    a = MultiOnlineStitcher(hip_nets, h, w, streams=2, warp_mode=warp_mode, fusion_mode=fusion_mode)
    b = MultiOnlineStitcher(hip_nets, h, w, streams=2, warp_mode=warp_mode, fusion_mode=fusion_mode, use_graph=False)
    for t in range(n):
        x = [hr[0][:, t].contiguous(), hr[1][:, t].contiguous(), lr[0][:, t].contiguous(), lr[1][:, t].contiguous()]
        ga, gb = a.push(*x), b.push(*x)
        for s in range(2):
            assert len(ga[s]) == len(gb[s])
            for fa, fb in zip(ga[s], gb[s]):
                assert torch.equal(fa, fb)
        for f0, f1 in zip(ga[0], ga[1]):
            assert torch.equal(f0, f1)


def test_multi_stream_of_one_equals_single_stream(dev, hip_nets):
    """MultiOnlineStitcher(streams=1) launches what OnlineStitcher launches (same batch sizes, same kernel choices): bit-identical."""
    from stabstitch2_amd.online import MultiOnlineStitcher, OnlineStitcher
    n, h, w = 10, 360, 480
    hr, lr = _stream_inputs(1, n, h, w, dev, seeds=[9])
    a, b = MultiOnlineStitcher(hip_nets, h, w, streams=1), OnlineStitcher(hip_nets, h, w)
    for t in range(n):
        x = [hr[0][:, t].contiguous(), hr[1][:, t].contiguous(), lr[0][:, t].contiguous(), lr[1][:, t].contiguous()]
        ga, gb = a.push(*x)[0], b.push(*x)
        assert len(ga) == len(gb)
        for fa, fb in zip(ga, gb):
            assert torch.equal(fa, fb), t


def _pushes_of_one_stream(dev, n=10, h=360, w=480, seed=9):
    """The n pushes of one stream as MultiOnlineStitcher(streams=1) takes them ([1,3,H,W] per view): window fill, capture, replays."""
    hr, lr = _stream_inputs(1, n, h, w, dev, seeds=[seed])
    return [[hr[0][:, t].contiguous(), hr[1][:, t].contiguous(), lr[0][:, t].contiguous(), lr[1][:, t].contiguous()] for t in range(n)]


def test_pipelined_multi_stream_of_one_equals_pipelined_single_stream(dev, hip_nets):
    """With two pushes in flight too: PipelinedMultiOnlineStitcher(streams=1) hands out PipelinedOnlineStitcher's frames, bit for bit,
    at every push and at flush()."""
    from stabstitch2_amd.online import PipelinedMultiOnlineStitcher, PipelinedOnlineStitcher
    h, w = 360, 480
    a, b = PipelinedMultiOnlineStitcher(hip_nets, h, w, streams=1), PipelinedOnlineStitcher(hip_nets, h, w)
    got = [(a.push(*x)[0], b.push(*x)) for x in _pushes_of_one_stream(dev)] + [(a.flush()[0], b.flush())]
    assert [len(gb) for _, gb in got] == [0] * 6 + [7, 0] + [1] * 3        # (one push of lag behind the first window)
    for t, (ga, gb) in enumerate(got):
        assert len(ga) == len(gb), t
        for fa, fb in zip(ga, gb):
            assert torch.equal(fa, fb), t


def test_multi_stream_of_one_push_u8_equals_single_stream(dev, hip_nets):
    """MultiOnlineStitcher(streams=1).push_u8 against OnlineStitcher.push_u8 on the same decoded frames: byte-equal video frames."""
    from stabstitch2_amd.online import MultiOnlineStitcher, OnlineStitcher
    h, w = 360, 480
    a, b = MultiOnlineStitcher(hip_nets, h, w, streams=1), OnlineStitcher(hip_nets, h, w)
    frames = 0
    for t, x in enumerate(_pushes_of_one_stream(dev)):
        u8 = [f.clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous() for f in x[:2]]        # [1,H,W,3]
        ga, gb = a.push_u8(*u8)[0], b.push_u8(u8[0][0], u8[1][0])
        assert len(ga) == len(gb), t
        for fa, fb in zip(ga, gb):
            assert fa.dtype == torch.uint8 and torch.equal(fa, fb), t
        frames += len(gb)
    assert frames == 10


@pytest.mark.parametrize('use_graph', [True, False])
def test_multi_stream_of_one_meshes_equal_single_stream(dev, hip_nets, use_graph):
    """meshes_only: MultiOnlineStitcher(streams=1) returns OnlineStitcher's smoothed meshes with a stream axis in front, bit for bit,
    captured and eager."""
    from stabstitch2_amd.online import MultiOnlineStitcher, OnlineStitcher
    h, w = 360, 480
    a = MultiOnlineStitcher(hip_nets, h, w, streams=1, meshes_only=True, use_graph=use_graph)
    b = OnlineStitcher(hip_nets, h, w, meshes_only=True, use_graph=use_graph)
    for t, x in enumerate(_pushes_of_one_stream(dev)):
        ga, gb = a.push(None, None, x[2], x[3]), b.push(None, None, x[2], x[3])
        assert (ga is None) == (gb is None) == (t < 6), t
        if gb is not None:
            k = 7 if t == 6 else 1
            for ma, mb in zip(ga, gb):
                assert tuple(ma.shape) == (1, k, 7, 9, 2) and tuple(mb.shape) == (k, 7, 9, 2) and torch.equal(ma[0], mb), t


def test_pipelined_multi_stream_of_one_reports_as_the_plain_stitchers(dev, hip_nets):
    """After the same ten pushes PipelinedMultiOnlineStitcher(streams=1) reads the same overflow_report() and canvas_box as the plain
    stitchers: MultiOnlineStitcher(streams=1)'s lists, whose one entry is OnlineStitcher's."""
    from stabstitch2_amd.online import MultiOnlineStitcher, OnlineStitcher, PipelinedMultiOnlineStitcher
    h, w = 360, 480
    p, m, o = (PipelinedMultiOnlineStitcher(hip_nets, h, w, streams=1), MultiOnlineStitcher(hip_nets, h, w, streams=1),
               OnlineStitcher(hip_nets, h, w))
    for x in _pushes_of_one_stream(dev):
        p.push(*x), m.push(*x), o.push(*x)
    want = o.overflow_report()
    assert want['frames_seen'] == 10 and want['box'] is not None
    assert p.overflow_report() == m.overflow_report() == [want]
    assert p.canvas_box == m.canvas_box == [o.canvas_box]
    p.flush()


def test_multi_stream_shared_canvas_size_renders_as_one_clip(dev, hip_nets):
    """Streams whose canvases have one size (the caller fixed them) render in ONE launch per push (the S current frames are a
    clip): same bytes as the per-stream launches of single-stream stitchers with the same canvases' inputs."""
    from stabstitch2_amd.online import MultiOnlineStitcher
    n, h, w = 10, 360, 480
    hr, lr = _stream_inputs(3, n, h, w, dev, seeds=[1, 2, 3])
    canvas = (-120.0, 600.0, -10.0, 372.0)
    a = MultiOnlineStitcher(hip_nets, h, w, streams=3, canvases=[canvas] * 3)                 # one size -> batched render
    b = MultiOnlineStitcher(hip_nets, h, w, streams=3, canvases=[canvas, (-121.0, 600.0, -10.0, 372.0), canvas])   # sizes differ -> per stream
    for t in range(n):
        x = [hr[0][:, t].contiguous(), hr[1][:, t].contiguous(), lr[0][:, t].contiguous(), lr[1][:, t].contiguous()]
        ga, gb = a.push(*x), b.push(*x)
        for s in (0, 2):                                   # streams 0 and 2 have the same canvas in both stitchers
            assert len(ga[s]) == len(gb[s])
            for fa, fb in zip(ga[s], gb[s]):
                assert torch.equal(fa, fb), (t, s)
    assert a.static['out_all'] is not None and b.static['out_all'] is None


def test_cost_volume_output_pitch_paths(dev):
    """The cost volume's epilogue has a vectorised path for the usual output pitch (channels padded to a multiple of 4) and a
    generic one for any other pitch: same values, zeros in the padding; both tile heights."""
    from stabstitch2_amd import _hip as H, ops
    torch.manual_seed(0)
    for r, d in ((5, 121), (3, 49)):
        a = torch.randn(2, 13, 21, 32, device=dev)
        b = torch.randn(2, 13, 21, 32, device=dev)
        ref = ops.cost_volume(a, b, r)                                # pitch d + 3
        assert ref.shape[-1] == d + 3 and float(ref[..., d:].abs().max()) == 0.0
        for ty in (4, 8):
            H.lib().ss_cost_volume_set_tile(ty)
            try:
                wide = torch.full((2, 13, 21, d + 7), 7.0, device=dev)
                H.call('ss_cost_volume', H.dptr(a), H.dptr(b), H.dptr(wide), 2, 13, 21, 32, r, d + 7, H.stream())
                assert torch.equal(ops.cost_volume(a, b, r), ref)
            finally:
                H.lib().ss_cost_volume_set_tile(0)
            assert torch.equal(wide[..., :d], ref[..., :d]) and float(wide[..., d:].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# Winograd F(4x4,3x3) (csrc/wino43.hip): the trunk's stride-1 3x3 layers on deep launches
@pytest.mark.parametrize('shape', [(3, 45, 60, 128, 128, True, True), (2, 90, 120, 64, 64, True, False),
                                   (2, 23, 30, 64, 128, False, True), (1, 8, 61, 32, 64, True, True),
                                   (2, 7, 9, 16, 64, False, False), (1, 17, 131, 48, 192, True, True)])
def test_conv_wino43_against_fp64(dev, shape):
    """nn.Conv2d(3x3, stride 1, pad 1) + folded-BN bias + residual + ReLU (spatial_network.py:132-136) on the F(4x4,3x3) kernel
    against the same layer in fp64: maps that end inside a tile block (rows and columns), more than one 60-pixel block per row,
    cin below one MFMA block, three cout blocks.  Tolerance: F(4x4,3x3)'s transform constants (4, -5, 8) cost ~20x the
    rounding error of F(2x2,3x3); measured 2e-5 .. 9e-5 of max|y| on these shapes, gate 2e-4 (F(2x2,3x3): 4e-5)."""
    from stabstitch2_amd import ops
    import torch.nn.functional as F
    n, h, w, cin, cout, with_res, relu = shape
    g = torch.Generator().manual_seed(1234 + h * w + cin)
    x = torch.randn(n, h, w, cin, generator=g).to(dev)
    wgt = (torch.randn(cout, 1, 3, 3, cin, generator=g) * (1.0 / (9 * cin)) ** 0.5).to(dev)
    bias = (torch.randn(cout, generator=g) * 0.1).to(dev)
    res = torch.randn(n, h, w, cout, generator=g).to(dev) if with_res else None
    ref = F.conv2d(x.permute(0, 3, 1, 2).double(), wgt[:, 0].permute(0, 3, 1, 2).double(), bias.double(), padding=1).permute(0, 2, 3, 1)
    if with_res:
        ref = ref + res.double()
    if relu:
        ref = torch.relu(ref)
    y = ops.conv_winograd43(x, wgt, bias, res, relu)
    scale = max(1.0, float(ref.abs().max()))
    close(y, ref.float(), 2e-4 * scale, 'F(4x4,3x3) vs fp64 conv %s' % (shape,))
    # a channel-padded destination keeps its padding; no bias
    wide = torch.full((n, h, w, cout + 8), 7.0, device=dev)
    ops.conv_winograd43(x, wgt, None, None, False, out=wide)
    assert float((wide[..., cout:] - 7.0).abs().max()) == 0.0
    ref0 = F.conv2d(x.permute(0, 3, 1, 2).double(), wgt[:, 0].permute(0, 3, 1, 2).double(), None, padding=1).permute(0, 2, 3, 1)
    close(wide[..., :cout], ref0.float(), 2e-4 * max(1.0, float(ref0.abs().max())), 'F(4x4,3x3), no bias, wide destination')


def test_conv_wino43_groups_and_limits(dev):
    """Grouped launches (group strides, one input shared by both groups) equal the single launches bit for bit; geometry the kernel
    does not take is refused, not mis-computed."""
    from stabstitch2_amd import ops, _hip
    g = torch.Generator().manual_seed(77)
    x = torch.randn(2, 3, 16, 60, 32, generator=g).to(dev)
    w = (torch.randn(2, 64, 1, 3, 3, 32, generator=g) / 17.0).to(dev)
    b = torch.randn(2, 64, generator=g).to(dev)
    r = torch.randn(2, 3, 16, 60, 64, generator=g).to(dev)
    y = ops.conv_winograd43(x, w, b, r, True)
    for k in range(2):
        one = ops.conv_winograd43(x[k].contiguous(), w[k].contiguous(), b[k].contiguous(), r[k].contiguous(), True)
        assert torch.equal(y[k], one)
    shared = ops.conv_winograd43(x[0].contiguous(), w, b, r, True)
    assert torch.equal(shared[0], y[0])
    lib = _hip.lib()
    assert lib.ss_wino43_packed_floats(64, 24) == 0 and lib.ss_wino43_packed_floats(48, 32) == 0
    assert lib.ss_wino43_packed_floats(64, 32) == 2 * 2 * 36 * 2 * 64 * 4
    xs = torch.randn(1, 8, 8, 32, generator=g).to(dev)
    pk = torch.zeros(1 << 16, device=dev)
    out = torch.zeros(1, 8, 8, 64, device=dev)
    with pytest.raises(_hip.HipError, match='unsupported'):         # cin % 16
        _hip.call('ss_conv3x3_wino43_nhwc', _hip.dptr(xs), _hip.dptr(pk), None, None, _hip.dptr(out), 1, 8, 8, 24, 64, 0, 64, 1, 0, 0, 0, _hip.stream())
    with pytest.raises(_hip.HipError, match='bad argument'):        # out_cs < cout
        _hip.call('ss_conv3x3_wino43_nhwc', _hip.dptr(xs), _hip.dptr(pk), None, None, _hip.dptr(out), 1, 8, 8, 32, 64, 0, 32, 1, 0, 0, 0, _hip.stream())


def test_wino43_dispatch_rule_and_pipeline_agreement(dev, hip_nets):
    """ops.conv takes F(4x4,3x3) for the deep launches of the 60 / 120-wide trunk maps only, and a whole clip estimated with it
    agrees with the F(2x2,3x3)-only engine far inside the reference gates (offsets / motions 1e-4 px)."""
    from stabstitch2_amd import ops, pipeline
    assert ops._uses_wino43(1, 3, 3, 1, (0, 1, 1), 128, 128, 45, 60, 64)
    assert ops._uses_wino43(1, 3, 3, 1, (0, 1, 1), 64, 64, 90, 120, 64)
    assert ops._uses_wino43(1, 3, 3, 1, (0, 1, 1), 256, 256, 23, 30, 64)          # 30-wide map: the 16 x 32 block geometry (round 5)
    assert not ops._uses_wino43(1, 3, 3, 1, (0, 1, 1), 128, 128, 11, 15, 64)      # regressor maps fill a third of such a block
    assert not ops._uses_wino43(1, 3, 3, 1, (0, 1, 1), 128, 128, 45, 60, 2)       # streaming-sized launch
    assert not ops._uses_wino43(1, 3, 3, 2, (0, 1, 1), 64, 128, 45, 60, 64)       # strided
    assert not ops._uses_wino43(1, 3, 3, 1, (0, 1, 1), 4, 64, 90, 120, 64)        # cin % 16
    _, lr = synth.make_clip_device(40, 360, 480, seed=5, device=dev)
    old = ops.WINO43
    try:
        ops.WINO43 = 'auto'
        with_43 = pipeline.joint_stage(hip_nets[0], hip_nets[1], lr[0], lr[1])
        assert ops.last_conv_path is not None
        ops.WINO43 = '0'
        without = pipeline.joint_stage(hip_nets[0], hip_nets[1], lr[0], lr[1])
    finally:
        ops.WINO43 = old
    # spatial motions come out of the DLT / decomposition, which amplifies offset differences (their gate against the reference
    # goldens is 5e-3 px, G8); temporal motions are network outputs (gate 1e-4)
    for x43, x23, name, tol in zip(with_43, without, ('spatial motions 1', 'spatial motions 2', 'temporal motions 1', 'temporal motions 2'),
                                   (5e-4, 5e-4, 1e-4, 1e-4)):
        d = float((x43 - x23).abs().max())
        assert 0.0 < d < tol, (name, d)       # (0 would mean the F(4x4,3x3) kernel never ran)


def test_reference_goldens_with_wino43_everywhere(dev, golden, hip_nets, clip16, monkeypatch):
    """The reference goldens (G8: offsets / motions of both nets, spatial_network.py:276-331, temporal_network.py:24-60; G9 / G10:
    the pipeline) with EVERY eligible stride-1 3x3 layer forced onto the F(4x4,3x3) kernel -- the golden clips are 16 frames,
    too shallow for the dispatch rule to pick it by itself.  Same gates as with F(2x2,3x3)."""
    import test_gpu_parity as T
    from stabstitch2_amd import ops
    calls = [0]
    real = ops.conv_winograd43

    def counted(*a, **k):
        calls[0] += 1
        return real(*a, **k)
    monkeypatch.setattr(ops, 'conv_winograd43', counted)
    monkeypatch.setattr(ops, 'WINO43', '1')
    T.test_nets_vs_reference(dev, golden, hip_nets, clip16)
    assert calls[0] >= 10, calls
    T.test_pipeline_vs_reference(dev, golden, hip_nets, clip16)


def test_conv_wino43_random_geometry(dev):
    """Sixteen seeded random geometries of the F(4x4,3x3) kernel against fp64: maps from 1 x 1 up to several tile blocks in both
    directions (rows not a multiple of 8, columns not a multiple of 60 / 4), 1-3 images, 16-80 input channels, residual / ReLU at
    random.  Same gate as test_conv_wino43_against_fp64."""
    from stabstitch2_amd import ops
    import torch.nn.functional as F
    rs = np.random.RandomState(20260929)
    for case in range(16):
        n = int(rs.randint(1, 4))
        h = int(rs.choice([1, 2, 3, 5, 8, 9, 17, 31, 46]))
        w = int(rs.choice([1, 2, 4, 7, 59, 60, 61, 64, 121, 139]))
        cin = int(rs.choice([16, 32, 48, 64, 80]))
        cout = int(rs.choice([64, 128]))
        with_res, relu = bool(rs.randint(2)), bool(rs.randint(2))
        g = torch.Generator().manual_seed(1000 + case)
        x = torch.randn(n, h, w, cin, generator=g).to(dev)
        wgt = (torch.randn(cout, 1, 3, 3, cin, generator=g) * (1.0 / (9 * cin)) ** 0.5).to(dev)
        bias = (torch.randn(cout, generator=g) * 0.1).to(dev)
        res = torch.randn(n, h, w, cout, generator=g).to(dev) if with_res else None
        ref = F.conv2d(x.permute(0, 3, 1, 2).double(), wgt[:, 0].permute(0, 3, 1, 2).double(), bias.double(), padding=1).permute(0, 2, 3, 1)
        if with_res:
            ref = ref + res.double()
        if relu:
            ref = torch.relu(ref)
        y = ops.conv_winograd43(x, wgt, bias, res, relu)
        close(y, ref.float(), 2e-4 * max(1.0, float(ref.abs().max())), 'F(4x4,3x3) random case %d: n %d %dx%d %d->%d res %d relu %d'
              % (case, n, h, w, cin, cout, with_res, relu))
