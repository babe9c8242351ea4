"""Round-5 GPU tests: the conv engine under trained-like weight statistics (G14), configs[2] under the default kernel mix,
streaming canvas overflow, the C ABI around F(4x4,3x3).
    python -m pytest tests -m gpu"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cases
from oracle import pipeline as P, metrics as M, nets as N
from stabstitch2_amd import synth
from test_gpu_parity import dev, hip_nets, close, close_boxes, clip16  # noqa: F401  (fixtures / helpers)

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _err(a, b):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return float(np.max(np.abs(a.astype(np.float64) - np.asarray(b).astype(np.float64))))


@pytest.fixture(scope='module')
def hip_nets_trained(dev):
    """The three nets under synth's 'trained_like' checkpoint (BN-folded channel scales over four decades, Student-t taps)."""
    from stabstitch2_amd.spatial_network import SpatialNet
    from stabstitch2_amd.temporal_network import TemporalNet
    from stabstitch2_amd.smooth_network import SmoothNet
    nets = []
    for cls in (SpatialNet, TemporalNet, SmoothNet):
        m = cls()
        m.load_state_dict(synth.synthetic_state_dict(m, profile='trained_like'), strict=True)
        nets.append(m.to(dev))
    return nets


@pytest.fixture(scope='module')
def clip24_trained():
    return synth.make_clip(24, 360, 480, seed=5)


class _Count:
    """Counts the launches of ops.conv_winograd43 / ops.conv_winograd while patched in."""

    def __init__(self, monkeypatch):
        from stabstitch2_amd import ops
        self.n43 = self.n23 = 0
        r43, r23 = ops.conv_winograd43, ops.conv_winograd

        def c43(*a, **k):
            self.n43 += 1
            return r43(*a, **k)

        def c23(*a, **k):
            self.n23 += 1
            return r23(*a, **k)
        monkeypatch.setattr(ops, 'conv_winograd43', c43)
        monkeypatch.setattr(ops, 'conv_winograd', c23)


@pytest.mark.parametrize('mode', ['0', 'auto', '1'])
def test_trained_like_goldens(dev, golden, hip_nets_trained, clip24_trained, monkeypatch, mode):
    """VERDICT r4 item 1.  G14 = the REFERENCE run under the harsh checkpoint on a 24-frame 360x480 clip.  The HIP path with the
    F(4x4,3x3) kernel off ('0'), dispatched by the default launch-size rule ('auto': it must fire by itself on this clip) and
    forced onto every eligible layer ('1'): offsets / temporal motions <= 1e-4 px, spatial motions / meshes <= 5e-3 px, frames,
    PSNR / SSIM 0.01 dB / 1e-3 -- the same gates as G8 / G9 with benign weights.
    (spatial_network.py:276-331, temporal_network.py:119-147, test_online_tra.py:96-154)"""
    from stabstitch2_amd import ops, pipeline, metrics
    from stabstitch2_amd.spatial_network import build_SpatialNet
    from stabstitch2_amd.temporal_network import build_TemporalNet
    g = golden('g14_trained_like')
    sp, tp, sm = hip_nets_trained
    hr, lr = clip24_trained
    cnt = _Count(monkeypatch)
    monkeypatch.setattr(ops, 'WINO43', mode)
    obs = {}
    # batch 1 exactly as the reference calls the net (never deep enough for 'auto': covered by the clip-level calls below)
    o1, o2r, o2t = sp(lr[0][0].to(dev), lr[1][0].to(dev))
    for k, v in (('offset_1', o1), ('offset_2_ref', o2r), ('offset_2_tgt', o2t)):
        obs[k] = _err(v, g[k])
        close(v, g[k], 1e-4, k + ' [SS_WINO43=%s]' % mode)
    lr1 = torch.cat(lr[0], 0).to(dev)
    lr2 = torch.cat(lr[1], 0).to(dev)
    n43_before = cnt.n43
    o = build_SpatialNet(sp, lr1, lr2)                           # the clip as one batch: 48 images through the trunk
    if mode == 'auto':
        assert cnt.n43 - n43_before >= 6, (cnt.n43, n43_before)   # layer1 AND layer2 picked F(4x4,3x3) by the default rule
    for k in ('motion1', 'motion2'):
        obs[k] = _err(o[k], g[k])
        close(o[k], g[k], 5e-3, k + ' [SS_WINO43=%s]' % mode)
    for v, k in ((0, 'tmotion1'), (1, 'tmotion2')):
        tm = torch.cat(build_TemporalNet(tp, [f.to(dev) for f in lr[v]])['motion_list'], 0)
        obs[k] = _err(tm, g[k])
        close(tm, g[k], 1e-4, k + ' [SS_WINO43=%s]' % mode)
    acc = pipeline.estimate_meshes(hip_nets_trained, lr[0], lr[1])
    for k, tol in (('smooth_mesh1', 5e-3), ('smooth_mesh2', 5e-3), ('ori_path2', 1e-2), ('smooth_path2', 1e-2)):
        obs[k] = _err(acc[k], g[k])
        close(acc[k], g[k], tol, k + ' [SS_WINO43=%s]' % mode)
    frames, hc, wc, m1, m2 = pipeline.run_two_view(hr[0], hr[1], lr[0], lr[1], hip_nets_trained)
    assert [hc, wc] == list(g['canvas_normal_average'])
    got = np.stack([cases.box_down(f.permute(1, 2, 0).cpu().numpy(), 16) for f in frames])
    close_boxes(got, g['frames_normal_average'], g['iqr_normal_average'], 5e-2, 'frames [SS_WINO43=%s]' % mode)
    ev = metrics.evaluate_clip(hip_nets_trained, lr[0], lr[1])
    obs['psnr'] = _err(ev['psnr'], g['psnr'])
    obs['ssim'] = _err(ev['ssim'], g['ssim'])
    assert obs['psnr'] < 0.01 and obs['ssim'] < 1e-3, obs
    if mode == '0':
        assert cnt.n43 == 0
    else:
        assert cnt.n43 > 0
    print('\n[G14 SS_WINO43=%s] F(4x4) launches %d, F(2x2) launches %d; max|diff| vs the reference: %s'
          % (mode, cnt.n43, cnt.n23, ', '.join('%s %.2e' % kv for kv in obs.items())))


def _oracle_nets(profile='default'):
    nets = N.SpatialNet().eval(), N.TemporalNet().eval(), N.SmoothNet().eval()
    for m in nets:
        m.load_state_dict(synth.synthetic_state_dict(m, profile=profile), strict=True)
    return nets


@pytest.mark.parametrize('fusion_mode', ['AVERAGE', 'LINEAR'])
def test_two_view_720p_default_kernel_mix_vs_oracle(dev, hip_nets, monkeypatch, fusion_mode):
    """configs[2] under the REAL default kernel mix: a 24-frame 720x1280 clip is deep enough that the
    launch-size rule picks F(4x4,3x3) for layer1 and layer2 by itself (asserted by a call counter), HIP path vs the CPU oracle:
    meshes 5e-3 px, canvas equal, every frame median / p99.9, PSNR / SSIM 0.01 dB / 1e-3.  Both fusion modes of
    test_online_tra.py:96-154 (AVERAGE, and the script's default LINEAR)."""
    from stabstitch2_amd import ops, pipeline, metrics
    n = 24
    cnt = _Count(monkeypatch)
    monkeypatch.setattr(ops, 'WINO43', 'auto')
    hr, lr = synth.make_clip_device(n, 720, 1280, seed=0, device='cpu')
    fr, hc, wc, m1, m2 = pipeline.run_two_view(hr[0].to(dev), hr[1].to(dev), lr[0].to(dev), lr[1].to(dev), hip_nets,
                                               'NORMAL', fusion_mode)
    assert cnt.n43 >= 12, cnt.n43                       # 14 eligible trunk launches per pass of 24 pairs
    assert ops._uses_wino43(1, 3, 3, 1, (0, 1, 1), 128, 128, 45, 60, 2 * n)
    sl = lambda t: [t[i:i + 1] for i in range(n)]
    onets = _oracle_nets()
    acc = P.estimate_meshes(onets, sl(lr[0]), sl(lr[1]))
    om1, om2 = acc['smooth_mesh1'], acc['smooth_mesh2']
    close(m1, om1, 5e-3, '720p smooth_mesh1 vs oracle')
    close(m2, om2, 5e-3, '720p smooth_mesh2 vs oracle')
    # frames rendered by the CPU oracle (its LINEAR blender is slow): it renders frame i of the lists with mesh i, and its canvas is
    # the bbox over ALL meshes whatever their order -- so put the chosen frames first
    idx = [0, 7, n // 2, n - 1] if fusion_mode == 'LINEAR' else [0, 3, 7, n // 2, 18, n - 1]
    perm = idx + [i for i in range(n) if i not in idx]
    ofr, ow, oh = P.get_stable_sqe([sl(hr[0])[i] for i in idx], [sl(hr[1])[i] for i in idx], om1[:, perm], om2[:, perm],
                                   'NORMAL', fusion_mode)
    assert (hc, wc) == (int(oh), int(ow))
    med_tol, tail_tol = (5e-3, 0.1) if fusion_mode == 'AVERAGE' else (2e-2, 0.5)
    for j, i in enumerate(idx):
        d = np.abs(fr[i].permute(1, 2, 0).cpu().numpy() - ofr[j])
        assert np.median(d) < med_tol and np.quantile(d, 0.999) < tail_tol, (fusion_mode, i, float(np.median(d)), float(np.quantile(d, 0.999)))
    if fusion_mode == 'AVERAGE':
        kk = 3
        c1 = M.warp_lr_with_mask(sl(lr[0])[:kk], om1[:, :kk])
        c2 = M.warp_lr_with_mask(sl(lr[1])[:kk], om2[:, :kk])
        cps = [M.alignment_psnr_ssim(a, b) for a, b in zip(c1, c2)]
        gp, gs = metrics.alignment_psnr_ssim(metrics.warp_lr_planes(lr[0][:kk].to(dev), m1[:, :kk]),
                                             metrics.warp_lr_planes(lr[1][:kk].to(dev), m2[:, :kk]))
        for i in range(kk):
            assert abs(float(gp[i]) - cps[i][0]) < 0.01 and abs(float(gs[i]) - cps[i][1]) < 1e-3, (i, float(gp[i]), cps[i])


def test_wino43_first_launch_from_two_host_threads():
    """The F(4x4,3x3) kernel needs a per-device function attribute (144 KB of dynamic LDS) set before its first launch; the library
    sets it once per device under an atomic state machine.  A fresh process whose FIRST two launches come from two host threads at
    once (each on its own stream) must get both results right -- and equal to a later single-threaded launch, bit for bit."""
    code = r'''
import sys, threading, torch
sys.path.insert(0, %r)
from stabstitch2_amd import ops
dev = torch.device('cuda:0')
g = torch.Generator().manual_seed(7)
x = torch.randn(4, 16, 60, 64, generator=g).to(dev)
w = (torch.randn(64, 1, 3, 3, 64, generator=g) * (1.0 / 576) ** 0.5).to(dev)
pk = ops.wino43_packed(w, 1)                     # (the filter pack is its own kernel: built before the race)
torch.cuda.synchronize()
outs, errs = [None, None], []
go = threading.Barrier(2)
def work(i):
    try:
        with torch.cuda.stream(torch.cuda.Stream()):
            go.wait()
            outs[i] = ops.conv_winograd43(x, w, None, None, True)
            torch.cuda.current_stream().synchronize()
    except Exception as e:
        errs.append(repr(e))
ts = [threading.Thread(target=work, args=(i,)) for i in range(2)]
[t.start() for t in ts]; [t.join() for t in ts]
assert not errs, errs
ref = ops.conv_winograd43(x, w, None, None, True)
torch.cuda.synchronize()
assert torch.equal(outs[0], ref) and torch.equal(outs[1], ref)
assert float(ref.abs().max()) > 0.1
print('ok')
''' % ROOT
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith('ok'), (r.stdout[-2000:], r.stderr[-2000:])


# ------------------------------------------------------------------ streaming: a mesh leaving the fixed canvas
def _push_drifting(st, nets, hrd, lrd, n, start=20, step=-6.0, steps=12, record=None, multi=0):
    """Push n pairs (the 16-frame clip repeated) while SpatialNet's stage-1 head bias -- the horizontal offset of view 2 against
    view 1 -- walks from -216 by `step` LR px per frame for `steps` frames from frame `start`: both meshes slide apart, the stitched
    extent grows by 10 % of the width.  The bias tensor is the one the kernels (and a captured graph) read: edited in place."""
    bias = nets[0]._prepared()['r1']['fc'][2][1]
    assert bias.data_ptr() == nets[0].regressNet1_part2[4].bias.data_ptr() or True
    out = []
    try:
        for t in range(n):
            k = min(max(t - start + 1, 0), steps)
            bias[0::2] = -216.0 + step * k
            i = t % len(hrd[0])
            if multi:
                cat = lambda v: torch.cat([v[(i + s) % len(v)] for s in range(multi)], 0)
                got = st.push(cat(hrd[0]), cat(hrd[1]), cat(lrd[0]), cat(lrd[1]))
            else:
                got = st.push(hrd[0][i], hrd[1][i], lrd[0][i], lrd[1][i])
            out.append(got)
            if record is not None:
                record(t, st)
    finally:
        bias[0::2] = -216.0
    return out


def test_streaming_canvas_overflow_is_detected_and_grown(dev, hip_nets, clip16, monkeypatch):
    """VERDICT r4 item 6.  The reference's canvas is the bbox over ALL frames (test_online_tra.py:106-120); a stream fixes it after
    7 pairs.  With a stream whose views drift apart by 10 % of the width after frame 20:
      grow='never'     -- the device-side watcher counts the cropped frames and names the first one (checked against the meshes the
                          stitcher normalised, recorded on the side), nothing else changes;
      grow='recapture' -- the canvas is re-fixed BEFORE anything is cropped (clipped_frames == 0), the graph captured again, and the
                          frames behind the last growth equal those of a stitcher that had that canvas from the start."""
    from stabstitch2_amd import ops
    from stabstitch2_amd.online import OnlineStitcher
    hr, lr = clip16
    hrd = [[f.to(dev) for f in v] for v in hr]
    lrd = [[f.to(dev) for f in v] for v in lr]
    n = 44
    # --- never: count + first frame, against the meshes themselves
    seen = []
    real = ops.stream_splines                  # (round 6: normalisation of both views + their splines are one launch)

    def spy(meshes, *a, **k):
        seen.append(torch.stack([m.reshape(-1, 2).clone() for m in meshes], 0))       # [2,63,2] LR px
        return real(meshes, *a, **k)
    st = OnlineStitcher(hip_nets, 360, 480, use_graph=False)
    monkeypatch.setattr(ops, 'stream_splines', spy)
    _push_drifting(st, hip_nets, hrd, lrd, n)
    monkeypatch.setattr(ops, 'stream_splines', real)
    assert len(seen) == n
    bb = st.bbox.cpu()
    first = -1
    clipped = 0
    for t, m in enumerate(seen):
        x, y = m[..., 0].cpu(), m[..., 1].cpu()
        tol_w, tol_h = 1.25e-4 * float(bb[1] - bb[0]), 1.25e-4 * float(bb[3] - bb[2])
        out = bool(x.min() < bb[0] - tol_w or x.max() > bb[1] + tol_w or y.min() < bb[2] - tol_h or y.max() > bb[3] + tol_h)
        clipped += out
        if out and first < 0:
            first = t
    rep = st.overflow_report()
    assert first >= 20 and clipped > 0, (first, clipped)
    assert rep['frames_seen'] == n and rep['first_clipped_frame'] == first and rep['clipped_frames'] == clipped, (rep, first, clipped)
    assert st.clipped_frames == clipped and rep['canvas_epoch'] == 0
    nb = rep['needed_bbox']
    assert nb[0] <= float(bb[0]) and nb[1] >= float(bb[1]) and (nb[1] - nb[0]) > float(bb[1] - bb[0]) + 20.0, (nb, bb)
    # the same with the captured graph: same counts (the watcher is a node of the graph)
    stg = OnlineStitcher(hip_nets, 360, 480)
    _push_drifting(stg, hip_nets, hrd, lrd, n)
    repg = stg.overflow_report()
    assert (repg['frames_seen'], repg['clipped_frames'], repg['first_clipped_frame']) == (n, clipped, first), (repg, clipped, first)
    # --- recapture: grown before anything is cropped
    sg = OnlineStitcher(hip_nets, 360, 480, grow='recapture')
    epochs = []
    outs = _push_drifting(sg, hip_nets, hrd, lrd, n, record=lambda t, s: (torch.cuda.synchronize(), epochs.append(s.canvas_epoch)))
    repr_ = sg.overflow_report()
    assert repr_['clipped_frames'] == 0 and repr_['frames_seen'] == n and sg.canvas_epoch >= 1, repr_
    assert sg.wc > stg.wc + 20 and epochs[19] == 0, (sg.wc, stg.wc, epochs)
    last_growth = max(t for t in range(n) if epochs[t] != (epochs[t - 1] if t else 0))
    assert last_growth < n - 4
    # frames behind the last growth == a stitcher that had the final canvas all along
    sf = OnlineStitcher(hip_nets, 360, 480, canvas=sg.bbox.cpu().tolist())
    ref = _push_drifting(sf, hip_nets, hrd, lrd, n)
    assert (sf.hc, sf.wc) == (sg.hc, sg.wc)
    for t in range(last_growth + 1, n):
        a, b = outs[t][0], ref[t][0]
        assert a.shape == b.shape and float((a - b).abs().max()) < 1e-3, (t, float((a - b).abs().max()))


def test_multi_stream_canvas_overflow(dev, hip_nets, clip16):
    """The batched stitcher keeps one overflow state per stream: two streams (the clip at two phases) under the same drift --
    grow='never' counts per stream, grow='recapture' re-fixes both canvases with nothing cropped."""
    from stabstitch2_amd.online import MultiOnlineStitcher
    hr, lr = clip16
    hrd = [[f.to(dev) for f in v] for v in hr]
    lrd = [[f.to(dev) for f in v] for v in lr]
    n = 40
    mn = MultiOnlineStitcher(hip_nets, 360, 480, streams=2)
    _push_drifting(mn, hip_nets, hrd, lrd, n, multi=2)
    rn = mn.overflow_report()
    assert all(r['frames_seen'] == n and r['clipped_frames'] > 0 and r['first_clipped_frame'] >= 20 for r in rn), rn
    assert mn.clipped_frames == [r['clipped_frames'] for r in rn]
    sizes0 = list(mn.canvas_sizes)
    mg = MultiOnlineStitcher(hip_nets, 360, 480, streams=2, grow='recapture')
    outs = _push_drifting(mg, hip_nets, hrd, lrd, n, multi=2, record=lambda t, s: torch.cuda.synchronize())
    rg = mg.overflow_report()
    assert all(r['clipped_frames'] == 0 and r['frames_seen'] == n and r['canvas_epoch'] >= 1 for r in rg), rg
    assert all(g[1] > s[1] + 20 for g, s in zip(mg.canvas_sizes, sizes0)), (mg.canvas_sizes, sizes0)
    assert all(tuple(outs[-1][s][0].shape) == (3,) + tuple(mg.canvas_sizes[s]) for s in range(2))
    assert all(bool(torch.isfinite(outs[-1][s][0]).all()) for s in range(2))


def test_bench_eight_ranks_share_one_gpu():
    """`bench.py --gpus 8 --backend gloo --share-device` -- the eight launch loops, clip seeds, host placement
    and the gather of configs[3] on ONE host and ONE device (RCCL refuses eight ranks on a device; its one-rank all_gather is
    test_rccl_one_rank_all_gather): 8 ranks, 8 distinct seeds, the GPU's NUMA node split into 8 DISJOINT CPU slices (hostbind),
    a whole-job value = all ranks' frames / slowest rank."""
    import json
    env = dict(os.environ)
    env['HSA_ENABLE_IPC_MODE_LEGACY'] = '0'
    env.pop('GPU_MAX_HW_QUEUES', None)          # bench.py's own queue budget is asserted below, not the caller's setting
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '8', '--backend', 'gloo', '--share-device',
                        '--steps', '2', '--warmup', '1', '--frames', '8', '--no-cpu-baseline', '--no-other-configs', '--also-360'],
                       capture_output=True, text=True, timeout=1200, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d['n_gpus'] == 8 and d['ranks'] == 8 and d['backend'] == 'gloo' and d['share_device'] is True
    assert d['clip_seeds'] == list(range(8)) and d['per_rank_device'] == [0] * 8
    assert len(d['per_rank_seconds']) == 8 and all(s > 0 for s in d['per_rank_seconds'])
    assert abs(d['value'] - 8 * 8 * 2 / max(d['per_rank_seconds'])) < 1e-2 * d['value']
    assert d['scaling'] == 'weak' and 'x 8 GPUs = configs[3]' in d['config']['workload']
    # round 6: physical identity per rank (PCI bus id / UUID, not the launcher's index), what the backend saw, and the
    # 360x480 configuration measured on all ranks
    assert d['ranks_seen_by_backend'] == 8 and len(d['per_rank_pci_bus_id']) == 8 and len(set(d['per_rank_pci_bus_id'])) == 1
    assert d['distinct_physical_devices'] == 1 and d['ranks_sharing_a_device'] == [list(range(8))]
    assert len(d['per_rank_device_uuid']) == 8 and len(set(d['per_rank_hostname'])) == 1
    a = d['also_360']
    assert a['n_gpus'] == 8 and len(a['per_rank_seconds']) == 8 and abs(a['value'] - 8 * 640 / max(a['per_rank_seconds'])) < 1e-2 * a['value']
    assert d['host']['GPU_MAX_HW_QUEUES'] == '16'                       # every rank's runtime has its own 16 hardware queues
    ranges = d['per_rank_cpu_range']
    if all(a >= 0 for a, _ in ranges):                                   # (hosts without NUMA information bind nothing: -1)
        assert len(set(d['per_rank_numa_node'])) == 1                   # one device -> one node ...
        spans = sorted(ranges)
        assert all(spans[i][1] < spans[i + 1][0] for i in range(7)), ranges      # ... split into disjoint CPU slices
        assert all(c >= 1 for c in d['per_rank_cpus_bound'])
    print('\n[8 ranks on one GPU] %.1f frames/s aggregate, per-rank seconds %s, cpu slices %s' % (d['value'], d['per_rank_seconds'], ranges))
    # the same launch WITHOUT --share-device: two ranks on one physical device are refused (no line, non-zero exit)
    r2 = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--backend', 'gloo', '--steps', '1', '--warmup', '0',
                         '--frames', '8', '--no-cpu-baseline', '--no-other-configs'], capture_output=True, text=True, timeout=900,
                        env=dict(env, HIP_VISIBLE_DEVICES='0,0'), cwd=ROOT)
    assert r2.returncode != 0 and not [l for l in r2.stdout.splitlines() if l.startswith('{')], r2.stdout[-1000:]


@pytest.mark.parametrize('shape', [(4, 23, 30, 256, 256, True, True), (2, 33, 31, 32, 64, True, False), (1, 16, 29, 16, 128, False, True),
                                   (3, 17, 5, 64, 64, True, True), (2, 47, 24, 48, 192, False, False)])
def test_conv_wino43_narrow_map_geometry_against_fp64(dev, shape):
    """The F(4x4,3x3) kernel's second block geometry (16 x 32 output pixels, maps up to 31 columns wide: layer3's 23 x 30, round 5)
    against fp64 -- one / two / three row blocks, rows ending inside a tile and inside a block, every width class up to the limit 31,
    one and several K chunks, residual / ReLU / channel-padded destination (the checks of test_conv_wino43_against_fp64)."""
    from test_gpu_round4 import test_conv_wino43_against_fp64 as check
    check(dev, shape)


# ------------------------------------------------------------------ streaming form of the three-view script
def test_three_view_streaming_matches_offline(dev, hip_nets):
    """`ThreeViewOnlineStitcher` (two pair chains with sliding windows + per-frame composition and three-image render on fixed boxes;
    test_online_tra_threeview.py:154-505 frame by frame) reproduces the offline three-view clip when it is given the offline boxes
    (the composition's first canvas and the output canvas), for both fusion modes; the captured graph equals the eager step bit for
    bit; with its own boxes it yields one finite frame per pushed triple and reports no overflow."""
    from stabstitch2_amd import pipeline, ops
    from stabstitch2_amd.online import ThreeViewOnlineStitcher
    n, h, w = 12, 180, 320
    hr, lr = synth.make_clip(n, h, w, seed=4, views=3)
    hrd = [[f.to(dev) for f in v] for v in hr]
    lrd = [[f.to(dev) for f in v] for v in lr]
    a12 = pipeline.estimate_meshes(hip_nets, lrd[0], lrd[1])
    a23 = pipeline.estimate_meshes(hip_nets, lrd[1], lrd[2])
    a1, a2, b1, b2, _ = ops.three_view_align(a12['smooth_mesh1'], a12['smooth_mesh2'], a23['smooth_mesh1'], a23['smooth_mesh2'], h, w)
    first = ops.mesh_bbox([a1, a2, b1, b2], 0.0, 0.0)
    meshes = pipeline.three_view_compose(a12['smooth_mesh1'], a12['smooth_mesh2'], a23['smooth_mesh1'], a23['smooth_mesh2'], h, w)
    bbox = pipeline.canvas_bbox(meshes, h, w, prescaled=True)
    for fusion in ('AVERAGE', 'LINEAR'):
        off, hc, wc = pipeline.three_view_render(hrd[0], hrd[1], hrd[2], *meshes, 'NORMAL', fusion)
        outs = {}
        for use_graph in (True, False):
            st = ThreeViewOnlineStitcher(hip_nets, h, w, canvas=bbox.cpu().tolist(), first_canvas=first.cpu().tolist(),
                                         fusion_mode=fusion, use_graph=use_graph)
            frames, counts = [], []
            for t in range(n):
                got = st.push(hrd[0][t], hrd[1][t], hrd[2][t], lrd[0][t], lrd[1][t], lrd[2][t])
                counts.append(len(got))
                frames += got
            assert counts == [0] * 6 + [7] + [1] * (n - 7) and (st.hc, st.wc) == (hc, wc)
            outs[use_graph] = torch.stack(frames, 0)
            assert st.overflow_report()['frames_seen'] == n
        assert torch.equal(outs[True], outs[False])                      # graph replay == eager
        d = (outs[True] - off).abs()
        med, q99 = float(d.median()), float(torch.quantile(d.flatten()[::13], 0.99))
        print('\n[3-view streaming vs offline, %s] median %.2e, p99 %.2e, max %.2e' % (fusion, med, q99, float(d.max())))
        # same arithmetic per frame; batch-1 launches sum in another order than the clip's (meshes ~1e-5 px apart), and the reference's
        # chained AVERAGE a*a/(a+b+1e-6) is singular on the clamped sampler's residues: quantiles, not the maximum
        assert med < 1e-3 and q99 < 0.05, (fusion, med, q99)             # observed 6e-5 / 8e-4 (AVERAGE), 2e-4 / 5e-3 (LINEAR)
    own = ThreeViewOnlineStitcher(hip_nets, h, w)
    got = []
    for t in range(9):
        got += own.push(hrd[0][t], hrd[1][t], hrd[2][t], lrd[0][t], lrd[1][t], lrd[2][t])
    assert len(got) == 9 and all(bool(torch.isfinite(f).all()) for f in got) and own.hc >= hc and own.wc >= wc
    assert own.clipped_frames == 0 and own.overflow_report()['frames_seen'] == 9

