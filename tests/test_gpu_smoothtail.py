"""SmoothNet's clip-only Conv3d stack on the GPU (libstabstitch_smoothtail.so): each ragged layer against the float64
statement of the full windows, the layers and the decoder against the conv engine's full computation bit for bit, and
pipeline.smooth_stage with the path against the stage without it.  Surface, resources and refusals: tests/test_smoothtail_abi.py.
    python -m pytest tests/test_gpu_smoothtail.py -m gpu"""
import numpy as np
import pytest
import torch

import ref64 as R
from stabstitch2_amd import synth

pytestmark = pytest.mark.gpu

PAIRS = ((0, 2), (2, 4), (4, 6))                  # (first_in, first_out) of the three layers
PAD = (2, 1, 1)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def hip_nets(dev):
    from stabstitch2_amd.spatial_network import SpatialNet
    from stabstitch2_amd.temporal_network import TemporalNet
    from stabstitch2_amd.smooth_network import SmoothNet
    nets = []
    for cls in (SpatialNet, TemporalNet, SmoothNet):
        m = cls()
        m.load_state_dict(synth.synthetic_state_dict(m), strict=True)
        nets.append(m.to(dev))
    return nets


@pytest.fixture(scope='module')
def motions(dev, hip_nets):
    """The motions of one 32-frame clip of three views, pairs (1,2) and (2,3): computed once, never changed."""
    from stabstitch2_amd import pipeline
    _, lr = synth.make_clip_device(32, 360, 480, seed=3, views=3, device=dev)
    out = []
    for a, b in ((0, 1), (1, 2)):
        acc = pipeline.estimate_meshes(hip_nets, lr[a], lr[b])
        out.append(tuple(acc[k].clone() for k in ('smotion1', 'smotion2', 'tmotion1', 'tmotion2')))
    return out


def _weights(seed, dev):
    """Three packed Conv3d layers [cout][kt][kh][kw][cin] + biases and a decoder: zero-mean weights of a scale that keeps the
    activations' magnitude from layer to layer (K = 5760 products, half the inputs cut by the ReLU before), biases of both signs."""
    rs = np.random.RandomState(seed)
    convs = [(torch.from_numpy((rs.standard_normal((128, 5, 3, 3, 128)) * (2.0 / 5760) ** 0.5).astype(np.float32)).to(dev),
              torch.from_numpy((rs.standard_normal(128) * 0.3).astype(np.float32)).to(dev)) for _ in range(3)]
    dec = (torch.from_numpy((rs.standard_normal((4, 128)) * 0.1).astype(np.float32)).to(dev),
           torch.from_numpy(rs.standard_normal(4).astype(np.float32)).to(dev))
    return convs, dec


def _frames(nw, first):
    """(window, frame) of every compact frame, in order."""
    return [(0, f) for f in range(7)] + [(k, f) for k in range(1, nw) for f in range(first, 7)]


def _expand(compact, nw, first, fill=0.0):
    """compact [frames,63,128] -> full [nw,7,63,128]; the frames a later window lacks hold `fill`."""
    full = torch.full((nw, 7, 63, compact.shape[-1]), fill, device=compact.device, dtype=compact.dtype)
    idx = torch.tensor(_frames(nw, first), device=compact.device)
    full[idx[:, 0], idx[:, 1]] = compact
    return full


def _select(full, nw, first):
    idx = torch.tensor(_frames(nw, first), device=full.device)
    return full[idx[:, 0], idx[:, 1]].contiguous()


# ------------------------------------------------------------------------------------------------ each layer against float64
@pytest.mark.parametrize('with_bias', [True, False], ids=['bias', 'nobias'])
@pytest.mark.parametrize('nw', [1, 2, 3, 26])
def test_each_ragged_layer_against_float64(dev, nw, with_bias):
    """ref64.conv_bound on the FULL windows (the layer's fp32 GPU input put back into [nw,128,7,7,9]; the frames a later window does
    not hold are zeros, and no needed output reads them), the needed frames selected.  Every layer is fed the previous GPU layer's
    output, so the bound -- dot_bound of the real products, any summation order -- stays per layer.  nw = 1: no later window;
    nw = 2: 12 / 10 / 8 tiles of 63 rows, 756 rows in layer 1; nw = 1, 2, 3 and 26 take K cuts of 5, 10, 14 and 90 tiles."""
    from stabstitch2_amd import ops
    convs, _ = _weights(11 + nw, dev)
    x = torch.from_numpy(np.random.RandomState(nw).standard_normal((nw * 7, 63, 128)).astype(np.float32)).to(dev)
    for (w, b), (first_in, first_out) in zip(convs, PAIRS):
        b = b if with_bias else None
        got = ops.smooth_tail_layer(x, w, b, nw, first_in, first_out)
        assert tuple(got.shape) == (7 + (nw - 1) * (7 - first_out), 63, 128)
        full = _expand(x, nw, first_in).view(nw, 7, 7, 9, 128).permute(0, 4, 1, 2, 3)          # [nw,c,t,h,w]
        val, bound = R.conv_bound(R.f32(full), R.f32(w.permute(0, 4, 1, 2, 3)), None if b is None else R.f32(b), pad=PAD, relu=True)
        sel = torch.tensor(_frames(nw, first_out))
        want = val.transpose(0, 2, 3, 4, 1).reshape(nw, 7, 63, 128)[sel[:, 0], sel[:, 1]]      # [frames,63,128]
        lim = bound.transpose(0, 2, 3, 4, 1).reshape(nw, 7, 63, 128)[sel[:, 0], sel[:, 1]]
        g = R.f64(got)
        assert np.isfinite(g).all()
        excess = np.abs(g - want) - lim
        assert excess.max() <= 0, ('layer', first_in, first_out, float(excess.max()), float(np.abs(g - want).max()))
        cut = float((g == 0).mean())
        assert 0.2 < cut < 0.8, cut                                      # the ReLU cuts both ways
        x = got


# ------------------------------------------------------------------------------------------------ against the conv engine, bit for bit
@pytest.mark.parametrize('nw', [1, 2, 3, 26, 34, 40])
def test_layers_and_decoder_equal_the_full_windows_bit_for_bit(dev, nw):
    """The three layers on all 7 frames of every window (ops.conv: conv_igemm_kernel and its split-K reduction) and ops.linear
    behind them, against the ragged layers and the scattering decoder: equal where the ragged path computes, untouched elsewhere.
    nw = 34: the clip of test_gpu_round3.test_smooth_stitch_vs_torch; nw = 40: no K cut."""
    from stabstitch2_amd import ops
    convs, dec = _weights(5, dev)
    x = torch.from_numpy(np.random.RandomState(100 + nw).standard_normal((nw, 7, 7, 9, 128)).astype(np.float32)).to(dev)
    full = x
    for w, b in convs:
        full = ops.conv(full, w, b, stride=1, pad=PAD, relu=True)
    want = ops.linear(full.view(-1, 128), dec[0], dec[1]).view(nw, 7, 63, 4)
    hid = x.view(nw * 7, 63, 128)
    for (w, b), (first_in, first_out) in zip(convs, PAIRS):
        hid = ops.smooth_tail_layer(hid, w, b, nw, first_in, first_out)
    assert torch.equal(hid, _select(full.view(nw, 7, 63, 128), nw, 6))
    delta = torch.full((nw, 7, 63, 4), float('nan'), device=dev)
    ops.smooth_tail_decode(hid, dec[0], dec[1], delta, nw)
    read = torch.zeros((nw, 7), dtype=torch.bool, device=dev)
    read[0] = True
    read[:, 6] = True
    assert torch.equal(delta[read], want[read])
    assert bool(torch.isnan(delta[~read]).all())                         # entries nobody reads stay unwritten
    # two runs, the same bits
    again = ops.smooth_tail_deltas(x, convs, dec, nw)
    assert torch.equal(again.view(nw, 7, 63, 4)[read], delta[read])


# ------------------------------------------------------------------------------------------------ the stage
def _nan_empty(monkeypatch):
    """Every fp32 torch.empty on a device comes back full of NaN: whatever a kernel reads without anybody having written it shows."""
    real = torch.empty

    def empty(*args, **kw):
        t = real(*args, **kw)
        if t.is_cuda and t.dtype == torch.float32:
            t.fill_(float('nan'))
        return t
    monkeypatch.setattr(torch, 'empty', empty)


@pytest.mark.parametrize('n', [7, 9, 32])
def test_smooth_stage_equals_the_stage_without_the_path(dev, hip_nets, motions, monkeypatch, n):
    """pipeline.smooth_stage on the first n frames of a clip's motions (n = 7: one window; 9: three; 32: the benchmark's 26), delta and
    every other allocation pre-filled with NaN: finite, within 2e-4 px of the stage on the conv engine (SS_SMOOTH_TAIL=0) -- the gate
    of two kernel choices of one computation -- and, since the sums are formed in the same order, equal."""
    from stabstitch2_amd import ops, pipeline
    s1, s2, t1, t2 = [m[:n].contiguous() for m in motions[0]]
    monkeypatch.setattr(ops, 'SMOOTH_TAIL', False)
    want = pipeline.smooth_stage(hip_nets[2], s1, s2, t1, t2)
    monkeypatch.setattr(ops, 'SMOOTH_TAIL', True)
    _nan_empty(monkeypatch)
    got = pipeline.smooth_stage(hip_nets[2], s1, s2, t1, t2)
    monkeypatch.undo()
    for k in ('ori_mesh1', 'ori_mesh2', 'smooth_mesh1', 'smooth_mesh2', 'ori_path2', 'smooth_path2'):
        assert tuple(got[k].shape) == (1, n, 7, 9, 2)
        assert bool(torch.isfinite(got[k]).all()), k
        err = float((got[k] - want[k]).abs().max())
        assert err <= 2e-4, (k, err)
        assert torch.equal(got[k], want[k]), k


def test_three_view_clip_equals_the_clip_without_the_path(dev, hip_nets, monkeypatch):
    """pipeline.run_three_view, 9 frames: both pairs' SmoothNet stages take the path; meshes within 2e-4 px (equal), frames equal."""
    from stabstitch2_amd import ops, pipeline
    hr, lr = synth.make_clip_device(9, 360, 480, seed=2, views=3, device=dev)
    monkeypatch.setattr(ops, 'SMOOTH_TAIL', False)
    want = pipeline.run_three_view(hr[0], hr[1], hr[2], lr[0], lr[1], lr[2], hip_nets)
    monkeypatch.setattr(ops, 'SMOOTH_TAIL', True)
    calls = []
    real = ops.smooth_tail_deltas
    monkeypatch.setattr(ops, 'smooth_tail_deltas', lambda *a, **k: calls.append(a[3]) or real(*a, **k))
    got = pipeline.run_three_view(hr[0], hr[1], hr[2], lr[0], lr[1], lr[2], hip_nets)
    assert calls == [3, 3]
    assert (got[1], got[2]) == (want[1], want[2])
    for g, w, name in zip(got[3:], want[3:], ('mesh1', 'middle', 'mesh3')):
        assert bool(torch.isfinite(g).all()), name
        assert float((g - w).abs().max()) <= 2e-4, name
        assert torch.equal(g, w), name
    assert torch.equal(got[0], want[0])


def test_the_deterministic_policy_keeps_the_conv_engine(dev, hip_nets, motions, monkeypatch):
    """deterministic=True promises clip == stream bit for bit and the stream keeps the conv engine: nothing of the library is launched."""
    from stabstitch2_amd import _smoothtail, ops, pipeline
    launched = []
    real = _smoothtail.call
    monkeypatch.setattr(_smoothtail, 'call', lambda name, *a: launched.append(name) or real(name, *a))
    monkeypatch.setattr(ops, 'SMOOTH_TAIL', True)
    s1, s2, t1, t2 = [m[:9].contiguous() for m in motions[1]]
    with ops.deterministic():
        det = pipeline.smooth_stage(hip_nets[2], s1, s2, t1, t2)
    assert launched == []
    plain = pipeline.smooth_stage(hip_nets[2], s1, s2, t1, t2)
    assert launched == ['sst_conv3d_layer'] * 3 + ['sst_decode_scatter']
    assert float((det['smooth_mesh2'] - plain['smooth_mesh2']).abs().max()) <= 2e-4
