"""The float64 references of tests/ref64.py, pinned on the CPU: each against the golden fixture of its operation (G2 - G7, G11)
and against the fp32 oracle on the inputs that tests/test_gpu_kernel_sweeps.py feeds the kernels, so that a wrong reference
cannot make a wrong kernel pass.  For every fixed (not derived) gate of the sweep the fp32 ORACLE has to pass that gate against
ref64 on the sweep's inputs with a factor 2 to spare: that is what shows an input class to be usable.

    python -m pytest tests/test_ref64.py            (no GPU needed)"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cases
import ref64 as R
import sweep_inputs as G
from oracle import samplers as S, nets as N, metrics as M, pipeline as P

torch.set_grad_enabled(False)
T = torch.from_numpy


def maxerr(a, b, what=''):
    a, b = R.f64(a), R.f64(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    e = float(np.abs(a - b).max()) if a.size else 0.0
    if os.environ.get('SS_VERBOSE'):
        print('  [ref64] %-50s max|diff| %.3e' % (what, e))
    return e


# ------------------------------------------------------------------------------------------------ cost volume
def test_cost_volume_golden(golden):
    g = golden('g3_costvol')
    a, b = cases.g3_inputs(False)
    for r, key in ((5, 'cv5'), (3, 'cv3')):
        cv, s = R.cost_volume(a, b, r)
        assert (np.abs(cv - g[key]) <= R.dot_bound(16, s)).all(), key
    fa, fb = cases.g3_inputs(True)
    cv, s = R.cost_volume(fa, fb, 5)
    assert (np.abs(cv[0, :, 22, :] - g['full5_rows']) <= R.dot_bound(128, s[0, :, 22, :])).all()


@pytest.mark.parametrize('n,c,h,w,r', [(1, 4, 2, 3, 5), (2, 12, 5, 17, 3), (1, 20, 9, 16, 5), (1, 36, 23, 31, 3), (1, 128, 45, 60, 5)])
def test_cost_volume_oracle_inside_derived_bound(n, c, h, w, r):
    """The fp32 oracle (a torch sum in its own order) against ref64 under the derived dot-product bound, and with room."""
    a, b = G.cv_inputs(n, c, h, w)
    cv, s = R.cost_volume(a, b, r)
    o = N.cost_volume(T(a), T(b), r).numpy()
    bound = R.dot_bound(c, s)
    ratio = float((np.abs(o - cv) / np.maximum(bound, 1e-300)).max())
    assert ratio <= 0.5, ratio          # observed 0.05 .. 0.16
    # a wrong displacement or a dropped channel is far outside it: the bound is ~1e-6 of S
    moved = np.roll(cv, 1, axis=1)
    live = (cv != 0) | (moved != 0)
    assert float((np.abs(moved - cv) > bound)[live].mean()) > 0.99


# ------------------------------------------------------------------------------------------------ CCL, L2 norm
def test_ccl_golden(golden):
    g = golden('g4_ccl')
    for full, key in ((False, 'flow'), (True, 'flow_full')):
        a, b = cases.g4_inputs(full)
        assert maxerr(R.ccl(a, b), g[key], 'ccl ' + key) < 1e-4        # observed 2e-6 / 1.4e-5: the fixture's own fp32 error


CCL_SHAPES = [(1, 1), (1, 7), (7, 1), (5, 7), (16, 16), (1, 257), (17, 15), (23, 30), (24, 32)]


@pytest.mark.parametrize('h,w', CCL_SHAPES)
@pytest.mark.parametrize('c', [4, 32, 68, 256])
def test_ccl_oracle_on_sweep_inputs(h, w, c):
    """oracle.nets.ccl (fp32 unfold + conv + softmax) against ref64 on the sweep's chain inputs.  The sweep's gate is
    max(1e-4, 4 e_oracle) with e_oracle measured per case, so nothing fixed is to be proven here; this pins the reference
    (an independent formulation: patches correlated as nine shifted Gram products) and records e_oracle."""
    x = G.ccl_chain(2, c, h, w)
    for scale in (10.0, 1.0):
        e = maxerr(N.ccl(T(x[0:1]), T(x[1:2]), scale), R.ccl(x[0:1], x[1:2], scale), 'ccl %dx%dx%d scale %g' % (h, w, c, scale))
        assert e < 5e-4, e          # observed <= 1.7e-4 (c = 4 on 24 x 32 and 1 x 257), 1.4e-5 at 23 x 30 x 256


def test_ccl_zero_vector_and_l2norm():
    x = G.ccl_chain(2, 32, 5, 7)
    x[0, :, 2, 3] = 0.0
    ref = R.ccl(x[0:1], x[1:2])
    assert np.isfinite(ref).all() and maxerr(N.ccl(T(x[0:1]), T(x[1:2])), ref, 'ccl zero vector') < 1e-4
    for c in (1, 63, 64, 65, 256):
        v = np.random.RandomState(c).normal(0, 1, (13, c)).astype(np.float32)
        v[5] = 0.0
        ref = R.l2norm(v, 1)
        assert (np.abs(F.normalize(T(v), p=2, dim=1).numpy() - ref) <= R.dot_bound(c, np.abs(ref))).all()
        assert (ref[5] == 0).all()


# ------------------------------------------------------------------------------------------------ homography
def test_homography_golden(golden):
    g = golden('g2_homo')
    U, th = cases.g2_inputs()
    for size, key in (((45, 60), 'out'), ((23, 31), 'out_small')):
        xn, yn, _ = R.homography_coords(th, *size)
        # 1e-4 as test_homography_sampler; the fixture is fp32: a coordinate 1e-6 px outside the image in fp64 is on the border in
        # fp32, where the clamped sampler jumps (sampler_slack under 1e-5 px)
        ref, slack = G.sampler_slack(R.bilinear_clamped, U, xn, yn, 1e-5 * 2 / 60, 1e-5 * 2 / 45)
        assert (np.abs(ref - g[key]) <= 1e-4 + slack).all(), key
        assert float((slack > 1e-4).mean()) < 0.05           # the identity's border rows and columns


@pytest.mark.parametrize('size', [(2, 2), (23, 31), (45, 60), (90, 121)])
def test_homography_oracle_on_sweep_inputs(size):
    """oracle.samplers.homography_warp against ref64 on the sweep's thetas.  e_oracle is what the sweep's tolerance is a multiple
    of (4 x); here it is recorded, held to a sane size, and the oracle is shown to meet the kernels' value gate itself."""
    oh, ow = size
    U = G.homo_input(1, 8)
    for name, th in G.homo_thetas(oh).items():
        e, o, taps_in = G.homo_oracle_error(U, th[None], oh, ow)
        if os.environ.get('SS_VERBOSE'):
            print('  [ref64] homography %-9s %-9s e_oracle %.2e px, %.0f %% of the pixels with all taps inside' % (name, size, e, 100 * taps_in.mean()))
        if name in ('identity', 'g2_mild', 'zero_row', 'under', 'over') and oh > 2:
            assert taps_in.mean() > 0.2, (name, taps_in.mean())
        assert e < 1e-4, (name, e)                          # px on a 60-pixel map; observed <= 3e-5
        ref, bound = G.homo_gate(U, th[None], oh, ow, e)
        assert (np.abs(o - ref) <= bound).all(), (name, float((np.abs(o - ref) - bound).max()))


def test_homography_zero_row_is_exact():
    """the `zero_row` theta's denominator is exactly 0 on the first row and the guard moves it to 1e-6 there (in fp64 and in the oracle)"""
    for oh in (23, 45, 90):
        th = G.homo_thetas(oh)['zero_row'][None]
        _, _, ts = R.homography_coords(th, oh, 31)
        assert (ts[0, 0] == 0).all() and (np.abs(ts[0, 1:]) > 1.0 / oh).all()
        gy = torch.linspace(-1, 1, oh)
        assert bool((gy * th[0, 2, 1] + th[0, 2, 2])[0] == 0)


# ------------------------------------------------------------------------------------------------ TPS
def test_tps_points_golden(golden):
    g = golden('g5_tps_points')
    nrigid, warped, query = cases.g5_meshes()
    assert maxerr(R.tps_points(query, nrigid, warped), g['p_a'], 'tps points a') < 1e-5
    assert maxerr(R.tps_points(query, warped, nrigid), g['p_b'], 'tps points b') < 1e-5
    assert maxerr(R.tps_points(warped, warped, nrigid), nrigid, 'interpolation') < 1e-5


@pytest.mark.parametrize('h,w', [(360, 480), (720, 1280)])
@pytest.mark.parametrize('n', [1, 7, 300])
def test_tps_oracle_on_sweep_inputs(n, h, w):
    """Gate 2e-5 normalised (points and the action of T): the fp32 oracle inside 1e-5 of ref64 on the sweep's meshes."""
    rigid, warped = G.tps_meshes(n, h, w)
    for src, tgt in ((rigid, warped), (warped, rigid)):
        T64 = R.tps_solve(src, tgt)
        assert maxerr(R.tps_action(S.tps_solve(T(src), T(tgt)), src), R.tps_action(T64, src), 'T action n=%d' % n) <= 1e-5
        q = G.tps_queries(n, 1000)
        assert maxerr(S.tps_points(T(q), T(src), T(tgt)), R.tps_points(q, src, tgt), 'points n=%d q=1000' % n) <= 1e-5   # observed <= 9.5e-6


def test_tsmotion_golden_and_oracle(golden):
    g8 = golden('g8_nets')
    sm, tm = g8['motion1'], g8['tmotion1']
    smesh, ts = R.tsmotion(sm, tm)
    assert maxerr(ts, g8['tsmotion1'], 'tsmotion vs reference') < 1e-3         # gate of the sweep 2e-3 px
    osm, ots = P.tsmotion_prepare([T(sm[i:i + 1]) for i in range(len(sm))], [T(tm[i:i + 1]) for i in range(len(tm))])
    assert maxerr(torch.cat(ots), ts, 'tsmotion oracle') < 1e-3 and maxerr(torch.cat(osm), smesh, 'smesh') < 1e-4
    sm, tm = G.tsm_inputs(40)                      # the sweep's synthetic motions: gate 2e-3 px, the oracle inside 1e-3
    _, ts = R.tsmotion(sm, tm)
    _, ots = P.tsmotion_prepare([T(sm[i:i + 1]) for i in range(len(sm))], [T(tm[i:i + 1]) for i in range(len(tm))])
    assert maxerr(torch.cat(ots), ts, 'tsmotion oracle, synthetic') < 1e-3
    sm3, tm3 = G.tsm_inputs(300)                   # n = 300 and lag 3: three interleaved streams, each through the oracle's loop
    _, ts3 = R.tsmotion(sm3, tm3, lag=3)
    for st in range(3):
        _, o3 = P.tsmotion_prepare([T(sm3[i:i + 1]) for i in range(st, 300, 3)], [T(tm3[i:i + 1]) for i in range(st, 300, 3)])
        assert maxerr(torch.cat(o3), ts3[st::3], 'tsmotion oracle n=300 lag 3 stream %d' % st) < 1e-3
    for lag in (2, 3):
        _, tl = R.tsmotion(sm, tm, lag=lag)
        assert (tl[:lag] == 0).all()
        for s in range(lag):                    # `lag` interleaved streams = `lag` independent lag-1 problems
            _, t1 = R.tsmotion(sm[s::lag], tm[s::lag])
            assert maxerr(tl[s::lag], t1, 'lag %d' % lag) < 1e-12


# ------------------------------------------------------------------------------------------------ dense warp
def test_tps_warp_golden(golden):
    g = golden('g6_tps_warp')
    U, src, tgt, size, ident = cases.g6_inputs()
    xn, yn = R.tps_dense_coords(src, R.tps_solve(src, tgt), *size)
    wn = R.bilinear_clamped(U, xn, yn)
    assert maxerr(wn[:, 3:5], g['normal'][:, 3:5], 'coords NORMAL (px)') < 2.5e-3
    assert maxerr(wn[:, 0:3], g['normal'][:, 0:3], 'intensity NORMAL') < 2e-3
    wf = R.grid_sample_zeros(U, xn, yn)
    assert (np.abs(wf - g['fast']) <= 2e-3 + 5e-3 * G.grad4(g['fast'])).all()


WARP_CASES = [(1, 2, 2, 8, 64), (3, 72, 96, 80, 120), (1, 251, 377, 300, 520), (1, 72, 96, 81, 129), (1, 72, 96, 85, 191),
              (1, 72, 96, 84, 128), (1, 72, 96, 87, 65)]


@pytest.mark.parametrize('b,h,w,hc,wc', WARP_CASES + [(1, 720, 1280, 780, 1900)])
def test_tps_warp_oracle_on_sweep_inputs(b, h, w, hc, wc):
    """Gate 5.2e-5 of the half extent on the sampling coordinate: the fp32 oracle (solve + evaluation) inside 2.6e-5 of ref64 on
    the sweep's meshes (sigma 12 px at 720p + a shift).  The largest canvas is sampled (every 7th row) to keep this on the CPU."""
    U, src, tgt = G.warp_case(b, h, w, hc, wc)
    xn, yn = R.tps_dense_coords(src, R.tps_solve(src, tgt), hc, wc)
    ox, oy = S.tps_dense_coords(T(src), T(tgt), hc, wc)
    step = 7 if hc > 400 else 1
    e = max(maxerr(ox.reshape(b, hc, wc)[:, ::step], xn[:, ::step], 'dense x %s' % ((h, w, hc, wc),)),
            maxerr(oy.reshape(b, hc, wc)[:, ::step], yn[:, ::step], 'dense y'))
    assert e <= 2.6e-5, e                               # observed 0.5 - 1.1e-5


@pytest.mark.parametrize('mode', ['NORMAL', 'FAST'])
@pytest.mark.parametrize('b,h,w,hc,wc', WARP_CASES + [(1, 720, 1280, 780, 1900)])
def test_tps_warp_oracle_meets_the_value_gate(b, h, w, hc, wc, mode):
    """The dense-warp VALUE gate (sweep_inputs.warp_gate: close_grad(base 2e-3, the coordinate tolerance) + the samplers' border slack +
    the clamped sampler's residue outside the frame) on the sweep's inputs: oracle.samplers.tps_warp in fp32, every plane and
    pixel, inside that gate built with HALF of every term (spare = 2); its ramp planes inside half of the coordinate gate."""
    U, src, tgt = G.warp_case(b, h, w, hc, wc)
    xn, yn = R.tps_dense_coords(src, R.tps_solve(src, tgt), hc, wc)
    o = S.tps_warp(T(U), T(src), T(tgt), (hc, wc), mode).numpy().astype(np.float64)
    ref, bound, x, y, inside = G.warp_gate(U, xn, yn, mode, spare=2.0)
    excess = np.abs(o - ref) - bound
    assert (excess <= 0).all(), (float(excess.max()), int((excess > 0).sum()), np.unravel_index(int(np.argmax(excess)), excess.shape))
    if inside.any():
        ex, ey = ((w, h) if mode == 'NORMAL' else (w - 1, h - 1))
        assert maxerr(o[:, 3][inside], x[inside], 'oracle x ramp %s' % mode) <= 0.5 * G.WARP_COORD_GATE * ex / 2
        assert maxerr(o[:, 4][inside], y[inside], 'oracle y ramp %s' % mode) <= 0.5 * G.WARP_COORD_GATE * ey / 2
    # the gate is not vacuous outside the frame: there the reference is 0 and the bound stays far below a grey level
    if mode == 'NORMAL' and h >= 72:
        far = ~inside
        assert float(np.median(bound[:, :3][np.broadcast_to(far[:, None], bound[:, :3].shape)])) < 0.5


# ------------------------------------------------------------------------------------------------ metrics
def test_psnr_ssim_golden(golden):
    g = golden('g11_metrics')
    a, b = cases.g11_images()
    one = np.ones((1, 36, 48), np.float32)
    p, s = R.psnr_ssim(np.concatenate((a.transpose(2, 0, 1), one)), np.concatenate((b.transpose(2, 0, 1), one)))
    assert abs(p - float(g['psnr'])) < 1e-6 and abs(s - float(g['ssim'])) < 1e-6


@pytest.mark.parametrize('h,w', [(7, 7), (36, 48), (9, 65), (65, 9), (130, 131), (360, 480)])
@pytest.mark.parametrize('mask', ['ones', 'binary', 'frac'])
def test_psnr_ssim_oracle_on_sweep_inputs(h, w, mask):
    """Gate 1e-6 on PSNR (dB) and SSIM: oracle.metrics (scipy's uniform_filter, fp64) inside 5e-7 of ref64's window sums."""
    w1, w2 = G.metric_planes(2, h, w, mask)
    if mask == 'frac':
        assert ((w1[:, 3] > 0) & (w1[:, 3] < 1)).any() or min(h, w) < 10
    for f in range(2):
        def six(x):
            return np.concatenate((x[f, 0:3], np.repeat(x[f, 3:4], 3, 0))).transpose(1, 2, 0)
        po, so = M.alignment_psnr_ssim(six(w1), six(w2))
        pr, sr = R.psnr_ssim(w1[f], w2[f])
        assert abs(po - pr) < 5e-7 and abs(so - sr) < 5e-7, (po - pr, so - sr)


def test_stability_distortion_oracle_on_sweep_inputs():
    """Gates 1e-4 (stability) and 1e-5 (distortion), those of test_pipeline_vs_reference: the fp32 oracle inside half of them."""
    for t in (7, 8, 50):
        p = G.metric_paths(t)
        assert abs(M.stability_score(T(p).view(1, t, 7, 9, 2)) - R.stability_score(p)) < 5e-5
    for t in (1, 64, 65, 200):
        m = G.metric_meshes(t)
        ref = R.distortion_score(m)
        assert ref > 0.5                                   # the stretched cells are counted
        assert abs(M.distortion_score(T(m).view(1, t, 7, 9, 2)) - ref) < 5e-6


# ------------------------------------------------------------------------------------------------ convolution
CONV_RAGGED = [                    # (n, cin, cout, (t,) h, w, k, stride, pad)
    (2, 5, 7, None, 9, 11, (3, 3), 2, (1, 2)), (1, 4, 3, None, 6, 5, (7, 7), 1, (3, 3)), (2, 3, 4, None, 5, 6, (2, 5), 3, (2, 3)),
    (3, 6, 5, None, 1, 1, (3, 3), 1, (1, 1)), (1, 2, 9, None, 2, 3, (7, 7), 2, (3, 3)), (1, 7, 2, None, 8, 8, (1, 1), 2, (0, 0)),
    (2, 3, 4, 6, 5, 7, (5, 3, 3), 1, (2, 1, 1)), (1, 4, 3, 7, 4, 5, (3, 3, 3), 1, (0, 1, 1)), (1, 2, 3, 5, 6, 6, (5, 5, 5), 2, (2, 0, 3)),
]


@pytest.mark.parametrize('n,cin,cout,t,h,w,k,stride,pad', CONV_RAGGED)
def test_conv_statement_against_torch_fp64(n, cin, cout, t, h, w, k, stride, pad):
    """ref64.conv (value), its S (the same convolution of absolute values) and conv_terms (a convolution of ones) against
    F.conv2d / F.conv3d in float64, with bias, residual and ReLU; pool_max against F.max_pool2d."""
    rs = np.random.RandomState(n + 10 * cin + 100 * h + w)
    x = rs.normal(0, 1, (n, cin, h, w) if t is None else (n, cin, t, h, w))
    wt = rs.normal(0, 1, (cout, cin) + k)
    b = rs.normal(0, 1, cout)
    if t is None:
        f = lambda a, c, bb: F.conv2d(T(a), T(c), None if bb is None else T(bb), stride=stride, padding=pad)
    else:
        f = lambda a, c, bb: F.conv3d(T(a), T(c), None if bb is None else T(bb), stride=(1, stride, stride), padding=pad)
    pre = f(x, wt, b).numpy()
    r = rs.normal(0, 1, pre.shape)
    val, s = R.conv(x, wt, b, r, stride, pad, relu=True)
    assert maxerr(val, np.maximum(pre + r, 0), 'conv') < 1e-12
    assert maxerr(s, f(np.abs(x), np.abs(wt), np.abs(b)).numpy() + np.abs(r), 'S') < 1e-12
    ones = f(np.ones((1,) + x.shape[1:]), np.ones((1,) + wt.shape[1:]), None).numpy()[0, 0]
    assert (R.conv_terms(x.shape, wt.shape, stride, pad) == np.rint(ones)).all()
    v2, bd = R.conv_bound(x, wt, b, r, stride, pad, relu=True)
    assert (v2 == val).all() and (bd == R.dot_bound(np.rint(ones) + 2, s)).all()
    if t is None:
        for (pk, ps, pp) in ((2, 2, 0), (3, 2, 1)):
            if val.shape[2] + 2 * pp >= pk and val.shape[3] + 2 * pp >= pk:
                assert (R.pool_max(val, pk, ps, pp) == F.max_pool2d(T(val), pk, ps, pp).numpy()).all()


def _fold_bn(conv, bn):
    sc = (bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps))
    return (conv.weight.double() * sc.view(-1, 1, 1, 1)).numpy(), (bn.bias.double() - bn.running_mean.double() * sc).numpy()


def test_conv_statement_against_the_oracle_layers():
    """ref64 against the fp32 oracle layers that the goldens pin (oracle/nets.py under the synthetic checkpoint, on G8's frames):
    the stem (conv 7x7/2, BatchNorm folded here in fp64, ReLU, max-pool 3/2/1), the first residual block's conv + BN + ReLU, a
    regressor conv + ReLU + conv + ReLU + MaxPool2d(2, 2), and SmoothNet's first Conv3d.  The oracle is fp32: 1e-5 relative to the
    largest value."""
    from stabstitch2_amd import synth
    sp, sm = N.SpatialNet().eval(), N.SmoothNet().eval()
    for m in (sp, sm):
        m.load_state_dict(synth.synthetic_state_dict(m), strict=True)
    _, lr = synth.make_clip(2, 360, 480, seed=0)
    x = torch.cat([lr[0][0], lr[1][1]])[:, :, 100:193, 200:321].contiguous()                 # 2 frames, a 93 x 121 window
    s1 = sp.feature_extractor_stage1
    w0, b0 = _fold_bn(s1[0], s1[1])
    want = s1[3](s1[2](s1[1](s1[0](x))))
    got, bound = R.stem_pool(x.numpy(), w0, b0)
    assert maxerr(got, want, 'stem + pool') <= 1e-5 * float(want.abs().max())
    blk = s1[4][0]
    w1, b1 = _fold_bn(blk.conv1, blk.bn1)
    want1 = blk.relu(blk.bn1(blk.conv1(want)))
    got1, _ = R.conv(want.numpy(), w1, b1, None, 1, 1, relu=True)
    assert maxerr(got1, want1, 'layer1 conv1') <= 1e-5 * float(want1.abs().max())
    reg = sp.regressNet1_part1
    z = T(G.conv_inputs(2, 2, 2, 45, 60)[0])
    wantp = reg[4](reg[3](reg[2](reg[1](reg[0](z)))))
    mid, _ = R.conv(z.numpy(), reg[0].weight.numpy(), None, None, 1, 1, relu=True)
    gotp, _ = R.conv_pool2(mid, reg[2].weight.numpy(), None, 1, 1, relu=True)
    assert gotp.shape == tuple(wantp.shape) and maxerr(gotp, wantp, 'regressor conv, conv, pool') <= 1e-5 * float(wantp.abs().max())
    c3 = sm.MotionPre.MotionConv3D[0]
    h = T(G.conv_inputs(1, 128, 128, 7, 9, (5, 3, 3), t=7)[0])
    want3 = F.relu(c3(h))
    got3, _ = R.conv(h.numpy(), c3.weight.numpy(), c3.bias.numpy(), None, 1, (2, 1, 1), relu=True)
    assert maxerr(got3, want3, 'conv3d') <= 1e-5 * float(want3.abs().max())


def _ig_operands(c):
    """x, w, bias, res of an implicit-GEMM case in torch's layouts (real channels only), and the conv arguments."""
    to, ho, wo, M, K = G.ig_geometry(c)
    out_hw = (ho, wo) if c['t'] is None else (to, ho, wo)
    return G.conv_inputs(c['n'], c['c_real'], c['cout'], c['h'], c['w'], c['k'], t=c['t'], out_hw=out_hw, bias=c['bias'], res=c['res'])


@pytest.mark.parametrize('c', G.IGEMM_CASES, ids=lambda c: c['name'])
def test_torch_fp32_conv_inside_the_direct_gate(c):
    """fp32 F.conv2d / conv3d (another fp32 sum, in torch's order) meets the direct-convolution gate dot_bound(K_real + 2, S) on every
    sweep input with a factor 2 to spare: the gate is usable, and torch's own error is where the derivation says."""
    x, wt, b, r = _ig_operands(c)
    pad = c['p'] if c['t'] is not None else c['p'][1:]
    ref, bound = R.conv_bound(x, wt, b, r, c['s'], pad, c['relu'])
    if c['t'] is None:
        o = F.conv2d(T(x), T(wt), None if b is None else T(b), stride=c['s'], padding=pad)
    else:
        o = F.conv3d(T(x), T(wt), None if b is None else T(b), stride=(1, c['s'], c['s']), padding=pad)
    if r is not None:
        o = o + T(r)
    o = F.relu(o) if c['relu'] else o
    ratio = float((np.abs(o.numpy() - ref) / bound).max())
    assert ratio <= 0.5, ratio                   # observed <= 0.16


@pytest.mark.parametrize('h,w', G.STEM_SIZES, ids=lambda v: str(v))
def test_torch_fp32_stem_inside_the_direct_gate(h, w):
    """the same for the stem's inputs: conv 7x7/2 + ReLU and the 3/2/1 max-pool of it (bound pooled by max), two filter banks"""
    x, wt, b = G.stem_inputs(5, h, w, 2)
    o = F.relu(F.conv2d(T(x), T(wt), T(b), stride=2, padding=3))
    ref, bound = R.stem(x, wt, b)
    assert float((np.abs(o.numpy() - ref) / bound).max()) <= 0.5
    pref, pbound = R.stem_pool(x, wt, b)
    assert float((np.abs(F.max_pool2d(o, 3, 2, 1).numpy() - pref) / pbound).max()) <= 0.5


def test_implicit_gemm_claims_follow_the_dispatch_rules():
    """Every implicit-GEMM case's claimed path (tile, address mode, TAIL, splits) is what conv.hip's rules, restated in
    sweep_inputs.igemm_plan, give for its shape; and the restated split-K plan is the library's own (ss_conv_workspace_need is
    host code: it answers without a GPU)."""
    from stabstitch2_amd import _hip as H
    for c in G.IGEMM_CASES:
        plan = G.ig_plan(c)
        assert G.ig_claim(plan) == c['claim'], (c['name'], c['claim'], G.ig_claim(plan), plan)
        kt, kh, kw = c['k']
        pt, ph, pw = c['p']
        to, ho, wo, M, K = G.ig_geometry(c)
        need = int(H.lib().ss_conv_workspace_need(c['n'], c['t'] or 1, c['h'], c['w'], c['cin'], c['cout'], kt, kh, kw, c['s'], pt, ph, pw,
                                                  c['groups']))
        sp = G.conv_splits(M, c['cout'], c['groups'], G.cdiv(K, 32))
        assert need == (c['groups'] * sp * M * c['cout'] if sp > 1 else 0), (c['name'], need, sp)
        assert (sp == plan['splits']) == c['ws'] or sp == 1, c['name']
    for case in G.POOL_REDUCE_CASES:
        n, h, w, cin, cout, groups, _ = case
        assert G.conv_splits(n * h * w, cout, groups, G.cdiv(9 * cin, 32)) > 1, case
    for (h, w, cin) in ((7, 16, 64), (16, 7, 64), (45, 60, 128), (23, 30, 256), (11, 15, 128), (5, 7, 128)):          # wino_blocks == the library's rule
        tbh, tbw = G.wino_blocks(h, w)
        wgs = lambda images: images * G.cdiv((h + 1) // 2, tbh) * G.cdiv((w + 1) // 2, tbw)
        eff = h * w / (4.0 * G.cdiv((h + 1) // 2, tbh) * tbh * G.cdiv((w + 1) // 2, tbw) * tbw)
        for images in (1, 95, 96, 191, 192):
            want = (wgs(images) >= 96) if eff >= 0.70 else (eff >= 0.60 and wgs(images) >= 192)
            assert bool(H.lib().ss_conv_uses_winograd(1, 3, 3, 1, cin, 64, h, w, images)) == want, (h, w, images)


def test_reach_table_names_every_conv_kernel_of_the_library():
    """The reach table of the convolution sweep against the gfx950 code objects of the built library: every instantiation of
    conv_igemm_kernel, splitk_reduce_kernel, conv_wino_kernel, conv_wino43* and stem_pool* that the library carries is either named
    by the table (with the cases claimed to launch it) or listed as unreachable from the C ABI with the reason, and the table names
    nothing the library lacks."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    import kernel_resources as KR
    from stabstitch2_amd import _hip as H
    have = {G.kernel_key(k) for k in KR.kernels(H.LIB_PATH)}
    have = {k for k in have if k.startswith(G.CONV_ENGINE_KERNELS)}
    assert len(have) >= 30, sorted(have)
    table = G.reach_table()
    assert not set(table) & set(G.UNREACHABLE)
    missing = sorted(have - set(table) - set(G.UNREACHABLE))
    assert not missing, 'instantiations in the library that no sweep case claims: %s' % missing
    stale = sorted((set(table) | set(G.UNREACHABLE)) - have)
    assert not stale, 'the table names kernels the library does not carry: %s' % stale
    assert all(table[k] for k in table)


W2_CPU = G.WINO2_CASES
W43_CPU = G.WINO43_CASES[:-1]       # (the 11-image case repeats the 46 x 120 geometry of its neighbours: the emulation is the same)


@pytest.mark.parametrize('m,case', [(2, c) for c in W2_CPU] + [(4, c) for c in W43_CPU], ids=lambda v: '-'.join(map(str, v)) if isinstance(v, tuple) else 'F%d' % v)
def test_winograd_emulation_inside_the_derived_ceiling(m, case):
    """The fp32 emulation of F(m x m, 3 x 3) (sweep_inputs.wino_emul32) against ref64 on every Winograd sweep input: inside the derived
    ceiling (1.01 (cin + T_m) + extra) u S_w with a factor 2 to spare, with bias + residual + ReLU and bare.  In exact arithmetic the
    Winograd form IS the convolution (checked in fp64); rho, the emulation's error in units of u S_w, is what the GPU gate uses."""
    n, h, w, cin, cout = case
    x, wt, b, r = G.conv_inputs(n, cin, cout, h, w, out_hw=(h, w), res=True)
    k = R.WINO[m]
    d = R.wino_tiles(x.astype(np.float64), m)
    u = np.einsum('ia,ocab,jb->ocij', k['G'], wt.astype(np.float64), k['G'])
    v = np.einsum('ia,nctuab,jb->nctuij', k['BT'], d, k['BT'])
    y = R.wino_untile(np.einsum('pi,notuij,qj->notupq', k['AT'], np.einsum('ocij,nctuij->notuij', u, v), k['AT']), h, w)
    exact, s_direct = R.conv(x, wt, None, None, 1, 1)
    assert maxerr(y, exact, 'fp64 Winograd form') <= 1e-11 * float(s_direct.max())
    for (bb, rr, relu) in ((b, r, True), (None, None, False)):
        ref, bound, rho, s_w = G.wino_gate(x, wt, m, bb, rr, relu)
        assert (s_w >= s_direct - 1e-9).all()                       # the transforms only grow the scale
        ceiling = R.wino_ceiling(cin, m, s_w)
        e = np.abs(G.wino_emul32(x, wt, m, bb, rr, relu).astype(np.float64) - ref)
        ratio = float((e / ceiling).max())
        if os.environ.get('SS_VERBOSE'):
            print('  [ref64] F(%d) %s rho %.3f, emulation / ceiling %.3f' % (m, case, rho, ratio))
        assert ratio <= 0.5, (ratio, rho)
        assert 0 < rho and (e <= bound).all()


# ------------------------------------------------------------------------------------------------ LINEAR fusion
def lb_oracle(ref, tgt, m1, m2, mask):
    """oracle.pipeline.linear_blender on [3,h,w] / [h,w] arrays; on an empty overlap (where the reference raises) the library's
    extension ovl_mask = 0, written with the oracle's own blur"""
    r, t, a, b = T(ref)[None], T(tgt)[None], T(m1)[None, None], T(m2)[None, None]
    if float((a * b).round().sum()) == 0:
        with pytest.raises(RuntimeError):
            P.linear_blender(r, t, a, b, mask=mask)
        mask1 = (P.gaussian_blur_21_20(a + a) * a + a).clamp(0, 1)
        return (mask1 if mask else r * mask1 + t * ((1 - mask1) * b))[0].numpy()
    return P.linear_blender(r, t, a, b, mask=mask)[0].numpy()


def worst(got, ref, bound):
    return float((np.abs(R.f64(got) - ref) / np.maximum(bound, 1e-300)).max())


def test_linear_blender_golden(golden):
    """ref64.linear_blender against G7 (the reference's own fp32 run on bilinear-warped masks): the gates of test_g7_fusion"""
    g = golden('g7_fusion')
    wm = g['warped_with_mask']
    mask1, planes = R.linear_blender(wm[0, 0:3], wm[1, 0:3], wm[0, 3], wm[1, 3])
    assert maxerr(planes, g['linear'][0] if g['linear'].ndim == 4 else g['linear'], 'G7 linear') < 1e-3
    assert maxerr(mask1, np.asarray(g['mask1']).reshape(mask1.shape), 'G7 mask1') < 1e-5


@pytest.mark.parametrize('pattern', G.LB_PATTERNS)
@pytest.mark.parametrize('hc,wc', G.LB_CANVASES)
def test_linear_blender_oracle_inside_derived_bound(hc, wc, pattern):
    """Every case of the LINEAR sweep: the generator's own conditions hold (lb_case asserts them: masks on the 1/64 lattice, exact
    products and unions, exact centroid sums, |vec| >= 1 px or exactly 0, the overlap the pattern names), and the fp32 oracle -- a
    441-tap 2-D convolution, not the separable form the bound counts -- stays within HALF of ref64.linear_blend_bound on mask1
    and on the planes.  The bound is a few 1e-6 on mask1 and a few 1e-3 of 255 on the planes: the sizes are asserted too."""
    ref, tgt, m1, m2 = G.lb_case(pattern, hc, wc)
    mask1, planes, bm, bp = R.linear_blend_bound(ref, tgt, m1, m2)
    assert mask1.min() >= 0 and mask1.max() <= 1 and np.isfinite(planes).all()
    assert bm.max() < 2e-5 and bp.max() < 1e-2, (bm.max(), bp.max())
    rm = worst(lb_oracle(ref, tgt, m1, m2, True)[0], mask1, bm)
    rp = worst(lb_oracle(ref, tgt, m1, m2, False), planes, bp)
    if os.environ.get('SS_VERBOSE'):
        print('  [ref64] linear_blender %-9s %3dx%-3d oracle / bound: mask1 %.3f planes %.3f (bounds <= %.1e, %.1e)' % (
            pattern, hc, wc, rm, rp, bm.max(), bp.max()))
    assert rm <= 0.5 and rp <= 0.5, (rm, rp)            # observed <= 0.19 and <= 0.25


@pytest.mark.parametrize('pattern', G.LB_PATTERNS)
@pytest.mark.parametrize('hc,wc', [(12, 65), (65, 63), (97, 129)])
def test_linear_blender_chain_oracle_inside_derived_bound(hc, wc, pattern):
    """The three-view chain of the sweep: the oracle applied twice (its own fp32 f12 fed on) within half of the chain's bound, the
    second pass's own + mask1 x the first pass's.  The union mask is exact in fp32."""
    ref, tgt, m1, m2 = G.lb_case(pattern, hc, wc)
    w3, m3 = G.lb_third(hc, wc)
    _, f12, _, b12 = R.linear_blend_bound(ref, tgt, m1, m2)
    union = (m1 + m2 - m1 * m2).astype(np.float32)
    assert np.array_equal(union.astype(np.float64), R.f64(m1) + R.f64(m2) - R.f64(m1) * R.f64(m2))
    assert np.round(R.f64(union) * R.f64(m3)).sum() > 0, 'the third view misses the union'
    mk2, want, bm2, b2 = R.linear_blend_bound(f12, w3, union, m3)
    o12 = lb_oracle(ref, tgt, m1, m2, False)
    assert worst(lb_oracle(o12, w3, union, m3, True)[0], mk2, bm2) <= 0.5
    assert worst(lb_oracle(o12, w3, union, m3, False), want, b2 + mk2[None] * b12) <= 0.5


def test_linear_blender_gate_sees_the_seeded_mistakes():
    """What the issue names as surviving the old suite is outside the derived bound when it is made in the STATEMENT (the kernels'
    own seeded faults are in LAB_NOTES.md U.3): half rounded away from zero instead of to even, the blur's border repeated instead of
    reflected, a blur weight off by 2e-4, the 1e-3 of the denominator as 1e-2 where the projection's range is small."""
    ref, tgt, m1, m2 = G.lb_case('half', 21, 21)
    mask1, _, bm, _ = R.linear_blend_bound(ref, tgt, m1, m2)
    away = np.where(R.f64(m1) * R.f64(m2) == 0.5, 1.0, R.f64(m2)).astype(np.float32)       # as if 0.5 had rounded to 1
    assert worst(R.linear_blender(None, None, m1, away)[0], mask1, bm) > 100
    ref, tgt, m1, m2 = G.lb_case('rects', 21, 21)
    mask1, _, bm, _ = R.linear_blend_bound(ref, tgt, m1, m2)
    assert worst(R.linear_blender(None, None, m1, m2, blur=lambda x: R.blur21(x, border='symmetric'))[0], mask1, bm) > 100
    skewed = R.gauss21()
    skewed[3] += 2e-4
    skewed[17] -= 2e-4
    assert worst(R.linear_blender(None, None, m1, m2, blur=lambda x: R.blur21(x, k=skewed))[0], mask1, bm) > 2
    ref, tgt, m1, m2 = G.lb_case('last', 11, 11)                                            # an overlap of a row and a column: a range of a few px
    mask1, _, bm, _ = R.linear_blend_bound(ref, tgt, m1, m2)
    assert worst(R.linear_blender(None, None, m1, m2, eps=1e-2)[0], mask1, bm) > 2


def test_astype_u8_restatement():
    """The cast the byte sweep compares ss_canvas_to_u8 with == oracle.frame_io.to_video_frame wherever int32 holds the value"""
    from oracle import frame_io as FIO
    astype_u8 = G.astype_u8
    x = np.array([[[-0.0, -1.5, 255.99, 256.0, 300.7, -0.99, 255.0, -256.0, -257.5, 2147483520.0, -2147483648.0, 17.5]]] * 3, np.float32)
    assert np.array_equal(astype_u8(x.transpose(1, 2, 0)), FIO.to_video_frame(x))
    assert astype_u8(np.array([1e10, np.inf, -np.inf, np.nan], np.float32)).tolist() == [0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------ mesh geometry
def test_geometry_golden(golden):
    """ref64.decompose / h2mesh against G1 (the reference's fp32 run: DLT through an fp32 8 x 8 inverse, H2Mesh through an fp32
    3 x 3 inverse -- the fixture is 1e-6 of an entry and 0.015 px of a vertex from float64) and against the oracle."""
    from oracle import geometry as OG
    g = golden('g1_dlt')
    off = cases.g1_offsets().numpy()
    for tag, scale in (('full', 1.0), ('feat', 8.0)):
        H, Ht, Hr = R.decompose(off, 360, 480, scale)
        assert maxerr(H, g['H_' + tag], 'G1 H_' + tag) < 2e-6 and maxerr(Ht, g['H_tgt_' + tag], 'G1 H_tgt_' + tag) < 2e-6
        assert maxerr(Hr, g['H_ref_' + tag], 'G1 H_ref_' + tag) < 5e-5
        oH, oHt, oHr = OG.decompose(T(off), 360, 480, scale=scale)
        assert maxerr(oH, H) < 2e-6 and maxerr(oHt, Ht) < 2e-6 and maxerr(oHr, Hr) < 5e-5
    _, Ht, Hr = R.decompose(off, 360, 480, 1.0)
    rigid = np.repeat(R.rigid_mesh(360, 480)[None], off.shape[0], 0)
    assert maxerr(rigid, g['rigid']) == 0.0
    assert maxerr(R.h2mesh(Hr, rigid), g['mesh_ref'], 'G1 mesh_ref') < 0.03 and maxerr(R.h2mesh(Ht, rigid), g['mesh_tgt'], 'G1 mesh_tgt') < 0.03
    # H maps the corners onto the moved corners, to float64's accuracy: the statement is a homography, not a fit to the fixture
    c = np.array([[0.0, 0.0, 1.0], [480.0, 0.0, 1.0], [0.0, 360.0, 1.0], [480.0, 360.0, 1.0]])
    p = np.einsum('nij,kj->nki', R.decompose(off, 360, 480, 1.0)[0], c)
    moved = R.f64(np.float32(c[None, :, :2]) + off.reshape(-1, 4, 2))                  # c + m as the reference forms it, in fp32
    assert np.abs(p[..., :2] / p[..., 2:] - moved).max() < 1e-9


@pytest.mark.parametrize('kind', ['zero', 'mild', 'large'])
@pytest.mark.parametrize('img_h,img_w', G.GEOM_SIZES)
def test_geometry_inputs(img_h, img_w, kind):
    """The geometry sweep's offsets are what they say: zero gives the identity exactly, the large quads are convex (asserted by the
    generator) and far worse conditioned than the mild ones, and the oracle's own error -- the sweep's gate is 4 x it -- stays small
    enough to tell a wrong kernel: below 1e-3 of the frame on the meshes."""
    from oracle import geometry as OG
    off = G.geom_offsets(65, kind, img_h, img_w)
    H, Ht, Hr = R.decompose(off, img_h, img_w, 1.0)
    if kind == 'zero':
        assert np.array_equal(H, np.repeat(np.eye(3)[None], 65, 0)) and np.array_equal(Hr, H)
    o_r, o_t = G.geom_residuals(65)
    m1, _ = R.spatial_meshes(off, o_r, o_t, img_h, img_w)
    _, _, oHr = OG.decompose(T(off), img_h, img_w, scale=1.0)
    rigid = OG.rigid_mesh(65, img_h, img_w)
    e = maxerr(OG.homography_to_mesh(oHr, rigid) + T(o_r).reshape(65, 7, 9, 2) - rigid, m1, 'spatial_meshes oracle %s %dx%d' % (kind, img_h, img_w))
    assert e < 1e-3 * img_w, e


# ------------------------------------------------------------------------------------------------ SmoothNet glue
@pytest.mark.parametrize('zero_first', [0, 1])
def test_smooth_statements_against_oracle(zero_first):
    """ref64.smooth_embed / smooth_finalize against the oracle's MotionPrediction embeddings and build_SmoothNet's bookkeeping on one
    window: the fp32 reading equals the oracle where the oracle performs the same single operations (the window sums, the mesh and
    path bookkeeping), and the float64 reading holds the oracle inside half of the derived bound."""
    t = 7
    rs = np.random.RandomState(31 + zero_first)
    sm = [(G.rigid_px(360, 480).reshape(1, 63, 2) + rs.normal(0, 4, (t, 63, 2))).astype(np.float32) for _ in range(2)]
    ts = [rs.normal(0, 2, (t, 63, 2)).astype(np.float32) for _ in range(2)]
    delta = rs.normal(0, 1.5, (1, t, 63, 4)).astype(np.float32)
    net = N.SmoothNet()
    mp = net.MotionPre
    emb = [p.detach().numpy() for p in (mp.embedding1[0].weight, mp.embedding1[0].bias, mp.embedding3[0].weight, mp.embedding3[0].bias)]
    tl = [[T(x[k]).reshape(1, 7, 9, 2) * (0 if zero_first and k == 0 else 1) for k in range(t)] for x in ts]
    sl = [[T(x[k]).reshape(1, 7, 9, 2) for k in range(t)] for x in sm]
    om1, om2, op1, op2, _, _ = net(sl[0], sl[1], tl[0], tl[1])
    hid = torch.cat((mp.embedding1(om1), mp.embedding3(op1), mp.embedding1(om2), mp.embedding3(op2)), dim=4).reshape(1, t, 63, 128)
    args = (sm[0], sm[1], ts[0], ts[1])
    ref = R.smooth_embed(*args, *emb, 1, t, 1, zero_first)
    s = R.smooth_embed(*args, *emb, 1, t, 1, zero_first, absum=True)
    assert (np.abs(hid.numpy() - ref) <= 0.5 * R.smooth_bound(t + 3, s)).all()
    d1, d2 = T(delta[..., 0:2]).reshape(1, t, 7, 9, 2), T(delta[..., 2:4]).reshape(1, t, 7, 9, 2)
    oracle = dict(ori_path1=op1, smooth_path1=op1 + d1, ori_mesh1=om1, smooth_mesh1=om1 - d1,
                  ori_path2=op2, smooth_path2=op2 + d2, ori_mesh2=om2, smooth_mesh2=om2 - d2)
    f32 = R.smooth_finalize(*args, delta, 1, t, 1, zero_first, dt=np.float32)
    f64 = R.smooth_finalize(*args, delta, 1, t, 1, zero_first)
    s = R.smooth_finalize(*args, delta, 1, t, 1, zero_first, absum=True)
    for k, v in oracle.items():
        assert np.array_equal(v.numpy().reshape(1, t, 63, 2), f32[k]), k
        assert (np.abs(f32[k] - f64[k]) <= 0.5 * R.smooth_bound(t, s[k])).all(), k


@pytest.mark.parametrize('nw,t', [(1, 7), (2, 2), (30, 7), (300, 2)])
def test_smooth_stitch_statement_against_oracle_loop(nw, t):
    """ref64.smooth_stitch against oracle.pipeline.smooth_stage's own accumulation (the path stitching of test_metric_ssd.py:433-436)
    run on the statement's per-window outputs: equal bit for bit in fp32, and the fp32 loop within half of the derived bound."""
    rs = np.random.RandomState(41 + nw + t)
    n = nw + t - 1
    sm = [rs.normal(100, 40, (n, 63, 2)).astype(np.float32) for _ in range(2)]
    ts = [rs.normal(0, 2, (n, 63, 2)).astype(np.float32) for _ in range(2)]
    delta = rs.normal(0, 1.5, (nw, t, 63, 4)).astype(np.float32)
    o = {k: T(v) for k, v in R.smooth_finalize(sm[0], sm[1], ts[0], ts[1], delta, nw, t, 1, 1, dt=np.float32).items()}
    acc = {}
    for k in range(nw):                                  # oracle.pipeline.smooth_stage, lines 164-174, on window k's outputs
        if k == 0:
            for key in o:
                acc[key] = o[key][k]
        else:
            for key in ('ori_mesh1', 'smooth_mesh1', 'ori_mesh2', 'smooth_mesh2'):
                acc[key] = torch.cat((acc[key], o[key][k, -1:]), dim=0)
            new_ori = acc['ori_path2'][-1] + (o['ori_path2'][k, -1] - o['ori_path2'][k, -2])
            acc['ori_path2'] = torch.cat((acc['ori_path2'], new_ori.unsqueeze(0)), dim=0)
            new_sm = acc['ori_path2'][-1] + (o['smooth_path2'][k, -1] - o['ori_path2'][k, -1])
            acc['smooth_path2'] = torch.cat((acc['smooth_path2'], new_sm.unsqueeze(0)), dim=0)
    f32 = R.smooth_stitch(sm[0], sm[1], ts[0], ts[1], delta, nw, t, dt=np.float32)
    f64 = R.smooth_stitch(sm[0], sm[1], ts[0], ts[1], delta, nw, t)
    s = R.smooth_stitch(sm[0], sm[1], ts[0], ts[1], delta, nw, t, absum=True)
    rounds = (2 * np.arange(n) + 6).reshape(n, 1, 1)
    for k in f32:
        assert np.array_equal(acc[k].numpy(), f32[k]), k
        assert (np.abs(f32[k] - f64[k]) <= 0.5 * R.smooth_bound(rounds, s[k])).all(), k


def test_window_shift_statement():
    ring, rows = np.arange(12.0).reshape(4, 3), 100 + np.arange(6.0).reshape(2, 3)
    work, new = R.window_shift(ring, rows)
    assert np.array_equal(work, np.concatenate((ring[1:], rows))) and np.array_equal(new, np.concatenate((ring[2:], rows)))
    one = R.window_shift(R.window_shift(ring, rows[:1])[1], rows[1:])[1]
    assert np.array_equal(one, new)                      # k rows at once == k single pushes
    assert np.array_equal(R.window_shift(ring, 100 + np.arange(15.0).reshape(5, 3))[1], 100 + np.arange(3.0, 15.0).reshape(4, 3))


# ------------------------------------------------------------------------------------------------ canvas normalisation, watcher
def test_canvas_statements_against_oracle():
    """ref64.scale_to_hr / canvas_normalize / canvas_recover / three_view_align: the fp32 reading equals oracle.pipeline's own fp32
    tensors bit for bit where it performs the same single operations (_scale_to_hr, norm_mesh on the shifted mesh, recover_mesh), and
    the float64 reading differs from it by a few roundings only."""
    from oracle import geometry as OG
    rs = np.random.RandomState(51)
    m = (G.rigid_px(360, 480) + rs.normal(0, 9, (5, 7, 9, 2))).astype(np.float32)               # [5,7,9,2] LR
    hr = P._scale_to_hr(T(m)[None], 720, 1280)[0]
    assert np.array_equal(hr.numpy(), R.scale_to_hr(m, 720, 1280, np.float32))
    box = np.array([-31.7, 1893.2, -44.1, 801.6], np.float32)
    wmin, wmax, hmin, hmax = (torch.tensor(float(v)) for v in box)
    nm = OG.norm_mesh(torch.stack((hr[..., 0] - wmin, hr[..., 1] - hmin), dim=3), hmax - hmin, wmax - wmin)
    n32 = R.canvas_normalize(hr.numpy(), box, np.float32)
    assert np.array_equal(nm.numpy(), n32.reshape(5, 63, 2))
    assert maxerr(n32, R.canvas_normalize(R.f64(hr), R.f64(box))) < 20 * R.U24
    rec = OG.recover_mesh(nm, hmax - hmin, wmax - wmin)
    assert np.array_equal(rec.numpy().reshape(5, 63, 2), R.canvas_recover(n32.reshape(5, 63, 2), box, np.float32))
    # three-view alignment against oracle.pipeline.three_view_compose's first lines (an fp32 mean in torch's order)
    m4 = [(m + np.float32(k)).reshape(5, 63, 2) for k in (0.0, 40.0, 43.3, 90.0)]
    a1, a2, b1, b2, mid, absdiff = R.three_view_align(*[R.f64(x) for x in m4], 720, 1280)
    s = [P._scale_to_hr(T(x).reshape(1, 5, 7, 9, 2), 720, 1280) for x in m4]
    off = (s[1] - s[2]).reshape(1, 5, -1, 2).mean(dim=2).unsqueeze(2).unsqueeze(2)
    ob1 = (s[2] + off).reshape(5, 63, 2)
    omid = ((s[1] + (s[2] + off)) / 2.0).reshape(5, 63, 2)
    scaled = 1.01 * 2 * R.U24 * 2000.0
    mean_b = R.dot_bound(63, absdiff, extra=2) + 2 * scaled
    assert (np.abs(ob1.numpy() - b1) <= 0.5 * (mean_b + scaled + R.U24 * np.abs(b1))).all()
    assert (np.abs(omid.numpy() - mid) <= 0.5 * (0.5 * mean_b + scaled + 2 * R.U24 * np.abs(mid))).all()


def test_canvas_watch_statement():
    """The watcher's restatement on hand-worked frames: counts, the first clipped index, extents, the strict comparisons at the slack
    and at the guard, a NaN counted as outside and dropped from the extents."""
    one, slack = np.float32(1.0), R.WATCH_SLACK
    pts = np.zeros((1, 4, 2), np.float32)
    wi, wf = np.array([[0, 0, -1, 0]], np.int32), np.array([[np.inf, -np.inf, np.inf, -np.inf]], np.float32)
    for frame, want in (([0.5, -1.0], [1, 0, -1, 1]), ([one + slack, 0.0], [2, 0, -1, 2]), ([np.nextafter(one + slack, np.float32(2)), 0.0], [3, 1, 2, 3]),
                        ([0.0, one - np.float32(0.1)], [4, 1, 2, 3]), ([0.0, np.nextafter(one - np.float32(0.1), one)], [5, 1, 2, 4]),
                        ([np.nan, 0.3], [6, 2, 2, 5])):
        pts[0, 2] = frame
        R.canvas_watch(pts, 0.1, wi, wf)
        assert wi[0].tolist() == want, (frame, wi)
    assert wf[0].tolist() == [0.0, float(np.nextafter(one + slack, np.float32(2))), -1.0, float(np.nextafter(one - np.float32(0.1), one))]
    wi2 = np.array([[0, 0, -1, 0]], np.int32)
    pts[0, 2] = [0.0, 0.95]
    R.canvas_watch(pts, 1e-4, wi2, wf)                     # a guard below the slack: near coincides with outside
    assert wi2[0].tolist() == [1, 0, -1, 0]


# ------------------------------------------------------------------------------------------------ the derived gates of the rest sweep
@pytest.mark.parametrize('views', [2, 3])
@pytest.mark.parametrize('frames', G.NORM_FRAMES)
def test_canvas_normalize_fp32_reading_inside_half_the_gate(frames, views):
    """Every case of the normalise sweep (one box and a box per frame, scaled and unscaled): the fp32 reading of the statement -- the
    bits the kernels must produce -- stays within half of ref64.canvas_normalize_bound."""
    meshes, box, boxes = G.norm_case(frames, views)
    for (ih, iw) in G.NORM_SIZES:
        for b in (box, boxes[:, None]):
            for m in meshes:
                ref, gate = R.canvas_normalize_bound(R.scale_to_hr(R.f64(m), ih, iw), b)
                assert worst(R.canvas_normalize(R.scale_to_hr(m, ih, iw, np.float32), b, np.float32), ref, gate) <= 0.5


@pytest.mark.parametrize('frames', G.NORM_FRAMES)
def test_three_view_fp32_reading_inside_half_the_gates(frames):
    """Every case of the three-view sweep: the fp32 reading of align (numpy's order of the 63-point mean), of the normalisation of its
    five meshes and of the recovery stays within half of three_view_align_bound, canvas_normalize_bound and canvas_recover_bound."""
    m4, box = G.three_view_case(frames)
    ref, gates = R.three_view_align_bound(*m4, 720, 1280)
    five = R.three_view_align(*m4, 720, 1280, np.float32)[:5]
    for k in range(3):
        assert worst(five[2 + k], ref[2 + k], gates[k]) <= 0.5, k
    for j in range(5):
        want, gate = R.canvas_normalize_bound(five[j], box)
        n32 = R.canvas_normalize(five[j], box, np.float32)
        assert worst(n32, want, gate) <= 0.5
        want, gate = R.canvas_recover_bound(n32, box)
        assert worst(R.canvas_recover(n32, box, np.float32), want, gate) <= 0.5
    origin = np.array([box[0], box[2]], np.float32)
    want, gate = R.canvas_shift_bound(five[4], origin)
    assert worst((five[4] - origin).astype(np.float32), want, gate) <= 0.5


@pytest.mark.parametrize('zero_first', [0, 1])
@pytest.mark.parametrize('nw,t,wstride', G.SMOOTH_SHAPES, ids=lambda v: str(v))
def test_smooth_fp32_reading_inside_half_the_gate(nw, t, wstride, zero_first):
    """Every case of the SmoothNet sweep: the fp32 reading of smooth_embed (300 windows of 7 frames in the sweep's four slices) and of
    smooth_finalize stays within half of ref64.smooth_bound."""
    sm, ts, delta, emb = G.smooth_case(nw, t, wstride)
    args = (sm[0], sm[1], ts[0], ts[1])
    step = nw if nw * t <= 600 else 75
    for w0 in range(0, nw, step):
        sl = [x[w0 * wstride:] for x in args]
        s = R.smooth_embed(*sl, *emb, step, t, wstride, zero_first, absum=True)
        assert worst(R.smooth_embed(*sl, *emb, step, t, wstride, zero_first, dt=np.float32),
                     R.smooth_embed(*sl, *emb, step, t, wstride, zero_first), R.smooth_bound(t + 3, s)) <= 0.5
    f32 = R.smooth_finalize(*args, delta, nw, t, wstride, zero_first, dt=np.float32)
    f64 = R.smooth_finalize(*args, delta, nw, t, wstride, zero_first)
    s = R.smooth_finalize(*args, delta, nw, t, wstride, zero_first, absum=True)
    for k in f32:
        assert worst(f32[k], f64[k], R.smooth_bound(t, s[k])) <= 0.5, k


@pytest.mark.parametrize('nw,t', G.STITCH_SHAPES)
def test_smooth_stitch_fp32_reading_inside_half_the_gate(nw, t):
    sm, ts, delta, _ = G.smooth_case(nw, t, 1, seed=1)
    n = nw + t - 1
    f32 = R.smooth_stitch(sm[0], sm[1], ts[0], ts[1], delta, nw, t, dt=np.float32)
    f64 = R.smooth_stitch(sm[0], sm[1], ts[0], ts[1], delta, nw, t)
    s = R.smooth_stitch(sm[0], sm[1], ts[0], ts[1], delta, nw, t, absum=True)
    rounds = (2 * np.arange(n) + 6).reshape(n, 1, 1)
    for k in f32:
        assert worst(f32[k], f64[k], R.smooth_bound(rounds, s[k])) <= 0.5, k


def test_watch_frames_are_what_the_sweep_says():
    """The watcher sweep's frames under the restatement: which frames are outside and near at each guard, the first clipped frame 3."""
    f = G.watch_frames()
    for guard, near in ((0.0, [0, 0, 0, 1, 0, 1, 1]), (1e-4, [0, 0, 0, 1, 0, 1, 1]), (0.02, [1, 1, 0, 1, 1, 1, 1])):
        wi = np.array([[0, 0, -1, 0]] * 7, np.int32)
        wf = np.array([[np.inf, -np.inf, np.inf, -np.inf]] * 7, np.float32)
        R.canvas_watch(f.reshape(7, 126, 2), guard, wi, wf)
        assert wi[:, 1].tolist() == [0, 0, 0, 1, 0, 1, 1] and wi[:, 3].tolist() == near, (guard, wi)
    assert f[1, 0, 10, 0] == np.float32(1.0) + R.WATCH_SLACK and f[1, 1, 62, 0] == -(np.float32(1.0) + R.WATCH_SLACK)


# ------------------------------------------------------------------------------------------------ the coverage table of the library
def test_library_reach_covers_every_kernel_of_the_library():
    """sweep_inputs.library_reach against the gfx950 code objects of the built library, keyed by overload: a kernel's key is its base
    name, followed by its parameter list wherever the library carries more than one parameter list under that name (taken from the
    demangled names of the code objects, never from the table's aliases), so a kernel added as an overload of a covered name needs
    a row of its own.  Every kernel the library carries is held to a float64 statement ('fp64'), bit for bit to numpy ('exact'),
    bit for bit to kernels that are ('identity', every chain followed to its end), or listed as unreachable from the C ABI with the
    reason; the table names nothing the library lacks, and every test it cites exists in the module it names.  Names that come back
    mangled (no llvm-cxxfilt, no c++filt) fail the test: base names alone cannot tell overloads apart."""
    import re
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(os.path.dirname(here), 'tools'))
    import kernel_resources as KR
    from stabstitch2_amd import _hip as H
    names = sorted(KR.kernels(H.LIB_PATH))
    mangled = [n for n in names if n.startswith('_Z') or '(' not in n]
    assert not mangled, ('the kernel names came back without their parameter lists (neither llvm-cxxfilt nor c++filt demangled '
                         'them): overloads cannot be told apart, e.g. %s' % mangled[:3])
    lists = G.parameter_lists(names)
    have = {G.overload_key(n, lists) for n in names}
    assert {k.split('(')[0] for k in have} == {G.kernel_key(n).split('<')[0] for n in names}
    assert len(have) >= 82, sorted(have)               # the floor of 70 under base names, raised by the 12 keys the overloads add
    table = G.library_reach()
    unreachable = {k.split('<')[0] for k in G.UNREACHABLE}
    assert not set(table) & unreachable
    missing = sorted(have - set(table) - unreachable)
    assert not missing, 'kernels of the library that the coverage table lacks: %s' % missing
    stale = sorted((set(table) | unreachable) - have)
    assert not stale, 'the coverage table names kernels the library does not carry: %s' % stale
    defined = {}
    for kernel, (kind, tests, held_to) in table.items():
        assert kind in ('fp64', 'identity', 'exact') and tests, kernel
        assert bool(held_to) == (kind == 'identity'), kernel
        for tid in tests:
            mod, name = tid.split('::')
            if mod not in defined:
                defined[mod] = set(re.findall(r'^def (test_\w+)\(', open(os.path.join(here, mod + '.py')).read(), re.M))
            assert name in defined[mod], 'the coverage table cites %s, which %s.py does not define' % (tid, mod)
            if kind != 'identity':
                assert mod in G.SWEEP_MODULES, (kernel, tid)

    def ends_rooted(kernel, seen=()):
        kind, _, held_to = table[kernel]
        if kind != 'identity':
            return True
        assert kernel not in seen, 'identity cycle through ' + kernel
        return all(k in table and ends_rooted(k, seen + (kernel,)) for k in held_to)
    for kernel in table:
        assert ends_rooted(kernel), kernel


def _library_table_against_its_code_objects(lib_path, table):
    """A per-instantiation reach table (sweep_inputs.blend_reach / seam_reach) against the gfx950 code objects of its library: nothing
    missing, nothing stale, every cited test defined in a sweep module."""
    import re
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(os.path.dirname(here), 'tools'))
    import kernel_resources as KR
    names = sorted(KR.kernels(lib_path))
    mangled = [n for n in names if n.startswith('_Z') or '(' not in n]
    assert not mangled, 'the kernel names came back mangled: template arguments cannot be read, e.g. %s' % mangled[:3]
    have = {G.instantiation_key(n) for n in names}
    assert len(have) == len(names), names
    missing = sorted(have - set(table))
    assert not missing, 'kernels of %s that its coverage table lacks: %s' % (os.path.basename(lib_path), missing)
    stale = sorted(set(table) - have)
    assert not stale, 'the coverage table names kernels that %s does not carry: %s' % (os.path.basename(lib_path), stale)
    defined = {}
    for kernel, (kind, tests) in table.items():
        assert kind in ('fp64', 'exact') and tests, kernel
        for tid in tests:
            mod, name = tid.split('::')
            assert mod in G.SWEEP_MODULES, (kernel, tid)
            if mod not in defined:
                defined[mod] = set(re.findall(r'^def (test_\w+)\(', open(os.path.join(here, mod + '.py')).read(), re.M))
            assert name in defined[mod], 'the coverage table cites %s, which %s.py does not define' % (tid, mod)
    return have


def test_blend_reach_covers_every_kernel_of_the_blend_library():
    """mb_prepare_kernel<2|3>, mb_reduce_kernel and the twelve mb_collapse_kernel<V, COARSE, OUT> that libstabstitch_blend.so carries."""
    from stabstitch2_amd import _blend
    have = _library_table_against_its_code_objects(_blend.LIB_PATH, G.blend_reach())
    assert len(have) == 15 and sum(k.startswith('mb_collapse_kernel<') for k in have) == 12, sorted(have)


def test_seam_reach_covers_every_kernel_of_the_seam_library():
    """sm_cost_kernel, sm_dp_kernel and sm_paint_kernel of libstabstitch_seam.so, each for two and for three views."""
    from stabstitch2_amd import _seam
    have = _library_table_against_its_code_objects(_seam.LIB_PATH, G.seam_reach())
    assert have == {'%s<%d>' % (k, v) for k in ('sm_cost_kernel', 'sm_dp_kernel', 'sm_paint_kernel') for v in (2, 3)}
