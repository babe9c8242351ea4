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
