"""CPU-only checks of the exposure compensation ("Exposure compensation"): its nine entry points exist on all three sides
of the ABI and refuse bad arguments with SS_ERR_ARG before any device work (every pointer below is host memory or NULL, so a launch
would fault instead); the float64 statement of the estimator (tests/exposure_ref.py) against hand-worked cases; and the stitchers'
refusals that need no device."""
import ctypes
import os
import re

import numpy as np
import pytest

import exposure_ref as E
from test_host_logic import built_lib  # noqa: F401  (fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
GAIN_RENDERS = ('ss_render_average_gains', 'ss_render_average_u8_gains', 'ss_render_average_clip_gains',
                'ss_render_average_clip_u8_gains', 'ss_render_linear_clip_gains', 'ss_render_linear_clip_u8_gains',
                'ss_render_linear_frames_gains', 'ss_render_linear_frames_u8_gains')
NAMES = ('ss_exposure_update',) + GAIN_RENDERS


def _ptr(buf):
    return ctypes.cast(buf, ctypes.c_void_p)


def test_exposure_symbols_exist_in_library_header_and_table(built_lib):
    from stabstitch2_amd import _hip
    hdr = open(os.path.join(ROOT, 'include', 'stabstitch_hip.h')).read()
    declared = set(re.findall(r'\bSS_API[^;]*?\b(ss_[a-z0-9_]+)\s*\(', hdr))
    for name in NAMES:
        assert hasattr(built_lib, name), name
        assert name in declared, name
        assert name in _hip.SIGNATURES, name
    assert sorted(_hip.SIGNATURES) == sorted(declared)


def test_exposure_update_refuses_bad_arguments(built_lib):
    views, hc, wc = 2, 45, 150
    per = built_lib.ss_render_footprint_floats(views, hc, wc)
    img = [(ctypes.c_float * 64)() for _ in range(3)]
    fp = (ctypes.c_float * (2 * per))()
    state, gains = (ctypes.c_float * 12)(), (ctypes.c_float * 64)()
    good = dict(imgs=(ctypes.c_void_p * 3)(*[ctypes.addressof(i) for i in img]), u8=0, img_fs=0, fp=_ptr(fp), per=per, fp_fs=per,
                frames=1, views=views, h=4, w=4, hc=hc, wc=wc, mode=0, alpha=0.1, sn=10.0, sg=0.1, lo=4.0, hi=251.0, mn=16,
                gmin=0.5, gmax=2.0, state=_ptr(state), gains=_ptr(gains))

    def call(**kw):
        a = dict(good, **kw)
        return built_lib.ss_exposure_update(a['imgs'], a['u8'], a['img_fs'], a['fp'], a['per'], a['fp_fs'], a['frames'], a['views'],
                                            a['h'], a['w'], a['hc'], a['wc'], a['mode'], a['alpha'], a['sn'], a['sg'], a['lo'],
                                            a['hi'], a['mn'], a['gmin'], a['gmax'], a['state'], a['gains'], None, None)

    for k in ('imgs', 'fp', 'state', 'gains'):
        assert call(**{k: None}) == ERR_ARG, k
    assert call(imgs=(ctypes.c_void_p * 3)(ctypes.addressof(img[0]), None, None)) == ERR_ARG          # a null view
    for v in (0, 1, 4):
        assert call(views=v, per=built_lib.ss_render_footprint_floats(max(v, 1), hc, wc)) == ERR_ARG, v
    assert call(views=3) == ERR_ARG                                               # (the row was built for two views)
    assert call(per=per - 1) == ERR_ARG and call(per=per + 4) == ERR_ARG and call(hc=hc + 8) == ERR_ARG and call(wc=wc + 64) == ERR_ARG
    assert call(frames=2, fp_fs=per - 1) == ERR_ARG                               # rows that would overlap
    assert call(frames=0) == ERR_ARG and call(frames=-1) == ERR_ARG
    assert call(lo=10.0, hi=9.0) == ERR_ARG and call(lo=float('nan')) == ERR_ARG
    for a in (0.0, -0.1, 1.5, float('nan')):
        assert call(alpha=a) == ERR_ARG, a
    assert call(gmin=2.5) == ERR_ARG and call(gmin=0.0) == ERR_ARG and call(gmax=float('nan')) == ERR_ARG
    assert call(sn=0.0) == ERR_ARG and call(sg=-1.0) == ERR_ARG and call(mn=0) == ERR_ARG
    assert call(mode=2) == ERR_ARG and call(mode=16) == ERR_ARG and call(u8=2) == ERR_ARG
    for k in ('h', 'w', 'hc', 'wc'):
        assert call(**{k: 1}) == ERR_ARG, k
    assert not any(state) and not any(gains)


def test_gain_renders_refuse_a_null_gains_pointer(built_lib):
    """Every gain form with valid host arguments but gains = NULL (and the AVERAGE forms with the folded opt-in) is refused before
    a launch; the same calls would otherwise fault on these host pointers."""
    buf = (ctypes.c_float * 4096)()
    imgs = (ctypes.c_void_p * 3)(*[ctypes.addressof(buf)] * 3)
    p, g = _ptr(buf), _ptr(buf)
    one_i = (ctypes.c_int * 1)(45)
    one_w = (ctypes.c_int * 1)(150)
    outs = (ctypes.c_void_p * 1)(ctypes.addressof(buf))
    L = built_lib
    assert L.ss_render_average_gains(imgs, p, p, None, 0, p, 2, 8, 8, 45, 150, 0, None, None) == ERR_ARG
    assert L.ss_render_average_u8_gains(imgs, p, p, None, 0, p, 2, 8, 8, 45, 150, 0, None, None) == ERR_ARG
    assert L.ss_render_average_clip_gains(imgs, p, p, None, 0, p, 2, 2, 8, 8, 45, 150, 0, None, None) == ERR_ARG
    assert L.ss_render_average_clip_u8_gains(imgs, p, p, None, 0, p, 2, 2, 8, 8, 45, 150, 0, None, None) == ERR_ARG
    assert L.ss_render_linear_clip_gains(imgs, p, p, p, None, 2, 2, 8, 8, 45, 150, 0, p, None, None) == ERR_ARG
    assert L.ss_render_linear_clip_u8_gains(imgs, p, p, p, None, 2, 2, 8, 8, 45, 150, 0, p, None, None) == ERR_ARG
    assert L.ss_render_linear_frames_gains(imgs, p, p, outs, 1, 2, 8, 8, one_i, one_w, 0, p, None, None) == ERR_ARG
    assert L.ss_render_linear_frames_u8_gains(imgs, p, p, outs, 1, 2, 8, 8, one_i, one_w, 0, p, None, None) == ERR_ARG
    # with gains: the folded radial term has no gain form, and the other refusals of the plain entries hold
    assert L.ss_render_average_gains(imgs, p, p, None, 0, p, 2, 8, 8, 45, 150, 16, g, None) == ERR_ARG
    assert L.ss_render_average_gains(imgs, p, p, None, 0, p, 4, 8, 8, 45, 150, 0, g, None) == ERR_ARG
    assert L.ss_render_average_gains(imgs, p, p, p, 7, p, 2, 8, 8, 45, 150, 0, g, None) == ERR_ARG          # a footprint of the wrong length
    assert L.ss_render_linear_frames_gains(imgs, p, p, outs, 33, 2, 8, 8, one_i, one_w, 0, p, g, None) == ERR_ARG


# ------------------------------------------------------------------------------------------------ the float64 statement
def _stats(n, ma, mb):
    return (n, np.full(3, n * ma), np.full(3, n * mb))


def test_two_views_meet_as_the_gain_prior_vanishes():
    """m_ba = gamma m_ab: the residual g_a m_ab - g_b m_ba of the minimiser falls with sigma_g and vanishes as sigma_g -> inf; both
    gains stay inside (min(1, 1 / gamma) .. max(1, gamma)) and the minimiser beats its neighbours in E."""
    m, gamma = 120.0, 0.8
    st = {(0, 1): _stats(500, m, gamma * m)}
    last = None
    for sg in (0.05, 0.1, 1.0, 10.0, 1e3, 1e5):
        g, kept = E.targets(st, 2, sigma_g=sg, clamp=False)
        assert kept
        res = abs(g[0, 0] * m - g[1, 0] * gamma * m)
        assert last is None or res < last, (sg, res, last)
        last = res
        assert g[0, 0] < 1.0 < g[1, 0] and g[1, 0] / g[0, 0] < 1.0 / gamma + 1e-12, (sg, g[:, 0])
        e0 = E.energy(g[:, 0], st, sigma_g=sg)
        for d in ((1e-4, 0), (-1e-4, 0), (0, 1e-4), (0, -1e-4)):
            assert E.energy(g[:, 0] + np.array(d), st, sigma_g=sg) > e0, (sg, d)
    assert last < 1e-6 * m, last
    # the default parameters: the known closed form of the symmetric two-view problem, d = r / (A_aa +- ...) checked through E's
    # stationarity instead: dE/dg = 0 within rounding
    g, _ = E.targets(st, 2)
    h = 1e-6
    for k in range(2):
        d = np.zeros(2)
        d[k] = h
        slope = (E.energy(g[:, 0] + d, st) - E.energy(g[:, 0] - d, st)) / (2 * h)
        assert abs(slope) < 1e-3 * E.energy(g[:, 0], st) + 1e-6, (k, slope)


def test_equal_means_give_gains_of_exactly_one():
    for v, st in ((2, {(0, 1): _stats(64, 97.3, 97.3)}),
                  (3, {(0, 1): _stats(64, 97.3, 97.3), (0, 2): _stats(30, 50.1, 50.1), (1, 2): _stats(99, 200.7, 200.7)})):
        g, kept = E.targets(st, v)
        assert kept and (g == 1.0).all(), g


def test_a_dropped_pair_leaves_its_views_at_one():
    g, kept = E.targets({(0, 1): _stats(15, 100.0, 80.0)}, 2)
    assert not kept and (g == 1.0).all()
    g, kept = E.targets({(0, 1): _stats(16, 100.0, 80.0)}, 2)
    assert kept and g[0, 0] < 1.0 < g[1, 0]
    # three views, only (0, 1) kept: view 2 stays at exactly 1, views 0 and 1 solve the two-view problem
    st = {(0, 1): _stats(400, 100.0, 80.0), (0, 2): _stats(3, 100.0, 10.0), (1, 2): _stats(0, 0.0, 0.0)}
    g3, kept = E.targets(st, 3)
    g2, _ = E.targets({(0, 1): st[(0, 1)]}, 2)
    assert kept and (g3[2] == 1.0).all() and np.array_equal(g3[:2], g2)


def test_three_view_chain_with_one_pair_missing():
    """Views 0 - 1 - 2 in a row, (0, 2) never overlap: the middle view ties the outer ones together -- darker and darker views get
    larger and larger gains, the result is the stationary point of E, and the clamp holds."""
    st = {(0, 1): _stats(300, 120.0, 96.0), (0, 2): _stats(0, 0.0, 0.0), (1, 2): _stats(200, 110.0, 88.0)}
    g, kept = E.targets(st, 3, clamp=False)
    assert kept and g[0, 0] < g[1, 0] < g[2, 0] and g[0, 0] < 1.0 < g[2, 0], g[:, 0]
    h = 1e-6
    for k in range(3):
        d = np.zeros(3)
        d[k] = h
        slope = (E.energy(g[:, 0] + d, st) - E.energy(g[:, 0] - d, st)) / (2 * h)
        assert abs(slope) < 1e-6 * E.energy(g[:, 0], st), (k, slope)
    gc, _ = E.targets(st, 3, gain_min=0.99, gain_max=1.01)
    assert gc.min() == 0.99 and gc.max() == 1.01


def test_usable_nodes_and_smoothing_by_hand():
    # a 45 x 150 canvas: lattice 7 x 7; rows i <= 5 (8 i <= 44) and columns j <= 4 (32 j <= 149) lie on it
    assert E.lattice_shape(45, 150) == (7, 7)
    oc = E.on_canvas(45, 150)
    assert oc[:6, :5].all() and not oc[6].any() and not oc[:, 5:].any()
    assert E.lattice_shape(64, 128) == (9, 5) and E.on_canvas(64, 128)[:8, :4].all() and not E.on_canvas(64, 128)[8].any()
    # constant images, identity coordinates: every on-canvas node inside [-1, 1]^2 counts; a coordinate one ulp beyond 1 does not
    lat = np.zeros((2, 7, 7, 2), np.float32)
    lat[0, 0, 0, 0] = np.nextafter(np.float32(1), np.float32(2))
    lat[1, 1, 1, 1] = -1.0
    imgs = [np.full((3, 9, 11), 100.0), np.full((3, 9, 11), 80.0)]
    for mode in ('NORMAL', 'FAST'):
        st, use, s = E.statistics(imgs, lat, 45, 150, mode)
        n, sa, sb = st[(0, 1)]
        assert n == 6 * 5 - 1 and not use[(0, 1)][0, 0] and use[(0, 1)][1, 1], (mode, n)
        assert np.allclose(sa, 100.0 * n) and np.allclose(sb, 80.0 * n)
    # thresholds: a view at 3 (< lo) or 252 (> hi) in one channel drops every node
    dark = [imgs[0], np.stack([np.full((9, 11), 80.0), np.full((9, 11), 3.0), np.full((9, 11), 80.0)])]
    assert E.statistics(dark, lat, 45, 150, 'NORMAL')[0][(0, 1)][0] == 0
    # smoothing: first kept frame sets, later ones move by alpha, a frame without a kept pair leaves the state alone
    s, started = np.ones((2, 3), np.float32), False
    s, started = E.smooth(s, started, np.full((2, 3), 1.2), False)
    assert not started and (s == 1).all()
    s, started = E.smooth(s, started, np.full((2, 3), 1.2), True)
    assert started and (s == np.float32(1.2)).all()
    s2, _ = E.smooth(s, started, np.full((2, 3), 0.8), True)
    want = np.float32(np.float32(1.2) + np.float32(np.float32(0.1) * np.float32(np.float32(0.8) - np.float32(1.2))))
    assert (s2 == want).all() and s2.dtype == np.float32
    s3, _ = E.smooth(s2, True, np.full((2, 3), 5.0), False)
    assert (s3 == s2).all()


# ------------------------------------------------------------------------------------------------ the stitchers' refusals
def test_stitchers_refuse_exposure_where_it_is_not_built():
    """Raised before a net or the device is looked at."""
    from stabstitch2_amd import online, ops
    with pytest.raises(ValueError, match='meshes_only'):
        online.OnlineStitcher(None, 180, 320, meshes_only=True, exposure=True)
    with pytest.raises(ValueError, match='ExposureParams'):
        online.OnlineStitcher(None, 180, 320, exposure=0.1)
    for cls, extra in ((online.MultiOnlineStitcher, dict(streams=2)), (online.ThreeViewOnlineStitcher, {}),
                       (online.PipelinedOnlineStitcher, {}), (online.PipelinedMultiOnlineStitcher, dict(streams=2)),
                       (online.PipelinedThreeViewOnlineStitcher, {})):
        for exp in (True, ops.ExposureParams()):
            with pytest.raises(ValueError, match='exposure'):
                cls(None, 180, 320, exposure=exp, **extra)
    p = ops.ExposureParams()
    assert tuple(p) == (0.1, 10.0, 0.1, 4.0, 251.0, 16, 0.5, 2.0) and ops.ExposureParams(alpha=0.5).alpha == 0.5
    assert tuple(p) == tuple(E.DEFAULTS[k] for k in p._fields)
