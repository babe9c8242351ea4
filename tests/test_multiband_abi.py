"""MULTIBAND fusion without a GPU: the second library's header, exports and ctypes table, what it refuses, its workspace formula, the
properties of the float64 statement (tests/multiband_ref.py), the calibration of the bound against the fp32 program, and the kernels
the built library carries.  The kernels themselves: tests/test_gpu_multiband.py.
    python -m pytest tests/test_multiband_abi.py"""
import ctypes
import itertools
import os
import re
import sys

import numpy as np
import pytest
import torch

import abi_surface as A
import multiband_ref as MR
import sweep_inputs as G
from oracle import samplers as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
T = torch.from_numpy
EPS64 = 2.0 ** -53


@pytest.fixture(scope='module')
def blend_lib():
    from stabstitch2_amd import _blend
    return A.built(_blend)


def warped(size, views, seed=11):
    """P of a real warp, by the CPU oracle's sampler: the texture planes of sweep_inputs.warp_case + the weight plane + ones."""
    h, w, hc, wc = size
    U, src, tgt = G.warp_case(views, h, w, hc, wc, seed=seed)
    return S.tps_warp(T(MR.stack5(U[:, :3], h, w)), T(src), T(tgt), (hc, wc), 'NORMAL').numpy()


def bands_of(hc, wc):
    return sorted({0, 1, 3, MR.max_bands(hc, wc)})


# ------------------------------------------------------------------------------------------------ the surface
def test_header_exports_and_ctypes_table_agree(blend_lib):
    from stabstitch2_amd import _blend, _hip
    declared, defines = A.check(_blend)
    assert len(declared) == 4
    assert defines['SSB_ERR_ARG'] == _blend.ERR_ARG == ERR_ARG and defines['SSB_MAX_VIEWS'] == _blend.MAX_VIEWS == 3
    assert defines['SSB_MAX_BANDS'] == _blend.MAX_BANDS == MR.MAX_BANDS == 6
    assert blend_lib.ssb_version() == 1
    # the main library's surface is as it was
    main = open(os.path.join(ROOT, 'include', 'stabstitch_hip.h')).read()
    assert len(set(re.findall(r'\bSS_API[^;]*?\b(ss_[a-z0-9_]+)\s*\(', main))) == 113 == len(_hip.SIGNATURES)
    assert not re.search(r'ssb_|multiband', main, re.I)


def test_every_refusal_comes_before_a_launch(blend_lib):
    """Host pointers throughout: a call that got as far as a launch would fault."""
    L = blend_lib
    buf = (ctypes.c_float * (1 << 16))()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    need = L.ssb_multiband_workspace_floats(1, 2, 16, 16, 2)
    assert 0 < need < (1 << 16) - 4
    for fn in (L.ssb_multiband_blend, L.ssb_multiband_blend_u8):
        assert fn(None, p, p, need, 1, 2, 16, 16, 2, None) == ERR_ARG
        assert fn(p, None, p, need, 1, 2, 16, 16, 2, None) == ERR_ARG
        assert fn(p, p, None, need, 1, 2, 16, 16, 2, None) == ERR_ARG
        assert fn(p, p, p, need - 1, 1, 2, 16, 16, 2, None) == ERR_ARG                        # a workspace one float short
        assert fn(p, p, p, need, 2, 2, 16, 16, 2, None) == ERR_ARG                            # ... or sized for fewer frames
        assert fn(p, p, ctypes.c_void_p(p.value + 4), need, 1, 2, 16, 16, 2, None) == ERR_ARG  # not 16-byte aligned
        for views in (0, 1, 4):
            assert fn(p, p, p, 1 << 40, 1, views, 16, 16, 2, None) == ERR_ARG
        for bands in (-1, 7):
            assert fn(p, p, p, 1 << 40, 1, 2, 16, 16, bands, None) == ERR_ARG
        for frames in (0, -1, 65536):
            assert fn(p, p, p, 1 << 40, frames, 2, 16, 16, 2, None) == ERR_ARG
        for hc, wc, bands in ((0, 16, 0), (16, 0, 0), (2, 16, 1), (16, 2, 1), (9, 16, 4), (16, 5, 3), (40000, 16, 0)):
            assert fn(p, p, p, 1 << 40, 1, 2, hc, wc, bands, None) == ERR_ARG, (hc, wc, bands)
    # the level rule: 9 -> 5 -> 3 -> 2: three reductions are allowed, a fourth is not; bands = 0 takes any canvas
    assert L.ssb_multiband_workspace_floats(1, 2, 9, 9, 3) > 0 and L.ssb_multiband_workspace_floats(1, 2, 9, 9, 4) == -1
    assert L.ssb_multiband_workspace_floats(1, 3, 1, 1, 0) == 4 * 2 * 4 + 4 * 4               # one padded row of four per plane
    assert L.ssb_multiband_workspace_floats(16384, 2, 8, 8, 0) == -1                          # frames x planes beyond the grid


def test_workspace_formula(blend_lib):
    L = blend_lib
    for (hc, wc), views, frames in itertools.product([(80, 120), (81, 129), (85, 191), (43, 67), (3, 3), (720, 1280), (1083, 1931)],
                                                     (2, 3), (1, 3)):
        for bands in range(0, MR.max_bands(hc, wc) + 1):
            assert L.ssb_multiband_workspace_floats(frames, views, hc, wc, bands) == MR.workspace_floats(frames, views, hc, wc, bands)
        if MR.max_bands(hc, wc) < MR.MAX_BANDS:
            assert L.ssb_multiband_workspace_floats(frames, views, hc, wc, MR.max_bands(hc, wc) + 1) == -1
            with pytest.raises(ValueError):
                MR.level_sizes(hc, wc, MR.max_bands(hc, wc) + 1)
    assert MR.level_sizes(85, 191, 5) == [(85, 191), (43, 96), (22, 48), (11, 24), (6, 12), (3, 6)]


def test_ops_refuse_bad_bands_before_touching_the_device(blend_lib):
    from stabstitch2_amd import ops
    for bad in (-1, 7, 2.0, None, True):
        with pytest.raises(ValueError, match='bands'):
            ops.check_bands(bad)
    with pytest.raises(ValueError, match='3 pixels'):
        ops.check_bands(4, 9, 9)
    assert ops.check_bands(3, 9, 9) == 3
    with pytest.raises(ValueError):
        ops.multiband_workspace(1, 4, 80, 120, 5, 'cpu')
    assert ops.multiband_workspace(2, 3, 80, 120, 5, 'cpu').numel() == MR.workspace_floats(2, 3, 80, 120, 5)
    assert np.array_equal(ops.multiband_weight_plane(7, 10, 'cpu').numpy(), MR.weight_plane(7, 10))
    assert 'MULTIBAND' not in ops.FUSIONS and not ops.fused_render('MULTIBAND')


# ------------------------------------------------------------------------------------------------ the statement, in float64
def test_weight_plane_is_a_product_of_border_distances():
    w = MR.weight_plane(5, 8)
    assert w.dtype == np.float32 and w[0].tolist() == [1, 2, 3, 4, 4, 3, 2, 1] and w[:, 0].tolist() == [1, 2, 3, 2, 1] and w[2, 3] == 12


def test_reduce_and_expand_reflect_without_repeating_the_edge():
    a = np.arange(7, dtype=np.float64) ** 2                             # 0 1 4 9 16 25 36
    r = MR.reduce(np.tile(a, (5, 1)))[0]
    assert r.tolist() == [(4 + 1 * 4 + 0 * 6 + 1 * 4 + 4) / 16, (0 + 4 + 24 + 36 + 16) / 16, (4 + 36 + 96 + 100 + 36) / 16,
                          (16 + 100 + 216 + 100 + 16) / 16]
    u = np.array([1.0, 5.0, 2.0])
    e6 = MR.expand(np.tile(u, (3, 1)), 5, 6)[0]                         # even size: the last odd output reflects m -> m - 2
    assert e6.tolist() == [(5 + 6 + 5) / 8, 3.0, (1 + 30 + 2) / 8, 3.5, (5 + 12 + 5) / 8, (2 + 5) / 2]
    assert MR.expand(np.tile(u, (3, 1)), 5, 5)[0].tolist() == e6.tolist()[:5]
    c = np.full((2, 9, 13), 7.0)
    assert (MR.reduce(c) == 7.0).all() and (MR.expand(MR.reduce(c), 9, 13) == 7.0).all()          # the taps sum to one, edges included


@pytest.mark.parametrize('views', [2, 3])
def test_identical_views_give_that_view_on_the_union(views):
    P = MR.made_up('hole', views, 81, 129)
    P[:, :3] = P[0, :3]
    for bands in (0, 3, 6):
        out, r, union = MR.blend(P, bands, raw=True)
        assert union.any() and not union.all()
        assert np.abs(out - P[0, :3])[:, union].max() <= 255 * EPS64 * MR.roundings(bands, views)
        assert (out[:, ~union] == 0).all()


@pytest.mark.parametrize('views', [2, 3])
@pytest.mark.parametrize('kind', MR.MADE_UP)
def test_zero_bands_is_the_hard_seam_composite(kind, views):
    P = MR.made_up(kind, views, 43, 67)
    valid, union, owner = MR.decisions(P)
    want = np.where(union[None], np.take_along_axis(P[:, :3].astype(np.float64), owner[None, None].repeat(3, 1), 0)[0], 0.0)
    assert np.array_equal(MR.blend(P, 0), want)
    assert np.array_equal(MR.blend(P, 0, np.float32), want.astype(np.float32))
    assert all(valid[owner[y, x], y, x] for y, x in zip(*np.nonzero(union)))
    if kind != 'empty':                                                  # every view owns something, and weights decide it
        assert len(np.unique(owner[union])) == views
    s = MR.filled(P)[1]
    for _ in range(3):                                                   # a partition of unity at every level, exactly
        assert (s.sum(0) == 1.0).all()
        s = MR.reduce(s)


def test_a_view_with_an_empty_mask_changes_nothing():
    P = MR.made_up('empty', 3, 81, 129)
    assert not (P[1, 4] >= 0.5).any()
    for bands in (0, 3, 6):
        assert np.array_equal(MR.blend(P, bands), MR.blend(P[[0, 2]], bands))


def test_bands_spread_a_brightness_step():
    """Two constant views 100 and 140 on an 80 x 200 canvas overlapping in columns 60..139: the largest step between neighbours along
    row 40 is the whole difference with no bands, and shrinks as the bands widen the transition; the seam is down the middle."""
    P = MR.side_by_side()
    owner = MR.decisions(P)[2]
    assert (owner[:, :100] == 0).all() and (owner[:, 100:] == 1).all()         # also at the top and bottom rows: the product form
    step = {b: float(np.abs(np.diff(MR.blend(P, b)[0, 40])).max()) for b in (0, 1, 4)}
    assert step[0] == 40.0
    assert 9.6 <= step[1] <= 10.94
    assert 1.04 <= step[4] <= 1.23
    with_min = P.copy()                                                  # the min of the four distances instead: ties over triangles
    for v, sl in ((0, slice(0, 140)), (1, slice(60, 200))):
        yy, xx = np.meshgrid(np.arange(80), np.arange(140), indexing='ij')
        with_min[v, 3, :, sl] = np.minimum(np.minimum(xx + 1, 140 - xx), np.minimum(yy + 1, 80 - yy))
    assert (MR.decisions(with_min)[2][0, 60:100] == 0).all() and (MR.decisions(with_min)[2][0, 100:140] == 0).all()


@pytest.mark.parametrize('views', [2, 3])
def test_the_view_order_does_not_matter_without_weight_ties(views):
    """On a canvas the views cover between them.  (Outside the union the statement gives view 0 the weight, so within reach of an
    uncovered area where two different views both end, the order does matter: by 11 grey levels on the warp of CASES[1].)"""
    hc, wc = 81, 129
    P = MR.made_up('hole', views, hc, wc)
    P[:, 4] = 0.0
    P[0, 4, :, :2 * wc // 3] = 1.0
    P[1, 4, :, wc // 3:] = 1.0
    P[views - 1, 4, hc // 2:, :] = 1.0
    P[:, 3] = np.floor(P[:, 3])
    for v in range(1, views):                                            # integer weights tie at isolated pixels: none is left
        P[v, 3] += np.float32(0.3 * v)
    valid = P[:, 4] >= 0.5
    assert valid.any(0).all()
    for a, b in itertools.combinations(range(views), 2):
        assert not (valid[a] & valid[b] & (P[a, 3] == P[b, 3])).any()
    assert (valid.sum(0) >= 2).mean() > 0.1
    ref = MR.blend(P, 4)
    for perm in itertools.permutations(range(views)):
        assert np.abs(MR.blend(P[list(perm)], 4) - ref).max() <= 255 * EPS64 * MR.roundings(4, views), perm


def test_the_pyramid_overshoots_and_the_clamp_holds_it():
    P = clamp_case(85, 191)
    out, r, union = MR.blend(P, 3, raw=True)
    assert r.min() < -20 and r.max() > 275 and out.min() == 0.0 and out.max() == 255.0


def clamp_case(hc, wc):
    """A 0 / 255 checkerboard next to a view that is 255 above the middle row and 0 below it: the detail of one on the level of the
    other leaves 0..255 on both sides."""
    yy, xx = np.meshgrid(np.arange(hc), np.arange(wc), indexing='ij')
    P = np.zeros((2, 5, hc, wc), np.float32)
    P[0, :3] = 255.0 * ((xx + yy) & 1)
    P[1, :3] = np.where(yy < hc // 2, 255.0, 0.0)
    P[0, 3] = wc - xx
    P[1, 3] = xx + 0.5
    P[:, 4] = 1.0
    return P


# ------------------------------------------------------------------------------------------------ the bound
def test_bound_is_not_vacuous():
    """E(B) = u * 255 * roundings(B, V), u = 2^-24, the count derived in multiband_ref.roundings from the fp32 program: a fiftieth of a
    grey level at five bands.  A wrong tap at a border costs grey levels."""
    assert MR.bound(5, 2) <= MR.bound(5, 3) <= 0.05
    assert MR.bound(5, 3) == 2.0 ** -24 * 255 * MR.roundings(5, 3) and MR.roundings(5, 3) == 1418
    assert all(MR.bound(b, 3) < MR.bound(b + 1, 3) for b in range(6))
    P = warped(MR.CASES[0], 2)
    hc, wc = P.shape[-2:]
    good = MR.blend(P, 3)
    real = MR._reflect
    try:
        MR._reflect = lambda i, n: np.clip(i, 0, n - 1)                  # the edge repeated instead of reflected
        bad = MR.blend(P, 3)
    finally:
        MR._reflect = real
    assert np.abs(bad - good).max() > 20 * MR.bound(3, 2)


@pytest.mark.parametrize('views', [2, 3])
@pytest.mark.parametrize('size', MR.CASES, ids=lambda s: '%dx%d_to_%dx%d' % s)
def test_fp32_program_stays_inside_half_the_bound(size, views):
    """Every case of the GPU sweep: real warps and the made-up masks, at 0, 1, 3 and the most bands the canvas allows, and the clamp
    case.  Observed: at most 0.026 of the bound (one band), 0.004 at six bands."""
    hc, wc = size[2:]
    inputs = [('warp', warped(size, views))] + [(k, MR.made_up(k, views, hc, wc)) for k in MR.MADE_UP] + [('clamp', clamp_case(hc, wc))]
    for name, P in inputs:
        v = P.shape[0]
        for bands in bands_of(hc, wc):
            err = float(np.abs(MR.blend(P, bands, np.float32).astype(np.float64) - MR.blend(P, bands)).max())
            if G.VERBOSE:
                print('  [multiband fp32] %s %s V%d B%d: %.2e = %.4f of the bound' % (size, name, v, bands, err, err / MR.bound(bands, v)))
            assert err <= 0.5 * MR.bound(bands, v), (name, bands, err)
    P = inputs[0][1]
    assert ((P[:, 4] >= 0.5).sum(0) >= 2).mean() >= 0.1                   # the warped views do overlap


@pytest.mark.parametrize('views', [2, 3])
def test_fp32_program_on_the_small_canvases_stays_under_a_fiftieth_of_the_bound(views):
    """The inputs of the GPU sweep's small canvases (multiband_ref.SMALL, small_case) at every band count each allows: the bound is not
    what would let a wrong tap through there.  Observed: at most 0.0175 of the bound.  The inputs are what the sweep says they are:
    untied weights, and from 2 x 2 upwards a valid and an invalid mask value."""
    for hc, wc in MR.SMALL:
        P = MR.small_case(views, hc, wc)
        valid = P[:, 4] >= 0.5
        assert len(np.unique(P[:, 3])) == P[:, 3].size and (min(hc, wc) < 2 or (valid.any() and not valid.all())), (hc, wc)
        for bands in range(MR.max_bands(hc, wc) + 1):
            err = float(np.abs(MR.blend(P, bands, np.float32).astype(np.float64) - MR.blend(P, bands)).max())
            assert err <= 0.02 * MR.bound(bands, views), (hc, wc, bands, err)
        with pytest.raises(ValueError):
            MR.blend(P, MR.max_bands(hc, wc) + 1)
    assert [MR.max_bands(*s) for s in MR.SMALL] == [0, 0, 0, 0, 0, 1, 1, 2, 2, 1, 1]


# ------------------------------------------------------------------------------------------------ the kernels of the library
def test_kernels_have_no_scratch_and_no_spills(blend_lib):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_resources as KR
    from stabstitch2_amd import _blend
    ks = KR.kernels(_blend.LIB_PATH)
    base = sorted(re.sub(r'<.*', '', n.replace('void ', '').replace('(anonymous namespace)::', '')).split('(')[0] for n in ks)
    assert base == ['mb_collapse_kernel'] * 12 + ['mb_prepare_kernel'] * 2 + ['mb_reduce_kernel'], sorted(ks)
    for n, e in ks.items():
        assert e['.private_segment_fixed_size'] == 0 and e['.vgpr_spill_count'] == 0 and e['.sgpr_spill_count'] == 0, (n, e)
        assert e.get('.agpr_count', 0) == 0 and e['.vgpr_count'] <= 168, (n, e)                 # three waves per SIMD at the least
        assert e['.group_segment_fixed_size'] == (35 * 72 * 4 + 35 * 33 * 4 if 'mb_reduce_kernel' in n else 0), (n, e)
        assert e['mfma_instructions'] == 0
