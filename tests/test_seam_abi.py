"""MULTIBAND's content-aware seam without a GPU: the third library's header, exports and ctypes table, what it refuses, its workspace
formula, the kernels the built library carries, and the properties of the restatement (tests/seam_ref.py) on made-up P.  The kernels
themselves: tests/test_gpu_seam.py.
    python -m pytest tests/test_seam_abi.py"""
import ctypes
import itertools
import os
import re
import sys

import numpy as np
import pytest

import abi_surface as A
import multiband_ref as MR
import seam_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1


@pytest.fixture(scope='module')
def seam_lib():
    from stabstitch2_amd import _seam
    return A.built(_seam)


# ------------------------------------------------------------------------------------------------ the surface
def test_header_exports_and_ctypes_table_agree(seam_lib):
    from stabstitch2_amd import _seam
    declared, defines = A.check(_seam)
    assert declared == ['ssm_multiband_seam', 'ssm_seam_workspace_bytes', 'ssm_version']
    assert defines['SSM_ERR_ARG'] == _seam.ERR_ARG == ERR_ARG and defines['SSM_MAX_VIEWS'] == _seam.MAX_VIEWS == 3
    assert defines['SSM_MU_MAX'] == _seam.MU_MAX == 65535 and defines['SSM_STATE_HEADER'] == _seam.STATE_HEADER == SR.HEADER
    assert defines['SSM_LDS_BYTES'] == _seam.LDS_BYTES == SR.LDS_BYTES == 160 * 1024 and defines['SSM_TILE_W'] == _seam.TILE_W
    assert seam_lib.ssm_version() == 1
    # (that the libraries before it do not know of it: test_native_binding.py, for every library)


def test_every_refusal_comes_before_a_launch(seam_lib):
    """Host pointers throughout: a call that got as far as a launch would fault."""
    L = seam_lib
    buf = (ctypes.c_int * (1 << 16))()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    fn = L.ssm_multiband_seam
    need = L.ssm_seam_workspace_bytes(1, 2, 16, 16, 4)
    assert 0 < need < 4 * ((1 << 16) - 4)
    st = SR.HEADER + 4
    big = 1 << 40
    assert fn(None, 1, 2, 16, 16, 4, 0, 8.0, p, st, p, need, None) == ERR_ARG
    assert fn(p, 1, 2, 16, 16, 4, 0, 8.0, p, st, None, need, None) == ERR_ARG
    assert fn(p, 1, 2, 16, 16, 4, 0, 8.0, p, st, p, need - 1, None) == ERR_ARG                       # a workspace one byte short
    assert fn(p, 2, 2, 16, 16, 4, 0, 8.0, p, st, p, need, None) == ERR_ARG                           # ... or sized for fewer frames
    assert fn(p, 1, 2, 16, 16, 4, 0, 8.0, p, st, ctypes.c_void_p(p.value + 4), need, None) == ERR_ARG  # not 16-byte aligned
    assert fn(p, 1, 2, 16, 16, 4, 0, 8.0, p, st - 1, p, need, None) == ERR_ARG                       # a state one int short
    assert fn(p, 1, 3, 16, 16, 4, 0, 8.0, p, st, p, big, None) == ERR_ARG                            # ... or of fewer views
    assert fn(p, 1, 2, 16, 16, 4, 0, 8.0, ctypes.c_void_p(p.value + 2), st, p, need, None) == ERR_ARG
    assert fn(ctypes.c_void_p(p.value + 2), 1, 2, 16, 16, 4, 0, 8.0, None, 0, p, need, None) == ERR_ARG
    for views in (0, 1, 4):
        assert fn(p, 1, views, 16, 16, 4, 0, 8.0, None, 0, p, big, None) == ERR_ARG
    for cell in (0, -4, 3, 5, 32):
        assert fn(p, 1, 2, 16, 16, cell, 0, 8.0, None, 0, p, big, None) == ERR_ARG
    for mu in (-1, 65536):
        assert fn(p, 1, 2, 16, 16, 4, mu, 8.0, None, 0, p, big, None) == ERR_ARG
    for prior in (-0.5, 255.5, float('nan'), float('inf')):
        assert fn(p, 1, 2, 16, 16, 4, 0, prior, None, 0, p, big, None) == ERR_ARG
    for frames in (0, -1, 65536):
        assert fn(p, frames, 2, 16, 16, 4, 0, 8.0, None, 0, p, big, None) == ERR_ARG
    for hc, wc in ((0, 16), (16, 0), (40000, 16), (16, 40000)):
        assert fn(p, 1, 2, hc, wc, 4, 0, 8.0, None, 0, p, big, None) == ERR_ARG
    # a grid whose rows and back pointers exceed the LDS of a workgroup: refused by both, a larger cell is taken
    assert L.ssm_seam_workspace_bytes(1, 2, 1100, 1950, 1) == -1 and fn(p, 1, 2, 1100, 1950, 1, 0, 8.0, None, 0, p, big, None) == ERR_ARG
    assert L.ssm_seam_workspace_bytes(1, 2, 1100, 1950, 4) > 0


def test_workspace_formula_and_lds_rule(seam_lib):
    from stabstitch2_amd import _seam
    L = seam_lib
    sizes = [(37, 61), (81, 129), (13, 2100), (1, 1), (3, 5), (720, 1280), (1083, 1931), (2160, 3840), (3000, 5000)]
    for (hc, wc), views, frames, c in itertools.product(sizes, (2, 3), (1, 5), SR.CELLS):
        want = SR.workspace_bytes(frames, views, hc, wc, c)
        assert L.ssm_seam_workspace_bytes(frames, views, hc, wc, c) == want, (hc, wc, views, frames, c)
        assert (want < 0) == (SR.lds_bytes(hc, wc, c) > SR.LDS_BYTES) and SR.lds_bytes(hc, wc, c) == _seam.lds_bytes(hc, wc, c)
        if want > 0:
            lay = _seam.layout(frames, views, hc, wc, c)
            assert want == 4 * lay['ints']
            assert lay['cost'][0] == 0 and lay['cost'][1][-2:] == (SR.grid(hc, wc, c)[0], (SR.grid(hc, wc, c)[1] + 3) & ~3)
    # the edge of the rule, exactly: 4 (16 + 2 wq4 + 3 hq) + hq wq4 / 4 <= 163840
    assert SR.lds_bytes(600, 1000, 1) == 4 * (16 + 2000 + 1800) + 150000 == 165264 and L.ssm_seam_workspace_bytes(1, 2, 600, 1000, 1) == -1
    assert SR.lds_bytes(594, 1000, 1) <= SR.LDS_BYTES < SR.lds_bytes(595, 1000, 1)
    assert L.ssm_seam_workspace_bytes(1, 2, 594, 1000, 1) > 0 and L.ssm_seam_workspace_bytes(1, 2, 595, 1000, 1) == -1
    # the default cell: 4 on a 720p panorama, larger ones as the canvas grows
    assert SR.default_cell(1083, 1931) == 4 == SR.default_cell(2160, 3840) and SR.default_cell(3000, 5000) == 8
    assert SR.default_cell(6000, 10000) == 16


def test_ops_refuse_bad_seam_arguments_before_touching_the_device(seam_lib):
    from stabstitch2_amd import ops, pipeline, online
    assert ops.seam_cell(1083, 1931) == 4 and ops.seam_cell(3000, 5000) == 8 and ops.seam_cell(37, 61, 1) == 1
    for bad in (0, 3, 32, 4.0, True, '4'):
        with pytest.raises(ValueError, match='cell'):
            ops.seam_cell(80, 120, bad)
    with pytest.raises(ValueError, match=r'larger cell, cell=2 fits'):
        ops.seam_cell(1083, 1931, 1)
    with pytest.raises(ValueError, match=r'larger cell, cell=8 fits'):
        ops.seam_cell(3000, 5000, 4)
    assert ops.seam_params(80, 120) == (4, 192, 8.0) and ops.seam_params(80, 120, 2, 0, 0) == (2, 0, 0.0)
    assert ops.seam_params(3000, 5000)[:2] == (8, 384)
    for mu in (-1, 65536, 1.5, True):
        with pytest.raises(ValueError, match='mu'):
            ops.seam_params(80, 120, mu=mu)
    for prior in (-1.0, 255.5, float('nan')):
        with pytest.raises(ValueError, match='prior'):
            ops.seam_params(80, 120, prior=prior)
    st = ops.seam_state(3, 81, 129, 4, 'cpu')
    assert st.dtype.is_floating_point is False and st.numel() == SR.HEADER + 2 * 21 and not st.any()
    assert ops.seam_state(2, 1083, 1931, None, 'cpu').numel() == SR.HEADER + 271
    with pytest.raises(ValueError):
        ops.seam_state(4, 81, 129, 4, 'cpu')
    assert ops.seam_workspace(5, 3, 81, 129, 2, 'cpu').numel() * 4 == SR.workspace_bytes(5, 3, 81, 129, 2)
    with pytest.raises(ValueError, match='cell'):
        ops.seam_workspace(1, 2, 1083, 1931, 1, 'cpu')
    # seam= is MULTIBAND's, its parameters are the DP seam's
    assert ops.check_seam(None) is None and ops.check_seam('dp') == 'dp' and ops.check_seam('geometric') == 'geometric'
    with pytest.raises(ValueError, match='seam'):
        ops.check_seam('graphcut')
    with pytest.raises(ValueError, match='MULTIBAND'):
        ops.check_seam('dp', 'LINEAR')
    assert pipeline.seam_options('MULTIBAND') == {} == pipeline.seam_options('MULTIBAND', 'geometric') == pipeline.seam_options('AVERAGE')
    assert pipeline.seam_options('MULTIBAND', 'dp', seam_mu=7) == dict(seam='dp', seam_cell=None, seam_mu=7, seam_prior=None)
    with pytest.raises(ValueError, match="seam='dp'"):
        pipeline.seam_options('MULTIBAND', 'geometric', seam_cell=4)
    for fusion in ('AVERAGE', 'FEATHER', 'LINEAR'):
        with pytest.raises(ValueError, match='MULTIBAND'):
            pipeline.seam_options(fusion, 'dp')
        for cls in (online.OnlineStitcher, online.ThreeViewOnlineStitcher):
            with pytest.raises(ValueError, match='MULTIBAND'):
                cls(None, 360, 480, fusion_mode=fusion, seam='dp')
    # classes that refuse MULTIBAND keep refusing it, with or without a seam
    for cls in (online.MultiOnlineStitcher, online.PipelinedOnlineStitcher):
        with pytest.raises((ValueError, TypeError)):
            cls(None, 360, 480, fusion_mode='MULTIBAND', seam='dp')


def test_kernels_have_no_scratch_and_no_spills(seam_lib):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_resources as KR
    from stabstitch2_amd import _seam
    ks = KR.kernels(_seam.LIB_PATH)
    base = sorted(re.sub(r'<.*', '', n.replace('void ', '').replace('(anonymous namespace)::', '')).split('(')[0] for n in ks)
    assert base == ['sm_cost_kernel'] * 2 + ['sm_dp_kernel'] * 2 + ['sm_paint_kernel'] * 2, sorted(ks)
    for n, e in ks.items():
        assert e['.private_segment_fixed_size'] == 0 and e['.vgpr_spill_count'] == 0 and e['.sgpr_spill_count'] == 0, (n, e)
        assert e.get('.agpr_count', 0) == 0 and e['.vgpr_count'] <= 168, (n, e)                 # three waves per SIMD at the least
        lds = SR.LDS_BYTES if 'sm_dp_kernel' in n else 0 if 'sm_paint_kernel' in n else 6 * 1024 * 4 + (8 * 2 + 16 * 1 if '<2>' in n else 8 * 3 + 16 * 3)
        assert e['.group_segment_fixed_size'] == lds, (n, e)
        assert e['mfma_instructions'] == 0


# ------------------------------------------------------------------------------------------------ the restatement
def test_tie_rules_of_the_dynamic_program():
    xs, cost = SR.dp(np.array([[5, 0, 5], [0, 9, 0]], np.int64))
    assert xs.tolist() == [1, 0] and cost == 0                          # the end point: the lowest of equal minima; it came from its right
    xs, cost = SR.dp(np.array([[0, 5, 0], [9, 0, 9]], np.int64))
    assert xs.tolist() == [0, 1] and cost == 0                          # left before right
    xs, cost = SR.dp(np.array([[0, 0, 0], [9, 0, 9], [0, 0, 0]], np.int64))
    assert xs.tolist() == [1, 1, 0] and cost == 0                       # straight before either; row 2 ends at the lowest x, from its right
    xs, cost = SR.dp(np.zeros((4, 1), np.int64))
    assert xs.tolist() == [0, 0, 0, 0] and cost == 0                    # a single column has no neighbours
    rs = np.random.RandomState(5)
    for _ in range(20):
        Ep = rs.randint(0, 50, (rs.randint(1, 9), rs.randint(1, 9))).astype(np.int64)
        xs, cost = SR.dp(Ep)
        assert cost == SR.optimum(Ep) == SR.path_cost(Ep, xs) and (np.abs(np.diff(xs)) <= 1).all()
    big = np.full((3, 2), 1 << 29, np.int64)
    assert SR.dp(big)[1] == SR.MCAP                                     # the cap of M


def test_cell_cost_truncates_and_divides_as_stated():
    P = np.zeros((2, 5, 2, 3), np.float32)
    P[:, 4] = 1.0
    P[0, :3, 0, 0], P[1, :3, 0, 0] = (10.6, 0.0, 300.0), (0.0, 0.7, 0.0)         # 10.6 + 0.7 + 300 = 311.3 -> 311
    P[0, :3, 0, 1], P[1, :3, 0, 1] = (255.0, 255.0, 255.0), (0.0, 0.0, -100.0)   # 865 -> 765
    P[0, 3], P[1, 3] = 3.0, 1.0                                                  # t = 0.5; prior 9 -> 4
    P[1, 4, 1, :] = 0.25                                                         # row 1: no overlap
    d, both = SR.pixel_cost(P[0], P[1], 9.0)
    assert d[0].tolist() == [311 + 4, 765 + 4, 4] and both.tolist() == [[True] * 3, [False] * 3]
    D, nb, E = SR.cell_cost(d, both, 2)
    assert D.tolist() == [[315 + 769, 4]] and nb.tolist() == [[2, 1]] and E.tolist() == [[1084 * 4 // 2, 16]]
    D, nb, E = SR.cell_cost(d, both, 1)
    assert E.tolist() == [[315, 769, 4], [SR.NONE] * 3]
    Ep = SR.energy(E)
    assert Ep.tolist() == [[315, 769, 4], [0, 0, 0]]                             # row 1 is free
    E[1, 2] = 7
    assert SR.energy(E)[1].tolist() == [SR.PEN, SR.PEN, 7]
    assert SR.energy(E, [2, 0], 3)[0].tolist() == [315 + 6, 769 + 3, 4] and SR.energy(E, [2, 0], 65535)[1, 2] == 7 + 2 * 65535
    assert SR.energy(np.zeros((1, 9), np.int32), [0], 65535)[0].tolist() == [0, 65535, 131070, 196605, 262140] + [SR.TCAP] * 4
    P[:, 3] = 0.0
    assert SR.pixel_cost(P[0], P[1], 255.0)[0][0, 2] == 0                         # no weight at all: t = 0


@pytest.mark.parametrize('cell,lo,hi', [(1, 24, 71), (4, 24, 72), (8, 32, 96)])
def test_identical_views_get_the_geometric_seam(cell, lo, hi):
    """The cost is the prior alone, the seam stays inside the overlap, and its labels are the blend's own owner map: the geometric seam
    of side-by-side views is vertical (slope 0), on a cell boundary here (cell 1: at the column where the weights tie)."""
    hc, wc = 40, 128
    P = SR.side_by_side(hc, wc, lo, hi)
    r = SR.seam(P, cell, 0, 255.0)
    xs = r['seams'][0, 0]
    assert r['order'] == [[0, 1]]
    assert (xs * cell >= lo).all() and (xs * cell + cell <= hi + cell - 1).all()
    prior_only = SR.energy(SR.cell_cost(*SR.pixel_cost(np.where(np.arange(5)[:, None, None] < 3, 0, P[0]).astype(np.float32),
                                                       np.where(np.arange(5)[:, None, None] < 3, 0, P[1]).astype(np.float32), 255.0), cell)[2])
    assert r['seam_cost'][0][0] == SR.path_cost(prior_only, xs) == SR.optimum(r['energy'][0][0])
    geo = SR.geometric_owner(P)
    new = SR.geometric_owner(r['P'])
    assert np.array_equal(new, geo)
    assert set(np.unique(r['P'][:, 3])) == {1.0, 2.0}


def test_zero_cost_follows_the_tie_rules():
    """prior = 0 and equal colours: every overlap cell costs 0, so the end point is the first overlap cell of the last row and the seam
    climbs straight from it."""
    P = SR.side_by_side(24, 64, 17, 50)
    for cell in (1, 2, 4):
        r = SR.seam(P, cell, 0, 0.0)
        first = 17 // cell
        assert r['seam_cost'] == [[0]] and r['seams'][0, 0].tolist() == [first] * SR.grid(24, 64, cell)[0], cell
    # an overlap that widens to the left below row 12: the lowest end point that a free path reaches, up along the diagonal, then straight
    P[1, 4, :12, :30] = 0.0
    r = SR.seam(P, 1, 0, 0.0)
    xs = r['seams'][0, 0]
    assert r['seam_cost'] == [[0]] and xs[12:].tolist() == list(range(29, 17, -1))
    assert (xs[:12] == 30).all()


RECT = (20, 44, 52, 76)          # rows 20..43, columns 52..75: cells 5..10 x 13..18 at cell 4, the overlap is cells 8..23


def mismatch_scene(rect=RECT, seed=0):
    return SR.mismatch(64, 128, 32, 96, rect, seed)


def test_mismatch_scene_the_seam_walks_around_the_object():
    P = mismatch_scene()
    y0, y1, x0, x1 = RECT
    assert (x0 - 32) // 4 >= 2 and (96 - x1) // 4 >= 2 and y0 // 4 >= (64 - x0) // 4 - 1         # margins; reachable at slope 1
    geo = SR.geometric_owner(P)
    assert set(np.unique(geo[y0:y1, x0:x1])) == {0, 1}                  # the geometric seam (columns 63 | 64) cuts the rectangle
    r = SR.seam(P, 4, 0, 8.0)
    xs = r['seams'][0, 0]
    colour_only = SR.energy(SR.cell_cost(*SR.pixel_cost(P[0], P[1], 0.0), 4)[2])
    assert SR.path_cost(colour_only, xs) == 0                           # no colour difference anywhere along the seam
    assert r['seam_cost'][0][0] == SR.optimum(r['energy'][0][0])
    own = SR.geometric_owner(r['P'])
    assert len(np.unique(own[y0:y1, x0:x1])) == 1
    k = int(own[y0, x0])
    # the blend of the painted P (bands = 0: the float64 statement without feathering): the rectangle is wholly that view's
    out = MR.blend(r['P'], 0)
    assert np.array_equal(out[:, y0:y1, x0:x1], P[k, :3, y0:y1, x0:x1].astype(np.float64))
    cut = MR.blend(P, 0)
    assert not np.array_equal(cut[:, y0:y1, x0:x1], P[0, :3, y0:y1, x0:x1]) and not np.array_equal(cut[:, y0:y1, x0:x1], P[1, :3, y0:y1, x0:x1])


def test_temporal_term_holds_or_releases_the_seam():
    hc, wc, c = 64, 128, 4
    A = SR.side_by_side(hc, wc, 32, 96)                                 # frame 1: nothing in the way
    B = mismatch_scene()                                                # frame 2: the object stands on frame 1's seam
    fresh_b = SR.seam(B, c, 0, 8.0)['seams'][0, 0]
    for mu, want_hold in ((65535, True), (0, False)):
        st = SR.fresh_state(2, hc, wc, c)
        a = SR.seam(A, c, mu, 8.0, st)['seams'][0, 0].copy()
        assert st[:8].tolist() == [1, 2, 16, 32, 4, 0, 1, -1] and np.array_equal(st[SR.HEADER:], a)
        b = SR.seam(B, c, mu, 8.0, st)['seams'][0, 0]
        assert np.array_equal(b, a) == want_hold and np.array_equal(b, fresh_b) == (not want_hold)
        assert np.array_equal(st[SR.HEADER:], b)
    assert not np.array_equal(fresh_b, SR.seam(A, c, 0, 8.0)['seams'][0, 0])
    # two frames in one call = two calls; no state = no temporal term
    st1, st2 = SR.fresh_state(2, hc, wc, c), SR.fresh_state(2, hc, wc, c)
    both = SR.seam(np.stack([A, B]), c, 300, 8.0, st1)
    one = [SR.seam(X, c, 300, 8.0, st2) for X in (A, B)]
    assert np.array_equal(both['seams'], np.stack([o['seams'][0] for o in one])) and np.array_equal(st1, st2)
    assert np.array_equal(SR.seam(np.stack([A, B]), c, 65535, 8.0)['seams'][1, 0], fresh_b)


def test_a_grid_or_order_change_drops_the_temporal_term():
    A, B = SR.side_by_side(64, 128, 32, 96), mismatch_scene()
    st = np.zeros(SR.HEADER + 64, np.int32)
    SR.seam(A, 4, 65535, 8.0, st)
    got = SR.seam(B, 2, 65535, 8.0, st)['seams'][0, 0]                  # another cell size: the stored seam is of another grid
    assert np.array_equal(got, SR.seam(B, 2, 0, 8.0)['seams'][0, 0]) and st[:5].tolist() == [1, 2, 32, 64, 2]
    st = SR.fresh_state(2, 64, 128, 4)
    SR.seam(A[::-1], 4, 65535, 8.0, st)                                 # the views swapped: order [1, 0]
    assert st[5:8].tolist() == [1, 0, -1]
    got = SR.seam(B, 4, 65535, 8.0, st)['seams'][0, 0]
    assert np.array_equal(got, SR.seam(B, 4, 0, 8.0)['seams'][0, 0]) and st[5:8].tolist() == [0, 1, -1]


def three_views(hc=48, wc=160):
    """Three views of one picture side by side: columns 0..69, 45..114, 90..159."""
    P = np.zeros((3, 5, hc, wc), np.float32)
    for v, (lo, hi) in enumerate(((0, 70), (45, 115), (90, 160))):
        P[v, :3, :, lo:hi] = SR.texture(hc, wc)[:, :, lo:hi]
        P[v, 3, :, lo:hi] = SR.weight_plane(hc, hi - lo)
        P[v, 4, :, lo:hi] = 1.0
    return P


def test_three_view_order_comes_out_of_the_extents():
    P = three_views()
    base = SR.seam(P, 4, 0, 8.0)
    assert base['order'] == [[0, 1, 2]] and set(np.unique(base['P'][:, 3])) == {1.0, 2.0, 3.0}
    assert (base['seams'][0, 1] >= base['seams'][0, 0]).all()
    own = SR.geometric_owner(base['P'])
    assert (own[:, :45] == 0).all() and (own[:, 70:90] == 1).all() and (own[:, 115:] == 2).all()
    for perm in itertools.permutations(range(3)):
        Q = P[list(perm)]                                               # view perm[i] is given as index i
        r = SR.seam(Q, 4, 0, 8.0)
        assert r['order'] == [[perm.index(v) for v in range(3)]]
        assert np.array_equal(r['seams'], base['seams']) and np.array_equal(r['P'], base['P'][list(perm)])
    # equal keys: the lower index first
    Q = P.copy()
    Q[2] = Q[0]
    assert SR.seam(Q, 4, 0, 8.0)['order'] == [[0, 2, 1]]


def test_empty_overlap_and_empty_view():
    P = SR.side_by_side(30, 90, 50, 40)                                 # columns 40..49 are nobody's: no overlap cell in any row
    P[0, 4, :, 40:] = 0.0
    r = SR.seam(P, 4, 200, 8.0, SR.fresh_state(2, 30, 90, 4))
    assert r['seam_cost'] == [[0]] and not r['seams'].any() and all((c[2] == SR.NONE).all() for c in r['cost'][0])
    valid = P[:, 4] >= 0.5
    own = SR.geometric_owner(r['P'])
    assert (own[valid[0]] == 0).all() and (own[valid[1]] == 1).all()      # validity decides where the views do not meet
    E = P.copy()
    E[1, 4] = 0.0                                                       # view 1 has no valid pixel: key +inf
    r = SR.seam(E, 4, 0, 8.0)
    assert r['order'] == [[0, 1]] and r['seam_cost'] == [[0]]
    E = P.copy()
    E[0, 4] = 0.0
    assert SR.seam(E, 4, 0, 8.0)['order'] == [[1, 0]]
    T3 = three_views()
    T3[1, 4] = 0.0                                                      # the middle view missing: the outer ones do not overlap here
    r = SR.seam(T3, 4, 0, 8.0)
    assert r['order'] == [[0, 2, 1]] and r['seam_cost'] == [[0, 0]]
    assert np.isfinite(MR.blend(r['P'], 2)).all()


def test_the_scenes_of_the_gpu_sweep_are_what_they_claim():
    """The made-up inputs of tests/test_gpu_seam.py's sweep of the indexing, on the restatement alone: the cap scene reaches M's cap
    (and only in its second frame), and on grids of more than 256 rows of cells an object over the middle third of the rows moves the
    seam in rows below 256 only, one over the last third in rows past 256 -- where the temporal term then holds the next frame."""
    P = SR.cap_scene()
    assert P.shape == (2, 2, 5, 4200, 8) and SR.lds_bytes(4200, 8, 1) == 58928
    r = SR.seam(P, 1, 65535, 8.0, SR.fresh_state(2, 4200, 8, 1))
    assert r['order'] == [[0, 1], [0, 1]] and r['seam_cost'] == [[88143], [SR.MCAP]]
    assert SR.optimum(r['energy'][0][0]) == 88143 and SR.optimum(r['energy'][1][0]) == 1101092922
    for (hc, wc), cell in (((300, 61), 1), ((530, 37), 2)):
        lo, hi, rect_x = wc // 4, 3 * wc // 4, (wc // 2 - wc // 8, wc // 2 + wc // 8)
        A = SR.side_by_side(hc, wc, lo, hi)
        last = {}
        for where, rows in (('middle', (hc // 3, 2 * hc // 3)), ('last', (2 * hc // 3, hc))):
            s = SR.seam(np.stack([A, SR.mismatch(hc, wc, lo, hi, rows + rect_x), A]), cell, 48 * cell, 8.0,
                        SR.fresh_state(2, hc, wc, cell))['seams'][:, 0]
            assert s.shape[1] > 256
            last[where] = (np.flatnonzero(s[0] != s[1]).max(), np.flatnonzero(s[2] != s[0]).max())
        assert max(last['middle']) < 256 <= min(last['last']), last
