"""MULTIBAND's content-aware seam on the GPU (libstabstitch_seam.so): the three kernels against the integer restatement
of tests/seam_ref.py bit for bit on P of real warps, the call shapes, the blend with a painted seam, the unchanged geometric seam, the
streaming stitchers and the pipeline under seam='dp' against the ops render of their own splines fed the same state sequence, and the
scene the feature is for: an object only one camera sees, standing on the geometric seam.  The kernels again where their indexing
changes -- several tile columns of the cost pass at cells above 1, grids of more than 256 rows of cells, the cap on M, a P that is not
16-byte aligned -- and the uint8 and long-video routes of the pipeline with bands= and either seam.  Every comparison is exact.
    python -m pytest tests -m gpu"""
import functools
import gc

import numpy as np
import pytest
import torch

import seam_ref as SR
import sweep_inputs as G
from test_gpu_parity import dev, hip_nets  # noqa: F401  (fixtures)
from test_gpu_multiband import PUSHES, SH, SW, _clip, _make, _push_all, _same, _same_lists

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
T = torch.from_numpy


@pytest.fixture(autouse=True)
def _no_garbage_inside_a_capture():
    gc.collect()
    yield
    gc.collect()


@functools.lru_cache(maxsize=None)
def _warp_inputs(size, views, frames, seed):
    h, w, hc, wc = size
    U, src, tgt = G.warp_case(frames * views, h, w, hc, wc, seed=seed)
    return np.ascontiguousarray(U[:, :3]), src, tgt


def _warped(dev, size, views, frames=1, seed=11, perm=None):
    """P [frames,views,5,hc,wc] of a real warp by the library's own ss_tps_warp_mask_nchw, the views of every frame reordered by perm."""
    from stabstitch2_amd import ops
    h, w, hc, wc = size
    U3, src, tgt = _warp_inputs(size, views, frames, seed)
    idx = np.arange(frames * views).reshape(frames, views)
    if perm is not None:
        idx = idx[:, list(perm)]
    idx = idx.reshape(-1)
    sd = T(src[idx]).to(dev)
    U = ops.multiband_stack([T(np.ascontiguousarray(U3[idx][v::views])).to(dev) for v in range(views)])
    P = ops.tps_warp(U, sd, ops.tps_solve(sd, T(tgt[idx]).to(dev)), hc, wc, 'NORMAL', with_mask=True)
    return P.view(frames, views, 5, hc, wc)


def _parts(ws, frames, views, hc, wc, cell):
    from stabstitch2_amd import _seam
    lay = _seam.layout(frames, views, hc, wc, cell)
    assert ws.numel() == lay['ints']
    host = ws.cpu().numpy()
    return {k: host[lay[k][0]:lay[k][0] + int(np.prod(lay[k][1]))].reshape(lay[k][1]) for k in lay if k != 'ints'}


def _against_the_restatement(dev, P, cell, mu, prior, with_state=True):
    """One call over all frames of P on the device against seam_ref on its host copy: cost planes, order, seams, their cost, the
    painted planes, the state.  -> the reference's result."""
    from stabstitch2_amd import ops
    n, v, _, hc, wc = P.shape
    Ph = P.cpu().numpy()
    hq, wq = SR.grid(hc, wc, cell)
    state = ops.seam_state(v, hc, wc, cell, dev) if with_state else None
    ws = ops.seam_workspace(n, v, hc, wc, cell, dev)
    ws.fill_(-7)
    got = ops.multiband_seam(P.clone(), cell, mu, prior, state, ws=ws)
    ref_state = SR.fresh_state(v, hc, wc, cell) if with_state else None
    ref = SR.seam(Ph, cell, mu, prior, ref_state)
    parts = _parts(ws, n, v, hc, wc, cell)
    for f in range(n):
        for p, (D, nb, E) in enumerate(ref['cost'][f]):
            for k, want in enumerate((D, nb, E)):
                assert np.array_equal(parts['cost'][f, p, k, :, :wq], want), ('cost', f, p, 'D nb E'.split()[k])
        assert parts['meta'][f, :3].tolist() == ref['order'][f] + [-1] * (3 - v), ('order', f)
        assert parts['meta'][f, 3:3 + v - 1].tolist() == ref['seam_cost'][f], ('seam cost', f)
        for p in range(v - 1):
            if ref['seam_cost'][f][p] == SR.MCAP:                  # M is capped, the optimum is uncapped int64
                assert SR.optimum(ref['energy'][f][p]) >= SR.MCAP, ('optimum at the cap', f, p)
            else:
                assert ref['seam_cost'][f][p] == SR.optimum(ref['energy'][f][p]), ('optimum', f, p)
    assert np.array_equal(parts['seams'], ref['seams'])
    assert np.array_equal(got.cpu().numpy(), ref['P'])
    if with_state:
        assert np.array_equal(state.cpu().numpy(), ref_state)
    return ref


# ================================================================================================ the kernels against the restatement
CASES = [  # (frame h, w, canvas hc, wc), views, cell, frames, view order
    ((72, 96, 37, 61), 2, 1, 1, None), ((72, 96, 37, 61), 2, 2, 1, None), ((72, 96, 37, 61), 2, 4, 1, None),      # partial edge cells
    ((72, 96, 37, 61), 3, 2, 1, (2, 0, 1)),
    ((72, 96, 81, 129), 2, 4, 5, None), ((72, 96, 81, 129), 3, 4, 5, (1, 2, 0)), ((72, 96, 81, 129), 3, 8, 1, (2, 1, 0)),
    ((72, 96, 81, 129), 2, 16, 1, None),
    ((36, 48, 7, 67), 2, 8, 5, None), ((36, 48, 7, 67), 3, 8, 1, None),                                          # hq = 1
    ((36, 1500, 13, 2100), 2, 1, 1, None), ((36, 1500, 13, 2100), 3, 1, 5, (0, 2, 1)),                                # wq > 4 x 256 columns
]


@pytest.mark.parametrize('size,views,cell,frames,perm', CASES,
                         ids=lambda x: 'x'.join(map(str, x)) if isinstance(x, tuple) else str(x))
def test_kernels_equal_the_restatement(dev, size, views, cell, frames, perm):
    P = _warped(dev, size, views, frames, perm=perm)
    hc, wc = size[2:]
    ref = _against_the_restatement(dev, P, cell, 48 * cell, 8.0)
    assert ref['seams'].shape == (frames, views - 1, SR.grid(hc, wc, cell)[0])
    assert any((nb > 0).any() for f in ref['cost'] for _, nb, _ in f)          # some overlap somewhere
    _against_the_restatement(dev, P, cell, 0, 255.0, with_state=False)


def test_view_order_follows_the_extents_on_the_device(dev):
    size = (72, 96, 81, 129)
    base = _against_the_restatement(dev, _warped(dev, size, 3), 4, 0, 8.0)
    for perm in ((1, 0, 2), (2, 1, 0), (1, 2, 0)):
        r = _against_the_restatement(dev, _warped(dev, size, 3, perm=perm), 4, 0, 8.0)
        assert r['order'][0] == [perm.index(v) for v in base['order'][0]]
        assert np.array_equal(r['seams'], base['seams'])


def test_made_up_scenes_on_the_device(dev):
    """Without a warp: the mismatch scene, an empty overlap, an empty view -- and a held seam (mu at its maximum) across two calls."""
    A, B = SR.side_by_side(64, 128, 32, 96), SR.mismatch(64, 128, 32, 96, (20, 44, 52, 76))
    for Ph in (A, B, np.stack([A, B, A])):
        P = T(Ph if Ph.ndim == 5 else Ph[None]).to(dev)
        _against_the_restatement(dev, P, 4, 65535, 8.0)
        _against_the_restatement(dev, P, 2, 7, 0.0)
    E = A.copy()
    E[1, 4] = 0.0
    N = SR.side_by_side(30, 90, 50, 40)
    N[0, 4, :, 40:] = 0.0
    for Ph in (E, N):
        _against_the_restatement(dev, T(Ph[None]).to(dev), 4, 200, 8.0)


# ================================================================================================ where the indexing changes
def _tile_columns(nb, cell):
    """The tile columns of the cost pass (SSM_TILE_W = 256 canvas columns each) that hold an overlap cell of the plane nb."""
    return sorted({int(cx) * cell // 256 for cx in np.flatnonzero((nb > 0).any(0))})


WIDE_CASES = [  # canvases over 256 columns at every cell size above 1: three tile columns, several tile rows
    ((36, 400, 37, 530), 2, 2, 1, None), ((36, 400, 37, 530), 3, 4, 5, (2, 0, 1)),
    ((72, 520, 81, 700), 2, 8, 1, None), ((72, 520, 81, 700), 3, 16, 5, (1, 2, 0)),
]


@pytest.mark.parametrize('size,views,cell,frames,perm', WIDE_CASES,
                         ids=lambda x: 'x'.join(map(str, x)) if isinstance(x, tuple) else str(x))
def test_kernels_equal_the_restatement_over_several_tile_columns(dev, size, views, cell, frames, perm):
    """cx0 = x0 >> shift with x0 > 0, the row flags of three tiles per row of cells and their OR, the extents of gx * gy tiles: frames
    wider than half the canvas, so that any two views overlap wherever the warp puts them."""
    hc, wc = size[2:]
    gx, gy = -(-wc // 256), -(-hc // max(4, cell))
    assert cell > 1 and gx == 3 and gy > 1
    P = _warped(dev, size, views, frames, perm=perm)
    ref = _against_the_restatement(dev, P, cell, 48 * cell, 8.0)
    assert ref['seams'].shape == (frames, views - 1, SR.grid(hc, wc, cell)[0])
    assert any((nb > 0).any() for f in ref['cost'] for _, nb, _ in f)          # some overlap somewhere
    held = sorted({t for f in ref['cost'] for _, nb, _ in f for t in _tile_columns(nb, cell)})
    print('\n[seam claim] %d x %d, V = %d, cell %d: gx %d, gy %d, overlap cells in the tile columns %s' % (hc, wc, views, cell, gx, gy, held))
    assert any(t > 0 for t in held)                                            # ... and some of it past the first tile column
    _against_the_restatement(dev, P, cell, 0, 255.0, with_state=False)


@pytest.mark.parametrize('cell', [2, 4, 16])
def test_made_up_scenes_on_either_side_of_a_tile_boundary(dev, cell):
    """Without a warp, on 37 x 530: an overlap that lies wholly in tile column 1 (every cell of tile columns 0 and 2 is NONE, the
    rows are not free), and one that straddles the boundary at column 256 with the object on it; two frames per call, so that with a
    state the second runs under the temporal term."""
    first = 256 // cell                                                       # the first cell column of tile column 1
    inside = SR.side_by_side(37, 530, 300, 420)
    across = SR.mismatch(37, 530, 200, 330, (12, 25, 240, 280))
    for with_state in (True, False):
        for name, scene in (('inside', inside), ('across', across)):
            P = T(np.stack([scene, scene])).to(dev)
            ref = _against_the_restatement(dev, P, cell, 48 * cell, 8.0, with_state=with_state)
            nb = ref['cost'][0][0][1]
            cols = np.flatnonzero((nb > 0).any(0))
            print('\n[seam claim] %s at cell %d%s: overlap cells in columns %d..%d, tile columns %s (tile column 1 starts at cell %d)'
                  % (name, cell, '' if with_state else ', no state', cols.min(), cols.max(), _tile_columns(nb, cell), first))
            if name == 'inside':
                assert cols.min() >= first and _tile_columns(nb, cell) == [1]      # no overlap cell has cx < 256 >> shift
            else:
                assert cols.min() < first <= cols.max() and _tile_columns(nb, cell) == [0, 1]


TALL_CASES = [((300, 61), 1, (320, 48)), ((530, 37), 2, (640, 30))]          # canvas, cell, the frame of the real warp (taller than the
#                                                                               canvas: every view reaches the rows of the second trip)


@pytest.mark.parametrize('canvas,cell,frame', TALL_CASES, ids=lambda x: 'x'.join(map(str, x)) if isinstance(x, tuple) else str(x))
def test_grids_of_more_than_256_rows_of_cells(dev, canvas, cell, frame):
    """hq = 300 and 265: every `for (y = tid; y < hq; y += 256)` loop of the dp kernel takes a second trip -- the xprev load, rowany,
    the seam and the state stores.  Frames A, B, A (B: an object only view 1 sees, on the geometric seam) in one call with a state and
    again as three calls.  With the object over the middle third of the rows the seams of A and B differ in rows 106..204 (87..177)
    only -- a seam leaves its column by one cell per row and is back long before row 256 -- so the object also stands over the last
    third: there the seams differ in rows >= 256, and the third frame, A again, is held to B's seam there by the temporal term."""
    from stabstitch2_amd import ops
    hc, wc = canvas
    hq = SR.grid(hc, wc, cell)[0]
    assert hq > 256 and SR.lds_bytes(hc, wc, cell) < 9 * 1024
    lo, hi, mu = wc // 4, 3 * wc // 4, 48 * cell
    x0, x1 = wc // 2 - wc // 8, wc // 2 + wc // 8
    A = SR.side_by_side(hc, wc, lo, hi)
    for where, rows in (('middle', (hc // 3, 2 * hc // 3)), ('last', (2 * hc // 3, hc))):
        clip = np.stack([A, SR.mismatch(hc, wc, lo, hi, rows + (x0, x1)), A])
        P = T(clip).to(dev)
        ref = _against_the_restatement(dev, P, cell, mu, 8.0)                  # one call: seams, painted planes, the state after it
        seams = ref['seams'][:, 0]
        differ, held = np.flatnonzero(seams[0] != seams[1]), np.flatnonzero(seams[2] != seams[0])
        print('\n[seam claim] %d x %d at cell %d, hq = %d, the object over the %s third: the seams of A and B differ in rows %d..%d, '
              'the held A and the fresh A in rows %d..%d' % (hc, wc, cell, hq, where, differ.min(), differ.max(), held.min(), held.max()))
        assert differ.size and held.size
        if where == 'last':
            assert differ.max() >= 256 and held.max() >= 256
        state, ref_state = ops.seam_state(2, hc, wc, cell, dev), SR.fresh_state(2, hc, wc, cell)
        SR.seam(clip, cell, mu, 8.0, ref_state)
        for f in range(3):                                                     # three calls
            assert np.array_equal(ops.multiband_seam(P[f].clone(), cell, mu, 8.0, state).cpu().numpy(), ref['P'][f]), (where, f)
        assert np.array_equal(state.cpu().numpy(), ref_state) and (ref_state[SR.HEADER + 256:] > 0).all()
    P = _warped(dev, frame + canvas, 2, 3)
    ref = _against_the_restatement(dev, P, cell, mu, 8.0)
    assert any((nb[256:] > 0).any() for f in ref['cost'] for _, nb, _ in f)    # overlap in the rows of the second trip
    _against_the_restatement(dev, P, cell, 0, 255.0, with_state=False)


def test_the_cap_on_M(dev):
    """SM_MCAP on the device: frame 1 is held at mu = 65535 to frame 0's seam at column 0, six columns away from its own overlap; M
    saturates at 1 << 30 some 4000 rows down, and from there every M of a row ties: straight, then left, then right, and the lowest
    x of the last row decide the seam."""
    hc, wc = 4200, 8
    assert SR.lds_bytes(hc, wc, 1) == 58928
    ref = _against_the_restatement(dev, T(SR.cap_scene()).to(dev), 1, 65535, 8.0)
    print('\n[seam claim] 4200 x 8 at cell 1: order %s, seam costs %s, the uncapped optimum of frame 1 %d'
          % (ref['order'], ref['seam_cost'], SR.optimum(ref['energy'][1][0])))
    assert ref['order'] == [[0, 1], [0, 1]] and ref['seam_cost'][0] == [88143]
    assert ref['seam_cost'][1] == [SR.MCAP] and SR.optimum(ref['energy'][1][0]) == 1101092922


@pytest.mark.parametrize('size,views,frames', [((72, 96, 37, 64), 2, 1), ((72, 96, 81, 128), 3, 2)],
                         ids=lambda x: 'x'.join(map(str, x)) if isinstance(x, tuple) else str(x))
def test_an_unaligned_P_takes_the_scalar_loads(dev, size, views, frames):
    """P at 4, 8 and 12 bytes past a 16-byte boundary (al4 == false: four scalar loads per quad) on canvases whose rows are whole quads,
    where the aligned call takes the 16-byte loads: the same painted planes, workspace and state, bit for bit, in place, and nothing
    written in front of P or behind it."""
    from stabstitch2_amd import ops
    from test_gpu_rest_sweeps import canaried, canaries_intact
    hc, wc = size[2:]
    cell, mu = 4, 192
    P = _warped(dev, size, views, frames).contiguous()
    assert wc % 4 == 0 and P.data_ptr() % 16 == 0
    ref = _against_the_restatement(dev, P, cell, mu, 8.0)
    assert any((nb > 0).any() for f in ref['cost'] for _, nb, _ in f)
    state = ops.seam_state(views, hc, wc, cell, dev)
    ws = ops.seam_workspace(frames, views, hc, wc, cell, dev).fill_(-7)
    want = ops.multiband_seam(P.clone(), cell, mu, 8.0, state, ws=ws)
    n, residues = P.numel(), []
    for off in (1, 2, 3):
        buf, mid = canaried(n + 4, dev)
        view = mid[off:off + n].view(P.shape)
        view.copy_(P)
        residues.append(view.data_ptr() % 16)
        assert view.data_ptr() % 16 != 0 and view.is_contiguous()
        state_u = ops.seam_state(views, hc, wc, cell, dev)
        ws_u = ops.seam_workspace(frames, views, hc, wc, cell, dev).fill_(-7)
        got = ops.multiband_seam(view, cell, mu, 8.0, state_u, ws=ws_u)
        assert got.data_ptr() == view.data_ptr() and torch.equal(got, want), off
        assert torch.equal(ws_u, ws) and torch.equal(state_u, state), off
        assert np.array_equal(got.cpu().numpy(), ref['P']), off
        canaries_intact(buf, n + 4, 'multiband_seam at float offset %d' % off)
        assert bool((mid[:off] == 7.0).all()) and bool((mid[off + n:] == 7.0).all()), off
    print('\n[seam claim] %d x %d, V = %d: data_ptr() %% 16 of the aligned P 0, of the views %s' % (hc, wc, views, residues))
    assert residues == [4, 8, 12]


# ================================================================================================ the call shapes
@pytest.mark.parametrize('views', [2, 3])
def test_frames_in_one_call_equal_one_call_per_frame(dev, views):
    from stabstitch2_amd import ops
    size = (72, 96, 81, 129)
    hc, wc = size[2:]
    P = _warped(dev, size, views, 5)
    s1, s2 = ops.seam_state(views, hc, wc, 4, dev), ops.seam_state(views, hc, wc, 4, dev)
    together = ops.multiband_seam(P.clone(), 4, 300, 8.0, s1)
    for f in range(5):
        _same(ops.multiband_seam(P[f].clone(), 4, 300, 8.0, s2), together[f], ('frame', f))
    assert torch.equal(s1, s2) and int(s1[0]) == 1
    # no state: no temporal term, whatever mu is
    _same(ops.multiband_seam(P.clone(), 4, 65535, 8.0), ops.multiband_seam(P.clone(), 4, 0, 8.0), 'state=None')
    held = ops.multiband_seam(P.clone(), 4, 65535, 8.0, ops.seam_state(views, hc, wc, 4, dev))
    assert not torch.equal(held, ops.multiband_seam(P.clone(), 4, 0, 8.0))              # (with a state mu does something)
    # a state of another grid is ignored and overwritten; the defaults are cell 4, mu 192, prior 8
    big = s1.new_zeros(200)
    big[:s1.numel()] = s1
    _same(ops.multiband_seam(P[0].clone(), 2, 65535, 8.0, big), ops.multiband_seam(P[0].clone(), 2, 0, 8.0), 'grid change')
    assert big[:5].tolist() == [1, views, 41, 65, 2]
    _same(ops.multiband_seam(P[0].clone()), ops.multiband_seam(P[0].clone(), 4, 192, 8.0), 'defaults')
    with pytest.raises(ValueError, match='state'):
        ops.multiband_seam(P[0].clone(), 4, 0, 8.0, s1[:10].clone())
    with pytest.raises(ValueError, match='cell'):
        ops.multiband_seam(P[0].clone(), 3)


# ================================================================================================ the blend with a painted seam
@pytest.mark.parametrize('views', [2, 3])
def test_render_with_the_dp_seam_is_the_blend_of_the_painted_planes(dev, views):
    """ops.render_multiband(seam='dp') == ops.multiband_blend of P with the REFERENCE-painted weights, fp32 and uint8, a frame and a
    clip with a state; seam='geometric' == the call without the argument, and launches nothing of the new library."""
    from stabstitch2_amd import ops, _seam
    size = (72, 96, 81, 129)
    h, w, hc, wc = size
    n = 3
    U3, src, tgt = _warp_inputs(size, views, n, 12)
    u8 = np.clip(np.rint(U3), 0, 255).astype(np.uint8)
    sd = T(src).to(dev)
    src_c, T_c = sd.view(n, views, 63, 2), ops.tps_solve(sd, T(tgt).to(dev)).view(n, views, 2, 66)
    frames = T(np.ascontiguousarray(u8.transpose(0, 2, 3, 1))).to(dev).view(n, views, h, w, 3)
    clips_u8 = [frames[:, v].contiguous() for v in range(views)]
    clips = [ops.ingest_u8(c)[0] for c in clips_u8]
    P = ops.tps_warp(ops.multiband_stack(clips), sd, T_c.view(n * views, 2, 66), hc, wc, 'NORMAL', with_mask=True).view(n, views, 5, hc, wc)
    ref = SR.seam(P.cpu().numpy(), 4, 100, 8.0, SR.fresh_state(views, hc, wc, 4))
    painted = T(ref['P']).to(dev)
    kw = dict(seam='dp', seam_cell=4, seam_mu=100, seam_prior=8.0)
    want, want8 = ops.multiband_blend(painted, 3), ops.multiband_blend(painted, 3, u8=True)
    _same(ops.render_multiband(clips, src_c, T_c, hc, wc, 'NORMAL', 3, seam_state=ops.seam_state(views, hc, wc, 4, dev), **kw), want, 'clip')
    _same(ops.render_multiband(clips_u8, src_c, T_c, hc, wc, 'NORMAL', 3, seam_state=ops.seam_state(views, hc, wc, 4, dev), **kw), want8,
          'clip u8')
    st = ops.seam_state(views, hc, wc, 4, dev)
    for f in range(n):
        _same(ops.render_multiband([c[f] for c in clips], src_c[f], T_c[f], hc, wc, 'NORMAL', 3, seam_state=st, **kw), want[f], ('frame', f))
    geo = ops.render_multiband(clips, src_c, T_c, hc, wc, 'NORMAL', 3)
    assert not torch.equal(geo, want)

    def no_launch(*a, **k):
        raise AssertionError('the geometric seam launched from libstabstitch_seam.so')
    real = _seam.call
    _seam.call = no_launch
    try:
        _same(ops.render_multiband(clips, src_c, T_c, hc, wc, 'NORMAL', 3, seam='geometric'), geo, 'geometric')
        _same(ops.render_multiband(clips_u8, src_c, T_c, hc, wc, 'NORMAL', 3, seam='geometric'),
              ops.render_multiband(clips_u8, src_c, T_c, hc, wc, 'NORMAL', 3), 'geometric u8')
        with pytest.raises(AssertionError, match='launched'):
            ops.render_multiband(clips, src_c, T_c, hc, wc, 'NORMAL', 3, seam='dp')
    finally:
        _seam.call = real
    for bad in (dict(seam='graphcut'), dict(seam=None), dict(seam_cell=4), dict(seam='geometric', seam_mu=3),
                dict(seam='dp', seam_cell=3), dict(seam='dp', seam_mu=-1), dict(seam='dp', seam_prior=300.0)):
        with pytest.raises(ValueError):
            ops.render_multiband(clips, src_c, T_c, hc, wc, 'NORMAL', 3, **bad)


# ================================================================================================ the scene the feature is for
def test_an_object_on_the_geometric_seam_stays_whole(dev):
    """Two cameras 32 columns apart see one picture, except for an object (a rectangle of another colour) that only camera 1 sees,
    standing where the geometric seam runs.  Through the real warp (pure shifts) and the real blend: with seam='dp' the rectangle in
    the output is one view's pixels, every one; with seam='geometric' it is cut -- part one view's, part the other's."""
    from stabstitch2_amd import ops
    h, w, hc, wc, shift = 64, 96, 64, 128, 32
    y0, y1, x0, x1 = 20, 44, 52, 76
    world = SR.texture(hc, wc, seed=3)
    v0, v1 = world[:, :, :w].copy(), world[:, :, shift:shift + w].copy()
    v1[:, y0:y1, x0 - shift:x1 - shift] = np.array([250.0, 5.0, 250.0], np.float32)[:, None, None]
    r = np.repeat(G.rigid_px(h, w), 2, axis=0)
    m = r.copy()
    m[1, ..., 0] += shift
    src, tgt = T(G.norm_px(m, hc, wc)).to(dev), T(G.norm_px(r, h, w)).to(dev)
    Tk = ops.tps_solve(src, tgt)
    imgs = [T(v0).to(dev), T(v1).to(dev)]
    P = ops.tps_warp(ops.multiband_stack(imgs), src, Tk, hc, wc, 'NORMAL', with_mask=True).cpu().numpy()
    inner = (slice(None), slice(y0 + 1, y1 - 1), slice(x0 + 1, x1 - 1))
    assert np.abs(P[0, :3][inner] - P[1, :3][inner]).sum(0).min() > 100                   # the object is in view 1 only
    as_view = [np.clip((P[0, :3] - P[1, :3]).astype(np.float32) + P[1, :3], 0, 255)[inner], P[1, :3][inner]]      # the blend's own fp32 form at bands = 0
    dp = ops.render_multiband(imgs, src, Tk, hc, wc, 'NORMAL', 0, seam='dp', seam_cell=4).cpu().numpy()
    geo = ops.render_multiband(imgs, src, Tk, hc, wc, 'NORMAL', 0, seam='geometric').cpu().numpy()
    assert sum(np.array_equal(dp[inner], a) for a in as_view) == 1
    assert not any(np.array_equal(geo[inner], a) for a in as_view)
    cut = [(geo[inner] == a).all(0) for a in as_view]
    assert cut[0].any() and cut[1].any() and (cut[0] | cut[1]).all()                   # the geometric seam: some of each


# ================================================================================================ the stitchers
KW = dict(seam='dp', seam_cell=4, seam_mu=150, seam_prior=8.0)


def _ops_kw():
    return dict(seam='dp', seam_cell=4, seam_mu=150, seam_prior=8.0)


def _dp_reference(dev, nets, views):
    """PUSHES deterministic pushes through the seam='dp' stitcher, once per view count -> its frames."""
    from test_gpu_multiband import _runs
    key = ('seam', views)
    if key not in _runs:
        st = _make(nets, views, deterministic=True, bands=3, **KW)
        _runs[key] = _push_all(st, dev, views)
        assert len(_runs[key]) == PUSHES and st._direct() and st.graph is not None and st.mode.seam['seam'] == 'dp'
    return _runs[key]


@pytest.mark.parametrize('views', [2, 3])
def test_stream_frames_are_the_dp_render_of_their_own_splines(dev, hip_nets, views, monkeypatch):
    """Every frame a seam='dp' stitcher hands out (the window's seven, then five behind the captured graph) == ops.render_multiband
    on the stitcher's own splines of that frame, fed one state through the same sequence; and it is not the geometric stream."""
    from stabstitch2_amd import online, ops
    c = _clip(dev)
    Cls = online.OnlineStitcher if views == 2 else online.ThreeViewOnlineStitcher
    st = _make(hip_nets, views, bands=3, **KW)
    solved = []
    inner = online._Stitcher._render_solved

    def spy(self, imgs, src, Tk, *a, **kw):
        solved.append((src.clone(), Tk.clone()))
        return inner(self, imgs, src, Tk, *a, **kw)
    monkeypatch.setattr(Cls, '_render_solved', spy)
    state, emitted, differs = None, 0, 0
    for t in range(PUSHES):
        solved.clear()
        got = st.push(*([c['hr'][v, t:t + 1] for v in range(views)] + [c['lr'][v, t:t + 1] for v in range(views)]))
        if not got:
            continue
        if state is None:
            state = ops.seam_state(views, st.hc, st.wc, 4, dev)
        splines, frames_t = (list(solved), range(7)) if len(got) == 7 else ([st._deferred[:2]], [t])
        for (src, Tk), ft, frame in zip(splines, frames_t, got):
            imgs = [c['hr'][v, ft] for v in range(views)]
            want = ops.render_multiband(imgs, src, Tk, st.hc, st.wc, 'NORMAL', 3, seam_state=state, **_ops_kw())
            assert frame.shape == (3, st.hc, st.wc) and torch.equal(frame, want), (views, t, ft)
            differs += not torch.equal(frame, ops.render_multiband(imgs, src, Tk, st.hc, st.wc, 'NORMAL', 3))
            emitted += 1
    assert emitted == PUSHES and st.graph is not None and st._direct() and differs > 0
    assert torch.equal(st.mode._seam_state[1], state)


@pytest.mark.parametrize('views', [2, 3])
def test_push_u8_and_push_many_equal_the_pushes_with_the_dp_seam(dev, hip_nets, views):
    from stabstitch2_amd import ops
    c = _clip(dev)
    ref = _dp_reference(dev, hip_nets, views)
    ref8 = [ops.canvas_to_u8(f[None])[0] for f in ref]
    _same_lists(_push_all(_make(hip_nets, views, deterministic=True, bands=3, **KW), dev, views, u8=True), ref8, 'push_u8')
    for u8 in (False, True):
        many = _make(hip_nets, views, deterministic=True, bands=3, **KW)
        got = []
        for t in range(0, PUSHES, 4):
            if u8:
                got += many.push_many_u8(*[c['u8'][v, t:t + 4] for v in range(views)])
            else:
                got += many.push_many(*([c['hr'][v, t:t + 4] for v in range(views)] + [c['lr'][v, t:t + 4] for v in range(views)]))
        _same_lists(got, ref8 if u8 else ref, 'push_many u8=%s' % u8)


def test_a_regrown_canvas_starts_from_a_fresh_state(dev, hip_nets):
    """grow='recapture' under a cropped canvas: the first frame on the grown canvas is rendered with a fresh state, the ones after it
    with that state carried on."""
    from stabstitch2_amd import ops
    c = _clip(dev)
    probe = _make(hip_nets, 2)
    _push_all(probe, dev, 2, n=7)
    bb = [float(x) for x in probe.bbox.cpu()]
    crop = [bb[0], bb[1] - 0.10 * (bb[1] - bb[0]), bb[2], bb[3]]
    st = _make(hip_nets, 2, canvas=crop, grow='recapture', bands=3, seam='dp', seam_cell=4, seam_mu=65535)
    size, state, checked, regrown = None, None, 0, 0
    for t in range(PUSHES):
        got = st.push(c['hr'][0, t:t + 1], c['hr'][1, t:t + 1], c['lr'][0, t:t + 1], c['lr'][1, t:t + 1])
        torch.cuda.synchronize()
        if len(got) == 7:
            size = (st.hc, st.wc)
            state = st.mode._seam_state[1].clone()               # as the window fill left it
        if len(got) == 1:
            if (st.hc, st.wc) != size:
                size, state, regrown = (st.hc, st.wc), ops.seam_state(2, st.hc, st.wc, 4, dev), regrown + 1
            src, Tk = st._deferred[:2]
            _same(got[0], ops.render_multiband([c['hr'][v, t] for v in range(2)], src, Tk, st.hc, st.wc, 'NORMAL', 3, seam='dp', seam_cell=4,
                                               seam_mu=65535, seam_state=state), ('frame', t))
            checked += 1
    assert checked == PUSHES - 7 and regrown >= 1 and st.canvas_epoch >= 1


def test_run_two_view_with_the_dp_seam_equals_its_frames_one_by_one(dev, hip_nets):
    """pipeline.run_two_view(seam='dp') on 12 frames (a chunk of 8 and one of 4, one state through both) == the same frames rendered
    one at a time by ops.render_multiband with one state; run_three_view takes the argument too."""
    from stabstitch2_amd import ops, pipeline
    c = _clip(dev)
    hr, lr = c['hr'], c['lr']
    frames, hc, wc, m1, m2 = pipeline.run_two_view(hr[0], hr[1], lr[0], lr[1], hip_nets, fusion_mode='MULTIBAND', bands=3, seam='dp',
                                                   seam_mu=150)
    _, _, src, Tk = pipeline.render_plan([m1, m2], SH, SW)
    cell = ops.seam_cell(hc, wc)
    state = ops.seam_state(2, hc, wc, cell, dev)
    for i in range(PUSHES):
        _same(ops.render_multiband([hr[0, i], hr[1, i]], src[i], Tk[i], hc, wc, 'NORMAL', 3, seam='dp', seam_mu=150, seam_state=state),
              frames[i], ('frame', i))
    geo = pipeline.run_two_view(hr[0], hr[1], lr[0], lr[1], hip_nets, fusion_mode='MULTIBAND', bands=3)[0]
    _same(pipeline.run_two_view(hr[0], hr[1], lr[0], lr[1], hip_nets, fusion_mode='MULTIBAND', bands=3, seam='geometric')[0], geo, 'geometric')
    assert not torch.equal(geo, frames)
    three = pipeline.run_three_view(hr[0], hr[1], hr[2], lr[0], lr[1], lr[2], hip_nets, fusion_mode='MULTIBAND', bands=3, seam='dp')
    assert three[0].shape[0] == PUSHES and not torch.equal(
        three[0], pipeline.run_three_view(hr[0], hr[1], hr[2], lr[0], lr[1], lr[2], hip_nets, fusion_mode='MULTIBAND', bands=3)[0])
    with pytest.raises(ValueError, match='MULTIBAND'):
        pipeline.run_two_view(hr[0], hr[1], lr[0], lr[1], hip_nets, fusion_mode='LINEAR', seam='dp')


def test_a_refit_viewport_keeps_one_state_under_the_dp_seam(dev, hip_nets, monkeypatch):
    """viewport= with grow='refit' and seam='dp' (push_u8, the window's seven frames and two steady-state ones): every frame is the
    ops render of the stitcher's splines of that frame at the viewport's size, fed ONE state that is never reset -- a refit moves the
    box under a fixed grid, and the state stays."""
    from stabstitch2_amd import online, ops
    from test_gpu_multiband import VIEWPORTS
    c = _clip(dev)
    hc, wc = VIEWPORTS[2]
    st = _make(hip_nets, 2, viewport=(hc, wc), grow='refit', bands=3, **KW)
    solved = []
    inner = online._Stitcher._render_solved

    def spy(self, imgs, src, Tk, *a, **kw):
        solved.append((src.clone(), Tk.clone()))
        return inner(self, imgs, src, Tk, *a, **kw)
    monkeypatch.setattr(online.OnlineStitcher, '_render_solved', spy)
    state, kept, emitted, differs = ops.seam_state(2, hc, wc, 4, dev), None, 0, 0
    for t in range(9):
        solved.clear()
        got = st.push_u8(c['u8'][0, t], c['u8'][1, t])
        if not got:
            continue
        splines, frames_t = (list(solved), range(7)) if len(got) == 7 else ([st._deferred[:2]], [t])
        assert len(splines) == len(got)
        for (src, Tk), ft, frame in zip(splines, frames_t, got):
            imgs = [c['u8'][v, ft] for v in range(2)]
            want = ops.render_multiband(imgs, src, Tk, hc, wc, 'NORMAL', 3, seam_state=state, **_ops_kw())
            assert frame.shape == (hc, wc, 3) and frame.dtype == torch.uint8 and torch.equal(frame, want), (t, ft)
            differs += not torch.equal(frame, ops.render_multiband(imgs, src, Tk, hc, wc, 'NORMAL', 3))
            emitted += 1
        if kept is None:
            kept = st.mode._seam_state[1]
        assert st.mode._seam_state[1] is kept and st.mode._seam_state[0] == (hc, wc, 2)       # the stream's one state
    assert emitted == 9 and differs > 0 and st.grow == 'refit' and (st.hc, st.wc) == (hc, wc) and st.mode.seam['seam'] == 'dp'
    assert torch.equal(kept, state) and int(state[0]) == 1


# ================================================================================================ the uint8 and the long routes
SEAMS = {'geometric': dict(seam='geometric'), 'dp': dict(seam='dp', seam_mu=150)}


def _held_to_the_ops_render(dev, video, hc, wc, meshes, seam, prescaled):
    """video uint8 [12,hc,wc,3] (device tensor or host array) == ops.canvas_to_u8 of ops.render_multiband at bands = 3, frame by frame,
    on the splines pipeline.render_plan makes of the returned meshes; with the DP seam one ops.seam_state runs through all frames."""
    from stabstitch2_amd import ops, pipeline
    c = _clip(dev)
    views = len(meshes)
    video = video if torch.is_tensor(video) else T(video).to(dev)
    assert video.shape == (PUSHES, hc, wc, 3) and video.dtype == torch.uint8
    phc, pwc, src, Tk = pipeline.render_plan(list(meshes), SH, SW, prescaled=prescaled)
    assert (phc, pwc) == (hc, wc)
    kw = dict(SEAMS[seam])
    if seam == 'dp':
        kw['seam_state'] = ops.seam_state(views, hc, wc, ops.seam_cell(hc, wc), dev)
    differs = 0
    for i in range(PUSHES):
        imgs = [c['hr'][v, i] for v in range(views)]
        want = ops.canvas_to_u8(ops.render_multiband(imgs, src[i], Tk[i], hc, wc, 'NORMAL', 3, **kw)[None])[0]
        assert torch.equal(video[i], want), (seam, 'frame', i)
        differs += not torch.equal(want, ops.canvas_to_u8(ops.render_multiband(imgs, src[i], Tk[i], hc, wc, 'NORMAL', 3)[None])[0])
    assert (differs > 0) == (seam == 'dp')                                     # the dp video is not the geometric one
    assert int(video.max()) > 100


@pytest.mark.parametrize('seam', sorted(SEAMS))
@pytest.mark.parametrize('views', [2, 3])
def test_the_uint8_routes_render_multiband_with_bands_and_either_seam(dev, hip_nets, views, seam):
    """pipeline.run_two_view_u8 / run_three_view_u8(fusion_mode='MULTIBAND', bands=3) on the 12-frame clip."""
    from stabstitch2_amd import pipeline
    c = _clip(dev)
    run = pipeline.run_two_view_u8 if views == 2 else pipeline.run_three_view_u8
    res = run(*[c['u8'][v] for v in range(views)], hip_nets, fusion_mode='MULTIBAND', device=dev, bands=3, **SEAMS[seam])
    _held_to_the_ops_render(dev, res[0], res[1], res[2], res[3:], seam, prescaled=views == 3)


@pytest.mark.parametrize('chunk,chunks', [(5, [(0, 5), (5, 10), (10, 12)]), (9, [(0, 9), (9, 12)])], ids=['chunk5', 'chunk9'])
@pytest.mark.parametrize('seam', sorted(SEAMS))
@pytest.mark.parametrize('views', [2, 3])
def test_the_long_routes_render_multiband_with_bands_and_either_seam(dev, hip_nets, views, seam, chunk, chunks):
    """pipeline.run_two_view_long / run_three_view_long (LongVideoStitcher) on host copies of the clip: chunks of 5, 5 and 2, and a
    chunk of 9 that MULTIBAND_FRAMES splits 8 + 1 followed by one of 3; the seam's state runs through the chunks."""
    from stabstitch2_amd import pipeline
    c = _clip(dev)
    assert pipeline.MULTIBAND_FRAMES == 8
    host = [c['u8'][v].cpu().numpy() for v in range(views)]
    run = pipeline.run_two_view_long if views == 2 else pipeline.run_three_view_long
    seen, parts = [], []

    def sink(frames, s, e):
        seen.append((s, e))
        parts.append(frames.numpy().copy())
    res = run(*host, hip_nets, fusion_mode='MULTIBAND', device=dev, chunk=chunk, sink=sink, bands=3, **SEAMS[seam])
    assert res[0] is None and seen == chunks
    _held_to_the_ops_render(dev, np.concatenate(parts), res[1], res[2], res[3:], seam, prescaled=views == 3)


def test_bands_without_multiband_is_refused_by_every_route(dev, hip_nets):
    from stabstitch2_amd import pipeline
    c = _clip(dev)
    u8 = [c['u8'][v] for v in range(3)]
    host = [x.cpu().numpy() for x in u8]
    routes = [lambda **k: pipeline.run_two_view_u8(u8[0], u8[1], hip_nets, device=dev, **k),
              lambda **k: pipeline.run_three_view_u8(u8[0], u8[1], u8[2], hip_nets, device=dev, **k),
              lambda **k: pipeline.run_two_view_long(host[0], host[1], hip_nets, device=dev, **k),
              lambda **k: pipeline.run_three_view_long(host[0], host[1], host[2], hip_nets, device=dev, **k),
              lambda **k: pipeline.LongVideoStitcher(hip_nets, dev, **k)]
    for route in routes:
        with pytest.raises(ValueError, match='bands'):
            route(fusion_mode='AVERAGE', bands=3)
        with pytest.raises(ValueError, match='bands'):
            route(fusion_mode='MULTIBAND', bands=7)
    assert pipeline.LongVideoStitcher(hip_nets, dev, fusion_mode='MULTIBAND').bands is None      # the default is unchanged
