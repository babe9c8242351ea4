"""The kernels the two earlier sweeps left out -- the LINEAR blender of render.hip and its fused renderers; the DLT, decomposition,
mesh, canvas-box, normalise, three-view and watcher kernels of geom.hip; the SmoothNet glue and the streaming windows of smooth.hip;
the byte and layout kernels of frameio.hip / conv.hip / render.hip -- against the float64 statements of tests/ref64.py or, where a
kernel only copies, permutes or performs single correctly rounded operations, bit for bit against numpy.  Every output element is
compared; seeds are fixed; shapes sit in `parametrize` lists so that a failure names its shape; the inputs are built in
tests/sweep_inputs.py, which tests/test_ref64.py shares.

Gates (the three kinds of tests/test_gpu_kernel_sweeps.py, no others):
  bit for bit   copies, permutes, byte casts, min / max, the watcher's documented update, every kernel that is a fixed sequence of
                single rounded fp32 operations (normalise, three-view, SmoothNet glue: the fp32 reading of ref64's statement in the
                same order), refusals, and the fused LINEAR renderers against the per-frame chain tps_warp_views + linear_blend
                (+ mask_union + linear_blend), whose blender is held to float64 here and whose warp is held to float64 by
                test_gpu_kernel_sweeps.test_tps_warp_views_against_fp64
  derived       ss_linear_blend: ref64.linear_blend_bound (operation counts and the conditioning of the projection of the very
                input); the float64 side of the bit-for-bit kernels: ref64.canvas_normalize_bound, canvas_recover_bound,
                three_view_align_bound (the 63-point mean in any order) and smooth_bound.  tests/test_ref64.py shows the fp32
                oracle or the fp32 reading inside half of each on every case of this file
  measured      4 e_oracle per output position, e_oracle = the fp32 oracle's own error against ref64 on the very input, computed
                in the test (`measured`): ss_tensor_dlt, ss_spatial_decompose, ss_spatial_meshes, ss_h2mesh -- fp64 inside,
                rounded once

    python -m pytest tests/test_gpu_rest_sweeps.py -m gpu          (SS_VERBOSE=1 prints every observed maximum beside its gate)"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import ref64 as R
import sweep_inputs as G
from sweep_inputs import host, within, refused, astype_u8          # noqa: F401
from test_gpu_kernel_sweeps import dev                  # noqa: F401  (the module's GPU fixture)

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
T = torch.from_numpy
F32 = np.float32
SS_ERR_ARG = -1


def same_bits(got, want, what):
    """bit for bit (so that -0.0 != 0.0 and NaNs compare by payload); names the first element that differs"""
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    want = np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    a = np.ascontiguousarray(got).view(np.uint8).reshape(got.shape + (got.itemsize,))
    b = np.ascontiguousarray(want).view(np.uint8).reshape(want.shape + (want.itemsize,))
    bad = (a != b).any(axis=-1)
    if bad.any():
        i = tuple(int(k[0]) for k in np.nonzero(bad))
        raise AssertionError('%s: %d of %d elements differ, first at %s: got %r, want %r' % (what, int(bad.sum()), bad.size, i, got[i], want[i]))


def canaried(n, dev, dtype=torch.float32, pad=64, value=7.0):
    """a tensor of n elements with `pad` canary elements either side -> (buffer, the middle view)"""
    buf = torch.full((n + 2 * pad,), value, device=dev, dtype=dtype)
    return buf, buf[pad:pad + n]


def canaries_intact(buf, n, what, pad=64, value=7.0):
    assert bool((buf[:pad] == value).all()) and bool((buf[pad + n:] == value).all()), what + ': wrote outside its buffer'


# ================================================================================================ LINEAR blender against fp64
@functools.lru_cache(maxsize=None)
def lb_ref(pattern, hc, wc):
    ref, tgt, m1, m2 = G.lb_case(pattern, hc, wc)
    return (ref, tgt, m1, m2) + R.linear_blend_bound(ref, tgt, m1, m2)


@pytest.mark.parametrize('pattern', G.LB_PATTERNS)
@pytest.mark.parametrize('hc,wc', G.LB_CANVASES)
def test_linear_blend_against_fp64(dev, hc, wc, pattern):
    """ss_linear_blend (lb_init, lb_centroid, lb_range, lb_premask, lb_blur twice, lb_final), mask1 and the blended planes, against
    ref64.linear_blender under the derived bound: every reflect index in use at 11 x 11, one row / column past the 4 x 64 blocks,
    no overlap, an overlap of one pixel, vec == 0, a product of exactly 0.5, a target in the last row and column only.  The
    workspace sits between canaries; both outputs at once give the bits of each alone."""
    from stabstitch2_amd import _hip as H, ops
    ref, tgt, m1, m2, mask1, planes, bm, bp = lb_ref(pattern, hc, wc)
    rd, td, m1d, m2d = (T(x).to(dev) for x in (ref, tgt, m1, m2))
    what = 'linear_blend %s %dx%d' % (pattern, hc, wc)
    mk = ops.linear_blend(None, None, m1d, m2d, True)
    within(mk, mask1, bm, what + ' mask1')                  # observed: see LAB_NOTES.md part U
    out = ops.linear_blend(rd, td, m1d, m2d)
    within(out, planes, bp, what + ' planes')
    n = int(H.lib().ss_linear_blend_workspace_floats(hc, wc))
    buf, ws = canaried(n, dev)
    both, bmk = torch.full((3, hc, wc), 7.0, device=dev), torch.full((hc, wc), 7.0, device=dev)
    H.call('ss_linear_blend', H.dptr(rd), H.dptr(td), H.dptr(m1d), H.dptr(m2d), H.dptr(both), H.dptr(bmk), hc, wc, H.dptr(ws), H.stream())
    canaries_intact(buf, n, what)
    assert torch.equal(both, out) and torch.equal(bmk, mk), what + ': both outputs at once'


@pytest.mark.parametrize('pattern', G.LB_PATTERNS)
@pytest.mark.parametrize('hc,wc', [(12, 65), (65, 63), (97, 129)])
def test_linear_blend_three_view_chain_against_fp64(dev, hc, wc, pattern):
    """linear_blend(f12, w3, mask_union(m1, m2), m3) against ref64.linear_blender applied twice.  The union of two masks on the
    1/64 lattice is exact in fp32 (ss_mask_union bit for bit); the first pass's error enters the second through `ref * mask1`, so
    the chain's bound is the second pass's own plus mask1 x the first pass's."""
    from stabstitch2_amd import ops
    ref, tgt, m1, m2, _, f12, _, b12 = lb_ref(pattern, hc, wc)
    w3, m3 = G.lb_third(hc, wc)
    union = (m1 + m2 - m1 * m2).astype(F32)
    assert np.array_equal(union.astype(np.float64), R.f64(m1) + R.f64(m2) - R.f64(m1) * R.f64(m2))
    mk2, want, bm2, b2 = R.linear_blend_bound(f12, w3, union, m3)
    rd, td, m1d, m2d, w3d, m3d = (T(x).to(dev) for x in (ref, tgt, m1, m2, w3, m3))
    un = ops.mask_union(m1d, m2d)
    same_bits(un, union, 'mask_union')
    got12 = ops.linear_blend(rd, td, m1d, m2d)
    what = 'three-view chain %s %dx%d' % (pattern, hc, wc)
    within(ops.linear_blend(None, None, un, m3d, True), mk2, bm2, what + ' mask1 of pass 2')
    within(ops.linear_blend(got12, w3d, un, m3d), want, b2 + mk2[None] * b12, what + ' planes')


def test_linear_blend_refusals(dev):
    """SS_ERR_ARG before any launch: a canvas side of 10, null combinations, a workspace that is not 8-byte aligned, 1 or 4 views."""
    from stabstitch2_amd import _hip as H
    z = torch.zeros(3 * 16 * 16 + 8, device=dev)
    p = H.dptr(z)
    big = torch.zeros(1 << 16, device=dev)
    ws, odd = H.dptr(big), H.dptr(big[1:])
    st = H.stream()
    for hc, wc in ((10, 16), (16, 10)):
        refused(SS_ERR_ARG, H.call, 'ss_linear_blend', p, p, p, p, p, None, hc, wc, ws, st)
    refused(SS_ERR_ARG, H.call, 'ss_linear_blend', p, p, None, p, p, None, 16, 16, ws, st)          # no reference mask
    refused(SS_ERR_ARG, H.call, 'ss_linear_blend', p, p, p, None, p, None, 16, 16, ws, st)          # no target mask
    refused(SS_ERR_ARG, H.call, 'ss_linear_blend', p, p, p, p, None, None, 16, 16, ws, st)          # no output at all
    refused(SS_ERR_ARG, H.call, 'ss_linear_blend', None, p, p, p, p, None, 16, 16, ws, st)          # planes wanted, no ref
    refused(SS_ERR_ARG, H.call, 'ss_linear_blend', p, None, p, p, p, None, 16, 16, ws, st)          # planes wanted, no tgt
    refused(SS_ERR_ARG, H.call, 'ss_linear_blend', p, p, p, p, p, None, 16, 16, None, st)           # no workspace
    refused(SS_ERR_ARG, H.call, 'ss_linear_blend', p, p, p, p, p, None, 16, 16, odd, st)            # workspace 4 bytes off 8-byte alignment
    views = (ctypes.c_void_p * 4)(*[z.data_ptr()] * 4)             # a `const float* const*` argument, as _hip.ptr_array builds it:
    views.dev = z.device.index                                     # H.call reads .dev to pick the device whose stream to use
    one = (ctypes.c_int * 1)(16)
    ten = (ctypes.c_int * 1)(10)
    outs = (ctypes.c_void_p * 1)(big.data_ptr())
    for name in ('ss_render_linear_clip', 'ss_render_linear_clip_u8'):
        for v in (1, 4):
            refused(SS_ERR_ARG, H.call, name, views, p, p, ws, None, 1, v, 8, 8, 16, 16, 0, ws, st)
        for hc, wc in ((10, 16), (16, 10)):
            refused(SS_ERR_ARG, H.call, name, views, p, p, ws, None, 1, 2, 8, 8, hc, wc, 0, ws, st)
        refused(SS_ERR_ARG, H.call, name, views, p, p, ws, None, 1, 2, 8, 8, 16, 16, 0, odd, st)
        refused(SS_ERR_ARG, H.call, name, views, p, p, None, None, 1, 2, 8, 8, 16, 16, 0, ws, st)
        refused(SS_ERR_ARG, H.call, name, views, None, p, ws, None, 1, 2, 8, 8, 16, 16, 0, ws, st)
        refused(SS_ERR_ARG, H.call, name, views, p, p, ws, None, 1, 2, 8, 8, 16, 16, 0, None, st)
    for name in ('ss_render_linear_frames', 'ss_render_linear_frames_u8'):
        for v in (1, 4):
            refused(SS_ERR_ARG, H.call, name, views, p, p, outs, 1, v, 8, 8, one, one, 0, ws, st)
        refused(SS_ERR_ARG, H.call, name, views, p, p, outs, 1, 2, 8, 8, ten, one, 0, ws, st)
        refused(SS_ERR_ARG, H.call, name, views, p, p, outs, 1, 2, 8, 8, one, ten, 0, ws, st)
        refused(SS_ERR_ARG, H.call, name, views, p, p, outs, 1, 2, 8, 8, one, one, 0, odd, st)
        refused(SS_ERR_ARG, H.call, name, views, p, p, outs, 33, 2, 8, 8, one, one, 0, ws, st)
        refused(SS_ERR_ARG, H.call, name, views, p, p, outs, 1, 2, 8, 8, None, one, 0, ws, st)
    assert int(H.lib().ss_linear_frames_workspace_floats(1, 2, ten, one)) <= 0


# ================================================================================================ fused LINEAR renderers, bit for bit
def lb_chain(ops, planes, src, Tk, hc, wc, mode):
    """the per-frame chain on one frame: planes = per-view [3,h,w] -> (fused [3,hc,wc], [mask1 of every pass])"""
    wv = ops.tps_warp_views(planes, src, Tk, hc, wc, mode)
    f = ops.linear_blend(wv[0, 0:3], wv[1, 0:3], wv[0, 3], wv[1, 3])
    mks = [ops.linear_blend(None, None, wv[0, 3], wv[1, 3], True)]
    if len(planes) == 3:
        un = ops.mask_union(wv[0, 3], wv[1, 3])
        mks.append(ops.linear_blend(None, None, un, wv[2, 3], True))
        f = ops.linear_blend(f, wv[2, 0:3], un, wv[2, 3])
    return f, mks, wv


@pytest.mark.parametrize('mode', ['NORMAL', 'FAST'])
@pytest.mark.parametrize('views', [2, 3])
@pytest.mark.parametrize('hc,wc', G.LB_RENDER_CANVASES + [(40, 51)], ids=lambda v: str(v))
def test_linear_renderers_equal_per_frame_chain(dev, hc, wc, views, mode):
    """ops.render_linear_clip and ops.render_linear_frames (fp32 planes and uint8 frames, mask1 of every pass) == the per-frame
    chain, bit for bit, at canvases below one strip in both directions, at the 11-row minimum, and one row / column past a strip;
    every strip height of ss_linear_clip_set_rows (0, 8, 21, 96) and the 64 x 64-tile kernel (-1); the ragged renderer with a
    different canvas per frame.  (40, 51): the second view lies entirely off the canvas (no overlap; a target mask of zeros, or of the clamped sampler's
    rounding residue alone, whose pixels then make up the target's centroid)."""
    from stabstitch2_amd import _hip, ops
    n = 2
    off = 1 if (hc, wc) == (40, 51) else None
    U, src, tgt = G.lb_render_case(n, views, hc, wc, off_canvas=off)
    sd = T(src).to(dev)
    Tk = ops.tps_solve(sd.view(-1, 63, 2), T(np.repeat(tgt[None], n * views, 0)).to(dev)).view(n, views, 2, 66)
    clips = [T(np.ascontiguousarray(U[:, v])).to(dev) for v in range(views)]                   # per view [n,3,h,w]
    u8 = [c.permute(0, 2, 3, 1).to(torch.uint8).contiguous() for c in clips]                   # whole numbers: exact
    chain = [lb_chain(ops, [c[i] for c in clips], sd[i], Tk[i], hc, wc, mode) for i in range(n)]
    if off is not None:                 # FAST: zeros; NORMAL: nothing but the clamped sampler's rounding residue (sweep_inputs.blend_residue)
        far = chain[0][2][off, 3]
        assert float(far.abs().max()) <= (0.0 if mode == 'FAST' else 1e-3), 'the off-canvas view reached the canvas'
        assert float((chain[0][2][0, 3] * far).round().abs().max()) == 0.0, 'an overlap with the off-canvas view'
    else:
        assert all(0.0 < float(chain[0][2][v, 3].mean()) < 1.0 for v in range(views)), 'a mask is empty or full: nothing to blend'
    want = torch.stack([c[0] for c in chain])
    want_mk = torch.stack([torch.stack(c[1]) for c in chain])
    want8 = ops.canvas_to_u8(want)
    try:
        for rows in (0, 8, 21, 96, -1):
            _hip.lib().ss_linear_clip_set_rows(rows)
            got, mk = ops.render_linear_clip(clips, sd, Tk, hc, wc, mode, want_masks=True)
            assert torch.equal(got, want), ('clip', rows, float((got - want).abs().max()))
            assert torch.equal(mk, want_mk), ('clip masks', rows, float((mk - want_mk).abs().max()))
            got8, mk8 = ops.render_linear_clip(u8, sd, Tk, hc, wc, mode, want_masks=True)
            assert torch.equal(got8, want8), ('clip u8', rows)
            assert torch.equal(mk8, want_mk), ('clip u8 masks', rows)
            if rows >= 0:                                       # the ragged renderer has the rolling form only
                fr = ops.render_linear_frames(clips, sd, Tk, [(hc, wc)] * n, mode)
                assert all(torch.equal(fr[i], want[i]) for i in range(n)), ('frames', rows)
                fr8 = ops.render_linear_frames(u8, sd, Tk, [(hc, wc)] * n, mode)
                assert all(torch.equal(fr8[i], want8[i]) for i in range(n)), ('frames u8', rows)
    finally:
        _hip.lib().ss_linear_clip_set_rows(0)
    # ragged: frame 1 on a canvas of its own (the normalised splines hold on any canvas)
    hc2, wc2 = wc + 3, hc + 60
    f1, _, _ = lb_chain(ops, [c[1] for c in clips], sd[1], Tk[1], hc2, wc2, mode)
    fr = ops.render_linear_frames(clips, sd, Tk, [(hc, wc), (hc2, wc2)], mode)
    assert torch.equal(fr[0], want[0]) and torch.equal(fr[1], f1), 'ragged frames'
    fr8 = ops.render_linear_frames(u8, sd, Tk, [(hc, wc), (hc2, wc2)], mode)
    assert torch.equal(fr8[0], want8[0]) and torch.equal(fr8[1], ops.canvas_to_u8(f1[None])[0]), 'ragged frames u8'


# ================================================================================================ canvas box
@pytest.mark.parametrize('npts', [1, 63, 64, 255, 256, 257, 63 * 300])
def test_mesh_bbox_bit_exact(dev, npts):
    """ss_mesh_bbox == numpy fp32 (x * img_w, then / 480; y * img_h, then / 360; min and max are exact): the single 256-thread
    block below, at and above one pass, scaled and unscaled (img_h = img_w = 0), fresh and accumulating into a box, the extreme at
    the first, the last and a middle point."""
    from stabstitch2_amd import _hip as H
    rs = np.random.RandomState(16000 + npts)
    for where in sorted({0, npts // 2, npts - 1}):
        m = rs.uniform(-50, 500, (npts, 2)).astype(F32)
        m[where] = [-77.3, 611.9]                              # x minimum and y maximum
        md = T(m).to(dev)
        for (ih, iw) in ((720.0, 1280.0), (360.0, 480.0), (0.0, 0.0)):
            x = (m[:, 0] * F32(iw)) / F32(480.0) if iw > 0 else m[:, 0]
            y = (m[:, 1] * F32(ih)) / F32(360.0) if ih > 0 else m[:, 1]
            want = np.array([x.min(), x.max(), y.min(), y.max()], F32)
            box = torch.full((4,), 7.0, device=dev)
            H.call('ss_mesh_bbox', H.dptr(md), npts, ih, iw, H.dptr(box), 0, H.stream())
            same_bits(box, want, 'mesh_bbox npts %d extreme at %d size %gx%g' % (npts, where, ih, iw))
            assert want[0] == x[where] and want[3] == y[where]
            for prior in ([-1e4, 1e4, -1e4, 1e4], [100.0, 101.0, 100.0, 101.0]):       # a box that wins, and one that loses
                acc = T(np.array(prior, F32)).to(dev)
                H.call('ss_mesh_bbox', H.dptr(md), npts, ih, iw, H.dptr(acc), 1, H.stream())
                p = np.array(prior, F32)
                same_bits(acc, np.array([min(want[0], p[0]), max(want[1], p[1]), min(want[2], p[2]), max(want[3], p[3])], F32),
                          'mesh_bbox accumulate')


# ================================================================================================ byte and layout kernels
def lr_reference(frames, lr_h, lr_w):
    from oracle import frame_io as FIO
    return np.stack([FIO.load_frame(f, lr_h, lr_w)[1] for f in frames])


@pytest.mark.parametrize('h,w,lr_h,lr_w', [
    (8, 12, 4, 6),          # exact 2 x: the area average (mode 1); w % 4 == 0: the 4-pixel HR kernel
    (6, 10, 3, 5),          # exact 2 x, w % 4 != 0: the 1-pixel HR kernel
    (9, 13, 9, 13),         # same size: the copy (mode 2)
    (37, 52, 20, 31),       # a non-integer downscale (mode 0)
    (5, 7, 11, 18),         # an upscale: the source index goes negative at the left / top edge
    (5, 1, 4, 3),           # w = 1: both x taps are pixel 0
    (1, 9, 3, 4),           # h = 1: both y taps are row 0
    (3, 8, 5, 70),          # more than one 64-column block of LR pixels
], ids=lambda v: str(v))
def test_ingest_u8_paths_bit_exact(dev, h, w, lr_h, lr_w):
    """ss_ingest_u8: HR planes are a copy (uint8 -> fp32) through the 4-pixel kernel (w % 4 == 0, 4-byte aligned base) and the
    1-pixel kernel (w % 4 != 0, or a base pointer at byte 1), LR in its three modes == oracle/frame_io.py, n = 0 a no-op."""
    from stabstitch2_amd import _hip as H, ops
    rs = np.random.RandomState(17000 + 131 * h + w)
    frames = rs.randint(0, 256, (3, h, w, 3)).astype(np.uint8)
    frames[1] = 255
    want_hr = np.ascontiguousarray(frames.transpose(0, 3, 1, 2)).astype(F32)
    want_lr = lr_reference(frames, lr_h, lr_w)
    n = frames.size
    for shift in (0, 1):                                       # the base pointer 4-byte aligned, and at byte 1
        buf = torch.zeros(n + 8, device=dev, dtype=torch.uint8)
        fd = buf[shift:shift + n].view(3, h, w, 3).copy_(T(frames).to(dev))
        assert fd.data_ptr() % 4 == shift
        hb, hr = canaried(n, dev)
        lb, lr = canaried(9 * lr_h * lr_w, dev)
        ops.ingest_u8(fd, lr_h, lr_w, hr_out=hr.view(3, 3, h, w), lr_out=lr.view(3, 3, lr_h, lr_w))
        same_bits(hr.view(3, 3, h, w), want_hr, 'ingest hr %dx%d shift %d' % (h, w, shift))
        same_bits(lr.view(3, 3, lr_h, lr_w), want_lr, 'ingest lr %dx%d -> %dx%d shift %d' % (h, w, lr_h, lr_w, shift))
        canaries_intact(hb, n, 'ingest hr')
        canaries_intact(lb, 9 * lr_h * lr_w, 'ingest lr')
    hr = torch.full((1, 3, h, w), 7.0, device=dev)
    lr = torch.full((1, 3, lr_h, lr_w), 7.0, device=dev)
    H.call('ss_ingest_u8', H.dptr(fd, dtype=torch.uint8), H.dptr(hr), H.dptr(lr), 0, h, w, lr_h, lr_w, H.stream())
    assert bool((hr == 7.0).all()) and bool((lr == 7.0).all()), 'n = 0 wrote something'


U8_EDGE_VALUES = [-0.0, -1.5, 255.99, 256.0, 300.7, 1e10, np.inf, -np.inf, np.nan, -0.99, 255.0, -256.0, -257.5, 2147483520.0, -2147483648.0]


@pytest.mark.parametrize('h,w', [(4, 4), (2, 6), (3, 5), (1, 1), (7, 37), (16, 64)], ids=lambda v: str(v))
def test_canvas_to_u8_paths_and_edge_values(dev, h, w):
    """ss_canvas_to_u8 through both kernels -- four pixels per thread (h w % 4 == 0 and aligned pointers) and one (h w % 4 != 0, or
    an output at byte 1, or a canvas 4 bytes past a 16-byte boundary) -- on random 0..256 planes with the edge values of the cast
    sown over every plane and lane position: -0.0, -1.5, 255.99, 256, 300.7, 1e10, +-inf, NaN, the int32 limits."""
    from stabstitch2_amd import _hip as H
    rs = np.random.RandomState(18000 + 131 * h + w)
    n = 2
    x = rs.uniform(0, 256, (n, 3, h, w)).astype(F32)
    flat = x.reshape(-1)
    pos = rs.permutation(flat.size)
    for k, p in enumerate(pos[:min(flat.size, 4 * len(U8_EDGE_VALUES))]):
        flat[p] = U8_EDGE_VALUES[k % len(U8_EDGE_VALUES)]
    want = astype_u8(x.transpose(0, 2, 3, 1))
    for in_shift, out_shift in ((0, 0), (0, 1), (1, 0)):
        cb = torch.zeros(x.size + 8, device=dev)
        cd = cb[in_shift:in_shift + x.size].view(n, 3, h, w).copy_(T(x).to(dev))
        ob = torch.full((x.size + 2 * 64,), 9, device=dev, dtype=torch.uint8)
        od = ob[64 + out_shift:64 + out_shift + x.size].view(n, h, w, 3)
        H.call('ss_canvas_to_u8', H.dptr(cd), H.dptr(od, dtype=torch.uint8), n, h, w, H.stream())
        same_bits(od, want, 'canvas_to_u8 %dx%d shifts %d %d' % (h, w, in_shift, out_shift))
        assert bool((ob[:64 + out_shift] == 9).all()) and bool((ob[64 + out_shift + x.size:] == 9).all()), 'wrote outside'


@pytest.mark.parametrize('c', [1, 3, 4, 63, 64, 65])
@pytest.mark.parametrize('n,h,w', [(1, 1, 1), (2, 3, 5), (1, 7, 37)])
def test_layout_kernels_bit_exact(dev, n, h, w, c):
    """ss_nchw_to_nhwc (the generic kernel, and the one-float4-per-pixel kernel for c_pad == 4 on a 16-byte aligned output -- and the
    generic one again when that output is not) and ss_nhwc_to_nchw (c_stride == c and > c): permutes with zero padding channels,
    odd h w, and the round trip."""
    from stabstitch2_amd import _hip as H, ops
    x = np.random.RandomState(19000 + c + 7 * h * w).normal(0, 1, (n, c, h, w)).astype(F32)
    xd = T(x).to(dev)
    pads = sorted({c, (c + 3) // 4 * 4, c + 5})
    for cp in pads:
        want = np.zeros((n, h, w, cp), F32)
        want[..., :c] = x.transpose(0, 2, 3, 1)
        for shift in (0, 1):                                    # out 16-byte aligned, and 4 bytes past
            buf = torch.full((want.size + 2 * 64,), 7.0, device=dev)
            out = buf[64 + shift:64 + shift + want.size].view(n, h, w, cp)
            assert out.data_ptr() % 16 == 4 * shift
            ops.nchw_to_nhwc(xd, cp, out)
            same_bits(out, want, 'nchw_to_nhwc c %d -> %d shift %d' % (c, cp, shift))
            assert bool((buf[:64 + shift] == 7.0).all()) and bool((buf[64 + shift + want.size:] == 7.0).all()), 'wrote outside'
            back = ops.nhwc_to_nchw(out.contiguous(), c) if shift == 0 else None
            if back is not None:
                same_bits(back, x, 'nhwc_to_nchw c %d of %d (round trip)' % (c, cp))


@pytest.mark.parametrize('n', [1, 255, 256, 257])
def test_elementwise_helpers_bit_exact(dev, n):
    """ss_add_mul ((x + add) * mul, two rounded operations), ss_mask_union (a + b - a b, three) and ss_fill_f32 == numpy fp32 in
    the same order, around the 256-thread block, between canaries."""
    from stabstitch2_amd import _hip as H, ops
    rs = np.random.RandomState(20000 + n)
    x = rs.normal(0, 100, n).astype(F32)
    a, b = rs.uniform(0, 1, n).astype(F32), rs.uniform(0, 1, n).astype(F32)
    xd, ad, bd = T(x).to(dev), T(a).to(dev), T(b).to(dev)
    for add, mul in ((1.0, 127.5), (-0.1, 1.0 / 3.0), (0.0, 1.0)):
        buf, out = canaried(n, dev)
        H.call('ss_add_mul', H.dptr(xd), H.dptr(out), add, mul, n, H.stream())
        same_bits(out, ((x + F32(add)).astype(F32) * F32(mul)).astype(F32), 'add_mul n %d' % n)
        canaries_intact(buf, n, 'add_mul')
        same_bits(ops.add_mul(xd, add, mul), ((x + F32(add)).astype(F32) * F32(mul)).astype(F32), 'ops.add_mul')
    buf, out = canaried(n, dev)
    H.call('ss_mask_union', H.dptr(ad), H.dptr(bd), H.dptr(out), n, H.stream())
    same_bits(out, ((a + b).astype(F32) - (a * b).astype(F32)).astype(F32), 'mask_union n %d' % n)
    canaries_intact(buf, n, 'mask_union')
    for v in (0.0, -0.0, 3.25, float('inf')):
        buf, out = canaried(n, dev)
        ops.fill(out, v)
        same_bits(out, np.full(n, v, F32), 'fill n %d' % n)
        canaries_intact(buf, n, 'fill')


# ================================================================================================ mesh geometry
def measured(oracle, ref, axes):
    """The measured gate 4 e_oracle, e_oracle = the fp32 oracle's own error against ref64 on the very input, taken per position
    of the output (the maximum over `axes`, the batch): the entries of a homography differ by six orders of magnitude."""
    return 4 * np.abs(host(oracle) - ref).max(axis=axes, keepdims=True)


@pytest.mark.parametrize('kind', ['zero', 'mild', 'large'])
@pytest.mark.parametrize('img_h,img_w', G.GEOM_SIZES)
@pytest.mark.parametrize('n', G.GEOM_BATCHES)
def test_dlt_decompose_meshes_against_fp64(dev, n, img_h, img_w, kind):
    """ss_tensor_dlt, ss_spatial_decompose and ss_spatial_meshes against numpy.linalg in float64, batches below, at and above one
    64-thread block, at 360 x 480 and 720 x 1280, on the identity, on offsets of the regressor's size and on quads near collapse.
    The kernels solve in fp64 and round once; the gate is 4 x the fp32 oracle's own error on the very input, per output position,
    so the conditioning of the large quads is in the gate by construction."""
    from oracle import geometry as OG
    from stabstitch2_amd import ops
    off = G.geom_offsets(n, kind, img_h, img_w)
    what = 'n %d %dx%d %s' % (n, img_h, img_w, kind)
    c = G.corner_points(n, img_h, img_w)
    dst = (c + off.reshape(n, 4, 2)).astype(F32)
    ref = R.dlt4(c, dst)
    within(ops.tensor_dlt(T(c).to(dev), T(dst).to(dev)), ref, measured(OG.dlt4(T(c), T(dst)), ref, 0), 'tensor_dlt ' + what)
    # theta_ref / theta_tgt of the first stage (1/8 scale, normalised coordinates)
    tr, tt = R.spatial_thetas(off, img_h, img_w)
    _, oHt, oHr = OG.decompose(T(off), img_h, img_w, scale=8.0)
    M = torch.tensor([[img_w / 8 / 2.0, 0.0, img_w / 8 / 2.0], [0.0, img_h / 8 / 2.0, img_h / 8 / 2.0], [0.0, 0.0, 1.0]])
    Mi = torch.inverse(M)
    ga, gb = ops.spatial_decompose(T(off).to(dev), img_h, img_w)
    within(ga, tr, measured(Mi @ oHr @ M, tr, 0), 'spatial_decompose theta_ref ' + what)
    within(gb, tt, measured(Mi @ oHt @ M, tt, 0), 'spatial_decompose theta_tgt ' + what)
    # the meshes of the second stage (full scale)
    o_r, o_t = G.geom_residuals(n)
    m1, m2 = R.spatial_meshes(off, o_r, o_t, img_h, img_w)
    _, oHt, oHr = OG.decompose(T(off), img_h, img_w, scale=1.0)
    rigid = OG.rigid_mesh(n, img_h, img_w)
    om1 = OG.homography_to_mesh(oHr, rigid) + T(o_r).reshape(n, 7, 9, 2) - rigid
    om2 = OG.homography_to_mesh(oHt, rigid) + T(o_t).reshape(n, 7, 9, 2) - rigid
    g1, g2 = ops.spatial_meshes(T(off).to(dev), T(o_r).to(dev), T(o_t).to(dev), img_h, img_w)
    within(g1, m1, measured(om1, m1, (0, 1, 2)), 'spatial_meshes motion1 ' + what)
    within(g2, m2, measured(om2, m2, (0, 1, 2)), 'spatial_meshes motion2 ' + what)


@pytest.mark.parametrize('npts', [1, 63, 64, 65])
@pytest.mark.parametrize('n', G.GEOM_BATCHES)
def test_h2mesh_against_fp64(dev, n, npts):
    """ss_h2mesh (one block row per item, 64 points per block) on the mild and the large homographies of the sweep, points over and
    around the frame; gate 4 x the oracle's error on the very input."""
    from stabstitch2_amd import ops
    img_h, img_w = 360, 480
    for kind in ('mild', 'large'):
        off = G.geom_offsets(n, kind, img_h, img_w, seed=5)
        c = G.corner_points(n, img_h, img_w)
        Hm = R.dlt4(c, (c + off.reshape(n, 4, 2)).astype(F32)).astype(F32)
        pts = np.random.RandomState(23000 + n + npts).uniform(-0.2, 1.2, (n, npts, 2)).astype(F32) * np.array([img_w, img_h], F32)
        ref = R.h2mesh(Hm, pts)
        hom = torch.cat((T(pts), torch.ones(n, npts, 1)), 2)
        t = torch.matmul(torch.inverse(T(Hm)), hom.transpose(1, 2))
        oracle = torch.stack((t[:, 0] / t[:, 2], t[:, 1] / t[:, 2]), 2)
        within(ops.h2mesh(T(Hm).to(dev), T(pts).to(dev)), ref, measured(oracle, ref, (0, 1)), 'h2mesh n %d npts %d %s' % (n, npts, kind))


# ================================================================================================ SmoothNet glue
@pytest.mark.parametrize('zero_first', [0, 1])
@pytest.mark.parametrize('nw,t,wstride', G.SMOOTH_SHAPES, ids=lambda v: str(v))
def test_smooth_embed_and_finalize(dev, nw, t, wstride, zero_first):
    """ss_smooth_embed and ss_smooth_finalize: every operation is one rounded fp32 operation in the reference's order (the window
    sums are sequential additions), so both equal the numpy fp32 reading of ref64's statement bit for bit; and they lie within the
    derived running-sum bound of its float64 reading, so that an order that is wrong but self-consistent shows too.  Every optional
    output of ss_smooth_finalize null in turn (nw = 2)."""
    from stabstitch2_amd import _hip as H, ops
    sm, ts, delta, emb = G.smooth_case(nw, t, wstride)
    smd, tsd, dd = [T(x).to(dev) for x in sm], [T(x).to(dev) for x in ts], T(delta).to(dev)
    args = (sm[0], sm[1], ts[0], ts[1])
    what = 'nw %d t %d wstride %d zero_first %d' % (nw, t, wstride, zero_first)
    embd = [T(e).to(dev) for e in emb]
    step = nw if nw * t <= 600 else 75      # 128 channels per vertex: 300 windows of 7 frames are compared as four launches of 75
    for w0 in range(0, nw, step):
        sl = [x[w0 * wstride:] for x in args]                               # window w0 starts at frame w0 * wstride
        got = ops.smooth_embed(*[x[w0 * wstride:] for x in (smd[0], smd[1], tsd[0], tsd[1])], *embd, step, t, wstride, zero_first)
        same_bits(got.view(step, t, 63, 128), R.smooth_embed(*sl, *emb, step, t, wstride, zero_first, dt=np.float32), 'smooth_embed ' + what)
        s = R.smooth_embed(*sl, *emb, step, t, wstride, zero_first, absum=True)
        within(got.view(step, t, 63, 128), R.smooth_embed(*sl, *emb, step, t, wstride, zero_first), R.smooth_bound(t + 3, s), 'smooth_embed ' + what)
    got = ops.smooth_finalize(smd[0], smd[1], tsd[0], tsd[1], dd, nw, t, wstride, zero_first)
    want32 = R.smooth_finalize(*args, delta, nw, t, wstride, zero_first, dt=np.float32)
    want64 = R.smooth_finalize(*args, delta, nw, t, wstride, zero_first)
    s = R.smooth_finalize(*args, delta, nw, t, wstride, zero_first, absum=True)
    for k in want32:
        same_bits(got[k].view(nw, t, 63, 2), want32[k], 'smooth_finalize %s %s' % (k, what))
        within(got[k].view(nw, t, 63, 2), want64[k], R.smooth_bound(t, s[k]), 'smooth_finalize %s %s' % (k, what))
    if nw == 2:
        names = ('ori_mesh1', 'ori_mesh2', 'ori_path1', 'ori_path2', 'smooth_mesh1', 'smooth_mesh2', 'smooth_path1', 'smooth_path2')
        for skip in names:
            outs = {k: (None if k == skip else torch.full((nw, t, 63, 2), 7.0, device=dev)) for k in names}
            H.call('ss_smooth_finalize', H.dptr(smd[0]), H.dptr(smd[1]), H.dptr(tsd[0]), H.dptr(tsd[1]), H.dptr(dd),
                   *[H.dptr(outs[k], True) for k in names], nw, t, wstride, zero_first, H.stream())
            for k in names:
                if k != skip:
                    same_bits(outs[k], want32[k], 'smooth_finalize without %s: %s' % (skip, k))


@pytest.mark.parametrize('nw,t', G.STITCH_SHAPES)
def test_smooth_stitch_against_frame_loop(dev, nw, t):
    """ss_smooth_stitch (+ smooth_path_chain; with nw = 1, n equals t and no chain launch happens) == the reference's frame loop over
    the sliding windows in numpy fp32, bit for bit, and within the derived bound of the float64 loop: the path of frame f has passed
    at most 2 f + 6 rounded operations.  Without the paths the meshes are the same; exactly one path output is SS_ERR_ARG."""
    from stabstitch2_amd import _hip as H, ops
    sm, ts, delta, _ = G.smooth_case(nw, t, 1, seed=1)
    n = nw + t - 1
    smd, tsd, dd = [T(x).to(dev) for x in sm], [T(x).to(dev) for x in ts], T(delta).to(dev)
    got = ops.smooth_stitch(smd[0], smd[1], tsd[0], tsd[1], dd, nw, t)
    want32 = R.smooth_stitch(sm[0], sm[1], ts[0], ts[1], delta, nw, t, dt=np.float32)
    want64 = R.smooth_stitch(sm[0], sm[1], ts[0], ts[1], delta, nw, t)
    s = R.smooth_stitch(sm[0], sm[1], ts[0], ts[1], delta, nw, t, absum=True)
    rounds = (2 * np.arange(n) + 6).reshape(n, 1, 1)
    for k in want32:
        same_bits(got[k].view(n, 63, 2), want32[k], 'smooth_stitch %s nw %d t %d' % (k, nw, t))
        within(got[k].view(n, 63, 2), want64[k], R.smooth_bound(rounds, s[k]), 'smooth_stitch %s nw %d t %d' % (k, nw, t))
    bare = ops.smooth_stitch(smd[0], smd[1], tsd[0], tsd[1], dd, nw, t, want_paths=False)
    assert all(torch.equal(bare[k], got[k]) for k in bare) and len(bare) == 4
    o = [torch.empty(n, 63, 2, device=dev) for _ in range(6)]
    for a, b in ((o[4], None), (None, o[5])):
        refused(SS_ERR_ARG, H.call, 'ss_smooth_stitch', H.dptr(smd[0]), H.dptr(smd[1]), H.dptr(tsd[0]), H.dptr(tsd[1]), H.dptr(dd),
                H.dptr(o[0]), H.dptr(o[1]), H.dptr(o[2]), H.dptr(o[3]), H.dptr(a, True), H.dptr(b, True), nw, t, H.stream())


# ================================================================================================ streaming windows
@pytest.mark.parametrize('per', [1, 3])
@pytest.mark.parametrize('rings', [1, 8])
@pytest.mark.parametrize('w,e', G.WINDOW_SHAPES, ids=lambda v: str(v))
def test_window_push_bit_exact(dev, w, e, rings, per):
    """ss_window_push / ss_window_push_groups == the documented shift (ring rows 1 .. W-1 move down, the source row becomes the
    last), a copy: (W - 1) E of exactly 2048 (the limit: 8 floats per thread) and of 1, E around the 256-thread block, 1 and 8 ring
    kinds x 1 and 3 streams, scattered source offsets, 0 / 1 / 8 state blocks moved in the same launch; canaries either side of the
    rings, the source and the state."""
    from stabstitch2_amd import ops
    total = rings * per
    ring, rows = G.ring_case(total, w, e, 1)
    rb, rd = canaried(ring.size, dev)
    rd.copy_(T(ring.reshape(-1)).to(dev))
    gap = 5
    src = np.full((rings, per * e + gap), 3.0, F32)                      # ring kind g's `per` rows back to back, then a gap
    src[:, :per * e] = rows.reshape(rings, per * e)
    order = list(range(rings))[::-1]                                     # offsets in descending order: nothing assumes them sorted
    flat = np.concatenate([src[g] for g in order])
    offs = [order.index(g) * (per * e + gap) for g in range(rings)]
    sb, sd = canaried(flat.size, dev)
    sd.copy_(T(flat).to(dev))
    want = np.stack([R.window_shift(ring[r], rows[r])[1] for r in range(total)])
    for blocks in (0, 1, 8):
        rd.copy_(T(ring.reshape(-1)).to(dev))
        block, delta, stride = 126, 130, 300
        st = np.random.RandomState(blocks).normal(0, 1, 8 * stride).astype(F32)
        tb, td = canaried(st.size, dev)
        td.copy_(T(st).to(dev))
        view = rd.view(rings, per, w, e) if per > 1 else rd.view(total, w, e)
        ops.window_push(view, sd, offs, state=td if blocks else None, blocks=blocks, block=block, stride=stride, delta=delta, per=per)
        same_bits(rd.view(total, w, e), want, 'window_push W %d E %d rings %d x %d blocks %d' % (w, e, rings, per, blocks))
        ws = st.copy()
        for b in range(blocks):
            ws[b * stride:b * stride + block] = st[b * stride + delta:b * stride + delta + block]
        same_bits(td, ws, 'window_push state blocks %d' % blocks)
        same_bits(sd, flat, 'window_push source')
        canaries_intact(rb, ring.size, 'window_push ring')
        canaries_intact(sb, flat.size, 'window_push src')
        canaries_intact(tb, st.size, 'window_push state')


@pytest.mark.parametrize('k', [1, 6, 7, 32])
@pytest.mark.parametrize('rings', [1, 8])
@pytest.mark.parametrize('w,e', [(7, 126), (7, 255), (7, 256), (7, 257), (8, 256), (2, 1), (2, 1024), (2048, 1)], ids=lambda v: str(v))
def test_window_advance_bit_exact(dev, w, e, rings, k):
    """ss_window_advance == k documented shifts: the work rows (ring rows 1 .. W-1, then the k new rows) and the ring (the last W work
    rows; from k >= W new rows only), W E of exactly 2048 and of 2, k of 1, W - 1, W and 32 at W = 7, 0 / 1 / 8 state blocks copied
    from a second tensor in the same launch; canaries either side of every buffer."""
    from stabstitch2_amd import ops
    ring, rows = G.ring_case(rings, w, e, k, seed=1)
    gap = 3
    flat = np.full((rings, k * e + gap), 3.0, F32)
    flat[:, :k * e] = rows.reshape(rings, k * e)
    offs = [r * (k * e + gap) for r in range(rings)]
    sb, sd = canaried(flat.size, dev)
    sd.copy_(T(flat.reshape(-1)).to(dev))
    want = [R.window_shift(ring[r], rows[r]) for r in range(rings)]
    for blocks in (0, 1, 8):
        rb, rd = canaried(ring.size, dev)
        rd.copy_(T(ring.reshape(-1)).to(dev))
        wb, wd = canaried(rings * (w - 1 + k) * e, dev)
        block, stride, sstride = 126, 130, 200
        st = np.random.RandomState(blocks + 9).normal(0, 1, 8 * stride).astype(F32)
        ss = np.random.RandomState(blocks + 19).normal(0, 1, 8 * sstride).astype(F32)
        tb, td = canaried(st.size, dev)
        td.copy_(T(st).to(dev))
        ssd = T(ss).to(dev)
        ops.window_advance(rd.view(rings, w, e), wd.view(rings, w - 1 + k, e), sd, offs, k, state=td if blocks else None,
                           state_src=ssd if blocks else None, blocks=blocks, block=block, stride=stride, src_stride=sstride)
        what = 'window_advance W %d E %d rings %d k %d blocks %d' % (w, e, rings, k, blocks)
        same_bits(wd.view(rings, w - 1 + k, e), np.stack([x[0] for x in want]), what + ' work')
        same_bits(rd.view(rings, w, e), np.stack([x[1] for x in want]), what + ' ring')
        ws = st.copy()
        for b in range(blocks):
            ws[b * stride:b * stride + block] = ss[b * sstride:b * sstride + block]
        same_bits(td, ws, what + ' state')
        for buf, n, name in ((rb, ring.size, 'ring'), (wb, rings * (w - 1 + k) * e, 'work'), (sb, flat.size, 'src'), (tb, st.size, 'state')):
            canaries_intact(buf, n, what + ' ' + name)


def test_window_refusals(dev):
    """Every refusal the host code of the streaming windows states, SS_ERR_ARG before any launch."""
    import ctypes
    from stabstitch2_amd import _hip as H
    buf = torch.zeros(1 << 16, device=dev)
    p = H.dptr(buf)
    far = H.dptr(buf[1 << 15:])
    st = H.stream()
    off1 = ctypes.cast((ctypes.c_longlong * 8)(*[0] * 8), ctypes.c_void_p)
    neg = ctypes.cast((ctypes.c_longlong * 8)(*[-1] * 8), ctypes.c_void_p)

    def push(groups=1, per=1, window=7, elems=126, state=None, blocks=0, block=0, stride=0, delta=0, ring=p, src=far, off=off1):
        return H.call('ss_window_push_groups', ring, src, off, groups, per, window, elems, state, blocks, block, stride, delta, st)
    for kw in (dict(ring=None), dict(src=None), dict(off=None), dict(groups=0), dict(groups=9), dict(per=0), dict(per=4097), dict(window=1),
               dict(elems=0), dict(window=2, elems=2049), dict(window=3, elems=1025),              # (W - 1) E > 2048
               dict(blocks=-1), dict(blocks=1, block=4, delta=4),                                   # blocks without a state tensor
               dict(state=far, blocks=1, block=0, delta=4), dict(state=far, blocks=1, block=8, delta=7),      # source overlaps destination
               dict(state=far, blocks=2, block=8, delta=8, stride=15)):                             # block 1 reaches into block 0's source
        refused(SS_ERR_ARG, lambda: push(**kw))

    def adv(rings=1, window=7, elems=126, k=1, state=None, ssrc=None, blocks=0, block=0, stride=0, sstride=0, ring=p, work=far, src=far, off=off1):
        return H.call('ss_window_advance', ring, work, src, off, rings, window, elems, k, state, ssrc, blocks, block, stride, sstride, st)
    third = H.dptr(buf[3 << 13:])
    for kw in (dict(ring=None), dict(work=None), dict(src=None), dict(off=None), dict(rings=0), dict(rings=9), dict(window=1), dict(elems=0),
               dict(k=0), dict(k=33), dict(window=2, elems=1025), dict(blocks=-1), dict(blocks=9),
               dict(work=p), dict(work=H.dptr(buf[7 * 126 - 1:])),                                  # work overlaps the ring (wholly, by one float)
               dict(off=neg),
               dict(blocks=1, block=4, ssrc=third), dict(blocks=1, block=4, state=third),           # one of the two state tensors missing
               dict(blocks=1, block=0, state=third, ssrc=far), dict(blocks=2, block=8, stride=7, sstride=8, state=third, ssrc=far),
               dict(blocks=2, block=8, stride=8, sstride=7, state=third, ssrc=far),
               dict(blocks=1, block=8, state=third, ssrc=H.dptr(buf[(3 << 13) + 7:])),              # a source block overlaps a destination block
               dict(blocks=2, block=8, stride=16, sstride=16, state=third, ssrc=H.dptr(buf[(3 << 13) + 16 + 4:]))):
        refused(SS_ERR_ARG, lambda: adv(**kw))


# ================================================================================================ canvas normalisation, three-view glue
@pytest.mark.parametrize('views', [2, 3])
@pytest.mark.parametrize('frames', G.NORM_FRAMES)
def test_canvas_normalize_kernels_bit_exact(dev, frames, views):
    """ss_mesh_normalize, ss_mesh_normalize_views and ss_mesh_normalize_views_boxes (packed and padded mesh_frame_stride; one box and
    a box per frame) perform a fixed sequence of single rounded fp32 operations per point -- x * img_w, / 480, - wmin, * 2, /
    (wmax - wmin), - 1 -- and equal numpy fp32 in that order bit for bit, scaled (720 x 1280) and unscaled (img_h = img_w = 0); against
    float64 they stay within ref64.canvas_normalize_bound (six roundings of numbers up to the largest coordinate, in the output's
    unit), so an order that is wrong but self-consistent shows."""
    from stabstitch2_amd import ops
    meshes, box, boxes = G.norm_case(frames, views)
    md = [T(m).to(dev) for m in meshes]
    bd, bsd = T(box).to(dev), T(boxes).to(dev)
    for (ih, iw) in G.NORM_SIZES:
        want32 = np.stack([R.canvas_normalize(R.scale_to_hr(m, ih, iw, F32), box, F32) for m in meshes], 1)           # [frames,V,63,2]
        want64, bound = (np.stack(x, 1) for x in zip(*[R.canvas_normalize_bound(R.scale_to_hr(R.f64(m), ih, iw), box) for m in meshes]))
        got = ops.mesh_normalize_views(md, bd, ih, iw)
        same_bits(got, want32, 'mesh_normalize_views frames %d views %d size %d' % (frames, views, ih))
        within(got, want64, bound, 'mesh_normalize_views vs float64')
        same_bits(ops.mesh_normalize(md[0], bd, ih, iw), want32[:, 0], 'mesh_normalize')
        wb32 = np.stack([R.canvas_normalize(R.scale_to_hr(m, ih, iw, F32), boxes[:, None], F32) for m in meshes], 1)
        wb64, bb = (np.stack(x, 1) for x in zip(*[R.canvas_normalize_bound(R.scale_to_hr(R.f64(m), ih, iw), boxes[:, None]) for m in meshes]))
        for stride in (126, 126 + 70):                              # packed, and padded: frame f's mesh `stride` floats after frame f - 1's
            padded = [torch.full((frames, stride), 7.0, device=dev) for _ in range(views)]
            for p, m in zip(padded, md):
                p[:, :126] = m.view(frames, 126)
            got = ops.mesh_normalize_views_boxes(padded, stride, bsd, ih, iw)
            same_bits(got, wb32, 'mesh_normalize_views_boxes stride %d' % stride)
            within(got, wb64, bb, 'mesh_normalize_views_boxes vs float64')
            if views <= 3:
                one = ops.stream_normalize_watch(padded, stride, bsd, ih, iw)              # the same arithmetic, a wave per frame
                same_bits(one, wb32, 'stream_normalize_watch (boxes) stride %d' % stride)
        one = ops.stream_normalize_watch([p[:1] for p in padded], stride, bd, ih, iw)
        same_bits(one, want32[:1], 'stream_normalize_watch (one box)')


@pytest.mark.parametrize('frames', G.NORM_FRAMES)
def test_three_view_glue_kernels(dev, frames):
    """ss_three_view_align: the four scaled meshes bit for bit against numpy fp32; what depends on the 63-point mean (b1, b2, mid) within
    the derived bound of an fp32 sum of 63 terms in any order (ref64.dot_bound on the mean of |w12_m2 - w23_m1|) plus the two
    roundings that follow, and mid == (a2 + b1) / 2 on the kernel's own b1, bit for bit.  ss_three_view_normalize and
    ss_three_view_finish: fixed sequences of single rounded operations, bit for bit against numpy fp32, and against float64 within
    their few roundings."""
    from stabstitch2_amd import ops
    m4, box = G.three_view_case(frames)
    md = [T(m).to(dev).view(1, frames, 7, 9, 2) for m in m4]
    ih, iw = 720, 1280
    got = [g.view(frames, 63, 2) for g in ops.three_view_align(*md, ih, iw)]
    (a1, a2, b1, b2, mid), (gate_b1, gate_b2, gate_mid) = R.three_view_align_bound(*m4, ih, iw)
    same_bits(got[0], R.scale_to_hr(m4[0], ih, iw, F32), 'three_view_align a1')
    same_bits(got[1], R.scale_to_hr(m4[1], ih, iw, F32), 'three_view_align a2')
    within(got[2], b1, gate_b1, 'three_view_align b1')
    within(got[3], b2, gate_b2, 'three_view_align b2')
    within(got[4], mid, gate_mid, 'three_view_align mid')
    g1 = got[2].cpu().numpy()
    same_bits(got[4], ((R.scale_to_hr(m4[1], ih, iw, F32) + g1) / F32(2.0)).astype(F32), 'three_view_align mid == (a2 + b1) / 2')
    # normalise the five aligned meshes on the first canvas: {a1, b2 | a2, b1 | mid, mid}
    five = [g.cpu().numpy() for g in got]
    bd = T(box).to(dev)
    nrm = ops.three_view_normalize(*[g.view(1, frames, 7, 9, 2) for g in got], bd)
    order = (0, 3, 1, 2, 4, 4)
    same_bits(nrm, np.stack([R.canvas_normalize(five[j], box, F32) for j in order]), 'three_view_normalize')
    want64, bound = (np.stack(x) for x in zip(*[R.canvas_normalize_bound(five[j], box) for j in order]))
    within(nrm, want64, bound, 'three_view_normalize vs float64')
    # back from the canvas' normalised coordinates
    n1, n3 = nrm[0].contiguous(), nrm[1].contiguous()
    fin = ops.three_view_finish(n1, n3, got[4].view(1, frames, 7, 9, 2), bd)
    h1, h3 = n1.cpu().numpy(), n3.cpu().numpy()
    wmin_hmin = np.array([box[0], box[2]], F32)
    for g, w32, (w64, bound), name in ((fin[0], R.canvas_recover(h1, box, F32), R.canvas_recover_bound(h1, box), 'mesh1'),
                                       (fin[2], R.canvas_recover(h3, box, F32), R.canvas_recover_bound(h3, box), 'mesh3'),
                                       (fin[1], (five[4] - wmin_hmin).astype(F32), R.canvas_shift_bound(five[4], wmin_hmin), 'middle')):
        same_bits(g.view(frames, 63, 2), w32, 'three_view_finish ' + name)
        within(g.view(frames, 63, 2), w64, bound, 'three_view_finish %s vs float64' % name)


# ================================================================================================ overflow watcher
@pytest.mark.parametrize('guard', [0.0, 1e-4, 0.02])
def test_canvas_watchers_against_the_documented_update(dev, guard):
    """ss_canvas_watch (a stream per frame of watch_frames, and the frames one after another into one row), ss_canvas_watch_frames (the
    seven frames in one launch, then again on the same row) and ss_stream_normalize_watch's watcher (the same points through an identity
    canvas) == the Python restatement of the header's meaning: counts, the first clipped index 3 (not 0) and its persistence, the
    running extents with the NaN dropped, bit for bit."""
    from stabstitch2_amd import ops
    f = G.watch_frames()
    k = f.shape[0]
    fd = T(f).to(dev)

    def state(n):
        return np.array([[0, 0, -1, 0]] * n, np.int32), np.array([[np.inf, -np.inf, np.inf, -np.inf]] * n, F32)
    # a stream per frame
    wi, wf = state(k)
    R.canvas_watch(f.reshape(k, 126, 2), guard, wi, wf)
    gi, gf = ops.canvas_watch_state(k, dev)
    ops.canvas_watch(fd, gi, gf, guard)
    same_bits(gi, wi, 'canvas_watch counts guard %g' % guard)
    same_bits(gf, wf, 'canvas_watch extents')
    assert wi[:, 1].tolist() == [0, 0, 0, 1, 0, 1, 1] and (guard < 0.02 or wi[:, 3].tolist() == [1, 1, 0, 1, 1, 1, 1])
    # one stream, frame after frame; then the k frames at once; then the same k again (the first clipped index stays)
    wi, wf = state(1)
    gi, gf = ops.canvas_watch_state(1, dev)
    hi, hf = ops.canvas_watch_state(1, dev)
    for rep in range(2):
        for j in range(k):
            R.canvas_watch(f[j].reshape(1, 126, 2), guard, wi, wf)
            ops.canvas_watch(fd[j:j + 1], gi, gf, guard)
        ops.canvas_watch_frames(fd, hi, hf, guard)
        for a, b, name in ((gi, wi, 'canvas_watch row'), (hi, wi, 'canvas_watch_frames row')):
            same_bits(a, b, '%s guard %g pass %d' % (name, guard, rep))
        same_bits(gf, wf, 'canvas_watch extents')
        same_bits(hf, wf, 'canvas_watch_frames extents')
    assert wi[0, :3].tolist() == [2 * k, 6, 3]
    # through ss_stream_normalize_watch on the canvas (-1, 1, -1, 1): ((x + 1) * 2) / 2 - 1 rounds, so the statement is fed the points the
    # launch itself wrote (their normalisation is held bit for bit by test_canvas_normalize_kernels_bit_exact)
    bb = torch.tensor([[-1.0, 1.0, -1.0, 1.0]] * k, device=dev)             # a canvas per stream, all the same
    si, sf = ops.canvas_watch_state(k, dev)
    out = ops.stream_normalize_watch([fd[:, 0].contiguous(), fd[:, 1].contiguous()], 126, bb, 0, 0, guard, si, sf)
    wi, wf = state(k)
    R.canvas_watch(out.cpu().numpy().reshape(k, 126, 2), guard, wi, wf)
    same_bits(si, wi, 'stream_normalize_watch counts')
    same_bits(sf, wf, 'stream_normalize_watch extents')
