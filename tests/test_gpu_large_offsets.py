"""The frame-sized kernels past element 2^31: every case of tests/large_offsets.py (its shapes are checked there without a GPU) takes ONE
buffer of an entry across its line -- element 2^31 of an fp32 or int32 buffer, byte 2^31 or byte 2^32 of a uint8 one -- with one frame
straddling the line and at least one whole frame beyond it, everything else small (a tiny frame under a huge canvas, or a tiny canvas
over huge frames; the views of a clip are one tensor passed for every view).

The reference is the same entry on a small batch that holds copies of the compared frames only (frame 0, the straddling frame, every
frame beyond the line) with their rows of source, T, gains and footprint, and the comparison is bit for bit: the project promises this
identity (a clip call equals its per-frame calls), and the small calls are what the other sweeps hold to float64 or numpy.  No two
frames of a clip are equal, so an index that wraps reads another frame's data and shows as a mismatch.  exposure_update and
multiband_seam couple their frames: their reference is the per-frame sequence with one carried state, and they also run with the
coupling off.  The PSNR / SSIM entry sums in fp64 with atomics: see test_psnr_ssim for its (derived) tolerance.

Every case checks the free device memory first and FAILS (no skip) when it is short, holds at most large_offsets.CAP bytes, and frees
its buffers before it returns.  Canaries surround the outputs that are not themselves the huge buffer where ops takes an out= (the
warps and the elementwise helpers allocate their own).
    python -m pytest tests/test_gpu_large_offsets.py -m gpu -s"""
import gc
import time

import pytest
import torch

import large_offsets as L

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
GUARD = 4096
SENTINEL = {torch.float32: -12345.0, torch.uint8: 0x5A}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    return torch.device('cuda:0')


def cases_of(family):
    return [c.id for c in L.CASES.values() if c.family == family]


# ================================================================================================ the frame of every case
def run_case(cid, body):
    """memory check -> body(case) -> everything freed; prints the case's time and peak memory (LAB_NOTES.md records them)"""
    case = L.CASES[cid]
    gc.collect()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    need = L.peak_bytes(case) + L.slack_bytes(case)
    free, _ = torch.cuda.mem_get_info()
    assert free >= need, 'case %s needs %d bytes of device memory, %d are free' % (cid, need, free)
    torch.cuda.reset_peak_memory_stats()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    body(case)
    torch.cuda.synchronize()
    secs = time.perf_counter() - t0
    peak = torch.cuda.max_memory_allocated() - base
    gc.collect()
    torch.cuda.empty_cache()
    print('\n[large_offsets] %-32s %6.2f s   peak %6.2f GiB   planned %6.2f GiB' % (cid, secs, peak / 2.0 ** 30, need / 2.0 ** 30))
    assert peak <= L.CAP, (cid, peak)
    assert torch.cuda.memory_allocated() <= base + (16 << 20), (cid, 'buffers left behind', torch.cuda.memory_allocated() - base)


def guarded(shape, dtype, dev):
    """-> (buffer with GUARD sentinels either side, its middle as a tensor of `shape`)"""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * GUARD,), SENTINEL[dtype], dtype=dtype, device=dev)
    return buf, buf[GUARD:GUARD + n].view(shape)


def intact(buf, what):
    s = SENTINEL[buf.dtype]
    assert bool((buf[:GUARD] == s).all()) and bool((buf[-GUARD:] == s).all()), (what, 'a canary was overwritten')


def same_frames(got, ref, idx, what):
    """got[k], ref[k] = frame idx[k] of the big call and of the small one: equal bit for bit, and no two of them equal each other"""
    assert len(got) == len(ref) == len(idx)
    for k, f in enumerate(idx):
        assert got[k].shape == ref[k].shape and got[k].dtype == ref[k].dtype, (what, f)
        assert torch.equal(got[k], ref[k]), (what, 'frame %d differs from the small call' % f)
    for k in range(1, len(idx)):
        assert not torch.equal(got[0], got[k]), (what, 'frames 0 and %d came out equal: the inputs are not distinct' % idx[k])


# ================================================================================================ inputs
def pattern_f32(h, w, dev, planes=3):
    """[planes,h,w] fp32, whole numbers in 16..235: a texture with structure in both directions"""
    y = torch.arange(h, device=dev, dtype=torch.float32)[:, None]
    x = torch.arange(w, device=dev, dtype=torch.float32)[None, :]
    cell = torch.floor(x / 8.0) * torch.floor(y / 4.0)            # < 2^24 for every size used here: exact
    out = torch.empty((planes, h, w), device=dev, dtype=torch.float32)
    for c in range(planes):
        torch.add(x * float(3 + 2 * c), y * float(5 + 4 * c), out=out[c])
        out[c].add_(cell).remainder_(220.0).add_(16.0)
    return out


def frame_f32(dst, base, f):
    """dst = frame f of the clip whose frame 0 is `base`: the same texture, another phase (distinct for f < 31)"""
    torch.add(base, 7.0 * f - 16.0, out=dst)
    dst.remainder_(220.0).add_(16.0)


def pattern_u8(rows, cols, dev):
    """[rows,cols] uint8, in uint8 arithmetic throughout (no wider temporary)"""
    r = torch.arange(rows, device=dev)
    c = torch.arange(cols, device=dev)
    out = torch.add((r * 5 % 256).to(torch.uint8)[:, None], (c * 3 % 256).to(torch.uint8)[None, :])
    out.bitwise_xor_(((r >> 2) % 256).to(torch.uint8)[:, None] * ((c >> 3) % 256).to(torch.uint8)[None, :])
    return out


def clip_f32(n, h, w, dev):
    base = pattern_f32(h, w, dev)
    clip = torch.empty((n, 3, h, w), device=dev, dtype=torch.float32)
    for f in range(n):
        frame_f32(clip[f], base, f)
    return clip


def clip_u8(n, rows, cols, dev, shape=None):
    """n frames of rows x cols bytes (frame f = the pattern + 7 f, wrapping), viewed as [n] + shape"""
    base = pattern_u8(rows, cols, dev)
    clip = torch.empty((n, rows, cols), device=dev, dtype=torch.uint8)
    for f in range(n):
        torch.add(base, 7 * f, out=clip[f])
    return clip if shape is None else clip.view((n,) + tuple(shape))


def make_clip(n, h, w, u8, dev):
    return clip_u8(n, h, w * 3, dev, (h, w, 3)) if u8 else clip_f32(n, h, w, dev)


def splines(n, views, dev, seed=0):
    """source [n,V,63,2] (where the frame's rigid mesh lands on the canvas, normalised: view v's frame covers a box of 0.62 x 0.70 of
    the canvas that moves right with v, 2 % jitter per control point, a shift per frame) and T [n,V,2,66]"""
    from stabstitch2_amd import ops
    g = torch.Generator().manual_seed(9100 + seed + 7 * n + views)
    gx, gy = torch.linspace(-1, 1, 9), torch.linspace(-1, 1, 7)
    grid = torch.stack((gx[None, :].expand(7, 9), gy[:, None].expand(7, 9)), -1)               # [7,9,2] (x, y)
    cx, cy = (-0.30, 0.05, 0.32), (-0.10, 0.12, -0.04)
    src = torch.empty((n, views, 7, 9, 2))
    for v in range(views):
        box = grid * torch.tensor([0.62, 0.70]) + torch.tensor([cx[v], cy[v]])
        src[:, v] = box + torch.randn((n, 7, 9, 2), generator=g) * 0.02 + (torch.rand((n, 1, 1, 2), generator=g) - 0.5) * 0.06
    src = src.view(n, views, 63, 2).contiguous().to(dev)
    T = ops.tps_solve_shared(src.view(n * views, 63, 2), grid.reshape(63, 2).contiguous().to(dev)).view(n, views, 2, 66)
    return src, T


def make_gains(n, views, dev, seed=0):
    g = torch.Generator().manual_seed(9200 + seed)
    return (0.8 + 0.4 * torch.rand((n, views, 3), generator=g)).to(dev)


def take(t, idx):
    return None if t is None else t[torch.tensor(idx, device=t.device)].contiguous()


# ================================================================================================ the clip renders
class _TileBlend:
    """ss_linear_clip_set_rows(-1): the 64 x 64-tile form of the clip blend kernel instead of the rolling one (identical output)"""

    def __enter__(self):
        from stabstitch2_amd import _hip
        _hip.lib().ss_linear_clip_set_rows(-1)

    def __exit__(self, *exc):
        from stabstitch2_amd import _hip
        _hip.lib().ss_linear_clip_set_rows(0)


def _clip_render(case, dev, call, again=None):
    """call(views, src, T, gains, out) -> [n, ...]: the big call, then the small one on copies of the compared frames"""
    a = case.args
    n, V = a['frames'], a['views']
    idx = L.compared(case)
    src, T = splines(n, V, dev)
    gains = make_gains(n, V, dev) if a['gains'] else None
    clip = make_clip(n, a['h'], a['w'], a['u8'], dev)
    shape = (n, a['hc'], a['wc'], 3) if a['u8'] else (n, 3, a['hc'], a['wc'])
    buf = None
    if case.buffers['out'].nbytes < (64 << 20):
        buf, out = guarded(shape, clip.dtype, dev)
    else:
        out = torch.empty(shape, device=dev, dtype=clip.dtype)
    def several(r):                        # a call returns out, or (out, mask1 of every blend pass)
        return r if isinstance(r, tuple) else (r,)

    got = [take(r, idx) for r in several(call([clip] * V, src, T, gains, out))]
    if buf is not None:
        intact(buf, case.id)
    if again is not None:                  # the same big call in another form of the kernel, into the same buffer
        with again:
            out.zero_()
            for g, r in zip(got, several(call([clip] * V, src, T, gains, out))):
                same_frames(take(r, idx), g, idx, case.id + ' (second form)')
                del r
    del out, buf
    small = take(clip, idx)
    ref = several(call([small] * V, take(src, idx), take(T, idx), take(gains, idx), None))
    assert len(got) == len(ref) == (2 if case.args.get('masks') else 1)
    for g, r in zip(got, ref):
        same_frames(g, r, idx, case.id)
        assert bool((g[0] != 0).any())


@pytest.mark.parametrize('cid', cases_of('linear_clip'))
def test_linear_clip(dev, cid):
    """ss_render_linear_clip(_u8)(_gains): the workspace W | F | scalars | partials past float 2^31 (10 frames of a 33.5 M-pixel
    canvas), and the view clips past float 2^31 / byte 2^31 / byte 2^32.  Where the workspace crosses, both forms of the blend kernel
    run (the rolling strips and the 64 x 64 tiles), and one of those cases also takes mask1_out [n][V-1][hc][wc]."""
    from stabstitch2_amd import ops

    def body(case):
        a = case.args
        _clip_render(case, dev, lambda views, src, T, gains, out: ops.render_linear_clip(views, src, T, a['hc'], a['wc'], 'NORMAL', out=out,
                                                                                         want_masks=a['masks'], gains=gains),
                     again=_TileBlend() if ('ws', L.L31) in case.crosses else None)
    run_case(cid, body)


@pytest.mark.parametrize('cid', cases_of('average_clip'))
def test_average_clip(dev, cid):
    """ss_render_average_clip(_u8)(_gains), AVERAGE and FEATHER: out past float 2^31 / byte 2^31 / byte 2^32 (one launch, the frame
    in grid.y), and the view clips past the same lines."""
    from stabstitch2_amd import ops

    def body(case):
        a = case.args
        fn = ops.render_average_clip_u8 if a['u8'] else ops.render_average_clip
        _clip_render(case, dev, lambda views, src, T, gains, out: fn(views, src, T, a['hc'], a['wc'], 'NORMAL', out=out, gains=gains,
                                                                     fusion=a['fusion']))
    run_case(cid, body)


@pytest.mark.parametrize('cid', cases_of('linear_frames'))
def test_linear_frames(dev, cid):
    """ss_render_linear_frames(_u8)(_gains) and ss_render_linear_frames_nv12 (its own overload of the warp kernel): ten ragged canvases
    whose W blocks pass float 2^31 -- w_off of the last frames, every f_off (three views) and every partials offset lie beyond it.
    Every frame's output is a buffer of its own, with canaries either side."""
    from stabstitch2_amd import ops

    def body(case):
        a = case.args
        n, V, sizes = a['frames'], a['views'], a['sizes']
        idx = L.compared(case)
        src, T = splines(n, V, dev)
        gains = make_gains(n, V, dev) if a['gains'] else None
        if a['nv12']:
            clip = clip_u8(n, a['h'] * 3 // 2, a['w'], dev)

            def render(views, src, T, sizes, gains, outs):
                return ops.render_linear_frames_nv12(views, src, T, sizes, 'NORMAL', outs=outs)
        else:
            clip = make_clip(n, a['h'], a['w'], a['u8'], dev)

            def render(views, src, T, sizes, gains, outs):
                return ops.render_linear_frames(views, src, T, sizes, 'NORMAL', outs=outs, gains=gains)
        dt = torch.uint8 if a['u8'] else torch.float32
        held = [guarded((hc, wc, 3) if a['u8'] else (3, hc, wc), dt, dev) for hc, wc in sizes]
        render([clip] * V, src, T, sizes, gains, [o for _, o in held])
        for f, (buf, _) in enumerate(held):
            intact(buf, '%s frame %d' % (case.id, f))
        got = [held[f][1].clone() for f in idx]
        del held, buf
        small = take(clip, idx)
        ref = render([small] * V, take(src, idx), take(T, idx), [sizes[f] for f in idx], take(gains, idx), None)
        same_frames(got, ref, idx, case.id)
        assert bool((got[0] != 0).any())
    run_case(cid, body)


# ================================================================================================ MULTIBAND
@pytest.mark.parametrize('cid', cases_of('multiband_warp'))
def test_multiband_warp(dev, cid):
    """ssw_multiband_warp(_u8), with and without gains: P past float 2^31, the frames past float 2^31 / byte 2^31 / byte 2^32."""
    from stabstitch2_amd import ops

    def body(case):
        a = case.args
        n, V = a['frames'], a['views']
        idx = L.compared(case)
        src, T = splines(n, V, dev)
        gains = make_gains(n, V, dev) if a['gains'] else None
        clip = make_clip(n, a['h'], a['w'], a['u8'], dev)
        P = ops.multiband_warp([clip] * V, src, T, a['hc'], a['wc'], 'NORMAL', gains=gains)
        got = take(P, idx)
        del P
        small = take(clip, idx)
        ref = ops.multiband_warp([small] * V, take(src, idx), take(T, idx), a['hc'], a['wc'], 'NORMAL', gains=take(gains, idx))
        same_frames(got, ref, idx, case.id)
        assert bool((got[0, :, 4] > 0.5).any())
    run_case(cid, body)


def _weights(hc, wc, dev):
    x = torch.arange(wc, device=dev, dtype=torch.float32)
    y = torch.arange(hc, device=dev, dtype=torch.float32)
    return torch.minimum(x + 1, wc - x)[None, :] * torch.minimum(y + 1, hc - y)[:, None]


def _fill_P_frame(dst, f, base, wgt):
    """dst [V,5,hc,wc] = frame f of a synthetic warp result: view v covers the columns [x0, x1) (a box that moves with v and f) with
    its own cut of the texture, its weight plane and a mask of ones; 0 elsewhere"""
    V, _, hc, wc = dst.shape
    dst.zero_()
    span = int(0.55 * wc)
    for v in range(V):
        x0 = int(wc * (0.04 + 0.2 * v)) + 8 * f
        x1 = min(x0 + span, wc)
        sh = 37 * v + 3 * f
        dst[v, 0:3, :, x0:x1] = base[:, :, sh:sh + (x1 - x0)]
        dst[v, 0:3, :, x0:x1].add_(float(2 * f))
        dst[v, 3, :, x0:x1] = wgt[:, 0:x1 - x0]
        dst[v, 4, 8 * v:, x0:x1] = 1.0


def _make_P(n, V, hc, wc, dev, frames=None):
    base = pattern_f32(hc, wc, dev)
    wgt = _weights(hc, wc, dev)
    frames = list(range(n)) if frames is None else frames
    P = torch.empty((len(frames), V, 5, hc, wc), device=dev, dtype=torch.float32)
    for k, f in enumerate(frames):
        _fill_P_frame(P[k], f, base, wgt)
    return P


@pytest.mark.parametrize('cid', cases_of('multiband_seam'))
def test_multiband_seam(dev, cid):
    """ssm_multiband_seam: P past float 2^31.  Without a state (the frames are independent) against a small batch of the compared
    frames; with a state (xprev is carried through the call) against the per-frame sequence with one carried state, every frame
    compared and the states equal at the end."""
    from stabstitch2_amd import ops

    def body(case):
        a = case.args
        n, V, hc, wc, cell = a['frames'], a['views'], a['hc'], a['wc'], a['cell']
        idx = L.compared(case)
        base, wgt = pattern_f32(hc, wc, dev), _weights(hc, wc, dev)
        P = torch.empty((n, V, 5, hc, wc), device=dev, dtype=torch.float32)
        for f in range(n):
            _fill_P_frame(P[f], f, base, wgt)
        # coupling off
        ops.multiband_seam(P, cell=cell)
        ref = torch.empty((len(idx), V, 5, hc, wc), device=dev, dtype=torch.float32)
        for k, f in enumerate(idx):
            _fill_P_frame(ref[k], f, base, wgt)
        ops.multiband_seam(ref, cell=cell)
        same_frames([P[f] for f in idx], list(ref), idx, case.id + ' without a state')
        assert float(P[0, :, 3].min()) != float(P[0, :, 3].max())                               # a seam was painted
        del ref
        # coupling on: the call's frames in order, xprev carried
        for f in range(n):
            _fill_P_frame(P[f], f, base, wgt)
        state = ops.seam_state(V, hc, wc, cell, dev)
        ops.multiband_seam(P, cell=cell, state=state)
        state2 = ops.seam_state(V, hc, wc, cell, dev)
        one = torch.empty((1, V, 5, hc, wc), device=dev, dtype=torch.float32)
        for f in range(n):
            _fill_P_frame(one[0], f, base, wgt)
            ops.multiband_seam(one, cell=cell, state=state2)
            assert torch.equal(one[0], P[f]), (case.id, 'with a state: frame %d differs from the per-frame sequence' % f)
        assert torch.equal(state, state2) and int(state[0]) == 1
    run_case(cid, body)


@pytest.mark.parametrize('cid', cases_of('multiband_blend'))
def test_multiband_blend(dev, cid):
    """ssb_multiband_blend(_u8), bands 0 and 2: P past float 2^31, the workspace past float 2^31 (the two grow together: 24 frames of
    a 9.4 M-pixel canvas take both across)."""
    from stabstitch2_amd import ops

    def body(case):
        a = case.args
        n, V, hc, wc, bands, u8 = a['frames'], a['views'], a['hc'], a['wc'], a['bands'], a['u8']
        idx = L.compared(case)
        P = _make_P(n, V, hc, wc, dev)
        dt = torch.uint8 if u8 else torch.float32
        buf, out = guarded((n, hc, wc, 3) if u8 else (n, 3, hc, wc), dt, dev)
        ops.multiband_blend(P, bands, out=out, u8=u8)
        got = take(out, idx)
        intact(buf, case.id)
        del out, buf
        ref = ops.multiband_blend(take(P, idx), bands, u8=u8)
        same_frames(got, ref, idx, case.id)
        assert bool((got[0] != 0).any())
    run_case(cid, body)


# ================================================================================================ the dense warp, exposure
@pytest.mark.parametrize('cid', cases_of('tps_warp'))
def test_tps_warp(dev, cid):
    """ss_tps_warp_nchw / ss_tps_warp_mask_nchw: U past float 2^31 (12 items of three 8192 x 8192 planes), out past float 2^31."""
    from stabstitch2_amd import ops

    def body(case):
        a = case.args
        b = a['frames']
        idx = L.compared(case)
        src, T = splines(b, 1, dev)
        src, T = src.view(b, 63, 2), T.view(b, 2, 66)
        U = clip_f32(b, a['h'], a['w'], dev)
        out = ops.tps_warp(U, src, T, a['hc'], a['wc'], 'NORMAL', with_mask=a['mask'])
        got = take(out, idx)
        del out
        ref = ops.tps_warp(take(U, idx), take(src, idx), take(T, idx), a['hc'], a['wc'], 'NORMAL', with_mask=a['mask'])
        same_frames(got, ref, idx, case.id)
    run_case(cid, body)


@pytest.mark.parametrize('cid', cases_of('exposure_update'))
def test_exposure_update(dev, cid):
    """ss_exposure_update: the view clips past float 2^31 / byte 2^31 / byte 2^32.  The gains smooth through the clip in order: the
    reference is the per-frame sequence with one carried state (every frame compared, the states equal at the end); the per-frame
    sums and targets of the diagnostics do not depend on the state and are compared with a small batch of the compared frames."""
    from stabstitch2_amd import ops

    def body(case):
        a = case.args
        n, V, h, w, hc, wc = a['frames'], a['views'], a['h'], a['w'], a['hc'], a['wc']
        idx = L.compared(case)
        src, T = splines(n, V, dev)
        fp = ops.render_footprints(src, T, h, w, hc, wc)
        params = ops.ExposureParams(alpha=0.25, lo=1.0, hi=254.0, min_nodes=4)
        clip = make_clip(n, h, w, a['u8'], dev)
        state = ops.exposure_state(dev)
        gbuf, gains = guarded((n, V, 3), torch.float32, dev)
        _, diag = ops.exposure_update([clip] * V, fp, hc, wc, state, params, gains=gains, want_diag=True)
        intact(gbuf, case.id)
        assert bool((diag[:, 36] == 1).all()) and bool((diag[:, 0] >= 4).all())               # every frame kept its pair (0, 1)
        state2 = ops.exposure_state(dev)
        one = torch.empty((1,) + tuple(clip.shape[1:]), device=dev, dtype=clip.dtype)
        for f in range(n):
            one[0].copy_(clip[f])
            g1, d1 = ops.exposure_update([one] * V, fp[f:f + 1].contiguous(), hc, wc, state2, params, want_diag=True)
            assert torch.equal(g1[0], gains[f]), (case.id, 'gains of frame %d differ from the per-frame sequence' % f)
            assert torch.equal(d1[0], diag[f]), (case.id, 'sums of frame %d differ from the per-frame sequence' % f)
        assert torch.equal(state, state2)
        del one
        g3, d3 = ops.exposure_update([take(clip, idx)] * V, take(fp, idx), hc, wc, ops.exposure_state(dev), params, want_diag=True)
        same_frames(list(diag[torch.tensor(idx, device=dev)]), list(d3), idx, case.id + ' diagnostics')
        del g3
    run_case(cid, body)


# ================================================================================================ frame I/O
def _lr_out(case, dev):
    n, (lh, lw) = case.args['frames'], case.args['lr']
    if case.buffers['lr'].nbytes < (64 << 20):
        return guarded((n, 3, lh, lw), torch.float32, dev)
    return None, torch.empty((n, 3, lh, lw), device=dev, dtype=torch.float32)


def _ingest(case, dev, frames, call):
    a = case.args
    idx = L.compared(case)
    buf, lr = _lr_out(case, dev)
    hr, lr = call(frames, a['lr'][0], a['lr'][1], a['want_hr'], lr)
    if buf is not None:
        intact(buf, case.id)
    got_lr, got_hr = take(lr, idx), take(hr, idx)
    del hr, lr, buf
    rhr, rlr = call(take(frames, idx), a['lr'][0], a['lr'][1], a['want_hr'], None)
    same_frames(got_lr, rlr, idx, case.id + ' lr')
    if a['want_hr']:
        same_frames(got_hr, rhr, idx, case.id + ' hr')


@pytest.mark.parametrize('cid', cases_of('ingest_u8'))
def test_ingest_u8(dev, cid):
    """ss_ingest_u8: the frames past byte 2^31 (hr past float 2^31 with them) and byte 2^32; four pixels a thread (w % 4 == 0) and one;
    the general resize and the exact 2 x 2 one."""
    from stabstitch2_amd import ops

    def body(case):
        a = case.args
        frames = make_clip(a['frames'], a['h'], a['w'], True, dev)
        _ingest(case, dev, frames, lambda fr, lh, lw, want, lr: ops.ingest_u8(fr, lh, lw, want_hr=want, lr_out=lr))
    run_case(cid, body)


@pytest.mark.parametrize('cid', cases_of('ingest_nv12'))
def test_ingest_nv12(dev, cid):
    """ss_ingest_nv12: hr past float 2^31; the NV12 frames (16384 x 16384: 403 MB each) past byte 2^31 and byte 2^32."""
    from stabstitch2_amd import ops

    def body(case):
        a = case.args
        frames = clip_u8(a['frames'], a['h'] * 3 // 2, a['w'], dev)
        _ingest(case, dev, frames, lambda fr, lh, lw, want, lr: ops.ingest_nv12(fr, lh, lw, want_hr=want, lr_out=lr))
    run_case(cid, body)


@pytest.mark.parametrize('cid', cases_of('canvas_to_u8'))
def test_canvas_to_u8(dev, cid):
    """ss_canvas_to_u8: the canvases past float 2^31 and the frames past byte 2^31 with them; four pixels a thread and one."""
    from stabstitch2_amd import ops

    def body(case):
        a = case.args
        idx = L.compared(case)
        canvas = clip_f32(a['frames'], a['h'], a['w'], dev)
        canvas[:, :, 0, :7] = torch.tensor([-1.5, 255.9, 256.0, 300.25, -300.0, 1e10, float('nan')], device=dev)      # the wrap and its edge
        out = ops.canvas_to_u8(canvas)
        got = take(out, idx)
        del out
        same_frames(got, ops.canvas_to_u8(take(canvas, idx)), idx, case.id)
    run_case(cid, body)


@pytest.mark.parametrize('cid', cases_of('bgr_to_nv12'))
def test_bgr_to_nv12(dev, cid):
    """ss_bgr_to_nv12: the BGR frames past byte 2^31 and 2^32, the NV12 frames past byte 2^31 and 2^32."""
    from stabstitch2_amd import ops

    def body(case):
        a = case.args
        idx = L.compared(case)
        bgr = make_clip(a['frames'], a['h'], a['w'], True, dev)
        out = ops.bgr_to_nv12(bgr)
        got = take(out, idx)
        del out
        same_frames(got, ops.bgr_to_nv12(take(bgr, idx)), idx, case.id)
    run_case(cid, body)


# ================================================================================================ elementwise over n
def _blocks(nblocks, block, dev, scale, wrap=None):
    """[nblocks, block] fp32, block f = a ramp (optionally wrapped) + f: no two blocks equal"""
    ramp = torch.arange(block, device=dev, dtype=torch.float32)
    if wrap:
        ramp.remainder_(float(wrap))
    ramp.mul_(scale)
    x = torch.empty((nblocks, block), device=dev, dtype=torch.float32)
    for f in range(nblocks):
        torch.add(ramp, f * scale * 3.0, out=x[f])
    return x


@pytest.mark.parametrize('cid', cases_of('add_mul'))
def test_add_mul(dev, cid):
    """ss_add_mul over n = 34 (2^26 + 1) > 2^31 elements; the compared blocks against the same entry on their copies."""
    from stabstitch2_amd import ops

    def body(case):
        n, block = case.args['frames'], case.args['block']
        idx = L.compared(case)
        x = _blocks(n, block, dev, 0.5)
        out = ops.add_mul(x.view(-1), 1.5, 0.75).view(n, block)
        got = take(out, idx)
        del out
        ref = ops.add_mul(take(x, idx).view(-1), 1.5, 0.75).view(len(idx), block)
        same_frames(got, ref, idx, case.id)
    run_case(cid, body)


@pytest.mark.parametrize('cid', cases_of('mask_union'))
def test_mask_union(dev, cid):
    """ss_mask_union over n > 2^31: a and b are one buffer read one block apart."""
    from stabstitch2_amd import ops

    def body(case):
        n, block = case.args['frames'], case.args['block']
        idx = L.compared(case)
        ab = _blocks(n + 1, block, dev, 1.0 / 1024.0, wrap=1000)
        flat = ab.view(-1)
        out = ops.mask_union(flat[:n * block], flat[block:]).view(n, block)
        got = take(out, idx)
        del out
        ref = ops.mask_union(take(ab, idx).view(-1), take(ab, [f + 1 for f in idx]).view(-1)).view(len(idx), block)
        same_frames(got, ref, idx, case.id)
    run_case(cid, body)


@pytest.mark.parametrize('cid', cases_of('fill'))
def test_fill(dev, cid):
    """ss_fill_f32 over n > 2^31, a block of canaries either side."""
    from stabstitch2_amd import ops

    def body(case):
        n, block = case.args['frames'], case.args['block']
        idx = L.compared(case)
        whole = torch.full(((n + 2) * block,), -7.0, device=dev, dtype=torch.float32)
        p = whole[block:(n + 1) * block]
        ops.fill(p, 3.25)
        small = ops.fill(torch.empty(block, device=dev, dtype=torch.float32), 3.25)
        for f in range(n):                                   # every block, not only the compared ones: it costs nothing here
            assert torch.equal(p[f * block:(f + 1) * block], small), (case.id, 'block %d' % f)
        assert idx[-1] == n - 1
        assert bool((whole[:block] == -7.0).all()) and bool((whole[(n + 1) * block:] == -7.0).all()), 'a canary was overwritten'
    run_case(cid, body)


# ================================================================================================ the metric
@pytest.mark.parametrize('cid', cases_of('psnr_ssim'))
def test_psnr_ssim(dev, cid):
    """ss_alignment_psnr_ssim: both stacks past float 2^31 (14 frames of one buffer of 15, read one frame apart).

    The entry adds its per-workgroup sums with fp64 atomics, so its result is not a function of the inputs alone.  The planes here
    hold whole numbers and the masks 0 or 1: every squared error is an integer and their sum stays below 2^53, so PSNR is exact in any
    order and is compared bit for bit.  SSIM is a mean of terms in [-1, 1]: B = ceil(w / 64) ceil(h / 4) partial sums added in any
    order differ by at most (B - 1) 2^-53 times the sum of their magnitudes, which the mean's divisor takes back to at most B 2^-53;
    two runs differ by at most twice that.  B = 167 936 here: 3.7e-11."""
    from stabstitch2_amd import metrics

    def body(case):
        n, h, w = case.args['frames'], case.args['h'], case.args['w']
        idx = L.compared(case)
        base = pattern_f32(h, w, dev)
        buf = torch.zeros((n + 1, 4, h, w), device=dev, dtype=torch.float32)
        for f in range(n + 1):
            frame_f32(buf[f, 0:3], base, f)
            buf[f, 3, 16 + 8 * f:h - 24, 40 + 16 * f:w - 8] = 1.0
        del base
        psnr, ssim = metrics.alignment_psnr_ssim(buf[:n], buf[1:])
        assert bool(torch.isfinite(psnr).all()) and bool(torch.isfinite(ssim).all())
        pairs = take(buf, sorted({f for i in idx for f in (i, i + 1)}))       # frames 0, 1 | s, s + 1, .. , n: the compared pairs
        where = {f: k for k, f in enumerate(sorted({f for i in idx for f in (i, i + 1)}))}
        tol = 2.0 * (-(-w // 64)) * (-(-h // 4)) * 2.0 ** -53
        for i in idx:
            p1, s1 = metrics.alignment_psnr_ssim(pairs[where[i]:where[i] + 1], pairs[where[i + 1]:where[i + 1] + 1])
            assert float(p1[0]) == float(psnr[i]), (case.id, 'PSNR of frame %d' % i, float(p1[0]), float(psnr[i]))
            assert abs(float(s1[0]) - float(ssim[i])) <= tol, (case.id, 'SSIM of frame %d' % i, float(s1[0]), float(ssim[i]), tol)
        assert len({float(v) for v in psnr[torch.tensor(idx, device=dev)]}) == len(idx)       # distinct frames, distinct results
    run_case(cid, body)
