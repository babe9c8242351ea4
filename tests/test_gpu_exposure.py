"""Exposure compensation on the device: ss_exposure_update against its float64 statement (tests/exposure_ref.py) on lattices read
back from ops.render_footprints; every gain-taking render against the plain entry points and the per-frame chains; OnlineStitcher
with exposure= against a by-hand chain of its own splines, and its contracts with exposure on.
    python -m pytest tests -m gpu"""
import gc

import numpy as np
import pytest
import torch

import exposure_ref as E
from stabstitch2_amd import synth
from test_gpu_parity import dev, hip_nets  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
F = np.float32
NF = 5                                     # frames per kernel case; frame 2 has no overlap at all
# (frame h, w, canvas hc, wc, view rectangles on the canvas (x0, x1) for V = 2 and V = 3): odd frames, canvases that are no
# multiples of 64 x 8 -- the lattice's last row and column lie beyond them, partial tiles on two sides
CASES = {
    'a': (37, 53, 45, 150, {2: [(0, 110), (40, 150)], 3: [(0, 70), (40, 110), (80, 150)]}),       # V = 3: a chain, (0, 2) never meet
    'b': (48, 64, 70, 97, {2: [(-2, 80), (20, 99)], 3: [(-2, 70), (20, 99), (28, 99)]}),
}
APART = {2: [(0, 60), (90, 150)], 3: [(0, 40), (55, 95), (110, 150)]}                          # no two views overlap
# A lattice of more than 256 nodes (tests/test_gpu_stream_sweeps.py; not in CASES: the render tests above walk CASES): 27 x 13 nodes
# on canvas (201, 330), the views' x edges on odd multiples of 16 and their frames 16 px taller than the canvas on either side, so
# that no node (32 j, 8 i) on the canvas is within 12 px of a view's border in any frame (the jitter is +- 1 px); the sixth entry is
# the apart rectangles of frame 2, the seventh the vertical margin
WIDE_CASES = {
    'c': (37, 53, 201, 330, {2: [(-16, 240), (80, 336)], 3: [(-16, 176), (80, 272), (208, 336)]},
          {2: [(-16, 112), (208, 336)], 3: [(-16, 80), (112, 208), (240, 336)]}, 16.0),
}
_cache = {}


def _meshes(dev, g, h, w, hc, rects, n, apart_at=None, apart=None, margin=3.0):
    """Per view [n,7,9,2] LR-scale meshes that put the frame on the canvas rectangle rects[v] x (-margin, hc + margin), jittered by
    +- 1 px."""
    out = []
    ty, tx = torch.meshgrid(torch.linspace(0, 1, 7), torch.linspace(0, 1, 9), indexing='ij')
    for v, rect in enumerate(rects):
        per = []
        for f in range(n):
            x0, x1 = (apart[v] if f == apart_at else rect)
            m = torch.stack((x0 + (x1 - x0) * tx, -margin + (hc + 2.0 * margin) * ty), -1) + (torch.rand((7, 9, 2), generator=g) - 0.5) * 2.0
            per.append(m * torch.tensor([480.0 / w, 360.0 / h]))
        out.append(torch.stack(per).contiguous().to(dev))
    return out


def _inputs(dev, name, views):
    """The seeded frames and meshes of a case on `dev` (the CPU will do) -> dict(f32, u8, meshes, h, w, hc, wc)."""
    if name in CASES:
        h, w, hc, wc, rects = CASES[name]
        apart, margin = {k: [(a * wc / 150.0, b * wc / 150.0) for a, b in r] for k, r in APART.items()}, 3.0
    else:
        h, w, hc, wc, rects, apart, margin = WIDE_CASES[name]
    g = torch.Generator().manual_seed(77 + 13 * views + ord(name))
    f32 = []
    for v in range(views):
        # smooth-ish texture: a coarse random grid upsampled, so neighbouring taps differ but no sample leaves [16, 235]
        coarse = torch.rand((NF, 3, h // 4 + 2, w // 4 + 2), generator=g)
        img = torch.nn.functional.interpolate(coarse, size=(h, w), mode='bilinear', align_corners=True)
        img = 16.0 + 219.0 * img
        if v == 1:
            img = 16.0 + 0.75 * (img - 16.0)
        f32.append(img.contiguous().to(dev))
    u8 = [x.permute(0, 2, 3, 1).round().clamp(0, 255).to(torch.uint8).contiguous() for x in f32]
    meshes = _meshes(dev, g, h, w, hc, rects[views], NF, apart_at=2, apart=apart[views], margin=margin)
    return dict(f32=f32, u8=u8, meshes=meshes, h=h, w=w, hc=hc, wc=wc)


def _case(dev, name, views):
    """-> dict(f32: V x [NF,3,h,w] in [16, 235], view 1 darker; u8: their rounding [NF,h,w,3]; src, T, fp [NF, .]; h, w, hc, wc)."""
    key = (name, views)
    if key not in _cache:
        from stabstitch2_amd import ops
        from stabstitch2_amd.spatial_network import get_rigid_mesh, get_norm_mesh
        c = _inputs(dev, name, views)
        h, w, hc, wc = c['h'], c['w'], c['hc'], c['wc']
        box = torch.tensor([0.0, float(wc), 0.0, float(hc)], device=dev)
        nrigid = get_norm_mesh(get_rigid_mesh(1, h, w, device=dev), h, w).contiguous()
        src, T = ops.stream_splines(c['meshes'], 126, box.repeat(NF, 1).contiguous(), nrigid, h, w)
        fp = ops.render_footprints(src, T, h, w, hc, wc)
        _cache[key] = dict(c, src=src, T=T, fp=fp)
    return _cache[key]


def _planes(c, u8, f, v):
    """Frame f of view v as the [3,h,w] array the float64 statement samples (uint8 -> fp32 is exact)."""
    if u8:
        return c['u8'][v][f].permute(2, 0, 1).cpu().numpy().astype(np.float64)
    return c['f32'][v][f].cpu().numpy().astype(np.float64)


def _diag_stats(d, views):
    return {p: (int(d[i * 9]), d[i * 9 + 1:i * 9 + 9:3].copy(), d[i * 9 + 2:i * 9 + 9:3].copy()) for i, p in enumerate(E.PAIRS[views])}


def _ulps(a, b):
    a, b = np.asarray(a, F), np.asarray(b, F)
    return float(np.max(np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.abs(b))))


# ================================================================================================ the estimator
def check_estimator(dev, name, views, u8, mode, ranges=None):
    """The body of test_statistics_targets_and_smoothing on case `name`.  ranges: index ranges [(first, last + 1)] of the lattice
    (node (i, j) has index i nx + j) in each of which pair (0, 1) must have at least 8 usable nodes in every frame with an overlap
    -> per frame and range, the number of usable nodes of pair (0, 1)."""
    from stabstitch2_amd import ops
    c = _case(dev, name, views)
    h, w, hc, wc = c['h'], c['w'], c['hc'], c['wc']
    P = ops.ExposureParams(min_nodes=4)
    imgs = c['u8'] if u8 else c['f32']
    st = ops.exposure_state(dev)
    gains, diag = ops.exposure_update(imgs, c['fp'], hc, wc, st, P, mode, want_diag=True)
    gains, diag, fp = gains.cpu().numpy(), diag.cpu().numpy(), c['fp'].cpu().numpy()
    s, started, kept_frames, reached = np.ones((views, 3), F), False, 0, []
    for f in range(NF):
        lat = E.footprint_lattice(fp[f], views, hc, wc)
        ref, use, smp = E.statistics([_planes(c, u8, f, v) for v in range(views)], lat, hc, wc, mode, P.lo, P.hi)
        oc = E.on_canvas(hc, wc)
        for v in range(views):                       # the margin to the thresholds, on every node that could count
            ins = oc & (np.abs(lat[v, ..., 0]) <= 1) & (np.abs(lat[v, ..., 1]) <= 1)
            assert (np.abs(smp[v][:, ins] - P.lo) >= 1.0).all() and (np.abs(smp[v][:, ins] - P.hi) >= 1.0).all(), (f, v)
        dev_stats = _diag_stats(diag[f], views)
        for p in E.PAIRS[views]:
            n, sa, sb = ref[p]
            assert dev_stats[p][0] == n, (f, p, dev_stats[p][0], n)
            bound = n * (8 * (w + h) + 19) * 255.0 * 2.0 ** -24
            assert np.abs(dev_stats[p][1] - sa).max() <= bound and np.abs(dev_stats[p][2] - sb).max() <= bound, (f, p, bound)
        if f == 2:
            assert all(ref[p][0] == 0 for p in E.PAIRS[views]), f
        else:
            assert ref[(0, 1)][0] >= P.min_nodes, (f, ref[(0, 1)][0])
        if name in ('a', 'c') and views == 3:
            assert ref[(0, 2)][0] == 0                # the chain with one pair missing
        if ranges is not None:
            per = [int(use[(0, 1)].reshape(-1)[a:b].sum()) for a, b in ranges]
            assert f == 2 or min(per) >= 8, (f, per)
            reached.append(per)
        want, kept = E.targets(dev_stats, views, P.sigma_n, P.sigma_g, P.min_nodes, P.gain_min, P.gain_max)
        got_t = diag[f, 27:27 + views * 3].reshape(views, 3)
        assert bool(diag[f, 36]) == kept and _ulps(got_t, want) <= 2.0, (f, got_t, want)
        kept_frames += kept
        s, started = E.smooth(s, started, got_t, kept, P.alpha)
        assert np.array_equal(gains[f], s), (f, gains[f], s)
    assert kept_frames == NF - 1 and float(np.abs(gains[-1] - 1).max()) > 0.01
    assert np.array_equal(st[:views * 3].cpu().numpy().reshape(views, 3), s) and int(st.view(torch.int32)[9]) == 1
    # five calls of one frame; and the same call again
    st1 = ops.exposure_state(dev)
    for f in range(NF):
        g1, d1 = ops.exposure_update([x[f:f + 1] for x in imgs], c['fp'][f:f + 1], hc, wc, st1, P, mode, want_diag=True)
        assert np.array_equal(g1.cpu().numpy()[0], gains[f]) and np.array_equal(d1.cpu().numpy()[0], diag[f]), f
    assert torch.equal(st1, st)
    st2 = ops.exposure_state(dev)
    g2, d2 = ops.exposure_update(imgs, c['fp'], hc, wc, st2, P, mode, want_diag=True)
    assert np.array_equal(g2.cpu().numpy(), gains) and np.array_equal(d2.cpu().numpy(), diag) and torch.equal(st2, st)
    return reached


@pytest.mark.parametrize('mode', ['NORMAL', 'FAST'])
@pytest.mark.parametrize('u8', [False, True], ids=['fp32', 'uint8'])
@pytest.mark.parametrize('views', [2, 3])
@pytest.mark.parametrize('name', ['a', 'b'])
def test_statistics_targets_and_smoothing(dev, name, views, u8, mode):
    """Five frames in one call.  Counts equal the numpy statement on the lattice read back, exactly; sums within
    n (8 (w + h) + 19) 255 2^-24 of float64 bilinear sampling: the fp32 pixel coordinate x = (xn + 1) w / 2 carries two roundings of
    a number <= w (2 u w with u = 2^-24; likewise y), each of the four tap weights is a product of two differences (u each, plus
    the coordinate's error) rounded once -- <= 2 u (w + h) + 3 u per weight on values <= 255 -- then four products (u each) and three
    additions (u each): 255 u [4 (2 (w + h) + 3) + 4 + 3]; the fp64 accumulation adds nothing visible.  Targets within 2 fp32 ulp
    of the float64 solve of the device's statistics; the smoothed sequence equals its fp32 statement bit for bit; one call of five
    frames equals five calls of one; two runs are bit-identical.  No sample of a counted or uncounted node is within one grey level
    of lo or hi (checked on the float64 statement), so no case passes by leaving nodes out."""
    check_estimator(dev, name, views, u8, mode)


@pytest.mark.parametrize('u8', [False, True], ids=['fp32', 'uint8'])
def test_thresholds_and_empty_overlaps(dev, u8):
    """View 0 carries a block of 0 and a block of 255, each a lattice cell wide on the canvas (frame columns 8..22 and 23..38 land
    on canvas x = 17..47 and 48..80: the nodes at x = 32 and x = 64 sit 15 px inside them): those nodes leave the count, which still
    equals the statement's.  No overlap at all, and an overlap of fewer than min_nodes nodes: gains of 1, state untouched, started
    flag clear."""
    from stabstitch2_amd import ops
    c = _case(dev, 'a', 2)
    h, w, hc, wc = c['h'], c['w'], c['hc'], c['wc']
    P = ops.ExposureParams(min_nodes=2)
    f = 0
    img0 = c['f32'][0][f:f + 1].clone()
    img0[..., 8:23] = 0.0
    img0[..., 23:39] = 255.0
    views = [img0, c['f32'][1][f:f + 1]]
    if u8:
        views = [x.permute(0, 2, 3, 1).round().clamp(0, 255).to(torch.uint8).contiguous() for x in views]
    lat = E.footprint_lattice(c['fp'][f].cpu().numpy(), 2, hc, wc)
    arrs = [(x[0].permute(2, 0, 1) if u8 else x[0]).cpu().numpy().astype(np.float64) for x in views]
    for mode in ('NORMAL', 'FAST'):
        ref, use, smp = E.statistics(arrs, lat, hc, wc, mode, P.lo, P.hi)
        plain = E.statistics([_planes(c, u8, f, 0), arrs[1]], lat, hc, wc, mode, P.lo, P.hi)[0]
        st = ops.exposure_state(dev)
        _, diag = ops.exposure_update(views, c['fp'][f:f + 1], hc, wc, st, P, mode, want_diag=True)
        n = int(diag[0, 0])
        assert n == ref[(0, 1)][0] and 0 < n < plain[(0, 1)][0], (mode, n, ref[(0, 1)][0], plain[(0, 1)][0])
        cols = np.nonzero(use[(0, 1)].any(0))[0].tolist()
        assert 1 not in cols and 2 not in cols, cols               # lattice columns 1, 2 = canvas x 32, 64
        ins = (np.abs(lat[0, ..., 0]) <= 1) & (np.abs(lat[0, ..., 1]) <= 1) & E.on_canvas(hc, wc)
        assert (smp[0][:, ins & (np.arange(lat.shape[2]) == 1)[None, :]] < 1.0).all()
        assert (smp[0][:, ins & (np.arange(lat.shape[2]) == 2)[None, :]] > 254.0).all()
    fresh = ops.exposure_state(dev)
    for frames, P2 in ((2, ops.ExposureParams(min_nodes=2)), (0, ops.ExposureParams())):       # frame 2: apart; frame 0: 12 nodes < 16
        imgs = [x[frames:frames + 1] for x in (c['u8'] if u8 else c['f32'])]
        st = ops.exposure_state(dev)
        g, diag = ops.exposure_update(imgs, c['fp'][frames:frames + 1], hc, wc, st, P2, 'NORMAL', want_diag=True)
        assert float(diag[0, 36]) == 0.0 and int(diag[0, 0]) < P2.min_nodes and (frames == 2) == (int(diag[0, 0]) == 0)
        assert bool((g == 1).all()) and torch.equal(st, fresh) and int(st.view(torch.int32)[9]) == 0


# ================================================================================================ the renders
def average_formula(w):
    f = w[0] * (w[0] / (w[0] + w[1] + 1e-6)) + w[1] * (w[1] / (w[0] + w[1] + 1e-6))
    for k in range(2, w.shape[0]):
        f = f * (f / (f + w[k] + 1e-6)) + w[k] * (w[k] / (f + w[k] + 1e-6))
    return f


def _renders(ops, c, imgs, mode, gains, footprint):
    """Every render form on the case's NF frames -> dict name -> [NF, ...] tensor; gains [NF,V,3] | None; footprint: bool."""
    hc, wc, src, T = c['hc'], c['wc'], c['src'], c['T']
    u8 = imgs[0].dtype == torch.uint8
    fp = c['fp'] if footprint else None
    g = (lambda f: None) if gains is None else (lambda f: gains[f])
    one = ops.render_average_u8 if u8 else ops.render_average
    clip = ops.render_average_clip_u8 if u8 else ops.render_average_clip
    out = {'average': torch.stack([one([x[f] for x in imgs], src[f], T[f], hc, wc, mode, footprint=None if fp is None else fp[f],
                                       gains=g(f)) for f in range(NF)]),
           'average_clip': clip(imgs, src, T, hc, wc, mode, footprint=fp, gains=gains)}
    if not footprint:
        out['linear_clip'] = ops.render_linear_clip(imgs, src, T, hc, wc, mode, gains=gains)
        out['linear_frames'] = torch.stack(ops.render_linear_frames(imgs, src, T, [(hc, wc)] * NF, mode, gains=gains))
    return out


def _distinct_gains(dev, views, values):
    """[NF,V,3]: a different value per view and channel, rotated from frame to frame."""
    v = torch.tensor(values, dtype=torch.float32)
    return torch.stack([v.roll(f)[:views * 3].reshape(views, 3) for f in range(NF)]).contiguous().to(dev)


@pytest.mark.parametrize('mode', ['NORMAL', 'FAST'])
@pytest.mark.parametrize('u8', [False, True], ids=['fp32', 'uint8'])
@pytest.mark.parametrize('views', [2, 3])
def test_gain_renders_reduce_to_the_plain_renders(dev, views, u8, mode):
    """Every gain form (AVERAGE single frame and clip, with and without footprints; LINEAR clip and frames) on both canvases:
    gains of exactly 1 (inputs <= 235) are bit-identical to the entry point without gains; power-of-two gains, a different one per
    view and channel, equal the plain render of the pre-scaled frames bit for bit (fp32 planes <= 60 with 2^-6 .. 2^2; uint8 frames
    <= 63 with gains from {1, 2, 4}, pre-multiplied bytes)."""
    from stabstitch2_amd import ops
    for name in CASES:
        c = _case(dev, name, views)
        imgs = c['u8'] if u8 else c['f32']
        ones = torch.ones((NF, views, 3), device=dev)
        if u8:
            small = [(x // 4).contiguous() for x in imgs]                            # <= 58
            gains = _distinct_gains(dev, views, [1.0, 2.0, 4.0, 2.0, 4.0, 1.0, 4.0, 1.0, 2.0])
            pre = [(x.permute(0, 3, 1, 2).float() * gains[:, v, :, None, None]).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
                   for v, x in enumerate(small)]
        else:
            small = [(x * (60.0 / 235.0)).contiguous() for x in imgs]
            gains = _distinct_gains(dev, views, [2.0 ** k for k in (-6, -5, -4, -3, -2, -1, 0, 1, 2)])
            pre = [(x * gains[:, v, :, None, None]).contiguous() for v, x in enumerate(small)]
        assert float(max(p.max() for p in pre)) <= 255.0 and len(set(gains[0].flatten().tolist())) == (3 if u8 else views * 3)
        for footprint in (False, True):
            plain, unit = _renders(ops, c, imgs, mode, None, footprint), _renders(ops, c, imgs, mode, ones, footprint)
            scaled, want = _renders(ops, c, small, mode, gains, footprint), _renders(ops, c, pre, mode, None, footprint)
            for k in plain:
                assert torch.equal(unit[k], plain[k]), ('unit gains', name, k, footprint)
                assert torch.equal(scaled[k], want[k]), ('power-of-two gains', name, k, footprint)
                assert float(want[k].float().abs().max()) > 1.0


@pytest.mark.parametrize('mode', ['NORMAL', 'FAST'])
@pytest.mark.parametrize('views', [2, 3])
def test_general_gains_equal_the_per_frame_chains(dev, views, mode):
    """Gains in 0.6 .. 1.7, fp32 planes and uint8 frames, both canvases.  LINEAR (clip and frames): bit-identical to tps_warp_views
    -> fp32 multiply of the three colour planes by the gains -> min(., 255) -> linear_blend (-> mask_union -> linear_blend).
    AVERAGE (single frame and clip, no footprint): bit-identical to the AVERAGE formula on tps_warp's per-view warps with the gain
    and the clamp applied to the warped value -- the identity test_gpu_kernel_sweeps holds the plain render to (bound 0), whose
    per-view warps that module holds to ref64's float64 sampler; the uint8 forms are canvas_to_u8 of it."""
    from stabstitch2_amd import ops
    cap = torch.tensor(255.0, device=dev)
    for name in CASES:
        c = _case(dev, name, views)
        hc, wc, src, T = c['hc'], c['wc'], c['src'], c['T']
        g = torch.Generator().manual_seed(5 + views)
        gains = (0.6 + 1.1 * torch.rand((NF, views, 3), generator=g)).to(dev)
        planes = [ops.ingest_u8(x)[0] for x in c['u8']]                               # the uint8 frames' fp32 planes (exact)
        for u8 in (False, True):
            imgs = c['u8'] if u8 else c['f32']
            src_planes = planes if u8 else c['f32']
            lin, avg = [], []
            for f in range(NF):
                wv = ops.tps_warp_views([x[f] for x in src_planes], src[f], T[f], hc, wc, mode)
                col = torch.minimum(wv[:, 0:3] * gains[f][:, :, None, None], cap)
                res = ops.linear_blend(col[0].contiguous(), col[1].contiguous(), wv[0, 3], wv[1, 3])
                if views == 3:
                    res = ops.linear_blend(res, col[2].contiguous(), ops.mask_union(wv[0, 3], wv[1, 3]), wv[2, 3])
                lin.append(res)
                w1 = ops.tps_warp(torch.stack([x[f] for x in src_planes]), src[f], T[f], hc, wc, mode)
                avg.append(average_formula(torch.minimum(w1 * gains[f][:, :, None, None], cap)))
            lin, avg = torch.stack(lin), torch.stack(avg)
            if u8:
                lin, avg = ops.canvas_to_u8(lin), ops.canvas_to_u8(avg)
            got = _renders(ops, c, imgs, mode, gains, False)
            assert torch.equal(got['linear_clip'], lin) and torch.equal(got['linear_frames'], lin), (name, u8)
            assert torch.equal(got['average'], avg) and torch.equal(got['average_clip'], avg), (name, u8)
            assert float((lin.float() - _renders(ops, c, imgs, mode, None, False)['linear_clip'].float()).abs().max()) > 1.0


@pytest.mark.parametrize('views', [2, 3])
def test_clamp_keeps_highlights_at_255(dev, views):
    """Frames of constant 200 under a gain of 2: 400 would wrap to 144 in the uint8 sink.  No byte falls below the render without
    gains -- LINEAR: anywhere; AVERAGE: wherever some view's sample is >= 1 (where every view is outside its image the fusion's
    a a / (a + b + 1e-6) is singular on the samplers' +-1e-5 residues: isolated bytes of any value, with or without gains).  AVERAGE: wherever every view's own sample (ops.tps_warp_views on the same frames: the render's sampler) is
    either >= 199.99 or exactly 0, with at least one of the former -- the 200-valued region, whichever views cover it -- every byte is
    255: 255 255 / (255 + 255 + 1e-6) twice and 255 255 / (255 + 0 + 1e-6) + 0 are exact in fp32.  (Elsewhere the NORMAL sampler's
    rounding residue outside a view's image, ~1e-5, enters the fusion's denominator and the byte may be 254.)  LINEAR: the blend is
    linear in the views' colours with the masks' weights, which gains do not touch, and every sample s <= 200 (1 + 1e-6) becomes
    min(2 s, 255) >= 1.2749 s: a value >= 199 without gains is >= 253.7 with them, one >= 200 is >= 254.9 (the weights themselves
    need not sum to 1: the blender's ramp carries a 1e-3 guard) -- bytes >= 253 and >= 254."""
    from stabstitch2_amd import ops
    c = _case(dev, 'a', views)
    hc, wc = c['hc'], c['wc']
    imgs = [torch.full_like(x, 200) for x in c['u8']]
    planes = [torch.full_like(x, 200.0) for x in c['f32']]
    gains = torch.full((NF, views, 3), 2.0, device=dev)
    for mode in ('NORMAL', 'FAST'):
        region, content = [], []
        for f in range(NF):
            wv = ops.tps_warp_views([x[f] for x in planes], c['src'][f], c['T'][f], hc, wc, mode)[:, 0:3]
            full = wv >= 199.99
            region.append(((full | (wv == 0)).all(0) & full.any(0)).permute(1, 2, 0))           # [hc,wc,3], the uint8 frames' layout
            content.append((wv >= 1.0).any(0).permute(1, 2, 0))
        region = torch.stack(region)
        assert int(region.sum()) > 10000, (mode, int(region.sum()))
        content = torch.stack(content)
        for footprint in (False, True):
            plain, got = _renders(ops, c, imgs, mode, None, footprint), _renders(ops, c, imgs, mode, gains, footprint)
            for k in plain:
                p, q = plain[k].int(), got[k].int()
                where = content if k.startswith('average') else torch.ones_like(content)
                assert bool((q >= p)[where].all()), (mode, k, 'wrapped bytes')
                if k.startswith('average'):
                    assert bool((p[region] >= 199).all()) and bool((q[region] == 255).all()), (mode, k, footprint)
                else:
                    assert int((p >= 199).sum()) > 10000 and bool((q[p >= 199] >= 253).all()) and bool((q[p >= 200] >= 254).all()), (mode, k)


# ================================================================================================ the stitcher
SH, SW, PUSHES = 180, 320, 12              # the streaming tests' size; 7 window-fill pushes + 5 steady-state ones
SCALE = (0.8, 0.9, 1.1)                    # view 2's channels before ingest
_runs = {}


@pytest.fixture(autouse=True)
def _no_garbage_inside_a_capture():
    """A stitcher that became cyclic garbage still owns HIP graphs; the collector must not meet it while another stitcher's graph
    is being captured (freeing device memory is not allowed then): collect between the tests, where nothing captures."""
    gc.collect()
    yield
    gc.collect()


def _stream(dev, scale=SCALE):
    """-> (u8 [2,N,SH,SW,3], hr [2,N,3,SH,SW], lr [2,N,3,360,480]): the synthetic clip, view 2 scaled per channel, rounded to the
    bytes a decoder would deliver, and ingest_u8's planes of those bytes (so push and push_u8 see the same frames)."""
    key = ('stream', scale)
    if key not in _runs:
        from stabstitch2_amd import ops, pipeline
        hr, _ = synth.make_clip_device(PUSHES, SH, SW, seed=4, views=2, device=dev)
        hr[1] = hr[1] * torch.tensor(scale, device=dev).view(1, 3, 1, 1)
        u8 = hr.permute(0, 1, 3, 4, 2).round().clamp(0, 255).to(torch.uint8).contiguous()
        loaded = [ops.ingest_u8(u8[v], pipeline.LR_H, pipeline.LR_W) for v in range(2)]
        _runs[key] = (u8, torch.stack([x[0] for x in loaded]), torch.stack([x[1] for x in loaded]))
    return _runs[key]


def _push_all(st, dev, scale=SCALE, u8=False, n=PUSHES):
    frames8, hr, lr = _stream(dev, scale)
    out = []
    for t in range(n):
        out += st.push_u8(frames8[0, t], frames8[1, t]) if u8 else st.push(hr[0, t:t + 1], hr[1, t:t + 1], lr[0, t:t + 1], lr[1, t:t + 1])
    return out


def _reference(dev, nets, fusion, warp='NORMAL'):
    """PUSHES pushes through an exposure stitcher (captured graph, direct render): frames and final gains, once per configuration."""
    key = ('ref', fusion, warp)
    if key not in _runs:
        from stabstitch2_amd import online
        st = online.OnlineStitcher(nets, SH, SW, warp_mode=warp, fusion_mode=fusion, exposure=True)
        frames = _push_all(st, dev)
        assert len(frames) == PUSHES and st._direct() and st.graph is not None
        _runs[key] = (frames, st.exposure_gains, st.graph_nodes)
    return _runs[key]


def _same(a, b, what):
    assert len(a) == len(b), (what, len(a), len(b))
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and x.dtype == y.dtype and torch.equal(x, y), (what, i)


def test_exposure_none_is_the_stitcher_without_the_keyword(dev, hip_nets):
    from stabstitch2_amd import online
    a = online.OnlineStitcher(hip_nets, SH, SW)
    b = online.OnlineStitcher(hip_nets, SH, SW, exposure=None)
    _same(_push_all(a, dev, n=9), _push_all(b, dev, n=9), 'exposure=None')
    assert a.graph_nodes == b.graph_nodes and b.exposure_gains is None and b._exp_state is None
    on = _reference(dev, hip_nets, 'AVERAGE')
    print('\n[graph nodes, AVERAGE] exposure off %s, on %s' % (a.graph_nodes, on[2]))


@pytest.mark.parametrize('warp', ['NORMAL', 'FAST'])
@pytest.mark.parametrize('fusion', ['AVERAGE', 'LINEAR'])
def test_frames_equal_the_by_hand_chain(dev, hip_nets, fusion, warp, monkeypatch):
    """Every frame the exposure stitcher hands out (the first window's seven and five steady-state pushes through the captured
    graph and the direct render) equals, bit for bit: the stitcher's own splines and footprint of that frame -> ops.exposure_update
    on a state of the test's own -> the gain render.  The final state equals the test's."""
    from stabstitch2_amd import online, ops, pipeline
    _, hr, lr = _stream(dev)
    st = online.OnlineStitcher(hip_nets, SH, SW, warp_mode=warp, fusion_mode=fusion, exposure=True)
    solved = []
    inner = online.OnlineStitcher._render_solved

    def spy(self, imgs, src, T, *a, **kw):       # (on the class: a spy stored on the stitcher would tie it into a reference cycle)
        solved.append((src.clone(), T.clone()))
        return inner(self, imgs, src, T, *a, **kw)
    monkeypatch.setattr(online.OnlineStitcher, '_render_solved', spy)
    mine = ops.exposure_state(dev)
    emitted = 0
    for t in range(PUSHES):
        solved.clear()
        got = st.push(hr[0, t:t + 1], hr[1, t:t + 1], lr[0, t:t + 1], lr[1, t:t + 1])
        if not got:
            continue
        if len(got) == 7:                            # the first window: its seven frames, in order
            assert len(solved) == 7
            splines, frames_t = list(solved), range(7)
        else:                                        # the step left its splines and footprint for the push's render
            splines, frames_t = [st._deferred[:2]], [t]
        for (src, T), ft, frame in zip(splines, frames_t, got):
            imgs = [hr[0, ft:ft + 1], hr[1, ft:ft + 1]]
            fp = ops.render_footprints(src[None], T[None], SH, SW, st.hc, st.wc)
            gains = ops.exposure_update(imgs, fp, st.hc, st.wc, mine, st.exposure, warp)
            if fusion == 'AVERAGE':
                want = ops.render_average(imgs, src, T, st.hc, st.wc, warp, footprint=fp[0] if pipeline.SKIP_OUTSIDE else None, gains=gains)
            else:
                want = ops.render_linear_frames(imgs, src[None], T[None], [(st.hc, st.wc)], warp, gains=gains)[0]
            assert torch.equal(frame, want), (fusion, warp, t, ft, float((frame - want).abs().max()))
            emitted += 1
    assert emitted == PUSHES and st.graph is not None
    assert torch.equal(st._exp_state, mine) and int(mine.view(torch.int32)[9]) == 1
    if warp == 'NORMAL':
        _same(_reference(dev, hip_nets, fusion)[0], _push_all(online.OnlineStitcher(hip_nets, SH, SW, fusion_mode=fusion, exposure=ops.ExposureParams()), dev),
              'exposure=True is ExposureParams()')


@pytest.mark.parametrize('fusion', ['AVERAGE', 'LINEAR'])
def test_push_u8_is_push_and_canvas_to_u8(dev, hip_nets, fusion):
    from stabstitch2_amd import online, ops
    ref, gains, _ = _reference(dev, hip_nets, fusion)
    st = online.OnlineStitcher(hip_nets, SH, SW, fusion_mode=fusion, exposure=True)
    got = _push_all(st, dev, u8=True)
    assert st._u8_steady()
    _same(got, [ops.canvas_to_u8(f[None])[0] for f in ref], 'push_u8 ' + fusion)
    assert torch.equal(st.exposure_gains, gains)


@pytest.mark.parametrize('u8', [False, True], ids=['fp32', 'uint8'])
@pytest.mark.parametrize('fusion', ['AVERAGE', 'LINEAR'])
def test_push_many_across_the_window_fill(dev, hip_nets, fusion, u8):
    """k = 4 under deterministic=True: three calls (the window fills inside the second) return the frames of twelve pushes, and the
    gain sequences end on the same bits."""
    from stabstitch2_amd import online
    frames8, hr, lr = _stream(dev)
    key = ('det', fusion, u8)
    one = online.OnlineStitcher(hip_nets, SH, SW, fusion_mode=fusion, exposure=True, deterministic=True)
    ref = _push_all(one, dev, u8=u8)
    many = online.OnlineStitcher(hip_nets, SH, SW, fusion_mode=fusion, exposure=True, deterministic=True)
    got = []
    for t in range(0, PUSHES, 4):
        if u8:
            got += many.push_many_u8(frames8[0, t:t + 4], frames8[1, t:t + 4])
        else:
            got += many.push_many(hr[0, t:t + 4], hr[1, t:t + 4], lr[0, t:t + 4], lr[1, t:t + 4])
    _same(got, ref, 'push_many %s %s' % key[1:])
    assert torch.equal(many.exposure_gains, one.exposure_gains) and many.batch_captures >= 1


@pytest.mark.parametrize('fusion', ['AVERAGE', 'LINEAR'])
def test_eager_and_in_graph_render_equal_the_direct_render(dev, hip_nets, fusion, monkeypatch):
    from stabstitch2_amd import online
    ref, gains, nodes = _reference(dev, hip_nets, fusion)
    eager = online.OnlineStitcher(hip_nets, SH, SW, fusion_mode=fusion, exposure=True, use_graph=False)
    _same(_push_all(eager, dev), ref, 'use_graph=False ' + fusion)
    assert torch.equal(eager.exposure_gains, gains)
    monkeypatch.setattr(online, 'DIRECT_RENDER', False)              # SS_DIRECT_RENDER=0: the update and the render inside the graph
    inside = online.OnlineStitcher(hip_nets, SH, SW, fusion_mode=fusion, exposure=True)
    _same(_push_all(inside, dev), ref, 'SS_DIRECT_RENDER=0 ' + fusion)
    assert not inside._direct() and inside.graph is not None and torch.equal(inside.exposure_gains, gains)
    print('\n[graph nodes, %s, exposure on] direct %s, in-graph %s' % (fusion, nodes, inside.graph_nodes))


def test_viewport_and_refit_run_with_exposure(dev, hip_nets):
    """A viewport (grow='never' and 'refit'): every frame has the viewport's size, the gains move off 1, and push_u8 equals push +
    canvas_to_u8 there too."""
    from stabstitch2_amd import online, ops
    for grow in ('never', 'refit'):
        a = online.OnlineStitcher(hip_nets, SH, SW, viewport=(150, 250), grow=grow, exposure=True)
        b = online.OnlineStitcher(hip_nets, SH, SW, viewport=(150, 250), grow=grow, exposure=True)
        fa, fb = _push_all(a, dev, n=9), _push_all(b, dev, u8=True, n=9)
        assert len(fa) == 9 and all(tuple(f.shape) == (3, 150, 250) for f in fa)
        _same(fb, [ops.canvas_to_u8(f[None])[0] for f in fa], 'viewport ' + grow)
        assert float((a.exposure_gains - 1).abs().max()) > 0.01 and torch.equal(a.exposure_gains, b.exposure_gains)


def test_recapture_growth_keeps_the_gain_state(dev, hip_nets):
    """A canvas cropped on its right side under grow='recapture': it grows, the graph is captured again, and the gains go on from
    where they were -- after every push the state equals the by-hand update from the state before it (a reset would set it to the
    frame's targets instead)."""
    from stabstitch2_amd import online, ops
    _, hr, lr = _stream(dev)
    probe = online.OnlineStitcher(hip_nets, SH, SW)
    _push_all(probe, dev, n=7)
    bb = [float(x) for x in probe.bbox.cpu()]
    crop = [bb[0], bb[1] - 0.10 * (bb[1] - bb[0]), bb[2], bb[3]]
    st = online.OnlineStitcher(hip_nets, SH, SW, canvas=crop, grow='recapture', exposure=True)
    first = None
    for t in range(PUSHES):
        before = st._exp_state.clone()
        got = st.push(hr[0, t:t + 1], hr[1, t:t + 1], lr[0, t:t + 1], lr[1, t:t + 1])
        torch.cuda.synchronize()                     # (the growth check reads the watcher one push later: make it land)
        if got and first is None:
            first = (st.hc, st.wc)
        if len(got) == 1:
            assert tuple(got[0].shape) == (3, st.hc, st.wc)
            src, T = st._deferred[:2]
            fp = ops.render_footprints(src[None], T[None], SH, SW, st.hc, st.wc)
            ops.exposure_update([hr[0, t:t + 1], hr[1, t:t + 1]], fp, st.hc, st.wc, before, st.exposure, 'NORMAL')
            assert torch.equal(before, st._exp_state) and int(before.view(torch.int32)[9]) == 1, t
    assert st.canvas_epoch >= 1 and (st.hc, st.wc) != first, (st.canvas_epoch, first, st.hc, st.wc)


def test_gains_pull_a_darker_view_up(dev, hip_nets, monkeypatch):
    """View 2 darkened uniformly to 0.8: after the first window the ratio of the views' gains lies strictly between 1 and 1 / 0.8 on
    every channel (the prior keeps it short of the full correction); every frame's targets are the float64 statement's on the
    device's statistics of that frame within 2 fp32 ulp, and the gains are those targets walked through the fp32 smoothing, bit for
    bit."""
    from stabstitch2_amd import online, ops
    _, hr, lr = _stream(dev, (0.8, 0.8, 0.8))
    st = online.OnlineStitcher(hip_nets, SH, SW, exposure=True)
    seen = []
    inner = online.OnlineStitcher._exposure_gains
    monkeypatch.setattr(online.OnlineStitcher, '_exposure_gains',
                        lambda self, views, fp: seen.append(([v.clone() for v in views], fp.clone())) or inner(self, views, fp))
    frames = _push_all(st, dev, (0.8, 0.8, 0.8), n=7)
    assert len(frames) == 7 and len(seen) == 7
    g = st.exposure_gains.numpy()
    ratio = g[1] / g[0]
    assert ((ratio > 1.0) & (ratio < 1.25)).all() and (g[0] < 1).all() and (g[1] > 1).all(), g
    mine, s, started = ops.exposure_state(dev), np.ones((2, 3), F), False
    P = st.exposure
    for views, fp in seen:
        _, diag = ops.exposure_update(views, fp, st.hc, st.wc, mine, P, 'NORMAL', want_diag=True)
        stats = _diag_stats(diag[0].cpu().numpy(), 2)
        assert stats[(0, 1)][0] >= P.min_nodes
        want, kept = E.targets(stats, 2, P.sigma_n, P.sigma_g, P.min_nodes, P.gain_min, P.gain_max)
        got_t = diag[0, 27:33].cpu().numpy().reshape(2, 3)
        assert kept and _ulps(got_t, want) <= 2.0, (got_t, want)
        assert ((want[1] / want[0] > 1.0) & (want[1] / want[0] < 1.25)).all(), want
        s, started = E.smooth(s, started, got_t, kept, P.alpha)
    assert torch.equal(mine, st._exp_state) and np.array_equal(g, s), (g, s)


def test_refused_configurations_raise(dev, hip_nets):
    from stabstitch2_amd import online
    with pytest.raises(ValueError, match='meshes_only'):
        online.OnlineStitcher(hip_nets, SH, SW, meshes_only=True, exposure=True)
    st = online.OnlineStitcher(hip_nets, SH, SW, exposure=True)
    nv = torch.zeros((SH * 3 // 2, SW), dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match='push_nv12'):
        st.push_nv12(nv, nv)
    for make in (lambda: online.MultiOnlineStitcher(hip_nets, SH, SW, streams=2, exposure=True),
                 lambda: online.ThreeViewOnlineStitcher(hip_nets, SH, SW, exposure=True),
                 lambda: online.PipelinedOnlineStitcher(hip_nets, SH, SW, exposure=True),
                 lambda: online.PipelinedMultiOnlineStitcher(hip_nets, SH, SW, streams=2, exposure=True),
                 lambda: online.PipelinedThreeViewOnlineStitcher(hip_nets, SH, SW, exposure=True)):
        with pytest.raises(ValueError, match='exposure'):
            make()
