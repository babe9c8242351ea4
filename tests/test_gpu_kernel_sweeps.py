"""The non-convolution kernels (corr.hip, geom.hip, render.hip, metrics.hip, the FC and pooling kernels of conv.hip) against the
float64 statements of tests/ref64.py, swept over the shapes and edges where tiled kernels go wrong: channel-chunk tails, maps
smaller than a tile or a radius, one row / column past a tile, tile counts below and off the XCD deal, partial canvas tiles, the
three input layouts of the CCL, denominators at the homography's guard.  Every output element is compared; seeds are fixed;
shapes sit in `parametrize` lists so that a failure names its shape.

Gates (tests/test_ref64.py shows on the CPU that the fp32 oracle meets each fixed one with a factor 2 to spare):
  bit for bit   padding channels, refusals, max-pool, the fused-render identities
  derived       sums of fp32 products: |got - ref64| <= (K + 4) 2^-24 S (ref64.dot_bound; cost volume, FC, L2 norm)
  project's     TPS points / action of T 2e-5 normalised, tsmotion 2e-3 px, PSNR / SSIM 1e-6, stability 1e-4, distortion 1e-5,
                dense-warp coordinate 5.2e-5 of the half extent (the project's 2.5e-3 px on a 96-px frame), warp values
                close_grad(base 2e-3), homography values close_grad(base 1e-4)
  measured      CCL max(1e-4, 4 e_oracle) and the homography coordinate 4 e_oracle, e_oracle = the fp32 oracle's own error
                against ref64 on the very input, computed in the test
  ADDED to the two close_grad value gates, because both samplers are discontinuous in the coordinate and a per-element comparison
  against float64 cannot hold without them (LAB_NOTES.md S.2; the fp32 oracle needs them as much as the kernels do):
    sweep_inputs.sampler_slack   the float64 reference's own change when the coordinate moves by the family's coordinate tolerance: at a pixel
                          within that tolerance of the image border (where the sampled value jumps to 0) either side is right
    sweep_inputs.blend_residue   NORMAL only, and only at pixels with a clamped tap (outside the image): the derived bound of the four-product
                          fp32 blend, whose products cancel to 0 only in exact arithmetic.  Inside the image nothing is added.

    python -m pytest tests/test_gpu_kernel_sweeps.py -m gpu          (SS_VERBOSE=1 prints every observed maximum beside its gate)"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ref64 as R
import sweep_inputs as G
from sweep_inputs import host, within, refused, VERBOSE          # noqa: F401  (the sweeps' shared helpers)
from oracle import nets as N

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
T = torch.from_numpy


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    return torch.device('cuda:0')


def nhwc(x, dev):
    """[n,c,h,w] numpy -> device NHWC by a torch permute (the layout kernels of the library are not part of these tests)"""
    return T(np.ascontiguousarray(np.transpose(x, (0, 2, 3, 1)))).to(dev)


def nchw_of(t, c=None):
    t = t if c is None else t[..., :c]
    return t.permute(0, 3, 1, 2)


# ================================================================================================ cost volume
CV_SHAPES = [                      # (n, c, h, w)
    (1, 4, 2, 3),                  # map smaller than the radius, one chunk of 4 channels, 1 tile
    (1, 12, 4, 16),                # exactly one TY = 4 tile, 12 = 16 - 4
    (2, 20, 5, 17),                # one row and one column past a tile; 20 = 16 + 4
    (1, 36, 8, 16),                # exactly one TY = 8 tile; 36 = 2 x 16 + 4
    (3, 12, 9, 17),                # one row past TY = 8; 3 x 3 x 2 = 18 tiles at TY 4, 12 at TY 8: not multiples of 8
    (1, 20, 23, 31),               # 12 / 6 tiles
    (1, 128, 45, 60),              # the pipeline's shape, 48 / 24 tiles
    (5, 4, 9, 33),                 # 45 / 30 tiles
    (1, 36, 3, 40),                # h < TY, three tiles in x
]


def cv_check(out, ref, s, c, d, what):
    assert float(out[..., d:].abs().max()) == 0.0 if out.shape[-1] > d else True, what + ': padding channels not 0'
    within(nchw_of(out, d), ref, R.dot_bound(c, s), what)              # observed: worst |diff| / bound 0.34, max |diff| 2.7e-7


@pytest.mark.parametrize('ty', [0, 4, 8])
@pytest.mark.parametrize('r', [3, 5])
@pytest.mark.parametrize('shape', CV_SHAPES, ids=lambda s: 'n%d_c%d_%dx%d' % s)
def test_cost_volume_against_fp64(dev, shape, r, ty):
    """ss_cost_volume (both output pitches) and ss_cost_volume_bidir, every instantiation (R 3 / 5 x TY 4 / 8 and the rule)."""
    from stabstitch2_amd import _hip as H, ops
    n, c, h, w = shape
    a, b = G.cv_inputs(n, c, h, w)
    ref, s = R.cost_volume(a, b, r)
    refb, sb = R.cost_volume(b, a, r)
    ad, bd = nhwc(a, dev), nhwc(b, dev)
    d = (2 * r + 1) ** 2
    assert H.lib().ss_cost_volume_set_tile(ty) == 0
    try:
        out = ops.cost_volume(ad, bd, r)                                    # pitch d + 3
        wide = torch.full((n, h, w, d + 7), 7.0, device=dev)
        H.call('ss_cost_volume', H.dptr(ad), H.dptr(bd), H.dptr(wide), n, h, w, c, r, d + 7, H.stream())
        tight = torch.full((n, h, w, d), 7.0, device=dev)
        H.call('ss_cost_volume', H.dptr(ad), H.dptr(bd), H.dptr(tight), n, h, w, c, r, d, H.stream())
        both = ops.cost_volume_bidir(ad, bd, r)
    finally:
        H.lib().ss_cost_volume_set_tile(0)
    assert out.shape[-1] == d + 3
    cv_check(out, ref, s, c, d, 'cost volume %s r%d ty%d' % (shape, r, ty))
    cv_check(wide, ref, s, c, d, 'cost volume pitch d+7')
    cv_check(tight, ref, s, c, d, 'cost volume pitch d')
    cv_check(both[0], ref, s, c, d, 'bidir forward')
    cv_check(both[1], refb, sb, c, d, 'bidir backward')


@pytest.mark.parametrize('ty', [0, 4, 8])
@pytest.mark.parametrize('r', [3, 5])
@pytest.mark.parametrize('c,h,w', [(12, 5, 17), (20, 9, 16), (36, 2, 3)])
def test_cost_volume_shifted_and_chain_against_fp64(dev, c, h, w, r, ty):
    """ss_cost_volume_shifted (a 3-view chain's split / shift and a generic one) and ss_cost_volume_chain_frames (views 2 / 3,
    k 1 / 3) against the fp64 volumes of the GATHERED pairs -- not against ss_cost_volume."""
    from stabstitch2_amd import _hip as H, ops
    d = (2 * r + 1) ** 2
    assert H.lib().ss_cost_volume_set_tile(ty) == 0
    try:
        x1, x2 = G.cv_inputs(3, c, h, w, seed=1)                             # 3 views, two time steps
        out = ops.cost_volume(nhwc(x1, dev), nhwc(x2, dev), r, chain=2)      # volumes [v0, v1 | v1, v2]
        ref, s = R.cost_volume(np.concatenate((x1[:2], x1[1:])), np.concatenate((x2[:2], x2[1:])), r)
        cv_check(out, ref, s, c, d, 'shifted chain of 3 views')
        y1, y2 = G.cv_inputs(4, c, h, w, seed=2)
        out = ops.cost_volume(nhwc(y1, dev), nhwc(y2, dev), r, n=3, split=1, shift=1)     # images 0, 2, 3
        ref, s = R.cost_volume(y1[[0, 2, 3]], y2[[0, 2, 3]], r)
        cv_check(out, ref, s, c, d, 'shifted split 1 shift 1')
        for views in (2, 3):
            for k in (1, 3):
                x, _ = G.cv_inputs(views * (k + 1), c, h, w, seed=3 + views + k)
                xv = x.reshape(views, k + 1, c, h, w)
                out = ops.cost_volume_chain_frames(T(np.ascontiguousarray(xv.transpose(0, 1, 3, 4, 2))).to(dev), r)
                first = np.stack([xv[sv + hh, j] for hh in range(2) for sv in range(views - 1) for j in range(k)])
                second = np.stack([xv[sv + hh, j + 1] for hh in range(2) for sv in range(views - 1) for j in range(k)])
                ref, s = R.cost_volume(first, second, r)
                cv_check(out.reshape(-1, h, w, out.shape[-1]), ref, s, c, d, 'chain_frames views %d k %d' % (views, k))
    finally:
        H.lib().ss_cost_volume_set_tile(0)


# ================================================================================================ CCL, L2 norm
CCL_SHAPES = [(1, 1), (1, 7), (7, 1), (5, 7), (16, 16), (1, 257), (17, 15), (23, 30), (24, 32)]


def ccl_call(f1, f2, n, h, w, c, scale, want_nchw=True, want_nhwc4=True):
    """ss_ccl on device pointers that may alias one tensor (ops.ccl takes the shapes from its tensors; here f1 / f2 are views)"""
    from stabstitch2_amd import _hip as H
    dev = f1.device
    ws = torch.empty(int(H.lib().ss_ccl_workspace_floats(n, h, w, c)), device=dev, dtype=torch.float32)
    a = torch.full((n, 2, h, w), 7.0, device=dev) if want_nchw else None
    b = torch.full((n, h, w, 4), 7.0, device=dev) if want_nhwc4 else None
    H.call('ss_ccl', H.dptr(f1), H.dptr(f2), H.dptr(a, True), H.dptr(b, True), n, h, w, c, float(scale), H.dptr(ws), H.stream())
    return a, b


@pytest.mark.parametrize('c', [4, 32, 68, 256])
@pytest.mark.parametrize('h,w', CCL_SHAPES)
def test_ccl_against_fp64(dev, h, w, c):
    """ss_ccl on a chain of four G4-style maps (every neighbouring pair has a peaked soft-argmax): n = 3 and n = 1, the three
    L2-normalise routings (two tensors; the halves of one tensor; f2 = f1 advanced by one image of a 4-image tensor), scale 10 and
    1, each output alone and both.  Gate per input: max(1e-4, 4 e_oracle), e_oracle = oracle.nets.ccl's own error against ref64."""
    x = G.ccl_chain(4, c, h, w)
    xd = nhwc(x, dev)                                                   # [4,h,w,c]
    img = h * w * c
    for scale in (10.0, 1.0):
        ref = R.ccl(x[0:3], x[1:4], scale)
        e_oracle = float(np.abs(host(N.ccl(T(x[0:3]), T(x[1:4]), scale)) - ref).max())
        gate = max(1e-4, 4 * e_oracle)              # observed: e_oracle <= 1.4e-4; kernel max |diff| 1.04e-4, worst |diff| / gate 0.24
        tag = 'ccl %dx%dx%d scale %g (e_oracle %.1e)' % (h, w, c, scale, e_oracle)
        # f2 = f1 advanced by one image of a 4-image tensor (the overlapping chain)
        f, f4 = ccl_call(xd[0:3], xd[1:4], 3, h, w, c, scale)
        within(f, ref, gate, tag + ' chain n=3')
        assert torch.equal(f4[..., :2].permute(0, 3, 1, 2), f) and float(f4[..., 2:].abs().max()) == 0.0
        # the two halves of one tensor
        halves = torch.cat((xd[0:3], xd[1:4]), 0).contiguous()
        f, f4 = ccl_call(halves[0:3], halves[3:6], 3, h, w, c, scale)
        within(f, ref, gate, tag + ' halves n=3')
        assert torch.equal(f4[..., :2].permute(0, 3, 1, 2), f) and float(f4[..., 2:].abs().max()) == 0.0
        f, _ = ccl_call(xd[0:1], xd[1:2], 1, h, w, c, scale, want_nhwc4=False)             # n = 1: the neighbour IS the other half
        within(f, ref[0:1], gate, tag + ' halves n=1')
        # two tensors: f2 BELOW f1 in memory, so that neither aliasing rule applies
        buf = torch.empty(7 * img + 64, device=dev)
        f2 = buf[:3 * img].view(3, h, w, c).copy_(xd[1:4])
        f1 = buf[4 * img:7 * img].view(3, h, w, c).copy_(xd[0:3])
        f, f4 = ccl_call(f1, f2, 3, h, w, c, scale)
        within(f, ref, gate, tag + ' two tensors n=3')
        assert torch.equal(f4[..., :2].permute(0, 3, 1, 2), f) and float(f4[..., 2:].abs().max()) == 0.0
        fa, none = ccl_call(f1, f2, 3, h, w, c, scale, want_nhwc4=False)
        none2, fb = ccl_call(f1, f2, 3, h, w, c, scale, want_nchw=False)
        assert none is None and none2 is None and torch.equal(fa, f) and torch.equal(fb, f4)
        f, _ = ccl_call(f1[1:2], f2[1:2], 1, h, w, c, scale)
        within(f, ref[1:2], gate, tag + ' two tensors n=1')


def test_ccl_zero_vector_and_refusals(dev):
    """An all-zero feature vector (F.normalize's 1e-12 clamp) stays finite and equals fp64; 25 x 31 = 775 > 768 positions is
    refused with SS_ERR_UNSUPPORTED, c % 4 != 0 with SS_ERR_ARG."""
    from stabstitch2_amd import ops
    x = G.ccl_chain(2, 32, 5, 7)
    x[0, :, 2, 3] = 0.0
    x[1, :, 0, 0] = 0.0
    ref = R.ccl(x[0:1], x[1:2])
    e_oracle = float(np.abs(host(N.ccl(T(x[0:1]), T(x[1:2]))) - ref).max())
    f, f4 = ops.ccl(nhwc(x[0:1], dev), nhwc(x[1:2], dev), 10.0)
    within(f, ref, max(1e-4, 4 * e_oracle), 'ccl with zero feature vectors')
    refused(-3, ops.ccl, torch.zeros(1, 25, 31, 4, device=dev), torch.zeros(1, 25, 31, 4, device=dev))
    refused(-1, ops.ccl, torch.zeros(1, 5, 6, 6, device=dev), torch.zeros(1, 5, 6, 6, device=dev))


@pytest.mark.parametrize('c', [1, 4, 63, 64, 65, 256])
@pytest.mark.parametrize('npix', [1, 13, 64, 770])
def test_l2norm_against_fp64(dev, npix, c):
    """ss_l2norm_nhwc alone (lane loop i += 64: c below, at and above one wave; pixel counts that are not multiples of the 4
    pixels of a workgroup), relative bound of a c-term sum of squares, one all-zero pixel."""
    from stabstitch2_amd import ops
    v = np.random.RandomState(100 * c + npix).normal(0, 1, (npix, c)).astype(np.float32)
    v[npix // 2] = 0.0
    ref = R.l2norm(v, 1)
    got = ops.l2norm(T(v).to(dev))
    within(got, ref, R.dot_bound(c, np.abs(ref)), 'l2norm %d x %d' % (npix, c))           # observed: worst |diff| / bound 0.27
    assert float(got[npix // 2].abs().max()) == 0.0


# ================================================================================================ homography sampler
@functools.lru_cache(maxsize=None)
def homo_case(name, oh, ow):
    th = G.homo_thetas(oh)[name][None]
    e, _, taps_in = G.homo_oracle_error(G.homo_input(1, 8), th, oh, ow)
    return th, e, taps_in


def homo_check(got, U, th, e, taps_in, oh, ow, what):
    ref, bound = G.homo_gate(U, th, oh, ow, e)
    within(got, ref, bound, what + ' values')
    if U.shape[1] >= 2 and taps_in.any():                  # the last two channels are the ramps: the sampling coordinate
        g, r = host(got)[:, -2:][:, :, taps_in[0]], ref[:, -2:][:, :, taps_in[0]]
        within(g / G.RAMP, r / G.RAMP, 4 * e, what + ' coords (px; gate 4 x e_oracle %.1e)' % e)     # observed: <= 1.1e-5 px, worst |diff| / gate 0.30


@pytest.mark.parametrize('name', ['identity', 'g2_mild', 'g2_far', 'zero_row', 'under', 'over'])
@pytest.mark.parametrize('oh,ow', [(2, 2), (23, 31), (45, 60), (90, 121)])
def test_homography_against_fp64(dev, oh, ow, name):
    """ss_homo_warp_nhwc (c 4 / 8 / 20), ss_homo_warp_nchw (c 1 / 3 / 5) and ss_homo_warp_pair_nhwc (in2 right behind in1, and
    overlapping it) on a 45 x 60 map of texture + ramp channels.  Coordinates (ramp channels, all taps inside): 4 x the fp32
    oracle's own error for that theta and size; values: close_grad(that tolerance, base 1e-4), every element."""
    from stabstitch2_amd import _hip as H, ops
    th, e, taps_in = homo_case(name, oh, ow)
    thd = T(np.repeat(th, 2, 0)).to(dev)
    for c in (4, 8, 20):
        U = G.homo_input(2, c)
        got = ops.homo_warp_nhwc(nhwc(U, dev), thd, oh, ow)
        homo_check(nchw_of(got), U, th, e, taps_in, oh, ow, 'homo nhwc c%d %s %dx%d' % (c, name, oh, ow))
    for c in (1, 3, 5):
        U = G.homo_input(2, c)
        got = ops.homo_warp_nchw(T(U).to(dev), thd, oh, ow)
        homo_check(got, U, th, e, taps_in, oh, ow, 'homo nchw c%d %s %dx%d' % (c, name, oh, ow))
    U = G.homo_input(4, 8)
    Ud = nhwc(U, dev)
    th4 = T(np.repeat(th, 4, 0)).to(dev)
    for first, second, tag in ((slice(0, 2), slice(2, 4), 'adjacent'), (slice(0, 2), slice(1, 3), 'overlapping')):
        out = torch.full((4, oh, ow, 8), 7.0, device=dev)
        H.call('ss_homo_warp_pair_nhwc', H.dptr(Ud[first]), H.dptr(Ud[second]), H.dptr(th4), H.dptr(out), 2, 45, 60, 8, oh, ow, H.stream())
        homo_check(nchw_of(out), np.concatenate((U[first], U[second])), th, e, taps_in, oh, ow, 'homo pair ' + tag)


def test_homography_mixed_thetas_in_one_batch(dev):
    """every image of a batch uses ITS theta: the six thetas as one batch of six"""
    from stabstitch2_amd import ops
    oh, ow = 23, 31
    names = ['identity', 'g2_mild', 'g2_far', 'zero_row', 'under', 'over']
    U = G.homo_input(6, 8)
    got = nchw_of(ops.homo_warp_nhwc(nhwc(U, dev), T(np.concatenate([homo_case(k, oh, ow)[0] for k in names])).to(dev), oh, ow))
    for i, k in enumerate(names):
        th, e, taps_in = homo_case(k, oh, ow)
        homo_check(got[i:i + 1], U[i:i + 1], th, e, taps_in, oh, ow, 'homo batch item ' + k)


# ================================================================================================ thin-plate spline
TPS_GATE = 2e-5            # normalised; test_tps_points_and_tsmotion's interpolation gate (oracle vs ref64 <= 1e-5: test_ref64)
                           # observed: action of T <= 2.6e-6, points <= 1.0e-5 (n = 300, q = 1000)


@pytest.mark.parametrize('h,w', [(360, 480), (720, 1280)])
@pytest.mark.parametrize('n', [1, 7, 300])
def test_tps_solve_by_its_action(dev, n, h, w):
    """ss_tps_solve, ss_tps_solve_shared_target and ss_tps_inverse: T is judged by what it does -- the spline with the kernel's T and
    with the fp64 T, both evaluated in fp64 on a 33 x 33 grid over [-1, 1]^2."""
    from stabstitch2_amd import _hip as H, ops
    rigid, warped = G.tps_meshes(n, h, w)
    for src, tgt, tag in ((rigid, warped, 'rigid -> warped'), (warped, rigid, 'warped -> rigid')):
        want = R.tps_action(R.tps_solve(src, tgt), src)
        got = ops.tps_solve(T(src).to(dev), T(tgt).to(dev))
        within(R.tps_action(host(got), src), want, TPS_GATE, 'tps_solve action n=%d %dx%d %s' % (n, h, w, tag))
    got = ops.tps_solve_shared(T(warped).to(dev), T(rigid[0]).to(dev))
    within(R.tps_action(host(got), warped), R.tps_action(R.tps_solve(warped, rigid), warped), TPS_GATE, 'tps_solve_shared_target action')
    winv = torch.empty((66, 66), device=dev, dtype=torch.float64)
    w0 = T(warped[0]).to(dev)
    H.call('ss_tps_inverse', H.dptr(w0), H.dptr(winv, dtype=torch.float64), H.stream())
    Tk = (host(winv) @ R.tps_rhs(rigid[0:1])[0]).T[None]
    within(R.tps_action(Tk, warped[0:1]), R.tps_action(R.tps_solve(warped[0:1], rigid[0:1]), warped[0:1]), TPS_GATE, 'tps_inverse action')


@pytest.mark.parametrize('n,q', [(1, 1), (7, 63), (1, 127), (7, 128), (1, 129), (7, 1000), (300, 1000), (300, 1)])
def test_tps_points_against_fp64(dev, n, q):
    """ss_tps_points at q below, at and above its 128-thread workgroup, queries over +-1.1, both directions of the G5 meshes at
    360 x 480 and 720 x 1280, through the kernel's own T (as torch_tps_transform_point.transformer runs it)."""
    from stabstitch2_amd import ops
    for (h, w) in ((360, 480), (720, 1280)):
        rigid, warped = G.tps_meshes(n, h, w)
        pts = G.tps_queries(n, q)
        for src, tgt in ((rigid, warped), (warped, rigid)):
            sd = T(src).to(dev)
            got = ops.tps_points(T(pts).to(dev), sd, ops.tps_solve(sd, T(tgt).to(dev)))
            within(got, R.tps_points(pts, src, tgt), TPS_GATE, 'tps_points n=%d q=%d %dx%d' % (n, q, h, w))


@pytest.mark.parametrize('lag', [1, 2, 3])
@pytest.mark.parametrize('n', [1, 7, 300])
def test_tsmotion_against_fp64(dev, n, lag, golden):
    """ss_tsmotion_lag (cached rigid inverse and per-frame elimination) and ss_tsmotion: 2e-3 px (test_tps_points_and_tsmotion);
    smesh = rigid + smotion is one fp32 addition."""
    from stabstitch2_amd import _hip as H, ops
    sm, tm = G.tsm_inputs(n)
    if n == 7:
        g8 = golden('g8_nets')
        sm, tm = g8['motion1'][:7], g8['tmotion1'][:7]
    smesh, ts = R.tsmotion(sm, tm, lag=lag)
    for cache in (True, False):
        old = ops.RIGID_INVERSE_CACHE
        ops.RIGID_INVERSE_CACHE = cache
        try:
            gs, gt = ops.tsmotion(T(sm).to(dev), T(tm).to(dev), lag=lag)
        finally:
            ops.RIGID_INVERSE_CACHE = old
        within(gt, ts, 2e-3, 'tsmotion n=%d lag %d cache %s (px)' % (n, lag, cache))          # observed <= 4.8e-4 px
        within(gs, smesh, R.dot_bound(1, np.abs(smesh), extra=1), 'smesh')
        assert float(gt[:lag].abs().max()) == 0.0
    if lag == 1:
        ws = torch.empty(int(H.lib().ss_tsmotion_workspace_floats(n)), device=dev)
        a, b = torch.empty(n, 7, 9, 2, device=dev), torch.empty(n, 7, 9, 2, device=dev)
        smd, tmd = T(sm).to(dev), T(tm).to(dev)
        H.call('ss_tsmotion', H.dptr(smd), H.dptr(tmd), H.dptr(a), H.dptr(b), n, 360.0, 480.0, None, H.dptr(ws), H.stream())
        within(b, ts, 2e-3, 'ss_tsmotion n=%d (px)' % n)


# ================================================================================================ dense TPS warp
COORD_GATE = G.WARP_COORD_GATE   # 5.2e-5 of the half extent: the project's 2.5e-3 px on a 96-px frame (test_tps_dense_warp_and_fusion), held as a
                           # normalised number at every size (oracle vs ref64 <= 1.3e-5 on these inputs: test_ref64)
                           # observed: worst |diff| / gate 0.10 (1.9e-3 px of 3.3e-2 at 720 x 1280); values: worst |diff| / bound 0.11
WARP_CASES = [             # (batch, h, w, hc, wc)          hc % 8, wc % 64
    (1, 2, 2, 8, 64),              # 0, 0    one full tile, the smallest frame the entry points take
    (3, 72, 96, 80, 120),          # 0, 56   the fixture's sizes, batch 3
    (1, 251, 377, 300, 520),       # 4, 8
    (1, 72, 96, 81, 129),          # 1, 1    a tile row with ya only; a tile column of one pixel
    (1, 72, 96, 85, 191),          # 5, 63   yb = ya + 4 valid for wave 0 only
    (1, 72, 96, 84, 128),          # 4, 0    yb past the canvas for every wave of the last tile row
    (1, 72, 96, 87, 65),           # 7, 1
    (1, 720, 1280, 780, 1900),     # 4, 44   the benchmark's frame
]


@functools.lru_cache(maxsize=None)
def warp_ref(case):
    b, h, w, hc, wc = case
    U, src, tgt = G.warp_case(b, h, w, hc, wc)
    xn, yn = R.tps_dense_coords(src, R.tps_solve(src, tgt), hc, wc)
    return U, src, tgt, xn, yn


def warp_check(got, U, xn, yn, mode, what, mask=False):
    """got [b,c(+1),hc,wc] against the fp64 sampler at the fp64 coordinates: the ramp planes (channels 3, 4 of U) give the sampling
    coordinate in pixels wherever all four taps are inside the frame, gate COORD_GATE of the half extent; every value of every plane
    (the ones-mask included) inside close_grad(base 2e-3, tol_px = that gate) incl. the sampler's border discontinuity.  NORMAL adds
    the derived bound of its four-product fp32 blend: outside the frame the clamped sampler's products cancel to 0 only in exact
    arithmetic (R.bilinear_clamped), and at 1280 px they are 1e4 .. 1e8 large."""
    h, w = U.shape[2:]
    if mask:
        U = np.concatenate((U, np.ones((U.shape[0], 1, h, w), np.float32)), 1)
    ref, bound, x, y, inside = G.warp_gate(U, xn, yn, mode)
    within(got, ref, bound, what + ' values')
    if U.shape[1] >= 5 and inside.any():
        g = host(got)
        ex, ey = ((w, h) if mode == 'NORMAL' else (w - 1, h - 1))
        within(g[:, 3][inside], x[inside], COORD_GATE * ex / 2, what + ' x coordinate (px)')
        within(g[:, 4][inside], y[inside], COORD_GATE * ey / 2, what + ' y coordinate (px)')


@pytest.mark.parametrize('mode', ['NORMAL', 'FAST'])
@pytest.mark.parametrize('case', WARP_CASES, ids=lambda c: 'b%d_%dx%d_to_%dx%d' % c)
def test_tps_dense_warp_against_fp64(dev, case, mode):
    """ss_tps_warp_nchw and ss_tps_warp_mask_nchw through the kernel's own ss_tps_solve (as torch_tps_transform.transformer runs
    them): ramp planes + texture, full and partial 64 x 8 canvas tiles, every pixel."""
    from stabstitch2_amd import ops
    b, h, w, hc, wc = case
    U, src, tgt, xn, yn = warp_ref(case)
    Ud, sd = T(U).to(dev), T(src).to(dev)
    Tk = ops.tps_solve(sd, T(tgt).to(dev))
    what = 'tps_warp %s %dx%d -> %dx%d' % (mode, h, w, hc, wc)
    warp_check(ops.tps_warp(Ud, sd, Tk, hc, wc, mode), U, xn, yn, mode, what)
    if hc * wc < 400000:
        warp_check(ops.tps_warp(Ud, sd, Tk, hc, wc, mode, with_mask=True), U, xn, yn, mode, what + ' +mask', mask=True)
    else:
        wm = ops.tps_warp(Ud[:, :3].contiguous(), sd, Tk, hc, wc, mode, with_mask=True)
        warp_check(wm[:, 3:4], U[:, :0], xn, yn, mode, what + ' mask plane', mask=True)


@pytest.mark.parametrize('mode', ['NORMAL', 'FAST'])
@pytest.mark.parametrize('case', [(3, 72, 96, 85, 191), (2, 72, 96, 81, 129), (3, 72, 96, 80, 120)], ids=lambda c: 'v%d_%dx%d_to_%dx%d' % c)
def test_tps_warp_views_against_fp64(dev, case, mode):
    """ss_tps_warp_views (per-view image pointers, 3 colour planes + the ones-mask) against fp64, 2 and 3 views"""
    from stabstitch2_amd import ops
    v, h, w, hc, wc = case
    U, src, tgt, xn, yn = warp_ref(case)
    sd = T(src).to(dev)
    Tk = ops.tps_solve(sd, T(tgt).to(dev))
    got = ops.tps_warp_views([T(np.ascontiguousarray(U[i, :3])).to(dev) for i in range(v)], sd, Tk, hc, wc, mode)
    warp_check(got, U[:, :3], xn, yn, mode, 'tps_warp_views %s %d views -> %dx%d' % (mode, v, hc, wc), mask=True)


# ================================================================================================ fused render identities
def average_formula(w):
    f = w[0] * (w[0] / (w[0] + w[1] + 1e-6)) + w[1] * (w[1] / (w[0] + w[1] + 1e-6))
    for k in range(2, w.shape[0]):
        f = f * (f / (f + w[k] + 1e-6)) + w[k] * (w[k] / (f + w[k] + 1e-6))
    return f


@pytest.mark.parametrize('mode', ['NORMAL', 'FAST'])
@pytest.mark.parametrize('views', [2, 3])
@pytest.mark.parametrize('h,w,hc,wc', [(72, 96, 80, 120), (72, 96, 81, 129), (72, 96, 85, 191), (72, 96, 84, 128), (72, 96, 87, 65),
                                       (251, 377, 300, 520)])
def test_fused_render_equals_formula_on_per_view_warps(dev, h, w, hc, wc, views, mode):
    """ss_render_average, _clip, _u8 and _clip_u8 == the AVERAGE formula applied to ss_tps_warp_nchw's per-view warps, bit for bit
    (test_full_size_properties_720p's identity, here for FAST, three views, partial canvas tiles and the uint8 forms).  The
    per-view warps are held to fp64 by test_tps_dense_warp_against_fp64; the singular a a / (a + b + 1e-6) is never compared."""
    from stabstitch2_amd import ops
    U, src, tgt = G.warp_case(2 * views, h, w, hc, wc, seed=11)
    u8 = np.clip(np.rint(U[:, :3]), 0, 255).astype(np.uint8)                       # [2 frames x views, 3, h, w]
    sd = T(src).to(dev)
    Tk = ops.tps_solve(sd, T(tgt).to(dev))
    frames_u8 = [T(np.ascontiguousarray(u8[i].transpose(1, 2, 0))).to(dev) for i in range(2 * views)]     # [h,w,3] each
    planes = [ops.ingest_u8(f[None])[0][0] for f in frames_u8]                     # [3,h,w] fp32, exact
    want = []
    for f in range(2):
        sl = slice(f * views, (f + 1) * views)
        wv = ops.tps_warp(torch.stack(planes[sl]), sd[sl], Tk[sl], hc, wc, mode)
        want.append(average_formula(wv))
        got = ops.render_average(planes[sl], sd[sl], Tk[sl], hc, wc, mode)
        assert torch.equal(got, want[f]), ('render_average', f, float((got - want[f]).abs().max()))
        got8 = ops.render_average_u8(frames_u8[sl], sd[sl], Tk[sl], hc, wc, mode)
        assert torch.equal(got8, ops.canvas_to_u8(want[f][None])[0]), ('render_average_u8', f)
    clip = [torch.stack([planes[f * views + v] for f in range(2)]) for v in range(views)]           # per view [2,3,h,w]
    src_c, T_c = sd.view(2, views, 63, 2), Tk.view(2, views, 2, 66)
    assert torch.equal(ops.render_average_clip(clip, src_c, T_c, hc, wc, mode), torch.stack(want))
    clip8 = [torch.stack([frames_u8[f * views + v] for f in range(2)]) for v in range(views)]
    assert torch.equal(ops.render_average_clip_u8(clip8, src_c, T_c, hc, wc, mode), ops.canvas_to_u8(torch.stack(want)))


# ================================================================================================ metrics
@pytest.mark.parametrize('mask', ['ones', 'binary', 'frac'])
@pytest.mark.parametrize('frames', [1, 5])
@pytest.mark.parametrize('h,w', [(7, 7), (36, 48), (9, 65), (65, 9), (130, 131), (360, 480)])
def test_psnr_ssim_against_fp64(dev, h, w, frames, mask):
    """ss_alignment_psnr_ssim: tile seams in x (w > 64) and y, one-pixel interiors, binary and fractional masks; 1e-6 on both
    (test_psnr_ssim_vs_skimage)."""
    from stabstitch2_amd import metrics
    w1, w2 = G.metric_planes(frames, h, w, mask)
    p, s = metrics.alignment_psnr_ssim(T(w1).to(dev), T(w2).to(dev))
    ref = np.array([R.psnr_ssim(w1[f], w2[f]) for f in range(frames)])
    within(p, ref[:, 0], 1e-6, 'psnr %dx%d x%d %s (dB)' % (h, w, frames, mask))            # observed <= 1.1e-14 dB, SSIM <= 1.7e-15
    within(s, ref[:, 1], 1e-6, 'ssim %dx%d x%d %s' % (h, w, frames, mask))


def test_metric_scores_against_fp64_and_refusals(dev):
    """ss_stability_score (t 7 / 8 / 50; gate 1e-4) and ss_distortion_score (t 1 / 64 / 65 / 200: one thread per frame in
    workgroups of 64; gate 1e-5), the gates of test_pipeline_vs_reference; h or w < 7 and t < 7 refused with SS_ERR_ARG."""
    from stabstitch2_amd import metrics
    for t in (7, 8, 50):
        p = G.metric_paths(t)
        within(metrics.stability_score(T(p).to(dev).view(1, t, 7, 9, 2)), R.stability_score(p), 1e-4, 'stability t=%d' % t)         # observed 1.0e-7
    for t in (1, 64, 65, 200):
        m = G.metric_meshes(t)
        within(metrics.distortion_score(T(m).to(dev).view(1, t, 7, 9, 2)), R.distortion_score(m), 1e-5, 'distortion t=%d' % t)     # observed 1.4e-7
    for (h, w) in ((6, 48), (48, 6)):
        z = torch.zeros(1, 4, h, w, device=dev)
        refused(-1, metrics.alignment_psnr_ssim, z, z)
    refused(-1, metrics.stability_score, torch.zeros(1, 6, 7, 9, 2, device=dev))


# ================================================================================================ FC, pooling
@pytest.mark.parametrize('k', [2, 4, 6, 132, 1536])
@pytest.mark.parametrize('m', [1, 2, 19, 64, 65])
def test_linear_against_fp64(dev, m, k):
    """ss_linear (any k: the scalar path for k % 4 != 0) and ss_linear_grouped (k % 4 == 0, 3 groups, separate destinations) under
    the derived bound of a k-term fp32 dot product (+ bias, + ReLU's exact max)."""
    from stabstitch2_amd import ops
    rs = np.random.RandomState(m * 1000 + k)
    nout, groups = 37, 3
    x = rs.normal(0, 1, (groups, m, k)).astype(np.float32)
    wt = (rs.normal(0, 1, (groups, nout, k)) / np.sqrt(k)).astype(np.float32)
    b = rs.normal(0, 1, (groups, nout)).astype(np.float32)
    x64, w64 = x.astype(np.float64), wt.astype(np.float64)
    pre = np.einsum('gmk,gnk->gmn', x64, w64) + b[:, None, :]
    s = np.einsum('gmk,gnk->gmn', np.abs(x64), np.abs(w64)) + np.abs(b[:, None, :])
    for relu in (False, True):
        ref = np.maximum(pre, 0) if relu else pre
        got = ops.linear(T(x[0]).to(dev), T(wt[0]).to(dev), T(b[0]).to(dev), relu=relu)
        within(got, ref[0], R.dot_bound(k + 1, s[0], extra=1), 'linear m=%d k=%d relu %d' % (m, k, relu))      # observed: worst |diff| / bound 0.50 (k = 2)
        if k % 4 == 0:
            gg = ops.linear_grouped(T(x).to(dev), T(wt).to(dev), T(b).to(dev), relu=relu)
            within(gg, ref, R.dot_bound(k + 1, s, extra=1), 'linear_grouped m=%d k=%d' % (m, k))
            assert torch.equal(gg[0], got)
    nob = ops.linear(T(x[0]).to(dev), T(wt[0]).to(dev), None)
    within(nob, pre[0] - b[0][None], R.dot_bound(k, s[0], extra=1), 'linear without bias')


@pytest.mark.parametrize('n,h,w,c,k,s,p', [(2, 45, 61, 128, 3, 2, 1), (1, 7, 9, 8, 2, 2, 0), (3, 5, 5, 16, 3, 1, 1), (1, 1, 1, 8, 3, 2, 1)])
def test_maxpool_split_bit_exact(dev, n, h, w, c, k, s, p):
    """ss_maxpool_nhwc_split == F.max_pool2d on each half of the channels, bit for bit"""
    from stabstitch2_amd import ops
    x = np.random.RandomState(h * w + c).normal(0, 1, (n, c, h, w)).astype(np.float32)
    ref = F.max_pool2d(T(x), k, s, p)
    ho, wo = ref.shape[2:]
    o0 = torch.full((n, ho, wo, c // 2), 7.0, device=dev)
    o1 = torch.full((n, ho, wo, c // 2), 7.0, device=dev)
    ops.maxpool_split(nhwc(x, dev), k, s, p, o0, o1)
    assert torch.equal(nchw_of(o0).cpu(), ref[:, :c // 2]) and torch.equal(nchw_of(o1).cpu(), ref[:, c // 2:])
