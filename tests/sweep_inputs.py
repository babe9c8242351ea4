"""Seeded inputs and gate constructions of the kernel sweeps, shared by tests/test_ref64.py (CPU: the fp32 oracle against
tests/ref64.py on these very inputs, under these very gates) and tests/test_gpu_kernel_sweeps.py / tests/test_gpu_conv_sweeps.py /
tests/test_gpu_rest_sweeps.py (the kernels), with the comparison helpers the three sweep files share (within, refused, host).
The float64 statements themselves are in tests/ref64.py and do not depend on anything here.  The middle holds the convolution
sweep: its cases, the dispatch rules of the convolution engine restated (which kernel a shape takes), an fp32 emulation of both
Winograd forms, and the reach table from kernel instantiation to the cases claimed to launch it; then the inputs of the LINEAR and
mesh-geometry sweeps and library_reach, the coverage table of every kernel of the library."""
import os

import numpy as np

from ref64 import F32, WATCH_SLACK, f64, dot_bound, linspace, bilinear_clamped, grid_sample_zeros, homography_coords

VERBOSE = bool(os.environ.get('SS_VERBOSE'))


# ------------------------------------------------------------------------------------------------ comparison helpers
def host(t):
    return t.detach().cpu().numpy().astype(np.float64) if hasattr(t, 'detach') else np.asarray(t, dtype=np.float64)


def within(got, ref, bound, what):
    """every element: |got - ref| <= bound (array or scalar); prints the worst |diff| / bound under SS_VERBOSE"""
    got, ref = host(got), host(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), what + ' has non-finite values'
    d = np.abs(got - ref)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), d.shape)
    excess = d - bound
    if VERBOSE:
        ratio = float((d / np.maximum(bound, 1e-300))[bound > 0].max()) if (bound > 0).any() else 0.0
        print('  [sweep] %-58s max|diff| %.3e  worst |diff|/bound %.3f' % (what, float(d.max()) if d.size else 0.0, ratio))
    i = np.unravel_index(int(np.argmax(excess)), excess.shape) if d.size else ()
    assert (excess <= 0).all(), '%s: |diff| %.3e > bound %.3e at %s (%d of %d elements out)' % (
        what, d[i], bound[i], i, int((excess > 0).sum()), d.size)


def refused(code, fn, *args):
    import pytest
    from stabstitch2_amd import _hip as H
    with pytest.raises(H.HipError) as ei:
        fn(*args)
    assert ei.value.code == code, (ei.value.code, code)


def astype_u8(x):
    """`.astype(np.uint8)` as include/stabstitch_hip.h documents it: truncation toward zero through int32, the low byte kept; a
    value int32 cannot hold (|v| >= 2^31, +-inf, NaN) gives 0."""
    x = np.asarray(x, F32)
    ok = np.abs(x) < 2147483648.0                               # False for NaN
    t = np.trunc(np.where(ok, x, 0)).astype(np.int64)
    return np.where(ok, t & 0xFF, 0).astype(np.uint8)


RAMP = 1.0 / 64.0           # ramp channels of the homography inputs hold index * RAMP (exact in fp32, same magnitude as the texture)


# ------------------------------------------------------------------------------------------------ gates
def grad4(b):
    """close_grad's gradient term: the largest jump to a 4-neighbour in the reference image b [..., H, W]."""
    b = f64(b)
    bp = np.pad(b, [(0, 0)] * (b.ndim - 2) + [(1, 1), (1, 1)], mode='edge')
    g = np.zeros_like(b)
    for dy, dx in ((0, 1), (2, 1), (1, 0), (1, 2)):
        g = np.maximum(g, np.abs(bp[..., dy:dy + b.shape[-2], dx:dx + b.shape[-1]] - b))
    return g


def sampler_slack(sampler, img, xn, yn, tol_x, tol_y):
    """How far the reference value itself moves when the sampling coordinate moves by (+-tol_x, +-tol_y) (normalised units).
    Both samplers are DISCONTINUOUS in the coordinate at the image border (the clamped sampler's weights collapse to 0 just
    outside, grid_sample drops a tap): at a pixel whose exact coordinate lies within the coordinate tolerance of a border either
    side is the right answer for a coordinate that is right to that tolerance, and close_grad's neighbour-jump term does not see
    it.  Elsewhere this is ~ tol * the true derivative, no larger than close_grad's own term."""
    ref = sampler(img, xn, yn)
    slack = np.zeros_like(ref)
    for sx in (-1.0, 1.0):
        for sy in (-1.0, 1.0):
            slack = np.maximum(slack, np.abs(sampler(img, xn + sx * tol_x, yn + sy * tol_y) - ref))
    return ref, slack


def blend_residue(img, xn, yn):
    """The rounding residue the CLAMPED sampler may return outside the image, 0 inside.  Where a tap index is clamped, the two
    taps of that axis coincide and carry opposite weights: the four products cancel in exact arithmetic, but each is of the size
    (distance to the image) x value and an fp32 sum (A + B) - A - B of them keeps the rounding of its three additions,
    gamma_4 sum |w v| at most (dot_bound with no further roundings).  Only those pixels get it: inside the image the same bound
    would be 2e-7 of the value and the gates' base terms cover it."""
    img = f64(img)
    h, w = img.shape[2:]
    x = (f64(xn) + 1.0) * w / 2.0
    y = (f64(yn) + 1.0) * h / 2.0
    clamped = (np.floor(x) < 0) | (np.floor(x) + 1 > w - 1) | (np.floor(y) < 0) | (np.floor(y) + 1 > h - 1)
    s = bilinear_clamped(img, xn, yn, absum=True)[1]
    return np.where(clamped[:, None], dot_bound(4, s, extra=0), 0.0)


WARP_COORD_GATE = 5.2e-5   # of the half extent: the project's 2.5e-3 px on a 96-px frame (test_tps_dense_warp_and_fusion), held as a
                           # normalised number at every frame size


def warp_gate(U, xn, yn, mode, spare=1.0):
    """The value gate of the dense-warp family -> (ref, bound, x, y, inside): close_grad(base 2e-3, tol_px = WARP_COORD_GATE in
    pixels of the frame) against the fp64 sampler at the fp64 coordinates (xn, yn), plus the two terms the samplers' own
    discontinuities need -- sampler_slack under the same coordinate tolerance and, NORMAL only, blend_residue outside the frame.
    x, y: the coordinates in pixels; inside: where all four taps lie inside the frame (there a ramp plane returns x or y).
    spare > 1 divides every term -- the base, the coordinate tolerance behind the gradient and slack terms, the residue -- by it: the
    gate the fp32 oracle has to meet with room (at a border discontinuity the bound is the jump itself whatever the tolerance, so
    it is the tolerance that is divided, not the bound)."""
    h, w = U.shape[2:]
    sampler = bilinear_clamped if mode == 'NORMAL' else grid_sample_zeros
    ex, ey = ((w, h) if mode == 'NORMAL' else (w - 1, h - 1))
    tol = WARP_COORD_GATE / spare
    ref, slack = sampler_slack(sampler, U, xn, yn, tol, tol)
    bound = 2e-3 / spare + np.maximum(tol * max(ex, ey) / 2 * grad4(ref), slack)
    if mode == 'NORMAL':
        bound = bound + blend_residue(U, xn, yn) / spare
    x, y = (xn + 1) * ex / 2, (yn + 1) * ey / 2
    inside = (x > 0.01) & (x < w - 1.01) & (y > 0.01) & (y < h - 1.01)
    return ref, bound, x, y, inside


def homo_oracle_error(U, th, oh, ow):
    """-> (e_oracle in pixels of the input map, the oracle's warp of U[:1], the mask of pixels with all four taps inside): the fp32
    oracle's own coordinate error for theta `th` [1,3,3] -- its normalised coordinates against homography_coords where they are
    in range, and its sampled ramp channels (the last two of U) against the fp64 ones where all four taps are inside the image.
    The homography family's coordinate tolerance is 4 x this."""
    import torch
    from oracle import samplers as S
    h, w = U.shape[2:]
    xn, yn, _ = homography_coords(th, oh, ow)
    ox, oy = S.homography_coords(torch.from_numpy(th), oh, ow)
    ox, oy = f64(ox).reshape(xn.shape), f64(oy).reshape(yn.shape)
    inr = (np.abs(xn) <= 1.0) & (np.abs(yn) <= 1.0)
    e = max(float((np.abs(ox - xn) * inr).max()) * w / 2, float((np.abs(oy - yn) * inr).max()) * h / 2)
    x, y = (xn + 1) * w / 2, (yn + 1) * h / 2
    taps_in = (x > 0.01) & (x < w - 1.01) & (y > 0.01) & (y < h - 1.01)
    o = f64(S.homography_warp(torch.from_numpy(U[:1]), torch.from_numpy(th), (oh, ow)))
    if taps_in.any():
        ref1 = bilinear_clamped(U[:1, -2:], xn, yn)
        e = max(e, float(np.abs(o[:, -2:] - ref1)[:, :, taps_in[0]].max()) / RAMP)
    return max(e, 1e-7), o, taps_in


def homo_gate(U, th, oh, ow, e):
    """The value gate of the homography family -> (ref, bound): close_grad(tol_px = 4 e, base 1e-4) against the fp64 warp of U
    [n,c,h,w] by theta `th` [1,3,3] (every image the same theta), with the sampler's border discontinuity under the same 4 e
    (sampler_slack) and its rounding residue outside the image (blend_residue)."""
    n, _, h, w = U.shape
    xn, yn, _ = homography_coords(th, oh, ow)
    xn, yn = np.repeat(xn, n, 0), np.repeat(yn, n, 0)
    ref, slack = sampler_slack(bilinear_clamped, U, xn, yn, 4 * e * 2 / w, 4 * e * 2 / h)
    return ref, 1e-4 + np.maximum(4 * e * grad4(ref), slack) + blend_residue(U, xn, yn)



# ------------------------------------------------------------------------------------------------ inputs of the sweeps
# Shared by tests/test_ref64.py (CPU: the fp32 oracle against the functions above on these very inputs) and
# tests/test_gpu_kernel_sweeps.py (the kernels against them).  Seeds fixed; every builder returns fp32 numpy arrays.
def cv_inputs(n, c, h, w, seed=0):
    rs = np.random.RandomState(1000 + seed + 7 * c + 131 * h + 17 * w)
    return (rs.normal(0, 1, (n, c, h, w)).astype(F32), rs.normal(0, 1, (n, c, h, w)).astype(F32))


def ccl_chain(images, c, h, w, seed=0):
    """The G4 construction (cases.g4_inputs) as a chain: image k + 1 = |image k rolled by (1, -1) + 0.3 N(0, 1)|, so that every
    neighbouring pair has a peaked soft-argmax.  [images,c,h,w]."""
    rs = np.random.RandomState(2000 + seed + 7 * c + 131 * h + 17 * w)
    out = [np.abs(rs.normal(0, 1, (c, h, w))).astype(F32)]
    for _ in range(images - 1):
        out.append(np.abs(np.roll(out[-1], (1, -1), axis=(1, 2)) + (0.3 * rs.normal(0, 1, (c, h, w))).astype(F32)).astype(F32))
    return np.stack(out)


HOMO_IN = (45, 60)          # input map of the homography sweep


def homo_input(n, c):
    """[n,c,45,60]: c - 2 texture channels N(0, 1), then an x-ramp and a y-ramp (index / 64): a sampled ramp value * 64 is the
    sampling coordinate in pixels wherever the four taps are inside the image."""
    h, w = HOMO_IN
    rs = np.random.RandomState(3000 + c)
    u = rs.normal(0, 1, (n, c, h, w)).astype(F32)
    if c >= 2:
        u[:, c - 2] = (np.arange(w, dtype=F32) * F32(RAMP))[None, None, :]
        u[:, c - 1] = (np.arange(h, dtype=F32) * F32(RAMP))[None, :, None]
    return u


def homo_thetas(out_h):
    """name -> theta [3,3] fp32.  `zero_row`: ts = gy + 1 is EXACTLY 0 on output row 0 and at least one grid step elsewhere (the
    first grid value is -1 in every linspace; the inner ones differ by an ulp between implementations -- start + step * i with or
    without a fused multiply-add -- so no inner row can be made exactly 0 for all of them); the numerators are O(1e-6) so that the
    guarded row (ts := 1e-6) samples a line inside the image and the other rows the neighbourhood of one point.  `under` / `over`: a constant ts of 0.9e-7 / 1.1e-7, either
    side of the guard's threshold, numerators O(1e-7): both in range, a moved threshold changes `over` tenfold."""
    num = np.array([[0.8, 0.1, 0.05], [-0.1, 0.7, -0.1]])
    th = {
        'identity': np.eye(3),
        'g2_mild': np.array([[1.02, 0.03, 0.10], [-0.02, 0.97, -0.05], [0.01, -0.02, 1.0]]),
        'g2_far': np.array([[0.8, 0.1, 0.9], [0.05, 1.3, -0.7], [0.15, 0.1, 1.0]]),
        'zero_row': np.concatenate((1e-6 * num, [[0.0, 1.0, 1.0]])),
        'under': np.concatenate((1e-7 * num, [[0.0, 0.0, 0.9e-7]])),
        'over': np.concatenate((1e-7 * num, [[0.0, 0.0, 1.1e-7]])),
    }
    return {k_: v.astype(F32) for k_, v in th.items()}


def rigid_px(h, w):
    import torch
    xs = torch.linspace(0.0, float(w), 9).numpy()
    ys = torch.linspace(0.0, float(h), 7).numpy()
    return np.stack(np.broadcast_arrays(xs[None, :], ys[:, None]), axis=2)[None].astype(F32)


def norm_px(mesh, h, w):
    out = np.empty_like(mesh, dtype=F32)
    out[..., 0] = mesh[..., 0] * F32(2.0) / F32(w) - F32(1.0)
    out[..., 1] = mesh[..., 1] * F32(2.0) / F32(h) - F32(1.0)
    return out.reshape(mesh.shape[0], -1, 2)


def tps_meshes(n, h, w, seed=107):
    """cases.g5_meshes at any frame size: sigma 6 px + a +-40 px shift, normalised for the (h, w) frame -> (rigid, warped) [n,63,2]."""
    rs = np.random.RandomState(seed + n + h)
    r = np.repeat(rigid_px(h, w), n, axis=0)
    warped = r + rs.normal(0, 6.0, r.shape).astype(F32) + rs.uniform(-40, 40, (n, 1, 1, 2)).astype(F32)
    return norm_px(r, h, w), norm_px(warped, h, w)


def tps_queries(n, q, seed=0):
    rs = np.random.RandomState(4000 + seed + q)
    return rs.uniform(-1.1, 1.1, (n, q, 2)).astype(F32)


def warp_case(b, h, w, hc, wc, seed=0):
    """Dense-warp inputs: U [b,5,h,w] = 3 smooth texture planes (0..255) + x-ramp + y-ramp (pixel indices); source [b,63,2] = the
    rigid mesh + N(0, sigma), sigma = 12 px at 720p scaled with the frame height, + a shift of up to half the frame, normalised on
    the canvas; target = the rigid mesh normalised on the frame."""
    rs = np.random.RandomState(5000 + seed + 3 * h + 5 * wc + 7 * hc)
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing='ij')
    U = np.empty((b, 5, h, w), F32)
    for i in range(b):
        for ch in range(3):
            fx, fy, ph = rs.uniform(0.02, 0.09), rs.uniform(0.02, 0.09), rs.uniform(0, 6.28)
            U[i, ch] = 127.5 + 100.0 * np.sin(fx * xx + ph) * np.cos(fy * yy + 0.5 * ph)
        U[i, 3] = xx
        U[i, 4] = yy
    r = np.repeat(rigid_px(h, w), b, axis=0)
    if 4 * h <= hc:
        # a frame far smaller than its canvas (2 x 2 -> 8 x 64): stretched over the canvas (a spline whose control points all lie in
        # one corner is extrapolated over the rest and no fixed coordinate tolerance applies), sigma in canvas pixels
        m = np.repeat(rigid_px(hc, wc), b, axis=0) + rs.normal(0, 12.0 * hc / 720.0, r.shape).astype(F32)
    else:
        m = r + rs.normal(0, 12.0 * h / 720.0, r.shape).astype(F32)
        m[..., 0] += rs.uniform(0, max(wc - w, 0) + 0.5 * w, (b, 1, 1)).astype(F32) - F32(0.25 * w)
        m[..., 1] += rs.uniform(0, max(hc - h, 0) + 0.25 * h, (b, 1, 1)).astype(F32) - F32(0.125 * h)
    return U, norm_px(m, hc, wc), norm_px(r, h, w)


def tsm_inputs(n, seed=0):
    """(smotion, tmotion) [n,7,9,2] in LR pixels of the size the nets produce: N(0, 3 px) + a common drift, N(0, 2 px)."""
    rs = np.random.RandomState(9000 + seed + n)
    sm = rs.normal(0, 3.0, (n, 7, 9, 2)) + rs.uniform(-20, 20, (n, 1, 1, 2))
    return sm.astype(F32), rs.normal(0, 2.0, (n, 7, 9, 2)).astype(F32)


def metric_planes(frames, h, w, mask, seed=0):
    """Two [frames,4,h,w] warps for psnr_ssim: colour = cases.g11_images' construction (uniform 0..255, second = first + N(0, 12)
    clipped); mask plane: 'ones', 'binary' (random 0 / 1) or 'frac' (a bilinear-warped ones plane: 1 inside, a fractional rim, 0)."""
    rs = np.random.RandomState(6000 + seed + 3 * h + w)
    a = rs.uniform(0, 255, (frames, 3, h, w)).astype(F32)
    b = np.clip(a + rs.normal(0, 12, a.shape), 0, 255).astype(F32)
    ms = []
    for k in range(2):
        if mask == 'ones':
            m = np.ones((frames, 1, h, w), F32)
        elif mask == 'binary':
            m = (rs.uniform(0, 1, (frames, 1, h, w)) < 0.8).astype(F32)
        else:
            ones = np.ones((frames, 1, h, w), F32)
            gx = linspace(w)[None, None, :] * (1.0 + 0.08 * k) + 0.1 * (k + 1)
            gy = linspace(h)[None, :, None] * 1.05 - 0.07 * (k + 1) + 0.02 * linspace(w)[None, None, :]
            gx = np.broadcast_to(gx, (frames, h, w)) + 0.0 * gy
            gy = np.broadcast_to(gy, (frames, h, w))
            m = bilinear_clamped(ones, gx, gy).astype(F32)
        ms.append(m)
    return np.concatenate((a, ms[0]), 1), np.concatenate((b, ms[1]), 1)


def metric_paths(t, seed=0):
    """A stitched smooth path [t,63,2] of pipeline-like size: the cumulative sum of ~1 px motions."""
    rs = np.random.RandomState(7000 + seed + t)
    return np.cumsum(rs.normal(0, 1.0, (t, 63, 2)), axis=0).astype(F32)


def metric_meshes(t, seed=0):
    """[t,7,9,2] LR meshes: rigid 360 x 480 + N(0, 4 px), a few cells stretched beyond the intra-grid limit of 120 px."""
    rs = np.random.RandomState(8000 + seed + t)
    m = np.repeat(rigid_px(360, 480), t, axis=0) + rs.normal(0, 4.0, (t, 7, 9, 2)).astype(F32)
    m[t // 2, :, 5:, 0] += F32(70.0)
    return m.astype(F32)


# ================================================================================================ convolution sweep
# Shared by tests/test_ref64.py (CPU) and tests/test_gpu_conv_sweeps.py (the kernels).
def conv_inputs(n, cin, cout, h, w, k=(1, 3, 3), t=None, out_hw=None, bias=True, res=False, seed=0):
    """Seeded operands of one convolution in torch's layouts: x [n,cin,(t,)h,w] N(0, 1), w [cout,cin,(kt,)kh,kw] N(0, 1 / K),
    bias [cout] N(0, 1) | None, res N(0, 1) of the output's shape (out_hw = (to, ho, wo) or (ho, wo)) | None."""
    kt, kh, kw = k
    rs = np.random.RandomState((11000 + seed + 7 * cin + 13 * cout + 131 * h + 17 * w + 3 * n + 1009 * kh + 10007 * kw + 5 * kt) % (2 ** 31))
    three = t is not None
    x = rs.normal(0, 1, (n, cin, t, h, w) if three else (n, cin, h, w)).astype(F32)
    wt = (rs.normal(0, 1, (cout, cin, kt, kh, kw) if three else (cout, cin, kh, kw)) / np.sqrt(cin * kt * kh * kw)).astype(F32)
    b = rs.normal(0, 1, cout).astype(F32) if bias else None
    r = rs.normal(0, 1, (n, cout) + tuple(out_hw)).astype(F32) if res else None
    return x, wt, b, r


def cdiv(a, b):
    return -(-a // b)


def conv_splits(M, cout, groups, nk, target=512):
    """conv.hip's conv_splits, restated: the number of K splits of an implicit-GEMM launch (1 = none)."""
    b64 = cdiv(M, 64) * cdiv(cout, 64) * groups
    want = (target + b64 - 1) // b64
    if want == 2 and nk < 32 and b64 * 5 >= target * 3:
        want = 1
    maxs = max(nk // 4, 1)
    splits = min(want, maxs)
    if splits <= 1:
        return 1
    return cdiv(nk, cdiv(nk, splits))


def igemm_plan(M, K, cout, taps, groups=1, workspace=True):
    """conv.hip's conv_dispatch + launch_auto, restated -> dict(tile, amode, tail, splits, tps, nk, b64, b128, b128m, kernel):
    what a launch of M output pixels, K = taps x channels, runs in the shipped library (no tuning knobs).  `kernel` is the
    instantiation's template argument list as kernel_key() prints it."""
    nk = cdiv(K, 32)
    splits = conv_splits(M, cout, groups, nk) if workspace else 1
    tps = cdiv(nk, splits)
    splits = cdiv(nk, tps)
    tail = K % 32 != 0 and K % 32 < 16
    b64 = cdiv(M, 64) * cdiv(cout, 64) * groups
    b128 = cdiv(M, 64) * (cout // 128) * groups
    b128m = cdiv(M, 128) * cdiv(cout, 64) * groups
    if splits == 1 and cout % 128 == 0 and b128 >= 2048 and not tail:
        tile, wm, wn, use_tail = '64x128', 1, 2, False
    elif splits == 1 and b128m >= 2048:
        tile, wm, wn, use_tail = '128x64', 2, 1, tail
    else:
        tile, wm, wn, use_tail = '64x64', 1, 1, tail
    bn = 64 * wn
    tab = tps * 8 * 8
    amode = 0 if (taps > 64 or tab > 24576) else (1 if taps <= 32 else 2)
    if amode == 1 and not use_tail and cout % bn == 0 and K % 32 == 0:
        amode = 3
    return dict(tile=tile, amode=amode, tail=use_tail, splits=splits, tps=tps, nk=nk, b64=b64, b128=b128, b128m=b128m,
                kernel='conv_igemm_kernel<2,2,%d,%d,1,1,32,%d,1,%d>' % (wm, wn, int(use_tail), amode))


def kernel_key(name):
    """A kernel name of the code object, mangled or demangled -> 'name<a,b,...>' with booleans as 0 / 1 ('name' without arguments)."""
    import re
    m = re.match(r'^_Z(\d+)', name)
    if m:
        start = m.end()
        base, rest = name[start:start + int(m.group(1))], name[start + int(m.group(1)):]
        t = re.match(r'^I((?:L[a-z]\d+E)+)E', rest)
        args = re.findall(r'L[a-z](\d+)E', t.group(1)) if t else []
        return base + ('<%s>' % ','.join(args) if args else '')
    m = re.match(r'^(?:void )?([A-Za-z_0-9]+)(?:<([^>]*)>)?', name)
    args = [a.strip() for a in (m.group(2) or '').split(',') if a.strip()]
    args = [{'true': '1', 'false': '0'}.get(a, a) for a in args]
    return m.group(1) + ('<%s>' % ','.join(args) if args else '')


def split_kernel_name(name):
    """A demangled kernel name of the code object -> (base name, parameter list without its parentheses); a name that is still
    mangled, or carries no parameter list, raises ValueError: overloads cannot be told apart without one."""
    import re
    m = re.match(r'^(?:void )?([A-Za-z_][A-Za-z_0-9]*)', name)
    if name.startswith('_Z') or not m or not name.endswith(')'):
        raise ValueError('not a demangled kernel name with its parameter list: %r' % name)
    depth = 0
    for i in range(len(name) - 1, m.end() - 1, -1):                         # the parenthesis that the last one closes
        depth += {')': 1, '(': -1}.get(name[i], 0)
        if depth == 0:
            return m.group(1), name[i + 1:-1]
    raise ValueError('not a demangled kernel name with its parameter list: %r' % name)


def parameter_lists(names):
    """Demangled kernel names -> {base name: the set of distinct parameter lists the names carry under it}."""
    lists = {}
    for n in names:
        base, params = split_kernel_name(n)
        lists.setdefault(base, set()).add(params)
    return lists


def overload_key(name, lists):
    """A demangled kernel name -> its key in library_reach: the base name, followed by the parenthesised parameter list whenever
    `lists` (parameter_lists of every kernel of the library) holds more than one parameter list under that base name.  Template
    arguments are dropped: the instantiations of one overload share a key."""
    base, params = split_kernel_name(name)
    return base + ('(%s)' % params if len(lists[base]) > 1 else '')


# ------------------------------------------------------------------------------------------------ fp32 Winograd, emulated
def _stage32(mat, d, axis):
    """One transform stage in fp32: out[i] = sum_a mat[i, a] d[a] along `axis`, term by term, every product and sum rounded."""
    d = np.moveaxis(d, axis, 0)
    out = np.zeros((mat.shape[0],) + d.shape[1:], F32)
    for i in range(mat.shape[0]):
        acc = None
        for a in range(mat.shape[1]):
            if mat[i, a] == 0:
                continue
            term = (F32(mat[i, a]) * d[a]).astype(F32)
            acc = term if acc is None else (acc + term).astype(F32)
        out[i] = acc
    return np.moveaxis(out, 0, axis)


def wino_emul32(x, w, m, bias=None, res=None, relu=False):
    """F(m x m, 3 x 3) of x [n,c,h,w], w [cout,c,3,3] as an fp32 program: filters G g G^T formed in fp64 and rounded once (as the
    pack kernels do), B^T d B and A^T M A stage by stage in fp32, the channel sum an fp32 matrix product per transform position,
    then bias, residual, ReLU in fp32 -> [n,cout,h,w] fp32.  Not the kernels' order of operations: a same-precision restatement
    whose distance from ref64 calibrates the Winograd gate (wino_rho)."""
    from ref64 import WINO, wino_tiles, wino_untile
    k = WINO[m]
    x, w = np.asarray(x, F32), np.asarray(w, F32)
    u = np.einsum('ia,ocab,jb->ijoc', k['G'], w.astype(np.float64), k['G']).astype(F32)            # [a,a,co,c]
    d = wino_tiles(x, m)                                                                         # [n,c,th,tw,a,a]
    v = _stage32(k['BT'], _stage32(k['BT'], d, 4), 5)
    n, c, th, tw, a, _ = v.shape
    vv = np.ascontiguousarray(v.transpose(4, 5, 1, 0, 2, 3).reshape(a, a, c, n * th * tw))
    mm = np.matmul(u, vv).reshape(a, a, w.shape[0], n, th, tw).transpose(3, 2, 4, 5, 0, 1)           # fp32 sum over c
    y = wino_untile(_stage32(k['AT'], _stage32(k['AT'], np.ascontiguousarray(mm), 4), 5), x.shape[2], x.shape[3])
    if bias is not None:
        y = (y + np.asarray(bias, F32).reshape(1, -1, 1, 1)).astype(F32)
    if res is not None:
        y = (y + np.asarray(res, F32)).astype(F32)
    return np.maximum(y, F32(0)) if relu else y


def wino_gate(x, w, m, bias=None, res=None, relu=False, spare=1.0):
    """-> (ref64 value, bound, rho, S_w): the Winograd gate min(ceiling, 4 rho u S_w) / spare per element, rho = max |emul32 - ref64| /
    (u S_w) of THIS input from the CPU emulation above (never from a kernel), ceiling = ref64.wino_ceiling."""
    import ref64 as R
    ref, _ = R.conv(x, w, bias, res, 1, 1, relu)
    s_w = R.wino_scale(x, w, m, bias, res)
    rho = float((np.abs(wino_emul32(x, w, m, bias, res, relu).astype(np.float64) - ref) / (R.U24 * s_w)).max())
    bound = np.minimum(R.wino_ceiling(x.shape[1], m, s_w), 4 * rho * R.U24 * s_w) / spare
    return ref, bound, rho, s_w


# ------------------------------------------------------------------------------------------------ cases of the implicit GEMM
def IG(name, n, h, w, cin, cout, k, s=1, p=(0, 0, 0), t=None, bias=True, res=False, relu=False, out_cs=None, groups=1, c_real=None,
       ws=True, claim=None, big=False):
    """One ss_conv_nhwc case.  k = (kt, kh, kw), p = (pt, ph, pw); cin: channels of the NHWC tensor (a multiple of 4), c_real of them
    real (the rest zero in input and filters: layout padding); ws=False: no workspace (no split-K).  claim = 'tile mode tail
    splits' the launch is claimed to take (checked against igemm_plan on the CPU, against a kernel trace in LAB_NOTES.md T)."""
    return dict(name=name, n=n, h=h, w=w, cin=cin, cout=cout, k=k, s=s, p=p, t=t, bias=bias, res=res, relu=relu, out_cs=out_cs or cout,
                groups=groups, c_real=c_real or cin, ws=ws, claim=claim, big=big)


def ig_geometry(c):
    kt, kh, kw = c['k']
    pt, ph, pw = c['p']
    t = c['t'] or 1
    to, ho, wo = t + 2 * pt - kt + 1, (c['h'] + 2 * ph - kh) // c['s'] + 1, (c['w'] + 2 * pw - kw) // c['s'] + 1
    return to, ho, wo, c['n'] * to * ho * wo, kt * kh * kw * c['cin']


def ig_plan(c):
    to, ho, wo, M, K = ig_geometry(c)
    return igemm_plan(M, K, c['cout'], c['k'][0] * c['k'][1] * c['k'][2], c['groups'], c['ws'])


def ig_claim(plan):
    return '%s m%d t%d s%d' % (plan['tile'], plan['amode'], int(plan['tail']), plan['splits'])


X1, X3 = (1, 1, 1), (1, 3, 3)
P1 = (0, 1, 1)
IGEMM_CASES = [
    # ---- the 64x64 tile around one tile of rows: 1x1, K = 32 (nk = 1, maxs = 1: no split), cout = 64 = BN, K % 32 == 0: mode 3
    IG('t64_M63', 1, 7, 9, 32, 64, X1, claim='64x64 m3 t0 s1'),
    IG('t64_M64', 1, 8, 8, 32, 64, X1, res=True, relu=True, claim='64x64 m3 t0 s1'),
    IG('t64_M65', 1, 5, 13, 32, 64, X1, claim='64x64 m3 t0 s1'),
    # ---- 128x64: splits == 1 and b128m = cdiv(M, 128) * cdiv(cout, 64) >= 2048.  M = 513 * 511 = 262143: cdiv = 2048, 127 rows in the last
    # tile.  cout = 3 keeps the float64 reference small (one tile of 64 columns either way); mode 3 needs cout % 64 == 0.
    IG('t128_m3', 1, 513, 511, 32, 64, X1, res=True, relu=True, big=True, claim='128x64 m3 t0 s1'),         # K = 32
    IG('t128_m1', 1, 513, 511, 20, 3, X1, big=True, claim='128x64 m1 t0 s1'),                               # K = 20: K % 32 = 20 >= 16
    IG('t128_m1_tail', 1, 513, 511, 4, 3, X3, p=P1, relu=True, big=True, claim='128x64 m1 t1 s1'),          # K = 36: K % 32 = 4
    IG('t128_m2', 1, 513, 511, 4, 3, (1, 6, 6), p=(0, 3, 3), big=True, claim='128x64 m2 t0 s1'),            # 36 taps, K = 144: 16; map 514 x 512: M = 263168
    IG('t128_m2_tail', 1, 513, 511, 4, 3, (1, 7, 7), p=(0, 3, 3), c_real=3, big=True, claim='128x64 m2 t1 s1'),   # 49 taps, K = 196: 4
    IG('t128_m0', 1, 513, 511, 4, 3, (2, 5, 7), p=(0, 2, 3), t=2, big=True, claim='128x64 m0 t0 s1'),       # 70 taps, K = 280: 24
    IG('t128_m0_tail', 1, 513, 511, 4, 3, (3, 5, 5), p=(0, 2, 2), t=3, big=True, claim='128x64 m0 t1 s1'),  # 75 taps, K = 300: 12
    # ---- 64x128: splits == 1, cout % 128 == 0, b128 = cdiv(M, 64) * (cout / 128) >= 2048, K % 32 == 0 or >= 16.  M = 363 * 361 = 131043:
    # cdiv = 2048, 35 rows in the last tile; cout = 256: M = 257 * 255 = 65535: 1024 * 2.
    IG('t64x128_m3', 1, 363, 361, 32, 128, X1, res=True, relu=True, big=True, claim='64x128 m3 t0 s1'),
    IG('t64x128_m3_c256', 1, 257, 255, 32, 256, X1, big=True, claim='64x128 m3 t0 s1'),
    IG('t64x128_m1', 1, 363, 361, 16, 128, X1, big=True, claim='64x128 m1 t0 s1'),                          # K = 16
    IG('t64x128_m2', 1, 364, 362, 4, 128, (1, 6, 6), p=(0, 2, 2), big=True, claim='64x128 m2 t0 s1'),       # 363 x 361 out, K = 144
    IG('t64x128_m0', 1, 363, 361, 4, 128, (2, 5, 7), p=(0, 2, 3), t=2, big=True, claim='64x128 m0 t0 s1'),  # K = 280
    # ---- address modes on the 64x64 tile.  mode 1: <= 32 taps and (cout % 64 != 0 or K % 32 != 0); K % 32 in {4, 12} takes TAIL
    IG('m1_cout3', 2, 9, 11, 32, 3, X1, claim='64x64 m1 t0 s1'),
    IG('m1_cout65', 2, 9, 11, 64, 65, X1, relu=True, claim='64x64 m1 t0 s1'),                               # nk = 2
    IG('m1_cout124', 1, 11, 15, 32, 124, X3, p=P1, res=True, claim='64x64 m1 t0 s2'),                       # K = 288, nk = 9, b64 = 6: maxs = 2
    IG('k4', 1, 9, 11, 4, 64, X3, p=P1, c_real=2, claim='64x64 m1 t1 s1'),                                  # K = 36
    IG('k12', 1, 9, 11, 12, 64, X3, p=P1, c_real=11, claim='64x64 m1 t1 s1'),                               # K = 108, nk = 4: maxs = 1
    IG('k16', 1, 9, 11, 16, 64, X3, p=P1, claim='64x64 m1 t0 s1'),                                          # K = 144, nk = 5
    IG('k20', 1, 9, 11, 20, 64, X3, p=P1, claim='64x64 m1 t0 s1'),                                          # K = 180, nk = 6
    IG('k28', 1, 9, 11, 28, 64, X3, p=P1, c_real=27, claim='64x64 m1 t0 s2'),                               # K = 252, nk = 8, b64 = 2: maxs = 2
    # mode 2: 33 .. 64 taps
    IG('m2_7x7', 2, 20, 24, 4, 64, (1, 7, 7), s=2, p=(0, 3, 3), c_real=3, relu=True, claim='64x64 m2 t1 s1'),    # K = 196, nk = 7
    IG('m2_8x8', 1, 12, 13, 4, 64, (1, 8, 8), p=(0, 4, 4), claim='64x64 m2 t0 s2'),                         # K = 256, nk = 8, b64 = 3
    IG('m2_5x3x3', 1, 7, 9, 4, 64, (5, 3, 3), p=(2, 1, 1), t=7, claim='64x64 m2 t0 s1'),                    # 45 taps, K = 180, nk = 6
    IG('m2_5x3x3_tail', 1, 7, 9, 8, 64, (5, 3, 3), p=(2, 1, 1), t=7, claim='64x64 m2 t1 s3'),               # K = 360: 8, nk = 12, b64 = 7: maxs = 3
    # mode 0: more than 64 taps, or a tap table past 24 KB (tiles_per_split * 64 bytes: an UNSPLIT K beyond 384 tiles)
    IG('m0_5x5x5', 1, 6, 7, 4, 64, (5, 5, 5), p=(2, 2, 2), t=5, claim='64x64 m0 t0 s4'),                    # K = 500: 20, nk = 16, b64 = 4: maxs = 4
    IG('m0_3x5x5_tail', 1, 6, 7, 4, 64, (3, 5, 5), p=(1, 2, 2), t=4, claim='64x64 m0 t1 s2'),               # K = 300: 12, nk = 10
    IG('m0_long_table', 1, 5, 5, 1368, 64, X3, p=P1, ws=False, claim='64x64 m0 t0 s1'),                     # K = 12312, nk = 385: 24640 B
    # ---- filter geometry
    IG('g_s2_p0', 2, 9, 11, 8, 64, X3, s=2, claim='64x64 m1 t1 s1'),                                        # K = 72: 8
    IG('g_s3_p2', 2, 10, 7, 8, 64, X3, s=3, p=(0, 2, 2), claim='64x64 m1 t1 s1'),                           # pad = k / 2 + 1
    IG('g_5x5_s2_p3', 1, 9, 12, 8, 64, (1, 5, 5), s=2, p=(0, 3, 3), claim='64x64 m1 t1 s1'),                # K = 200: 8
    IG('g_pad_asym', 1, 6, 9, 8, 64, X3, p=(0, 0, 2), claim='64x64 m1 t1 s1'),
    IG('g_map_lt_filter', 3, 2, 3, 4, 64, (1, 7, 7), p=(0, 3, 3), claim='64x64 m2 t1 s1'),                  # a 2 x 3 map under a 7 x 7 filter
    IG('g_1x1_map', 5, 1, 1, 64, 64, X3, p=P1, res=True, relu=True, claim='64x64 m3 t0 s4'),                # K = 576, nk = 18, b64 = 1
    # ---- split-K plans (want = ceil(512 / b64), cut to maxs = nk / 4, then re-divided)
    IG('sk_b64_511', 1, 64, 73, 128, 448, X3, p=P1, claim='64x64 m3 t0 s2'),                                # nk = 36 >= 32: want 2
    IG('sk_b64_512', 1, 64, 64, 128, 512, X3, p=P1, claim='64x64 m3 t0 s1'),                                # want 1
    IG('sk_exc_b64_307', 1, 64, 307, 32, 64, X3, p=P1, res=True, relu=True, claim='64x64 m3 t0 s2'),        # nk = 9 < 32, 5 * 307 < 1536: cut (5 + 4)
    IG('sk_exc_b64_308', 1, 64, 77, 32, 256, X3, p=P1, claim='64x64 m3 t0 s1'),                             # 5 * 308 >= 1536: the round-6 exception
    IG('sk_exc_nk31', 1, 64, 77, 992, 256, X1, claim='64x64 m3 t0 s1'),                                     # b64 = 308, nk = 31: exception
    IG('sk_exc_nk32', 1, 64, 77, 1024, 256, X1, claim='64x64 m3 t0 s2'),                                    # nk = 32: cut
    IG('sk_b64_256', 1, 64, 64, 64, 256, X3, p=P1, claim='64x64 m3 t0 s2'),                                 # nk = 18: want 2 (5 * 256 < 1536)
    IG('sk_b64_255', 1, 64, 85, 64, 192, X3, p=P1, res=True, relu=True, claim='64x64 m3 t0 s3'),            # want 3: 6 + 6 + 6
    IG('sk_b64_171', 1, 64, 57, 64, 192, X3, p=P1, claim='64x64 m3 t0 s3'),
    IG('sk_b64_170', 1, 64, 85, 64, 128, X3, p=P1, relu=True, claim='64x64 m3 t0 s4'),                      # want 4 = maxs: 5 + 5 + 5 + 3
    IG('sk_maxs', 1, 3, 5, 32, 64, X3, p=P1, res=True, claim='64x64 m3 t0 s2'),                             # b64 = 1: want 512, maxs = 9 / 4 = 2
    IG('sk_last_tail_tile', 2, 23, 30, 72, 64, X3, p=P1, res=True, relu=True, claim='64x64 m1 t1 s5'),      # K = 648: 8, nk = 21, maxs = 5: 5 x 4 + 1
    IG('sk_out_cs', 1, 11, 15, 32, 64, X3, p=P1, res=False, relu=True, out_cs=72, claim='64x64 m3 t0 s2'),
    # ---- conv3d: SmoothNet's 128 -> 128 layers on the 7 x 9 mesh, window t = 7 and a clip of 32, with and without temporal padding
    IG('c3d_5x3x3_t7', 2, 7, 9, 128, 128, (5, 3, 3), p=(2, 1, 1), t=7, relu=True, claim='64x64 m2 t0 s18'),      # K = 5760, nk = 180, b64 = 28: want 19, 10 tiles each
    IG('c3d_5x3x3_t7_nopad', 2, 7, 9, 128, 128, (5, 3, 3), p=(0, 1, 1), t=7, relu=True, claim='64x64 m2 t0 s36'),        # to = 3, b64 = 12: want 43, 5 tiles each
    IG('c3d_3x3x3_t7', 2, 7, 9, 128, 128, (3, 3, 3), p=(1, 1, 1), t=7, claim='64x64 m3 t0 s18'),                 # K = 3456, nk = 108: 6 tiles each
    IG('c3d_5x3x3_t32', 1, 7, 9, 128, 128, (5, 3, 3), p=(2, 1, 1), t=32, relu=True, claim='64x64 m2 t0 s8'),     # b64 = 64
    IG('c3d_3x3x3_t32_nopad', 1, 7, 9, 128, 128, (3, 3, 3), p=(0, 1, 1), t=32, claim='64x64 m3 t0 s9'),
]


# ------------------------------------------------------------------------------------------------ pool in the split-K reduction, groups
POOL_REDUCE_CASES = [              # (n, h, w, cin, cout, groups, out_cs): 3 x 3 / pad 1, every one of them splits (b64 <= 12, nk = 9 or 18)
    (2, 12, 16, 32, 64, 1, 64),        # even Ho, Wo
    (2, 11, 15, 32, 64, 1, 64),        # odd: the last row and column are dropped
    (1, 11, 16, 64, 128, 2, 128),      # two groups, odd Ho, even Wo
    (1, 2, 3, 32, 64, 1, 72),          # the smallest map the entry takes; out_cs > cout
    (3, 5, 6, 32, 64, 2, 80),          # two groups and out_cs > cout
]


# ------------------------------------------------------------------------------------------------ the stem
STEM_SIZES = [(1, 1), (2, 2), (7, 8), (8, 9), (9, 7), (45, 61), (61, 45)]          # (h, w); 360 x 480 is a case of its own
STEM_K, STEM_TAPS = 7 * 24, 7      # ss_conv_stem3's K axis is (filter row, 24): K % 32 = 8 -> TAIL, 7 table entries -> mode 1


def stem_inputs(n, h, w, groups, seed=0):
    """x [n,3,h,w] N(0, 1), w [groups * 64,3,7,7] N(0, 0.1), bias [groups * 64] N(0, 1) (BatchNorm already folded)."""
    rs = np.random.RandomState(12000 + seed + 131 * h + 17 * w + 3 * n + groups)
    return (rs.normal(0, 1, (n, 3, h, w)).astype(F32), rs.normal(0, 0.1, (groups * 64, 3, 7, 7)).astype(F32),
            rs.normal(0, 1, groups * 64).astype(F32))


def stem_plan(n, h, w, cout, groups=1):
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    return igemm_plan(n * ho * wo, STEM_K, cout, STEM_TAPS, groups, workspace=False)


# ------------------------------------------------------------------------------------------------ F(2x2,3x3)
def wino_blocks(h, w):
    """wino.hip's wino_blocks: (8, 4) or (4, 8) blocks of 2 x 2 tiles, whichever wastes fewer tile slots (a tie goes to 8 x 4)."""
    th, tw = (h + 1) // 2, (w + 1) // 2
    e84 = h * w / (4.0 * cdiv(th, 8) * 8 * cdiv(tw, 4) * 4)
    e48 = h * w / (4.0 * cdiv(th, 4) * 4 * cdiv(tw, 8) * 8)
    return (8, 4) if e84 >= e48 else (4, 8)


def wino2_kernel(h, w, res=False, pool=False, sliced=False):
    tbh, tbw = wino_blocks(h, w)
    if pool:
        return 'conv_wino_kernel<%d,%d,2,0,1,0,1>' % (tbh, tbw)
    return 'conv_wino_kernel<%d,%d,2,%d,%d,%d,0>' % (tbh, tbw, int(res), int(not sliced), int(sliced))


_W2_SIZES = [1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 33]
_W2_MAPS = ([(1, s) for s in _W2_SIZES] + [(s, 1) for s in _W2_SIZES[1:]] +
            [(2, 3), (3, 2), (7, 16), (16, 7), (8, 8), (9, 17), (17, 9), (15, 33), (33, 15), (16, 16), (31, 31), (33, 33), (31, 8)])
_W2_COUT = [64, 128, 192]
_W2_CIN = [4, 20, 40, 60, 64, 160, 36, 52]                             # chunk tails (cin % 16): 4, 4, 8, 12, 0, 0, 4, 4
WINO2_CASES = [(2, h, w, _W2_CIN[i % len(_W2_CIN)], _W2_COUT[i % 3]) for i, (h, w) in enumerate(_W2_MAPS)]      # (n, h, w, cin, cout)


# ------------------------------------------------------------------------------------------------ F(4x4,3x3)
def wino43_kernel(w, cin, res):
    return 'conv_wino43p_kernel<%d,%d,%d>' % (int(res), int(cin == 16), int(w <= 31))


def wino43_blocks(n, h, w, cout, groups=1):
    bh, bw = (16, 32) if w <= 31 else (8, 60)
    return n * cdiv(h, bh) * cdiv(w, bw) * (cout // 64)            # per group


WINO43_CASES = [                   # (n, h, w, cin, cout)      geometry 16 x 32 for w <= 31, else 8 x 60
    (1, 1, 1, 16, 64), (2, 7, 4, 48, 64), (1, 8, 29, 64, 64), (1, 9, 30, 80, 64), (1, 15, 31, 16, 128), (1, 16, 32, 48, 64),
    (1, 17, 33, 64, 64), (1, 46, 59, 16, 64), (2, 8, 60, 64, 64), (1, 9, 61, 80, 64), (1, 15, 119, 48, 64), (1, 16, 120, 64, 128),
    (1, 17, 121, 16, 64), (1, 1, 33, 64, 64), (1, 46, 1, 48, 64),
    (11, 46, 120, 32, 128),        # 11 x 6 x 2 x 2 = 264 blocks: more than the 256 CUs, so persistent workgroups take several
]


# ------------------------------------------------------------------------------------------------ the reach table
# Kernels of the convolution engine that the product library carries but no call of the C ABI launches: named here so that the
# table below does not claim them.
UNREACHABLE = {
    'stem_pool_kernel': 'ss_stem_pool launches stem_pool_kernel_half unconditionally (SP_SPLIT_DEFAULT in stem.hip); the two-halves '
                        'kernel is selected by a knob of the tuning build only',
}
CONV_ENGINE_KERNELS = ('conv_igemm_kernel', 'splitk_reduce_kernel', 'conv_wino_kernel', 'conv_wino43', 'stem_pool')


def reach_table():
    """instantiation (kernel_key form) -> the cases of tests/test_gpu_conv_sweeps.py claimed to launch it.  Built from the case
    lists above through the restated dispatch rules (igemm_plan, wino_blocks, wino43_kernel); tests/test_ref64.py holds it to the
    kernels of the built library, LAB_NOTES.md part T to a kernel trace of the sweep."""
    table = {}

    def add(kernel, case):
        table.setdefault(kernel, []).append(case)
    for c in IGEMM_CASES:
        p = ig_plan(c)
        add(p['kernel'], 'igemm[%s]' % c['name'])
        if p['splits'] > 1:
            add('splitk_reduce_kernel', 'igemm[%s]' % c['name'])
    for case in POOL_REDUCE_CASES:
        add('splitk_reduce_kernel', 'pool_in_reduce[%s]' % '-'.join(map(str, case)))
    for (h, w, n, gs) in [(h, w, 5, (1, 2)) for (h, w) in STEM_SIZES] + [(360, 480, 7, (1,))]:
        for g in gs:
            add(stem_plan(n, h, w, 64, g)['kernel'], 'stem[%dx%d-g%d]' % (h, w, g))
            add('stem_pool_kernel_half', 'stem[%dx%d-g%d]' % (h, w, g))
            add('stem_pool_pack_kernel', 'stem[%dx%d-g%d]' % (h, w, g))
    for (n, h, w, cin, cout) in WINO2_CASES:
        name = 'wino2[%d-%d-%d-%d-%d]' % (n, h, w, cin, cout)
        for res in (False, True):
            add(wino2_kernel(h, w, res), name)
            add(wino2_kernel(h, w, res, sliced=True), name)
        if h >= 2 and w >= 2:
            add(wino2_kernel(h, w, pool=True), name)
    for (n, h, w, cin, cout) in WINO43_CASES:
        for res in (False, True):
            add(wino43_kernel(w, cin, res), 'wino43[%d-%d-%d-%d-%d]' % (n, h, w, cin, cout))
    return table


# ================================================================================================ LINEAR fusion sweep
# Shared by tests/test_ref64.py (CPU) and tests/test_gpu_rest_sweeps.py (the kernels).
LB_CANVASES = [(11, 11), (11, 64), (12, 65), (21, 21), (20, 130), (64, 64), (65, 63), (97, 129), (200, 300)]       # (hc, wc)
LB_PATTERNS = ['rects', 'inside', 'disjoint', 'one_pixel', 'symmetric', 'ones', 'half', 'last']
LB_VEC_ZERO = ('symmetric', 'ones')            # the centroids coincide on purpose: vec == 0 exactly, proj == 0
LB_NO_OVERLAP = ('disjoint',)


def _cover(n, a, b):
    """How much of pixel x (the interval x +- 0.5) lies in [a, b], x = 0 .. n - 1; a, b multiples of 1/64 -> multiples of 1/64."""
    x = np.arange(n, dtype=np.float64)
    return np.clip(np.minimum(x + 0.5, b) - np.maximum(x - 0.5, a), 0.0, 1.0)


def _rect(h, w, r0, r1, c0, c1):
    """A soft-edged rectangle: min of the row and the column coverage (a product would leave the 1/64 lattice)."""
    return np.minimum(_cover(h, r0, r1)[:, None], _cover(w, c0, c1)[None, :])


def _q(v):
    return np.floor(v) + 19.0 / 64.0            # a fractional border on the 1/64 lattice


def lb_masks(pattern, h, w):
    """-> (m1, m2) [h,w] float64 on the 1/64 lattice, see LB_PATTERNS / the issue's list."""
    one = np.ones((h, w))
    if pattern == 'rects':                      # two soft-edged rectangles with fractional borders that overlap
        return _rect(h, w, _q(0.08 * h), _q(0.86 * h), -1.0, _q(0.62 * w)), _rect(h, w, _q(0.2 * h), h + 1.0, _q(0.33 * w), _q(0.9 * w))
    if pattern == 'inside':                     # the target inside the reference, off its centre
        return _rect(h, w, -1.0, h + 1.0, -1.0, w + 1.0), _rect(h, w, _q(0.55 * h), _q(0.9 * h), _q(0.5 * w), _q(0.85 * w))
    if pattern == 'disjoint':                   # no overlap: the range keys are never written, om is never used
        return _rect(h, w, -1.0, _q(0.7 * h), -1.0, _q(0.35 * w)), _rect(h, w, _q(0.2 * h), h + 1.0, np.floor(0.35 * w) + 2.0, w + 1.0)
    if pattern == 'one_pixel':                  # binary rectangles that share one pixel: pmax == pmin, the denominator is the 1e-3
        r0, c0 = h // 2, w // 2
        m1, m2 = np.zeros((h, w)), np.zeros((h, w))
        m1[:r0 + 1, :c0 + 1] = 1.0
        m2[r0:, c0:] = 1.0
        return m1, m2
    if pattern == 'symmetric':                  # both symmetric about the canvas centre: vec == 0 exactly
        a, b = _q(0.1 * h) , _q(0.1 * w)
        c, d = _q(0.3 * h), _q(0.3 * w)
        return _rect(h, w, a, h - 1 - a, b, w - 1 - b), _rect(h, w, c, h - 1 - c, d, w - 1 - d)
    if pattern == 'ones':                       # the overlap touches all four borders, the reflect halo feeds every edge pixel
        return one, one.copy()
    if pattern == 'half':                       # m1 = 1, m2 = 0.5 around a block of ones: the product 0.5 rounds to 0 (half to even).
        m2 = np.full((h, w), 0.5)               # m2 = 0 on the left quarter moves its centroid right, so proj grows with the column and
        m2[h // 3:, w // 2 + 1:] = 1.0          # the 0.5 pixels left of the block lie BELOW the overlap's projection range: counted as
        m2[:, :w // 4] = 0.0                    # overlap (half rounded away from zero) they would stretch the range
        return one, m2
    if pattern == 'last':                       # the target's non-zero pixels are only in the last column and the last row
        m2 = np.zeros((h, w))
        m2[h - 1, :] = 1.0
        m2[:, w - 1] = 47.0 / 64.0
        m2[h - 1, w - 1] = 1.0
        return _rect(h, w, _q(0.15 * h), h + 1.0, _q(0.1 * w), w + 1.0), m2
    raise KeyError(pattern)


def lb_case(pattern, hc, wc, seed=0):
    """One LINEAR blender input -> (ref [3,hc,wc], tgt [3,hc,wc], m1 [hc,wc], m2 [hc,wc]) fp32: images uniform 0..255, masks from
    lb_masks.  Asserted here, for every case: the masks are multiples of 1/64 in [0, 1], so that m1 m2 (a multiple of 1/4096) and the
    union m1 + m2 - m1 m2 are exact in fp32 and round() takes the same branch in every precision; the index sums behind the
    centroids stay below 2^24, so that an fp32 `.float().mean()` IS the exact mean rounded once; |vec| >= 1 px unless the pattern
    makes it vanish, so that the cancellation in vec stays bounded; the overlap is what the pattern says."""
    rs = np.random.RandomState(13000 + seed + 131 * hc + 17 * wc + LB_PATTERNS.index(pattern))
    m1, m2 = lb_masks(pattern, hc, wc)
    for m in (m1, m2):
        assert m.shape == (hc, wc) and (m >= 0).all() and (m <= 1).all() and (m * 64 == np.round(m * 64)).all(), pattern
    assert np.array_equal((m1.astype(F32) * m2.astype(F32)).astype(np.float64), m1 * m2)
    un32 = m1.astype(F32) + m2.astype(F32) - m1.astype(F32) * m2.astype(F32)
    assert np.array_equal(un32.astype(np.float64), m1 + m2 - m1 * m2)
    for m in (m1, m2):
        assert max(np.nonzero(m)[0].sum(), np.nonzero(m)[1].sum()) < 2 ** 24
    ovl = np.round(m1 * m2)
    assert (ovl.sum() == 0) == (pattern in LB_NO_OVERLAP), (pattern, ovl.sum())
    if pattern == 'one_pixel':
        assert ovl.sum() == 1
    if pattern == 'half':
        assert ((m1 * m2) == 0.5).any() and (ovl[(m1 * m2) == 0.5] == 0).all()
    cen = [np.array([np.nonzero(m)[0].mean(), np.nonzero(m)[1].mean()]) for m in (m1, m2)]
    vec = cen[1].astype(F32).astype(np.float64) - cen[0].astype(F32).astype(np.float64)
    if pattern in LB_VEC_ZERO:
        assert (vec == 0).all(), (pattern, vec)
    else:
        assert np.hypot(*vec) >= 1.0, (pattern, hc, wc, vec)
    ref = rs.uniform(0, 255, (3, hc, wc)).astype(F32)
    tgt = rs.uniform(0, 255, (3, hc, wc)).astype(F32)
    return ref, tgt, m1.astype(F32), m2.astype(F32)


def lb_third(hc, wc, seed=0):
    """The third view of a chain: (w3 [3,hc,wc], m3 [hc,wc]) fp32, a soft rectangle over the lower right of the canvas (it overlaps
    the union of every pattern's pair) on the 1/64 lattice: the union of the first two is on the 1/4096 lattice and its product with
    m3 on the 2^-18 one, still exact in fp32."""
    rs = np.random.RandomState(14000 + seed + 131 * hc + 17 * wc)
    m3 = _rect(hc, wc, _q(0.35 * hc), hc + 1.0, _q(0.45 * wc), wc + 1.0)
    return rs.uniform(0, 255, (3, hc, wc)).astype(F32), m3.astype(F32)


LB_RENDER_CANVASES = [(40, 50), (11, 70), (97, 65), (80, 129)]      # hc < 64 and wc < 64; hc == 11; one row past the 96-row strip and
                                                                    # one column past a 64-column strip; one column past two strips
LB_RENDER_FRAME = (72, 96)


def lb_render_case(frames, views, hc, wc, off_canvas=None, seed=0):
    """Inputs of the fused LINEAR renderers: `frames` frames of `views` views of 72 x 96 (warp_case's textures, rounded to whole
    numbers so that the uint8 frames hold the same values) and hand-built splines -> (U [frames,views,3,72,96] fp32, source
    [frames,views,63,2] canvas-normalised, target [63,2]).  View v's frame is mapped onto a box of 0.62 x 0.7 of the canvas whose
    corner moves right and down with v (so that neighbouring views overlap in part, and the masks have fractional borders), with
    2 % jitter per control point and frame.  off_canvas: that view's box starts two canvas widths to the right -- nothing of it
    overlaps the others; its warped mask is all zero under FAST and holds the clamped sampler's rounding residue (blend_residue, a
    few 1e-5 at a few pixels) under NORMAL."""
    h, w = LB_RENDER_FRAME
    U, _, tgt = warp_case(frames * views, h, w, hc, wc, seed=20 + seed)
    rs = np.random.RandomState(15000 + seed + 131 * hc + 17 * wc + views)
    r = rigid_px(h, w)[0]                                                    # [7,9,2]
    src = np.empty((frames, views, 7, 9, 2), F32)
    for f in range(frames):
        for v in range(views):
            ox = (0.02, 0.33, 0.38)[v] * wc + (2.0 * wc if v == off_canvas else 0.0)
            oy = (0.05, 0.25, 0.28)[v] * hc
            src[f, v, ..., 0] = ox + r[..., 0] * (0.62 * wc / w) + rs.normal(0, 0.02 * wc, (7, 9))
            src[f, v, ..., 1] = oy + r[..., 1] * (0.70 * hc / h) + rs.normal(0, 0.02 * hc, (7, 9))
    U3 = np.rint(U[:, :3]).clip(0, 255).astype(F32).reshape(frames, views, 3, h, w)
    return U3, norm_px(src.reshape(frames * views, 7, 9, 2), hc, wc).reshape(frames, views, 63, 2), tgt[0]


# ================================================================================================ mesh geometry sweep
GEOM_BATCHES = [1, 63, 64, 65, 300]            # one item per thread in 64-thread blocks, or one block per item
GEOM_SIZES = [(360, 480), (720, 1280)]


def geom_offsets(n, kind, img_h, img_w, seed=0):
    """offset8 [n,8] fp32: 'zero' (the identity), 'mild' (up to 8 % of the frame, the size the regressor produces), 'large' (every
    corner pulled 40 % of the way to the centre and jittered by 5 %: a quad of about a quarter of the area, near collapse for a
    DLT but still convex)."""
    rs = np.random.RandomState(21000 + seed + n + img_h + {'zero': 0, 'mild': 1, 'large': 2}[kind])
    size = np.array([img_w, img_h], np.float64)
    if kind == 'zero':
        return np.zeros((n, 8), F32)
    if kind == 'mild':
        return (rs.uniform(-0.08, 0.08, (n, 4, 2)) * size).reshape(n, 8).astype(F32)
    c = np.array([[0.0, 0.0], [img_w, 0.0], [0.0, img_h], [img_w, img_h]])
    m = 0.4 * (size / 2 - c)[None] + rs.uniform(-0.05, 0.05, (n, 4, 2)) * size
    q = c[None] + m                                                          # still convex: the corners keep their cyclic order
    for a, b, d in ((0, 1, 3), (1, 3, 2), (3, 2, 0), (2, 0, 1)):
        e1, e2 = q[:, b] - q[:, a], q[:, d] - q[:, b]
        assert (e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0] > 0).all()
    return m.reshape(n, 8).astype(F32)


def geom_residuals(n, seed=0):
    """(off_ref, off_tgt) [n,126] fp32: the second stage's per-vertex residuals, N(0, 3 px)"""
    rs = np.random.RandomState(22000 + seed + n)
    return rs.normal(0, 3.0, (n, 126)).astype(F32), rs.normal(0, 3.0, (n, 126)).astype(F32)


# ================================================================================================ SmoothNet glue, windows, canvas normalisation, watcher
# Shared by tests/test_ref64.py (CPU: the fp32 reading of each statement inside half of its gate on these very cases) and
# tests/test_gpu_rest_sweeps.py (the kernels).
def corner_points(n, img_h, img_w):
    return np.repeat(np.array([[0.0, 0.0], [img_w, 0.0], [0.0, img_h], [img_w, img_h]], F32)[None], n, 0)




def smooth_case(nw, t, wstride, seed=0):
    """smesh1/2, tsmotion1/2 [n,63,2] of pipeline-like size (LR meshes around the rigid grid, ~2 px motions), delta [nw,t,63,4],
    the two embeddings' weights [32,2] and biases [32]; n = (nw - 1) wstride + t frames"""
    n = (nw - 1) * wstride + t
    rs = np.random.RandomState(24000 + seed + 7 * nw + 131 * t + wstride)
    rigid = rigid_px(360, 480).reshape(1, 63, 2)
    sm = [(rigid + rs.normal(0, 4.0, (n, 63, 2))).astype(F32) for _ in range(2)]
    ts = [rs.normal(0, 2.0, (n, 63, 2)).astype(F32) for _ in range(2)]
    delta = rs.normal(0, 1.5, (nw, t, 63, 4)).astype(F32)
    emb = [rs.normal(0, 0.5, s).astype(F32) for s in ((32, 2), (32,), (32, 2), (32,))]
    return sm, ts, delta, emb


SMOOTH_SHAPES = [(nw, t, ws) for t in (2, 7) for nw in (1, 2, 30, 300) for ws in (1, t)]




def ring_case(rings, w, e, k, seed=0):
    rs = np.random.RandomState(25000 + seed + rings + 7 * w + 131 * e + k)
    return rs.normal(0, 1, (rings, w, e)).astype(F32), rs.normal(0, 1, (rings, k, e)).astype(F32)


WINDOW_SHAPES = [(2, 2048), (2049, 1), (7, 126), (7, 255), (7, 256), (7, 257), (2, 1), (5, 512), (8, 292)]      # (W, E): (W - 1) E <= 2048




def norm_case(frames, views, seed=0):
    """LR meshes [views][frames,63,2] around the rigid 360 x 480 grid, shifted per view, and canvas boxes in HR pixels of a 720 x 1280
    frame: one box, and one per frame"""
    rs = np.random.RandomState(26000 + seed + frames + 7 * views)
    rigid = rigid_px(360, 480).reshape(1, 63, 2)
    meshes = [(rigid + rs.normal(0, 9.0, (frames, 63, 2)) + [110.0 * v, 7.0 * v]).astype(F32) for v in range(views)]
    box = np.array([-31.7, 1893.2, -44.1, 801.6], F32)
    boxes = (box[None] + rs.uniform(-20, 20, (frames, 4))).astype(F32)
    return meshes, box, boxes


def watch_frames():
    """Seven frames [7,2,63,2] of two views inside the canvas, each with one point moved: exactly on +-1; exactly on -(1 + slack) and on +(1 + slack)
    (inside) and one fp32 step beyond (outside); exactly on the guard distance 1 - 0.02 (not near) and one step beyond (near); a NaN in
    lane 37 of the second view.  Frames 0 .. 2 are inside: the first clipped frame is frame 3."""
    rs = np.random.RandomState(27000)
    f = rs.uniform(-0.9, 0.9, (7, 2, 63, 2)).astype(F32)
    one, slack, g = F32(1.0), WATCH_SLACK, F32(0.02)
    edge = one + slack
    near = one - g
    f[0, 0, 5] = [1.0, -1.0]
    f[1, 1, 62] = [-edge, 0.0]
    f[1, 0, 10] = [edge, 0.0]
    f[2, 0, 17, 1] = near
    f[3, 1, 40, 0] = np.nextafter(edge, F32(2.0))
    f[4, 0, 63 - 1, 1] = np.nextafter(near, F32(2.0))
    f[5, 1, 37, 1] = np.nan
    f[6, 0, 0, 1] = -np.nextafter(edge, F32(2.0))
    return f


def three_view_case(frames):
    """The four LR meshes of a three-view alignment [4][frames,63,2] (w12_m1, w12_m2, w23_m1, w23_m2: the pair (2, 3)'s first mesh is
    the pair (1, 2)'s second moved by 3.3 px) and the first canvas' box"""
    meshes, box, _ = norm_case(frames, 3, seed=3)
    return [meshes[0], meshes[1], (meshes[1] + F32(3.3)).astype(F32), meshes[2]], box


NORM_FRAMES = [1, 7, 300]
NORM_SIZES = [(720, 1280), (0, 0)]             # scaled from LR, and HR already (img_h = img_w = 0)
STITCH_SHAPES = [(1, 2), (1, 7), (2, 2), (2, 7), (30, 2), (30, 7), (300, 2), (300, 7)]       # (nw, t)


# ================================================================================================ the coverage table of the library
KS, CS, RS_ = 'test_gpu_kernel_sweeps', 'test_gpu_conv_sweeps', 'test_gpu_rest_sweeps'
SS, NV, EX, VP = 'test_gpu_stream_sweeps', 'test_gpu_nv12', 'test_gpu_exposure', 'test_gpu_viewport'
MB, SM = 'test_gpu_multiband', 'test_gpu_seam'
SWEEP_MODULES = (KS, CS, RS_, SS, NV, EX, VP, MB, SM)      # the modules whose kernel-level tests compare with numpy or a float64 statement
LB_CHAIN = ('lb_init_kernel', 'lb_centroid_kernel', 'lb_range_kernel', 'lb_premask_kernel', 'lb_blur_kernel', 'lb_final_kernel')

# Short names of the overloads' keys: alias -> the key overload_key() gives, base name + the parameter list of the code object.  The
# table below is written with the aliases; tests/test_ref64.py takes the parameter lists from the code objects and never from here,
# so an alias that matches no kernel of the library shows as a stale row.
_AVG = 'float const*, float const*, float const*, float*, int, int, int, int, int, long long, long long, long long'
_CLIP = 'float const*, float const*, float*, unsigned int*, int, int, int, int, int, long long'
_FRAMES = 'float const*, float const*, float*, unsigned int*, int, int, int, long long, LbFrameTab'
_LATTICE = 'float const*, float const*, float*, long long, int, int, int, int, int, float, int*, float*'
OVERLOAD_ALIASES = {
    'render_average_kernel(RenderViews)': 'render_average_kernel(RenderViews, %s)' % _AVG,
    'render_average_kernel(GainViews)': 'render_average_kernel(GainViews, %s)' % _AVG,
    'render_average_kernel(Nv12Views)': 'render_average_kernel(Nv12Views, float const*, float const*, float const*, unsigned char*, '
                                        'unsigned char*, int, int, int, int, int, int, long long, long long)',
    'lb_clip_warp_kernel(RenderViews)': 'lb_clip_warp_kernel(RenderViews, %s)' % _CLIP,
    'lb_clip_warp_kernel(GainViews)': 'lb_clip_warp_kernel(GainViews, %s)' % _CLIP,
    'lb_frames_warp_kernel(RenderViews)': 'lb_frames_warp_kernel(RenderViews, %s)' % _FRAMES,
    'lb_frames_warp_kernel(GainViews)': 'lb_frames_warp_kernel(GainViews, %s)' % _FRAMES,
    'lb_frames_warp_kernel(Nv12Views)': 'lb_frames_warp_kernel(Nv12Views, float const*, float const*, float*, unsigned int*, int, int, '
                                        'int, LbFrameTab)',
    'render_lattice_kernel(footprint)': 'render_lattice_kernel(%s)' % _LATTICE,
    'render_lattice_kernel(footprint, SsCanvasFit)': 'render_lattice_kernel(%s, SsCanvasFit)' % _LATTICE,
    'canvas_watch_kernel(watch)': 'canvas_watch_kernel(float const*, int, float, int*, float*)',
    'canvas_watch_kernel(watch, SsCanvasFit)': 'canvas_watch_kernel(float const*, int, float, int*, float*, SsCanvasFit)',
    'canvas_watch_frames_kernel(watch)': 'canvas_watch_frames_kernel(float const*, int, int, float, int*, float*)',
    'canvas_watch_frames_kernel(watch, SsCanvasFit)': 'canvas_watch_frames_kernel(float const*, int, int, float, int*, float*, SsCanvasFit)',
    'ingest_hr1_kernel(bgr)': 'ingest_hr1_kernel(unsigned char const*, float*, long long, int)',
    'ingest_hr1_kernel(y, uv)': 'ingest_hr1_kernel(unsigned char const*, unsigned char const*, int, long long, float*, int, int)',
    'ingest_lr_kernel(bgr)': 'ingest_lr_kernel(unsigned char const*, float*, int, int, int, int, int, double, double)',
    'ingest_lr_kernel(y, uv)': 'ingest_lr_kernel(unsigned char const*, unsigned char const*, int, long long, float*, int, int, int, int, '
                               'double, double)',
    'canvas_u8x1_kernel(fp32)': 'canvas_u8x1_kernel(float const*, unsigned char*, long long, int)',
}
AVG, AVG_GAINS, AVG_NV12 = ('render_average_kernel(%s)' % v for v in ('RenderViews', 'GainViews', 'Nv12Views'))
CAST1 = 'canvas_u8x1_kernel(fp32)'
BGR_TO_NV12 = 'canvas_u8x1_kernel(unsigned char const*, unsigned char*, unsigned char*, int, long long, int, int)'
EXPOSURE = 'render_lattice_kernel(ExposureArgs)'


def library_reach():
    """Every kernel of the built library by its overload key (overload_key above) -> (kind, tests, held_to).  The key is the base
    name where the library carries one parameter list under it, and base name + parameter list where it carries several: kernels
    added as overloads of an existing name (the exposure estimator under the footprint sampler's, BGR -> NV12 under the byte cast's,
    the NV12, gain and refit forms of the renders and watchers) have rows of their own.  All template instantiations of one
    parameter list share an entry (the convolution engine's are told apart by reach_table above); rows are written with the short
    names of OVERLOAD_ALIASES and returned under the full keys.
      'fp64'      the sweep tests that compare it with a statement of tests/ref64.py or tests/exposure_ref.py
      'identity'  the test that holds it bit for bit to the kernels `held_to`, every one of them 'fp64', 'exact' or 'identity' in turn
      'exact'     copy, permute, byte and min / max kernels: the test that holds them bit for bit to numpy
    Kernels that no call of the C ABI launches are in UNREACHABLE.  tests/test_ref64.py holds the table to the code objects of the
    built library (nothing missing, nothing stale, the parameter lists taken from the demangled names), follows every identity
    chain to an 'fp64' or 'exact' end and checks that the cited tests exist."""
    t = {}
    full = lambda n: OVERLOAD_ALIASES.get(n, n)

    def add(kind, names, tests, held_to=()):
        for n in (names.split() if isinstance(names, str) else names):      # (a list where a key holds blanks)
            assert full(n) not in t, n
            t[full(n)] = (kind, tuple(tests), tuple(full(k) for k in held_to))
    # ---- the two earlier sweeps
    add('fp64', 'cost_volume_kernel', [KS + '::test_cost_volume_against_fp64', KS + '::test_cost_volume_shifted_and_chain_against_fp64'])
    add('fp64', 'ccl_softmax_kernel', [KS + '::test_ccl_against_fp64'])
    add('fp64', 'l2norm_kernel', [KS + '::test_l2norm_against_fp64', KS + '::test_ccl_against_fp64'])
    add('fp64', 'homo_warp_kernel', [KS + '::test_homography_against_fp64'])
    add('fp64', 'tps_solve_kernel tps_inverse_kernel', [KS + '::test_tps_solve_by_its_action'])
    add('fp64', 'tps_points_kernel', [KS + '::test_tps_points_against_fp64'])
    add('fp64', 'tsm_prepare_kernel tsm_finish_kernel tsm_fused_kernel', [KS + '::test_tsmotion_against_fp64'])
    add('fp64', 'tps_warp_kernel', [KS + '::test_tps_dense_warp_against_fp64'])
    add('fp64', 'tps_warp_views_kernel', [KS + '::test_tps_warp_views_against_fp64'])
    add('identity', [AVG], [KS + '::test_fused_render_equals_formula_on_per_view_warps'], ['tps_warp_kernel', CAST1, 'canvas_u8x4_kernel'])
    add('identity', ['render_lattice_kernel(footprint)', 'render_order_kernel'], ['test_gpu_parity::test_render_footprint_skipping'], [AVG])
    add('fp64', 'psnr_ssim_kernel psnr_ssim_finish_kernel', [KS + '::test_psnr_ssim_against_fp64'])
    add('fp64', 'stability_kernel distortion_kernel max_reduce_kernel', [KS + '::test_metric_scores_against_fp64_and_refusals'])
    add('fp64', 'linear_kernel linear_grouped_kernel', [KS + '::test_linear_against_fp64'])
    add('exact', 'maxpool_kernel', [KS + '::test_maxpool_split_bit_exact'])
    add('fp64', 'conv_igemm_kernel splitk_reduce_kernel', [CS + '::test_implicit_gemm_against_fp64', CS + '::test_conv_pool_in_reduce_against_fp64'])
    add('fp64', 'stem_pool_kernel_half stem_pool_pack_kernel nchw_to_nhwc3_padded_kernel', [CS + '::test_stem_against_fp64'])
    add('fp64', 'conv_wino_kernel wino_pack_kernel wino_pack3_kernel', [CS + '::test_winograd_f2_against_fp64'])
    add('fp64', 'conv_wino43p_kernel wino43_pack_kernel', [CS + '::test_winograd_f4_against_fp64'])
    # ---- LINEAR fusion
    add('fp64', ' '.join(LB_CHAIN), [RS_ + '::test_linear_blend_against_fp64', RS_ + '::test_linear_blend_three_view_chain_against_fp64'])
    add('identity', ['lb_clip_warp_kernel(RenderViews)', 'lb_clip_reduce_kernel', 'lb_clip_blend_kernel', 'lb_clip_blend_rows_kernel',
                     'lb_frames_warp_kernel(RenderViews)', 'lb_frames_reduce_kernel', 'lb_frames_blend_rows_kernel'],
        [RS_ + '::test_linear_renderers_equal_per_frame_chain'],
        LB_CHAIN + ('tps_warp_views_kernel', 'mask_union_kernel', CAST1, 'canvas_u8x4_kernel'))
    # ---- mesh geometry
    add('fp64', 'tensor_dlt_kernel spatial_decompose_kernel spatial_meshes_kernel', [RS_ + '::test_dlt_decompose_meshes_against_fp64'])
    add('fp64', 'h2mesh_kernel', [RS_ + '::test_h2mesh_against_fp64'])
    add('exact', 'mesh_bbox_kernel', [RS_ + '::test_mesh_bbox_bit_exact'])
    add('fp64', 'mesh_normalize_kernel mesh_normalize_views_kernel stream_normalize_watch_kernel', [RS_ + '::test_canvas_normalize_kernels_bit_exact'])
    add('fp64', 'three_view_align_kernel three_view_normalize_kernel three_view_finish_kernel', [RS_ + '::test_three_view_glue_kernels'])
    add('exact', ['canvas_watch_kernel(watch)', 'canvas_watch_frames_kernel(watch)'], [RS_ + '::test_canvas_watchers_against_the_documented_update'])
    add('identity', 'three_view_splines_kernel', ['test_gpu_round6::test_three_view_splines_equal_the_seven_launches'],
        ['three_view_align_kernel', 'three_view_normalize_kernel', 'tps_solve_kernel', 'tps_points_kernel', 'three_view_finish_kernel',
         'stream_normalize_watch_kernel'])
    add('identity', 'stream_splines_kernel', ['test_gpu_round6::test_stream_splines_equal_normalise_plus_solve'],
        ['stream_normalize_watch_kernel', 'mesh_normalize_views_kernel', 'tps_solve_kernel'])
    # ---- SmoothNet glue, streaming windows
    add('fp64', 'smooth_embed_kernel smooth_finalize_kernel', [RS_ + '::test_smooth_embed_and_finalize'])
    add('fp64', 'smooth_stitch_kernel smooth_path_chain_kernel', [RS_ + '::test_smooth_stitch_against_frame_loop'])
    add('exact', 'window_push_kernel', [RS_ + '::test_window_push_bit_exact'])
    add('exact', 'window_advance_kernel', [RS_ + '::test_window_advance_bit_exact'])
    # ---- byte and layout kernels
    add('exact', ['ingest_hr4_kernel', 'ingest_hr1_kernel(bgr)', 'ingest_lr_kernel(bgr)'], [RS_ + '::test_ingest_u8_paths_bit_exact'])
    add('exact', ['canvas_u8x4_kernel', CAST1], [RS_ + '::test_canvas_to_u8_paths_and_edge_values'])
    add('exact', 'nchw_to_nhwc_kernel nchw_to_nhwc4_kernel nhwc_to_nchw_kernel', [RS_ + '::test_layout_kernels_bit_exact'])
    add('exact', 'affine_kernel mask_union_kernel fill_kernel', [RS_ + '::test_elementwise_helpers_bit_exact'])
    # ---- the overloads of the streaming features: viewport refit, NV12 in and out, exposure gains
    add('exact', ['canvas_watch_kernel(watch, SsCanvasFit)', 'canvas_watch_frames_kernel(watch, SsCanvasFit)',
                  'render_lattice_kernel(footprint, SsCanvasFit)'], [VP + '::test_fit_kernels_equal_the_restatement_bit_for_bit'])
    add('exact', ['ingest_hr1_kernel(y, uv)', 'ingest_lr_kernel(y, uv)'], [SS + '::test_ingest_nv12_paths_bit_exact'])
    add('exact', [BGR_TO_NV12], [NV + '::test_bgr_to_nv12_equals_numpy', SS + '::test_bgr_to_nv12_into_strided_frames'])
    add('fp64', [EXPOSURE], [EX + '::test_statistics_targets_and_smoothing', SS + '::test_exposure_beyond_one_wave_and_one_trip'])
    add('identity', [AVG_NV12], [NV + '::test_render_average_nv12_equals_the_u8_render_and_its_nv12',
                                 SS + '::test_render_average_nv12_at_the_tile_edges'], [AVG, BGR_TO_NV12])
    add('identity', ['lb_frames_warp_kernel(Nv12Views)'], [NV + '::test_render_linear_frames_nv12_equals_the_u8_render'],
        ['lb_frames_warp_kernel(RenderViews)'])
    gains = [EX + '::test_gain_renders_reduce_to_the_plain_renders', EX + '::test_general_gains_equal_the_per_frame_chains']
    add('identity', [AVG_GAINS], gains, [AVG, 'tps_warp_kernel', CAST1, 'canvas_u8x4_kernel'])
    add('identity', ['lb_clip_warp_kernel(GainViews)'], gains, ['lb_clip_warp_kernel(RenderViews)', 'tps_warp_views_kernel'])
    add('identity', ['lb_frames_warp_kernel(GainViews)'], gains, ['lb_frames_warp_kernel(RenderViews)', 'tps_warp_views_kernel'])
    return t


# ================================================================================================ the blend and the seam libraries
def instantiation_key(name):
    """A demangled kernel name of libstabstitch_blend.so / libstabstitch_seam.so -> 'base<a,b,...>' as kernel_key writes it (booleans
    as 0 / 1), the anonymous namespace dropped.  These two libraries are keyed by instantiation: there are 15 + 6 of them."""
    return kernel_key(name.replace('(anonymous namespace)::', ''))


def blend_reach():
    """Every kernel instantiation of libstabstitch_blend.so -> (kind, tests), as library_reach: 'fp64' the tests that hold it to the
    float64 statement of tests/multiband_ref.py inside its bound, 'exact' the tests that hold the uint8 output bit for bit to numpy's
    cast of the fp32 output (which the same tests hold to float64).  mb_collapse_kernel<V, COARSE, OUT>: COARSE = 0 is the top level
    of the pyramid; OUT = 0 writes a level (so <V,0,0> needs a band, <V,1,0> two), 1 the fp32 frame, 2 the uint8 frame -- with
    COARSE = 0 at bands = 0 only.  tests/test_ref64.py holds the table to the code objects, test_gpu_multiband's launch witness to what
    the smallest calls launch."""
    t = {}
    fp64 = [MB + '::test_blend_of_real_warps_against_fp64', MB + '::test_blend_of_made_up_masks_against_fp64',
            MB + '::test_blend_of_small_canvases_against_fp64', MB + '::test_several_frames_in_one_call_against_fp64',
            MB + '::test_tied_weights_go_to_the_lowest_view']
    u8 = [MB + '::test_blend_of_small_canvases_against_fp64', MB + '::test_several_frames_in_one_call_against_fp64']
    t['mb_reduce_kernel'] = ('fp64', tuple(fp64))
    for v in (2, 3):
        t['mb_prepare_kernel<%d>' % v] = ('fp64', tuple(fp64))
        for coarse in (0, 1):
            t['mb_collapse_kernel<%d,%d,0>' % (v, coarse)] = ('fp64', tuple(fp64))
            t['mb_collapse_kernel<%d,%d,1>' % (v, coarse)] = ('fp64', tuple(fp64))
            t['mb_collapse_kernel<%d,%d,2>' % (v, coarse)] = ('exact', tuple(u8))
    return t


def seam_reach():
    """Every kernel instantiation of libstabstitch_seam.so -> ('exact', tests): the tests that hold it bit for bit to the integer
    restatement of tests/seam_ref.py."""
    tests = tuple(SM + '::' + n for n in (
        'test_kernels_equal_the_restatement', 'test_kernels_equal_the_restatement_over_several_tile_columns',
        'test_made_up_scenes_on_the_device', 'test_made_up_scenes_on_either_side_of_a_tile_boundary',
        'test_grids_of_more_than_256_rows_of_cells', 'test_the_cap_on_M', 'test_an_unaligned_P_takes_the_scalar_loads'))
    three = tuple(SM + '::' + n for n in (
        'test_kernels_equal_the_restatement', 'test_kernels_equal_the_restatement_over_several_tile_columns',
        'test_view_order_follows_the_extents_on_the_device', 'test_an_unaligned_P_takes_the_scalar_loads'))
    return {'%s<%d>' % (k, v): ('exact', tests if v == 2 else three) for k in ('sm_cost_kernel', 'sm_dp_kernel', 'sm_paint_kernel')
            for v in (2, 3)}
