"""Seeded inputs and gate constructions of the kernel sweeps, shared by tests/test_ref64.py (CPU: the fp32 oracle against
tests/ref64.py on these very inputs, under these very gates) and tests/test_gpu_kernel_sweeps.py / tests/test_gpu_conv_sweeps.py
(the kernels).  The float64 statements themselves are in tests/ref64.py and do not depend on anything here.  The second half
holds the convolution sweep: its cases, the dispatch rules of the convolution engine restated (which kernel a shape takes), an fp32
emulation of both Winograd forms, and the reach table from kernel instantiation to the cases claimed to launch it."""
import numpy as np

from ref64 import F32, f64, dot_bound, linspace, bilinear_clamped, grid_sample_zeros, homography_coords

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
