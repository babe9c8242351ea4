"""Seeded inputs and gate constructions of the kernel sweeps, shared by tests/test_ref64.py (CPU: the fp32 oracle against
tests/ref64.py on these very inputs, under these very gates) and tests/test_gpu_kernel_sweeps.py (the kernels).  The float64
statements themselves are in tests/ref64.py and do not depend on anything here."""
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
