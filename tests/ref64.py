"""Plain float64 statements of the operations of the hot path, one function per operation.

Written from the definitions in oracle/ (nets.py cost volume, CCL and the layers' nn.Conv2d / nn.Conv3d, samplers.py, metrics.py,
pipeline.py), Lavin & Gray 2015 for the Winograd forms and the comments
of include/stabstitch_hip.h; numpy only, no tiling, no tricks -- loops over displacements and taps.  Every function takes
what the kernel takes (fp32 values, promoted here) and returns, beside the value, what the caller's tolerance needs (the sum
of the absolute products of a dot product, the denominator of a projective map).

Where the reference algorithm rounds on purpose the statement keeps that rounding and raises only the rest: the TPS system
is ASSEMBLED in fp32 and solved in fp64 (oracle.samplers.tps_solve), psnr_ssim rounds plane * mask to fp32 first.

tests/test_ref64.py pins each of these against the golden fixture of its operation and against the fp32 oracle.  The sweeps'
seeded inputs and the construction of their gates are in tests/sweep_inputs.py; nothing here knows the kernels or the oracle."""
import numpy as np

F32 = np.float32
U24 = 2.0 ** -24            # unit roundoff of fp32


def f64(x):
    if hasattr(x, 'detach'):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=np.float64)


def f32(x):
    if hasattr(x, 'detach'):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=F32)


def dot_bound(k, s, extra=4):
    """Forward bound of an fp32 sum of k products in ANY order, s = sum of the absolute products: (k + extra) u s, u = 2^-24
    (|fl(x . y) - x . y| <= gamma_k |x| . |y|; the 1.01 is gamma_k's 1 / (1 - k u) for k u < 0.01).  `extra` roundings follow
    the sum (a division, a leaky-ReLU multiply, a final store)."""
    assert np.all(np.asarray(k) * U24 < 0.01)
    return (1.01 * k + extra) * U24 * s


# ------------------------------------------------------------------------------------------------ correlation
def cost_volume(x1, x2, r):
    """x1, x2 [n,c,h,w] -> (cv [n,(2r+1)^2,h,w], S [n,(2r+1)^2,h,w]): cv[j*K+i, y, x] = leaky_relu_0.1(mean_c x1[c,y,x] *
    x2[c,y+j-r,x+i-r]), zero outside; S = (sum_c |x1 x2|) / c, the scale of the derived tolerance."""
    x1, x2 = f64(x1), f64(x2)
    n, c, h, w = x1.shape
    k = 2 * r + 1
    x2p = np.zeros((n, c, h + 2 * r, w + 2 * r))
    x2p[:, :, r:r + h, r:r + w] = x2
    cv = np.empty((n, k * k, h, w))
    s = np.empty((n, k * k, h, w))
    for j in range(k):
        for i in range(k):
            prod = x1 * x2p[:, :, j:j + h, i:i + w]
            m = prod.sum(axis=1) / c
            cv[:, j * k + i] = np.where(m > 0, m, 0.1 * m)
            s[:, j * k + i] = np.abs(prod).sum(axis=1) / c
    return cv, s


def l2norm(x, axis):
    """F.normalize(x, p=2, dim=axis): x / max(||x||_2, 1e-12)."""
    x = f64(x)
    return x / np.maximum(np.sqrt((x * x).sum(axis=axis, keepdims=True)), 1e-12)


def ccl(f1, f2, scale=10.0):
    """Contextual correlation layer, f1, f2 [n,c,h,w] -> flow [n,2,h,w] (ch0 = dx, ch1 = dy): L2-normalise over channels, correlate
    the (zero padded) 3 x 3 patch of n2 around k with the patch of n1 around p, softmax(scale x) over k, expected (k - p)."""
    n1, n2 = l2norm(f1, 1), l2norm(f2, 1)
    n, c, h, w = n1.shape
    P = h * w
    out = np.empty((n, 2, h, w))
    ky, kx = np.divmod(np.arange(P), w)
    for b in range(n):
        a = np.zeros((c, h + 2, w + 2))
        a[:, 1:-1, 1:-1] = n1[b]
        d = np.zeros((c, h + 2, w + 2))
        d[:, 1:-1, 1:-1] = n2[b]
        match = np.zeros((P, P))                                   # [k, p]
        for dy in range(3):
            for dx in range(3):
                pa = a[:, dy:dy + h, dx:dx + w].reshape(c, P)
                pk = d[:, dy:dy + h, dx:dx + w].reshape(c, P)
                match += pk.T @ pa
        z = match * scale
        z -= z.max(axis=0, keepdims=True)
        e = np.exp(z)
        prob = e / e.sum(axis=0, keepdims=True)
        fy = (prob * (ky[:, None] - ky[None, :])).sum(axis=0)
        fx = (prob * (kx[:, None] - kx[None, :])).sum(axis=0)
        out[b, 0] = fx.reshape(h, w)
        out[b, 1] = fy.reshape(h, w)
    return out


# ------------------------------------------------------------------------------------------------ samplers
def linspace(n):
    """torch.linspace(-1, 1, n) as fp32 VALUES (the grid the kernels and the oracle share), promoted to fp64."""
    import torch
    return torch.linspace(-1.0, 1.0, n).numpy().astype(np.float64)


def homography_coords(theta, out_h, out_w):
    """theta [n,3,3] (fp32 values) -> (xn, yn, ts) [n,out_h,out_w]: the projective map of the normalised grid with the
    reference's guard, ts += 1e-6 where |ts| < 1e-7.  `ts` is returned BEFORE the guard (the caller's conditioning)."""
    th = f64(theta).reshape(-1, 3, 3)
    gx = linspace(out_w)[None, None, :]
    gy = linspace(out_h)[None, :, None]
    t = [th[:, k, 0, None, None] * gx + th[:, k, 1, None, None] * gy + th[:, k, 2, None, None] for k in range(3)]
    ts = t[2] + 1e-6 * (np.abs(t[2]) < 1e-7)
    return t[0] / ts, t[1] / ts, t[2]


def bilinear_clamped(img, xn, yn, absum=False):
    """The reference's clamped-index bilinear gather: img [n,c,h,w]; xn, yn [n,...] normalised, x = (xn + 1) w / 2.  Indices are
    clamped to the image and the CLAMPED values enter the weights -> [n,c,...].  absum: also the sum of the four |weight x value|:
    outside the image the four products cancel exactly in exact arithmetic (two clamped taps coincide, their weights are opposite)
    but are each of the size of (distance to the image)^2 x value, and what an fp32 sum of them returns is rounding residue of
    THAT size -- the scale of the derived bound dot_bound(4, .) of the blend."""
    img = f64(img)
    n, c, h, w = img.shape
    x = (f64(xn) + 1.0) * w / 2.0
    y = (f64(yn) + 1.0) * h / 2.0
    x0 = np.floor(np.clip(x, -4.0, w + 4.0)).astype(np.int64)
    y0 = np.floor(np.clip(y, -4.0, h + 4.0)).astype(np.int64)
    x1, y1 = x0 + 1, y0 + 1
    x0, x1 = np.clip(x0, 0, w - 1), np.clip(x1, 0, w - 1)
    y0, y1 = np.clip(y0, 0, h - 1), np.clip(y1, 0, h - 1)
    bi = np.arange(n).reshape((n,) + (1,) * (x.ndim - 1))
    out = np.empty((n, c) + x.shape[1:])
    s = np.empty_like(out) if absum else None
    for ch in range(c):
        pl = img[:, ch]
        terms = ((x1 - x) * (y1 - y) * pl[bi, y0, x0], (x1 - x) * (y - y0) * pl[bi, y1, x0],
                 (x - x0) * (y1 - y) * pl[bi, y0, x1], (x - x0) * (y - y0) * pl[bi, y1, x1])
        out[:, ch] = terms[0] + terms[1] + terms[2] + terms[3]
        if absum:
            s[:, ch] = np.abs(terms[0]) + np.abs(terms[1]) + np.abs(terms[2]) + np.abs(terms[3])
    return (out, s) if absum else out


def grid_sample_zeros(img, xn, yn):
    """F.grid_sample(bilinear, padding zeros, align_corners=True): x = (xn + 1) / 2 (w - 1), out-of-range taps contribute 0."""
    img = f64(img)
    n, c, h, w = img.shape
    x = (f64(xn) + 1.0) / 2.0 * (w - 1)
    y = (f64(yn) + 1.0) / 2.0 * (h - 1)
    x0 = np.floor(np.clip(x, -4.0, w + 4.0)).astype(np.int64)
    y0 = np.floor(np.clip(y, -4.0, h + 4.0)).astype(np.int64)
    bi = np.arange(n).reshape((n,) + (1,) * (x.ndim - 1))
    out = np.zeros((n, c) + x.shape[1:])
    for (xx, yy, wt) in ((x0, y0, (x0 + 1 - x) * (y0 + 1 - y)), (x0 + 1, y0, (x - x0) * (y0 + 1 - y)),
                         (x0, y0 + 1, (x0 + 1 - x) * (y - y0)), (x0 + 1, y0 + 1, (x - x0) * (y - y0))):
        ok = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
        xc, yc = np.clip(xx, 0, w - 1), np.clip(yy, 0, h - 1)
        for ch in range(c):
            out[:, ch] += np.where(ok, wt * img[:, ch][bi, yc, xc], 0.0)
    return out


def homography_warp(img, theta, out_h, out_w):
    xn, yn, _ = homography_coords(theta, out_h, out_w)
    return bilinear_clamped(img, xn, yn)


# ------------------------------------------------------------------------------------------------ thin-plate spline
def tps_system(source):
    """source [n,63,2] -> W [n,66,66] (fp64 holding fp32 values): [[P, R], [0, P^T]], P = [1, Sx, Sy], R_ij = d2 log(d2 + 1e-6),
    assembled in fp32 -- the reference's rounding, which the kernels reproduce."""
    s = f32(source)
    n, m, _ = s.shape
    p = np.concatenate((np.ones((n, m, 1), F32), s), axis=2)
    diff = p[:, :, None, :] - p[:, None, :, :]
    d2 = (diff * diff).sum(axis=3, dtype=F32)
    rb = (d2 * np.log(d2 + F32(1e-6), dtype=F32)).astype(F32)
    W = np.zeros((n, m + 3, m + 3))
    W[:, :m, :3] = p
    W[:, :m, 3:] = rb
    W[:, m:, 3:] = p.transpose(0, 2, 1)
    return W


def tps_rhs(target):
    t = f64(target)
    rhs = np.zeros((t.shape[0], t.shape[1] + 3, 2))
    rhs[:, :t.shape[1]] = t
    return rhs


def tps_solve(source, target):
    """source, target [n,63,2] -> T [n,2,66] in fp64: the fp32-assembled system (tps_system) solved in fp64."""
    return np.linalg.solve(tps_system(source), tps_rhs(target)).transpose(0, 2, 1)


def tps_eval(T, source, xq, yq):
    """T [n,2,66], source [n,63,2], xq / yq [n,Q] or [Q] -> (xs, ys) [n,Q]: T . [1, x, y, r_1 .. r_63], r = d2 log(d2 + 1e-6)."""
    T, s = f64(T), f64(source)
    n = s.shape[0]
    xq = np.broadcast_to(f64(xq), (n,) + np.shape(xq)[-1:])
    yq = np.broadcast_to(f64(yq), (n,) + np.shape(yq)[-1:])
    xs = T[:, 0, 0, None] + T[:, 0, 1, None] * xq + T[:, 0, 2, None] * yq
    ys = T[:, 1, 0, None] + T[:, 1, 1, None] * xq + T[:, 1, 2, None] * yq
    for k in range(s.shape[1]):
        dx = xq - s[:, k, 0, None]
        dy = yq - s[:, k, 1, None]
        d2 = dx * dx + dy * dy
        rb = d2 * np.log(d2 + 1e-6)
        xs = xs + T[:, 0, 3 + k, None] * rb
        ys = ys + T[:, 1, 3 + k, None] * rb
    return xs, ys


def tps_points(point, source, target):
    """torch_tps_transform_point.transformer: point [n,Q,2] through the spline source -> target."""
    p = f64(point)
    xs, ys = tps_eval(tps_solve(source, target), source, p[:, :, 0], p[:, :, 1])
    return np.stack((xs, ys), axis=2)


def tps_action(T, source, steps=33):
    """The spline (source, T) evaluated on a steps x steps grid over [-1, 1]^2 -> [n, steps * steps, 2]: how a T is judged."""
    g = np.linspace(-1.0, 1.0, steps)
    gx, gy = np.meshgrid(g, g)
    xs, ys = tps_eval(T, source, gx.reshape(-1), gy.reshape(-1))
    return np.stack((xs, ys), axis=2)


def tps_dense_coords(source, T, out_h, out_w):
    """Normalised sampling coordinates of every canvas pixel, (xn, yn) [n,out_h,out_w], from a GIVEN T (fp64 or the kernel's)."""
    n = f64(source).shape[0]
    gx = np.broadcast_to(linspace(out_w)[None, :], (out_h, out_w)).reshape(-1)
    gy = np.broadcast_to(linspace(out_h)[:, None], (out_h, out_w)).reshape(-1)
    xs, ys = tps_eval(T, source, gx, gy)
    return xs.reshape(n, out_h, out_w), ys.reshape(n, out_h, out_w)


def tsmotion(smotion, tmotion, img_h=360, img_w=480, lag=1):
    """test_online_tra.py:309-347 for one view: smotion, tmotion [n,7,9,2] (LR px) -> (smesh, tsmotion) [n,7,9,2]; frame k pairs with
    frame k - lag, the first `lag` frames get 0.  The normalised rigid mesh (the spline's source) is rounded to fp32, as the
    reference's is; the rest is fp64."""
    import torch
    sm, tm = f64(smotion), f64(tmotion)
    n = sm.shape[0]
    xs = torch.linspace(0.0, float(img_w), 9).numpy().astype(np.float64)
    ys = torch.linspace(0.0, float(img_h), 7).numpy().astype(np.float64)
    rigid = np.stack(np.broadcast_arrays(xs[None, :], ys[:, None]), axis=2)[None]
    scale = np.array([2.0 / img_w, 2.0 / img_h])

    def norm(m):
        return (m * scale - 1.0).reshape(m.shape[0], 63, 2)
    nrigid32 = norm(rigid).astype(F32)
    smesh = rigid + sm
    ts = np.zeros_like(sm)
    if n > lag:
        prev = norm(smesh[:n - lag])
        cur = norm(rigid + tm[lag:])
        out = tps_points(cur, np.repeat(nrigid32, n - lag, axis=0), prev)
        ts[lag:] = ((out + 1.0) / scale).reshape(-1, 7, 9, 2) - smesh[lag:]
    return smesh, ts


# ------------------------------------------------------------------------------------------------ metrics
def psnr_ssim(w1, w2):
    """w1, w2 [4,h,w] fp32 (3 colour planes 0..255 + mask plane) -> (psnr, ssim) of (w1 ov, w2 ov), ov = m1 m2: the products
    m1 * m2 and plane * ov are rounded to fp32 (the reference multiplies fp32 arrays), everything after is fp64 with scikit-image
    0.15 semantics: data range 255, 7 x 7 uniform window, sample covariance, SSIM map averaged over [3:-3, 3:-3], channel mean."""
    a, b = f32(w1), f32(w2)
    ov = (a[3] * b[3]).astype(F32)
    x = (a[:3] * ov[None]).astype(F32).astype(np.float64)
    y = (b[:3] * ov[None]).astype(F32).astype(np.float64)
    _, h, w = x.shape
    psnr = 10.0 * np.log10(255.0 ** 2 / np.mean((x - y) ** 2))
    c1, c2 = (0.01 * 255.0) ** 2, (0.03 * 255.0) ** 2

    def box(v):                                   # mean over the 7 x 7 window centred on every interior pixel
        s = np.zeros((3, h - 6, w - 6))
        for dy in range(7):
            for dx in range(7):
                s += v[:, dy:dy + h - 6, dx:dx + w - 6]
        return s / 49.0
    ux, uy, uxx, uyy, uxy = box(x), box(y), box(x * x), box(y * y), box(x * y)
    cn = 49.0 / 48.0
    vx, vy, vxy = cn * (uxx - ux * ux), cn * (uyy - uy * uy), cn * (uxy - ux * uy)
    s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
    return float(psnr), float(s.mean())


def stability_score(path):
    """path [t,63,2] (or [t,7,9,2]): test_metric_ssd.py:459-468, 7-tap path differences, weights 0.1 / 0.3 / 0.9."""
    p = f64(path).reshape(np.shape(path)[0], -1)
    t = p.shape[0]
    mid = p[3:t - 3]
    tot = 0.0
    for lag, wt in ((3, 0.1), (2, 0.3), (1, 0.9)):
        tot += wt * (np.mean((p[3 - lag:t - 3 - lag] - mid) ** 2) + np.mean((p[3 + lag:t - 3 + lag] - mid) ** 2))
    return float(tot)


def distortion_score(mesh):
    """mesh [t,7,9,2] (LR px): max over frames of inter + intra grid loss as the reference EXECUTES them on its 5-D tensors
    (test_metric_ssd.py:38-87, 473-482; see oracle.metrics.inter_grid for the axis the cosine is reduced over)."""
    m = f64(mesh)
    best = -np.inf
    for f in range(m.shape[0]):
        v = m[f]                                             # [7,9,2]
        we = v[:, 0:8] - v[:, 1:9]                           # [7,8,2]
        a, b = we[:, 0:7], we[:, 1:8]
        dw = 1 - (a * b).sum(1) / (np.sqrt((a * a).sum(1)) * np.sqrt((b * b).sum(1)))      # [7,2]
        dw = dw[0:6] + dw[1:7]
        he = v[0:6] - v[1:7]                                 # [6,9,2]
        a, b = he[0:5], he[1:6]
        dh = 1 - (a * b).sum(1) / (np.sqrt((a * a).sum(1)) * np.sqrt((b * b).sum(1)))      # [5,2]
        dh = dh[:, 0:8] + dh[:, 1:9]                         # [5,2] + [5,1]: the reference's broadcast
        inter = dw.mean() + dh.mean()
        dx = v[:, 1:9, 0] - v[:, 0:8, 0]
        dy = v[1:7, :, 1] - v[0:6, :, 1]
        intra = np.maximum(dx - 120.0, 0).mean() + np.maximum(dy - 120.0, 0).mean()
        best = max(best, inter + intra)
    return float(best)


# ------------------------------------------------------------------------------------------------ convolution
def _conv_geometry(x, w, stride, pad):
    """2-D operands get a temporal axis of 1; pad: a number (h and w), (ph, pw) or (pt, ph, pw).  The temporal stride is 1."""
    if x.ndim == 4:
        x, w = x[:, :, None], w[:, :, None]
    pad = (0, pad, pad) if np.isscalar(pad) else ((0,) + tuple(pad) if len(pad) == 2 else tuple(pad))
    n, c, t, h, wd = x.shape
    co, cw, kt, kh, kw = w.shape
    assert cw == c, (x.shape, w.shape)
    to, ho, wo = t + 2 * pad[0] - kt + 1, (h + 2 * pad[1] - kh) // stride + 1, (wd + 2 * pad[2] - kw) // stride + 1
    assert to > 0 and ho > 0 and wo > 0, (x.shape, w.shape, stride, pad)
    return x, w, pad, (to, ho, wo)


def conv(x, w, bias=None, res=None, stride=1, pad=0, relu=False):
    """nn.Conv2d / nn.Conv3d (+ bias, + residual, + ReLU): x [n,c,(t,)h,w], w [cout,c,(kt,)kh,kw], zero padding `pad` on h and w (and
    t when three are given), stride on h and w -> (value, S), both [n,cout,(to,)ho,wo]; S is the same loop on absolute values,
    sum |x||w| + |bias| + |res|: the scale of dot_bound.  Per image (and block of output rows) the taps are gathered one by one into
    [tap][c][to][rows][wo] and contracted with w in one product over (tap, c) -- the definition, in no particular order."""
    two = np.ndim(x) == 4
    x, w, (pt, ph, pw), (to, ho, wo) = _conv_geometry(f64(x), f64(w), stride, pad)
    n, c, t, h, wd = x.shape
    co, _, kt, kh, kw = w.shape
    xp = np.zeros((n, c, t + 2 * pt, h + 2 * ph, wd + 2 * pw))
    xp[:, :, pt:pt + t, ph:ph + h, pw:pw + wd] = x
    wk = w.reshape(co, c, kt * kh * kw).transpose(0, 2, 1)                      # [cout][tap][c]
    val = np.empty((n, co, to, ho, wo))
    s = np.empty_like(val)
    rows = max(1, (1 << 23) // (kt * kh * kw * c * to * wo))                  # output rows per pass: the gathered taps stay <= 64 MB
    for b in range(n):
        for y0 in range(0, ho, rows):
            y1 = min(y0 + rows, ho)
            cols = np.empty((kt * kh * kw, c, to, y1 - y0, wo))
            for dt in range(kt):
                for dy in range(kh):
                    for dx in range(kw):
                        ys = y0 * stride + dy
                        cols[(dt * kh + dy) * kw + dx] = xp[b, :, dt:dt + to, ys:ys + (y1 - y0 - 1) * stride + 1:stride,
                                                            dx:dx + (wo - 1) * stride + 1:stride]
            val[b, :, :, y0:y1] = np.tensordot(wk, cols, axes=([1, 2], [0, 1]))
            s[b, :, :, y0:y1] = np.tensordot(np.abs(wk), np.abs(cols), axes=([1, 2], [0, 1]))
    if bias is not None:
        bb = f64(bias).reshape(1, co, 1, 1, 1)
        val, s = val + bb, s + np.abs(bb)
    if res is not None:
        rr = f64(res).reshape(val.shape)
        val, s = val + rr, s + np.abs(rr)
    if relu:
        val = np.maximum(val, 0.0)
    return (val[:, :, 0], s[:, :, 0]) if two else (val, s)


def conv_terms(x_shape, w_shape, stride=1, pad=0):
    """How many REAL products every output element of `conv` sums (taps that fall into the zero padding do not count; nor may the
    caller count channels that exist only as layout padding: w_shape carries the real channel count) -> [(to,)ho,wo]."""
    two = len(x_shape) == 4
    x, w, pad, out = _conv_geometry(np.empty(x_shape, np.int8), np.empty(w_shape, np.int8), stride, pad)
    cnt = []
    for size, k, p, st, o in zip(x.shape[2:], w.shape[2:], pad, (1, stride, stride), out):
        pos = np.arange(o)[:, None] * st - p + np.arange(k)[None, :]
        cnt.append(((pos >= 0) & (pos < size)).sum(axis=1))
    terms = w.shape[1] * cnt[0][:, None, None] * cnt[1][None, :, None] * cnt[2][None, None, :]
    return terms[0] if two else terms


def pool_max(v, k, stride, pad):
    """nn.MaxPool2d(k, stride, pad), floor mode, -inf padding, over the last two axes of any array: of a value it is the pooled
    value; of a per-element error bound it is the bound of the pooled element (the maximum of the bounds in its window)."""
    v = f64(v)
    h, w = v.shape[-2:]
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    vp = np.full(v.shape[:-2] + (h + 2 * pad, w + 2 * pad), -np.inf)
    vp[..., pad:pad + h, pad:pad + w] = v
    out = np.full(v.shape[:-2] + (ho, wo), -np.inf)
    for dy in range(k):
        for dx in range(k):
            out = np.maximum(out, vp[..., dy:dy + (ho - 1) * stride + 1:stride, dx:dx + (wo - 1) * stride + 1:stride])
    return out


def conv_bound(x, w, bias=None, res=None, stride=1, pad=0, relu=False, extra=4):
    """-> (value, bound) of `conv`: bound = dot_bound(K_real + 2, S, extra) per element, K_real from conv_terms (+ 2: bias, residual).
    It holds for every order of the sum, so a split-K kernel needs nothing added; ReLU is exact."""
    val, s = conv(x, w, bias, res, stride, pad, relu)
    k = conv_terms(np.shape(x), np.shape(w), stride, pad) + 2
    return val, dot_bound(k[None, None], s, extra)


def conv_pool2(x, w, bias=None, stride=1, pad=0, relu=True, extra=4):
    """`conv` followed by nn.MaxPool2d(2, 2) (floor: the last row / column of an odd map is dropped) -> (value, bound)."""
    val, b = conv_bound(x, w, bias, None, stride, pad, relu, extra)
    return pool_max(val, 2, 2, 0), pool_max(b, 2, 2, 0)


def stem(x, w, bias=None, extra=4):
    """The network stem: Conv2d(3, cout, 7, stride 2, pad 3) with BatchNorm folded into (w, bias), ReLU -> (value, bound), and
    stem_pool: the same followed by MaxPool2d(3, 2, 1)."""
    return conv_bound(x, w, bias, None, 2, 3, True, extra)


def stem_pool(x, w, bias=None, extra=4):
    val, b = stem(x, w, bias, extra)
    return pool_max(val, 3, 2, 1), pool_max(b, 3, 2, 1)


# Winograd minimal filtering F(m x m, 3 x 3), Y = A^T [ (G g G^T) . (B^T d B) ] A  (Lavin & Gray 2015), m = 2 and 4
WINO = {
    2: dict(BT=np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=np.float64),
            G=np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=np.float64),
            AT=np.array([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=np.float64)),
    4: dict(BT=np.array([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0],
                         [0, 4, 0, -5, 0, 1]], dtype=np.float64),
            G=np.array([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6],
                        [0, 0, 1]], dtype=np.float64),
            AT=np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], dtype=np.float64)),
}


def wino_tiles(x, m):
    """x [n,c,h,w] -> d [n,c,th,tw,m+2,m+2]: the (m + 2)^2 input windows of the m x m output tiles of a 3 x 3 / pad 1 convolution,
    tiles laid out from output pixel (0, 0) (th = ceil(h / m)), zeros outside the image."""
    n, c, h, w = x.shape
    th, tw, a = -(-h // m), -(-w // m), m + 2
    xp = np.zeros((n, c, th * m + 2, tw * m + 2), dtype=x.dtype)
    xp[:, :, 1:1 + h, 1:1 + w] = x
    d = np.empty((n, c, th, tw, a, a), dtype=x.dtype)
    for i in range(a):
        for j in range(a):
            d[..., i, j] = xp[:, :, i:i + th * m:m, j:j + tw * m:m]
    return d


def wino_untile(y, h, w):
    """[n,co,th,tw,m,m] -> [n,co,h,w]"""
    n, co, th, tw, m, _ = y.shape
    return y.transpose(0, 1, 2, 4, 3, 5).reshape(n, co, th * m, tw * m)[:, :, :h, :w]


def wino_scale(x, w, m, bias=None, res=None):
    """The scale of the rounding error of F(m x m, 3 x 3) on x [n,c,h,w], w [cout,c,3,3] -> S_w [n,cout,h,w]:
    |A^T| [ sum_c (|G||g_c||G^T|) . (|B^T||d_c||B|) ] |A| per output tile (+ |bias| + |res|), the Winograd form evaluated on
    absolute values -- what dot_bound's S is to a direct sum.  It exceeds the direct S by the growth of the transforms
    (|B^T| . |B| has row sums up to 4 for m = 2 and 100 for m = 4)."""
    x, w = f64(x), f64(w)
    k = WINO[m]
    bt, g, at = np.abs(k['BT']), np.abs(k['G']), np.abs(k['AT'])
    u = np.einsum('ia,ocab,jb->ocij', g, np.abs(w), g)
    v = np.einsum('ia,nctuab,jb->nctuij', bt, wino_tiles(np.abs(x), m), bt)
    n, c, th, tw, a, _ = v.shape
    prod = np.einsum('ijoc,ijcq->ijoq', u.transpose(2, 3, 0, 1), v.transpose(4, 5, 1, 0, 2, 3).reshape(a, a, c, n * th * tw))
    prod = prod.reshape(a, a, w.shape[0], n, th, tw).transpose(3, 2, 4, 5, 0, 1)           # [n,co,th,tw,a,a]
    s = wino_untile(np.einsum('pi,notuij,qj->notupq', at, prod, at), x.shape[2], x.shape[3])
    if bias is not None:
        s = s + np.abs(f64(bias)).reshape(1, -1, 1, 1)
    if res is not None:
        s = s + np.abs(f64(res))
    return s


# roundings of the transforms of one output element, beside the cin of the channel sum: a row of a transform matrix with k
# non-zero entries costs at most k - 1 additions (its constants are fused or powers of two in the kernels: v_fma / v_pk_fma), the
# filter transform is formed in fp64 and rounded once.  m = 2 (wino.hip): B^T rows have 2 entries -> 1 + 1, A^T rows 3 -> 2 + 2,
# filters 1: 7.  m = 4 (wino43.hip): B^T rows up to 4 entries -> 3 + 3 (and one more each where 5 x is not fused: 4 + 4), A^T rows 5
# -> 4 + 4, filters 1: 17.
WINO_ROUNDINGS = {2: 7, 4: 17}


def wino_ceiling(cin, m, s_w, extra=3):
    """The derived ceiling of F(m x m, 3 x 3) in fp32: (1.01 (cin + T_m) + extra) u S_w; extra: bias, residual, store."""
    return (1.01 * (cin + WINO_ROUNDINGS[m]) + extra) * U24 * s_w
