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


# ------------------------------------------------------------------------------------------------ LINEAR fusion
def gauss21():
    """The 21 weights of GaussianBlur((21, 21), sigma 20): exp(-0.5 (t / 20)^2) on t = -10 .. 10, normalised, in float64."""
    t = np.arange(-10, 11, dtype=np.float64)
    k = np.exp(-0.5 * (t / 20.0) ** 2)
    return k / k.sum()


def blur21(x, k=None, border='reflect'):
    """x [h,w] (h, w >= 11) -> the separable 21-tap Gaussian of x with a reflect border (the border pixel is not repeated)."""
    k = gauss21() if k is None else k
    h, w = x.shape
    xp = np.pad(x, ((0, 0), (10, 10)), mode=border)
    y = sum(k[i] * xp[:, i:i + w] for i in range(21))
    yp = np.pad(y, ((10, 10), (0, 0)), mode=border)
    return sum(k[i] * yp[i:i + h, :] for i in range(21))


def linear_blender(ref, tgt, ref_m, tgt_m, parts=False, blur=blur21, eps=1e-3):
    """The reference's linear_blender (test_online_tra.py:34-58): ref, tgt [3,h,w] | None, ref_m, tgt_m [h,w] -> (mask1 [h,w],
    planes [3,h,w] | None).

      cen_k   the centroid (row, column) of the non-zero pixels of mask k; vec = cen2 - cen1
      ovl     round(ref_m tgt_m) (half to even), ref_only = ref_m - ovl
      proj    (r - cen1_r) vec_r + (c - cen1_c) vec_c on the overlap; ovl_mask = (proj - min) / (max - min + 1e-3) there, 0 elsewhere
      mask1   clamp(blur21(ref_only + (1 - ovl_mask) ref_m) ref_m + ref_only, 0, 1)
      planes  ref mask1 + tgt (1 - mask1) tgt_m

    Two places are stated, not inherited.  The reference DEFINES the centroids as fp32 numbers (`.float().mean()`) and vec cancels,
    so they are the exact mean (integer sums, one division) rounded through f32, and float64 from there on.  On an empty overlap
    the reference raises (`proj.min()` of nothing); the library defines ovl_mask = 0 there, and that extension is what is stated
    here -- it also covers an empty target mask, whose centroid (0 / 0) is then never used.
    parts: also return dict(om, X, P, den, overlap) for the derived bound (linear_blend_bound): P = the largest |a| + |b| of
    proj = a + b over the overlap, den = max - min + 1e-3."""
    m1, m2 = f64(ref_m), f64(tgt_m)
    h, w = m1.shape
    assert h >= 11 and w >= 11, (h, w)
    r1, c1 = np.nonzero(m1)
    assert r1.size, 'the reference mask is empty'
    cen1 = (float(F32(r1.sum() / r1.size)), float(F32(c1.sum() / r1.size)))
    ovl = np.round(m1 * m2)
    ref_only = m1 - ovl
    om = np.zeros_like(m1)
    r, c = np.nonzero(ovl)
    P, den = 0.0, eps
    if r.size:
        r2, c2 = np.nonzero(m2)
        cen2 = (float(F32(r2.sum() / r2.size)), float(F32(c2.sum() / r2.size)))
        vec = (cen2[0] - cen1[0], cen2[1] - cen1[1])
        a, b = (r - cen1[0]) * vec[0], (c - cen1[1]) * vec[1]
        proj = a + b
        den = proj.max() - proj.min() + eps
        om[r, c] = (proj - proj.min()) / den
        P = float((np.abs(a) + np.abs(b)).max())
    X = ref_only + (1.0 - om) * m1
    mask1 = np.clip(blur(X) * m1 + ref_only, 0.0, 1.0)
    planes = None
    if ref is not None:
        planes = f64(ref) * mask1[None] + f64(tgt) * ((1.0 - mask1) * m2)[None]
    if parts:
        return mask1, planes, dict(om=om, X=X, P=P, den=float(den), overlap=int(r.size))
    return mask1, planes


LB_WEIGHT_U = 32            # relative error of one fp32 blur weight in units of u: the argument (i - 10) / 20, its square and the
                            # halving 3 u of an argument <= 0.125 (0.4 u of the value), expf 2 ulp = 4 u, the 21-term sum of positive
                            # numbers 21 u, the division 1 u: 27 u, rounded up


def linear_blend_bound(ref, tgt, ref_m, tgt_m):
    """-> (mask1, planes | None, bound_mask1 [h,w], bound_planes [3,h,w] | None): linear_blender and the derived bound of an fp32
    evaluation of it in which every operation is one correctly rounded IEEE operation or a fused multiply-add (u = 2^-24), for
    masks on which round(ref_m tgt_m) is decided exactly (sweep_inputs.lb_case asserts it) and centroids defined as above:

      proj    vec = cen2 - cen1, r - cen1, the product, the sum:    d_p   = 1.01 * 4 u P
      om      numerator 2 d_p + u n, denominator 2 d_p + 2 u den + u 1e-3 (the constant in fp32), the division u, om <= 1:
                                                                   d_om  = 1.01 (4 d_p / den + 4 u)
              (0 on an overlap of one pixel: proj - min is x - x there in every precision, and on none)
      X       1 - om, the product with ref_m, the sum (X <= 2):     d_X   = ref_m d_om + 4.04 u
      blur    per pass a 21-term fp32 accumulation (dot_bound's gamma_21) with weights of relative error LB_WEIGHT_U u, on
              X >= 0 -- so the scale of both is the blur itself; the input's error passes through (the weights sum to 1):
                                                                   d_B   = blur21(d_X) + 2 (1.01 * 21 + LB_WEIGHT_U) u 1.01 blur21(X)
      mask1   blur * ref_m, + ref_only, the clamp contracts:        d_M   = ref_m d_B + 2.02 u (blur21(X) ref_m + ref_only)
      planes  ref mask1 + tgt ((1 - mask1) tgt_m): the inputs' d_M, 2 roundings on the first product and sum, 4 on the second:
                                                                   d_out = (|ref| + |tgt| tgt_m) d_M + 1.01 u (2 |ref| mask1 + 4 |tgt| mask2)"""
    mask1, planes, p = linear_blender(ref, tgt, ref_m, tgt_m, parts=True)
    m1, m2 = f64(ref_m), f64(tgt_m)
    d_p = 1.01 * 4 * U24 * p['P']
    d_om = 1.01 * (4 * d_p / p['den'] + 4 * U24) if p['overlap'] > 1 else 0.0
    d_x = m1 * d_om * (np.round(m1 * m2) != 0) + 4.04 * U24
    bl = blur21(p['X'])
    d_b = blur21(d_x) + 2 * (1.01 * 21 + LB_WEIGHT_U) * U24 * 1.01 * bl
    d_m = m1 * d_b + 2.02 * U24 * (bl * m1 + (m1 - np.round(m1 * m2)))
    d_out = None
    if planes is not None:
        a, b = np.abs(f64(ref)), np.abs(f64(tgt))
        d_out = (a + b * m2[None]) * d_m[None] + 1.01 * U24 * (2 * a * mask1[None] + 4 * b * ((1.0 - mask1) * m2)[None])
    return mask1, planes, d_m, d_out


# ------------------------------------------------------------------------------------------------ mesh geometry
def dlt4(src, dst):
    """utils/torch_DLT.py: the homography src -> dst from four correspondences, src, dst [n,4,2] -> H [n,3,3] with H[2,2] = 1;
    rows per corner (x, y) -> (u, v): [x y 1 0 0 0 -ux -uy] h = u, [0 0 0 x y 1 -vx -vy] h = v, solved in float64."""
    d = f64(dst)
    n = d.shape[0]
    s = np.broadcast_to(f64(src), d.shape)
    x, y, u, v = s[..., 0], s[..., 1], d[..., 0], d[..., 1]
    one, zero = np.ones_like(x), np.zeros_like(x)
    A = np.stack((np.stack((x, y, one, zero, zero, zero, -u * x, -u * y), -1),
                  np.stack((zero, zero, zero, x, y, one, -v * x, -v * y), -1)), 2).reshape(n, 8, 8)
    h = np.linalg.solve(A, d.reshape(n, 8, 1)).reshape(n, 8)
    return np.concatenate((h, np.ones((n, 1))), 1).reshape(n, 3, 3)


def decompose(offset8, img_h, img_w, scale=1.0):
    """spatial_network.py:72-93 / 291-300: offset8 [n,8] -> (H, H_tgt, H_ref) [n,3,3]: H = DLT(c, c + m), H_tgt = DLT(c, c + m / 2),
    H_ref = H^-1 H_tgt, every corner point divided by `scale`.  The corner points are the fp32 numbers the reference forms (c + m
    and c + m / 2 are one fp32 addition each; / 2 and / scale are exact for the powers of two in use); float64 from there."""
    m = f32(offset8).reshape(-1, 4, 2)
    c = np.array([[0.0, 0.0], [img_w, 0.0], [0.0, img_h], [img_w, img_h]], F32)[None]
    sc = F32(scale)
    H = dlt4(c / sc, (c + m) / sc)
    Ht = dlt4(c / sc, (c + m / F32(2.0)) / sc)
    return H, Ht, np.linalg.inv(H) @ Ht


def spatial_thetas(offset8, img_h, img_w):
    """spatial_network.py:291-300 -> (theta_ref, theta_tgt) [n,3,3]: M^-1 H M of the decomposition at 1/8 scale, M = [[w/2, 0, w/2],
    [0, h/2, h/2], [0, 0, 1]] at the feature size (w, h) = (img_w / 8, img_h / 8)."""
    _, Ht, Hr = decompose(offset8, img_h, img_w, 8.0)
    fw, fh = img_w / 8.0 / 2.0, img_h / 8.0 / 2.0
    M = np.array([[fw, 0, fw], [0, fh, fh], [0, 0, 1.0]])
    Mi = np.linalg.inv(M)
    return Mi @ Hr @ M, Mi @ Ht @ M


def h2mesh(H, mesh):
    """spatial_network.py:20-36: H [n,3,3], mesh [n,...,2] -> persp_divide(H^-1 [x y 1]^T), the shape of mesh."""
    m = f64(mesh)
    p = m.reshape(m.shape[0], -1, 2)
    t = np.linalg.inv(f64(H)) @ np.concatenate((p, np.ones(p.shape[:2] + (1,))), 2).transpose(0, 2, 1)
    return np.stack((t[:, 0] / t[:, 2], t[:, 1] / t[:, 2]), 2).reshape(m.shape)


def rigid_mesh(img_h, img_w):
    """[7,9,2] (x, y): torch.linspace(0, size, 9 | 7) as fp32 VALUES, promoted"""
    import torch
    xs = torch.linspace(0.0, float(img_w), 9).numpy().astype(np.float64)
    ys = torch.linspace(0.0, float(img_h), 7).numpy().astype(np.float64)
    return np.stack(np.broadcast_arrays(xs[None, :], ys[:, None]), axis=2)


def spatial_meshes(offset8, off_ref, off_tgt, img_h, img_w):
    """build_SpatialNet's tail: (motion1, motion2) [n,7,9,2] = H2Mesh(H_ref | H_tgt, rigid) + off_ref | off_tgt - rigid, the
    decomposition at full scale."""
    _, Ht, Hr = decompose(offset8, img_h, img_w, 1.0)
    n = Hr.shape[0]
    rigid = np.repeat(rigid_mesh(img_h, img_w)[None], n, 0)
    return (h2mesh(Hr, rigid) + f64(off_ref).reshape(n, 7, 9, 2) - rigid, h2mesh(Ht, rigid) + f64(off_tgt).reshape(n, 7, 9, 2) - rigid)


# ------------------------------------------------------------------------------------------------ SmoothNet glue
# One statement, three readings.  dt = float64: the statement.  dt = float32: every operation below is one numpy fp32 operation, in
# the reference's order -- the sequential fp32 program the kernels must reproduce bit for bit.  absum=True (float64, inputs taken
# by absolute value, every subtraction an addition): S, the scale of the derived bound smooth_bound, as conv's S is to dot_bound.
def _prep(x, dt, absum):
    x = np.asarray(f64(x) if dt == np.float64 else f32(x), dt)
    return np.abs(x) if absum else x


def _sub(a, b, absum):
    return a + b if absum else a - b


def window_flows(ts, nw, t, wstride, zero_first, dt=np.float64, absum=False):
    """smooth_network.py:139-144 per sliding window: ts [n,63,2] -> tsflow [nw,t,63,2], window wi covers frames wi wstride + [0, t);
    tsflow[0] = ts[first] (0 with zero_first: test_online_tra.py:362-366), tsflow[s] = tsflow[s - 1] + ts[first + s]."""
    ts = _prep(ts, dt, absum)
    out = np.empty((nw, t) + ts.shape[1:], dt)
    for wi in range(nw):
        b = wi * wstride
        acc = np.zeros_like(ts[b]) if zero_first else ts[b].copy()
        out[wi, 0] = acc
        for s in range(1, t):
            acc = acc + ts[b + s]
            out[wi, s] = acc
    return out


def window_meshes(sm, nw, t, wstride, dt=np.float64, absum=False):
    sm = _prep(sm, dt, absum)
    return np.stack([sm[wi * wstride:wi * wstride + t] for wi in range(nw)])


def smooth_embed(sm1, sm2, ts1, ts2, e1w, e1b, e3w, e3b, nw, t, wstride, zero_first, dt=np.float64, absum=False):
    """smooth_network.py:29-34, 66-72: hidden [nw,t,63,128] = cat(ReLU(Linear_1(smesh1)), ReLU(Linear_3(tsflow1)), ReLU(Linear_1(smesh2)),
    ReLU(Linear_3(tsflow2))), Linear(2 -> 32): (x w[c,0] + y w[c,1]) + b[c]."""
    def lin(p, w, b):
        w, b = _prep(w, dt, absum), _prep(b, dt, absum)
        o = (p[..., 0:1] * w[:, 0] + p[..., 1:2] * w[:, 1]) + b
        return o if absum else np.maximum(o, dt(0))
    return np.concatenate((lin(window_meshes(sm1, nw, t, wstride, dt, absum), e1w, e1b),
                           lin(window_flows(ts1, nw, t, wstride, zero_first, dt, absum), e3w, e3b),
                           lin(window_meshes(sm2, nw, t, wstride, dt, absum), e1w, e1b),
                           lin(window_flows(ts2, nw, t, wstride, zero_first, dt, absum), e3w, e3b)), axis=-1)


def smooth_finalize(sm1, sm2, ts1, ts2, delta, nw, t, wstride, zero_first, dt=np.float64, absum=False):
    """smooth_network.py:145-157 per window: delta [nw,t,63,4] -> the eight outputs [nw,t,63,2]: ori_mesh = smesh, ori_path = tsflow,
    smooth_mesh = ori_mesh - delta, smooth_path = ori_path + delta (delta[..., 0:2] for view 1, [..., 2:4] for view 2)."""
    d = _prep(delta, dt, absum).reshape(nw, t, -1, 4)
    out = {}
    for k, (sm, ts, dd) in enumerate(((sm1, ts1, d[..., 0:2]), (sm2, ts2, d[..., 2:4])), 1):
        om, op = window_meshes(sm, nw, t, wstride, dt, absum), window_flows(ts, nw, t, wstride, zero_first, dt, absum)
        out.update({'ori_mesh%d' % k: om, 'ori_path%d' % k: op, 'smooth_mesh%d' % k: _sub(om, dd, absum), 'smooth_path%d' % k: op + dd})
    return out


def smooth_stitch(sm1, sm2, ts1, ts2, delta, nw, t, dt=np.float64, absum=False):
    """The reference's frame loop over the sliding windows (test_online_tra.py:377-392, test_metric_ssd.py:415-436), n = nw + t - 1
    frames, stride 1, the first tsmotion of every window zeroed: window 0 gives its t frames, window k >= 1 its last one;
        ori_path[f]    = ori_path[f - 1] + (op_w[t - 1] - op_w[t - 2])
        smooth_path[f] = ori_path[f]     + (sp_w[t - 1] - op_w[t - 1])         (f >= t, w = f - t + 1)
    -> dict(ori_mesh1/2, smooth_mesh1/2, ori_path2, smooth_path2) [n,63,2]."""
    o = smooth_finalize(sm1, sm2, ts1, ts2, delta, nw, t, 1, 1, dt, absum)
    out = {}
    for k in ('ori_mesh1', 'ori_mesh2', 'smooth_mesh1', 'smooth_mesh2'):
        out[k] = np.concatenate((o[k][0], o[k][1:, -1]), 0)
    ori, sm = list(o['ori_path2'][0]), list(o['smooth_path2'][0])
    for w in range(1, nw):
        ori.append(ori[-1] + _sub(o['ori_path2'][w, -1], o['ori_path2'][w, -2], absum))
        sm.append(ori[-1] + _sub(o['smooth_path2'][w, -1], o['ori_path2'][w, -1], absum))
    out['ori_path2'], out['smooth_path2'] = np.stack(ori), np.stack(sm)
    return out


def smooth_bound(roundings, s):
    """The gate of a sequential fp32 evaluation with at most `roundings` rounded operations between an input and the output, s = the
    same evaluation on absolute values with every subtraction an addition: 2 x 1.01 roundings u s.  The rigorous forward bound is
    half of it (each operation multiplies what it has by (1 + d), |d| <= u, and what it has never exceeds s); a correct fp32 program
    comes close to that half where an output is two operations from its inputs (0.93 of it on 75600 such outputs of the sweep),
    so the gate carries the factor 2 that every derived gate is shown to leave the fp32 reading (tests/test_ref64.py).  A wrong
    order or a dropped term moves an output by its own size, 1e6 gates away; the bits are held separately."""
    assert np.all(np.asarray(roundings) * U24 < 0.01)
    return 2 * 1.01 * roundings * U24 * s


def window_shift(ring, rows):
    """The streaming windows' documented shift (include/stabstitch_hip.h, ss_window_push / ss_window_advance): ring [W,E] and the k new
    rows [k,E] -> (work [W-1+k,E] = ring rows 1 .. W-1 then the new rows, the new ring = the last W rows of work); a copy."""
    work = np.concatenate((ring[1:], rows), 0)
    return work, work[-ring.shape[0]:]


# ------------------------------------------------------------------------------------------------ canvas normalisation, watcher
def scale_to_hr(mesh, img_h, img_w, dt=np.float64):
    """test_online_tra.py:103-104: LR mesh [...,2] -> HR pixels, x * img_w / 480, y * img_h / 360 (the product, then the division);
    img_h = img_w = 0: the mesh is HR already."""
    m = np.asarray(mesh, dt)
    if img_w <= 0 and img_h <= 0:
        return m.copy()
    return np.stack(((m[..., 0] * dt(img_w)) / dt(480.0), (m[..., 1] * dt(img_h)) / dt(360.0)), -1)


def canvas_normalize(mesh_hr, bbox, dt=np.float64):
    """test_online_tra.py:129-136: HR mesh [...,2] on the canvas bbox = (wmin, wmax, hmin, hmax) -> [-1, 1]:
    ((x - wmin) * 2) / (wmax - wmin) - 1, the same in y; bbox broadcasts against the mesh's leading axes."""
    m, b = np.asarray(mesh_hr, dt), np.asarray(bbox, dt)
    ow, oh = b[..., 1] - b[..., 0], b[..., 3] - b[..., 2]
    return np.stack((((m[..., 0] - b[..., 0]) * dt(2.0)) / ow - dt(1.0), ((m[..., 1] - b[..., 2]) * dt(2.0)) / oh - dt(1.0)), -1)


def canvas_recover(nmesh, bbox, dt=np.float64):
    """test_online_tra.py:85-91 on the canvas: [-1, 1] -> canvas pixels, ((v + 1) * extent) / 2."""
    m, b = np.asarray(nmesh, dt), np.asarray(bbox, dt)
    return np.stack((((m[..., 0] + dt(1.0)) * (b[..., 1] - b[..., 0])) / dt(2.0), ((m[..., 1] + dt(1.0)) * (b[..., 3] - b[..., 2])) / dt(2.0)), -1)


def three_view_align(w12_m1, w12_m2, w23_m1, w23_m2, img_h, img_w, dt=np.float64):
    """test_online_tra_threeview.py:345-380: four LR meshes [n,63,2] -> (a1, a2, b1, b2, mid) in HR pixels: the pair (2, 3) is shifted
    by the per-frame mean over the 63 vertices of (w12_m2 - w23_m1); mid = (a2 + b1) / 2.  -> also `absdiff`, the mean of
    |w12_m2 - w23_m1|: the scale of the bound of an fp32 mean taken in any order."""
    a1, a2, b1, b2 = (scale_to_hr(m, img_h, img_w, dt) for m in (w12_m1, w12_m2, w23_m1, w23_m2))
    off = (a2 - b1).mean(axis=1, keepdims=True, dtype=dt)
    absdiff = np.abs(a2 - b1).mean(axis=1, keepdims=True, dtype=dt)
    b1, b2 = b1 + off, b2 + off
    return a1, a2, b1, b2, (a2 + b1) / dt(2.0), absdiff


WATCH_SLACK = F32(2.5e-4)


def canvas_watch(src, guard, watch_i, watch_f):
    """The overflow watcher of a streaming canvas as include/stabstitch_hip.h documents it: src [streams,P,2] canvas-normalised control
    points of one push ([-1, 1] = inside), watch_i [streams,4] = {frames seen, frames with a point outside, index of the first such
    frame (-1), frames with a point within `guard` of an edge or outside}, watch_f [streams,4] = running {xmin, xmax, ymin, ymax};
    updated in place.  Outside: a NaN point, or a coordinate beyond +-(1 + 2.5e-4) (the rounding slack); a guard not above the slack
    makes `near` coincide with `outside`.  All comparisons are strict and between fp32 numbers."""
    src = f32(src)
    one, g = F32(1.0), F32(guard)
    g = g if g > WATCH_SLACK else -WATCH_SLACK
    for s in range(src.shape[0]):
        x, y = src[s, :, 0], src[s, :, 1]
        bad = bool(np.isnan(src[s]).any())
        xmin, xmax, ymin, ymax = np.fmin.reduce(x), np.fmax.reduce(x), np.fmin.reduce(y), np.fmax.reduce(y)       # a NaN operand is dropped
        lo, hi = min(xmin, ymin), max(xmax, ymax)
        out = bad or lo < -one - WATCH_SLACK or hi > one + WATCH_SLACK
        near = out or lo < -one + g or hi > one - g
        seen = int(watch_i[s, 0])
        if out:
            watch_i[s, 1] += 1
            if watch_i[s, 2] < 0:
                watch_i[s, 2] = seen
        if near:
            watch_i[s, 3] += 1
        watch_i[s, 0] = seen + 1
        watch_f[s] = (np.fmin(watch_f[s, 0], xmin), np.fmax(watch_f[s, 1], xmax), np.fmin(watch_f[s, 2], ymin), np.fmax(watch_f[s, 3], ymax))


def ulp_bound(roundings, value, scale):
    """|fp32 sequence - float64| for `roundings` single rounded operations on numbers whose size, in the output's unit, is at most
    max(|value|, scale): 1.01 roundings u max(|value|, scale)."""
    return 1.01 * roundings * U24 * np.maximum(np.abs(value), scale)


def canvas_normalize_bound(mesh_hr, bbox):
    """-> (canvas_normalize in float64, its gate): the fp32 sequence is x * img_w, / 480, - wmin, * 2, / extent, - 1 -- six roundings
    (two fewer without the scaling) of numbers no larger than M = the largest coordinate or box entry, which in the output's unit
    is 2 M / extent of that axis."""
    m, b = f64(mesh_hr), f64(bbox)
    big = max(float(np.abs(m).max()), float(np.abs(b).max()))
    scale = np.stack((2 * big / (b[..., 1] - b[..., 0]), 2 * big / (b[..., 3] - b[..., 2])), -1)
    ref = canvas_normalize(m, b)
    return ref, ulp_bound(6, ref, np.broadcast_to(scale, ref.shape))


def canvas_recover_bound(nmesh, bbox):
    """-> (canvas_recover in float64, its gate): v + 1, * extent, / 2 -- three roundings of numbers up to (|v| + 1) extent."""
    n, b = f64(nmesh), f64(bbox)
    ext = np.stack((b[..., 1] - b[..., 0], b[..., 3] - b[..., 2]), -1)
    ref = canvas_recover(n, b)
    return ref, ulp_bound(3, ref, np.broadcast_to((np.abs(n) + 1) * ext, ref.shape))


def three_view_align_bound(w12_m1, w12_m2, w23_m1, w23_m2, img_h, img_w):
    """-> (a1, a2, b1, b2, mid in float64, the gates of b1, b2, mid): the two roundings of the scaling on every coordinate (`scaled`),
    the 63-point fp32 mean of the differences in ANY order (dot_bound on the mean of their absolute values, + their inputs' 2 x
    scaled), then b + off (one rounding) and (a2 + b1) / 2 (two)."""
    a1, a2, b1, b2, mid, absdiff = three_view_align(*[f64(m) for m in (w12_m1, w12_m2, w23_m1, w23_m2)], img_h, img_w)
    big = max(float(np.abs(x).max()) for x in (a1, a2, b1, b2))
    scaled = 1.01 * 2 * U24 * big
    mean_b = dot_bound(63, absdiff, extra=2) + 2 * scaled
    return (a1, a2, b1, b2, mid), (mean_b + scaled + U24 * np.abs(b1), mean_b + scaled + U24 * np.abs(b2),
                                   0.5 * mean_b + scaled + 2 * U24 * np.abs(mid))


def canvas_shift_bound(mesh_hr, origin):
    """-> (mesh - origin in float64, its gate): ONE rounding of a number up to |mesh| + |origin|.  A single rounding can reach its
    bound u |value| exactly, so the gate counts two: the factor 2 every derived gate leaves the fp32 reading."""
    m, o = f64(mesh_hr), f64(origin)
    ref = m - o
    return ref, ulp_bound(2, ref, 0.0)
