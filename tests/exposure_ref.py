"""Float64 numpy statement of the exposure estimator (include/stabstitch_hip.h, ss_exposure_update): which lattice nodes count, the
per-pair statistics, the Brown-Lowe normal equations per channel, and the fp32 smoothing walk.  tests/test_exposure_abi.py checks it
against hand-worked cases, tests/test_gpu_exposure.py holds the kernel to it."""
import numpy as np

import ref64 as R

F = np.float32
DEFAULTS = dict(alpha=0.1, sigma_n=10.0, sigma_g=0.1, lo=4.0, hi=251.0, min_nodes=16, gain_min=0.5, gain_max=2.0)
PAIRS = {2: [(0, 1)], 3: [(0, 1), (0, 2), (1, 2)]}


def lattice_shape(hc, wc):
    return (hc + 7) // 8 + 1, 2 * ((wc + 63) // 64) + 1


def footprint_lattice(row, views, hc, wc):
    """One footprint row (fp32 [ss_render_footprint_floats]) -> its lattice [V,ny,nx,2] (xn, yn), fp32."""
    ny, nx = lattice_shape(hc, wc)
    return np.asarray(row[:views * ny * nx * 2], F).reshape(views, ny, nx, 2)


def on_canvas(hc, wc):
    """[ny,nx] bool: node (i, j) = canvas pixel (32 j, 8 i) lies on the canvas (the lattice's last row / column may not)."""
    ny, nx = lattice_shape(hc, wc)
    return (8 * np.arange(ny)[:, None] <= hc - 1) & (32 * np.arange(nx)[None, :] <= wc - 1)


def samples(img, lat, mode):
    """img [3,h,w] (any real dtype; uint8 frames come as their fp32 planes: the conversion is exact), lat [ny,nx,2] fp32 ->
    float64 samples [3,ny,nx] of the render's sampler of `mode` at the stored coordinates."""
    xn, yn = lat[None, ..., 0], lat[None, ..., 1]
    fn = R.bilinear_clamped if mode == 'NORMAL' else R.grid_sample_zeros
    return fn(np.asarray(img, np.float64)[None], xn, yn)[0]


def statistics(imgs, lat, hc, wc, mode, lo=4.0, hi=251.0):
    """imgs: V arrays [3,h,w]; lat [V,ny,nx,2] -> ({pair: (n, Sa [3], Sb [3])}, {pair: usable [ny,nx]}, samples [V,3,ny,nx])."""
    v = len(imgs)
    inside = [(np.abs(lat[k, ..., 0]) <= F(1)) & (np.abs(lat[k, ..., 1]) <= F(1)) for k in range(v)]      # the stored fp32 values
    s = np.stack([samples(imgs[k], lat[k], mode) for k in range(v)])
    ok = [inside[k] & on_canvas(hc, wc) & ((s[k] >= lo) & (s[k] <= hi)).all(0) for k in range(v)]
    stats, use = {}, {}
    for (a, b) in PAIRS[v]:
        u = ok[a] & ok[b]
        use[(a, b)] = u
        stats[(a, b)] = (int(u.sum()), s[a][:, u].sum(1), s[b][:, u].sum(1))
    return stats, use, s


def targets(stats, views, sigma_n=10.0, sigma_g=0.1, min_nodes=16, gain_min=0.5, gain_max=2.0, clamp=True):
    """stats {pair: (n, Sa [3], Sb [3])} -> (target gains [V,3] float64, kept: was any pair kept).  Per channel the minimiser of
    sum n [(g_a m_ab - g_b m_ba)^2 / sigma_n^2 + ((1 - g_a)^2 + (1 - g_b)^2) / sigma_g^2] over the kept pairs, written for the
    deviation d = g - 1 and scaled by sigma_n^2:  A d = r,  A_aa = sum n (m_a^2 + lam),  A_ab = -n m_a m_b,
    r_a = sum n m_a (m_b - m_a),  lam = sigma_n^2 / sigma_g^2.  A view in no kept pair keeps 1."""
    lam = (float(sigma_n) * float(sigma_n)) / (float(sigma_g) * float(sigma_g))
    kept = [(p, st) for p, st in stats.items() if st[0] >= min_nodes and st[0] > 0]
    g = np.ones((views, 3))
    involved = sorted({k for p, _ in kept for k in p})
    if not kept:
        return g, False
    idx = {k: i for i, k in enumerate(involved)}
    for c in range(3):
        A = np.zeros((len(involved), len(involved)))
        r = np.zeros(len(involved))
        for (a, b), (n, sa, sb) in kept:
            n = float(n)
            ma, mb = float(sa[c]) / n, float(sb[c]) / n
            ia, ib = idx[a], idx[b]
            A[ia, ia] += n * (ma * ma + lam)
            A[ib, ib] += n * (mb * mb + lam)
            A[ia, ib] -= n * ma * mb
            A[ib, ia] -= n * ma * mb
            r[ia] += n * ma * (mb - ma)
            r[ib] += n * mb * (ma - mb)
        d = np.linalg.solve(A, r)
        for k in involved:
            g[k, c] = 1.0 + d[idx[k]]
    if clamp:
        g = np.clip(g, float(gain_min), float(gain_max))
    return g, True


def energy(g, stats, sigma_n=10.0, sigma_g=0.1, min_nodes=16, c=0):
    """E(g) of channel c (the definition, for checking that `targets` minimises it)."""
    e = 0.0
    for (a, b), (n, sa, sb) in stats.items():
        if n < min_nodes:
            continue
        ma, mb = sa[c] / n, sb[c] / n
        e += n * ((g[a] * ma - g[b] * mb) ** 2 / sigma_n ** 2 + ((1 - g[a]) ** 2 + (1 - g[b]) ** 2) / sigma_g ** 2)
    return e


def smooth(state, started, target, kept, alpha=0.1):
    """One frame of the smoothing walk in fp32, one rounding per operation: state, target [V,3] -> (state, started)."""
    if not kept:
        return np.asarray(state, F).copy(), started
    t = np.asarray(target, np.float64).astype(F)
    if not started:
        return t.copy(), True
    s = np.asarray(state, F)
    return F(s + F(F(alpha) * F(t - s))), True
