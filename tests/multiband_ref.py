"""MULTIBAND fusion stated in numpy: the Laplacian-pyramid blend of warped views (include/stabstitch_blend.h).

`blend(P, bands, np.float64)` is the statement the kernels are held to; `blend(P, bands, np.float32)` is the same program with every
operation rounded to fp32, in the order written here, which calibrates `bound`.

Input P [V][5][hc][wc]: warped B, G, R, the warped weight plane, the ones-mask (ss_tps_warp_mask_nchw on frame planes + weight_plane).
Decisions (exact on the input, the same in either precision):
    valid_v = P[v][4] >= 0.5;  union = any valid;  owner = the valid view with the largest P[v][3] (ties: the lowest index; 0 outside
    the union);  seam weights s_v = (owner == v);  filled views c'_v = valid_v ? c_v : (union ? c_owner : 0).
Pyramid: sizes n' = (n + 1) / 2; reduce = separable [1 4 6 4 1] / 16 at the even positions; expand: even outputs
(u[t-1] + 6 u[t] + u[t+1]) / 8, odd outputs (u[t] + u[t+1]) / 2; indices reflected without repeating the edge (-1 -> 1, n -> n - 2).
Blend:  r_B = sum_v G_B(s_v) G_B(c'_v);  r_l = sum_v G_l(s_v) (G_l(c'_v) - expand(G_{l+1}(c'_v))) + expand(r_{l+1});
        out = union ? min(max(r_0, 0), 255) : 0."""
import numpy as np

MAX_BANDS = 6
U32 = 2.0 ** -24


def weight_plane(h, w):
    """min(x + 1, w - x) * min(y + 1, h - y): small integers, exact in fp32.  The product, not the min of the four distances: two
    side-by-side views limited by the same vertical distance would tie over whole triangles."""
    x = np.arange(w)
    y = np.arange(h)
    return (np.minimum(x + 1, w - x)[None, :] * np.minimum(y + 1, h - y)[:, None]).astype(np.float32)


def level_sizes(hc, wc, bands):
    """[(h_l, w_l)] for l = 0..bands; ValueError where the library returns an argument error."""
    if not 0 <= bands <= MAX_BANDS:
        raise ValueError('bands must be 0..%d, got %r' % (MAX_BANDS, bands))
    out = [(hc, wc)]
    for _ in range(bands):
        h, w = out[-1]
        if h < 3 or w < 3:
            raise ValueError('a %d x %d level cannot be reduced (%d bands on %d x %d)' % (h, w, bands, hc, wc))
        out.append(((h + 1) // 2, (w + 1) // 2))
    return out


def max_bands(hc, wc):
    b = 0
    while b < MAX_BANDS and min(hc, wc) >= 3:
        hc, wc, b = (hc + 1) // 2, (wc + 1) // 2, b + 1
    return b


def workspace_floats(frames, views, hc, wc, bands):
    """The formula of include/stabstitch_blend.h."""
    a = [h * ((w + 3) & ~3) for h, w in level_sizes(hc, wc, bands)]
    k = views - 1
    return frames * (4 * k * sum(a) + 3 * sum(a[1:]) + 4 * a[0])


def _reflect(i, n):
    i = np.where(i < 0, -i, i)
    return np.where(i >= n, 2 * n - 2 - i, i)


def _reduce1(a, axis):
    n = a.shape[axis]
    t = 2 * np.arange((n + 1) // 2)
    tap = [np.take(a, _reflect(t + j, n), axis=axis) for j in (-2, -1, 0, 1, 2)]
    f = a.dtype.type
    return (((tap[0] + tap[4]) + f(4) * (tap[1] + tap[3])) + f(6) * tap[2]) * f(0.0625)


def reduce(a):
    """[..., h, w] -> [..., (h + 1) / 2, (w + 1) / 2]: along x, then along y."""
    return _reduce1(_reduce1(a, -1), -2)


def _expand1(u, n, axis):
    m = u.shape[axis]
    assert m == (n + 1) // 2
    f = u.dtype.type
    t = np.arange(m)
    um, up = np.take(u, _reflect(t - 1, m), axis=axis), np.take(u, _reflect(t + 1, m), axis=axis)
    even = ((um + up) + f(6) * u) * f(0.125)
    odd = (u + up) * f(0.5)
    shape = list(u.shape)
    shape[axis] = 2 * m
    out = np.empty(shape, u.dtype)
    sl = [slice(None)] * u.ndim
    sl[axis] = slice(0, None, 2)
    out[tuple(sl)] = even
    sl[axis] = slice(1, None, 2)
    out[tuple(sl)] = odd
    sl[axis] = slice(0, n)
    return out[tuple(sl)]


def expand(u, h, w):
    """[..., (h + 1) / 2, (w + 1) / 2] -> [..., h, w]: along x, then along y."""
    return _expand1(_expand1(u, w, -1), h, -2)


def decisions(P):
    """-> valid [V,hc,wc] bool, union [hc,wc] bool, owner [hc,wc] int."""
    valid = P[:, 4] >= 0.5
    union = valid.any(0)
    owner = np.argmax(np.where(valid, P[:, 3].astype(np.float64), -np.inf), axis=0)          # first of equal maxima
    return valid, union, np.where(union, owner, 0)


def filled(P, dtype=np.float64):
    """-> c' [V,3,hc,wc], s [V,hc,wc] in `dtype`, union."""
    valid, union, owner = decisions(P)
    v = P.shape[0]
    c = P[:, :3].astype(dtype)
    co = np.take_along_axis(c, np.broadcast_to(owner[None, None], (1,) + c.shape[1:]), axis=0)[0]
    co = np.where(union[None], co, dtype(0))
    cf = np.where(valid[:, None], c, co[None])
    s = (owner[None] == np.arange(v)[:, None, None]).astype(dtype)
    return cf, s, union


def blend(P, bands=5, dtype=np.float64, raw=False):
    """P [V,5,hc,wc] -> out [3,hc,wc] in `dtype` (raw=True: also r_0 before the clamp and the union)."""
    P = np.asarray(P)
    hc, wc = P.shape[-2:]
    sizes = level_sizes(hc, wc, bands)
    cf, s, union = filled(P, dtype)
    gc, gs = [cf], [s]
    for _ in range(bands):
        gc.append(reduce(gc[-1]))
        gs.append(reduce(gs[-1]))

    def fuse(lap, wgt):
        r = wgt[0][None] * lap[0]
        for v in range(1, lap.shape[0]):
            r = r + wgt[v][None] * lap[v]
        return r
    r = fuse(gc[bands], gs[bands])
    for l in range(bands - 1, -1, -1):
        h, w = sizes[l]
        r = fuse(gc[l] - expand(gc[l + 1], h, w), gs[l]) + expand(r, h, w)
    out = np.where(union[None], np.minimum(np.maximum(r, dtype(0)), dtype(255)), dtype(0)).astype(dtype)
    return (out, r, union) if raw else out


# ------------------------------------------------------------------------------------------------ inputs of the tests
# frame h, w, canvas hc, wc: odd at every level, even and then odd, narrower than any tile
CASES = [(72, 96, 80, 120), (72, 96, 81, 129), (72, 96, 85, 191), (72, 96, 84, 128), (72, 96, 87, 65), (36, 48, 43, 67)]
MADE_UP = ('hole', 'empty', 'disjoint')


def stack5(U3, h, w):
    """[V,3,h,w] colour planes -> [V,5,h,w] with the weight plane and a ones plane: warped by a sampler, this is P."""
    v = U3.shape[0]
    U = np.empty((v, 5, h, w), np.float32)
    U[:, :3] = U3
    U[:, 3] = weight_plane(h, w)
    U[:, 4] = 1.0
    return U


def made_up(kind, views, hc, wc, seed=0):
    """P [V,5,hc,wc] without a warp: uniform-noise colours (the worst case for the roundings), weight planes without ties, and masks
    with fractional rims around 0.5 and
      'hole':     a rectangle missing inside view 0, where another view or nobody covers it;
      'empty':    view 1 has no valid pixel at all;
      'disjoint': the views do not touch, with uncovered canvas between them."""
    rs = np.random.RandomState(77 + seed + 3 * hc + 5 * wc + 11 * views)
    P = np.zeros((views, 5, hc, wc), np.float32)
    P[:, :3] = rs.uniform(0, 255, (views, 3, hc, wc))
    yy, xx = np.meshgrid(np.arange(hc), np.arange(wc), indexing='ij')
    for v in range(views):
        cx, cy = wc * (v + 1.0) / (views + 1.0), hc * (0.4 + 0.1 * v)
        P[v, 3] = (np.maximum(wc - np.abs(xx - cx), 0) * np.maximum(hc - np.abs(yy - cy), 0) + 0.25 * v + 0.125).astype(np.float32)
    m = np.zeros((views, hc, wc), np.float32)
    if kind == 'disjoint':
        band = wc // (2 * views)
        for v in range(views):
            m[v, 2:hc - 3, 2 * v * band + 1:2 * v * band + band] = 1.0
    else:
        m[0, :, :2 * wc // 3] = 1.0
        m[0, hc // 4:hc // 2, wc // 6:wc // 2] = 0.0                     # the hole: its right part lies inside view 1
        m[1, hc // 8:, wc // 3:] = 1.0
        if views == 3:
            m[2, hc // 2:, :] = 1.0
        if kind == 'empty':
            m[1] = 0.0
    rim = rs.uniform(0, 1, m.shape) < 0.05                               # fractional values on both sides of the threshold
    m = np.where(rim & (m > 0), rs.choice(np.array([0.5, 0.51, 0.75], np.float32), m.shape), m)
    m = np.where(rim & (m == 0), rs.choice(np.array([0.0, 0.49, 0.25], np.float32), m.shape), m)
    P[:, 4] = m
    return P


# canvases (hc, wc) down to one pixel: one row, one column, the smallest legal reduce (3 -> 2), a 2 x 2 level at the top of a pyramid
# (4 x 4, 5 x 5 through 3 x 3, 6 x 7 through 3 x 4), one tile wide and three pixels high and the other way round
SMALL = [(1, 1), (1, 9), (9, 1), (2, 2), (2, 67), (3, 3), (4, 4), (5, 5), (6, 7), (3, 130), (130, 3)]


def small_case(views, hc, wc, seed=0):
    """P [V,5,hc,wc] for the canvases of SMALL: uniform-noise colours; weights a permutation of 1..V hc wc (no two equal, so every
    owner decision is between different numbers); masks Bernoulli(0.7), a quarter of them moved to made_up's fractional values on
    their own side of 0.5.  From 2 x 2 upwards one entry is set valid and one invalid, so that both occur whatever the draw."""
    rs = np.random.RandomState(911 + seed + 7 * hc + 13 * wc + 31 * views)
    P = np.zeros((views, 5, hc, wc), np.float32)
    P[:, :3] = rs.uniform(0, 255, (views, 3, hc, wc))
    P[:, 3] = (rs.permutation(views * hc * wc) + 1).reshape(views, hc, wc)
    m = (rs.uniform(0, 1, (views, hc, wc)) < 0.7).astype(np.float32)
    if hc >= 2 and wc >= 2:
        m[0, 0, 0], m[0, -1, -1] = 1.0, 0.0
    rim = rs.uniform(0, 1, m.shape) < 0.25
    hi, lo = rs.choice(np.array([0.5, 0.51, 0.75], np.float32), m.shape), rs.choice(np.array([0.0, 0.49, 0.25], np.float32), m.shape)
    P[:, 4] = np.where(rim, np.where(m > 0, hi, lo), m)
    return P


def tied(P):
    """A copy of P whose weight planes are equal in all views on the left half of the canvas (view 0's): where several views are valid
    there the owner is the first of equal maxima.  -> (P, the pixels [hc,wc] where at least two valid views tie for the maximum)."""
    P = P.copy()
    wc = P.shape[-1]
    P[1:, 3, :, :wc // 2] = P[0, 3, :, :wc // 2]
    valid = P[:, 4] >= 0.5
    w = np.where(valid, P[:, 3].astype(np.float64), -np.inf)
    at_max = valid & (w == w.max(0)[None])
    return P, at_max.sum(0) >= 2


def side_by_side(h=80, w=200, lo=60, hi=140, a=100.0, b=140.0):
    """Two constant views on an h x w canvas overlapping in columns lo..hi-1, each weighted by the weight plane of its own footprint."""
    P = np.zeros((2, 5, h, w), np.float32)
    P[0, :3], P[1, :3] = a, b
    P[0, 3, :, :hi] = weight_plane(h, hi)
    P[1, 3, :, lo:] = weight_plane(h, w - lo)
    P[0, 4, :, :hi] = 1.0
    P[1, 4, :, lo:] = 1.0
    return P


def roundings(bands, views):
    """Count of fp32 roundings, in units of u * 255, that can reach one pixel of blend(P, bands, float32) for colours in 0..255.
    Reduce and expand are convex combinations, so an error made above a level is carried down without growing; each rounding is at most
    u times the size of its result.
      a 1-D reduce: four sums and the product by 6 (the products by 4 and by 1/16 are exact): 5, so G_l carries 10 l;
      a 1-D expand: even outputs two sums and the product by 6, odd outputs one sum: <= 3, so 6 per expand;
      a Laplacian at level l, |L| <= 2 * 255: G_l (10 l) + G_{l+1} (10 (l + 1)) + the expand (6) + the difference (2) = 20 l + 18;
      its weights, in 0..1: 10 l roundings of size u each, times |L| <= 2 * 255: 20 l per view;
      the products w L: u |w L| each, and sum_v w_v |L_v| <= 2 * 255: 2; the V - 1 sums of the fuse, of results <= 2 * 255: 2 (V - 1);
      per level below the bottom: the expand of r (|r| <= 2 * 255 with the overshoot: 12) and the sum with it (2): 14;
      4 on top for the forms that start from differences of the filled views (the difference, the final sum with the last view)."""
    n = 4 + 14 * bands
    for l in range(bands + 1):
        n += (20 * l + 18) + 20 * l * views + 2 + 2 * (views - 1)
    return n


def bound(bands, views):
    """E(B): the most a pixel of an fp32 evaluation may differ from blend(P, B, float64), in grey levels."""
    return U32 * 255.0 * roundings(bands, views)
