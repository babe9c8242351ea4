"""The content-aware seam of MULTIBAND fusion, stated as an integer and fp32 program in numpy.  The kernels of
libstabstitch_seam.so (stabstitch2_amd/csrc/seam.hip) are held to it bit for bit: the per-pixel cost is fp32 with one rounding per
operation, everything after it is integer arithmetic, so no result depends on the order of a sum.

    seam(P, cell, mu, prior, state)   the program: cost planes, view order, seams, painted weights, the state after the call
    optimum(Ep)                       independently: the minimal cost of a top-to-bottom path, a plain int64 recurrence that returns no path

Definitions (P [n][V][5][hc][wc] fp32 as the warp writes it: B, G, R, the warped weight plane W, the ones-mask; valid = mask >= 0.5):
  cells     hq = ceil(hc / c), wq = ceil(wc / c); the last row and column of cells may be partial
  order     per view the first and last canvas column with a valid pixel; key = xmin + xmax (a view without one: +inf); the views sorted
            by (key, index); seams run top to bottom between neighbours of that order
  pixel     for a pair (a, b), where both are valid:  t = (Wa + Wb) > 0 ? |Wa - Wb| / (Wa + Wb) : 0,
            d = min(765, (int)((|Ba - Bb| + |Ga - Gb|) + |Ra - Rb|)) + (int)(prior * t)            (truncations)
  cell      D = sum of d, nb = count over the cell's both-valid pixels; E = nb > 0 ? (D * c * c) / nb : NONE
            a row of cells without any overlap cell is free (E = 0 throughout); elsewhere NONE costs PEN = 1 << 19
  temporal  + min(mu * |x - xprev[y]|, 1 << 18) on every cell of row y when the state holds a seam of this pair on this grid and order
  dp        M[0][x] = E'[0][x];  M[y][x] = min(E'[y][x] + min(M[y-1][x-1], M[y-1][x], M[y-1][x+1]), 1 << 30), neighbours outside the row
            left out, a tie taken straight, then left, then right; the end point is the lowest x that minimises the last row
  labels    cell cx of row y is left of the seam when cx <= x(y).  Three views: two seams found independently, the second raised to
            max(x12, x01); label = (cx > x01) + (cx > x12)
  paint     plane 3 of the view at place k of the order becomes V - |k - label| at every pixel of the cell
  state     int32 [16 + (V - 1) * hq]: per seam a header of 8 {valid, V, hq, wq, c, order[3] (-1 past V)} at 8 * p, then xprev [V - 1][hq]
            (each seam as the dp found it, before the second is raised).  A frame whose grid or order differs from the stored one runs
            without the temporal term; either way the state is overwritten.  All zero = fresh."""
import numpy as np

PEN = 1 << 19
TCAP = 1 << 18
MCAP = 1 << 30
NONE = -1
HEADER = 16
INF = np.iinfo(np.int32).max
LDS_BYTES = 163840
CELLS = (1, 2, 4, 8, 16)


def grid(hc, wc, c):
    return -(-hc // c), -(-wc // c)


def lds_bytes(hc, wc, c):
    """What the dp's workgroup keeps in LDS: 16 ints, two rows of M, three columns of hq ints, 2 bits per cell."""
    hq, wq = grid(hc, wc, c)
    wq4 = (wq + 3) & ~3
    return 4 * (16 + 2 * wq4 + 3 * hq) + hq * wq4 // 4


def workspace_bytes(frames, views, hc, wc, c):
    """The formula of include/stabstitch_seam.h; -1 where the library refuses."""
    if not (1 <= frames <= 65535 and views in (2, 3) and 1 <= hc <= 32768 and 1 <= wc <= 32768 and c in CELLS):
        return -1
    if lds_bytes(hc, wc, c) > LDS_BYTES:
        return -1
    hq, wq = grid(hc, wc, c)
    wq4 = (wq + 3) & ~3
    gx = -(-wc // 256)
    nblk = gx * -(-hc // max(4, c))
    return 4 * frames * (views * (views - 1) // 2 * (3 * hq * wq4 + hq * gx) + nblk * views * 2 + (views - 1) * hq + 8)


def default_cell(hc, wc):
    for c in (4, 8, 16):
        if lds_bytes(hc, wc, c) <= LDS_BYTES:
            return c
    raise ValueError('no cell fits')


def pairs(views):
    return [(a, b) for a in range(views) for b in range(a + 1, views)]


def pair_index(a, b, views):
    lo, hi = min(a, b), max(a, b)
    return 0 if views == 2 else lo + hi - 1


def pixel_cost(Pa, Pb, prior):
    """[5,hc,wc] x 2 -> d int32 [hc,wc] (meaningless where a view is invalid), both [hc,wc] bool."""
    f = np.float32
    Pa, Pb = Pa.astype(f), Pb.astype(f)
    dc = (np.abs(Pa[0] - Pb[0]) + np.abs(Pa[1] - Pb[1])) + np.abs(Pa[2] - Pb[2])
    s = Pa[3] + Pb[3]
    pos = s > 0
    t = np.where(pos, np.abs(Pa[3] - Pb[3]) / np.where(pos, s, f(1)), f(0)).astype(f)
    both = (Pa[4] >= 0.5) & (Pb[4] >= 0.5)
    d = np.minimum(765, np.where(both, dc, f(0)).astype(np.int32)) + np.where(both, f(prior) * t, f(0)).astype(np.int32)
    return d.astype(np.int32), both


def cell_cost(d, both, c):
    """-> D, nb, E int32 [hq,wq] (E = NONE where nb = 0)."""
    hc, wc = d.shape
    hq, wq = grid(hc, wc, c)
    pad = lambda a: np.pad(a, ((0, hq * c - hc), (0, wq * c - wc)))
    D = pad(np.where(both, d, 0).astype(np.int64)).reshape(hq, c, wq, c).sum((1, 3))
    nb = pad(both.astype(np.int64)).reshape(hq, c, wq, c).sum((1, 3))
    E = np.where(nb > 0, (D * c * c) // np.maximum(nb, 1), NONE)
    return D.astype(np.int32), nb.astype(np.int32), E.astype(np.int32)


def view_order(P):
    """P [V,5,hc,wc] -> the views sorted by (xmin + xmax, index), a view without a valid pixel last."""
    keys = []
    for v in range(P.shape[0]):
        cols = np.flatnonzero((P[v, 4] >= 0.5).any(0))
        keys.append((int(cols[0] + cols[-1]) if cols.size else INF, v))
    return [v for _, v in sorted(keys)]


def energy(E, xprev=None, mu=0):
    """E [hq,wq] with NONE -> E' int64: free rows, the penalty, the temporal term."""
    hq, wq = E.shape
    anyrow = (E >= 0).any(1)
    Ep = np.where(anyrow[:, None], np.where(E >= 0, E, PEN), 0).astype(np.int64)
    if xprev is not None:
        x = np.arange(wq, dtype=np.int64)[None, :]
        Ep = Ep + np.minimum(int(mu) * np.abs(x - np.asarray(xprev, np.int64)[:, None]), TCAP)
    return Ep


def dp(Ep):
    """E' [hq,wq] -> (x(y) int32 [hq], the seam's cost): the recurrence and the tie rules of the definition."""
    hq, wq = Ep.shape
    M = Ep[0].copy()
    back = np.zeros((hq, wq), np.int8)
    big = np.int64(1) << 62
    for y in range(1, hq):
        left = np.concatenate(([big], M[:-1]))
        right = np.concatenate((M[1:], [big]))
        best, code = M.copy(), np.zeros(wq, np.int8)
        m = left < best
        best, code = np.where(m, left, best), np.where(m, 1, code)
        m = right < best
        best, code = np.where(m, right, best), np.where(m, 2, code)
        M = np.minimum(Ep[y] + best, MCAP)
        back[y] = code
    x = int(np.argmin(M))                                  # the first of equal minima
    cost = int(M[x])
    xs = np.empty(hq, np.int32)
    xs[hq - 1] = x
    for y in range(hq - 1, 0, -1):
        x += (0, -1, 1)[back[y, x]]
        xs[y - 1] = x
    return xs, cost


def optimum(Ep):
    """The minimal sum of E' along a path that moves at most one cell sideways per row -- computed bottom-up in int64 without back
    pointers, tie rules or the cap (so it equals dp()'s cost while that stays below 1 << 30)."""
    Ep = np.asarray(Ep, np.int64)
    best = Ep[-1].copy()
    for y in range(Ep.shape[0] - 2, -1, -1):
        pad = np.pad(best, 1, constant_values=np.iinfo(np.int64).max)
        best = Ep[y] + np.minimum(np.minimum(pad[:-2], pad[1:-1]), pad[2:])
    return int(best.min())


def path_cost(Ep, xs):
    return int(sum(int(Ep[y, x]) for y, x in enumerate(xs)))


def labels(seams, wq):
    """seams [V-1][hq] -> label [hq,wq]."""
    cx = np.arange(wq)[None, :]
    x01 = np.asarray(seams[0])[:, None]
    lab = (cx > x01).astype(np.int32)
    if len(seams) == 2:
        lab += cx > np.maximum(np.asarray(seams[1])[:, None], x01)
    return lab


def paint(P, order, seams, c):
    """P [V,5,hc,wc] -> a copy with plane 3 of every view painted."""
    V, _, hc, wc = P.shape
    hq, wq = grid(hc, wc, c)
    lab = np.repeat(np.repeat(labels(seams, wq), c, 0), c, 1)[:hc, :wc]
    out = P.copy()
    for k, v in enumerate(order):
        out[v, 3] = (V - np.abs(k - lab)).astype(np.float32)
    return out


def fresh_state(views, hc, wc, c):
    return np.zeros(HEADER + (views - 1) * grid(hc, wc, c)[0], np.int32)


def seam(P, cell, mu, prior, state=None):
    """The program.  P [n,V,5,hc,wc] (or [V,5,hc,wc]) -> dict: 'P' painted copy, 'cost' [n][NP] of (D, nb, E), 'order' [n] lists,
    'seams' int32 [n,V-1,hq], 'seam_cost' [n][V-1], 'energy' [n][V-1] the E' each seam was found on.  state: None, or the int32 array,
    advanced IN PLACE through the frames in order."""
    P = np.asarray(P, np.float32)
    single = P.ndim == 4
    P = P[None] if single else P
    n, V, _, hc, wc = P.shape
    hq, wq = grid(hc, wc, cell)
    res = dict(P=np.empty_like(P), cost=[], order=[], seams=np.zeros((n, V - 1, hq), np.int32), seam_cost=[], energy=[])
    for f in range(n):
        cost = []
        for a, b in pairs(V):
            d, both = pixel_cost(P[f, a], P[f, b], prior)
            cost.append(cell_cost(d, both, cell))
        order = view_order(P[f])
        packed = order + [-1] * (3 - V)
        sc, en = [], []
        for p in range(V - 1):
            xprev = None
            if state is not None:
                hdr = state[8 * p:8 * p + 8]
                if hdr.tolist() == [1, V, hq, wq, cell] + packed:
                    xprev = state[HEADER + p * hq:HEADER + (p + 1) * hq].copy()
            Ep = energy(cost[pair_index(order[p], order[p + 1], V)][2], xprev, mu)
            xs, c = dp(Ep)
            res['seams'][f, p] = xs
            sc.append(c)
            en.append(Ep)
            if state is not None:
                state[8 * p:8 * p + 8] = [1, V, hq, wq, cell] + packed
                state[HEADER + p * hq:HEADER + (p + 1) * hq] = xs
        res['P'][f] = paint(P[f], order, res['seams'][f], cell)
        res['cost'].append(cost)
        res['order'].append(order)
        res['seam_cost'].append(sc)
        res['energy'].append(en)
    if single:
        res['P'] = res['P'][0]
    return res


# ------------------------------------------------------------------------------------------------ inputs of the tests
def weight_plane(h, w):
    x, y = np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32)
    return (np.minimum(x + 1, w - x)[None, :] * np.minimum(y + 1, h - y)[:, None]).astype(np.float32)


def texture(hc, wc, seed=0):
    """Smooth colours [3,hc,wc] in 0..255 that both views of a made-up scene share."""
    yy, xx = np.meshgrid(np.arange(hc, dtype=np.float32), np.arange(wc, dtype=np.float32), indexing='ij')
    return np.stack([np.float32(128) + np.float32(100) * np.sin((xx * (k + 2) + yy * (3 - k) + seed) / np.float32(17)) for k in range(3)]) \
        .astype(np.float32)


def side_by_side(hc, wc, lo, hi, colours=None, seed=0):
    """Two views of ONE picture on an hc x wc canvas: view 0 covers columns 0..hi-1, view 1 columns lo..wc-1, each weighted by the
    weight plane of its own footprint -> P [2,5,hc,wc].  The geometric seam runs down the middle of columns lo..hi-1."""
    P = np.zeros((2, 5, hc, wc), np.float32)
    P[:, :3] = texture(hc, wc, seed) if colours is None else colours
    P[0, 3, :, :hi] = weight_plane(hc, hi)
    P[1, 3, :, lo:] = weight_plane(hc, wc - lo)
    P[0, 4, :, :hi] = 1.0
    P[1, 4, :, lo:] = 1.0
    P[0, :4, :, hi:] = 0.0
    P[1, :4, :, :lo] = 0.0
    return P


def mismatch(hc, wc, lo, hi, rect, seed=0, colour=(250.0, 5.0, 250.0)):
    """side_by_side where view 1 shows another colour in the rectangle rect = (y0, y1, x0, x1): an object only one camera saw there."""
    P = side_by_side(hc, wc, lo, hi, seed=seed)
    y0, y1, x0, x1 = rect
    P[1, :3, y0:y1, x0:x1] = np.asarray(colour, np.float32)[:, None, None]
    return P


def cap_scene():
    """P [2,2,5,4200,8], two frames for one call at cell 1, mu = 65535: colours texture (+7 in view 1), each view weighted by the
    weight plane of its own footprint.  Frame 0: view 0 on columns 0..1, view 1 on 0..7; frame 1: view 0 on 0..7, view 1 on 6..7 --
    held to frame 0's seam six columns from its own overlap, M reaches the cap 1 << 30 some 4000 rows down."""
    hc, wc = 4200, 8
    P = np.zeros((2, 2, 5, hc, wc), np.float32)
    colours = texture(hc, wc)
    spans = [[(0, 2), (0, 8)], [(0, 8), (6, 8)]]                              # [frame][view] -> its valid columns
    for f in range(2):
        for v in range(2):
            a, b = spans[f][v]
            P[f, v, :3, :, a:b] = (colours + np.float32(7 * v))[:, :, a:b]
            P[f, v, 3, :, a:b] = weight_plane(hc, b - a)
            P[f, v, 4, :, a:b] = 1.0
    return P


def geometric_owner(P):
    """The owner map the blend derives from plane 3 (the valid view with the largest weight, the lowest index among equals)."""
    valid = P[:, 4] >= 0.5
    owner = np.argmax(np.where(valid, P[:, 3].astype(np.float64), -np.inf), axis=0)
    return np.where(valid.any(0), owner, 0)
