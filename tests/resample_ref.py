"""The fixed-size output of a rectangle (libstabstitch_resample.so), stated in numpy: the float64 definition the kernels
are held to, a sequential fp32 restatement of the kernel's own arithmetic, and the gate between the two.  A plain helper module.

Definition (include/stabstitch_resample.h has the same text).  rect (y0, x0, h, w) is intersected with the Hc x Wc frame: R; an empty
R gives black (0.0, bytes 0, Y 16 / U = V = 128).  The window is R ('stretch') or the centred part of R with the output's aspect
('fill'), in double, one operation after the other.  Per axis, window [o, o + len) over n_out outputs, R's range [lo, hi):
scale = len / n_out, support = max(scale, 1), c_i = o + scale (i + 0.5), taps j in [max(lo, floor(c_i - support + 0.5)),
min(hi, floor(c_i + support + 0.5))), weight max(0, 1 - |j + 0.5 - c_i| / support) divided by the sum over the taps kept (ascending)."""
import math

import numpy as np

import nv12_ref as NV

FRAME = (43, 67)
# (rectangle, what it exercises); the last but one overhangs the frame, the last is empty
RECTS = [(5, 7, 30, 50), (0, 0, 43, 67), (13, 17, 30, 50), (5, 7, 1, 1), (5, 7, 2, 2), (0, 0, 43, 1), (40, 60, 30, 50), (5, 7, 0, 9)]
SIZES = [(30, 50), (16, 24), (69, 115), (4, 7), (2, 2), (31, 64), (32, 65), (16, 22)]
ASPECTS = ('fill', 'stretch')
# the kernel's staged path: both supports <= 5 (2 * support + 2 <= 12 table entries) and the tap rows of a 16-row tile <= 48
STAGED_K, STAGED_ROWS, TILE_H = 12, 48, 16


def clip(rect, Hc, Wc):
    """R = rect intersected with the frame -> (ya, xa, yb, xb) or None when empty."""
    y0, x0, h, w = (int(v) for v in rect)
    ya, xa, yb, xb = max(y0, 0), max(x0, 0), min(y0 + h, Hc), min(x0 + w, Wc)
    if h <= 0 or w <= 0 or yb <= ya or xb <= xa:
        return None
    return ya, xa, yb, xb


def window(rect, Hc, Wc, Hout, Wout, aspect):
    """(fy, fx, fh, fw) as Python floats (doubles), zeros for an empty R: the rule of the header, operation for operation."""
    R = clip(rect, Hc, Wc)
    if R is None:
        return 0.0, 0.0, 0.0, 0.0
    ya, xa, yb, xb = R
    rh, rw = yb - ya, xb - xa
    fy, fx, fh, fw = float(ya), float(xa), float(rh), float(rw)
    if aspect == 'fill':
        if rw * Hout > rh * Wout:
            fw = float(rh) * float(Wout) / float(Hout)
            fx = float(xa) + (float(rw) - fw) / 2.0
        elif rw * Hout < rh * Wout:
            fh = float(rw) * float(Hout) / float(Wout)
            fy = float(ya) + (float(rh) - fh) / 2.0
    else:
        assert aspect == 'stretch'
    return fy, fx, fh, fw


def taps(o, length, n_out, lo, hi):
    """One axis -> list over the outputs of (t0, float64 weights of taps t0 .. t0 + len - 1, normalised)."""
    scale = length / float(n_out)
    support = scale if scale > 1.0 else 1.0
    out = []
    for i in range(n_out):
        c = o + scale * (float(i) + 0.5)
        t0 = int(max(math.floor((c - support) + 0.5), float(lo)))
        t1 = int(min(math.floor((c + support) + 0.5), float(hi)))
        w = [max(0.0, 1.0 - abs((float(j) + 0.5) - c) / support) for j in range(t0, t1)]
        s = 0.0
        for v in w:                      # ascending, as the kernel adds them
            s += v
        out.append((t0, np.array([v / s for v in w], dtype=np.float64)))
    return out


def axes(rect, Hc, Wc, Hout, Wout, aspect):
    """-> (row taps, column taps) or None for an empty R."""
    R = clip(rect, Hc, Wc)
    if R is None:
        return None
    fy, fx, fh, fw = window(rect, Hc, Wc, Hout, Wout, aspect)
    return taps(fy, fh, Hout, R[0], R[2]), taps(fx, fw, Wout, R[1], R[3])


def tap_counts(rect, Hc, Wc, Hout, Wout, aspect):
    """(ky, kx): the most taps any output has per axis; (0, 0) for an empty R."""
    ax = axes(rect, Hc, Wc, Hout, Wout, aspect)
    if ax is None:
        return 0, 0
    return max(len(w) for _, w in ax[0]), max(len(w) for _, w in ax[1])


def staged(rect, Hc, Wc, Hout, Wout, aspect):
    """Does every tile of the kernel take the staged path (True), none (False), or some (None)?  The kernel's own rule."""
    R = clip(rect, Hc, Wc)
    if R is None:
        return False
    fy, fx, fh, fw = window(rect, Hc, Wc, Hout, Wout, aspect)
    if 2.0 * max(fh / Hout, 1.0) + 2.0 > STAGED_K or 2.0 * max(fw / Wout, 1.0) + 2.0 > STAGED_K:
        return False
    ty = taps(fy, fh, Hout, R[0], R[2])
    fits = []
    for t in range(0, Hout, TILE_H):
        last = min(t + TILE_H, Hout) - 1
        fits.append(ty[last][0] + len(ty[last][1]) - ty[t][0] <= STAGED_ROWS)
    return True if all(fits) else False if not any(fits) else None


def _matrix(tp, n_in, dtype=np.float64):
    M = np.zeros((len(tp), n_in), dtype=dtype)
    for i, (t0, w) in enumerate(tp):
        M[i, t0:t0 + len(w)] = w
    return M


def resample(planes, size, rect, aspect='fill'):
    """planes [..., Hc, Wc] (any leading axes) -> float64 [..., Hout, Wout]: the definition."""
    planes = np.asarray(planes, dtype=np.float64)
    Hc, Wc = planes.shape[-2:]
    Hout, Wout = size
    ax = axes(rect, Hc, Wc, Hout, Wout, aspect)
    if ax is None:
        return np.zeros(planes.shape[:-2] + (Hout, Wout))
    return _matrix(ax[0], Hc) @ planes @ _matrix(ax[1], Wc).T


def to_bytes(v):
    """floor(v + 0.5), saturated: the uint8 outputs."""
    return np.clip(np.floor(np.asarray(v, dtype=np.float64) + 0.5), 0, 255).astype(np.uint8)


def resample_u8(frames, size, rect, aspect='fill'):
    """uint8 [n,Hc,Wc,3] -> (uint8 [n,Hout,Wout,3], the float64 values [n,Hout,Wout,3] they were rounded from)."""
    v = resample(np.moveaxis(np.asarray(frames), -1, -3), size, rect, aspect)
    v = np.moveaxis(v, -3, -1)
    return to_bytes(v), v


def nv12(bgr_bytes):
    """uint8 [n,H,W,3] -> NV12 [n,H*3/2,W] through tests/nv12_ref.py."""
    return np.stack([NV.bgr_to_nv12(f) for f in bgr_bytes])


# ---- the sequential fp32 restatement: the kernel's arithmetic, operation for operation
def fmaf(a, b, c):
    """fp32 fma of fp32 arrays, exactly: a * b is exact in float64 (24 + 24 bits), the float64 sum is rounded once and its error e is
    known (TwoSum), and rounding that sum to fp32 differs from rounding the true value only where the float64 sum sits exactly on an
    fp32 midpoint while e != 0: there e decides the direction."""
    a, b, c = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (a, b, c))
    s = a * b
    t = s + c
    bb = t - s
    e = (s - (t - bb)) + (c - bb)
    r = t.astype(np.float32)
    r64 = r.astype(np.float64)
    up = np.nextafter(r, np.float32(np.inf)).astype(np.float64)
    dn = np.nextafter(r, np.float32(-np.inf)).astype(np.float64)
    fix_up = (r64 < t) & (e > 0) & ((t - r64) == (up - t))
    fix_dn = (r64 > t) & (e < 0) & ((r64 - t) == (t - dn))
    return np.where(fix_up, up, np.where(fix_dn, dn, r64)).astype(np.float32)


def resample_f32_sequential(planes, size, rect, aspect='fill'):
    """planes [..., Hc, Wc] with fp32-exact values -> fp32 [..., Hout, Wout] as the kernel computes it: the double weights rounded to
    fp32 once; per output row its tap rows in ascending order, for each the horizontal sum hrow = fmaf(wx_k, pixel_k, hrow) over
    ascending k from 0, then acc = fmaf(wy_j, hrow, acc) from 0.  numpy has no fmaf: `fmaf` above restates it exactly."""
    planes = np.asarray(planes, dtype=np.float32)
    Hc, Wc = planes.shape[-2:]
    Hout, Wout = size
    lead = planes.shape[:-2]
    ax = axes(rect, Hc, Wc, Hout, Wout, aspect)
    out = np.zeros(lead + (Hout, Wout), dtype=np.float32)
    if ax is None:
        return out
    ty, tx = ax
    kx = max(len(w) for _, w in tx)
    x0 = np.array([t0 for t0, _ in tx])
    cn = np.array([len(w) for _, w in tx])
    wx = np.zeros((kx, Wout), dtype=np.float32)
    for i, (_, w) in enumerate(tx):
        wx[:len(w), i] = w.astype(np.float32)
    # the horizontal pass of every source row any output row reads, tap by tap (a tap past a column's count: weight 0 would still
    # round-trip through fmaf unchanged -- h + 0 * p == h -- so the padded taps change nothing)
    rows = sorted({j for t0, w in ty for j in range(t0, t0 + len(w))})
    hrow = {}
    for j in rows:
        h = np.zeros(lead + (Wout,), dtype=np.float32)
        for k in range(kx):
            xi = np.minimum(x0 + k, Wc - 1)
            h = np.where(k < cn, fmaf(wx[k], planes[..., j, xi], h), h)
        hrow[j] = h
    for i, (t0, w) in enumerate(ty):
        acc = np.zeros(lead + (Wout,), dtype=np.float32)
        for j, wj in enumerate(w.astype(np.float32)):
            acc = fmaf(wj, hrow[t0 + j], acc)
        out[..., i, :] = acc
    return out


def bound(ky, kx):
    """The gate |fp32 result - float64 definition| <= bound, for values in 0 .. 255, from the arithmetic alone: u = 2^-24 is the unit
    roundoff of fp32.  Each axis's weights are rounded once (relative u each; they sum to 1, so at most 255 u per axis: 2), the
    horizontal chain rounds kx partial sums and the vertical one ky, each partial sum at most 255 (1 + small) (255 u each: kx + ky),
    and one more 255 u (c = 3 in all) covers the second-order terms and the rounded weights' sum differing from 1 by up to k u."""
    return 255.0 * (ky + kx + 3) * 2.0 ** -24
