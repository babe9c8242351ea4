"""FEATHER fusion (SS_FUSE_FEATHER, include/stabstitch_hip.h) stated for the tests: in float64 on ref64's spline and samplers, as an
fp32 numpy program in the kernel's order of operations, and the per-pixel bound between a float64 statement and any fp32 reading of
it.  Not the reference's: the definition is the header's.

    w_v = max(min(1 - |xn_v|, 1 - |yn_v|), 0);  out = sum_v w_v c_v / sum_v w_v where the sum of weights is positive, else 0

with (xn_v, yn_v) view v's normalised sampling coordinate at the canvas pixel and c_v what the render's sampler returns there
(NORMAL: ref64.bilinear_clamped, FAST: ref64.grid_sample_zeros), after min(g c, 255) where gains are given."""
import numpy as np

import ref64 as R
import sweep_inputs as G

F32 = np.float32
COORD_GATE = G.WARP_COORD_GATE      # the coordinate gate of test_tps_dense_warp_against_fp64, normalised: what a weight may be off by
R_MIN = 1e-4                        # |min(1 - |xn|, 1 - |yn|)| below this: the fp32 decision w > 0 may differ -- pixel left out
DEN_MIN = 1e-3                      # 0 < den below this: left out
ULP255 = float(np.spacing(F32(255.0)))


def border_distance(xn, yn):
    """r = min(1 - |xn|, 1 - |yn|) in the dtype of the coordinates: the weight before its clamp at 0 (negative outside the image)."""
    one = xn.dtype.type(1)
    return np.minimum(one - np.abs(xn), one - np.abs(yn))


def fuse(c, w):
    """c [V,C,...], w [V,...] -> (out [C,...], den [...]) in the dtype of the operands and the fixed order: num = ((w0 c0) + (w1 c1))
    [+ (w2 c2)], den = (w0 + w1) [+ w2], one rounding per operation; out = num / den where den > 0, else 0."""
    num, den = w[0][None] * c[0], w[0]
    for v in range(1, c.shape[0]):
        num = num + w[v][None] * c[v]
        den = den + w[v]
    ok = den > 0
    out = np.where(ok[None], num / np.where(ok, den, den.dtype.type(1))[None], num.dtype.type(0))
    return out.astype(c.dtype), den


def sample(U, xn, yn, mode, gains=None):
    """U [V,3,h,w], (xn, yn) [V,hc,wc] -> c [V,3,hc,wc] in float64: the render's sampler, then min(g c, 255) with gains [V,3]."""
    c = (R.bilinear_clamped if mode == 'NORMAL' else R.grid_sample_zeros)(U, xn, yn)
    if gains is not None:
        c = np.minimum(R.f64(gains)[:, :, None, None] * c, 255.0)
    return c


def feather64(U, source, target, hc, wc, mode, gains=None):
    """The float64 statement of one frame: U [V,3,h,w] (V = 2 | 3 views), source / target [V,63,2] the views' control points on the
    canvas / the frame -> dict(out [3,hc,wc], c [V,3,hc,wc], w, r [V,hc,wc], den [hc,wc], xn, yn)."""
    xn, yn = R.tps_dense_coords(source, R.tps_solve(source, target), hc, wc)
    c = sample(U, xn, yn, mode, gains)
    r = border_distance(xn, yn)
    w = np.maximum(r, 0.0)
    out, den = fuse(c, w)
    return dict(out=out, c=c, w=w, r=r, den=den, xn=xn, yn=yn)


def feather32(c, xn, yn):
    """The fp32 restatement: sampled channels c [V,3,hc,wc] and coordinates [V,hc,wc] of an fp32 program -> out [3,hc,wc] fp32 by
    the kernel's operations in the kernel's order."""
    c, xn, yn = np.asarray(c, F32), np.asarray(xn, F32), np.asarray(yn, F32)
    w = np.maximum(border_distance(xn, yn), F32(0))
    out, _ = fuse(c, w)
    assert out.dtype == F32 and w.dtype == F32
    return out


def left_out(ref):
    """The pixels a comparison leaves out [hc,wc]: some view within R_MIN of its image border (either side), or 0 < den < DEN_MIN."""
    return (np.abs(ref['r']) < R_MIN).any(0) | ((ref['den'] > 0) & (ref['den'] < DEN_MIN))


def sample_gate(U, ref, mode, gains=None):
    """The dense-warp sweep's own intensity gate (sweep_inputs.warp_gate: same sampler, same coordinates) for every c_v [V,3,hc,wc];
    with gains scaled by them (min(., 255) is 1-Lipschitz) plus the product's rounding."""
    _, bound, _, _, _ = G.warp_gate(np.asarray(U, F32), ref['xn'], ref['yn'], mode)
    if gains is not None:
        bound = R.f64(gains)[:, :, None, None] * bound + ULP255
    return bound


def bound(ref, cgate):
    """|fp32 reading - ref['out']| per pixel [3,hc,wc], outside left_out(ref), for a reading whose coordinates lie within COORD_GATE
    of the float64 ones and whose samples within cgate [V,3,hc,wc] of the float64 samples.  With ~ for the reading's quantities,
        out~ - out = sum_v w~_v (c~_v - c_v) / den~  +  sum_v (w~_v - w_v) (c_v - out) / den~      (sum_v w_v (c_v - out) = 0),
    and w is 1-Lipschitz in either coordinate, so |w~_v - w_v| <= dw = COORD_GATE -- except for a view with r_v <= -R_MIN, whose
    reading's weight is exactly 0 like the statement's (dw < R_MIN): such a view enters neither term.  den~ >= den - A dw with A the
    number of the other views.  Three parts:
        samples   sum_v (w_v + dw) cgate_v / (den - A dw)
        weights   sum_v |c_v - out| dw / (den - A dw)
        the fuse  8 ulp of 255: a product and V - 1 sums in num, V - 1 sums in den, the quotient -- 2 V <= 6 roundings of relative
                  size 2^-24 on values <= 255 (255 x 2^-24 is one ulp of 255), 8 with room for their compounding
    Where den = 0 (no view reaches the pixel, by more than R_MIN each) the reading is exactly 0: the bound is 0."""
    active = ref['r'] >= R_MIN                                              # [V,hc,wc]  (left_out has removed -R_MIN < r < R_MIN)
    dw = COORD_GATE
    den_lo = np.maximum(ref['den'] - active.sum(0) * dw, DEN_MIN / 2)       # (den >= DEN_MIN wherever it counts)
    a = active[:, None]
    samples = (np.where(a, (ref['w'][:, None] + dw) * cgate, 0.0)).sum(0)
    weights = (np.where(a, np.abs(ref['c'] - ref['out'][None]) * dw, 0.0)).sum(0)
    b = (samples + weights) / den_lo[None] + 8.0 * ULP255
    return np.where((ref['den'] > 0)[None], b, 0.0)


def worst(got, ref, U, mode, gains=None, cap=0.01):
    """A reading `got` [3,hc,wc] of the statement `ref` (feather64) -> (worst |got - out| / bound over the compared pixels, the share
    of the canvas left out).  More than `cap` of the canvas left out is a failure of the case, not of the reading."""
    out_px = left_out(ref)
    share = float(out_px.mean())
    assert share <= cap, 'the comparison leaves out %.2f %% of the canvas (cap %.2f %%)' % (100 * share, 100 * cap)
    b = bound(ref, sample_gate(U, ref, mode, gains))
    d = np.abs(R.f64(got) - ref['out'])
    keep = np.broadcast_to(~out_px[None], d.shape)
    assert np.isfinite(R.f64(got)).all()
    exact = keep & (b == 0)
    assert (d[exact] == 0).all(), 'a pixel no view reaches is not 0'
    ratio = np.where(keep & (b > 0), d / np.where(b > 0, b, 1.0), 0.0)
    return float(ratio.max()), share
