"""The convolution engine (conv.hip, stem.hip, wino.hip, wino43.hip) against the float64 statements of tests/ref64.py, with one case or
more for every kernel instantiation the shipped library carries: the three implicit-GEMM tiles, the four address modes, the TAIL
variants, every kind of split-K plan and its reduction (with residual, with the 2 x 2 pool, with a padded output pitch), groups,
SmoothNet's 3-D convolutions, the stem kernels, F(2x2,3x3) on both block shapes (fp32, bf16x9, pool epilogue) and F(4x4,3x3) on both
block geometries.  The library has no knobs: a path is reached by a shape that takes it, the arithmetic that shows why sits beside the
case in tests/sweep_inputs.py, tests/test_ref64.py checks it on the CPU against the restated dispatch rules and holds the resulting
reach table to the kernels of the built library, and LAB_NOTES.md part T holds it to a kernel trace of this file.  Every output
element is compared; seeds are fixed; shapes sit in `parametrize` lists so that a failure names its shape.

Gates:
  derived       implicit GEMM (split or not), pool in the reduction, conv3d, ss_conv_stem3, ss_stem_pool:
                |got - ref64| <= dot_bound(K_real + 2, S) per element, K_real = the REAL products of that element (no padded taps, no
                padded channels), S = sum |x||w| + |bias| + |res|; any order of summation, so split-K adds nothing; ReLU and max exact
  Winograd      fp32 and bf16x9: min(derived ceiling (1.01 (cin + T_m) + 3) u S_w, 4 rho u S_w): S_w = the Winograd form on absolute
                values (ref64.wino_scale), rho = the error of an fp32 CPU emulation of the same form on the same input in units of
                u S_w (sweep_inputs.wino_gate; never from a kernel), 4 = the project's margin for another summation order
  bit for bit   one-hot inputs on the implicit-GEMM paths (every output is one weight or zero), padding channels, grouped launches
                against single ones, persistent against one-block-per-workgroup F(4x4,3x3), pool kernels against pooling the
                un-pooled kernel's map, refusals

    python -m pytest tests/test_gpu_conv_sweeps.py -m gpu          (SS_VERBOSE=1 prints every observed maximum beside its gate)"""
import functools

import numpy as np
import pytest
import torch

import ref64 as R
import sweep_inputs as G
from test_gpu_kernel_sweeps import dev, within, refused, host, nhwc, VERBOSE          # noqa: F401  (dev is the module's GPU fixture)

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
T = torch.from_numpy
FILL = 7.0                 # what output buffers hold before a launch: padding channels must still hold it afterwards


def channels_last(x, c_pad=None):
    """[n,c,(t,)h,w] numpy -> [n,(t,)h,w,c_pad] numpy, channels zero-padded"""
    y = np.moveaxis(x, 1, -1)
    if c_pad and c_pad > y.shape[-1]:
        y = np.concatenate((y, np.zeros(y.shape[:-1] + (c_pad - y.shape[-1],), y.dtype)), axis=-1)
    return np.ascontiguousarray(y)


def channels_first(t):
    return np.moveaxis(host(t), -1, 1)


def pack_filters(wt, cin):
    """torch's [cout,c,(kt,)kh,kw] -> the engine's [cout,kt,kh,kw,cin]"""
    if wt.ndim == 4:
        wt = wt[:, :, None]
    return channels_last(wt, cin)


# ================================================================================================ implicit GEMM
def ig_launch(c, dev, x_l, w_l, b=None, r_l=None, relu=False):
    """ss_conv_nhwc on channels-last numpy operands of case c -> device out [n,to,ho,wo,out_cs], FILL where nothing is written"""
    from stabstitch2_amd import _hip as H
    to, ho, wo, M, K = G.ig_geometry(c)
    kt, kh, kw = c['k']
    pt, ph, pw = c['p']
    t = c['t'] or 1
    n, h, w, cin, cout, ocs = c['n'], c['h'], c['w'], c['cin'], c['cout'], c['out_cs']
    assert x_l.size == n * t * h * w * cin and w_l.size == cout * K
    xd, wd = T(x_l).to(dev), T(w_l).to(dev)
    bd = T(b).to(dev) if b is not None else None
    out = torch.full((n, to, ho, wo, ocs), FILL, device=dev)
    rd = None
    if r_l is not None:                                       # the residual has the output's pitch
        rd = torch.zeros((n, to, ho, wo, ocs), device=dev)
        rd[..., :cout] = T(r_l).to(dev).view(n, to, ho, wo, cout)
    need = int(H.lib().ss_conv_workspace_need(n, t, h, w, cin, cout, kt, kh, kw, c['s'], pt, ph, pw, 1)) if c['ws'] else 0
    ws = torch.empty(need, device=dev) if need > 0 else None
    assert (need > 0) == (G.ig_plan(c)['splits'] > 1), (c['name'], need)
    H.call('ss_conv_nhwc', H.dptr(xd), H.dptr(wd), H.dptr(bd, True), H.dptr(rd, True), H.dptr(out), n, t, h, w, cin, cout, kt, kh, kw,
           c['s'], pt, ph, pw, int(relu), ocs, 1, 0, 0, 0, H.dptr(ws, True), need, H.stream())
    return out


@pytest.mark.parametrize('c', G.IGEMM_CASES, ids=lambda c: c['name'])
def test_implicit_gemm_against_fp64(dev, c):
    """ss_conv_nhwc, one launch per case, against ref64.conv under the derived bound of an fp32 sum of the element's real products."""
    to, ho, wo, M, K = G.ig_geometry(c)
    three = c['t'] is not None
    x, wt, b, r = G.conv_inputs(c['n'], c['c_real'], c['cout'], c['h'], c['w'], c['k'], t=c['t'], out_hw=(to, ho, wo) if three else (ho, wo),
                                bias=c['bias'], res=c['res'])
    ref, bound = R.conv_bound(x, wt, b, r, c['s'], c['p'] if three else c['p'][1:], c['relu'])
    out = ig_launch(c, dev, channels_last(x, c['cin']), pack_filters(wt, c['cin']), b, None if r is None else channels_last(r), c['relu'])
    cout = c['cout']
    if c['out_cs'] > cout:
        assert bool((out[..., cout:] == FILL).all()), 'padding channels written'
    got = channels_first(out[..., :cout])
    within(got if three else got[:, :, 0], ref, bound, 'igemm %s [%s]' % (c['name'], c['claim']))     # observed: max |diff| 9.5e-6, worst |diff| / bound 0.21


def impulse_sites(c):
    """(image, t, y, x, channel) of the one-hot inputs of a case: the four corners, the middle of the four edges, the centre, and a
    site in the LAST real channel (next to the layout padding); channels and frames rotate."""
    h, w, t, cr, n = c['h'], c['w'], c['t'] or 1, c['c_real'], c['n']
    pos = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, w // 2), (h - 1, w // 2), (h // 2, 0), (h // 2, w - 1), (h // 2, w // 2)]
    sites = [(i % n, (0, t - 1, t // 2)[i % 3], y, x, i % cr) for i, (y, x) in enumerate(pos)]
    sites.append(((n - 1), t // 2, h // 3, w // 3, cr - 1))
    return sorted(set(sites))


def impulse_footprint(c, site):
    """{(image, to, oy, ox): (dt, dy, dx)}: the outputs one one-hot input reaches and the tap through which it does"""
    to, ho, wo, M, K = G.ig_geometry(c)
    kt, kh, kw = c['k']
    pt, ph, pw = c['p']
    b, ti, y, x, ch = site
    fp = {}
    for dt in range(kt):
        ot = ti + pt - dt
        if not 0 <= ot < to:
            continue
        for dy in range(kh):
            if (y + ph - dy) % c['s'] or not 0 <= (y + ph - dy) // c['s'] < ho:
                continue
            for dx in range(kw):
                if (x + pw - dx) % c['s'] or not 0 <= (x + pw - dx) // c['s'] < wo:
                    continue
                fp[(b, ot, (y + ph - dy) // c['s'], (x + pw - dx) // c['s'])] = (dt, dy, dx)
    return fp


@pytest.mark.parametrize('c', G.IGEMM_CASES, ids=lambda c: c['name'])
def test_implicit_gemm_impulse_identities(dev, c):
    """A one-hot input makes every output exactly one weight or exactly zero, on every tile, address mode and split-K plan: what
    iid data cannot show -- a tap read from the wrong neighbour under a mask that is right on average.  No bias, residual or ReLU;
    compared with ==.  Sites whose footprints overlap go into separate launches."""
    to, ho, wo, M, K = G.ig_geometry(c)
    t = c['t'] or 1
    wt = G.conv_inputs(1, c['c_real'], c['cout'], 1, 1, c['k'], t=1, bias=False)[1]               # [cout,c,kt,kh,kw]
    w_l = pack_filters(wt, c['cin'])
    launches = []
    for site in impulse_sites(c):
        fp = impulse_footprint(c, site)
        for sites, taken in launches:
            if not taken.keys() & fp.keys():
                sites.append((site, fp))
                taken.update(fp)
                break
        else:
            launches.append(([(site, fp)], dict(fp)))
    hits = 0
    for sites, _ in launches:
        x_l = np.zeros((c['n'], t, c['h'], c['w'], c['cin']), np.float32)
        want = np.zeros((c['n'], to, ho, wo, c['cout']), np.float32)
        for (b, ti, y, x, ch), fp in sites:
            x_l[b, ti, y, x, ch] = 1.0
            for (ob, ot, oy, ox), (dt, dy, dx) in fp.items():
                want[ob, ot, oy, ox] = wt[:, ch, dt, dy, dx]
                hits += 1
        out = ig_launch(c, dev, x_l, w_l)
        got = out[..., :c['cout']].cpu().numpy()
        bad = np.argwhere(got != want)
        assert bad.size == 0, 'igemm %s [%s]: %d outputs differ from the one weight they should be, first at %s' % (
            c['name'], c['claim'], len(bad), bad[0])
        if c['out_cs'] > c['cout']:
            assert bool((out[..., c['cout']:] == FILL).all())
    assert hits > 0


# ================================================================================================ pool in the split-K reduction
@pytest.mark.parametrize('case', G.POOL_REDUCE_CASES, ids=lambda v: '-'.join(map(str, v)))
def test_conv_pool_in_reduce_against_fp64(dev, case):
    """ss_conv_pool2_nhwc (3 x 3 / pad 1 + bias + ReLU + MaxPool2d(2, 2), the pool inside the split-K reduction): even and odd maps,
    two groups, out_cs > cout; the bound of a pooled element is the largest bound in its window."""
    from stabstitch2_amd import _hip as H
    n, h, w, cin, cout, groups, ocs = case
    hp, wp = h // 2, w // 2
    xs, ws_, bs = [], [], []
    out = torch.full((groups, n, hp, wp, ocs), FILL, device=dev)
    for g in range(groups):
        x, wt, b, _ = G.conv_inputs(n, cin, cout, h, w, seed=g)
        xs.append(x), ws_.append(wt), bs.append(b)
    xd = T(np.stack([channels_last(x) for x in xs])).to(dev)
    wd = T(np.stack([pack_filters(wt, cin) for wt in ws_])).to(dev)
    bd = T(np.stack(bs)).to(dev)
    need = int(H.lib().ss_conv_workspace_need(n, 1, h, w, cin, cout, 1, 3, 3, 1, 0, 1, 1, groups))
    assert need > 0
    ws = torch.empty(need, device=dev)
    H.call('ss_conv_pool2_nhwc', H.dptr(xd), H.dptr(wd), H.dptr(bd), H.dptr(out), n, h, w, cin, cout, 3, 3, 1, 1, 1, 1, ocs, groups,
           xd[0].numel(), wd[0].numel(), out[0].numel(), H.dptr(ws), need, H.stream())
    assert ocs == cout or bool((out[..., cout:] == FILL).all()), 'padding channels written'
    for g in range(groups):
        ref, bound = R.conv_pool2(xs[g], ws_[g], bs[g], 1, 1, relu=True)
        within(channels_first(out[g, ..., :cout]), ref, bound, 'conv + pool in reduce %s group %d' % (case, g))     # observed: max |diff| 1.6e-6, worst |diff| / bound 0.007


def test_conv_pool_in_reduce_refusals(dev):
    """Ho or Wo of 1: SS_ERR_ARG; a launch that would not split (K of one tile): SS_ERR_UNSUPPORTED, nothing written."""
    from stabstitch2_amd import _hip as H
    x = torch.zeros(1, 4, 4, 32, device=dev)
    wt = torch.zeros(64 * 9 * 32, device=dev)
    out = torch.full((1, 2, 2, 64), FILL, device=dev)
    ws = torch.empty(1 << 16, device=dev)

    def pool(h, w, k, pad):
        H.call('ss_conv_pool2_nhwc', H.dptr(x), H.dptr(wt), None, H.dptr(out), 1, h, w, 32, 64, k, k, 1, pad, pad, 1, 64, 1, 0, 0, 0,
               H.dptr(ws), ws.numel(), H.stream())
    refused(-1, pool, 1, 4, 3, 1)
    refused(-1, pool, 4, 1, 3, 1)
    refused(-3, pool, 4, 4, 1, 0)                  # K = 32: one K tile, never split
    assert bool((out == FILL).all())


# ================================================================================================ groups
@pytest.mark.parametrize('groups,shared,cin,res', [(2, False, 8, True), (3, False, 8, False), (2, True, 8, True), (3, True, 32, True)])
def test_implicit_gemm_groups(dev, groups, shared, cin, res):
    """ss_conv_nhwc with 2 and 3 groups, each group against ref64; a shared input (in_gs = 0); group strides LARGER than the tensors
    (the gaps between the groups' outputs keep what they held); cin = 8 (K = 72, nk = 3: never split) also bit for bit against one
    launch per group, cin = 32 (K = 288, nk = 9, maxs = 2) with bias, residual and ReLU through a grouped split-K reduction."""
    from stabstitch2_amd import _hip as H
    n, h, w, cout, gap = 2, 9, 11, 64, 40
    ops_ = [G.conv_inputs(n, cin, cout, h, w, out_hw=(h, w), res=res, seed=10 + g) for g in range(groups)]
    x_e, w_e, o_e = n * h * w * cin, cout * 9 * cin, n * h * w * cout
    xbuf = torch.zeros(groups, x_e + gap, device=dev)
    wbuf = torch.zeros(groups, w_e + gap, device=dev)
    obuf = torch.full((groups, o_e + gap), FILL, device=dev)
    rbuf = torch.zeros(groups, o_e + gap, device=dev)
    for g, (x, wt, b, r) in enumerate(ops_):
        xbuf[g, :x_e] = T(channels_last(ops_[0][0] if shared else x)).to(dev).view(-1)
        wbuf[g, :w_e] = T(pack_filters(wt, cin)).to(dev).view(-1)
        if res:
            rbuf[g, :o_e] = T(channels_last(r)).to(dev).view(-1)
    bd = T(np.stack([o[2] for o in ops_])).to(dev)
    need = int(H.lib().ss_conv_workspace_need(n, 1, h, w, cin, cout, 1, 3, 3, 1, 0, 1, 1, groups))
    assert (need > 0) == (cin == 32)
    ws = torch.empty(need, device=dev) if need else None
    H.call('ss_conv_nhwc', H.dptr(xbuf), H.dptr(wbuf), H.dptr(bd), H.dptr(rbuf) if res else None, H.dptr(obuf), n, 1, h, w, cin, cout, 1, 3, 3,
           1, 0, 1, 1, 1, cout, groups, 0 if shared else x_e + gap, w_e + gap, o_e + gap, H.dptr(ws, True), need, H.stream())
    assert bool((obuf[:, o_e:] == FILL).all()), 'the gap behind a group was written'
    for g, (x, wt, b, r) in enumerate(ops_):
        xin = ops_[0][0] if shared else x
        ref, bound = R.conv_bound(xin, wt, b, r, 1, 1, True)
        got = obuf[g, :o_e].view(n, h, w, cout)
        within(channels_first(got), ref, bound, 'grouped igemm group %d of %d' % (g, groups))          # observed: worst |diff| / bound 0.05
        if cin == 8:
            c = G.IG('single', n, h, w, cin, cout, G.X3, p=G.P1)
            one = ig_launch(c, dev, channels_last(xin), pack_filters(wt, cin), b, channels_last(r) if res else None, True)
            assert torch.equal(one.view(n, h, w, cout), got), 'group %d differs from its own launch' % g


# ================================================================================================ the stem
def stem_pack(wt, groups):
    """[g * 64,3,7,7] -> ss_conv_stem3's [g,64,7,24]: wgt[co][dh][3 dw + c] = w[co][c][dh][dw], entries 21 .. 23 zero"""
    p = np.zeros((groups * 64, 7, 24), np.float32)
    p[:, :, :21] = wt.transpose(0, 2, 3, 1).reshape(groups * 64, 7, 21)
    return p.reshape(groups, 64, 7, 24)


def stem_check(dev, n, h, w, groups, what, split=False):
    from stabstitch2_amd import ops
    x, wt, b = G.stem_inputs(n, h, w, groups)
    val, bound = R.stem(x, wt, b)                                                            # [n, g * 64, ho, wo]
    buf = ops.stem_input(T(x).to(dev))
    pk = T(stem_pack(wt, groups)).to(dev)
    bd = T(b).to(dev)
    conv = ops.conv_stem(buf, pk if groups > 1 else pk[0], bd.view(groups, 64) if groups > 1 else bd, relu=True)
    conv = conv if groups > 1 else conv[None]                                               # [g,n,ho,wo,64]
    ho, wo = val.shape[2:]
    got = host(conv).transpose(1, 0, 4, 2, 3).reshape(n, groups * 64, ho, wo)
    within(got, val, bound, 'ss_conv_stem3 ' + what)                                         # observed: max |diff| 4.0e-6, worst |diff| / bound 0.16
    pooled = ops.stem_pool(buf, pk.view(groups * 64, 7, 24), bd)                              # [g,n,hp,wp,64]
    pv, pb = R.pool_max(val, 3, 2, 1), R.pool_max(bound, 3, 2, 1)
    got = host(pooled).transpose(1, 0, 4, 2, 3).reshape(n, groups * 64, pv.shape[2], pv.shape[3])
    within(got, pv, pb, 'ss_stem_pool ' + what)                                              # observed: the same 4.0e-6 and 0.16
    if split:                # batches beyond one launch's 32-bit offsets go in several launches: two frames per launch here
        old = ops.STEM_POOL_MAX_BYTES
        ops.STEM_POOL_MAX_BYTES = 2 * h * (w + 8) * 12 + 1
        try:
            again = ops.stem_pool(buf, pk.view(groups * 64, 7, 24), bd)
        finally:
            ops.STEM_POOL_MAX_BYTES = old
        assert torch.equal(again, pooled)


@pytest.mark.parametrize('groups', [1, 2])
@pytest.mark.parametrize('h,w', G.STEM_SIZES, ids=lambda v: str(v))
def test_stem_against_fp64(dev, h, w, groups):
    """ss_conv_stem3 (K = 7 x 24 = 168: K % 32 = 8, the TAIL variant of the 64 x 64 tile in address mode 1; 147 real products) and
    ss_stem_pool (one kernel: conv + ReLU + MaxPool2d(3, 2, 1)) on maps from 1 x 1 up, one and two filter banks, 5 frames, the
    several-launches path of ops.stem_pool included."""
    stem_check(dev, 5, h, w, groups, '%dx%d g%d' % (h, w, groups), split=True)


def test_stem_full_frames_on_the_128_row_tile(dev):
    """Seven 360 x 480 frames: M = 7 x 180 x 240 = 302400, b128m = cdiv(M, 128) = 2363 >= 2048 -> ss_conv_stem3 runs the 128 x 64 tile
    (TAIL, mode 1); ss_stem_pool on the same frames."""
    assert G.stem_plan(7, 360, 480, 64)['kernel'] == 'conv_igemm_kernel<2,2,2,1,1,1,32,1,1,1>'
    stem_check(dev, 7, 360, 480, 1, '7 x 360x480')


# ================================================================================================ F(2x2,3x3)
def wino_operands(dev, x, wt, b, r):
    wd = T(np.ascontiguousarray(wt.transpose(0, 2, 3, 1)[:, None])).to(dev)                    # [cout,1,3,3,cin]
    return nhwc(x, dev), wd, T(b).to(dev), nhwc(r, dev)


@functools.lru_cache(maxsize=4)
def wino_case(m, case):
    """the operands of a Winograd case and its three gates: bias + residual + ReLU, bare, bias + ReLU (the pool kernel's)"""
    n, h, w, cin, cout = case
    x, wt, b, r = G.conv_inputs(n, cin, cout, h, w, out_hw=(h, w), res=True)
    gates = {'brr': G.wino_gate(x, wt, m, b, r, True), 'bare': G.wino_gate(x, wt, m)}
    if m == 2 and h >= 2 and w >= 2:
        gates['br'] = G.wino_gate(x, wt, m, b, None, True)
    return x, wt, b, r, gates


def wino_within(got, gate, what):
    ref, bound, rho, s_w = gate
    if VERBOSE:
        d = np.abs(host(got) - ref)
        print('  [sweep] %-58s rho %.3f  max|diff| / (u S_w) %.3f' % (what, rho, float((d / (R.U24 * s_w)).max())))
    within(got, ref, bound, what)          # observed, worst |diff| / gate: F(2x2) fp32 0.65, bf16x9 0.68, pool 0.39; F(4x4) 0.50 (kernel error <= 2.7 rho)


@pytest.mark.parametrize('case', G.WINO2_CASES, ids=lambda v: '-'.join(map(str, v)))
def test_winograd_f2_against_fp64(dev, case):
    """ss_conv3x3_wino_nhwc, ss_conv3x3_wino3_nhwc (bf16x9) and ss_conv3x3_wino_pool2_nhwc on maps from 1 x 1 to 33 x 33 (1 x N and
    N x 1 included: both block shapes), channel-chunk tails 4, 8, 12, 64 / 128 / 192 filters, with and without a residual.  The
    pool kernel is also held bit for bit to the 2 x 2 floor pool of the un-pooled kernel's map (odd maps drop a row / column)."""
    from stabstitch2_amd import ops
    n, h, w, cin, cout = case
    x, wt, b, r, gates = wino_case(2, case)
    xd, wd, bd, rd = wino_operands(dev, x, wt, b, r)
    tag = 'F(2x2) %s %dx%d blocks' % (case, *G.wino_blocks(h, w))
    old = ops.WINO_MATH
    try:
        for math in ('f32', 'bf16x9'):
            ops.WINO_MATH = math
            wino_within(ops.conv_winograd(xd, wd, bd, rd, True).permute(0, 3, 1, 2), gates['brr'], '%s %s bias res relu' % (tag, math))
            wino_within(ops.conv_winograd(xd, wd).permute(0, 3, 1, 2), gates['bare'], '%s %s bare' % (tag, math))
    finally:
        ops.WINO_MATH = old
    if 'br' in gates:
        ref, bound, rho, s_w = gates['br']
        pooled = ops.conv_winograd(xd, wd, bd, None, True, pool2=True)
        wino_within(pooled.permute(0, 3, 1, 2), (R.pool_max(ref, 2, 2, 0), R.pool_max(bound, 2, 2, 0), rho, R.pool_max(s_w, 2, 2, 0)),
                    tag + ' pool epilogue')
        full = ops.conv_winograd(xd, wd, bd, None, True)
        assert torch.equal(pooled, ops.maxpool(full, 2, 2, 0)), 'pool epilogue differs from pooling the stored map'


def test_winograd_f2_groups_and_refusals(dev):
    """Two groups and a shared input, bit for bit against one launch per group (both block shapes); cin % 4, cout % 64, out_cs <
    cout and a pooled map below 2 x 2: SS_ERR_ARG, as include/stabstitch_hip.h states."""
    from stabstitch2_amd import _hip as H, ops
    for (h, w) in ((9, 17), (7, 16)):
        ins = [G.conv_inputs(2, 36, 64, h, w, out_hw=(h, w), res=True, seed=20 + g) for g in range(2)]
        xs = torch.stack([nhwc(i[0], dev) for i in ins])
        wg = torch.stack([wino_operands(dev, *i)[1] for i in ins])
        bg = torch.stack([T(i[2]).to(dev) for i in ins])
        rg = torch.stack([nhwc(i[3], dev) for i in ins])
        for shared in (False, True):
            got = ops.conv_winograd(xs[0] if shared else xs, wg, bg, rg, True)
            for g in range(2):
                one = ops.conv_winograd(xs[0] if shared else xs[g], wg[g].contiguous(), bg[g].contiguous(), rg[g].contiguous(), True)
                assert torch.equal(got[g], one), (h, w, shared, g)
    z = torch.zeros(1 << 16, device=dev)

    def wino(entry, cin, cout, ocs, h=4, w=4):
        extra = () if 'pool' in entry else (None,)
        H.call(entry, H.dptr(z), H.dptr(z), None, *extra, H.dptr(z), 1, h, w, cin, cout, 0, ocs, 1, 0, 0, 0, H.stream())
    for entry in ('ss_conv3x3_wino_nhwc', 'ss_conv3x3_wino3_nhwc', 'ss_conv3x3_wino_pool2_nhwc'):
        refused(-1, wino, entry, 6, 64, 64)
        refused(-1, wino, entry, 8, 32, 32)
        refused(-1, wino, entry, 8, 64, 60)
    refused(-1, wino, 'ss_conv3x3_wino_pool2_nhwc', 8, 64, 64, 1, 4)
    refused(-1, wino, 'ss_conv3x3_wino_pool2_nhwc', 8, 64, 64, 4, 1)


# ================================================================================================ F(4x4,3x3)
@pytest.mark.parametrize('case', G.WINO43_CASES, ids=lambda v: '-'.join(map(str, v)))
def test_winograd_f4_against_fp64(dev, case):
    """ss_conv3x3_wino43_nhwc on both block geometries (16 x 32 for maps up to 31 wide, else 8 x 60), widths around every block and
    tile edge, cin 16 (its own instantiation) / 48 / 64 / 80, residual and ReLU both ways, fewer blocks than CUs and (the last
    case) more; persistent workgroups against one workgroup per block, bit for bit."""
    from stabstitch2_amd import _hip as H, ops
    n, h, w, cin, cout = case
    x, wt, b, r, gates = wino_case(4, case)
    xd, wd, bd, rd = wino_operands(dev, x, wt, b, r)
    tag = 'F(4x4) %s %s, %d blocks' % (case, '16x32' if w <= 31 else '8x60', G.wino43_blocks(n, h, w, cout))
    a = ops.conv_winograd43(xd, wd, bd, rd, True)
    bare = ops.conv_winograd43(xd, wd)
    wino_within(a.permute(0, 3, 1, 2), gates['brr'], tag + ' bias res relu')
    wino_within(bare.permute(0, 3, 1, 2), gates['bare'], tag + ' bare')
    assert H.lib().ss_wino43_set_persistent(0) == 0
    try:
        a1 = ops.conv_winograd43(xd, wd, bd, rd, True)
        bare1 = ops.conv_winograd43(xd, wd)
    finally:
        H.lib().ss_wino43_set_persistent(1)
    assert torch.equal(a, a1) and torch.equal(bare, bare1), 'persistent workgroups changed the result'


def test_winograd_f4_groups_padding_and_refusals(dev):
    """Two groups and a shared input bit for bit against one launch per group (both geometries); out_cs > cout keeps the padding;
    cin % 16 or cout % 64: SS_ERR_UNSUPPORTED, out_cs < cout: SS_ERR_ARG."""
    from stabstitch2_amd import _hip as H, ops
    for (h, w) in ((9, 30), (9, 61)):
        ins = [G.conv_inputs(2, 48, 64, h, w, out_hw=(h, w), res=True, seed=30 + g) for g in range(2)]
        xs = torch.stack([nhwc(i[0], dev) for i in ins])
        wg = torch.stack([wino_operands(dev, *i)[1] for i in ins])
        bg = torch.stack([T(i[2]).to(dev) for i in ins])
        rg = torch.stack([nhwc(i[3], dev) for i in ins])
        for shared in (False, True):
            got = ops.conv_winograd43(xs[0] if shared else xs, wg, bg, rg, True)
            for g in range(2):
                one = ops.conv_winograd43(xs[0] if shared else xs[g], wg[g].contiguous(), bg[g].contiguous(), rg[g].contiguous(), True)
                assert torch.equal(got[g], one), (h, w, shared, g)
        wide = torch.full((2, h, w, 72), FILL, device=dev)
        ops.conv_winograd43(xs[0], wg[0].contiguous(), bg[0].contiguous(), None, True, out=wide)
        assert torch.equal(wide[..., :64], ops.conv_winograd43(xs[0], wg[0].contiguous(), bg[0].contiguous(), None, True))
        assert bool((wide[..., 64:] == FILL).all()), 'padding channels written'
    z = torch.zeros(1 << 16, device=dev)

    def w43(cin, cout, ocs):
        H.call('ss_conv3x3_wino43_nhwc', H.dptr(z), H.dptr(z), None, None, H.dptr(z), 1, 4, 4, cin, cout, 0, ocs, 1, 0, 0, 0, H.stream())
    refused(-3, w43, 24, 64, 64)
    refused(-3, w43, 16, 32, 32)
    refused(-1, w43, 16, 64, 60)
