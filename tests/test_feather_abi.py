"""FEATHER fusion without a GPU: the flag in the header and the ctypes module, what the C ABI and ops refuse, the properties of the
float64 statement (tests/feather_ref.py), the calibration of its bound against an fp32 reading, and the kernels the built library
carries for it.  The kernels themselves: tests/test_gpu_feather.py.
    python -m pytest tests/test_feather_abi.py"""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import feather_ref as FR
import sweep_inputs as G
from oracle import samplers as S
from test_host_logic import built_lib  # noqa: F401  (fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
T = torch.from_numpy
# frame h, w, canvas hc, wc: the tile-edge canvases of the AVERAGE sweep, and a small frame on a canvas of one partial tile column
CASES = [(72, 96, 80, 120), (72, 96, 81, 129), (72, 96, 85, 191), (72, 96, 84, 128), (72, 96, 87, 65), (36, 48, 43, 67)]


def _ptr(buf):
    return ctypes.cast(buf, ctypes.c_void_p)


# ------------------------------------------------------------------------------------------------ the flag
def test_flag_is_in_the_header_and_the_ctypes_module(built_lib):
    from stabstitch2_amd import _hip, ops
    hdr = open(os.path.join(ROOT, 'include', 'stabstitch_hip.h')).read()
    defines = {k: int(v) for k, v in re.findall(r'^#define (SS_(?:WARP|FUSE)_[A-Z_]+) (\d+)\b', hdr, re.M)}
    assert defines == _hip.MODE_FLAGS and defines['SS_FUSE_FEATHER'] == 32
    bits = [v for v in defines.values() if v > 1]
    assert all(v & (v - 1) == 0 for v in bits) and len(set(bits)) == len(bits)          # bits of their own, above the warp modes
    assert ops.FUSIONS == {'AVERAGE': 0, 'FEATHER': 32}
    assert ops.fused_render('AVERAGE') and ops.fused_render('FEATHER') and not ops.fused_render('LINEAR') and not ops.fused_render('MEDIAN')
    declared = set(re.findall(r'\bSS_API[^;]*?\b(ss_[a-z0-9_]+)\s*\(', hdr))
    assert len(declared) == 113 and sorted(_hip.SIGNATURES) == sorted(declared)        # the flag adds no entry point


def test_feather_with_the_folded_radial_term_is_refused(built_lib):
    """SS_FUSE_FEATHER | SS_WARP_EPS_FOLD on every entry that takes either, with arguments that are valid otherwise (refused before
    a launch: the pointers are host memory); so are the bits above it."""
    buf = (ctypes.c_float * 4096)()
    imgs = (ctypes.c_void_p * 3)(*[ctypes.addressof(buf)] * 3)
    p = _ptr(buf)
    L = built_lib
    for mode in (32 | 16, 32 | 16 | 1, 64, 32 | 64, 32 | 2, 128 | 32, 256 | 32):
        assert L.ss_render_average(imgs, p, p, None, 0, p, 2, 8, 8, 45, 150, mode, None) == ERR_ARG, mode
        assert L.ss_render_average_u8(imgs, p, p, None, 0, p, 3, 8, 8, 45, 150, mode, None) == ERR_ARG, mode
        assert L.ss_render_average_clip(imgs, p, p, None, 0, p, 2, 2, 8, 8, 45, 150, mode, None) == ERR_ARG, mode
        assert L.ss_render_average_clip_u8(imgs, p, p, None, 0, p, 2, 3, 8, 8, 45, 150, mode, None) == ERR_ARG, mode
        assert L.ss_render_average_gains(imgs, p, p, None, 0, p, 2, 8, 8, 45, 150, mode, p, None) == ERR_ARG, mode
        assert L.ss_render_average_u8_gains(imgs, p, p, None, 0, p, 3, 8, 8, 45, 150, mode, p, None) == ERR_ARG, mode
        assert L.ss_render_average_clip_gains(imgs, p, p, None, 0, p, 2, 2, 8, 8, 45, 150, mode, p, None) == ERR_ARG, mode
        assert L.ss_render_average_clip_u8_gains(imgs, p, p, None, 0, p, 2, 3, 8, 8, 45, 150, mode, p, None) == ERR_ARG, mode
        pitch = (ctypes.c_int * 3)(8, 8, 8)
        assert L.ss_render_average_nv12(imgs, imgs, pitch, p, p, None, 0, p, p, 150, 1, 2, 8, 8, 44, 150, mode, None) == ERR_ARG, mode
    # the flag does not soften the other refusals: a null view, a view count, a footprint of the wrong length, null gains
    none = (ctypes.c_void_p * 3)(ctypes.addressof(buf), None, None)
    assert L.ss_render_average(none, p, p, None, 0, p, 2, 8, 8, 45, 150, 32, None) == ERR_ARG
    assert L.ss_render_average(imgs, p, p, None, 0, p, 4, 8, 8, 45, 150, 33, None) == ERR_ARG
    assert L.ss_render_average_u8(imgs, p, p, p, 7, p, 2, 8, 8, 45, 150, 32, None) == ERR_ARG
    assert L.ss_render_average_gains(imgs, p, p, None, 0, p, 2, 8, 8, 45, 150, 32, None, None) == ERR_ARG
    assert L.ss_render_average_nv12(imgs, imgs, pitch, p, p, None, 0, p, p, 150, 1, 2, 8, 8, 45, 150, 32, None) == ERR_ARG     # odd hc


def test_ops_refuse_an_unknown_fusion_before_touching_the_device(monkeypatch):
    from stabstitch2_amd import ops
    x = torch.zeros((3, 4, 4))
    for fn in (ops.render_average, ops.render_average_u8, ops.render_average_clip, ops.render_average_clip_u8, ops.render_average_nv12):
        for bad in ('LINEAR', 'feather', None, 32):
            with pytest.raises(ValueError, match="'AVERAGE' or 'FEATHER'"):
                fn([x, x], x, x, 8, 64, fusion=bad)
    monkeypatch.setattr(ops, 'RENDER_EPS_FOLD', True)                 # SS_RENDER_EPS_FOLD=1: no FEATHER form
    for fn in (ops.render_average, ops.render_average_clip_u8, ops.render_average_nv12):
        with pytest.raises(ValueError, match='SS_RENDER_EPS_FOLD'):
            fn([x, x], x, x, 8, 64, fusion='FEATHER')
    assert ops._avg_mode('FAST') == 17 and ops._avg_mode('NORMAL', 'AVERAGE') == 16
    monkeypatch.setattr(ops, 'RENDER_EPS_FOLD', False)
    assert ops._avg_mode('FAST', 'FEATHER') == 33 and ops._avg_mode('NORMAL', 'FEATHER') == 32 and ops._avg_mode('FAST') == 1


def test_stitchers_refuse_feather_with_the_folded_radial_term(monkeypatch):
    from stabstitch2_amd import online, ops

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.p = torch.nn.Parameter(torch.zeros(1))
    nets = (Net(), Net(), Net())
    monkeypatch.setattr(ops, 'RENDER_EPS_FOLD', True)
    with pytest.raises(ValueError, match='SS_RENDER_EPS_FOLD'):
        online._Stitcher(nets, 180, 320, 0.03, 'NORMAL', 'FEATHER', True, 'never', meshes_only=True)
    st = online._Stitcher(nets, 180, 320, 0.03, 'NORMAL', 'AVERAGE', True, 'never', meshes_only=True)
    assert st._fused
    monkeypatch.setattr(ops, 'RENDER_EPS_FOLD', False)
    assert online._Stitcher(nets, 180, 320, 0.03, 'NORMAL', 'FEATHER', True, 'never', meshes_only=True)._fused
    for other in ('LINEAR', 'MEDIAN'):                                # neither takes the fused render: today's paths
        assert not online._Stitcher(nets, 180, 320, 0.03, 'NORMAL', other, True, 'never', meshes_only=True)._fused


# ------------------------------------------------------------------------------------------------ the statement
def _case(views, seed=11, size=(72, 96, 81, 129)):
    h, w, hc, wc = size
    U, src, tgt = G.warp_case(views, h, w, hc, wc, seed=seed)
    return np.ascontiguousarray(U[:, :3]), src, tgt, hc, wc


@pytest.mark.parametrize('mode', ['NORMAL', 'FAST'])
def test_one_view_alone_gives_its_sample(mode):
    """Where one view has a positive weight and the others none, the fusion is that view's sample (to the rounding of w c / w)."""
    U, src, tgt, hc, wc = _case(3)
    ref = FR.feather64(U, src, tgt, hc, wc, mode)
    pos = ref['w'] > 0
    seen = 0
    for v in range(3):
        alone = pos[v] & (pos.sum(0) == 1)
        seen += int(alone.sum())
        d = np.abs(ref['out'] - ref['c'][v])[:, alone]
        assert d.size and d.max() <= 255 * 2.0 ** -51, (v, d.max())
    assert seen > 500
    nobody = pos.sum(0) == 0
    assert nobody.any() and (ref['out'][:, nobody] == 0).all() and (ref['den'][nobody] == 0).all()


@pytest.mark.parametrize('mode', ['NORMAL', 'FAST'])
def test_identical_views_give_their_sample(mode):
    U, src, tgt, hc, wc = _case(3)
    same = [np.repeat(a[:1], 3, axis=0) for a in (U, src, tgt)]
    ref = FR.feather64(*same, hc, wc, mode)
    inside = ref['den'] > 0
    assert inside.mean() > 0.2
    assert np.abs(ref['out'] - ref['c'][0])[:, inside].max() <= 255 * 2.0 ** -50
    c32 = ref['c'].astype(np.float32)
    o32 = FR.feather32(c32, ref['xn'], ref['yn'])
    assert np.abs(o32.astype(np.float64) - c32[0])[:, inside].max() <= 4 * FR.ULP255          # three products, two + two sums, a quotient


@pytest.mark.parametrize('mode', ['NORMAL', 'FAST'])
@pytest.mark.parametrize('views', [2, 3])
def test_fusion_is_symmetric_in_the_views(views, mode):
    """Every permutation of the views gives the same frame: up to the summation order in float64 and in the fp32 restatement (where
    AVERAGE's chain ((1 (+) 2) (+) 3) depends on the order at the size of the samples)."""
    import itertools
    U, src, tgt, hc, wc = _case(views)
    ref = FR.feather64(U, src, tgt, hc, wc, mode)
    c32, x32, y32 = ref['c'].astype(np.float32), ref['xn'].astype(np.float32), ref['yn'].astype(np.float32)
    o32 = FR.feather32(c32, x32, y32)
    for perm in itertools.permutations(range(views)):
        p = list(perm)
        other = FR.feather64(U[p], src[p], tgt[p], hc, wc, mode)
        assert np.abs(other['out'] - ref['out']).max() <= 255 * 2.0 ** -49, perm
        ok = ~FR.left_out(ref)
        assert np.abs(FR.feather32(c32[p], x32[p], y32[p]).astype(np.float64) - o32)[:, ok].max() <= 8 * FR.ULP255, perm


def test_fp32_restatement_follows_the_fixed_order():
    """((w0 c0) + (w1 c1)) + (w2 c2) over (w0 + w1) + w2, every operation rounded to fp32, on operands where another order or a
    fused multiply-add gives another result."""
    f = np.float32
    w = np.array([0.3, 0.7, 0.1], f)
    c = np.array([200.1, 13.7, 99.9], f)
    num = f(f(f(w[0] * c[0]) + f(w[1] * c[1])) + f(w[2] * c[2]))
    den = f(f(w[0] + w[1]) + w[2])
    xn = (f(1) - w).reshape(3, 1, 1)                                           # 1 - |xn| = w up to the rounding of xn
    w_ = np.maximum(FR.border_distance(xn, np.zeros_like(xn)), f(0))
    num = f(f(f(w_[0, 0, 0] * c[0]) + f(w_[1, 0, 0] * c[1])) + f(w_[2, 0, 0] * c[2]))
    den = f(f(w_[0, 0, 0] + w_[1, 0, 0]) + w_[2, 0, 0])
    got = FR.feather32(np.broadcast_to(c.reshape(3, 1, 1, 1), (3, 3, 1, 1)), xn, np.zeros_like(xn))
    assert got.dtype == f and (got == f(num / den)).all()
    # outside every view: 0, not 0 / 0
    far = np.full((2, 1, 1), 1.5, f)
    assert (FR.feather32(np.full((2, 3, 1, 1), 7, f), far, far) == 0).all()
    # a NaN-free clamp: a weight is never negative
    assert (np.maximum(FR.border_distance(np.array([-3.0, 0.5]), np.array([0.0, -2.0])), 0.0) == 0).all()


@pytest.mark.parametrize('mode', ['NORMAL', 'FAST'])
@pytest.mark.parametrize('seed', [11, 12])
@pytest.mark.parametrize('views', [2, 3])
@pytest.mark.parametrize('size', CASES, ids=lambda s: '%dx%d_to_%dx%d' % s)
def test_fp32_restatement_stays_inside_half_the_bound(size, views, seed, mode):
    """The calibration of feather_ref.bound on every case of the GPU sweep: the fp32 oracle's coordinates and samples
    (oracle.samplers, PyTorch on the CPU) fused by the fp32 restatement stay within half of the bound around the float64 statement;
    the comparison leaves out at most 1 % of the canvas (observed <= 0.22 %; worst ratio observed 0.08), and the views overlap."""
    h, w, hc, wc = size
    U, src, tgt, _, _ = _case(views, seed, size)
    ref = FR.feather64(U, src, tgt, hc, wc, mode)
    ox, oy = S.tps_dense_coords(T(src), T(tgt), hc, wc)
    c32 = S.tps_warp(T(U), T(src), T(tgt), (hc, wc), mode).numpy()
    o32 = FR.feather32(c32, ox.reshape(views, hc, wc).numpy(), oy.reshape(views, hc, wc).numpy())
    ratio, share = FR.worst(o32, ref, U, mode)
    assert ratio <= 0.5, (ratio, share)
    reached = (ref['w'] > 0).sum(0)
    assert (reached >= 2).mean() >= 0.15 and (reached == views).mean() >= 0.05
    b = FR.bound(ref, FR.sample_gate(U, ref, mode))
    keep = ~FR.left_out(ref) & (ref['den'] > 0)
    assert np.median(b[:, keep]) < 0.05                                   # (not vacuous: a twentieth of a grey level)


# ------------------------------------------------------------------------------------------------ the kernels of the library
def test_library_carries_the_twelve_instantiations_without_scratch(built_lib):
    """FEATHER is the fused render with another formula: 12 instantiations of render_average_kernel under its three parameter lists
    (RenderViews, GainViews: V x {fp32, u8}; Nv12Views: V x NV12OUT), told apart from AVERAGE's by the leading tag alone, with no
    scratch and no spills, and none above 64 VGPRs: 8 waves per SIMD, the step of the AVERAGE siblings or (three fp32 views: 66 / 68
    VGPRs there) one above it."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_resources as KR
    from stabstitch2_amd import _hip
    ks = KR.kernels(_hip.LIB_PATH)
    lists = G.parameter_lists(sorted(ks))
    render = {n: e for n, e in ks.items() if G.split_kernel_name(n)[0] == 'render_average_kernel'}
    feather = {n: e for n, e in render.items() if re.match(r'^(void )?render_average_kernel<FeatherFuse, ', n)}
    average = {n: e for n, e in render.items() if n not in feather}
    assert len(average) == 16 and len(feather) == 12, sorted(render)
    per_list = {}
    for n in feather:
        per_list.setdefault(G.overload_key(n, lists).split('(', 1)[1].split(',')[0], []).append(n)
    assert {k: len(v) for k, v in per_list.items()} == {'RenderViews': 4, 'GainViews': 4, 'Nv12Views': 4}, per_list
    assert {G.overload_key(n, lists) for n in feather} == {G.overload_key(n, lists) for n in average}          # no new overload key
    assert len(lists['render_average_kernel']) == 3
    for n, e in feather.items():
        assert e['.private_segment_fixed_size'] == 0 and e['.vgpr_spill_count'] == 0 and e['.sgpr_spill_count'] == 0, (n, e)
        assert e['.vgpr_count'] <= 64 and e.get('.agpr_count', 0) == 0, (n, e)
        assert e['.group_segment_fixed_size'] == (6144 if '<FeatherFuse, 3,' in n else 4096), (n, e)
