"""CPU-only checks of the NV12 frame format ("Frame formats"): the four entry points exist on all three sides of the ABI
and refuse a surface they cannot read -- odd height or width, an odd pitch, a pitch below the width, a UV plane that is not 2-byte
aligned, an odd canvas for NV12 output -- with SS_ERR_ARG before any device work (every pointer below is host memory or NULL, so a
launch would fault instead); and the two colour statements of tests/nv12_ref.py, which the GPU tests hold the kernels to byte for
byte, are themselves held to the real-valued BT.601 formulas over all 2^24 byte triples."""
import ctypes
import os
import re

import numpy as np

import nv12_ref as N
from test_host_logic import built_lib  # noqa: F401  (fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
NAMES = ('ss_ingest_nv12', 'ss_bgr_to_nv12', 'ss_render_average_nv12', 'ss_render_linear_frames_nv12')


def test_nv12_symbols_exist_in_library_header_and_table(built_lib):
    from stabstitch2_amd import _hip
    hdr = open(os.path.join(ROOT, 'include', 'stabstitch_hip.h')).read()
    declared = set(re.findall(r'\bSS_API[^;]*?\b(ss_[a-z0-9_]+)\s*\(', hdr))
    for name in NAMES:
        assert hasattr(built_lib, name), name
        assert name in declared, name
        assert name in _hip.SIGNATURES, name
    assert len(declared) >= 104 and sorted(declared) == sorted(_hip.SIGNATURES)


# ------------------------------------------------------------------------------------------------ refusals
class _Host:
    """Host buffers standing in for device memory: a refused call never reads them, and `untouched` says that none was written."""

    def __init__(self):
        self.bufs = {k: (ctypes.c_ubyte * 8192)() for k in ('y', 'y2', 'y3', 'out', 'out_uv', 'hr', 'lr', 'src', 'T', 'ws')}

    def p(self, k, off=0):
        return ctypes.c_void_p(ctypes.addressof(self.bufs[k]) + off)

    def even(self, k):                              # an address inside the buffer that IS 2-byte aligned
        return ctypes.addressof(self.bufs[k]) & 1

    def untouched(self):
        return not any(any(b) for b in self.bufs.values())


BAD_SURFACES = (dict(h=13), dict(w=17), dict(pitch=19), dict(pitch=14), dict(uv_off=1), dict(h=0), dict(w=-2))


def test_ingest_nv12_refuses_bad_surfaces(built_lib):
    b = _Host()
    good = dict(h=12, w=16, pitch=16, uv_off=0, fs=0, n=1, lr_h=6, lr_w=8, y='y', hr='hr', lr='lr')

    def call(**kw):
        a = dict(good, **kw)
        y = b.p(a['y'], b.even('y')) if a['y'] else None
        uv = b.p('y', b.even('y') + 4096 + a['uv_off']) if a.get('uv', True) else None
        return built_lib.ss_ingest_nv12(y, uv, a['pitch'], a['fs'], b.p('hr') if a['hr'] else None, b.p('lr') if a['lr'] else None,
                                        a['n'], a['h'], a['w'], a['lr_h'], a['lr_w'], None)

    for bad in BAD_SURFACES:
        assert call(**bad) == ERR_ARG, bad
    assert call(y=None) == ERR_ARG and call(uv=None) == ERR_ARG and call(hr=None, lr=None) == ERR_ARG
    assert call(n=-1) == ERR_ARG and call(fs=-2) == ERR_ARG and call(fs=193, n=2) == ERR_ARG
    assert call(lr_h=0) == ERR_ARG and call(lr_w=0) == ERR_ARG
    assert call(n=0) == 0                                                        # (nothing to do is not an error, and launches nothing)
    assert b.untouched()


def test_bgr_to_nv12_refuses_bad_surfaces(built_lib):
    b = _Host()
    good = dict(h=12, w=16, pitch=16, uv_off=0, fs=0, n=1)

    def call(bgr=True, y=True, uv=True, **kw):
        a = dict(good, **kw)
        return built_lib.ss_bgr_to_nv12(b.p('out') if bgr else None, b.p('y', b.even('y')) if y else None,
                                        b.p('y', b.even('y') + 4096 + a['uv_off']) if uv else None, a['pitch'], a['fs'], a['n'],
                                        a['h'], a['w'], None)

    for bad in BAD_SURFACES:
        assert call(**bad) == ERR_ARG, bad
    assert call(bgr=False) == ERR_ARG and call(y=False) == ERR_ARG and call(uv=False) == ERR_ARG
    assert call(n=-1) == ERR_ARG and call(fs=-2) == ERR_ARG and call(fs=289, n=2) == ERR_ARG
    assert call(n=0) == 0
    assert b.untouched()


def _views(b, views, a):
    ks = ('y', 'y2', 'y3')[:views]
    ys = (ctypes.c_void_p * views)(*[ctypes.addressof(b.bufs[k]) + b.even(k) for k in ks])
    uvs = (ctypes.c_void_p * views)(*[ctypes.addressof(b.bufs[k]) + b.even(k) + 4096 + (a['uv_off'] if i == a['which'] else 0)
                                      for i, k in enumerate(ks)])
    pitches = (ctypes.c_int * views)(*[a['pitch'] if i == a['which'] else 16 for i in range(views)])
    return ys, uvs, pitches


def test_render_average_nv12_refuses_bad_surfaces(built_lib):
    b = _Host()
    good = dict(h=12, w=16, pitch=16, uv_off=0, which=0, views=2, hc=18, wc=70, fmt=0, opitch=70, ouv_off=0, mode=0)

    def call(out=True, ouv=True, **kw):
        a = dict(good, **kw)
        ys, uvs, pitches = _views(b, max(a['views'], 1) if a['views'] <= 3 else 3, a)
        return built_lib.ss_render_average_nv12(ys, uvs, pitches, b.p('src'), b.p('T'), None, 0, b.p('out') if out else None,
                                                b.p('out_uv', b.even('out_uv') + a['ouv_off']) if ouv else None, a['opitch'],
                                                a['fmt'], a['views'], a['h'], a['w'], a['hc'], a['wc'], a['mode'], None)

    for which in (0, 1):
        for bad in BAD_SURFACES:
            assert call(which=which, **bad) == ERR_ARG, (which, bad)
    assert call(views=3, which=2, pitch=17) == ERR_ARG and call(views=1) == ERR_ARG and call(views=4) == ERR_ARG
    assert call(out=False) == ERR_ARG and call(mode=2) == ERR_ARG and call(mode=16) == ERR_ARG and call(fmt=2) == ERR_ARG
    # NV12 out: an even canvas, an even output pitch >= wc, an aligned UV plane that is there
    nv = dict(fmt=1, hc=18, wc=70, opitch=70)
    for bad in (dict(hc=19), dict(wc=71), dict(opitch=71), dict(opitch=68), dict(ouv_off=1)):
        assert call(**dict(nv, **bad)) == ERR_ARG, bad
    assert call(ouv=False, **nv) == ERR_ARG
    assert b.untouched()


def test_render_linear_frames_nv12_refuses_bad_surfaces(built_lib):
    b = _Host()
    good = dict(h=12, w=16, pitch=16, uv_off=0, which=0, views=2, hc=18, wc=70, mode=0, fs=0, frames=1)

    def call(ws=True, strides=True, **kw):
        a = dict(good, **kw)
        v = min(max(a['views'], 1), 3)
        ys, uvs, pitches = _views(b, v, a)
        fs = (ctypes.c_longlong * v)(*[a['fs'] if i == a['which'] else 0 for i in range(v)])
        outs = (ctypes.c_void_p * 1)(ctypes.addressof(b.bufs['out']))
        hc, wc = (ctypes.c_int * 1)(a['hc']), (ctypes.c_int * 1)(a['wc'])
        return built_lib.ss_render_linear_frames_nv12(ys, uvs, pitches, fs if strides else None, b.p('src'), b.p('T'), outs,
                                                      a['frames'], a['views'], a['h'], a['w'], hc, wc, a['mode'],
                                                      b.p('ws') if ws else None, None)

    for which in (0, 1):
        for bad in BAD_SURFACES:
            assert call(which=which, **bad) == ERR_ARG, (which, bad)
    assert call(views=3, which=2, uv_off=1) == ERR_ARG and call(views=1) == ERR_ARG and call(views=4) == ERR_ARG
    assert call(fs=-2) == ERR_ARG and call(fs=289) == ERR_ARG and call(strides=False) == ERR_ARG
    assert call(ws=False) == ERR_ARG and call(frames=0) == ERR_ARG and call(frames=33) == ERR_ARG and call(mode=2) == ERR_ARG
    assert call(hc=10) == ERR_ARG and call(wc=65536) == ERR_ARG
    assert b.untouched()


# ------------------------------------------------------------------------------------------------ the colour statements
def test_nv12_to_bgr_stays_within_one_grey_level_of_bt601():
    """All 2^24 (Y, U, V) triples against the real-valued BT.601 limited-range matrix (255/219 on luma below; luma under 16 counts
    as 16, as in the statement; both sides clamped to 0..255).  The statement's constants are that matrix rounded to three decimals
    in 20-bit fixed point: 239 * (255/219 - 1.164) = 0.09 of drift plus 0.5 of rounding and the chroma coefficients' 1e-3 -- the
    gate is one grey level; 0.69 is what comes out."""
    U, V = np.meshgrid(np.arange(256), np.arange(256), indexing='ij')
    u, v = U - 128.0, V - 128.0
    worst = 0.0
    for Y in range(256):
        B, G, R = N.yuv_to_bgr(np.full_like(U, Y), U, V)
        c = max(0, Y - 16) * 255.0 / 219.0
        real = (np.clip(c + 2.017232 * u, 0, 255), np.clip(c - 0.391762 * u - 0.812968 * v, 0, 255), np.clip(c + 1.596027 * v, 0, 255))
        worst = max(worst, max(float(np.abs(got - ref).max()) for got, ref in zip((B, G, R), real)))
    print('max |statement - BT.601| = %.4f grey levels' % worst)
    assert worst <= 1.0, worst


def test_bgr_to_nv12_maps_every_byte_triple_into_the_limited_range_without_a_clamp():
    G, R = np.meshgrid(np.arange(256), np.arange(256), indexing='ij')
    lo, hi = [1 << 30] * 3, [-(1 << 30)] * 3
    for B in range(256):
        for i, a in enumerate((N.bgr_to_y(B, G, R),) + N.bgr_to_uv(B, G, R)):
            lo[i], hi[i] = min(lo[i], int(a.min())), max(hi[i], int(a.max()))
    assert (lo, hi) == ([16, 16, 16], [235, 240, 240]), (lo, hi)
    # black: what a tile that no view reaches must hold
    assert int(N.bgr_to_y(0, 0, 0)) == 16 and tuple(int(a) for a in N.bgr_to_uv(0, 0, 0)) == (128, 128)


def test_round_trip_of_in_gamut_triples():
    """(Y, U, V) -> B, G, R -> (Y, U, V) over every triple with Y >= 16 whose three colour values need no clamp (a uniform 2 x 2
    block: its rounded mean is the pixel): Y comes back within 1, U and V exactly."""
    U, V = np.meshgrid(np.arange(256), np.arange(256), indexing='ij')
    u, v = U - 128, V - 128
    dy = du = dv = seen = 0
    for Y in range(16, 256):
        c = (Y - 16) * 1220542 + N.HALF
        raw = ((c + 2116026 * u) >> 20, (c - 409993 * u - 852492 * v) >> 20, (c + 1673527 * v) >> 20)
        ok = np.ones(U.shape, bool)
        for a in raw:
            ok &= (a >= 0) & (a <= 255)
        if not ok.any():
            continue
        B, G, R = N.yuv_to_bgr(np.full_like(U, Y), U, V)
        assert all((got == a)[ok].all() for got, a in zip((B, G, R), raw))
        u2, v2 = N.bgr_to_uv(B, G, R)
        seen += int(ok.sum())
        dy = max(dy, int(np.abs(N.bgr_to_y(B, G, R) - Y)[ok].max()))
        du, dv = max(du, int(np.abs(u2 - U)[ok].max())), max(dv, int(np.abs(v2 - V)[ok].max()))
    assert seen > 2_000_000, seen
    assert (dy, du, dv) == (1, 0, 0), (dy, du, dv)


def test_frame_functions_agree_with_the_per_pixel_statements():
    """nv12_to_bgr / bgr_to_nv12 on a small frame against the scalar statements spelled out pixel by pixel: the plane layout, the
    (y >> 1, x >> 1) chroma pair, U before V, and the rounded 2 x 2 mean."""
    rng = np.random.default_rng(3)
    h, w = 6, 8
    f = N.random_nv12(rng, h, w)
    bgr = N.nv12_to_bgr(f)
    for y in range(h):
        for x in range(w):
            U, V = int(f[h + (y >> 1), (x >> 1) * 2]), int(f[h + (y >> 1), (x >> 1) * 2 + 1])
            assert tuple(bgr[y, x]) == tuple(int(a) for a in N.yuv_to_bgr(int(f[y, x]), U, V))
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    nv = N.bgr_to_nv12(img)
    assert nv.shape == (9, 8)
    for y in range(h):
        for x in range(w):
            assert int(nv[y, x]) == int(N.bgr_to_y(*[int(c) for c in img[y, x]]))
    for by in range(h // 2):
        for bx in range(w // 2):
            m = [(int(img[2 * by:2 * by + 2, 2 * bx:2 * bx + 2, c].astype(int).sum()) + 2) >> 2 for c in range(3)]
            assert (int(nv[h + by, 2 * bx]), int(nv[h + by, 2 * bx + 1])) == tuple(int(a) for a in N.bgr_to_uv(*m))
