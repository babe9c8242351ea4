"""CPU-only checks of the fixed-size streaming output (online.py: viewport=, grow='refit'): the four entry points behind it exist on
all three sides of the ABI and refuse bad arguments with SS_ERR_ARG before any device work (every pointer below is host memory or
NULL, so a launch would fault instead); the device-side refit (csrc/common.h: canvas_fit_aspect / canvas_fit_update) is restated
here in numpy fp32 -- one operation after the other, as the __f*_rn intrinsics read -- and its properties are checked on seeded
boxes and extents (tests/test_gpu_viewport.py holds the kernels to this restatement bit for bit); and the kernels the library had
before the refit arrived as new instantiations of three of them keep their machine code."""
import ctypes
import functools
import os
import re
import sys

import numpy as np
import pytest

from test_host_logic import built_lib  # noqa: F401  (fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
NAMES = ('ss_canvas_watch_fit', 'ss_canvas_watch_frames_fit', 'ss_render_footprints_watch_fit', 'ss_box_fit_aspect')
F = np.float32
SLACK = F(2.5e-4)
INITIAL_ROW = (np.inf, -np.inf, np.inf, -np.inf)


# ------------------------------------------------------------------------------------------------ the restatement
def fit_aspect(box, wout, hout):
    """canvas_fit_aspect: (x0, x1, y0, y1) letterboxed about its centre to wout : hout -> four np.float32."""
    x0, x1, y0, y1 = (F(v) for v in box)
    wout, hout = F(wout), F(hout)
    with np.errstate(all='ignore'):
        ow, oh = F(x1 - x0), F(y1 - y0)
        pw, ph = F(ow * hout), F(oh * wout)
        if pw > ph:
            d = F(F(F(pw / wout) - oh) * F(0.5))
            y0, y1 = F(y0 - d), F(y1 + d)
        elif ph > pw:
            d = F(F(F(ph / hout) - ow) * F(0.5))
            x0, x1 = F(x0 - d), F(x1 + d)
    return x0, x1, y0, y1


def fit_trigger(wf, guard):
    g = F(guard) if F(guard) > SLACK else -SLACK
    lo, hi = np.fmin(F(wf[0]), F(wf[2])), np.fmax(F(wf[1]), F(wf[3]))
    return bool(lo < F(F(-1.0) + g) or hi > F(F(1.0) - g))


def fit_update(box, epoch, ext0, wf, guard, margin, zoom_limit, wout, hout):
    """canvas_fit_update on one stream's state -> (box [4], epoch, wf [4]) after it (fp32 / int; the inputs when nothing is committed)."""
    box = np.asarray(box, F)
    wf = np.asarray(wf, F)
    same = (box.copy(), int(epoch), wf.copy())
    if not fit_trigger(wf, guard):
        return same
    margin, zoom_limit, one, half = F(margin), F(zoom_limit), F(1.0), F(0.5)
    wmin, wmax, hmin, hmax = box
    with np.errstate(all='ignore'):
        ow, oh = F(wmax - wmin), F(hmax - hmin)
        x0 = F(wmin + F(F(F(np.fmin(wf[0], -one) + one) * ow) * half))
        x1 = F(wmin + F(F(F(np.fmax(wf[1], one) + one) * ow) * half))
        y0 = F(hmin + F(F(F(np.fmin(wf[2], -one) + one) * oh) * half))
        y1 = F(hmin + F(F(F(np.fmax(wf[3], one) + one) * oh) * half))
        x0, x1, y0, y1 = np.fmin(x0, wmin), np.fmax(x1, wmax), np.fmin(y0, hmin), np.fmax(y1, hmax)
        gw, gh = F(margin * F(x1 - x0)), F(margin * F(y1 - y0))
        x0, x1, y0, y1 = F(x0 - gw), F(x1 + gw), F(y0 - gh), F(y1 + gh)
        x0, x1, y0, y1 = fit_aspect((x0, x1, y0, y1), wout, hout)
        if not all(np.isfinite(v) for v in (x0, x1, y0, y1)):
            return same
        if F(x1 - x0) > F(zoom_limit * F(ext0[0])) or F(y1 - y0) > F(zoom_limit * F(ext0[1])):
            return same
        moved = np.fmax(np.fmax(F(wmin - x0), F(x1 - wmax)), np.fmax(F(hmin - y0), F(y1 - hmax)))
        if moved < half:
            return same
    return np.array([x0, x1, y0, y1], F), int(epoch) + 1, np.array(INITIAL_ROW, F)


# ------------------------------------------------------------------------------------------------ the ABI
def _ptr(buf):
    return ctypes.cast(buf, ctypes.c_void_p)


def test_canvas_fit_symbols_exist_in_library_header_and_table(built_lib):
    from stabstitch2_amd import _hip
    hdr = open(os.path.join(ROOT, 'include', 'stabstitch_hip.h')).read()
    declared = set(re.findall(r'\bSS_API[^;]*?\b(ss_[a-z0-9_]+)\s*\(', hdr))
    for name in NAMES:
        assert hasattr(built_lib, name), name
        assert name in declared, name
        assert name in _hip.SIGNATURES, name


def _state():
    return dict(src=(ctypes.c_float * 4096)(), wi=(ctypes.c_int * 16)(), wf=(ctypes.c_float * 16)(), box=(ctypes.c_float * 16)(),
                epoch=(ctypes.c_int * 4)(), ext0=(ctypes.c_float * 8)())


def _untouched(b):
    return not any(b['wi']) and not any(b['wf']) and not any(b['box']) and not any(b['epoch'])


@pytest.mark.parametrize('frames', [False, True])
def test_canvas_watch_fit_refuses_bad_arguments(built_lib, frames):
    fn = built_lib.ss_canvas_watch_frames_fit if frames else built_lib.ss_canvas_watch_fit
    b = _state()
    good = dict(src=_ptr(b['src']), n=2, views=2, guard=0.02, wi=_ptr(b['wi']), wf=_ptr(b['wf']), box=_ptr(b['box']),
                epoch=_ptr(b['epoch']), ext0=_ptr(b['ext0']), margin=0.03, zoom=2.0, hout=480, wout=640)

    def call(**kw):
        a = dict(good, **kw)
        return fn(a['src'], a['n'], a['views'], a['guard'], a['wi'], a['wf'], a['box'], a['epoch'], a['ext0'], a['margin'],
                  a['zoom'], a['hout'], a['wout'], None)

    for k in ('src', 'wi', 'wf', 'box', 'epoch', 'ext0'):
        assert call(**{k: None}) == ERR_ARG, k
    assert call(n=0) == ERR_ARG and call(n=-2) == ERR_ARG                      # streams (frames for the frames entry)
    assert call(views=0) == ERR_ARG
    for k in ('guard', 'margin', 'zoom'):
        assert call(**{k: -0.5}) == ERR_ARG and call(**{k: float('nan')}) == ERR_ARG, k
    for k in ('hout', 'wout'):
        assert call(**{k: 10}) == ERR_ARG and call(**{k: 65536}) == ERR_ARG and call(**{k: -1}) == ERR_ARG, k
    assert _untouched(b)


def test_render_footprints_watch_fit_refuses_bad_arguments(built_lib):
    b = _state()
    T, fp = (ctypes.c_float * 4096)(), (ctypes.c_float * 4096)()
    good = dict(src=_ptr(b['src']), T=_ptr(T), fp=_ptr(fp), frames=2, views=2, h=360, w=480, hc=480, wc=640, guard=0.02,
                wi=_ptr(b['wi']), wf=_ptr(b['wf']), box=_ptr(b['box']), epoch=_ptr(b['epoch']), ext0=_ptr(b['ext0']), margin=0.03,
                zoom=2.0)

    def call(**kw):
        a = dict(good, **kw)
        return built_lib.ss_render_footprints_watch_fit(a['src'], a['T'], a['fp'], a['frames'], a['views'], a['h'], a['w'], a['hc'],
                                                        a['wc'], a['guard'], a['wi'], a['wf'], a['box'], a['epoch'], a['ext0'],
                                                        a['margin'], a['zoom'], None)

    for k in ('src', 'T', 'fp', 'wi', 'wf', 'box', 'epoch', 'ext0'):
        assert call(**{k: None}) == ERR_ARG, k
    assert call(frames=0) == ERR_ARG and call(frames=-1) == ERR_ARG             # (frame = stream)
    assert call(views=0) == ERR_ARG and call(views=4) == ERR_ARG
    for k in ('guard', 'margin', 'zoom'):
        assert call(**{k: -0.5}) == ERR_ARG and call(**{k: float('nan')}) == ERR_ARG, k
    for k in ('hc', 'wc'):                                                       # the viewport is the canvas size
        assert call(**{k: 10}) == ERR_ARG and call(**{k: 65536}) == ERR_ARG, k
    assert _untouched(b) and not any(fp)


def test_box_fit_aspect_refuses_bad_arguments(built_lib):
    box, ext0 = (ctypes.c_float * 8)(), (ctypes.c_float * 4)()
    fn = built_lib.ss_box_fit_aspect
    assert fn(None, _ptr(ext0), 2, 480, 640, None) == ERR_ARG
    assert fn(_ptr(box), _ptr(ext0), 0, 480, 640, None) == ERR_ARG and fn(_ptr(box), None, -1, 480, 640, None) == ERR_ARG
    for bad in (10, 65536, 0, -5):
        assert fn(_ptr(box), _ptr(ext0), 2, bad, 640, None) == ERR_ARG and fn(_ptr(box), _ptr(ext0), 2, 480, bad, None) == ERR_ARG
    assert not any(box) and not any(ext0)


# ------------------------------------------------------------------------------------------------ properties of the restatement
def _ulp(v):
    return float(np.spacing(np.abs(F(v))))


def _cases(n, seed):
    """Seeded canvases as the stitchers meet them: extents of 40 .. 4000 px, an origin within one extent of zero (so that a
    coordinate is no larger than a few extents -- the aspect bound below counts roundings of COORDINATES in ulps of an EXTENT), running
    extents that leave the box on a random subset of its sides, viewports from 11 to 4000 px, margins 0 .. 0.1."""
    rng = np.random.default_rng(seed)
    for _ in range(n):
        ow, oh = rng.uniform(40, 4000, 2)
        x0, y0 = rng.uniform(-1, 0.2) * ow, rng.uniform(-1, 0.2) * oh
        box = np.array([x0, x0 + ow, y0, y0 + oh], F)
        sides = rng.integers(0, 2, 4).astype(bool)
        over = rng.uniform(0.0, 0.4, 4)
        inner = rng.uniform(0.5, 0.99, 4)
        wf = np.where(sides, 1.0 + over, inner) * np.array([-1, 1, -1, 1])
        yield box, wf.astype(F), tuple(int(v) for v in rng.integers(11, 4000, 2)), float(rng.uniform(0, 0.1))


def test_fit_never_moves_a_side_inward_and_commits_at_the_viewports_aspect():
    """400 seeded canvases, zoom limit out of the way: every box that comes back contains the one that went in, side by side; a commit
    leaves the box at the viewport's aspect -- |ow * Hout - oh * Wout| <= 4 ulp of either product: the letterboxed extent is a quotient
    (0.5 ulp), halved differences move two coordinates (0.5 ulp each, of coordinates no larger than the extent here), the extent and
    its product round once more each (0.5 + 0.5) -- < 3 ulp in all, 4 asserted; a commit resets the extents and counts one epoch."""
    commits = 0
    for box, wf, (hout, wout), margin in _cases(400, 7):
        ext0 = (box[1] - box[0], box[3] - box[2])
        nb, ep, nwf = fit_update(box, 3, ext0, wf, 0.02, margin, 1e6, wout, hout)
        assert nb[0] <= box[0] and nb[1] >= box[1] and nb[2] <= box[2] and nb[3] >= box[3], (box, nb)
        if ep == 3:
            assert (nb == box).all() and (nwf == wf).all()
            continue
        commits += 1
        assert ep == 4 and tuple(nwf) == INITIAL_ROW and fit_trigger(wf, 0.02)
        a, b = F(F(nb[1] - nb[0]) * F(hout)), F(F(nb[3] - nb[2]) * F(wout))
        assert abs(float(a) - float(b)) <= 4 * max(_ulp(a), _ulp(b)), (box, nb, hout, wout, a, b)
    assert commits > 250, commits


def test_aspect_step_alone():
    """It only expands, about the centre, on one axis; equal products are left alone bit for bit; the result sits at the viewport's
    aspect within the same 4 ulp."""
    for box, _, (hout, wout), _ in _cases(300, 11):
        nb = np.array(fit_aspect(box, wout, hout), F)
        assert nb[0] <= box[0] and nb[1] >= box[1] and nb[2] <= box[2] and nb[3] >= box[3]
        assert (nb[0] == box[0] and nb[1] == box[1]) or (nb[2] == box[2] and nb[3] == box[3])
        a, b = F(F(nb[1] - nb[0]) * F(hout)), F(F(nb[3] - nb[2]) * F(wout))
        assert abs(float(a) - float(b)) <= 4 * max(_ulp(a), _ulp(b)), (box, nb, hout, wout)
    for box, vp in (((-64, 576, -60, 420), (480, 640)), ((0, 1280, 0, 720), (360, 640)), ((3, 14, 5, 16), (11, 11))):
        assert tuple(fit_aspect(box, vp[1], vp[0])) == tuple(F(v) for v in box)


def test_trigger_is_false_for_the_initial_row_and_inside_the_guard():
    for guard in (0.0, 1e-4, 0.02, 0.5):
        assert not fit_trigger(INITIAL_ROW, guard)
        box = np.array([-64, 576, -60, 420], F)
        nb, ep, nwf = fit_update(box, 0, (640, 480), INITIAL_ROW, guard, 0.03, 2.0, 640, 480)
        assert (nb == box).all() and ep == 0 and tuple(nwf) == INITIAL_ROW
    assert not fit_trigger((-0.9, 0.9, -0.9, 0.9), 0.05) and fit_trigger((-0.96, 0.9, -0.9, 0.9), 0.05)
    assert fit_trigger((-0.9, 0.9, -0.9, 0.951), 0.05)
    # a guard below the rounding slack: only a point beyond the edge by more than the slack asks for a growth
    assert not fit_trigger((-1.0, 1.0, -1.0, 1.0002), 0.0) and fit_trigger((-1.0, 1.0, -1.0, 1.0003), 0.0)


def test_the_three_refusals_leave_every_output_equal_to_its_input():
    box = np.array([-64, 576, -60, 420], F)
    ext0 = (640, 480)

    def unchanged(wf, margin=0.03, zoom=2.0, b=box, e0=ext0, vp=(480, 640)):
        nb, ep, nwf = fit_update(b, 5, e0, wf, 0.02, margin, zoom, vp[1], vp[0])
        return np.array_equal(nb, np.asarray(b, F), equal_nan=True) and ep == 5 and (nwf == np.asarray(wf, F)).all()

    grows = (-1.2, 0.9, -0.9, 0.9)
    assert not unchanged(grows)                                                  # (the case below the refusals does commit)
    # a coordinate that is not finite: extents that overflow fp32 once scaled to pixels, and a box that is not finite itself
    assert unchanged((-3e38, 0.9, -0.9, 0.9), zoom=float('inf'))
    assert unchanged(grows, b=(-64, np.inf, -60, 420), zoom=float('inf'))
    assert unchanged(grows, b=(np.nan, 576, -60, 420), zoom=float('inf'))
    # an extent beyond zoom_limit x the initial one -- in x, in y, and through the letterbox alone
    assert unchanged((-3.5, 0.9, -0.9, 0.9)) and unchanged((-0.9, 0.9, -0.9, 3.5))
    assert unchanged((-2.5, 0.9, -0.9, 0.9), e0=(640, 300))
    assert not unchanged((-2.5, 0.9, -0.9, 0.9), zoom=4.0)
    # every side moved by less than half a pixel: margin 0 and a mesh that only touches the edge
    assert unchanged((-1.001, 0.9, -0.9, 0.9), margin=0.0) and unchanged((-1.0, 1.0, -1.0, 1.0), margin=0.0)
    assert not unchanged((-1.01, 0.9, -0.9, 0.9), margin=0.0)


# ------------------------------------------------------------------------------------------------ the old kernels keep their code
def norm(name):
    """A demangled kernel name as the listings compare it: without the leading `void `, and with three spellings undone that a
    source-only change gives a kernel whose machine code stays.  A flag template whose flag = 0 form is the old plain function: `<0>`
    dropped.  A kernel that became a template on its descriptor (the type of its first parameter): the trailing `, XxxViews`
    template argument dropped when it equals that type.  render_average_kernel's GainViews form, once a template of its own
    without the FOLD flag and now an instantiation of the common one: its `, false` for FOLD dropped."""
    name = re.sub(r'^(\w+)<0>\(', r'\1(', re.sub(r'^void ', '', name))
    name = re.sub(r'^(\w+<[^()]*?), (\w+Views)>\(\2([,)])', r'\1>(\2\3', name)
    return re.sub(r'^(render_average_kernel<\d, \w+), false>\(GainViews,', r'\1>(GainViews,', name)


@functools.lru_cache(maxsize=None)
def built_digests():
    """tools/kernel_resources.py --digest-masked of the built library, by normalised name (disassembled once for both listings)."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_resources as KR
    from stabstitch2_amd import _hip
    return {norm(k): v for k, v in KR.digests(_hip.LIB_PATH, mask_kernarg_offsets=True).items()}


def check_listing(listing, count):
    """The built library against a committed listing of `count` kernels: every kernel of the listing is still in the library, under
    its normalised name, with the same instruction stream."""
    parent = {}
    for ln in open(os.path.join(ROOT, 'tests', 'golden', listing)):
        digest, name = ln.rstrip('\n').split('  ', 1)
        parent[norm(name)] = digest
    assert len(parent) == count
    have = built_digests()
    assert not sorted(set(parent) - set(have)), 'kernels that left the library'
    changed = sorted(k for k in parent if have[k] != parent[k])
    assert not changed, 'kernels whose machine code changed: %s' % changed


def test_kernels_from_before_the_refit_keep_their_machine_code(built_lib):
    """tools/kernel_resources.py --digest-masked on the built library against the listing taken from the library before the refit
    (tests/golden/viewport_parent_isa_digest.txt, same compiler and flags): every kernel instantiation that library had is still
    there with the same instruction stream.  The refit rides on canvas_watch_kernel, canvas_watch_frames_kernel and
    render_lattice_kernel as a compile-time flag; their flag = 0 instantiations are the kernels as they were (a name that gained
    `<0>` is the same kernel).  A later change that edits a kernel on purpose regenerates the listing with that command."""
    check_listing('viewport_parent_isa_digest.txt', 144)


def test_kernels_from_before_the_render_unification_keep_their_machine_code(built_lib):
    """The same against the listing of the library before render.hip's kernel copies were folded into templates on the view
    descriptor (tests/golden/render_unify_parent_isa_digest.txt: all 175 kernels of that library, the NV12 and exposure kernels the
    listing above predates among them).  The listing is the PARENT's: a source-only change of the kernels is accepted when this
    passes unedited (LAB_NOTES.md, "Source-only changes"), and a change that edits a kernel on purpose regenerates it."""
    check_listing('render_unify_parent_isa_digest.txt', 175)
