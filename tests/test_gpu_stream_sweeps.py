"""The kernels that the streaming features added as overloads of existing names -- the exposure estimator, the NV12 ingest kernels,
BGR -> NV12 and the NV12 AVERAGE render -- at the shapes where their indexing can go wrong and which their feature tests
(test_gpu_exposure.py, test_gpu_nv12.py) do not reach: a lattice of more than one wave and more than one trip of the stride loop;
frames wider than one 64-column block, upscaled, 2 x 2, and cut from a taller buffer (a frame stride larger than the frame);
canvases that are one tile, exact tile multiples, one pixel or one 2 x 2 block past a tile, and odd.  The gates are the feature
tests': the estimator against the float64 statement of tests/exposure_ref.py, the byte kernels bit for bit against numpy
(tests/nv12_ref.py, oracle/frame_io.py), the NV12 render bit for bit against the packed-BGR render of the converted frames (which
test_gpu_kernel_sweeps.py roots in float64).  sweep_inputs.library_reach cites these tests for those kernels.
    python -m pytest tests/test_gpu_stream_sweeps.py -m gpu"""
import numpy as np
import pytest
import torch

import exposure_ref as E
import nv12_ref as N
import test_gpu_exposure as X
import test_gpu_nv12 as V12
from test_gpu_linear_frames import _kernel_names
from test_gpu_parity import dev  # noqa: F401  (fixture)
from test_gpu_rest_sweeps import canaried, canaries_intact, lr_reference, same_bits

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
F32 = np.float32
PAD = V12.PAD
FILL = 0xAB


# ================================================================================================ a. the exposure estimator
WIDE = 'c'                                  # test_gpu_exposure.WIDE_CASES: frames (37, 53) on canvas (201, 330), 27 x 13 = 351 nodes
WIDE_RANGES = [(0, 64), (64, 128), (128, 192), (192, 256), (256, 351)]      # the four waves' first trip, and the second trip
WIDE_ON_CANVAS = [55, 55, 54, 54, 68]       # nodes on the canvas per range (the last lattice row and the last two columns are not)


@pytest.mark.parametrize('mode', ['NORMAL', 'FAST'])
@pytest.mark.parametrize('u8', [False, True], ids=['fp32', 'uint8'])
@pytest.mark.parametrize('views', [2, 3])
def test_exposure_beyond_one_wave_and_one_trip(dev, views, u8, mode):
    """test_gpu_exposure.test_statistics_targets_and_smoothing (its assertions, its derived bounds: check_estimator) on a lattice of
    351 nodes, 286 of them on the canvas: every wave of the workgroup holds nodes, and threads 0 .. 94 take a second trip of the
    stride loop.  In every frame but the one without overlap, pair (0, 1) has at least 8 usable nodes in each of the index ranges
    [0, 64), [64, 128), [128, 192), [192, 256) and [256, 351) -- V = 2: 25, 25, 25, 25, 30; V = 3: 15, 15, 15, 15, 18, measured on
    the float64 lattice of the same meshes before the first run on a GPU -- so a wrong partial of waves 1 .. 3, a wrong order of
    their sum (fp64, but the counts are exact) or a wrong stride changes a count or a sum beyond its bound."""
    h, w, hc, wc = X.WIDE_CASES[WIDE][:4]
    ny, nx = E.lattice_shape(hc, wc)
    assert (ny, nx) == (27, 13) and WIDE_RANGES[-1][1] == ny * nx
    oc = E.on_canvas(hc, wc).reshape(-1)
    assert [int(oc[a:b].sum()) for a, b in WIDE_RANGES] == WIDE_ON_CANVAS
    reached = X.check_estimator(dev, WIDE, views, u8, mode, ranges=WIDE_RANGES)
    print('\n[exposure %s V=%d %s %s] usable nodes of pair (0, 1) per index range and frame: %s' % (
        WIDE, views, 'uint8' if u8 else 'fp32', mode, reached))
    assert len(reached) == X.NF and reached[2] == [0] * len(WIDE_RANGES)


# ================================================================================================ b. NV12 ingest
def _nv12_batch(dev, seed, n, h, w, pad, gap):
    """n random NV12 frames [n,h*3/2,w] -> (numpy frames, the device batch: a view of a buffer [n, h*3/2 + gap, w + pad] of other
    random bytes -- pitch w + pad, frame stride (h*3/2 + gap) rows)."""
    rng = np.random.default_rng(seed)
    rows = h // 2 * 3
    dense = np.stack([N.random_nv12(rng, h, w) for _ in range(n)], 0)
    buf = np.random.default_rng(seed + 1).integers(0, 256, (n, rows + gap, w + pad), dtype=np.uint8)
    buf[:, :rows, :w] = dense
    return dense, torch.from_numpy(buf).to(dev)[:, :rows, :w]


@pytest.mark.parametrize('gap', [0, 2], ids=['frames', 'strided'])
@pytest.mark.parametrize('pad', [0, PAD], ids=['dense', 'padded'])
@pytest.mark.parametrize('h,w,lr_h,lr_w', [
    (6, 130, 6, 130),       # same size (mode 2): three 64-column blocks of HR and of LR pixels
    (8, 132, 4, 66),        # exact half (mode 1): two LR blocks
    (6, 130, 5, 71),        # a general downscale (mode 0): two LR blocks
    (4, 6, 9, 13),          # an upscale: the source index goes negative at the left / top edge
    (2, 2, 1, 1),           # the smallest surface: one chroma row, one chroma pair; exact half
    (2, 2, 3, 3),           # ... upscaled
], ids=lambda v: str(v))
def test_ingest_nv12_paths_bit_exact(dev, h, w, lr_h, lr_w, pad, gap):
    """ss_ingest_nv12, n = 3, against numpy alone: nv12_ref.nv12_to_bgr, then the plane split (uint8 -> fp32) and the LR resize of
    oracle/frame_io.py in its three modes -- the shapes of test_gpu_rest_sweeps.test_ingest_u8_paths_bit_exact, even.  The batch is
    dense, has a padded pitch, is cut from a taller buffer (two gap rows between the frames), or both; padding and gap rows hold
    other random bytes.  The outputs sit between canaries."""
    from stabstitch2_amd import ops
    n = 3
    dense, nv = _nv12_batch(dev, 31000 + 131 * h + w + lr_w, n, h, w, pad, gap)
    assert nv.stride(1) == w + pad and nv.stride(0) == (h // 2 * 3 + gap) * (w + pad)
    bgr = np.stack([N.nv12_to_bgr(f) for f in dense], 0)
    want_hr = np.ascontiguousarray(bgr.transpose(0, 3, 1, 2)).astype(F32)
    want_lr = lr_reference(bgr, lr_h, lr_w)
    hb, hr = canaried(n * 3 * h * w, dev)
    lb, lr = canaried(n * 3 * lr_h * lr_w, dev)
    what = '%dx%d -> %dx%d pad %d gap %d' % (h, w, lr_h, lr_w, pad, gap)
    ops.ingest_nv12(nv, lr_h, lr_w, hr_out=hr.view(n, 3, h, w), lr_out=lr.view(n, 3, lr_h, lr_w))
    same_bits(hr.view(n, 3, h, w), want_hr, 'ingest_nv12 hr ' + what)
    same_bits(lr.view(n, 3, lr_h, lr_w), want_lr, 'ingest_nv12 lr ' + what)
    canaries_intact(hb, n * 3 * h * w, 'ingest_nv12 hr')
    canaries_intact(lb, n * 3 * lr_h * lr_w, 'ingest_nv12 lr')
    lb2, lr2 = canaried(n * 3 * lr_h * lr_w, dev)
    none, lr_only = ops.ingest_nv12(nv, lr_h, lr_w, want_hr=False, lr_out=lr2.view(n, 3, lr_h, lr_w))
    assert none is None
    same_bits(lr_only, want_lr, 'ingest_nv12 lr alone ' + what)
    canaries_intact(lb2, n * 3 * lr_h * lr_w, 'ingest_nv12 lr alone')


# ================================================================================================ c. BGR -> NV12
@pytest.mark.parametrize('size', [(2, 2), (10, 260)], ids=lambda v: str(v))
def test_bgr_to_nv12_into_strided_frames(dev, size):
    """ss_bgr_to_nv12, n = 3, into frames cut from a taller and wider buffer: pitch w + 14, frame stride two rows more than the
    frame.  Every frame equals nv12_ref.bgr_to_nv12; padding and gap rows keep their fill.  (10, 260): three 64-block columns and
    two 4-block rows of 2 x 2 blocks, the last of each partial."""
    from stabstitch2_amd import ops
    h, w = size
    n, rows, gap = 3, h // 2 * 3, 2
    bgr = np.random.default_rng(41 + w).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    ref = np.stack([N.bgr_to_nv12(f) for f in bgr], 0)
    buf = torch.full((n, rows + gap, w + PAD), FILL, dtype=torch.uint8, device=dev)
    out = buf[:, :rows, :w]
    res = ops.bgr_to_nv12(torch.from_numpy(bgr).to(dev), out=out)
    same_bits(res, ref, 'bgr_to_nv12 %dx%d' % (h, w))
    untouched = torch.ones_like(buf, dtype=torch.bool)
    untouched[:, :rows, :w] = False
    assert bool((buf[untouched] == FILL).all()), 'bgr_to_nv12 wrote into the padding or the gap rows'


# ================================================================================================ d. the NV12 AVERAGE render
# canvas (hc, wc) -> its box (wmin, wmax, hmin, hmax) in HR px for frames (24, 36), whose views lie on about [0, 36 + 6 (V - 1)] x
# [0, 24]: wider and taller than the views, so that a picture and black both occur.  (2, 2): the canvas' four pixels are the
# box's corners -- two inside views, two beyond them.
EDGE_CANVASES = {
    (2, 2): (10.0, 60.0, 5.0, 20.0),        # the smallest canvas the entry point accepts
    (8, 64): (-14.0, 62.0, -10.0, 34.0),    # exactly one tile
    (16, 128): (-14.0, 62.0, -10.0, 34.0),  # exact tile multiples: no lane past an edge
    (10, 66): (-14.0, 62.0, -10.0, 34.0),   # one 2 x 2 block into the next tile each way
    (9, 65): (-14.0, 62.0, -10.0, 34.0),    # odd: the row at y = 8 has no partner (rowb == false); a last tile column of one pixel
    (7, 63): (-14.0, 62.0, -10.0, 34.0),    # odd: one short of a tile each way
}
# frames (2, 2): view v's frame lies on [6 v, 6 v + 2] x [0, 2] HR px, but what a sampler shows of it does not: the clamped sampler
# of NORMAL has content only where its two taps differ, [6 v, 6 v + 1) x [0, 1); the zero-padded sampler of FAST, whose taps are
# one source pixel = the whole frame apart, wherever one tap is inside, (6 v - 2, 6 v + 4) x (-2, 4).  One box per mode, so that
# both show a picture of more than 50 pixels and more than a quarter of black for two and for three views
SMALL_FRAME_BOX = {'NORMAL': (-0.25, 7.25, -0.25, 1.25), 'FAST': (-14.0, 22.0, -5.0, 7.0)}


def _edge_runs(mode):
    """-> [(frame (h, w), canvas (hc, wc), box)] of test_render_average_nv12_at_the_tile_edges"""
    return [((24, 36), c, EDGE_CANVASES[c]) for c in EDGE_CANVASES] + [((2, 2), c, SMALL_FRAME_BOX[mode]) for c in ((9, 65), (10, 66))]


FOOTPRINT_REFUSED = ()                      # canvases ops.render_footprints refuses: none of these


def _render_frames(dev, seed, h, w, pad):
    """One random NV12 frame with pitch w + pad (luma >= 32: no pixel of a frame converts to black, so black on the canvas means
    outside every view) -> (device NV12 [h*3/2,w], its conversion uint8 [h,w,3])."""
    rng = np.random.default_rng(seed)
    dense = N.random_nv12(rng, h, w)
    dense[:h] = 32 + dense[:h] % 224
    padding = np.random.default_rng(seed + 1).integers(0, 256, (h // 2 * 3, pad), dtype=np.uint8)
    bgr = N.nv12_to_bgr(dense)
    assert int(bgr.sum(-1).min()) > 0
    return V12._surface(dev, np.concatenate((dense, padding), 1), w), torch.from_numpy(bgr).to(dev)


@pytest.mark.parametrize('pad', [0, PAD], ids=['dense', 'padded'])
@pytest.mark.parametrize('footprint', [False, True], ids=['everywhere', 'footprint'])
@pytest.mark.parametrize('mode', ['NORMAL', 'FAST'])
@pytest.mark.parametrize('views', [2, 3])
def test_render_average_nv12_at_the_tile_edges(dev, views, mode, footprint, pad):
    """ops.render_average_nv12 against ops.render_average_u8 on the converted frames, byte for byte, on the canvases of
    EDGE_CANVASES with frames (24, 36), and on (9, 65) and (10, 66) with frames (2, 2) (one chroma row).  BGR output on every
    canvas, into a tensor between canaries; NV12 output on the even ones against nv12_ref.bgr_to_nv12 of the BGR result, into a
    padded surface whose padding keeps its fill.  ops.render_footprints accepts every one of these canvases (FOOTPRINT_REFUSED is
    empty): all of them run with and without footprint.  Every canvas shows a picture and black."""
    from stabstitch2_amd import _hip as H, ops
    runs = _edge_runs(mode)
    for (h, w), (hc, wc), box in runs:
        boxes = tuple(b for (f, _, b) in runs if f == (h, w))
        src, T = V12._splines(dev, views, h, w, boxes)
        i = [c for (f, c, _) in runs if f == (h, w)].index((hc, wc))
        what = (h, w, hc, wc)
        fp = None
        if footprint:
            try:
                fp = ops.render_footprints(src[i:i + 1], T[i:i + 1], h, w, hc, wc)[0]
            except H.HipError:
                assert (hc, wc) in FOOTPRINT_REFUSED, what
                continue
            assert (hc, wc) not in FOOTPRINT_REFUSED, what
        per_view = [_render_frames(dev, 700 + 10 * v + h, h, w, pad) for v in range(views)]
        nv, bgr = [p[0] for p in per_view], [p[1] for p in per_view]
        ref = ops.render_average_u8(bgr, src[i], T[i], hc, wc, mode, footprint=fp)
        buf, mid = canaried(hc * wc * 3, dev, dtype=torch.uint8, value=FILL)
        got = ops.render_average_nv12(nv, src[i], T[i], hc, wc, mode, footprint=fp, out=mid.view(hc, wc, 3))
        same_bits(got, ref.cpu().numpy(), 'render_average_nv12 bgr %s' % (what,))
        canaries_intact(buf, hc * wc * 3, 'render_average_nv12 bgr %s' % (what,), value=FILL)
        if hc % 2 == 0 and wc % 2 == 0:
            sbuf, out = V12._padded_out(dev, hc // 2 * 3, wc, PAD)
            res = ops.render_average_nv12(nv, src[i], T[i], hc, wc, mode, footprint=fp, out_format='nv12', out=out)
            same_bits(res, N.bgr_to_nv12(ref.cpu().numpy()), 'render_average_nv12 nv12 %s' % (what,))
            assert bool((sbuf[:, wc:] == FILL).all()), what
        # the case is what it claims: samples inside the frames (a picture) and outside them (black)
        px = ref.view(-1, 3).sum(1)
        assert int((px == 0).sum()) > hc * wc // 4 and int((px > 0).sum()) > min(50, hc * wc // 4), (what, int((px == 0).sum()), int((px > 0).sum()))


# ================================================================================================ e. the launches
def test_the_overloads_are_what_is_launched(dev):
    """The smallest call of each of a. to d. under torch.profiler: the launched kernels include the overload that the coverage
    table's row names, told by its parameter list -- ExposureArgs, Nv12Views, the two-plane pointer lists of the NV12 ingest and
    of BGR -> NV12.  Should the profiler report names without parameter lists, base name and template arguments are matched
    instead (the NV12 ingest and BGR -> NV12 kernels then by base name alone) and the test says so in its output."""
    from stabstitch2_amd import ops
    c = X._case(dev, 'a', 2)
    st = ops.exposure_state(dev)
    dense, nv = _nv12_batch(dev, 5, 1, 2, 2, 0, 0)
    bgr = torch.from_numpy(np.stack([N.nv12_to_bgr(f) for f in dense], 0)).to(dev)
    src, T = V12._splines(dev, 2, 24, 36, tuple(b for (f, _, b) in _edge_runs('NORMAL') if f == (24, 36)))
    frames = [_render_frames(dev, 700 + 10 * v + 24, 24, 36, 0)[0] for v in range(2)]
    calls = [
        (lambda: ops.exposure_update([x[:1] for x in c['f32']], c['fp'][:1], c['hc'], c['wc'], st, None, 'NORMAL'),
         [('render_lattice_kernel', '(ExposureArgs)', '<2, false>')]),
        (lambda: ops.ingest_nv12(nv, 1, 1),
         [('ingest_hr1_kernel', '(unsigned char const*, unsigned char const*, int, long long, float*, int, int)', ''),
          ('ingest_lr_kernel', '(unsigned char const*, unsigned char const*, int, long long, float*, int, int, int, int, double, double)', '<1>')]),
        (lambda: ops.bgr_to_nv12(bgr),
         [('canvas_u8x1_kernel', '(unsigned char const*, unsigned char*, unsigned char*, int, long long, int, int)', '')]),
        (lambda: ops.render_average_nv12(frames, src[0], T[0], 2, 2, 'NORMAL'),
         [('render_average_kernel', '(Nv12Views, ', '<2, false>')]),
    ]
    for fn, wanted in calls:
        fn()                                         # (once outside the profiler: module load, workspace)
        _, names = _kernel_names(fn)
        with_lists = any('(' in k for k in names)
        squeeze = lambda k: k.replace(' ', '')
        for base, params, targs in wanted:
            if with_lists:
                hit = [k for k in names if base in k and squeeze(params) in squeeze(k)]
            else:
                hit = [k for k in names if base in k and squeeze(targs) in squeeze(k)]
            print('\n[launch witness] %s%s: matched by %s: %s' % (base, params, 'parameter list' if with_lists else 'base name and template arguments', hit or names))
            assert hit, (base, params, names)
