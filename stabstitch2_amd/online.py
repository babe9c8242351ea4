"""True streaming mode: frames are pushed one pair at a time, the 7-frame SmoothNet window
slides over a ring buffer, TemporalNet features of the previous frame are cached, and every push renders at most one new
frame onto a FIXED canvas.

The reference is only "online" up to the smoothing window: its renderer waits for the whole clip because the canvas is
the bounding box over all frames (test_online_tra.py:106-120).  Here the canvas is fixed when the first window is
complete (bbox of its 7 frames grown by `margin`), or given by the caller; with the offline bbox passed in, the stream
reproduces the offline frames (tests/test_gpu_parity.py::test_online_matches_offline).  Per pushed pair the arithmetic is
exactly the reference's per-frame arithmetic (test_online_tra.py:284-392 with k = t).

Canvas overflow (round 5): the reference would have sized the canvas from ALL frames; here every push also runs a one-wave watcher
(`ss_canvas_watch`) that records, on the device, whether the frame's mesh left the fixed canvas (`clipped_frames`,
`overflow_report()`: read lazily, no sync on the push path).  `grow='never'` (default) keeps the canvas and counts;
`grow='recapture'` re-fixes the canvas (union of the old one and everything seen, plus the margin) and re-captures the graph as soon
as a frame comes within half the margin of an edge -- checked through an asynchronous copy of the watcher state one push later, so
a gradual drift grows the canvas BEFORE anything is cropped (an abrupt jump still crops the frames in between; they are counted).

Fixed-size output: `viewport=(Hout, Wout)` makes every frame of a stream Hout x Wout from construction on -- the canvas box (the box
the stitcher would have had, letterboxed to the viewport's aspect) is decoupled from the pixel count, and the render samples the
continuous warp at the viewport's lattice.  `grow='refit'` (viewport only) then re-fixes the BOX on the device, inside the launch
that carries the watcher (`ss_canvas_watch_fit`, `ss_render_footprints_watch_fit`), as soon as the running extents come within the
guard of an edge: the picture zooms out, and nothing on the host changes -- no new shape, no new buffer, no capture, no sync.

Once the window is full every push runs the same ~150 small kernels on buffers of fixed size, so the steady state is
captured ONCE into a HIP graph (state lives in static tensors: the rings are shifted, not rotated) and each push is
two input copies + one graph launch: the Python / ctypes launch overhead (~1 ms per pair, more than the kernels'
own time at batch 1) disappears.  `use_graph=False` runs the same code eagerly.

That step -- from the LR frames to the newest smoothed meshes -- is written once (_PairStep) for S two-view streams: OnlineStitcher
runs it with S = 1, MultiOnlineStitcher with its S, ThreeViewOnlineStitcher through a chain of two pairs; a class adds only what
follows the meshes (its render), and the forms with two pushes in flight (_TwoInFlight) cut the same step in two.  The k-frame step
behind push_many is written once beside it (_PairStep._batch_meshes: one pair, or the two pairs of a chain of three views).
"""
import collections
import contextlib
import os
import time

import torch

from . import layers as L
from . import ops, pipeline
from .spatial_network import build_SpatialNet, get_rigid_mesh, get_norm_mesh

WINDOW = pipeline.WINDOW
_warmup = {}


def _new_graph():
    """A CUDAGraph that keeps its hipGraph_t (torch >= 2.5: keep_graph=True) so that `_graph_nodes` can count its nodes."""
    try:
        return torch.cuda.CUDAGraph(keep_graph=True)
    except TypeError:
        return torch.cuda.CUDAGraph()


def _graph_nodes(g):
    """Nodes of a captured graph (hipGraphGetNodes on the raw handle), None where the runtime / torch does not expose it.  The
    streaming push is bound by its node count (a node costs >= 4.5 us whatever it does): bench.py prints it."""
    try:
        import ctypes
        raw = g.raw_cuda_graph()
        n = ctypes.c_size_t(0)
        hip = ctypes.CDLL('libamdhip64.so')
        if hip.hipGraphGetNodes(ctypes.c_void_p(raw), None, ctypes.byref(n)) != 0:
            return None
        return int(n.value)
    except Exception:
        return None


def _warmup_stream(dev):
    """One capture warm-up stream per device, shared by every stitcher."""
    s = _warmup.get(dev)
    if s is None:
        s = torch.cuda.Stream(dev)
        _warmup[dev] = s
    return s


_LR_SHAPES = ((1, 3, pipeline.LR_H, pipeline.LR_W), (3, pipeline.LR_H, pipeline.LR_W))


def _check_shapes(what, frames, allowed):
    """Frame-size check of a push: shapes only (host side, no device sync), run before the push changes any state.  A stitcher's
    splines, footprints and static buffers are built for ITS height and width, and the render wrappers take H and W from the frame
    they are given: a frame of another size (or a transposed one of the same element count) would render rescaled, wrong geometry."""
    for f in frames:
        shp = None if f is None else tuple(f.shape)
        if shp not in allowed:
            raise ValueError('%s must be %s, got %s' % (what, ' or '.join(str(list(a)) for a in allowed),
                                                        None if shp is None else list(shp)))


def _spatial_temporal_heads(spatial, temporal, f64, prev_feat, feat, b, tm_out, chain=False):
    """SpatialNet behind its stage-1 trunk (f64 [2b,45,60,128], view 1 first) and TemporalNet's regressor on the cached /
    current features (prev_feat, feat [2b,45,60,128], view-major) -> (offset_1, offset_2_ref, offset_2_tgt); the temporal
    motions of view 1 / view 2 are written to tm_out = (t1 [b,126], t2 [b,126]).  With layers.QUAD the four regressor heads
    share their launches (layers.run_regressor_quad), else they run as SpatialNet's pair and TemporalNet's own.
    chain: f64 holds b + 1 images of a CHAIN of views (v1 .. v_{b+1}); pair i = (v_i, v_{i+1}) -- the first views are images
    0 .. b-1, the second views images 1 .. b, overlapping slices of one trunk pass (three views: the middle one passes the
    trunks once, threeview:154-343 runs it through both pair passes)."""
    o2 = 1 if chain else b
    if not L.QUAD:
        assert not chain
        off = spatial.forward_features(f64, b, pipeline.LR_H, pipeline.LR_W)
        temporal.motions_from_features(prev_feat, feat, out_slices=[(0, b, tm_out[0]), (b, 2 * b, tm_out[1])])
        return off
    off1 = _heads_a(spatial, f64, b, chain)
    return (off1,) + _heads_b(spatial, temporal, f64, off1, prev_feat, feat, b, tm_out, chain)


def _heads_a(spatial, f64, b, chain=False):
    """First half of the heads (up to the global homography offsets): SpatialNet's stage-2 trunk + contextual correlation +
    regressNet1 -> offset_1 [b,8].  (PipelinedOnlineStitcher cuts the push between the halves.)
    chain: True -- pair i = images (i, i + 1) of f64 (a chain of views); an int o -- pair i = images (i, i + o) (a chain of views
    holding o frames each, view-major: ThreeViewOnlineStitcher.push_many); False -- pair i = images (i, i + b)."""
    o2 = (1 if chain is True else int(chain)) if chain else b
    f32 = L.run_stage2(f64, spatial._prepared()['s2'])
    return spatial.offset1_from_features(f32[:b], f32[o2:o2 + b])


def _heads_b(spatial, temporal, f64, off1, prev_feat, feat, b, tm_out, chain=False):
    """Second half: decomposition, warps, both nets' cost volumes, the four regressor heads in shared launches
    -> (offset_2_ref, offset_2_tgt); temporal motions into tm_out."""
    o2 = 1 if chain else b
    cv_s = spatial.cv_from_offset1(f64[:b], f64[o2:o2 + b], off1, pipeline.LR_H, pipeline.LR_W)
    cv_t = ops.cost_volume(prev_feat, feat, 3, chain=b if chain else 0)      # [2b] volumes, view-major (chain: from b + 1 views stored once)
    off_ref = torch.empty((b, 126), device=f64.device, dtype=torch.float32)
    off_tgt = torch.empty((b, 126), device=f64.device, dtype=torch.float32)
    L.run_regressor_quad(cv_s, cv_t.view((2, b) + tuple(cv_t.shape[1:])), L.get_quad(spatial, temporal),
                         [off_ref, off_tgt, tm_out[0], tm_out[1]])
    return off_ref, off_tgt


def _check_u8(what, frames, shape):
    """push_u8's frames: uint8 tensors alike, each of `shape` ([H,W,3], or [S,H,W,3] for S streams); run before any state changes."""
    if any(f.dtype != torch.uint8 or f.dim() != len(shape) or f.shape[-1] != 3 or tuple(f.shape) != tuple(frames[0].shape)
           for f in frames):
        raise ValueError('push_u8 takes %s' % what)
    _check_shapes('uint8 frames', frames, (shape,))


def _check_nv12_stitcher(st, out, what):
    """What every NV12 entry refuses before it looks at a frame: the output format, a stitcher that renders nothing, odd frame sizes."""
    if out not in ('bgr', 'nv12'):
        raise ValueError("%s: out must be 'bgr' or 'nv12', got %r" % (what, out))
    if st.meshes_only:                   # (chain=True stitchers are meshes_only)
        raise ValueError('%s renders frames: not for meshes_only stitchers' % what)
    if st.h % 2 or st.w % 2:
        raise ValueError('NV12 frames have an even height and width: not for a %d x %d stitcher' % (st.h, st.w))


def _check_nv12(st, frames, out):
    """push_nv12's arguments: decoded NV12 frames uint8 [H*3/2, W] of the stitcher's H x W (dense columns, any row stride >= W) and
    the output format; run before any state changes."""
    _check_nv12_stitcher(st, out, 'push_nv12')
    shape = (st.h // 2 * 3, st.w)
    if any(f.dtype != torch.uint8 or tuple(f.shape) != shape or f.stride(-1) != 1 or f.stride(0) < st.w for f in frames):
        raise ValueError('push_nv12 takes %d uint8 NV12 frames [%d,%d] = [H*3/2, W] with dense columns (a row stride > W is fine), got %s'
                         % (len(frames), shape[0], shape[1], [(str(f.dtype), tuple(f.shape), tuple(f.stride())) for f in frames]))
    if out == 'nv12':
        _even_viewport(st, "push_nv12(out='nv12')")


def _even_viewport(st, what):
    if st.viewport is None or st.viewport[0] % 2 or st.viewport[1] % 2:
        raise ValueError("%s needs a stitcher built with an even viewport=(Hout, Wout): an NV12 frame has an even, fixed size "
                         '(this stitcher: viewport=%r)' % (what, st.viewport))


def _check_many_nv12(st, views, out, what, count=None):
    """The arguments of push_many_nv12 (count=None: 1..BATCH_MAX surfaces per view) and of MultiOnlineStitcher.push_nv12 (count = S):
    every view a tensor [k,H*3/2,W] or a list of k NV12 surfaces of the stitcher's H x W, and the output format; shapes only, run
    before any state changes -> the views' surface lists."""
    _check_nv12_stitcher(st, out, what)
    surfs = []
    for v in views:
        if torch.is_tensor(v) and v.dim() != 3:
            raise ValueError('%s takes every view as an NV12 tensor [k,%d,%d] or a list of k NV12 surfaces, got a tensor %s'
                             % (what, st.h // 2 * 3, st.w, tuple(v.shape)))
        s, h, w, _ = ops.nv12_surfaces(v)
        if (h, w) != (st.h, st.w):
            raise ValueError('%s takes NV12 surfaces [%d,%d] = [H*3/2, W] of this stitcher, got [%d,%d]'
                             % (what, st.h // 2 * 3, st.w, h // 2 * 3, w))
        surfs.append(s)
    k = len(surfs[0])
    if any(len(s) != k for s in surfs):
        raise ValueError('%s: the NV12 views differ in length: %s' % (what, [len(s) for s in surfs]))
    if count is not None and k != count:
        raise ValueError('%s takes %d NV12 surfaces per view (one per stream), got %d' % (what, count, k))
    if count is None and not 1 <= k <= BATCH_MAX:
        raise ValueError('%s takes 1 to %d frames of every view per call, got %d' % (what, BATCH_MAX, k))
    if out == 'nv12':
        _even_viewport(st, "%s(out='nv12')" % what)
    return surfs


def _stacked(frames):
    """uint8 frames of one size as ONE tensor [n,...]: the frames themselves where they already lie back to back in one allocation (the
    frames of a batched render), else a copy."""
    f0, step = frames[0], frames[0].numel()
    base = f0.untyped_storage().data_ptr()
    if all(f.shape == f0.shape and f.is_contiguous() and f.untyped_storage().data_ptr() == base
           and f.data_ptr() == f0.data_ptr() + i * step for i, f in enumerate(frames)):
        return f0.as_strided((len(frames),) + tuple(f0.shape), (step,) + tuple(f0.stride()))
    return torch.stack(list(frames))


def _to_u8(x):
    """A push's frames (a list, or a list per stream) as uint8 video frames [Hc,Wc,3]: ops.canvas_to_u8 of each fp32 canvas; frames
    the render wrote as uint8 stay as they are."""
    if torch.is_tensor(x):
        return x if x.dtype == torch.uint8 else ops.canvas_to_u8(x.reshape((1,) + tuple(x.shape[-3:])))[0]
    return [_to_u8(y) for y in x]


def _frames_to_nv12(frames):
    """uint8 video frames of one size -> their NV12 frames, views of one tensor [n,Hc*3/2,Wc]: one ops.bgr_to_nv12 launch."""
    return list(ops.bgr_to_nv12(_stacked(frames)).unbind(0)) if frames else []


def _exposure_params(exposure, meshes_only=False):
    """OnlineStitcher's exposure= -> None | ops.ExposureParams (True: the defaults)."""
    if exposure is None or exposure is False:
        return None
    if meshes_only:
        raise ValueError('exposure compensation scales rendered frames: not for meshes_only stitchers')
    if exposure is True:
        return ops.ExposureParams()
    if not isinstance(exposure, ops.ExposureParams):
        raise ValueError('exposure must be None, True or an ops.ExposureParams, got %r' % (exposure,))
    return exposure


def _no_exposure(cls, exposure):
    if exposure is not None and exposure is not False:
        raise ValueError('%s has no exposure compensation yet: it is built for OnlineStitcher only' % cls)


def _no_coverage(cls, track_coverage):
    if track_coverage:
        raise ValueError('%s has no track_coverage: it is built for OnlineStitcher and ThreeViewOnlineStitcher' % cls)


def _canvas_size(bb):
    """(Hc, Wc) of a canvas (wmin, wmax, hmin, hmax), CPU fp32 [4]."""
    return int((bb[3] - bb[2]).int()), int((bb[1] - bb[0]).int())


@contextlib.contextmanager
def _kept(state):
    """The body may advance the state tensors: their values are put back at its end (and whenever it calls the `restore` it is given)."""
    keep = [t.clone() for t in state]

    def restore():
        for t, v in zip(state, keep):
            t.copy_(v)
    yield restore
    restore()


def _capture(dev, state, warmup, steps, per_push=1):
    """Capture each of `steps` into a HIP graph.  The eager warm-up runs first, on the shared warm-up stream and on a copy of the state,
    so that the push being captured is applied exactly once (by the replay that follows); captures do not execute, and the state is
    the pre-push state afterwards.  -> (graphs, nodes of one push: the first `per_push` graphs; None where not exposed)."""
    cur = torch.cuda.current_stream(dev)
    with _kept(state) as restore:
        side = _warmup_stream(dev)
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            warmup()
        cur.wait_stream(side)
        restore()
        graphs = []
        for fn in steps:
            g = _new_graph()
            with torch.cuda.graph(g):
                fn()
            graphs.append(g)
    nodes = 0
    for g in graphs[:per_push]:
        n = _graph_nodes(g)
        nodes = None if nodes is None or n is None else nodes + n
    return graphs, nodes


class _CanvasWatch:
    """Overflow state of N fixed canvases (N = S for MultiOnlineStitcher, else 1).  The device rows that ops.canvas_watch updates on
    every push (wi [N,4] int32: frames seen / clipped / first clipped / near an edge; wf [N,4] fp32: running normalised extents), the
    totals of the canvases each row had before, and for grow='recapture' a pinned copy of the rows one push behind and the arithmetic
    that re-fixes a canvas around everything seen on it."""

    def __init__(self, n, margin, dev, viewport=None, refit=False, zoom_limit=2.0):
        self.n, self.margin, self.dev = n, margin, dev
        self.viewport, self.refit, self.zoom_limit = viewport, bool(refit), float(zoom_limit)
        self.fit = None                                # grow='refit': ops.CanvasFit -- box [N,4] / epoch [N] / ext0 [N,2] on the device
        self.wi = self.wf = None                       # device rows of the current canvases (None: no canvas yet)
        self.boxes = None                              # the current canvases (wmin, wmax, hmin, hmax in HR px), CPU fp32 [N,4]
        self.totals = [[0, 0, -1] for _ in range(n)]  # frames seen / clipped / first clipped frame on EARLIER canvases
        self.epoch = [0] * n                           # growths per canvas
        self.near_handled = [0] * n
        self._host = self._event = None                # grow='recapture': pinned copy of the rows, one push behind

    @property
    def guard(self):
        """`near` threshold of the watcher in canvas-normalised units: half the margin the canvas was grown by."""
        return max(0.0, float(self.margin)) * 0.5 / (1.0 + 2.0 * max(0.0, float(self.margin))) * 2.0

    def args(self, s=None):
        """(guard, watch_i, watch_f) of all rows, or of row s, for the launches that carry the watcher."""
        if s is None:
            return self.guard, self.wi, self.wf
        return self.guard, self.wi[s:s + 1], self.wf[s:s + 1]

    def fit_boxes(self, dev_boxes, fit_state=None):
        """A viewport: the canvases dev_boxes (device fp32 [N,4], the tensor the push's launches read) are letterboxed in place to its
        aspect (ops.box_fit_aspect), or -- fit_state = (epoch [N], ext0 [N,2]) -- taken as they are with that state carried over; with
        grow='refit' they become the device-side state of the refit.  -> the boxes, CPU fp32 [N,4] (synchronises)."""
        hout, wout = self.viewport
        if fit_state is None:
            _, epoch, ext0 = ops.canvas_fit_state(self.n, self.dev)
            ops.box_fit_aspect(dev_boxes, hout, wout, ext0)
        else:
            epoch, ext0 = fit_state
        if self.refit:
            self.fit = ops.CanvasFit(dev_boxes.view(self.n, 4), epoch, ext0, max(0.0, float(self.margin)), self.zoom_limit, hout, wout)
        return dev_boxes.cpu().reshape(self.n, 4)

    def fit_args(self, s=None):
        """The ops.CanvasFit of all rows, or of row s, for the launches that carry the watcher (None unless grow='refit')."""
        f = self.fit
        if f is None or s is None:
            return f
        return f._replace(box=f.box[s:s + 1], epoch=f.epoch[s:s + 1], ext0=f.ext0[s:s + 1])

    def fit_state(self):
        """The refit's step-mutated tensors (box, epoch): state of the captured step beside the watcher rows."""
        return [] if self.fit is None else [self.fit.box, self.fit.epoch]

    def current(self):
        """-> (boxes CPU fp32 [N,4], growths per canvas); grow='refit': read from the device (synchronises)."""
        if self.fit is None:
            return self.boxes, list(self.epoch)
        return self.fit.box.cpu(), self.fit.epoch.cpu().tolist()

    def start(self, boxes, state=None):
        """Watch these canvases (CPU fp32 [N,4]) from now on: fresh rows, or state = (wi, wf) carried over."""
        self.boxes = boxes
        self.wi, self.wf = state if state is not None else ops.canvas_watch_state(self.n, self.dev)
        self.near_handled = [0] * self.n
        self._event = None

    def report(self):
        """Synchronises.  -> one dict per canvas: {'frames_seen', 'clipped_frames', 'first_clipped_frame' (stream frame index, -1 =
        none), 'near_frames' (current canvas), 'canvas_epoch', 'needed_bbox' (wmin, wmax, hmin, hmax in HR px: the current canvas
        united with every mesh seen on it), 'box' (the current canvas, HR px; None before it is fixed)}."""
        wi = None if self.wi is None else self.wi.cpu().tolist()
        wf = None if self.wf is None else self.wf.cpu()
        boxes, epochs = self.current()
        reps = []
        for s in range(self.n):
            seen, clipped, first = self.totals[s]
            rep = {'frames_seen': seen, 'clipped_frames': clipped, 'first_clipped_frame': first, 'near_frames': 0,
                   'canvas_epoch': epochs[s], 'needed_bbox': None,
                   'box': None if boxes is None else tuple(float(x) for x in boxes[s])}
            if wi is not None:
                w = wi[s]
                if w[1] > 0 and first < 0:
                    rep['first_clipped_frame'] = seen + w[2]
                rep['frames_seen'] = seen + w[0]
                rep['clipped_frames'] = clipped + w[1]
                rep['near_frames'] = w[3]
                rep['needed_bbox'] = tuple(float(x) for x in self._needed_bbox(s, wf[s], boxes[s]))
            reps.append(rep)
        return reps

    def _needed_bbox(self, s, wf, bb=None):
        """Running normalised extents [xmin, xmax, ymin, ymax] on canvas s (bb: its box, read elsewhere) -> union with the canvas, HR
        pixels."""
        bb = self.boxes[s] if bb is None else bb
        ow, oh = float(bb[1] - bb[0]), float(bb[3] - bb[2])
        x0 = float(bb[0]) + (min(float(wf[0]), -1.0) + 1.0) * ow / 2.0
        x1 = float(bb[0]) + (max(float(wf[1]), 1.0) + 1.0) * ow / 2.0
        y0 = float(bb[2]) + (min(float(wf[2]), -1.0) + 1.0) * oh / 2.0
        y1 = float(bb[2]) + (max(float(wf[3]), 1.0) + 1.0) * oh / 2.0
        return x0, x1, y0, y1

    def _regrow(self, s, wi, wf):
        """Re-fix canvas s around everything seen on it (+ margin), fresh row.  -> False when there is nothing to grow by."""
        x0, x1, y0, y1 = self._needed_bbox(s, wf)
        gw, gh = self.margin * (x1 - x0), self.margin * (y1 - y0)
        old = [float(v) for v in self.boxes[s]]
        if max(abs(a - b) for a, b in zip(old, (x0 - gw, x1 + gw, y0 - gh, y1 + gh))) < 0.5:
            # nothing to grow by (e.g. margin 0 and a mesh that only touches the edge): keep the canvas, the output buffer and the
            # captured graph -- a recapture costs a sync, an allocation and a capture, and would be asked for again next push
            self.near_handled[s] = int(wi[3])
            return False
        seen, clipped, first = self.totals[s]
        if wi[1] > 0 and first < 0:
            first = seen + wi[2]
        self.totals[s] = [seen + wi[0], clipped + wi[1], first]
        self.boxes[s] = torch.tensor([x0 - gw, x1 + gw, y0 - gh, y1 + gh], dtype=torch.float32)
        fi, ff = ops.canvas_watch_state(1, self.dev)
        self.wi[s].copy_(fi[0])
        self.wf[s].copy_(ff[0])
        self.near_handled[s] = 0
        self.epoch[s] += 1
        return True

    def poll(self):
        """Start of a steady-state push (grow='recapture'): look at the rows of the push before, copied to pinned memory behind it --
        no wait: if the copy has not landed yet the check happens one push later.  -> the canvases that were re-fixed."""
        if self._event is None or not self._event.query():
            return []
        near = self._host[0][:, 3].tolist()
        cand = [s for s in range(self.n) if near[s] > self.near_handled[s]]
        if not cand:
            return []
        # (rare path, synchronises: the device rows may be a push ahead of the pinned copy -- take everything seen so far)
        wi, wf = self.wi.cpu(), self.wf.cpu()
        grown = [s for s in cand if self._regrow(s, wi[s].tolist(), wf[s])]
        self._event = None
        return grown

    def post_copy(self):
        """End of a steady-state push (grow='recapture'): copy the rows to pinned memory behind it."""
        if self._host is None:
            self._host = (torch.empty((self.n, 4), dtype=torch.int32).pin_memory(),
                          torch.empty((self.n, 4), dtype=torch.float32).pin_memory())
        self._host[0].copy_(self.wi, non_blocking=True)
        self._host[1].copy_(self.wf, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.dev))
        self._event = ev


# ------------------------------------------------------------------ how a fusion mode renders
class _Deferred(collections.namedtuple('_Deferred', 'src T fp efp')):
    """What a step that does not render itself leaves for the push's render: the control points and splines (src, T) of one frame
    ([V,63,2], [V,2,66]) or of n ([n,V,63,2], [n,V,2,66]), the footprint row(s) fp the render skips tiles by (None: it skips none) and
    the footprint rows efp [n, .] the exposure update samples (None: no exposure compensation)."""
    __slots__ = ()


class _Render:
    """How ONE fusion mode renders in the streaming stitchers: built once by _Stitcher.__init__ (`mode`) from the mode, the switches
    and the class, and the only code that knows it.  `direct`: does the steady-state push of this stitcher launch the render itself,
    outside the graph, on the caller's frames?  `skip`: does the render skip tiles by footprint?  `nv12`: does it sample NV12 frames
    (and hand NV12 out)?  `ragged`: is its direct render of S streams ONE render over canvases of any sizes, into fresh tensors?
    A kind provides, with left = the step's _Deferred and hc, wc = the canvas size (it changes under grow='recapture'):
      render_into(imgs, left, hc, wc, gains, out)      one frame inside the step (window fill, use_graph=False, no direct render)
      frame(imgs, left, hc, wc, u8, gains)             the push's own render of one frame: fp32 planes, or uint8 in -> uint8 out
      frame_nv12(imgs, left, hc, wc, out)              the same from NV12 frames -> the uint8 frame or NV12 (`out`)
      batch(views, left, hc, wc, u8, gains, out)       n frames on canvases of one size -> [n, ...]
      streams(imgs, left, sizes, u8)                   S frames on S canvases: left one record (see `ragged`; or the canvases share
                                                       a size) or one per stream -> S frames
    It holds no reference to its stitcher (a cycle would keep the stitcher's buffers until the collector runs)."""
    skip = False
    nv12 = True
    ragged = False

    def __init__(self, st):
        self.fusion, self.warp, self.h, self.w, self.dev = st.fusion_mode, st.warp_mode, st.h, st.w, st.dev
        self.exposure = st.exposure is not None
        self.direct = bool(self._takes_direct(st) and st.use_graph and not st.meshes_only)

    def canvas_changed(self):
        """The stitcher's canvas was set or regrown: whatever the kind remembers about the old one goes."""

    def needs_footprints(self):
        """Does the captured step end with a footprint launch?  (exposure: the footprint lattice is the estimator's sample set, made
        whatever the fusion is)"""
        return self.skip or self.exposure

    def carry(self, src, watch, fit):
        """The overflow watcher watch = (guard, watch_i, watch_f) has not seen src [n,V,63,2] yet (fit, grow='refit': the ops.CanvasFit
        the launch that carries it re-fixes the boxes with): -> (watch, fit) for the footprint launch where the step has one; else it
        runs here, as a launch of its own -> (None, None)."""
        if watch is None or self.needs_footprints():
            return watch, fit
        ops.canvas_watch(src, watch[1], watch[2], watch[0], fit=fit)
        return None, None

    def footprints(self, src, T, hc, wc, watch=None, fit=None):
        """End of a step, n frames on canvases of one size: the watcher (`carry`) and the footprint launch where the step needs one
        -> (fp, efp) of the _Deferred, n rows each."""
        watch, fit = self.carry(src, watch, fit)
        if not self.needs_footprints():
            return None, None
        rows = ops.render_footprints(src, T, self.h, self.w, hc, wc, watch=watch, fit=None if watch is None else fit)
        return rows if self.skip else None, rows if self.exposure else None


class _FusedRender(_Render):
    """AVERAGE | FEATHER: the fused single-launch render (ops.render_average*, the formula its `fusion`)."""
    skip = property(lambda self: pipeline.SKIP_OUTSIDE)      # same footprint skipping as the offline render (pipeline.render_frames)
    # (the NV12 render has no SS_RENDER_EPS_FOLD form: with that opt-in set the fp32 route keeps the two formats equal)
    nv12 = property(lambda self: not ops.RENDER_EPS_FOLD)

    def _takes_direct(self, st):
        return DIRECT_RENDER

    def render_into(self, imgs, left, hc, wc, gains, out):
        return ops.render_average(imgs, left.src, left.T, hc, wc, self.warp, out=out, footprint=left.fp, gains=gains, fusion=self.fusion)

    def frame(self, imgs, left, hc, wc, u8, gains=None):
        if u8:                           # uint8 frames in, the uint8 video frame out: no fp32 frame planes, no fp32 canvas
            return ops.render_average_u8(list(imgs), left.src, left.T, hc, wc, self.warp, footprint=left.fp, gains=gains,
                                         fusion=self.fusion)
        return self.render_into([f.reshape(1, 3, self.h, self.w) for f in imgs], left, hc, wc, gains, None)

    def frame_nv12(self, imgs, left, hc, wc, out):
        """The render writes the requested format itself (NV12_FUSED_SINK off: the uint8 frame, and the sink makes NV12 of it)."""
        if out == 'nv12' and not NV12_FUSED_SINK:
            return ops.bgr_to_nv12(ops.render_average_nv12(list(imgs), left.src, left.T, hc, wc, self.warp, footprint=left.fp,
                                                           fusion=self.fusion))
        return ops.render_average_nv12(list(imgs), left.src, left.T, hc, wc, self.warp, footprint=left.fp, out_format=out,
                                       fusion=self.fusion)

    def batch(self, views, left, hc, wc, u8=False, gains=None, out=None):
        render = ops.render_average_clip_u8 if u8 else ops.render_average_clip
        return render(views, left.src, left.T, hc, wc, self.warp, out=out, footprint=left.fp, gains=gains, fusion=self.fusion)

    def streams(self, imgs, left, sizes, u8):
        """One clip-style launch when the canvases share a size, else one launch per stream."""
        if isinstance(left, _Deferred):
            return list(self.batch([f.contiguous() for f in imgs], left, sizes[0][0], sizes[0][1], u8))
        # (uint8 frames [H,W,3], fp32 ones [1,3,H,W])
        return [self.frame([f[s] if u8 else f[s:s + 1] for f in imgs], left[s], hc, wc, u8) for s, (hc, wc) in enumerate(sizes)]


class _LinearRender(_Render):
    """LINEAR.  Inside the step the per-frame chain (warp, blender launches); the push's own render is the fused three launches (four
    with three views) of ops.render_linear_frames -- for all S streams of a MultiOnlineStitcher at once, whatever their canvas sizes;
    bit-identical frames."""
    ragged = True

    def __init__(self, st):
        _Render.__init__(self, st)
        self._ws = {}                    # chunk -> ((canvas sizes, views), workspace), re-made when a canvas changes

    def _takes_direct(self, st):
        return DIRECT_RENDER and DIRECT_LINEAR and st._LINEAR_DIRECT

    def _frames(self, views, src, T, sizes, nv12=False, gains=None, outs=None):
        """n frames on their own canvases `sizes` (ops.render_linear_frames, <= 32 frames per call) with the workspaces this stitcher
        holds; they are re-made when a canvas is set or regrown (the sizes are their key).  nv12: the views are NV12 frames
        [n,H*3/2,W] (any pitch), sampled where they lie."""
        res = []
        for c in range(0, len(sizes), 32):
            key = (tuple(sizes[c:c + 32]), len(views))
            if self._ws.get(c, (None, None))[0] != key:
                self._ws[c] = (key, ops.linear_frames_workspace(key[0], key[1], self.dev))
            if nv12:
                res += ops.render_linear_frames_nv12([f[c:c + 32] for f in views], src[c:c + 32], T[c:c + 32], key[0],
                                                     self.warp, ws=self._ws[c][1])
                continue
            res += ops.render_linear_frames([f[c:c + 32].contiguous() for f in views], src[c:c + 32], T[c:c + 32], key[0],
                                            self.warp, ws=self._ws[c][1], outs=None if outs is None else outs[c:c + 32],
                                            gains=None if gains is None else gains[c:c + 32])
        return res

    def render_into(self, imgs, left, hc, wc, gains, out):
        src, T = left.src, left.T
        if gains is not None:                # with exposure: the fused render at n = 1 (bit-identical to the chain below)
            return self._frames([f.reshape(1, 3, self.h, self.w) for f in imgs], src[None], T[None], [(hc, wc)], gains=gains,
                                outs=None if out is None else [out])[0]
        w = ops.tps_warp_views(imgs, src, T, hc, wc, self.warp)                   # [V,4,Hc,Wc]
        res = ops.linear_blend(w[0, 0:3], w[1, 0:3], w[0, 3], w[1, 3])
        if len(imgs) == 3:
            res = ops.linear_blend(res, w[2, 0:3], ops.mask_union(w[0, 3], w[1, 3]), w[2, 3])
        return res if out is None else out.copy_(res)

    def frame(self, imgs, left, hc, wc, u8, gains=None):
        """The fused three / four launches at n = 1; uint8 frames in -> the uint8 video frame out."""
        shp = (1, self.h, self.w, 3) if u8 else (1, 3, self.h, self.w)
        return self._frames([f.reshape(shp) for f in imgs], left.src[None], left.T[None], [(hc, wc)], gains=gains)[0]

    def frame_nv12(self, imgs, left, hc, wc, out):
        """The render writes the uint8 frame (its blend walks a rolling row window) and the sink makes NV12 of it."""
        bgr = self._frames([f[None] for f in imgs], left.src[None], left.T[None], [(hc, wc)], nv12=True)[0]
        return ops.bgr_to_nv12(bgr) if out == 'nv12' else bgr

    def batch(self, views, left, hc, wc, u8=False, gains=None, out=None):
        """The fused clip render (bit-identical per frame to the chain of render_into)."""
        return ops.render_linear_clip(views, left.src, left.T, hc, wc, self.warp, out=out, gains=gains)

    def streams(self, imgs, left, sizes, u8):
        """ONE ragged render over the S streams' own canvases (chunks of 32 streams)."""
        return self._frames(list(imgs), left.src, left.T, sizes)


class _MultibandRender(_Render):
    """MULTIBAND (ops.render_multiband: the existing warp + the pyramid blend): in the steady state always launched by the push or the
    batch, on the caller's frames, behind a graph that ends with the splines and the watcher -- as the direct LINEAR render is.  One
    canvas, one push in flight; no NV12 source or sink (push_nv12: ingest, push, the sinks)."""
    nv12 = False

    def __init__(self, st):
        _Render.__init__(self, st)
        self.bands = st.bands
        self.seam = dict(st.seam)            # {} (the geometric seam: no launch of it exists) or ops.render_multiband's seam='dp' keywords
        self._seam_state = None              # ((hc, wc, views), ops.seam_state): the stream's previous seams on this canvas

    def _takes_direct(self, st):
        return True

    def canvas_changed(self):
        self._seam_state = None

    def _seam(self, views, hc, wc):
        """The seam keywords of one render on the hc x wc canvas: with the DP seam, the stream's state with them -- a fresh one after
        the canvas was set or regrown (`canvas_changed`) or changed its size."""
        if not self.seam:
            return self.seam
        key = (hc, wc, views)
        if self._seam_state is None or self._seam_state[0] != key:
            self._seam_state = (key, ops.seam_state(views, hc, wc, self.seam['seam_cell'], self.dev))
        return dict(self.seam, seam_state=self._seam_state[1])

    def render_into(self, imgs, left, hc, wc, gains, out):      # the window fill, and every push without a graph
        return ops.render_multiband(list(imgs), left.src, left.T, hc, wc, self.warp, self.bands, out=out, u8=False,
                                    **self._seam(len(imgs), hc, wc))

    def frame(self, imgs, left, hc, wc, u8, gains=None):        # uint8 frames in -> the uint8 video frame out of the last collapse pass
        shp = (self.h, self.w, 3) if u8 else (3, self.h, self.w)
        return ops.render_multiband([f.reshape(shp) for f in imgs], left.src, left.T, hc, wc, self.warp, self.bands,
                                    **self._seam(len(imgs), hc, wc))

    def batch(self, views, left, hc, wc, u8=False, gains=None, out=None):
        """pipeline.MULTIBAND_FRAMES frames per call: each in the launches of one (the DP seam takes a call's frames in order)."""
        src, T = left.src, left.T
        k, c = src.shape[0], pipeline.MULTIBAND_FRAMES
        if out is None:
            out = torch.empty((k, hc, wc, 3) if u8 else (k, 3, hc, wc), device=self.dev, dtype=views[0].dtype)
        seam = self._seam(len(views), hc, wc)
        for s in range(0, k, c):
            ops.render_multiband([f[s:s + c] for f in views], src[s:s + c], T[s:s + c], hc, wc, self.warp, self.bands, out=out[s:s + c],
                                 **seam)
        return out


# ------------------------------------------------------------------ steady state (window full, canvas fixed)
# The static tensors a steady-state step advances (_PairStep has their layout); the canvas watcher's rows (ops.canvas_watch) count
# every run of the step and are state too.
_STATE = ('prev_feat', 'pair_s', 'ring')


class _Stitcher:
    """What the three plain stitchers share: their common fields, the canvas watcher, the twin trunk and its weights check, and the
    steady-state push -- poll the watcher (grow='recapture'), recapture after reloaded weights, load the push's inputs, run the step
    eagerly (use_graph=False) or capture it on first use and replay it, copy the watcher rows behind it, hand the frames out (rendered
    now from the caller's frames with the direct render, else copies of the graph's output).  _load and _step_static are _PairStep's
    for the two-view stitchers (ThreeViewOnlineStitcher: its own, around its chains'); a subclass provides the window-fill push and the
    tail behind the meshes; one with S canvases also _regrown / _render_direct / overflow_report.  How the fusion mode renders, in
    every one of these places, is `self.mode`'s to say (_Render)."""
    _U8_STEADY = True        # push_u8 in the steady state: the resize writes the graph's LR inputs, the render samples the uint8 frames
    _LINEAR_DIRECT = True    # may LINEAR fusion take the direct render (DIRECT_LINEAR)?  Not with two pushes in flight (_TwoInFlight)
    _MULTIBAND = False       # does the class render MULTIBAND fusion?  (one canvas, one push in flight: the two plain stitchers)

    def __init__(self, nets, height, width, margin, warp_mode, fusion_mode, use_graph, grow, meshes_only=False, canvases=1,
                 viewport=None, zoom_limit=2.0, exposure=None, bands=None, seam=None, track_coverage=False):
        self.exposure = _exposure_params(exposure, meshes_only)      # None: no launch, buffer or graph node of it exists
        self.bands = None
        # MULTIBAND's seam (seam = the dict of the constructor's seam= keywords): {} = the geometric one
        self.seam = pipeline.seam_options(fusion_mode, **(seam or {}))
        if self.seam and (meshes_only or not self._MULTIBAND):
            raise ValueError("%s has no seam=: OnlineStitcher and ThreeViewOnlineStitcher render fusion_mode='MULTIBAND'"
                             % type(self).__name__)
        if fusion_mode == 'MULTIBAND':
            if self.exposure is not None:
                raise ValueError("exposure= has no fusion_mode='MULTIBAND' form: the warp it uses takes no gains")
            if not meshes_only and not self._MULTIBAND:
                raise ValueError("%s has no fusion_mode='MULTIBAND': OnlineStitcher and ThreeViewOnlineStitcher do" % type(self).__name__)
            self.bands = ops.check_bands(ops.MULTIBAND_BANDS if bands is None else bands)
        elif bands is not None:
            raise ValueError("bands= belongs to fusion_mode='MULTIBAND', got %r" % (fusion_mode,))
        if grow not in ('never', 'recapture', 'refit'):
            raise ValueError("grow must be 'never', 'recapture' or 'refit'")
        if viewport is not None:
            try:
                viewport = (int(viewport[0]), int(viewport[1]))
                ok = len(viewport) == 2 and all(11 <= v <= 65535 for v in viewport)
            except (TypeError, ValueError, IndexError):
                ok = False
            if not ok:
                raise ValueError('viewport must be (Hout, Wout) with each of them in 11..65535, got %r' % (viewport,))
            if meshes_only:
                raise ValueError('viewport sizes rendered frames: not for meshes_only stitchers')
            if grow == 'recapture':
                raise ValueError("grow='recapture' changes the frame size: not with a viewport (grow='refit' keeps it)")
        elif grow == 'refit':
            raise ValueError("grow='refit' needs a viewport: it re-fixes the canvas box under a fixed frame size")
        if not float(zoom_limit) >= 0.0:
            raise ValueError('zoom_limit must be >= 0, got %r' % (zoom_limit,))
        self.grow = grow
        self.viewport, self.zoom_limit = viewport, float(zoom_limit)
        self.hc, self.wc = viewport if viewport is not None else (None, None)
        self._canvas_set = False         # is the canvas box fixed yet?  (with a viewport hc / wc are known before it is)
        self.nets = nets
        self.spatial, self.temporal, self.smooth = nets
        self.dev = next(self.spatial.parameters()).device
        self.h, self.w = height, width
        self.margin = margin
        self.warp_mode, self.fusion_mode = warp_mode, fusion_mode
        # AVERAGE | FEATHER: the fused single-launch render (ops.render_average*, the formula its `fusion`)
        self._fused = ops.fused_render(fusion_mode)
        if fusion_mode == 'FEATHER' and ops.RENDER_EPS_FOLD:
            raise ValueError('SS_RENDER_EPS_FOLD has no FEATHER form')
        self.use_graph = use_graph
        self.meshes_only = bool(meshes_only)
        # how this mode renders -- the direct render, the uint8 steady state, footprint skipping, NV12 written by the render and the
        # batch renders all ask `mode`, not the mode's name
        self.mode = (_FusedRender if self._fused else _MultibandRender if fusion_mode == 'MULTIBAND' else _LinearRender)(self)
        self._deferred = None            # direct render: the _Deferred the step left for the push's render
        # track_coverage: one ops.coverage_state of the current canvas, every frame handed out on it AND-ed in behind its render, outside
        # the graph; off: no launch, buffer or field of it does anything
        self.track_coverage = bool(track_coverage)
        if self.track_coverage:
            if meshes_only:
                raise ValueError('track_coverage follows rendered frames: not for meshes_only stitchers')
            if grow == 'refit':
                raise ValueError("track_coverage has no grow='refit' form: the box moves on the device without the host knowing")
            if use_graph and not self.mode.direct:
                raise ValueError('track_coverage needs the push to launch its render itself: not with a captured step that renders '
                                 'inside its graph (SS_DIRECT_RENDER=0 / SS_DIRECT_LINEAR=0 with use_graph=True)')
        self._cover = None               # the ops.CoverageState, from _set_canvas on
        self.coverage_frames = 0         # frames handed out on the current canvas (track_coverage)
        # overflow of the fixed canvas(es), and the device-side refit of their boxes; meshes_only: never started
        self.watch = _CanvasWatch(canvases, margin, self.dev, viewport, grow == 'refit', zoom_limit)
        self.static = None               # steady-state buffers (inputs, rings, output) once the window is full
        self.graph = None
        self.graph_nodes = None          # nodes of the captured steady-state graph (None: not captured / not exposed)
        self.trunk_pair = None
        self.trunk_versions = None
        self.frames_in = 0
        self._batch = collections.OrderedDict()   # push_many: batch size k -> its work buffers and graph, least recently used first
        self.graph_nodes_batch = {}      # push_many: nodes of the steady-state graph captured for batch size k (None: not exposed)
        self.batch_captures = 0          # push_many: graphs captured so far
        # exposure compensation: the stream's gain state (ops.exposure_state) -- it belongs to the stream, not to a canvas or a
        # graph, and survives a regrow / recapture
        self._exp_state = None if self.exposure is None else ops.exposure_state(self.dev)

    # ------------------------------------------------------------------ canvas overflow
    def overflow_report(self):
        """Synchronises.  -> {'frames_seen', 'clipped_frames', 'first_clipped_frame' (stream frame index, -1 = none), 'near_frames'
        (current canvas), 'canvas_epoch', 'needed_bbox' (wmin, wmax, hmin, hmax in HR px: the current canvas united with every
        mesh seen on it), 'box' (the current canvas, HR px; None before it is fixed)}."""
        return self.watch.report()[0]

    @property
    def clipped_frames(self):
        """Frames emitted so far whose mesh reached outside the canvas they were rendered on (per stream for S streams; synchronises)."""
        rep = self.overflow_report()
        return [r['clipped_frames'] for r in rep] if isinstance(rep, list) else rep['clipped_frames']

    def _sync_state(self):
        """Before the device state is read: nothing here -- the reading copy waits for the caller's stream, which runs every push."""

    @property
    def canvas_epoch(self):
        """Growths of the canvas (grow='recapture' / 'refit'; per stream for MultiOnlineStitcher).  grow='refit': the count lives on
        the device -- synchronises."""
        if self.watch.fit is not None:
            self._sync_state()
        epochs = self.watch.current()[1]
        return epochs if isinstance(self, MultiOnlineStitcher) else epochs[0]

    @property
    def canvas_box(self):
        """The canvas box (wmin, wmax, hmin, hmax) in HR pixels the next frame is rendered on (per stream for MultiOnlineStitcher;
        None before the first window is complete).  grow='refit': the box lives on the device -- synchronises."""
        if self.watch.fit is not None:
            self._sync_state()
        boxes = self.watch.current()[0]
        if boxes is None:
            return [None] * self.watch.n if isinstance(self, MultiOnlineStitcher) else None
        boxes = [tuple(float(x) for x in b) for b in boxes]
        return boxes if isinstance(self, MultiOnlineStitcher) else boxes[0]

    def _set_canvas(self):
        """The canvas is fixed at self.bbox: its size, a fresh watcher on it.  With a viewport the size is the viewport's, and the
        box is letterboxed to its aspect (on the device, in place: it is the tensor every later launch reads -- and grow='refit'
        rewrites)."""
        self._canvas_set = True
        self.mode.canvas_changed()
        if self.viewport is not None:
            self.bbox = self.bbox.to(torch.float32).contiguous()
            self.watch.start(self.watch.fit_boxes(self.bbox))
            self._cover_reset()
            return
        bb = self.bbox.cpu()
        self.hc, self.wc = _canvas_size(bb)
        self.watch.start(bb[None])
        self._cover_reset()

    def _regrown(self, rows):
        """grow='recapture': the watcher re-fixed the canvas -- new box, new size, a new output buffer (the graph is captured again)."""
        self.bbox = self.watch.boxes[0].to(self.dev)
        self.hc, self.wc = _canvas_size(self.watch.boxes[0])
        self.mode.canvas_changed()
        self._cover_reset()
        if self.static['out'] is not None:
            self.static['out'] = torch.empty((3, self.hc, self.wc), device=self.dev)

    # ------------------------------------------------------------------ coverage of the frames handed out (track_coverage)
    def _cover_reset(self):
        """The canvas was set or regrown: coverage starts again, on its size."""
        if self.track_coverage:
            self._cover = ops.coverage_state(self.hc, self.wc, self.dev)
            self.coverage_frames = 0

    def _cover_add(self, src, T):
        """The frame(s) of the splines src [V,63,2] | [k,V,63,2], T were handed out on the current canvas: one accumulate launch on
        the push's stream, behind their render."""
        if self._cover is not None:
            ops.coverage_update(self._cover, src, T, self.h, self.w, self.warp_mode)
            self.coverage_frames += 1 if src.dim() == 3 else int(src.shape[0])

    def covered_rect(self, even=False):
        """(y0, x0, h, w): the largest rectangle that every frame handed out on the current canvas covers (ops.covered_rect: largest
        area, then smallest y0, smallest x0, largest width; even: h and w rounded down to even) -- the window to cut from all of them
        for a video without a border; None before the canvas is fixed.  track_coverage stitchers only.  Synchronises (16 bytes)."""
        if not self.track_coverage:
            raise ValueError('covered_rect needs a stitcher built with track_coverage=True')
        if self._cover is None:
            return None
        return tuple(int(v) for v in ops.covered_rect(self._cover, even).cpu().tolist())

    def covered_rect_device(self, even=False):
        """covered_rect() left on the device: int32 [4] = (y0, x0, h, w) of the state at this moment, a new tensor per call -- the
        search's three launches on the push's stream, no synchronisation, nothing read back; None before the canvas is fixed.
        What ops.resample and to_size take as rect=."""
        if not self.track_coverage:
            raise ValueError('covered_rect_device needs a stitcher built with track_coverage=True')
        if self._cover is None:
            return None
        return ops.covered_rect(self._cover, even)

    def to_size(self, frames, size, aspect='fill', rect=None, out=None, out_format='bgr'):
        """What a push* just returned -- fp32 [3,hc,wc] | [k,3,hc,wc], or uint8 [hc,wc,3] | [k,hc,wc,3] -- resampled to exactly
        size = (Hout, Wout) on the covered rectangle: ops.resample (aspect, out, out_format: its own), one launch, nothing read back.
        rect=None uses covered_rect_device() of this moment: every frame is free of border, and the picture zooms in a little whenever
        the rectangle shrinks.  rect= a tensor the caller holds (an earlier covered_rect_device(), say after a warm-up) gives a
        steady zoom, at the price of border wherever a later frame covers less.  Which one is the caller's choice; the push, its
        graph and its frames are the same either way."""
        if not self.track_coverage:
            raise ValueError('to_size needs a stitcher built with track_coverage=True')
        ops._resample_size('to_size', size, aspect)
        if self._cover is None:
            raise ValueError('to_size: no canvas is fixed yet, so no frame has been handed out')
        want = (self.hc, self.wc)
        if not torch.is_tensor(frames) or frames.dim() not in (3, 4) or \
                (tuple(frames.shape[-3:-1]) if frames.dtype == torch.uint8 else tuple(frames.shape[-2:])) != want:
            raise ValueError('to_size takes frames of the current %d x %d canvas, as a push returns them, got %s'
                             % (want + ((frames.dtype, tuple(frames.shape)) if torch.is_tensor(frames) else type(frames).__name__,)))
        if rect is None:
            rect = self.covered_rect_device()
        elif not torch.is_tensor(rect):
            raise ValueError('to_size: rect is None or an int32 [4] device tensor (covered_rect_device), got %r' % (rect,))
        return ops.resample(frames, size, rect=rect, aspect=aspect, out=out, out_format=out_format)

    # ------------------------------------------------------------------ steady state
    def _versions(self):
        return tuple(n.weights_version for n in self.nets)

    def _trunk(self):
        """The twin stage-1 trunk (SpatialNet's and TemporalNet's stage-1 filters stacked: one grouped launch per layer)."""
        if self.trunk_pair is None:
            self.trunk_pair = L.pair_trunks(self.spatial._prepared()['s1'], self.temporal._prepared()['s1'])
            self.trunk_versions = self._versions()
        return self.trunk_pair

    def _stale_trunk(self):
        """Was a net reloaded / moved since the twin trunk was stacked (and the graphs captured)?  Both hold the OLD weights (the graphs
        by address): the caller drops them, to rebuild and recapture instead of silently stitching with stale filters."""
        return self.trunk_pair is not None and self.trunk_versions != self._versions()

    def _state(self):
        st = self.static
        return ([st[k] for k in _STATE] + ([] if self.meshes_only else [self.watch.wi, self.watch.wf] + self.watch.fit_state()) +
                ([] if self._exp_state is None else [self._exp_state]))

    @property
    def exposure_gains(self):
        """The smoothed exposure gains [2,3] (view, channel) the last frame was rendered with (ones before the first frame with a
        usable overlap); None without exposure=.  Synchronises."""
        if self._exp_state is None:
            return None
        self._sync_state()
        return self._exp_state[:6].reshape(2, 3).cpu()

    def _exposure_gains(self, views, fp):
        """The gains of the n frames `views` (V x [n,3,H,W] fp32 or [n,H,W,3] uint8) with footprint rows fp [n, .]: the stream's
        state advanced through them in order -> [n,V,3]."""
        return ops.exposure_update(views, fp, self.hc, self.wc, self._exp_state, self.exposure, self.warp_mode)

    def _drop_graphs(self):
        """The canvas grew or a net was reloaded: the captured steady-state graphs hold the old canvas / weights by address."""
        self.graph = None
        for B in self._batch.values():
            B['graph'] = None

    def _direct(self):
        """Does the steady-state push launch its render itself, outside the graph, on the caller's frames (DIRECT_RENDER; LINEAR
        fusion: DIRECT_LINEAR too, plain stitchers only)?  Decided when the stitcher is built."""
        return self.mode.direct

    def _u8_steady(self):
        return self.static is not None and self._direct() and self._U8_STEADY

    def _refresh(self):
        """Start of a steady-state push or batch: the watcher's growth check (grow='recapture'), then the weights check; either drops
        the captured graphs."""
        if self.grow == 'recapture' and not self.meshes_only:
            rows = self.watch.poll()
            if rows:
                self._regrown(rows)
                self._drop_graphs()
        if self._stale_trunk():
            self.trunk_pair = None
            self._drop_graphs()

    def _push_static(self, *frames, u8=None, nv12=None):
        """One steady-state push: frames = its HR frames then its LR frames, or u8 = its decoded uint8 frames (push_u8), or nv12 =
        (its decoded NV12 frames, the output format) (push_nv12).  The step -- and so the captured graph -- is the same for all three:
        they differ in what writes the graph's LR inputs in front of it and in the render behind it."""
        self._refresh()
        if nv12 is not None:                 # the cv2-exact resize of the converted bytes writes the graph's LR inputs
            for img, lr in zip(nv12[0], self._lr_inputs()):
                ops.ingest_nv12(img, pipeline.LR_H, pipeline.LR_W, want_hr=False, lr_out=lr)
        else:
            self._load(frames, u8)
        if not self.use_graph:
            self._step_static()
        else:
            if self.graph is None:
                (self.graph,), self.graph_nodes = _capture(self.dev, self._state(), self._step_static, [self._step_static])
            self.graph.replay()
        self.frames_in += 1
        if self.meshes_only:             # the newest smoothed meshes (m1, m2): copies, the step's own tensors are reused
            return tuple(m.clone() for m in self.last_meshes)
        if self.grow == 'recapture':
            self.watch.post_copy()
        if nv12 is not None:
            out = [self.mode.frame_nv12(nv12[0], self._deferred, self.hc, self.wc, nv12[1])]
        else:
            out = self._take(self._deferred, self.static['out'], u8 or frames[:len(frames) // 2], u8 is not None)
        if self._cover is not None and self._direct():       # (a step that renders itself has added its frame: _render_solved)
            self._cover_add(self._deferred.src, self._deferred.T)
        return out

    def _take(self, left, out, imgs, u8):
        """A push's frames: without the direct render copies of the step's output `out`; with it, rendered now from the caller's
        frames imgs (HR frames, or uint8 frames when u8) and the _Deferred `left` by the step into new tensors."""
        if not self._direct():
            return [[o.clone()] for o in out] if isinstance(out, list) else [out.clone()]
        return self._render_direct(left, imgs, u8)

    def _render_solved(self, imgs, src, T, out=None, watch=None, fit=None):
        """src [V,63,2] normalised control points on this canvas, T [V,2,66] their splines -> the stitched frame of the V = 2 | 3 views
        imgs [1,3,H,W] (written to `out` if given; out=_DEFER: nothing is rendered -> the _Deferred for the push's render, kept in
        self._deferred).  watch = (guard, watch_i [1,4], watch_f [1,4]): the overflow watcher has not seen `src` yet; fit
        (grow='refit'): the ops.CanvasFit of this canvas -- the launch that carries the watcher re-fixes the box behind it."""
        fp, efp = self.mode.footprints(src[None], T[None], self.hc, self.wc, watch, fit)
        left = _Deferred(src, T, None if fp is None else fp[0], efp)
        if out is _DEFER:                    # (exposure: the update reads the frames the render reads -- the push runs both on the caller's)
            self._deferred = left
            return left
        gains = None
        if efp is not None:
            gains = self._exposure_gains([f.reshape(1, 3, self.h, self.w) for f in imgs], efp)
        frame = self.mode.render_into(imgs, left, self.hc, self.wc, gains, out)
        self._cover_add(src, T)
        return frame

    def _grown(self, bb):
        """A box (wmin, wmax, hmin, hmax) grown by the margin on every side, on the device."""
        bb = bb.cpu()
        gw, gh = self.margin * (bb[1] - bb[0]), self.margin * (bb[3] - bb[2])
        return torch.stack((bb[0] - gw, bb[1] + gw, bb[2] - gh, bb[3] + gh)).to(self.dev)

    def _render_direct(self, left, imgs, u8):
        """One canvas, two or three views."""
        gains = None
        if left.efp is not None:             # the gains through this frame, from the caller's frames, in front of the render launch
            shp = (1, self.h, self.w, 3) if u8 else (1, 3, self.h, self.w)
            gains = self._exposure_gains([f.reshape(shp) for f in imgs], left.efp)
        return [self.mode.frame(imgs, left, self.hc, self.wc, u8, gains)]

    def _push_u8(self, imgs):
        """push_u8 of V views (checked): in the steady state with the direct render the resize writes the graph's LR inputs and the
        render samples the uint8 frames; every other configuration, and the window fill, goes ingest_u8 -> _push -> canvas_to_u8."""
        with ops.deterministic(self.deterministic):
            if self._u8_steady():
                return self._push_static(u8=tuple(i.contiguous() for i in imgs))
            if imgs[0].dim() == 4:           # S streams: every view's [S,H,W,3] where it lies, a launch per view
                hr, lr = zip(*[ops.ingest_u8(i, pipeline.LR_H, pipeline.LR_W) for i in imgs])
            else:                            # one stream: its V frames [H,W,3] in one launch
                hr, lr = (t.split(1) for t in ops.ingest_u8(torch.stack(imgs, 0), pipeline.LR_H, pipeline.LR_W))
            return _to_u8(self._push(*hr, *lr))

    def _push_nv12(self, imgs, out):
        """push_nv12 of V views (checked): the steady state with the direct render samples the caller's NV12 frames where the mode
        has an NV12 render; every other configuration, and the window fill, goes ingest_nv12 -> _push -> canvas_to_u8
        (-> bgr_to_nv12)."""
        with ops.deterministic(self.deterministic):
            if self._u8_steady() and self.mode.nv12:
                return self._push_static(nv12=(imgs, out))
            v = len(imgs)
            hr = torch.empty((v, 3, self.h, self.w), device=self.dev)
            lr = torch.empty((v, 3, pipeline.LR_H, pipeline.LR_W), device=self.dev)
            for k, img in enumerate(imgs):
                ops.ingest_nv12(img, pipeline.LR_H, pipeline.LR_W, hr_out=hr[k:k + 1], lr_out=lr[k:k + 1])
            frames = self._push(*([hr[k:k + 1] for k in range(v)] + [lr[k:k + 1] for k in range(v)]))
            frames = _to_u8(frames)
            return [ops.bgr_to_nv12(f) for f in frames] if out == 'nv12' else frames

    # ------------------------------------------------------------------ k frames of every view per call (one canvas)
    # A subclass provides _push (one plain push), push_u8, _batch_buffers (the per-k work buffers, 'lr' [V,k,3,360,480] among
    # them: _PairStep's) and _step_batch (the capturable batched step: _PairStep._batch_meshes, then what follows the meshes,
    # ending with _leave_batch: the _Deferred in B['deferred']).
    def _push_many(self, frames):
        """push_many of V views: frames = the V HR batches [k,3,H,W] then the V LR batches [k,3,360,480]."""
        k = self._check_many(frames)
        v = len(frames) // 2
        _check_shapes('HR frames', frames[:v], ((k, 3, self.h, self.w),))
        _check_shapes('LR frames', frames[v:], ((k, 3, pipeline.LR_H, pipeline.LR_W),))
        if any(f.dtype != torch.float32 for f in frames):
            raise ValueError('push_many takes fp32 frames')
        frames = tuple(f.contiguous() for f in frames)
        with ops.deterministic(self.deterministic):
            out, i = [], 0
            while self.static is None and i < k:          # window fill: one frame of every view at a time
                out += self._push(*[f[i:i + 1] for f in frames])
                i += 1
            if i < k:
                out += self._push_batch(k - i, tuple(f[i:] for f in frames), None)
            return out

    def _push_many_u8(self, frames):
        """push_many_u8 of V views: frames = the V decoded uint8 batches [k,H,W,3]."""
        k = self._check_many(frames)
        _check_u8('%d uint8 [k,H,W,3] tensors' % len(frames), frames, (k, self.h, self.w, 3))
        frames = tuple(f.contiguous() for f in frames)
        with ops.deterministic(self.deterministic):
            out, i = [], 0
            while self.static is None and i < k:
                out += self.push_u8(*[f[i] for f in frames])
                i += 1
            if i < k:
                out += self._push_batch(k - i, None, tuple(f[i:] for f in frames))
            return out

    def _push_many_nv12(self, views, out):
        """push_many_nv12 of V views: every view's k decoded NV12 surfaces -> packed BGR in ONE converter launch for all V k of them
        (ops.nv12_to_bgr), then _push_many_u8; out='nv12': one ops.bgr_to_nv12 over the call's frames behind it."""
        surfs = _check_many_nv12(self, views, out, 'push_many_nv12')
        if not L.QUAD:
            raise ValueError('push_many needs the shared regressor launches (SS_QUAD_REGRESSOR=1)')
        k = len(surfs[0])
        bgr = ops.nv12_to_bgr([s for view in surfs for s in view])
        frames = self._push_many_u8(tuple(bgr[v * k:(v + 1) * k] for v in range(len(surfs))))
        return _frames_to_nv12(frames) if out == 'nv12' else frames

    def _check_many(self, frames):
        """push_many's refusals that do not depend on the frame type -> k."""
        if self.meshes_only:
            raise ValueError('push_many renders frames: not for meshes_only stitchers')
        if not L.QUAD:
            raise ValueError('push_many needs the shared regressor launches (SS_QUAD_REGRESSOR=1)')
        if any(not torch.is_tensor(f) or f.dim() == 0 for f in frames):
            raise ValueError('push_many takes batched device tensors')
        k = int(frames[0].shape[0])
        if any(int(f.shape[0]) != k for f in frames):
            raise ValueError('push_many: the frame batches differ in length: %s' % [int(f.shape[0]) for f in frames])
        if not 1 <= k <= BATCH_MAX:
            raise ValueError('push_many takes 1 to %d frames of every view per call, got %d' % (BATCH_MAX, k))
        return k

    def _batch_entry(self, k):
        """Work buffers (and graph) of batch size k, allocated once; the least recently used size beyond BATCH_GRAPHS is dropped."""
        B = self._batch.pop(k, None)
        if B is None:
            B = dict(self._batch_buffers(k), k=k, graph=None, deferred=None)
        self._batch[k] = B
        while len(self._batch) > BATCH_GRAPHS:
            self._batch.popitem(last=False)
        return B

    def _push_batch(self, k, frames, u8):
        """k steady-state frames of every view: frames = (V HR batches, V LR batches) [k,...], or u8 = V decoded batches [k,H,W,3]."""
        self._refresh()
        B = self._batch_entry(k)
        views = len(u8) if u8 is not None else len(frames) // 2
        for v in range(views):
            if u8 is not None:               # the cv2-exact resize writes the step's LR inputs
                ops.ingest_u8(u8[v], pipeline.LR_H, pipeline.LR_W, want_hr=False, lr_out=B['lr'][v])
            else:
                B['lr'][v].copy_(frames[views + v])
        if not self.use_graph:
            self._step_batch(B)
        else:
            if B['graph'] is None:
                (B['graph'],), self.graph_nodes_batch[k] = _capture(self.dev, self._state(), lambda: self._step_batch(B),
                                                                    [lambda: self._step_batch(B)])
                self.batch_captures += 1
            B['graph'].replay()
        self.frames_in += k
        if self.grow == 'recapture':
            self.watch.post_copy()
        out = self._render_batch(B['deferred'], u8 if u8 is not None else frames[:views], u8 is not None)
        self._cover_add(B['deferred'].src, B['deferred'].T)
        return out

    def _leave_batch(self, B, src, T):
        """End of a batched step: the watcher over its k frames src [k,V,63,2], the footprints where the step needs them, and the
        _Deferred in B['deferred']."""
        guard, wi, wf = self.watch.args()
        ops.canvas_watch_frames(src, wi, wf, guard, fit=self.watch.fit_args())
        B['deferred'] = _Deferred(src, T, *self.mode.footprints(src, T, self.hc, self.wc))

    def _render_batch(self, left, imgs, u8):
        """The batch's frames from the caller's frames imgs (V x [k,3,H,W] fp32, or [k,H,W,3] uint8 when u8) in one render."""
        views = [f.contiguous() for f in imgs]
        # exposure: the k frames' gains in one update (stream order, bit-identical to k single-frame updates)
        gains = None if left.efp is None else self._exposure_gains(views, left.efp)
        return list(self.mode.batch(views, left, self.hc, self.wc, u8, gains).unbind(0))


class _PairStep:
    """Mixin: the steady-state step of S two-view streams advancing together, from their LR frames to their newest smoothed meshes --
    THE place where a streaming push advances its state.  OnlineStitcher runs it with S = 1, MultiOnlineStitcher with its S (chain:
    the S pairs are the neighbours of a chain of S + 1 views, each passing the trunks once), ThreeViewOnlineStitcher through its
    `chains`.  State layout (_pair_static; fixed addresses, the step is captured):
      lr1, lr2 [S,3,360,480] back to back (chain: lrc [S+1,3,360,480]), hr1, hr2 [S,3,H,W] only where the graph renders
      pair_s [2 views][prev, new][S][126]   spatial motions of the previous and the current pair
      pair_t [2 views][zero, new][S][126]   temporal motions (slot 0 stays zero; rewritten in full by every push)
      ring   [smesh v0, smesh v1, tsm v0, tsm v1][S][7][126]     the sliding SmoothNet windows
      prev_feat [2 S,45,60,128] view-major (chain: [S+1,45,60,128])   TemporalNet stage-1 features of the previous frame
    A class provides _init_static (the state its window fill left -> _pair_static) and _tail (what follows the meshes).
    push_many's k frames per call advance the same state through `_batch_meshes` (one pair, or the pairs of a chain)."""
    S, chain = 1, False

    def _pair_static(self, prev_feat, pair_s, ring):
        d, S, e = self.dev, self.S, 126
        lr = torch.empty((2, S, 3, pipeline.LR_H, pipeline.LR_W), device=d)       # both views back to back: one layout launch per push
        # frame copies only where the graph renders (meshes_only: no render; direct: the push renders from the caller's frames)
        inside = not self.meshes_only and not self._direct()
        hr = torch.empty((2, S, 3, self.h, self.w), device=d) if inside else (None, None)
        self.static = {'hr1': hr[0], 'hr2': hr[1], 'lr1': lr[0], 'lr2': lr[1],
                       # (chain: the S + 1 views once -- pair s holds views s and s + 1; ops.cost_volume(chain=S) pairs them up)
                       'lrc': torch.empty((S + 1, 3, pipeline.LR_H, pipeline.LR_W), device=d) if self.chain else None,
                       'prev_feat': prev_feat, 'pair_s': pair_s, 'pair_t': torch.zeros((2, 2, S, e), device=d), 'ring': ring,
                       'ts_out': torch.empty((2, 4 * S, e), device=d),
                       # the render's targets inside the graph: per class ('out_all': all streams' canvases as one tensor)
                       'out': None, 'out_all': None}

    def _load(self, frames, u8):
        st, S = self.static, self.S
        if u8 is not None:               # decoded uint8 frames (push_u8): the cv2-exact resize writes the graph's LR inputs itself
            for img, lr in zip(u8, (st['lr1'], st['lr2'])):
                ops.ingest_u8(img.reshape(S, self.h, self.w, 3), pipeline.LR_H, pipeline.LR_W, want_hr=False, lr_out=lr)
            return
        hr1, hr2, lr1, lr2 = frames
        if self.chain:                   # (pair s = views s, s + 1: lr1 holds views 0 .. S-1, lr2's last row is view S)
            st['lrc'][:S].copy_(lr1); st['lrc'][S:].copy_(lr2[S - 1:])
        else:
            st['lr1'].copy_(lr1.reshape(st['lr1'].shape)); st['lr2'].copy_(lr2.reshape(st['lr2'].shape))
        if st['hr1'] is not None:        # (meshes_only: the frames are not looked at, None will do; direct: rendered where they lie)
            st['hr1'].copy_(hr1.reshape(st['hr1'].shape)); st['hr2'].copy_(hr2.reshape(st['hr2'].shape))

    def _step_static(self):
        """One steady-state push on the static buffers (capturable: no host sync, no data-dependent shapes; every result
        lands in place -- no torch op in the step besides the copy of the cached features)."""
        st = self.static
        f2, off1 = self._stage_a(st['lrc'] if self.chain else (st['lr1'], st['lr2']))
        out = st['out'] if st['out_all'] is None else st['out_all']
        self._stage_b(f2[0], f2[1], off1, st['hr1'], st['hr2'], _DEFER if self._direct() else out)

    def _stage_a(self, lr):
        """First half of a steady-state push -- it touches NO stream state: both nets' stage-1 trunks on the LR frames (one grouped
        launch per layer: SpatialNet and TemporalNet read the same frames through trunks of identical architecture), then
        SpatialNet's stage-2 trunk, contextual correlation and regressNet1.
        lr: the two views' frames (lr1, lr2), [S,3,360,480] each, or -- chain -- the S + 1 views' frames [S+1,3,360,480], each once
        -> (f2 [2(net), 2 S view-major (chain: S + 1), 45,60,128]: f2[0] SpatialNet's, f2[1] TemporalNet's features; offset_1 [S,8] |
        None)."""
        f2 = L.run_stage1_pair([lr] if self.chain else list(lr), self._trunk())
        return f2, (_heads_a(self.spatial, f2[0], self.S, self.chain) if L.QUAD else None)

    def _stage_b(self, f64, feat, off1, hr1, hr2, out):
        """Second half: everything that reads or advances the streams' state (cached features, previous motions, the sliding
        windows) -> the smoothed meshes of the S newest windows, then the class's `_tail`: the render of the new frames into `out`
        (out=_DEFER: splines and footprints only, the push launches the render itself), or the meshes themselves (meshes_only)."""
        st, S, e = self.static, self.S, 126
        ps, pt = st['pair_s'], st['pair_t']
        tm_out = (pt[0, 1], pt[1, 1])
        if off1 is None:
            off1, off_ref, off_tgt = _spatial_temporal_heads(self.spatial, self.temporal, f64, st['prev_feat'], feat, S, tm_out,
                                                             chain=self.chain)
        else:
            off_ref, off_tgt = _heads_b(self.spatial, self.temporal, f64, off1, st['prev_feat'], feat, S, tm_out, self.chain)
        ops.spatial_meshes(off1, off_ref, off_tgt, pipeline.LR_H, pipeline.LR_W,
                           out=(ps[0, 1].view(S, 7, 9, 2), ps[1, 1].view(S, 7, 9, 2)))
        st['prev_feat'].copy_(feat)
        # tsmotion of all streams and both views as ONE batch of 4 S frames laid out [view][prev, new][stream]: frame k pairs
        # with frame k - S (its own stream's previous frame); the rows of the `prev` halves are computed and ignored
        ops.tsmotion(ps.view(4 * S, 7, 9, 2), pt.view(4 * S, 7, 9, 2), pipeline.LR_H, pipeline.LR_W,
                     out=(st['ts_out'][0], st['ts_out'][1]), lag=S)
        # shift the 4 S rings, append this push's rows (smesh v0, smesh v1, tsm v0, tsm v1 of every stream), and make the
        # current spatial motions the previous ones
        ops.window_push(st['ring'] if S > 1 else st['ring'].view(4, WINDOW, e), st['ts_out'],
                        [1 * S * e, 3 * S * e, (4 * S + 1 * S) * e, (4 * S + 3 * S) * e], state=ps,
                        blocks=2, block=S * e, stride=2 * S * e, delta=S * e, per=S)
        r = st['ring'].view(4, S * WINDOW, 7, 9, 2)
        outs, _ = self.smooth.run_windows(r[0], r[1], r[2], r[3], S, WINDOW, WINDOW, 1)       # S windows, one per stream
        self._tail(outs['smooth_mesh1'], outs['smooth_mesh2'], hr1, hr2, out)                # [S,7,7,9,2]

    # ------------------------------------------------------------------ k frames of every view per call
    def _batch_buffers(self, k):
        """The work buffers of `_batch_meshes` at batch size k (its docstring has their layout)."""
        d, S, e = self.dev, self.S, 126
        fh, fw = pipeline.LR_H // 8, pipeline.LR_W // 8
        B = {'lr': torch.empty((S + 1, k, 3, pipeline.LR_H, pipeline.LR_W), device=d),
             'feat': torch.empty((S + 1, k + 1, fh, fw, 128), device=d),
             'sw': torch.empty((2, S, k + 1, e), device=d),
             'tt': torch.zeros((2, S, k + 1, e), device=d),              # (slot 0 stays zero)
             'ts': torch.empty((2, 2 * S * (k + 1), e), device=d),
             'work': torch.empty((4 * S, WINDOW - 1 + k, e), device=d)}
        if S > 1:                        # the heads' outputs [pair view][pair][k], back to back: see _batch_meshes
            B['sn'], B['tn'] = torch.empty((2, S * k, e), device=d), torch.empty((2, S * k, e), device=d)
        return B

    def _batch_meshes(self, B):
        """A chain of V = S + 1 views advanced by k frames from B['lr'] (capturable) -> the smoothed windows (m1, m2) [nw,7,7,9,2];
        prev_feat, the previous motions pair_s[:, 0] and ring are read once and left as k `_step_static` runs leave them (the
        `new` slot pair_s[:, 1], scratch of a single push, is not written).  Per frame the launches of
        `_stage_a` / `_stage_b`, the networks seeing the k frames as one batch.  A single pair is the chain of two views: this
        runs for OnlineStitcher (S = 1) and for ThreeViewOnlineStitcher's chains (S = 2, chain) and for nothing else --
        independent streams times k frames would need another trunk layout.  Layout (B = _batch_buffers(k)):
          lr   [V][k]        the views' LR frames, each view once: one trunk pass over V k images, view-major; pair (s, j) --
                             chain s, frame j -- is images (s k + j, (s + 1) k + j) of its output
          feat [V][k + 1]    TemporalNet's features [previous frame, the k frames]: volume (v, j) pairs slots (j, j + 1) of view
                             v, read where they lie (ss_cost_volume_chain_frames)
          sw, tt [2 pair views][S][k + 1][126]   spatial / temporal motions [previous | zero, the k frames] of every sequence
          ts   [2][2 S (k + 1)][126]             tsmotion's (smesh, tsmotion) of those rows: row j pairs with row j - 1 of its
                                                 sequence, slot 0's rows are computed and ignored
          work [4 S][W - 1 + k][126]             the k sliding windows of ring r = q S + s, ring kind q (smesh of the first /
                                                 second pair view, tsmotion of the first / second) <- rows 1 .. k of its sequence
        SmoothNet runs each kind's rows as ONE run of nw windows, window w starting at row w: frame j of chain s is window
        s (W - 1 + k) + j (the W - 1 windows that straddle two chains are computed and ignored), its mesh that window's last."""
        st, S, k, e = self.static, self.S, B['k'], 126
        assert (S, self.chain) in ((1, False), (2, True)), 'the k-frame step runs one pair, or the two pairs of a chain of three views'
        F, sw, tt, ts = B['feat'], B['sw'], B['tt'], B['ts']
        f2 = L.run_stage1_pair([B['lr'].view((S + 1) * k, 3, pipeline.LR_H, pipeline.LR_W)], self._trunk())   # [2(net), V k, 45,60,128]
        f64 = f2[0]
        off1 = _heads_a(self.spatial, f64, S * k, k)
        F[:, 0].copy_(st['prev_feat'])
        F[:, 1:].copy_(f2[1].view(F[:, 1:].shape))
        cv_s = self.spatial.cv_from_offset1(f64[:S * k], f64[k:k + S * k], off1, pipeline.LR_H, pipeline.LR_W)
        cv_t = ops.cost_volume_chain_frames(F, 3)                               # [2 (pair view), S, k, 45,60,52]
        off_ref = torch.empty((S * k, e), device=self.dev, dtype=torch.float32)
        off_tgt = torch.empty((S * k, e), device=self.dev, dtype=torch.float32)
        # the heads write [pair view][pair][k] rows back to back.  S = 1: those are rows 1 .. k of sw[v] / tt[v], written in place;
        # S > 1: there they are strided by pair, so sn / tn take them
        sn, tn = (sw[:, 0, 1:], tt[:, 0, 1:]) if S == 1 else (B['sn'], B['tn'])
        L.run_regressor_quad(cv_s, cv_t.view((2, S * k) + tuple(cv_t.shape[3:])), L.get_quad(self.spatial, self.temporal),
                             [off_ref, off_tgt, tn[0], tn[1]])
        st['prev_feat'].copy_(F[:, k])
        ops.spatial_meshes(off1, off_ref, off_tgt, pipeline.LR_H, pipeline.LR_W,
                           out=(sn[0].view(S * k, 7, 9, 2), sn[1].view(S * k, 7, 9, 2)))
        ps = st['pair_s']                                                       # [pair view][previous, new][S][126]
        # the previous spatial motions into slot 0 of every sequence, and the newest made the previous ones (pair_s[:, 0]; the `new`
        # slot pair_s[:, 1], which every push writes before it reads it, stays as it is).  S = 1: ss_window_advance below carries
        # that move (`move`); S > 1: sw and tt are put together from sn / tn, and the move is a copy
        if S == 1:
            sw[:, :, 0].copy_(ps[:, 0])
            move = dict(state=ps, state_src=sw.view(-1)[k * e:], blocks=2, block=e, stride=2 * e, src_stride=(k + 1) * e)
        else:
            torch.cat((ps[:, 0].view(2, S, 1, e), sn.view(2, S, k, e)), 2, out=sw)
            tt[:, :, 1:].copy_(tn.view(2, S, k, e))
            ps[:, 0].copy_(sw[:, :, k])
            move = {}
        ops.tsmotion(sw.view(-1, 7, 9, 2), tt.view(-1, 7, 9, 2), pipeline.LR_H, pipeline.LR_W, out=(ts[0], ts[1]))
        n1 = k + 1
        offs = [((q // 2) * 2 * S * n1 + ((q % 2) * S + s) * n1 + 1) * e for q in range(4) for s in range(S)]
        ops.window_advance(st['ring'].view(4 * S, WINDOW, e), B['work'], ts, offs, k, **move)
        wk = B['work'].view(4, S * (WINDOW - 1 + k), 7, 9, 2)
        nw = (S - 1) * (WINDOW - 1 + k) + k
        outs, _ = self.smooth.run_windows(wk[0], wk[1], wk[2], wk[3], nw, WINDOW, 1, 1)
        return outs['smooth_mesh1'], outs['smooth_mesh2']


class OnlineStitcher(_PairStep, _Stitcher):
    """One live two-view stream (the module docstring): the window fill (`_push`), then _PairStep's steady-state step with S = 1; the
    tail behind the meshes is `_render` -- splines, watcher, footprints, exposure and every fusion mode, MULTIBAND included."""
    _MULTIBAND = True

    def __init__(self, nets, height, width, canvas=None, margin=0.03, warp_mode='NORMAL', fusion_mode='AVERAGE',
                 use_graph=True, grow='never', meshes_only=False, deterministic=False, viewport=None, zoom_limit=2.0, exposure=None,
                 bands=None, seam=None, seam_cell=None, seam_mu=None, seam_prior=None, track_coverage=False):
        """canvas: optional (wmin, wmax, hmin, hmax) in HR pixels (e.g. the offline bbox).
        track_coverage: keep, on the device, which canvas pixels EVERY frame handed out so far covers: one small launch
        per push (per push_many call) behind the render, outside the graph; `covered_rect()` then gives the largest rectangle with
        picture in every pixel of every frame, `coverage_frames` the frames it stands for.  It starts again when the canvas changes
        (grow='recapture').  Not with meshes_only, grow='refit', or a captured step that renders inside its graph.
        seam: None / 'geometric' (MULTIBAND's seam where the warped weight planes cross) or 'dp' -- the content-aware seam (DESIGN.md 7f;
        only with MULTIBAND): ops.multiband_seam between the warp and the blend of every frame handed out, on a grid of seam_cell x
        seam_cell cells, with seam_mu holding the seam to the previous frame's and seam_prior to the geometric one (defaults:
        ops.seam_params).  The previous seams belong to the stream AND its canvas: they are forgotten when the canvas is set and at every
        grow='recapture' regrow (grow='refit' moves the box under a fixed grid on the device: the state stays).
        fusion_mode: 'AVERAGE', 'FEATHER', 'LINEAR' or 'MULTIBAND' -- the Laplacian-pyramid blend of `bands` levels
        (0..6, default 5; only with MULTIBAND): the existing warp of B, G, R and a weight plane, then the pyramid launches, always
        launched by the push on the caller's frames (the graph ends with the splines); not with exposure=.
        exposure: None (default: nothing of it exists), True (ops.ExposureParams() defaults) or an ops.ExposureParams -- exposure
        compensation of the two cameras: every frame handed out (the first window's seven, in order, included) is rendered with
        per-view, per-channel gains estimated on that frame's overlap (the footprint lattice: DESIGN.md, "Exposure compensation")
        and smoothed through that frame; `exposure_gains` reads them.  The gain state belongs to the stream: a regrown or recaptured
        canvas keeps it.  Not with meshes_only, not with push_nv12.
        viewport: optional (Hout, Wout), each in 11..65535 -- the size of EVERY frame this stitcher returns ([3,Hout,Wout] fp32,
        [Hout,Wout,3] uint8 from push_u8 / push_many_u8; the first window's seven included), known from construction: `hc, wc ==
        Hout, Wout`, so an encoder or a pinned result ring can be sized before the first push.  The canvas box is the box the
        stitcher would have had (the first window's box grown by `margin`, or `canvas`), letterboxed about its centre to the
        viewport's aspect (it only ever expands; untouched when ow * Hout == oh * Wout in fp32); the render samples the continuous
        warp at the viewport's pixel lattice.  A viewport smaller than the box is POINT-SAMPLED: nothing prefilters, fine detail
        aliases.  None (default): the size is the box' extent in whole pixels, as ever.
        deterministic: every push under the conv engine's geometry-only kernel policy (ops.deterministic): with the offline canvas the
        stream's frames equal the resident clip's (pipeline.run_two_view(..., deterministic=True)) bit for bit; ~1.6x slower pushes.
        meshes_only: no canvas, no render -- `push` returns the newly smoothed meshes (m1, m2) [k,7,9,2] (k = 7 on the 7th push,
        then 1) or None; the building block of ThreeViewOnlineStitcher, which captures the graph itself (use_graph is ignored).
        grow: 'never' -- the canvas fixed after the first window stays (frames whose mesh leaves it are cropped and COUNTED:
        `clipped_frames`); 'recapture' -- the canvas grows (and the steady-state graph is captured again) when a mesh comes within
        half the margin of its edge; `canvas_epoch` counts the growths, `hc` / `wc` / `bbox` change with them; 'refit' (only with a
        viewport; 'recapture' not with one) -- the BOX is re-fixed on the device, inside the push's own launches, as soon as the
        watcher's running extents come within that guard: the picture zooms out (the new box contains the old one), while graphs,
        output buffers, workspaces and `hc` / `wc` stay as they are -- nothing is captured again, nothing synchronises.  A growth is
        refused, and such frames are cropped and counted as under 'never', when the new box is not finite, when an extent would
        exceed `zoom_limit` x the one the canvas was set with (a diverging mesh must not shrink the picture to nothing), or when no
        side moves by half a pixel.  `canvas_epoch`, `canvas_box` and `overflow_report()` then read the device (they synchronise).
        push_many takes one refit per call, behind the batch's watcher: a drift inside one call can crop up to k counted frames."""
        _exposure_params(exposure, meshes_only)
        _Stitcher.__init__(self, nets, height, width, margin, warp_mode, fusion_mode, use_graph, grow, meshes_only,
                           viewport=viewport, zoom_limit=zoom_limit, exposure=exposure, bands=bands,
                           seam=dict(seam=seam, seam_cell=seam_cell, seam_mu=seam_mu, seam_prior=seam_prior),
                           track_coverage=track_coverage)
        self.deterministic = bool(deterministic)
        self.last_meshes = None
        self.bbox = None if canvas is None else torch.tensor(canvas, dtype=torch.float32, device=self.dev)
        self.nrigid = get_norm_mesh(get_rigid_mesh(1, height, width, device=self.dev), height, width).contiguous()
        self.prev_feat = None            # TemporalNet stage-1 features of the previous frame, both views [2,45,60,128]
        self.prev_smotion = None         # [2,7,9,2]
        self.ring_smesh = [[], []]       # last WINDOW spatial meshes per view, each [1,7,9,2]
        self.ring_tsm = [[], []]
        self.ring_hr = []                # HR frames waiting for their smoothed mesh (only until the first window)

    @torch.no_grad()
    def _render(self, hr1, hr2, mesh1, mesh2, out=None):
        """mesh* [1,7,9,2] LR-scale smoothed meshes of ONE frame -> stitched frame [3,Hc,Wc] (written to `out` if given).  Control
        points + splines in one launch, the watcher inside the footprint launch."""
        src4, T4 = ops.stream_splines([mesh1, mesh2], 126, self.bbox, self.nrigid, self.h, self.w)
        return self._render_solved([hr1, hr2], src4[0], T4[0], out, watch=self.watch.args(), fit=self.watch.fit_args())

    # ------------------------------------------------------------------ steady state (window full, canvas fixed)
    def _init_static(self):
        """The window fill's state in the S = 1 layout of _PairStep; an output canvas only where the graph renders."""
        e = 126
        pair_s = torch.zeros((2, 2, 1, e), device=self.dev)
        pair_s[:, 0, 0] = self.prev_smotion.reshape(2, e)
        ring = torch.stack([torch.cat(r, 0).reshape(1, WINDOW, e) for r in (self.ring_smesh[0], self.ring_smesh[1],
                                                                             self.ring_tsm[0], self.ring_tsm[1])], 0).contiguous()
        self._pair_static(self.prev_feat.clone(), pair_s, ring)
        if self.static['hr1'] is not None:
            self.static['out'] = torch.empty((3, self.hc, self.wc), device=self.dev)

    def _tail(self, m1, m2, hr1, hr2, out):
        m1, m2 = m1[0, -1:], m2[0, -1:]          # the newest frame's meshes [1,7,9,2]
        if self.meshes_only:
            self.last_meshes = (m1, m2)
            return
        self._render(hr1, hr2, m1, m2, out=out)

    @torch.no_grad()
    def push(self, hr1, hr2, lr1, lr2):
        """One frame pair: hr* [1,3,H,W] (0..255), lr* [1,3,360,480] ([-1,1]), device tensors.
        -> list of newly stitched frames (empty for the first 6 pushes, 7 frames on the 7th, then one per push).
        meshes_only: -> None for the first 6 pushes, then (m1, m2) [k,7,9,2] (k = 7 on the 7th push, then 1)."""
        self._check_push((hr1, hr2), (lr1, lr2))
        with ops.deterministic(self.deterministic):
            return self._push(hr1, hr2, lr1, lr2)

    def _check_push(self, hr, lr):
        """hr* [1,3,H,W] / [3,H,W] of this stitcher's H x W (meshes_only: None will do), lr* [1,3,360,480] / [3,360,480]."""
        if self.meshes_only:
            hr = [f for f in hr if f is not None]
        _check_shapes('HR frames', hr, ((1, 3, self.h, self.w), (3, self.h, self.w)))
        _check_shapes('LR frames', lr, _LR_SHAPES)

    @torch.no_grad()
    def push_u8(self, img1, img2):
        """One DECODED frame pair: img* uint8 [H,W,3] device tensors in cv2.imread's layout and channel order (the reference's frame
        loop, test_online_tra.py:252-278) -> list of stitched VIDEO frames uint8 [Hc,Wc,3] (`.astype(np.uint8)` of the fused values,
        :413), empty for the first 6 pushes, 7 frames on the 7th, then one per push.  Byte for byte ops.ingest_u8 -> push ->
        ops.canvas_to_u8; in the steady state (direct render: AVERAGE, or LINEAR with DIRECT_LINEAR) the cv2-exact resize writes the graph's LR inputs and
        the render samples the uint8 frames and writes the uint8 frame itself: no fp32 frame planes, no fp32 canvas.
        PipelinedOnlineStitcher: the frames of the PREVIOUS push come back, `flush_u8()` for the last; a stream is fed through
        push_u8 or through push, not both."""
        if self.meshes_only:
            raise ValueError('push_u8 renders frames: not for meshes_only stitchers')
        _check_u8('two uint8 [H,W,3] frames', (img1, img2), (self.h, self.w, 3))
        return self._push_u8((img1, img2))

    def _lr_inputs(self):
        return [self.static['lr1'], self.static['lr2']]

    @torch.no_grad()
    def push_nv12(self, img1, img2, out='bgr'):
        """One DECODED frame pair as a hardware decoder delivers it: img* uint8 NV12 [H*3/2,W] device tensors (rows 0..H-1 the Y
        plane, then the interleaved UV plane; a row stride > W -- a padded decoder surface -- is accepted) -> list of stitched video
        frames with push_u8's cadence: out='bgr' uint8 [Hc,Wc,3], byte for byte push_u8 of the frames converted to packed BGR
        ("Frame formats"); out='nv12' uint8 [Hc*3/2,Wc], byte for byte ops.bgr_to_nv12 of those -- what an encoder takes;
        it needs a stitcher built with an even viewport=(Hout, Wout).  In the steady state with the direct render no BGR frame
        exists on either side: the resize and the render's taps convert the bytes they read, and AVERAGE fusion writes NV12 itself
        (LINEAR: the uint8 frame, then the sink).  A stream is fed through one of push, push_u8 and push_nv12; the output format
        may change from push to push (the captured graph does not depend on it).  Not for the Pipelined / Multi stitchers."""
        if getattr(self, 'exposure', None) is not None:
            raise ValueError('push_nv12 has no exposure compensation yet: feed an exposure stitcher through push_u8 or push')
        _check_nv12(self, (img1, img2), out)
        return self._push_nv12((img1, img2), out)

    def _push(self, hr1, hr2, lr1, lr2):
        if self.static is not None:
            return self._push_static(hr1, hr2, lr1, lr2)
        t = self.frames_in
        # spatial warp of this pair
        o = build_SpatialNet(self.spatial, lr1, lr2)
        smotion = torch.cat((o['motion1'], o['motion2']), 0)                        # [2,7,9,2]
        # temporal warp: only the new frame goes through the trunk, the previous features are cached
        feat = self.temporal.features([lr1, lr2])                                   # [2,45,60,128]
        if t == 0:
            tmotion = torch.zeros_like(smotion)
        else:
            tmotion = self.temporal.motions_from_features(self.prev_feat, feat)
        self.prev_feat = feat
        # tsmotion of frame t from smotion_{t-1} (frame 0: zero)
        for v in range(2):
            if t == 0:
                smesh = get_rigid_mesh(1, pipeline.LR_H, pipeline.LR_W, device=self.dev) + smotion[v:v + 1]
                tsm = torch.zeros_like(smesh)
            else:
                pair_s = torch.cat((self.prev_smotion[v:v + 1], smotion[v:v + 1]), 0)
                pair_t = torch.cat((torch.zeros_like(tmotion[v:v + 1]), tmotion[v:v + 1]), 0)
                sm2, ts2 = ops.tsmotion(pair_s, pair_t, pipeline.LR_H, pipeline.LR_W)
                smesh, tsm = sm2[1:2], ts2[1:2]
            self.ring_smesh[v] = (self.ring_smesh[v] + [smesh])[-WINDOW:]
            self.ring_tsm[v] = (self.ring_tsm[v] + [tsm])[-WINDOW:]
        self.prev_smotion = smotion
        self.frames_in += 1
        if not self._canvas_set and not self.meshes_only:
            self.ring_hr.append((hr1, hr2))
        if self.frames_in < WINDOW:
            return None if self.meshes_only else []
        # smooth the current window (first tsmotion of the window counts as zero)
        sm = [torch.cat(self.ring_smesh[v], 0).contiguous() for v in range(2)]
        ts = [torch.cat(self.ring_tsm[v], 0).contiguous() for v in range(2)]
        outs, _ = self.smooth.run_windows(sm[0], sm[1], ts[0], ts[1], 1, WINDOW, 1, 1)
        m1, m2 = outs['smooth_mesh1'][0], outs['smooth_mesh2'][0]                   # [7,7,9,2]
        if self.meshes_only:                                                       # first window: 7 meshes, then the static step
            self.ring_hr = []
            self._init_static()
            self.last_meshes = (m1, m2)
            return self.last_meshes
        if not self._canvas_set:                                                   # first window: fix the canvas, emit 7
            if self.bbox is None:
                self.bbox = self._grown(ops.mesh_bbox([m1, m2], self.h, self.w))
            self._set_canvas()
            frames = [self._render(h1, h2, m1[i:i + 1], m2[i:i + 1]) for i, (h1, h2) in enumerate(self.ring_hr)]
            self.ring_hr = []
            self._init_static()              # from the next push on: static buffers (+ HIP graph)
            return frames
        return [self._render(hr1, hr2, m1[-1:], m2[-1:])]

    # ------------------------------------------------------------------ k frame pairs of the stream per call
    @torch.no_grad()
    def push_many(self, hr1, hr2, lr1, lr2):
        """k consecutive frame pairs of the stream in one call, 1 <= k <= BATCH_MAX: hr* [k,3,H,W] (0..255), lr* [k,3,360,480]
        ([-1,1]), fp32 device tensors -> the newly stitched frames [3,Hc,Wc] in stream order: what k calls of `push` return, joined
        (nothing for the first 6 frames, 7 at the 7th, then one per frame).  The frames of one call are views of one new tensor that
        no later call writes.  Frames before the first window is complete go through `push` one at a time; the rest of the call runs
        as ONE batched step (per frame the arithmetic of `push`; the networks see the k frames as one batch), captured into a HIP graph
        per batch size (BATCH_GRAPHS sizes kept, least recently used dropped).  The canvas is fixed within a call: with
        grow='recapture' a drift inside one call can crop up to k frames (counted) before the canvas grows at the next call.
        `push`, `push_u8` and `push_many(_u8)` interleave freely on one stitcher."""
        return self._push_many((hr1, hr2, lr1, lr2))

    @torch.no_grad()
    def push_many_u8(self, frames1, frames2):
        """k DECODED frame pairs: uint8 [k,H,W,3] device tensors (cv2 layout) -> stitched video frames uint8 [Hc,Wc,3], byte for byte
        what k calls of `push_u8` return, joined (see push_many)."""
        return self._push_many_u8((frames1, frames2))

    @torch.no_grad()
    def push_many_nv12(self, frames1, frames2, out='bgr'):
        """k DECODED frame pairs as a hardware decoder delivers them, 1 <= k <= BATCH_MAX: every view an NV12 device tensor
        [k,H*3/2,W] (any row and frame stride) or a list of k surfaces [H*3/2,W], each with its own pitch -- a decoder's surface pool
        -> the stitched video frames with push_many_u8's cadence: out='bgr' uint8 [Hc,Wc,3], byte for byte push_many_u8 of the frames
        converted to packed BGR; out='nv12' uint8 [Hc*3/2,Wc], byte for byte ops.bgr_to_nv12 of those, views of one
        tensor (an even viewport=, as push_nv12).  All 2 k surfaces are converted in ONE launch, the rest is push_many_u8: every
        fusion mode, seam=, viewport=, every grow and exposure= work as they do there.  Interleaves freely with the other entries."""
        return self._push_many_nv12((frames1, frames2), out)

    def _step_batch(self, B):
        """k consecutive steady-state frame pairs of the stream from B['lr'] (capturable): _PairStep's k-frame step, then the
        splines of the k frames in one launch; ends with the watcher and the footprints in B['deferred']."""
        m1, m2 = self._batch_meshes(B)                                           # [k,7,7,9,2]: frame j's mesh is window j's last
        src, T = ops.stream_splines([m1[0, -1], m2[0, -1]], WINDOW * 126, self.bbox, self.nrigid, self.h, self.w, frames=B['k'])
        self._leave_batch(B, src, T)


BATCH_MAX = 32                         # push_many: frames of every view per call
BATCH_GRAPHS = 4                       # batch sizes whose steady-state graphs (and work buffers) push_many keeps


# Steady-state AVERAGE render OUTSIDE the captured graph, on the caller's own HR frames and into a fresh tensor: the graph ends with the
# splines / footprints, the push saves the copies of the HR frames into static buffers and the clone of the static canvas (720p, three
# views: 66 + 50 MB of HBM traffic, ~35 us of a 1.1 ms push).  Same kernel, same operands: frames bit-identical.  Read when a stitcher
# is constructed.
DIRECT_RENDER = os.environ.get('SS_DIRECT_RENDER', '1') != '0'
# LINEAR fusion joins it (OnlineStitcher, MultiOnlineStitcher, ThreeViewOnlineStitcher): the graph ends with the splines and the
# watcher, the push renders through ops.render_linear_frames -- three launches (four with three views) for all S streams of a
# MultiOnlineStitcher, whatever their canvas sizes, instead of the per-frame chain warp + 7 blender launches + copy per stream; under
# push_u8 from the uint8 frames to the uint8 video frame.  Bit-identical frames.  Read when a stitcher is constructed.
DIRECT_LINEAR = os.environ.get('SS_DIRECT_LINEAR', '1') != '0'
# push_nv12(out='nv12') under AVERAGE fusion: the render writes NV12 itself (ops.render_average_nv12, out_format='nv12'); '0': it
# writes the uint8 frame and ops.bgr_to_nv12 follows, as under LINEAR.  Byte-identical frames (LAB_NOTES.md has the timing).
NV12_FUSED_SINK = os.environ.get('SS_NV12_FUSED_SINK', '1') != '0'
_DEFER = object()                      # `out=_DEFER`: compute splines and footprints, leave the render launch to the push
FUSED_SPLINES = os.environ.get('SS_FUSED_SPLINES', '1') != '0'   # ThreeViewOnlineStitcher: composition + splines in one launch
PIPE_STREAM_CANDIDATES = 5        # streams tried pairwise by _TwoInFlight._pick_streams
PIPE_PROBE_PUSHES = 8


class _TwoInFlight:
    """Mixin: the steady-state push as two halves on two HIP streams, two pushes in flight (PipelinedOnlineStitcher,
    PipelinedMultiOnlineStitcher).  A batch-1 push is a dependent chain of ~80 small launches that leaves most of the chip idle
    (profiles/r06_stream_timeline.txt: 0.86 ms; a graph node costs >= 4.5 us whatever it does), and nothing inside ONE push overlaps
    any further (LAB_NOTES R6.1-2).  Consecutive pushes do: the first half of a push -- both trunks, SpatialNet's stage-2 trunk,
    contextual correlation, regressNet1 (`_stage_a`) -- touches no stream state, so push t + 1's first half runs beside push t's second
    half (`_stage_b`: decomposition, cost volumes, regressor heads, tsmotion, sliding window, SmoothNet, render).  Each half is its own
    HIP graph per buffer parity; hand-over buffers are double-buffered, events order the halves.  Per frame the launches and their
    operands are the plain stitcher's: results are bit-identical.  What changes is WHEN a result is handed out: `push` returns the
    frames of the PREVIOUS push (valid on the caller's stream), `flush()` the last ones.
    LINEAR fusion stays inside the graphs here (_LINEAR_DIRECT = False): with two pushes in flight the direct LINEAR render would
    need a workspace per buffer parity.
    grow='refit' (with a viewport) holds with two pushes in flight: only second halves touch the canvas box (the splines launch reads
    it, the launch that carries the watcher rewrites it), and the second halves and direct renders of consecutive pushes all run in
    order on the ONE stream sb -- the box push t rewrites is the box push t + 1 reads.  grow='recapture' is not offered.
    The halves of a _PairStep push (_pipe_alloc / _pipe_load / _run_a / _run_b) are here; a subclass adds its output buffers to
    _pipe_alloc (and _pipe_empty for S streams), PipelinedThreeViewOnlineStitcher has its own three-view loads and second half."""
    _LINEAR_DIRECT = False
    _MULTIBAND = False       # (MULTIBAND is launched by the push on the caller's frames: not with two pushes in flight)

    def _pipe_init(self):
        if not L.QUAD:
            raise ValueError('%s needs the shared regressor launches (SS_QUAD_REGRESSOR=1)' % type(self).__name__)
        self.pipe = None
        self._pending = None             # (event behind it, result) of the newest enqueued push
        self._t = 0

    # ------------------------------------------------------------------ the halves of a _PairStep push, per buffer parity p
    def _pipe_alloc(self):
        """Both parities' inputs and hand-over buffers of S two-view streams; the class adds its outputs ('out', 'out_all')."""
        d, S = self.dev, self.S
        two = lambda *shape: [torch.empty(shape, device=d) for _ in range(2)]
        return {'lr': two(2, S, 3, pipeline.LR_H, pipeline.LR_W),
                'hr': [(None, None)] * 2 if self._direct() else two(2, S, 3, self.h, self.w),       # (direct render: no copies)
                'f2': two(2, 2 * S, pipeline.LR_H // 8, pipeline.LR_W // 8, 128), 'off1': two(S, 8)}

    def _pipe_load(self, p, sa, sb, hr1, hr2, lr1, lr2):
        lr, hr = self.pipe['lr'][p], self.pipe['hr'][p]
        if hr1.dtype == torch.uint8:         # push_u8: decoded frames -- the cv2-exact resize writes this parity's LR inputs
            with torch.cuda.stream(sa):
                for v, img in enumerate((hr1, hr2)):
                    ops.ingest_u8(img.reshape(self.S, self.h, self.w, 3), pipeline.LR_H, pipeline.LR_W, want_hr=False, lr_out=lr[v])
            for t in (hr1, hr2):
                t.record_stream(sa)
                t.record_stream(sb)
            return
        with torch.cuda.stream(sa):
            lr[0].copy_(lr1.reshape(lr[0].shape)); lr[1].copy_(lr2.reshape(lr[1].shape))
        if not self._direct():                  # (direct render: the second stream's render reads the caller's frames)
            with torch.cuda.stream(sb):
                hr[0].copy_(hr1.reshape(hr[0].shape)); hr[1].copy_(hr2.reshape(hr[1].shape))
        for t in (hr1, hr2):
            t.record_stream(sb)
        for t in (lr1, lr2):
            t.record_stream(sa)

    def _run_a(self, p):
        """The first half; the two nets' features are handed over with a copy each (PipelinedOnlineStitcher: its own, with one)."""
        P = self.pipe
        f2, off1 = self._stage_a(P['lr'][p])
        P['f2'][p][0].copy_(f2[0])
        P['f2'][p][1].copy_(f2[1])
        P['off1'][p].copy_(off1)

    def _run_b(self, p):
        P = self.pipe
        f2, (hr1, hr2) = P['f2'][p], P['hr'][p]
        out = P['out'][p] if P['out_all'][p] is None else P['out_all'][p]
        self._stage_b(f2[0], f2[1], P['off1'][p], hr1, hr2, _DEFER if self._direct() else out)

    def _capture_pipe(self):
        """Warm both halves up eagerly on a copy of the state (parity 0 holds the current push's inputs), then capture each half for
        each buffer parity."""
        torch.cuda.synchronize(self.dev)
        P = self.pipe
        P['deferred'] = [None, None]

        def half_b(p):
            self._run_b(p)
            P['deferred'][p] = self._deferred              # (direct render: the second half left this parity's splines and footprints)
        steps = [lambda p=p, fn=fn: fn(p) for p in (0, 1) for fn in (self._run_a, half_b)]
        graphs, self.graph_nodes = _capture(self.dev, self._state(), lambda: (self._run_a(0), self._run_b(0)), steps,
                                            per_push=2)    # nodes of one push (both halves)
        P['ga'], P['gb'] = graphs[0::2], graphs[1::2]
        torch.cuda.synchronize(self.dev)

    def _enqueue(self, p, sa, sb, load=None):
        """One push's two halves behind the events that order them; -> the event behind the second half."""
        P = self.pipe
        cur = torch.cuda.current_stream(self.dev)
        ev_in = torch.cuda.Event()
        ev_in.record(cur)
        sa.wait_event(ev_in)
        sb.wait_event(ev_in)
        if P['eB'][p] is not None:
            sa.wait_event(P['eB'][p])                # the second half of push t - 2 has read this parity's hand-over buffers
        if load is not None:
            load()
        with torch.cuda.stream(sa):
            P['ga'][p].replay()
            ea = torch.cuda.Event()
            ea.record(sa)
        with torch.cuda.stream(sb):
            sb.wait_event(ea)
            P['gb'][p].replay()
            eb = torch.cuda.Event()
            eb.record(sb)
        P['eB'][p] = eb
        return eb

    def _pick_streams(self):
        """Choose the two streams by measurement.  Which hardware queue (and which of the command processor's pipes) a HIP stream
        lands on is the runtime's choice -- round-robin over GPU_MAX_HW_QUEUES by creation order, so it depends on every stream the
        process has made before -- and two streams that share a queue, or whose queues the firmware serves from one pipe, turn the
        0.89 ms three-view push into 1.3 - 4 ms (LAB_NOTES R6.5; priorities do not help).  The graphs replay on any stream, so: make
        PIPE_STREAM_CANDIDATES streams, replay the captured halves with the push's own event pattern on every pair, keep the fastest
        pair, restore the state the replays advanced.  ~0.1 s, once."""
        cands = [torch.cuda.Stream(self.dev) for _ in range(PIPE_STREAM_CANDIDATES)]
        cur = torch.cuda.current_stream(self.dev)
        best, self.stream_probe_ms = None, []
        with _kept(self._state()):
            for i, sa in enumerate(cands):
                for sb in cands[i + 1:]:
                    ms = None
                    for pushes in (2, PIPE_PROBE_PUSHES):        # the first pass pages the graphs onto the streams
                        self.pipe['eB'] = [None, None]
                        torch.cuda.synchronize(self.dev)
                        t0 = time.perf_counter()
                        prev = None
                        for t in range(pushes):
                            eb = self._enqueue(t & 1, sa, sb)
                            if prev is not None:
                                cur.wait_event(prev)
                            prev = eb
                        torch.cuda.synchronize(self.dev)
                        ms = (time.perf_counter() - t0) / pushes * 1e3
                    self.stream_probe_ms.append(round(ms, 4))
                    if best is None or ms < best[0]:
                        best = (ms, sa, sb)
            self.pipe['eB'] = [None, None]
        torch.cuda.synchronize(self.dev)
        self.pipe['sa'], self.pipe['sb'] = best[1], best[2]

    def _push_static(self, *frames, u8=None):
        # (push_u8: the uint8 frames take the HR frames' place, there are no LR frames)
        return self._push_pipelined(*(frames if u8 is None else u8 + (None,) * len(u8)))

    def _push_pipelined(self, *inputs):
        if self.pipe is None:
            self.pipe = dict(self._pipe_alloc(), sa=None, sb=None, ga=[None, None], gb=[None, None], eB=[None, None])
        if self._stale_trunk():
            # the twin trunk and ALL four graphs hold the old weights by address -- drain, recapture
            torch.cuda.synchronize(self.dev)
            self.trunk_pair = None
            self.pipe['ga'] = [None, None]
            self.pipe['gb'] = [None, None]
        P, p = self.pipe, self._t & 1
        if P['ga'][p] is None:
            # the capture warm-up reads parity 0's inputs: load them on the caller's stream first
            cur = torch.cuda.current_stream(self.dev)
            self._pipe_load(p, cur, cur, *inputs)
            self._capture_pipe()
            if P['sa'] is None:
                self._pick_streams()
        sa, sb = P['sa'], P['sb']
        eb = self._enqueue(p, sa, sb, lambda: self._pipe_load(p, sa, sb, *inputs))
        with torch.cuda.stream(sb):
            imgs = inputs[:len(inputs) // 2]             # the HR frames (push_u8: the uint8 frames)
            result = self._take(P['deferred'][p], P['out'][p], imgs, imgs[0].dtype == torch.uint8)
            eb = torch.cuda.Event()
            eb.record(sb)
        P['eB'][p] = eb
        prev, self._pending = self._pending, (eb, result)
        self._t += 1
        self.frames_in += 1
        return self._hand_out(prev)

    def _pipe_empty(self):
        return []

    def _hand_out(self, item):
        if item is None:
            return self._pipe_empty()
        cur = torch.cuda.current_stream(self.dev)
        cur.wait_event(item[0])
        for t in _tensors_of(item[1]):
            t.record_stream(cur)
        return item[1]

    def flush(self):
        """-> the result of the newest push (what `push` would have returned one push later), valid on the caller's stream."""
        item, self._pending = self._pending, None
        return self._hand_out(item)

    def flush_u8(self):
        """`flush()` for streams fed through push_u8: the last result as uint8 video frames."""
        return _to_u8(self.flush())

    def overflow_report(self):
        self._sync_state()
        return super().overflow_report()

    def _sync_state(self):
        """The pushes run on the pipe's own streams: all of them must have ended before the device state is read."""
        if getattr(self, 'pipe', None) is not None:
            torch.cuda.synchronize(self.dev)

    @staticmethod
    def _check_grow(grow):
        if grow not in ('never', 'refit'):
            raise ValueError("grow must be 'never' or 'refit' for a stitcher with two pushes in flight, got %r" % (grow,))


def _tensors_of(x):
    if torch.is_tensor(x):
        yield x
    elif isinstance(x, (list, tuple)):
        for y in x:
            yield from _tensors_of(y)


_BATCH_AND_NV12 = ('push_many', 'push_many_u8', 'push_nv12', 'push_many_nv12')


def _refusals(cls, plain, *names):
    """The entries `names` of the plain stitcher that its form with two pushes in flight does not offer: methods that refuse."""
    def refusal(name):
        def method(self, *frames, **kw):
            raise ValueError('%s has no %s: use %s.%s' % (cls, name, plain, name))
        return method
    return [refusal(name) for name in names]


class PipelinedOnlineStitcher(_TwoInFlight, OnlineStitcher):
    """OnlineStitcher with TWO pushes in flight (round 6; opt-in; see _TwoInFlight).  Frames bit-identical to OnlineStitcher
    (tests/test_gpu_round6.py), handed out one push late:
        st = PipelinedOnlineStitcher(nets, H, W)
        for pair in stream: for frame in st.push(*pair): ...
        for frame in st.flush(): ...
    0.64 ms per push = 1559 frames/s at 720p against 0.85 ms / 1171.  The canvas is fixed after the first window (grow='never';
    overflow is counted as in OnlineStitcher) or, with a viewport, re-fixed on the device (grow='refit').  LINEAR fusion renders inside the graphs (no direct LINEAR render: _TwoInFlight)."""

    def __init__(self, nets, height, width, canvas=None, margin=0.03, warp_mode='NORMAL', fusion_mode='AVERAGE', deterministic=False,
                 grow='never', viewport=None, zoom_limit=2.0, exposure=None, track_coverage=False):
        """grow: 'never', or 'refit' with a viewport (see OnlineStitcher and _TwoInFlight)."""
        _no_exposure('PipelinedOnlineStitcher', exposure)
        _no_coverage('PipelinedOnlineStitcher', track_coverage)
        self._check_grow(grow)
        OnlineStitcher.__init__(self, nets, height, width, canvas, margin, warp_mode, fusion_mode, use_graph=True, grow=grow,
                                meshes_only=False, deterministic=deterministic, viewport=viewport, zoom_limit=zoom_limit)
        self._pipe_init()

    push_many, push_many_u8, push_nv12, push_many_nv12 = _refusals('PipelinedOnlineStitcher', 'OnlineStitcher', *_BATCH_AND_NV12)

    def _pipe_alloc(self):
        out = [None, None] if self._direct() else [torch.empty((3, self.hc, self.wc), device=self.dev) for _ in range(2)]
        return dict(_TwoInFlight._pipe_alloc(self), out=out, out_all=[None, None])

    def _run_a(self, p):
        """The first half; both nets' features are handed over with ONE copy (a graph node less than the shared form's two)."""
        P = self.pipe
        f2, off1 = self._stage_a(P['lr'][p])
        P['f2'][p].copy_(f2)
        P['off1'][p].copy_(off1)


class MultiOnlineStitcher(_PairStep, _Stitcher):
    """S independent live video pairs advancing one frame per push as ONE batch (the sharding unit of the
    path -- independent streams -- inside one GPU).  A single stream at batch 1 is launch-bound (~150 small launches per
    pushed pair); S streams run the same launches on S-fold batches, so the aggregate frame rate grows almost linearly until
    the kernels fill the chip.  Every stream keeps its own sliding window, cached TemporalNet features and FIXED canvas
    (canvases may differ in size); per stream and push the arithmetic is the single-stream stitcher's (test_online_tra.py:
    284-392 with k = t) -- the networks see the S pairs as one batch, the render goes stream by stream.

        st = MultiOnlineStitcher(nets, 720, 1280, streams=8)
        frames = st.push(hr1, hr2, lr1, lr2)      # hr* [S,3,H,W], lr* [S,3,360,480] -> S lists of new frames [3,Hc_s,Wc_s]

    The first WINDOW pushes fill every stream's window through S single-stream stitchers (eager; they hold the streams' canvases
    afterwards); from then on the step -- _PairStep's, the code OnlineStitcher runs with S = 1 -- runs on their states joined along
    the stream axis and is captured into one HIP graph.  Results equal S
    single-stream stitchers up to the conv engine's launch-size-dependent kernel choice (Winograd / implicit GEMM / split-K are picked
    per launch size, so a batch of S sums in another order than S batches of one: motions differ by ~1e-5 px); within a batch every
    stream's result is independent of its neighbours bit for bit (tests/test_gpu_round4.py)."""

    def __init__(self, nets, height, width, streams, canvases=None, margin=0.03, warp_mode='NORMAL', fusion_mode='AVERAGE',
                 use_graph=True, grow='never', meshes_only=False, deterministic=False, chain=False, viewport=None, zoom_limit=2.0,
                 exposure=None, track_coverage=False):
        """grow: as OnlineStitcher -- 'never' counts the frames whose mesh left their stream's canvas (`clipped_frames`, per
        stream), 'recapture' re-fixes the canvases of the streams that come near an edge and captures the graph again, 'refit' (with
        a viewport) re-fixes each stream's box on the device inside the push's launches.
        viewport: (Hout, Wout), ONE for all streams: every stream's frames have that size, each on its own box (OnlineStitcher).
        meshes_only: no canvases, no render -- `push` returns the S streams' newly smoothed meshes (m1, m2) [S,k,7,9,2] (k = 7 on the
        7th push, then 1) or None; ThreeViewOnlineStitcher runs its two pair chains as such a batch of two and captures the graph
        itself (use_graph is ignored)."""
        _no_exposure(type(self).__name__, exposure)
        _no_coverage(type(self).__name__, track_coverage)
        _Stitcher.__init__(self, nets, height, width, margin, warp_mode, fusion_mode, use_graph, grow, meshes_only,
                           canvases=max(1, int(streams)), viewport=viewport, zoom_limit=zoom_limit)
        self.deterministic = bool(deterministic)      # geometry-only kernel policy: S batched streams == S single streams, bit for bit
        # chain: the S pairs are the neighbours of a chain of S + 1 views (pair s = views s, s + 1: ThreeViewOnlineStitcher's two
        # chains).  The steady-state step then takes the S + 1 LR frames once (static['lrc'] [S+1,3,360,480]) and every inner view
        # passes the trunks ONCE; the window-fill pushes go pair by pair as usual.  meshes_only streams only.
        self.chain = bool(chain)
        if self.chain and not meshes_only:
            raise ValueError('chain=True needs meshes_only=True')
        self.last_meshes = None
        self.S = int(streams)
        if self.S < 1:
            raise ValueError('streams must be >= 1')
        if canvases is not None and len(canvases) != self.S:
            raise ValueError('one canvas per stream')
        self.single = [OnlineStitcher(nets, height, width, None if canvases is None else canvases[s], margin, warp_mode,
                                      fusion_mode, use_graph=False, meshes_only=meshes_only, deterministic=deterministic,
                                      grow='refit' if grow == 'refit' else 'never', viewport=viewport, zoom_limit=zoom_limit)
                       for s in range(self.S)]                   # window fill; then the streams' canvases (watched and grown here)

    @property
    def canvas_sizes(self):
        """[(Hc, Wc)] per stream (None before the first window is complete)."""
        return [(s.hc, s.wc) for s in self.single]

    def _init_static(self):
        """The batched state from the S single-stream states (each has just completed its first window, in the same layout with
        S = 1): joined along the stream axis."""
        one = [s.static for s in self.single]
        if self.chain:                    # each view once: the first view of every pair, then the last pair's second
            prev_feat = torch.stack([o['prev_feat'][0] for o in one] + [one[-1]['prev_feat'][1]], 0).contiguous()
        else:                             # [2,1,...] per stream -> view-major [2 S,...]
            prev_feat = torch.stack([o['prev_feat'] for o in one], 1).flatten(0, 1)
        self._pair_static(prev_feat, torch.cat([o['pair_s'] for o in one], 2), torch.cat([o['ring'] for o in one], 1))
        st = self.static
        if not self.meshes_only:
            st['bboxes'] = torch.stack([s.bbox for s in self.single], 0).contiguous()        # [S,4] the streams' fixed canvases
            # the streams' watcher rows (their first windows are counted) go on as rows of one [S,4] state (ops.canvas_watch)
            rows = (torch.cat([s.watch.wi for s in self.single], 0).contiguous(),
                    torch.cat([s.watch.wf for s in self.single], 0).contiguous())
            if self.viewport is not None:         # the boxes are fitted already; grow='refit': the streams' fit states go on as rows too
                fit = None
                if self.grow == 'refit':
                    fit = (torch.cat([s.watch.fit.epoch for s in self.single], 0).contiguous(),
                           torch.cat([s.watch.fit.ext0 for s in self.single], 0).contiguous())
                self.watch.start(self.watch.fit_boxes(st['bboxes'], fit_state=fit or (None, None)), rows)
            else:
                self.watch.start(st['bboxes'].cpu(), rows)
            self._canvas_set = True
            self._alloc_outputs()
        for s in self.single:                     # the per-stream buffers and watchers are not needed any more (bbox / canvas stay)
            s.static = None
            s.watch = None

    def _alloc_outputs(self):
        st, S, d = self.static, self.S, self.dev
        sizes = self.canvas_sizes
        st['one_size'] = len(set(sizes)) == 1                   # equal canvas sizes: one render launch for all streams
        st['out_all'] = st['out'] = None
        if self._direct() and self.mode.ragged:                 # the push renders all streams into fresh tensors
            return
        if st['one_size']:
            st['out_all'] = torch.empty((S, 3) + sizes[0], device=d)
            st['out'] = [st['out_all'][s] for s in range(S)]
        else:
            st['out'] = [torch.empty((3, hc, wc), device=d) for hc, wc in sizes]

    # ------------------------------------------------------------------ canvas overflow (per stream)
    def overflow_report(self):
        """Synchronises.  -> one dict per stream (OnlineStitcher.overflow_report)."""
        return self.watch.report()

    def _regrown(self, rows):
        """grow='recapture': the watcher re-fixed the canvases of these streams -- new boxes, sizes and outputs (the graph is captured
        again)."""
        for s in rows:
            one = self.single[s]
            one.bbox = self.watch.boxes[s].to(self.dev)
            one.hc, one.wc = _canvas_size(self.watch.boxes[s])
            self.static['bboxes'][s].copy_(one.bbox)
        self._alloc_outputs()

    def _tail(self, m1, m2, hr1, hr2, out):
        """The S newest frames from the streams' smoothed windows m1, m2 [S,7,7,9,2]: rendered into `out` -- one tensor [S,3,Hc,Wc]
        where the canvases share a size, else one per stream -- or, out=_DEFER, left as self._deferred (one _Deferred over the S
        streams, or one per stream) for the push's own render."""
        if self.meshes_only:
            self.last_meshes = (m1[:, -1:], m2[:, -1:])                                       # [S,1,7,9,2]
            return
        st, e, defer = self.static, 126, out is _DEFER
        # every stream's newest smoothed mesh on its own canvas: control points and ONE batched TPS solve for the 2 S splines in one
        # launch (a solve is latency-bound, ~48 us whether it holds 2 systems or 16), the watcher on the footprint launch(es), then
        # the render stream by stream
        src, T = ops.stream_splines([m1[0, -1], m2[0, -1]], WINDOW * e, st['bboxes'], self.single[0].nrigid, self.h, self.w)
        mode, (hc, wc) = self.mode, self.canvas_sizes[0]
        watch, fit = mode.carry(src, self.watch.args(), self.watch.fit_args())
        if st['one_size'] or (defer and mode.ragged):
            # all streams render onto canvases of ONE size (e.g. the caller fixed them): the S current frames are a clip; or, whatever
            # the sizes, in one ragged render launched by the push (it has no footprint launch: hc, wc are not looked at)
            left = _Deferred(src, T, mode.footprints(src, T, hc, wc, watch, fit)[0], None)
            if defer:
                self._deferred = left
            else:
                mode.batch([hr1, hr2], left, hc, wc, out=out)
            return
        # canvases of several sizes: stream by stream, on the streams' own stitchers (defer: their records, kept here)
        left = [one._render_solved(None if defer else [hr1[s:s + 1], hr2[s:s + 1]], src[s], T[s], out=_DEFER if defer else out[s],
                                   watch=None if watch is None else self.watch.args(s),
                                   fit=None if watch is None else self.watch.fit_args(s)) for s, one in enumerate(self.single)]
        if defer:
            self._deferred = left

    def _render_direct(self, left, imgs, u8):
        """S canvases, two views."""
        if not u8:
            imgs = [f.reshape(self.S, 3, self.h, self.w) for f in imgs]
        return [[f] for f in self.mode.streams(list(imgs), left, self.canvas_sizes, u8)]

    @torch.no_grad()
    def push_u8(self, frames1, frames2):
        """One DECODED frame pair of every stream: uint8 [S,H,W,3] device tensors (cv2 layout) -> S lists of stitched video frames
        uint8 [Hc,Wc,3]; byte for byte ops.ingest_u8 -> push -> ops.canvas_to_u8 (see OnlineStitcher.push_u8)."""
        S = self.S
        if self.meshes_only or self.chain:
            raise ValueError('push_u8 renders frames of independent streams: not for meshes_only / chain stitchers')
        _check_u8('two uint8 [%d,H,W,3] tensors' % S, (frames1, frames2), (S, self.h, self.w, 3))
        return self._push_u8((frames1, frames2))

    @torch.no_grad()
    def push_nv12(self, frames1, frames2, out='bgr'):
        """One DECODED frame pair of every stream as NV12 surfaces: each view a device tensor [S,H*3/2,W] or a list of S surfaces
        [H*3/2,W], each with its own pitch -> S lists of stitched video frames, uint8 [Hc,Wc,3] (out='bgr'), byte for byte push_u8 of
        the converted frames, or NV12 [Hc*3/2,Wc] (out='nv12', even viewport), byte for byte ops.bgr_to_nv12 of those.  The 2 S
        surfaces are converted in one launch (ops.nv12_to_bgr), then push_u8 runs."""
        S = self.S
        surfs = _check_many_nv12(self, (frames1, frames2), out, 'push_nv12', count=S)
        bgr = ops.nv12_to_bgr(surfs[0] + surfs[1])
        outs = self.push_u8(bgr[:S], bgr[S:])
        return [_frames_to_nv12(per) for per in outs] if out == 'nv12' else outs

    @torch.no_grad()
    def push(self, hr1, hr2, lr1, lr2):
        """One frame pair of every stream: hr* [S,3,H,W] (0..255), lr* [S,3,360,480] ([-1,1]), device tensors.
        -> S lists of newly stitched frames (empty for the first 6 pushes, 7 frames each on the 7th, then one per push)."""
        S = self.S
        if lr1.shape[0] != S or lr2.shape[0] != S or (not self.meshes_only and (hr1.shape[0] != S or hr2.shape[0] != S)):
            raise ValueError('expected %d streams per push' % S)          # (meshes_only: hr1 / hr2 are not looked at, None will do)
        hr = [f for f in (hr1, hr2) if f is not None] if self.meshes_only else (hr1, hr2)
        _check_shapes('HR frames', hr, ((S, 3, self.h, self.w),))
        _check_shapes('LR frames', (lr1, lr2), ((S, 3, pipeline.LR_H, pipeline.LR_W),))
        with ops.deterministic(self.deterministic):
            return self._push(hr1, hr2, lr1, lr2)

    def _push(self, hr1, hr2, lr1, lr2):
        if self.static is not None:
            return self._push_static(hr1, hr2, lr1, lr2)
        hs = (lambda h, s: None) if self.meshes_only else (lambda h, s: h[s:s + 1])
        outs = [one.push(hs(hr1, s), hs(hr2, s), lr1[s:s + 1], lr2[s:s + 1]) for s, one in enumerate(self.single)]
        self.frames_in += 1
        if self.single[0].static is not None:      # every stream's first window is complete: switch to the batched step
            self._init_static()
        if self.meshes_only:
            if outs[0] is None:
                return None
            self.last_meshes = (torch.stack([o[0] for o in outs], 0), torch.stack([o[1] for o in outs], 0))   # [S,7,7,9,2]
            return self.last_meshes
        return outs


class PipelinedMultiOnlineStitcher(_TwoInFlight, MultiOnlineStitcher):
    """MultiOnlineStitcher (S live pairs advancing together) with TWO pushes in flight (round 6; opt-in; see _TwoInFlight): every
    stream's frames bit-identical to MultiOnlineStitcher's, handed out one push late:
        st = PipelinedMultiOnlineStitcher(nets, H, W, streams=8)
        for batch in source: per_stream = st.push(*batch)        # S lists: [] x 6, 7 frames, [] (one push of lag), then 1 frame each
        per_stream = st.flush()
    Canvases are fixed after the first window (grow='never') or, with a viewport, re-fixed on the device (grow='refit').  LINEAR
    fusion renders inside the graphs, stream by stream (no direct LINEAR render: _TwoInFlight)."""
    _U8_STEADY = False       # push_u8: ingest_u8 -> push -> canvas_to_u8

    def __init__(self, nets, height, width, streams, canvases=None, margin=0.03, warp_mode='NORMAL', fusion_mode='AVERAGE',
                 deterministic=False, grow='never', viewport=None, zoom_limit=2.0, exposure=None, track_coverage=False):
        """grow: 'never', or 'refit' with a viewport (see MultiOnlineStitcher and _TwoInFlight)."""
        _no_exposure('PipelinedMultiOnlineStitcher', exposure)
        _no_coverage('PipelinedMultiOnlineStitcher', track_coverage)
        self._check_grow(grow)
        MultiOnlineStitcher.__init__(self, nets, height, width, streams, canvases, margin, warp_mode, fusion_mode, use_graph=True,
                                     grow=grow, meshes_only=False, deterministic=deterministic, viewport=viewport,
                                     zoom_limit=zoom_limit)
        self._pipe_init()

    push_nv12, = _refusals('PipelinedMultiOnlineStitcher', 'MultiOnlineStitcher', 'push_nv12')

    def _pipe_alloc(self):
        P, S = _TwoInFlight._pipe_alloc(self), self.S
        if self.static['one_size']:
            P['out_all'] = [torch.empty_like(self.static['out_all']) for _ in range(2)]
            P['out'] = [[oa[s] for s in range(S)] for oa in P['out_all']]
        else:
            P['out_all'] = [None, None]
            P['out'] = [[torch.empty_like(o) for o in self.static['out']] for _ in range(2)]
        return P

    def _pipe_empty(self):
        return [[] for _ in range(self.S)]


class ThreeViewOnlineStitcher(_Stitcher):
    """Streaming form of the three-view script (test_online_tra_threeview.py:154-505, whose frame loops run the same sliding
    windows as the two-view script): one frame TRIPLE per push.  Two pair chains -- (view 1, view 2) and (view 2, view 3), run as ONE
    batch of two streams (`MultiOnlineStitcher(streams=2, meshes_only=True, chain=True)`: ring buffers, cached TemporalNet features,
    sliding SmoothNet windows; every launch serves both pairs, and the middle view passes the trunks ONCE per push: three image
    passes, not four) -- deliver the newest smoothed meshes; the composition (mesh alignment, middle plane, TPS re-projection of the
    outer views: threeview:345-420) and the three-image render (:421-505) run per frame on two FIXED boxes: the composition's "first
    canvas" (the box the reference takes over all frames of the aligned meshes: a normalisation frame, nothing is cropped by it) and
    the output canvas.  Both are fixed when the first window is complete (its 7 frames' boxes grown by `margin`) or given by the
    caller; with the offline boxes passed in the stream reproduces the offline frames (tests/test_gpu_round5.py, against the CPU
    oracle at 720p: tests/test_gpu_round6.py).  The steady state -- both chains, composition, render -- is ONE HIP graph.

        st = ThreeViewOnlineStitcher(nets, H, W)
        for frame in st.push(hr1, hr2, hr3, lr1, lr2, lr3): ...      # [], ..., 7 frames on the 7th push, then 1: [3,Hc,Wc] fp32

    Overflow of the fixed output canvas is watched as in OnlineStitcher (`clipped_frames`, `overflow_report()`); grow='recapture'
    re-fixes the OUTPUT canvas (and captures the graph again) when a mesh comes within half the margin of its edge.  `viewport` and
    grow='refit' as in OnlineStitcher, on the OUTPUT box only: the first canvas is a normalisation frame and stays as it is.
    `push_many` / `push_many_u8` take k consecutive triples per call (see OnlineStitcher.push_many)."""
    _MULTIBAND = True

    def __init__(self, nets, height, width, canvas=None, first_canvas=None, margin=0.03, warp_mode='NORMAL', fusion_mode='AVERAGE',
                 use_graph=True, grow='never', deterministic=False, viewport=None, zoom_limit=2.0, exposure=None, bands=None, seam=None,
                 seam_cell=None, seam_mu=None, seam_prior=None, track_coverage=False):
        """deterministic: every push under the conv engine's geometry-only kernel policy (ops.deterministic; as OnlineStitcher's):
        push_many's frames then equal single pushes' bit for bit.
        fusion_mode='MULTIBAND', bands= and seam= (seam_cell=, seam_mu=, seam_prior=): as OnlineStitcher's, over the three views at once
        (two seams, between the views that neighbour each other on the canvas).  track_coverage: as OnlineStitcher's, over the three
        views."""
        pipeline.seam_options(fusion_mode, seam, seam_cell, seam_mu, seam_prior)
        _no_exposure(type(self).__name__, exposure)
        # the two pair chains as a batch of two streams over the CHAIN of three views: every launch serves both pairs, view 2's
        # trunk features are computed once
        self.chains = MultiOnlineStitcher(nets, height, width, streams=2, margin=margin, warp_mode=warp_mode, fusion_mode=fusion_mode,
                                          use_graph=False, meshes_only=True, deterministic=deterministic, chain=True)
        _Stitcher.__init__(self, nets, height, width, margin, warp_mode, fusion_mode, use_graph, grow, viewport=viewport,
                           zoom_limit=zoom_limit, bands=bands,
                           seam=dict(seam=seam, seam_cell=seam_cell, seam_mu=seam_mu, seam_prior=seam_prior),
                           track_coverage=track_coverage)
        self.deterministic = bool(deterministic)
        box = lambda b: None if b is None else torch.tensor(b, dtype=torch.float32, device=self.dev)
        self.bbox, self.first_canvas = box(canvas), box(first_canvas)
        self.nrigid = get_norm_mesh(get_rigid_mesh(1, height, width, device=self.dev), height, width).contiguous()
        self.ring_hr = []

    # the twin trunk lives in the pair chains
    trunk_pair = property(lambda self: self.chains.trunk_pair, lambda self, v: setattr(self.chains, 'trunk_pair', v))
    trunk_versions = property(lambda self: self.chains.trunk_versions, lambda self, v: setattr(self.chains, 'trunk_versions', v))

    # ------------------------------------------------------------------ composition + render of k frames
    def _compose(self, m12, m23):
        """Pair meshes (m1, m2) [k,7,9,2] of both chains -> (mesh1, middle, mesh3) [1,k,7,9,2] in first-canvas pixels."""
        k = m12[0].shape[0]
        sh = lambda m: m.reshape(1, k, 7, 9, 2)
        return pipeline.three_view_compose(sh(m12[0]), sh(m12[1]), sh(m23[0]), sh(m23[1]), self.h, self.w,
                                           first_canvas=self.first_canvas)

    def _compose_render(self, m1, m2, imgs, out):
        """One steady-state triple from the chains' newest meshes m1, m2 [2,1,7,9,2] (stream 0 = pair (1,2), stream 1 = pair (2,3)):
        composition + the render's splines as ONE launch (FUSED_SPLINES; else the seven launches it replaces), then the render."""
        if FUSED_SPLINES:
            meshes, src, T = ops.three_view_splines(m1[0], m2[0], m1[1], m2[1], self.first_canvas, self.bbox, self.nrigid, self.h, self.w)
            splines = (src[0], T[0])
        else:
            meshes, splines = self._compose((m1[0], m2[0]), (m1[1], m2[1])), None
        self.last_composed = meshes
        return self._render(imgs, meshes, out=out, splines=splines)

    def _render(self, imgs, meshes, out=None, splines=None):
        """imgs: three [1,3,H,W]; meshes: (mesh1, middle, mesh3) [1,1,7,9,2] in first-canvas pixels -> [3,Hc,Wc].
        splines = (src [3,63,2], T [3,2,66]) from ops.three_view_splines: the steady-state push has them already, and the overflow
        watcher runs inside the footprint launch (or as a launch of its own when there is none)."""
        if splines is not None:
            return self._render_solved(imgs, splines[0], splines[1], out, watch=self.watch.args(), fit=self.watch.fit_args())
        if self.watch.fit is not None:       # grow='refit': the watcher runs in a launch that carries the refit, behind the box' last reader
            src = ops.stream_normalize_watch([m.contiguous() for m in meshes], 126, self.bbox, 0.0, 0.0)[0]
            T = ops.tps_solve_shared(src, self.nrigid)
            return self._render_solved(imgs, src, T, out, watch=self.watch.args(), fit=self.watch.fit_args())
        src = ops.stream_normalize_watch([m.contiguous() for m in meshes], 126, self.bbox, 0.0, 0.0,
                                         *self.watch.args())[0]                   # [3,63,2] on the output canvas, watcher updated
        return self._render_solved(imgs, src, ops.tps_solve_shared(src, self.nrigid), out)

    # ------------------------------------------------------------------ steady state
    def _state(self):
        return [self.chains.static[k] for k in _STATE] + [self.watch.wi, self.watch.wf] + self.watch.fit_state()

    def _stage_a(self, lr):
        """The first half of a push is the chains' (_PairStep._stage_a over the three views' frames [3,3,360,480])."""
        return self.chains._stage_a(lr)

    def _step_static(self):
        ch, hr = self.chains, self.static['hr']
        ch._step_static()
        m1, m2 = ch.last_meshes                                  # [2,1,7,9,2]: stream 0 = pair (1,2), stream 1 = pair (2,3)
        imgs = None if hr is None else [hr[0:1], hr[1:2], hr[2:3]]
        self._compose_render(m1, m2, imgs, _DEFER if self._direct() else self.static['out'])

    def _load(self, frames, u8):
        c, st = self.chains.static, self.static
        for k in range(3):                                                     # each view once: three frames, three LR frames
            if u8 is not None:                                                 # decoded uint8 frames: resized into the graph's LR inputs
                ops.ingest_u8(u8[k][None], pipeline.LR_H, pipeline.LR_W, want_hr=False, lr_out=c['lrc'][k:k + 1])
                continue
            h, l = frames[k], frames[3 + k]
            if not self._direct():                                                # (direct: the render reads the caller's frames)
                st['hr'][k:k + 1].copy_(h.reshape(st['hr'][k:k + 1].shape))
            c['lrc'][k:k + 1].copy_(l.reshape(c['lrc'][k:k + 1].shape))

    @torch.no_grad()
    def push_u8(self, img1, img2, img3):
        """One DECODED frame triple: uint8 [H,W,3] device tensors (cv2 layout) -> list of stitched video frames uint8 [Hc,Wc,3]; byte for
        byte ops.ingest_u8 -> push -> ops.canvas_to_u8 (see OnlineStitcher.push_u8)."""
        imgs = (img1, img2, img3)
        _check_u8('three uint8 [H,W,3] frames', imgs, (self.h, self.w, 3))
        return self._push_u8(imgs)

    def _lr_inputs(self):
        return [self.chains.static['lrc'][k:k + 1] for k in range(3)]

    @torch.no_grad()
    def push_nv12(self, img1, img2, img3, out='bgr'):
        """One DECODED frame triple: uint8 NV12 [H*3/2,W] device tensors -> list of stitched video frames, uint8 [Hc,Wc,3] (out='bgr')
        or NV12 [Hc*3/2,Wc] (out='nv12', even viewport); byte for byte push_u8 of the converted frames (see OnlineStitcher.push_nv12)."""
        imgs = (img1, img2, img3)
        _check_nv12(self, imgs, out)
        return self._push_nv12(imgs, out)

    @torch.no_grad()
    def push(self, hr1, hr2, hr3, lr1, lr2, lr3):
        """One frame triple: hr* [1,3,H,W] (0..255), lr* [1,3,360,480] ([-1,1]), device tensors.
        -> list of newly stitched frames (empty for the first 6 pushes, 7 frames on the 7th, then one per push)."""
        _check_shapes('HR frames', (hr1, hr2, hr3), ((1, 3, self.h, self.w), (3, self.h, self.w)))
        _check_shapes('LR frames', (lr1, lr2, lr3), _LR_SHAPES)
        with ops.deterministic(self.deterministic):
            return self._push(hr1, hr2, hr3, lr1, lr2, lr3)

    def _push(self, hr1, hr2, hr3, lr1, lr2, lr3):
        if self.static is not None:
            return self._push_static(hr1, hr2, hr3, lr1, lr2, lr3)
        sh = lambda t, c: t.reshape((1,) + tuple(c))
        got = self.chains.push(None, None, torch.cat((sh(lr1, lr1.shape[-3:]), sh(lr2, lr2.shape[-3:])), 0),
                               torch.cat((sh(lr2, lr2.shape[-3:]), sh(lr3, lr3.shape[-3:])), 0))
        self.ring_hr.append((hr1, hr2, hr3))
        self.frames_in += 1
        if got is None:
            return []
        m12, m23 = (got[0][0], got[1][0]), (got[0][1], got[1][1])                  # per chain: (m1, m2) [7,7,9,2]
        # first window complete: fix the first canvas and the output canvas, render its 7 frames, switch to the static step
        if self.first_canvas is None:
            k = m12[0].shape[0]
            shp = lambda m: m.reshape(1, k, 7, 9, 2)
            a1, a2, b1, b2, _ = ops.three_view_align(shp(m12[0]), shp(m12[1]), shp(m23[0]), shp(m23[1]), self.h, self.w)
            self.first_canvas = self._grown(ops.mesh_bbox([a1, a2, b1, b2], 0.0, 0.0))
        meshes = self._compose(m12, m23)                                           # three x [1,7,7,9,2]
        if self.bbox is None:
            self.bbox = self._grown(pipeline.canvas_bbox(meshes, self.h, self.w, prescaled=True))
        self._set_canvas()
        frames = [self._render(list(hr), [m[:, i:i + 1] for m in meshes]) for i, hr in enumerate(self.ring_hr)]
        self.ring_hr = []
        # (frame copies and an output canvas only where the graph renders: the direct render reads the caller's frames)
        self.static = {'out': None if self._direct() else torch.empty((3, self.hc, self.wc), device=self.dev),
                       'hr': None if self._direct() else torch.empty((3, 3, self.h, self.w), device=self.dev)}
        return frames

    # ------------------------------------------------------------------ k frame triples of the stream per call
    @torch.no_grad()
    def push_many(self, hr1, hr2, hr3, lr1, lr2, lr3):
        """k consecutive frame triples of the stream in one call, 1 <= k <= BATCH_MAX: hr* [k,3,H,W] (0..255), lr* [k,3,360,480]
        ([-1,1]), fp32 device tensors -> the newly stitched frames [3,Hc,Wc] in stream order: what k calls of `push` return, joined.
        Frames before the first window is complete go through `push` one at a time; the rest of the call runs as ONE batched step
        (per frame the arithmetic of `push`: both pair chains, composition, splines), captured into a HIP graph per batch size
        (BATCH_GRAPHS sizes kept); the render runs outside the graph on the caller's frames.  Canvas growth, reloads and
        interleaving with `push` / `push_u8` as in OnlineStitcher.push_many."""
        return self._push_many((hr1, hr2, hr3, lr1, lr2, lr3))

    @torch.no_grad()
    def push_many_u8(self, frames1, frames2, frames3):
        """k DECODED frame triples: uint8 [k,H,W,3] device tensors (cv2 layout) -> stitched video frames uint8 [Hc,Wc,3], byte for
        byte what k calls of `push_u8` return, joined (see push_many)."""
        return self._push_many_u8((frames1, frames2, frames3))

    @torch.no_grad()
    def push_many_nv12(self, frames1, frames2, frames3, out='bgr'):
        """k DECODED frame triples as NV12 surfaces ([k,H*3/2,W] tensors or lists of k surfaces) -> stitched video frames, uint8
        [Hc,Wc,3] (out='bgr') or NV12 [Hc*3/2,Wc] (out='nv12', even viewport): the 3 k surfaces converted in one launch, then
        push_many_u8 (see OnlineStitcher.push_many_nv12)."""
        return self._push_many_nv12((frames1, frames2, frames3), out)

    def _batch_buffers(self, k):
        return self.chains._batch_buffers(k)

    def _step_batch(self, B):
        """k consecutive steady-state frame triples from B['lr'] (capturable): the chains' k-frame step (_PairStep._batch_meshes
        over the three views), then composition + splines of the k frames in one launch; ends with the watcher and the footprints
        (B['deferred'])."""
        k = B['k']
        m1, m2 = self.chains._batch_meshes(B)                    # [nw,7,7,9,2]: pair (2,3)'s windows start WINDOW - 1 + k further
        c1 = WINDOW - 1 + k
        meshes, src, T = ops.three_view_splines(m1[0, -1], m2[0, -1], m1[c1, -1], m2[c1, -1], self.first_canvas, self.bbox,
                                                self.nrigid, self.h, self.w, frames=k, frame_stride=WINDOW * 126)
        self.last_composed = meshes
        self._leave_batch(B, src, T)


class PipelinedThreeViewOnlineStitcher(_TwoInFlight, ThreeViewOnlineStitcher):
    """ThreeViewOnlineStitcher with TWO pushes in flight (round 6; opt-in; see _TwoInFlight): the three views' trunks and the two
    pairs' stage-1 heads of triple t + 1 run beside triple t's regressor heads, smoothing, composition and three-image render.  Frames
    bit-identical to ThreeViewOnlineStitcher's, handed out one push late (`flush()` for the last); boxes fixed after the first window
    (grow='never') or, with a viewport, the output box re-fixed on the device (grow='refit').
    LINEAR fusion renders inside the graphs (no direct LINEAR render: _TwoInFlight)."""
    _U8_STEADY = False       # push_u8: ingest_u8 -> push -> canvas_to_u8

    def __init__(self, nets, height, width, canvas=None, first_canvas=None, margin=0.03, warp_mode='NORMAL', fusion_mode='AVERAGE',
                 grow='never', viewport=None, zoom_limit=2.0, exposure=None, track_coverage=False):
        """grow: 'never', or 'refit' with a viewport (see ThreeViewOnlineStitcher and _TwoInFlight)."""
        _no_exposure('PipelinedThreeViewOnlineStitcher', exposure)
        _no_coverage('PipelinedThreeViewOnlineStitcher', track_coverage)
        self._check_grow(grow)
        ThreeViewOnlineStitcher.__init__(self, nets, height, width, canvas, first_canvas, margin, warp_mode, fusion_mode,
                                         use_graph=True, grow=grow, viewport=viewport, zoom_limit=zoom_limit)
        self._pipe_init()

    push_many, push_many_u8, push_nv12, push_many_nv12 = _refusals('PipelinedThreeViewOnlineStitcher', 'ThreeViewOnlineStitcher',
                                                                   *_BATCH_AND_NV12)

    def _pipe_alloc(self):
        d = self.dev
        two = lambda *shape: [torch.empty(shape, device=d) for _ in range(2)]
        # (each view once: three LR frames, the trunks' features of three images; _TwoInFlight._run_a hands them over)
        return {'lr': two(3, 3, pipeline.LR_H, pipeline.LR_W), 'hr': [None, None] if self._direct() else two(3, 3, self.h, self.w),
                'f2': two(2, 3, pipeline.LR_H // 8, pipeline.LR_W // 8, 128), 'off1': two(2, 8),
                'out': [None, None] if self._direct() else two(3, self.hc, self.wc)}

    def _pipe_load(self, p, sa, sb, hr1, hr2, hr3, lr1, lr2, lr3):
        P = self.pipe
        for k, (h, l) in enumerate(((hr1, lr1), (hr2, lr2), (hr3, lr3))):
            with torch.cuda.stream(sa):
                P['lr'][p][k:k + 1].copy_(l.reshape(P['lr'][p][k:k + 1].shape))
            if not self._direct():              # (direct render: the second stream's render reads the caller's frames)
                with torch.cuda.stream(sb):
                    P['hr'][p][k:k + 1].copy_(h.reshape(P['hr'][p][k:k + 1].shape))
            h.record_stream(sb)
            l.record_stream(sa)

    def _run_b(self, p):
        P, ch = self.pipe, self.chains
        ch._stage_b(P['f2'][p][0], P['f2'][p][1], P['off1'][p], None, None, None)
        m1, m2 = ch.last_meshes                                  # [2,1,7,9,2]: stream 0 = pair (1,2), stream 1 = pair (2,3)
        hr = P['hr'][p]
        imgs = None if hr is None else [hr[0:1], hr[1:2], hr[2:3]]
        self._compose_render(m1, m2, imgs, _DEFER if self._direct() else P['out'][p])


class HostFrameStream:
    """The reference's frame loop end to end, one pair (or triple) at a time: decoded uint8 frames in HOST memory in, stitched uint8
    video frames in pinned host memory out (test_online_tra.py:250-278 reads and resizes a frame pair per iteration, :409-417 writes
    the fused frame) -- the PCIe copies of neighbouring pushes hidden behind the current push on three HIP streams:

        st = OnlineStitcher(nets, H, W)                            # or ThreeViewOnlineStitcher
        for frame in HostFrameStream(st).run(source):              # source yields (img1, img2[, img3]) uint8 [H,W,3] host frames
            writer.write(frame.numpy())                            # uint8 [Hc,Wc,3], pinned host memory

    The upload of pair t + prefetch is enqueued before pair t's launches (`stitcher.push_u8` on the compute stream: the resize feeds the
    graph, the render samples the uploaded uint8 frames and writes the uint8 frame); the download of push t - 1's frame is enqueued
    behind push t's launches and runs beside them.  Which copy may start is decided on the HOST, not by GPU-side waits of a copy stream
    on a compute event: with pushes of 0.8 ms those waits cost 0.13 - 0.17 ms each and serialised copies and compute (1.08 ms per push;
    `tools/diag_host_stream2.py`) -- the host waits for push t - 1's end event while push t is already queued, and a staging slot is reused
    only when its last reader is known to have ended.  Frames come out in order, `depth` frames late at most; a yielded tensor stays
    valid until `depth` more frames have been yielded.  Pinned (page-locked) input frames upload asynchronously; pageable ones (numpy
    arrays) work and stall the loop for their copy.

    frame_format='nv12': the source yields decoded NV12 frames uint8 [H*3/2,W] ([S,H*3/2,W] for S streams), half the bytes of packed
    BGR over the link.  They are uploaded as they are and converted on the device -- all views of a push in one launch
    (ops.nv12_to_bgr) on the compute stream -- in front of `push_u8` / `push_many_u8`: one route for every stitcher class, the
    pipelined ones included, and byte for byte the frames of a `push_nv12` loop.  out='nv12': ops.bgr_to_nv12 on the compute stream in
    front of the download, the pinned results are [Hc*3/2,Wc]; the stitcher needs an even viewport= (checked here).
    batch=k, 1 < k <= BATCH_MAX: consecutive items of the source are grouped k at a time (the last group may be shorter), each
    group uploaded into one staging slot [k,...] per view and pushed with `push_many_u8`; frames are still yielded one
    by one, in order.  Not for stitchers without push_many_u8 (Pipelined*, Multi*).  A group that completes the first window hands out
    up to k + 6 frames at once; the pinned ring holds 2 depth + batch + 8 frames (2 depth + 9 at batch 1), which keeps the promise
    above for such a burst: when a download overwrites the slot of frame i, at most `depth` frames wait undelivered, so frame
    i + depth + 1 has been yielded."""

    def __init__(self, stitcher, depth=4, prefetch=2, streams=None, batch=1, frame_format='bgr', out='bgr'):
        if frame_format not in ('bgr', 'nv12'):
            raise ValueError("HostFrameStream: frame_format must be 'bgr' or 'nv12', got %r" % (frame_format,))
        if out not in ('bgr', 'nv12'):
            raise ValueError("HostFrameStream: out must be 'bgr' or 'nv12', got %r" % (out,))
        if isinstance(batch, bool) or not isinstance(batch, int) or not 1 <= batch <= BATCH_MAX:
            raise ValueError('HostFrameStream: batch must be an int in 1..%d, got %r' % (BATCH_MAX, batch))
        if batch > 1 and (isinstance(stitcher, _TwoInFlight) or not hasattr(stitcher, 'push_many_u8')):
            raise ValueError('HostFrameStream(batch=%d) pushes with push_many_u8, which %s does not have: use batch=1'
                             % (batch, type(stitcher).__name__))
        if frame_format == 'nv12' and (stitcher.h % 2 or stitcher.w % 2):
            raise ValueError('NV12 frames have an even height and width: not for a %d x %d stitcher' % (stitcher.h, stitcher.w))
        if out == 'nv12':
            _even_viewport(stitcher, "HostFrameStream(out='nv12')")
        self.st, self.dev = stitcher, stitcher.dev
        self.depth, self.prefetch = int(depth), max(1, int(prefetch))
        self.batch, self.frame_format, self.out = batch, frame_format, out
        self.up, self.comp, self.down = streams if streams is not None else pipeline.io_streams(self.dev)
        self._in, self._free, self._k = None, None, 0          # ring of prefetch + 3 uploaded groups and the end events of their readers
        self._host, self._hk = None, 0                          # ring of 2 depth + batch + 8 pinned result frames (batch + 6 arrive at once)

    def _stage(self, group):
        """Upload one group of the source's items (batch=1: one item, into slots of the item's own shape; else up to `batch` items
        into slots [batch,...] per view) -> (slot, items in it, the upload's end event)."""
        st = self.st
        lead = (st.S,) if isinstance(st, MultiOnlineStitcher) else ()      # (S streams: every view's frames carry a stream axis)
        shape = lead + ((st.h // 2 * 3, st.w) if self.frame_format == 'nv12' else (st.h, st.w, 3))
        items = []
        for frames in group:
            src = [torch.from_numpy(f) if not torch.is_tensor(f) else f for f in frames]
            _check_shapes('uint8 NV12 frames' if self.frame_format == 'nv12' else 'uint8 frames', src, (shape,))   # before the upload
            if self.frame_format == 'nv12' and any(t.dtype != torch.uint8 for t in src):
                raise ValueError('NV12 frames are uint8, got %s' % [str(t.dtype) for t in src])
            items.append(src)
        views = len(items[0])
        if any(len(src) != views for src in items):
            raise ValueError('the items of the source differ in their number of views: %s' % [len(src) for src in items])
        slot = shape if self.batch == 1 else (self.batch,) + shape
        n = self.prefetch + 3
        if self._in is None or tuple(self._in[0][0].shape) != slot or len(self._in[0]) != views:
            torch.cuda.synchronize(self.dev)
            self._in = [[torch.empty(slot, dtype=torch.uint8, device=self.dev) for _ in range(views)] for _ in range(n)]
            self._free = [None] * n
        j = self._k % n
        self._k += 1
        if self._free[j] is not None:
            self._free[j].synchronize()          # host-side: the push that read this slot ended long ago (returns at once)
        with torch.cuda.stream(self.up):
            for i, src in enumerate(items):
                for dst, t in zip(self._in[j], src):
                    (dst if self.batch == 1 else dst[i]).copy_(t, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self.up)
        return j, len(items), ev

    def _push(self, j, m):
        """The push of staging slot j (m items) on the current stream -> its frames in the output format, a flat list."""
        frames = self._in[j] if self.batch == 1 else [f[:m] for f in self._in[j]]
        if self.frame_format == 'nv12':
            # all views' surfaces in one converter launch: [V * n, H, W, 3], view-major
            surfs = [s for f in frames for s in (f.unbind(0) if f.dim() == 3 else (f,))]
            bgr = ops.nv12_to_bgr(surfs)
            n = len(surfs) // len(frames)
            frames = [bgr[v * n:(v + 1) * n] if self._in[j][0].dim() == 3 else bgr[v] for v in range(len(frames))]
        outs = self.st.push_u8(*frames) if self.batch == 1 else self.st.push_many_u8(*frames)
        return self._format(outs)

    def _format(self, outs):
        outs = list(_tensors_of(outs))
        return _frames_to_nv12(outs) if self.out == 'nv12' else outs

    def _host_slot(self, shape):
        n = 2 * self.depth + self.batch + 8
        if self._host is None or tuple(self._host[0].shape) != tuple(shape):
            torch.cuda.synchronize(self.dev)
            self._host = [torch.empty(tuple(shape), dtype=torch.uint8).pin_memory() for _ in range(n)]
        h = self._host[self._hk % n]
        self._hk += 1
        return h

    def _download(self, item, results):
        """item = (end event of a push, its frames): wait for the push on the HOST, then copy its frames down on the download stream."""
        done, outs = item
        if not outs:
            return
        done.synchronize()
        with torch.cuda.stream(self.down):
            for o in outs:
                h = self._host_slot(o.shape)
                h.copy_(o, non_blocking=True)
                o.record_stream(self.down)
                e = torch.cuda.Event()
                e.record(self.down)
                results.append((e, h))

    @torch.no_grad()
    def run(self, source):
        from collections import deque
        import itertools
        items = iter(source)
        it = iter(lambda: tuple(itertools.islice(items, self.batch)), ())      # the source's items, `batch` at a time
        staged, results = deque(), deque()
        prev = None                                          # the previous push: (end event, frames still on the device)
        for _ in range(self.prefetch):
            nxt = next(it, None)
            if nxt is not None:
                staged.append(self._stage(nxt))
        while staged:
            j, m, ev = staged.popleft()
            nxt = next(it, None)
            if nxt is not None:
                staged.append(self._stage(nxt))              # a later group's upload is enqueued before this group's launches
            with torch.cuda.stream(self.comp):
                self.comp.wait_event(ev)
                outs = self._push(j, m)
                done = torch.cuda.Event()
                done.record(self.comp)
            self._free[j] = done
            if prev is not None:
                self._download(prev, results)                # push t - 1's frames go down while push t (queued above) computes
            prev = (done, outs)
            while len(results) > self.depth:
                e, h = results.popleft()
                e.synchronize()
                yield h
        if prev is not None:
            self._download(prev, results)
        if hasattr(self.st, 'flush_u8'):                     # a pipelined stitcher still holds its last push's frame
            with torch.cuda.stream(self.comp):
                outs = self._format(self.st.flush_u8())
                done = torch.cuda.Event()
                done.record(self.comp)
            self._download((done, outs), results)
        while results:
            e, h = results.popleft()
            e.synchronize()
            yield h
