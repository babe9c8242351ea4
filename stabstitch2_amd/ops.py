"""Thin tensor-level wrappers over the C ABI: allocate outputs with torch, launch on the current stream of the
device that owns the tensors, return device tensors.  These wrappers do no arithmetic of their own (the few
mesh-sized torch expressions of the path live in pipeline.py and are named there)."""
import collections
import os
import threading

import ctypes

import torch

from . import _hip as H
from . import _blend as B, _cover as CV, _mbwarp as W, _resample as RS, _seam as S, _smoothtail as ST, _surfaces as F


def _f(t):
    return t if (t.dtype == torch.float32 and t.is_contiguous()) else t.contiguous().float()


class _Built:
    """A device buffer built once by kernels on some stream (packed filters, cached inverses, constant meshes) and then
    read by launches on any stream: remembers the stream it was built on and an event behind the build, so that a first
    use from ANOTHER stream waits for it.  Building inside a HIP-graph capture is refused (the buffer would come from the
    graph's private pool and be replayed over by later eager launches): warm the path up eagerly before capturing."""
    __slots__ = ('value', 'stream', 'event', 'tag')

    def __init__(self, build, device, what, tag=None):
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('stabstitch2_amd: %s would be built inside a HIP-graph capture; run the path once eagerly '
                               '(warm-up) before capturing' % what)
        self.value = build()
        self.stream = torch.cuda.current_stream(device)
        self.event = torch.cuda.Event()
        self.event.record(self.stream)
        self.tag = tag

    def get(self, device):
        if self.event is None or torch.cuda.is_current_stream_capturing():
            # (inside a capture no event may be queried; the eager warm-up that built the buffer was submitted before the
            # capture began, and torch.cuda.graph synchronises the device on entry)
            return self.value
        cur = torch.cuda.current_stream(device)
        if cur != self.stream:
            if self.event.query():
                self.event = None               # finished long ago: nothing to wait for any more
            else:
                cur.wait_event(self.event)
        return self.value


# ------------------------------------------------------------------ layout
def nchw_to_nhwc(x, c_pad=None, out=None):
    n, c, h, w = x.shape
    c_pad = c_pad or ((c + 3) // 4) * 4
    if out is None:
        out = torch.empty((n, h, w, c_pad), device=x.device, dtype=torch.float32)
    assert tuple(out.shape) == (n, h, w, c_pad)
    H.call('ss_nchw_to_nhwc', H.dptr(_f(x)), H.dptr(out), n, c, h, w, c_pad, H.stream())
    return out


def nhwc_to_nchw(x, c=None):
    n, h, w, cs = x.shape
    c = c or cs
    out = torch.empty((n, c, h, w), device=x.device, dtype=torch.float32)
    H.call('ss_nhwc_to_nchw', H.dptr(x), H.dptr(out), n, c, h, w, cs, H.stream())
    return out


def adjacent(a, b):
    """Do two contiguous fp32 tensors lie back to back in memory (b right behind a)?  Then a launch over both reads them as one."""
    return (a.is_contiguous() and b.is_contiguous() and a.dtype == b.dtype == torch.float32 and a.device == b.device and
            b.data_ptr() == a.data_ptr() + a.numel() * 4)


def stem_input(xs):
    """NCHW frames (one tensor [n,3,h,w] or a list of them, laid back to back) -> [N,h,w+8,3]: the stem convolution's
    input layout (3 zero pixels left, 5 right; ss_nchw_to_nhwc3_padded)."""
    xs = xs if isinstance(xs, (list, tuple)) else [xs]
    total = sum(x.shape[0] for x in xs)
    h, w = xs[0].shape[2], xs[0].shape[3]
    buf = torch.empty((total, h, w + 8, 3), device=xs[0].device, dtype=torch.float32)
    o, i = 0, 0
    xs = [_f(x) for x in xs]
    while i < len(xs):
        x = xs[i]
        assert x.shape[1] == 3 and tuple(x.shape[2:]) == (h, w), x.shape
        n = x.shape[0]
        while i + 1 < len(xs) and adjacent(xs[i], xs[i + 1]):        # frames that lie back to back in memory: one launch
            i += 1
            assert xs[i].shape[1] == 3 and tuple(xs[i].shape[2:]) == (h, w), xs[i].shape
            n += xs[i].shape[0]
        H.call('ss_nchw_to_nhwc3_padded', H.dptr(x), H.dptr(buf[o:o + n]), n, h, w, H.stream())
        o += n
        i += 1
    return buf


def conv_stem(buf, wgt, bias=None, relu=True):
    """7x7 / stride 2 / pad 3 stem on `stem_input` frames.  wgt [cout,7,24] (layers.pack_stem3) -> [n,ho,wo,cout];
    wgt [g,cout,7,24] / bias [g,cout]: g stems reading the SAME frames in one launch -> [g,n,ho,wo,cout]."""
    n, h, wp, _ = buf.shape
    w = wp - 8
    grouped = wgt.dim() == 4
    g = wgt.shape[0] if grouped else 1
    cout = wgt.shape[-3]
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    out = torch.empty(((g, n, ho, wo, cout) if grouped else (n, ho, wo, cout)), device=buf.device, dtype=torch.float32)
    H.call('ss_conv_stem3', H.dptr(buf), H.dptr(wgt), H.dptr(bias, True), H.dptr(out), n, h, w, cout, int(relu), cout, g,
           0, wgt[0].numel() if grouped else 0, out[0].numel() if grouped else 0, H.stream())
    return out


# The whole stem (conv 7x7/2 + folded BN + ReLU + max-pool 3/2/1) in one kernel (csrc/stem.hip); SS_STEM_FUSED=0 runs the
# two-kernel path (ss_conv_stem3 + ss_maxpool_nhwc) for A/B measurements and the equivalence test.
STEM_FUSED = os.environ.get('SS_STEM_FUSED', '1') == '1'


def stem_pool_packed(wgt):
    """Filters of ss_stem_pool in its register layout, built on first use from a `layers.pack_stem3` tensor ([64,7,24], or
    [g*64,7,24] / [g,64,7,24] for g banks) and kept on it like the Winograd packs."""
    g = wgt.numel() // (64 * 168)
    assert wgt.numel() == g * 64 * 168, wgt.shape
    ent = getattr(wgt, '_stem_packed', None)
    tag = (wgt._version, wgt.data_ptr())
    if ent is None or ent.tag != tag:
        def build():
            pk = torch.empty(int(H.lib().ss_stem_pool_packed_floats(g)), device=wgt.device, dtype=torch.float32)
            H.call('ss_stem_pool_pack', H.dptr(wgt), H.dptr(pk), g, H.stream())
            return pk
        ent = _Built(build, wgt.device, 'the stem filter pack', tag)
        wgt._stem_packed = ent
    return ent.get(wgt.device), g


STEM_POOL_MAX_BYTES = 1 << 32        # bytes of row-packed input one ss_stem_pool launch can address


def stem_pool(buf, wgt, bias=None):
    """Conv2d(3,64,7,2,3) + folded BN + ReLU + MaxPool2d(3,2,1) on `stem_input` frames [n,h,w+8,3] in one kernel.
    wgt [g*64,7,24] (+ bias [g*64]): g filter banks reading the same frames -> [g,n,hp,wp,64] (each bank contiguous)."""
    n, h, wp8, _ = buf.shape
    w = wp8 - 8
    pk, g = stem_pool_packed(wgt)
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    hp, wp = (ho - 1) // 2 + 1, (wo - 1) // 2 + 1
    out = torch.empty((g, n, hp, wp, 64), device=buf.device, dtype=torch.float32)
    # one launch addresses its frames with 32-bit byte offsets (< 4 GiB of row-packed input, ss_stem_pool returns
    # SS_ERR_UNSUPPORTED beyond: ~2000 LR frames): larger batches go in several launches, each bank's slice written in place
    per = max(1, (STEM_POOL_MAX_BYTES - 1) // (h * wp8 * 12))
    for s in range(0, n, per):
        e = min(s + per, n)
        H.call('ss_stem_pool', H.dptr(buf[s:e]), H.dptr(pk), H.dptr(bias, True), H.dptr(out[0, s:e]), e - s, h, w, g,
               out[0].numel(), H.stream())
    return out


# ------------------------------------------------------------------ conv / pool / fc
# Deterministic kernel policy.  By default the conv engine picks a layer's kernel by LAUNCH SIZE as well as by
# geometry (F(4x4,3x3) needs >= 512 workgroups, F(2x2,3x3) >= 96, small launches are cut along K, FC layers with >= 16 rows run on
# the conv engine): a frame's last digits depend on how many frames share its launches (~1e-5 px between a 32-frame clip, two
# 16-frame passes and a stream).  Under the policy every choice follows the layer's GEOMETRY alone -- the Winograd rules as if the
# launch were large, no split-K (and no pool-in-reduction), FC always on the one-wave-per-neuron kernel -- so a frame's result is
# bit-identical whatever the batch: resident clip == chunked passes == streamed (tests/test_gpu_round6.py).  Price: small launches
# lose split-K's parallelism (batch-1 streaming ~1.6x slower, clips unchanged to ~1 %).
#     with ops.deterministic(): ...          or        pipeline.run_two_view(..., deterministic=True), OnlineStitcher(..., deterministic=True)
DETERMINISTIC = os.environ.get('SS_DETERMINISTIC', '0') == '1'        # the process default; `with ops.deterministic():` overrides it per THREAD
_PIN_IMAGES = 1 << 20
_policy_tls = threading.local()


def is_deterministic():
    """Is the geometry-only kernel policy in force for the calling thread (a `with ops.deterministic():` block, else the process
    default SS_DETERMINISTIC)?"""
    return getattr(_policy_tls, 'on', DETERMINISTIC)


class deterministic:
    """Context manager: the geometry-only kernel policy inside the block, for the calling thread (flag=False: leave the policy in
    force as it is)."""

    def __init__(self, flag=True):
        self.flag = bool(flag)
        self.old = None

    def __enter__(self):
        self.old = getattr(_policy_tls, 'on', None)
        if self.flag:
            _policy_tls.on = True
        return self

    def __exit__(self, *exc):
        if self.old is None:
            if hasattr(_policy_tls, 'on'):
                del _policy_tls.on
        else:
            _policy_tls.on = self.old
        return False


def conv_workspace(device, floats):
    """Split-K scratch for ONE launch, sized by ss_conv_workspace_need and taken from torch's caching allocator on the
    launch stream (stream-ordered: the block may be reused as soon as the reduce kernel behind it has been enqueued,
    and inside a HIP-graph capture it comes from the graph's own pool).  Most launches need none."""
    if floats <= 0:
        return None
    return torch.empty(int(floats), device=device, dtype=torch.float32)


def _conv_ws_need(n, t, h, w, c, cout, kt, kh, kw, stride, pt, ph, pw, groups):
    if is_deterministic():     # no workspace = no split-K (ss_conv_nhwc: "a NULL workspace disables splitting")
        return 0
    return int(H.lib().ss_conv_workspace_need(n, t, h, w, c, cout, kt, kh, kw, stride, pt, ph, pw, groups))


# Winograd F(2x2,3x3) for the stride-1 3x3 layers (csrc/wino.hip).  Host-level switch for A/B measurements and the
# parity tests; the dispatch rule itself is the library's (ss_conv_uses_winograd).
WINOGRAD = os.environ.get('SS_WINOGRAD', '1') == '1'


# Winograd F(4x4,3x3) (csrc/wino43.hip) where its 8 x 60-pixel tile blocks fit the map and the launch is deep enough:
# 'auto' = the rule below, '0' = never, '1' = wherever the kernel's geometry constraints hold (tests / A-B runs)
WINO43 = os.environ.get('SS_WINO43', 'auto')
WINO43_MIN_CIN = int(os.environ.get('SS_WINO43_MIN_CIN', '0'))      # 0 = the library's default (64)
WINO43_MIN_WGS = int(os.environ.get('SS_WINO43_MIN_WGS', '0'))      # 0 = the library's default (512); 1 pins the kernel choice
                                                                    # per layer whatever the batch (reproducible runs)


def _uses_wino43(kt, kh, kw, stride, pad, cin, cout, ho, wo, images, groups=1):
    """The library's rule (ss_conv_uses_wino43) behind the host switches: SS_WINO43 = 0 never, 1 wherever the kernel's geometry
    constraints hold (all thresholds 1), auto = the library's thresholds (or SS_WINO43_MIN_WGS / SS_WINO43_MIN_CIN)."""
    if WINO43 == '0' or not WINOGRAD or WINO_MATH != 'f32' or tuple(pad) != (0, 1, 1):
        return False
    forced = WINO43 == '1'
    return bool(H.lib().ss_conv_uses_wino43(int(kt), int(kh), int(kw), int(stride), int(cin), int(cout), int(ho), int(wo),
                                            int(images), int(groups), 1 if (forced or is_deterministic()) else WINO43_MIN_WGS,
                                            1 if forced else WINO43_MIN_CIN, 1 if forced else 0))


_WINO43_REFUSED = set()      # device indices whose first F(4x4,3x3) launch answered SS_ERR_DEVICE (no 144 KB of LDS per workgroup)


# F(4x4,3x3) with persistent workgroups (csrc/wino43.hip, conv_wino43p_kernel; bit-identical to the one-block-per-workgroup kernel).
# SS_WINO43_PERSIST=0 = the latter, for A/B runs; the knob is the library's process-wide, output-neutral ss_wino43_set_persistent.
WINO43_PERSIST = os.environ.get('SS_WINO43_PERSIST', '1') == '1'
_w43_persist_set = [None]


def _try_wino43(x, wgt, bias, res, relu, out):
    """ops.conv's use of the F(4x4,3x3) kernel.  The kernel needs 144 KB of LDS per workgroup; a device that cannot give it (not
    gfx950) makes the library answer SS_ERR_DEVICE at the first launch, nothing has been launched then: THAT device is remembered
    and its layers go to F(2x2,3x3) / the implicit GEMM from now on (other devices of the process keep the kernel).  A launch whose
    sizes the kernel cannot address (SS_ERR_UNSUPPORTED) falls through for this launch only.  -> the result, or None."""
    if x.device.index in _WINO43_REFUSED:
        return None
    if _w43_persist_set[0] != WINO43_PERSIST:
        H.lib().ss_wino43_set_persistent(int(WINO43_PERSIST))
        _w43_persist_set[0] = WINO43_PERSIST
    try:
        return conv_winograd43(x, wgt, bias, res, relu, out)
    except H.HipError as e:
        if e.code not in (-3, -4) or WINO43 == '1':          # (SS_WINO43=1 = "force it": then the error is the answer)
            raise
        if e.code == -4:
            _WINO43_REFUSED.add(x.device.index)
        return None


def _uses_winograd(kt, kh, kw, stride, pad, cin, cout, ho, wo, images):
    return bool(WINOGRAD and kt == 1 and tuple(pad) == (0, 1, 1) and
                H.lib().ss_conv_uses_winograd(int(kt), int(kh), int(kw), int(stride), int(cin), int(cout), int(ho),
                                              int(wo), _PIN_IMAGES if is_deterministic() else int(images)))


# which kernel the most recent ops.conv / ops.conv_grouped / ops.conv_winograd call launched ('wino' | 'igemm'): read by
# bench.ConvProbe for its executed-flop accounting (the dispatch is not re-derived there)
last_conv_path = None


def conv_executed_flop_ratio(kt, kh, kw, stride, cin, cout, out_shape):
    """Executed MFMA flop / direct-convolution flop of the launch the engine picks for this geometry (the library's own dispatch
    rules, as ops.conv / ops.conv_grouped apply them): 36/144 on F(4x4,3x3), 16/36 on F(2x2,3x3), else 1."""
    if len(out_shape) == 5 and kt == 1:          # grouped 2-D launch [g,n,ho,wo,c]
        groups, per_group = out_shape[0], out_shape[1]
    else:
        groups, per_group = 1, out_shape[0]
    ho, wo = out_shape[-3], out_shape[-2]
    if _uses_wino43(kt, kh, kw, stride, (0, 1, 1), cin, cout, ho, wo, per_group, groups):
        return 36.0 / 144.0
    return 16.0 / 36.0 if _uses_winograd(kt, kh, kw, stride, (0, 1, 1), cin, cout, ho, wo, per_group * groups) else 1.0


# Arithmetic of the Winograd layers' GEMMs.  'f32' (default): v_mfma_f32_32x32x2_f32.  'bf16x9' (opt-in, SS_WINO_MATH):
# every fp32 x fp32 product formed exactly from three bf16 slices per operand (nine slice products) on the bf16 matrix
# pipe, fp32 accumulation -- agrees with 'f32' to fp32 rounding, not bit for bit (csrc/wino.hip, SLICED).
WINO_MATH = os.environ.get('SS_WINO_MATH', 'f32')


def wino_packed(wgt, groups, sliced=False):
    """Transformed + packed filters of a 3x3 weight tensor ([cout,1,3,3,cin] or [g,cout,1,3,3,cin]), built on first use
    by ss_wino_pack / ss_wino_pack3 and kept on the tensor (prepared weights are rebuilt, hence re-packed, whenever a net
    is reloaded; an in-place edit of the tensor bumps its version counter and re-packs too)."""
    attr = '_wino_packed3' if sliced else '_wino_packed'
    ent = getattr(wgt, attr, None)
    tag = (wgt._version, wgt.data_ptr())
    if ent is None or ent.tag != tag:
        cout, cin = wgt.shape[-5], wgt.shape[-1]
        per = int((H.lib().ss_wino_packed3_floats if sliced else H.lib().ss_wino_packed_floats)(cout, cin))

        def build():
            pk = torch.empty((groups, per), device=wgt.device, dtype=torch.float32)
            H.call('ss_wino_pack3' if sliced else 'ss_wino_pack', H.dptr(wgt), H.dptr(pk), cout, cin, groups, H.stream())
            return pk
        ent = _Built(build, wgt.device, 'the Winograd filter pack', tag)
        setattr(wgt, attr, ent)
    return ent.get(wgt.device)


def wino43_packed(wgt, groups):
    """F(4x4,3x3) transformed + packed filters of a 3x3 weight tensor (kept on the tensor like wino_packed)."""
    ent = getattr(wgt, '_wino43_packed', None)
    tag = (wgt._version, wgt.data_ptr())
    if ent is None or ent.tag != tag:
        cout, cin = wgt.shape[-5], wgt.shape[-1]
        per = int(H.lib().ss_wino43_packed_floats(cout, cin))
        assert per > 0, (cout, cin)

        def build():
            pk = torch.empty((groups, per), device=wgt.device, dtype=torch.float32)
            H.call('ss_wino43_pack', H.dptr(wgt), H.dptr(pk), cout, cin, groups, H.stream())
            return pk
        ent = _Built(build, wgt.device, 'the F(4x4,3x3) filter pack', tag)
        setattr(wgt, '_wino43_packed', ent)
    return ent.get(wgt.device)


def conv_winograd43(x, wgt, bias=None, res=None, relu=False, out=None):
    """3x3 / stride 1 / pad 1 convolution on the fused Winograd F(4x4,3x3) kernel (csrc/wino43.hip), unconditionally.
    x nhwc [n,h,w,c] (or [g,n,h,w,c] with wgt [g,cout,1,3,3,c]); cin % 16 == 0, cout % 64 == 0."""
    grouped = wgt.dim() == 6
    g = wgt.shape[0] if grouped else 1
    cout, cin = wgt.shape[-5], wgt.shape[-1]
    assert tuple(wgt.shape[-4:-1]) == (1, 3, 3) and x.shape[-1] == cin, (wgt.shape, x.shape)
    shared = grouped and x.dim() == 4
    n, h, w = x.shape[-4], x.shape[-3], x.shape[-2]
    global last_conv_path
    last_conv_path = 'wino43'
    if out is None:
        out = torch.empty(((g, n, h, w, cout) if grouped else (n, h, w, cout)), device=x.device, dtype=torch.float32)
    pk = wino43_packed(wgt, g)
    H.call('ss_conv3x3_wino43_nhwc', H.dptr(x), H.dptr(pk), H.dptr(bias, True), H.dptr(res, True), H.dptr(out),
           n, h, w, cin, cout, int(relu), out.shape[-1], g, 0 if (shared or not grouped) else x[0].numel(),
           pk.shape[1], out[0].numel() if grouped else 0, H.stream())
    return out


POOL_FUSED = os.environ.get('SS_POOL_FUSED', '1') == '1'      # the regressors' 2x2 max-pool inside the Winograd epilogue


def conv_winograd(x, wgt, bias=None, res=None, relu=False, out=None, pool2=False):
    """3x3 / stride 1 / pad 1 convolution on the fused Winograd F(2x2,3x3) kernel, unconditionally (ops.conv applies the
    library's dispatch rule).  x nhwc [n,h,w,c] (or [g,n,h,w,c] with wgt [g,cout,1,3,3,c]: grouped launch).
    pool2: followed by MaxPool2d(2, 2) in the same kernel -> [.., h // 2, w // 2, cout] (no residual; fp32 MFMA arithmetic only)."""
    grouped = wgt.dim() == 6
    g = wgt.shape[0] if grouped else 1
    cout, cin = wgt.shape[-5], wgt.shape[-1]
    assert tuple(wgt.shape[-4:-1]) == (1, 3, 3) and x.shape[-1] == cin, (wgt.shape, x.shape)
    shared = grouped and x.dim() == 4
    n, h, w = x.shape[-4], x.shape[-3], x.shape[-2]
    sliced = WINO_MATH == 'bf16x9'
    global last_conv_path
    last_conv_path = 'wino'
    in_gs = 0 if (shared or not grouped) else x[0].numel()
    if pool2:
        assert res is None and not sliced
        if out is None:
            out = torch.empty(((g, n, h // 2, w // 2, cout) if grouped else (n, h // 2, w // 2, cout)), device=x.device,
                              dtype=torch.float32)
        pk = wino_packed(wgt, g, False)
        H.call('ss_conv3x3_wino_pool2_nhwc', H.dptr(x), H.dptr(pk), H.dptr(bias, True), H.dptr(out), n, h, w, cin, cout,
               int(relu), out.shape[-1], g, in_gs, pk.shape[1], out[0].numel() if grouped else 0, H.stream())
        return out
    if out is None:
        out = torch.empty(((g, n, h, w, cout) if grouped else (n, h, w, cout)), device=x.device, dtype=torch.float32)
    pk = wino_packed(wgt, g, sliced)
    H.call('ss_conv3x3_wino3_nhwc' if sliced else 'ss_conv3x3_wino_nhwc', H.dptr(x), H.dptr(pk), H.dptr(bias, True), H.dptr(res, True), H.dptr(out),
           n, h, w, cin, cout, int(relu), out.shape[-1], g, in_gs,
           pk.shape[1], out[0].numel() if grouped else 0, H.stream())
    return out


def pool2_is_fused(x, wgt, stride=1, pad=(0, 1, 1)):
    """Does ops.conv / ops.conv_grouped (pool2=True) run convolution + MaxPool2d(2, 2) as ONE kernel for these operands?
    (Where the Winograd kernel is dispatched; elsewhere the two are separate launches.)"""
    cout, kt, kh, kw, cin = wgt.shape[-5:]
    groups = wgt.shape[0] if wgt.dim() == 6 else 1
    n, h, w = x.shape[-4], x.shape[-3], x.shape[-2]
    return bool(POOL_FUSED and WINO_MATH != 'bf16x9' and _uses_winograd(kt, kh, kw, stride, pad, cin, cout, h, w, n * groups))


POOL_SPLITK = os.environ.get('SS_POOL_SPLITK', '1') == '1'      # the 2x2 max-pool inside the split-K reduction of small launches


def pool2_in_reduce(x, wgt, stride=1, pad=(0, 1, 1)):
    """Does a pool2 convolution of these operands that is NOT on the Winograd kernel take its pool inside the split-K reduction
    (one conv launch + one reduce launch), rather than in a max-pool launch of its own?"""
    cout, kt, kh, kw, cin = wgt.shape[-5:]
    groups = wgt.shape[0] if wgt.dim() == 6 else 1
    n, h, w, c = x.shape[-4:]
    return bool(POOL_SPLITK and kt == 1 and pad[0] == 0 and
                _conv_ws_need(n, 1, h, w, c, cout, 1, kh, kw, stride, 0, pad[1], pad[2], groups) > 0)


def _conv_pool2_splitk(x, wgt, bias, stride, pad, relu, groups):
    """conv + ReLU + MaxPool2d(2, 2) as ONE implicit-GEMM launch + its split-K reduction (which takes the pool), for launches
    that split along K; None when this launch would not (the caller then pools in a launch of its own).
    x [n,h,w,c] / [g,n,h,w,c] (or 4-D shared by g groups); wgt [cout,1,kh,kw,cin] / [g,cout,1,kh,kw,cin]."""
    if not POOL_SPLITK:
        return None
    grouped = wgt.dim() == 6
    cout, kt, kh, kw, cin = wgt.shape[-5:]
    n, h, w, c = x.shape[-4:]
    pt, ph, pw = pad
    if kt != 1 or pt != 0:
        return None
    need = _conv_ws_need(n, 1, h, w, c, cout, 1, kh, kw, stride, 0, ph, pw, groups)
    if need <= 0:
        return None
    ho = (h + 2 * ph - kh) // stride + 1
    wo = (w + 2 * pw - kw) // stride + 1
    shape = (groups, n, ho // 2, wo // 2, cout) if grouped else (n, ho // 2, wo // 2, cout)
    out = torch.empty(shape, device=x.device, dtype=torch.float32)
    ws = conv_workspace(x.device, need)
    shared = grouped and x.dim() == 4
    global last_conv_path
    last_conv_path = 'igemm'
    H.call('ss_conv_pool2_nhwc', H.dptr(x), H.dptr(wgt), H.dptr(bias, True), H.dptr(out), n, h, w, c, cout, kh, kw, stride, ph, pw,
           int(relu), cout, groups, 0 if (shared or not grouped) else x[0].numel(), wgt[0].numel() if grouped else 0,
           out[0].numel() if grouped else 0, H.dptr(ws), ws.numel(), H.stream())
    return out


def conv(x, wgt, bias=None, res=None, stride=1, pad=(0, 1, 1), relu=False, out=None, pool2=False):
    """x nhwc [n,h,w,c] or [n,t,h,w,c]; wgt [cout,kt,kh,kw,cin] (cin == x channels).
    pool2: the convolution is followed by MaxPool2d(2, 2) -- inside the Winograd kernel where that kernel runs, else as a
    second launch."""
    if pool2:
        assert x.dim() == 4 and out is None and res is None
        if pool2_is_fused(x, wgt, stride, pad):
            return conv_winograd(x, wgt, bias, None, relu, None, pool2=True)
        y = _conv_pool2_splitk(x, wgt, bias, stride, pad, relu, 1)
        return y if y is not None else maxpool(conv(x, wgt, bias, None, stride, pad, relu), 2, 2, 0)
    five = x.dim() == 5
    if five:
        n, t, h, w, c = x.shape
    else:
        n, h, w, c = x.shape
        t = 1
    cout, kt, kh, kw, cin = wgt.shape
    assert cin == c, (cin, c)
    pt, ph, pw = pad
    to = t + 2 * pt - kt + 1
    ho = (h + 2 * ph - kh) // stride + 1
    wo = (w + 2 * pw - kw) // stride + 1
    if out is None:
        shape = (n, to, ho, wo, cout) if five else (n, ho, wo, cout)
        out = torch.empty(shape, device=x.device, dtype=torch.float32)
    if not five and _uses_wino43(kt, kh, kw, stride, pad, c, cout, ho, wo, n):
        y = _try_wino43(x, wgt, bias, res, relu, out)
        if y is not None:
            return y
    if not five and _uses_winograd(kt, kh, kw, stride, pad, c, cout, ho, wo, n):
        return conv_winograd(x, wgt, bias, res, relu, out)
    global last_conv_path
    last_conv_path = 'igemm'
    ws = conv_workspace(x.device, _conv_ws_need(n, t, h, w, c, cout, kt, kh, kw, stride, pt, ph, pw, 1))
    H.call('ss_conv_nhwc', H.dptr(x), H.dptr(wgt), H.dptr(bias, True), H.dptr(res, True), H.dptr(out),
           n, t, h, w, c, cout, kt, kh, kw, stride, pt, ph, pw, int(relu), out.shape[-1],
           1, 0, 0, 0, H.dptr(ws, True), 0 if ws is None else ws.numel(), H.stream())
    return out


def conv_grouped(x, wgt, bias=None, res=None, stride=1, pad=(0, 1, 1), relu=False, pool2=False, out=None):
    """G independent convolutions of identical geometry in ONE launch: x [G,n,h,w,c], wgt [G,cout,kt,kh,kw,cin],
    bias [G,cout] | None, res [G,n,ho,wo,cout] | None -> [G,n,ho,wo,cout]; a 4-D x [n,h,w,c] is shared by all groups.  Used where the reference runs twin
    sub-networks (regressNet2 ref/tgt, the SpatialNet and TemporalNet trunks in streaming mode)."""
    g2, cout, kt, kh, kw, cin = wgt.shape
    shared = x.dim() == 4                # one input read by every group (group stride 0)
    if shared:
        n, h, w, c = x.shape
        g = g2
    else:
        g, n, h, w, c = x.shape
    assert g2 == g and cin == c and kt == 1, (wgt.shape, x.shape)
    pt, ph, pw = pad
    ho = (h + 2 * ph - kh) // stride + 1
    wo = (w + 2 * pw - kw) // stride + 1
    if pool2:      # conv + MaxPool2d(2, 2): one kernel on the Winograd path, two launches otherwise -> [g,n,ho//2,wo//2,cout]
        assert res is None and out is None
        if pool2_is_fused(x, wgt, stride, pad):
            return conv_winograd(x, wgt, bias, None, relu, None, pool2=True)
        y = _conv_pool2_splitk(x, wgt, bias, stride, pad, relu, g)
        if y is not None:
            return y
        y = conv_grouped(x, wgt, bias, None, stride, pad, relu)
        return maxpool(y.view(g * n, ho, wo, cout), 2, 2, 0).view(g, n, ho // 2, wo // 2, cout)
    if out is None:
        out = torch.empty((g, n, ho, wo, cout), device=x.device, dtype=torch.float32)
    assert tuple(out.shape) == (g, n, ho, wo, cout) and out.is_contiguous()
    if _uses_wino43(kt, kh, kw, stride, pad, c, cout, ho, wo, n, g):
        y = _try_wino43(x, wgt, bias, res, relu, out)
        if y is not None:
            return y
    if _uses_winograd(kt, kh, kw, stride, pad, c, cout, ho, wo, n * g):
        return conv_winograd(x, wgt, bias, res, relu, out)
    global last_conv_path
    last_conv_path = 'igemm'
    ws = conv_workspace(x.device, _conv_ws_need(n, 1, h, w, c, cout, kt, kh, kw, stride, pt, ph, pw, g))
    H.call('ss_conv_nhwc', H.dptr(x), H.dptr(wgt), H.dptr(bias, True), H.dptr(res, True), H.dptr(out),
           n, 1, h, w, c, cout, kt, kh, kw, stride, pt, ph, pw, int(relu), cout,
           g, 0 if shared else x[0].numel(), wgt[0].numel(), out[0].numel(), H.dptr(ws, True),
           0 if ws is None else ws.numel(), H.stream())
    return out


def maxpool(x, k, stride, pad=0, out=None):
    n, h, w, c = x.shape
    ho = (h + 2 * pad - k) // stride + 1
    wo = (w + 2 * pad - k) // stride + 1
    if out is None:
        out = torch.empty((n, ho, wo, c), device=x.device, dtype=torch.float32)
    H.call('ss_maxpool_nhwc', H.dptr(x), H.dptr(out), n, h, w, c, k, stride, pad, H.stream())
    return out


def maxpool_split(x, k, stride, pad, out0, out1):
    """Pool x [n,h,w,c]; channels [0,c/2) -> out0, [c/2,c) -> out1 (each [n,ho,wo,c/2], preallocated)."""
    n, h, w, c = x.shape
    H.call('ss_maxpool_nhwc_split', H.dptr(x), H.dptr(out0), H.dptr(out1), n, h, w, c, k, stride, pad, H.stream())
    return out0, out1


def linear(x, w, b=None, relu=False, out=None):
    m, k = x.shape
    nout = w.shape[0]
    assert w.shape[1] == k
    if out is None:
        out = torch.empty((m, nout), device=x.device, dtype=torch.float32)
    assert out.numel() == m * nout
    H.call('ss_linear', H.dptr(x), H.dptr(w), H.dptr(b, True), H.dptr(out), m, k, nout, int(relu), H.stream())
    return out


# ------------------------------------------------------------------ correlation
def linear_grouped(x, w, b=None, relu=False, outs=None):
    """G fully connected layers of identical shape in one launch: x [G,m,k], w [G,nout,k], b [G,nout] | None ->
    [G,m,nout]; outs: list of G contiguous destination tensors of m * nout floats each (any addresses) instead."""
    g, m, k = x.shape
    nout = w.shape[1]
    assert w.shape[0] == g and w.shape[2] == k and x.is_contiguous()
    res = None
    if outs is None:
        res = torch.empty((g, m, nout), device=x.device, dtype=torch.float32)
        outs = [res[i] for i in range(g)]
    assert len(outs) == g and all(o.numel() == m * nout for o in outs)
    arr = H.ptr_array(outs)
    H.call('ss_linear_grouped', H.dptr(x), x[0].numel(), H.dptr(w), H.dptr(b, True), arr, g, m, k, nout, int(relu), H.stream())
    return res


def ccl(f1, f2, scale=10.0, want_nchw=True, want_nhwc4=True):
    """f1, f2 nhwc [n,h,w,c] -> (flow NCHW [n,2,h,w] | None, flow nhwc4 [n,h,w,4] | None)."""
    n, h, w, c = f1.shape
    ws = torch.empty(int(H.lib().ss_ccl_workspace_floats(n, h, w, c)), device=f1.device, dtype=torch.float32)
    a = torch.empty((n, 2, h, w), device=f1.device, dtype=torch.float32) if want_nchw else None
    b = torch.empty((n, h, w, 4), device=f1.device, dtype=torch.float32) if want_nhwc4 else None
    H.call('ss_ccl', H.dptr(f1), H.dptr(f2), H.dptr(a, True), H.dptr(b, True), n, h, w, c, float(scale),
           H.dptr(ws), H.stream())
    return a, b


def l2norm(x):
    """F.normalize(x, p=2, dim=channels) on an nhwc tensor."""
    out = torch.empty_like(x)
    H.call('ss_l2norm_nhwc', H.dptr(x), H.dptr(out), x.numel() // x.shape[-1], x.shape[-1], H.stream())
    return out


def cost_volume(x1, x2, r, out=None, chain=0, n=None, split=0, shift=0):
    """nhwc in -> nhwc [n,h,w,pad4((2r+1)^2)] (padding channels are zero).
    chain = S > 0: x1 / x2 hold the S + 1 views of a chain of S pairs ONCE; -> the 2 S volumes [first views | second views] of the
    pairs (ss_cost_volume_shifted), equal to the volumes of cat(x[:S], x[1:]).
    n volumes with split / shift (ss_cost_volume_shifted): volume b reads image b + (b >= split ? shift : 0) of x1 and x2 (k frames of
    one stream: x1 = the [2 views][k + 1] features, x2 the same one image further, split = k, shift = 1)."""
    d = (2 * r + 1) ** 2
    cs = ((d + 3) // 4) * 4
    images, h, w, c = x1.shape
    shifted = n is not None
    if chain:
        assert not shifted and images == chain + 1 and tuple(x2.shape) == tuple(x1.shape)
        n, split, shift = 2 * chain, chain, 1 - chain
    elif shifted:
        assert 0 <= split and 0 <= split + shift and tuple(x2.shape) == tuple(x1.shape)
        assert max(min(split, n) - 1, n - 1 + (shift if n > split else 0)) < images, 'cost_volume: a shifted volume reads past the inputs'
    else:
        n = images
    if out is None:
        out = torch.empty((n, h, w, cs), device=x1.device, dtype=torch.float32)
    assert tuple(out.shape) == (n, h, w, cs)
    if chain or shifted:
        H.call('ss_cost_volume_shifted', H.dptr(x1), H.dptr(x2), H.dptr(out), n, h, w, c, r, cs, split, shift, H.stream())
    else:
        H.call('ss_cost_volume', H.dptr(x1), H.dptr(x2), H.dptr(out), n, h, w, c, r, cs, H.stream())
    return out


def cost_volume_chain_frames(x, r, out=None):
    """x [V,k+1,h,w,c] contiguous: the features of V >= 2 views of a chain over k frames, slot 0 = each view's previous frame ->
    [2,V-1,k,h,w,pad4((2r+1)^2)]: the volumes [first views | second views] of the V - 1 pairs, volume (hh, s, j) = cost_volume of
    (x[s + hh, j], x[s + hh, j + 1]), in ONE launch (ss_cost_volume_chain_frames)."""
    views, k1, h, w, c = x.shape
    k = k1 - 1
    cs = ((((2 * r + 1) ** 2) + 3) // 4) * 4
    assert x.is_contiguous() and x.dtype == torch.float32
    shape = (2, views - 1, k, h, w, cs)
    if out is None:
        out = torch.empty(shape, device=x.device, dtype=torch.float32)
    assert tuple(out.shape) == shape and out.is_contiguous()
    H.call('ss_cost_volume_chain_frames', H.dptr(x), H.dptr(out), views, k, h, w, c, r, cs, H.stream())
    return out


def cost_volume_bidir(x1, x2, r, out=None):
    """Both directions in one launch: nhwc in -> [2,n,h,w,pad4((2r+1)^2)] = (cost_volume(x1, x2), cost_volume(x2, x1))."""
    n, h, w, c = x1.shape
    cs = (((2 * r + 1) ** 2 + 3) // 4) * 4
    if out is None:
        out = torch.empty((2, n, h, w, cs), device=x1.device, dtype=torch.float32)
    assert tuple(out.shape) == (2, n, h, w, cs) and tuple(x2.shape) == tuple(x1.shape)
    H.call('ss_cost_volume_bidir', H.dptr(x1), H.dptr(x2), H.dptr(out), n, h, w, c, r, cs, H.stream())
    return out


# ------------------------------------------------------------------ geometry
def tensor_dlt(src, dst):
    n = src.shape[0]
    out = torch.empty((n, 3, 3), device=src.device, dtype=torch.float32)
    H.call('ss_tensor_dlt', H.dptr(_f(src)), H.dptr(_f(dst)), H.dptr(out), n, H.stream())
    return out


def spatial_decompose(offset8, img_h, img_w):
    n = offset8.shape[0]
    ab = torch.empty((2, n, 3, 3), device=offset8.device, dtype=torch.float32)      # (back to back: homo_warp_pair reads them as one)
    a, b = ab[0], ab[1]
    H.call('ss_spatial_decompose', H.dptr(offset8), H.dptr(a), H.dptr(b), n, float(img_h), float(img_w), H.stream())
    return a, b


def spatial_meshes(offset8, off_ref, off_tgt, img_h, img_w, out=None):
    n = offset8.shape[0]
    if out is not None:
        m1, m2 = out
        assert m1.numel() == n * 126 and m2.numel() == n * 126
    else:
        m1 = torch.empty((n, 7, 9, 2), device=offset8.device, dtype=torch.float32)
        m2 = torch.empty((n, 7, 9, 2), device=offset8.device, dtype=torch.float32)
    H.call('ss_spatial_meshes', H.dptr(offset8), H.dptr(off_ref), H.dptr(off_tgt), H.dptr(m1), H.dptr(m2), n,
           float(img_h), float(img_w), H.stream())
    return m1, m2


def homo_warp_nhwc(x, theta, out_h, out_w):
    n, h, w, c = x.shape
    out = torch.empty((n, out_h, out_w, c), device=x.device, dtype=torch.float32)
    H.call('ss_homo_warp_nhwc', H.dptr(x), H.dptr(theta), H.dptr(out), n, h, w, c, out_h, out_w, H.stream())
    return out


def homo_warp_pair(x1, x2, th1, th2, out_h, out_w):
    """(homo_warp_nhwc(x1, th1), homo_warp_nhwc(x2, th2)) -- as ONE launch when both the maps and the transforms lie back to back in
    memory (the two views' halves of a trunk output, spatial_decompose's pair), else two."""
    if adjacent(x1, x2) and adjacent(th1, th2) and x1.shape[1:] == x2.shape[1:]:
        n1, n2 = x1.shape[0], x2.shape[0]
        out = torch.empty((n1 + n2, out_h, out_w, x1.shape[3]), device=x1.device, dtype=torch.float32)
        H.call('ss_homo_warp_nhwc', H.dptr(x1), H.dptr(th1), H.dptr(out), n1 + n2, x1.shape[1], x1.shape[2], x1.shape[3], out_h, out_w,
               H.stream())
        return out[:n1], out[n1:]
    if (adjacent(th1, th2) and x1.shape == x2.shape and x1.is_contiguous() and x2.is_contiguous() and x1.device == x2.device):
        # views of ONE tensor a whole number of images apart (a chain of pairs: views [0:n] and [1:n+1]): still one launch
        img = x1[0].numel() * 4
        d = x2.data_ptr() - x1.data_ptr()
        if 0 <= d <= x1.numel() * 4 and d % img == 0 and x1.untyped_storage().data_ptr() == x2.untyped_storage().data_ptr():
            n = x1.shape[0]
            out = torch.empty((2 * n, out_h, out_w, x1.shape[3]), device=x1.device, dtype=torch.float32)
            H.call('ss_homo_warp_pair_nhwc', H.dptr(x1), H.dptr(x2), H.dptr(th1), H.dptr(out), n, x1.shape[1], x1.shape[2], x1.shape[3],
                   out_h, out_w, H.stream())
            return out[:n], out[n:]
    return homo_warp_nhwc(x1, th1, out_h, out_w), homo_warp_nhwc(x2, th2, out_h, out_w)


def homo_warp_nchw(x, theta, out_h, out_w):
    n, c, h, w = x.shape
    out = torch.empty((n, c, out_h, out_w), device=x.device, dtype=torch.float32)
    H.call('ss_homo_warp_nchw', H.dptr(x), H.dptr(theta), H.dptr(out), n, c, h, w, out_h, out_w, H.stream())
    return out


def tps_solve(source, target):
    n = source.shape[0]
    T = torch.empty((n, 2, 66), device=source.device, dtype=torch.float32)
    H.call('ss_tps_solve', H.dptr(_f(source)), H.dptr(_f(target)), H.dptr(T), n, H.stream())
    return T


def tps_solve_shared(source, target):
    """n control-point sets [n,63,2] against ONE target [63,2] / [1,63,2] -> T [n,2,66] (no broadcast copy)."""
    n = source.shape[0]
    assert target.numel() == 126
    T = torch.empty((n, 2, 66), device=source.device, dtype=torch.float32)
    H.call('ss_tps_solve_shared_target', H.dptr(_f(source)), H.dptr(_f(target)), H.dptr(T), n, H.stream())
    return T


def tps_points(point, source, T):
    n, q, _ = point.shape
    out = torch.empty((n, q, 2), device=point.device, dtype=torch.float32)
    H.call('ss_tps_points', H.dptr(_f(point)), H.dptr(_f(source)), H.dptr(T), H.dptr(out), n, q, H.stream())
    return out


_rigid_winv = {}
RIGID_INVERSE_CACHE = True      # host switch for A/B runs and the equivalence test


def rigid_winv(img_h, img_w, device):
    """fp64 W^-1 of the TPS system whose control points are the normalised RIGID mesh of an (img_h, img_w) image: a
    constant of the tsmotion composition, computed once per (size, device) by ss_tps_inverse."""
    device = torch.device(device)
    key = (int(img_h), int(img_w), str(device))
    ent = _rigid_winv.get(key)
    if ent is None:
        def build():
            xs = torch.linspace(0.0, float(img_w), 9)
            ys = torch.linspace(0.0, float(img_h), 7)
            m = torch.stack((xs.view(1, -1).expand(7, -1), ys.view(-1, 1).expand(-1, 9)), 2).reshape(63, 2)
            src = torch.stack((m[:, 0] * 2. / float(img_w) - 1., m[:, 1] * 2. / float(img_h) - 1.), 1).contiguous().to(device)
            w = torch.empty((66, 66), device=device, dtype=torch.float64)
            H.call('ss_tps_inverse', H.dptr(src), H.dptr(w, dtype=torch.float64), H.stream())
            return w
        ent = _Built(build, device, 'the cached rigid-mesh TPS inverse')
        _rigid_winv[key] = ent
    return ent.get(device)


def tsmotion(smotion, tmotion, img_h=360, img_w=480, out=None, lag=1):
    """smotion, tmotion [n,7,9,2] -> (smesh, tsmotion) [n,7,9,2] (out: the two preallocated result tensors).
    lag: frame k pairs with frame k - lag (S interleaved streams advancing together: lag = S)."""
    n = smotion.shape[0]
    ws = torch.empty(int(H.lib().ss_tsmotion_workspace_floats(n)), device=smotion.device, dtype=torch.float32)
    if out is None:
        smesh = torch.empty((n, 7, 9, 2), device=smotion.device, dtype=torch.float32)
        tsm = torch.empty((n, 7, 9, 2), device=smotion.device, dtype=torch.float32)
    else:
        smesh, tsm = out
        assert smesh.numel() == n * 126 and tsm.numel() == n * 126 and smesh.is_contiguous() and tsm.is_contiguous()
    winv = rigid_winv(img_h, img_w, smotion.device) if RIGID_INVERSE_CACHE else None
    H.call('ss_tsmotion_lag', H.dptr(_f(smotion)), H.dptr(_f(tmotion)), H.dptr(smesh), H.dptr(tsm), n, int(lag), float(img_h),
           float(img_w), H.dptr(winv, True, dtype=torch.float64), H.dptr(ws), H.stream())
    return smesh, tsm


def window_push(ring, src, src_off, state=None, blocks=0, block=0, stride=0, delta=0, per=1):
    """Streaming mode: ring [R,W,...] (contiguous, fixed address) drops slot 0 of every ring and appends the row at
    src.flatten()[src_off[r]:][:E]; optionally moves `blocks` blocks of `block` floats inside `state` (block b at b * stride
    <- the floats `delta` further) in the same launch (ss_window_push).
    per > 1: ring [G, per, W, ...] -- G ring kinds x `per` streams, ring (g, j) takes src.flatten()[src_off[g] + j * E:][:E]."""
    import ctypes
    if per > 1:
        r, w = ring.shape[0], ring.shape[2]
        e = ring[0, 0, 0].numel()
        assert ring.shape[1] == per
    else:
        r, w = ring.shape[0], ring.shape[1]
        e = ring[0, 0].numel()
    assert ring.is_contiguous() and src.is_contiguous() and len(src_off) == r
    assert all(0 <= o and o + per * e <= src.numel() for o in src_off)
    if blocks:
        assert state.is_contiguous() and (blocks - 1) * stride + delta + block <= state.numel()
        assert delta >= block and (blocks == 1 or stride >= delta + block), 'window_push: overlapping state blocks'
    offs = (ctypes.c_longlong * r)(*src_off)
    H.call('ss_window_push_groups', H.dptr(ring), H.dptr(src), ctypes.cast(offs, ctypes.c_void_p), r, per, w, e,
           H.dptr(state, True), blocks, block, stride, delta, H.stream())
    return ring


def window_advance(ring, work, src, src_off, k, state=None, state_src=None, blocks=0, block=0, stride=0, src_stride=0):
    """k frames of one stream (ss_window_advance): ring [R,W,...] and work [R,W-1+k,...] (contiguous) -- work[r] <- ring[r] rows
    1..W-1 then the k rows at src.flatten()[src_off[r] + j * E:][:E]; ring[r] <- the last W rows of work[r]; in the same launch
    `blocks` blocks of `block` floats: state.flatten()[b * stride:][:block] <- state_src.flatten()[b * src_stride:][:block]."""
    r, w = ring.shape[0], ring.shape[1]
    e = ring[0, 0].numel()
    assert ring.is_contiguous() and work.is_contiguous() and src.is_contiguous() and len(src_off) == r
    assert tuple(work.shape[:2]) == (r, w - 1 + k) and work[0, 0].numel() == e
    assert all(0 <= o and o + k * e <= src.numel() for o in src_off)
    if blocks:
        assert state.is_contiguous() and state_src.is_contiguous()
        assert (blocks - 1) * stride + block <= state.numel() and (blocks - 1) * src_stride + block <= state_src.numel()
    offs = (ctypes.c_longlong * r)(*src_off)
    H.call('ss_window_advance', H.dptr(ring), H.dptr(work), H.dptr(src), ctypes.cast(offs, ctypes.c_void_p), r, w, e, int(k),
           H.dptr(state, True), H.dptr(state_src, True), blocks, block, stride, src_stride, H.stream())
    return work


# ------------------------------------------------------------------ render
MODES = {'NORMAL': 0, 'FAST': 1}
# Opt-in (SS_RENDER_EPS_FOLD=1): the fused AVERAGE renders fold the reference's + 1e-6 into their row table
# (SS_WARP_EPS_FOLD): not the reference's arithmetic (~1e-3 px), never the default.
RENDER_EPS_FOLD = os.environ.get('SS_RENDER_EPS_FOLD', '0') == '1'


FUSIONS = {'AVERAGE': 0, 'FEATHER': H.MODE_FLAGS['SS_FUSE_FEATHER']}      # the fused single-launch render's fusion formulas (SS_FUSE_FEATHER)


def fused_render(fusion_mode):
    """Whether a fusion mode is one of the fused single-launch render's (ss_render_average*): what the clip and streaming paths ask
    where they choose between that render and the LINEAR chain."""
    return fusion_mode in FUSIONS


def _fusion_bit(fusion):
    """fusion= of the render_average* forms -> its bit of `mode`.  FEATHER: every view weighted by its distance to its own image
    border, w = max(min(1 - |xn|, 1 - |yn|), 0), all views at once (include/stabstitch_hip.h, SS_FUSE_FEATHER); it has no folded
    variant."""
    if fusion not in FUSIONS:
        raise ValueError("fusion must be 'AVERAGE' or 'FEATHER', got %r" % (fusion,))
    if FUSIONS[fusion] and RENDER_EPS_FOLD:
        raise ValueError('SS_RENDER_EPS_FOLD has no FEATHER form')
    return FUSIONS[fusion]


def _avg_mode(mode, fusion='AVERAGE'):
    return MODES[mode] | _fusion_bit(fusion) | (16 if RENDER_EPS_FOLD else 0)


def tps_warp(U, source, T, hc, wc, mode='NORMAL', with_mask=False):
    b, c, h, w = U.shape
    out = torch.empty((b, c + int(with_mask), hc, wc), device=U.device, dtype=torch.float32)
    H.call('ss_tps_warp_mask_nchw' if with_mask else 'ss_tps_warp_nchw', H.dptr(_f(U)), H.dptr(_f(source)),
           H.dptr(T), H.dptr(out), b, c, h, w, hc, wc, MODES[mode], H.stream())
    return out


def render_footprints(source, T, h, w, hc, wc, watch=None, fit=None):
    """source [n,V,63,2], T [n,V,2,66], images h x w -> footprints [n, ss_render_footprint_floats] of every (frame, view) on
    the hc x wc canvas (tile-corner sampling coordinates, mesh hulls, tile order), two small launches for the whole clip.
    watch = (guard, watch_i [n,4], watch_f [n,4]): the streaming overflow watcher (ops.canvas_watch on `source`, frame = stream) inside
    the same launches.  fit (a CanvasFit over the same n streams, with watch; its viewport is hc x wc): the watcher's wave goes on with
    the device-side refit of the streams' boxes (ss_render_footprints_watch_fit)."""
    n, v = source.shape[0], source.shape[1]
    per = int(H.lib().ss_render_footprint_floats(v, hc, wc))
    fp = torch.empty((n, per), device=source.device, dtype=torch.float32)
    if watch is None:
        H.call('ss_render_footprints', H.dptr(_f(source)), H.dptr(_f(T)), H.dptr(fp), n, v, h, w, hc, wc, H.stream())
    elif fit is not None:
        guard, wi, wf = watch
        assert tuple(wi.shape) == (n, 4) and tuple(wf.shape) == (n, 4) and (fit.hout, fit.wout) == (hc, wc)
        H.call('ss_render_footprints_watch_fit', H.dptr(_f(source)), H.dptr(_f(T)), H.dptr(fp), n, v, h, w, hc, wc, float(guard),
               H.dptr(wi, dtype=torch.int32), H.dptr(wf), *_fit_state(fit, n), float(fit.margin), float(fit.zoom_limit), H.stream())
    else:
        guard, wi, wf = watch
        assert tuple(wi.shape) == (n, 4) and tuple(wf.shape) == (n, 4)
        H.call('ss_render_footprints_watch', H.dptr(_f(source)), H.dptr(_f(T)), H.dptr(fp), n, v, h, w, hc, wc, float(guard),
               H.dptr(wi, dtype=torch.int32), H.dptr(wf), H.stream())
    return fp


def _fp_args(footprint):
    return H.dptr(footprint, True), (0 if footprint is None else footprint.numel())


class ExposureParams(collections.namedtuple('ExposureParams', 'alpha sigma_n sigma_g lo hi min_nodes gain_min gain_max')):
    """Parameters of exposure_update (include/stabstitch_hip.h, ss_exposure_update): smoothing factor alpha in (0, 1], the error
    model's sigma_n (grey levels) and sigma_g (gain), the usable sample range [lo, hi], the fewest nodes a view pair needs to count,
    and the clamp [gain_min, gain_max] of the target gains."""
    __slots__ = ()

    def __new__(cls, alpha=0.1, sigma_n=10.0, sigma_g=0.1, lo=4.0, hi=251.0, min_nodes=16, gain_min=0.5, gain_max=2.0):
        return super().__new__(cls, float(alpha), float(sigma_n), float(sigma_g), float(lo), float(hi), int(min_nodes),
                               float(gain_min), float(gain_max))


EXPOSURE_DIAG = 40      # doubles per frame of exposure_update's diagnostics


def exposure_state(device):
    """A stream's exposure state [12] fp32: smoothed gains [3][3] (1), word 9 the started flag (int 0), two spare words."""
    st = torch.zeros(12, device=device, dtype=torch.float32)
    st[:9] = 1.0
    return st


def _clip_views(views, u8=None):
    """The views of one launch, all alike: decoded uint8 frames [n,h,w,3] or fp32 planes [n,3,h,w] (u8: which; default: what the
    first view's type says) -> (n, h, w, u8)."""
    if u8 is None:
        u8 = views[0].dtype == torch.uint8
    if u8:
        n, h, w, _ = views[0].shape
    else:
        n, _, h, w = views[0].shape
    assert all(tuple(t.shape) == ((n, h, w, 3) if u8 else (n, 3, h, w)) for t in views)
    return n, h, w, u8


def exposure_update(views, footprint, hc, wc, state, params=None, mode='NORMAL', gains=None, want_diag=False):
    """Exposure gains of n consecutive frames of a stream, smoothed through each of them: views = list of 2|3 contiguous device
    tensors [n,3,h,w] fp32 (0..255) or [n,h,w,3] uint8 (a single frame may come without the n axis); footprint [n, ss_render_footprint_floats]
    (or one row) = the frames' rows of render_footprints on the hc x wc canvas; state = exposure_state(device), advanced in place;
    -> gains [n,V,3] fp32, what the renders' gains= takes (with want_diag also [n, EXPOSURE_DIAG] float64: per pair (0,1), (0,2),
    (1,2) and channel (n, Sa, Sb), at 27 the targets [V,3], at 36 whether a pair was kept).  One launch for n = 1, two otherwise; no
    host synchronisation.  Bit-identical to n single-frame calls."""
    p = ExposureParams() if params is None else params
    v = len(views)
    views = [t if t.dim() == 4 else t[None] for t in views]
    n, h, w, u8 = _clip_views(views)
    fp = footprint if footprint.dim() == 2 else footprint[None]
    assert fp.shape[0] == n and fp.stride(1) == 1 and tuple(state.shape) == (12,)
    if gains is None:
        gains = torch.empty((n, v, 3), device=state.device, dtype=torch.float32)
    assert tuple(gains.shape) == (n, v, 3)
    diag = torch.empty((n, EXPOSURE_DIAG), device=state.device, dtype=torch.float64) if want_diag else None
    arr = H.ptr_array(views, dtype=torch.uint8 if u8 else torch.float32)
    fpp = H.DevPtr(fp.data_ptr())
    fpp.dev = fp.device.index
    assert fp.is_cuda and fp.dtype == torch.float32
    H.call('ss_exposure_update', arr, int(u8), (3 if u8 else 12) * h * w, fpp, fp.shape[1], fp.stride(0) if n > 1 else fp.shape[1],
           n, v, h, w, hc, wc, MODES[mode], p.alpha, p.sigma_n, p.sigma_g, p.lo, p.hi, p.min_nodes, p.gain_min, p.gain_max,
           H.dptr(state), H.dptr(gains), H.dptr(diag, True, dtype=torch.float64), H.stream())
    return (gains, diag) if want_diag else gains


def _gains(gains, n, v):
    """gains= of a render of n frames of v views -> its device pointer ([n,V,3] fp32; [V,3] for one frame)."""
    if tuple(gains.shape) not in ((n, v, 3),) + (((v, 3),) if n == 1 else ()):
        raise ValueError('gains must be [%d,%d,3], got %s' % (n, v, tuple(gains.shape)))
    return H.dptr(gains)


def _render_average(views, source, T, hc, wc, mode, out, footprint, gains, u8, clip, fusion='AVERAGE'):
    """The four render_average* below, and with gains= their _gains entries.  u8: decoded uint8 frames [..,h,w,3] -> uint8 [..,hc,wc,3]
    instead of fp32 planes [..,3,h,w] -> [..,3,hc,wc]; clip: a leading frame axis n on views, source, T, footprint and out."""
    v = len(views)
    fuse = _fusion_bit(fusion)
    dt = torch.uint8 if u8 else torch.float32
    if not u8 and not clip:
        views = [_f(i) for i in views]
    h, w = views[0].shape[-3:-1] if u8 else views[0].shape[-2:]
    n = 1
    if clip:
        assert views[0].dim() == 4
        n, h, w, _ = _clip_views(views, u8)
        assert source.shape[0] == n and T.shape[0] == n
    arr = H.ptr_array(views, dtype=dt)
    shape = ((n,) if clip else ()) + ((hc, wc, 3) if u8 else (3, hc, wc))
    if out is None:
        out = torch.empty(shape, device=views[0].device, dtype=dt)
    assert not clip or tuple(out.shape) == shape
    if clip:                             # the footprint's size: one row of the clip's [n, row] block
        fp, fpn = H.dptr(footprint, True), (0 if footprint is None else footprint.shape[-1])
    else:                                # all of what the single frame was handed
        fp, fpn = _fp_args(footprint)
    name = 'ss_render_average' + ('_clip' if clip else '') + ('_u8' if u8 else '')
    outp = _u8ptr(out) if u8 else H.dptr(out)
    frames = (n,) if clip else ()        # the clip entries take the frame count in front of the view count
    args = (arr, H.dptr(_f(source)), H.dptr(T), fp, fpn, outp) + frames + (v, h, w, hc, wc)
    if gains is not None:                # exposure gains [n,V,3] (exposure_update): sampled values scaled and clamped to 255;
        H.call(name + '_gains', *args, MODES[mode] | fuse, _gains(gains, n, v), H.stream())      # (these entries have no folded variant)
    else:
        H.call(name, *args, _avg_mode(mode, fusion), H.stream())
    return out


def render_average(imgs, source, T, hc, wc, mode='NORMAL', out=None, footprint=None, gains=None, fusion='AVERAGE'):
    """imgs: list of 2|3 device tensors [1,3,h,w] / [3,h,w]; source [V,63,2]; T [V,2,66] -> [3,hc,wc].
    footprint: this frame's row of `render_footprints` (views that cannot reach a tile are skipped there and count as
    exactly 0 -- a deliberate deviation from the reference, whose clamped sampler returns a rounding residue of up to
    ~1e-2 grey levels outside a view's image; the skip test samples each 64 x 8 tile at six points and is not a proof),
    or None (every view evaluated everywhere: the reference's arithmetic at every pixel).
    fusion (here and in the _u8, _clip, _clip_u8 and _nv12 forms): 'AVERAGE', the reference's chained a a / (a + b + 1e-6), or
    'FEATHER', border-distance weights over all views at once (_fusion_bit) -- with it a footprint changes nothing at all."""
    return _render_average(imgs, source, T, hc, wc, mode, out, footprint, gains, u8=False, clip=False, fusion=fusion)


def render_average_u8(frames, source, T, hc, wc, mode='NORMAL', out=None, footprint=None, gains=None, fusion='AVERAGE'):
    """The fused AVERAGE render straight from decoded uint8 frames to the uint8 video frame: frames = list of 2|3 device
    tensors [h,w,3] uint8 (cv2 channel order); -> uint8 [hc,wc,3] = `.astype(np.uint8)` of the fused values.  Equal,
    bit for bit, to ingest (uint8 -> fp32 planes) + render_average + canvas_to_u8; the fp32 planes and canvas are never
    written."""
    return _render_average(frames, source, T, hc, wc, mode, out, footprint, gains, u8=True, clip=False, fusion=fusion)


def render_average_clip(views, source, T, hc, wc, mode='NORMAL', out=None, footprint=None, gains=None, fusion='AVERAGE'):
    """A whole clip in one launch: views = list of 2|3 contiguous device tensors [n,3,h,w]; source [n,V,63,2];
    T [n,V,2,66]; footprint [n, ss_render_footprint_floats] | None -> [n,3,hc,wc].  Bit-identical to n render_average calls."""
    return _render_average(views, source, T, hc, wc, mode, out, footprint, gains, u8=False, clip=True, fusion=fusion)


def render_average_clip_u8(views, source, T, hc, wc, mode='NORMAL', out=None, footprint=None, gains=None, fusion='AVERAGE'):
    """The same from decoded uint8 clips: views = list of 2|3 contiguous device tensors [n,h,w,3] uint8 -> uint8 [n,hc,wc,3]."""
    return _render_average(views, source, T, hc, wc, mode, out, footprint, gains, u8=True, clip=True, fusion=fusion)


def tps_warp_views(imgs, source, T, hc, wc, mode='NORMAL'):
    """imgs: list of V <= 3 device tensors [1,3,h,w] / [3,h,w] -> [V,4,hc,wc] (3 colour planes + ones-mask plane)."""
    v = len(imgs)
    imgs = [_f(i) for i in imgs]
    h, w = imgs[0].shape[-2:]
    arr = H.ptr_array(imgs)
    out = torch.empty((v, 4, hc, wc), device=imgs[0].device, dtype=torch.float32)
    H.call('ss_tps_warp_views', arr, H.dptr(_f(source)), H.dptr(T), H.dptr(out), v, h, w, hc, wc, MODES[mode],
           H.stream())
    return out


def add_mul(x, add, mul):
    out = torch.empty_like(x)
    H.call('ss_add_mul', H.dptr(x), H.dptr(out), float(add), float(mul), x.numel(), H.stream())
    return out


def mask_union(a, b):
    out = torch.empty_like(a)
    H.call('ss_mask_union', H.dptr(a), H.dptr(b), H.dptr(out), a.numel(), H.stream())
    return out


def _u8ptr(t):
    return H.dptr(t, dtype=torch.uint8)


def ingest_u8(frames, lr_h=360, lr_w=480, want_hr=True, hr_out=None, lr_out=None):
    """frames uint8 [n,h,w,3] (decoded, cv2 channel order) -> (hr [n,3,h,w] in 0..255 | None,
    lr [n,3,lr_h,lr_w] = cv2.resize(...)/127.5-1).  Replaces test_online_tra.py:252-278."""
    n, h, w, c = frames.shape
    if c != 3:
        raise ValueError('frames must be [n,h,w,3] uint8')
    dev = frames.device
    hr = None
    if want_hr:
        hr = hr_out if hr_out is not None else torch.empty((n, 3, h, w), device=dev, dtype=torch.float32)
    lr = lr_out if lr_out is not None else torch.empty((n, 3, lr_h, lr_w), device=dev, dtype=torch.float32)
    H.call('ss_ingest_u8', _u8ptr(frames), H.dptr(hr, allow_none=True), H.dptr(lr), n, h, w, lr_h, lr_w, H.stream())
    return hr, lr


def canvas_to_u8(canvas, out=None):
    """fp32 [n,3,h,w] -> uint8 [n,h,w,3] with `.astype(np.uint8)` semantics (test_online_tra.py:413)."""
    n, c, h, w = canvas.shape
    if c != 3:
        raise ValueError('canvas must be [n,3,h,w]')
    if out is None:
        out = torch.empty((n, h, w, 3), device=canvas.device, dtype=torch.uint8)
    H.call('ss_canvas_to_u8', H.dptr(canvas), _u8ptr(out), n, h, w, H.stream())
    return out


# ---- NV12 frames ("Frame formats"): uint8 [H*3/2, W] -- rows 0..H-1 the Y plane, rows H.. the interleaved UV plane -- or
# [n, H*3/2, W]; the columns are dense, the row stride is the pitch (>= W: a decoder surface is a view of a wider buffer)
def _nv12_geometry(t, batched=False):
    """-> (h, w, pitch, frame stride) of an NV12 device tensor; the frame stride is 0 for a single frame."""
    if not t.is_cuda:
        raise H.HipError('stabstitch2_amd kernels need device tensors (got %s); there is no CPU path' % t.device)
    if t.dtype != torch.uint8 or t.dim() != (3 if batched else 2) or t.shape[-2] % 3 or t.stride(-1) != 1:
        raise ValueError('an NV12 frame is a uint8 tensor [%sH*3/2, W] with dense columns, got %s %s strides %s'
                         % ('n, ' if batched else '', t.dtype, tuple(t.shape), tuple(t.stride())))
    return t.shape[-2] // 3 * 2, t.shape[-1], t.stride(-2), (t.stride(0) if batched else 0)


def _nv12_ptr(t, offset=0):
    p = H.DevPtr(t.data_ptr() + offset)
    p.dev = t.device.index
    return p


def _nv12_views(frames, batched=False):
    """list of V NV12 tensors of one size -> (y**, uv**, pitch*, frame_stride*, h, w) host arrays for the NV12 renders."""
    geo = [_nv12_geometry(f, batched) for f in frames]
    h, w = geo[0][:2]
    if any(g[:2] != (h, w) for g in geo) or any(f.device != frames[0].device for f in frames):
        raise ValueError('the NV12 views of one render share a size and a GPU')
    v = len(frames)
    ys = (ctypes.c_void_p * v)(*[f.data_ptr() for f in frames])
    uvs = (ctypes.c_void_p * v)(*[f.data_ptr() + h * g[2] for f, g in zip(frames, geo)])
    ys.dev = uvs.dev = frames[0].device.index
    return ys, uvs, (ctypes.c_int * v)(*[g[2] for g in geo]), (ctypes.c_longlong * v)(*[g[3] for g in geo]), h, w


def ingest_nv12(frames, lr_h=360, lr_w=480, want_hr=True, hr_out=None, lr_out=None):
    """frames NV12 [n,H*3/2,W] (or one frame [H*3/2,W]) -> (hr [n,3,H,W] in 0..255, B,G,R planes | None, lr [n,3,lr_h,lr_w]):
    byte for byte ingest_u8 of the frames converted to packed BGR, which are never written."""
    if frames.dim() == 2:
        frames = frames[None]
    h, w, pitch, fs = _nv12_geometry(frames, True)
    n, dev = frames.shape[0], frames.device
    hr = None
    if want_hr:
        hr = hr_out if hr_out is not None else torch.empty((n, 3, h, w), device=dev, dtype=torch.float32)
    lr = lr_out if lr_out is not None else torch.empty((n, 3, lr_h, lr_w), device=dev, dtype=torch.float32)
    H.call('ss_ingest_nv12', _nv12_ptr(frames), _nv12_ptr(frames, h * pitch), pitch, fs, H.dptr(hr, allow_none=True), H.dptr(lr),
           n, h, w, lr_h, lr_w, H.stream())
    return hr, lr


def bgr_to_nv12(bgr, out=None):
    """uint8 video frames [n,h,w,3] (or [h,w,3]) in B,G,R order -> NV12 [n,h*3/2,w] ([h*3/2,w]); out: an NV12 tensor to write
    (its row stride is the pitch).  h and w even."""
    single = bgr.dim() == 3
    if single:
        bgr = bgr[None]
    n, h, w, c = bgr.shape
    if c != 3 or h % 2 or w % 2:
        raise ValueError('bgr_to_nv12 takes uint8 [n,h,w,3] frames of even height and width, got %s' % (tuple(bgr.shape),))
    if out is None:
        out = torch.empty((n, h // 2 * 3, w), device=bgr.device, dtype=torch.uint8)
    elif out.dim() == 2:
        out = out[None]
    oh, ow, pitch, fs = _nv12_geometry(out, True)
    if (out.shape[0], oh, ow) != (n, h, w):
        raise ValueError('bgr_to_nv12: out must be NV12 [%d,%d,%d], got %s' % (n, h // 2 * 3, w, tuple(out.shape)))
    H.call('ss_bgr_to_nv12', _u8ptr(bgr), _nv12_ptr(out), _nv12_ptr(out, h * pitch), pitch, fs, n, h, w, H.stream())
    return out[0] if single else out


def nv12_surfaces(frames):
    """The surfaces of an NV12 argument: a tensor [n,H*3/2,W] (any row stride >= W, any frame stride), one frame [H*3/2,W], or a list of
    such 2-D tensors, each with its own pitch -> (list of 2-D surfaces, H, W, is it the single frame?).  Shapes, dtypes and strides
    only: no device is looked at.  What is no NV12 surface -- and an odd pitch, which the converter refuses -- is a ValueError."""
    single = torch.is_tensor(frames) and frames.dim() == 2
    if torch.is_tensor(frames):
        surf = [frames] if single else (list(frames.unbind(0)) if frames.dim() == 3 else [])
    else:
        surf = list(frames)
    s0 = surf[0] if surf and torch.is_tensor(surf[0]) else None
    if s0 is None or any(not torch.is_tensor(f) or f.dtype != torch.uint8 or f.dim() != 2 or f.shape != s0.shape or f.shape[0] % 3
                         or f.shape[0] == 0 or f.shape[1] == 0 or f.shape[1] % 2 or f.stride(1) != 1 or f.stride(0) < f.shape[1]
                         or f.stride(0) % 2 or f.device != s0.device for f in surf):
        raise ValueError('NV12 frames are uint8 tensors [n,H*3/2,W], one frame [H*3/2,W] or a list of such frames on one GPU: even H and '
                         'W, dense columns, an even row stride >= W; got %s'
                         % ([(str(f.dtype), tuple(f.shape), tuple(f.stride())) if torch.is_tensor(f) else type(f).__name__ for f in surf]
                            if surf else (tuple(frames.shape) if torch.is_tensor(frames) else 'an empty list'),))
    return surf, s0.shape[0] // 3 * 2, s0.shape[1], single


def nv12_to_bgr(frames, out=None):
    """Decoded NV12 surfaces -> the uint8 video frames [n,H,W,3] in B,G,R order ([H,W,3] for the single frame), byte for byte
    tests/nv12_ref.py's nv12_to_bgr.  frames: a device tensor [n,H*3/2,W] (any row stride >= W, any frame stride), one frame
    [H*3/2,W], or a list of such 2-D tensors each with its own pitch -- a decoder's surface pool; the UV plane of a surface is its rows
    H.. .  ONE launch for up to 96 surfaces (libstabstitch_surfaces.so), more go in chunks.  out: [n,H,W,3] uint8 to write, its frames
    dense, its frame stride free."""
    surf, h, w, single = nv12_surfaces(frames)
    n, dev = len(surf), surf[0].device
    if not surf[0].is_cuda:
        raise H.HipError('stabstitch2_amd kernels need device tensors (got %s); there is no CPU path' % dev)
    if out is None:
        out = torch.empty((n, h, w, 3), device=dev, dtype=torch.uint8)
    else:
        if single and out.dim() == 3:
            out = out[None]
        if out.dtype != torch.uint8 or tuple(out.shape) != (n, h, w, 3) or out.device != dev or not out[0].is_contiguous() \
                or (n > 1 and out.stride(0) < 3 * h * w):
            raise ValueError('nv12_to_bgr: out must be uint8 [%d,%d,%d,3] with dense frames on %s, got %s %s strides %s'
                             % (n, h, w, dev, out.dtype, tuple(out.shape), tuple(out.stride())))
    stride = out.stride(0) if n > 1 else 3 * h * w
    for c in range(0, n, F.MAX_SURFACES):
        part = surf[c:c + F.MAX_SURFACES]
        m = len(part)
        ys = (ctypes.c_void_p * m)(*[f.data_ptr() for f in part])
        uvs = (ctypes.c_void_p * m)(*[f.data_ptr() + h * f.stride(0) for f in part])
        ys.dev = dev.index
        F.call('ssf_nv12_to_bgr', ys, uvs, (ctypes.c_int * m)(*[f.stride(0) for f in part]), m, h, w, _nv12_ptr(out[c]), stride,
               H.stream())
    return out[0] if single else out


def render_average_nv12(frames, source, T, hc, wc, mode='NORMAL', out=None, footprint=None, out_format='bgr', fusion='AVERAGE'):
    """render_average_u8 from decoded NV12 frames: frames = list of 2|3 NV12 device tensors [H*3/2,W]; out_format 'bgr' -> the uint8
    video frame [hc,wc,3] (byte for byte render_average_u8 of the converted frames), 'nv12' -> that frame as NV12 [hc*3/2,wc]
    (byte for byte bgr_to_nv12 of it; hc, wc even).  Neither the converted frames nor, for 'nv12', the BGR frame are written."""
    if out_format not in ('bgr', 'nv12'):
        raise ValueError("out_format must be 'bgr' or 'nv12'")
    fuse = _fusion_bit(fusion)
    ys, uvs, pitches, _, h, w = _nv12_views(list(frames))
    dev = frames[0].device
    fp, fpn = _fp_args(footprint)
    if out_format == 'bgr':
        if out is None:
            out = torch.empty((hc, wc, 3), device=dev, dtype=torch.uint8)
        o_y, o_uv, o_pitch = _u8ptr(out), None, 0
    else:
        if hc % 2 or wc % 2:
            raise ValueError('NV12 output needs an even canvas, got %d x %d' % (hc, wc))
        if out is None:
            out = torch.empty((hc // 2 * 3, wc), device=dev, dtype=torch.uint8)
        oh, ow, o_pitch, _ = _nv12_geometry(out)
        if (oh, ow) != (hc, wc):
            raise ValueError('render_average_nv12: out must be NV12 [%d,%d], got %s' % (hc // 2 * 3, wc, tuple(out.shape)))
        o_y, o_uv = _nv12_ptr(out), _nv12_ptr(out, hc * o_pitch)
    H.call('ss_render_average_nv12', ys, uvs, pitches, H.dptr(_f(source)), H.dptr(T), fp, fpn, o_y, o_uv, o_pitch,
           int(out_format == 'nv12'), len(frames), h, w, hc, wc, MODES[mode] | fuse, H.stream())
    return out


def render_linear_frames_nv12(views, source, T, sizes, mode='NORMAL', outs=None, ws=None):
    """render_linear_frames from decoded NV12 frames: views = list of 2|3 NV12 device tensors [n,H*3/2,W] -> the uint8 video frames
    [hc_i,wc_i,3], byte for byte render_linear_frames of the converted frames (NV12 frames out: bgr_to_nv12 behind it)."""
    ys, uvs, pitches, strides, h, w = _nv12_views(list(views), True)
    n, v, dev = views[0].shape[0], len(views), views[0].device
    assert source.shape[0] == n and T.shape[0] == n and len(sizes) == n and all(t.shape[0] == n for t in views)
    sizes = [(int(a), int(b)) for a, b in sizes]
    if outs is None:
        outs = [torch.empty((hc, wc, 3), device=dev, dtype=torch.uint8) for hc, wc in sizes]
    assert len(outs) == n and all(tuple(o.shape) == (hc, wc, 3) and o.dtype == torch.uint8 for o, (hc, wc) in zip(outs, sizes))
    if ws is None:
        ws = linear_frames_workspace(sizes, v, dev)
    hcs = (ctypes.c_int * n)(*[s[0] for s in sizes])
    wcs = (ctypes.c_int * n)(*[s[1] for s in sizes])
    H.call('ss_render_linear_frames_nv12', ys, uvs, pitches, strides, H.dptr(_f(source)), H.dptr(T),
           H.ptr_array(outs, dtype=torch.uint8), n, v, h, w, hcs, wcs, MODES[mode], H.dptr(ws), H.stream())
    return list(outs)


def linear_blend(ref, tgt, ref_m, tgt_m, want_mask=False, out=None):
    """ref,tgt [3,hc,wc]; ref_m,tgt_m [hc,wc] -> fused [3,hc,wc] (or mask1 [hc,wc])."""
    hc, wc = ref_m.shape[-2:]
    ws = torch.empty(int(H.lib().ss_linear_blend_workspace_floats(hc, wc)), device=ref_m.device, dtype=torch.float32)
    if not want_mask and out is None:
        out = torch.empty((3, hc, wc), device=ref_m.device, dtype=torch.float32)
    if want_mask:
        out = None
    mk = torch.empty((hc, wc), device=ref_m.device, dtype=torch.float32) if want_mask else None
    H.call('ss_linear_blend', H.dptr(ref, True), H.dptr(tgt, True), H.dptr(_f(ref_m)), H.dptr(_f(tgt_m)),
           H.dptr(out, True), H.dptr(mk, True), hc, wc, H.dptr(ws), H.stream())
    return mk if want_mask else out


def render_linear_clip(views, source, T, hc, wc, mode='NORMAL', out=None, want_masks=False, gains=None):
    """LINEAR fusion of a whole clip in three launches (four with three views): views = list of 2|3 contiguous device tensors
    [n,3,h,w] fp32 -> [n,3,hc,wc]; or [n,h,w,3] uint8 -> the uint8 video frames [n,hc,wc,3].  source [n,V,63,2]; T [n,V,2,66].
    want_masks: also return the blender's mask1 of every pass [n,V-1,hc,wc].  Bit-identical to the per-frame chain
    tps_warp_views + linear_blend (+ mask_union + linear_blend)."""
    v = len(views)
    n, h, w, u8 = _clip_views(views)
    assert source.shape[0] == n and T.shape[0] == n
    dev = views[0].device
    arr = H.ptr_array(views, dtype=torch.uint8 if u8 else torch.float32)
    shape = (n, hc, wc, 3) if u8 else (n, 3, hc, wc)
    if out is None:
        out = torch.empty(shape, device=dev, dtype=views[0].dtype)
    assert tuple(out.shape) == shape and out.dtype == views[0].dtype
    ws = torch.empty(int(H.lib().ss_linear_clip_workspace_floats(n, v, hc, wc)), device=dev, dtype=torch.float32)
    mk = torch.empty((n, v - 1, hc, wc), device=dev, dtype=torch.float32) if want_masks else None
    # gains: exposure gains [n,V,3] -- the colour planes scaled and clamped, the masks untouched
    H.call('ss_render_linear_clip' + ('_u8' if u8 else '') + ('' if gains is None else '_gains'), arr, H.dptr(_f(source)), H.dptr(T),
           _u8ptr(out) if u8 else H.dptr(out), H.dptr(mk, True), n, v, h, w, hc, wc, MODES[mode], H.dptr(ws),
           *(() if gains is None else (_gains(gains, n, v),)), H.stream())
    return (out, mk) if want_masks else out


def linear_frames_workspace(sizes, views, device):
    """Workspace of render_linear_frames for these canvases [(hc, wc)] (a stitcher holds it across pushes)."""
    n = len(sizes)
    hcs = (ctypes.c_int * n)(*[int(s[0]) for s in sizes])
    wcs = (ctypes.c_int * n)(*[int(s[1]) for s in sizes])
    need = int(H.lib().ss_linear_frames_workspace_floats(n, views, hcs, wcs))
    if need <= 0:
        raise ValueError('render_linear_frames: 1..32 frames of 2|3 views on canvases of 11..65535 pixels a side, got %d x %d views on %s'
                         % (n, views, list(sizes)))
    return torch.empty(need, device=device, dtype=torch.float32)


def render_linear_frames(views, source, T, sizes, mode='NORMAL', outs=None, ws=None, gains=None):
    """LINEAR fusion of n frames that each have their OWN canvas in three launches (four with three views) whatever n is: views =
    list of 2|3 contiguous device tensors [n,3,h,w] fp32 -> list of n frames [3,hc_i,wc_i]; or [n,h,w,3] uint8 -> the uint8 video
    frames [hc_i,wc_i,3].  source [n,V,63,2]; T [n,V,2,66]; sizes = n pairs (hc, wc); 1 <= n <= 32.  outs: n tensors to write;
    ws: linear_frames_workspace(sizes, V, device).  Bit-identical, frame by frame, to render_linear_clip called with that one
    frame on that canvas."""
    v = len(views)
    n, h, w, u8 = _clip_views(views)
    assert source.shape[0] == n and T.shape[0] == n and len(sizes) == n
    dev, dt = views[0].device, views[0].dtype
    sizes = [(int(a), int(b)) for a, b in sizes]
    shapes = [(hc, wc, 3) if u8 else (3, hc, wc) for hc, wc in sizes]
    if outs is None:
        outs = [torch.empty(shp, device=dev, dtype=dt) for shp in shapes]
    assert len(outs) == n and all(tuple(o.shape) == shp and o.dtype == dt for o, shp in zip(outs, shapes))
    if ws is None:
        ws = linear_frames_workspace(sizes, v, dev)
    hcs = (ctypes.c_int * n)(*[s[0] for s in sizes])
    wcs = (ctypes.c_int * n)(*[s[1] for s in sizes])
    H.call('ss_render_linear_frames' + ('_u8' if u8 else '') + ('' if gains is None else '_gains'), H.ptr_array(views, dtype=dt),
           H.dptr(_f(source)), H.dptr(T), H.ptr_array(outs, dtype=dt), n, v, h, w, hcs, wcs, MODES[mode], H.dptr(ws),
           *(() if gains is None else (_gains(gains, n, v),)), H.stream())
    return list(outs)


# ------------------------------------------------------------------ MULTIBAND fusion (libstabstitch_blend.so)
MULTIBAND_BANDS = 5
_weight_planes = {}


def multiband_weight_plane(h, w, device):
    """The plane that decides MULTIBAND's seam, [h,w] fp32: min(x + 1, w - x) * min(y + 1, h - y) (small integers, exact).  Warped next
    to B, G, R, the view with the larger value owns a canvas pixel.  Built once per size and device."""
    device = torch.device(device)
    key = (int(h), int(w), device.type, device.index)

    def build():
        x = torch.arange(w, dtype=torch.float32)
        y = torch.arange(h, dtype=torch.float32)
        return (torch.minimum(x + 1, w - x)[None, :] * torch.minimum(y + 1, h - y)[:, None]).contiguous().to(device)
    if device.type != 'cuda':
        return build()
    b = _weight_planes.get(key)
    if b is None:
        b = _weight_planes[key] = _Built(build, device, 'the MULTIBAND weight plane')
    return b.get(device)


def check_bands(bands, hc=None, wc=None):
    """ValueError for a band count the blend refuses (on this canvas, when one is given)."""
    if not isinstance(bands, int) or isinstance(bands, bool) or not 0 <= bands <= B.MAX_BANDS:
        raise ValueError('bands must be an integer 0..%d, got %r' % (B.MAX_BANDS, bands))
    if hc is not None and B.lib().ssb_multiband_workspace_floats(1, 2, int(hc), int(wc), bands) < 0:
        raise ValueError('MULTIBAND: %d bands need every reduced level of the %d x %d canvas to be at least 3 pixels a side'
                         % (bands, hc, wc))
    return bands


def multiband_workspace(frames, views, hc, wc, bands, device):
    """The workspace of multiband_blend for `frames` frames in one call (ssb_multiband_workspace_floats)."""
    need = int(B.lib().ssb_multiband_workspace_floats(frames, views, hc, wc, bands))
    if need < 0:
        raise ValueError('multiband_blend: 2|3 views, 0..%d bands, every reduced level at least 3 pixels a side; got %d frames of %d '
                         'views on %d x %d with %r bands' % (B.MAX_BANDS, frames, views, hc, wc, bands))
    return torch.empty(need, device=device, dtype=torch.float32)


def multiband_blend(P, bands=MULTIBAND_BANDS, out=None, ws=None, u8=False):
    """Laplacian-pyramid blend of warped views: P [V,5,hc,wc] (or [n,V,5,hc,wc]: n frames in the launches of one) = per view the warped
    B, G, R, the warped multiband_weight_plane and the ones-mask, as tps_warp(.., with_mask=True) writes them -> [3,hc,wc] fp32
    ([n,3,hc,wc]), or with u8 the video frame [hc,wc,3] uint8 ([n,hc,wc,3]) = canvas_to_u8 of the same values.  2 * bands + 2 launches."""
    clip = P.dim() == 5
    if P.dim() not in (4, 5) or P.shape[-3] != 5:
        raise ValueError('P must be [V,5,hc,wc] or [n,V,5,hc,wc], got %s' % (tuple(P.shape),))
    n = P.shape[0] if clip else 1
    v, hc, wc = P.shape[-4], P.shape[-2], P.shape[-1]
    if ws is None:
        ws = multiband_workspace(n, v, hc, wc, bands, P.device)
    shape = ((n,) if clip else ()) + ((hc, wc, 3) if u8 else (3, hc, wc))
    dt = torch.uint8 if u8 else torch.float32
    if out is None:
        out = torch.empty(shape, device=P.device, dtype=dt)
    if tuple(out.shape) != shape:
        raise ValueError('out must be %s, got %s' % (shape, tuple(out.shape)))
    B.call('ssb_multiband_blend_u8' if u8 else 'ssb_multiband_blend', H.dptr(P), H.dptr(out, dtype=dt), H.dptr(ws), ws.numel(), n, v, hc, wc,
           bands, H.stream())
    return out


def multiband_stack(imgs):
    """What MULTIBAND warps: imgs = list of V views, each fp32 planes [3,h,w] / [1,3,h,w] / [n,3,h,w] or decoded uint8 frames [h,w,3] /
    [n,h,w,3] (through the existing ingest) -> U [n*V,4,h,w], frame-major: B, G, R and the weight plane."""
    v = len(imgs)
    u8 = imgs[0].dtype == torch.uint8
    imgs = [i if i.dim() == 4 else i[None] for i in imgs]
    if u8:
        n, h, w, _ = imgs[0].shape
        want = (n, h, w, 3)
    else:
        n, _, h, w = imgs[0].shape
        want = (n, 3, h, w)
    if any(tuple(i.shape) != want or i.dtype != imgs[0].dtype for i in imgs):
        raise ValueError('the views of one MULTIBAND render must have one shape and type, got %s' % [tuple(i.shape) for i in imgs])
    dev = imgs[0].device
    U = torch.empty((n * v, 4, h, w), device=dev, dtype=torch.float32)
    Uv = U.view(n, v, 4, h, w)
    Uv[:, :, 3] = multiband_weight_plane(h, w, dev)
    for k, img in enumerate(imgs):
        if u8 and n == 1:                # straight into the stack: U[k, 0:3] is contiguous
            H.call('ss_ingest_u8', _u8ptr(img), H.dptr(U[k, 0:3]), None, 1, h, w, 0, 0, H.stream())
        elif u8:
            hr = torch.empty((n, 3, h, w), device=dev, dtype=torch.float32)
            H.call('ss_ingest_u8', _u8ptr(img), H.dptr(hr), None, n, h, w, 0, 0, H.stream())
            Uv[:, k, 0:3] = hr
        else:
            Uv[:, k, 0:3] = img
    return U


def multiband_warp(imgs, source, T, hc, wc, mode='NORMAL', gains=None):
    """The direct warp of MULTIBAND fusion (libstabstitch_mbwarp.so), one launch: imgs as multiband_stack takes them;
    source [V,63,2] / [n,V,63,2]; T [V,2,66] / [n,V,2,66] -> P [V,5,hc,wc] / [n,V,5,hc,wc], what multiband_seam and multiband_blend
    read.  Without gains it equals `tps_warp(multiband_stack(imgs), source, T, hc, wc, mode, with_mask=True)` bit for bit, and the
    stack is never written.  gains [n,V,3] ([V,3] for one frame; exposure_update): planes 0..2 become min(g * s, 255), as in the fused
    renders; the weight plane and the mask are untouched."""
    v = len(imgs)
    clip = source.dim() == 4
    u8 = imgs[0].dtype == torch.uint8
    imgs = [i if i.dim() == 4 else i[None] for i in imgs]
    if u8:
        n, h, w, _ = imgs[0].shape
        want = (n, h, w, 3)
    else:
        n, _, h, w = imgs[0].shape
        want = (n, 3, h, w)
    if any(tuple(i.shape) != want or i.dtype != imgs[0].dtype for i in imgs):
        raise ValueError('the views of one MULTIBAND render must have one shape and type, got %s' % [tuple(i.shape) for i in imgs])
    if (clip and source.shape[0] != n) or (not clip and n != 1) or source.shape[-3] != v or T.numel() != n * v * 132:
        raise ValueError('source %s and T %s do not match %d frames of %d views' % (tuple(source.shape), tuple(T.shape), n, v))
    g = None if gains is None else _gains(gains, n, v)
    dt = torch.uint8 if u8 else torch.float32
    if not u8:
        imgs = [_f(i) for i in imgs]
    P = torch.empty(((n, v, 5, hc, wc) if clip else (v, 5, hc, wc)), device=imgs[0].device, dtype=torch.float32)
    W.call('ssw_multiband_warp_u8' if u8 else 'ssw_multiband_warp', H.ptr_array(imgs, dtype=dt), H.dptr(_f(source)), H.dptr(T), g,
           H.dptr(P), n, v, h, w, hc, wc, MODES[mode], H.stream())
    return P


# ------------------------------------------------------------------ MULTIBAND's content-aware seam (libstabstitch_seam.so)
SEAM_PRIOR = 8.0
SEAMS = ('geometric', 'dp')


def seam_cell(hc, wc, cell=None):
    """The cell size of the seam's grid on a hc x wc canvas: `cell` checked (one of 1, 2, 4, 8, 16 whose dynamic program fits the LDS
    of one workgroup), or for None the smallest of 4, 8, 16 that fits.  ValueError names a larger cell where one helps."""
    if cell is None:
        for c in (4, 8, 16):
            if S.lds_bytes(hc, wc, c) <= S.LDS_BYTES:
                return c
        raise ValueError('the DP seam has no cell size for a %d x %d canvas: its rows and back pointers exceed the LDS at cell 16' % (hc, wc))
    if isinstance(cell, bool) or not isinstance(cell, int) or cell not in S.CELLS:
        raise ValueError('seam cell must be one of %s, got %r' % (S.CELLS, cell))
    if S.lds_bytes(hc, wc, cell) > S.LDS_BYTES:
        fit = [c for c in S.CELLS if c > cell and S.lds_bytes(hc, wc, c) <= S.LDS_BYTES]
        raise ValueError('the DP seam at cell=%d on a %d x %d canvas needs %d bytes of LDS, a workgroup has %d: %s'
                         % (cell, hc, wc, S.lds_bytes(hc, wc, cell), S.LDS_BYTES,
                            'use a larger cell, cell=%d fits' % fit[0] if fit else 'no larger cell fits either'))
    return cell


def seam_params(hc, wc, cell=None, mu=None, prior=None):
    """-> (cell, mu, prior) with the defaults filled in (cell: seam_cell; mu = 48 * cell; prior = SEAM_PRIOR) and checked."""
    cell = seam_cell(hc, wc, cell)
    mu = 48 * cell if mu is None else mu
    if isinstance(mu, bool) or not isinstance(mu, int) or not 0 <= mu <= S.MU_MAX:
        raise ValueError('seam mu must be an integer 0..%d, got %r' % (S.MU_MAX, mu))
    prior = SEAM_PRIOR if prior is None else float(prior)
    if not 0.0 <= prior <= S.PRIOR_MAX:
        raise ValueError('seam prior must be in 0..%g, got %r' % (S.PRIOR_MAX, prior))
    return cell, mu, prior


def seam_state(views, hc, wc, cell=None, device='cuda'):
    """The seam state of one stream on one canvas (int32, all zero = fresh): what multiband_seam's temporal term remembers -- the grid,
    the view order and the previous seams.  `state.zero_()` forgets it."""
    if views not in (2, 3):
        raise ValueError('the DP seam takes 2 or 3 views, got %r' % (views,))
    hq = S.grid(hc, wc, seam_cell(hc, wc, cell))[0]
    return torch.zeros(S.STATE_HEADER + (views - 1) * hq, device=device, dtype=torch.int32)


def seam_workspace(frames, views, hc, wc, cell, device):
    """The int32 workspace of multiband_seam for `frames` frames in one call (ssm_seam_workspace_bytes; _seam.layout names its parts)."""
    need = int(S.lib().ssm_seam_workspace_bytes(frames, views, hc, wc, cell))
    if need < 0:
        raise ValueError('multiband_seam: 1..65535 frames of 2|3 views, a cell of %s whose grid fits the LDS; got %d frames of %d views '
                         'on %d x %d at cell %r' % (S.CELLS, frames, views, hc, wc, cell))
    return torch.empty(need // 4, device=device, dtype=torch.int32)


def multiband_seam(P, cell=None, mu=None, prior=None, state=None, ws=None):
    """The content-aware seam of MULTIBAND fusion, in place: P [V,5,hc,wc] or [n,V,5,hc,wc] as tps_warp(.., with_mask=True) writes it;
    plane 3 of every view becomes the small integer seam weights that multiband_blend then reads -- a top-to-bottom minimal-cost seam per
    pair of neighbouring views on a grid of cell x cell cells (tests/seam_ref.py is the definition).  mu: the cost of moving the seam
    one cell sideways against the previous frame's (needs `state`, ops.seam_state; the frames of a clip are taken in order); prior: the
    pull towards the geometric seam.  Three launches whatever n is.  -> P."""
    clip = P.dim() == 5
    if P.dim() not in (4, 5) or P.shape[-3] != 5:
        raise ValueError('P must be [V,5,hc,wc] or [n,V,5,hc,wc], got %s' % (tuple(P.shape),))
    n = P.shape[0] if clip else 1
    v, hc, wc = P.shape[-4], P.shape[-2], P.shape[-1]
    if v not in (2, 3):
        raise ValueError('the DP seam takes 2 or 3 views, got %d' % v)
    cell, mu, prior = seam_params(hc, wc, cell, mu, prior)
    if ws is None:
        ws = seam_workspace(n, v, hc, wc, cell, P.device)
    if state is not None and (state.dtype != torch.int32 or state.numel() < S.STATE_HEADER + (v - 1) * S.grid(hc, wc, cell)[0]):
        raise ValueError('seam state: int32 of at least %d values for %d views on this grid (ops.seam_state), got %s of %d'
                         % (S.STATE_HEADER + (v - 1) * S.grid(hc, wc, cell)[0], v, state.dtype, state.numel()))
    S.call('ssm_multiband_seam', H.dptr(P), n, v, hc, wc, cell, mu, prior, H.dptr(state, True, dtype=torch.int32),
           0 if state is None else state.numel(), H.dptr(ws, dtype=torch.int32), 4 * ws.numel(), H.stream())
    return P


def check_seam(seam, fusion_mode='MULTIBAND'):
    """ValueError for a seam that does not exist, or for seam= with a fusion mode that has none (None: not given)."""
    if seam is None:
        return None
    if fusion_mode != 'MULTIBAND':
        raise ValueError("seam= belongs to fusion_mode='MULTIBAND', got %r" % (fusion_mode,))
    if seam not in SEAMS:
        raise ValueError('seam must be one of %s, got %r' % (SEAMS, seam))
    return seam


def render_multiband(imgs, source, T, hc, wc, mode='NORMAL', bands=MULTIBAND_BANDS, out=None, ws=None, u8=None, seam='geometric',
                     seam_state=None, seam_cell=None, seam_mu=None, seam_prior=None, gains=None):
    """MULTIBAND fusion of one frame or of n: imgs as multiband_stack takes them; source [V,63,2] / [n,V,63,2]; T [V,2,66] / [n,V,2,66]
    -> [3,hc,wc] / [n,3,hc,wc] fp32, or the uint8 video frame(s) [hc,wc,3] / [n,hc,wc,3] (u8: default, what the input is).  One warp
    launch of the existing ss_tps_warp_mask_nchw over every (frame, view) and four planes, then multiband_blend: exactly
    `multiband_blend(tps_warp(multiband_stack(imgs), source, T, hc, wc, mode, with_mask=True))`.
    seam='dp': multiband_seam(P, seam_cell, seam_mu, seam_prior, seam_state) between the two (three more launches); 'geometric', the
    default, is the seam where the warped weight planes cross and launches nothing more.
    gains [n,V,3] ([V,3] for one frame; exposure_update): the warp is multiband_warp(gains=) instead -- one launch from the frames, no
    stack -- so the seam and the blend both see the compensated colours.  Without gains the launches are the ones above."""
    v = len(imgs)
    clip = source.dim() == 4
    if gains is not None:
        n = imgs[0].shape[0] if imgs[0].dim() == 4 else 1
        if tuple(gains.shape) not in ((n, v, 3),) + (((v, 3),) if n == 1 else ()):
            raise ValueError('gains must be [%d,%d,3], got %s' % (n, v, tuple(gains.shape)))
    if u8 is None:
        u8 = imgs[0].dtype == torch.uint8
    check_bands(bands, hc, wc)
    if check_seam(seam) is None:
        raise ValueError('seam must be one of %s, got None' % (SEAMS,))
    if seam == 'dp':
        seam_params(hc, wc, seam_cell, seam_mu, seam_prior)
    elif seam_state is not None or seam_cell is not None or seam_mu is not None or seam_prior is not None:
        raise ValueError("seam_state=, seam_cell=, seam_mu= and seam_prior= belong to seam='dp'")
    if gains is not None:
        P = multiband_warp(imgs, source, T, hc, wc, mode, gains=gains)
        if seam == 'dp':
            multiband_seam(P, seam_cell, seam_mu, seam_prior, seam_state)
        return multiband_blend(P, bands, out=out, ws=ws, u8=u8)
    U = multiband_stack(imgs)
    n = U.shape[0] // v
    if (clip and source.shape[0] != n) or (not clip and n != 1) or source.shape[-3] != v:
        raise ValueError('source %s does not match %d frames of %d views' % (tuple(source.shape), n, v))
    P = tps_warp(U, _f(source).view(n * v, 63, 2), T.view(n * v, 2, 66), hc, wc, mode, with_mask=True)
    P = P.view(n, v, 5, hc, wc) if clip else P
    if seam == 'dp':
        multiband_seam(P, seam_cell, seam_mu, seam_prior, seam_state)
    return multiband_blend(P, bands, out=out, ws=ws, u8=u8)


def mesh_bbox(meshes, img_h, img_w, bbox=None):
    """meshes: list of LR-scale tensors [...,2] -> device tensor [4] = wmin, wmax, hmin, hmax (HR px).
    bbox: an existing box to fold these meshes into (in place)."""
    acc = bbox is not None
    if bbox is None:
        bbox = torch.empty(4, device=meshes[0].device, dtype=torch.float32)
    for i, m in enumerate(meshes):
        m = _f(m)
        H.call('ss_mesh_bbox', H.dptr(m), m.numel() // 2, float(img_h), float(img_w), H.dptr(bbox), int(acc or i > 0),
               H.stream())
    return bbox


def mesh_normalize(mesh, bbox, img_h, img_w):
    """LR-scale mesh [...,2] -> canvas-normalised [N,63,2]."""
    m = _f(mesh)
    out = torch.empty((m.numel() // 126, 63, 2), device=m.device, dtype=torch.float32)
    H.call('ss_mesh_normalize', H.dptr(m), H.dptr(bbox), H.dptr(out), m.numel() // 2, float(img_h), float(img_w),
           H.stream())
    return out


def mesh_normalize_views(meshes, bbox, img_h, img_w):
    """meshes: V tensors [..., N,7,9,2] (N frames each) -> the render's control points [N,V,63,2] on the canvas `bbox`."""
    v = len(meshes)
    n = meshes[0].numel() // 126
    out = torch.empty((n, v, 63, 2), device=meshes[0].device, dtype=torch.float32)
    for k, m in enumerate(meshes):
        m = _f(m)
        assert m.numel() == n * 126
        H.call('ss_mesh_normalize_views', H.dptr(m), H.dptr(bbox), H.dptr(out), n, k, v, float(img_h), float(img_w), H.stream())
    return out


def canvas_watch_state(streams, device):
    """Fresh (watch_i [S,4] int32, watch_f [S,4] fp32) for ops.canvas_watch."""
    wi = torch.tensor([[0, 0, -1, 0]] * streams, dtype=torch.int32, device=device)
    inf = float('inf')
    wf = torch.tensor([[inf, -inf, inf, -inf]] * streams, dtype=torch.float32, device=device)
    return wi, wf


CanvasFit = collections.namedtuple('CanvasFit', 'box epoch ext0 margin zoom_limit hout wout')
CanvasFit.__doc__ = """State and policy of the device-side canvas refit (ss_canvas_watch_fit): box [S,4] fp32 (wmin, wmax, hmin, hmax in HR px),
epoch [S] int32, ext0 [S,2] fp32 (the extents the canvases were set with) -- device tensors the launches rewrite in place -- and the
margin, the zoom limit and the viewport (hout, wout)."""


def canvas_fit_state(n, device):
    """Fresh (box [n,4] fp32, epoch [n] int32, ext0 [n,2] fp32) of the device-side refit, all zero: set the boxes, then
    box_fit_aspect(box, hout, wout, ext0)."""
    return (torch.zeros((n, 4), dtype=torch.float32, device=device), torch.zeros((n,), dtype=torch.int32, device=device),
            torch.zeros((n, 2), dtype=torch.float32, device=device))


def box_fit_aspect(boxes, hout, wout, ext0=None):
    """boxes [n,4] (or [4]) letterboxed in place about their centres to the viewport's aspect wout : hout (ss_box_fit_aspect: the
    aspect step of the refit alone; a box only ever expands); ext0 [n,2]: receives the fitted (width, height)."""
    n = boxes.numel() // 4
    assert boxes.is_contiguous() and boxes.numel() == 4 * n and (ext0 is None or (ext0.is_contiguous() and ext0.numel() == 2 * n))
    H.call('ss_box_fit_aspect', H.dptr(boxes), H.dptr(ext0, True), n, int(hout), int(wout), H.stream())
    return boxes


def _fit_state(fit, s):
    """The three state pointers of a CanvasFit over s streams."""
    assert fit.box.numel() == 4 * s and fit.epoch.numel() == s and fit.ext0.numel() == 2 * s
    return H.dptr(fit.box), H.dptr(fit.epoch, dtype=torch.int32), H.dptr(fit.ext0)


def canvas_watch(src, watch_i, watch_f, guard, fit=None):
    """src [S,V,63,2] canvas-normalised control points of one push -> updates the streams' overflow state (ss_canvas_watch).
    fit (a CanvasFit over the S streams): the same wave goes on with the device-side refit of the streams' boxes (ss_canvas_watch_fit)."""
    s, v = src.shape[0], src.shape[1]
    assert src.is_contiguous() and tuple(watch_i.shape) == (s, 4) and tuple(watch_f.shape) == (s, 4)
    if fit is not None:
        H.call('ss_canvas_watch_fit', H.dptr(src), s, v, float(guard), H.dptr(watch_i, dtype=torch.int32), H.dptr(watch_f),
               *_fit_state(fit, s), float(fit.margin), float(fit.zoom_limit), int(fit.hout), int(fit.wout), H.stream())
        return
    H.call('ss_canvas_watch', H.dptr(src), s, v, float(guard), H.dptr(watch_i, dtype=torch.int32), H.dptr(watch_f), H.stream())


def canvas_watch_frames(src, watch_i, watch_f, guard, fit=None):
    """src [k,V,63,2] canvas-normalised control points of k consecutive frames of ONE stream -> its watcher row watch_i [1,4] /
    watch_f [1,4] updated frame by frame (ss_canvas_watch_frames; equal to k canvas_watch calls).  fit (a CanvasFit of that one
    stream): ONE refit of its box behind the batch's last frame (ss_canvas_watch_frames_fit)."""
    k, v = src.shape[0], src.shape[1]
    assert src.is_contiguous() and tuple(watch_i.shape) == (1, 4) and tuple(watch_f.shape) == (1, 4)
    if fit is not None:
        H.call('ss_canvas_watch_frames_fit', H.dptr(src), k, v, float(guard), H.dptr(watch_i, dtype=torch.int32), H.dptr(watch_f),
               *_fit_state(fit, 1), float(fit.margin), float(fit.zoom_limit), int(fit.hout), int(fit.wout), H.stream())
        return
    H.call('ss_canvas_watch_frames', H.dptr(src), k, v, float(guard), H.dptr(watch_i, dtype=torch.int32), H.dptr(watch_f), H.stream())


def stream_normalize_watch(meshes, frame_stride, bboxes, img_h, img_w, guard=0.0, watch_i=None, watch_f=None):
    """One push's render control points of all views + the overflow watcher in ONE launch: meshes = V tensors whose stream s starts
    `frame_stride` floats after stream s - 1; bboxes [4] (one canvas) or [S,4] (a canvas per stream) -> [S,V,63,2]; equal, bit for
    bit, to mesh_normalize_views(_boxes) (+ canvas_watch when the watcher state is given)."""
    v = len(meshes)
    s = 1 if bboxes.dim() == 1 else bboxes.shape[0]
    for m in meshes:
        assert m.is_contiguous() and m.dtype == torch.float32
    out = torch.empty((s, v, 63, 2), device=bboxes.device, dtype=torch.float32)
    arr = H.ptr_array(list(meshes))
    H.call('ss_stream_normalize_watch', arr, v, int(frame_stride), H.dptr(bboxes), 0 if bboxes.dim() == 1 else 4, H.dptr(out), s,
           float(img_h), float(img_w), float(guard), H.dptr(watch_i, True, dtype=torch.int32), H.dptr(watch_f, True), H.stream())
    return out


def stream_splines(meshes, frame_stride, bboxes, nrigid, img_h, img_w, frames=None):
    """One push's render control points AND their splines in ONE launch (ss_stream_splines): arguments as stream_normalize_watch
    -> (src [S,V,63,2], T [S,V,2,66]), equal bit for bit to stream_normalize_watch + tps_solve_shared.  The overflow watcher is not
    touched: render_footprints(..., watch=...) or canvas_watch(src, ...).
    frames = k with ONE canvas bboxes [4]: k frames of one stream on it (frame i's meshes i * frame_stride floats further) -> [k,...]."""
    v = len(meshes)
    s = 1 if bboxes.dim() == 1 else bboxes.shape[0]
    if frames is not None:
        assert bboxes.dim() == 1 and frames >= 1
        s = int(frames)
    for m in meshes:
        assert m.is_contiguous() and m.dtype == torch.float32
    assert nrigid.numel() == 126 and nrigid.is_contiguous()
    src = torch.empty((s, v, 63, 2), device=bboxes.device, dtype=torch.float32)
    T = torch.empty((s, v, 2, 66), device=bboxes.device, dtype=torch.float32)
    arr = H.ptr_array(list(meshes))
    H.call('ss_stream_splines', arr, v, int(frame_stride), H.dptr(bboxes), 0 if bboxes.dim() == 1 else 4, H.dptr(nrigid), H.dptr(src),
           H.dptr(T), s, float(img_h), float(img_w), H.stream())
    return src, T


def mesh_normalize_views_boxes(meshes, frame_stride, bboxes, img_h, img_w):
    """Per-frame canvases: meshes = list of V tensors whose frame f starts `frame_stride` floats after frame f - 1 (the tensor
    handed in starts at frame 0's mesh); bboxes [n,4] -> [n,V,63,2]."""
    n, v = bboxes.shape[0], len(meshes)
    out = torch.empty((n, v, 63, 2), device=bboxes.device, dtype=torch.float32)
    for k, m in enumerate(meshes):
        assert m.is_contiguous() and m.dtype == torch.float32
        H.call('ss_mesh_normalize_views_boxes', H.dptr(m), int(frame_stride), H.dptr(bboxes), H.dptr(out), n, k, v, float(img_h),
               float(img_w), H.stream())
    return out


def h2mesh(Hm, mesh):
    """H [n,3,3], mesh [n,...,2] -> persp_divide(H^-1 [x y 1]^T), same shape as mesh (spatial_network.py:20-36)."""
    n = Hm.shape[0]
    m = _f(mesh)
    out = torch.empty_like(m)
    H.call('ss_h2mesh', H.dptr(_f(Hm)), H.dptr(m), H.dptr(out), n, m.numel() // (2 * n), H.stream())
    return out


def three_view_align(w12_m1, w12_m2, w23_m1, w23_m2, img_h, img_w):
    """Four LR meshes [1,N,7,9,2] -> (a1, a2, b1, b2, mid) [1,N,7,9,2] in HR pixels: pair (2,3) shifted by the per-frame mean
    offset, middle plane (threeview:345-380)."""
    n = w12_m1.numel() // 126
    outs = [torch.empty((1, n, 7, 9, 2), device=w12_m1.device, dtype=torch.float32) for _ in range(5)]
    H.call('ss_three_view_align', H.dptr(_f(w12_m1)), H.dptr(_f(w12_m2)), H.dptr(_f(w23_m1)), H.dptr(_f(w23_m2)),
           *[H.dptr(o) for o in outs], n, float(img_h), float(img_w), H.stream())
    return outs


def three_view_normalize(a1, a2, b1, b2, mid, bbox):
    """The five aligned meshes [1,N,7,9,2] (HR pixels) normalised on the first canvas in one launch -> [6, N, 63, 2] =
    {a1, b2 | a2, b1 | mid, mid}: points [0:2], sources [2:4], targets [4:6] of the two re-projections' batched TPS solve."""
    n = mid.numel() // 126
    out = torch.empty((6, n, 63, 2), device=mid.device, dtype=torch.float32)
    H.call('ss_three_view_normalize', H.dptr(_f(a1)), H.dptr(_f(a2)), H.dptr(_f(b1)), H.dptr(_f(b2)), H.dptr(_f(mid)), H.dptr(bbox),
           H.dptr(out), n * 63, H.stream())
    return out


def three_view_finish(n1, n3, mid, bbox):
    """Re-projected outer meshes n1 / n3 [N,63,2] (normalised on the first canvas `bbox`) and the untranslated middle mesh
    -> (mesh1, middle, mesh3) [1,N,7,9,2] in first-canvas pixels."""
    n = mid.numel() // 126
    outs = [torch.empty((1, n, 7, 9, 2), device=mid.device, dtype=torch.float32) for _ in range(3)]
    H.call('ss_three_view_finish', H.dptr(_f(n1)), H.dptr(_f(n3)), H.dptr(_f(mid)), H.dptr(bbox), *[H.dptr(o) for o in outs],
           n * 63, H.stream())
    return outs


def three_view_splines(m12_1, m12_2, m23_1, m23_2, first_box, out_box, nrigid, img_h, img_w, frames=None, frame_stride=126):
    """The streaming three-view push between the chains' smoothed meshes and the render in ONE launch (ss_three_view_splines =
    three_view_align -> three_view_normalize -> tps_solve -> tps_points -> three_view_finish on the first canvas, then the final
    meshes normalised on the output canvas and tps_solve_shared onto the rigid mesh; bit-identical to those launches).
    m*: [k,7,9,2] contiguous, LR scale -> ((mesh1, middle, mesh3) [1,k,7,9,2] first-canvas pixels, src [k,3,63,2], T [k,3,2,66]).
    frames = k: each m* is frame 0's mesh [7,9,2] and frame f's lies f * frame_stride floats further in the same storage (the
    window-last meshes of SmoothNet's windows: frame_stride = 7 * 126).
    The overflow watcher is not touched: render_footprints(..., watch=...) or canvas_watch(src, ...)."""
    if frames is None:
        assert frame_stride == 126
        k = m12_1.numel() // 126
        for m in (m12_1, m12_2, m23_1, m23_2):
            assert m.is_contiguous() and m.dtype == torch.float32 and m.numel() == k * 126
    else:
        k = int(frames)
        assert k >= 1 and frame_stride >= 126
        for m in (m12_1, m12_2, m23_1, m23_2):
            assert m.is_contiguous() and m.dtype == torch.float32 and m.numel() == 126
            assert m.storage_offset() + (k - 1) * frame_stride + 126 <= m.untyped_storage().nbytes() // 4, 'frames past the storage'
    assert nrigid.numel() == 126 and nrigid.is_contiguous()
    d = m12_1.device
    outs = [torch.empty((1, k, 7, 9, 2), device=d, dtype=torch.float32) for _ in range(3)]
    src = torch.empty((k, 3, 63, 2), device=d, dtype=torch.float32)
    T = torch.empty((k, 3, 2, 66), device=d, dtype=torch.float32)
    H.call('ss_three_view_splines', H.dptr(m12_1), H.dptr(m12_2), H.dptr(m23_1), H.dptr(m23_2), int(frame_stride), H.dptr(first_box),
           H.dptr(out_box), H.dptr(nrigid), *[H.dptr(o) for o in outs], H.dptr(src), H.dptr(T), k, float(img_h), float(img_w), H.stream())
    return tuple(outs), src, T


def fill(t, value=0.0):
    """t[...] = value in place (t contiguous fp32)."""
    H.call('ss_fill_f32', H.dptr(t), float(value), t.numel(), H.stream())
    return t


# ------------------------------------------------------------------ smooth glue
def smooth_embed(sm1, sm2, ts1, ts2, e1w, e1b, e3w, e3b, nw, t, wstride, zero_first):
    hidden = torch.empty((nw, t, 7, 9, 128), device=sm1.device, dtype=torch.float32)
    H.call('ss_smooth_embed', H.dptr(sm1), H.dptr(sm2), H.dptr(ts1), H.dptr(ts2), H.dptr(e1w), H.dptr(e1b),
           H.dptr(e3w), H.dptr(e3b), H.dptr(hidden), nw, t, wstride, int(zero_first), H.stream())
    return hidden


def smooth_finalize(sm1, sm2, ts1, ts2, delta, nw, t, wstride, zero_first):
    names = ('ori_mesh1', 'ori_mesh2', 'ori_path1', 'ori_path2', 'smooth_mesh1', 'smooth_mesh2', 'smooth_path1',
             'smooth_path2')
    outs = {k: torch.empty((nw, t, 7, 9, 2), device=sm1.device, dtype=torch.float32) for k in names}
    H.call('ss_smooth_finalize', H.dptr(sm1), H.dptr(sm2), H.dptr(ts1), H.dptr(ts2), H.dptr(delta),
           *[H.dptr(outs[k]) for k in names], nw, t, wstride, int(zero_first), H.stream())
    return outs



def smooth_stitch(sm1, sm2, ts1, ts2, delta, nw, t, want_paths=True):
    """The clip's tensors straight from the sliding windows (ss_smooth_stitch): sm*/ts* [n,7,9,2] with n = nw + t - 1,
    delta [nw,t,7,9,4] -> dict(ori_mesh1/2, smooth_mesh1/2 [1,n,7,9,2] (+ ori_path2, smooth_path2))."""
    n = nw + t - 1
    assert sm1.shape[0] == n and delta.numel() == nw * t * 63 * 4
    names = ['ori_mesh1', 'ori_mesh2', 'smooth_mesh1', 'smooth_mesh2'] + (['ori_path2', 'smooth_path2'] if want_paths else [])
    outs = {k: torch.empty((1, n, 7, 9, 2), device=sm1.device, dtype=torch.float32) for k in names}
    H.call('ss_smooth_stitch', H.dptr(sm1), H.dptr(sm2), H.dptr(ts1), H.dptr(ts2), H.dptr(delta),
           H.dptr(outs['ori_mesh1']), H.dptr(outs['ori_mesh2']), H.dptr(outs['smooth_mesh1']), H.dptr(outs['smooth_mesh2']),
           H.dptr(outs.get('ori_path2'), True), H.dptr(outs.get('smooth_path2'), True), nw, t, H.stream())
    return outs


# ------------------------------------------------------------------ SmoothNet of a stitched clip (libstabstitch_smoothtail.so)
SMOOTH_TAIL = os.environ.get('SS_SMOOTH_TAIL', '1') == '1'      # '0': smooth_stage runs every frame of every window on the conv engine
SMOOTH_TAIL_FRAMES = ((0, 2), (2, 4), (4, 6))                   # (first_in, first_out) of the three Conv3d layers, window k >= 1


def smooth_tail_usable(nw, t):
    """Does pipeline.smooth_stage take the clip-only path for `nw` windows of `t` frames?  Not under the deterministic policy (it
    promises clip == stream bit for bit and the stream keeps the conv engine's kernels), only for the 7-frame window the kernels are
    written for, and only up to one launch's windows."""
    return SMOOTH_TAIL and not is_deterministic() and t == 7 and 0 < nw <= ST.MAX_WINDOWS


def smooth_tail_seg_tiles(nw):
    """The K tiles of one partial sum: the cut ss_conv_nhwc makes for [nw,7,7,9,128] x Conv3d(128,128,(5,3,3)), so that the clip-only
    layers add up what the full windows would, bit for bit (ss_conv_workspace_need = splits * M * cout floats, 0 without a cut)."""
    need = _conv_ws_need(nw, 7, 7, 9, 128, 128, 5, 3, 3, 1, 2, 1, 1, 1)
    splits = max(1, need // (nw * 7 * 63 * 128))
    return -(-ST.K_TILES // splits)


def smooth_tail_layer(x, wgt, bias, nw, first_in, first_out, seg_tiles=None):
    """One ragged Conv3d(128,128,(5,3,3)) + bias + ReLU (sst_conv3d_layer): x compact [frames_in,63,128] (window 0: 7 frames, later
    windows frames first_in..6; first_in = 0 is ss_smooth_embed's [nw,7,7,9,128]) -> compact [frames_out,63,128]."""
    if seg_tiles is None:
        seg_tiles = smooth_tail_seg_tiles(nw)
    frames_in, frames_out = 7 + (nw - 1) * (7 - first_in), 7 + (nw - 1) * (7 - first_out)
    if x.numel() != frames_in * 63 * 128 or tuple(wgt.shape) != (128, 5, 3, 3, 128):
        raise ValueError('smooth_tail_layer: %s / %s do not match %d windows from frame %d' % (tuple(x.shape), tuple(wgt.shape), nw, first_in))
    out = torch.empty((frames_out, 63, 128), device=x.device, dtype=torch.float32)
    nseg = -(-ST.K_TILES // max(1, seg_tiles))
    ws = torch.empty(nseg * out.numel(), device=x.device, dtype=torch.float32) if nseg > 1 else None
    ST.call('sst_conv3d_layer', H.dptr(x), H.dptr(wgt), H.dptr(bias, True), H.dptr(out), H.dptr(ws, True),
            0 if ws is None else ws.numel(), nw, first_in, first_out, seg_tiles, H.stream())
    return out


def smooth_tail_decode(hid, w, b, delta, nw, first=6):
    """Linear(128,4) on compact rows, scattered into delta [nw,7,7,9,4] where ss_smooth_stitch reads (sst_decode_scatter); the
    rest of delta stays as it is."""
    if hid.numel() != (7 + (nw - 1) * (7 - first)) * 63 * 128 or delta.numel() != nw * 7 * 63 * 4 or tuple(w.shape) != (4, 128):
        raise ValueError('smooth_tail_decode: %s / %s do not match %d windows from frame %d' % (tuple(hid.shape), tuple(delta.shape), nw, first))
    ST.call('sst_decode_scatter', H.dptr(hid), H.dptr(w), H.dptr(b, True), H.dptr(delta), nw, first, H.stream())
    return delta


def smooth_tail_deltas(hid, convs, dec, nw, out=None):
    """SmoothNet behind the embedding for a stitched clip: hid [nw,7,7,9,128] (ss_smooth_embed), convs: the three packed
    (weight, bias) pairs, dec: the packed decoder -> delta [nw,7,7,9,4], written at window 0's frames and at frame 6 of every later
    window (what ss_smooth_stitch reads; the other entries are never written).  Same launches as the conv engine takes."""
    if out is None:
        out = torch.empty((nw, 7, 7, 9, 4), device=hid.device, dtype=torch.float32)
    seg_tiles = smooth_tail_seg_tiles(nw)
    for (w, b), (first_in, first_out) in zip(convs, SMOOTH_TAIL_FRAMES):
        hid = smooth_tail_layer(hid, w, b, nw, first_in, first_out, seg_tiles)
    return smooth_tail_decode(hid, dec[0], dec[1], out, nw)


# ------------------------------------------------------------------ coverage and the largest covered rectangle (libstabstitch_cover.so)
MIN_MASK = 0.5       # a view covers a pixel where its warped ones-mask is >= this: MULTIBAND's validity rule (tests/multiband_ref.py)


class CoverageState(collections.namedtuple('CoverageState', 'bitmap ws hc wc')):
    """A running coverage of a hc x wc canvas: bitmap int64 [hc, ceil(wc / 64)] (bit i of word j = column 64 j + i; the AND of every
    frame's coverage so far) and the workspace `ws` (uint8) that covered_rect searches it with."""
    __slots__ = ()


def coverage_words(wc):
    return (int(wc) + 63) // 64


def _cover_canvas(what, hc, wc):
    for v in (hc, wc):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError('%s: the canvas size must be two ints, got %r x %r' % (what, hc, wc))
    if hc <= 1 or wc <= 1 or wc > CV.MAX_WIDTH or hc * wc >= 2 ** 31 or (hc + 7) // 8 > 65535:
        raise ValueError('%s: no coverage of a %d x %d canvas (2 .. %d columns, fewer than 2^31 pixels)' % (what, hc, wc, CV.MAX_WIDTH))


def _cover_args(what, source, T, h, w, mode, min_mask):
    """The checks coverage and coverage_update share -> (source [n,V,63,2], T, n, v, min_mask)."""
    if not torch.is_tensor(source) or not torch.is_tensor(T):
        raise ValueError('%s takes the splines as tensors: source [n,V,63,2], T [n,V,2,66]' % what)
    if source.dim() == 3:
        source = source[None]
    if source.dim() != 4 or tuple(source.shape[2:]) != (63, 2) or source.shape[1] not in (2, 3) or source.shape[0] < 1:
        raise ValueError('%s: source must be [n,V,63,2] with V = 2 | 3, got %s' % (what, tuple(source.shape)))
    n, v = int(source.shape[0]), int(source.shape[1])
    if T.numel() != n * v * 132 or tuple(T.shape[-2:]) != (2, 66):
        raise ValueError('source %s and T %s do not match %d frames of %d views' % (tuple(source.shape), tuple(T.shape), n, v))
    if source.dtype != torch.float32 or T.dtype != torch.float32:
        raise ValueError('%s takes fp32 splines, got %s and %s' % (what, source.dtype, T.dtype))
    if mode not in MODES:
        raise ValueError("%s: mode must be 'NORMAL' or 'FAST', got %r" % (what, mode))
    for x in (h, w):
        if isinstance(x, bool) or not isinstance(x, int) or x <= 1:
            raise ValueError('%s: the image size must be two ints > 1, got %r x %r' % (what, h, w))
    if isinstance(min_mask, bool) or not isinstance(min_mask, (int, float)) or not 0.0 < float(min_mask) <= 1.0:
        raise ValueError('%s: min_mask must lie in (0, 1], got %r' % (what, min_mask))
    return source, T, n, v, float(min_mask)


def coverage(source, T, h, w, hc, wc, mode='NORMAL', min_mask=MIN_MASK):
    """Which pixels of the hc x wc canvas each frame covers, one launch: source [n,V,63,2] ([V,63,2]: one frame), T [n,V,2,66]: the
    splines the renders take, of V images h x w -> bitmaps int64 [n, hc, ceil(wc / 64)], bit i of word j = column 64 j + i (pad bits
    0).  A pixel is covered where some view's warped ones-mask -- the mask plane of tps_warp(..., with_mask=True) and of
    multiband_warp, bit for bit -- is >= min_mask."""
    source, T, n, v, min_mask = _cover_args('coverage', source, T, h, w, mode, min_mask)
    _cover_canvas('coverage', hc, wc)
    if n > CV.MAX_FRAMES:
        raise ValueError('coverage takes at most %d frames per call, got %d' % (CV.MAX_FRAMES, n))
    out = torch.empty((n, hc, coverage_words(wc)), device=source.device, dtype=torch.int64)
    CV.call('ssc_coverage', H.dptr(_f(source)), H.dptr(_f(T)), H.dptr(out, dtype=torch.int64), n, v, h, w, hc, wc, MODES[mode], min_mask,
            0, H.stream())
    return out


def coverage_state(hc, wc, device):
    """A fresh CoverageState of a hc x wc canvas: every column < wc covered, and covered_rect's workspace."""
    _cover_canvas('coverage_state', hc, wc)
    bitmap = torch.full((hc, coverage_words(wc)), -1, device=device, dtype=torch.int64)
    if wc % 64:
        bitmap[:, -1] = (1 << (wc % 64)) - 1
    ws = torch.empty(int(CV.lib().ssc_rect_workspace_bytes(hc, wc)), device=device, dtype=torch.uint8)
    return CoverageState(bitmap, ws, hc, wc)


def coverage_update(state, source, T, h, w, mode='NORMAL', min_mask=MIN_MASK):
    """state.bitmap &= the coverage of every frame of source [n,V,63,2] / T [n,V,2,66] (as `coverage` takes them), in one launch
    that loops over the frames; -> state."""
    if not isinstance(state, CoverageState):
        raise ValueError('coverage_update takes a CoverageState (ops.coverage_state), got %r' % type(state).__name__)
    source, T, n, v, min_mask = _cover_args('coverage_update', source, T, h, w, mode, min_mask)
    CV.call('ssc_coverage', H.dptr(_f(source)), H.dptr(_f(T)), H.dptr(state.bitmap, dtype=torch.int64), n, v, h, w, state.hc, state.wc,
            MODES[mode], min_mask, 1, H.stream())
    return state


def covered_rect(bitmap_or_state, even=False, wc=None, ws=None):
    """The largest rectangle of covered pixels -> int32 [4] = (y0, x0, h, w) on the device (largest area, then smallest y0, then
    smallest x0, then largest width; zeros when nothing is covered; even: h and w rounded down to even).  Nothing synchronises.
    bitmap_or_state: a CoverageState, or a bitmap int64 [hc, W64] ([1, hc, W64]) with wc= its width in pixels (ws: a workspace of
    ssc_rect_workspace_bytes(hc, wc) bytes to search it with, else a new one).  A stack of n > 1 bitmaps is refused: the library
    ANDs frames where it computes them -- run the frames through coverage_update and pass the state."""
    if isinstance(bitmap_or_state, CoverageState):
        if wc is not None or ws is not None:
            raise ValueError('covered_rect: wc= and ws= belong to a bare bitmap, a CoverageState has its own')
        bitmap, ws, hc, wc = bitmap_or_state
    else:
        bitmap = bitmap_or_state
        if not torch.is_tensor(bitmap) or bitmap.dtype != torch.int64 or bitmap.dim() not in (2, 3):
            raise ValueError('covered_rect takes a CoverageState or an int64 bitmap [hc, W64]')
        if bitmap.dim() == 3:
            if bitmap.shape[0] != 1:
                raise ValueError('covered_rect takes one bitmap, got a stack of %d: AND the frames with coverage_update and pass '
                                 'its state' % bitmap.shape[0])
            bitmap = bitmap[0]
        if isinstance(wc, bool) or not isinstance(wc, int):
            raise ValueError('covered_rect: a bare bitmap needs wc=, its width in pixels')
        hc = int(bitmap.shape[0])
        _cover_canvas('covered_rect', hc, wc)
        if bitmap.shape[1] != coverage_words(wc):
            raise ValueError('covered_rect: a bitmap of %d words per row is not %d pixels wide' % (bitmap.shape[1], wc))
        need = int(CV.lib().ssc_rect_workspace_bytes(hc, wc))
        if ws is None:
            ws = torch.empty(need, device=bitmap.device, dtype=torch.uint8)
        elif not torch.is_tensor(ws) or ws.dtype != torch.uint8 or ws.numel() < need:
            raise ValueError('covered_rect: ws must be a uint8 tensor of at least %d bytes' % need)
    rect = torch.empty(4, device=bitmap.device, dtype=torch.int32)
    CV.call('ssc_covered_rect', H.dptr(bitmap, dtype=torch.int64), hc, wc, int(bool(even)), H.dptr(ws, dtype=torch.uint8), ws.numel(),
            H.dptr(rect, dtype=torch.int32), H.stream())
    return rect


# ------------------------------------------------------------------ fixed-size output of a rectangle (libstabstitch_resample.so)
def _resample_size(what, size, aspect):
    if not isinstance(size, (tuple, list)) or len(size) != 2 or any(isinstance(v, bool) or not isinstance(v, int) or v < 1 for v in size):
        raise ValueError('%s: size must be (Hout, Wout) as two ints >= 1, got %r' % (what, size))
    if not isinstance(aspect, str) or aspect not in RS.ASPECTS:
        raise ValueError("%s: aspect must be 'fill' or 'stretch', got %r" % (what, aspect))
    return int(size[0]), int(size[1]), RS.ASPECTS[aspect]


def _resample_rect(what, rect, hc, wc, dev):
    """rect of resample / to_size -> (rect_dev pointer | None, y0, x0, h, w)."""
    if rect is None:
        return None, 0, 0, hc, wc
    if torch.is_tensor(rect):
        if rect.dtype != torch.int32 or tuple(rect.shape) != (4,) or not rect.is_contiguous():
            raise ValueError('%s: a rect tensor is int32 [4] = (y0, x0, h, w), as covered_rect returns it, got %s %s'
                             % (what, rect.dtype, tuple(rect.shape)))
        if rect.device != dev:
            raise ValueError('%s: the rect tensor lives on %s, the frames on %s' % (what, rect.device, dev))
        return rect, 0, 0, 0, 0
    if not isinstance(rect, (tuple, list)) or len(rect) != 4 or any(isinstance(v, bool) or not isinstance(v, int) or v < 0 for v in rect):
        raise ValueError('%s: rect must be None, (y0, x0, h, w) as non-negative ints or an int32 [4] device tensor, got %r' % (what, rect))
    return (None,) + tuple(int(v) for v in rect)


def resample_window(rect, frame_hw, size, aspect='fill'):
    """(fy, fx, fh, fw): the window of rect = (y0, x0, h, w) on a frame of frame_hw = (Hc, Wc) that `resample` reads for an output of
    `size` -- ssr_source_window, the function the kernel runs; zeros when the rectangle misses the frame."""
    hout, wout, asp = _resample_size('resample_window', size, aspect)
    hc, wc, _ = _resample_size('resample_window', frame_hw, aspect)
    if torch.is_tensor(rect):
        raise ValueError('resample_window takes the rectangle as four ints: a device rectangle stays on the device')
    _, y0, x0, h, w = _resample_rect('resample_window', rect, hc, wc, None)
    out = (ctypes.c_double * 4)()
    H.check_side(RS.lib().ssr_source_window((ctypes.c_int * 4)(y0, x0, h, w), hc, wc, hout, wout, asp, out), 'ssr_source_window')
    return tuple(float(v) for v in out)


def resample(frames, size, rect=None, aspect='fill', out=None, out_format='bgr'):
    """The rectangle `rect` of every frame, resampled with the triangle prefilter (PIL's; interpolate(mode='bilinear',
    antialias=True)) to exactly size = (Hout, Wout), ONE launch whatever n:
    fp32 [n,3,H,W] -> fp32 [n,3,Hout,Wout], unrounded; uint8 [n,H,W,3] -> uint8 [n,Hout,Wout,3] (floor(v + 0.5)), or with
    out_format='nv12' -> NV12 [n,Hout*3/2,Wout], byte for byte bgr_to_nv12 of those bytes (Hout, Wout even).  A single frame
    ([3,H,W] / [H,W,3]) gives a single frame.
    rect: None (the whole frame), (y0, x0, h, w) as non-negative ints, or the int32 [4] device tensor covered_rect returns -- that
    one is read inside the kernel: nothing synchronises, nothing is read back.  The rectangle is clipped to the frame; where
    nothing is left the output is black.  aspect: 'fill' resamples the centred part of the rectangle with the output's aspect,
    'stretch' all of it.  No pixel outside the rectangle contributes.
    out: a tensor to write -- NV12 with its row stride as the pitch (as bgr_to_nv12 takes it), BGR frames with a free frame stride
    (as nv12_to_bgr takes them), fp32 dense."""
    what = 'resample'
    if not torch.is_tensor(frames) or frames.dtype not in (torch.float32, torch.uint8) or frames.dim() not in (3, 4):
        raise ValueError('resample takes fp32 [n,3,H,W] or uint8 [n,H,W,3] frames (or one frame), got %s'
                         % ((frames.dtype, tuple(frames.shape)) if torch.is_tensor(frames) else type(frames).__name__,))
    u8 = frames.dtype == torch.uint8
    single = frames.dim() == 3
    if single:
        frames = frames[None]
    if frames.shape[3 if u8 else 1] != 3 or 0 in frames.shape:
        raise ValueError('resample takes fp32 [n,3,H,W] or uint8 [n,H,W,3] frames, got %s %s' % (frames.dtype, tuple(frames.shape)))
    n = int(frames.shape[0])
    hc, wc = (int(frames.shape[1]), int(frames.shape[2])) if u8 else (int(frames.shape[2]), int(frames.shape[3]))
    hout, wout, asp = _resample_size(what, size, aspect)
    if out_format not in ('bgr', 'nv12'):
        raise ValueError("resample: out_format must be 'bgr' or 'nv12', got %r" % (out_format,))
    nv12 = out_format == 'nv12'
    if nv12 and (not u8 or hout % 2 or wout % 2):
        raise ValueError("resample: out_format='nv12' takes uint8 frames and an even size, got %s and %d x %d" % (frames.dtype, hout, wout))
    if n > RS.MAX_FRAMES or hc * wc >= 2 ** 31 or hout * wout >= 2 ** 31 or (hout + 15) // 16 > 65535 or (wout + 63) // 64 > 65535:
        raise ValueError('resample: at most %d frames of fewer than 2^31 pixels, in and out, per call' % RS.MAX_FRAMES)
    dev = frames.device
    rdev, y0, x0, h, w = _resample_rect(what, rect, hc, wc, dev)
    shape = (n, hout // 2 * 3, wout) if nv12 else (n, hout, wout, 3) if u8 else (n, 3, hout, wout)
    if out is not None:
        if torch.is_tensor(out) and single and out.dim() == len(shape) - 1:
            out = out[None]
        ok = torch.is_tensor(out) and out.dtype == frames.dtype and tuple(out.shape) == shape and out.device == dev
        if ok and nv12:
            ok = out.stride(2) == 1 and out.stride(1) >= wout and out.stride(1) % 2 == 0 and out.stride(0) % 2 == 0 \
                and (n == 1 or out.stride(0) >= out.stride(1) * shape[1])
        elif ok and u8:
            ok = out[0].is_contiguous() and (n == 1 or out.stride(0) >= 3 * hout * wout)
        elif ok:
            ok = out.is_contiguous()
        if not ok:
            raise ValueError('resample: out must be %s %s on %s (NV12: dense columns, an even row stride >= Wout; BGR: dense frames, a '
                             'frame stride >= a frame; fp32: dense), got %s'
                             % (frames.dtype, list(shape), dev, (out.dtype, tuple(out.shape), tuple(out.stride()), out.device)
                                if torch.is_tensor(out) else type(out).__name__))
    if not frames.is_cuda:
        raise ValueError('resample needs device tensors (got %s); there is no CPU path' % dev)
    if out is None:
        out = torch.empty(shape, device=dev, dtype=frames.dtype)
    if not frames.is_contiguous():
        frames = frames.contiguous()
    tail = (n, hc, wc, hout, wout, asp, H.dptr(rdev, allow_none=True, dtype=torch.int32), y0, x0, h, w, H.stream())
    if nv12:
        pitch = out.stride(1)
        fs = out.stride(0) if n > 1 else pitch * shape[1]
        RS.call('ssr_resample_u8_nv12', _u8ptr(frames), _nv12_ptr(out), _nv12_ptr(out, hout * pitch), pitch, fs, *tail)
    elif u8:
        RS.call('ssr_resample_u8', _u8ptr(frames), _nv12_ptr(out), out.stride(0) if n > 1 else 3 * hout * wout, *tail)
    else:
        RS.call('ssr_resample_f32', H.dptr(frames), H.dptr(out), *tail)
    return out[0] if single else out
