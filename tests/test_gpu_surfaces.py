"""The NV12 surface converter on the GPU (libstabstitch_surfaces.so) and the batched NV12 routes built on it:
ops.nv12_to_bgr against tests/nv12_ref.py, its launches, its addressing past byte 2^31, then push_many_nv12, MultiOnlineStitcher.push_nv12
and HostFrameStream's frame_format / out / batch keywords against the packed-BGR routes they are defined by.  Every comparison is exact.
    python -m pytest tests/test_gpu_surfaces.py -m gpu -s"""
import gc
import re

import numpy as np
import pytest
import torch

import nv12_ref as N
import sweep_inputs as G
from stabstitch2_amd import synth
from test_gpu_nv12 import PAD, SH, SW, VIEWPORTS, _surface
from test_gpu_parity import dev, hip_nets  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
T = torch.from_numpy
GUARD = 64                                   # bytes of canary either side of an output (a multiple of 8: `out` keeps its alignment)
FILL = 0x5A


def _case(dev, seed, n, h, w, pad, gap_rows=0, lead=0):
    """n random NV12 frames with random padding -> (the device view [n,h*3/2,w] of a buffer [n, h*3/2 + gap_rows, lead + w + pad],
    their conversion by nv12_ref, numpy uint8 [n,h,w,3])."""
    rng = np.random.default_rng(seed)
    rows = h // 2 * 3
    buf = rng.integers(0, 256, (n, rows + gap_rows, lead + w + pad), dtype=np.uint8)
    for f in buf:
        f[:rows, lead:lead + w] = N.random_nv12(rng, h, w)
    ref = np.stack([N.nv12_to_bgr(np.ascontiguousarray(f[:rows, lead:lead + w])) for f in buf], 0)
    return T(buf).to(dev)[:, :rows, lead:lead + w], ref


def _fenced(dev, n, h, w, gap=0):
    """-> (buffer, its view [n,h,w,3] with `gap` bytes between frames), canaries of GUARD bytes either side, everything FILL"""
    fs = h * w * 3 + gap
    buf = torch.full((GUARD + n * fs + GUARD,), FILL, dtype=torch.uint8, device=dev)
    return buf, buf[GUARD:GUARD + n * fs].view(n, fs)[:, :h * w * 3].view(n, h, w, 3)


def _intact(buf, out, what):
    """Only `out`'s own bytes differ from FILL-or-result: the canaries and the gaps between frames keep their fill."""
    n, h, w, _ = out.shape
    fs = out.stride(0) if n > 1 else h * w * 3
    body = buf[GUARD:GUARD + n * fs].view(n, fs)
    assert bool((buf[:GUARD] == FILL).all()) and bool((buf[GUARD + n * fs:] == FILL).all()), (what, 'a canary was overwritten')
    assert bool((body[:, h * w * 3:] == FILL).all()), (what, 'a gap was written')


def _equal(got, ref, what):
    assert got.dtype == torch.uint8 and tuple(got.shape) == tuple(ref.shape), (what, got.dtype, got.shape, ref.shape)
    assert np.array_equal(got.cpu().numpy(), ref), what


# ================================================================================================ the kernel
# (h, w), pad: (12, 16) the aligned path, (14, 18) the fallback by width, pad 14 the fallback by pitch, pad 16 aligned again,
# (10, 264) more than one workgroup along x (32 threads x 8 pixels) plus an aligned tail, (10, 260) the fallback at that width
SIZES = [((2, 2), 0), ((12, 16), 0), ((14, 18), 0), ((12, 16), 14), ((12, 16), 16), ((10, 264), 0), ((10, 260), 0)]


@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('size,pad', SIZES, ids=['%dx%d+%d' % (s[0], s[1], p) for s, p in SIZES])
def test_converter_equals_numpy(dev, size, pad, n):
    from stabstitch2_amd import ops
    h, w = size
    nv, ref = _case(dev, 1000 + 7 * h + w + pad + n, n, h, w, pad)
    assert nv.stride(1) == w + pad
    if h * w >= 2000:
        assert int(nv[:, :h].min()) < 16 and int(nv[:, h:].max()) > 240            # luma below black, chroma beyond the range
    buf, out = _fenced(dev, n, h, w)
    res = ops.nv12_to_bgr(nv, out=out)
    assert res.data_ptr() == out.data_ptr()
    _equal(out, ref, 'batch')
    _intact(buf, out, 'batch')
    _equal(ops.nv12_to_bgr(nv), ref, 'fresh output')
    _equal(ops.nv12_to_bgr(nv[n - 1]), ref[n - 1], 'one frame')                     # [h*3/2, w] -> [h, w, 3]
    _equal(ops.nv12_to_bgr(list(nv.unbind(0))), ref, 'a list of its frames')


@pytest.mark.parametrize('size', [(12, 16), (10, 264)], ids=['12x16', '10x264'])
def test_converter_variants(dev, size):
    """A frame gap; three surfaces with three pitches, one of them unaligned; columns that start 2 bytes into a buffer; an out_stride
    with a gap, aligned and not."""
    from stabstitch2_amd import ops
    h, w = size
    nv, ref = _case(dev, 50 + w, 3, h, w, 8, gap_rows=5)                            # frames 5 rows apart
    assert nv.stride(0) == (h // 2 * 3 + 5) * (w + 8)
    _equal(ops.nv12_to_bgr(nv), ref, 'a frame gap')
    parts = [_case(dev, 60 + w + p, 1, h, w, p) for p in (0, 8, 14)]                  # pitches w, w + 8, w + 14 (not a multiple of 8)
    surf = [p[0][0] for p in parts]
    assert [s.stride(0) for s in surf] == [w, w + 8, w + 14]
    buf, out = _fenced(dev, 3, h, w)
    ops.nv12_to_bgr(surf, out=out)
    _equal(out, np.concatenate([p[1] for p in parts], 0), 'three pitches')
    _intact(buf, out, 'three pitches')
    nv2, ref2 = _case(dev, 70 + w, 2, h, w, 6, lead=2)                              # the pointers are 2-byte aligned only
    assert nv2.data_ptr() % 8 == 2 and nv2.stride(1) % 8 == 0
    _equal(ops.nv12_to_bgr(nv2), ref2, 'columns from byte 2')
    for gap in (40, 42):                                                            # out_stride % 8 == 0, and not
        buf, out = _fenced(dev, 3, h, w, gap=gap)
        assert out.stride(0) == 3 * h * w + gap
        ops.nv12_to_bgr(nv, out=out)
        _equal(out, ref, ('out_stride gap', gap))
        _intact(buf, out, ('out_stride gap', gap))


def test_a_refused_call_is_a_value_error_and_launches_nothing(dev):
    """The binding's one path the CPU tests cannot reach (tests/test_native_binding.py has the others): real device pointers and a
    real stream through _surfaces.call, SSF_ERR_ARG mapped to ValueError with `out` untouched -- then the same call with the right
    count.  4 x 8 with pitch 16: the smallest geometry ssf_nv12_to_bgr takes on its aligned path."""
    import ctypes
    from stabstitch2_amd import _hip, _surfaces, ops
    h, w = 4, 8
    nv, ref = _case(dev, 77, 2, h, w, 8)
    surf = list(nv.unbind(0))
    assert [s.stride(0) for s in surf] == [16, 16]
    buf, out = _fenced(dev, 2, h, w)
    ys = (ctypes.c_void_p * 2)(*[s.data_ptr() for s in surf])
    uvs = (ctypes.c_void_p * 2)(*[s.data_ptr() + h * s.stride(0) for s in surf])
    pitches = (ctypes.c_int * 2)(16, 16)
    ys.dev = nv.device.index

    def convert(n):
        _surfaces.call('ssf_nv12_to_bgr', ys, uvs, pitches, n, h, w, _hip.dptr(out, dtype=torch.uint8), 3 * h * w, _hip.stream())

    with pytest.raises(ValueError, match='^ssf_nv12_to_bgr refused its arguments$'):
        convert(0)
    torch.cuda.synchronize(dev)
    assert bool((buf == FILL).all())
    convert(2)
    _equal(out, ref, 'the same call with n = 2')
    assert torch.equal(out, ops.nv12_to_bgr(surf))
    _intact(buf, out, 'n = 2')


def _ours(names):
    return [k for k in names if re.search(r'\bsf_[a-z]+_kernel', k)]


def test_96_surfaces_in_one_launch_and_97_in_two(dev):
    from stabstitch2_amd import ops
    from test_gpu_linear_frames import _kernel_names
    h, w = 4, 8
    nv, ref = _case(dev, 9, 97, h, w, 0)
    ops.nv12_to_bgr(nv[:1])                      # (module load outside the profiler)
    for n, launches in ((96, 1), (97, 2)):
        surf = list(nv[:n].unbind(0))
        buf, out = _fenced(dev, n, h, w)
        _, names = _kernel_names(lambda: ops.nv12_to_bgr(surf, out=out))
        assert len(_ours(names)) == launches and len(names) == launches, names
        _equal(out, ref[:n], n)
        _intact(buf, out, n)
    _equal(ops.nv12_to_bgr(nv), ref, 'a batch of 97')


def test_launch_witness(dev):
    """The smallest aligned and unaligned calls launch the two instantiations and nothing else of this library, one launch each.
    Should the profiler report names without template arguments, base names are matched instead and the test says so."""
    from stabstitch2_amd import ops
    from test_gpu_linear_frames import _kernel_names
    launched = []
    for w in (8, 2):                             # (2, 8): one aligned thread; (2, 2): one 2 x 2 block
        nv, ref = _case(dev, 3 + w, 1, 2, w, 0)
        ops.nv12_to_bgr(nv)
        res, names = _kernel_names(lambda: ops.nv12_to_bgr(nv))
        assert len(names) == 1 and len(_ours(names)) == 1, names
        _equal(res, ref, w)
        launched += names
    if all('<' in k for k in launched):
        got = [G.instantiation_key(k) for k in launched]
        print('\n[launch witness] matched by template arguments: %s' % got)
        assert got == ['sf_convert_kernel<1>', 'sf_convert_kernel<0>'], got
    else:
        print('\n[launch witness] the profiler reports no template arguments; matched by base name: %s' % launched)
        assert all(re.search(r'\bsf_convert_kernel', k) for k in launched)


def test_out_crosses_byte_2_31_inside_a_surface(dev):
    """Three surfaces of 16384 x 16384 in one call: `out` is 2.4 GB and byte 2^31 lies inside surface 2, whose offset
    surface * out_stride a 32-bit product would wrap.  Surface 2 equals the same entry on that surface alone, bit for bit; no two
    surfaces are equal, so a wrapped offset shows.  About 4.4 GB of buffers, compared on the device; fails (no skip) when memory is short."""
    from stabstitch2_amd import ops
    h = w = 16384
    frame = 3 * h * w
    assert 2 * frame < (1 << 31) < 3 * frame
    gc.collect()
    torch.cuda.empty_cache()
    need = 3 * (h // 2 * 3) * w + 4 * frame + (256 << 20)
    free, _ = torch.cuda.mem_get_info()
    assert free >= need, 'needs %d bytes of device memory, %d are free' % (need, free)
    gen = torch.Generator(device=dev).manual_seed(5)
    surf = [torch.randint(0, 256, (h // 2 * 3, w), dtype=torch.uint8, device=dev, generator=gen) for _ in range(3)]
    out = ops.nv12_to_bgr(surf)
    assert tuple(out.shape) == (3, h, w, 3) and out.stride(0) == frame
    for s in (2, 0):
        alone = ops.nv12_to_bgr(surf[s])
        assert torch.equal(out[s], alone), ('surface', s)
        if s == 2:
            assert not torch.equal(out[0], alone)
        del alone
    # the small frames' statement holds the large call's first rows to numpy
    for s in range(3):
        ref = N.nv12_to_bgr(torch.cat((surf[s][:2], surf[s][h:h + 1]), 0).cpu().numpy())      # rows 0, 1 and their chroma row: a 2-row frame
        assert np.array_equal(out[s, :2].cpu().numpy(), ref), s
    del out, surf
    gc.collect()
    torch.cuda.empty_cache()


# ================================================================================================ the routes
NF = 14                                      # frames of the clip: calls of (4, 5, 3) use twelve, HostFrameStream's groups all
_cache = {}


def _clip(dev):
    """test_gpu_nv12's clip, NF frames long: -> (NV12 frames numpy [3][NF] of [SH*3/2, SW], their packed BGR on the device)."""
    if 'clip' not in _cache:
        hr, _ = synth.make_clip_device(NF, SH, SW, seed=4, views=3, device=dev)
        u8 = hr.permute(0, 1, 3, 4, 2).round().clamp(0, 255).to(torch.uint8).cpu().numpy()
        nv = [[N.bgr_to_nv12(u8[v, t]) for t in range(NF)] for v in range(3)]
        bgr = [torch.stack([T(N.nv12_to_bgr(f)) for f in per]).to(dev) for per in nv]
        _cache['clip'] = (nv, bgr)
    return _cache['clip']


def _dense(dev, per, a, b):
    return T(np.stack(per[a:b], 0)).to(dev)


def _padded(dev, per, a, b):
    """A list of surfaces, every one a view of its own wider buffer: pitches SW + PAD, SW + PAD + 2, .."""
    return [_surface(dev, np.concatenate((f, np.full((f.shape[0], PAD + 2 * i), 0x5A, np.uint8)), 1), SW) for i, f in enumerate(per[a:b])]


def _same_frames(got, ref, out, what):
    assert len(got) == len(ref), (what, len(got), len(ref))
    for i, (a, b) in enumerate(zip(got, ref)):
        if out == 'bgr':
            assert a.shape == b.shape and a.dtype == torch.uint8 and torch.equal(a, b), (what, i)
        else:
            hc, wc = b.shape[:2]
            assert tuple(a.shape) == (hc // 2 * 3, wc) and a.dtype == torch.uint8, (what, i, a.shape)
            assert np.array_equal(a.cpu().numpy(), N.bgr_to_nv12(b.cpu().numpy())), (what, i)


CALLS = ((0, 4), (4, 9), (9, 12))            # the window fills inside the second call; then one batched call more
CONFIGS = [('two', 'NORMAL', 'AVERAGE', {}), ('two', 'FAST', 'LINEAR', {}), ('two', 'NORMAL', 'MULTIBAND', dict(seam='dp')),
           ('three', 'NORMAL', 'AVERAGE', {})]


@pytest.mark.parametrize('cls,warp,fusion,extra', CONFIGS, ids=['%s-%s-%s' % c[:3] for c in CONFIGS])
def test_push_many_nv12_equals_push_many_u8_of_the_converted_frames(dev, hip_nets, cls, warp, fusion, extra):
    """Calls of (4, 5, 3) frames: out='bgr' hands out push_many_u8's frames of the converted input byte for byte, out='nv12' their
    numpy BGR -> NV12 as views of one tensor, with push_many_u8's cadence, batch graphs and captures.  One stitcher takes dense
    batches, lists of padded surfaces, dense batches with the formats bgr, nv12, bgr; the other the opposite choices."""
    from stabstitch2_amd import online
    views = 2 if cls == 'two' else 3
    Cls = online.OnlineStitcher if cls == 'two' else online.ThreeViewOnlineStitcher
    mk = lambda: Cls(hip_nets, SH, SW, warp_mode=warp, fusion_mode=fusion, viewport=VIEWPORTS[views], **extra)      # noqa: E731
    nv, bgr = _clip(dev)
    ref_st = mk()
    ref = [ref_st.push_many_u8(*[b[a:e] for b in bgr[:views]]) for a, e in CALLS]
    assert [len(r) for r in ref] == [0, 9, 3] and ref_st.batch_captures == 2 and sorted(ref_st.graph_nodes_batch) == [2, 3]
    for first in (0, 1):
        st = mk()
        for c, (a, e) in enumerate(CALLS):
            form, out = (_dense, 'bgr') if (c + first) % 2 == 0 else (_padded, 'nv12')
            got = st.push_many_nv12(*[form(dev, per, a, e) for per in nv[:views]], out=out)
            _same_frames(got, ref[c], out, (first, c))
            if out == 'nv12' and got:
                base = got[0].untyped_storage().data_ptr()
                assert all(g.untyped_storage().data_ptr() == base for g in got)          # views of one tensor
        assert st.frames_in == ref_st.frames_in == 12
        assert st.graph_nodes_batch == ref_st.graph_nodes_batch and st.batch_captures == ref_st.batch_captures


def test_push_many_nv12_on_an_exposure_stitcher(dev, hip_nets):
    from stabstitch2_amd import online
    nv, bgr = _clip(dev)
    mk = lambda: online.OnlineStitcher(hip_nets, SH, SW, viewport=VIEWPORTS[2], exposure=True)      # noqa: E731
    ref_st, st = mk(), mk()
    for c, (a, e) in enumerate(CALLS):
        ref = ref_st.push_many_u8(bgr[0][a:e], bgr[1][a:e])
        out = ('bgr', 'nv12', 'bgr')[c]
        got = st.push_many_nv12(_dense(dev, nv[0], a, e), _padded(dev, nv[1], a, e), out=out)
        _same_frames(got, ref, out, c)
        assert torch.equal(st.exposure_gains, ref_st.exposure_gains), c
    with pytest.raises(ValueError, match='exposure'):                # the single-frame entry stays refused
        st.push_nv12(_dense(dev, nv[0], 0, 1)[0], _dense(dev, nv[1], 0, 1)[0])
    assert st.frames_in == 12


def test_interleaved_with_push_nv12_and_push_u8(dev, hip_nets):
    """push_many_nv12, push_nv12 and push_u8 on one stitcher == the same sequence all in BGR; push_nv12 launches nothing of the new
    library (it samples the surfaces itself)."""
    from stabstitch2_amd import online
    from test_gpu_linear_frames import _kernel_names
    nv, bgr = _clip(dev)
    mk = lambda: online.OnlineStitcher(hip_nets, SH, SW, viewport=VIEWPORTS[2])      # noqa: E731
    ref_st, st = mk(), mk()
    one = lambda t: [_dense(dev, nv[v], t, t + 1)[0] for v in range(2)]              # noqa: E731
    seq = [('many', 0, 4), ('nv12', 4, 5), ('nv12', 5, 6), ('nv12', 6, 7), ('u8', 7, 8), ('many', 8, 11), ('nv12', 11, 12),
           ('many', 12, 14)]
    names = None
    for kind, a, e in seq:
        if kind == 'many':
            ref = ref_st.push_many_u8(bgr[0][a:e], bgr[1][a:e])
            got = st.push_many_nv12(_padded(dev, nv[0], a, e), _dense(dev, nv[1], a, e))
        elif kind == 'u8':
            ref, got = ref_st.push_u8(bgr[0][a], bgr[1][a]), st.push_u8(bgr[0][a], bgr[1][a])
        else:
            ref = ref_st.push_u8(bgr[0][a], bgr[1][a])
            if a == 11:
                got, names = _kernel_names(lambda: st.push_nv12(*one(a)))
            else:
                got = st.push_nv12(*one(a))
        _same_frames(got, ref, 'bgr', (kind, a))
    assert names and not _ours(names), names
    assert st.frames_in == ref_st.frames_in == NF and st.graph_nodes == ref_st.graph_nodes


@pytest.mark.parametrize('canvases', ['viewport', 'two sizes'])
def test_multi_push_nv12_equals_push_u8_of_the_converted_frames(dev, hip_nets, canvases):
    """Two streams (views 0, 1 and views 1, 2 of the clip), nine pushes: canvases of one size (a viewport; the output format changes
    from push to push) and canvases of two sizes."""
    from stabstitch2_amd import online
    nv, bgr = _clip(dev)
    kw = dict(viewport=VIEWPORTS[2]) if canvases == 'viewport' else dict(canvases=[(-10.0, 470.0, -8.0, 190.0), (-20.0, 480.0, -5.0, 188.0)])
    mk = lambda: online.MultiOnlineStitcher(hip_nets, SH, SW, streams=2, **kw)      # noqa: E731
    ref_st, st = mk(), mk()
    for t in range(9):
        ref = ref_st.push_u8(torch.stack((bgr[0][t], bgr[1][t])), torch.stack((bgr[1][t], bgr[2][t])))
        out = 'nv12' if canvases == 'viewport' and t % 2 == 0 else 'bgr'
        if t % 2:
            f1, f2 = _dense(dev, [nv[0][t], nv[1][t]], 0, 2), _dense(dev, [nv[1][t], nv[2][t]], 0, 2)
        else:
            f1, f2 = _padded(dev, [nv[0][t], nv[1][t]], 0, 2), _padded(dev, [nv[1][t], nv[2][t]], 0, 2)
        got = st.push_nv12(f1, f2, out=out)
        assert len(got) == len(ref) == 2
        for s in range(2):
            _same_frames(got[s], ref[s], out, (t, s))
    assert [len(r) for r in ref] == [1, 1] and st.graph_nodes == ref_st.graph_nodes
    sizes = st.canvas_sizes
    assert sizes == ref_st.canvas_sizes and (sizes[0] == sizes[1]) == (canvases == 'viewport'), sizes


def _host(per_view, frames):
    """-> the source of a HostFrameStream: per frame a tuple of pinned host frames, one per view"""
    return [tuple((T(v[t]) if isinstance(v[t], np.ndarray) else v[t].cpu()).pin_memory() for v in per_view) for t in range(frames)]


@pytest.mark.parametrize('out', ['bgr', 'nv12'])
@pytest.mark.parametrize('cls', ['two', 'three'])
def test_host_stream_nv12_equals_a_push_nv12_loop(dev, hip_nets, cls, out):
    """frame_format='nv12' (upload, the converter, push_u8) against the native NV12 route, nine frames."""
    from stabstitch2_amd import online
    views = 2 if cls == 'two' else 3
    Cls = online.OnlineStitcher if cls == 'two' else online.ThreeViewOnlineStitcher
    nv, _ = _clip(dev)
    ref_st = Cls(hip_nets, SH, SW, viewport=VIEWPORTS[views])
    ref = [f for t in range(9) for f in ref_st.push_nv12(*[T(nv[v][t]).to(dev) for v in range(views)], out=out)]
    runner = online.HostFrameStream(Cls(hip_nets, SH, SW, viewport=VIEWPORTS[views]), frame_format='nv12', out=out)
    got = [f.clone() for f in runner.run(_host(nv[:views], 9))]
    torch.cuda.synchronize()
    assert len(got) == len(ref) == 9
    hc, wc = VIEWPORTS[views]
    for i, (a, b) in enumerate(zip(got, ref)):
        assert not a.is_cuda and tuple(a.shape) == ((hc, wc, 3) if out == 'bgr' else (hc // 2 * 3, wc))
        assert torch.equal(a, b.cpu()), (cls, out, i)


def test_host_stream_nv12_over_a_pipelined_stitcher(dev, hip_nets):
    from stabstitch2_amd import online
    nv, bgr = _clip(dev)
    mk = lambda: online.PipelinedOnlineStitcher(hip_nets, SH, SW, viewport=VIEWPORTS[2])      # noqa: E731
    ref = [f.clone() for f in online.HostFrameStream(mk()).run(_host(bgr[:2], 10))]
    for out in ('bgr', 'nv12'):
        got = [f.clone() for f in online.HostFrameStream(mk(), frame_format='nv12', out=out).run(_host(nv[:2], 10))]
        torch.cuda.synchronize()
        assert len(ref) == 10
        _same_frames(got, ref, out, out)


def test_host_stream_batch_equals_push_many_u8_of_the_same_groups(dev, hip_nets):
    """batch=4 over 14 frames: groups of 4, 4, 4, 2."""
    from stabstitch2_amd import online
    nv, bgr = _clip(dev)
    ref_st = online.OnlineStitcher(hip_nets, SH, SW)
    ref = [f for a in range(0, NF, 4) for f in ref_st.push_many_u8(bgr[0][a:a + 4], bgr[1][a:a + 4])]
    st = online.OnlineStitcher(hip_nets, SH, SW)
    got = [f.clone() for f in online.HostFrameStream(st, batch=4).run(_host(bgr[:2], NF))]
    torch.cuda.synchronize()
    assert len(ref) == NF and (st.hc, st.wc) == (ref_st.hc, ref_st.wc)
    _same_frames([g.to(dev) for g in got], ref, 'bgr', 'batch=4')
    assert st.graph_nodes_batch == ref_st.graph_nodes_batch and st.batch_captures == ref_st.batch_captures == 3
    # three views, NV12 both ways
    ref3 = online.ThreeViewOnlineStitcher(hip_nets, SH, SW, viewport=VIEWPORTS[3])
    ref = [f for a in range(0, NF, 4) for f in ref3.push_many_u8(*[b[a:a + 4] for b in bgr])]
    run3 = online.HostFrameStream(online.ThreeViewOnlineStitcher(hip_nets, SH, SW, viewport=VIEWPORTS[3]), batch=4, frame_format='nv12',
                                  out='nv12')
    got = [f.clone() for f in run3.run(_host(nv, NF))]
    torch.cuda.synchronize()
    _same_frames([g.to(dev) for g in got], ref, 'nv12', 'three views, batch=4, NV12')


def test_host_stream_batch_is_batch_one_when_deterministic_and_keeps_its_promise(dev, hip_nets):
    """deterministic=True stitchers: batch=4 == batch=1, over 30 frames (the clip twice and two frames more), NV12 in and out.  The
    batched run has depth=1, so its pinned ring (2 depth + batch + 8 = 14 tensors) wraps twice: a tensor yielded `depth` frames
    earlier is unchanged whenever a later one arrives, and when the run ends."""
    from stabstitch2_amd import online
    nv, _ = _clip(dev)
    order = list(range(NF)) * 2 + [0, 1]
    source = _host([[per[t] for t in order] for per in nv[:2]], len(order))
    mk = lambda: online.OnlineStitcher(hip_nets, SH, SW, viewport=VIEWPORTS[2], deterministic=True)      # noqa: E731
    ref = [f.clone() for f in online.HostFrameStream(mk(), frame_format='nv12', out='nv12').run(source)]
    depth = 1
    runner = online.HostFrameStream(mk(), depth=depth, batch=4, frame_format='nv12', out='nv12')
    held, got = [], []
    for f in runner.run(source):
        held.append(f)
        got.append(f.clone())
        for i in range(max(0, len(held) - 1 - depth), len(held)):
            assert torch.equal(held[i], got[i]), ('overwritten', i, len(held))
    assert len(got) == len(ref) == len(order)
    assert len({h.data_ptr() for h in held}) == 2 * depth + 4 + 8 < len(order)          # the ring did wrap
    for i in range(len(held) - 1 - depth, len(held)):
        assert torch.equal(held[i], got[i]), ('overwritten at the end', i)
    for i, (a, b) in enumerate(zip(got, ref)):
        assert torch.equal(a, b), i
