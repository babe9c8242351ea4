"""ctypes binding of libstabstitch_hip.so (the C ABI declared in include/stabstitch_hip.h).

There is no CPU fallback: if the shared library is missing or a tensor is not a contiguous fp32
CUDA(HIP) tensor, the call raises.  PyTorch is used only for device memory and streams.
"""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))

# The native libraries, in the order they were added: the names of their binding modules in this package.  Each module describes its
# library with LIB_PATH, HEADER (under include/), API (the macro in front of a declaration), PREFIX (of every exported symbol) and
# SIGNATURES, and has lib() and call().  The build, its surface check and the tests go over this list ("Adding a native
# library").
LIBRARIES = ('_hip', '_blend', '_seam', '_mbwarp', '_surfaces')
# Libraries behind a path that the five above also cover (the same description, the same loader and launch path): the build and its
# surface check go over them too.  _smoothtail: SmoothNet's Conv3d stack of a stitched clip.
EXTRA_LIBRARIES = ('_smoothtail',)
# Libraries of features added since (what the renders do not change for): the tuple a later library's module goes to.  The two above
# are pinned by their tests.  _cover: coverage bitmaps and the largest fully covered rectangle.
FEATURE_LIBRARIES = ('_cover',)
# That tuple is pinned by its test as well (tests/test_cover_abi.py), so this is the open one: a later library's module goes to ITS
# end, and its test asserts membership, not equality.  _resample: fixed-size antialiased output of the covered rectangle.
LATER_LIBRARIES = ('_resample',)


def all_libraries():
    """Every native library's binding module name, oldest first: what the build compiles and its surface check goes over."""
    return LIBRARIES + EXTRA_LIBRARIES + FEATURE_LIBRARIES + LATER_LIBRARIES

LIB_PATH = os.path.join(_HERE, 'libstabstitch_hip.so')
HEADER, API, PREFIX = 'stabstitch_hip.h', 'SS_API', 'ss_'
ERR_ARG = -1                  # SS?_ERR_ARG of every side library's header: `check_side` makes it a ValueError

c_fp = ctypes.c_void_p        # device pointer
c_i = ctypes.c_int
c_f = ctypes.c_float
c_ll = ctypes.c_longlong
c_st = ctypes.c_void_p        # hipStream_t

# the bits of the renders' `mode` argument, as the header defines them
MODE_FLAGS = {'SS_WARP_NORMAL': 0, 'SS_WARP_FAST': 1, 'SS_WARP_EPS_FOLD': 16, 'SS_FUSE_FEATHER': 32}

# name -> (restype, argtypes); mirrors include/stabstitch_hip.h one to one
SIGNATURES = {
    'ss_version': (c_i, []),
    'ss_error_string': (ctypes.c_char_p, [c_i]),
    'ss_nchw_to_nhwc': (c_i, [c_fp, c_fp, c_i, c_i, c_i, c_i, c_i, c_st]),
    'ss_nhwc_to_nchw': (c_i, [c_fp, c_fp, c_i, c_i, c_i, c_i, c_i, c_st]),
    'ss_conv_workspace_need': (c_ll, [c_i] * 14),
    'ss_conv_nhwc': (c_i, [c_fp, c_fp, c_fp, c_fp, c_fp] + [c_i] * 15 + [c_i, c_ll, c_ll, c_ll, c_fp, c_ll, c_st]),
    'ss_conv_pool2_nhwc': (c_i, [c_fp, c_fp, c_fp, c_fp] + [c_i] * 13 + [c_ll, c_ll, c_ll, c_fp, c_ll, c_st]),
    'ss_nchw_to_nhwc3_padded': (c_i, [c_fp, c_fp, c_i, c_i, c_i, c_st]),
    'ss_conv_stem3': (c_i, [c_fp, c_fp, c_fp, c_fp] + [c_i] * 7 + [c_ll] * 3 + [c_st]),
    'ss_stem_pool_packed_floats': (c_ll, [c_i]),
    'ss_stem_pool_pack': (c_i, [c_fp, c_fp, c_i, c_st]),
    'ss_stem_pool': (c_i, [c_fp, c_fp, c_fp, c_fp, c_i, c_i, c_i, c_i, c_ll, c_st]),
    'ss_wino_packed_floats': (c_ll, [c_i, c_i]),
    'ss_wino_packed3_floats': (c_ll, [c_i, c_i]),
    'ss_wino_pack': (c_i, [c_fp, c_fp, c_i, c_i, c_i, c_st]),
    'ss_wino_pack3': (c_i, [c_fp, c_fp, c_i, c_i, c_i, c_st]),
    'ss_conv_uses_winograd': (c_i, [c_i] * 9),
    'ss_conv3x3_wino_nhwc': (c_i, [c_fp] * 5 + [c_i] * 8 + [c_ll] * 3 + [c_st]),
    'ss_conv3x3_wino3_nhwc': (c_i, [c_fp] * 5 + [c_i] * 8 + [c_ll] * 3 + [c_st]),
    'ss_wino43_packed_floats': (c_ll, [c_i, c_i]),
    'ss_conv_uses_wino43': (c_i, [c_i] * 13),
    'ss_wino43_pack': (c_i, [c_fp, c_fp, c_i, c_i, c_i, c_st]),
    'ss_conv3x3_wino43_nhwc': (c_i, [c_fp] * 5 + [c_i] * 8 + [c_ll] * 3 + [c_st]),
    'ss_conv3x3_wino_pool2_nhwc': (c_i, [c_fp] * 4 + [c_i] * 8 + [c_ll] * 3 + [c_st]),
    'ss_maxpool_nhwc': (c_i, [c_fp, c_fp] + [c_i] * 7 + [c_st]),
    'ss_maxpool_nhwc_split': (c_i, [c_fp, c_fp, c_fp] + [c_i] * 7 + [c_st]),
    'ss_linear': (c_i, [c_fp, c_fp, c_fp, c_fp, c_i, c_i, c_i, c_i, c_st]),
    'ss_linear_grouped': (c_i, [c_fp, c_ll, c_fp, c_fp, ctypes.POINTER(c_fp), c_i, c_i, c_i, c_i, c_i, c_st]),
    'ss_ccl_workspace_floats': (c_ll, [c_i, c_i, c_i, c_i]),
    'ss_ccl': (c_i, [c_fp, c_fp, c_fp, c_fp, c_i, c_i, c_i, c_i, c_f, c_fp, c_st]),
    'ss_l2norm_nhwc': (c_i, [c_fp, c_fp, c_ll, c_i, c_st]),
    'ss_cost_volume': (c_i, [c_fp, c_fp, c_fp, c_i, c_i, c_i, c_i, c_i, c_i, c_st]),
    'ss_cost_volume_bidir': (c_i, [c_fp, c_fp, c_fp, c_i, c_i, c_i, c_i, c_i, c_i, c_st]),
    'ss_cost_volume_shifted': (c_i, [c_fp, c_fp, c_fp] + [c_i] * 8 + [c_st]),
    'ss_cost_volume_chain_frames': (c_i, [c_fp, c_fp] + [c_i] * 7 + [c_st]),
    'ss_cost_volume_set_tile': (c_i, [c_i]),
    'ss_wino43_set_persistent': (c_i, [c_i]),
    'ss_tensor_dlt': (c_i, [c_fp, c_fp, c_fp, c_i, c_st]),
    'ss_spatial_decompose': (c_i, [c_fp, c_fp, c_fp, c_i, c_f, c_f, c_st]),
    'ss_spatial_meshes': (c_i, [c_fp, c_fp, c_fp, c_fp, c_fp, c_i, c_f, c_f, c_st]),
    'ss_homo_warp_nhwc': (c_i, [c_fp, c_fp, c_fp, c_i, c_i, c_i, c_i, c_i, c_i, c_st]),
    'ss_homo_warp_pair_nhwc': (c_i, [c_fp, c_fp, c_fp, c_fp, c_i, c_i, c_i, c_i, c_i, c_i, c_st]),
    'ss_homo_warp_nchw': (c_i, [c_fp, c_fp, c_fp, c_i, c_i, c_i, c_i, c_i, c_i, c_st]),
    'ss_tps_solve': (c_i, [c_fp, c_fp, c_fp, c_i, c_st]),
    'ss_tps_solve_shared_target': (c_i, [c_fp, c_fp, c_fp, c_i, c_st]),
    'ss_tps_points': (c_i, [c_fp, c_fp, c_fp, c_fp, c_i, c_i, c_st]),
    'ss_tsmotion_workspace_floats': (c_ll, [c_i]),
    'ss_tps_inverse': (c_i, [c_fp, c_fp, c_st]),
    'ss_tsmotion': (c_i, [c_fp, c_fp, c_fp, c_fp, c_i, c_f, c_f, c_fp, c_fp, c_st]),
    'ss_tsmotion_lag': (c_i, [c_fp, c_fp, c_fp, c_fp, c_i, c_i, c_f, c_f, c_fp, c_fp, c_st]),
    'ss_tps_warp_nchw': (c_i, [c_fp, c_fp, c_fp, c_fp] + [c_i] * 7 + [c_st]),
    'ss_tps_warp_mask_nchw': (c_i, [c_fp, c_fp, c_fp, c_fp] + [c_i] * 7 + [c_st]),
    'ss_tps_warp_views': (c_i, [ctypes.POINTER(c_fp), c_fp, c_fp, c_fp] + [c_i] * 6 + [c_st]),
    'ss_add_mul': (c_i, [c_fp, c_fp, c_f, c_f, c_ll, c_st]),
    'ss_mask_union': (c_i, [c_fp, c_fp, c_fp, c_ll, c_st]),
    'ss_ingest_u8': (c_i, [c_fp, c_fp, c_fp, c_i, c_i, c_i, c_i, c_i, c_st]),
    'ss_canvas_to_u8': (c_i, [c_fp, c_fp, c_i, c_i, c_i, c_st]),
    'ss_ingest_nv12': (c_i, [c_fp, c_fp, c_i, c_ll, c_fp, c_fp, c_i, c_i, c_i, c_i, c_i, c_st]),
    'ss_bgr_to_nv12': (c_i, [c_fp, c_fp, c_fp, c_i, c_ll, c_i, c_i, c_i, c_st]),
    'ss_render_average': (c_i, [ctypes.POINTER(c_fp), c_fp, c_fp, c_fp, c_ll, c_fp] + [c_i] * 6 + [c_st]),
    'ss_render_average_u8': (c_i, [ctypes.POINTER(c_fp), c_fp, c_fp, c_fp, c_ll, c_fp] + [c_i] * 6 + [c_st]),
    'ss_render_average_nv12': (c_i, [ctypes.POINTER(c_fp), ctypes.POINTER(c_fp), ctypes.POINTER(c_i), c_fp, c_fp, c_fp, c_ll, c_fp, c_fp] +
                               [c_i] * 8 + [c_st]),
    'ss_render_average_clip': (c_i, [ctypes.POINTER(c_fp), c_fp, c_fp, c_fp, c_ll, c_fp] + [c_i] * 7 + [c_st]),
    'ss_render_average_clip_u8': (c_i, [ctypes.POINTER(c_fp), c_fp, c_fp, c_fp, c_ll, c_fp] + [c_i] * 7 + [c_st]),
    'ss_render_footprint_floats': (c_ll, [c_i, c_i, c_i]),
    'ss_render_footprints': (c_i, [c_fp, c_fp, c_fp] + [c_i] * 6 + [c_st]),
    'ss_render_footprints_watch': (c_i, [c_fp, c_fp, c_fp] + [c_i] * 6 + [c_f, c_fp, c_fp, c_st]),
    'ss_render_footprints_watch_fit': (c_i, [c_fp, c_fp, c_fp] + [c_i] * 6 + [c_f, c_fp, c_fp, c_fp, c_fp, c_fp, c_f, c_f, c_st]),
    'ss_linear_blend_workspace_floats': (c_ll, [c_i, c_i]),
    'ss_linear_blend': (c_i, [c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, c_i, c_i, c_fp, c_st]),
    'ss_linear_clip_workspace_floats': (c_ll, [c_i, c_i, c_i, c_i]),
    'ss_linear_clip_set_rows': (c_i, [c_i]),
    'ss_render_linear_clip': (c_i, [ctypes.POINTER(c_fp), c_fp, c_fp, c_fp, c_fp] + [c_i] * 7 + [c_fp, c_st]),
    'ss_render_linear_clip_u8': (c_i, [ctypes.POINTER(c_fp), c_fp, c_fp, c_fp, c_fp] + [c_i] * 7 + [c_fp, c_st]),
    'ss_linear_frames_workspace_floats': (c_ll, [c_i, c_i, ctypes.POINTER(c_i), ctypes.POINTER(c_i)]),
    'ss_render_linear_frames': (c_i, [ctypes.POINTER(c_fp), c_fp, c_fp, ctypes.POINTER(c_fp)] + [c_i] * 4 +
                                [ctypes.POINTER(c_i), ctypes.POINTER(c_i), c_i, c_fp, c_st]),
    'ss_render_linear_frames_u8': (c_i, [ctypes.POINTER(c_fp), c_fp, c_fp, ctypes.POINTER(c_fp)] + [c_i] * 4 +
                                   [ctypes.POINTER(c_i), ctypes.POINTER(c_i), c_i, c_fp, c_st]),
    'ss_render_linear_frames_nv12': (c_i, [ctypes.POINTER(c_fp), ctypes.POINTER(c_fp), ctypes.POINTER(c_i), ctypes.POINTER(c_ll), c_fp, c_fp,
                                           ctypes.POINTER(c_fp)] + [c_i] * 4 + [ctypes.POINTER(c_i), ctypes.POINTER(c_i), c_i, c_fp, c_st]),
    'ss_exposure_update': (c_i, [ctypes.POINTER(c_fp), c_i, c_ll, c_fp, c_ll, c_ll] + [c_i] * 7 + [c_f] * 5 + [c_i, c_f, c_f, c_fp, c_fp,
                                 c_fp, c_st]),
    'ss_render_average_gains': (c_i, [ctypes.POINTER(c_fp), c_fp, c_fp, c_fp, c_ll, c_fp] + [c_i] * 6 + [c_fp, c_st]),
    'ss_render_average_u8_gains': (c_i, [ctypes.POINTER(c_fp), c_fp, c_fp, c_fp, c_ll, c_fp] + [c_i] * 6 + [c_fp, c_st]),
    'ss_render_average_clip_gains': (c_i, [ctypes.POINTER(c_fp), c_fp, c_fp, c_fp, c_ll, c_fp] + [c_i] * 7 + [c_fp, c_st]),
    'ss_render_average_clip_u8_gains': (c_i, [ctypes.POINTER(c_fp), c_fp, c_fp, c_fp, c_ll, c_fp] + [c_i] * 7 + [c_fp, c_st]),
    'ss_render_linear_clip_gains': (c_i, [ctypes.POINTER(c_fp), c_fp, c_fp, c_fp, c_fp] + [c_i] * 7 + [c_fp, c_fp, c_st]),
    'ss_render_linear_clip_u8_gains': (c_i, [ctypes.POINTER(c_fp), c_fp, c_fp, c_fp, c_fp] + [c_i] * 7 + [c_fp, c_fp, c_st]),
    'ss_render_linear_frames_gains': (c_i, [ctypes.POINTER(c_fp), c_fp, c_fp, ctypes.POINTER(c_fp)] + [c_i] * 4 +
                                      [ctypes.POINTER(c_i), ctypes.POINTER(c_i), c_i, c_fp, c_fp, c_st]),
    'ss_render_linear_frames_u8_gains': (c_i, [ctypes.POINTER(c_fp), c_fp, c_fp, ctypes.POINTER(c_fp)] + [c_i] * 4 +
                                         [ctypes.POINTER(c_i), ctypes.POINTER(c_i), c_i, c_fp, c_fp, c_st]),
    'ss_mesh_bbox': (c_i, [c_fp, c_i, c_f, c_f, c_fp, c_i, c_st]),
    'ss_mesh_normalize': (c_i, [c_fp, c_fp, c_fp, c_i, c_f, c_f, c_st]),
    'ss_canvas_watch': (c_i, [c_fp, c_i, c_i, c_f, c_fp, c_fp, c_st]),
    'ss_canvas_watch_frames': (c_i, [c_fp, c_i, c_i, c_f, c_fp, c_fp, c_st]),
    'ss_canvas_watch_fit': (c_i, [c_fp, c_i, c_i, c_f, c_fp, c_fp, c_fp, c_fp, c_fp, c_f, c_f, c_i, c_i, c_st]),
    'ss_canvas_watch_frames_fit': (c_i, [c_fp, c_i, c_i, c_f, c_fp, c_fp, c_fp, c_fp, c_fp, c_f, c_f, c_i, c_i, c_st]),
    'ss_box_fit_aspect': (c_i, [c_fp, c_fp, c_i, c_i, c_i, c_st]),
    'ss_stream_normalize_watch': (c_i, [ctypes.c_void_p, c_i, c_ll, c_fp, c_i, c_fp, c_i, c_f, c_f, c_f, c_fp, c_fp, c_st]),
    'ss_mesh_normalize_views': (c_i, [c_fp, c_fp, c_fp, c_i, c_i, c_i, c_f, c_f, c_st]),
    'ss_mesh_normalize_views_boxes': (c_i, [c_fp, c_ll, c_fp, c_fp, c_i, c_i, c_i, c_f, c_f, c_st]),
    'ss_fill_f32': (c_i, [c_fp, c_f, c_ll, c_st]),
    'ss_h2mesh': (c_i, [c_fp, c_fp, c_fp, c_i, c_i, c_st]),
    'ss_three_view_align': (c_i, [c_fp] * 9 + [c_i, c_f, c_f, c_st]),
    'ss_three_view_finish': (c_i, [c_fp] * 7 + [c_ll, c_st]),
    'ss_three_view_splines': (c_i, [c_fp] * 4 + [c_ll] + [c_fp] * 8 + [c_i, c_f, c_f, c_st]),
    'ss_stream_splines': (c_i, [ctypes.c_void_p, c_i, c_ll, c_fp, c_i, c_fp, c_fp, c_fp, c_i, c_f, c_f, c_st]),
    'ss_three_view_normalize': (c_i, [c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, c_ll, c_st]),
    'ss_smooth_embed': (c_i, [c_fp] * 9 + [c_i] * 4 + [c_st]),
    'ss_smooth_finalize': (c_i, [c_fp] * 13 + [c_i] * 4 + [c_st]),
    'ss_smooth_stitch': (c_i, [c_fp] * 11 + [c_i] * 2 + [c_st]),
    'ss_window_push': (c_i, [c_fp, c_fp, ctypes.c_void_p, c_i, c_i, c_i, c_fp, c_i, c_i, c_ll, c_ll, c_st]),
    'ss_window_push_groups': (c_i, [c_fp, c_fp, ctypes.c_void_p, c_i, c_i, c_i, c_i, c_fp, c_i, c_i, c_ll, c_ll, c_st]),
    'ss_window_advance': (c_i, [c_fp, c_fp, c_fp, ctypes.c_void_p, c_i, c_i, c_i, c_i, c_fp, c_fp, c_i, c_i, c_ll, c_ll, c_st]),
    'ss_alignment_psnr_ssim': (c_i, [c_fp, c_fp, c_fp, c_fp, c_i, c_i, c_i, c_st]),
    'ss_stability_score': (c_i, [c_fp, c_fp, c_i, c_st]),
    'ss_distortion_score': (c_i, [c_fp, c_fp, c_fp, c_i, c_st]),
}

_lib = None


def load(path, signatures):
    """ctypes handle of the library at `path` with the restype / argtypes of `signatures` set; raises if it has not been built."""
    if not os.path.exists(path):
        raise ImportError(
            'stabstitch2_amd: %s not found. Build it with `python -c "import __graft_entry__ as g; g.build()"` '
            'or stabstitch2_amd/csrc/build.sh (hipcc --offload-arch=gfx950). There is no CPU fallback.' % path)
    handle = ctypes.CDLL(path)
    for name, (res, args) in signatures.items():
        fn = getattr(handle, name)
        fn.restype = res
        fn.argtypes = args
    return handle


def lib():
    """The loaded library (loads on first use; raises if it has not been built)."""
    global _lib
    if _lib is None:
        _lib = load(LIB_PATH, SIGNATURES)
    return _lib


class HipError(RuntimeError):
    code = 0


def check(code, what):
    """The main library's return codes: anything but 0 is a HipError with the library's own text."""
    if code != 0:
        err = HipError('%s failed: %s (%d)' % (what, lib().ss_error_string(code).decode(), code))
        err.code = code
        raise err


def check_side(code, what):
    """The side libraries' return codes: an argument the library refuses is a ValueError, a failed launch a HipError."""
    if code == ERR_ARG:
        raise ValueError('%s refused its arguments' % what)
    if code != 0:
        err = HipError('%s failed: launch error (%d)' % (what, code))
        err.code = code
        raise err


class DevPtr(ctypes.c_void_p):
    """Device pointer that remembers which GPU it lives on (so that `call` can pick that GPU's stream)."""
    dev = None


class _CurrentStream:
    """Placeholder for "the current HIP stream of the device the pointer arguments live on"; resolved by `call`."""


_STREAM = _CurrentStream()


def stream():
    return _STREAM


def dptr(t, allow_none=False, dtype=torch.float32):
    """Device pointer of a contiguous device tensor of `dtype` (fp32 unless stated)."""
    if t is None:
        if allow_none:
            return None
        raise ValueError('null tensor passed to a HIP kernel')
    if not t.is_cuda:
        raise HipError('stabstitch2_amd kernels need device tensors (got %s); there is no CPU path' % t.device)
    if t.dtype != dtype or not t.is_contiguous():
        raise HipError('stabstitch2_amd kernels need contiguous %s tensors (got %s, contiguous=%s)'
                       % (str(dtype).replace('torch.', ''), t.dtype, t.is_contiguous()))
    p = DevPtr(t.data_ptr())
    p.dev = t.device.index
    return p


def ptr_array(tensors, dtype=torch.float32):
    """`const float* const*` argument: array of device pointers (all tensors checked like `dptr`); carries the device."""
    ps = [dptr(t, dtype=dtype) for t in tensors]
    arr = (ctypes.c_void_p * len(ps))(*[p.value for p in ps])
    arr.dev = ps[0].dev
    if any(p.dev != arr.dev for p in ps):
        raise HipError('tensors of one launch live on different GPUs')
    return arr


def launch(lib, name, args, host_ok=False):
    """The one launch path of the five libraries -> the entry point's return code.  `lib`: the binding module's `lib`.  Launches on
    the GPU that owns the pointer arguments, on THAT device's current stream (not the current device's): nets moved to cuda:1 keep
    working while cuda:0 is current, and launches stay ordered with the torch ops that produced their inputs.  A call without device
    pointers (workspace queries, version) is an error unless `host_ok`."""
    dev = None
    for a in args:
        d = getattr(a, 'dev', None)
        if d is not None:
            if dev is None:
                dev = d
            elif d != dev:
                raise HipError('%s: tensors of one launch live on different GPUs (cuda:%d and cuda:%d)' % (name, dev, d))
    if dev is None:
        if host_ok:
            return getattr(lib(), name)(*args)
        raise HipError('%s needs device tensors; there is no CPU path' % name)
    fn = getattr(lib(), name)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    args = tuple(st if a is _STREAM else a for a in args)
    if dev == torch.cuda.current_device():
        return fn(*args)
    with torch.cuda.device(dev):
        return fn(*args)


def call(name, *args):
    """`launch` on the main library; a call without device pointers is allowed."""
    code = launch(lib, name, args, True)
    if code != 0:                            # `check`, without a second Python call per launch: a push is ~80 of these, host-bound
        check(code, name)
