"""Addressing widths of the four libraries, as a table and as planned shapes.

ROWS gives one row to every exported function of include/stabstitch_hip.h, stabstitch_blend.h, stabstitch_seam.h and
stabstitch_mbwarp.h that takes a count of frames, items or elements (every integer parameter whose name is not in NOT_A_COUNT:
the rule fails closed), of one of three kinds:

    'wide'      its frame-sized buffers may exceed 2^31 elements; `cases` names the GPU cases (CASES below, run by
                tests/test_gpu_large_offsets.py) that take each such buffer across the line; `not_crossed` names a buffer that no case
                within CAP can take across, with the arithmetic
    'refuses'   it has a documented limit: `limit` is the expression, `test` the CPU test that shows the refusal
    'small'     no argument combination the entry accepts in this project puts a buffer past 2^31 elements: `bound` says why

CASES are the shapes of the GPU cases, planned here so that tests/test_large_offsets_abi.py can check their arithmetic without a
GPU: which buffer crosses which line (element 2^31 of a 4-byte buffer; byte 2^31 or byte 2^32 of a 1-byte buffer), that one frame
straddles the line and at least one whole frame lies beyond it, and that the case stays under CAP bytes of device memory."""
import collections
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L31, L32 = 1 << 31, 1 << 32
CAP = 20 << 30                      # bytes of device memory a case may hold at its peak

HEADERS = (('stabstitch_hip.h', 'SS_API'), ('stabstitch_blend.h', 'SSB_API'), ('stabstitch_seam.h', 'SSM_API'),
           ('stabstitch_mbwarp.h', 'SSW_API'))
# Integer parameters that are NOT a count of frames, items or elements: sizes of ONE item, strides, modes, flags and thresholds.  Every
# other int / long long parameter counts (n, frames, b, streams, nw, t, n_points, n_pixels, m, groups, rings, per, k, q, images today):
# a new entry whose parameter has a new name needs a row, or its name here.
NOT_A_COUNT = frozenset((
    'code', 'c', 'h', 'w', 'c_pad', 'c_stride', 'cin', 'cout', 'kt', 'kh', 'kw', 'stride', 'pad', 'pad_t', 'pad_h', 'pad_w', 'relu', 'out_cs',
    'in_gs', 'w_gs', 'out_gs', 'u_gs', 'ws_floats', 'ws_bytes', 'state_ints', 'ho', 'wo', 'min_wgs', 'min_cin', 'min_fill_pct', 'on', 'nout',
    'x_group_stride', 'r', 'split', 'shift', 'views', 'view', 'ty', 'out_h', 'out_w', 'lag', 'hc', 'wc', 'hout', 'wout', 'mode',
    'footprint_floats', 'out_pitch', 'out_format', 'rows', 'u8', 'img_fs', 'fp_fs', 'min_nodes', 'accumulate', 'mesh_frame_stride',
    'bbox_frame_stride', 'wstride', 'zero_first', 'window', 'elems', 'blocks', 'block', 'delta', 'src_stride', 'lr_h', 'lr_w', 'pitch',
    'frame_stride', 'bands', 'cell', 'mu'))


def prototypes():
    """{exported function: [names of its int / long long value parameters]} parsed out of the four headers."""
    out = {}
    for hdr, api in HEADERS:
        text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', hdr)).read(), flags=re.S)
        text = re.sub(r'^\s*#.*$', '', text, flags=re.M)            # the macro's own definitions
        for m in re.finditer(r'\b%s\s+[^;(]*?\b(\w+)\s*\(([^;]*?)\)\s*;' % api, text, flags=re.S):
            params = [p.strip() for p in m.group(2).replace('\n', ' ').split(',')]
            out[m.group(1)] = [p.split()[-1] for p in params if re.match(r'(const\s+)?(int|long long)\s+\w+$', p)]
    return out


def counted(protos=None):
    """The exported functions that take a count."""
    protos = prototypes() if protos is None else protos
    return sorted(n for n, ints in protos.items() if set(ints) - NOT_A_COUNT)


# ================================================================================================ the table
ROWS = {}


def _rows(names, **row):
    for n in names.split():
        assert n not in ROWS, n
        ROWS[n] = dict(row)


def tests_of(row):
    """the CPU tests a row cites (one name or several)"""
    t = row.get('test', ())
    return (t,) if isinstance(t, str) else tuple(t)


ABI = 'tests.test_large_offsets_abi::'
_CONV_TEST = ABI + 'test_conv_engine_refuses_what_32_bits_cannot_address'
_rows('ss_conv_nhwc ss_conv_stem3', kind='refuses', test=_CONV_TEST,
      limit='M < 2^31, in_elems * 4 < 2^31, w_elems * 4 < 2^31, M * out_cs * 4 < 2^32 (SS_ERR_UNSUPPORTED)')
_rows('ss_conv_pool2_nhwc', kind='refuses', test=_CONV_TEST,
      limit='only launches that split K, split-K workspace < 2^31 floats; M < 2^31, in_elems * 4 < 2^31 (SS_ERR_UNSUPPORTED)')
_rows('ss_conv3x3_wino_nhwc ss_conv3x3_wino3_nhwc ss_conv3x3_wino_pool2_nhwc ss_conv3x3_wino43_nhwc', kind='refuses', test=_CONV_TEST,
      limit='in_elems * 4 < 2^32, out_elems * 4 < 2^32, workgroups < 2^31 (SS_ERR_UNSUPPORTED)')
_rows('ss_stem_pool', kind='refuses', test=_CONV_TEST, limit='n * h * (w + 8) * 12 bytes < 2^32, workgroups < 2^31 (SS_ERR_UNSUPPORTED)')
_rows('ss_conv_workspace_need ss_conv_uses_winograd ss_conv_uses_wino43 ss_stem_pool_packed_floats ss_ccl_workspace_floats '
      'ss_tsmotion_workspace_floats ss_linear_clip_workspace_floats ss_linear_frames_workspace_floats ssb_multiband_workspace_floats '
      'ssm_seam_workspace_bytes', kind='small', bound='host arithmetic in long long: nothing is addressed')
_rows('ss_stem_pool_pack ss_wino_pack ss_wino_pack3 ss_wino43_pack', kind='small',
      bound='filter banks: groups x cout x cin x 16 taps of a network layer, a few MB')
_NET = 'by use, not by the ABI: network glue on LR maps (360 x 480 and below, <= 512 channels), n a window of LR frames; the conv '\
       'engine between these launches refuses n * h * w * c * 4 >= 2^31 bytes, so no map of the chain reaches 2^29 elements '\
       '(ss_nchw_to_nhwc refuses ONE image of 2^31 pixels: test_counts_past_the_grid_are_refused)'
_rows('ss_nchw_to_nhwc ss_nhwc_to_nchw ss_nchw_to_nhwc3_padded ss_maxpool_nhwc ss_maxpool_nhwc_split ss_linear ss_linear_grouped ss_ccl '
      'ss_l2norm_nhwc ss_cost_volume ss_cost_volume_bidir ss_cost_volume_shifted ss_cost_volume_chain_frames ss_homo_warp_nhwc '
      'ss_homo_warp_pair_nhwc ss_homo_warp_nchw', kind='small', bound=_NET)
_MESH = 'per item 63 control points (126 floats), a 3 x 3 or 66 x 66 matrix, or a watcher row: 2^31 elements would take > 490 000 '\
        'frames of one call, the entries that ride frames in a grid axis stop at 65535'
_rows('ss_tensor_dlt ss_spatial_decompose ss_spatial_meshes ss_tps_solve ss_tps_solve_shared_target ss_tps_points ss_tsmotion '
      'ss_tsmotion_lag ss_mesh_bbox ss_mesh_normalize ss_h2mesh ss_three_view_align ss_three_view_normalize ss_three_view_finish '
      'ss_three_view_splines ss_stream_splines ss_canvas_watch ss_canvas_watch_frames ss_canvas_watch_fit ss_canvas_watch_frames_fit '
      'ss_box_fit_aspect ss_stream_normalize_watch ss_mesh_normalize_views ss_mesh_normalize_views_boxes ss_stability_score '
      'ss_distortion_score', kind='small', bound=_MESH)
_rows('ss_smooth_embed ss_smooth_finalize ss_smooth_stitch', kind='small',
      bound='nw windows of t frames of a 7 x 9 mesh with 128 channels: 8064 floats per (window, frame)')
_rows('ss_window_push ss_window_push_groups ss_window_advance', kind='small',
      bound='(window - 1) * elems <= 2048 and <= 8 rings, <= 8 state blocks: refused beyond (tests.test_push_many_abi)')
_rows('ss_render_footprints ss_render_footprints_watch ss_render_footprints_watch_fit', kind='small',
      bound='per frame ss_render_footprint_floats: the lattice is refused above 4096 x 4096 nodes (SS_ERR_UNSUPPORTED), a 4K canvas '
            'has 0.2 M floats; frame offsets are long long')
_LIN_MASK = 'mask1_out is 1 (2) planes per frame against the 8 (11) of the workspace (lin_ws_v2_f32_gains writes and compares it)'
_rows('ss_render_linear_clip ss_render_linear_clip_gains', kind='wide', cases=['lin_ws_v2_f32_gains', 'lin_views_v2_f32'],
      limit='frames <= 65535', test=ABI + 'test_counts_past_the_grid_are_refused',
      not_crossed={'out': 'out is 3 of the 8 (11 with three views) planes per frame that the workspace holds: an out of 2^31 floats '
                          'comes with a workspace of >= 8/3 * 8 GiB = 21.3 GiB > CAP', 'mask1_out': _LIN_MASK})
_rows('ss_render_linear_clip_u8 ss_render_linear_clip_u8_gains', kind='wide',
      cases=['lin_ws_v3_u8', 'lin_views_v3_u8_31_gains', 'lin_views_v2_u8_32'], limit='frames <= 65535', test=ABI + 'test_counts_past_the_grid_are_refused',
      not_crossed={'out': 'out is 3 bytes per canvas pixel against 32 (44) bytes of workspace: 2^31 bytes of out come with 21.3 GiB',
                   'mask1_out': _LIN_MASK})
_rows('ss_render_linear_frames ss_render_linear_frames_gains', kind='wide', cases=['linf_ws_v2_f32_gains'])
_rows('ss_render_linear_frames_u8 ss_render_linear_frames_u8_gains', kind='wide', cases=['linf_ws_v3_u8'])
_rows('ss_render_linear_frames_nv12', kind='wide', cases=['linf_nv12_ws_v3'], limit='frames <= 32',
      test='tests.test_nv12_abi::test_render_linear_frames_nv12_refuses_bad_surfaces')
_rows('ss_render_average_clip ss_render_average_clip_gains', kind='wide',
      cases=['avg_out_v2_f32', 'avg_out_v3_f32_feather_gains', 'avg_views_v2_f32_gains', 'avg_views_v3_f32_feather'])
_rows('ss_render_average_clip_u8 ss_render_average_clip_u8_gains', kind='wide',
      cases=['avg_out_v2_u8_31_feather_gains', 'avg_out_v3_u8_32', 'avg_views_v3_u8_31_gains', 'avg_views_v2_u8_32_feather'])
_rows('ssw_multiband_warp', kind='wide', cases=['mbw_P_v2_f32_gains', 'mbw_imgs_v3_f32'], limit='frames * views <= 65535',
      test='tests.test_mbwarp_abi::test_every_refusal_comes_before_a_launch')
_rows('ssw_multiband_warp_u8', kind='wide', cases=['mbw_P_v3_u8', 'mbw_imgs_v2_u8_31_gains', 'mbw_imgs_v2_u8_32'],
      limit='frames * views <= 65535', test='tests.test_mbwarp_abi::test_every_refusal_comes_before_a_launch')
_rows('ssm_multiband_seam', kind='wide', cases=['seam_P_v2', 'seam_P_v3'], limit='frames <= 65535, hc and wc <= 32768, the grid fits the LDS',
      test='tests.test_seam_abi::test_every_refusal_comes_before_a_launch',
      not_crossed={'ws': 'the LDS rule holds a frame to 655 360 cells: the workspace is at most 9 ints per cell against 15 floats of P '
                         'per pixel (three views, cell 1), so 2^31 ints of it come with >= 14.3 GB of P, 22.9 GB > CAP; narrow canvases '
                         '(wc <= 27, where the padded rows tip the ratio) need >= 8.5 M sequential rows of the dynamic program'})
_rows('ssb_multiband_blend', kind='wide', cases=['mbb_P_v2_b0_f32'], limit='frame_floats < 2^31 - 1, frames * 4 * (views - 1) <= 65535',
      test=ABI + 'test_multiband_plan_refuses_a_frame_of_2_31_floats',
      not_crossed={'out': 'out is 3 planes per frame against 10 (15) of P: 2^31 floats of out come with >= 28.6 GB of P'})
_rows('ssb_multiband_blend_u8', kind='wide', cases=['mbb_ws_v2_b2_u8', 'mbb_P_v3_b2_u8'],
      limit='frame_floats < 2^31 - 1, frames * 4 * (views - 1) <= 65535', test=ABI + 'test_multiband_plan_refuses_a_frame_of_2_31_floats',
      not_crossed={'out': 'out is 3 bytes per pixel against 40 (60) bytes of P: 2^31 bytes of out come with >= 28.6 GB of P'})
_rows('ss_tps_warp_nchw', kind='wide', cases=['tps_U_nomask'], limit='b <= 65535, hc <= 524280', test=ABI + 'test_counts_past_the_grid_are_refused')
_rows('ss_tps_warp_mask_nchw', kind='wide', cases=['tps_out_mask'], limit='b <= 65535, hc <= 524280', test=ABI + 'test_counts_past_the_grid_are_refused')
_rows('ss_exposure_update', kind='wide', cases=['exp_views_v2_f32', 'exp_views_v3_u8_31', 'exp_views_v2_u8_32'], limit='frames <= 65535', test=ABI + 'test_counts_past_the_grid_are_refused')
_rows('ss_ingest_u8', kind='wide', cases=['ingest_u8_hr4', 'ingest_u8_hr1', 'ingest_u8_in32'], limit='h * w <= 2^31 - 1 (one frame); with lr: n <= 65535, lr_h <= 262140; n * h * w / 256 < 2^31 - 1',
      test=(ABI + 'test_frame_io_refuses_a_frame_of_2_31_pixels', ABI + 'test_counts_past_the_grid_are_refused'))
_rows('ss_canvas_to_u8', kind='wide', cases=['canvas_u8_x4', 'canvas_u8_x1'], limit='h * w <= 2^31 - 1 (one frame); n * h * w / 256 < 2^31 - 1',
      test=ABI + 'test_frame_io_refuses_a_frame_of_2_31_pixels',
      not_crossed={'out@2^32': '2^32 bytes of out are 2^32 floats of canvas: 16 GiB + 4 GiB + the straddling frame > CAP'})
_rows('ss_ingest_nv12', kind='wide', cases=['ingest_nv12_hr', 'ingest_nv12_in31', 'ingest_nv12_in32'], limit='n <= 65535, h <= 262140', test=ABI + 'test_counts_past_the_grid_are_refused')
_rows('ss_bgr_to_nv12', kind='wide', cases=['bgr_nv12_in31', 'bgr_nv12_in32_out31', 'bgr_nv12_out32'], limit='n <= 65535, h <= 524280', test=ABI + 'test_counts_past_the_grid_are_refused')
_rows('ss_add_mul', kind='wide', cases=['add_mul_n'])
_rows('ss_mask_union', kind='wide', cases=['mask_union_n'])
_rows('ss_fill_f32', kind='wide', cases=['fill_n'])
_rows('ss_alignment_psnr_ssim', kind='wide', cases=['psnr_ssim_stacks'], limit='frames <= 65535, h <= 262140', test=ABI + 'test_counts_past_the_grid_are_refused')


# ================================================================================================ the planned shapes
class Buf(collections.namedtuple('Buf', 'bytes_per starts ends total')):
    """One device buffer of a case: element size, the element range [starts[f], ends[f]) of every frame's block, all its elements."""
    __slots__ = ()

    @property
    def nbytes(self):
        return self.bytes_per * self.total

    def frames_at(self, line):
        """-> (the frame whose block holds element `line` - 1 and element `line`, the frames wholly at or beyond `line`)"""
        straddle = [f for f, (s, e) in enumerate(zip(self.starts, self.ends)) if s < line < e]
        beyond = [f for f, s in enumerate(self.starts) if s >= line]
        return straddle, beyond


def uniform(bytes_per, per, frames, total=None):
    return Buf(bytes_per, [f * per for f in range(frames)], [(f + 1) * per for f in range(frames)], per * frames if total is None else total)


def small(bytes_per, total):
    return Buf(bytes_per, [0], [total], total)


TINY_FRAME = (24, 41)               # h, w of a frame under a huge canvas
TINY_CANVAS = (40, 50)              # hc, wc over huge frames
BIG_CANVAS = (4096, 8190)           # 33.5 M pixels: 8 planes of it are 2^31 - 524 288 floats
BIG_CANVAS_V3 = (4096, 5460)        # 22.4 M pixels: 12 planes of it are the same
HUGE_CANVAS = (8192, 16380)         # 134 M pixels
BIG_FRAME = (8192, 8192)
HUGE_FRAME = (16384, 16384)
LBC_PW = 8


def cdiv(a, b):
    return -(-a // b)


def linear_clip_ws(frames, views, hc, wc):
    """ss_linear_clip_workspace_floats restated (tests/test_large_offsets_abi.py holds it to the library)."""
    ohw, p = hc * wc, views - 1
    tiles = cdiv(wc, 64) * cdiv(hc, 8)
    return frames * (views * 4 * ohw + (3 * ohw if views == 3 else 0) + p * 32 + tiles * 4 * p * LBC_PW) + 1


def multiband_plan(views, hc, wc, bands):
    """mb_plan of csrc/blend.hip restated: floats of one frame's workspace."""
    k = views - 1
    h, w, a = hc, wc, []
    for l in range(bands + 1):
        a.append(h * ((w + 3) & ~3))
        h, w = (h + 1) // 2, (w + 1) // 2
    return 4 * k * sum(a) + 3 * sum(a[1:]) + 4 * a[0]


Case = collections.namedtuple('Case', 'id family args buffers crosses also')
CASES = collections.OrderedDict()


def _case(id_, family, buffers, crosses, also=(), **args):
    assert id_ not in CASES, id_
    CASES[id_] = Case(id_, family, args, buffers, list(crosses), list(also))


def _clip_buffers(frames, views, u8, h, w, hc, wc, linear, masks=False):
    """the buffers of a clip render: the view clip (one tensor, passed for every view), out, and LINEAR's workspace"""
    b = collections.OrderedDict()
    b['views'] = uniform(1 if u8 else 4, 3 * h * w, frames)
    b['out'] = uniform(1 if u8 else 4, 3 * hc * wc, frames)
    if linear:
        b['ws'] = uniform(4, views * 4 * hc * wc, frames, linear_clip_ws(frames, views, hc, wc))
    if masks:
        b['mask1'] = uniform(4, (views - 1) * hc * wc, frames)
    return b


def _clip(id_, family, frames, views, u8, frame, canvas, crosses, gains=False, fusion=None, also=(), masks=False):
    _case(id_, family, _clip_buffers(frames, views, u8, frame[0], frame[1], canvas[0], canvas[1], family == 'linear_clip', masks), crosses,
          also, frames=frames, views=views, u8=u8, h=frame[0], w=frame[1], hc=canvas[0], wc=canvas[1], gains=gains, fusion=fusion,
          masks=masks)


# ---- LINEAR clip: the workspace under a tiny frame; the view clips over a tiny canvas
_clip('lin_ws_v2_f32_gains', 'linear_clip', 10, 2, False, TINY_FRAME, BIG_CANVAS, [('ws', L31)], gains=True, masks=True)
_clip('lin_ws_v3_u8', 'linear_clip', 10, 3, True, TINY_FRAME, BIG_CANVAS_V3, [('ws', L31)])
_clip('lin_views_v2_f32', 'linear_clip', 12, 2, False, BIG_FRAME, TINY_CANVAS, [('views', L31)])
_clip('lin_views_v3_u8_31_gains', 'linear_clip', 12, 3, True, BIG_FRAME, TINY_CANVAS, [('views', L31)], gains=True)
_clip('lin_views_v2_u8_32', 'linear_clip', 23, 2, True, BIG_FRAME, TINY_CANVAS, [('views', L32)], also=[('views', L31)])


# ---- LINEAR frames: ragged canvases, the offsets w_off / f_off / part_off past the line
def _ragged(id_, views, u8, sizes, gains, nv12=False):
    h, w = (TINY_FRAME[0], TINY_FRAME[1] - 1) if nv12 else TINY_FRAME           # (NV12 frames have even sides)
    b = collections.OrderedDict()
    b['views'] = uniform(1 if u8 else 4, h * w * 3 // 2 if nv12 else 3 * h * w, len(sizes))
    p = views - 1
    w_off, f_off, part_off, wt, ft, pt = [], [], [], 0, 0, 0
    for hc, wc in sizes:
        w_off.append(wt); f_off.append(ft); part_off.append(pt)
        wt += views * 4 * hc * wc
        ft += 3 * hc * wc if views == 3 else 0
        pt += cdiv(wc, 64) * cdiv(hc, 8) * 4 * p * LBC_PW
    total = sum(linear_clip_ws(1, views, hc, wc) - 1 for hc, wc in sizes) + 1
    b['ws'] = Buf(4, w_off, [o + views * 4 * hc * wc for o, (hc, wc) in zip(w_off, sizes)], total)
    b['outs'] = small(1 if u8 else 4, sum(3 * hc * wc for hc, wc in sizes))
    _case(id_, 'linear_frames', b, [('ws', L31)], frames=len(sizes), views=views, u8=u8, h=h, w=w, sizes=list(sizes), gains=gains,
          nv12=nv12, f_off=[o + wt for o in f_off], part_off=part_off)


_ragged('linf_ws_v2_f32_gains', 2, False, [(BIG_CANVAS[0] - 3 * i, BIG_CANVAS[1] + 5 * i) for i in range(10)], True)
_ragged('linf_ws_v3_u8', 3, True, [(BIG_CANVAS_V3[0] + 2 * i, BIG_CANVAS_V3[1] - 3 * i) for i in range(10)], False)
# the NV12 overload of lb_frames_warp_kernel adds w_off, part_off and the frames' own strides itself
_ragged('linf_nv12_ws_v3', 3, True, [(BIG_CANVAS_V3[0] - 4 * i, BIG_CANVAS_V3[1] + 2 * i) for i in range(10)], False, nv12=True)

# ---- AVERAGE / FEATHER clip: out under a tiny frame; the view clips over a tiny canvas
_clip('avg_out_v2_f32', 'average_clip', 7, 2, False, TINY_FRAME, HUGE_CANVAS, [('out', L31)], fusion='AVERAGE')
_clip('avg_out_v3_f32_feather_gains', 'average_clip', 7, 3, False, TINY_FRAME, HUGE_CANVAS, [('out', L31)], gains=True, fusion='FEATHER')
_clip('avg_out_v2_u8_31_feather_gains', 'average_clip', 7, 2, True, TINY_FRAME, HUGE_CANVAS, [('out', L31)], gains=True, fusion='FEATHER')
_clip('avg_out_v3_u8_32', 'average_clip', 12, 3, True, TINY_FRAME, HUGE_CANVAS, [('out', L32)], fusion='AVERAGE', also=[('out', L31)])
_clip('avg_views_v2_f32_gains', 'average_clip', 12, 2, False, BIG_FRAME, TINY_CANVAS, [('views', L31)], gains=True, fusion='AVERAGE')
_clip('avg_views_v3_f32_feather', 'average_clip', 12, 3, False, BIG_FRAME, TINY_CANVAS, [('views', L31)], fusion='FEATHER')
_clip('avg_views_v3_u8_31_gains', 'average_clip', 12, 3, True, BIG_FRAME, TINY_CANVAS, [('views', L31)], gains=True, fusion='AVERAGE')
_clip('avg_views_v2_u8_32_feather', 'average_clip', 23, 2, True, BIG_FRAME, TINY_CANVAS, [('views', L32)], fusion='FEATHER',
      also=[('views', L31)])


# ---- the direct MULTIBAND warp: P under a tiny frame; the frames over a tiny canvas
def _mbw(id_, frames, views, u8, frame, canvas, crosses, gains=False, also=()):
    b = collections.OrderedDict()
    b['imgs'] = uniform(1 if u8 else 4, 3 * frame[0] * frame[1], frames)
    b['P'] = uniform(4, views * 5 * canvas[0] * canvas[1], frames)
    _case(id_, 'multiband_warp', b, crosses, also, frames=frames, views=views, u8=u8, h=frame[0], w=frame[1], hc=canvas[0], wc=canvas[1],
          gains=gains)


_mbw('mbw_P_v2_f32_gains', 8, 2, False, TINY_FRAME, BIG_CANVAS, [('P', L31)], gains=True)
_mbw('mbw_P_v3_u8', 6, 3, True, TINY_FRAME, BIG_CANVAS, [('P', L31)])
_mbw('mbw_imgs_v3_f32', 12, 3, False, BIG_FRAME, TINY_CANVAS, [('imgs', L31)])
_mbw('mbw_imgs_v2_u8_31_gains', 12, 2, True, BIG_FRAME, TINY_CANVAS, [('imgs', L31)], gains=True)
_mbw('mbw_imgs_v2_u8_32', 23, 2, True, BIG_FRAME, TINY_CANVAS, [('imgs', L32)], also=[('imgs', L31)])

# ---- the DP seam: P (cell 16: the grid of a 4096 x 8190 canvas is 256 x 512 cells)
SEAM_CELL = 16
for _v, _n in ((2, 8), (3, 6)):
    _case('seam_P_v%d' % _v, 'multiband_seam', collections.OrderedDict(P=uniform(4, _v * 5 * BIG_CANVAS[0] * BIG_CANVAS[1], _n)), [('P', L31)],
          frames=_n, views=_v, hc=BIG_CANVAS[0], wc=BIG_CANVAS[1], cell=SEAM_CELL)


# ---- the blend: P and the workspace grow together (10 against 8 .. 10.3 planes per frame with two views)
def _mbb(id_, frames, views, bands, u8, canvas, crosses, also=()):
    hc, wc = canvas
    b = collections.OrderedDict()
    b['P'] = uniform(4, views * 5 * hc * wc, frames)
    b['ws'] = uniform(4, multiband_plan(views, hc, wc, bands), frames)
    b['out'] = uniform(1 if u8 else 4, 3 * hc * wc, frames)
    _case(id_, 'multiband_blend', b, crosses, also, frames=frames, views=views, bands=bands, u8=u8, hc=hc, wc=wc)


_mbb('mbb_P_v2_b0_f32', 24, 2, 0, False, (3072, 3108), [('P', L31)])
_mbb('mbb_ws_v2_b2_u8', 24, 2, 2, True, (3072, 3048), [('ws', L31)], also=[('P', L31)])
_mbb('mbb_P_v3_b2_u8', 24, 3, 2, True, (3072, 2072), [('P', L31)], also=[('ws', L31)])


# ---- the generic dense warp
def _tps(id_, b, c, mask, frame, canvas, crosses):
    bufs = collections.OrderedDict()
    bufs['U'] = uniform(4, c * frame[0] * frame[1], b)
    bufs['out'] = uniform(4, (c + int(mask)) * canvas[0] * canvas[1], b)
    _case(id_, 'tps_warp', bufs, crosses, frames=b, c=c, mask=mask, h=frame[0], w=frame[1], hc=canvas[0], wc=canvas[1])


_tps('tps_U_nomask', 12, 3, False, BIG_FRAME, TINY_CANVAS, [('U', L31)])
_tps('tps_out_mask', 7, 3, True, TINY_FRAME, (8192, 12000), [('out', L31)])

# ---- exposure: the view clips (the lattice of a 96 x 256 canvas is 12 x 8 nodes)
EXPOSURE_CANVAS = (96, 256)
for _id, _n, _v, _u8, _line in (('exp_views_v2_f32', 12, 2, False, L31), ('exp_views_v3_u8_31', 12, 3, True, L31),
                                ('exp_views_v2_u8_32', 23, 2, True, L32)):
    _case(_id, 'exposure_update', collections.OrderedDict(views=uniform(1 if _u8 else 4, 3 * BIG_FRAME[0] * BIG_FRAME[1], _n)),
          [('views', _line)], [('views', L31)] if _line == L32 else [], frames=_n, views=_v, u8=_u8, h=BIG_FRAME[0], w=BIG_FRAME[1],
          hc=EXPOSURE_CANVAS[0], wc=EXPOSURE_CANVAS[1])


# ---- frame I/O
def _io(id_, family, n, h, w, bufs, crosses, also=(), **args):
    _case(id_, family, collections.OrderedDict(bufs), crosses, also, frames=n, h=h, w=w, **args)


_H, _W = BIG_FRAME
_io('ingest_u8_hr4', 'ingest_u8', 12, _H, _W, [('in', uniform(1, 3 * _H * _W, 12)), ('hr', uniform(4, 3 * _H * _W, 12)),
                                                ('lr', uniform(4, 3 * 36 * 48, 12))],
    [('in', L31), ('hr', L31)], want_hr=True, lr=(36, 48))                      # w % 4 == 0: four pixels a thread; general resize
_io('ingest_u8_hr1', 'ingest_u8', 12, _H, _W - 2, [('in', uniform(1, 3 * _H * (_W - 2), 12)), ('hr', uniform(4, 3 * _H * (_W - 2), 12)),
                                                    ('lr', uniform(4, 3 * (_H // 2) * (_W // 2 - 1), 12))],
    [('in', L31), ('hr', L31)], want_hr=True, lr=(_H // 2, _W // 2 - 1))        # w % 4 != 0: a pixel a thread; the exact 2 x 2 resize
_io('ingest_u8_in32', 'ingest_u8', 23, _H, _W, [('in', uniform(1, 3 * _H * _W, 23)), ('lr', uniform(4, 3 * 36 * 48, 23))],
    [('in', L32)], [('in', L31)], want_hr=False, lr=(36, 48))
_io('ingest_nv12_hr', 'ingest_nv12', 12, _H, _W, [('in', uniform(1, _H * _W * 3 // 2, 12)), ('hr', uniform(4, 3 * _H * _W, 12)),
                                                   ('lr', uniform(4, 3 * 36 * 48, 12))], [('hr', L31)], want_hr=True, lr=(36, 48))
_HH, _HW = HUGE_FRAME
_io('ingest_nv12_in31', 'ingest_nv12', 7, _HH, _HW, [('in', uniform(1, _HH * _HW * 3 // 2, 7)), ('lr', uniform(4, 3 * 36 * 48, 7))],
    [('in', L31)], want_hr=False, lr=(36, 48))
_io('ingest_nv12_in32', 'ingest_nv12', 12, _HH, _HW, [('in', uniform(1, _HH * _HW * 3 // 2, 12)), ('lr', uniform(4, 3 * 36 * 48, 12))],
    [('in', L32)], [('in', L31)], want_hr=False, lr=(36, 48))
_io('canvas_u8_x4', 'canvas_to_u8', 12, _H, _W, [('in', uniform(4, 3 * _H * _W, 12)), ('out', uniform(1, 3 * _H * _W, 12))],
    [('in', L31), ('out', L31)])                                                # h * w % 4 == 0: four pixels a thread
_io('canvas_u8_x1', 'canvas_to_u8', 12, _H - 1, _W - 1, [('in', uniform(4, 3 * (_H - 1) * (_W - 1), 12)),
                                                         ('out', uniform(1, 3 * (_H - 1) * (_W - 1), 12))], [('in', L31), ('out', L31)])
_io('bgr_nv12_in31', 'bgr_to_nv12', 12, _H, _W, [('in', uniform(1, 3 * _H * _W, 12)), ('out', uniform(1, _H * _W * 3 // 2, 12))],
    [('in', L31)])
_io('bgr_nv12_in32_out31', 'bgr_to_nv12', 23, _H, _W, [('in', uniform(1, 3 * _H * _W, 23)), ('out', uniform(1, _H * _W * 3 // 2, 23))],
    [('in', L32), ('out', L31)], [('in', L31)])
_io('bgr_nv12_out32', 'bgr_to_nv12', 12, _HH, _HW, [('in', uniform(1, 3 * _HH * _HW, 12)), ('out', uniform(1, _HH * _HW * 3 // 2, 12))],
    [('out', L32)], [('in', L31), ('in', L32), ('in', 1 << 33), ('out', L31)])

# ---- elementwise over n: a "frame" is a block of 2^26 + 1 elements (no power of two: block and wave boundaries move through it)
EW_BLOCK, EW_BLOCKS = (1 << 26) + 1, 34
_case('add_mul_n', 'add_mul', collections.OrderedDict(x=uniform(4, EW_BLOCK, EW_BLOCKS), out=uniform(4, EW_BLOCK, EW_BLOCKS)),
      [('x', L31), ('out', L31)], frames=EW_BLOCKS, block=EW_BLOCK)
# a and b are one buffer of 35 blocks read one block apart (a third buffer of this size would exceed CAP)
_case('mask_union_n', 'mask_union', collections.OrderedDict(ab=uniform(4, EW_BLOCK, EW_BLOCKS + 1), out=uniform(4, EW_BLOCK, EW_BLOCKS)),
      [('ab', L31), ('out', L31)], frames=EW_BLOCKS, block=EW_BLOCK)
_case('fill_n', 'fill', collections.OrderedDict(p=uniform(4, EW_BLOCK, EW_BLOCKS), canaries=small(4, 2 * EW_BLOCK)), [('p', L31)],
      frames=EW_BLOCKS, block=EW_BLOCK)

# ---- PSNR / SSIM: both stacks are 14 frames of one buffer of 15, read one frame apart
METRIC_FRAME = (8192, 5240)
_case('psnr_ssim_stacks', 'psnr_ssim', collections.OrderedDict(w12=uniform(4, 4 * METRIC_FRAME[0] * METRIC_FRAME[1], 15)), [('w12', L31)],
      frames=14, h=METRIC_FRAME[0], w=METRIC_FRAME[1])


# ================================================================================================ what a case compares, what it holds
def compared(case):
    """Frame 0, every straddling frame and every frame wholly beyond a line of `crosses`, ascending."""
    idx = {0}
    for name, line in case.crosses:
        s, b = case.buffers[name].frames_at(line)
        idx.update(s)
        idx.update(b)
    return sorted(f for f in idx if f < case.args['frames'])


# outputs whose compared frames are cloned while the big buffers are still held, then kept beside the reference call
OUTPUTS = {'linear_clip': ('out', 'mask1'), 'linear_frames': ('outs',), 'average_clip': ('out',), 'multiband_warp': ('P',), 'multiband_seam': (),
           'multiband_blend': ('out',), 'tps_warp': ('out',), 'exposure_update': (), 'ingest_u8': ('hr', 'lr'), 'ingest_nv12': ('hr', 'lr'),
           'canvas_to_u8': ('out',), 'bgr_to_nv12': ('out',), 'add_mul': ('out',), 'mask_union': ('out',), 'fill': (), 'psnr_ssim': ()}
# buffers of the big call that the reference call allocates again for the compared frames only
REFERENCE = {'linear_clip': ('views', 'out', 'ws', 'mask1'), 'linear_frames': ('ws', 'outs'), 'average_clip': ('views', 'out'),
             'multiband_warp': ('imgs', 'P'), 'multiband_seam': ('P',), 'multiband_blend': ('P', 'ws', 'out'), 'tps_warp': ('U', 'out'),
             'exposure_update': ('views',), 'ingest_u8': ('in', 'hr', 'lr'), 'ingest_nv12': ('in', 'hr', 'lr'), 'canvas_to_u8': ('in', 'out'),
             'bgr_to_nv12': ('in', 'out'), 'add_mul': ('x', 'out'), 'mask_union': ('ab', 'out'), 'fill': (), 'psnr_ssim': ('w12', 'w12')}


def _frames_bytes(buf, frames):
    return buf.bytes_per * sum(buf.ends[f] - buf.starts[f] for f in frames if f < len(buf.starts))


def peak_bytes(case):
    """Device bytes a case plans to hold at its worst moment: every buffer of the big call + the clones of the compared output
    frames; or, once the big call's outputs and workspace are freed, its inputs + those clones + the reference call's buffers.
    (Splines, gains, footprints and the input pattern of one frame come on top: inside `slack_bytes`.)"""
    c = compared(case)
    big = sum(b.nbytes for b in case.buffers.values())
    inputs = sum(b.nbytes for n, b in case.buffers.items() if n not in OUTPUTS[case.family] and n != 'ws')
    kept = sum(_frames_bytes(case.buffers[n], c) for n in OUTPUTS[case.family] if n in case.buffers)
    ref = sum(_frames_bytes(case.buffers[n], c) for n in REFERENCE[case.family] if n in case.buffers)
    return max(big + kept, inputs + kept + ref)


def slack_bytes(case):
    """the inputs of one frame as a pattern and one temporary of it (the generators work frame by frame)"""
    per = max(b.bytes_per * max(e - s for s, e in zip(b.starts, b.ends)) for b in case.buffers.values())
    return min(2 * per + (64 << 20), 2 << 30)
