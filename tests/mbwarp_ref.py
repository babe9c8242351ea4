"""Helpers of the direct MULTIBAND warp's tests (libstabstitch_mbwarp.so): the reach table of its four kernel
instantiations and the input builders.  tests/test_mbwarp_abi.py holds the table to the code objects, tests/test_gpu_mbwarp.py's launch
witness to what the smallest calls launch."""
import numpy as np

import sweep_inputs as G

F32 = np.float32
GW = 'tests.test_gpu_mbwarp'
FRAME = (24, 41)                            # h, w: a uint8 row of 123 bytes, no multiple of 4
# canvases (hc, wc): 43 x 67 -- a second tile column of 3 pixels and a last tile row whose `yb` rows (44..47) lie past the canvas;
# 3 x 9 -- waves 3 of the only workgroup return whole, and every `yb` row is past the canvas; 81 x 129 -- eleven tile rows, three columns
CANVASES = [(43, 67), (3, 9), (81, 129)]


def reach():
    """Every kernel instantiation of libstabstitch_mbwarp.so, mw_warp_kernel<U8, GAINS> as sweep_inputs.kernel_key writes it ->
    ('exact', tests): the tests that hold it bit for bit -- without gains to ss_tps_warp_mask_nchw on the stacked planes, with gains
    to the fp32 product and minimum of the plain planes."""
    plain = tuple(GW + '::' + n for n in ('test_plain_warp_equals_stack_and_warp', 'test_canaries_and_a_nan_plane_in_front_of_the_frames'))
    gains = tuple(GW + '::' + n for n in ('test_gains_scale_and_clamp_the_colour_planes', 'test_render_multiband_with_gains'))
    return {'mw_warp_kernel<%d,%d>' % (u8, g): ('exact', gains if g else plain) for u8 in (0, 1) for g in (0, 1)}


def warp_inputs(n, views, hc, wc, seed=0, off_canvas=True):
    """n frames of `views` views of FRAME on a hc x wc canvas -> (frames uint8 [n,views,h,w,3], source [n,views,63,2], target
    [n*views,63,2]): sweep_inputs.warp_case's textures (rounded: fp32 and uint8 inputs then hold the same values) and splines.
    off_canvas: item 0's control points are moved left until the leftmost lies 0.2 (normalised: a tenth of the canvas) beyond the
    canvas edge -- part of that view leaves the canvas, and on a canvas wider than the frame part of the canvas lies outside it."""
    h, w = FRAME
    U, src, tgt = G.warp_case(n * views, h, w, hc, wc, seed=seed)
    u8 = np.clip(np.rint(U[:, :3]), 0, 255).astype(np.uint8)
    src = src.copy()
    if off_canvas:
        src[0, :, 0] += F32(-1.2) - src[0, :, 0].min()
    frames = np.ascontiguousarray(u8.transpose(0, 2, 3, 1)).reshape(n, views, h, w, 3)
    return frames, np.ascontiguousarray(src.reshape(n, views, 63, 2)), tgt


def gains_case(n, views, seed=0):
    """Gains [n,views,3] in [0.5, 2], every (frame, view) row different; entry [0, 0, 0] is 2: with textures that reach 227 it drives
    samples past 255."""
    rs = np.random.RandomState(900 + seed)
    g = rs.uniform(0.5, 2.0, (n, views, 3)).astype(F32)
    g[0, 0, 0] = 2.0
    return g


def side_by_side_meshes(n, rects, height):
    """Per view a mesh [1,n,7,9,2] in canvas pixels (render_frames' prescaled=True) that puts the frame on the rectangle
    rects[v] = (x0, x1) x (0, height): identity-like splines, overlapping where the rectangles do."""
    ty, tx = np.meshgrid(np.linspace(0, 1, 7), np.linspace(0, 1, 9), indexing='ij')
    out = []
    for x0, x1 in rects:
        m = np.stack((x0 + (x1 - x0) * tx, height * ty), -1).astype(F32)
        out.append(np.ascontiguousarray(np.broadcast_to(m, (1, n, 7, 9, 2))))
    return out
