"""The addressing table of tests/large_offsets.py, held complete without a GPU: every exported function that takes a count has a row,
every test a row cites exists, every planned GPU case crosses the line it claims by a straddling frame and a whole frame and stays
under the memory cap; and the refusals that the table cites from here (host pointers throughout: a call that got as far as a launch
would fault).
    python -m pytest tests/test_large_offsets_abi.py"""
import ast
import ctypes
import os

import pytest

import large_offsets as L
from test_host_logic import built_lib  # noqa: F401  (fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_UNSUPPORTED = -1, -3
FAMILIES = ('linear_clip', 'linear_frames', 'average_clip', 'multiband_warp', 'multiband_seam', 'multiband_blend', 'tps_warp',
            'exposure_update', 'ingest_u8', 'ingest_nv12', 'canvas_to_u8', 'bgr_to_nv12', 'add_mul', 'mask_union', 'fill', 'psnr_ssim')


# ------------------------------------------------------------------------------------------------ 1. the table is complete
def test_every_exported_function_with_a_count_has_a_row():
    protos = L.prototypes()
    assert len([n for n in protos if n.startswith('ss_')]) == 113 and len(protos) == 113 + 4 + 3 + 3, len(protos)
    counted = L.counted(protos)
    missing = [n for n in counted if n not in L.ROWS]
    assert not missing, 'exported functions that take a count and have no row in large_offsets.ROWS: %s' % missing
    stale = [n for n in L.ROWS if n not in protos]
    assert not stale, 'rows without an exported function: %s' % stale
    uncounted = [n for n in L.ROWS if n not in counted]
    assert not uncounted, 'rows of functions that take no count: %s' % uncounted
    # what has no row takes no count: versions, knobs, packed sizes, the single-frame renders and blends
    for n in sorted(set(protos) - set(L.ROWS)):
        assert not (set(protos[n]) - L.NOT_A_COUNT), (n, protos[n])
    # the rule fails closed: an integer parameter with a name nobody has classified counts, so a new entry needs a row
    assert L.counted({'ss_new_entry': ['nframes', 'h', 'w']}) == ['ss_new_entry'] and L.counted({'ss_new_knob': ['mode']}) == []
    assert not ({'n', 'frames', 'b', 'streams', 'nw', 't', 'n_points', 'n_pixels', 'm', 'groups', 'k', 'q'} & L.NOT_A_COUNT)
    for n in ('ss_render_average', 'ss_render_average_u8', 'ss_render_average_nv12', 'ss_linear_blend', 'ss_tps_warp_views', 'ss_version'):
        assert n in protos and n not in L.ROWS, n


def test_rows_are_well_formed():
    for name, row in L.ROWS.items():
        assert row['kind'] in ('wide', 'refuses', 'small'), name
        if row['kind'] == 'wide':
            assert row['cases'] and all(c in L.CASES for c in row['cases']), (name, row['cases'])
            assert set(row) <= {'kind', 'cases', 'limit', 'test', 'not_crossed'}, name
            assert ('limit' in row) == ('test' in row), name
        elif row['kind'] == 'refuses':
            assert row['limit'] and row['test'] and set(row) == {'kind', 'limit', 'test'}, name
        else:
            assert row['bound'] and '\n' not in row['bound'] and set(row) == {'kind', 'bound'}, name
    used = {c for row in L.ROWS.values() for c in row.get('cases', ())}
    assert used == set(L.CASES), sorted(used ^ set(L.CASES))           # no case without a row that names it
    assert {c.family for c in L.CASES.values()} == set(FAMILIES)


def _defined_tests(path):
    tree = ast.parse(open(path).read())
    return {n.name for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name.startswith('test_')}


def test_every_cited_test_exists():
    cited = sorted({t for row in L.ROWS.values() for t in L.tests_of(row)})
    assert len(cited) >= 6
    for ref in cited:
        mod, fn = ref.split('::')
        path = os.path.join(ROOT, *mod.split('.')) + '.py'
        assert os.path.exists(path), ref
        assert fn in _defined_tests(path), ref
    # a citation has to exercise the limit it is cited for: a count limit of 65535 (32) is shown by a call with 65536 (33)
    for name, row in L.ROWS.items():
        if 'test' in row:
            body = ''
            for ref in L.tests_of(row):
                mod, fn = ref.split('::')
                tree = ast.parse(open(os.path.join(ROOT, *mod.split('.')) + '.py').read())
                body += ast.unparse([n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == fn][0])
                if fn == 'test_counts_past_the_grid_are_refused':
                    assert "'%s'" % name in body, (name, 'is not called by the test it cites')
            if '65535' in row['limit']:
                assert '65536' in body or '32768' in body, (name, row['test'])
            if '<= 32' in row['limit'].replace('<= 32768', ''):
                assert '33' in body, (name, row['test'])
            if '2^31 - 1 (one frame)' in row['limit']:
                assert '46341' in body, (name, row['test'])
    # and the GPU cases a row names are cases the GPU module runs: it takes its parameters from L.CASES by family
    gpu = open(os.path.join(ROOT, 'tests', 'test_gpu_large_offsets.py')).read()
    for fam in FAMILIES:
        assert "cases_of('%s')" % fam in gpu, fam


# ------------------------------------------------------------------------------------------------ 2. the planned shapes
@pytest.mark.parametrize('cid', list(L.CASES))
def test_case_crosses_its_line_and_fits(cid):
    case = L.CASES[cid]
    n = case.args['frames']
    declared = set(case.crosses) | set(case.also)
    assert case.crosses and len(declared) == len(case.crosses) + len(case.also)
    for name, line in declared:
        buf = case.buffers[name]
        assert line in (L.L31, L.L32, 1 << 33) and (buf.bytes_per == 1 or line == L.L31), (name, line)
        assert buf.bytes_per in (1, 4)
        straddle, beyond = buf.frames_at(line)
        assert len(straddle) == 1, (cid, name, 'no frame straddles the line', straddle)      # elements on both sides of it
        assert beyond and beyond[0] == straddle[0] + 1, (cid, name, beyond)                   # a whole frame beyond
        assert buf.total > line
    # one buffer per case: nothing else reaches a line (what grows together with the crossed buffer is declared in `also`)
    for name, buf in case.buffers.items():
        for line in (L.L31,) + ((L.L32, 1 << 33) if buf.bytes_per == 1 else ()):
            if (name, line) not in declared:
                assert buf.total <= line, (cid, name, 'crosses %d undeclared' % line, buf.total)
    # a 1-byte buffer that is taken across byte 2^32 has a sibling case at byte 2^31, or crosses it in the same case on other frames
    for name, line in case.crosses:
        if line == L.L32:
            assert (name, L.L31) in declared
    c = L.compared(case)
    assert c[0] == 0 and len(c) >= 3 and c[-1] == n - 1 and len(c) <= 8, c
    assert L.peak_bytes(case) + L.slack_bytes(case) <= L.CAP, (cid, L.peak_bytes(case), L.slack_bytes(case))
    for buf in case.buffers.values():                                                          # frames are blocks of their buffer
        assert all(0 <= s < e <= buf.total for s, e in zip(buf.starts, buf.ends))
        assert all(e <= s2 for e, s2 in zip(buf.ends, buf.starts[1:]))


def test_one_byte_buffers_cross_both_lines():
    """every uint8 buffer family of the table is taken across byte 2^31 in one case and across byte 2^32 in another"""
    for fam, name in (('linear_clip', 'views'), ('average_clip', 'views'), ('average_clip', 'out'), ('multiband_warp', 'imgs'),
                      ('exposure_update', 'views'), ('ingest_u8', 'in'), ('ingest_nv12', 'in'), ('bgr_to_nv12', 'in'), ('bgr_to_nv12', 'out')):
        lines = {line for c in L.CASES.values() if c.family == fam and c.buffers[name].bytes_per == 1 for n, line in c.crosses if n == name}
        assert {L.L31, L.L32} <= lines, (fam, name, lines)


def test_planned_workspaces_equal_the_libraries(built_lib):
    from stabstitch2_amd import _blend, _seam
    for case in L.CASES.values():
        a = case.args
        if case.family == 'linear_clip':
            assert case.buffers['ws'].total == built_lib.ss_linear_clip_workspace_floats(a['frames'], a['views'], a['hc'], a['wc'])
            assert case.buffers['ws'].ends[-1] <= case.buffers['ws'].total
        elif case.family == 'linear_frames':
            n = a['frames']
            hcs = (ctypes.c_int * n)(*[s[0] for s in a['sizes']])
            wcs = (ctypes.c_int * n)(*[s[1] for s in a['sizes']])
            assert case.buffers['ws'].total == built_lib.ss_linear_frames_workspace_floats(n, a['views'], hcs, wcs)
            # the three offset tables of LbFrameTab: W of the straddling frame holds the line, every F block and every partials block
            # lies beyond it
            if a['views'] == 3:
                assert min(a['f_off']) >= L.L31
            assert case.buffers['ws'].ends[-1] >= L.L31 and a['part_off'][0] == 0
        elif case.family == 'multiband_blend':
            need = _blend.lib().ssb_multiband_workspace_floats(a['frames'], a['views'], a['hc'], a['wc'], a['bands'])
            assert need == case.buffers['ws'].total > 0
        elif case.family == 'multiband_seam':
            need = _seam.lib().ssm_seam_workspace_bytes(a['frames'], a['views'], a['hc'], a['wc'], a['cell'])
            assert 0 < need < (1 << 28)                       # accepted, and small beside P
            assert _seam.lds_bytes(a['hc'], a['wc'], a['cell']) <= _seam.LDS_BYTES


def test_what_the_table_calls_out_of_reach_is():
    """the `not_crossed` notes, as arithmetic: the buffers that grow with a larger one cannot reach their line under CAP"""
    # LINEAR: out of 2^31 elements (fp32: floats, uint8: bytes) against the workspace of the same frames
    for views in (2, 3):
        for out_bytes_per in (4, 1):
            pixels = L.L31 / 3.0                                           # frames * hc * wc of an out at the line
            ws = 4 * pixels * (views * 4 + (3 if views == 3 else 0))
            assert ws + out_bytes_per * L.L31 > L.CAP
    # the blend: out against P
    for views in (2, 3):
        assert 4 * (L.L31 / 3.0) * views * 5 > L.CAP
    # canvas_to_u8: byte 2^32 of out is float 2^32 of the canvas, 16 GiB + 4 GiB = CAP before the straddling frame ends
    assert 4 * (L.L32 + 1) + (L.L32 + 1) > L.CAP
    # the seam: at most 655 360 cells a frame; with three views and cell 1 the workspace is 9 ints a cell, P 15 floats a pixel
    assert 4 * L.L31 + 4 * L.L31 * 15 / 9.0 > L.CAP


# ------------------------------------------------------------------------------------------------ 3. the refusals cited from here
def test_multiband_plan_refuses_a_frame_of_2_31_floats():
    """mb_plan (csrc/blend.hip): offsets inside one frame's workspace are ints in the kernels, so frame_floats < 2^31 - 1; frames x
    planes ride in gridDim.z, so frames * 4 * (views - 1) <= 65535.  Refused by the workspace query and by both entries."""
    from stabstitch2_amd import _blend
    B = _blend.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    # two views, no bands: 8 planes of hc x wc a frame
    assert L.multiband_plan(2, 16384, 16380, 0) == 8 * 16384 * 16380 < (1 << 31) - 1
    assert B.ssb_multiband_workspace_floats(1, 2, 16384, 16380, 0) == 8 * 16384 * 16380
    assert L.multiband_plan(2, 16384, 16384, 0) == 1 << 31
    assert B.ssb_multiband_workspace_floats(1, 2, 16384, 16384, 0) == -1
    assert B.ssb_multiband_workspace_floats(1, 3, 32768, 32768, 0) == -1
    assert L.multiband_plan(3, 16384, 12000, 5) > (1 << 31) and B.ssb_multiband_workspace_floats(1, 3, 16384, 12000, 5) == -1
    for fn in (B.ssb_multiband_blend, B.ssb_multiband_blend_u8):
        assert fn(p, p, p, 1 << 40, 1, 2, 16384, 16384, 0, None) == ERR_ARG
    # the grid: 16383 frames of two views ride (65532 planes), 16384 do not; three views: 8191 and 8192
    assert B.ssb_multiband_workspace_floats(16383, 2, 8, 8, 0) == 16383 * L.multiband_plan(2, 8, 8, 0)
    assert B.ssb_multiband_workspace_floats(16384, 2, 8, 8, 0) == -1
    assert B.ssb_multiband_workspace_floats(8191, 3, 8, 8, 0) > 0 and B.ssb_multiband_workspace_floats(8192, 3, 8, 8, 0) == -1
    for fn in (B.ssb_multiband_blend, B.ssb_multiband_blend_u8):
        assert fn(p, p, p, 1 << 40, 16384, 2, 8, 8, 0, None) == ERR_ARG
    # frames whose workspace passes 2^31 floats TOGETHER are taken: the frame offset is 64 bits (the GPU cases run such calls)
    assert B.ssb_multiband_workspace_floats(24, 2, 3072, 3048, 2) == 24 * L.multiband_plan(2, 3072, 3048, 2) > (1 << 31)
    assert all(v == 0.0 for v in buf)


def test_frame_io_refuses_a_frame_of_2_31_pixels(built_lib):
    """ss_ingest_u8 and ss_canvas_to_u8 address n * h * w with 64 bits, but the pixels of ONE frame are an int in their kernels:
    h * w <= 2^31 - 1, SS_ERR_ARG beyond, before any launch."""
    buf = (ctypes.c_float * 64)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    for h, w in ((46341, 46341), (32768, 65536), (65536, 65536), (2, 1 << 30)):
        assert h * w > (1 << 31) - 1
        assert built_lib.ss_ingest_u8(p, p, None, 1, h, w, 0, 0, None) == ERR_ARG, (h, w)
        assert built_lib.ss_ingest_u8(p, None, p, 1, h, w, 36, 48, None) == ERR_ARG, (h, w)
        assert built_lib.ss_canvas_to_u8(p, p, 1, h, w, None) == ERR_ARG, (h, w)
        assert built_lib.ss_ingest_u8(p, p, None, 0, h, w, 0, 0, None) == ERR_ARG            # even with nothing to do
    assert 46340 * 46341 <= (1 << 31) - 1
    assert built_lib.ss_ingest_u8(p, p, None, 0, 46340, 46341, 0, 0, None) == 0              # n = 0 returns before a launch
    assert built_lib.ss_canvas_to_u8(p, p, 0, 46340, 46341, None) == 0
    assert all(v == 0.0 for v in buf)


def test_conv_engine_refuses_what_32_bits_cannot_address(built_lib):
    """The conv engine addresses 32 bits on purpose (buffer descriptors): each entry returns SS_ERR_UNSUPPORTED for sizes past its
    limits, before any launch.  16 images of 1024 x 1024 x 64 are 2^32 bytes of input."""
    buf = (ctypes.c_float * 64)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    n, h, w, c = 16, 1024, 1024, 64
    assert n * h * w * c * 4 == 1 << 32
    Lb = built_lib
    assert Lb.ss_conv_nhwc(p, p, None, None, p, n, 1, h, w, c, c, 1, 3, 3, 1, 0, 1, 1, 0, c, 1, 0, 0, 0, None, 0, None) == ERR_UNSUPPORTED
    assert Lb.ss_conv_nhwc(p, p, None, None, p, n // 2, 1, h, w, c, c, 1, 3, 3, 1, 0, 1, 1, 0, c, 1, 0, 0, 0, None, 0, None) == ERR_UNSUPPORTED
    assert Lb.ss_conv_pool2_nhwc(p, p, None, p, n, h, w, c, c, 3, 3, 1, 1, 1, 1, c, 1, 0, 0, 0, None, 0, None) == ERR_UNSUPPORTED
    for name in ('ss_conv3x3_wino_nhwc', 'ss_conv3x3_wino3_nhwc', 'ss_conv3x3_wino43_nhwc'):
        assert getattr(Lb, name)(p, p, None, None, p, n, h, w, c, c, 0, c, 1, 0, 0, 0, None) == ERR_UNSUPPORTED, name
    assert Lb.ss_conv3x3_wino_pool2_nhwc(p, p, None, p, n, h, w, c, c, 0, c, 1, 0, 0, 0, None) == ERR_UNSUPPORTED
    # the stem: 3-channel frames, 12 bytes a padded pixel: 350 frames of 1024 x 1016 (+ 8) are 4.4e9 bytes
    assert 350 * 1024 * (1016 + 8) * 12 >= 1 << 32
    assert Lb.ss_stem_pool(p, p, None, p, 350, 1024, 1016, 1, 0, None) == ERR_UNSUPPORTED
    assert 350 * 1024 * (1016 + 8) * 3 * 4 >= 1 << 31
    assert Lb.ss_conv_stem3(p, p, None, p, 350, 1024, 1016, 64, 1, 64, 1, 0, 0, 0, None) == ERR_UNSUPPORTED
    assert all(v == 0.0 for v in buf)


def test_counts_past_the_grid_are_refused(built_lib):
    """The wide entries that ride frames (items, rows) in a 16-bit grid axis refuse one more than it holds with SS_ERR_ARG, before any
    launch and before any partial work: otherwise valid arguments, host pointers."""
    Lb = built_lib
    buf = (ctypes.c_double * 4096)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    views = (ctypes.c_void_p * 3)(p.value, p.value, p.value)
    big = 65536
    # LINEAR clip, all four entries: frames <= 65535
    for name in ('ss_render_linear_clip', 'ss_render_linear_clip_u8'):
        assert getattr(Lb, name)(views, p, p, p, None, big, 2, 8, 8, 16, 16, 0, p, None) == ERR_ARG, name
    for name in ('ss_render_linear_clip_gains', 'ss_render_linear_clip_u8_gains'):
        assert getattr(Lb, name)(views, p, p, p, None, big, 2, 8, 8, 16, 16, 0, p, p, None) == ERR_ARG, name
    # exposure: frames <= 65535 (the footprint row is the right one for two views on 45 x 150)
    per = Lb.ss_render_footprint_floats(2, 45, 150)
    for frames, want in ((big, ERR_ARG), (big + 1, ERR_ARG)):
        assert Lb.ss_exposure_update(views, 0, 0, p, per, per, frames, 2, 4, 4, 45, 150, 0, 0.1, 10.0, 0.1, 4.0, 251.0, 16, 0.5, 2.0, p, p,
                                     None, None) == want, ('ss_exposure_update', frames)
    # NV12 in and out: n <= 65535, and the rows of a frame in grid.y
    uv = ctypes.c_void_p(p.value + 4096)
    assert Lb.ss_ingest_nv12(p, uv, 16, 0, p, p, big, 12, 16, 6, 8, None) == ERR_ARG, 'ss_ingest_nv12'
    assert Lb.ss_ingest_nv12(p, uv, 16, 0, p, None, 1, 262144, 16, 6, 8, None) == ERR_ARG
    assert Lb.ss_bgr_to_nv12(p, p, uv, 16, 0, big, 12, 16, None) == ERR_ARG, 'ss_bgr_to_nv12'
    assert Lb.ss_bgr_to_nv12(p, p, uv, 16, 0, 1, 524288, 16, None) == ERR_ARG
    # packed frames in: with lr the frames ride in grid.z -- refused BEFORE the hr planes are launched (hr is host memory here)
    assert Lb.ss_ingest_u8(p, p, p, big, 4, 4, 2, 2, None) == ERR_ARG, 'ss_ingest_u8'
    assert Lb.ss_ingest_u8(p, p, p, 1, 4, 4, 262144, 2, None) == ERR_ARG
    # the dense warp: items in grid.z, row tiles in grid.y
    for name in ('ss_tps_warp_nchw', 'ss_tps_warp_mask_nchw'):
        assert getattr(Lb, name)(p, p, p, p, big, 3, 8, 8, 16, 16, 0, None) == ERR_ARG, name
        assert getattr(Lb, name)(p, p, p, p, 1, 3, 8, 8, 524288, 16, 0, None) == ERR_ARG, name
    # the metric: frames in grid.z, rows in grid.y (refused before its workspace is cleared)
    assert Lb.ss_alignment_psnr_ssim(p, p, p, p, big, 8, 8, None) == ERR_ARG, 'ss_alignment_psnr_ssim'
    assert Lb.ss_alignment_psnr_ssim(p, p, p, p, 1, 262144, 8, None) == ERR_ARG
    # layout plumbing: the pixels of ONE image are an int in the kernels
    assert Lb.ss_nchw_to_nhwc(p, p, 1, 3, 46341, 46341, 4, None) == ERR_ARG, 'ss_nchw_to_nhwc'
    assert all(v == 0.0 for v in buf)
