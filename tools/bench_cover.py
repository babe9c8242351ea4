#!/usr/bin/env python
"""Coverage and the largest covered rectangle at 720p two-view on a 785 x 1995 canvas.
    python tools/bench_cover.py [--calls 1000] [--clip-calls 30] [--rounds 5] [--commit ID] [--out FILE]
ops.coverage_update at n = 1 and n = 32 frames, NORMAL and FAST, beside ops.render_average_clip on the same (src, T) and frames; then
ops.covered_rect on three bitmaps: the clip's own, all ones, and a staircase (row y covered up to column y wc / hc).
coverage_update is timed two ways: `fresh` -- an all-ones state copied in front of every call (one small copy launch more), every
tile evaluates every frame until its words are zero -- and `running` -- the state left by the previous call, what a stream pays from
its second frame on: the tiles whose words are already zero leave at once.  The render runs as the clip path runs it, skipping tiles
by footprint (`skip`), and once evaluating every view at every pixel (`all`), which is what the coverage pass does.
In one process; windows of calls interleaved over all units and repeated `rounds` times; per unit the median window and the spread
between its windows; the n = 32 render twice (A, A': the run-to-run spread).  Times are a host clock around a window of calls that
ends in a device synchronise, so they hold each path's launch overhead.
No threshold is fixed in advance.  profiles/cover_720p.txt holds the output."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

from bench_stream_feather import window
from stabstitch2_amd import ops, pipeline, synth

H, W, HC, WC, N = 720, 1280, 785, 1995, 32


def splines(dev, n):
    """n frames of two 720p views side by side on the canvas, an overlap of 565 columns, +- 6 px of seeded jitter per frame."""
    g = torch.Generator().manual_seed(3)
    ty, tx = torch.meshgrid(torch.linspace(0, 1, 7), torch.linspace(0, 1, 9), indexing='ij')
    meshes = []
    for x0 in (0.0, float(WC - W)):
        m = torch.stack((x0 + W * tx, 32.0 + H * ty), -1)[None] + (torch.rand((n, 7, 9, 2), generator=g) - 0.5) * 12.0
        meshes.append(m[None].contiguous().to(dev))
    box = torch.tensor([0.0, float(WC), 0.0, float(HC)], device=dev)
    _, _, src, T = pipeline.render_plan(meshes, H, W, prescaled=True, bbox=box, size=(HC, WC))
    return src, T


def pack(mask):
    """bool [hc, wc] -> int64 [hc, W64], bit i of word j = column 64 j + i."""
    hc, wc = mask.shape
    w64 = (wc + 63) // 64
    padded = np.zeros((hc, w64 * 64), dtype=np.uint64)
    padded[:, :wc] = mask
    return np.bitwise_or.reduce(padded.reshape(hc, w64, 64) << np.arange(64, dtype=np.uint64), axis=-1).view(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=1000)
    ap.add_argument('--clip-calls', type=int, default=30)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--commit', default='unknown')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_cover.py measures on the GPU; there is none here')
    dev = torch.device('cuda:0')
    torch.set_grad_enabled(False)
    hr, _ = synth.make_clip_device(N, H, W, seed=0, views=2, device=dev)
    clips = [hr[v].contiguous() for v in range(2)]
    src, T = splines(dev, N)
    fp = ops.render_footprints(src, T, H, W, HC, WC)
    out = torch.empty((N, 3, HC, WC), device=dev)
    ones = ops.coverage_state(HC, WC, dev)
    state = {m: ops.coverage_state(HC, WC, dev) for m in ('NORMAL', 'FAST')}

    def render(n, mode, skip):
        return lambda i: ops.render_average_clip([c[:n] for c in clips], src[:n], T[:n], HC, WC, mode, out=out[:n],
                                                 footprint=fp[:n] if skip else None)

    def fresh(n, mode):
        def call(i):
            state[mode].bitmap.copy_(ones.bitmap)
            ops.coverage_update(state[mode], src[:n], T[:n], H, W, mode)
        return call

    def running(n, mode):
        return lambda i: ops.coverage_update(state[mode], src[:n], T[:n], H, W, mode)

    # the three bitmaps of the search
    clip_state = ops.coverage_update(ops.coverage_state(HC, WC, dev), src, T, H, W, 'NORMAL')
    yy, xx = np.indices((HC, WC))
    stairs = ops.CoverageState(torch.from_numpy(pack(xx < yy * WC // HC)).to(dev), ones.ws, HC, WC)
    rects = {k: tuple(ops.covered_rect(s).cpu().tolist()) for k, s in (('clip', clip_state), ('ones', ones), ('staircase', stairs))}
    if rects['ones'] != (0, 0, HC, WC) or rects['clip'][2] * rects['clip'][3] <= 0:
        raise SystemExit('the rectangles are wrong: %s' % rects)
    # the clip's bitmap is what the renders' mask planes say
    mask = ops.multiband_warp([c[:2] for c in clips], src[:2], T[:2], HC, WC)[:, :, 4]
    bits = (ops.coverage(src[:2], T[:2], H, W, HC, WC)[..., None] >> torch.arange(64, device=dev)) & 1
    if not torch.equal(bits.reshape(2, HC, -1)[..., :WC].bool(), (mask >= 0.5).any(1)):
        raise SystemExit('the coverage differs from the mask planes')

    big, small = args.clip_calls, args.calls
    units = [('render_average_clip  n=32 NORMAL skip', render(N, 'NORMAL', True), big, N),
             ("render_average_clip' n=32 NORMAL skip", render(N, 'NORMAL', True), big, N),
             ('render_average_clip  n=32 NORMAL all ', render(N, 'NORMAL', False), big, N),
             ('render_average_clip  n=32 FAST   skip', render(N, 'FAST', True), big, N),
             ('coverage_update      n=32 NORMAL fresh', fresh(N, 'NORMAL'), big, N),
             ('coverage_update      n=32 FAST   fresh', fresh(N, 'FAST'), big, N),
             ('coverage_update      n=32 NORMAL running', running(N, 'NORMAL'), big, N),
             ('render_average_clip  n=1  NORMAL skip', render(1, 'NORMAL', True), small, 1),
             ('render_average_clip  n=1  FAST   skip', render(1, 'FAST', True), small, 1),
             ('coverage_update      n=1  NORMAL fresh', fresh(1, 'NORMAL'), small, 1),
             ('coverage_update      n=1  FAST   fresh', fresh(1, 'FAST'), small, 1),
             ('coverage_update      n=1  NORMAL running', running(1, 'NORMAL'), small, 1),
             ('coverage_update      n=1  FAST   running', running(1, 'FAST'), small, 1),
             ('covered_rect         clip     ', lambda i: ops.covered_rect(clip_state), small, 1),
             ('covered_rect         ones     ', lambda i: ops.covered_rect(ones), small, 1),
             ('covered_rect         staircase', lambda i: ops.covered_rect(stairs), small, 1)]
    lines = ['coverage and covered rectangle, two %dx%d views on a %dx%d canvas, synthetic splines; %d (n=32: %d) calls per window, '
             '%d rounds' % (H, W, HC, WC, small, big, args.rounds),
             'GPU %s, commit %s' % (torch.cuda.get_device_name(0), args.commit),
             'rectangles (y0, x0, h, w): clip %s, ones %s, staircase %s' % (rects['clip'], rects['ones'], rects['staircase']),
             'coverage of the first two frames == (mask plane >= 0.5).any(view), bit for bit']
    for _, fn, _, _ in units:                    # warm-up: every shape of the timed windows
        for i in range(5):
            fn(i)
    torch.cuda.synchronize()
    us = {name: [] for name, _, _, _ in units}
    for _ in range(args.rounds):
        for name, fn, calls, _ in units:
            us[name].append(window(fn, calls, 1) * 1e3)
    med = {}
    for name, _, _, n in units:
        v = us[name]
        med[name] = statistics.median(v)
        lines.append('  %-42s %9.1f us per call (%7.1f per frame)   spread %6.1f us over %d windows [%s]'
                     % (name, med[name], med[name] / n, max(v) - min(v), len(v), ' '.join('%.1f' % x for x in v)))
    a, a2 = units[0][0], units[1][0]
    aa = max(abs(med[a] - med[a2]), max(us[a]) - min(us[a]), max(us[a2]) - min(us[a2]))
    lines.append('  A/A spread of the n=32 render: %.1f us' % aa)
    for cov, ren in ((units[4][0], a), (units[5][0], units[3][0]), (units[4][0], units[2][0]), (units[9][0], units[7][0]),
                     (units[10][0], units[8][0])):
        lines.append('  %s / %s: x %.2f' % (' '.join(cov.split()), ' '.join(ren.split()), med[cov] / med[ren]))
    r = [med[units[k][0]] for k in (13, 14, 15)]
    lines.append('  covered_rect ones / clip: x %.2f; staircase / clip: x %.2f' % (r[1] / r[0], r[2] / r[0]))
    print('\n'.join(lines), flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
