#!/usr/bin/env python
"""Steady-state streaming with LINEAR fusion: the direct render (online.DIRECT_LINEAR: the graph ends with the splines, the push
renders through ss_render_linear_frames) against the in-graph per-frame chain, A/B in ONE process.
    python tools/bench_stream_linear.py [--pushes 300] [--rounds 3] [--streams 8] [--height 720 --width 1280] [--out FILE]
Four cases: OnlineStitcher.push, OnlineStitcher.push_u8, MultiOnlineStitcher(streams) on its own canvases, ThreeViewOnlineStitcher.push.
Per case two stitchers per setting; their windows of `pushes` pushes are interleaved (off, on, off, on, ...) and repeated `rounds`
times, so both settings see the same clocks and the same neighbours.  Per setting: the median window (ms per push, frames/s) and the
spread between the windows of that one setting (max - min) -- a difference between the settings below that spread is not a difference.
profiles/stream_linear_720p.txt holds the output."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault('GPU_MAX_HW_QUEUES', '16')
import torch

import bench
from stabstitch2_amd import online, synth

N = 16                                   # frames of the synthetic clip; the pushes cycle through it


def build(cls, flag, *a, **kw):
    online.DIRECT_LINEAR = flag          # read when a stitcher is constructed
    try:
        return cls(*a, fusion_mode='LINEAR', **kw)
    finally:
        online.DIRECT_LINEAR = True


def window(push, pushes):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(pushes):
        push(t % N)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / pushes * 1e3


def run_case(name, make, frames_per_push, args, lines):
    """make(flag) -> (stitcher, push(i)).  Two stitchers per setting, warmed up past the window fill and the capture."""
    units = [(flag, k) + make(flag) for k in range(2) for flag in (False, True)]          # off0, on0, off1, on1
    for _, _, st, push in units:
        for t in range(12):
            push(t)
    torch.cuda.synchronize()
    ms = {False: [], True: []}
    for _ in range(args.rounds):
        for flag, _, st, push in units:
            ms[flag].append(window(push, args.pushes))
    st_off, st_on = units[0][2], units[1][2]
    assert st_on._direct() and not st_off._direct()
    sizes = getattr(st_on, 'canvas_sizes', None) or [(st_on.hc, st_on.wc)]
    lines.append('%s   (%d frame(s) per push, canvas %s)' % (name, frames_per_push, ' '.join('%dx%d' % s for s in sizes)))
    med = {}
    for flag in (False, True):
        v = ms[flag]
        med[flag] = statistics.median(v)
        lines.append('  DIRECT_LINEAR %-3s  %.4f ms per push  %8.1f frames/s   spread %.4f ms over %d windows of %d pushes [%s]   graph nodes %s'
                     % ('on' if flag else 'off', med[flag], frames_per_push * 1e3 / med[flag], max(v) - min(v), len(v), args.pushes,
                        ' '.join('%.4f' % x for x in v), (st_on if flag else st_off).graph_nodes))
    spread = max(max(ms[f]) - min(ms[f]) for f in (False, True))
    d = med[True] - med[False]
    lines.append('  direct - in-graph: %+.4f ms per push (%+.1f %%); larger spread of one setting %.4f ms -> %s'
                 % (d, 100.0 * d / med[False], spread, 'direct is slower' if d > spread else
                    ('direct is faster' if -d > spread else 'no difference beyond the spread')))
    print('\n'.join(lines[-4:]), flush=True)
    del units
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pushes', type=int, default=300)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--streams', type=int, default=8)
    ap.add_argument('--height', type=int, default=720)
    ap.add_argument('--width', type=int, default=1280)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.set_grad_enabled(False)
    nets, _ = bench.build_nets(dev)
    h, w, S = args.height, args.width, args.streams
    hr, lr = synth.make_clip_device(N, h, w, seed=0, views=3, device=dev)
    u8 = hr[:2].permute(0, 1, 3, 4, 2).round().clamp(0, 255).to(torch.uint8).contiguous()
    lines = ['streaming, fusion LINEAR, %dx%d, synthetic nets and texture; %d pushes per window, %d rounds, 2 stitchers per setting'
             % (h, w, args.pushes, args.rounds)]

    def single(flag):
        st = build(online.OnlineStitcher, flag, nets, h, w)
        return st, lambda i: st.push(hr[0][i:i + 1], hr[1][i:i + 1], lr[0][i:i + 1], lr[1][i:i + 1])

    def single_u8(flag):
        st = build(online.OnlineStitcher, flag, nets, h, w)
        return st, lambda i: st.push_u8(u8[0][i], u8[1][i])

    # stream s runs s frames ahead in the clip: [N,S,...] batches, built once
    idx = [[(i + s) % N for s in range(S)] for i in range(N)]
    mh = [torch.stack([hr[v][idx[i]] for i in range(N)]) for v in range(2)]
    ml = [torch.stack([lr[v][idx[i]] for i in range(N)]) for v in range(2)]

    def multi(flag):
        st = build(online.MultiOnlineStitcher, flag, nets, h, w, streams=S)
        return st, lambda i: st.push(mh[0][i], mh[1][i], ml[0][i], ml[1][i])

    def three(flag):
        st = build(online.ThreeViewOnlineStitcher, flag, nets, h, w)
        return st, lambda i: st.push(hr[0][i:i + 1], hr[1][i:i + 1], hr[2][i:i + 1], lr[0][i:i + 1], lr[1][i:i + 1], lr[2][i:i + 1])

    run_case('OnlineStitcher.push', single, 1, args, lines)
    run_case('OnlineStitcher.push_u8', single_u8, 1, args, lines)
    run_case('MultiOnlineStitcher(streams=%d).push' % S, multi, S, args, lines)
    run_case('ThreeViewOnlineStitcher.push', three, 1, args, lines)
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
