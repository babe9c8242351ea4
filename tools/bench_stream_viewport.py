#!/usr/bin/env python
"""Streaming with a fixed output size: what `viewport=` + grow='refit' costs per push, and what a canvas growth costs in ONE push.
    python tools/bench_stream_viewport.py [--pushes 300] [--rounds 3] [--height 720 --width 1280] [--out FILE]
Per fusion mode (AVERAGE, LINEAR), OnlineStitcher.push in one process:
  steady state -- the plain stitcher twice (A/A: the run-to-run spread) and the same stitcher with a viewport of its natural size on
      its own box under grow='refit' (the refit rides in the launch that carries the watcher: no graph node more); windows of
      `pushes` pushes, interleaved (A, A', refit, A, A', refit, ...) and repeated `rounds` times; per stitcher the median window and
      the spread between its windows -- a difference below the spread is not a difference;
  drifting stream -- the views slide apart by 10 % of the width (SpatialNet's stage-1 head bias walks, as tests/test_gpu_round5.py's
      _push_drifting does) over 44 pushes, every push timed on its own (host clock around push + synchronize): the MAXIMUM single-push
      latency under grow='recapture' (new output, new capture inside the push that grows) and under grow='refit' (four floats
      rewritten on the device), beside the median push of the same run and the number of growths.
profiles/stream_viewport_720p.txt holds the output."""
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


def window(push, pushes):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(pushes):
        push(t % N)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / pushes * 1e3


def steady(fusion, nets, hr, lr, h, w, args, lines):
    mk = lambda **kw: online.OnlineStitcher(nets, h, w, fusion_mode=fusion, **kw)
    pusher = lambda st: (lambda i: st.push(hr[0][i:i + 1], hr[1][i:i + 1], lr[0][i:i + 1], lr[1][i:i + 1]))
    a = mk()
    for t in range(12):
        pusher(a)(t)
    box, size = a.canvas_box, (a.hc, a.wc)
    units = [('plain A ', a), ('plain A\'', mk(canvas=box)), ('refit   ', mk(canvas=box, viewport=size, grow='refit'))]
    for _, st in units[1:]:
        for t in range(12):
            pusher(st)(t)
    torch.cuda.synchronize()
    assert all((st.hc, st.wc) == size for _, st in units)
    ms = {name: [] for name, _ in units}
    for _ in range(args.rounds):
        for name, st in units:
            ms[name].append(window(pusher(st), args.pushes))
    lines.append('%s, steady state: canvas %dx%d, box %s' % (fusion, size[0], size[1], ' '.join('%.2f' % v for v in box)))
    med = {}
    for name, st in units:
        v = ms[name]
        med[name] = statistics.median(v)
        lines.append('  %s %.4f ms per push  %8.1f frames/s   spread %.4f ms over %d windows of %d pushes [%s]   graph nodes %s'
                     % (name, med[name], 1e3 / med[name], max(v) - min(v), len(v), args.pushes, ' '.join('%.4f' % x for x in v),
                        st.graph_nodes))
    names = [n for n, _ in units]
    aa = abs(med[names[0]] - med[names[1]])
    spread = max(max(ms[n]) - min(ms[n]) for n in names)
    d = med[names[2]] - min(med[names[0]], med[names[1]])
    lines.append('  A/A: |A - A\'| %.4f ms, largest spread of one stitcher %.4f ms;  refit - faster plain: %+.4f ms per push (%+.2f %%) -> %s'
                 % (aa, spread, d, 100.0 * d / min(med[names[0]], med[names[1]]),
                    'inside the A/A spread' if abs(d) <= max(aa, spread) else 'OUTSIDE the A/A spread'))
    rep = units[2][1].overflow_report()
    lines.append('  refit stitcher afterwards: epoch %d, clipped %d of %d frames' % (rep['canvas_epoch'], rep['clipped_frames'], rep['frames_seen']))
    print('\n'.join(lines[-6:]), flush=True)
    return size


def drifting(fusion, grow, nets, hr, lr, h, w, size, lines, pushes=44, start=20, steps=12):
    kw = dict(viewport=size) if grow == 'refit' else {}
    st = online.OnlineStitcher(nets, h, w, fusion_mode=fusion, grow=grow, **kw)
    bias = nets[0]._prepared()['r1']['fc'][2][1]          # the tensor the kernels (and the captured graph) read: edited in place
    base = bias[0::2].clone()
    step = -6.0                                             # LR px per frame, 72 px in all: the drift of the test
    ms, epochs = [], []
    try:
        for t in range(pushes):
            bias[0::2] = base + step * min(max(t - start + 1, 0), steps)
            i = t % N
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st.push(hr[0][i:i + 1], hr[1][i:i + 1], lr[0][i:i + 1], lr[1][i:i + 1])
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
            epochs.append(st.canvas_epoch)
    finally:
        bias[0::2] = base
    rep = st.overflow_report()
    steady_ms = ms[9:]                                      # behind the window fill and the first capture
    grew = [t for t in range(1, pushes) if epochs[t] != epochs[t - 1]]
    worst = max(range(9, pushes), key=lambda t: ms[t])
    lines.append('  grow=%-9s max single push %.3f ms (push %d), median %.3f ms, growths %d (seen at pushes %s), clipped %d of %d, canvas %dx%d'
                 % (grow, ms[worst], worst, statistics.median(steady_ms), rep['canvas_epoch'], grew, rep['clipped_frames'],
                    rep['frames_seen'], st.hc, st.wc))
    print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pushes', type=int, default=300)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--height', type=int, default=720)
    ap.add_argument('--width', type=int, default=1280)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.set_grad_enabled(False)
    nets, _ = bench.build_nets(dev)
    h, w = args.height, args.width
    hr, lr = synth.make_clip_device(N, h, w, seed=0, views=2, device=dev)
    lines = ['streaming with a fixed output size, OnlineStitcher.push, %dx%d, synthetic nets and texture; %d pushes per window, %d rounds'
             % (h, w, args.pushes, args.rounds)]
    for fusion in ('AVERAGE', 'LINEAR'):
        size = steady(fusion, nets, hr, lr, h, w, args, lines)
        lines.append('%s, drifting stream (44 pushes, each timed alone; the first 9 -- window fill, first capture -- left out of max and median):'
                     % fusion)
        for grow in ('recapture', 'refit'):
            drifting(fusion, grow, nets, hr, lr, h, w, size, lines)
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
