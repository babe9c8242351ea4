#!/usr/bin/env python
"""What exposure compensation costs per steady-state push of OnlineStitcher.
    python tools/bench_stream_exposure.py [--pushes 300] [--rounds 3] [--height 720 --width 1280] [--commit ID] [--out FILE] [--off-only]
                                          [--only a|b|c|d --fusion AVERAGE|LINEAR]
Per fusion mode (AVERAGE, LINEAR), on one canvas box, in one process, view 2's channels scaled by (0.8, 0.9, 1.1):
  (a)  push_u8, exposure=None, twice (A, A': the run-to-run spread);
  (b)  push_u8, exposure=True;
  (c)  push_many_u8 at k = 8, exposure=None;        (d)  the same, exposure=True    (ms per FRAME: a call's time / 8).
Windows of `pushes` pushes (calls for (c), (d): pushes / 8 of them), interleaved over the units and repeated `rounds` times; per unit
the median window and the spread between its windows -- a difference below the A/A spread is not a difference.  The graph's node count
stands beside every unit: exposure adds no node to a direct-render push (the update runs outside the graph, in front of the render),
and the footprint launches to a LINEAR one.
--off-only: units (a) and (c) only, without the keyword -- runs on a checkout from before exposure= existed (the yardstick: the
exposure-off arm of this build must match it within the spread).  --only: that unit of that fusion mode alone, no comparisons (for a
kernel trace: rocprofv3 --kernel-trace -- python tools/bench_stream_exposure.py --only b --pushes 40 --rounds 1, then
tools/push_timeline.py).  profiles/stream_exposure_720p.txt holds the output."""
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
K = 8                                    # push_many_u8's batch
SCALE = (0.8, 0.9, 1.1)


def window(push, calls, per_call):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(calls):
        push(t)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / (calls * per_call) * 1e3


def run(fusion, nets, u8, h, w, args, lines):
    first = len(lines)
    probe = online.OnlineStitcher(nets, h, w, fusion_mode=fusion)
    for t in range(8):
        probe.push_u8(u8[0][t], u8[1][t])
    box = probe.canvas_box
    del probe

    def unit(exposure, many):
        kw = {} if args.off_only else {'exposure': exposure}
        st = online.OnlineStitcher(nets, h, w, fusion_mode=fusion, canvas=box, **kw)
        if many:
            return st, (lambda i: st.push_many_u8(u8[0][(i % 2) * K:(i % 2) * K + K], u8[1][(i % 2) * K:(i % 2) * K + K])), K
        return st, (lambda i: st.push_u8(u8[0][i % N], u8[1][i % N])), 1

    kinds = [('(a)  push_u8 off A          ', None, False), ('(a)  push_u8 off A\'         ', None, False)]
    if not args.off_only:
        kinds.append(('(b)  push_u8 exposure      ', True, False))
    kinds.append(('(c)  push_many_u8 k=8 off   ', None, True))
    if not args.off_only:
        kinds.append(('(d)  push_many_u8 k=8 exp. ', True, True))
    if args.only:
        kinds = [k for k in kinds if k[0].startswith('(%s)' % args.only)][:1]
    units = []
    for name, exposure, many in kinds:
        st, push, per = unit(exposure, many)
        for t in range(12):                  # the window fill, the capture, a few replays
            st.push_u8(u8[0][t], u8[1][t]) if t < 8 else push(t)
        units.append((name, st, push, per))
    torch.cuda.synchronize()
    ms = {name: [] for name, _, _, _ in units}
    for _ in range(args.rounds):
        for name, _, push, per in units:
            ms[name].append(window(push, max(1, args.pushes // per), per))
    lines.append('%s: box %s, canvas %dx%d' % (fusion, ' '.join('%.2f' % v for v in box), units[0][1].hc, units[0][1].wc))
    med = {}
    for name, st, _, per in units:
        v = ms[name]
        med[name] = statistics.median(v)
        nodes = st.graph_nodes if per == 1 else st.graph_nodes_batch.get(K)
        lines.append('  %s %.4f ms per frame  %8.1f frames/s   spread %.4f ms over %d windows [%s]   graph nodes %s'
                     % (name, med[name], 1e3 / med[name], max(v) - min(v), len(v), ' '.join('%.4f' % x for x in v), nodes))
    names = [n for n, _, _, _ in units]
    if args.only:
        print('\n'.join(lines[first:]), flush=True)
        return
    aa = max(abs(med[names[0]] - med[names[1]]), max(max(ms[n]) - min(ms[n]) for n in names[:2]))
    lines.append('  A/A spread %.4f ms' % aa)
    if not args.off_only:
        a = min(med[names[0]], med[names[1]])
        b, c, d = med[names[2]], med[names[3]], med[names[4]]
        verdict = lambda x: 'inside the A/A spread' if abs(x) <= aa else 'OUTSIDE the A/A spread'
        lines.append('  (b) - (a) = %+.4f ms (%+.2f %%): exposure on a push_u8 -> %s' % (b - a, 100.0 * (b - a) / a, verdict(b - a)))
        lines.append('  (d) - (c) = %+.4f ms (%+.2f %%) per frame: exposure on push_many_u8 at k = %d -> %s'
                     % (d - c, 100.0 * (d - c) / c, K, verdict(d - c)))
        g = units[2][1].exposure_gains
        lines.append('  gains after the run: view 1 %s, view 2 %s' % (' '.join('%.4f' % x for x in g[0]), ' '.join('%.4f' % x for x in g[1])))
    print('\n'.join(lines[first:]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pushes', type=int, default=300)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--height', type=int, default=720)
    ap.add_argument('--width', type=int, default=1280)
    ap.add_argument('--commit', default='unknown')
    ap.add_argument('--out', default=None)
    ap.add_argument('--off-only', action='store_true')
    ap.add_argument('--only', default=None, choices=('a', 'b', 'c', 'd'))
    ap.add_argument('--fusion', default=None, choices=('AVERAGE', 'LINEAR'))
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.set_grad_enabled(False)
    nets, _ = bench.build_nets(dev)
    h, w = args.height, args.width
    hr, _ = synth.make_clip_device(N, h, w, seed=0, views=2, device=dev)
    hr[1] = hr[1] * torch.tensor(SCALE, device=dev).view(1, 3, 1, 1)
    u8 = hr.permute(0, 1, 3, 4, 2).round().clamp(0, 255).to(torch.uint8).contiguous()
    lines = ['streaming exposure compensation, OnlineStitcher steady state, %dx%d, synthetic nets and texture, view 2 x (%s); '
             '%d pushes per window, %d rounds%s' % (h, w, ', '.join('%.1f' % s for s in SCALE), args.pushes, args.rounds,
                                                    ' (exposure-off arms only)' if args.off_only else ''),
             'GPU %s, commit %s' % (torch.cuda.get_device_name(0), args.commit)]
    print('\n'.join(lines), flush=True)
    for fusion in ((args.fusion,) if args.fusion else ('AVERAGE', 'LINEAR')):
        run(fusion, nets, u8, h, w, args, lines)
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
