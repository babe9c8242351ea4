#!/usr/bin/env python
"""The three fusion modes per steady-state push of OnlineStitcher, side by side.
    python tools/bench_stream_feather.py [--pushes 300] [--rounds 3] [--height 720 --width 1280] [--commit ID] [--out FILE]
                                         [--modes AVERAGE,LINEAR,FEATHER] [--only MODE --many]
On one canvas box, in one process, per fusion mode:
  push_u8            ms per push;
  push_many_u8 k=8   ms per FRAME (a call's time / 8);
AVERAGE's push_u8 twice (A, A': the run-to-run spread).  Windows of `pushes` pushes (pushes / 8 calls for push_many_u8), interleaved
over all units and repeated `rounds` times; per unit the median window and the spread between its windows -- a difference below the
A/A spread is not a difference.  The graph's node count stands beside every unit: FEATHER's equals AVERAGE's (the same launches,
another instantiation of the render kernel).
--modes AVERAGE,LINEAR runs on a checkout from before FEATHER existed (the yardstick: AVERAGE and LINEAR of this build must match it
within the spread -- their kernels are the same machine code).  --only MODE [--many]: that unit alone, no comparisons (for a kernel
trace: rocprofv3 --kernel-trace -- python tools/bench_stream_feather.py --only FEATHER --pushes 40 --rounds 1).
profiles/stream_feather_720p.txt holds the output."""
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


def window(push, calls, per_call):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(calls):
        push(t)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / (calls * per_call) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pushes', type=int, default=300)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--height', type=int, default=720)
    ap.add_argument('--width', type=int, default=1280)
    ap.add_argument('--commit', default='unknown')
    ap.add_argument('--out', default=None)
    ap.add_argument('--modes', default='AVERAGE,LINEAR,FEATHER')
    ap.add_argument('--only', default=None)
    ap.add_argument('--many', action='store_true')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.set_grad_enabled(False)
    nets, _ = bench.build_nets(dev)
    h, w = args.height, args.width
    hr, _ = synth.make_clip_device(N, h, w, seed=0, views=2, device=dev)
    u8 = hr.permute(0, 1, 3, 4, 2).round().clamp(0, 255).to(torch.uint8).contiguous()
    modes = [args.only] if args.only else args.modes.split(',')
    lines = ['streaming fusion modes, OnlineStitcher steady state, %dx%d, synthetic nets and texture; %d pushes per window, %d rounds'
             % (h, w, args.pushes, args.rounds), 'GPU %s, commit %s' % (torch.cuda.get_device_name(0), args.commit)]
    probe = online.OnlineStitcher(nets, h, w, fusion_mode='AVERAGE')
    for t in range(8):
        probe.push_u8(u8[0][t], u8[1][t])
    box = probe.canvas_box
    del probe

    def unit(fusion, many):
        st = online.OnlineStitcher(nets, h, w, fusion_mode=fusion, canvas=box)
        if many:
            return st, (lambda i: st.push_many_u8(u8[0][(i % 2) * K:(i % 2) * K + K], u8[1][(i % 2) * K:(i % 2) * K + K])), K
        return st, (lambda i: st.push_u8(u8[0][i % N], u8[1][i % N])), 1

    kinds = []
    for m in modes:
        if not args.only or not args.many:
            kinds.append(('%-8s push_u8          ' % m, m, False))
        if m == 'AVERAGE' and not args.only:
            kinds.append(("AVERAGE' push_u8          ", m, False))
        if not args.only or args.many:
            kinds.append(('%-8s push_many_u8 k=%d ' % (m, K), m, True))
    units = []
    for name, fusion, many in kinds:
        st, push, per = unit(fusion, many)
        for t in range(12):                  # the window fill, the capture, a few replays
            st.push_u8(u8[0][t], u8[1][t]) if t < 8 else push(t)
        units.append((name, st, push, per))
    torch.cuda.synchronize()
    ms = {name: [] for name, _, _, _ in units}
    for _ in range(args.rounds):
        for name, _, push, per in units:
            ms[name].append(window(push, max(1, args.pushes // per), per))
    lines.append('box %s, canvas %dx%d' % (' '.join('%.2f' % v for v in box), units[0][1].hc, units[0][1].wc))
    med = {}
    for name, st, _, per in units:
        v = ms[name]
        med[name] = statistics.median(v)
        nodes = st.graph_nodes if per == 1 else st.graph_nodes_batch.get(K)
        lines.append('  %s %.4f ms per frame  %8.1f frames/s   spread %.4f ms over %d windows [%s]   graph nodes %s'
                     % (name, med[name], 1e3 / med[name], max(v) - min(v), len(v), ' '.join('%.4f' % x for x in v), nodes))
    if not args.only and modes[0] == 'AVERAGE':
        a, a2 = kinds[0][0], kinds[1][0]
        aa = max(abs(med[a] - med[a2]), max(ms[a]) - min(ms[a]), max(ms[a2]) - min(ms[a2]))
        lines.append('  A/A spread %.4f ms' % aa)
        verdict = lambda x: 'inside the A/A spread' if abs(x) <= aa else 'OUTSIDE the A/A spread'
        base = min(med[a], med[a2])
        for m in modes[1:]:
            one, many = med['%-8s push_u8          ' % m], med['%-8s push_many_u8 k=%d ' % (m, K)]
            lines.append('  %s - AVERAGE: push_u8 %+.4f ms (%+.2f %%) -> %s; push_many_u8 %+.4f ms per frame (%+.2f %%)'
                         % (m, one - base, 100.0 * (one - base) / base, verdict(one - base),
                            many - med['%-8s push_many_u8 k=%d ' % ('AVERAGE', K)],
                            100.0 * (many - med['%-8s push_many_u8 k=%d ' % ('AVERAGE', K)]) / med['%-8s push_many_u8 k=%d ' % ('AVERAGE', K)]))
        if 'FEATHER' in modes and 'LINEAR' in modes:
            f, l = med['%-8s push_u8          ' % 'FEATHER'], med['%-8s push_u8          ' % 'LINEAR']
            lines.append('  FEATHER - LINEAR: push_u8 %+.4f ms (%+.2f %%)' % (f - l, 100.0 * (f - l) / l))
    print('\n'.join(lines), flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
