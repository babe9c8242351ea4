#!/usr/bin/env python
"""The four fusion modes per steady-state push of OnlineStitcher, side by side (tools/bench_stream_feather.py with MULTIBAND).
    python tools/bench_stream_multiband.py [--pushes 300] [--rounds 3] [--height 720 --width 1280] [--bands 5] [--commit ID]
                                           [--out FILE] [--modes AVERAGE,LINEAR,FEATHER,MULTIBAND] [--only MODE --many]
On one canvas box, in one process, per fusion mode: push_u8 in ms per push, push_many_u8 at k = 8 in ms per FRAME; AVERAGE's push_u8
twice (A, A': the run-to-run spread).  Windows interleaved over all units, repeated `rounds` times; per unit the median window and the
spread between its windows.  MULTIBAND is reported against LINEAR: the warp launch and the 2 * bands + 2 pyramid launches are launched
by the push behind the graph (the node count beside it is the graph's alone).
The yardstick for the three older modes is tools/bench_stream_feather.py of the parent commit in the same session: they must not
move beyond their A/A spread.  --only MULTIBAND [--many]: that unit alone (for a kernel trace:
rocprofv3 --kernel-trace --stats -- python tools/bench_stream_multiband.py --only MULTIBAND --pushes 40 --rounds 1).
profiles/stream_multiband_720p.txt holds the output."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault('GPU_MAX_HW_QUEUES', '16')
import torch

import bench
from bench_stream_feather import K, N, window
from stabstitch2_amd import online, synth


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pushes', type=int, default=300)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--height', type=int, default=720)
    ap.add_argument('--width', type=int, default=1280)
    ap.add_argument('--bands', type=int, default=5)
    ap.add_argument('--commit', default='unknown')
    ap.add_argument('--out', default=None)
    ap.add_argument('--modes', default='AVERAGE,LINEAR,FEATHER,MULTIBAND')
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
    lines = ['streaming fusion modes, OnlineStitcher steady state, %dx%d, synthetic nets and texture; %d pushes per window, %d rounds; '
             'MULTIBAND with %d bands' % (h, w, args.pushes, args.rounds, args.bands),
             'GPU %s, commit %s' % (torch.cuda.get_device_name(0), args.commit)]
    probe = online.OnlineStitcher(nets, h, w, fusion_mode='AVERAGE')
    for t in range(8):
        probe.push_u8(u8[0][t], u8[1][t])
    box = probe.canvas_box
    del probe

    def unit(fusion, many):
        kw = dict(bands=args.bands) if fusion == 'MULTIBAND' else {}
        st = online.OnlineStitcher(nets, h, w, fusion_mode=fusion, canvas=box, **kw)
        if many:
            return st, (lambda i: st.push_many_u8(u8[0][(i % 2) * K:(i % 2) * K + K], u8[1][(i % 2) * K:(i % 2) * K + K])), K
        return st, (lambda i: st.push_u8(u8[0][i % N], u8[1][i % N])), 1

    one_name, many_name = (lambda m: '%-9s push_u8          ' % m), (lambda m: '%-9s push_many_u8 k=%d ' % (m, K))
    kinds = []
    for m in modes:
        if not args.only or not args.many:
            kinds.append((one_name(m), m, False))
        if m == 'AVERAGE' and not args.only:
            kinds.append((one_name("AVERAGE'"), m, False))
        if not args.only or args.many:
            kinds.append((many_name(m), m, True))
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
        a, a2 = one_name('AVERAGE'), one_name("AVERAGE'")
        aa = max(abs(med[a] - med[a2]), max(ms[a]) - min(ms[a]), max(ms[a2]) - min(ms[a2]))
        lines.append('  A/A spread %.4f ms' % aa)
        for m in modes[1:]:
            for ref in ('AVERAGE', 'LINEAR'):
                if ref == m or ref not in modes:
                    continue
                d1, dk = med[one_name(m)] - med[one_name(ref)], med[many_name(m)] - med[many_name(ref)]
                lines.append('  %s - %s: push_u8 %+.4f ms (%+.2f %%, x %.2f); push_many_u8 %+.4f ms per frame (%+.2f %%, x %.2f)'
                             % (m, ref, d1, 100.0 * d1 / med[one_name(ref)], med[one_name(m)] / med[one_name(ref)],
                                dk, 100.0 * dk / med[many_name(ref)], med[many_name(m)] / med[many_name(ref)]))
    print('\n'.join(lines), flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
