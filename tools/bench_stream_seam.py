#!/usr/bin/env python
"""MULTIBAND's two seams per steady-state push of OnlineStitcher, side by side (tools/bench_stream_multiband.py with seam=).
    python tools/bench_stream_seam.py [--pushes 300] [--rounds 3] [--height 720 --width 1280] [--bands 5] [--cell C] [--commit ID]
                                      [--out FILE] [--seams geometric,dp] [--only SEAM --many]
On one canvas box, in one process, per seam: push_u8 in ms per push, push_many_u8 at k = 8 in ms per FRAME; the geometric seam's
push_u8 twice (G, G': the run-to-run spread).  Windows interleaved over all units, repeated `rounds` times; per unit the median window
and the spread between its windows.  seam='dp' adds three launches per call (cost, dp, paint: DESIGN.md 7f) between the warp and the
blend, launched by the push behind the graph (the node count beside it is the graph's alone).
The yardstick for the geometric rows is tools/bench_stream_multiband.py --modes AVERAGE,MULTIBAND of the parent commit in the same
session: they run the same launches and must not move beyond the A/A spread.  --seams geometric runs on a commit without the feature
too.  --only dp [--many]: that unit alone (for a kernel trace:
rocprofv3 --kernel-trace --stats -- python tools/bench_stream_seam.py --only dp --pushes 40 --rounds 1).
profiles/stream_seam_720p.txt holds the output."""
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
    ap.add_argument('--cell', type=int, default=None)
    ap.add_argument('--commit', default='unknown')
    ap.add_argument('--out', default=None)
    ap.add_argument('--seams', default='geometric,dp')
    ap.add_argument('--only', default=None)
    ap.add_argument('--many', action='store_true')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.set_grad_enabled(False)
    nets, _ = bench.build_nets(dev)
    h, w = args.height, args.width
    hr, _ = synth.make_clip_device(N, h, w, seed=0, views=2, device=dev)
    u8 = hr.permute(0, 1, 3, 4, 2).round().clamp(0, 255).to(torch.uint8).contiguous()
    seams = [args.only] if args.only else args.seams.split(',')
    lines = ['MULTIBAND seams, OnlineStitcher steady state, %dx%d, synthetic nets and texture; %d pushes per window, %d rounds; %d bands, '
             'seam cell %s' % (h, w, args.pushes, args.rounds, args.bands, args.cell or 'default'),
             'GPU %s, commit %s' % (torch.cuda.get_device_name(0), args.commit)]
    probe = online.OnlineStitcher(nets, h, w, fusion_mode='AVERAGE')
    for t in range(8):
        probe.push_u8(u8[0][t], u8[1][t])
    box = probe.canvas_box
    del probe

    def unit(seam, many):
        kw = dict(seam='dp', seam_cell=args.cell) if seam == 'dp' else {}      # (the geometric seam: as a commit without seam= builds it)
        st = online.OnlineStitcher(nets, h, w, fusion_mode='MULTIBAND', bands=args.bands, canvas=box, **kw)
        if many:
            return st, (lambda i: st.push_many_u8(u8[0][(i % 2) * K:(i % 2) * K + K], u8[1][(i % 2) * K:(i % 2) * K + K])), K
        return st, (lambda i: st.push_u8(u8[0][i % N], u8[1][i % N])), 1

    one_name, many_name = (lambda m: '%-10s push_u8          ' % m), (lambda m: '%-10s push_many_u8 k=%d ' % (m, K))
    kinds = []
    for m in seams:
        if not args.only or not args.many:
            kinds.append((one_name(m), m, False))
        if m == 'geometric' and not args.only:
            kinds.append((one_name("geometric'"), m, False))
        if not args.only or args.many:
            kinds.append((many_name(m), m, True))
    units = []
    for name, seam, many in kinds:
        st, push, per = unit(seam, many)
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
    if not args.only and seams[0] == 'geometric':
        a, a2 = one_name('geometric'), one_name("geometric'")
        aa = max(abs(med[a] - med[a2]), max(ms[a]) - min(ms[a]), max(ms[a2]) - min(ms[a2]))
        lines.append('  A/A spread %.4f ms' % aa)
        for m in seams[1:]:
            d1, dk = med[one_name(m)] - med[a], med[many_name(m)] - med[many_name('geometric')]
            lines.append('  %s - geometric: push_u8 %+.4f ms (%+.2f %%, x %.2f); push_many_u8 %+.4f ms per frame (%+.2f %%, x %.2f)'
                         % (m, d1, 100.0 * d1 / med[a], med[one_name(m)] / med[a], dk, 100.0 * dk / med[many_name('geometric')],
                            med[many_name(m)] / med[many_name('geometric')]))
    print('\n'.join(lines), flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
