#!/usr/bin/env python
"""MULTIBAND's warp, two ways, on one 720p frame pair and a 785 x 1995 canvas.
    python tools/bench_multiband_warp.py [--calls 4000] [--rounds 5] [--mode NORMAL] [--commit ID] [--out FILE]
The two-step path -- ops.multiband_stack (a weight-plane copy and one ingest per view into U [2][4][720][1280]) followed by
ops.tps_warp(with_mask=True) -- against the direct warp ops.multiband_warp (libstabstitch_mbwarp.so), from fp32 planes and from uint8
frames, without gains and with them.  In one process; windows of `calls` calls interleaved over all units and repeated `rounds`
times; per unit the median window and the spread between its windows; the two-step fp32 path twice (A, A': the run-to-run spread).
Times are a host clock around `calls` calls that end in a device synchronise, so they hold the launch overhead of each path: one
launch for the direct warp, a copy kernel per plane group and the warp for the two-step path.  Before anything is timed the planes
of every unit are compared: without gains they must be equal bit for bit.
No threshold is fixed in advance: the output says which path was faster and by how much against the A/A spread.
profiles/multiband_warp_720p.txt holds the output."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

from bench_stream_feather import window
from stabstitch2_amd import ops, pipeline, synth

H, W, HC, WC = 720, 1280, 785, 1995


def splines(dev):
    """Two 720p views side by side on the canvas, an overlap of 565 columns, +- 6 px of seeded jitter on the control points."""
    g = torch.Generator().manual_seed(3)
    ty, tx = torch.meshgrid(torch.linspace(0, 1, 7), torch.linspace(0, 1, 9), indexing='ij')
    meshes = []
    for x0 in (0.0, float(WC - W)):
        m = torch.stack((x0 + W * tx, 32.0 + H * ty), -1) + (torch.rand((7, 9, 2), generator=g) - 0.5) * 12.0
        meshes.append(m[None, None].contiguous().to(dev))
    box = torch.tensor([0.0, float(WC), 0.0, float(HC)], device=dev)
    _, _, src, T = pipeline.render_plan(meshes, H, W, prescaled=True, bbox=box, size=(HC, WC))
    return src, T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=4000)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--mode', default='NORMAL')
    ap.add_argument('--commit', default='unknown')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_multiband_warp.py measures on the GPU; there is none here')
    dev = torch.device('cuda:0')
    torch.set_grad_enabled(False)
    hr, _ = synth.make_clip_device(1, H, W, seed=0, views=2, device=dev)
    u8 = [hr[v].permute(0, 2, 3, 1).round().clamp(0, 255).to(torch.uint8).contiguous() for v in range(2)]
    f32 = [ops.ingest_u8(x)[0] for x in u8]
    src, T = splines(dev)
    gains = torch.tensor([[[0.91, 0.93, 0.95], [1.07, 1.05, 1.03]]], device=dev)
    mode = args.mode

    def two_step(imgs):
        return ops.tps_warp(ops.multiband_stack(imgs), src.view(2, 63, 2), T.view(2, 2, 66), HC, WC, mode, with_mask=True)

    units = [('two-step  fp32          ', lambda i: two_step(f32)),
             ("two-step' fp32          ", lambda i: two_step(f32)),
             ('two-step  uint8         ', lambda i: two_step(u8)),
             ('direct    fp32          ', lambda i: ops.multiband_warp(f32, src, T, HC, WC, mode)),
             ('direct    fp32  + gains ', lambda i: ops.multiband_warp(f32, src, T, HC, WC, mode, gains=gains)),
             ('direct    uint8         ', lambda i: ops.multiband_warp(u8, src, T, HC, WC, mode)),
             ('direct    uint8 + gains ', lambda i: ops.multiband_warp(u8, src, T, HC, WC, mode, gains=gains))]
    lines = ['MULTIBAND warp, one %dx%d frame pair on a %dx%d canvas, %s, synthetic texture; %d calls per window, %d rounds'
             % (H, W, HC, WC, mode, args.calls, args.rounds), 'GPU %s, commit %s' % (torch.cuda.get_device_name(0), args.commit)]
    want = two_step(f32).view(torch.int32)
    same = [torch.equal(fn(0).view(-1, 5, HC, WC).view(torch.int32), want) for _, fn in units]
    if [s for (n, _), s in zip(units, same) if 'gains' not in n] != [True] * 5 or any(s for (n, _), s in zip(units, same) if 'gains' in n):
        raise SystemExit('the planes differ where they must not (or the gains changed nothing): %s' % same)
    lines.append('planes without gains: bit-identical over all five units; with gains: differ, as they must')
    for _, fn in units:                          # warm-up: every shape of the timed windows
        for i in range(20):
            fn(i)
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in units}
    for _ in range(args.rounds):
        for name, fn in units:
            ms[name].append(window(fn, args.calls, 1) * 1e3)
    med = {}
    for name, _ in units:
        v = ms[name]
        med[name] = statistics.median(v)
        lines.append('  %s %8.1f us per call   spread %6.1f us over %d windows [%s]' % (name, med[name], max(v) - min(v), len(v),
                                                                                      ' '.join('%.1f' % x for x in v)))
    a, a2 = units[0][0], units[1][0]
    aa = max(abs(med[a] - med[a2]), max(ms[a]) - min(ms[a]), max(ms[a2]) - min(ms[a2]))
    lines.append('  A/A spread %.1f us' % aa)
    for name, _ in units[3:]:
        base = units[2][0] if 'uint8' in name else a
        d = med[name] - med[base]
        verdict = 'faster' if d < -aa else ('slower' if d > aa else 'within the A/A spread')
        lines.append('  %s - %s: %+8.1f us (x %.2f): %s' % (name.strip(), base.strip(), d, med[name] / med[base], verdict))
    print('\n'.join(lines), flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
