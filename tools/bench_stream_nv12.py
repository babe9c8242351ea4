#!/usr/bin/env python
"""Streaming from decoder surfaces to encoder surfaces: what NV12 in and out costs per steady-state push, against packed BGR.
    python tools/bench_stream_nv12.py [--pushes 300] [--rounds 3] [--height 720 --width 1280] [--commit ID] [--out FILE]
Per fusion mode (AVERAGE, LINEAR), OnlineStitcher on one box with one even viewport, in one process:
  (a)  push_u8 on pre-converted BGR frames, twice (A, A': the run-to-run spread) -- the floor that excludes every conversion;
  (b)  push_nv12(out='bgr'): the resize and the render's taps convert the bytes they read;
  (c)  push_nv12(out='nv12'): the same, and the video frame leaves as NV12 (AVERAGE: written by the render; LINEAR: by the sink);
  (c') AVERAGE only: (c) with online.NV12_FUSED_SINK off -- the render writes BGR, ops.bgr_to_nv12 follows;
  (d') push_u8 + ops.bgr_to_nv12 on pre-converted frames: the three-step chain WITHOUT its first step, a lower bound of every
       chain whatever converter it uses;
  (d)  the chain a user would otherwise run: NV12 -> BGR of both frames, push_u8, ops.bgr_to_nv12.  The library has no NV12 -> BGR
       pass of its own (that is the point); the converter here is the integer statement in torch ops (checked once against
       ops.ingest_nv12), a dozen elementwise launches per frame -- what a PyTorch user writes without a kernel of their own.
Windows of `pushes` pushes, interleaved over the units and repeated `rounds` times; per unit the median window and the spread between
its windows -- a difference below the A/A spread is not a difference.  profiles/stream_nv12_720p.txt holds the output."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault('GPU_MAX_HW_QUEUES', '16')
import torch

import bench
from stabstitch2_amd import online, ops, synth

N = 16                                   # frames of the synthetic clip; the pushes cycle through it


def nv12_to_bgr_torch(f, h):
    """The NV12 -> BGR statement ("Frame formats") in torch ops: NV12 uint8 [h*3/2,w] -> uint8 [h,w,3]."""
    w = f.shape[1]
    c = (f[:h].to(torch.int32) - 16).clamp_(min=0) * 1220542 + (1 << 19)
    uv = f[h:].view(h // 2, w // 2, 2).to(torch.int32) - 128
    uv = uv.repeat_interleave(2, 0).repeat_interleave(2, 1)
    u, v = uv[..., 0], uv[..., 1]
    planes = ((c + 2116026 * u) >> 20, (c - 409993 * u - 852492 * v) >> 20, (c + 1673527 * v) >> 20)
    return torch.stack(planes, -1).clamp_(0, 255).to(torch.uint8)


def window(push, pushes):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(pushes):
        push(t % N)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / pushes * 1e3


def run(fusion, nets, nv, bgr, h, w, args, lines):
    first = len(lines)
    probe = online.OnlineStitcher(nets, h, w, fusion_mode=fusion)
    for t in range(8):
        probe.push_u8(bgr[0][t], bgr[1][t])
    box = probe.canvas_box
    vp = (probe.hc // 2 * 2, probe.wc // 2 * 2)
    del probe
    mk = lambda: online.OnlineStitcher(nets, h, w, fusion_mode=fusion, canvas=box, viewport=vp)

    def unit(kind):
        st = mk()
        if kind == 'u8':
            return st, lambda i: st.push_u8(bgr[0][i], bgr[1][i])
        if kind == 'u8+sink':
            return st, lambda i: [ops.bgr_to_nv12(f) for f in st.push_u8(bgr[0][i], bgr[1][i])]
        if kind == 'chain':
            return st, lambda i: [ops.bgr_to_nv12(f) for f in st.push_u8(nv12_to_bgr_torch(nv[0][i], h), nv12_to_bgr_torch(nv[1][i], h))]
        if kind == 'nv12-unfused':
            def push(i):
                online.NV12_FUSED_SINK = False
                try:
                    return st.push_nv12(nv[0][i], nv[1][i], out='nv12')
                finally:
                    online.NV12_FUSED_SINK = True
            return st, push
        fmt = kind.split(':')[1]
        return st, lambda i: st.push_nv12(nv[0][i], nv[1][i], out=fmt)

    kinds = [('(a)  push_u8 A            ', 'u8'), ('(a)  push_u8 A\'           ', 'u8'), ('(b)  push_nv12 -> bgr     ', 'nv12:bgr'),
             ('(c)  push_nv12 -> nv12    ', 'nv12:nv12')]
    if fusion == 'AVERAGE':
        kinds.append(('(c\') push_nv12, sink apart', 'nv12-unfused'))
    kinds += [('(d\') push_u8 + sink       ', 'u8+sink'), ('(d)  convert, push_u8, sink', 'chain')]
    units = []
    for name, kind in kinds:
        st, push = unit(kind)
        for t in range(12):                  # the window fill, the capture, a few replays
            push(t)
        units.append((name, st, push))
    torch.cuda.synchronize()
    ms = {name: [] for name, _, _ in units}
    for _ in range(args.rounds):
        for name, _, push in units:
            ms[name].append(window(push, args.pushes))
    lines.append('%s: box %s, viewport %dx%d' % (fusion, ' '.join('%.2f' % v for v in box), vp[0], vp[1]))
    med = {}
    for name, st, _ in units:
        v = ms[name]
        med[name] = statistics.median(v)
        lines.append('  %s %.4f ms per push  %8.1f frames/s   spread %.4f ms over %d windows of %d pushes [%s]   graph nodes %s'
                     % (name, med[name], 1e3 / med[name], max(v) - min(v), len(v), args.pushes, ' '.join('%.4f' % x for x in v),
                        st.graph_nodes))
    names = [n for n, _, _ in units]
    aa = max(abs(med[names[0]] - med[names[1]]), max(max(ms[n]) - min(ms[n]) for n in names[:2]))
    a = min(med[names[0]], med[names[1]])
    b, c = med[names[2]], med[names[3]]
    dl, d = med[names[-2]], med[names[-1]]
    verdict = lambda x: 'inside the A/A spread' if abs(x) <= aa else 'OUTSIDE the A/A spread'
    lines.append('  A/A spread %.4f ms' % aa)
    lines.append('  (b) - (a)  = %+.4f ms (%+.2f %%): the price of the fused taps -> %s' % (b - a, 100.0 * (b - a) / a, verdict(b - a)))
    lines.append('  (c) - (d\') = %+.4f ms (%+.2f %%): against the chain without its converter -> %s' % (c - dl, 100.0 * (c - dl) / dl, verdict(c - dl)))
    lines.append('  (c) - (d)  = %+.4f ms (%+.2f %%): against the chain with the torch-op converter -> %s' % (c - d, 100.0 * (c - d) / d, verdict(c - d)))
    if fusion == 'AVERAGE':
        cu = med[names[4]]
        lines.append('  (c) - (c\') = %+.4f ms (%+.2f %%): the render writing NV12 itself against render + sink -> %s'
                     % (c - cu, 100.0 * (c - cu) / cu, verdict(c - cu)))
    print('\n'.join(lines[first:]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pushes', type=int, default=300)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--height', type=int, default=720)
    ap.add_argument('--width', type=int, default=1280)
    ap.add_argument('--commit', default='unknown')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.set_grad_enabled(False)
    nets, _ = bench.build_nets(dev)
    h, w = args.height, args.width
    hr, _ = synth.make_clip_device(N, h, w, seed=0, views=2, device=dev)
    u8 = hr.permute(0, 1, 3, 4, 2).round().clamp(0, 255).to(torch.uint8).contiguous()
    nv = [ops.bgr_to_nv12(u8[v]) for v in range(2)]                              # what a decoder would deliver
    bgr = [torch.stack([nv12_to_bgr_torch(nv[v][i], h) for i in range(N)], 0) for v in range(2)]
    planes, _ = ops.ingest_nv12(nv[0][:2], 8, 8)                                  # the torch converter is the library's statement
    assert torch.equal(planes.permute(0, 2, 3, 1).to(torch.uint8), bgr[0][:2])
    lines = ['streaming NV12 in / out, OnlineStitcher steady state, %dx%d, synthetic nets and texture; %d pushes per window, %d rounds'
             % (h, w, args.pushes, args.rounds),
             'GPU %s, commit %s' % (torch.cuda.get_device_name(0), args.commit)]
    print('\n'.join(lines), flush=True)
    for fusion in ('AVERAGE', 'LINEAR'):
        run(fusion, nets, nv, bgr, h, w, args, lines)
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
