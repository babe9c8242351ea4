#!/usr/bin/env python
"""The fixed-size output of the covered rectangle at 720p two-view: ops.resample of the rectangle (39, 7, 704, 1980)
of 785 x 1995 frames -- the canvas and the rectangle of profiles/cover_720p.txt -- to 1080 x 1920, 720 x 1280 and 352 x 990, n = 1
and n = 32 frames, as fp32 planes, BGR bytes and NV12.
    python tools/bench_resample.py [--calls 300] [--clip-calls 10] [--rounds 5] [--commit ID] [--out FILE]
Each unit stands beside
  torch: the route a user has without this library -- slice, contiguous / permute / float, torch.nn.functional.interpolate(
         mode='bilinear', antialias=True), then for bytes + 0.5 / floor / clamp / uint8 / permute / contiguous, then for NV12
         ops.bgr_to_nv12.  interpolate takes no fractional window, so that route reads the 'fill' window rounded to whole pixels;
  copy:  one device copy of (the window's bytes + the output's bytes) / 2 -- it reads and writes that much, the traffic of reading
         the window once and writing the output once: the memory floor.
In one process; windows of calls interleaved over all units and repeated `rounds` times; per unit the median window and the spread
between its windows; one unit twice (A, A': the run-to-run spread).  Times are a host clock around a window of calls that ends in a
device synchronise, so they hold each path's launch overhead.  Before any timing every output of ops.resample is compared with
tests/resample_ref.py (frame 0 and the last frame; the n = 32 call against the n = 1 calls).
No threshold is fixed in advance.  profiles/resample_720p.txt holds the output."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch
import torch.nn.functional as F

import resample_ref as R
from bench_stream_feather import window
from stabstitch2_amd import ops

HC, WC, N = 785, 1995, 32
RECT = (39, 7, 704, 1980)
SIZES = [(1080, 1920), (720, 1280), (352, 990)]
FORMATS = ('f32', 'u8', 'nv12')


def torch_route(frames, size, fmt):
    """The same picture without the library, on the 'fill' window rounded to whole pixels."""
    fy, fx, fh, fw = ops.resample_window(RECT, (HC, WC), size)
    y0, x0, h, w = int(round(fy)), int(round(fx)), int(round(fh)), int(round(fw))
    if fmt == 'f32':
        return lambda i: F.interpolate(frames[:, :, y0:y0 + h, x0:x0 + w].contiguous(), size=size, mode='bilinear', antialias=True,
                                       align_corners=False)

    def bgr(i):
        x = frames[:, y0:y0 + h, x0:x0 + w, :].permute(0, 3, 1, 2).float()
        x = F.interpolate(x, size=size, mode='bilinear', antialias=True, align_corners=False)
        return x.add_(0.5).floor_().clamp_(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    if fmt == 'u8':
        return bgr
    return lambda i: ops.bgr_to_nv12(bgr(i))


def check(f32, u8, dev):
    """Every output of ops.resample against the reference, on frame 0 and the last frame; -> lines for the report."""
    lines = []
    for size in SIZES:
        ky, kx = R.tap_counts(RECT, HC, WC, size[0], size[1], 'fill')
        bound = R.bound(ky, kx)
        for k in (0, N - 1):
            ref = R.resample(f32[k].cpu().numpy().astype(np.float64), size, RECT, 'fill')
            got = ops.resample(f32[k], size, rect=RECT).cpu().numpy()
            err = float(np.abs(got - ref).max())
            want8 = R.to_bytes(np.moveaxis(R.resample(np.moveaxis(u8[k].cpu().numpy(), -1, 0), size, RECT, 'fill'), 0, -1))
            got8 = ops.resample(u8[k], size, rect=RECT)
            differ = float((got8.cpu().numpy() != want8).mean())
            if err > bound or differ > 0.02 or np.abs(got8.cpu().numpy().astype(int) - want8).max() > 1:
                raise SystemExit('ops.resample is wrong at %s frame %d: fp32 err %.3e (bound %.3e), bytes differing %.5f' % (size, k, err, bound, differ))
            if not torch.equal(ops.resample(u8[k], size, rect=RECT, out_format='nv12'), ops.bgr_to_nv12(got8)):
                raise SystemExit('the NV12 output differs from bgr_to_nv12 of the BGR output at %s' % (size,))
            lines.append('  checked %4d x %4d frame %2d: fp32 max|err| %.2e (bound %.2e, %d x %d taps), bytes differing from the reference %.4f %%, '
                         'NV12 == bgr_to_nv12' % (size + (k, err, bound, ky, kx, 100 * differ)))
        rd = torch.tensor(RECT, dtype=torch.int32, device=dev)
        all32 = ops.resample(f32, size, rect=rd)
        all8 = ops.resample(u8, size, rect=rd)
        for k in (0, N - 1):
            if not torch.equal(all32[k], ops.resample(f32[k], size, rect=RECT)) or not torch.equal(all8[k], ops.resample(u8[k], size, rect=RECT)):
                raise SystemExit('the n = %d call differs from the single frames at %s' % (N, size))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=300)
    ap.add_argument('--clip-calls', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--commit', default='unknown')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_resample.py measures on the GPU; there is none here')
    dev = torch.device('cuda:0')
    torch.set_grad_enabled(False)
    g = torch.Generator(device=dev).manual_seed(0)
    u8 = torch.randint(0, 256, (N, HC, WC, 3), generator=g, device=dev, dtype=torch.uint8)
    f32 = u8.permute(0, 3, 1, 2).float().contiguous()
    rd = torch.tensor(RECT, dtype=torch.int32, device=dev)
    lines = ['ops.resample of the rectangle %s of %d x %d frames (aspect fill, rectangle on the device); %d (n=32: %d) calls per window, %d rounds'
             % (RECT, HC, WC, args.calls, args.clip_calls, args.rounds),
             'GPU %s, commit %s' % (torch.cuda.get_device_name(0), args.commit)]
    lines += check(f32, u8, dev)

    units = []
    for n in (1, N):
        for size in SIZES:
            fy, fx, fh, fw = ops.resample_window(RECT, (HC, WC), size)
            for fmt in FORMATS:
                src = (f32 if fmt == 'f32' else u8)[:n]
                px_out = size[0] * size[1]
                out_bytes = n * px_out * (12 if fmt == 'f32' else 3 if fmt == 'u8' else 1.5)
                win_bytes = n * fh * fw * (12 if fmt == 'f32' else 3)
                half = int((out_bytes + win_bytes) / 2)
                a, b = torch.empty(half, device=dev, dtype=torch.uint8), torch.empty(half, device=dev, dtype=torch.uint8)
                shape = (n, 3) + size if fmt == 'f32' else (n,) + size + (3,) if fmt == 'u8' else (n, size[0] // 2 * 3, size[1])
                out = torch.empty(shape, device=dev, dtype=src.dtype)
                new = (lambda src, size, out, fmt: lambda i: ops.resample(src, size, rect=rd, out=out,
                                                                         out_format='nv12' if fmt == 'nv12' else 'bgr'))(src, size, out, fmt)
                name = 'n=%-2d %4dx%-4d %-4s' % (n, size[0], size[1], fmt)
                calls = args.calls if n == 1 else args.clip_calls
                units.append((name + ' new  ', new, calls))
                units.append((name + ' torch', torch_route(src, size, fmt), calls))
                units.append((name + ' copy ', (lambda a, b: lambda i: b.copy_(a))(a, b), calls))
    aa_name = 'n=32 1080x1920 f32  new  '
    aa = [u for u in units if u[0] == aa_name][0]
    units.append((aa_name.rstrip() + "'", aa[1], aa[2]))
    for _, fn, _ in units:                       # warm-up: every shape of the timed windows
        for i in range(3):
            fn(i)
    torch.cuda.synchronize()
    us = {name: [] for name, _, _ in units}
    for _ in range(args.rounds):
        for name, fn, calls in units:
            us[name].append(window(fn, calls, 1) * 1e3)
    med = {name: statistics.median(v) for name, v in us.items()}
    spread = max(abs(med[aa_name] - med[aa_name.rstrip() + "'"]), max(us[aa_name]) - min(us[aa_name]))
    lines.append("  A/A spread (%s and its twin, medians %.1f and %.1f us): %.1f us = %.2f %%"
                 % (aa_name.strip(), med[aa_name], med[aa_name.rstrip() + "'"], spread, 100 * spread / med[aa_name]))
    lines.append('  %-24s %10s %10s %8s %10s %8s   windows of new [us]' % ('unit', 'new us', 'torch us', 'torch/new', 'copy us', 'new/copy'))
    slower = []
    for k in range(0, len(units) - 1, 3):
        base = units[k][0][:-6]
        new, tor, cop = (med[units[k + j][0]] for j in range(3))
        lines.append('  %-24s %10.1f %10.1f %8.2f %10.1f %8.2f   [%s]' % (base, new, tor, tor / new, cop, new / cop,
                                                                        ' '.join('%.1f' % x for x in us[units[k][0]])))
        if not new * (1 + spread / med[aa_name]) < tor:
            slower.append(base.strip())
    lines.append('  units where the new call is NOT faster than the torch route by more than the A/A spread: %s' % (', '.join(slower) or 'none'))
    print('\n'.join(lines), flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
