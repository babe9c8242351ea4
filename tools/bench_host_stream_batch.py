"""NV12 at batch rates, 720p two-view, every arm in ONE process and interleaved round by round:
  1. the converter alone (ops.nv12_to_bgr, 16 surfaces = k 8 x two views) against its byte count at the rate ops.canvas_to_u8 reaches here
  2. push_many_u8 against push_many_nv12 at k = 8 and 16 (device tensors in, frames on the device out), with an A/A pair
  3. HostFrameStream, host to host: batch 1 / 4 / 8 / 16 x (BGR in + out, NV12 in + out), with an A/A pair of batch 1 BGR
  4. batch 1: push_nv12 (the native route) against ops.nv12_to_bgr + push_u8 (HostFrameStream's route)
    python tools/bench_host_stream_batch.py [--frames 320] [--rounds 3] [--out FILE]
Times are host clocks around work that ends in a device synchronise; the converter is timed with device events."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from stabstitch2_amd import ops, synth  # noqa: E402
from stabstitch2_amd.online import HostFrameStream, OnlineStitcher  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--frames', type=int, default=320, help='frames per arm and round (a multiple of 16)')
ap.add_argument('--rounds', type=int, default=3)
ap.add_argument('--height', type=int, default=720)
ap.add_argument('--width', type=int, default=1280)
ap.add_argument('--out', default=None, help='also write the report to this file')
args = ap.parse_args()
assert torch.cuda.is_available(), 'a measurement needs the GPU: there is no fallback'
assert args.frames % 16 == 0
dev = torch.device('cuda:0')
torch.set_grad_enabled(False)
H, W, N = args.height, args.width, 32
VIEWPORT = (H + 96, W + 448)                 # even: NV12 out needs a fixed even frame size
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


nets, _ = bench.build_nets(dev)
hr, _ = synth.make_clip_device(N, H, W, seed=0, views=2, device=dev)
bgr = [hr[v].clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous() for v in range(2)]      # [N,H,W,3] per view
nv = [ops.bgr_to_nv12(b) for b in bgr]                                                               # [N,H*3/2,W] per view
bgr = [ops.nv12_to_bgr(x) for x in nv]           # the BGR arms see the very frames the NV12 arms convert to
host_bgr = [[b[t].cpu().pin_memory() for t in range(N)] for b in bgr]
host_nv = [[x[t].cpu().pin_memory() for t in range(N)] for x in nv]
del hr
mk = lambda: OnlineStitcher(nets, H, W, viewport=VIEWPORT)      # noqa: E731


def sync_time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = fn()
    torch.cuda.synchronize()
    return n, time.perf_counter() - t0


# ------------------------------------------------------------------ 1. the converter alone
def event_ms(fn, reps=200):
    for _ in range(20):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


surf = list(nv[0][:8].unbind(0)) + list(nv[1][:8].unbind(0))
out16 = torch.empty((16, H, W, 3), dtype=torch.uint8, device=dev)
canvas = torch.rand((16, 3, H, W), device=dev) * 255
# the launch alone: the entry point called with host arrays made once (ops.nv12_to_bgr checks 16 tensors and builds them per call;
# back-to-back launches cannot be timed faster than the host enqueues them)
import ctypes  # noqa: E402

from stabstitch2_amd import _surfaces  # noqa: E402
_ys = (ctypes.c_void_p * 16)(*[f.data_ptr() for f in surf])
_uvs = (ctypes.c_void_p * 16)(*[f.data_ptr() + H * f.stride(0) for f in surf])
_ps = (ctypes.c_int * 16)(*[f.stride(0) for f in surf])
_fn, _st = _surfaces.lib().ssf_nv12_to_bgr, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def launch_alone():
    assert _fn(_ys, _uvs, _ps, 16, H, W, out16.data_ptr(), 3 * H * W, _st) == 0


conv, kern, c2u, fill = [], [], [], []
for _ in range(args.rounds):
    conv.append(event_ms(lambda: ops.nv12_to_bgr(surf, out=out16)))
    kern.append(event_ms(launch_alone))
    c2u.append(event_ms(lambda: ops.canvas_to_u8(canvas, out=out16)))
    fill.append(event_ms(lambda: out16.fill_(7)))        # the same 3 B/px written in whole lines, nothing read
px = 16 * H * W
t_conv, t_c2u, t_fill = statistics.median(conv), statistics.median(c2u), statistics.median(fill)
rate = 15.0 * px / (t_c2u * 1e-3)                # canvas_to_u8: 12 B/px in, 3 B/px out
bound = 4.5 * px / rate * 1e3
t_kern = statistics.median(kern)
say('1. converter, 16 surfaces %dx%d: %.4f ms per ops.nv12_to_bgr call (rounds %s)' % (H, W, t_conv, [round(x, 4) for x in conv]))
say('   the launch alone (host arrays made once): %.4f ms (rounds %s), %.0f GB/s of its 4.5 B/px'
    % (t_kern, [round(x, 4) for x in kern], 4.5 * px / t_kern / 1e6))
say('   canvas_to_u8 on 16 frames: %.4f ms, %.0f GB/s of its 15 B/px -> byte-bound time of the converter %.4f ms, ratio %.2f (launch alone)'
    % (t_c2u, rate / 1e9, bound, t_kern / bound))
say('   a fill of the same output (3 B/px written, nothing read): %.4f ms, %.0f GB/s' % (t_fill, 3.0 * px / t_fill / 1e6))
del canvas, out16


# ------------------------------------------------------------------ 2. / 4. device arms
def many_arm(kind, k):
    st = mk()
    def run(frames):
        n = 0
        for a in range(0, frames, k):
            t = a % N
            if kind == 'u8':
                n += len(st.push_many_u8(bgr[0][t:t + k], bgr[1][t:t + k]))
            else:
                n += len(st.push_many_nv12(nv[0][t:t + k], nv[1][t:t + k]))
        return n
    return run


def single_arm(kind):
    st = mk()
    def run(frames):
        n = 0
        for a in range(frames):
            t = a % N
            if kind == 'native':
                n += len(st.push_nv12(nv[0][t], nv[1][t]))
            else:
                b = ops.nv12_to_bgr([nv[0][t], nv[1][t]])
                n += len(st.push_u8(b[0], b[1]))
        return n
    return run


def host_arm(batch, fmt):
    runner = HostFrameStream(mk(), batch=batch, frame_format=fmt, out=fmt)
    src = host_nv if fmt == 'nv12' else host_bgr
    def run(frames):
        return sum(1 for _ in runner.run((src[0][t % N], src[1][t % N]) for t in range(frames)))
    return run


arms = {}
for k in (8, 16):
    arms['push_many_u8 k=%d' % k] = many_arm('u8', k)
    arms['push_many_u8 k=%d (A/A)' % k] = many_arm('u8', k)
    arms['push_many_nv12 k=%d' % k] = many_arm('nv12', k)
arms['push_nv12 native'] = single_arm('native')
arms['nv12_to_bgr + push_u8'] = single_arm('convert')
for batch in (1, 4, 8, 16):
    for fmt in ('bgr', 'nv12'):
        arms['HostFrameStream batch=%d %s' % (batch, fmt)] = host_arm(batch, fmt)
arms['HostFrameStream batch=1 bgr (A/A)'] = host_arm(1, 'bgr')

for name, run in arms.items():                   # the window fill, the graph captures, every shape of the timed window
    run(64)
torch.cuda.synchronize()
fps = {name: [] for name in arms}
for r in range(args.rounds):
    for name, run in arms.items():
        n, dt = sync_time(lambda: run(args.frames))
        fps[name].append(n / dt)
hc, wc = VIEWPORT
pcie = {'bgr': 2 * 3 * H * W + 3 * hc * wc, 'nv12': 2 * 3 * H * W // 2 + 3 * hc * wc // 2}
say('2-4. frames/s, median of %d interleaved rounds of %d frames (every round in brackets); canvas %dx%d' % (args.rounds, args.frames, hc, wc))
for name, v in fps.items():
    extra = ''
    if name.startswith('HostFrameStream'):
        extra = '   %.2f MB over PCIe per frame' % (pcie['nv12' if 'nv12' in name else 'bgr'] / 1e6)
    say('   %-36s %8.1f   [%s]%s' % (name, statistics.median(v), ', '.join('%.1f' % x for x in v), extra))
say(json.dumps({'converter_call_ms': t_conv, 'converter_launch_ms': t_kern, 'converter_bound_ms': bound, 'fps': {k: statistics.median(v) for k, v in fps.items()}}))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
