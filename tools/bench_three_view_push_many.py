#!/usr/bin/env python
"""ThreeViewOnlineStitcher.push_many against push on ONE stream of frame triples at 720x1280: steady stitched frames/s per batch
size k, one JSON line.
    python tools/bench_three_view_push_many.py [--frames 256] [--only many8]
Same rules as tools/bench_push_many.py: bench.py's synthetic clip (32 frames, cycled; views=3) and weights, the default kernel
policy, AVERAGE with the direct render unless named.  Per configuration a fresh stitcher: the window fill (7 pushes), the capture
and 3 warm batches, then >= `frames` stitched frames timed on the host clock up to a synchronise.  `push` (batch 1) runs in the same
process as the baseline.  --only runs one configuration (e.g. under rocprofv3 --kernel-trace --stats)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench
from stabstitch2_amd import synth
from stabstitch2_amd.online import ThreeViewOnlineStitcher, WINDOW

CLIP = 32
# name -> (k, fusion, uint8, deterministic); k = 0: `push`, one triple per call
CONFIGS = {'push': (0, 'AVERAGE', False, False),
           'many1': (1, 'AVERAGE', False, False), 'many2': (2, 'AVERAGE', False, False), 'many4': (4, 'AVERAGE', False, False),
           'many8': (8, 'AVERAGE', False, False), 'many16': (16, 'AVERAGE', False, False),
           'many8_linear': (8, 'LINEAR', False, False), 'many8_u8': (8, 'AVERAGE', True, False),
           'many8_deterministic': (8, 'AVERAGE', False, True)}


def run(nets, clip, h, w, k, fusion, u8, deterministic, frames):
    """-> (stitched frames/s, graph nodes per call)."""
    hr, lr, img = clip
    st = ThreeViewOnlineStitcher(nets, h, w, fusion_mode=fusion, deterministic=deterministic)
    one = lambda t: [hr[v, t:t + 1] for v in range(3)] + [lr[v, t:t + 1] for v in range(3)]
    for t in range(WINDOW):                                      # window fill, one triple at a time
        if u8:
            st.push_u8(img[0][t], img[1][t], img[2][t])
        else:
            st.push(*one(t))
    if k == 0:
        calls = [(lambda t=t: st.push(*one(t))) for t in range(CLIP)]
        per = 1
    else:
        starts = range(0, CLIP - k + 1, k)
        if u8:
            calls = [(lambda s=s: st.push_many_u8(*[img[v][s:s + k] for v in range(3)])) for s in starts]
        else:
            calls = [(lambda s=s: st.push_many(*([hr[v, s:s + k] for v in range(3)] + [lr[v, s:s + k] for v in range(3)])))
                     for s in starts]
        per = k
    for i in range(4):                                           # the capture + 3 warm calls
        calls[i % len(calls)]()
    torch.cuda.synchronize()
    n = -(-frames // per)
    t0 = time.perf_counter()
    got = 0
    for i in range(n):
        got += len(calls[i % len(calls)]())
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert got == n * per, (got, n, per)
    nodes = st.graph_nodes if k == 0 else st.graph_nodes_batch.get(k)
    return got / dt, nodes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=256)
    ap.add_argument('--height', type=int, default=720)
    ap.add_argument('--width', type=int, default=1280)
    ap.add_argument('--only', choices=sorted(CONFIGS), default=None)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.set_grad_enabled(False)
    nets, _ = bench.build_nets(dev)
    hr, lr = synth.make_clip_device(CLIP, args.height, args.width, seed=0, views=3, device=dev)
    img = [hr[v].permute(0, 2, 3, 1).round().clamp(0, 255).to(torch.uint8).contiguous() for v in range(3)]
    names = [args.only] if args.only else list(CONFIGS)
    fps, nodes = {}, {}
    for name in names:
        k, fusion, u8, det = CONFIGS[name]
        f, g = run(nets, (hr, lr, img), args.height, args.width, k, fusion, u8, det, args.frames)
        fps[name] = round(f, 1)
        nodes[name] = g
    res = {'metric': 'three_view_push_many_stitched_fps', 'height': args.height, 'width': args.width, 'frames_timed': args.frames,
           'fps': fps, 'graph_nodes_per_call': nodes}
    if 'push' in fps and 'many8' in fps:
        res['many8_over_push'] = round(fps['many8'] / fps['push'], 3)
    if 'many8' in fps and 'many16' in fps:
        res['many16_over_many8'] = round(fps['many16'] / fps['many8'], 3)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
