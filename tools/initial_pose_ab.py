#!/usr/bin/env python
"""A/B of the initial pose (pose/initialization.py estimate_translation over a batch of B frames), in ONE process:

  composed   : kernel='composed' on device tensors, one call over the batch -- the host functions as they stood before the fused
               path: per frame a nonzero, a boolean gather, two medians, a second gather and an .item()
  fused      : kernel='fused', check=True (the default: one ops.depth_init call and one copy of the counts to the host)
  fused_nochk: kernel='fused', check=False (nothing synchronises inside the call)
  depth_init : ops.depth_init alone on prepared tensors (the memset and the two launches plus the wrapper's allocations)

Frames of 240x320 and 480x640 with a disc mask over about a quarter of the frame, a smooth depth with noise and 2 % far
outliers.  Every repetition is a host clock around the call and a device synchronise (the composed path synchronises by
itself several times per frame, so device events would not bracket it).  After --warmup untimed calls per arm, --reps
repetitions per arm in alternating blocks of five; per arm the median, the extremes, the 10th / 90th percentiles and the
spread (max - min).  `fused_wins`: the fused median lies below the composed median by more than the larger of the two spreads.
The translations of the arms are compared bit for bit before anything is timed.

    python tools/initial_pose_ab.py [--frames 240x320,480x640] [--batches 1,8,64] [--json profiles/initial_pose_ab.json]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from latentfusion_amd import ops  # noqa: E402
from latentfusion_amd.pose import initialization as ini  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--frames', default='240x320,480x640')
ap.add_argument('--batches', default='1,8,64')
ap.add_argument('--reps', type=int, default=30)
ap.add_argument('--warmup', type=int, default=5)
ap.add_argument('--json', default=os.path.join(ROOT, 'profiles', 'initial_pose_ab.json'))
a = ap.parse_args()
if a.reps < 20:
    sys.exit('initial_pose_ab.py: at least 20 repetitions')
if not torch.cuda.is_available():
    sys.exit('initial_pose_ab.py measures on the GPU: no device found')
DEV = 'cuda'
BLOCK = 5


def frames(B, H, W, seed):
    """depth, mask (B,1,H,W) and intrinsics (B,3,3): a disc over a quarter of the frame, its centre jittered per frame."""
    g = torch.Generator().manual_seed(seed)
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing='ij')
    radius = math.sqrt(0.25 * H * W / math.pi)
    c = torch.rand(B, 2, generator=g) * 0.1 + 0.45
    mask = ((y - c[:, 0, None, None] * H) ** 2 + (x - c[:, 1, None, None] * W) ** 2 <= radius ** 2).float()
    depth = 0.9 + 0.1 * x / W + 0.05 * y / H + 0.004 * torch.rand(B, H, W, generator=g)
    depth = torch.where(torch.rand(B, H, W, generator=g) < 0.02, depth * 3.0, depth)
    K = torch.tensor([[572.4, 0.0, W / 2.0], [0.0, 573.6, H / 2.0], [0.0, 0.0, 1.0]]).expand(B, 3, 3).contiguous()
    return depth[:, None].contiguous(), mask[:, None].contiguous(), K


def once(fn):
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def summary(t):
    s = sorted(t)
    return {'median_ms': statistics.median(s), 'min_ms': s[0], 'max_ms': s[-1], 'p10_ms': s[len(s) // 10],
            'p90_ms': s[len(s) - 1 - len(s) // 10], 'spread_ms': s[-1] - s[0], 'reps': len(s)}


def ab(fns):
    for fn in fns.values():
        for _ in range(a.warmup):
            once(fn)
    times = {k: [] for k in fns}
    order = list(fns)
    for r in range((a.reps + BLOCK - 1) // BLOCK):
        for k in (order if r % 2 == 0 else order[::-1]):
            times[k] += [once(fns[k]) for _ in range(BLOCK)]
    return {k: summary(t) for k, t in times.items()}


def measure(H, W, B):
    depth, mask, K = (t.to(DEV) for t in frames(B, H, W, 100 * B + H))
    res = {'H': H, 'W': W, 'B': B, 'mask_share': float(mask.mean())}
    fns = {'composed': lambda: ini.estimate_translation(depth, mask, K, kernel='composed'),
           'fused': lambda: ini.estimate_translation(depth, mask, K, kernel='fused'),
           'fused_nochk': lambda: ini.estimate_translation(depth, mask, K, kernel='fused', check=False),
           'depth_init': lambda: ops.depth_init(depth, mask, K)}
    want, got = torch.stack(fns['composed'](), dim=-1), torch.stack(fns['fused'](), dim=-1)
    res['fused_equals_composed'] = bool(torch.equal(want, got))
    res.update(ab(fns))
    c, f = res['composed'], res['fused']
    res['composed_over_fused'] = c['median_ms'] / f['median_ms']
    res['fused_wins'] = bool(c['median_ms'] - f['median_ms'] > max(c['spread_ms'], f['spread_ms']))
    return res


results = {'device': torch.cuda.get_device_name(0), 'reps': a.reps, 'warmup': a.warmup, 'threads': torch.get_num_threads(),
           'command': f'python tools/initial_pose_ab.py --frames {a.frames} --batches {a.batches} --reps {a.reps}', 'shapes': []}
for frame in a.frames.split(','):
    H, W = (int(v) for v in frame.split('x'))
    for B in [int(v) for v in a.batches.split(',')]:
        results['shapes'].append(measure(H, W, B))
        print(json.dumps(results['shapes'][-1]), flush=True)
        if a.json:                                                 # (after every shape: a later one may not finish)
            os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
            with open(a.json, 'w') as f:
                json.dump(results, f, indent=1)
                f.write('\n')
