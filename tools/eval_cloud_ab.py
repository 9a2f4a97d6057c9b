#!/usr/bin/env python
"""A/B of the evaluation point cloud (Observation.pointcloud, three.utils.farthest_points, pointcloud.eval_points), in ONE
process, composed on device tensors against fused:

  pointcloud       obs.pointcloud(segment=True) of 16 views of 480x640 (the synthetic observation: a disc mask of radius
                   150 px, its depth made positive everywhere)
  farthest_points  (N, K) = (2000, 32), (8000, 4096) and (80000, 4096) on randn clouds; the last is beyond the resident form, so
                   the fused arm runs streamed
  eval_points      pointcloud.eval_points of a 4-view observation down to 4096 points, end to end
  fps_forms        ops.farthest_points at (8000, 4096) in the resident and in the streamed form (both fused: which form to
                   prefer where both apply)

The composed arm is the host loop as it stands: per pick an argmax with its .item(), a pairwise_distance, a minimum and a masked
write.  Every repetition is a host clock around the call and a device synchronise (the composed path synchronises by itself,
so device events would not bracket it).  After --warmup untimed calls per arm, --reps repetitions per arm in alternating blocks
of five; per arm the median, the extremes, the 10th / 90th percentiles and the spread (max - min).  `fused_wins`: the fused
median lies below the composed median by more than the larger of the two spreads.  No ratio is promised.

    python tools/eval_cloud_ab.py [--reps 30] [--json profiles/eval_cloud_ab.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from latentfusion_amd import ops, pointcloud, synth  # noqa: E402
from latentfusion_amd.three.utils import farthest_points  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=30)
ap.add_argument('--warmup', type=int, default=5)
ap.add_argument('--only', default='', help='comma-separated subset of: pointcloud, farthest_points, eval_points, fps_forms')
ap.add_argument('--json', default=os.path.join(ROOT, 'profiles', 'eval_cloud_ab.json'))
a = ap.parse_args()
if a.reps < 20:
    sys.exit('eval_cloud_ab.py: at least 20 repetitions')
if not torch.cuda.is_available():
    sys.exit('eval_cloud_ab.py measures on the GPU: no device found')
DEV = 'cuda'
BLOCK = 5
ONLY = set(filter(None, a.only.split(',')))


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


def verdict(res, base='composed', new='fused'):
    c, f = res[base], res[new]
    res[f'{base}_over_{new}'] = c['median_ms'] / f['median_ms']
    res[f'{new}_wins'] = bool(c['median_ms'] - f['median_ms'] > max(c['spread_ms'], f['spread_ms']))
    return res


def cloud(n, seed):
    return torch.randn(n, 3, generator=torch.Generator().manual_seed(seed)).clamp(-4, 4).to(DEV)


def observation(views):
    """The synthetic observation with its depth (0 outside the disc) made positive everywhere: the two arms then keep the same
    pixels (the composed path keeps some zero-depth pixels by accident, the kernel none)."""
    obs = synth.make_observation(views, 0)
    obs.depth = torch.where(obs.depth == 0, torch.full_like(obs.depth, 1.05), obs.depth)
    return obs.to(DEV)


def measure_pointcloud():
    obs = observation(16)
    want, got = obs.pointcloud(kernel='composed'), obs.pointcloud(kernel='fused')
    res = {'what': 'pointcloud', 'views': 16, 'H': 480, 'W': 640, 'points': int(want.shape[0]),
           'same_point_count': want.shape == got.shape,
           'max_abs_diff': float((want - got).abs().max()) if want.shape == got.shape else None}
    res.update(ab({'composed': lambda: obs.pointcloud(kernel='composed'), 'fused': lambda: obs.pointcloud(kernel='fused')}))
    return verdict(res)


def measure_fps(n, k):
    x = cloud(n, n + k)
    fns = {kern: (lambda kern=kern: farthest_points(x, k, F.pairwise_distance, return_center_indexes=True, kernel=kern))
           for kern in ('composed', 'fused')}
    want, got = fns['composed'](), fns['fused']()
    res = {'what': 'farthest_points', 'N': n, 'K': k, 'fused_form': 'resident' if n <= ops._lib.LF_FPS_RESIDENT_MAX else 'streamed',
           'same_picks': bool(torch.equal(want[1], got[1]))}
    res.update(ab(fns))
    return verdict(res)


def measure_eval_points():
    obs = observation(4)
    fns = {kern: (lambda kern=kern: pointcloud.eval_points(obs, 4096, kernel=kern)) for kern in ('composed', 'fused')}
    res = {'what': 'eval_points', 'views': 4, 'H': 480, 'W': 640, 'n_points': 4096, 'cloud': int(obs.pointcloud().shape[0])}
    res.update(ab(fns))
    return verdict(res)


def measure_forms(n, k):
    x = cloud(n, n + k)
    fns = {form: (lambda form=form: ops.farthest_points(x, k, want=('centers', 'owner'), form=form)) for form in ('streamed', 'resident')}
    res = {'what': 'fps_forms', 'N': n, 'K': k,
           'same_bits': all(bool(torch.equal(u, v)) for u, v in zip(fns['streamed']().values(), fns['resident']().values()))}
    res.update(ab(fns))
    return verdict(res, base='streamed', new='resident')


JOBS = [('pointcloud', measure_pointcloud), ('farthest_points', lambda: measure_fps(2000, 32)),
        ('farthest_points', lambda: measure_fps(8000, 4096)), ('farthest_points', lambda: measure_fps(80000, 4096)),
        ('eval_points', measure_eval_points), ('fps_forms', lambda: measure_forms(8000, 4096))]
results = {'device': torch.cuda.get_device_name(0), 'reps': a.reps, 'warmup': a.warmup, 'threads': torch.get_num_threads(),
           'command': f'python tools/eval_cloud_ab.py --reps {a.reps}' + (f' --only {a.only}' if a.only else ''), 'rows': []}
for what, job in JOBS:
    if ONLY and what not in ONLY:
        continue
    results['rows'].append(job())
    print(json.dumps(results['rows'][-1]), flush=True)
    if a.json:                                                     # (after every row: a later one may not finish)
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            json.dump(results, f, indent=1)
            f.write('\n')
