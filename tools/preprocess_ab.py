#!/usr/bin/env python
"""A/B of the observation preprocessing (LatentFusionModel.preprocess_observation = Observation.zoom -> prepare -> normalize on a
device observation of V frames of 480x640), in ONE process:

  composed : preprocess_kernel='composed': per map a boxes.cpu(), per frame and map two linspace + scale / shift / stack, one
             lf_grid_sample2d_fwd per map, then the element-wise chains of prepare / normalize
  fused    : preprocess_kernel='fused': the boxes stay on the device and ONE lf_obs_prepare launch writes the three maps

and of build_latent_object on SYN(128,16) with 16 views both ways (fused: the kernel also writes the encoder's stacked input).
V in {1, 16, 128} x T in {128, 256}; for T = 256 the SYN(128,16) model's input size and camera distance are overridden for the
preprocessing call only (it reads nothing else of the model).  Every repetition is a host clock around the call and a device
synchronise (the composed path synchronises by itself three times, so device events would not bracket it).  After --warmup
untimed calls per arm, --reps repetitions per arm in alternating blocks of five; per arm the median, the extremes, the 10th /
90th percentiles and the spread (max - min).  `fused_wins`: the fused median lies below the composed median by more than the
larger of the two spreads.  Before anything is timed the nearest maps of the two arms are compared bit for bit and the colour's
largest difference is recorded (the two crop lattices differ in their last bits: include/lf_hip.h).

    python tools/preprocess_ab.py [--views 1,16,128] [--sizes 128,256] [--json profiles/observation_prepare_ab.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from latentfusion_amd import consts, synth  # noqa: E402
from latentfusion_amd.recon.utils import optimal_camera_dist  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--views', default='1,16,128')
ap.add_argument('--sizes', default='128,256')
ap.add_argument('--reps', type=int, default=30)
ap.add_argument('--warmup', type=int, default=5)
ap.add_argument('--json', default=os.path.join(ROOT, 'profiles', 'observation_prepare_ab.json'))
a = ap.parse_args()
if a.reps < 20:
    sys.exit('preprocess_ab.py: at least 20 repetitions')
if not torch.cuda.is_available():
    sys.exit('preprocess_ab.py measures on the GPU: no device found')
DEV = 'cuda'
BLOCK = 5
S, C = 128, 16


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


def arm(model, kernel, fn):
    def run():
        model.preprocess_kernel = kernel
        try:
            return fn()
        finally:
            model.preprocess_kernel = 'composed'
    return run


def verdict(res):
    c, f = res['composed'], res['fused']
    res['composed_over_fused'] = c['median_ms'] / f['median_ms']
    res['fused_wins'] = bool(c['median_ms'] - f['median_ms'] > max(c['spread_ms'], f['spread_ms']))
    return res


def save(results):
    if a.json:                                                     # (after every shape: a later one may not finish)
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            json.dump(results, f, indent=1)
            f.write('\n')


model, _ = synth.build_model(S, C, 'gru', seed=0, device=DEV)
results = {'device': torch.cuda.get_device_name(0), 'reps': a.reps, 'warmup': a.warmup, 'threads': torch.get_num_threads(),
           'command': f'python tools/preprocess_ab.py --views {a.views} --sizes {a.sizes} --reps {a.reps}', 'frame': '480x640',
           'preprocess_observation': [], 'build_latent_object': []}
own = (model.input_size, model.camera_dist)
for V in [int(v) for v in a.views.split(',')]:
    obs = synth.make_observation(V, seed=100 + V, device=DEV)
    for T in [int(v) for v in a.sizes.split(',')]:
        model.input_size, model.camera_dist = T, optimal_camera_dist(consts.INTRINSIC[1][1], T, 0.5, slack=128 / T)
        fns = {k: arm(model, k, lambda: model.preprocess_observation(obs)) for k in ('composed', 'fused')}
        want, got = fns['composed'](), fns['fused']()
        res = {'V': V, 'T': T, 'nearest_maps_equal': bool(torch.equal(want.depth, got.depth) and torch.equal(want.mask, got.mask)),
               'colour_max_abs_diff': float((want.color - got.color).abs().max())}
        res.update(ab(fns))
        results['preprocess_observation'].append(verdict(res))
        print(json.dumps(res), flush=True)
        save(results)
        del want, got
    del obs
    torch.cuda.empty_cache()
model.input_size, model.camera_dist = own

obs = synth.make_observation(16, seed=116, device=DEV)
with torch.no_grad():
    fns = {k: arm(model, k, lambda: model.build_latent_object(obs)) for k in ('composed', 'fused')}
    want, got = fns['composed'](), fns['fused']()
    res = {'model': f'SYN({S},{C})', 'V': 16, 'T': S,
           'volume_rel_l2': float((want.double() - got.double()).norm() / want.double().norm())}
    res.update(ab(fns))
results['build_latent_object'].append(verdict(res))
print(json.dumps(res), flush=True)
save(results)
