#!/usr/bin/env python
"""A/B of the generator step's loss tail ALONE (GeneratorStep.losses behind the decoder: hard smooth-L1 depth term, BCE mask term,
Beta prior, total, and the backward to `depth` and `mask_logits`), in ONE process:

  composed : losses.HardPixelLoss (smooth_l1 / mean(dim=1) / topk / mean) + BCEWithLogitsLoss + losses.beta_prior_loss on
             sigmoid(logits), and their autograd nodes
  fused    : one ops.recon_losses call (lf_recon_loss_fwd: three launches; lf_recon_loss_bwd: one)

on `images` frames of S x S (depth = tanh(randn) against a target, logits = 4 randn against a {0, 1} mask), weights 25 / 25 / 1,
Beta parameter 0.01.  Every repetition is a host clock around forward + backward and a device synchronise.  After --warmup
untimed calls per arm, --reps repetitions per arm in alternating blocks of five; per arm the median, the extremes, the 10th /
90th percentiles and the spread (max - min).  `fused_wins`: the fused median lies below the composed median by more than the
larger of the two spreads.  Before anything is timed the arms' totals and gradients are compared, and the device kernels of one
call per arm are counted under the profiler.

    python tools/train_loss_ab.py [--shapes 8x128x4096,...] [--json profiles/train_loss_ab.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from latentfusion_amd import losses, ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--shapes', default='8x128x4096,8x128x16384,8x256x16384,40x128x4096,24x256x16384', help='images x frame x k')
ap.add_argument('--reps', type=int, default=30)
ap.add_argument('--warmup', type=int, default=5)
ap.add_argument('--json', default=os.path.join(ROOT, 'profiles', 'train_loss_ab.json'))
a = ap.parse_args()
if a.reps < 20:
    sys.exit('train_loss_ab.py: at least 20 repetitions')
if not torch.cuda.is_available():
    sys.exit('train_loss_ab.py measures on the GPU: no device found')
DEV = 'cuda'
BLOCK = 5
W_DEPTH, W_MASK, W_BETA, BETA = 25.0, 25.0, 1.0, 0.01


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


def device_kernels(fn):
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if e.device_type == DeviceType.CUDA]


def tail(kernel, depth, depth_gt, logits, mask_gt, k):
    """-> (total, d total / d depth, d total / d logits)."""
    if kernel == 'fused':
        terms = ops.recon_losses(depth, depth_gt, 'smooth_l1', k, logits, mask_gt, BETA)
        d, m, b = terms[0], terms[1], terms[2]
    else:
        d = losses.reduce_loss(losses.HardPixelLoss(nn.SmoothL1Loss, k, kernel='composed')(depth, depth_gt))
        m = losses.reduce_loss(F.binary_cross_entropy_with_logits(logits, mask_gt, reduction='none'))
        b = losses.beta_prior_loss(torch.sigmoid(logits), alpha=BETA, beta=BETA)
    total = W_DEPTH * d + W_MASK * m + W_BETA * b
    return (total.detach(),) + torch.autograd.grad(total, (depth, logits))


def save(results):
    if a.json:                                                     # (after every shape: a later one may not finish)
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            json.dump(results, f, indent=1)
            f.write('\n')


results = {'device': torch.cuda.get_device_name(0), 'reps': a.reps, 'warmup': a.warmup, 'threads': torch.get_num_threads(),
           'command': f'python tools/train_loss_ab.py --shapes {a.shapes} --reps {a.reps}', 'weights': [W_DEPTH, W_MASK, W_BETA],
           'shapes': []}
for spec in a.shapes.split(','):
    n, S, k = (int(v) for v in spec.split('x'))
    gen = torch.Generator().manual_seed(n + S + k)
    depth = torch.tanh(torch.randn(n, 1, S, S, generator=gen)).to(DEV).requires_grad_(True)
    depth_gt = torch.tanh(torch.randn(n, 1, S, S, generator=gen)).to(DEV)
    logits = (4 * torch.randn(n, 1, S, S, generator=gen)).to(DEV).requires_grad_(True)
    mask_gt = (torch.rand(n, 1, S, S, generator=gen) < 0.4).float().to(DEV)
    fns = {kern: (lambda kern=kern: tail(kern, depth, depth_gt, logits, mask_gt, k)) for kern in ('composed', 'fused')}
    want, got = fns['composed'](), fns['fused']()
    rel = [float((g.double() - w.double()).norm() / w.double().norm()) for w, g in zip(want, got)]
    res = {'images': n, 'frame': S, 'k': k, 'total_rel_diff': rel[0], 'depth_grad_rel_l2': rel[1], 'logit_grad_rel_l2': rel[2]}
    for kern, fn in fns.items():
        names = device_kernels(fn)
        res[kern + '_device_kernels'] = len(names)
        if kern == 'fused':
            res['fused_launches'] = len([x for x in names if 'tl_' in x])
    res.update(ab(fns))
    c, f = res['composed'], res['fused']
    res['composed_over_fused'] = c['median_ms'] / f['median_ms']
    res['fused_wins'] = bool(c['median_ms'] - f['median_ms'] > max(c['spread_ms'], f['spread_ms']))
    results['shapes'].append(res)
    print(json.dumps(res), flush=True)
    save(results)
    del depth, depth_gt, logits, mask_gt, want, got
    torch.cuda.empty_cache()
