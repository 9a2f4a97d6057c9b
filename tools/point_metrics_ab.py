#!/usr/bin/env python
"""A/B of pose scoring (ADD, ADD-S, ADD-sym, proj2d of B camera pairs on a model cloud of P points), in ONE process:

  host      : pose/metrics.py camera_metrics per pair on the CPU (the only form before camera_metrics_batch): wall clock over 4
              pairs, reported per pair
  aten      : the ADD-S part alone on device tensors as the reference shapes it, torch.cdist(..).min() in row blocks of 1000 per pair
  batch     : camera_metrics_batch on the device (all six metrics of all pairs)
  nn_dist   : the lf_nn_dist launch alone (mean only, as camera_metrics_batch issues it)

Device arms: HIP events around blocks of calls (about --block-seconds each) after a warm-up and one untimed block, the median over
--blocks blocks, aten and nn_dist alternated.  Beside each: candidate pairs per second (B P^2 / time), that rate as a share of the
VALU issue rate implied by the kernel's ISA (profiles/points_isa.txt: VALU_PER_PAIR vector instructions per (query, candidate),
one wave64 instruction per 2 cycles per SIMD, 1024 SIMDs at 2.4 GHz), the peak device memory of the aten form and of ours, and
the largest difference of the two ADD-S values.

    python tools/point_metrics_ab.py [--points 1500,10000,30000] [--pairs 1,16,128] [--json profiles/point_metrics_ab.json]
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
from latentfusion_amd import ops, three  # noqa: E402
from latentfusion_amd.modules.geometry import Camera  # noqa: E402
from latentfusion_amd.pose import metrics  # noqa: E402

VALU_PER_PAIR = 6.5                      # profiles/points_isa.txt, the loop of nn_dist_kernel<4, false>
VALU_ISSUE_PER_S = 1024 * 2.4e9 / 2 * 64   # lanes x wave64 VALU instructions per second, whole chip

ap = argparse.ArgumentParser()
ap.add_argument('--points', default='1500,10000,30000')
ap.add_argument('--pairs', default='1,16,128')
ap.add_argument('--blocks', type=int, default=5)
ap.add_argument('--block-seconds', type=float, default=0.2)
ap.add_argument('--warmup', type=int, default=2)
ap.add_argument('--json', default=os.path.join(ROOT, 'profiles', 'point_metrics_ab.json'))
a = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit('point_metrics_ab.py measures on the GPU: no device found')
DEV = 'cuda'
SCALE = 0.35


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def reps_for(fn):
    for _ in range(a.warmup):
        fn()
    torch.cuda.synchronize()
    return max(1, min(2000, int(a.block_seconds * 1e3 / max(timed(fn, 1), 1e-3))))


def stats(t, reps):
    return {'median_ms': statistics.median(t), 'min_ms': min(t), 'max_ms': max(t), 'reps_per_block': reps}


def ab(fns):
    """{arm: stats} of the callables: each its own block length, one untimed block, then alternating blocks in both orders."""
    reps = {k: reps_for(fn) for k, fn in fns.items()}
    for k, fn in fns.items():
        timed(fn, reps[k])
    times = {k: [] for k in fns}
    order = list(fns)
    for r in range(a.blocks):
        for k in (order if r % 2 == 0 else order[::-1]):
            times[k].append(timed(fns[k], reps[k]))
    return {k: stats(t, reps[k]) for k, t in times.items()}


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def cameras(B, seed):
    """B poses about 1.2 in front of a 500-pixel pinhole, and a hypothesis a few degrees and millimetres off each."""
    g = torch.Generator().manual_seed(seed)
    K = torch.tensor([[500.0, 0.0, 320.0], [0.0, 500.0, 240.0], [0.0, 0.0, 1.0]]).expand(B, 3, 3).contiguous()
    q = three.quaternion.normalize(torch.randn(B, 4, generator=g))
    dq = three.quaternion.normalize(torch.cat([torch.ones(B, 1), 0.05 * torch.randn(B, 3, generator=g)], dim=1))
    t = torch.cat([0.05 * torch.randn(B, 2, generator=g), 1.2 + 0.05 * torch.randn(B, 1, generator=g)], dim=1)
    out = []
    for quat_, trans in ((q, t), (three.quaternion.normalize(three.quaternion.qmul(dq, q)), t + 0.01 * torch.randn(B, 3, generator=g))):
        out.append(Camera(K, None, log_quaternion=three.quaternion.qlog(quat_)[:, 1:], translation=trans))
    return out


def aten_add_s(points, e_gt, e_ev):
    out = []
    for b in range(e_gt.shape[0]):
        p_gt, p_ev = three.transform_coords(points, e_gt[b:b + 1]), three.transform_coords(points, e_ev[b:b + 1])
        out.append(torch.cat([torch.cdist(p_gt[i:i + 1000], p_ev).min(dim=1).values for i in range(0, p_gt.shape[0], 1000)]).mean())
    return torch.stack(out)


def measure(P, B, host_cache):
    g = torch.Generator().manual_seed(P)
    points = (torch.rand(P, 3, generator=g) - 0.5) * 0.4
    gt, ev = cameras(B, 1000 + B)
    res = {'P': P, 'B': B, 'candidate_pairs': B * P * P}
    if P not in host_cache:                                          # per pair: does not depend on B
        n = 4
        hgt, hev = cameras(n, 999)
        metrics.camera_metrics(hgt[0], hev[0], points, SCALE)
        t0 = time.perf_counter()
        for i in range(n):
            metrics.camera_metrics(hgt[i], hev[i], points, SCALE)
        host_cache[P] = {'ms_per_pair': (time.perf_counter() - t0) * 1e3 / n, 'pairs_timed': n, 'threads': torch.get_num_threads()}
    res['host_camera_metrics'] = host_cache[P]
    gtd, evd, pd = gt.to(DEV), ev.to(DEV), points.to(DEV)
    e_gt, e_ev = gtd.obj_to_cam.contiguous(), evd.obj_to_cam.contiguous()
    t1, t2 = e_gt[:, :3].contiguous(), e_ev[:, :3].contiguous()
    fns = {'aten_cdist_min': lambda: aten_add_s(pd, e_gt, e_ev),
           'lf_nn_dist': lambda: ops.nn_dist(pd, pd, t1, t2, want=('mean',))['mean']}
    ours, theirs = fns['lf_nn_dist'](), fns['aten_cdist_min']()
    res['add_s_max_abs_diff_ours_vs_aten'] = float((ours - theirs).abs().max())
    res.update(ab(fns))
    res['camera_metrics_batch'] = ab({'batch': lambda: metrics.camera_metrics_batch(gtd, evd, pd, SCALE)})['batch']
    for k in ('aten_cdist_min', 'lf_nn_dist'):
        rate = B * P * P / (res[k]['median_ms'] * 1e-3)
        res[k]['candidate_pairs_per_s'] = rate
    res['lf_nn_dist']['share_of_valu_issue_rate'] = res['lf_nn_dist']['candidate_pairs_per_s'] * VALU_PER_PAIR / VALU_ISSUE_PER_S
    res['aten_cdist_min']['peak_bytes'] = peak_bytes(fns['aten_cdist_min'])
    res['lf_nn_dist']['peak_bytes'] = peak_bytes(fns['lf_nn_dist'])
    res['camera_metrics_batch']['peak_bytes'] = peak_bytes(lambda: metrics.camera_metrics_batch(gtd, evd, pd, SCALE))
    res['nn_dist_over_aten'] = res['lf_nn_dist']['median_ms'] / res['aten_cdist_min']['median_ms']
    res['batch_over_host'] = res['camera_metrics_batch']['median_ms'] / (res['host_camera_metrics']['ms_per_pair'] * B)
    return res


results = {'device': torch.cuda.get_device_name(0), 'blocks': a.blocks, 'block_seconds': a.block_seconds,
           'valu_per_pair': VALU_PER_PAIR, 'valu_issue_per_s': VALU_ISSUE_PER_S,
           'command': f'python tools/point_metrics_ab.py --points {a.points} --pairs {a.pairs}', 'shapes': []}
host_cache = {}
for P in [int(v) for v in a.points.split(',')]:
    for B in [int(v) for v in a.pairs.split(',')]:
        results['shapes'].append(measure(P, B, host_cache))
        print(json.dumps(results['shapes'][-1]), flush=True)
        if a.json:                                                 # (after every shape: a later one may not finish)
            os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
            with open(a.json, 'w') as f:
                json.dump(results, f, indent=1)
                f.write('\n')
