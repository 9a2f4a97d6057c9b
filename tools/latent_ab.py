#!/usr/bin/env python
"""A/B of the engines' latent loss term, latent_kernel 'autograd' against 'fused', in ONE process:

  autograd : the ATen cosine chain; on a gradient call the pose loss and the 2-D decoder as autograd nodes
  fused    : lf_latent_cosine_fwd + lf_latent_cosine_bwd_epi; a gradient call keeps the explicit decoder and the two-launch loss

Per shape (a renderer and a number of hypotheses N) two engines on the same target time RenderLoopEngine.forward_backward with a
FIXED target code zt, as a gradient call and as a ranking call (need_grad=False, masked depth): HIP events around blocks of
calls (about --block-seconds each) after a warm-up and one untimed block per arm, the median over --blocks blocks, the two arms
alternated and run in both orders.  Beside each, for context only: the time of ONE LatentFusionModel.compute_latent_code call
(the other per-iteration cost of the latent presets; not touched by the option), and the launch time of the two new kernels
alone at the shape's projected latent with the share of the HBM rate (8.0 TB/s) their algorithmic bytes reach.

Shapes: SYN(128,16) at N = 16 with the adam_latent preset's weights (its num_samples), and the released architecture at
N = 16 and N = 128.

    python tools/latent_ab.py [--shapes syn128:16,released:16,released:128] [--json profiles/latent_fused_ab.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from latentfusion_amd import ops, synth  # noqa: E402
from latentfusion_amd._lib import LF_EPI_LRELU, LF_EPI_PIXELNORM  # noqa: E402
from latentfusion_amd.engine import RenderLoopEngine  # noqa: E402
from latentfusion_amd.modules.geometry import Camera  # noqa: E402
from latentfusion_amd.observation import Observation  # noqa: E402
from latentfusion_amd.pose import estimation, utils as pu  # noqa: E402

HBM_BYTES_PER_S = 8.0e12

ap = argparse.ArgumentParser()
ap.add_argument('--shapes', default='syn128:16,released:16,released:128')
ap.add_argument('--blocks', type=int, default=7)
ap.add_argument('--block-seconds', type=float, default=0.3)
ap.add_argument('--warmup', type=int, default=3)
ap.add_argument('--json', default=os.path.join(ROOT, 'profiles', 'latent_fused_ab.json'))
a = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit('latent_ab.py measures on the GPU: no device found')
DEV = 'cuda'
ARMS = ('autograd', 'fused')
WEIGHTS = dict(estimation._load_toml(os.path.join(ROOT, 'configs', 'adam_latent.toml'))['loss_weights'])


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def reps_for(fn):
    """Calls per block: about --block-seconds of work, judged after the warm-up."""
    for _ in range(a.warmup):
        fn()
    torch.cuda.synchronize()
    return max(2, min(2000, int(a.block_seconds * 1e3 / max(timed(fn, 2), 1e-3))))


def ab(fns):
    """{arm: stats} of the two callables: common block length, one untimed block each, then alternating blocks in both orders."""
    reps = max(reps_for(fn) for fn in fns.values())
    for fn in fns.values():
        timed(fn, reps)
    times = {k: [] for k in fns}
    for r in range(a.blocks):
        for k in (ARMS if r % 2 == 0 else ARMS[::-1]):
            times[k].append(timed(fns[k], reps))
    out = {k: {'median_ms': statistics.median(t), 'min_ms': min(t), 'max_ms': max(t), 'blocks_ms': t} for k, t in times.items()}
    out['reps_per_block'] = reps
    out['fused_over_autograd'] = out['fused']['median_ms'] / out['autograd']['median_ms']
    return out


def one(fn):
    reps = reps_for(fn)
    timed(fn, reps)
    t = [timed(fn, reps) for _ in range(a.blocks)]
    return {'median_ms': statistics.median(t), 'min_ms': min(t), 'max_ms': max(t), 'reps_per_block': reps}


def build(kind):
    """(model, z_obj, target with colour) of a renderer family, seeded."""
    if kind == 'released':
        model, _ = synth.build_released_model(DEV, seed=0)
    else:
        S = int(kind[3:])
        model, _ = synth.build_model(S, 16, 'gru', seed=0, device=DEV)
    model.freeze()
    ref = synth.make_observation(8, seed=100, device=DEV)
    td = synth.make_observation_data(1, seed=200)
    target = Observation(td['color'], td['depth'], td['mask'], Camera(td['intrinsic'], td['extrinsic'])).to(DEV)
    with torch.no_grad():
        z_obj = model.build_latent_object(ref)
    return model, z_obj, target


def measure(kind, N, built):
    model, z_obj, target = built
    torch.manual_seed(300)
    cams = pu.sample_cameras_with_estimate(N, estimation.PoseEstimator.initial_pose(target))
    zc = cams.zoom(None, model.input_size, model.camera_dist).to(DEV)
    with torch.no_grad():
        zt = model.compute_latent_code(target, zc).detach()
    engs = {k: RenderLoopEngine(model.photographer, z_obj, target, WEIGHTS, latent_kernel=k) for k in ARMS}
    grabbed = {}
    inner = engs['fused']._tail_fwd

    def tail_fwd(*args):
        tail = inner(*args)
        grabbed['zp'], grabbed['pnorm'] = tail.zp, tail.pnorm
        return tail
    engs['fused']._tail_fwd = tail_fwd
    with model.frozen():
        out = {k: engs[k].forward_backward(zc, z_target_latent=zt) for k in ARMS}
    engs['fused']._tail_fwd = inner
    torch.cuda.synchronize()
    (la, ga), (lf, gf) = out['autograd'], out['fused']
    res = {'renderer': kind, 'N': N, 'zt_shape': list(zt.shape), 'zp_shape': list(grabbed['zp'].shape),
           'explicit_decoder': engs['fused'].dec is not None, 'conv_mode': engs['fused'].conv_mode,
           'fused_idle': grabbed['pnorm'] is None,
           'outputs_agree': {'losses_max_abs_diff': float((la - lf).abs().max()),
                             'latent_max_abs_diff': float((la[:, 5] - lf[:, 5]).abs().max()),
                             'gparams_max_rel_l2': float(((ga - gf).norm(dim=1) / ga.norm(dim=1)).max())}}
    with model.frozen():
        res['gradient_call'] = ab({k: (lambda e=engs[k]: e.forward_backward(zc, z_target_latent=zt)) for k in ARMS})
        with torch.no_grad():
            res['ranking_call'] = ab({k: (lambda e=engs[k]: e.forward_backward(zc, need_grad=False, z_target_latent=zt,
                                                                               masked_depth=True)) for k in ARMS})
            res['compute_latent_code_context'] = one(lambda: model.compute_latent_code(target, zc))
    # the two kernels alone at this shape's projected latent (zt: as the engine hands it over, N rows in its own layout)
    if grabbed['pnorm'] is not None:
        zp, pnorm = grabbed['zp'], grabbed['pnorm']
        n, C, h, w = zp.shape
        g_in = torch.randn_like(zp)
        ztf = zt.to(torch.float32)
        sums = ops.latent_cosine_fwd(zp, ztf)
        elems = n * C * h * w
        kern = {'lf_latent_cosine_fwd': (lambda: ops.latent_cosine_fwd(zp, ztf), 2 * elems * 4),
                'lf_latent_cosine_bwd_epi': (lambda: ops.latent_cosine_bwd_epi(g_in, zp, pnorm, ztf, sums, 0.2 / n,
                                                                               LF_EPI_LRELU | LF_EPI_PIXELNORM),
                                             (4 * elems + n * h * w) * 4)}
        res['kernels'] = {}
        for name, (fn, nbytes) in kern.items():
            t = one(fn)
            t['algorithmic_bytes'] = nbytes
            t['share_of_8_TB_per_s'] = nbytes / (t['median_ms'] * 1e-3) / HBM_BYTES_PER_S
            t['note'] = 'launch time through the ops wrapper (output and scratch allocation included), HIP events around a block'
            res['kernels'][name] = t
    return res


results = {'device': torch.cuda.get_device_name(0), 'weights': WEIGHTS, 'blocks': a.blocks, 'block_seconds': a.block_seconds,
           'command': 'python tools/latent_ab.py --shapes ' + a.shapes, 'shapes': []}
cache = {}
for spec in a.shapes.split(','):
    kind, N = spec.split(':')
    if kind not in cache:
        cache.clear()                                              # one renderer resident at a time
        torch.cuda.empty_cache()
        cache[kind] = build(kind)
    try:
        results['shapes'].append(measure(kind, int(N), cache[kind]))
    except torch.cuda.OutOfMemoryError as e:                      # written down as it is; the smaller shapes stand
        results['shapes'].append({'renderer': kind, 'N': int(N), 'error': 'out of memory: ' + str(e).split('\n')[0]})
        torch.cuda.empty_cache()
    print(json.dumps(results['shapes'][-1]), flush=True)
    if a.json:                                                     # (after every shape: a later one may not finish)
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            json.dump(results, f, indent=1)
            f.write('\n')
