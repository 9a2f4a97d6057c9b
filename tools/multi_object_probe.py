"""Several objects in one pose loop: per-object iterations/s of K objects x n hypotheses refined in ONE batched loop
(GradientPoseEstimator.estimate_batch with a list of K volumes, engine_multi.MultiTargetEngine on the indexed resampler)
against the same K (object, target) pairs refined one after another (estimate per pair: what the estimator did before it
took a volume list), for K in {1, 2, 4, 8} and n in {1, 8}, on

  * SYN(128,16): the headline renderer, K latent objects each built from its own 16 views with the GRU fuser;
  * the released architecture (synth.build_released_model, 16^3 x 256 latent volumes; seeded random volumes).

Both sides run the adam_quick preset with convergence disabled, in one process.  One iteration's cost is the difference of
two loop lengths (K_LONG - K_SHORT iterations), each loop bracketed by HIP events, so that engine construction and the
first call's allocations cancel.  The two variants ALTERNATE (batched, sequential, batched, ...) and the median of REPEATS
such differences is reported for each.  Per-object iterations/s: batched 1 / t_batched_iteration (every object advances once
per batched iteration), sequential 1 / (sum over the K pairs of one single-pair iteration).
Writes profiles/multi_object_probe.json.

    python tools/multi_object_probe.py [--models syn,released] [--out profiles/multi_object_probe.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

K_SHORT, K_LONG, REPEATS = 3, 13, 3


def _targets(K, dev):
    from latentfusion_amd import synth
    from latentfusion_amd.modules.geometry import Camera
    from latentfusion_amd.observation import Observation
    out = []
    for t in range(K):
        d = synth.make_observation_data(1, seed=200 + t)
        out.append(Observation(d['color'], d['depth'], d['mask'], Camera(d['intrinsic'], d['extrinsic'])).to(dev))
    return out


def _cameras(targets, n):
    from latentfusion_amd.pose import utils as pu
    torch.manual_seed(300)
    return [pu.sample_cameras_with_estimate(n, t.camera.to('cpu')) for t in targets]


def _loop_ms(fn, k):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn(k)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _per_iter_ms(fns):
    """For every variant the median over REPEATS of (t(K_LONG) - t(K_SHORT)) / (K_LONG - K_SHORT), the variants alternating."""
    for fn in fns:
        fn(1)                                                      # warm-up: packs, allocator pools, code objects
    vals = [[] for _ in fns]
    for _ in range(REPEATS):
        for v, fn in zip(vals, fns):
            v.append((_loop_ms(fn, K_LONG) - _loop_ms(fn, K_SHORT)) / (K_LONG - K_SHORT))
    return [sorted(v)[len(v) // 2] for v in vals]


def probe_model(name, model, volumes, dev, Ks=(1, 2, 4, 8), ns=(1, 8)):
    from latentfusion_amd.pose import estimation
    cfg = estimation._load_toml(os.path.join(ROOT, 'configs', 'adam_quick.toml'))
    rows = []
    all_targets = _targets(max(Ks), dev)
    for n in ns:
        est = estimation.load_from_config(cfg, model, converge_patience=10 ** 6, num_samples=n, ranking_size=n)
        for K in Ks:
            targets, zs = all_targets[:K], volumes[:K]
            cams = _cameras(targets, n)

            def batched(k):
                est.num_iters = k
                est.estimate_batch(zs, targets, cameras=[c.clone() for c in cams])

            def sequential(k):
                est.num_iters = k
                for z, t, c in zip(zs, targets, cams):
                    est.estimate(z, t, camera=c.clone())
            tb, ts = _per_iter_ms((batched, sequential))
            batched(1)
            groups = list(est.last_batch_groups)                     # targets per batched loop (one loop: [K])
            row = {'model': name, 'K': K, 'n': n, 'N': K * n, 'batch_groups': groups,
                   'batched_ms_per_iteration': round(tb, 4), 'sequential_ms_per_round': round(ts, 4),
                   'per_object_it_s_batched': round(1000.0 / tb, 2), 'per_object_it_s_sequential': round(1000.0 / ts, 2),
                   'gain': round(ts / tb, 3), 'batched_ms_per_hypothesis_iteration': round(tb / (K * n), 4)}
            print(json.dumps(row), flush=True)
            rows.append(row)
            torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--models', default='syn,released')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'multi_object_probe.json'))
    a = ap.parse_args()
    from latentfusion_amd import synth
    from latentfusion_amd.modules.geometry import Camera
    from latentfusion_amd.observation import Observation
    dev = 'cuda'
    KMAX = 8
    out = {'what': __doc__.strip().split('\n\n')[0], 'device': torch.cuda.get_device_name(0), 'torch': torch.__version__,
           'k_short': K_SHORT, 'k_long': K_LONG, 'repeats': REPEATS, 'order': 'batched and sequential alternate within a repeat',
           'preset': 'adam_quick (convergence disabled)', 'rows': []}
    t0 = time.time()
    if 'syn' in a.models.split(','):
        S, C, V = 128, 16, 16
        model, _ = synth.build_model(S, C, 'gru', seed=0, device=dev)
        model.freeze()
        volumes = []
        for k in range(KMAX):
            rd = synth.make_observation_data(V, seed=100 + k)
            ref = Observation(rd['color'], rd['depth'], rd['mask'],
                              Camera(rd['intrinsic'], rd['extrinsic'], width=rd['width'], height=rd['height'])).to(dev)
            with torch.no_grad():
                volumes.append(model.build_latent_object(ref))
            del ref
        torch.cuda.empty_cache()
        out['rows'] += probe_model('SYN(128,16) 16 views GRU', model, volumes, dev)
        del model, volumes
        torch.cuda.empty_cache()
    if 'released' in a.models.split(','):
        model, _ = synth.build_released_model(dev, seed=0)
        model.freeze()
        volumes = [torch.randn(1, 1, 256, 16, 16, 16, generator=torch.Generator().manual_seed(5 + k)).to(dev) for k in range(KMAX)]
        out['rows'] += probe_model('released architecture (seeded random volumes)', model, volumes, dev)
    out['wall_s'] = round(time.time() - t0, 1)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
    print('wrote', a.out)


if __name__ == '__main__':
    main()
