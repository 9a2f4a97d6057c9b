"""Several targets in one pose loop: per-target iterations/s of T targets x n hypotheses refined in ONE batched loop
(GradientPoseEstimator.estimate_batch on engine_multi.MultiTargetEngine) against the same targets refined one after
another (estimate per target), for T in {1, 2, 4, 8} and n in {1, 8}, on

  * SYN(128,16): the headline renderer, latent object built from 16 views with the GRU fuser;
  * the released architecture (synth.build_released_model, 16^3 x 256 latent volume; seeded random volume).

Both sides run the adam_quick preset with convergence disabled, in one process.  One iteration's cost is the difference of
two loop lengths (K_LONG - K_SHORT iterations), each loop bracketed by HIP events, so that engine construction and the
first call's allocations cancel.  Per-target iterations/s: batched 1 / t_batched_iteration (every target advances once per
batched iteration), sequential 1 / (sum over the T targets of one single-target iteration).
Writes profiles/multi_target_probe.json.

--per-target-plan adds a third variant, the batched loop with GradientPoseEstimator(per_target_plan=True) (every wide
Winograd launch takes the frequency split of one target's rows, lf_wino_fused_gemm_part: the batch then reproduces estimate()
bit for bit on wide renderers, at the price of more partial sums written and re-read).  The three variants alternate inside
every repeat -- batch plan, per-target plan, sequential -- and each row carries the spread (max - min over the repeats,
relative to the median) of every variant, the yardstick for "slower than sequential".  SYN(128,16) has no wide layer: its
two batched columns are a control that must not move.  Writes profiles/multi_target_part_plan_probe.json.

    python tools/multi_target_probe.py [--models syn,released] [--per-target-plan] [--out FILE]
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


def _targets(T, dev):
    from latentfusion_amd import synth
    from latentfusion_amd.modules.geometry import Camera
    from latentfusion_amd.observation import Observation
    out = []
    for t in range(T):
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


def _per_iter_ms(fn):
    """Median over REPEATS of (t(K_LONG) - t(K_SHORT)) / (K_LONG - K_SHORT)."""
    fn(1)                                                          # warm-up: packs, allocator pools, code objects
    vals = sorted((_loop_ms(fn, K_LONG) - _loop_ms(fn, K_SHORT)) / (K_LONG - K_SHORT) for _ in range(REPEATS))
    return vals[len(vals) // 2]


def _alternating_ms(fns):
    """{name: (median, spread)} of the per-iteration cost of several variants measured in turn inside every repeat; spread =
    (max - min) / median over the REPEATS."""
    for fn in fns.values():
        fn(1)                                                      # warm-up: packs, allocator pools, code objects
    vals = {k: [] for k in fns}
    for _ in range(REPEATS):
        for k, fn in fns.items():
            vals[k].append((_loop_ms(fn, K_LONG) - _loop_ms(fn, K_SHORT)) / (K_LONG - K_SHORT))
    out = {}
    for k, v in vals.items():
        v.sort()
        med = v[len(v) // 2]
        out[k] = (med, (v[-1] - v[0]) / med)
    return out


def probe_part_plan(name, model, z_obj, dev, Ts=(1, 2, 4, 8), ns=(1, 8)):
    """probe_model with the per-target launch plan as a third variant (--per-target-plan)."""
    from latentfusion_amd.pose import estimation
    cfg = estimation._load_toml(os.path.join(ROOT, 'configs', 'adam_quick.toml'))
    rows = []
    all_targets = _targets(max(Ts), dev)
    for n in ns:
        ests = {flag: estimation.load_from_config(cfg, model, converge_patience=10 ** 6, num_samples=n, ranking_size=n,
                                                  per_target_plan=flag) for flag in (False, True)}
        for T in Ts:
            targets = all_targets[:T]
            cams = _cameras(targets, n)

            def batched(k, est):
                est.num_iters = k
                est.estimate_batch(z_obj, targets, cameras=[c.clone() for c in cams])

            def sequential(k):
                ests[False].num_iters = k
                for t, c in zip(targets, cams):
                    ests[False].estimate(z_obj, t, camera=c.clone())
            m = _alternating_ms({'batch_plan': lambda k: batched(k, ests[False]), 'per_target_plan': lambda k: batched(k, ests[True]),
                                 'sequential': sequential})
            (tb, sb), (tp, sp), (ts, ss) = m['batch_plan'], m['per_target_plan'], m['sequential']
            row = {'model': name, 'T': T, 'n': n, 'N': T * n,
                   'batched_ms_per_iteration': round(tb, 4), 'per_target_plan_ms_per_iteration': round(tp, 4),
                   'sequential_ms_per_round': round(ts, 4),
                   'per_target_it_s_batched': round(1000.0 / tb, 2), 'per_target_it_s_per_target_plan': round(1000.0 / tp, 2),
                   'per_target_it_s_sequential': round(1000.0 / ts, 2),
                   'gain': round(ts / tb, 3), 'gain_per_target_plan': round(ts / tp, 3),
                   'per_target_plan_over_batch_plan': round(tp / tb, 3),
                   'spread': {'batch_plan': round(sb, 4), 'per_target_plan': round(sp, 4), 'sequential': round(ss, 4)},
                   'per_target_plan_slower_than_sequential_beyond_spread': bool(T > 1 and tp > ts * (1.0 + max(sp, ss)))}
            print(json.dumps(row), flush=True)
            rows.append(row)
            torch.cuda.empty_cache()
    return rows


def probe_model(name, model, z_obj, dev, Ts=(1, 2, 4, 8), ns=(1, 8)):
    from latentfusion_amd.pose import estimation
    cfg = estimation._load_toml(os.path.join(ROOT, 'configs', 'adam_quick.toml'))
    rows = []
    all_targets = _targets(max(Ts), dev)
    for n in ns:
        est = estimation.load_from_config(cfg, model, converge_patience=10 ** 6, num_samples=n, ranking_size=n)
        for T in Ts:
            targets = all_targets[:T]
            cams = _cameras(targets, n)

            def batched(k):
                est.num_iters = k
                est.estimate_batch(z_obj, targets, cameras=[c.clone() for c in cams])

            def sequential(k):
                est.num_iters = k
                for t, c in zip(targets, cams):
                    est.estimate(z_obj, t, camera=c.clone())
            tb = _per_iter_ms(batched)
            groups = list(est.last_batch_groups)                     # targets per batched loop (one loop: [T])
            ts = _per_iter_ms(sequential)
            row = {'model': name, 'T': T, 'n': n, 'N': T * n, 'batch_groups': groups,
                   'batched_ms_per_iteration': round(tb, 4), 'sequential_ms_per_round': round(ts, 4),
                   'per_target_it_s_batched': round(1000.0 / tb, 2), 'per_target_it_s_sequential': round(1000.0 / ts, 2),
                   'gain': round(ts / tb, 3), 'batched_ms_per_hypothesis_iteration': round(tb / (T * n), 4)}
            print(json.dumps(row), flush=True)
            rows.append(row)
            torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--models', default='syn,released')
    ap.add_argument('--per-target-plan', action='store_true',
                    help='also measure the batched loop with per_target_plan=True, the three variants alternating')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, 'profiles', 'multi_target_part_plan_probe.json' if a.per_target_plan else 'multi_target_probe.json')
    probe = probe_part_plan if a.per_target_plan else probe_model
    from latentfusion_amd import synth
    from latentfusion_amd.modules.geometry import Camera
    from latentfusion_amd.observation import Observation
    dev = 'cuda'
    out = {'what': __doc__.strip().split('\n\n')[0], 'per_target_plan': bool(a.per_target_plan), 'device': torch.cuda.get_device_name(0), 'torch': torch.__version__,
           'k_short': K_SHORT, 'k_long': K_LONG, 'repeats': REPEATS, 'preset': 'adam_quick (convergence disabled)',
           'rows': []}
    t0 = time.time()
    if 'syn' in a.models.split(','):
        S, C, V = 128, 16, 16
        model, _ = synth.build_model(S, C, 'gru', seed=0, device=dev)
        model.freeze()
        rd = synth.make_observation_data(V, seed=100)
        ref = Observation(rd['color'], rd['depth'], rd['mask'],
                          Camera(rd['intrinsic'], rd['extrinsic'], width=rd['width'], height=rd['height'])).to(dev)
        with torch.no_grad():
            z_obj = model.build_latent_object(ref)
        del ref
        torch.cuda.empty_cache()
        out['rows'] += probe('SYN(128,16) 16 views GRU', model, z_obj, dev)
        del model, z_obj
        torch.cuda.empty_cache()
    if 'released' in a.models.split(','):
        model, _ = synth.build_released_model(dev, seed=0)
        model.freeze()
        z_obj = torch.randn(1, 1, 256, 16, 16, 16, generator=torch.Generator().manual_seed(5)).to(dev)
        out['rows'] += probe('released architecture (seeded random volume)', model, z_obj, dev)
    out['wall_s'] = round(time.time() - t0, 1)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
    print('wrote', a.out)


if __name__ == '__main__':
    main()
