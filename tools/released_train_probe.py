#!/usr/bin/env python
"""The generator training step (recon/training.GeneratorStep; reference tools/train/train_reconstruct.py:421-535) on the
RELEASED architecture (synth.build_released_model: 256^2 inputs, 16^3 x 256 volume, 68 M parameters): 1 object, V_in input
and V_out output views (the recipe's 8 + 24 by default), fp32 or the bf16 autocast policy.

Reports, with WIDE_WGRAD (lf_conv_bwd_weight_wide) on and off in one process:
  * step time (median of --steps after --warmup) and peak memory;
  * the weight gradient of every routed layer class (dims, Cin -> Cout, batch x extent, launches per step), timed on the
    same random operands with lf_conv_bwd_weight_wide and lf_conv_bwd_weight, with FLOPs and TF/s;
  * whether two steps' gradients are bit-identical (report only).

    python tools/released_train_probe.py [--views-in 8] [--views-out 24] [--steps 5] [--warmup 2] [--amp] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _batch(model, vin, vout, dev):
    from latentfusion_amd import synth
    obs_in = model.preprocess_observation(synth.make_observation(vin, seed=1, device=dev))
    obs_out = model.preprocess_observation(synth.make_observation(vout, seed=2, device=dev))
    return {'in': {'camera': obs_in.camera, 'image': obs_in.color.unsqueeze(0), 'mask': obs_in.mask.unsqueeze(0)},
            'out_gt': {'camera': obs_out.camera, 'depth': obs_out.depth.unsqueeze(0), 'mask': obs_out.mask.unsqueeze(0)}}


def _time_steps(step, batch, steps, warmup):
    for _ in range(warmup):
        step.run_iteration(batch, is_step=False)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        step.run_iteration(batch, is_step=False)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return ts, torch.cuda.max_memory_allocated() / 2 ** 30


def _record_classes(step, batch):
    """(dims, N, D, H, W, Cin, Cout) -> launches per step of every weight gradient ops_train routes to the wide kernel."""
    from latentfusion_amd import ops_train
    seen = {}
    orig = ops_train.conv_bwd_weight

    def rec(x, gp, dims, cin, he, want_bias=True, bf16=None):
        cout = gp.shape[1]
        if ops_train._wide_wgrad_ok(x, gp, dims, cin, cout):
            if dims == 0:
                key = (0, 1, 1, 1, gp.shape[0], cin, cout)
            else:
                N = gp.shape[0]
                D, H, W = gp.shape[2:] if dims == 3 else (1,) + tuple(gp.shape[2:])
                key = (dims, N, D, H, W, cin, cout)
            seen[key] = seen.get(key, 0) + 1
        return orig(x, gp, dims, cin, he, want_bias, bf16)
    ops_train.conv_bwd_weight = rec
    try:
        step.run_iteration(batch, is_step=False)
        torch.cuda.synchronize()
    finally:
        ops_train.conv_bwd_weight = orig
    return seen


def _time_class(key, reps=5):
    from latentfusion_amd import _lib
    L = _lib.lib()
    dims, N, D, H, W, cin, cout = key
    rows = N * D * H * W
    taps = {0: 1, 2: 9, 3: 27}[dims]
    g = torch.Generator(device='cuda').manual_seed(0)
    x = torch.randn(rows * cin, device='cuda', generator=g)
    gp = torch.randn(rows * cout, device='cuda', generator=g)
    gw = torch.empty(taps * cout * cin, device='cuda')
    res = {}
    outs = {}
    for name, entry, sb in (('wide', L.lf_conv_bwd_weight_wide, L.lf_conv_bwd_weight_wide_scratch_bytes),
                            ('generic', L.lf_conv_bwd_weight, L.lf_conv_bwd_weight_scratch_bytes)):
        nb = sb(dims, N, D, H, W, cin, cout)
        scr = torch.empty(nb // 4 + 4, device='cuda')
        stream = torch.cuda.current_stream().cuda_stream

        def run():
            rc = entry(x.data_ptr(), gp.data_ptr(), gw.data_ptr(), scr.data_ptr(), scr.numel() * 4, dims, N, D, H, W, cin, cout,
                       ctypes.c_float(1.0), stream)
            assert rc == 0, (name, rc)
        run()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        res[name + '_ms'] = statistics.median(ts)
        outs[name] = gw.clone()
        del scr
    flops = 2.0 * taps * cin * cout * rows
    res['gflop'] = flops / 1e9
    res['wide_tflops'] = flops / res['wide_ms'] / 1e9
    res['generic_tflops'] = flops / res['generic_ms'] / 1e9
    res['speedup'] = res['generic_ms'] / res['wide_ms']
    d = (outs['wide'] - outs['generic']).abs().max().item()
    res['max_abs_diff_vs_generic_rel'] = d / max(outs['generic'].abs().max().item(), 1e-30)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--views-in', type=int, default=8)
    ap.add_argument('--views-out', type=int, default=24)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--amp', action='store_true', help='bf16 autocast policy (GeneratorStep(use_amp=True))')
    ap.add_argument('--skip-classes', action='store_true', help='no per-class weight-gradient A/B')
    ap.add_argument('--modes', default='on,off,on', help='WIDE_WGRAD settings timed in turn (on / off)')
    ap.add_argument('--out', default=None)
    ap.add_argument('--loss-kernel', choices=('composed', 'fused'), default='composed',
                    help='loss tail: the ATen chain or ops.recon_losses (GeneratorStep(loss_kernel=...))')
    a = ap.parse_args()
    dev = 'cuda:0'
    from latentfusion_amd import ops_train, synth
    from latentfusion_amd.recon import training
    model, _ = synth.build_released_model(device=dev, seed=0)
    step = training.GeneratorStep(model.sculptor, model.fuser, model.photographer, use_amp=a.amp, loss_kernel=a.loss_kernel)
    batch = _batch(model, a.views_in, a.views_out, dev)
    out = {'arch': 'released', 'params_M': sum(q.numel() for q in step.flat.params) / 1e6, 'objects': 1,
           'views_in': a.views_in, 'views_out': a.views_out, 'amp': a.amp, 'loss_kernel': a.loss_kernel, 'device': torch.cuda.get_device_name(0)}
    saved = ops_train.WIDE_WGRAD
    for on in [m == 'on' for m in a.modes.split(',')]:   # on / off / on: the second "on" shows drift within the process
        ops_train.WIDE_WGRAD = on
        ts, peak = _time_steps(step, batch, a.steps, a.warmup)
        key = 'wide_wgrad_on' if on else 'wide_wgrad_off'
        if key in out:
            key += '_repeat'
        out[key] = {'step_ms_median': 1e3 * statistics.median(ts), 'step_ms': [1e3 * t for t in ts], 'peak_mem_GiB': peak}
        print(key, json.dumps(out[key]), flush=True)
    ops_train.WIDE_WGRAD = True
    step.run_iteration(batch, is_step=False)
    g1 = step.flat.grad.clone()
    step.run_iteration(batch, is_step=False)
    g2 = step.flat.grad.clone()
    out['grads_finite'] = bool(torch.isfinite(g1).all())
    out['two_steps_bit_identical'] = bool(torch.equal(g1, g2))
    out['two_steps_max_rel_diff'] = float((g1 - g2).abs().max() / g1.abs().max().clamp_min(1e-30))
    out['loss'] = {k: float(v) for k, v in step.run_iteration(batch, is_step=False).items()}
    ops_train.WIDE_WGRAD = saved
    if not a.skip_classes:
        seen = _record_classes(step, batch)
        classes = []
        for key, n in sorted(seen.items()):
            r = _time_class(key)
            dims, N, D, H, W, cin, cout = key
            r.update({'dims': dims, 'batch_extent': [N, D, H, W], 'cin': cin, 'cout': cout, 'launches_per_step': n})
            classes.append(r)
            print(json.dumps(r), flush=True)
        out['classes'] = classes
        out['wgrad_ms_per_step_wide'] = sum(c['wide_ms'] * c['launches_per_step'] for c in classes)
        out['wgrad_ms_per_step_generic'] = sum(c['generic_ms'] * c['launches_per_step'] for c in classes)
    if 'wide_wgrad_on' in out and 'wide_wgrad_off' in out:
        out['speedup_step'] = out['wide_wgrad_off']['step_ms_median'] / out['wide_wgrad_on']['step_ms_median']
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
