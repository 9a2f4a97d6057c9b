"""A/B of the released architecture's coarse search (BASELINE cfg 3, the workload of bench.cfg3_report) with the 3-D camera
blocks on the fp32 Winograd GEMM (conv_mode='winograd', wino_fused_kernel<3,4,2,2,2>) against the split-precision one
(conv_mode='f16x3', wino_fused_f16x3_kernel): synth.build_released_model, 8 reference views, cross_entropy_linemod
(N = 128 renders per iteration, no gradient).  Both modes in ONE process, timed blocks alternating, medians reported; then one
instrumented run per mode gives the per-launch times of the camera-block kernels from HIP events.  Prints one JSON line.
Mode 'f16x3_3d': conv_mode='f16x3' with the 2-D decoder kept on the fp32 pair (an empty ops.WIDE2D_F16X3_ROUTE): the f16x3 mode
as it was before the split-precision decoder, for the A/B of that change (--modes f16x3_3d,f16x3).

    python tools/cfg3_f16x3_ab.py [--iters 4] [--blocks 3] [--modes winograd,f16x3]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=4, help='cross-entropy iterations per timed block')
    ap.add_argument('--blocks', type=int, default=3, help='timed blocks per mode (alternating)')
    ap.add_argument('--modes', default='winograd,f16x3', help='comma-separated conv modes (rocprofv3 runs: one mode)')
    a = ap.parse_args()
    import numpy as np
    import torch

    from latentfusion_amd import ops, synth
    from latentfusion_amd.modules.geometry import Camera
    from latentfusion_amd.observation import Observation
    from latentfusion_amd.pose import estimation
    dev = 'cuda'
    model, _ = synth.build_released_model(dev, seed=0)
    model.freeze()
    ref = synth.make_observation(8, seed=100, device=dev)
    td = synth.make_observation_data(1, seed=200)
    target = Observation(td['color'], td['depth'], td['mask'], Camera(td['intrinsic'], td['extrinsic'])).to(dev)
    z_obj = model.build_latent_object(ref)
    cfg = estimation._load_toml(os.path.join(ROOT, 'configs', 'cross_entropy_linemod.toml'))
    cfg['args']['num_iters'] = a.iters
    n_r = cfg['args']['num_samples']
    modes = tuple(a.modes.split(','))
    gemm_tag = {'winograd': 'wino3d_fused', 'f16x3': 'wino3d_fused_f16x3', 'f16x3_3d': 'wino3d_fused_f16x3'}
    input_tag = {'winograd': 'wino3d_input', 'f16x3': 'wino3d_input_f16x3', 'f16x3_3d': 'wino3d_input_f16x3'}
    route = ops.WIDE2D_F16X3_ROUTE

    def run(mode):
        torch.manual_seed(300)
        np.random.seed(300)
        ops.WIDE2D_F16X3_ROUTE = {} if mode == 'f16x3_3d' else route
        try:
            est = estimation.load_from_config(cfg, model, conv_mode='f16x3' if mode == 'f16x3_3d' else mode)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            best = est.estimate(z_obj, target, camera=target.camera)
            torch.cuda.synchronize()
        finally:
            ops.WIDE2D_F16X3_ROUTE = route
        return time.perf_counter() - t0, best

    for m in modes:                                                  # warm-up: weight packs, code objects, allocator
        run(m)
    times = {m: [] for m in modes}
    rank = {}
    for _ in range(a.blocks):
        for m in modes:
            t, best = run(m)
            times[m].append(t)
            rank[m] = torch.cat((best.log_quaternion, best.translation), dim=1).cpu()
    launch = {}
    for m in modes:
        dec_tags = ('wino2d_input', 'wino2d_fused', 'wino2d_input_f16x3', 'wino2d_fused_f16x3')
        ops.KERNEL_TIMER_TAGS = {gemm_tag[m], input_tag[m], *dec_tags}
        ops.KERNEL_TIMER = []
        try:
            run(m)
            torch.cuda.synchronize()
            ev = ops.KERNEL_TIMER
        finally:
            ops.KERNEL_TIMER, ops.KERNEL_TIMER_TAGS = None, None
        gemm = [e0.elapsed_time(e1) for n_, e0, e1 in ev if n_ == gemm_tag[m]]
        inp = [e0.elapsed_time(e1) for n_, e0, e1 in ev if n_ == input_tag[m]]
        launch[m] = {'kernel': 'wino_fused_kernel<3,4,2,2,2>' if m == 'winograd' else 'wino_fused_f16x3_kernel',
                     'gemm_ms_median': statistics.median(gemm) if gemm else None, 'gemm_launches': len(gemm),
                     'input_transform_ms_median': statistics.median(inp) if inp else None,
                     'decoder_2d_ms_per_iter': {t: sum(e0.elapsed_time(e1) for n_, e0, e1 in ev if n_ == t) / a.iters
                                                for t in dec_tags}}
    it_s = {m: a.iters / statistics.median(times[m]) for m in modes}
    out = {'workload': f'cfg 3: released architecture (seeded), 8 views, cross_entropy_linemod, {n_r} renders/iteration, '
                       f'{a.iters} iterations per block, {a.blocks} alternating blocks per mode, medians',
           'iters_per_s': it_s, 'run_s': times, 'launch': launch,
           'rankings_finite': {m: bool(torch.isfinite(rank[m]).all()) for m in modes},
           'device': torch.cuda.get_device_name(0)}
    if len(modes) == 2 and 'f16x3' in modes:
        base = [m for m in modes if m != 'f16x3'][0]
        out['speedup_f16x3'] = it_s['f16x3'] / it_s[base]
        out['speedup_baseline'] = base
    g16 = launch.get('f16x3', {}).get('gemm_ms_median')
    if g16:
        macs = 64 * n_r * 8 ** 3 * 256 * 256                         # Winograd-domain MACs of one 128-render 256 -> 256 launch
        out['f16x3_gemm_f16_pflops'] = 3 * 2 * macs / (g16 * 1e-3) / 1e15      # three f16 products per fp32 product
        out['f16x3_gemm_v_read_tb_s'] = 64 * n_r * 8 ** 3 * 256 * 4 / (g16 * 1e-3) / 1e12   # V (hi + lo) read once
    print(json.dumps(out))


if __name__ == '__main__':
    main()
