#!/usr/bin/env python
"""Outputs and launch counts of the render-loop engines over their configurations, for comparing two checkouts of this repository
bit for bit (a refactor of engine.py / engine_multi.py / experimental.py must change neither).

    python tools/engine_parity.py run OUT_DIR              every configuration: OUT_DIR/<name>.{losses,gparams}.npy of the first and
                                                           of a second call, OUT_DIR/launches.json = {name: {entry point: launches}}
                                                           counted by _lib.BYTE_LOG around the second call
    python tools/engine_parity.py compare A B C OUT.json   A, B: two runs of the parent, C: one run of the change

Only the engines' public surface is used (constructors, forward_backward, set_streams), so the same file runs against either
checkout: put it beside the checkout's `latentfusion_amd` (it imports the package of the tree it lies in)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
DEV = 'cuda:0'
W = {'depth': 1.0, 'ov_depth': 0.3, 'iou': 0.2, 'mask': 0.4}


def _run(out):
    import torch
    sys.path.insert(0, ROOT)
    from latentfusion_amd import _lib, synth
    from latentfusion_amd.engine import RenderLoopEngine
    from latentfusion_amd.engine_multi import MultiTargetEngine
    from latentfusion_amd.experimental import RenderLoopEngineX
    from latentfusion_amd.modules.geometry import Camera
    from latentfusion_amd.observation import Observation
    from latentfusion_amd.pose import estimation, utils as pu
    from latentfusion_amd.recon.models import Photographer

    os.makedirs(out, exist_ok=True)
    launches = {}

    def golden(name):
        return torch.load(os.path.join(GOLDEN, name + '.pt'), weights_only=False)

    def camera(d, device=DEV):
        return Camera(d['K'].to(device), None, d['z_span'], d['viewport'].to(device), width=d['width'], height=d['height'],
                      log_quaternion=d['log_q'].to(device), translation=d['t'].to(device))

    def target_of(g):
        tg = g['target']
        return Observation(None, tg['depth'], tg['mask'].float(), camera(tg['cam'], 'cpu')).to(DEV)

    def frozen(ck):
        ph = Photographer.from_checkpoint(ck).to(DEV)
        for p in ph.parameters():
            p.requires_grad_(False)
        return ph

    def record(name, call):
        """Two calls: the first also builds whatever the engine builds lazily, the second is the steady state that is counted."""
        for tag in ('first', 'second'):
            if tag == 'second':
                _lib.BYTE_LOG = {}
            try:
                losses, gparams = call()
                torch.cuda.synchronize()
            finally:
                if tag == 'second':
                    launches[name] = {k: v[0] for k, v in sorted(_lib.BYTE_LOG.items())}
                    _lib.BYTE_LOG = None
            np.save(os.path.join(out, f'{name}.{tag}.losses.npy'), losses.detach().cpu().numpy())
            if gparams is not None:
                np.save(os.path.join(out, f'{name}.{tag}.gparams.npy'), gparams.detach().cpu().numpy())
        print('done', name, flush=True)

    def three_forms(name, make, cam, zt):
        """need_grad, the masked ranking form, and the latent term (gradient and ranking) of one engine configuration."""
        eng = make(W)
        record(name + '.grad', lambda: eng.forward_backward(cam))
        record(name + '.rank_masked', lambda: eng.forward_backward(cam, need_grad=False, masked_depth=True))
        engl = make(dict(W, latent=0.5))
        record(name + '.latent_grad', lambda: engl.forward_backward(cam, z_target_latent=zt))
        record(name + '.latent_rank', lambda: engl.forward_backward(cam, need_grad=False, z_target_latent=zt))

    # ---- the headline SYN model ----
    S, C, N = 128, 16, 8
    model, _ = synth.build_model(S, C, 'gru', seed=0, device=DEV, bias_std=0.05)
    model.freeze()
    ph = model.photographer
    tg0 = synth.make_observation(1, 5, DEV)
    gen = torch.Generator().manual_seed(9)
    z_obj = torch.randn(1, 1, C, S, S, S, generator=gen).to(DEV)
    torch.manual_seed(300)
    init = pu.sample_cameras_with_estimate(N, estimation.PoseEstimator.initial_pose(tg0))
    cam = init.zoom(None, model.input_size, model.camera_dist).to(DEV)
    c2 = ph.projection_block.conv.module.weight.shape[0]
    zt = torch.randn(1, c2, S, S, generator=gen).to(DEV)
    for mode, kw in (('winograd', {}), ('winograd_nofuse', {'fuse_projection': False}), ('fp32', {}), ('f16x3', {})):
        three_forms('syn.' + mode, lambda w, m=mode.split('_')[0], kw=kw: RenderLoopEngine(ph, z_obj, tg0, w, conv_mode=m, **kw),
                    cam, zt)

    # ---- several targets in one batch ----
    targets = [Observation(None, torch.roll(tg0.depth, sh, (-2, -1)).contiguous(), torch.roll(tg0.mask, sh, (-2, -1)).contiguous(),
                           tg0.camera) for sh in ((0, 0), (9, -14))]
    n = N // 2
    for lat in (False, True):
        engm = MultiTargetEngine(ph, z_obj, targets, dict(W, latent=0.5) if lat else W)
        kw = {'z_target_latent': zt.expand(2, -1, -1, -1).contiguous()} if lat else {}
        tag = 'multi.latent' if lat else 'multi'
        record(tag + '.grad', lambda: engm.forward_backward(cam, n, **kw))
        record(tag + '.rank_masked', lambda: engm.forward_backward(cam, n, need_grad=False, masked_depth=not lat, **kw))

    # ---- the experimental variants ----
    engx = RenderLoopEngineX(ph, z_obj, tg0, W, conv_mode='winograd_f16x3')
    record('x.winograd_f16x3.grad', lambda: engx.forward_backward(cam))
    record('x.winograd_f16x3.rank', lambda: engx.forward_backward(cam, need_grad=False))
    engx = RenderLoopEngineX(ph, z_obj, tg0, W, fuse_projection=('fwd', 'bwd'))
    record('x.fuse_fwd_bwd.grad', lambda: engx.forward_backward(cam))
    engx = RenderLoopEngineX(ph, z_obj, tg0, W).set_streams(2)
    record('x.streams2.grad', lambda: engx.forward_backward(cam))
    del engx, engm, model, ph, z_obj, zt
    torch.cuda.empty_cache()

    # ---- golden renderers: the three variants of g5, the occlusion-16 renderer of g28, the released width of g20 ----
    t7 = golden('g7_adam_trace')
    g5 = golden('g5_decode')
    for variant in ('factor', 'sum', 'occlusion'):
        r = g5[variant]
        eng = RenderLoopEngine(frozen(r['ck']), r['z_obj'].to(DEV), target_of(t7), W)
        cam5 = camera(r['cam'])
        record(f'g5.{variant}.grad', lambda: eng.forward_backward(cam5))
        record(f'g5.{variant}.rank', lambda: eng.forward_backward(cam5, need_grad=False))
    g28 = golden('g28_occlusion16')
    cam28 = camera(g28['init']).zoom(None, g28['S'], g28['camera_dist'])
    for proj in ('factor', 'sum'):
        eng = RenderLoopEngine(frozen(g28['variants'][proj]['photographer']), g28['z_obj'].to(DEV), target_of(g28),
                               dict(g28['cfg']['loss_weights']))
        record(f'g28.{proj}.grad', lambda: eng.forward_backward(cam28))
        record(f'g28.{proj}.rank', lambda: eng.forward_backward(cam28, need_grad=False))
    g20 = golden('g20_released_width')
    ph20, cam20 = frozen(g20['photographer']), camera(g20['loss']['zoomed'])
    for mode in ('winograd', 'f16x3'):
        eng = RenderLoopEngine(ph20, g20['z_obj'].to(DEV), target_of(t7), g20['loss']['weights'], conv_mode=mode)
        record(f'g20.{mode}.grad', lambda: eng.forward_backward(cam20))
        record(f'g20.{mode}.rank_masked', lambda: eng.forward_backward(cam20, need_grad=False, masked_depth=True))
    with open(os.path.join(out, 'launches.json'), 'w') as f:
        json.dump(launches, f, indent=1, sort_keys=True)
    print('wrote', len(launches), 'configurations to', out)


def _max_diff(a, b):
    x, y = np.load(a), np.load(b)
    if x.shape != y.shape:
        return float('inf')
    return 0.0 if x.tobytes() == y.tobytes() else float(np.nanmax(np.abs(x.astype(np.float64) - y.astype(np.float64))))


def _compare(a, b, c, out_json):
    """a, b: the parent twice; c: the change.  Per array: bitwise equality with the parent wherever the parent equals itself,
    else the change is held to the parent's own run-to-run difference."""
    names = sorted(f for f in os.listdir(a) if f.endswith('.npy'))
    missing = sorted(set(names) ^ set(f for f in os.listdir(c) if f.endswith('.npy')))
    la, lb, lc = (json.load(open(os.path.join(d, 'launches.json'))) for d in (a, b, c))
    arrays, unstable, failed = {}, [], list(missing)
    for f in names:
        if f in missing:
            continue
        own, got = _max_diff(os.path.join(a, f), os.path.join(b, f)), _max_diff(os.path.join(a, f), os.path.join(c, f))
        arrays[f] = {'parent_vs_parent_max_abs': own, 'change_vs_parent_max_abs': got, 'bitwise': got == 0.0}
        if own != 0.0:
            unstable.append(f)
        if got > own:
            failed.append(f)
    launch_diff = {}
    for name in sorted(set(la) | set(lc)):
        pa, pc = la.get(name, {}), lc.get(name, {})
        d = {k: [pa.get(k, 0), pc.get(k, 0)] for k in sorted(set(pa) | set(pc)) if pa.get(k, 0) != pc.get(k, 0)}
        if d or la.get(name) != lb.get(name):
            launch_diff[name] = {'parent_vs_change': d, 'parent_runs_agree': la.get(name) == lb.get(name)}
    res = {'what': 'tools/engine_parity.py: the parent commit run twice (A, B) against this change (C)',
           'configurations': len(la), 'arrays': len(names), 'arrays_bitwise_equal_to_parent': sum(v['bitwise'] for v in arrays.values()),
           'parent_disagrees_with_itself': unstable, 'arrays_failing': failed,
           'launch_count_differences': launch_diff, 'launches_per_call': lc,
           'pass': not failed and not any(v['parent_vs_change'] for v in launch_diff.values()),
           'per_array': {k: v for k, v in arrays.items() if not v['bitwise']}}
    with open(out_json, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps({k: res[k] for k in ('configurations', 'arrays', 'arrays_bitwise_equal_to_parent',
                                          'parent_disagrees_with_itself', 'arrays_failing', 'launch_count_differences', 'pass')}, indent=1))
    return 0 if res['pass'] else 1


if __name__ == '__main__':
    if len(sys.argv) == 3 and sys.argv[1] == 'run':
        _run(sys.argv[2])
    elif len(sys.argv) == 6 and sys.argv[1] == 'compare':
        sys.exit(_compare(*sys.argv[2:6]))
    else:
        sys.exit(__doc__)
