#!/usr/bin/env python
"""A/B of the IBR reprojection (latentfusion_amd.ibr, kernel = 'composed' | 'fused') in ONE process, at
  * the released render size (256^2, C = 3) with V_o = 1 and V_i = 8, 16, and with V_o = 8, V_i = 8 (released architecture
    with seeded weights: the depths and masks the reprojection is fed come from its renderer), and
  * the g23 fixture's own size (tests/golden/g23_ibr_generator.pt).

Per size and arm: `forward_ms`, ibr.reproject_views_batch alone on fixed depths (for 'fused' including the host packing of
the camera records, and `kernel_ms` = ops.ibr_reproject on packed records, the launch alone), and `reprojections_ms`,
LatentFusionModel._render_reprojections as a whole (two renders + reprojection + mask).  HIP events around blocks of calls
sized to 0.2 s or more, after a warm-up and one untimed (cold-start) block per arm; the median over `--blocks` blocks, arms
alternated and run in both orders.  `fused_bytes` is what lf_ibr_reproject_fwd has to move (inputs once, outputs once) and
`kernel_frac_of_hbm` that over kernel_ms over the 8.0 TB/s HBM3E rate.

    python tools/ibr_ab.py [--json profiles/ibr_fused_ab.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from latentfusion_amd import ibr, ops, synth  # noqa: E402
from latentfusion_amd.modules.geometry import Camera  # noqa: E402

HBM_BYTES_PER_S = 8.0e12

ap = argparse.ArgumentParser()
ap.add_argument('--blocks', type=int, default=7)
ap.add_argument('--block-s', type=float, default=0.2)
ap.add_argument('--warmup', type=int, default=5)
ap.add_argument('--json', default=os.path.join(ROOT, 'profiles', 'ibr_fused_ab.json'))
a = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit('ibr_ab.py measures on the GPU: no device found')
DEV = 'cuda'


def block(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def ab(arms):
    """{name: fn} -> {name: {median_ms, min_ms, max_ms, reps_per_block}}"""
    reps = {}
    for k, fn in arms.items():
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        once = block(fn, 3)
        reps[k] = max(3, int(a.block_s * 1e3 / max(once, 1e-3)) + 1)
        block(fn, reps[k])                                   # the cold-start block: run, not counted
    times = {k: [] for k in arms}
    names = list(arms)
    for r in range(a.blocks):
        for k in (names if r % 2 == 0 else names[::-1]):
            times[k].append(block(arms[k], reps[k]))
    return {k: {'median_ms': statistics.median(t), 'min_ms': min(t), 'max_ms': max(t), 'reps_per_block': reps[k]}
            for k, t in times.items()}


def measure(model, z_obj, color_in, cam_in, cam_out):
    """color_in (V_i,C,H,W), flat cameras of one object."""
    with torch.no_grad():
        y_in, _, _ = model.photographer.decode(z_obj, cam_in)
        y_out, _, _ = model.photographer.decode(z_obj, cam_out)
        image, d_in, d_out, mask = color_in.unsqueeze(0).contiguous(), y_in['depth'], y_out['depth'], y_out['mask']
        v_i, c, h, w = color_in.shape
        v_o = len(cam_out)
        rec = ops.pack_ibr_cameras(cam_in, cam_out, batch_size=1)
        fwd = ab({'composed': lambda: ibr.reproject_views_batch(image, d_in, d_out, cam_in, cam_out, kernel='composed'),
                  'fused': lambda: ibr.reproject_views_batch(image, d_in, d_out, cam_in, cam_out, kernel='fused'),
                  'fused_kernel': lambda: ops.ibr_reproject(image, d_in, d_out, rec, mask_out=mask)})

        def whole(kernel):
            model.ibr_kernel = kernel
            return model._render_reprojections(z_obj, color_in, cam_in, cam_out)
        rp = ab({'composed': lambda: whole('composed'), 'fused': lambda: whole('fused')})
        ref, got = whole('composed'), whole('fused')
        model.ibr_kernel = None
    n_bytes = 4 * (v_i * (c + 1) * h * w + 2 * v_o * h * w + v_o * v_i * (c + 1) * h * w)
    kernel_ms = fwd['fused_kernel']['median_ms']
    return {'shape': {'V_o': v_o, 'V_i': v_i, 'C': c, 'H': h, 'W': w},
            'forward_ms': {'composed': fwd['composed'], 'fused': fwd['fused']}, 'kernel_ms': fwd['fused_kernel'],
            'reprojections_ms': rp, 'fused_bytes': n_bytes,
            'kernel_frac_of_hbm': n_bytes / (kernel_ms * 1e-3) / HBM_BYTES_PER_S,
            'forward_fused_over_composed': fwd['fused']['median_ms'] / fwd['composed']['median_ms'],
            'reprojections_fused_over_composed': rp['fused']['median_ms'] / rp['composed']['median_ms'],
            'max_abs_diff_fused_vs_composed': {'image_reproj': float((got[2] - ref[2]).abs().max()),
                                               'depth_reproj': float((got[3] - ref[3]).abs().max())}}


res = {'device': torch.cuda.get_device_name(0), 'hbm_bytes_per_s': HBM_BYTES_PER_S, 'blocks': a.blocks,
       'block_s_at_least': a.block_s, 'sizes': {}}

# released render size
model, _ = synth.build_released_model(DEV, seed=0)
model.freeze()
with torch.no_grad():
    z_obj = model.build_latent_object(synth.make_observation(8, seed=100, device=DEV))
    views = model.preprocess_observation(synth.make_observation(24, seed=101, device=DEV))
for name, v_o, v_i in (('released_256_Vo1_Vi8', 1, 8), ('released_256_Vo1_Vi16', 1, 16), ('released_256_Vo8_Vi8', 8, 8)):
    res['sizes'][name] = measure(model, z_obj, views.color[:v_i], views.camera[0:v_i], views.camera[16:16 + v_o])
    print(name, json.dumps(res['sizes'][name]), flush=True)
del model, z_obj, views
torch.cuda.empty_cache()

# the g23 fixture's own size
from latentfusion_amd.modules.unet import UNet2d  # noqa: E402
from latentfusion_amd.recon import fusion  # noqa: E402
from latentfusion_amd.recon.inference import LatentFusionModel  # noqa: E402
from latentfusion_amd.recon.models import Photographer, Sculptor  # noqa: E402

golden = os.path.join(ROOT, 'tests', 'golden')
g = torch.load(os.path.join(golden, 'g23_ibr_generator.pt'), weights_only=False)
e = torch.load(os.path.join(golden, 'g10_encode_pool_mean.pt'), weights_only=False)


def prod_camera(d):
    return Camera(d['K'].to(DEV), None, d['z_span'], d['viewport'].to(DEV), width=d['width'], height=d['height'],
                  log_quaternion=d['log_q'].to(DEV), translation=d['t'].to(DEV))


model = LatentFusionModel(Sculptor.from_checkpoint(e['sculptor']), fusion.from_checkpoint(e['fuser']),
                          Photographer.from_checkpoint(g['photographer']), g['camera_dist'], DEV,
                          generator=UNet2d.from_checkpoint(g['generator']))
res['sizes']['g23_fixture'] = measure(model, g['z_obj'].to(DEV), g['color_in'].to(DEV), prod_camera(g['cam_in']),
                                      prod_camera(g['cam_out']))
print('g23_fixture', json.dumps(res['sizes']['g23_fixture']), flush=True)

if a.json:
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
