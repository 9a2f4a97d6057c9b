#!/usr/bin/env python
"""A/B of the ranking path's factor projection at the released shape (M = 128 * 16^2 rows, K = 16 * 256, Cout = 256), in ONE
process:

  library : torch.addmm (library GEMM) + leaky_relu_ + lf_pixelnorm_fwd, exactly as RenderLoopEngine._factor_fwd issues them
  mfma    : lf_rows_gemm_epi (one launch)

HIP events around blocks of `--reps` calls (0.1 s or more each) after a warm-up and one untimed block per arm, the median
over `--blocks` blocks, the two arms alternated and run in both orders (A B then B A per round).  Reported per arm: median / min / max ms per call, and the fraction of the
fp32-MFMA peak (2 M K Cout FLOP over 157.3 TFLOP/s).  With --cfg3 the cross_entropy_linemod preset on the released
architecture (128 renders per iteration, as bench.py's cfg 3 block runs it) is timed under both settings as well.

    python tools/proj_rows_ab.py [--cfg3] [--json profiles/proj_rows_gemm_ab.json]
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
from latentfusion_amd import _lib, ops  # noqa: E402
from latentfusion_amd._lib import LF_EPI_LRELU, LF_EPI_PIXELNORM, check  # noqa: E402

PEAK_F32_MFMA = 157.3e12

ap = argparse.ArgumentParser()
ap.add_argument('--renders', type=int, default=128)
ap.add_argument('--size', type=int, default=16)
ap.add_argument('--channels', type=int, default=256)
ap.add_argument('--cout', type=int, default=256)
ap.add_argument('--reps', type=int, default=200)
ap.add_argument('--blocks', type=int, default=9)
ap.add_argument('--warmup', type=int, default=200)
ap.add_argument('--cfg3', action='store_true')
ap.add_argument('--cfg3-iters', type=int, default=6)
ap.add_argument('--json', default=os.path.join(ROOT, 'profiles', 'proj_rows_gemm_ab.json'))
a = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit('proj_rows_ab.py measures on the GPU: no device found')
DEV = 'cuda'
L = _lib.lib()
S, C, cout = a.size, a.channels, a.cout
M, K = a.renders * S * S, S * C
flags = LF_EPI_LRELU | LF_EPI_PIXELNORM
g = torch.Generator().manual_seed(0)
x2 = torch.randn(M, K, generator=g).to(DEV)
w = torch.randn(cout, K, generator=g).to(DEV)
pb = (0.1 * torch.randn(cout, generator=g)).to(DEV)
phe = (2.0 / K) ** 0.5
rows_t = w.t().contiguous()                    # [K][cout], engine.proj_rows_t
wpack = ops.pack_rows_gemm(w)
st = torch.cuda.current_stream().cuda_stream


def library():
    rows = torch.addmm(pb, x2, rows_t, alpha=phe)
    torch.nn.functional.leaky_relu_(rows, ops.SLOPE)
    pnorm = torch.empty(M, device=DEV, dtype=torch.float32)
    check(L.lf_pixelnorm_fwd(rows.data_ptr(), rows.data_ptr(), pnorm.data_ptr(), M, cout, ops.PN_EPS, st), 'lf_pixelnorm_fwd')
    return rows, pnorm


def mfma():
    return ops.rows_gemm_epilogue(x2, wpack, pb, phe, cout, flags)


def block(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / a.reps


arms = {'library': library, 'mfma': mfma}
for fn in arms.values():
    for _ in range(a.warmup):
        fn()
torch.cuda.synchronize()
for fn in arms.values():                       # one untimed block each: the clocks settle under the load they will be timed at
    block(fn)
(yl, nl), (ym, nm) = library(), mfma()
torch.cuda.synchronize()
agree = {'y_max_abs_diff': float((yl - ym).abs().max()), 'norm_max_rel_diff': float(((nl - nm).abs() / nl).max())}
# both arms against the fp64 formula on every 128th row
rows = torch.arange(0, M, 128, device=DEV)
y64 = torch.nn.functional.leaky_relu(torch.mm(x2[rows].double(), w.double().t()) * phe + pb.double(), ops.SLOPE)
y64 = y64 / torch.sqrt(torch.mean(y64 ** 2, dim=1, keepdim=True) + ops.PN_EPS)
agree['rows_checked_against_fp64'] = int(rows.numel())
agree['library_max_abs_err_vs_fp64'] = float((yl[rows].double() - y64).abs().max())
agree['mfma_max_abs_err_vs_fp64'] = float((ym[rows].double() - y64).abs().max())
del y64
del yl, nl, ym, nm
times = {k: [] for k in arms}
for r in range(a.blocks):
    for k in (('library', 'mfma') if r % 2 == 0 else ('mfma', 'library')):
        times[k].append(block(arms[k]))
flop = 2.0 * M * K * cout
floor_ms = flop / PEAK_F32_MFMA * 1e3
res = {'shape': {'M': M, 'K': K, 'Cout': cout}, 'reps_per_block': a.reps, 'blocks': a.blocks,
       'flop': flop, 'fp32_mfma_peak_tflops': PEAK_F32_MFMA / 1e12, 'floor_ms': floor_ms, 'outputs_agree': agree,
       'device': torch.cuda.get_device_name(0)}
for k, t in times.items():
    med = statistics.median(t)
    res[k] = {'median_ms': med, 'min_ms': min(t), 'max_ms': max(t), 'blocks_ms': t, 'frac_of_fp32_mfma_peak': floor_ms / med}
res['mfma_over_library'] = res['mfma']['median_ms'] / res['library']['median_ms']

if a.cfg3:
    import numpy as np
    from latentfusion_amd import synth
    from latentfusion_amd.modules.geometry import Camera
    from latentfusion_amd.observation import Observation
    from latentfusion_amd.pose import estimation
    model, _ = synth.build_released_model(DEV, seed=0)
    model.freeze()
    ref = synth.make_observation(8, seed=100, device=DEV)
    td = synth.make_observation_data(1, seed=200)
    target = Observation(td['color'], td['depth'], td['mask'], Camera(td['intrinsic'], td['extrinsic'])).to(DEV)
    z_obj = model.build_latent_object(ref)
    cfg = estimation._load_toml(os.path.join(ROOT, 'configs', 'cross_entropy_linemod.toml'))
    cfg['args']['num_iters'] = a.cfg3_iters
    runs = {'library': [], 'mfma': []}
    for r in range(4):                                             # round 0 warms both settings up
        for k in (('library', 'mfma') if r % 2 == 0 else ('mfma', 'library')):
            est = estimation.load_from_config(cfg, model, proj_kernel=k)
            torch.manual_seed(300)
            np.random.seed(300)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            est.estimate(z_obj, target, camera=target.camera)
            torch.cuda.synchronize()
            if r > 0:
                runs[k].append(a.cfg3_iters / (time.perf_counter() - t0))
            assert est.last_scored_on_engine
    res['cfg3_iters_per_s'] = {k: {'median': statistics.median(v), 'min': min(v), 'max': max(v), 'runs': v} for k, v in runs.items()}
    res['cfg3_iters_per_s']['renders_per_iteration'] = cfg['args']['num_samples']

print(json.dumps(res))
if a.json:
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
