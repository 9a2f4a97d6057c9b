"""Per-layer A/B of the wide 2-D convolutions: the fp32 pair (lf_wino2d_input_transform + lf_wino_fused_gemm, ops.wide_conv)
against the split-precision pair (lf_wino2d_input_transform_f16x3 + lf_wino_fused2d_f16x3_gemm, ops.wide_conv_f16x3), forward
(He, bias, LeakyReLU) and data gradient, for every layer shape of the released architecture's image decoder at the 128 renders
of a cross-entropy iteration (BASELINE cfg 3) and at the smaller batches of the other estimators (32, 16, 8), and of the
released-width model's decoder (golden g20) at 4 renders.  Both forms in ONE process, calls alternating, each timed with HIP
events around the whole op; medians.  Then one instrumented pass per form splits the time into input transform and GEMM
(ops.KERNEL_TIMER).  Prints one JSON line per (layer, batch, direction) and a summary line: for every (Cin, Cout, H, W) the
smallest measured batch from which on f16x3 wins at every larger measured batch -- the table ops.WIDE2D_F16X3_ROUTE.

    python tools/wide2d_f16x3_ab.py [--reps 15] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (Cin, Cout, H, W, N) of the decoder convolutions (conv1 and conv2 of every block; models.Photographer.decode_features)
RELEASED = [(256, 512, 16, 16), (512, 512, 16, 16), (512, 512, 8, 8), (512, 512, 4, 4), (1024, 512, 8, 8),
            (512, 256, 16, 16), (256, 256, 16, 16), (256, 196, 32, 32), (196, 196, 32, 32), (196, 128, 64, 64),
            (128, 128, 64, 64), (128, 64, 128, 128), (64, 64, 128, 128)]
G20 = [(64, 96, 16, 16), (96, 96, 16, 16), (96, 64, 8, 8), (64, 64, 8, 8), (64, 64, 16, 16), (64, 64, 32, 32)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--out', default=None, help='also write the lines to this file')
    a = ap.parse_args()
    import torch

    from latentfusion_amd import ops
    from latentfusion_amd._lib import LF_EPI_LRELU
    dev = 'cuda'
    lines = []
    wins = {}                                                          # (Cin, Cout, H, W) -> {N: f16x3 faster}
    parts = {'fp32': ('wino2d_input', 'wino2d_fused'), 'f16x3': ('wino2d_input_f16x3', 'wino2d_fused_f16x3')}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        return e0, e1

    for shapes, N in ((RELEASED, 128), (RELEASED, 32), (RELEASED, 16), (RELEASED, 8), (G20, 4)):
        for cin, cout, H, W in shapes:
            g = torch.Generator(device=dev).manual_seed(cin * 7 + cout)
            x = ops.cl(torch.randn(N, cin, H, W, device=dev, generator=g))
            gy = ops.cl(torch.randn(N, cout, H, W, device=dev, generator=g) * 1e-3)
            w = torch.randn(cout, cin, 3, 3, device=dev, generator=g)
            b = torch.randn(cout, device=dev, generator=g) * 0.1
            he = ops.he_constant(w)
            forms = {
                ('fwd', 'fp32'): lambda: ops.wide_conv(x, w, b, he, LF_EPI_LRELU),
                ('fwd', 'f16x3'): lambda: ops.wide_conv_f16x3(x, w, b, he, LF_EPI_LRELU),
                ('bwd', 'fp32'): lambda: ops.wide_conv(gy, w, None, he, 0, transpose=True),
                ('bwd', 'f16x3'): lambda: ops.wide_conv_f16x3(gy, w, None, he, 0, transpose=True),
            }
            for fn in forms.values():                                  # warm-up: packs, code objects, allocator
                fn()
            ev = {k: [] for k in forms}
            for _ in range(a.reps):
                for k, fn in forms.items():
                    ev[k].append(timed(fn))
            torch.cuda.synchronize()
            split = {}
            for k, fn in forms.items():                                # transform / GEMM, one instrumented pass each
                ops.KERNEL_TIMER_TAGS = set(parts[k[1]])
                ops.KERNEL_TIMER = []
                try:
                    for _ in range(5):
                        fn()
                    torch.cuda.synchronize()
                    split[k] = [statistics.median(e0.elapsed_time(e1) for n_, e0, e1 in ops.KERNEL_TIMER if n_ == t)
                                for t in parts[k[1]]]
                finally:
                    ops.KERNEL_TIMER, ops.KERNEL_TIMER_TAGS = None, None
            for d in ('fwd', 'bwd'):
                ms = {m: statistics.median(e0.elapsed_time(e1) for e0, e1 in ev[(d, m)]) for m in ('fp32', 'f16x3')}
                ci, co = (cin, cout) if d == 'fwd' else (cout, cin)
                tiles = N * ((H + 1) // 2) * ((W + 1) // 2)
                macs = 16 * tiles * ci * co
                rec = {'layer': f'{cin}->{cout}', 'dir': d, 'conv': [ci, co, H, W], 'N': N, 'fp32_ms': ms['fp32'],
                       'f16x3_ms': ms['f16x3'], 'speedup': ms['fp32'] / ms['f16x3'],
                       'fp32_transform_gemm_ms': split[(d, 'fp32')], 'f16x3_transform_gemm_ms': split[(d, 'f16x3')],
                       'f16x3_f16_pflops': 3 * 2 * macs / (ms['f16x3'] * 1e-3) / 1e15,
                       'f16x3_v_tb_s': 2 * 16 * tiles * ((ci + 31) // 32 * 32) * 4 / (ms['f16x3'] * 1e-3) / 1e12}
                lines.append(rec)
                print(json.dumps(rec), flush=True)
                wins.setdefault((ci, co, H, W), {})[N] = ms['f16x3'] < ms['fp32']
            del x, gy, w
            torch.cuda.empty_cache()
    route = []
    for key, byn in sorted(wins.items()):
        ns = sorted(byn, reverse=True)
        n_min = None
        for n in ns:                                                   # largest batch first: stop at the first loss
            if not byn[n]:
                break
            n_min = n
        if n_min is not None:
            route.append(list(key) + [n_min])
    summary = {'summary': 'f16x3 faster at every measured batch >= N_min: (Cin, Cout, H, W, N_min)', 'route': route, 'reps': a.reps,
               'device': torch.cuda.get_device_name(0)}
    print(json.dumps(summary))
    if a.out:
        with open(a.out, 'w') as f:
            for r in lines + [summary]:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
