#!/usr/bin/env python
"""Results of the wide Winograd convolutions under a given build of the library, for a byte-for-byte comparison of two builds.

    python tools/wide_conv_dump.py --lib PATH/liblf_hip.so --out DIR      # one process per build: writes DIR/<case>.npy
    python tools/wide_conv_dump.py --compare DIR_A DIR_B [--json OUT]     # sha256 of every array of both runs; exit 1 on a difference

The cases are fixed and seeded: the shapes of test_wide_conv_fused_gemm (fp32 form, 2-D and 3-D), test_wide_f16x3_gpu.SHAPES
(f16x3 3-D), the first, fourth and last of test_wide2d_f16x3_gpu.SHAPES (f16x3 2-D) and the two direct-write shapes of
test_wide_direct_store_gpu (64 -> 512 on 16^3 x 8 and 14^3 x 12, both forms; also depth-inner) -- each as a forward with
bias + LeakyReLU + PixelNorm (y and the norm) and as a data gradient.  profiles/wide_wino_shared_ab.json is the comparison of
the commit that moved the kernels' shared skeleton into csrc/wino_ring.inc against its parent."""
import argparse
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FP32 = [(3, 64, 64, 8, 2), (3, 72, 132, 6, 1), (3, 260, 64, 5, 3), (2, 64, 64, 13, 2), (2, 196, 128, 9, 1), (2, 68, 320, 6, 2),
        (3, 256, 256, 16, 2), (2, 512, 256, 32, 1)]                       # (dims, cin, cout, S, N)
F16X3_3D = [(64, 64, 8, 2), (72, 132, 6, 1), (260, 64, 5, 3), (256, 256, 16, 2)]            # (cin, cout, S, N)
F16X3_2D = [(256, 512, 16, 16, 2), (512, 512, 4, 4, 2), (72, 132, 7, 9, 2)]                 # (cin, cout, H, W, N)
DIRECT = [(64, 512, 16, 8), (64, 512, 14, 12)]                                              # (cin, cout, S, N): no frequency split


def cases():
    """(name, form, cin, cout, spatial, N, depth_inner)"""
    out = [(f'fp32_{d}d_{ci}_{co}_{S}_{N}', 'fp32', ci, co, (S,) * d, N, False) for d, ci, co, S, N in FP32]
    out += [(f'f16x3_3d_{ci}_{co}_{S}_{N}', 'f16x3', ci, co, (S,) * 3, N, False) for ci, co, S, N in F16X3_3D]
    out += [(f'f16x3_2d_{ci}_{co}_{H}x{W}_{N}', 'f16x3', ci, co, (H, W), N, False) for ci, co, H, W, N in F16X3_2D]
    for ci, co, S, N in DIRECT:
        for form in ('fp32', 'f16x3'):
            for di in (False, True):
                out.append((f'direct{"_di" if di else ""}_{form}_{ci}_{co}_{S}_{N}', form, ci, co, (S,) * 3, N, di))
    return out


def dump(lib, out):
    import numpy as np
    import torch
    from latentfusion_amd import _lib
    _lib.LIB_PATH = os.path.abspath(lib)
    from latentfusion_amd import ops
    from latentfusion_amd._lib import LF_EPI_LRELU, LF_EPI_PIXELNORM
    os.makedirs(out, exist_ok=True)
    for i, (name, form, cin, cout, sp, N, di) in enumerate(cases()):
        g = torch.Generator().manual_seed(1000 + i)
        x = ops.cl(torch.randn((N, cin) + sp, generator=g).cuda())
        w = torch.randn((cout, cin) + (3,) * len(sp), generator=g).cuda()
        b = (torch.randn(cout, generator=g) * 0.1).cuda()
        gin = ops.cl(torch.randn((N, cin) + sp, generator=g).cuda())
        wt = torch.randn((cin, cout) + (3,) * len(sp), generator=g).cuda()          # data gradient with the forward's grid: cin -> cout
        conv = ops.wide_conv if form == 'fp32' else ops.wide_conv_f16x3
        kw = dict(depth_inner=True) if di else {}
        y, nrm = conv(x, w, b, ops.he_constant(w), LF_EPI_LRELU | LF_EPI_PIXELNORM, **kw)
        gx, _ = conv(gin, wt, None, ops.he_constant(wt), 0, transpose=True, **kw)
        gx2, _ = conv(ops.cl(y.permute(0, 4, 3, 1, 2)) if di else y, w, None, ops.he_constant(w), 0, transpose=True)   # cout -> cin
        torch.cuda.synchronize()
        for tag, t in (('y', y), ('norm', nrm), ('gx', gx), ('gx_back', gx2)):
            np.save(os.path.join(out, f'{name}.{tag}.npy'), t.cpu().numpy())
        print(name, tuple(y.shape), flush=True)


def compare(a, b, out_json):
    names = sorted(f for f in os.listdir(a) if f.endswith('.npy'))
    rows, bad = [], []
    for f in names:
        ha = hashlib.sha256(open(os.path.join(a, f), 'rb').read()).hexdigest()
        pb = os.path.join(b, f)
        hb = hashlib.sha256(open(pb, 'rb').read()).hexdigest() if os.path.exists(pb) else None
        rows.append({'file': f, 'sha256_a': ha, 'sha256_b': hb, 'identical': ha == hb})
        if ha != hb:
            bad.append(f)
    missing = sorted(set(f for f in os.listdir(b) if f.endswith('.npy')) - set(names))
    res = {'a': os.path.basename(os.path.normpath(a)), 'b': os.path.basename(os.path.normpath(b)), 'arrays': len(rows), 'identical': len(rows) - len(bad), 'only_in_b': missing, 'files': rows}
    if out_json:
        with open(out_json, 'w') as f:
            json.dump(res, f, indent=1)
    print(f'{len(rows)} arrays, {len(bad)} differ' + (': ' + ', '.join(bad) if bad else '') + (f'; only in b: {missing}' if missing else ''))
    return 1 if bad or missing or not rows else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--lib')
    ap.add_argument('--out')
    ap.add_argument('--compare', nargs=2, metavar=('DIR_A', 'DIR_B'))
    ap.add_argument('--json')
    a = ap.parse_args()
    if a.compare:
        return compare(a.compare[0], a.compare[1], a.json)
    if not (a.lib and a.out):
        ap.error('--lib and --out, or --compare')
    dump(a.lib, a.out)
    return 0


if __name__ == '__main__':
    sys.exit(main())
