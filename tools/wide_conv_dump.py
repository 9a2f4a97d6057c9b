#!/usr/bin/env python
"""Results of the wide Winograd convolutions under a given build of the library, for a byte-for-byte comparison of two builds.

    python tools/wide_conv_dump.py --lib PATH/liblf_hip.so --out DIR      # one process per build: writes DIR/<case>.npy
    python tools/wide_conv_dump.py --compare DIR_A DIR_B [--json OUT]     # sha256 of every array of both runs; exit 1 on a difference
    python tools/wide_conv_dump.py --cases ring --lib ... --out DIR       # the second case list: the ring 16 -> 16 convolutions

The cases are fixed and seeded: the shapes of test_wide_conv_fused_gemm (fp32 form, 2-D and 3-D), test_wide_f16x3_gpu.SHAPES
(f16x3 3-D), the first, fourth and last of test_wide2d_f16x3_gpu.SHAPES (f16x3 2-D) and the two direct-write shapes of
test_wide_direct_store_gpu (64 -> 512 on 16^3 x 8 and 14^3 x 12, both forms; also depth-inner) -- each as a forward with
bias + LeakyReLU + PixelNorm (y and the norm) and as a data gradient.  profiles/wide_wino_shared_ab.json is the comparison of
the commit that moved the kernels' shared skeleton into csrc/wino_ring.inc against its parent.

--cases ring: the ring convolutions of csrc/conv_split.hip and csrc/conv_gru.hip (profiles/ring_shared_ab.json: the commit that
moved their tile walk into csrc/ring_walk.inc against its parent) -- lf_conv3d_c16_split as forward, plain data gradient and data
gradient with the previous layer's epilogue + amax in / out; the 12 (addend, storage) forms of lf_conv3d_c16_ring_bf16_io; the
20 instantiated forms of lf_conv3d_c16_ring_multi and lf_conv3d_c16_ring_blend; each at a small ragged shape and at a shape
that gives every workgroup several tiles (the split form: test_split_conv3d_matches_fp64's; the bf16 forms: the walk shape of
test_tile_walk_of_three_or_more_tiles_per_workgroup, from the device's CU count).  Outputs start as zeros."""
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


# lf_conv3d_c16_ring_multi: (x stored as bf16, LF_RING_EX_*, per group (y stored as bf16, addend: None / 'f32' / 'bf16' /
# 'self' = in place over the output, round)) -- one entry per instantiated ring_multi_kernel<NG, IN16, EX, FL>
RING_MULTI = [
    (True, 'NONE', [(True, 'bf16', False), (False, 'f32', False)]), (False, 'RH', [(True, 'bf16', False), (True, 'bf16', False)]),
    (True, 'ABWD', [(True, 'self', True), (True, None, True)]),
    (True, 'NONE', [(False, 'f32', False)]), (True, 'NONE', [(True, 'f32', False)]), (True, 'NONE', [(True, 'bf16', False)]),
    (True, 'NONE', [(True, None, True)]), (True, 'NONE', [(False, 'bf16', False)]),
    (False, 'NONE', [(True, 'bf16', False)]), (False, 'NONE', [(True, 'f32', False)]),
    (False, 'RH', [(True, 'bf16', False)]), (False, 'RH', [(True, 'f32', False)]), (True, 'RH', [(True, 'bf16', False)]),
    (True, 'BLEND', [(True, 'bf16', False)]), (True, 'BLEND', [(True, 'f32', False)]),
    (True, 'ABWD', [(True, 'self', True)]), (True, 'ABWD', [(False, 'bf16', True)]),
    (True, 'PREV', [(True, None, True)]), (True, 'BLOCK', [(True, None, True)]), (False, 'BLOCK', [(True, None, True)]),
]


def dump_ring(lib, out):
    import numpy as np
    import torch
    from latentfusion_amd import _lib
    _lib.LIB_PATH = os.path.abspath(lib)
    from latentfusion_amd import ops, ops_train
    from latentfusion_amd._lib import LF_EPI_LRELU, LF_EPI_PIXELNORM
    os.makedirs(out, exist_ok=True)
    cl3 = torch.channels_last_3d
    flags = LF_EPI_LRELU | LF_EPI_PIXELNORM
    g = torch.Generator().manual_seed(2000)

    def vol(shape, b16=False, scale=1.0):
        v = (torch.randn(shape, generator=g) * scale).cuda().contiguous(memory_format=cl3)
        return v.to(torch.bfloat16) if b16 else v

    def save(name, **arrays):
        torch.cuda.synchronize()
        for tag, t in arrays.items():
            if t is not None:
                np.save(os.path.join(out, f'{name}.{tag}.npy'), (t.view(torch.int16) if t.dtype == torch.bfloat16 else t).cpu().numpy())
        print(name, flush=True)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    walk = (1, 16, 9, 37, 16 * (4 * cus // 25 + 1) - 13)
    w = [torch.randn(16, 16, 3, 3, 3, generator=g).cuda() for _ in range(2)]
    bias = (torch.randn(16, generator=g) * 0.1).cuda()
    he = ops.he_constant(w[0])
    for shape in ((1, 16, 5, 7, 9), (2, 16, 36, 64, 64)):
        tag = 'split_' + 'x'.join(map(str, shape))
        x, gin = vol(shape), vol(shape)
        sp, spt = ops.pack_conv3d_c16_split(w[0]), ops.pack_conv3d_c16_split(w[0], transpose=True)
        y, nrm = ops.conv3d_c16_split(x, sp, bias, he, flags)
        gx, _ = ops.conv3d_c16_split(gin, spt, None, he, 0)
        tiny = gin * 3e-7
        am_in, am_out = ops.amax_buffer(tiny.abs().max(), 'cuda'), ops.amax_buffer(None, 'cuda')
        gp, _ = ops.conv3d_c16_split(tiny, spt, None, he, 0, prev=(y, nrm, flags), amax_in=am_in, amax_out=am_out)
        save(tag, y=y, norm=nrm, gx=gx, gx_prev=gp, amax=am_out)
    bpk = torch.stack([ops.pack_conv3d_c16_ring_bf16(t) for t in w]).contiguous()
    for shape in ((1, 16, 7, 35, 50), walk):
        tag = 'bf16io_' + 'x'.join(map(str, shape))
        x, add = ops.round_bf16(vol(shape)), ops.round_bf16(vol(shape))
        for io in range(4):
            xi = x.to(torch.bfloat16) if io & 1 else x
            y, nrm = ops.conv3d_c16_ring_bf16_io(xi, bpk[0], bias, he, flags, 1, out_bf16=bool(io & 2))
            save(f'{tag}_fwd_io{io}', y=y, norm=nrm)
        for io in range(8):
            xi = x.to(torch.bfloat16) if io & 1 else x
            y, _ = ops.conv3d_c16_ring_bf16_io(xi, bpk[0], None, he, 0, 0, addend=add.to(torch.bfloat16) if io & 4 else add, out_bf16=bool(io & 2))
            save(f'{tag}_add_io{io}', y=y)
    L = _lib.lib()
    for shape in ((2, 16, 5, 11, 19), walk):
        N, _, D, H, W = shape
        tag = 'multi_' + 'x'.join(map(str, shape))
        zeros = lambda b16: torch.zeros(shape, device='cuda', dtype=torch.bfloat16 if b16 else torch.float32).contiguous(memory_format=cl3)   # noqa: E731
        act = torch.nn.functional.leaky_relu(vol(shape), 0.2)
        anrm = torch.sqrt((act * act).mean(dim=1) + 1e-8).reshape(-1).contiguous()
        act = (act / anrm.view(N, 1, D, H, W)).to(torch.bfloat16).contiguous(memory_format=cl3)
        for k, (x16, ex, groups) in enumerate(RING_MULTI):
            x = vol(shape, x16)
            outs, res = [], {}
            for q, (o16, add, rnd) in enumerate(groups):
                y = vol(shape, True, 2.0) if add == 'self' else zeros(o16)
                a = y if add == 'self' else (None if add is None else vol(shape, add == 'bf16'))
                outs.append((y, a, rnd))
                res[f'y{q}'] = y
            kw = {}
            if ex == 'RH':
                kw = dict(e0=vol(shape) if x16 else None, o2=zeros(True))
            elif ex == 'BLEND':
                kw = dict(e0=vol(shape), e1=vol(shape, True, 2.0), o2=zeros(False))
            elif ex == 'ABWD':
                kw = dict(e0=vol(shape), e1=vol(shape), o2=zeros(False))
            elif ex == 'PREV':
                kw = dict(e0=act, e1=anrm, o2=torch.zeros(16 * 1025, device='cuda'))
            elif ex == 'BLOCK':
                kw = dict(e0=bias, o2=torch.zeros(N * D * H * W, device='cuda'))
            ops_train.ring_multi(x, bpk[:len(groups)].contiguous(), he, outs, extra=getattr(_lib, 'LF_RING_EX_' + ex), **kw)
            save(f'{tag}_{k:02d}_{ex.lower()}', o2=kw.get('o2'), **res)
        rh, cand, h, upre = vol(shape, True), vol(shape, True), vol(shape), vol(shape, True, 2.0)
        hn, h16 = zeros(False), zeros(True)
        _lib.check(L.lf_conv3d_c16_ring_blend(rh.data_ptr(), bpk[0].data_ptr(), cand.data_ptr(), cand.data_ptr(), h.data_ptr(), upre.data_ptr(),
                                              hn.data_ptr(), h16.data_ptr(), N, D, H, W, he, torch.cuda.current_stream().cuda_stream), 'blend')
        save(f'{tag}_blend', cand=cand, h_new=hn, h_new_bf16=h16)


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
    ap.add_argument('--cases', choices=('wide', 'ring'), default='wide', help='which fixed case list to dump')
    ap.add_argument('--compare', nargs=2, metavar=('DIR_A', 'DIR_B'))
    ap.add_argument('--json')
    a = ap.parse_args()
    if a.compare:
        return compare(a.compare[0], a.compare[1], a.json)
    if not (a.lib and a.out):
        ap.error('--lib and --out, or --compare')
    (dump_ring if a.cases == 'ring' else dump)(a.lib, a.out)
    return 0


if __name__ == '__main__':
    sys.exit(main())
