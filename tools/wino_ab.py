#!/usr/bin/env python
"""A/B timing of several builds of the Winograd conv kernel in ONE process (box-to-box variance is ~3 %, more than
most of the deltas being chased):

    hipcc -x hip --offload-arch=gfx950 -O3 -std=c++17 -fPIC -fno-gpu-rdc -shared -Ilatentfusion_amd/csrc \
          latentfusion_amd/csrc/conv_wino.hip -o scratch/a.so        (one per variant)
    python tools/wino_ab.py scratch/a.so scratch/b.so ...

Each variant is checked against the first one (max |diff| of forward and fused-backward outputs) and timed
round-robin: forward (bias + LeakyReLU + PixelNorm), data-gradient fused with the previous layer's backward and the
forward with the factor projection riding on it (lf_conv3d_c16_wino_projfwd).  A whole liblf_hip.so works as a variant
too (the parent commit's against this one's), and `path@0` / `path@1` selects the scalar / packed transforms of that
library through lf_set_tuning(7, .) before each of its calls; `path@8=0` / `path@8=1` (any `key=value`, comma-separated) the
generic kernels / the compile-time epilogue forms.  The plain data gradient (no previous layer) is timed as well.
One warm-up round is run and discarded.  `--json FILE` (first argument) also writes every round's time per variant and call, with median and min-to-max spread.
Ablation variants are builds with -DWINO_ABL=bits; every bit is described at the top of csrc/wino16_math.h."""
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from latentfusion_amd import ops  # noqa: E402
from latentfusion_amd._lib import LF_EPI_LRELU, LF_EPI_PIXELNORM  # noqa: E402

JSON = None
if sys.argv[1:2] == ['--json']:
    JSON = sys.argv[2]
    del sys.argv[1:3]
P = ctypes.c_void_p
S, N, ROUNDS = 128, 8, 7
g = torch.Generator().manual_seed(0)
x = ops.cl(torch.randn(N, 16, S, S, S, generator=g).cuda())
w = torch.randn(16, 16, 3, 3, 3, generator=g).cuda()
b = (torch.randn(16, generator=g) * 0.1).cuda()
he = ops.he_constant(w)
up, upt = ops.pack_conv3d_c16_wino(w), ops.pack_conv3d_c16_wino(w, transpose=True)
flags = LF_EPI_LRELU | LF_EPI_PIXELNORM
st = torch.cuda.current_stream().cuda_stream


wp = torch.randn(16, 16 * S, generator=g).cuda()
wA, phe = ops.pack_wino_proj(wp), ops.he_constant(wp.view(16, 16 * S, 1, 1))
PJ = []                                                       # per variant: the projfwd call


def bind(spec):
    path, _, pack = spec.partition('@')
    L = ctypes.CDLL(os.path.abspath(path))
    f0 = L.lf_conv3d_c16_wino
    f0.restype = ctypes.c_int
    f0.argtypes = [P, P, P, P, P] + [ctypes.c_int] * 4 + [ctypes.c_float, ctypes.c_uint, ctypes.c_float, ctypes.c_float, P, P, ctypes.c_uint, P, P]
    p0 = L.lf_conv3d_c16_wino_projfwd
    p0.restype = ctypes.c_int
    p0.argtypes = [P, P, P, P, P] + [ctypes.c_int] * 4 + [ctypes.c_float, ctypes.c_uint, ctypes.c_float, ctypes.c_float, P, P, P, P,
                                                          ctypes.c_float, ctypes.c_uint, P]

    def select():
        if pack:
            for kv in pack.split(','):
                k, _, v = kv.rpartition('=')
                L.lf_set_tuning(int(k or 7), int(v))

    def f(*a):
        select()
        return f0(*a)

    def pj(y, nrm, zp, pn):
        select()
        return p0(x.data_ptr(), up.data_ptr(), b.data_ptr(), y.data_ptr(), nrm.data_ptr(), N, S, S, S, he, flags, 0.2, 1e-8,
                  wA.data_ptr(), None, zp.data_ptr(), pn.data_ptr(), phe, flags, st)
    PJ.append(pj)
    return f


def run(f, y, nrm, gout):
    assert f(x.data_ptr(), up.data_ptr(), b.data_ptr(), y.data_ptr(), nrm.data_ptr(), N, S, S, S, he, flags, 0.2, 1e-8,
             None, None, 0, None, st) == 0
    return lambda plain=False: f(x.data_ptr(), upt.data_ptr(), None, gout.data_ptr(), None, N, S, S, S, he, 0, 0.2, 1e-8,
                                 None if plain else y.data_ptr(), None if plain else nrm.data_ptr(), 0 if plain else flags, None, st)


# `path:fwd` / `path:bwd` restricts a variant to one of the two calls (builds with a hard-wired epilogue)
specs = [(a.split(':') + ['both'])[:2] for a in sys.argv[1:]]
sys.argv[1:] = [a for a, _ in specs]
only = [o for _, o in specs]
fs = [bind(p) for p in sys.argv[1:]]
zps = []
outs = []
for i, f in enumerate(fs):
    y, nrm, go = torch.empty_like(x), torch.empty(N * S ** 3, device='cuda'), torch.empty_like(x)
    bw = run(fs[0] if only[i] == 'bwd' else f, y, nrm, go)
    if only[i] != 'fwd':
        assert bw() == 0
    else:
        go.copy_(outs[0][2])
    zp, pn = ops.empty_cl((N, 16, S, S), 'cuda'), torch.empty(N * S * S, device='cuda')
    assert PJ[i](torch.empty_like(x), torch.empty_like(nrm), zp, pn) == 0
    torch.cuda.synchronize()
    outs.append((y, nrm, go, bw))
    zps.append((zp, pn))
for i, p in enumerate(sys.argv[1:]):
    print(f'{p}: fwd diff vs first {(outs[i][0] - outs[0][0]).abs().max().item():.2e}, bwd diff {(outs[i][2] - outs[0][2]).abs().max().item():.2e}, '
          f'projfwd zp diff {(zps[i][0] - zps[0][0]).abs().max().item():.2e}; bit-identical to first: '
          f'{torch.equal(outs[i][0], outs[0][0]) and torch.equal(outs[i][2], outs[0][2]) and torch.equal(zps[i][0], zps[0][0])}')
tf = [[] for _ in fs]
tb = [[] for _ in fs]
tp = [[] for _ in fs]
tg = [[] for _ in fs]
for r in range(ROUNDS + 1):
    for i, f in enumerate(fs):
        y, nrm, go, bw = outs[i]
        for which, acc in ((0, tf), (1, tb), (2, tg)):
            if only[i] == ('bwd', 'fwd', 'fwd')[which]:
                acc[i].append(float('nan'))
                continue
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(5):
                if which == 0:
                    f(x.data_ptr(), up.data_ptr(), b.data_ptr(), y.data_ptr(), nrm.data_ptr(), N, S, S, S, he, flags, 0.2, 1e-8, None, None, 0, None, st)
                else:
                    bw(which == 2)
            e1.record()
            torch.cuda.synchronize()
            acc[i].append(e0.elapsed_time(e1) / 5)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(5):
            PJ[i](y, nrm, *zps[i])
        e1.record()
        torch.cuda.synchronize()
        tp[i].append(e0.elapsed_time(e1) / 5)
for acc in (tf, tb, tp, tg):                                  # round 0 is the warm-up (clocks still ramping): discarded
    for i in range(len(fs)):
        del acc[i][0]
for i, p in enumerate(sys.argv[1:]):
    a, c, d, e = sorted(tf[i]), sorted(tb[i]), sorted(tp[i]), sorted(tg[i])
    print(f'{p}: fwd median {a[len(a) // 2]:.4f} ms (min {a[0]:.4f}), bwd+prev median {c[len(c) // 2]:.4f} ms (min {c[0]:.4f}), '
          f'bwd plain median {e[len(e) // 2]:.4f} ms (min {e[0]:.4f}), projfwd median {d[len(d) // 2]:.4f} ms (min {d[0]:.4f})')
if JSON:
    rec = {'shape': [N, 16, S, S, S], 'rounds': ROUNDS, 'launches_per_round': 5, 'unit': 'ms', 'variants': {}}
    for i, p in enumerate(sys.argv[1:]):
        rec['variants'][p] = {}
        for name, acc in (('fwd', tf), ('dgrad_prev', tb), ('dgrad_plain', tg), ('projfwd', tp)):
            v = sorted(acc[i])
            rec['variants'][p][name] = {'median': round(v[len(v) // 2], 4), 'spread': round(v[-1] - v[0], 4),
                                       'rounds': [round(t, 4) for t in acc[i]]}
    with open(JSON, 'w') as fh:
        json.dump(rec, fh, indent=1)
        fh.write('\n')
