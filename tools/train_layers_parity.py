#!/usr/bin/env python
"""Outputs, gradients and launch counts of the training step's autograd layers over their configurations, for comparing two
checkouts of this repository bit for bit (a refactor of ops_train.py / gru_train.py must change none of them).

    python tools/train_layers_parity.py run OUT_DIR              every configuration: OUT_DIR/<name>.<first|second>.<array>.npy (output,
                                                                 every input and parameter gradient) of a first and of a second call,
                                                                 OUT_DIR/launches.json = {name: {entry point: launches}} counted by
                                                                 _lib.BYTE_LOG around the second call
    python tools/train_layers_parity.py compare A B C OUT.json   A, B: two runs of the parent, C: one run of the change

Configurations: fusion.GRUFuser(16) (the fused ConvGRU recurrence: fp32, autocast on the step recurrence, autocast on the ring
recurrence; 1, 2, 3, 5 views; inside and outside the bf16 weight-gradient domain; fp32 / bf16 views; everything trainable, gates
frozen, views without gradient; WGRAD_STREAM on / off; GRU_WGRAD_CHUNK 16 / 2 / 0) and the 16 -> 16 layers under the storage policy
(a chained pair of 3x3x3 layers, with and without a second consumer of the first one's output, and a 1x1x1 layer).

Only public surface is used (fusion.GRUFuser, ops.conv3x3 / conv1x1 / autocast, the module switches of ops_train), so the same
file runs against either checkout: put it beside the checkout's `latentfusion_amd` (it imports the package of the tree it lies in)."""
import itertools
import json
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
IN_DOMAIN, BELOW_DOMAIN = (11, 20, 41), (5, 12, 20)        # 9020 / 1200 voxels: the bf16 weight-gradient kernel starts at 8192


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def _run(out):
    import torch
    sys.path.insert(0, ROOT)
    from latentfusion_amd import _lib, ops, ops_train
    from latentfusion_amd.recon import fusion

    os.makedirs(out, exist_ok=True)
    launches = {}

    def record(name, call):
        """Two calls: the first also builds the cached weight packs, the second is the steady state that is counted."""
        for tag in ('first', 'second'):
            if tag == 'second':
                _lib.BYTE_LOG = {}
            try:
                arrays = call()
                torch.cuda.synchronize()
            finally:
                if tag == 'second':
                    launches[name] = {k: v[0] for k, v in sorted(_lib.BYTE_LOG.items())}
                    _lib.BYTE_LOG = None
            for k, t in arrays.items():
                if t is not None:
                    np.save(os.path.join(out, f'{name}.{tag}.{k}.npy'), t.detach().float().cpu().numpy())
        print('done', name, flush=True)

    def switches(**kw):
        for k, v in kw.items():
            assert hasattr(ops_train, k), k
            setattr(ops_train, k, v)
    defaults = {k: getattr(ops_train, k) for k in ('GRU_RING', 'WGRAD_STREAM', 'GRU_WGRAD_CHUNK')}

    # ---- the fused ConvGRU recurrence through fusion.GRUFuser(16) ----
    def gru_case(mode, V, vol, store, train, stream, chunk):
        name = f'gru.{mode}.V{V}.{"x".join(map(str, vol))}.{store}.{train}.stream{int(stream)}.chunk{chunk}'
        ac = mode != 'fp32'
        torch.manual_seed(_seed('gru-weights'))
        fu = fusion.GRUFuser(16).to(DEV)
        with torch.no_grad():
            for gate in (fu.gru.update_gate, fu.gru.reset_gate, fu.gru.out_gate):
                gate.bias.normal_(0.0, 0.3)
        if train == 'frozen':
            for p in fu.parameters():
                p.requires_grad_(False)
        g = torch.Generator().manual_seed(_seed('gru', V, vol))
        z0 = torch.randn(1, V, 16, *vol, generator=g).to(DEV)
        gout = torch.randn(1, 1, 16, *vol, generator=g).to(DEV)
        if store == 'bf16':
            z0 = z0.to(torch.bfloat16)
        params = dict(fu.named_parameters())

        def call():
            switches(GRU_RING=mode == 'ac_ring', WGRAD_STREAM=stream, GRU_WGRAD_CHUNK=chunk)
            try:
                z = z0.clone().requires_grad_(train != 'z_nograd')
                for p in params.values():
                    p.grad = None
                with ops.autocast(ac):
                    y, _ = fu(z, None, None, None)
                res = {'out': y}
                if z.requires_grad or train != 'frozen':
                    (y * gout).sum().backward()
                res['gz'] = z.grad
                res.update({'g.' + k: p.grad for k, p in params.items()})
                return res
            finally:
                switches(**defaults)
        record(name, call)

    for mode in ('fp32', 'ac_step', 'ac_ring'):
        vols = (IN_DOMAIN,) if mode == 'ac_ring' else (IN_DOMAIN, BELOW_DOMAIN)
        stores = ('fp32',) if mode == 'fp32' else ('fp32', 'bf16')
        for V, vol, store, train, stream in itertools.product((1, 2, 3, 5), vols, stores, ('all', 'frozen', 'z_nograd'), (True, False)):
            gru_case(mode, V, vol, store, train, stream, 16)
    for chunk, store, stream in itertools.product((2, 0), ('fp32', 'bf16'), (True, False)):
        gru_case('ac_ring', 5, IN_DOMAIN, store, 'all', stream, chunk)

    # ---- the 16 -> 16 layers under the storage policy: a Block-style chained pair of 3x3x3 layers, a 1x1x1 layer ----
    def params16(key, k, bias):
        g = torch.Generator().manual_seed(_seed(key))
        w = torch.randn(16, 16, k, k, k, generator=g).to(DEV).requires_grad_(True)
        b = (torch.randn(16, generator=g) * 0.3).to(DEV).requires_grad_(True) if bias else None
        return w, b

    def conv_case(kind, store, bias, stream):
        name = f'conv16.{kind}.{store}.bias{int(bias)}.stream{int(stream)}'
        g = torch.Generator().manual_seed(_seed('conv16', kind))
        shape = (2, 16) + IN_DOMAIN
        x0 = ops.cl(torch.randn(shape, generator=g).to(DEV))
        gy = ops.cl(torch.randn(shape, generator=g).to(DEV)).to(torch.bfloat16)
        gy1 = ops.cl(torch.randn(shape, generator=g).to(DEV)).to(torch.bfloat16)
        if store == 'bf16':
            x0 = x0.to(torch.bfloat16)
        (w1, b1), (w2, b2) = params16('w1', 1 if kind.startswith('pw') else 3, bias), params16('w2', 3, bias)

        def call():
            switches(WGRAD_STREAM=stream)
            try:
                x = x0.clone().requires_grad_(True)
                for p in (w1, b1, w2, b2):
                    if p is not None:
                        p.grad = None
                with ops.autocast(True):
                    if kind.startswith('pw'):
                        y = ops.conv1x1(x, w1, b1, lrelu=kind == 'pw_lrelu')
                        y.backward(gy)
                        return {'out': y, 'gx': x.grad, 'gw1': w1.grad, 'gb1': b1.grad if bias else None}
                    y1 = ops.conv3x3(x, w1, b1)
                    y2 = ops.conv3x3(y1, w2, b2, chain=True)
                    if kind == 'pair_second_consumer':
                        torch.autograd.backward((y2, y1), (gy, gy1))
                    else:
                        y2.backward(gy)
                return {'out': y2, 'mid': y1, 'gx': x.grad, 'gw1': w1.grad, 'gw2': w2.grad,
                        'gb1': b1.grad if bias else None, 'gb2': b2.grad if bias else None}
            finally:
                switches(**defaults)
        record(name, call)

    for kind, store, bias, stream in itertools.product(('pair', 'pw', 'pw_lrelu'), ('fp32', 'bf16'), (True, False), (True, False)):
        conv_case(kind, store, bias, stream)
    for stream in (True, False):
        conv_case('pair_second_consumer', 'bf16', True, stream)

    with open(os.path.join(out, 'launches.json'), 'w') as f:
        json.dump(launches, f, indent=1, sort_keys=True)
    print('wrote', len(launches), 'configurations to', out)


def _max_diff(a, b):
    x, y = np.load(a), np.load(b)
    if x.shape != y.shape:
        return float('inf')
    return 0.0 if x.tobytes() == y.tobytes() else float(np.nanmax(np.abs(x.astype(np.float64) - y.astype(np.float64))))


def _compare(a, b, c, out_json):
    """a, b: the parent twice; c: the change.  Every array of the change must equal the parent's bit for bit; an array on which
    the parent disagrees with itself is reported (`parent_disagrees_with_itself`) and fails here too: such a configuration
    is then compared by the existing tests' tolerances instead."""
    names = sorted(f for f in os.listdir(a) if f.endswith('.npy'))
    missing = sorted(set(names) ^ set(f for f in os.listdir(c) if f.endswith('.npy')))
    la, lb, lc = (json.load(open(os.path.join(d, 'launches.json'))) for d in (a, b, c))
    unstable, failed, per_array = [], list(missing), {}
    for f in names:
        if f in missing:
            continue
        own, got = _max_diff(os.path.join(a, f), os.path.join(b, f)), _max_diff(os.path.join(a, f), os.path.join(c, f))
        if own != 0.0:
            unstable.append(f)
        if got != 0.0:
            failed.append(f)
            per_array[f] = {'parent_vs_parent_max_abs': own, 'change_vs_parent_max_abs': got}
    launch_diff = {}
    for name in sorted(set(la) | set(lc)):
        pa, pc = la.get(name, {}), lc.get(name, {})
        d = {k: [pa.get(k, 0), pc.get(k, 0)] for k in sorted(set(pa) | set(pc)) if pa.get(k, 0) != pc.get(k, 0)}
        if d or la.get(name) != lb.get(name):
            launch_diff[name] = {'parent_vs_change': d, 'parent_runs_agree': la.get(name) == lb.get(name)}
    res = {'what': 'tools/train_layers_parity.py: the parent commit run twice (A, B) against this change (C)',
           'configurations': len(la), 'arrays': len(names), 'arrays_bitwise_equal_to_parent': len(names) - len(failed),
           'parent_disagrees_with_itself': unstable, 'arrays_failing': failed, 'launch_count_differences': launch_diff,
           'pass': not failed and not launch_diff, 'per_array': per_array, 'launches_per_call': lc}
    with open(out_json, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps({k: res[k] for k in ('configurations', 'arrays', 'arrays_bitwise_equal_to_parent', 'parent_disagrees_with_itself',
                                          'arrays_failing', 'launch_count_differences', 'pass')}, indent=1))
    return 0 if res['pass'] else 1


if __name__ == '__main__':
    if len(sys.argv) == 3 and sys.argv[1] == 'run':
        _run(sys.argv[2])
    elif len(sys.argv) == 6 and sys.argv[1] == 'compare':
        sys.exit(_compare(*sys.argv[2:6]))
    else:
        sys.exit(__doc__)
