#!/usr/bin/env python
"""Host cost of ops.launch per call against the inline form it replaced, on a stub library (no device, no shared object):
lf_conv3d_c16_wino, 18 C arguments, five optional pointers of which two are given.  Writes both figures and the budget
check of DESIGN.md ("One launch helper") to profiles/launch_helper_host.json.

    python tools/launch_helper_host.py [--launches-per-step 1003 --step-ms 55.0]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from latentfusion_amd import _lib, ops  # noqa: E402
from latentfusion_amd._lib import check  # noqa: E402
from latentfusion_amd.ops import PN_EPS, SLOPE, _ptr, _timed  # noqa: E402


def _stream():
    return 0


class _Stub:
    @staticmethod
    def lf_conv3d_c16_wino(*args):
        return 0


def inline(x, upack, bias, y, norm, N, D, H, W, he, flags, py, pn, pf, amax_out):
    """The call site of ops.conv3d_c16_wino before the helper, verbatim."""
    L = _lib.lib()
    with _timed('conv3d_c16_wino'):
        check(L.lf_conv3d_c16_wino(_ptr(x), _ptr(upack), _ptr(bias) if bias is not None else None, _ptr(y),
                                   _ptr(norm) if norm is not None else None, N, D, H, W, he, flags, SLOPE, PN_EPS,
                                   _ptr(py) if py is not None else None, _ptr(pn) if pn is not None else None, pf,
                                   _ptr(amax_out) if amax_out is not None else None, _stream()), 'lf_conv3d_c16_wino')


def helper(x, upack, bias, y, norm, N, D, H, W, he, flags, py, pn, pf, amax_out):
    ops.launch('lf_conv3d_c16_wino', x, upack, bias, y, norm, N, D, H, W, he, flags, SLOPE, PN_EPS, py, pn, pf, amax_out,
               tag='conv3d_c16_wino')


def per_call_us(fns, args, calls, repeats):
    """Best mean over `calls` calls of each function; the functions take turns, so a busy spell of the machine hits both."""
    best = [float('inf')] * len(fns)
    for _ in range(repeats):
        for k, fn in enumerate(fns):
            t0 = time.perf_counter()
            for _ in range(calls):
                fn(*args)
            best[k] = min(best[k], (time.perf_counter() - t0) / calls)
    return [b * 1e6 for b in best]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=5000)
    ap.add_argument('--repeats', type=int, default=40)
    ap.add_argument('--launches-per-step', type=int, default=None, help="cfg 5 library_launches_per_step of the parent's bench run")
    ap.add_argument('--step-ms', type=float, default=None, help="cfg 5 median ms_per_step of the parent's bench run")
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'launch_helper_host.json'))
    a = ap.parse_args()
    _lib._lib = _Stub()
    ops._stream = _stream
    t = [torch.zeros(16) for _ in range(6)]
    args = (t[0], t[1], t[2], t[3], t[4], 8, 32, 32, 32, 0.068, 3, None, None, 0, None)
    res = {'entry_point': 'lf_conv3d_c16_wino', 'c_arguments': 18, 'optional_pointers': 5, 'calls': a.calls, 'repeats': a.repeats,
           'statistic': 'best of repeats (the two forms take turns), mean over calls', 'python': sys.version.split()[0]}
    res['inline_us'], res['launch_us'] = (round(v, 3) for v in per_call_us((inline, helper), args, a.calls, a.repeats))
    res['extra_us'] = round(res['launch_us'] - res['inline_us'], 3)
    if a.launches_per_step and a.step_ms:
        extra_ms = max(res['extra_us'], 0.0) * a.launches_per_step / 1e3
        res.update(launches_per_step=a.launches_per_step, step_ms=a.step_ms, extra_ms_per_step=round(extra_ms, 4),
                   extra_share_of_step=round(extra_ms / a.step_ms, 6), budget_share=0.005,
                   within_budget=bool(extra_ms / a.step_ms < 0.005))
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
