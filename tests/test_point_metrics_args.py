"""Host side of the batched pose metrics (pose/metrics.py: camera_metrics_batch, best_distance_device; ops.nn_dist,
ops.points_pair_dist): the CPU fallback against the per-pair functions on the g13 fixture, the length rules, the wrappers'
argument checks (which raise before any library call) and the binding table.  No GPU."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ('rotation_dist', 'translation_dist', 'add', 'add_s', 'add_sym', 'proj2d')


def prod_camera(d):
    from latentfusion_amd.modules.geometry import Camera
    return Camera(d['K'].clone(), None, d['z_span'], d['viewport'].clone(), width=d['width'], height=d['height'],
                  log_quaternion=d['log_q'].clone(), translation=d['t'].clone())


@pytest.fixture(scope='module')
def g13(golden):
    g = golden('g13_metrics')
    return g, prod_camera(g['gt']), prod_camera(g['ev'])


def _stack(per_pair, key):
    return torch.stack([torch.as_tensor(m[key], dtype=torch.float32).reshape(()) for m in per_pair])


def test_cpu_fallback_equals_the_per_pair_functions(g13):
    from latentfusion_amd.pose import metrics
    g, gt, ev = g13
    per_pair = metrics.camera_metrics(gt, ev, g['points'], g['scale'])
    got = metrics.camera_metrics_batch(gt, ev, g['points'], g['scale'])
    assert tuple(got) == KEYS == tuple(per_pair[0])
    for k in KEYS:
        assert got[k].shape == (3,) and got[k].dtype == torch.float32 and got[k].device.type == 'cpu'
        assert torch.equal(got[k], _stack(per_pair, k)), k
    # and the fixture itself, at the bound of test_pose_metrics_golden
    for i, want in enumerate(g['metrics']):
        for k, v in want.items():
            assert abs(float(got[k][i]) - v) <= 1e-5 * max(1.0, abs(v)), (k, i)


def test_one_ground_truth_against_all_hypotheses(g13):
    from latentfusion_amd.pose import metrics
    g, gt, ev = g13
    got = metrics.camera_metrics_batch(gt[0], ev, g['points'], g['scale'])
    per_pair = [metrics.camera_metrics(gt[0], ev[i], g['points'], g['scale']) for i in range(3)]
    for k in KEYS:
        assert torch.equal(got[k], _stack(per_pair, k)), k


def test_length_rules(g13):
    from latentfusion_amd.modules.geometry import Camera
    from latentfusion_amd.pose import metrics
    g, gt, ev = g13
    for n_gt, n_ev in ((1, 1), (1, 3), (3, 3), (2, 2)):
        assert metrics.camera_metrics_batch(gt[:n_gt], ev[:n_ev], None, 1.0)['rotation_dist'].shape == (n_ev,)
    ev6 = Camera.cat([ev, ev])
    for n_gt, n_ev in ((2, 3), (3, 1), (3, 2), (3, 6), (2, 6)):
        with pytest.raises(ValueError):
            metrics.camera_metrics_batch(gt[:n_gt], ev6[:n_ev], g['points'], g['scale'])


def test_no_points_and_switches(g13):
    from latentfusion_amd.pose import metrics
    g, gt, ev = g13
    assert tuple(metrics.camera_metrics_batch(gt, ev, None, g['scale'])) == KEYS[:2]
    full = metrics.camera_metrics_batch(gt, ev, g['points'], g['scale'])
    for off in ('add', 'add_s', 'add_sym', 'proj2d'):
        got = metrics.camera_metrics_batch(gt, ev, g['points'], g['scale'], **{'use_' + off: False})
        assert set(got) == set(KEYS) - {off}                      # honoured for EVERY pair, unlike the per-pair recursion
        for k in got:
            assert torch.equal(got[k], full[k])


def test_layout_is_that_of_concat_camera_metrics(g13):
    from latentfusion_amd.pose import metrics
    g, gt, ev = g13
    cat = metrics.concat_camera_metrics(metrics.camera_metrics(gt, ev, g['points'], g['scale']))
    got = {k: v.tolist() for k, v in metrics.camera_metrics_batch(gt, ev, g['points'], g['scale']).items()}
    assert list(got) == list(cat)
    for k in cat:
        assert len(got[k]) == len(cat[k]) == 3
        assert got[k] == [float(torch.as_tensor(v, dtype=torch.float32)) for v in cat[k]]


def test_wrapper_checks_raise_before_any_library_call(monkeypatch):
    from latentfusion_amd import _lib, ops

    def no_library():
        raise AssertionError('the library was asked for')
    monkeypatch.setattr(_lib, 'lib', no_library)
    x = torch.zeros(5, 3)
    with pytest.raises(ValueError, match='device'):
        ops.nn_dist(x, x)                                         # host tensors
    with pytest.raises(ValueError, match='device'):
        ops.points_pair_dist(x, torch.zeros(2, 4, 4), torch.zeros(2, 4, 4))
    with pytest.raises(ValueError, match='want'):
        ops.nn_dist(x, x, want=())
    with pytest.raises(ValueError, match='want'):
        ops.nn_dist(x, x, want=('dist', 'squared'))
    with pytest.raises(ValueError):
        ops.nn_dist([[0.0, 0.0, 0.0]], x)                         # not a tensor
    # shape and dtype rules, on meta tensors that claim to be on the device (no GPU needed: nothing may reach the library)
    dev = torch.empty(5, 3, device='meta')
    monkeypatch.setattr(torch.Tensor, 'is_cuda', property(lambda self: self.device.type == 'meta'))
    bad = [dict(x1=dev.double(), x2=dev), dict(x1=dev, x2=dev.half()), dict(x1=torch.empty(5, 4, device='meta'), x2=dev),
           dict(x1=torch.empty(15, device='meta'), x2=dev), dict(x1=torch.empty(0, 3, device='meta'), x2=dev),
           dict(x1=torch.empty(2, 5, 3, device='meta'), x2=torch.empty(3, 5, 3, device='meta')),
           dict(x1=dev, x2=dev, T1=torch.empty(2, 4, 4, device='meta')),
           dict(x1=dev, x2=dev, T1=torch.empty(2, 3, 4, device='meta'), T2=torch.empty(3, 3, 4, device='meta')),
           dict(x1=torch.empty(2, 5, 3, device='meta'), x2=dev, T2=torch.empty(1, 3, 4, device='meta')),
           dict(x1=dev, x2=dev, T2=torch.empty(2, 3, 4, device='meta', dtype=torch.float64))]
    for kw in bad:
        with pytest.raises(ValueError):
            ops.nn_dist(**kw)
    m44, m34 = torch.empty(2, 4, 4, device='meta'), torch.empty(2, 3, 4, device='meta')
    bad = [(dev, m44, m34), (dev, m44, torch.empty(3, 4, 4, device='meta')), (dev, torch.empty(2, 4, 3, device='meta'), m44),
           (dev.double(), m44, m44), (dev, m44.double(), m44), (torch.empty(5, 2, device='meta'), m34, m34),
           (torch.empty(3, 5, 3, device='meta'), m44, m44), (dev, m44[0], m44[0])]
    for args in bad:
        with pytest.raises(ValueError):
            ops.points_pair_dist(*args)


def test_new_entry_points_are_bound_with_the_headers_argument_counts():
    from latentfusion_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'lf_hip.h')).read()
    header = re.sub(r'/\*.*?\*/', ' ', header, flags=re.S)
    for name in ('lf_nn_dist_scratch_bytes', 'lf_nn_dist', 'lf_points_pair_dist_scratch_bytes', 'lf_points_pair_dist'):
        proto = re.search(r'\b' + name + r'\s*\(([^)]*)\)', header)
        assert proto is not None, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(proto.group(1).split(',')), name
    L = _lib.lib()
    assert L.lf_nn_dist_scratch_bytes(3, 257, 1025) == 3 * 5 * 8 and L.lf_nn_dist_scratch_bytes(0, 1, 1) == 0
    assert L.lf_points_pair_dist_scratch_bytes(7, 1500) == 7 * 24 * 8 and L.lf_points_pair_dist_scratch_bytes(1, 0) == 0
