"""Host side of the fused initial pose (ops.depth_init, pose/initialization.py `kernel`, PoseEstimator `init_kernel`): the
wrapper's argument checks (which raise before any library call), the option values, the way a TOML preset carries
init_kernel, what 'fused' does without a GPU, and the binding table.  No GPU."""
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Stub:
    device = 'cpu'
    photographer = object()


def _estimators(**extra):
    from latentfusion_amd.pose import estimation
    kw = dict(model=_Stub(), ranking_size=4, loss_weights={'depth': 1.0}, **extra)
    return (estimation.PoseEstimator(**kw),
            estimation.MetropolisPoseEstimator(num_samples=4, num_iters=1, **kw),
            estimation.CrossEntropyPoseEstimator(num_samples=8, num_elites=2, num_iters=1, num_gmm_components=2, learning_rate=0.9, **kw),
            estimation.GradientPoseEstimator(learning_rate=0.01, num_samples=4, num_iters=1, converge_threshold=1e-6,
                                             converge_patience=10, **kw))


def test_wrapper_checks_raise_before_any_library_call(monkeypatch):
    from latentfusion_amd import _lib, ops

    def no_library():
        raise AssertionError('the library was asked for')
    monkeypatch.setattr(_lib, 'lib', no_library)
    host = torch.ones(2, 1, 8, 8)
    with pytest.raises(ValueError, match='device'):
        ops.depth_init(host, host)                                               # host tensors
    with pytest.raises(ValueError):
        ops.depth_init(host.tolist(), host)                                      # not a tensor
    # shape, dtype and value rules on meta tensors that claim to be on the device: nothing may reach the library
    # (meta tensors carry shape, dtype and device but no storage, so every rule can be tried where there is no GPU; for the
    # wrapper to take them as device tensors Tensor.is_cuda is patched for the rest of this test -- monkeypatch restores it)
    monkeypatch.setattr(torch.Tensor, 'is_cuda', property(lambda self: self.device.type == 'meta'))

    def meta(*shape, dtype=torch.float32):
        return torch.empty(*shape, device='meta', dtype=dtype)
    d, mk, K = meta(2, 1, 8, 8), meta(2, 1, 8, 8), meta(2, 3, 3)
    bad = [dict(depth=d.double()), dict(depth=d.half()), dict(mask=mk.double()), dict(mask=mk.to(torch.int32)),
           dict(mask=mk.to(torch.int8)), dict(depth=meta(2, 2, 8, 8), mask=meta(2, 2, 8, 8)), dict(depth=meta(8, 8), mask=meta(8, 8)),
           dict(depth=meta(2, 1, 1, 8, 8), mask=meta(2, 1, 1, 8, 8)), dict(depth=meta(0, 1, 8, 8), mask=meta(0, 1, 8, 8)),
           dict(depth=meta(2, 1, 0, 8), mask=meta(2, 1, 0, 8)), dict(mask=meta(2, 1, 8, 9)), dict(mask=meta(3, 1, 8, 8)),
           dict(mask=host), dict(depth=host),
           dict(depth=meta(1 << 15, 1 << 8, 1 << 8), mask=meta(1 << 15, 1 << 8, 1 << 8, dtype=torch.uint8)),
           dict(intrinsic=meta(3, 3, 3)), dict(intrinsic=meta(2, 3, 2)), dict(intrinsic=meta(2, 2, 3)), dict(intrinsic=meta(3, 3)),
           dict(intrinsic=meta(2, 3, 3, dtype=torch.float64)), dict(intrinsic=torch.eye(3).repeat(2, 1, 1)),
           dict(intrinsic=[[1.0, 0.0, 0.0]] * 3),
           dict(m=0.0), dict(m=-1.0), dict(m=float('nan')), dict(m=None), dict(m='3'), dict(m=True),
           dict(erode_radius=-1), dict(erode_radius=9), dict(erode_radius=1.0), dict(erode_radius=None), dict(erode_radius=True)]
    for over in bad:
        kw = dict(dict(depth=d, mask=mk, intrinsic=K), **over)
        with pytest.raises(ValueError):
            ops.depth_init(**kw)
    # and the forms it accepts get as far as the library
    for kw in (dict(depth=d, mask=mk, intrinsic=K), dict(depth=meta(2, 8, 8), mask=meta(2, 8, 8, dtype=torch.bool)),
               dict(depth=d, mask=meta(2, 8, 8, dtype=torch.uint8), intrinsic=meta(1, 3, 4), m=2, erode_radius=8)):
        with pytest.raises(AssertionError, match='the library was asked for'):
            ops.depth_init(**kw)


def test_kernel_values():
    from latentfusion_amd.pose import initialization as ini
    assert ini.KERNEL == 'composed' and ini.KERNELS == ('composed', 'fused')
    assert ini.select_kernel(None) == 'composed' and ini.select_kernel('fused') == 'fused'
    for fn in (ini.estimate_translation, ini.estimate_initial_pose):
        p = inspect.signature(fn).parameters
        assert (p['kernel'].default, p['erode_radius'].default, p['check'].default) == (None, 0, True)
    d = torch.zeros(1, 1, 8, 8)
    d[0, 0, 2:6, 2:7] = torch.linspace(0.5, 0.6, 20).view(4, 5)
    mk, K = (d > 0).float(), torch.eye(3).unsqueeze(0)
    for bad in ('hip', 'Fused', '', 0, True):
        with pytest.raises(ValueError, match='kernel'):
            ini.estimate_translation(d, mk, K, kernel=bad)
        with pytest.raises(ValueError, match='kernel'):
            ini.estimate_initial_pose(d, mk, K, 8, 8, kernel=bad)
    # the default is the host path, unchanged
    a = ini.estimate_initial_pose(d, mk, K, 8, 8)
    b = ini.estimate_initial_pose(d, mk, K, 8, 8, kernel='composed', erode_radius=0, check=False)
    assert torch.equal(a.translation, b.translation) and float(a.translation[0, 2]) == pytest.approx(0.55, abs=1e-6)


def test_erode_radius_is_refused_on_the_composed_path():
    from latentfusion_amd.observation import Observation
    from latentfusion_amd.modules.geometry import Camera
    from latentfusion_amd.pose import initialization as ini
    d = torch.zeros(1, 1, 8, 8)
    d[0, 0, 2:6, 2:7] = torch.linspace(0.5, 0.6, 20).view(4, 5)
    mk, K = (d > 0).float(), torch.eye(3).unsqueeze(0)
    for kw in (dict(erode_radius=1), dict(erode_radius=3, kernel='composed')):
        with pytest.raises(ValueError, match='erode_radius'):
            ini.estimate_translation(d, mk, K, **kw)
        with pytest.raises(ValueError, match='erode_radius'):
            ini.estimate_initial_pose(d, mk, K, 8, 8, **kw)
    for bad in (-1, 9, 1.5, None):
        for kernel in ('composed', 'fused'):
            with pytest.raises(ValueError, match='erode_radius'):
                ini.estimate_translation(d, mk, K, kernel=kernel, erode_radius=bad)
    obs = Observation(None, d, mk, Camera(K, torch.eye(4).unsqueeze(0), width=8, height=8))
    with pytest.raises(ValueError, match='erode_radius'):
        obs.estimate_camera(erode_radius=2)
    with pytest.raises(ValueError, match='erode_radius'):
        obs.zoom_estimate(1.0, 4, erode_radius=2)
    for fn in (Observation.estimate_camera, Observation.zoom_estimate):
        p = inspect.signature(fn).parameters
        assert (p['kernel'].default, p['erode_radius'].default) == (None, 0)


def test_estimators_take_init_kernel(monkeypatch):
    from latentfusion_amd.pose import estimation
    for est in _estimators():
        assert est.init_kernel == 'composed'
    for v in ('composed', 'fused'):
        for est in _estimators(init_kernel=v):
            assert est.init_kernel == v
    for bad in ('hip', None, 'autograd', ''):
        with pytest.raises(ValueError, match='init_kernel'):
            estimation.PoseEstimator(model=_Stub(), ranking_size=4, loss_weights={}, init_kernel=bad)
    # initial_pose stays a classmethod of one argument; the estimators' own draws go through the option
    assert inspect.signature(estimation.PoseEstimator.initial_pose).parameters.keys() == {'target_obs'}
    assert isinstance(inspect.getattr_static(estimation.PoseEstimator, 'initial_pose'), classmethod)
    assert inspect.signature(estimation.PoseEstimator.initial_pose_batch).parameters['kernel'].default is None
    # an estimate without given cameras draws its initial pose through the option: _initial_pose for one target,
    # initial_pose_batch for estimate_batch (both recorded here and cut short)
    from latentfusion_amd.modules.geometry import Camera
    from latentfusion_amd.observation import Observation
    d = torch.zeros(1, 1, 8, 8)
    d[0, 0, 2:6, 2:7] = torch.linspace(0.5, 0.6, 20).view(4, 5)
    obs = Observation(None, d, (d > 0).float(), Camera(torch.eye(3).unsqueeze(0), torch.eye(4).unsqueeze(0), width=8, height=8))
    calls = []

    class Reached(Exception):
        pass

    def record(name):
        def fn(self, *args, **kwargs):
            calls.append((type(self).__name__, name, self.init_kernel))
            raise Reached
        return fn
    monkeypatch.setattr(estimation.PoseEstimator, '_initial_pose', record('_initial_pose'))
    monkeypatch.setattr(estimation.PoseEstimator, 'initial_pose_batch', record('initial_pose_batch'))
    ests = _estimators(init_kernel='fused')[1:]
    for est in ests:
        with pytest.raises(Reached):
            est._estimate(None, obs)
    with pytest.raises(Reached):
        ests[-1].estimate_batch(None, [obs, obs])
    assert calls == [('MetropolisPoseEstimator', '_initial_pose', 'fused'), ('CrossEntropyPoseEstimator', '_initial_pose', 'fused'),
                     ('GradientPoseEstimator', '_initial_pose', 'fused'), ('GradientPoseEstimator', 'initial_pose_batch', 'fused')]
    monkeypatch.undo()
    with pytest.raises(ValueError, match='kernel'):
        _estimators()[0].initial_pose_batch([], kernel='hip')


@pytest.mark.parametrize('preset', ['adam_latent.toml', 'cross_entropy_latent.toml'])
@pytest.mark.parametrize('value', ['fused', 'composed', None])
def test_toml_option_reaches_the_constructor(preset, value):
    from latentfusion_amd.pose import estimation
    config = estimation._load_toml(os.path.join(ROOT, 'configs', preset))
    assert 'init_kernel' not in config['args']                                   # the shipped presets keep the default
    config = dict(config, args=dict(config['args']))
    if value is not None:
        config['args']['init_kernel'] = value
    est = estimation.load_from_config(config, _Stub())
    assert est.init_kernel == (value or 'composed')
    assert estimation.load_from_config(config, _Stub(), init_kernel='fused').init_kernel == 'fused'
    bad = dict(config, args=dict(config['args'], init_kernel='hip'))
    with pytest.raises(ValueError, match='init_kernel'):
        estimation.load_from_config(bad, _Stub())


def test_fused_without_a_gpu_raises(monkeypatch):
    """No silent fall-back: with no GPU in the process 'fused' is an error that says so, on every way in."""
    from latentfusion_amd import _lib
    from latentfusion_amd.modules.geometry import Camera
    from latentfusion_amd.observation import Observation
    from latentfusion_amd.pose import estimation, initialization as ini
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    monkeypatch.setattr(_lib, 'lib', lambda: (_ for _ in ()).throw(AssertionError('the library was asked for')))
    d = torch.zeros(1, 1, 8, 8)
    d[0, 0, 2:6, 2:7] = torch.linspace(0.5, 0.6, 20).view(4, 5)
    mk, K = (d > 0).float(), torch.eye(3).unsqueeze(0)
    obs = Observation(None, d, mk, Camera(K, torch.eye(4).unsqueeze(0), width=8, height=8))
    est = estimation.PoseEstimator(model=_Stub(), ranking_size=4, loss_weights={}, init_kernel='fused')
    for call in (lambda: ini.estimate_translation(d, mk, K, kernel='fused'),
                 lambda: ini.estimate_initial_pose(d, mk, K, 8, 8, kernel='fused', check=False),
                 lambda: obs.estimate_camera(kernel='fused'), lambda: obs.zoom_estimate(1.0, 4, kernel='fused'),
                 lambda: est.initial_pose_batch([obs]), lambda: est._initial_pose(obs),
                 lambda: estimation.PoseEstimator(model=_Stub(), ranking_size=4, loss_weights={}).initial_pose_batch([obs], kernel='fused')):
        with pytest.raises(RuntimeError, match='GPU'):
            call()
    # the default and the classmethod do not care
    assert torch.equal(est.initial_pose(obs).translation, obs.estimate_camera().translation)
    assert torch.equal(estimation.PoseEstimator(model=_Stub(), ranking_size=4, loss_weights={}).initial_pose_batch([obs])[0].translation,
                       est.initial_pose(obs).translation)


def test_entry_points_are_bound_with_the_headers_argument_counts():
    from latentfusion_amd import _lib
    from latentfusion_amd.csrc import build
    assert 'depth_init.hip' in build.SOURCES and 'depth_init.hip' not in build.EXTRA          # the default flags only
    header = open(os.path.join(ROOT, 'include', 'lf_hip.h')).read()
    assert 'pose/initialization.py:8-86' in header
    header = re.sub(r'/\*.*?\*/', ' ', header, flags=re.S)
    for name, arity in (('lf_depth_init_scratch_bytes', 3), ('lf_depth_init', 16)):
        proto = re.search(r'\b' + name + r'\s*\(([^)]*)\)', header)
        assert proto is not None, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(proto.group(1).split(',')) == arity, name
    L = _lib.lib()
    assert L.lf_depth_init_scratch_bytes(3, 17, 23) >= 3 * 17 * 23 * 4 and L.lf_depth_init_scratch_bytes(3, 17, 23) % 4 == 0
    assert L.lf_depth_init_scratch_bytes(0, 1, 1) == 0 and L.lf_depth_init_scratch_bytes(1 << 15, 1 << 8, 1 << 8) == 0
    # the argument rules are decided on the host, before anything is launched: no GPU is needed to see them
    assert L.lf_depth_init(None, None, 0, None, 1, 3.0, 0, None, None, None, None, 0, 1, 1, 1, None) == -1
