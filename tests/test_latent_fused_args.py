"""CPU tests of the host side of the fused latent term (lf_latent_cosine_fwd / lf_latent_cosine_bwd_epi): the rules of the
`latent_kernel` option in the engines and the estimators as far as they are decidable without a GPU, the way a TOML preset
carries it to the engine's constructor, and the binding table against the header.  No kernel is launched here."""
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_select_latent_kernel_rules():
    from latentfusion_amd.engine import LATENT_KERNELS, RenderLoopEngine, select_latent_kernel
    assert LATENT_KERNELS == ('autograd', 'fused')
    assert RenderLoopEngine.LATENT_KERNEL == 'autograd'                      # the default does not change
    assert select_latent_kernel(None, 'autograd') == 'autograd'              # None -> the class default
    assert select_latent_kernel(None, 'fused') == 'fused'
    assert select_latent_kernel('fused', 'autograd') == 'fused'
    assert select_latent_kernel('autograd', 'fused') == 'autograd'
    for bad in ('aten', 'Fused', '', True, 0):
        with pytest.raises(ValueError):
            select_latent_kernel(bad, 'autograd')
    with pytest.raises(ValueError):
        select_latent_kernel(None, 'hip')


def test_engines_take_latent_kernel():
    from latentfusion_amd.engine import RenderLoopEngine
    from latentfusion_amd.engine_multi import MultiTargetEngine
    from latentfusion_amd.experimental import RenderLoopEngineX
    for cls in (RenderLoopEngine, MultiTargetEngine, RenderLoopEngineX):
        p = inspect.signature(cls.__init__).parameters
        assert 'latent_kernel' in p and p['latent_kernel'].default is None, cls
        assert cls.LATENT_KERNEL == 'autograd'
    # the positional order of the earlier arguments is unchanged (the new one comes last)
    names = list(inspect.signature(RenderLoopEngine.__init__).parameters)
    assert names[:8] == ['self', 'photographer', 'z_obj', 'target_obs', 'loss_weights', 'conv_mode', 'fuse_projection', 'proj_kernel']
    assert names[-1] == 'latent_kernel'


class _Stub:
    device = 'cpu'
    photographer = object()


class _DeviceVolume:
    """Stands in for a device-resident volume: _engine_for only asks where it lives before it constructs the engine."""
    is_cuda = True


def _estimators(**extra):
    from latentfusion_amd.pose import estimation
    kw = dict(model=_Stub(), ranking_size=4, loss_weights={'depth': 1.0, 'latent': 0.2}, **extra)
    return (estimation.PoseEstimator(**kw),
            estimation.CrossEntropyPoseEstimator(num_samples=8, num_elites=2, num_iters=1, num_gmm_components=2, learning_rate=0.9, **kw),
            estimation.GradientPoseEstimator(learning_rate=0.01, num_samples=4, num_iters=1, converge_threshold=1e-6,
                                             converge_patience=10, **kw))


def test_estimators_take_latent_kernel():
    from latentfusion_amd.pose import estimation
    for est in _estimators():
        assert est.latent_kernel is None
    for v in ('autograd', 'fused', None):
        for est in _estimators(latent_kernel=v):
            assert est.latent_kernel == v
    with pytest.raises(ValueError):
        estimation.PoseEstimator(model=_Stub(), ranking_size=4, loss_weights={}, latent_kernel='aten')
    # on the host there is no engine (the volume is not on a device): the option is carried, nothing is built
    est = estimation.PoseEstimator(model=_Stub(), ranking_size=4, loss_weights={}, latent_kernel='fused')
    assert est._engine_for(torch.zeros(1, 1, 4, 2, 2, 2), None) is None


@pytest.mark.parametrize('preset', ['adam_latent.toml', 'cross_entropy_latent.toml'])
@pytest.mark.parametrize('value', ['fused', 'autograd', None])
def test_toml_option_reaches_the_engine_constructor(monkeypatch, preset, value):
    """[args] latent_kernel = "fused" of a preset -> load_from_config -> the estimator -> the keyword the engine is built with."""
    from latentfusion_amd import engine
    from latentfusion_amd.pose import estimation
    config = estimation._load_toml(os.path.join(ROOT, 'configs', preset))
    assert 'latent' in config['loss_weights'] and 'latent_kernel' not in config['args']      # the shipped presets keep the default
    config = dict(config, args=dict(config['args']))
    if value is not None:
        config['args']['latent_kernel'] = value
    est = estimation.load_from_config(config, _Stub())
    assert est.latent_kernel == value
    built = []

    class Recorder:
        LOSS_KEYS = engine.RenderLoopEngine.LOSS_KEYS

        @staticmethod
        def supports(photographer, loss_weights):
            return True

        def __init__(self, *args, **kwargs):
            built.append((args, kwargs))
    monkeypatch.setattr(engine, 'RenderLoopEngine', Recorder)
    eng = est._engine_for(_DeviceVolume(), None, getattr(est, 'loss_schedules', ()))
    assert isinstance(eng, Recorder) and len(built) == 1
    assert built[0][1]['latent_kernel'] == value and built[0][1]['proj_kernel'] is None
    # a keyword of load_from_config overrides the file, as for every other argument
    assert estimation.load_from_config(config, _Stub(), latent_kernel='fused').latent_kernel == 'fused'
    bad = dict(config, args=dict(config['args'], latent_kernel='aten'))
    with pytest.raises(ValueError):
        estimation.load_from_config(bad, _Stub())


def test_estimate_batch_hands_the_option_to_the_multi_target_engine():
    from latentfusion_amd.pose import estimation
    src = inspect.getsource(estimation.GradientPoseEstimator.estimate_batch)
    call = src[src.index('MultiTargetEngine('):]
    assert 'latent_kernel=self.latent_kernel' in call[:call.index('_run_batch')]


def test_new_symbols_are_bound_with_the_header_arity():
    from latentfusion_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'lf_hip.h')).read()
    header = re.sub(r'/\*.*?\*/', ' ', header, flags=re.S)
    want = {'lf_latent_cosine_scratch_bytes': 3, 'lf_latent_cosine_fwd': 15, 'lf_latent_cosine_bwd_epi': 17}
    for name, arity in want.items():
        assert name in _lib.SIGNATURES and name not in _lib.EXPERIMENTAL_SIGNATURES, name
        m = re.search(r'\b' + name + r'\s*\(([^)]*)\)', header)
        assert m, name
        assert len(m.group(1).split(',')) == arity == len(_lib.SIGNATURES[name][1]), name
    assert _lib.SIGNATURES['lf_latent_cosine_scratch_bytes'][0] is _lib.c_size_t
    L = _lib.lib()                                               # loads (and resolves the symbols) without a GPU
    # the scratch rule: 4 floats per slice of LAT_ITERS * (256 / lanes per pixel) pixels, per row; 0 outside the domain
    q = L.lf_latent_cosine_scratch_bytes
    assert q(1, 1, 4) == 16 and q(7, 1024, 4) == 7 * 16 and q(7, 1025, 4) == 7 * 2 * 16
    assert q(1, 256, 16) == 16 and q(8, 128 * 128, 16) == 8 * 64 * 16
    assert q(1, 128, 20) == 16 and q(1, 129, 20) == 16 * 2 and q(2, 16, 256) == 2 * 16 and q(2, 17, 256) == 2 * 2 * 16
    assert q(3, 100, 16) == 3 * q(1, 100, 16)                    # per row: the split never follows the batch
    for bad in ((0, 16, 16), (1, 0, 16), (1, 16, 0), (1, 16, 6), (1, 16, 260), (-1, 16, 16)):
        assert q(*bad) == 0, bad


def test_wrappers_reject_host_tensors():
    from latentfusion_amd import _lib, ops
    zp = torch.zeros(2, 16, 4, 4).contiguous(memory_format=torch.channels_last)
    zt = torch.zeros(1, 16, 4, 4)
    with pytest.raises(_lib.LFHipError, match='device tensor'):
        ops.latent_cosine_fwd(zp, zt)
    with pytest.raises(_lib.LFHipError, match='device tensor'):
        ops.latent_cosine_bwd_epi(None, zp, None, zt, torch.zeros(2, 4), 1.0, 0)
