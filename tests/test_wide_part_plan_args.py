"""Host side of the per-target launch plan: the ops.wide_parts scope, the estimator's and the TOML's per_target_plan option,
and the f16x3 refusal, which is raised from the arguments alone (no device, no model is touched)."""
import pytest
import torch


def test_wide_parts_nests_and_restores():
    from latentfusion_amd import ops
    assert ops.WIDE_PARTS is None
    with ops.wide_parts(4):
        assert ops.WIDE_PARTS == 4
        with ops.wide_parts(2):
            assert ops.WIDE_PARTS == 2
            with ops.wide_parts(None):                     # (None: the batch's own plan inside an outer scope)
                assert ops.WIDE_PARTS is None
            assert ops.WIDE_PARTS == 2
        assert ops.WIDE_PARTS == 4
    assert ops.WIDE_PARTS is None
    with pytest.raises(RuntimeError):
        with ops.wide_parts(3):
            raise RuntimeError('inside')
    assert ops.WIDE_PARTS is None                          # restored when the block raises


@pytest.mark.parametrize('bad', [0, -1, 2.0, '2', True])
def test_wide_parts_rejects_what_is_no_positive_int(bad):
    from latentfusion_amd import ops
    with pytest.raises(ValueError):
        ops.wide_parts(bad)
    assert ops.WIDE_PARTS is None


def test_scope_gives_part_n_of_a_batch():
    from latentfusion_amd import ops
    assert ops._wide_part_n(8) is None
    with ops.wide_parts(2):
        assert ops._wide_part_n(8) == 2
        with pytest.raises(ValueError, match='does not divide'):
            ops._wide_part_n(7)


def test_entry_points_are_in_the_ctypes_table():
    import ctypes
    from latentfusion_amd import _lib
    plain, part = _lib.SIGNATURES['lf_wino_fused_gemm'], _lib.SIGNATURES['lf_wino_fused_gemm_part']
    assert part[0] is plain[0] and part[1] == plain[1][:-1] + [ctypes.c_int] + plain[1][-1:]
    qplain, qpart = _lib.SIGNATURES['lf_wino_fused_scratch_bytes'], _lib.SIGNATURES['lf_wino_fused_scratch_bytes_part']
    assert qpart[0] is qplain[0] and qpart[1] == qplain[1] + [ctypes.c_int]


_ARGS = dict(learning_rate=0.01, num_samples=2, num_iters=2, ranking_size=2, converge_threshold=-1.0, converge_patience=1,
             loss_weights={'depth': 1.0})


def test_estimator_takes_and_forwards_the_option(monkeypatch):
    from latentfusion_amd import engine_multi
    from latentfusion_amd.pose import estimation
    assert estimation.GradientPoseEstimator(model=None, **_ARGS).per_target_plan is False
    est = estimation.GradientPoseEstimator(model=None, per_target_plan=True, **_ARGS)
    assert est.per_target_plan is True
    cfg = {'type': 'gradient', 'args': {k: v for k, v in _ARGS.items() if k != 'loss_weights'}, 'loss_weights': {'depth': 1.0}}
    assert estimation.load_from_config(cfg, None).per_target_plan is False
    cfg['args']['per_target_plan'] = True
    assert estimation.load_from_config(cfg, None).per_target_plan is True
    assert estimation.load_from_config(cfg, None, per_target_plan=False).per_target_plan is False

    # estimate_batch hands it to the engine it builds
    seen = {}

    class Stop(Exception):
        pass

    class FakeEngine(engine_multi.MultiTargetEngine):
        def __init__(self, *a, **kw):
            seen.update(kw)
            raise Stop

    class Cam:
        z_span = 1.0

        def __len__(self):
            return 2

        def zoom(self, *a):
            return self

        def to(self, dev):
            return self

    class Target:
        depth = torch.zeros(1, 1, 4, 4)

        def __len__(self):
            return 1

        def to(self, dev):
            return self

    class Model:
        photographer, input_size, camera_dist, device = None, 4, 1.0, 'cpu'

    est.model = Model()
    monkeypatch.setattr(engine_multi, 'MultiTargetEngine', FakeEngine)
    monkeypatch.setattr(est, '_multi_engine_applies', lambda z: True)
    with pytest.raises(Stop):
        est.estimate_batch(torch.zeros(1), [Target(), Target()], cameras=[Cam(), Cam()])
    assert seen['per_target_plan'] is True


def test_f16x3_is_refused_before_any_gpu_work():
    from latentfusion_amd.engine_multi import MultiTargetEngine
    from latentfusion_amd.pose import estimation
    with pytest.raises(NotImplementedError, match='batch-wide'):
        estimation.GradientPoseEstimator(model=None, per_target_plan=True, conv_mode='f16x3', **_ARGS)
    # (the engine refuses from its arguments: neither the photographer nor the volume nor a target is looked at)
    with pytest.raises(NotImplementedError, match='batch-wide'):
        MultiTargetEngine(None, None, [], {}, conv_mode='f16x3', per_target_plan=True)
    estimation.GradientPoseEstimator(model=None, per_target_plan=False, conv_mode='f16x3', **_ARGS)     # the default is untouched
