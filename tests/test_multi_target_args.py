"""CPU: GradientPoseEstimator.estimate_batch validates its targets and cameras before anything is rendered."""
import pytest
import torch


def _obs(h=48, w=64, frames=1):
    from latentfusion_amd.modules.geometry import Camera
    from latentfusion_amd.observation import Observation
    K = torch.tensor([[500.0, 0.0, w / 2], [0.0, 500.0, h / 2], [0.0, 0.0, 1.0]]).expand(frames, -1, -1)
    E = torch.eye(4).expand(frames, -1, -1).clone()
    E[:, 2, 3] = 1.0
    return Observation(torch.zeros(frames, 3, h, w), torch.ones(frames, 1, h, w), torch.ones(frames, 1, h, w),
                       Camera(K, E, width=w, height=h))


def _cams(n):
    from latentfusion_amd.modules.geometry import Camera
    return Camera(torch.eye(3).expand(n, -1, -1), None, log_quaternion=torch.zeros(n, 3),
                  translation=torch.tensor([[0.0, 0.0, 1.0]]).expand(n, -1))


def _est():
    from latentfusion_amd.pose import estimation
    return estimation.GradientPoseEstimator(model=None, learning_rate=0.01, num_samples=4, num_iters=2, ranking_size=2,
                                            converge_threshold=1e-6, converge_patience=5,
                                            loss_weights={'depth': 1.0, 'ov_depth': 0.3, 'iou': 0.2, 'mask': 0.4})


def test_estimate_batch_rejects_mismatched_lengths():
    with pytest.raises(ValueError, match='camera batches for'):
        _est().estimate_batch(None, [_obs(), _obs()], cameras=[_cams(4)])


def test_estimate_batch_rejects_unequal_camera_counts():
    with pytest.raises(ValueError, match='same number of hypotheses'):
        _est().estimate_batch(None, [_obs(), _obs()], cameras=[_cams(4), _cams(3)])


def test_estimate_batch_rejects_different_frame_sizes():
    with pytest.raises(ValueError, match='frame size'):
        _est().estimate_batch(None, [_obs(), _obs(h=40)], cameras=[_cams(4), _cams(4)])


def test_estimate_batch_rejects_a_multi_frame_target():
    with pytest.raises(ValueError, match='one frame per target'):
        _est().estimate_batch(None, [_obs(), _obs(frames=2)], cameras=[_cams(4), _cams(4)])


def test_estimate_batch_rejects_an_empty_target_list():
    with pytest.raises(ValueError):
        _est().estimate_batch(None, [])


def test_batch_groups_keep_realistic_batches_in_one_loop():
    """The grouping is decided by the rows one loop can carry (MultiTargetEngine.MAX_ROWS, the loss passes' grid rows),
    not by a per-sample bound: the headline's 8 x 8 and the 16-hypothesis presets' 8 x 16 run as ONE loop."""
    from latentfusion_amd.engine_multi import MultiTargetEngine
    from latentfusion_amd.pose.estimation import GradientPoseEstimator
    groups = GradientPoseEstimator._batch_groups
    assert MultiTargetEngine.MAX_ROWS == 65535
    for T, n in ((2, 8), (8, 8), (8, 16), (3, 1), (64, 128)):
        assert groups(T, n) == [(0, T)], (T, n)
    assert groups(3, 30000) == [(0, 2), (2, 3)]                      # whole targets per loop
    assert groups(5, 65535) == [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5)]
    with pytest.raises(ValueError):
        groups(2, 65536)
