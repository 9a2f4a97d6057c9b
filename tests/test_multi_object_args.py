"""CPU: the host logic of the several-objects pose loop -- per-target volume lists are validated before anything is rendered
(estimate_batch, MultiTargetEngine), volumes are de-duplicated by tensor identity, and the indexed resampler's table is range
checked on the host."""
import pytest
import torch


def _obs(h=48, w=64):
    from latentfusion_amd.modules.geometry import Camera
    from latentfusion_amd.observation import Observation
    K = torch.tensor([[500.0, 0.0, w / 2], [0.0, 500.0, h / 2], [0.0, 0.0, 1.0]]).expand(1, -1, -1)
    E = torch.eye(4).expand(1, -1, -1).clone()
    E[:, 2, 3] = 1.0
    return Observation(torch.zeros(1, 3, h, w), torch.ones(1, 1, h, w), torch.ones(1, 1, h, w), Camera(K, E, width=w, height=h))


def _cams(n):
    from latentfusion_amd.modules.geometry import Camera
    return Camera(torch.eye(3).expand(n, -1, -1), None, log_quaternion=torch.zeros(n, 3),
                  translation=torch.tensor([[0.0, 0.0, 1.0]]).expand(n, -1))


def _est(**kw):
    from latentfusion_amd.pose import estimation
    return estimation.GradientPoseEstimator(model=None, learning_rate=0.01, num_samples=4, num_iters=2, ranking_size=2,
                                            converge_threshold=1e-6, converge_patience=5,
                                            loss_weights={'depth': 1.0, 'ov_depth': 0.3, 'iou': 0.2, 'mask': 0.4}, **kw)


def _vol(S=8, C=4, dtype=torch.float32):
    return torch.zeros(1, 1, C, S, S, S, dtype=dtype)


def test_distinct_volumes_go_by_tensor_identity():
    from latentfusion_amd.engine_multi import distinct_volumes
    A, B = _vol(), _vol()
    vols, index = distinct_volumes([A, B, A, A, B])
    assert len(vols) == 2 and vols[0] is A and vols[1] is B and index == [0, 1, 0, 0, 1]
    # equal values in different tensors stay two volumes; a view is another tensor object as well
    vols, index = distinct_volumes([A, A.clone(), A.view(A.shape)])
    assert len(vols) == 3 and index == [0, 1, 2]
    assert distinct_volumes([B]) == ([B], [0])
    assert distinct_volumes([]) == ([], [])


def test_check_volumes_wants_one_like_tensor_per_target():
    from latentfusion_amd.engine_multi import check_volumes
    A, B = _vol(), _vol()
    assert check_volumes((A, B, A), 3) == [A, B, A] and check_volumes(iter([A]), 1)[0] is A
    with pytest.raises(ValueError, match='one entry per target'):
        check_volumes([A, B], 3)
    with pytest.raises(ValueError, match='one entry per target'):
        check_volumes([], 1)
    with pytest.raises(ValueError, match='differ in shape'):
        check_volumes([A, _vol(S=16)], 2)
    with pytest.raises(ValueError, match='differ in shape'):
        check_volumes([A, _vol(C=8)], 2)
    with pytest.raises(ValueError, match='dtype'):
        check_volumes([A, _vol(dtype=torch.float64)], 2)
    with pytest.raises(ValueError, match='expected a tensor'):
        check_volumes([A, None], 2)
    # the leading singleton dimensions are not part of a volume's shape
    assert len(check_volumes([A, A.reshape(1, 4, 8, 8, 8)], 2)) == 2


def test_estimate_batch_rejects_a_bad_volume_list_before_rendering():
    targets, cams = [_obs(), _obs(), _obs()], [_cams(4), _cams(4), _cams(4)]
    A, B = _vol(), _vol()
    with pytest.raises(ValueError, match='2 volumes for 3 targets'):
        _est().estimate_batch([A, B], targets, cameras=cams)
    with pytest.raises(ValueError, match='differ in shape'):
        _est().estimate_batch([A, B, _vol(S=16)], targets, cameras=cams)
    with pytest.raises(ValueError, match='expected a tensor'):
        _est().estimate_batch([A, B, 'C'], targets, cameras=cams)
    # the target / camera checks still come first, and sharding stays refused with a well-formed list
    with pytest.raises(ValueError, match='camera batches for'):
        _est().estimate_batch([A, B, A], targets, cameras=cams[:2])
    with pytest.raises(NotImplementedError):
        _est(shard_hypotheses=True).estimate_batch([A, B, A], targets, cameras=cams)


def test_multi_target_engine_rejects_a_bad_volume_list_before_building():
    from latentfusion_amd.engine_multi import MultiTargetEngine
    targets = [_obs(), _obs()]
    w = {'depth': 1.0}
    with pytest.raises(ValueError, match='one entry per target'):
        MultiTargetEngine(None, [_vol()], targets, w)
    with pytest.raises(ValueError, match='differ in shape'):
        MultiTargetEngine(None, [_vol(), _vol(S=16)], targets, w)
    with pytest.raises(ValueError, match='dtype'):
        MultiTargetEngine(None, [_vol(), _vol(dtype=torch.float16)], targets, w)


def test_volume_table_is_range_checked_on_the_host():
    from latentfusion_amd import ops
    t = ops.volume_table([2, 0, 0, 1, 2, 1, 0], 3, 'cpu')
    assert t.dtype == torch.int32 and t.tolist() == [2, 0, 0, 1, 2, 1, 0] and t.is_contiguous()
    for bad in ([0, 3], [-1, 0], [0, 1, 7]):
        with pytest.raises(ValueError, match='outside'):
            ops.volume_table(bad, 3, 'cpu')
    with pytest.raises(ValueError):
        ops.volume_table([], 3, 'cpu')
    with pytest.raises(ValueError):
        ops.volume_table([0], 0, 'cpu')


def test_indexed_entry_points_are_declared_bound_and_exported():
    """The three product entry points: in the header, in the ctypes table with the header's arity, and in the library."""
    import os
    from latentfusion_amd import _lib
    names = ('lf_resample3d_fwd_indexed', 'lf_resample3d_bwd_coef_indexed', 'lf_resample3d_bwd_coef_indexed_scratch_bytes')
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'lf_hip.h')).read()
    for n in names:
        assert n + '(' in header and n in _lib.SIGNATURES, n
    assert len(_lib.SIGNATURES['lf_resample3d_fwd_indexed'][1]) == 12
    assert len(_lib.SIGNATURES['lf_resample3d_bwd_coef_indexed'][1]) == 15
    L = _lib.lib()
    # the scratch query is host arithmetic: the partition of lf_resample3d_bwd_coef_part, 0 for an empty partition
    assert L.lf_resample3d_bwd_coef_indexed_scratch_bytes(8, 8, 128, 128, 128) == L.lf_resample3d_bwd_coef_scratch_bytes(8, 128, 128, 128)
    assert L.lf_resample3d_bwd_coef_indexed_scratch_bytes(6, 2, 32, 32, 32) == L.lf_resample3d_bwd_coef_part_scratch_bytes(6, 2, 32, 32, 32)
    assert L.lf_resample3d_bwd_coef_indexed_scratch_bytes(8, 0, 32, 32, 32) == 0
