"""GradientPoseEstimator.estimate_batch: T = 3 targets in one batched loop returns EXACTLY what three sequential estimate()
calls return -- best cameras (and so the ranking), stat_history (every loss term, the rank loss, convergence counters) and
camera_history -- with one target converging early, with a latent term, and on the module-path fallback."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _shifted(target, dy, dx):
    from latentfusion_amd.observation import Observation
    return Observation(torch.roll(target.color, (dy, dx), (-2, -1)).contiguous(),
                       torch.roll(target.depth, (dy, dx), (-2, -1)).contiguous(),
                       torch.roll(target.mask, (dy, dx), (-2, -1)).contiguous(), target.camera.clone())


def _setup(fuser='pool:mean'):
    from latentfusion_amd import synth
    from latentfusion_amd.pose import estimation, utils as pu
    model, _ = synth.build_model(32, 16, fuser, seed=4, device=DEV, bias_std=0.05)
    tg0 = synth.make_observation(1, 5, 'cpu')
    targets = [_shifted(tg0, 0, 0), _shifted(tg0, 9, -14), _shifted(tg0, -7, 11)]
    z_obj = torch.randn(1, 1, 16, 32, 32, 32, generator=torch.Generator().manual_seed(9)).to(DEV)
    cams = []
    for t, tg in enumerate(targets):
        c = pu.sample_cameras_with_estimate(4, estimation.PoseEstimator.initial_pose(tg))
        g = torch.Generator().manual_seed(70 + t)
        cams.append(c._like(log_quaternion=c.log_quaternion + 0.05 * torch.randn(c.log_quaternion.shape, generator=g)))
    return model, z_obj, targets, cams


def _estimator(model, **kw):
    from latentfusion_amd.pose import estimation
    args = dict(model=model, learning_rate=0.01, num_samples=4, num_iters=8, ranking_size=3, converge_threshold=-1.0,
                converge_patience=1, optimizer='adam', loss_weights={'depth': 1.0, 'ov_depth': 0.3, 'iou': 0.2, 'mask': 0.4},
                track_stats=True, return_camera_history=True)
    args.update(kw)
    return estimation.GradientPoseEstimator(**args)


def _assert_same(got, want):
    best_g, stats_g, hist_g = got
    best_w, stats_w, hist_w = want
    for f in ('log_quaternion', 'translation', 'viewport', 'intrinsic'):
        assert torch.equal(getattr(best_g, f), getattr(best_w, f)), f
    assert set(stats_g) == set(stats_w)
    for k in stats_w:
        assert torch.equal(stats_g[k], stats_w[k]), k
    assert len(hist_g) == len(hist_w)
    for (rg, cg), (rw, cw) in zip(hist_g, hist_w):
        assert torch.equal(rg, rw)
        assert torch.equal(cg.log_quaternion, cw.log_quaternion) and torch.equal(cg.translation, cw.translation)


def _clone(cams):
    return [c.clone() for c in cams]


def test_estimate_batch_equals_sequential_with_an_early_converging_target():
    model, z_obj, targets, cams = _setup()
    # calibration: the per-step improvements of every target's best loss, no convergence
    probe = _estimator(model)
    deltas = [probe.estimate(z_obj, t, camera=c)[1]['delta'][1:].tolist() for t, c in zip(targets, _clone(cams))]
    # a threshold under which (patience 1) some target converges at an earlier step than another one
    thr = None
    for cand in sorted({d for ds in deltas for d in ds if d > 0}):
        th = cand * (1 + 1e-4)
        first = [next((s for s, d in enumerate(ds) if d < th), None) for ds in deltas]
        if any(f is not None and f < len(deltas[0]) - 1 for f in first) and len(set(first)) > 1:
            thr = th
            break
    assert thr is not None, deltas
    est = _estimator(model, converge_threshold=thr)
    want = [est.estimate(z_obj, t, camera=c) for t, c in zip(targets, _clone(cams))]
    got = est.estimate_batch(z_obj, targets, cameras=_clone(cams))
    lengths = [len(w[2]) for w in want]
    assert min(lengths) < 8 and len(set(lengths)) > 1, lengths          # one target stopped early, the others went on
    for g, w in zip(got, want):
        _assert_same(g, w)


def test_estimate_batch_equals_sequential_with_a_latent_term():
    model, z_obj, targets, cams = _setup('gru')
    w = {'depth': 1.0, 'ov_depth': 0.3, 'iou': 0.0, 'mask': 0.0, 'latent': 0.2}
    est = _estimator(model, loss_weights=w, num_iters=4)
    want = [est.estimate(z_obj, t, camera=c) for t, c in zip(targets, _clone(cams))]
    got = est.estimate_batch(z_obj, targets, cameras=_clone(cams))
    assert 'latent_loss' in want[0][1]
    for g, w_ in zip(got, want):
        _assert_same(g, w_)


def test_estimate_batch_module_path_fallback_and_drawn_cameras():
    model, z_obj, targets, cams = _setup()
    est = _estimator(model, use_engine=False, num_iters=3)
    want = [est.estimate(z_obj, t, camera=c) for t, c in zip(targets, _clone(cams))]
    got = est.estimate_batch(z_obj, targets, cameras=_clone(cams))
    for g, w in zip(got, want):
        _assert_same(g, w)
    # cameras=None: initial_pose + sample_cameras_with_estimate per target, in target order, on the engine
    est = _estimator(model, num_iters=3, track_stats=False, return_camera_history=False)
    torch.manual_seed(0)
    want = [est.estimate(z_obj, t) for t in targets]
    torch.manual_seed(0)
    got = est.estimate_batch(z_obj, targets)
    for g, w in zip(got, want):
        assert torch.equal(g.log_quaternion, w.log_quaternion) and torch.equal(g.translation, w.translation)


def test_estimate_batch_of_one_target_equals_estimate():
    """T = 1 through the batched driver: the same loop as estimate(), on MultiTargetEngine with one record."""
    model, z_obj, targets, cams = _setup()
    est = _estimator(model, num_iters=3)
    want = est.estimate(z_obj, targets[0], camera=cams[0].clone())
    got = est.estimate_batch(z_obj, targets[:1], cameras=[cams[0].clone()])
    assert est.last_batch_groups == [1] and len(got) == 1
    _assert_same(got[0], want)


def test_estimate_batch_refuses_sharding():
    model, z_obj, targets, cams = _setup()
    est = _estimator(model, shard_hypotheses=True)
    with pytest.raises(NotImplementedError):
        est.estimate_batch(z_obj, targets, cameras=cams)


def test_estimate_batch_runs_2x8_at_the_headline_shape_as_one_loop():
    """SYN(128,16) (the headline renderer), 2 targets x 8 hypotheses: ONE batched loop of 16 rows (not two single-target
    loops), and exactly the two sequential estimates."""
    from latentfusion_amd import synth
    from latentfusion_amd.pose import estimation, utils as pu
    model, _ = synth.build_model(128, 16, 'pool:mean', seed=2, device=DEV, bias_std=0.05)
    tg0 = synth.make_observation(1, 5, 'cpu')
    targets = [_shifted(tg0, 0, 0), _shifted(tg0, 12, -9)]
    z_obj = torch.randn(1, 1, 16, 128, 128, 128, generator=torch.Generator().manual_seed(3)).to(DEV)
    cams = [pu.sample_cameras_with_estimate(8, estimation.PoseEstimator.initial_pose(t)) for t in targets]
    est = _estimator(model, num_samples=8, num_iters=3, ranking_size=4)
    want = [est.estimate(z_obj, t, camera=c) for t, c in zip(targets, _clone(cams))]
    got = est.estimate_batch(z_obj, targets, cameras=_clone(cams))
    assert est.last_batch_groups == [2]
    for g, w in zip(got, want):
        _assert_same(g, w)
