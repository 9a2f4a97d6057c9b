"""GradientPoseEstimator.estimate_batch over several objects: estimate_batch([zA, zB, zA], targets) in ONE batched loop
returns EXACTLY what the three estimate(z_t, target_t) calls return -- best cameras (and so the ranking), stat_history and
camera_history -- with one target converging early, with a latent term, and on the module-path fallback; 2 objects x 8
hypotheses at the headline shape run as one loop."""
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
    """Two SYN(32,16) objects fused from different reference views; z_objs = [A, B, A] for three shifted target frames."""
    from latentfusion_amd import synth
    from latentfusion_amd.pose import estimation, utils as pu
    model, _ = synth.build_model(32, 16, fuser, seed=4, device=DEV, bias_std=0.05)
    with torch.no_grad():
        zA = model.build_latent_object(synth.make_observation(4, 21, DEV))
        zB = model.build_latent_object(synth.make_observation(4, 22, DEV))
    assert not torch.equal(zA, zB)
    tg0 = synth.make_observation(1, 5, 'cpu')
    targets = [_shifted(tg0, 0, 0), _shifted(tg0, 9, -14), _shifted(tg0, -7, 11)]
    cams = []
    for t, tg in enumerate(targets):
        c = pu.sample_cameras_with_estimate(4, estimation.PoseEstimator.initial_pose(tg))
        g = torch.Generator().manual_seed(70 + t)
        cams.append(c._like(log_quaternion=c.log_quaternion + 0.05 * torch.randn(c.log_quaternion.shape, generator=g)))
    return model, [zA, zB, zA], targets, cams


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


def _sequential(est, zs, targets, cams):
    return [est.estimate(z, t, camera=c) for z, t, c in zip(zs, targets, _clone(cams))]


def test_estimate_batch_over_objects_equals_the_sequential_estimates():
    model, zs, targets, cams = _setup()
    est = _estimator(model)
    want = _sequential(est, zs, targets, cams)
    got = est.estimate_batch(zs, targets, cameras=_clone(cams))
    assert est.last_batch_groups == [3]                               # one loop
    for g, w in zip(got, want):
        _assert_same(g, w)
    # the objects matter: target 0 refined against B does not give target 0's result against A
    other = est.estimate(zs[1], targets[0], camera=cams[0].clone())
    assert not torch.equal(other[1]['rank_loss'], want[0][1]['rank_loss'])


def test_estimate_batch_over_objects_with_an_early_converging_target():
    model, zs, targets, cams = _setup()
    probe = _estimator(model)
    deltas = [r[1]['delta'][1:].tolist() for r in _sequential(probe, zs, targets, cams)]
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
    want = _sequential(est, zs, targets, cams)
    got = est.estimate_batch(zs, targets, cameras=_clone(cams))
    lengths = [len(w[2]) for w in want]
    assert min(lengths) < 8 and len(set(lengths)) > 1, lengths          # one target stopped early, the others went on
    for g, w in zip(got, want):
        _assert_same(g, w)


def test_estimate_batch_over_objects_with_a_latent_term():
    model, zs, targets, cams = _setup('gru')
    w = {'depth': 1.0, 'ov_depth': 0.3, 'iou': 0.0, 'mask': 0.0, 'latent': 0.2}
    est = _estimator(model, loss_weights=w, num_iters=4)
    want = _sequential(est, zs, targets, cams)
    got = est.estimate_batch(zs, targets, cameras=_clone(cams))
    assert 'latent_loss' in want[0][1]
    for g, w_ in zip(got, want):
        _assert_same(g, w_)


def test_estimate_batch_over_objects_module_path_fallback_and_arguments():
    model, zs, targets, cams = _setup()
    est = _estimator(model, use_engine=False, num_iters=3)
    want = _sequential(est, zs, targets, cams)
    got = est.estimate_batch(zs, targets, cameras=_clone(cams))
    assert est.last_batch_groups == [1, 1, 1]
    for g, w in zip(got, want):
        _assert_same(g, w)
    with pytest.raises(ValueError, match='one entry per target'):
        est.estimate_batch(zs[:2], targets, cameras=_clone(cams))
    with pytest.raises(NotImplementedError):
        _estimator(model, shard_hypotheses=True).estimate_batch(zs, targets, cameras=_clone(cams))


def test_estimate_batch_runs_2_objects_x8_at_the_headline_shape_as_one_loop():
    """SYN(128,16) (the headline renderer), 2 objects x 8 hypotheses: ONE batched loop of 16 rows over two resident volumes,
    and exactly the two sequential estimates."""
    from latentfusion_amd import synth
    from latentfusion_amd.pose import estimation, utils as pu
    model, _ = synth.build_model(128, 16, 'pool:mean', seed=2, device=DEV, bias_std=0.05)
    tg0 = synth.make_observation(1, 5, 'cpu')
    targets = [_shifted(tg0, 0, 0), _shifted(tg0, 12, -9)]
    zs = [torch.randn(1, 1, 16, 128, 128, 128, generator=torch.Generator().manual_seed(s)).to(DEV) for s in (3, 4)]
    cams = [pu.sample_cameras_with_estimate(8, estimation.PoseEstimator.initial_pose(t)) for t in targets]
    est = _estimator(model, num_samples=8, num_iters=3, ranking_size=4)
    want = _sequential(est, zs, targets, cams)
    got = est.estimate_batch(zs, targets, cameras=_clone(cams))
    assert est.last_batch_groups == [2]
    for g, w in zip(got, want):
        _assert_same(g, w)
