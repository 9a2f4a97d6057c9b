"""MultiTargetEngine(per_target_plan=True) and GradientPoseEstimator(per_target_plan=True) on the released-width renderer
(golden g20: wide 3-D camera blocks and a wide 2-D decoder, engine plan _WideWinograd): three shifted targets x n = 2
perturbed hypotheses in one loop give, per target, EXACTLY what RenderLoopEngine / estimate() give on that target alone --
every wide launch takes the frequency split of one target's rows (lf_wino_fused_gemm_part).  With the default (False) the
same comparison holds only within rounding (tests/test_multi_target_engine_gpu.py); it is not asserted either way here.
The ranking form (forward only, masked depth) is exact with proj_kernel='mfma' (lf_rows_gemm_epi is row-independent) and
within the single-target tolerance close() with 'library' (the library picks its GEMM kernel by the row count)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def close(a, b, atol=1e-5, rtol=1e-4):
    torch.testing.assert_close(a.detach().cpu().contiguous(), b.detach().cpu().contiguous(), atol=atol, rtol=rtol)


def prod_camera(d, device=DEV):
    from latentfusion_amd.modules.geometry import Camera
    return Camera(d['K'].to(device), None, d['z_span'], d['viewport'].to(device), width=d['width'],
                  height=d['height'], log_quaternion=d['log_q'].to(device), translation=d['t'].to(device))


def _shifted_targets(target, shifts):
    """Different target frames of the same size: the frame rolled by (dy, dx) pixels."""
    from latentfusion_amd.observation import Observation
    out = []
    for dy, dx in shifts:
        out.append(Observation(None, torch.roll(target.depth, (dy, dx), (-2, -1)).contiguous(),
                               torch.roll(target.mask, (dy, dx), (-2, -1)).contiguous(), target.camera))
    return out


def _perturbed(cam, n, seed):
    """n hypotheses near `cam`'s first n (a different set per target), on cam's device."""
    g = torch.Generator().manual_seed(seed)
    c = cam[:n]
    dev = c.log_quaternion.device
    return c._like(log_quaternion=c.log_quaternion + 0.05 * torch.randn(c.log_quaternion.shape, generator=g).to(dev),
                   translation=c.translation + 0.005 * torch.randn(c.translation.shape, generator=g).to(dev))


def _compare(ph, z_obj, targets, cams, weights, n, exact=True, need_grad=True, masked_depth=False, **kw):
    """MultiTargetEngine(per_target_plan=True) on all rows against RenderLoopEngine per target (z_obj: a volume or one per target)."""
    from latentfusion_amd.engine import RenderLoopEngine
    from latentfusion_amd.engine_multi import MultiTargetEngine
    from latentfusion_amd.modules.geometry import Camera
    eng = MultiTargetEngine(ph, z_obj, targets, weights, per_target_plan=True, **kw)
    lm, gm = eng.forward_backward(Camera.cat(cams), n, need_grad=need_grad, masked_depth=masked_depth)
    torch.cuda.synchronize()
    assert lm.shape[0] == len(targets) * n
    for t, (tg, c) in enumerate(zip(targets, cams)):
        one = RenderLoopEngine(ph, z_obj[t] if isinstance(z_obj, list) else z_obj, tg, weights, **kw)
        l1, g1 = one.forward_backward(c, need_grad=need_grad, masked_depth=masked_depth)
        torch.cuda.synchronize()
        r = slice(t * n, (t + 1) * n)
        if need_grad:
            print(f'target {t}: max |loss diff| {(lm[r] - l1).abs().max().item():.3e}, max |grad diff| {(gm[r] - g1).abs().max().item():.3e}')
        else:
            print(f'target {t}: max |loss diff| {(lm[r] - l1).abs().max().item():.3e}')
        if exact:
            assert torch.equal(lm[r], l1), t
            if need_grad:
                assert torch.equal(gm[r], g1), t
        else:
            close(lm[r], l1)
    assert not torch.equal(lm[:n, :4], lm[n:2 * n, :4])             # the targets differ
    return eng


@functools.lru_cache(maxsize=None)
def _g20_model(golden):
    from latentfusion_amd.recon import fusion
    from latentfusion_amd.recon.inference import LatentFusionModel
    from latentfusion_amd.recon.models import Photographer, Sculptor
    g = golden('g20_released_width')
    return LatentFusionModel(Sculptor.from_checkpoint(g['sculptor']), fusion.from_checkpoint(g['fuser']),
                             Photographer.from_checkpoint(g['photographer']), g['camera_dist'], DEV)


def _g20(golden, device=DEV):
    from latentfusion_amd.observation import Observation
    g, t7 = golden('g20_released_width'), golden('g7_adam_trace')
    tg = t7['target']
    target = Observation(None, tg['depth'], tg['mask'].float(), prod_camera(tg['cam'], 'cpu')).to(device)
    return g, _g20_model(golden), _shifted_targets(target, [(0, 0), (10, 12), (-8, -6)])


def _volumes(g):
    zA = g['z_obj'].to(DEV)
    zB = torch.roll(zA, (2, -1), (-1, -2)).contiguous()
    return [zA, zB, zA]


def test_engine_with_gradients_bit_identical_per_target(golden):
    from latentfusion_amd.engine import _WideWinograd
    g, model, targets = _g20(golden)
    n = 2
    zc = prod_camera(g['loss']['zoomed'])
    cams = [_perturbed(zc, n, 50 + t) for t in range(3)]
    with model.frozen():
        eng = _compare(model.photographer, g['z_obj'].to(DEV), targets, cams, g['loss']['weights'], n)
    assert type(eng.plan) is _WideWinograd and eng.per_target_plan and eng.plan.part_n is None


@pytest.mark.parametrize('proj_kernel', ['mfma', 'library'])
def test_engine_ranking_form(golden, proj_kernel):
    g, model, targets = _g20(golden)
    n = 2
    zc = prod_camera(g['loss']['zoomed'])
    cams = [_perturbed(zc, n, 60 + t) for t in range(3)]
    with model.frozen():
        _compare(model.photographer, g['z_obj'].to(DEV), targets, cams, g['loss']['weights'], n, exact=proj_kernel == 'mfma',
                 need_grad=False, masked_depth=True, proj_kernel=proj_kernel)


def test_engine_several_objects(golden):
    g, model, targets = _g20(golden)
    n = 2
    zc = prod_camera(g['loss']['zoomed'])
    cams = [_perturbed(zc, n, 70 + t) for t in range(3)]
    with model.frozen():
        _compare(model.photographer, _volumes(g), targets, cams, g['loss']['weights'], n)


def _estimator(model, weights, **kw):
    from latentfusion_amd.pose import estimation
    args = dict(model=model, learning_rate=0.01, num_samples=2, num_iters=6, ranking_size=2, converge_threshold=-1.0,
                converge_patience=1, optimizer='adam', loss_weights=weights, track_stats=True, return_camera_history=True,
                per_target_plan=True)
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


@pytest.mark.parametrize('objects', ['one', 'ABA'])
def test_estimate_batch_equals_sequential_estimates(golden, objects):
    """3 targets x 2 hypotheses, 6 Adam iterations, convergence off, histories on."""
    g, model, targets = _g20(golden, 'cpu')
    init = prod_camera(g['loss']['init'], 'cpu')
    cams = [_perturbed(init, 2, 80 + t) for t in range(3)]
    est = _estimator(model, g['loss']['weights'])
    z = g['z_obj'].to(DEV) if objects == 'one' else _volumes(g)
    want = [est.estimate(z[t] if isinstance(z, list) else z, tg, camera=c.clone()) for t, (tg, c) in enumerate(zip(targets, cams))]
    got = est.estimate_batch(z, targets, cameras=[c.clone() for c in cams])
    assert est.last_batch_groups == [3] and len(want[0][2]) == 6
    for t, (g_, w_) in enumerate(zip(got, want)):
        print(f'target {t}: max |rank_loss diff| over the loop {(g_[1]["rank_loss"] - w_[1]["rank_loss"]).abs().max().item():.3e}')
    for g_, w_ in zip(got, want):
        _assert_same(g_, w_)


def test_f16x3_is_refused(golden):
    from latentfusion_amd.engine_multi import MultiTargetEngine
    g, model, targets = _g20(golden)
    with pytest.raises(NotImplementedError, match='batch-wide'):
        MultiTargetEngine(model.photographer, g['z_obj'].to(DEV), targets, g['loss']['weights'], conv_mode='f16x3',
                          per_target_plan=True)
    with pytest.raises(NotImplementedError, match='batch-wide'):
        _estimator(model, g['loss']['weights'], conv_mode='f16x3')


def test_option_changes_nothing_on_a_16_channel_renderer():
    from latentfusion_amd import synth
    from latentfusion_amd.engine_multi import MultiTargetEngine
    from latentfusion_amd.modules.geometry import Camera
    from latentfusion_amd.pose import estimation, utils as pu
    model, _ = synth.build_model(32, 16, 'pool:mean', seed=4, device=DEV, bias_std=0.05)
    model.freeze()
    tg0 = synth.make_observation(1, 5, DEV)
    targets = _shifted_targets(tg0, [(0, 0), (9, -14), (-7, 11)])
    z_obj = torch.randn(1, 1, 16, 32, 32, 32, generator=torch.Generator().manual_seed(9)).to(DEV)
    init = pu.sample_cameras_with_estimate(8, estimation.PoseEstimator.initial_pose(tg0))
    init = init.zoom(None, model.input_size, model.camera_dist).to(DEV)
    weights = {'depth': 1.0, 'ov_depth': 0.3, 'iou': 0.2, 'mask': 0.4}
    n = 3
    cams = Camera.cat([_perturbed(init, n, 20 + t) for t in range(3)])
    out = []
    for flag in (False, True):
        eng = MultiTargetEngine(model.photographer, z_obj, targets, weights, per_target_plan=flag)
        assert not eng.plan.wide
        l, gp = eng.forward_backward(cams, n)
        lr, _ = eng.forward_backward(cams, n, need_grad=False, masked_depth=True)
        torch.cuda.synchronize()
        out.append((l, gp, lr))
    assert all(torch.equal(a, b) for a, b in zip(*out))
