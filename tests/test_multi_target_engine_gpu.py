"""engine_multi.MultiTargetEngine: T = 3 targets x n hypotheses in one call against RenderLoopEngine once per target.
Losses and camera gradients are BIT-identical for the kernels whose per-hypothesis arithmetic does not depend on the batch
(the loss and the coefficient gradient are partitioned per target by construction); the two documented exceptions are
checked at the single-target tests' tolerances:
  * the wide ranking-only path (no gradient): its factor projection is a library GEMM whose kernel choice follows M = N S^2,
    so the summation order of a row can change with the batch -- test_engine_gpu.py's close() (atol 1e-5, rtol 1e-4);
  * conv_mode 'f16x3': the gradients' power-of-two scales come from a max over the whole batch, so a row's split operands
    depend on its batch mates -- losses at close(), gradients at the batch-partition tolerance of
    test_engine_hypothesis_groups_on_streams_are_bit_identical (atol 1e-6 max|g|, rtol 2e-5);
  * the released-width renderer (golden g20) with gradients, like every renderer with wide (>= 64-channel) layers: its
    wide 3-D blocks and wide 2-D decoder layers run on lf_wino_fused_gemm, which picks its workgroup configuration
    (pick_fused_cfg, wino_fused.hip) and its frequency split (wino_ring::Plan::split) from T = N x tiles, so a row's summation order
    changes with the batch size and the forward already differs in the last bits -- losses at close(), gradients at
    atol 2e-3 max|g|, rtol 2e-5 (one evaluation; measured 1.1e-4 absolute on a largest component of 0.19).  Over a loop
    Adam amplifies such differences: estimate_batch does not reproduce estimate on these renderers."""
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
    """n hypotheses near `cam`'s first n (a different set per target)."""
    g = torch.Generator().manual_seed(seed)
    c = cam[:n]
    return c._like(log_quaternion=c.log_quaternion + 0.05 * torch.randn(c.log_quaternion.shape, generator=g).to(DEV),
                   translation=c.translation + 0.005 * torch.randn(c.translation.shape, generator=g).to(DEV))


def _compare(ph, z_obj, targets, cams, weights, n, exact=True, need_grad=True, masked_depth=False, gtol=None, **kw):
    from latentfusion_amd.engine import RenderLoopEngine
    from latentfusion_amd.engine_multi import MultiTargetEngine
    from latentfusion_amd.modules.geometry import Camera
    eng = MultiTargetEngine(ph, z_obj, targets, weights, **kw)
    allc = Camera.cat(cams)
    lm, gm = eng.forward_backward(allc, n, need_grad=need_grad, masked_depth=masked_depth)
    torch.cuda.synchronize()
    assert lm.shape[0] == len(targets) * n
    for t, (tg, c) in enumerate(zip(targets, cams)):
        one = RenderLoopEngine(ph, z_obj, tg, weights, **kw)
        l1, g1 = one.forward_backward(c, need_grad=need_grad, masked_depth=masked_depth)
        torch.cuda.synchronize()
        r = slice(t * n, (t + 1) * n)
        if exact:
            assert torch.equal(lm[r], l1), t
            if need_grad:
                assert torch.equal(gm[r], g1), t
        else:
            close(lm[r], l1)
            if need_grad:
                close(gm[r], g1, atol=gtol * g1.abs().max().item(), rtol=2e-5)
    # the targets differ: row groups scored against one frame would not reproduce the per-target results
    assert not torch.equal(lm[:n, :4], lm[n:2 * n, :4]) or n == 0
    return eng, lm, gm


def _syn():
    from latentfusion_amd import synth
    from latentfusion_amd.pose import estimation
    model, _ = synth.build_model(32, 16, 'pool:mean', seed=4, device=DEV, bias_std=0.05)
    model.freeze()
    tg0 = synth.make_observation(1, 5, DEV)
    targets = _shifted_targets(tg0, [(0, 0), (9, -14), (-7, 11)])
    z_obj = torch.randn(1, 1, 16, 32, 32, 32, generator=torch.Generator().manual_seed(9)).to(DEV)
    from latentfusion_amd.pose import utils as pu
    init = pu.sample_cameras_with_estimate(8, estimation.PoseEstimator.initial_pose(tg0))
    init = init.zoom(None, model.input_size, model.camera_dist).to(DEV)
    return model, z_obj, targets, init


@pytest.mark.parametrize('conv_mode,n', [('winograd', 1), ('winograd', 4), ('fp32', 3)])
def test_syn_engine_bit_identical_per_target(conv_mode, n):
    model, z_obj, targets, init = _syn()
    weights = {'depth': 1.0, 'ov_depth': 0.3, 'iou': 0.2, 'mask': 0.4}
    cams = [_perturbed(init, n, 20 + t) for t in range(3)]
    eng, lm, gm = _compare(model.photographer, z_obj, targets, cams, weights, n, conv_mode=conv_mode)
    assert eng.conv_mode == conv_mode
    # the ranking form (forward only, masked depth) as well
    _compare(model.photographer, z_obj, targets, cams, weights, n, need_grad=False, masked_depth=True, conv_mode=conv_mode)


def test_syn_engine_f16x3_within_single_target_tolerance():
    model, z_obj, targets, init = _syn()
    weights = {'depth': 1.0, 'ov_depth': 0.3, 'iou': 0.2, 'mask': 0.4}
    n = 3
    cams = [_perturbed(init, n, 30 + t) for t in range(3)]
    _compare(model.photographer, z_obj, targets, cams, weights, n, exact=False, gtol=1e-6, conv_mode='f16x3')


def test_occlusion_renderer_g28_bit_identical_per_target(golden):
    from latentfusion_amd.observation import Observation
    from latentfusion_amd.recon.models import Photographer
    g = golden('g28_occlusion16')
    ph = Photographer.from_checkpoint(g['variants']['factor']['photographer']).to(DEV)
    for p in ph.parameters():
        p.requires_grad_(False)
    tg = g['target']
    target = Observation(None, tg['depth'], tg['mask'].float(), prod_camera(tg['cam'], 'cpu')).to(DEV)
    targets = _shifted_targets(target, [(0, 0), (6, 8), (-5, -9)])
    init = prod_camera(g['init']).zoom(None, g['S'], g['camera_dist'])
    n = 2
    cams = [_perturbed(init, n, 40 + t) for t in range(3)]
    eng, _, _ = _compare(ph, g['z_obj'].to(DEV), targets, cams, dict(g['cfg']['loss_weights']), n)
    assert eng.occ is not None


def _g20(golden):
    from latentfusion_amd.observation import Observation
    from latentfusion_amd.recon import fusion
    from latentfusion_amd.recon.inference import LatentFusionModel
    from latentfusion_amd.recon.models import Photographer, Sculptor
    g, t7 = golden('g20_released_width'), golden('g7_adam_trace')
    model = LatentFusionModel(Sculptor.from_checkpoint(g['sculptor']), fusion.from_checkpoint(g['fuser']),
                              Photographer.from_checkpoint(g['photographer']), g['camera_dist'], DEV)
    tg = t7['target']
    target = Observation(None, tg['depth'], tg['mask'].float(), prod_camera(tg['cam'], 'cpu')).to(DEV)
    return g, model, _shifted_targets(target, [(0, 0), (10, 12), (-8, -6)]), prod_camera(g['loss']['zoomed'])


def test_wide_branch_g20_with_gradients_within_rounding_per_target(golden):
    g, model, targets, zc = _g20(golden)
    n = 2
    cams = [_perturbed(zc, n, 50 + t) for t in range(3)]
    with model.frozen():
        eng, _, _ = _compare(model.photographer, g['z_obj'].to(DEV), targets, cams, g['loss']['weights'], n, exact=False,
                             gtol=2e-3)
    from latentfusion_amd.engine import _WideWinograd
    assert type(eng.plan) is _WideWinograd


def test_wide_branch_g20_ranking_within_single_target_tolerance(golden):
    g, model, targets, zc = _g20(golden)
    n = 2
    cams = [_perturbed(zc, n, 60 + t) for t in range(3)]
    with model.frozen():
        _compare(model.photographer, g['z_obj'].to(DEV), targets, cams, g['loss']['weights'], n, exact=False, need_grad=False,
                 masked_depth=True)


def test_multi_target_engine_arguments():
    model, z_obj, targets, init = _syn()
    from latentfusion_amd.engine_multi import MultiTargetEngine
    from latentfusion_amd.modules.geometry import Camera
    from latentfusion_amd.observation import Observation
    weights = {'depth': 1.0, 'ov_depth': 0.3, 'iou': 0.2, 'mask': 0.4}
    eng = MultiTargetEngine(model.photographer, z_obj, targets, weights)
    cams = Camera.cat([init[:2]] * 3)
    with pytest.raises(ValueError):
        eng.forward_backward(cams, 3)                               # 6 rows are not 3 targets x 3
    with pytest.raises(NotImplementedError):
        MultiTargetEngine(model.photographer, z_obj, targets, weights, conv_mode='winograd_f16x3')
    with pytest.raises(NotImplementedError):
        MultiTargetEngine(model.photographer, z_obj, targets, weights, fuse_projection=('fwd', 'bwd'))
    with pytest.raises(NotImplementedError):
        eng.set_streams(2)
    assert eng.max_batch() >= 64
    eng._max_batch = 5                                               # (a renderer whose largest batch is 5 rows)
    with pytest.raises(ValueError, match='largest batch'):
        eng.forward_backward(cams, 2)
    cropped = Observation(None, targets[0].depth[..., :-1], targets[0].mask[..., :-1], targets[0].camera)
    with pytest.raises(ValueError, match='frame size'):
        MultiTargetEngine(model.photographer, z_obj, [targets[0], cropped], weights)
