"""engine_multi.MultiTargetEngine over SEVERAL objects: z_obj = [A, B, A], one volume per target, in one call against
RenderLoopEngine on that (object, target) pair alone.  Losses and camera gradients are BIT-identical wherever the
one-object multi-target engine is (16-channel renderers in conv_mode 'winograd' / 'fp32', the occlusion renderer); conv_mode
'f16x3' and the wide g20 renderer are held to exactly the tolerances tests/test_multi_target_engine_gpu.py names for them
(close() on losses; gradients at atol 1e-6 / 2e-3 x max|g|, rtol 2e-5), for the same reason: batch-dependent summation.
The iteration issues the launches of the one-object engine, entry point by entry point, except that the two resampler
launches are the indexed ones."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
WEIGHTS = {'depth': 1.0, 'ov_depth': 0.3, 'iou': 0.2, 'mask': 0.4}
RENAMED = {'lf_resample3d_fwd': 'lf_resample3d_fwd_indexed', 'lf_resample3d_bwd_coef_part': 'lf_resample3d_bwd_coef_indexed'}


def close(a, b, atol=1e-5, rtol=1e-4):
    torch.testing.assert_close(a.detach().cpu().contiguous(), b.detach().cpu().contiguous(), atol=atol, rtol=rtol)


def prod_camera(d, device=DEV):
    from latentfusion_amd.modules.geometry import Camera
    return Camera(d['K'].to(device), None, d['z_span'], d['viewport'].to(device), width=d['width'],
                  height=d['height'], log_quaternion=d['log_q'].to(device), translation=d['t'].to(device))


def _shifted_targets(target, shifts):
    from latentfusion_amd.observation import Observation
    return [Observation(None, torch.roll(target.depth, (dy, dx), (-2, -1)).contiguous(),
                        torch.roll(target.mask, (dy, dx), (-2, -1)).contiguous(), target.camera) for dy, dx in shifts]


def _perturbed(cam, n, seed):
    g = torch.Generator().manual_seed(seed)
    c = cam[:n]
    return c._like(log_quaternion=c.log_quaternion + 0.05 * torch.randn(c.log_quaternion.shape, generator=g).to(DEV),
                   translation=c.translation + 0.005 * torch.randn(c.translation.shape, generator=g).to(DEV))


def _compare(ph, z_objs, targets, cams, weights, n, exact=True, gtol=None, **kw):
    """The multi-object engine on (z_objs[t], targets[t]) rows against RenderLoopEngine per pair."""
    from latentfusion_amd.engine import RenderLoopEngine
    from latentfusion_amd.engine_multi import MultiTargetEngine
    from latentfusion_amd.modules.geometry import Camera
    eng = MultiTargetEngine(ph, z_objs, targets, weights, **kw)
    lm, gm = eng.forward_backward(Camera.cat(cams), n)
    torch.cuda.synchronize()
    assert lm.shape[0] == len(targets) * n
    for t, (z, tg, c) in enumerate(zip(z_objs, targets, cams)):
        l1, g1 = RenderLoopEngine(ph, z, tg, weights, **kw).forward_backward(c)
        torch.cuda.synchronize()
        r = slice(t * n, (t + 1) * n)
        if exact:
            assert torch.equal(lm[r], l1), t
            assert torch.equal(gm[r], g1), t
        else:
            close(lm[r], l1)
            close(gm[r], g1, atol=gtol * g1.abs().max().item(), rtol=2e-5)
    return eng, lm, gm


def _syn():
    """Two SYN(32,16) objects fused from different reference views, three shifted target frames."""
    from latentfusion_amd import synth
    from latentfusion_amd.pose import estimation, utils as pu
    model, _ = synth.build_model(32, 16, 'pool:mean', seed=4, device=DEV, bias_std=0.05)
    model.freeze()
    with torch.no_grad():
        zA = model.build_latent_object(synth.make_observation(4, 21, DEV))
        zB = model.build_latent_object(synth.make_observation(4, 22, DEV))
    assert zA.shape == zB.shape and not torch.equal(zA, zB)
    tg0 = synth.make_observation(1, 5, DEV)
    targets = _shifted_targets(tg0, [(0, 0), (9, -14), (-7, 11)])
    init = pu.sample_cameras_with_estimate(8, estimation.PoseEstimator.initial_pose(tg0))
    init = init.zoom(None, model.input_size, model.camera_dist).to(DEV)
    return model, zA, zB, targets, init


@pytest.mark.parametrize('conv_mode', ['winograd', 'fp32'])
@pytest.mark.parametrize('n', [1, 4])
def test_syn_objects_a_b_a_bit_identical_per_object_and_target(conv_mode, n):
    from latentfusion_amd.engine import RenderLoopEngine
    model, zA, zB, targets, init = _syn()
    cams = [_perturbed(init, n, 20 + t) for t in range(3)]
    eng, lm, gm = _compare(model.photographer, [zA, zB, zA], targets, cams, WEIGHTS, n, conv_mode=conv_mode)
    assert eng.conv_mode == conv_mode
    assert eng.zs.shape[0] == 2 and eng.vol_of == [0, 1, 0]           # A is resident once
    # the objects differ: target 0's rows rendered from B do not reproduce the rows rendered from A
    lB, gB = RenderLoopEngine(model.photographer, zB, targets[0], WEIGHTS, conv_mode=conv_mode).forward_backward(cams[0])
    torch.cuda.synchronize()
    assert not torch.equal(lm[:n], lB) and not torch.equal(gm[:n], gB)


def test_syn_objects_f16x3_within_the_multi_target_tolerance():
    model, zA, zB, targets, init = _syn()
    n = 3
    cams = [_perturbed(init, n, 30 + t) for t in range(3)]
    _compare(model.photographer, [zA, zB, zA], targets, cams, WEIGHTS, n, exact=False, gtol=1e-6, conv_mode='f16x3')


def test_occlusion_renderer_g28_two_objects_bit_identical(golden):
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
    zA = g['z_obj'].to(DEV)
    zB = torch.roll(zA, (3, -2), (-1, -3)).contiguous()              # a second object: the first one's volume displaced
    n = 2
    cams = [_perturbed(init, n, 40 + t) for t in range(3)]
    eng, _, _ = _compare(ph, [zA, zB, zA], targets, cams, dict(g['cfg']['loss_weights']), n)
    assert eng.occ is not None


def test_wide_branch_g20_two_objects_within_the_multi_target_tolerance(golden):
    from latentfusion_amd.engine import _WideWinograd
    from latentfusion_amd.observation import Observation
    from latentfusion_amd.recon import fusion
    from latentfusion_amd.recon.inference import LatentFusionModel
    from latentfusion_amd.recon.models import Photographer, Sculptor
    g, t7 = golden('g20_released_width'), golden('g7_adam_trace')
    model = LatentFusionModel(Sculptor.from_checkpoint(g['sculptor']), fusion.from_checkpoint(g['fuser']),
                              Photographer.from_checkpoint(g['photographer']), g['camera_dist'], DEV)
    tg = t7['target']
    target = Observation(None, tg['depth'], tg['mask'].float(), prod_camera(tg['cam'], 'cpu')).to(DEV)
    targets = _shifted_targets(target, [(0, 0), (10, 12), (-8, -6)])
    zc = prod_camera(g['loss']['zoomed'])
    zA = g['z_obj'].to(DEV)
    zB = torch.roll(zA, (2, -1), (-1, -2)).contiguous()
    n = 2
    cams = [_perturbed(zc, n, 50 + t) for t in range(3)]
    with model.frozen():
        eng, _, _ = _compare(model.photographer, [zA, zB, zA], targets, cams, g['loss']['weights'], n, exact=False, gtol=2e-3)
    assert type(eng.plan) is _WideWinograd


def test_a_one_element_list_equals_the_tensor_form():
    from latentfusion_amd.engine_multi import MultiTargetEngine
    model, zA, zB, targets, init = _syn()
    n = 4
    cam = _perturbed(init, n, 60)
    lt, gt = MultiTargetEngine(model.photographer, zA, targets[:1], WEIGHTS).forward_backward(cam, n)
    ll, gl = MultiTargetEngine(model.photographer, [zA], targets[:1], WEIGHTS).forward_backward(cam, n)
    torch.cuda.synchronize()
    assert torch.equal(ll, lt) and torch.equal(gl, gt)
    # and the ranking form (forward only, masked depth)
    lt, _ = MultiTargetEngine(model.photographer, zB, targets[:1], WEIGHTS).forward_backward(cam, n, need_grad=False, masked_depth=True)
    ll, _ = MultiTargetEngine(model.photographer, [zB], targets[:1], WEIGHTS).forward_backward(cam, n, need_grad=False, masked_depth=True)
    torch.cuda.synchronize()
    assert torch.equal(ll, lt)


def _launches(eng, cam, n):
    """{entry point: launches} of one steady-state iteration (the second call), counted by _lib.BYTE_LOG as
    tools/engine_parity.py does."""
    from latentfusion_amd import _lib
    eng.forward_backward(cam, n)
    torch.cuda.synchronize()
    _lib.BYTE_LOG = {}
    try:
        eng.forward_backward(cam, n)
        torch.cuda.synchronize()
        return {k: v[0] for k, v in _lib.BYTE_LOG.items()}
    finally:
        _lib.BYTE_LOG = None


@pytest.mark.parametrize('n', [1, 4])
def test_k_objects_issue_the_launches_of_one_object(n):
    from latentfusion_amd.engine_multi import MultiTargetEngine
    from latentfusion_amd.modules.geometry import Camera
    model, zA, zB, targets, init = _syn()
    cam = Camera.cat([_perturbed(init, n, 70 + t) for t in range(3)])
    one = _launches(MultiTargetEngine(model.photographer, zA, targets, WEIGHTS), cam, n)
    many = _launches(MultiTargetEngine(model.photographer, [zA, zB, zA], targets, WEIGHTS), cam, n)
    assert set(RENAMED) <= set(one) and not set(RENAMED.values()) & set(one)
    assert many == {RENAMED.get(k, k): v for k, v in one.items()}
    assert many['lf_resample3d_fwd_indexed'] == 1 and many['lf_resample3d_bwd_coef_indexed'] == 1


def test_multi_object_engine_arguments():
    from latentfusion_amd.engine_multi import MultiTargetEngine
    model, zA, zB, targets, init = _syn()
    ph = model.photographer
    with pytest.raises(ValueError, match='one entry per target'):
        MultiTargetEngine(ph, [zA, zB], targets, WEIGHTS)             # 2 volumes, 3 targets
    with pytest.raises(ValueError, match='differ in shape'):
        MultiTargetEngine(ph, [zA, zB[..., :16, :16, :16].contiguous(), zA], targets, WEIGHTS)
    with pytest.raises(ValueError, match='differ in shape'):
        MultiTargetEngine(ph, [zA, zB.double(), zA], targets, WEIGHTS)
    with pytest.raises(ValueError, match='differ in shape'):
        MultiTargetEngine(ph, [zA, zB.cpu(), zA], targets, WEIGHTS)
    eng = MultiTargetEngine(ph, [zA, zB, zB], targets, WEIGHTS)
    assert eng.zs.shape[0] == 2 and eng.vol_of == [0, 1, 1]
    eng.forward_backward(_cat3(init, 2), 2)
    eng.forward_backward(_cat3(init, 2), 2)
    assert list(eng._tables) == [2]                                   # the table is built once per n
    with pytest.raises(ValueError):
        eng.forward_backward(_cat3(init, 2), 3)                       # 6 rows are not 3 targets x 3


def _cat3(init, n):
    from latentfusion_amd.modules.geometry import Camera
    return Camera.cat([init[:n]] * 3)
