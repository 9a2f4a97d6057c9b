"""The generator training step (recon/training.GeneratorStep; reference tools/train/train_reconstruct.py:421-535) on the
RELEASED architecture (synth.build_released_model: 256^2 inputs, 16^3 x 256 volume, 515 -> 256 ConvGRU gates, 512-channel
U-Net levels, 68 M parameters), where every wide weight gradient runs on lf_conv_bwd_weight_wide.

1 object, 2 input + 1 output views (one ConvGRU step with gradients), the trainer's hard smooth-L1 depth and BCE mask losses
x 25 as in g27, against the oracle's step (nets.encode + nets.decode + the same losses) on the CPU from the same checkpoints:
  fp32      loss terms to 1e-4 relative, every parameter's gradient to 1 % rel-L2, whole-vector cosine > 0.9999 (g27's bounds);
  autocast  finite losses and gradients; whole-gradient cosine with the oracle's fp32 gradient >= the cosine the oracle's own
            torch.autocast('cpu', bfloat16) step reaches - 0.03 (g27's rule).
Plus: a SYN(32,16) step (no layer of it routes to the wide kernel) gives bit-identical gradients with WIDE_WGRAD on and off.

CPU oracle wall time (fp32 and bf16 steps together): about 4 s on 8 threads."""
import pytest
import torch
import torch.nn.functional as F

import lf_oracle as O
from lf_oracle import nets

pytestmark = pytest.mark.gpu
DEV = 'cuda'
W_DEPTH = W_MASK = 25.0


def _obs(model, n, seed):
    from latentfusion_amd import synth
    return model.preprocess_observation(synth.make_observation(n, seed=seed, device=DEV))


def _ocam(cam):
    cam = cam.to('cpu')
    return O.Cam(cam.intrinsic, cam.log_quaternion, cam.translation, viewport=cam.viewport, z_span=cam.z_span, width=cam.width,
                 height=cam.height)


@pytest.fixture(scope='module')
def released():
    """(model, checkpoints, input / output observations, oracle results {fp32, bf16}: (loss terms, {(k, name): grad}))."""
    from latentfusion_amd import losses as L, synth
    torch.set_num_threads(min(16, torch.get_num_threads()))
    model, (sck, fck, pck, dist) = synth.build_released_model(device=DEV, seed=0)
    oi, oo = _obs(model, 2, 1), _obs(model, 1, 2)
    cks = {k: {**ck, 'state_dict': {n: v.clone().requires_grad_(True) for n, v in ck['state_dict'].items()}}
           for k, ck in (('s', sck), ('f', fck), ('p', pck))}
    cin, cout = _ocam(oi.camera), _ocam(oo.camera)
    depth_t, mask_t = oo.depth.unsqueeze(0).cpu(), oo.mask.unsqueeze(0).cpu()
    S = model.photographer.output_size if hasattr(model.photographer, 'output_size') else 256

    def oracle(autocast):
        for ck in cks.values():
            for v in ck['state_dict'].values():
                v.grad = None
        with torch.autocast('cpu', dtype=torch.bfloat16, enabled=autocast):
            z = nets.encode(cks['s'], cks['f'], cin, oi.color.cpu(), None, oi.mask.cpu())
            y, _, _ = nets.decode(cks['p'], z, cout, apply_mask=False)
        l_depth = L.reduce_loss(L.get_recon_criterion('hard_smooth_l1', S * S // 4)(y['depth'].float(), depth_t))
        l_mask = L.reduce_loss(L.get_recon_criterion('binary_cross_entropy')(y['mask_logits'].float(), mask_t))
        (W_DEPTH * l_depth + W_MASK * l_mask).backward()
        return ({'depth_recon': float(l_depth), 'mask_recon': float(l_mask)},
                {(k, n): v.grad.clone() for k, ck in cks.items() for n, v in ck['state_dict'].items() if v.grad is not None})
    ref = {'fp32': oracle(False), 'bf16': oracle(True)}
    return model, oi, oo, S, ref


def _hip_step(model, oi, oo, S, amp):
    from latentfusion_amd.recon import training
    step = training.GeneratorStep(model.sculptor, model.fuser, model.photographer, g_depth_recon_loss_k=S * S // 4, use_amp=amp,
                                  g_depth_recon_loss_weight=W_DEPTH, g_mask_recon_loss_weight=W_MASK)
    batch = {'in': {'camera': oi.camera, 'image': oi.color.unsqueeze(0), 'mask': oi.mask.unsqueeze(0)},
             'out_gt': {'camera': oo.camera, 'depth': oo.depth.unsqueeze(0), 'mask': oo.mask.unsqueeze(0)}}
    out = step.run_iteration(batch, is_step=False)
    torch.cuda.synchronize()
    mods = {'s': model.sculptor, 'f': model.fuser, 'p': model.photographer}
    got = {(k, n): p.grad.detach().cpu().clone() for k, m in mods.items() for n, p in m.named_parameters() if p.grad is not None}
    return {k: float(v) for k, v in out.items()}, got


def _cat(d, keys):
    return torch.cat([d[k].reshape(-1) for k in keys]).double()


def _wide_launched(fn):
    from latentfusion_amd import _lib
    _lib.BYTE_LOG = {}
    try:
        r = fn()
        log = dict(_lib.BYTE_LOG)
    finally:
        _lib.BYTE_LOG = None
    return r, log


def test_released_step_fp32_against_the_oracle(released):
    model, oi, oo, S, ref = released
    (loss, got), log = _wide_launched(lambda: _hip_step(model, oi, oo, S, False))
    assert log.get('lf_conv_bwd_weight_wide', [0])[0] >= 30, log.get('lf_conv_bwd_weight_wide')
    want_loss, want = ref['fp32']
    for k in ('depth_recon', 'mask_recon'):
        assert abs(loss[k] - want_loss[k]) < 1e-4 * abs(want_loss[k]), (k, loss[k], want_loss[k])
    assert set(want) <= set(got), set(want) - set(got)
    for key, w in want.items():
        rel = float((got[key] - w).norm() / w.norm().clamp_min(1e-30))
        assert rel < 1e-2, (key, rel)
    keys = sorted(want)
    assert F.cosine_similarity(_cat(got, keys), _cat(want, keys), dim=0).item() > 0.9999


def test_released_step_autocast_against_the_oracle(released):
    model, oi, oo, S, ref = released
    (loss, got), log = _wide_launched(lambda: _hip_step(model, oi, oo, S, True))
    assert log.get('lf_conv_bwd_weight_wide', [0])[0] >= 30, log.get('lf_conv_bwd_weight_wide')
    assert all(torch.isfinite(torch.tensor(v)) for v in loss.values()), loss
    assert all(bool(torch.isfinite(g).all()) for g in got.values())
    _, g32 = ref['fp32']
    _, g16 = ref['bf16']
    keys = sorted(g32)
    cos_hip = F.cosine_similarity(_cat(got, keys), _cat(g32, keys), dim=0).item()
    cos_orc = F.cosine_similarity(_cat(g16, keys), _cat(g32, keys), dim=0).item()
    print(f'released autocast: cos(HIP bf16 grad, oracle fp32 grad) {cos_hip:.4f}; oracle bf16 {cos_orc:.4f}')
    assert cos_hip > cos_orc - 0.03, (cos_hip, cos_orc)


def test_syn_step_unchanged_by_the_wide_switch():
    """SYN(32,16): every weight gradient keeps its 16-channel kernel, so the switch changes no bit of the step's gradients."""
    from latentfusion_amd import ops_train, synth
    from latentfusion_amd.recon import training
    S = 32
    model, _ = synth.build_model(S, 16, 'gru', seed=0, device=DEV, bias_std=0.1)
    oi, oo = _obs(model, 4, 1), _obs(model, 2, 2)
    batch = {'in': {'camera': oi.camera, 'image': oi.color.unsqueeze(0), 'mask': oi.mask.unsqueeze(0)},
             'out_gt': {'camera': oo.camera, 'depth': oo.depth.unsqueeze(0), 'mask': oo.mask.unsqueeze(0)}}
    saved = ops_train.WIDE_WGRAD
    try:
        for amp in (False, True):
            step = training.GeneratorStep(model.sculptor, model.fuser, model.photographer, g_depth_recon_loss_k=S * S // 4, use_amp=amp)
            grads = []
            for on in (True, False):
                ops_train.WIDE_WGRAD = on
                _, log = _wide_launched(lambda: step.run_iteration(batch, is_step=False))
                torch.cuda.synchronize()
                assert 'lf_conv_bwd_weight_wide' not in log
                grads.append(step.flat.grad.clone())
            assert torch.equal(grads[0], grads[1]), amp
    finally:
        ops_train.WIDE_WGRAD = saved
