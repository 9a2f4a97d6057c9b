"""Host side of the fused training losses (ops.recon_losses, losses.HardPixelLoss `kernel`, GeneratorStep `loss_kernel`): the
wrapper's argument checks (which raise before any library call), the option values and the errors of 'fused' where it does not
apply, the composed path unchanged, the scheduled k, and the binding table.  No GPU."""
import inspect
import os
import re

import pytest
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _no_library(monkeypatch):
    from latentfusion_amd import _lib

    def no_library():
        raise AssertionError('the library was asked for')
    monkeypatch.setattr(_lib, 'lib', no_library)


def test_wrapper_checks_raise_before_any_library_call(monkeypatch):
    from latentfusion_amd import ops
    _no_library(monkeypatch)
    host = torch.zeros(2, 1, 8, 8)
    with pytest.raises(ValueError, match='device'):
        ops.recon_losses(host, host, 'l1', 4)                                    # host tensors
    with pytest.raises(ValueError, match='device'):
        ops.recon_losses(None, None, 'l1', 0, host, host, 0.01)
    with pytest.raises(ValueError):
        ops.recon_losses(host.tolist(), host, 'l1', 4)                           # not a tensor
    # the other rules on meta tensors that claim to be on the device (see tests/test_depth_init_args.py)
    monkeypatch.setattr(torch.Tensor, 'is_cuda', property(lambda self: self.device.type == 'meta'))

    def meta(*shape, dtype=torch.float32):
        return torch.empty(*shape, device='meta', dtype=dtype)
    x, z = meta(2, 1, 8, 8), meta(2, 3, 1, 8, 8)
    good = dict(x=x, y=x, base='smooth_l1', k=16, mask_logits=z, mask_target=z, beta_param=0.01)
    bad = [dict(y=meta(2, 1, 8, 9)), dict(y=meta(3, 1, 8, 8)), dict(x=meta(2, 8, 8), y=meta(2, 8, 8)),
           dict(x=meta(2, 1, 1, 8, 8), y=meta(2, 1, 1, 8, 8)), dict(x=meta(2, 5, 8, 8), y=meta(2, 5, 8, 8)),
           dict(x=meta(0, 1, 8, 8), y=meta(0, 1, 8, 8)), dict(x=meta(2, 1, 0, 8), y=meta(2, 1, 0, 8)),
           dict(x=x.to(torch.int32)), dict(y=host), dict(x=host), dict(y=None), dict(x=None),
           dict(k=-1), dict(k=65), dict(k=4.0), dict(k=None), dict(k=True),
           dict(base='huber'), dict(base='L1'), dict(base=None), dict(base=0), dict(base=nn.L1Loss),
           dict(mask_target=meta(2, 3, 1, 8, 9)), dict(mask_target=None), dict(mask_logits=None), dict(mask_target=host),
           dict(mask_logits=host), dict(mask_logits=meta(0), mask_target=meta(0)), dict(mask_logits=z.to(torch.int64)),
           dict(beta_param=None), dict(beta_param=0.0), dict(beta_param=-1.0), dict(beta_param='0.01'), dict(beta_param=True),
           dict(x=None, y=None, mask_logits=None, mask_target=None)]
    for over in bad:
        with pytest.raises(ValueError):
            ops.recon_losses(**dict(good, **over))
    # and the forms it accepts get as far as the library: both parts, either part alone, k = 0, k = H * W, 4 channels, bf16 in
    for kw in (good, dict(good, k=0), dict(good, k=64, base='l1'), dict(good, mask_logits=None, mask_target=None, beta_param=None),
               dict(good, x=None, y=None), dict(good, x=meta(2, 4, 8, 8), y=meta(2, 4, 8, 8)),
               dict(good, x=x.to(torch.bfloat16), mask_logits=z.to(torch.bfloat16))):
        with pytest.raises(AssertionError, match='the library was asked for'):
            ops.recon_losses(**kw)
    p = inspect.signature(ops.recon_losses).parameters
    assert list(p) == ['x', 'y', 'base', 'k', 'mask_logits', 'mask_target', 'beta_param']
    assert all(p[n].default is None for n in ('mask_logits', 'mask_target', 'beta_param'))


def test_option_values_and_fused_errors(monkeypatch):
    from latentfusion_amd import losses
    _no_library(monkeypatch)
    assert losses.KERNEL == 'composed' and losses.KERNELS == ('composed', 'fused')
    assert losses.select_kernel(None) == 'composed' and losses.select_kernel('fused') == 'fused'
    p = inspect.signature(losses.HardPixelLoss.__init__).parameters
    assert (p['reduction'].default, p['kernel'].default) == ('mean', None)
    assert inspect.signature(losses.get_recon_criterion).parameters['kernel'].default is None
    for bad in ('hip', 'Fused', '', 0, True):
        with pytest.raises(ValueError, match='kernel'):
            losses.HardPixelLoss(nn.L1Loss, 4, kernel=bad)
        with pytest.raises(ValueError, match='kernel'):
            losses.get_recon_criterion('hard_l1', 4, kernel=bad)
    for t in ('hard_l1', 'hard_smooth_l1'):
        assert losses.get_recon_criterion(t, 7, kernel='fused').kernel == 'fused'
        assert losses.get_recon_criterion(t, 7).kernel is None
    assert isinstance(losses.get_recon_criterion('smooth_l1', kernel='fused'), nn.SmoothL1Loss)
    # 'fused' where it does not apply: the message names the composed path
    with pytest.raises(ValueError, match='composed'):
        losses.HardPixelLoss(nn.L1Loss, 4, reduction='sum', kernel='fused')
    with pytest.raises(ValueError, match='composed'):
        losses.HardPixelLoss(nn.MSELoss, 4, kernel='fused')
    with pytest.raises(ValueError, match='composed'):
        losses.HardPixelLoss(nn.SmoothL1Loss, 4, kernel='fused', beta=0.5)
    x, y = torch.randn(2, 1, 4, 4), torch.randn(2, 1, 4, 4)
    with pytest.raises(ValueError, match='composed'):
        losses.HardPixelLoss(nn.L1Loss, 4, kernel='fused')(x, y)                 # CPU tensors
    # the module switch is read at call time and meets the same rules
    crit_sum, crit_mse, crit = (losses.HardPixelLoss(nn.L1Loss, 4, reduction='sum'), losses.HardPixelLoss(nn.MSELoss, 4),
                                losses.HardPixelLoss(nn.SmoothL1Loss, 4))
    monkeypatch.setattr(losses, 'KERNEL', 'fused')
    for c in (crit_sum, crit_mse, crit):
        with pytest.raises(ValueError, match='composed'):
            c(x, y)
    assert torch.equal(losses.HardPixelLoss(nn.SmoothL1Loss, 4, kernel='composed')(x, y),
                       torch.topk(nn.functional.smooth_l1_loss(x, y, reduction='none').mean(dim=1).reshape(2, -1), 4).values.mean())


def _parent_hard_pixel(base, x, y, k, reduction):
    """The composed chain as it stood before the switch existed, written out."""
    from latentfusion_amd.losses import reduce_loss
    x, y = x.reshape(-1, *x.shape[-3:]), y.reshape(-1, *y.shape[-3:])
    loss = base(reduction='none')(x, y)
    loss = reduce_loss(loss, dim=1, reduction=reduction).reshape(x.size(0), -1)
    loss, _ = torch.topk(loss, k=k, dim=1, largest=True)
    return reduce_loss(loss, reduction)


def test_composed_path_is_unchanged_and_k_is_read_per_call(monkeypatch):
    from latentfusion_amd import losses
    _no_library(monkeypatch)
    gen = torch.Generator().manual_seed(5)
    x = (1.5 * torch.tanh(torch.randn(2, 3, 2, 9, 11, generator=gen))).requires_grad_(True)
    y = torch.tanh(torch.randn(2, 3, 2, 9, 11, generator=gen))
    for base in (nn.L1Loss, nn.SmoothL1Loss):
        for reduction in ('mean', 'sum'):
            want = _parent_hard_pixel(base, x, y, 20, reduction)
            gw, = torch.autograd.grad(want, x)
            for kernel in (None, 'composed'):
                got = losses.HardPixelLoss(base, 20, reduction=reduction, kernel=kernel)(x, y)
                gg, = torch.autograd.grad(got, x)
                assert torch.equal(got, want) and torch.equal(gg, gw), (base.__name__, reduction, kernel)
    crit = losses.get_recon_criterion('hard_smooth_l1', 99)
    assert crit.k == 99
    for k in (99, 50, 1):                                                        # the reference halves k at its milestones
        crit.k = k
        assert torch.equal(crit(x, y), _parent_hard_pixel(nn.SmoothL1Loss, x, y, k, 'mean'))
    crit.k = 100
    with pytest.raises(RuntimeError):
        crit(x, y)                                                               # torch.topk refuses k > H * W


class _Net(nn.Module):
    def __init__(self):
        super().__init__()
        self.w = nn.Parameter(torch.zeros(3))


def test_generator_step_construction():
    from latentfusion_amd import losses
    from latentfusion_amd.recon import training
    assert inspect.signature(training.GeneratorStep.__init__).parameters['loss_kernel'].default is None
    assert training.GeneratorStep(_Net(), None, _Net()).loss_kernel == 'composed'
    assert training.GeneratorStep(_Net(), None, _Net(), loss_kernel='composed').loss_kernel == 'composed'
    for t in ('l1', 'smooth_l1', 'hard_l1', 'hard_smooth_l1'):
        step = training.GeneratorStep(_Net(), None, _Net(), loss_kernel='fused', g_depth_recon_loss_type=t, g_depth_recon_loss_k=77)
        assert step.loss_kernel == 'fused'
        assert getattr(step.depth_criterion, 'k', 77) == 77
    for bad in ('hip', 'Fused', '', 0):
        with pytest.raises(ValueError, match='loss_kernel'):
            training.GeneratorStep(_Net(), None, _Net(), loss_kernel=bad)
    for mask_type in ('l1', 'smooth_l1', 'hard_l1'):
        with pytest.raises(ValueError, match='binary_cross_entropy'):
            training.GeneratorStep(_Net(), None, _Net(), loss_kernel='fused', g_mask_recon_loss_type=mask_type)
        assert training.GeneratorStep(_Net(), None, _Net(), g_mask_recon_loss_type=mask_type).loss_kernel == 'composed'
    with pytest.raises(ValueError, match='composed'):
        training.GeneratorStep(_Net(), None, _Net(), loss_kernel='fused', g_depth_recon_loss_type='binary_cross_entropy')
    old = losses.KERNEL
    try:
        losses.KERNEL = 'fused'                                                  # None = the module switch, read at construction
        assert training.GeneratorStep(_Net(), None, _Net()).loss_kernel == 'fused'
    finally:
        losses.KERNEL = old


@pytest.mark.parametrize('tool', ['train_probe.py', 'released_train_probe.py'])
def test_tools_take_loss_kernel(tool):
    src = open(os.path.join(ROOT, 'tools', tool)).read()
    assert re.search(r"'--loss-kernel', choices=\('composed', 'fused'\), default='composed'", src)
    assert 'loss_kernel=a.loss_kernel' in src


def test_entry_points_are_bound_with_the_headers_argument_counts():
    from latentfusion_amd import _lib
    from latentfusion_amd.csrc import build
    assert 'train_loss.hip' in build.SOURCES and 'train_loss.hip' not in build.EXTRA          # the default flags only
    header = open(os.path.join(ROOT, 'include', 'lf_hip.h')).read()
    assert 'losses.py:33-57' in header and 'losses.py:94-99' in header and 'train_reconstruct.py:491-521' in header
    header = re.sub(r'/\*.*?\*/', ' ', header, flags=re.S)
    for name, arity in (('lf_recon_loss_scratch_bytes', 5), ('lf_recon_loss_fwd', 21), ('lf_recon_loss_bwd', 20)):
        proto = re.search(r'\b' + name + r'\s*\(([^)]*)\)', header)
        assert proto is not None, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(proto.group(1).split(',')) == arity, name
    assert _lib.SIGNATURES['lf_recon_loss_scratch_bytes'][0] is _lib.c_size_t
    L = _lib.lib()
    q = L.lf_recon_loss_scratch_bytes
    assert q(3, 1, 17, 23, 100) >= 3 * 17 * 23 * 4 + 3 * 8 + 16 and q(3, 1, 17, 23, 100) % 4 == 0
    assert q(3, 4, 17, 23, 0) == q(3, 1, 17, 23, 0) > 0 and q(0, 0, 0, 0, 5000) == 3 * 16
    # outside the domain: 0, decided on the host
    for args in ((0, 0, 0, 0, 0), (0, 1, 8, 8, 0), (1, 0, 8, 8, 0), (1, 5, 8, 8, 0), (1, 1, 0, 8, 0), (1, 1, 8, -1, 0),
                 (1, 1, 8, 8, -1), (1, 1, 1 << 16, 1 << 15, 0), (1 << 20, 1, 1 << 10, 1 << 10, 0), (0, 0, 0, 0, (1 << 40) + 1)):
        assert q(*args) == 0, args
    # the argument rules are decided on the host, before anything is launched: no GPU is needed to see them
    assert L.lf_recon_loss_fwd(None, None, 0, 0, None, None, 0.0, 0.0, 0.0, None, None, None, None, None, 0, 1, 1, 1, 1, 1, None) == -1
    assert L.lf_recon_loss_bwd(None, None, None, 0, 0, None, None, None, None, 0.0, 0.0, 0.0, None, None, 1, 1, 1, 1, 1, None) == -1
