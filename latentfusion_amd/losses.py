"""Reconstruction losses of the generator's training step (latentfusion/losses.py:33-103,
latentfusion/trainutils.py:102-133): hard-pixel mining over a base loss, the reductions, the Beta prior
on the predicted mask, and the criterion / optimiser factories with the reference's names and defaults."""
import torch
from torch import nn, optim


def reduce_loss(loss, reduction='mean', dim=None):
    """losses.py:59-72."""
    if reduction is None:
        return loss
    if reduction == 'mean':
        return loss.mean() if dim is None else loss.mean(dim=dim)
    if reduction == 'sum':
        return loss.sum() if dim is None else loss.sum(dim=dim)
    raise ValueError(f'Unknown reduction {reduction!r}')


# How the training losses are evaluated: 'composed' = the ATen chain below (the default, CPU and device alike); 'fused' = the HIP
# kernels of ops.recon_losses (device tensors only, opt-in through `kernel=` / GeneratorStep's `loss_kernel=`)
KERNEL = 'composed'
KERNELS = ('composed', 'fused')


def select_kernel(kernel, name='kernel'):
    """`kernel` or, for None, the module switch; anything else than the two names is a ValueError."""
    kernel = KERNEL if kernel is None else kernel
    if not isinstance(kernel, str) or kernel not in KERNELS:
        raise ValueError(f'{name} {kernel!r}: one of {KERNELS}')
    return kernel


def fused_base(base_loss):
    """The name ops.recon_losses knows a base-loss module by, or None when the fused kernels do not provide it."""
    if type(base_loss) is nn.L1Loss:
        return 'l1'
    if type(base_loss) is nn.SmoothL1Loss and base_loss.beta == 1.0:
        return 'smooth_l1'
    return None


class HardPixelLoss(nn.Module):
    """Mean (or sum) of the k largest per-pixel losses of every image (losses.py:33-56): the base loss is
    evaluated per element, reduced over channels, and the k hardest pixels of each (B*V) image are kept.
    kernel: None (= KERNEL), 'composed' or 'fused' (ops.recon_losses: device tensors, reduction='mean', L1 or smooth-L1 with
    beta 1).  `k` is read at every call, so a trainer may schedule it."""

    def __init__(self, base_loss, k, reduction='mean', kernel=None, **kwargs):
        super().__init__()
        self.base_loss = base_loss(reduction='none', **kwargs)
        self.k = k
        self.reduction = reduction
        self.kernel = None if kernel is None else select_kernel(kernel)
        if self.kernel == 'fused':
            self._fused_base()

    def _fused_base(self):
        base = fused_base(self.base_loss)
        if self.reduction != 'mean' or base is None:
            raise ValueError(f"kernel='fused' provides reduction='mean' over nn.L1Loss or nn.SmoothL1Loss (beta 1), not "
                             f"reduction={self.reduction!r} over {type(self.base_loss).__name__}: use the composed path "
                             f"(kernel='composed')")
        return base

    def forward(self, x, y):
        if x.dim() > 4:
            x = x.reshape(-1, *x.shape[-3:])
        if y.dim() > 4:
            y = y.reshape(-1, *y.shape[-3:])
        if x.dim() != 4:
            raise ValueError('x must be in BCHW format')
        if y.dim() != 4:
            raise ValueError('y must be in BCHW format')
        if select_kernel(self.kernel) == 'fused':
            base = self._fused_base()
            if not (x.is_cuda and y.is_cuda):
                raise ValueError("kernel='fused' needs device tensors: on the CPU use the composed path (kernel='composed')")
            from . import ops
            return ops.recon_losses(x, y, base, self.k)[0]
        loss = self.base_loss(x, y)
        loss = reduce_loss(loss, dim=1, reduction=self.reduction).reshape(x.size(0), -1)
        loss, _ = torch.topk(loss, k=self.k, dim=1, largest=True)
        return reduce_loss(loss, self.reduction)


def lsgan_loss(input, target, reduction='mean'):
    """Least-squares GAN loss (losses.py:75-77)."""
    return reduce_loss((input.squeeze() - target) ** 2, reduction=reduction)


def multiscale_lsgan_loss(inputs, target, reduction='mean'):
    loss = 0
    for x in inputs:
        loss = loss + lsgan_loss(x, target, reduction)
    return loss


def _log_beta(alpha, beta):
    alpha, beta = torch.tensor(alpha), torch.tensor(beta)
    return torch.lgamma(alpha) + torch.lgamma(beta) - torch.lgamma(alpha + beta)


def beta_prior_loss(tensor, alpha, beta, reduction='mean', eps=1e-4):
    """Negative log-density of Beta(alpha, beta) clamped at 0 (losses.py:94-100)."""
    loss = ((alpha - 1.0) * torch.log(tensor.clamp(min=eps)) + (beta - 1.0) * torch.log((1.0 - tensor).clamp(min=eps))
            - _log_beta(alpha, beta).to(tensor.device))
    return reduce_loss((-loss).clamp(min=0), reduction=reduction)


def get_recon_criterion(loss_type, k=2000, kernel=None):
    """trainutils.py:114-133 (the VGG perceptual variant needs torchvision weights and is not provided).  kernel: passed on to
    HardPixelLoss; the other criteria are plain torch modules."""
    select_kernel(kernel)
    if loss_type == 'smooth_l1':
        return nn.SmoothL1Loss()
    if loss_type == 'l1':
        return nn.L1Loss()
    if loss_type == 'hard_l1':
        return HardPixelLoss(nn.L1Loss, k=k, kernel=kernel)
    if loss_type == 'hard_smooth_l1':
        return HardPixelLoss(nn.SmoothL1Loss, k=k, kernel=kernel)
    if loss_type == 'binary_cross_entropy':
        return nn.BCEWithLogitsLoss(reduction='none')
    raise ValueError(f'Unknown recon_loss_type {loss_type!r}.')


def get_optimizer(parameters, name, lr):
    """trainutils.py:102-111: note the GAN-style betas (0.0, 0.99)."""
    if name == 'adam':
        return optim.Adam(parameters, lr=lr, betas=(0.0, 0.99))
    if name == 'adamw':
        return optim.AdamW(parameters, lr=lr, betas=(0.0, 0.99))
    if name == 'sgd':
        return optim.SGD(parameters, lr=lr)
    raise ValueError(f'Unknown optimizer {name!r}')
