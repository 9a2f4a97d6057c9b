"""The render-and-score engine over several target frames of one object in one batch.

T targets x n hypotheses, grouped by target (row i belongs to target i // n), run through ONE sequence of launches of
RenderLoopEngine.  Everything below the loss already works per hypothesis; what is per target here:
  * the pose loss reads each row's own target frame (lf_pose_loss_fwd_mt / _fwd_masked_mt / _bwd_mt) and its sums'
    gradients are those of the mean over the row's own target, so the optimised quantity is sum_t mean_{i in t} total_i;
  * the coefficient gradient of the resampler sums each row as a launch of n rows would (lf_resample3d_bwd_coef_part with
    part_n = n): its fixed-order block partition no longer follows the batch size;
  * the latent term's cosine distance is evaluated per target slice.
So per target the losses and camera gradients are bit-identical to RenderLoopEngine on that target's n rows alone for the
kernels whose per-sample arithmetic does not depend on the batch.  Exceptions (tests/test_multi_target_engine_gpu.py names
their tolerances): conv_mode 'f16x3' (batch-wide gradient scales) and every renderer with wide (>= 64-channel) layers, the
released architecture included: lf_wino_fused_gemm picks its workgroup configuration (pick_fused_cfg) and its frequency
split (fused_zsplit) from the batch's tile count N x tiles, so a row's summation order follows the batch size.
"""
import torch

from . import _lib, ops
from ._lib import check
from .engine import RenderLoopEngine, _PoseLoss, _pose_loss_bwd, _pose_loss_fwd, _s


class MultiTargetEngine(RenderLoopEngine):
    """RenderLoopEngine for T single-frame targets of the same object and frame size, n hypotheses each.

    forward_backward(camera, n) takes the T * n cameras grouped by target and returns the single-target engine's layout:
    (losses (T*n, 8), gparams (T*n, 10) or None), gparams = d(sum_t mean over target t's rows of the weighted loss).
    Batch size: MAX_ROWS = 65535 rows, the grid limit of the launches that give every row a grid row (the loss passes,
    lf_pose_loss_bwd_rows / _cols); a call above it is refused with a ValueError, and GradientPoseEstimator.estimate_batch
    splits its targets into groups of whole targets below it.  Every other per-batch limit (tile counts x N within 2^31,
    32-bit offsets inside a slab) is checked by the kernels themselves, which reject an unsafe shape with LF_EINVAL
    (LFHipError here), as they do for RenderLoopEngine: this engine accepts what n rows per target need whenever the
    single-target engine accepts n."""

    MAX_ROWS = 65535

    def __init__(self, photographer, z_obj, targets, loss_weights, conv_mode='auto', fuse_projection=None):
        targets = list(targets)
        if not targets:
            raise ValueError('MultiTargetEngine needs at least one target')
        for i, t in enumerate(targets):
            if len(t) != 1:
                raise ValueError(f'target {i} holds {len(t)} frames: every target is one single-frame Observation')
        sizes = {tuple(t.depth.shape[-2:]) for t in targets}
        if len(sizes) != 1:
            raise ValueError(f'the targets differ in frame size: {sorted(sizes)}')
        if conv_mode not in RenderLoopEngine.CONV_MODES:
            # (e.g. 'winograd_f16x3' of experimental.RenderLoopEngineX)
            raise NotImplementedError(f'conv_mode {conv_mode!r}: the multi-target engine runs {RenderLoopEngine.CONV_MODES}')
        if fuse_projection is True or (isinstance(fuse_projection, (tuple, list, set)) and 'bwd' in fuse_projection):
            raise NotImplementedError('the fused projection backward is an experimental.RenderLoopEngineX option')
        super().__init__(photographer, z_obj, targets[0], loss_weights, conv_mode=conv_mode, fuse_projection=fuse_projection)
        dev = self.dev
        # one resident [T][H*W] buffer each (raw device pointers reach the kernels: nothing host-resident)
        self.tdepth = torch.stack([t.depth.reshape(-1).float().to(dev) for t in targets]).contiguous()
        self.tmask = torch.stack([t.mask.reshape(-1).float().to(dev) for t in targets]).contiguous()
        self.T = len(targets)
        self._n = None
        self._max_batch = self.MAX_ROWS

    def max_batch(self):
        """Largest number of rows (targets x hypotheses) one call may carry (MAX_ROWS)."""
        return self._max_batch

    def set_streams(self, k):
        raise NotImplementedError('hypothesis groups on several streams are an experimental.RenderLoopEngineX option')

    def forward_backward_graph(self, camera, params):
        raise NotImplementedError('hipGraph replay is an experimental.RenderLoopEngineX option')

    def forward_backward(self, camera, n, need_grad=True, z_target_latent=None, params=None, masked_depth=False):
        """camera: T * n hypotheses grouped by target; z_target_latent: (T * n, ...) rows grouped alike, or (T, ...) one code per
        target.  Returns (losses (T*n, 8), gparams (T*n, 10) or None) as RenderLoopEngine.forward_backward."""
        n = int(n)
        N = len(camera) if params is None else params.shape[0]
        if n < 1 or N != self.T * n:
            raise ValueError(f'{N} hypotheses are not {self.T} targets x n = {n}')
        if N > self._max_batch:
            raise ValueError(f'{N} rows exceed the largest batch this renderer can launch ({self._max_batch}): '
                             'split the targets into smaller groups')
        if z_target_latent is not None and z_target_latent.shape[0] != N:
            if z_target_latent.shape[0] != self.T:
                raise ValueError(f'z_target_latent has {z_target_latent.shape[0]} rows: expected {N} or {self.T}')
            z_target_latent = z_target_latent.repeat_interleave(n, dim=0)
        self._n = n
        try:
            return RenderLoopEngine.forward_backward(self, camera, need_grad, z_target_latent, params, masked_depth)
        finally:
            self._n = None

    # ---- the per-target pieces ----
    def _loss_fwd(self, lg, coefs, masked_depth):
        return _pose_loss_fwd(lg, coefs, self.tdepth, self.tmask, self.weights, self.H, self.W, masked_depth, (self.T, self._n))

    def _loss_bwd(self, lg, coefs, gsums, glogits, g_cf, scratch):
        _pose_loss_bwd(lg, coefs, self.tdepth, self.tmask, gsums, glogits, g_cf, scratch, self.H, self.W, (self.T, self._n))

    def _loss_autograd(self, logits, coefs):
        # (_PoseLoss over [T][H*W] target frames: d(total) is taken per row)
        return _PoseLoss.apply(logits, coefs, self.tdepth, self.tmask, self.weights, self.H, self.W, (self.T, self._n))

    def _objective(self, total):
        # sum over the targets of each target's mean: every row's gradient is what its own single-target loop sees
        return total.view(self.T, self._n).mean(dim=1).sum()

    def _latent_distance(self, zp, zt, n):
        # (one cosine distance per target slice: the same reductions, over the same shapes, as the single-target engine)
        k = self._n
        return torch.cat([RenderLoopEngine._latent_distance(self, zp[t * k:(t + 1) * k], zt[t * k:(t + 1) * k], k)
                          for t in range(self.T)])

    def _bwd_coef(self, g, cf20, gcoef18, n):
        L = _lib.lib()
        S = self.S
        nbytes = L.lf_resample3d_bwd_coef_part_scratch_bytes(n, self._n, S, S, S)
        scratch = torch.empty(nbytes // 4 + 1, device=self.dev, dtype=torch.float32)
        with ops._timed('resample_bwd_coef'):
            check(L.lf_resample3d_bwd_coef_part(g.data_ptr(), self.z.data_ptr(), 1, cf20.data_ptr(), gcoef18.data_ptr(),
                                                scratch.data_ptr(), scratch.numel() * 4, n, S, S, S, self.C, self._n, _s()),
                  'lf_resample3d_bwd_coef_part')
