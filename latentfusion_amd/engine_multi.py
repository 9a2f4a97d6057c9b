"""The render-and-score engine over several target frames in one batch: frames of one object, or of several objects.

T targets x n hypotheses, grouped by target (row i belongs to target i // n), run through ONE sequence of launches of
RenderLoopEngine.  Everything below the loss already works per hypothesis; what is per target here:
  * the pose loss reads each row's own target frame (lf_pose_loss_fwd_mt / _fwd_masked_mt / _bwd_mt) and its sums'
    gradients are those of the mean over the row's own target, so the optimised quantity is sum_t mean_{i in t} total_i;
  * the coefficient gradient of the resampler sums each row as a launch of n rows would (lf_resample3d_bwd_coef_part with
    part_n = n): its fixed-order block partition no longer follows the batch size;
  * the latent term's cosine distance is evaluated per target slice (latent_kernel 'autograd'), or for all T * n rows in one
    lf_latent_cosine_fwd launch ('fused': that kernel's partial sums follow the row's shape only, never the batch), its
    gradient scaled by 1 / n of the row's own target.
So per target the losses and camera gradients are bit-identical to RenderLoopEngine on that target's n rows alone for the
kernels whose per-sample arithmetic does not depend on the batch.  On renderers with wide (>= 64-channel) layers, the released
architecture included, that needs per_target_plan=True: lf_wino_fused_gemm picks its frequency split
(wino_ring::Plan::split, csrc/wino_ring.h) from the batch's tile count N x tiles, so by default a row's summation order
follows the batch size; with the option every wide launch takes the split of ONE target's rows (lf_wino_fused_gemm_part).
Exceptions that remain (tests/test_multi_target_engine_gpu.py, tests/test_multi_target_part_plan_gpu.py name their
tolerances): conv_mode 'f16x3' (batch-wide input and gradient scales; refused with per_target_plan) and the ranking form's
factor projection with proj_kernel 'library' (the library picks its GEMM kernel by the row count; 'mfma' is row-independent).

Several objects (a scene's frame holds a few, each with its own latent volume): `z_obj` is then a sequence of T volumes, one
per target.  Nothing below the resampler is per object -- camera blocks, projection, decoder, loss and optimiser work per row
with shared weights -- so the only change to an iteration is that the two resampler launches take a per-row table of volumes
(lf_resample3d_fwd_indexed, lf_resample3d_bwd_coef_indexed: the one-volume kernels' source compiled a second time with the
table lookup, csrc/resample_gather.inc); per row they are bit-identical to the one-volume entry points on that row's volume, so everything above holds per (object, target) as it does per target.
"""
import torch

from . import _lib, ops
from .engine import LF_MAP_O2C, RenderLoopEngine, _PoseLoss, _pose_loss_bwd, _pose_loss_fwd


def distinct_volumes(z_objs):
    """(volumes, index): the distinct tensor OBJECTS of a sequence in order of first appearance, and for every entry its
    position among them.  Identity, not value: the caller that passes one tensor for three frames of an object says so by
    passing the same tensor, and comparing 128 MiB volumes element by element is not a constructor's business."""
    vols, index, seen = [], [], {}
    for z in z_objs:
        k = seen.get(id(z))
        if k is None:
            k = seen[id(z)] = len(vols)
            vols.append(z)
        index.append(k)
    return vols, index


def check_volumes(z_objs, num_targets):
    """Argument check of a per-target volume list (engine and estimator): one tensor per target, alike in shape, dtype and
    device."""
    z_objs = list(z_objs)
    if len(z_objs) != num_targets:
        raise ValueError(f'{len(z_objs)} volumes for {num_targets} targets: a volume list holds one entry per target')
    for i, z in enumerate(z_objs):
        if not isinstance(z, torch.Tensor):
            raise ValueError(f'volume {i} is a {type(z).__name__}: expected a tensor')
        if z.dim() < 4:
            raise ValueError(f'volume {i} has shape {tuple(z.shape)}: expected (.., C, S, S, S)')
    kinds = {(tuple(z.shape[-4:]), z.dtype, z.device) for z in z_objs}
    if len(kinds) != 1:
        raise ValueError('the volumes differ in shape, dtype or device: ' + ', '.join(
            f'{shape} {dtype} {dev}' for shape, dtype, dev in sorted(kinds, key=str)))
    return z_objs


class MultiTargetEngine(RenderLoopEngine):
    """RenderLoopEngine for T single-frame targets of the same frame size, n hypotheses each.

    z_obj: one volume shared by all targets (the one-object form: one resident volume and the one-volume resampler entry
    points, as before), or a sequence of T volumes of one shape, dtype and device, entry t the object of target t.  Entries
    that are the same tensor object share one resident copy ("3 frames of A, 2 of B" keeps two volumes), and the renderer's
    object-frame blocks run once per distinct volume.  Resident memory grows by one volume per distinct object: 128 MiB each
    at SYN(128,16) (16 channels x 128^3 fp32).  The per-row table of volumes is built once per n.

    forward_backward(camera, n) takes the T * n cameras grouped by target and returns the single-target engine's layout:
    (losses (T*n, 8), gparams (T*n, 10) or None), gparams = d(sum_t mean over target t's rows of the weighted loss).
    Batch size: MAX_ROWS = 65535 rows, the grid limit of the launches that give every row a grid row (the loss passes,
    lf_pose_loss_bwd_rows / _cols); a call above it is refused with a ValueError, and GradientPoseEstimator.estimate_batch
    splits its targets into groups of whole targets below it.  Every other per-batch limit (tile counts x N within 2^31,
    32-bit offsets inside a slab) is checked by the kernels themselves, which reject an unsafe shape with LF_EINVAL
    (LFHipError here), as they do for RenderLoopEngine: this engine accepts what n rows per target need whenever the
    single-target engine accepts n."""

    MAX_ROWS = 65535

    def __init__(self, photographer, z_obj, targets, loss_weights, conv_mode='auto', fuse_projection=None, proj_kernel=None,
                 per_target_plan=False, latent_kernel=None):
        """per_target_plan: every fp32 wide (>= 64-channel) Winograd launch of a call -- the camera blocks' convolutions and data
        gradients, and the 2-D decoder's under ops.wide_parts -- takes the frequency split of a launch of ONE target's n rows
        (lf_wino_fused_gemm_part, part_n = n), so on wide renderers too every target's losses and camera gradients are
        bit-identical to RenderLoopEngine on its rows alone.  False (default): the batch's own plan, as before.  On a renderer
        without wide layers the option changes nothing; with conv_mode 'f16x3' it is refused (NotImplementedError): that
        form's input and gradient scales are maxima over the whole batch, which no launch plan undoes.
        latent_kernel: as RenderLoopEngine's; 'fused' evaluates the latent term of all T * n rows in one launch, bit-identical
        per target to RenderLoopEngine(latent_kernel='fused') on that target's rows."""
        self.per_target_plan = bool(per_target_plan)
        if self.per_target_plan and conv_mode == 'f16x3':
            raise NotImplementedError("per_target_plan with conv_mode 'f16x3': the split-precision kernels scale their inputs and "
                                      'gradients by batch-wide maxima, so a per-target launch plan would not reproduce the '
                                      'single-target loop')
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
        vols = index = None
        if isinstance(z_obj, (list, tuple)):
            vols, index = distinct_volumes(check_volumes(z_obj, len(targets)))
            z_obj = vols[0]
        super().__init__(photographer, z_obj, targets[0], loss_weights, conv_mode=conv_mode, fuse_projection=fuse_projection,
                         proj_kernel=proj_kernel, latent_kernel=latent_kernel)
        dev = self.dev
        # several objects: the distinct volumes back to back [K][S][S][S][C], self.z the first of them (a view: no second copy)
        self.zs = self.vol_of = None
        if vols is not None:
            self.zs = ops.cl(torch.cat([self.z] + [self._resident_volume(photographer, z) for z in vols[1:]]))
            self.z = self.zs[:1]
            self.vol_of = index
            self._tables = {}
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
        part = n if self.per_target_plan else None
        if part is not None and self.plan.wide:
            self.plan.part_n = part                              # the camera blocks' launches (engine._WideWinograd)
        try:
            with ops.wide_parts(part):                            # the decoder's wide 2-D layers (ops._Conv3x3), forward and backward
                return RenderLoopEngine.forward_backward(self, camera, need_grad, z_target_latent, params, masked_depth)
        finally:
            self._n = None
            if self.plan.wide:
                self.plan.part_n = None

    # ---- the per-target pieces ----
    def _loss_fwd(self, lg, coefs, masked_depth):
        return _pose_loss_fwd(lg, coefs, self.tdepth, self.tmask, self.weights, self.H, self.W, 'masked' if masked_depth else 'logits',
                              (self.T, self._n))

    def _loss_bwd(self, lg, coefs, gsums, glogits, g_cf, scratch):
        _pose_loss_bwd(lg, coefs, self.tdepth, self.tmask, gsums, glogits, g_cf, scratch, self.H, self.W, (self.T, self._n))

    def _loss_autograd(self, logits, coefs):
        # (_PoseLoss over [T][H*W] target frames: d(total) is taken per row)
        return _PoseLoss.apply(logits, coefs, self.tdepth, self.tmask, self.weights, self.H, self.W, (self.T, self._n))

    def _objective(self, total):
        # sum over the targets of each target's mean: every row's gradient is what its own single-target loop sees
        return total.view(self.T, self._n).mean(dim=1).sum()

    def _mean_rows(self, n):
        return self._n

    def _latent_distance(self, zp, zt, n):
        # (one cosine distance per target slice: the same reductions, over the same shapes, as the single-target engine)
        k = self._n
        return torch.cat([RenderLoopEngine._latent_distance(self, zp[t * k:(t + 1) * k], zt[t * k:(t + 1) * k], k)
                          for t in range(self.T)])

    def _table(self, rows):
        """Volume of every row (n rows per target, grouped by target) as the device table of the indexed resampler."""
        n = self._n
        if rows != self.T * n:
            raise ValueError(f'{rows} rows are not {self.T} targets x n = {n}')
        if n not in self._tables:
            self._tables[n] = ops.volume_table([k for k in self.vol_of for _ in range(n)], self.zs.shape[0], self.dev)
        return self._tables[n]

    def _resample(self, cf20, n):
        if self.zs is None:
            return RenderLoopEngine._resample(self, cf20, n)
        S = self.S
        x0 = ops.empty_cl((n, self.C, S, S, S), self.dev)
        table = self._table(n)
        ops.launch('lf_resample3d_fwd_indexed', self.zs.data_ptr(), self.zs.shape[0], table.data_ptr(), cf20.data_ptr(), LF_MAP_O2C,
                   x0.data_ptr(), n, S, S, S, self.C, tag='resample_fwd')
        return x0

    def _bwd_coef(self, g, cf20, gcoef18, n):
        # (one path: a table of volumes only chooses the entry point, its scratch rule and how the volume is named)
        L = _lib.lib()
        S = self.S
        if self.zs is None:
            name, vol = 'lf_resample3d_bwd_coef_part', (self.z.data_ptr(), 1)
        else:
            name, vol = 'lf_resample3d_bwd_coef_indexed', (self.zs.data_ptr(), self.zs.shape[0], self._table(n).data_ptr())
        nbytes = getattr(L, name + '_scratch_bytes')(n, self._n, S, S, S)
        scratch = torch.empty(nbytes // 4 + 1, device=self.dev, dtype=torch.float32)
        ops.launch(name, g.data_ptr(), *vol, cf20.data_ptr(), gcoef18.data_ptr(), scratch.data_ptr(), scratch.numel() * 4, n, S, S,
                   S, self.C, self._n, tag='resample_bwd_coef')
