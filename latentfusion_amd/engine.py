"""Fused render-and-score engine of the gradient pose loop.

One call = the forward AND backward of
    camera params -> coefficient blocks -> O2C resample -> camera conv3d blocks -> factor projection
                  -> 2-D decoder + heads -> interpret_logits -> uncrop -> pose loss
for N pose hypotheses of one latent object, returning the per-sample losses and
d(mean weighted loss)/d(log_quaternion, translation, viewport).

Compared with driving the same kernels through the generic autograd modules this removes the
~600 tiny ATen launches per iteration of the camera algebra and of the loss (they become
lf_camera_coefs, lf_pose_loss_fwd/bwd and lf_camera_coefs_bwd), keeps the 3-D activations in
preallocated buffers and sequences the heavy kernels explicitly.  A PLAIN 2-D decoder (blocks without rescaling or skip
concatenations: the SYN family) is sequenced explicitly as well since round 4 -- every data-gradient kernel applies the
LeakyReLU' / PixelNorm' of the layer feeding it, so no separate epilogue-backward pass runs; a generic U-Net (the released
model) runs through the autograd ops on its (N,C,h,w) maps.

Numerically it is the same computation as Photographer.decode + default_pose_loss
(reference recon/models.py:397-505, pose/estimation.py:70-118); tests/test_engine_gpu.py checks it
against the module path and against the reference's golden loop trace.
"""
import collections
import contextlib
import math

import torch

from . import _lib, ops
from ._lib import LF_EPI_LRELU, LF_EPI_PIXELNORM, LF_MAP_O2C

NCOEF = 24
NPAR = 10


class _CameraCoefs(torch.autograd.Function):
    """(N,10) camera parameters -> (N,24) coefficient blocks (lf_camera_coefs)."""

    @staticmethod
    def forward(ctx, params, intr, cube, z_span, h, w):
        n = params.shape[0]
        coefs = torch.empty(n, NCOEF, device=params.device, dtype=torch.float32)
        jac = torch.empty(n, NCOEF, NPAR, device=params.device, dtype=torch.float32)
        ops.launch('lf_camera_coefs', params.contiguous().data_ptr(), intr.contiguous().data_ptr(), cube, z_span, h, w,
                   coefs.data_ptr(), jac.data_ptr(), n)
        ctx.save_for_backward(jac)
        return coefs

    @staticmethod
    def backward(ctx, g):
        jac, = ctx.saved_tensors
        n = jac.shape[0]
        gp = torch.empty(n, NPAR, device=jac.device, dtype=torch.float32)
        ops.launch('lf_camera_coefs_bwd', g.contiguous().data_ptr(), jac.data_ptr(), gp.data_ptr(), n)
        return gp, None, None, None, None, None


def camera_params(camera):
    return torch.cat((camera.log_quaternion, camera.translation, camera.viewport), dim=1)


def camera_intrinsics(camera):
    K = camera.intrinsic
    return torch.stack((K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]), dim=1).contiguous()


def camera_coefs(camera, cube_size, crop_h, crop_w):
    """Differentiable (w.r.t. log_quaternion / translation / viewport) coefficient blocks."""
    return _CameraCoefs.apply(camera_params(camera), camera_intrinsics(camera), float(cube_size), float(camera.z_span),
                              int(crop_h), int(crop_w))


_LOSS_FORMS = {'logits': '', 'masked': '_masked', 'depth': '_depth'}


def _pose_loss_entry(direction, mode, tn):
    """Name of the pose-loss entry point of a form ('logits' | 'masked' | 'depth') for one target frame (tn None) or for rows
    grouped by target (tn = (T, n)).  (A form the library does not export fails where it is looked up.)"""
    return 'lf_pose_loss_' + direction + _LOSS_FORMS[mode] + ('_mt' if tn is not None else '')


def _pose_loss_scratch(lg, H, W):
    N, _, h, w = lg.shape
    nbytes = _lib.lib().lf_pose_loss_scratch_bytes(N, h, w, H, W)
    return torch.empty(nbytes // 4 + 1, device=lg.device, dtype=torch.float32)


def _pose_loss_fwd(lg, cf, tdepth, tmask, weights, H, W, mode='logits', tn=None, sums=None):
    """THE launch of the fused pose loss of lg [N][h*w][2]: (losses (N,8), gsums, scratch).  mode: 'logits' (head outputs),
    'masked' (the forward-only ranking form: no gsums are formed) or 'depth' (metric depth crop + mask logit); tn = (T, n): rows
    grouped by target against [T][H*W] frames (the _mt entry points); sums: an (N,8) buffer of the caller's to keep them."""
    name = _pose_loss_entry('fwd', mode, tn)
    N, _, h, w = lg.shape
    scratch = _pose_loss_scratch(lg, H, W)
    if sums is None:
        sums = torch.empty(N, 8, device=lg.device, dtype=torch.float32)
    losses = torch.empty(N, 8, device=lg.device, dtype=torch.float32)
    gsums = torch.empty(N, 8, device=lg.device, dtype=torch.float32)
    out = () if mode == 'masked' else (gsums.data_ptr(),)
    ops.launch(name, lg.data_ptr(), cf.data_ptr(), tdepth.data_ptr(), tmask.data_ptr(), weights.data_ptr(), sums.data_ptr(),
               losses.data_ptr(), *out, scratch.data_ptr(), scratch.numel() * 4, N, *(tn or ()), h, w, H, W)
    return losses, gsums, scratch


def _pose_loss_bwd(lg, cf, tdepth, tmask, gsums, glogits, gcoefs, scratch, H, W, tn=None, mode='logits'):
    """THE launch of the loss backward: d/d(logits) and coefficient entries 18..23 (0..17 of gcoefs are not written)."""
    name = _pose_loss_entry('bwd', mode, tn)
    N, _, h, w = lg.shape
    ops.launch(name, lg.data_ptr(), cf.data_ptr(), tdepth.data_ptr(), tmask.data_ptr(), gsums.data_ptr(), glogits.data_ptr(),
               gcoefs.data_ptr(), scratch.data_ptr(), scratch.numel() * 4, N, *(tn or ()), h, w, H, W)


class _PoseLoss(torch.autograd.Function):
    """Fused default_pose_loss over head logits.  Returns (total (N,), components (N,8)); tn = (T, n): several target frames."""

    @staticmethod
    def forward(ctx, logits, coefs, tdepth, tmask, weights, H, W, tn=None):
        lg = ops.cl(logits)                                   # (N,2,h,w) channels-last == [N][h*w][2]
        cf = coefs.detach().contiguous()
        losses, gsums, scratch = _pose_loss_fwd(lg, cf, tdepth, tmask, weights, H, W, tn=tn)
        ctx.save_for_backward(lg, cf, tdepth, tmask, gsums, scratch)
        ctx.dims = (H, W, tn)
        ctx.mark_non_differentiable(losses)
        return losses[:, 4].clone(), losses

    @staticmethod
    def backward(ctx, g_total, _g_losses):
        lg, cf, tdepth, tmask, gsums, scratch = ctx.saved_tensors
        H, W, tn = ctx.dims
        # gsums were formed for d(mean over the rows of one target); rescale to the incoming per-sample gradient
        gs = (gsums * (g_total * (tn[1] if tn is not None else lg.shape[0])).unsqueeze(1)).contiguous()
        glogits = torch.empty_like(lg)
        gcoefs = torch.zeros(lg.shape[0], NCOEF, device=lg.device, dtype=torch.float32)
        _pose_loss_bwd(lg, cf, tdepth, tmask, gs, glogits, gcoefs, scratch, H, W, tn)
        return glogits, gcoefs, None, None, None, None, None, None


def pose_loss(logits, coefs, tdepth, tmask, weights, H, W):
    return _PoseLoss.apply(logits, coefs, tdepth, tmask, weights, H, W)


@contextlib.contextmanager
def _frozen(params):
    """Clears the `requires_grad` flags of `params` for the duration of the block."""
    # the engine differentiates w.r.t. the cameras only: with trainable parameters (the default of a model that was not frozen:
    # eval() is a pure mode switch, as in the reference) the autograd pieces would save activations for, and launch,
    # weight-gradient kernels nobody reads
    live = [p for p in params if p.requires_grad]
    for p in live:
        p.requires_grad_(False)
    try:
        yield
    finally:
        for p in live:
            p.requires_grad_(True)


# ---------------------------------------------------------------------------------------------------------------------------
# The camera-block plan: WHICH kernels drive the camera blocks' 3x3x3 convolutions is decided here, once per engine
# (select_camera_blocks), and nowhere else.  A family holds the packs it launches and answers
#   forward(li, x, flags, depth_inner)               -> (y, norm); the 16-channel Winograd family's last layer, when the factor
#                                                       projection rides along (ride_projection), -> (y, norm, zp, pnorm)
#   data_grad(i, g, acts, norms, flags, bounds)      -> gradient w.r.t. the input of layer i
#   grad_bounds()                                    -> per-call max-abs rows of the gradient volumes, or None
# and the constants
#   folds_prev         the data-gradient kernels apply the LeakyReLU' / PixelNorm' of the layer FEEDING them in their store: `g` is
#                      d/d(pre-activation of layer i); otherwise `g` is d/d(output of layer i) and data_grad runs the separate
#                      epilogue-backward pass first
#   wide               >= 64-channel Winograd GEMM (the ranking form may take the factor projection as a library GEMM)
#   wino16             the 16-channel Winograd kernels: the forward projection can ride in the last layer's launch, and the
#                      occlusion module is sequenced on the same kernels
#   plain_factor_only  split-precision arithmetic: measured for the plain 'factor' renderer only
# ---------------------------------------------------------------------------------------------------------------------------
def _prev(i, acts, norms, flags):
    return (acts[i], norms[i - 1], flags) if i > 0 else None


class _CameraBlocks:
    folds_prev = wide = wino16 = plain_factor_only = False

    def __init__(self, convs, z):
        self.w = [c.module.weight for c in convs]
        self.bias = [c.bias for c in convs]
        self.he = [ops.he_constant(w) for w in self.w]
        self.dev = z.device

    def grad_bounds(self):
        return None


class _Fp32Direct(_CameraBlocks):
    """Direct implicit GEMM on the fp32 MFMA (every channel count)."""

    def __init__(self, convs, z):
        super().__init__(convs, z)
        self.packs = [(ops.pack_conv3x3(w), ops.pack_conv3x3(w, transpose=True)) for w in self.w]
        self.folds_prev = _block_kinds([tuple(w.shape[:2]) for w in self.w], z.shape[1])[0]     # whole records of 16 channels

    def forward(self, li, x, flags, depth_inner=False):
        return ops._conv3x3_raw(x, self.packs[li][0], self.bias[li], self.w[li].shape[0], self.he[li], flags, True)

    def data_grad(self, i, g, acts, norms, flags, bounds):
        if self.folds_prev:
            return ops.conv3x3_bwd_data(g, self.packs[i][1], self.w[i].shape[1], self.he[i], _prev(i, acts, norms, flags))
        gpre = ops._epilogue_bwd(g, acts[i + 1], norms[i], flags)
        return ops._conv3x3_raw(gpre, self.packs[i][1], None, self.w[i].shape[1], self.he[i], 0, False)[0]


class _Winograd16(_CameraBlocks):
    """16 -> 16 blocks: F(2x2x2,3x3x3) minimal filtering in fp32 (lf_conv3d_c16_wino)."""
    folds_prev = wino16 = True

    def __init__(self, convs, z):
        super().__init__(convs, z)
        self.packs = [(ops.pack_conv3d_c16_wino(w), ops.pack_conv3d_c16_wino(w, transpose=True)) for w in self.w]
        self.rider = None

    def ride_projection(self, proj_pack, proj_bias, proj_he):
        """The factor projection joins the last layer's launch (lf_conv3d_c16_wino_projfwd)."""
        self.rider = (proj_pack, proj_bias, proj_he)

    def forward(self, li, x, flags, depth_inner=False):
        if self.rider is not None and li == len(self.w) - 1:
            return ops.conv3d_c16_wino_projfwd(x, self.packs[li][0], self.bias[li], self.he[li], flags, *self.rider, flags)
        return ops.conv3d_c16_wino(x, self.packs[li][0], self.bias[li], self.he[li], flags)

    def data_grad(self, i, g, acts, norms, flags, bounds):
        return ops.conv3d_c16_wino(g, self.packs[i][1], None, self.he[i], 0, prev=_prev(i, acts, norms, flags))[0]


class _Direct16F16x3(_CameraBlocks):
    """16 -> 16 blocks: direct convolution, each fp32 product from three f16 MFMAs (lf_conv3d_c16_split)."""
    # the max-abs of each gradient volume (order-independent atomic max inside the producing kernel) lets the kernels pre-scale
    # tiny gradients by an exact power of two: row i + 1 bounds the gradient entering layer i, the projection backward fills the
    # last row
    folds_prev = plain_factor_only = True
    _pack, _conv = staticmethod(ops.pack_conv3d_c16_split), staticmethod(ops.conv3d_c16_split)

    def __init__(self, convs, z):
        super().__init__(convs, z)
        self.packs = [(self._pack(w), self._pack(w, transpose=True)) for w in self.w]
        self.x0_bound = None                                     # (a bound of the first layer's input, where the kernel takes one)

    def grad_bounds(self):
        return ops.amax_buffer(None, self.dev, rows=len(self.w) + 1)

    def forward(self, li, x, flags, depth_inner=False):
        return self._conv(x, self.packs[li][0], self.bias[li], self.he[li], flags, amax_in=self.x0_bound if li == 0 else None)

    def data_grad(self, i, g, acts, norms, flags, bounds):
        return self._conv(g, self.packs[i][1], None, self.he[i], 0, prev=_prev(i, acts, norms, flags), amax_in=bounds[i + 1],
                          amax_out=bounds[i])[0]


class _WideWinograd(_CameraBlocks):
    """Wide blocks (released model: 256 -> 256 on 16^3): Winograd input transform + lf_wino_fused_gemm (ops.wide_conv)."""
    # (fused fp32-MFMA GEMM / output transform / epilogue kernel; the packs are cached on the parameters)
    wide = True
    # rows per part of the launches (lf_wino_fused_gemm_part); None: the batch's own plan.  engine_multi.MultiTargetEngine with
    # per_target_plan=True sets it to the hypotheses per target for the duration of a call
    part_n = None

    def forward(self, li, x, flags, depth_inner=False):
        return ops.wide_conv(x, self.w[li], self.bias[li], self.he[li], flags, depth_inner=depth_inner, part_n=self.part_n)

    def data_grad(self, i, g, acts, norms, flags, bounds):
        gpre = ops._epilogue_bwd(g, acts[i + 1], norms[i], flags)
        return ops.wide_conv(gpre, self.w[i], None, self.he[i], 0, transpose=True, part_n=self.part_n)[0]


class _WideWinogradF16x3(_CameraBlocks):
    """Wide blocks on the split-precision Winograd GEMM (ops.wide_conv_f16x3)."""
    # the weights' scale is chosen at packing, the inputs' from a bound held in a device buffer -- the first block reads the
    # resampled volume, a convex combination of z (|x| <= max|z|), every later one a PixelNorm output (|x| <= sqrt(Cin));
    # gradients' bounds are measured where they are produced (ops.epilogue_bwd_amax)
    wide = plain_factor_only = True

    def __init__(self, convs, z):
        super().__init__(convs, z)
        self.x_bound = [ops.amax_buffer(z.abs().amax(), self.dev)] + [
            ops.amax_buffer(torch.tensor(math.sqrt(w.shape[1])), self.dev) for w in self.w[1:]]
        for w in self.w:                                         # packed now (cached on the parameter), not inside the first call
            ops._pk(w, 'wxf', lambda w_: ops.pack_conv_wino_fused_f16x3(w_))
            ops._pk(w, 'wxb', lambda w_: ops.pack_conv_wino_fused_f16x3(w_, transpose=True))

    def forward(self, li, x, flags, depth_inner=False):
        return ops.wide_conv_f16x3(x, self.w[li], self.bias[li], self.he[li], flags, depth_inner=depth_inner, amax_in=self.x_bound[li])

    def data_grad(self, i, g, acts, norms, flags, bounds):
        amax = ops.amax_buffer(None, self.dev)
        gpre = ops.epilogue_bwd_amax(g, acts[i + 1], norms[i], flags, amax)
        return ops.wide_conv_f16x3(gpre, self.w[i], None, self.he[i], 0, transpose=True, amax_in=amax)[0]


CONV_MODES = ('auto', 'fp32', 'winograd', 'f16x3')


def _block_kinds(shapes, C):
    """(all blocks 16 -> 16 on a 16-channel volume, all blocks wide) of the (cout, cin) of the camera-block convolutions."""
    c16 = C == 16 and len(shapes) > 0 and all(tuple(sh) == (16, 16) for sh in shapes)
    wide = len(shapes) > 0 and all(co >= 64 and ci >= 64 and co % 4 == 0 and ci % 4 == 0 for co, ci in shapes)
    return c16, wide


def select_camera_blocks(conv_mode, shapes, C):
    """(resolved conv_mode, family) for the (cout, cin) `shapes` of the camera-block convolutions on a C-channel volume: 'auto'
    resolution and the refusals.  Pure host logic (tests/test_host_logic.py); experimental.select_camera_blocks adds its family."""
    if conv_mode not in CONV_MODES:
        raise ValueError(conv_mode)
    c16, wide = _block_kinds(shapes, C)
    if conv_mode == 'auto':
        conv_mode = 'winograd' if (c16 or wide) else 'fp32'
    if conv_mode == 'f16x3' and not (c16 or wide):
        raise NotImplementedError('f16x3 mode is implemented for 16->16 and wide (>= 64 channel) camera blocks')
    if conv_mode == 'winograd' and not (c16 or wide):
        raise NotImplementedError('winograd mode needs 16->16 or wide (>= 64 channel) camera blocks')
    if conv_mode == 'fp32':
        return conv_mode, _Fp32Direct
    if conv_mode == 'winograd':
        return conv_mode, _Winograd16 if c16 else _WideWinograd
    return conv_mode, _Direct16F16x3 if c16 else _WideWinogradF16x3


PROJ_KERNELS = ('library', 'mfma')


def select_proj_kernel(proj_kernel, default, K, cout):
    """Resolved `proj_kernel` of a RenderLoopEngine whose factor projection is K = D * C -> cout (K = cout = None: the renderer
    has no factor projection): None -> `default`; 'mfma' outside lf_rows_gemm_epi's domain is refused, never replaced by the
    library GEMM.  Pure host logic (tests/test_rows_gemm_pack.py)."""
    if proj_kernel is None:
        proj_kernel = default
    if proj_kernel not in PROJ_KERNELS:
        raise ValueError(f'proj_kernel {proj_kernel!r}: one of {PROJ_KERNELS}')
    if proj_kernel == 'mfma':
        if K is None or cout is None:
            raise NotImplementedError("proj_kernel 'mfma' needs the 'factor' projection")
        if not (K >= 4 and K % 4 == 0 and 16 <= cout <= 256 and cout % 4 == 0):
            raise NotImplementedError(f"proj_kernel 'mfma': lf_rows_gemm_epi takes K % 4 == 0 and 16 <= Cout <= 256, Cout % 4 == 0; "
                                      f'this projection is K = {K}, Cout = {cout}')
    return proj_kernel


LATENT_KERNELS = ('autograd', 'fused')


def select_latent_kernel(latent_kernel, default):
    """Resolved `latent_kernel` of a RenderLoopEngine: None -> `default`; anything but LATENT_KERNELS is refused.  Pure host logic
    (tests/test_latent_fused_args.py)."""
    if latent_kernel is None:
        latent_kernel = default
    if latent_kernel not in LATENT_KERNELS:
        raise ValueError(f'latent_kernel {latent_kernel!r}: one of {LATENT_KERNELS}')
    return latent_kernel


# What a tail forward (camera blocks' output -> projected latent) hands on: zp / pnorm: the projected latent and its PixelNorm
# factors as buffers (explicit decoder, ranking latent term); feat: the same latent as the autograd decoder / latent term reads
# it; leaf: the tensor autograd differentiates the 2-D part back to; occ_saved: what the explicit occlusion backward reads;
# lat: (zt, sums, gscale) of a fused latent term, whose gradient _proj_pre_grad adds at zp (None: no such term).
_Tail = collections.namedtuple('_Tail', 'zp pnorm feat leaf occ_saved lat', defaults=(None,))


class RenderLoopEngine:
    """Explicit forward+backward of N pose hypotheses through a Photographer and the fused pose loss.

    An engine is a per-(object, target) INFERENCE object, driven from one host thread: it caches packed weights, the output of
    the object-frame blocks and the resident volume at construction, and it freezes the renderer's trainable parameters for
    the duration of a call (their `requires_grad` flags are restored on return).  Rebuild it after any weight update; do not
    share the model with a concurrently running training step.

    The camera blocks' kernels are a plan chosen once at construction (`self.plan`, select_camera_blocks above); a call runs the
    stages of _forward_backward_group in the order of the module docstring.  A subclass contributes kernel families by naming
    another selection function in `_select_blocks` (experimental.RenderLoopEngineX: 'winograd_f16x3')."""

    LOSS_KEYS = ('depth', 'ov_depth', 'iou', 'mask')
    EXPLICIT_DECODER = True          # A/B switch (tools/engine_ab.py): False runs a plain 2-D decoder through autograd like a generic one
    EXPLICIT_OCCLUSION = True        # A/B switch (tools/variant_probe.py): False runs the occlusion module through autograd
    PROJ_GEMM = True                 # wide blocks, ranking only: depth-innermost last block + library GEMM for the factor projection
    PROJ_KERNEL = 'library'          # what the PROJ_GEMM branch launches when proj_kernel is None: 'library' (addmm + leaky_relu_ +
                                     # lf_pixelnorm_fwd) or 'mfma' (lf_rows_gemm_epi, one launch)
    LATENT_KERNEL = 'autograd'       # what evaluates the 'latent' loss term when latent_kernel is None: 'autograd' (ATen cosine chain,
                                     # the loss and the 2-D decoder as autograd nodes) or 'fused' (lf_latent_cosine_fwd / _bwd_epi)

    @staticmethod
    def supports(photographer, loss_weights):
        """Renderers the engine sequences: the 'factor' projection (explicit kernels end to end) and -- through the
        depth-column kernels lf_column_softmax_* / lf_column_scale_* / lf_column_reduce_sum_* -- the 'sum' projection and the
        occlusion module (reference recon/models.py:378-395,427-437)."""
        return (photographer.projection_type in ('factor', 'sum')
                and not photographer.skip_connections
                and all(b.interpolate is None for b in photographer.camera_blocks)
                and photographer.predict_depth and photographer.predict_mask and not photographer.predict_color
                and photographer.camera_config[-1] % 4 == 0)

    CONV_MODES = CONV_MODES
    FUSE_FORMS = ('fwd',)
    _select_blocks = staticmethod(select_camera_blocks)

    def __init__(self, photographer, z_obj, target_obs, loss_weights, conv_mode='auto', fuse_projection=None, proj_kernel=None,
                 latent_kernel=None):
        """conv_mode selects the kernels of the 16->16 camera-block convolutions:
        'fp32'     direct implicit-GEMM on the fp32 MFMA (works for every channel count);
        'winograd' F(2x2x2,3x3x3) minimal filtering, all-fp32 arithmetic (fp32 MFMA + fp32 transforms);
        'f16x3'    each fp32 product from three f16 MFMAs with fp32 accumulation: on 16->16 blocks the direct kernel
                   (documented preset: bench `alt`), on wide (>= 64-channel) blocks the F(2x2x2,3x3x3) Winograd GEMM
                   lf_wino_fused_f16x3_gemm for every camera-block convolution and data gradient; the 2-D decoder's wide
                   layers of the shapes and batches in ops.WIDE2D_F16X3_ROUTE on lf_wino_fused2d_f16x3_gemm (forward and data gradient);
        'auto'     (default) 'winograd' when the blocks are 16->16 or >= 64 channels wide, else 'fp32'.
        All stay within the fp32 kernel's distance of an fp64 reference (tests/test_engine_gpu.py).
        fuse_projection: None = the default (factor projection forward fused into the last block's Winograd launch where the
        shapes allow), False = two launches, ('fwd',) = required.
        proj_kernel: what the factor projection of a ranking call on wide blocks (PROJ_GEMM) launches: 'library' = the library
        GEMM + leaky_relu_ + lf_pixelnorm_fwd, 'mfma' = lf_rows_gemm_epi (one launch, fixed K order, no library GEMM on the
        path); None = PROJ_KERNEL.  'mfma' on a projection outside that kernel's domain raises NotImplementedError.
        The option only chooses what that branch launches: on 16-channel blocks, the 'sum' projection's or the occlusion
        module's tail, and on calls with need_grad=True the branch does not run and the option is idle (no pack is built;
        `proj_rows_pack` is None).
        latent_kernel: what evaluates the 'latent' loss term (cosine distance of the projected latent to z_target_latent):
        'autograd' = the ATen chain of _latent_distance, on a gradient call with the pose loss and the 2-D decoder as autograd
        nodes; 'fused' = lf_latent_cosine_fwd for the distance (ranking and gradient calls) and lf_latent_cosine_bwd_epi for its
        gradient, added at the projected latent inside the projection's epilogue backward, so that a gradient call keeps the
        explicit decoder and the two-launch loss; None = LATENT_KERNEL.  'fused' needs the projection's PixelNorm buffer: on
        tails without one (the 'sum' projection, a tail run as modules) and on calls without a latent term the option is idle
        and the existing path runs.
        (Measured-and-rejected variants -- three-term Winograd products, the fused projection backward, hypothesis groups on
        several streams, hipGraph replay -- live in experimental.RenderLoopEngineX.)"""
        self.ph = photographer
        self.cube = photographer.cube_size
        dev = z_obj.device
        self.z = self._resident_volume(photographer, z_obj)
        self.S = self.z.shape[-1]
        self.C = self.z.shape[1]
        self.crop = photographer.out_size
        # (the loss kernels take raw device pointers: a host-resident target must not reach them)
        self.tdepth = target_obs.depth.reshape(-1).float().to(dev).contiguous()
        self.tmask = target_obs.mask.reshape(-1).float().to(dev).contiguous()
        self.H, self.W = target_obs.depth.shape[-2:]
        self.set_weights(loss_weights)
        convs = [conv for blk in photographer.camera_blocks for conv in (blk.conv1, blk.conv2)]
        self.nconv = len(convs)
        self.conv_mode, family = self._select_blocks(conv_mode, [tuple(c.module.weight.shape[:2]) for c in convs], self.C)
        # 'sum' projection / occlusion module: the tail between the camera blocks and the 2-D decoder runs through the
        # depth-column ops (autograd functions over lf_column_*), the rest of the iteration stays explicit
        self.generic_tail = photographer.projection_type != 'factor' or photographer.occlusion_module is not None
        if self.generic_tail and family.plain_factor_only:
            raise NotImplementedError("the split-precision conv modes drive the plain 'factor' renderer only")
        self.plan = family(convs, self.z)
        C, D = (convs[-1].module.weight.shape[0] if convs else self.C), self.S
        self.Cl = C                                                  # channels of the last camera block's output
        # the occlusion module on this library's kernels, sequenced here like the camera blocks (round 5); None: its
        # architecture is not the one planned for, it runs as the module with autograd
        self.occ = None
        if photographer.occlusion_module is not None and self.plan.wino16 and C == 16 and RenderLoopEngine.EXPLICIT_OCCLUSION:
            self.occ = self._plan_occlusion(photographer.occlusion_module)
        cout, pw = C, None
        self.proj = None
        factor = photographer.projection_type == 'factor'
        self.proj_kernel = select_proj_kernel(proj_kernel, self.PROJ_KERNEL, D * C if factor else None,
                                              photographer.projection_block.conv.module.weight.shape[0] if factor else None)
        self.latent_kernel = select_latent_kernel(latent_kernel, self.LATENT_KERNEL)
        self.proj_rows_pack = None
        if factor:
            pw = photographer.projection_block.conv.module.weight
            cout = pw.shape[0]
            # [D*C][cout], K = d*C + c: the projection as one row-major GEMM over depth-innermost rows (PROJ_GEMM)
            self.proj_rows_t = pw.detach().reshape(cout, C, D).permute(2, 1, 0).reshape(D * C, cout).contiguous()
            self.proj = (pw, photographer.projection_block.conv.bias, ops.he_constant(pw),
                         ops.pack_conv1x1(pw.reshape(cout, C, D).permute(0, 2, 1).reshape(cout, D * C)),
                         ops.pack_conv1x1(pw.reshape(cout, C, D).permute(2, 1, 0).reshape(D * C, cout)))
        # factor projection fused into the Winograd kernel of the last camera block (lf_conv3d_c16_wino_projfwd; round 4):
        # bit-identical to the two-launch form, measured -0.07 ms per iteration
        can_fuse = self.plan.wino16 and cout == 16 and C == 16 and not self.generic_tail
        if fuse_projection is None:
            fuse_projection = ('fwd',) if can_fuse else ()
        elif fuse_projection is False:
            fuse_projection = ()
        elif fuse_projection is True:
            fuse_projection = self.FUSE_FORMS
        if any(f not in self.FUSE_FORMS for f in fuse_projection):
            raise ValueError(f'fuse_projection {fuse_projection!r}: this engine fuses {self.FUSE_FORMS}')
        if fuse_projection and not can_fuse:
            raise NotImplementedError("fuse_projection needs conv_mode 'winograd' on 16-channel blocks and a 16-channel projection")
        self.fuse_projection = tuple(fuse_projection)
        self.proj_fused = None
        if self.fuse_projection:
            wdm = pw.reshape(cout, C, D).permute(0, 2, 1).reshape(cout, D * C)        # depth-major K, as ppack
            self.proj_fused = (ops.pack_wino_proj(wdm), ops.pack_wino_proj(wdm, transpose=True))
        if 'fwd' in self.fuse_projection:
            self.plan.ride_projection(self.proj_fused[0], self.proj[1], self.proj[2])
        self._wide_factor = self.plan.wide and not self.generic_tail          # (where PROJ_GEMM applies to a ranking call)
        if self.proj_kernel == 'mfma' and self._wide_factor:
            # the matrix of proj_rows_t as [cout][K] rows, as lf_rows_gemm_epi reads it (only where that branch can run)
            self.proj_rows_pack = ops.pack_rows_gemm(pw.detach().reshape(cout, C, D).permute(0, 2, 1).reshape(cout, D * C))
        self.dev = dev
        self._params = list(photographer.parameters())
        self._intr = None                                            # (K, version, gathered): the intrinsics do not change during a loop
        # the output heads (1x1 convolutions without activation, reference blocks.py:108-119) as ONE pointwise convolution
        # with their weights stacked along the output channels: same arithmetic per channel, one launch each way instead
        # of a launch per head plus a concatenation
        self.heads = None
        obs = list(photographer.output_blocks)
        if len(obs) > 1 and all(getattr(ob, 'activation', None) is None and getattr(ob.conv, 'kernel_size', 0) == 1
                                and ob.conv.bias is not None for ob in obs):
            self.heads = (torch.cat([ob.conv.module.weight.detach() for ob in obs], dim=0).contiguous(),
                          torch.cat([ob.conv.bias.detach() for ob in obs], dim=0).contiguous())
        # a plain 2-D decoder is sequenced by the engine itself (no autograd graph, fused epilogue backward)
        self.dec = None
        dec = photographer.image_decoder
        blocks2d = list(dec.down_blocks) + list(dec.up_blocks)
        plain = (dec.input_block is None and dec.output_block is None and self.heads is not None
                 and (not self.generic_tail or (self.occ is not None and photographer.projection_type == 'factor'))
                 and (len(dec.up_blocks) < 2 or len(dec.down_blocks) < 2)               # no skip concatenation happens
                 and all(getattr(b, 'interpolate', True) is None for b in blocks2d) and len(blocks2d) > 0
                 and all(c.module.weight.dim() == 4 and tuple(c.module.weight.shape[2:]) == (3, 3) and c.module.weight.shape[0] <= 64
                         for b in blocks2d for c in (b.conv1, b.conv2)))
        if plain and RenderLoopEngine.EXPLICIT_DECODER:
            self.dec = []
            for blk in blocks2d:
                for conv in (blk.conv1, blk.conv2):
                    w = conv.module.weight
                    self.dec.append((w, conv.bias, ops.he_constant(w), ops.pack_conv3x3(w), ops.pack_conv3x3(w, transpose=True)))
            hw = self.heads[0]
            self.heads_pack = (ops.he_constant(hw), ops.pack_conv1x1(hw.reshape(hw.shape[0], hw.shape[1])),
                               ops.pack_conv1x1(hw.reshape(hw.shape[0], hw.shape[1]).t()))

    @staticmethod
    def _resident_volume(photographer, z_obj):
        """The volume the resampler reads: (1,C,S,S,S) channels-last, after the renderer's object-frame blocks."""
        z = ops.cl(z_obj.reshape(1, *z_obj.shape[-4:]))
        if len(photographer.object_blocks):
            # object-frame blocks act on the volume BEFORE the camera transform (reference recon/models.py:410-415): every
            # hypothesis sees the same input, so they are evaluated once per object here, not once per hypothesis per call
            with torch.no_grad():
                zo = z
                for blk in photographer.object_blocks:
                    zo = blk(zo)
            z = ops.cl(zo.detach())
        return z

    def set_weights(self, loss_weights):
        self.weights = torch.tensor([loss_weights.get(k, 0.0) for k in self.LOSS_KEYS], dtype=torch.float32,
                                    device=self.z.device)
        self.w_latent = float(loss_weights.get('latent', 0.0))

    # -----------------------------------------------------------------------------------------
    def forward_backward(self, camera, need_grad=True, z_target_latent=None, params=None, masked_depth=False):
        """Returns (losses (N,8): depth, ov_depth, iou, mask, weighted total, latent, 0, 0; gparams (N,10) or None).

        z_target_latent (N or 1, C2, h, w): the latent code of the target under every hypothesis
        (LatentFusionModel.compute_latent_code); with a non-zero 'latent' weight the cosine distance between it and the
        renderer's projected latent joins the loss (reference pose/estimation.py:112-116), column 5 of `losses`.

        masked_depth (forward only): the loss as the cross-entropy / Metropolis estimators evaluate it -- the crop depth
        times the crop's sigmoid mask before the uncrop (reference pose/estimation.py:207-216; lf_pose_loss_fwd_masked)."""
        # `params`: the (N,10) block [log_quaternion | translation | viewport] when the caller already holds it (the estimators'
        # cameras are views of one such tensor), else it is gathered from the camera; the intrinsics are gathered once
        if masked_depth and need_grad:
            raise ValueError('masked_depth is the forward-only loss form of the ranking estimators (no gradient is defined here)')
        if self.w_latent != 0.0 and z_target_latent is None:
            raise ValueError("the loss weights carry a 'latent' term: pass z_target_latent (LatentFusionModel.compute_latent_code)")
        params = (camera_params(camera) if params is None else params).detach().contiguous()
        K = camera.intrinsic
        # (keyed on the tensor OBJECT, which the cache keeps alive, and its version counter: an address alone could be
        # reused by another camera's intrinsics)
        if self._intr is None or self._intr[0] is not K or self._intr[1] != K._version:
            self._intr = (K, K._version, camera_intrinsics(camera))
        intr = self._intr[2]
        n = params.shape[0]
        zt = z_target_latent if (z_target_latent is not None and self.w_latent != 0.0) else None
        if zt is not None and zt.shape[0] == 1 and n > 1:
            zt = zt.expand(n, *zt.shape[1:])
        with _frozen(self._params):
            return self._run(params, intr, float(camera.z_span), need_grad, zt, masked_depth)

    def _run(self, params, intr, z_span, need_grad, zt, masked_depth):
        """All hypotheses as one group on the current stream (experimental.RenderLoopEngineX splits them over streams)."""
        return self._forward_backward_group(params, intr, z_span, need_grad, 1.0, zt, masked_depth)

    # ---- occlusion module on explicit kernels ----
    @staticmethod
    def _plan_occlusion(om):
        """Weights of UNet3d(17, 1, [[17, 16], [16, 16]]) without rescaling (the occlusion module as the reference
        constructs it, recon/models.py:305-306 over modules/unet.py, with a [[17, 16], [16, 16]] block configuration) packed for the explicit sequence, or None for any other shape:
        input block 1x1x1 17 -> 17 (lf_occ_input_*), conv 17 -> 16 as a 16 -> 16 Winograd launch over outputs 0..15 of the input
        block plus the 1 -> 16 convolution of its output 16 (lf_occ_conv17_*), three 16 -> 16 convolutions, output block 1x1x1 16 -> 1 without activation."""
        from .modules.blocks import OutputBlock
        blocks = list(om.down_blocks) + list(om.up_blocks)
        ib, ob = om.input_block, om.output_block
        if (ib is None or not isinstance(ob, OutputBlock) or ob.activation is not None or len(om.down_blocks) != 1
                or len(om.up_blocks) != 1 or any(b.interpolate is not None for b in blocks)):
            return None
        w1, wo = ib.conv.module.weight, ob.conv.module.weight
        convs = [c for b in blocks for c in (b.conv1, b.conv2)]
        shapes = [tuple(c.module.weight.shape) for c in convs]
        if (tuple(w1.shape) != (17, 17, 1, 1, 1) or tuple(wo.shape) != (1, 16, 1, 1, 1) or shapes[0] != (16, 17, 3, 3, 3)
                or any(sh != (16, 16, 3, 3, 3) for sh in shapes[1:]) or ib.conv.bias is None or ob.conv.bias is None):
            return None
        dev = w1.device
        wi = torch.zeros(17, 20, device=dev, dtype=torch.float32)
        wi[:, :17] = w1.detach().reshape(17, 17) * ops.he_constant(w1)
        bi = torch.zeros(20, device=dev, dtype=torch.float32)
        bi[:17] = ib.conv.bias.detach()
        w2 = convs[0].module.weight.detach()
        w2a = w2[:, :16].contiguous()
        he2 = ops.he_constant(w2)
        w27 = (w2[:, 16].reshape(16, 27).t() * he2).float().contiguous()              # [tap][co]
        pk = ops.pack_conv3d_c16_wino
        first = (convs[0].bias, he2, pk(w2a), pk(w2a, transpose=True), w27)
        rest = [(c.bias, ops.he_constant(c.module.weight), pk(c.module.weight), pk(c.module.weight, transpose=True)) for c in convs[1:]]
        wo2 = wo.detach().reshape(1, 16)
        head = (ob.conv.bias, ops.he_constant(wo), ops.pack_conv1x1(wo2))
        return dict(wi=wi.contiguous(), bi=bi, first=first, rest=rest, head=head, head_w16=wo2.reshape(16).float().contiguous())

    def _occlusion_fwd(self, zc, flags):
        """zc: output of the last camera block (n,16,S,S,S).  Returns (zs = zc * softmax_D(occlusion logits), saved); zs is None
        before a factor projection, which scales its operand itself (lf_conv1x1_fwd_scaled): the scaled volume is never written."""
        o, dev = self.occ, self.dev
        n, _, D, H, W = zc.shape
        P = H * W
        ta, t16 = ops.empty_cl(zc.shape, dev), torch.empty(n, 1, D, H, W, device=dev, dtype=torch.float32)
        ops.launch('lf_occ_input_fwd', zc.data_ptr(), o['wi'].data_ptr(), o['bi'].data_ptr(), ta.data_ptr(), t16.data_ptr(), n, D,
                   P, ops.SLOPE, tag='occ_input_fwd')
        b2, he2, pa, _pat, w27 = o['first']
        pre = ops.empty_cl(zc.shape, dev)
        ops.launch('lf_occ_conv17_fwd', t16.data_ptr(), w27.data_ptr(), pre.data_ptr(), n, D, H, W, tag='occ_conv17_fwd')
        y, nrm = ops.conv3d_c16_wino(ta, pa, b2, he2, flags, prev=(pre, None, _lib.LF_EPI_ADD), out=pre)
        ys, ns = [y], [nrm]
        for (b, he, pk, _pkt) in o['rest']:
            y, nrm = ops.conv3d_c16_wino(ys[-1], pk, b, he, flags)
            ys.append(y)
            ns.append(nrm)
        hb, hhe, hpk = o['head']
        wocc = torch.empty(n, 1, D, H, W, device=dev, dtype=torch.float32)
        if D <= 256:
            # (round 6) output block + softmax over the depth column in one pass over the last activation: no logits volume
            ops.launch('lf_column_softmax_head_fwd', ys[-1].data_ptr(), o['head_w16'].data_ptr(),
                       hb.data_ptr() if hb is not None else None, hhe, wocc.data_ptr(), None, n, D, P, tag='column_softmax_head')
        else:
            logits = torch.empty(n, 1, D, H, W, device=dev, dtype=torch.float32)
            ops._conv1x1_raw(ys[-1], hpk, hb, n, D * P, 16, 1, D * P * 16, 0, 1, logits, hhe, 0)
            ops.launch('lf_column_softmax_fwd', logits.data_ptr(), wocc.data_ptr(), None, n, D, P, tag='column_softmax')
        if self.proj is not None:
            return None, (ta, t16, ys, ns, wocc)
        zs = ops.empty_cl(zc.shape, dev)
        ops.launch('lf_column_scale_fwd', zc.data_ptr(), wocc.data_ptr(), zs.data_ptr(), n * D * P, 16)
        return zs, (ta, t16, ys, ns, wocc)

    def _occlusion_bwd(self, g_zs, zc, saved, flags, prev, proj_bwd=None):
        """d/d(zs) -> d/d(zc): the scaling, the softmax, the output block, the four convolutions (each data-gradient launch folds
        in the LeakyReLU' / PixelNorm' of the layer it lands on) and the input block, plus the direct term of the scaling.
        prev = (zc, norm, flags) of the camera-block layer that produced zc: its epilogue backward is applied on the way out."""
        o, dev = self.occ, self.dev
        ta, t16, ys, ns, wocc = saved
        n, _, D, H, W = zc.shape
        P = H * W
        # (the direct term g_zs * wocc of the scaling joins the input block's backward below: no volume is written for it)
        gl = torch.empty_like(wocc)
        if proj_bwd is not None and D <= 256:
            # (round 6) the weights' gradient sum_c zc * g_zs, g_zs recomputed from the projection's 2-D gradient, and the softmax
            # backward over each pixel's depth column in one launch: one read of zc; neither g_zs nor gw exist as volumes
            ops.launch('lf_occ_weight_grad_softmax_bwd', zc.data_ptr(), proj_bwd[0].data_ptr(), proj_bwd[1].data_ptr(), proj_bwd[2],
                       wocc.data_ptr(), gl.data_ptr(), n, D, P, tag='occ_weight_grad_softmax_bwd')
        else:
            gw = torch.empty_like(wocc)
            if proj_bwd is not None:
                ops.launch('lf_occ_weight_grad', zc.data_ptr(), proj_bwd[0].data_ptr(), proj_bwd[1].data_ptr(), proj_bwd[2],
                           gw.data_ptr(), n, D, P)
            else:
                ops.launch('lf_column_scale_bwd', g_zs.data_ptr(), zc.data_ptr(), wocc.data_ptr(), None, gw.data_ptr(), n * D * P,
                           16)
            ops.launch('lf_column_softmax_bwd', wocc.data_ptr(), gw.data_ptr(), None, gl.data_ptr(), n, D, P)
        hhe = o['head'][1]
        g = ops.empty_cl(zc.shape, dev)
        ops.launch('lf_occ_head_bwd', gl.data_ptr(), o['head_w16'].data_ptr(), hhe, ys[-1].data_ptr(), ns[-1].data_ptr(), flags,
                   ops.SLOPE, g.data_ptr(), n * D * P, tag='occ_head_bwd')
        for i in range(len(o['rest']) - 1, -1, -1):
            _b, he, _pk, pkt = o['rest'][i]
            g = ops.conv3d_c16_wino(g, pkt, None, he, 0, prev=(ys[i], ns[i], flags))[0]
        _b2, he2, _pa, pat, w27 = o['first']
        # (round 6) LeakyReLU' of the input block's outputs 0..15 rides in the store of this data gradient (prev = ta, no norm): the
        # input block's backward then does not read ta
        gp16 = torch.empty_like(t16)
        # (measured, round 6: this launch on a second stream BESIDE the Winograd data gradient that reads the same g is slower -- the
        # persistent Winograd workgroups hold every CU, the side kernel took 1.33 ms instead of 0.38 and stretched its neighbour:
        # 63.4 against 64.4 it/s)
        gta = ops.conv3d_c16_wino(g, pat, None, he2, 0, prev=(ta, None, LF_EPI_LRELU))[0]
        ops.launch('lf_occ_conv17_bwd', g.data_ptr(), t16.data_ptr(), w27.data_ptr(), gp16.data_ptr(), n, D, H, W, ops.SLOPE,
                   tag='occ_conv17_bwd')
        gz = ops.empty_cl(zc.shape, dev)
        if proj_bwd is not None:
            gp2d, ppack_t, phe = proj_bwd
            ops.launch('lf_occ_input_bwd_proj', gta.data_ptr(), gp16.data_ptr(), o['wi'].data_ptr(), gp2d.data_ptr(),
                       ppack_t.data_ptr(), phe, wocc.data_ptr(), gz.data_ptr(), n, D, P, ops.SLOPE, zc.data_ptr(),
                       prev[1].data_ptr(), prev[2], tag='occ_input_bwd')
            return gz
        ops.launch('lf_occ_input_bwd', gta.data_ptr(), None, gp16.data_ptr(), o['wi'].data_ptr(), g_zs.data_ptr(), wocc.data_ptr(),
                   gz.data_ptr(), n * D * P, ops.SLOPE, zc.data_ptr(), prev[1].data_ptr(), prev[2], tag='occ_input_bwd')
        return gz

    # ---- one evaluation, stage by stage ----
    def _forward_backward_group(self, params, intr, z_span, need_grad, grad_scale, zt=None, masked_depth=False):
        """coefficients -> resample -> camera blocks -> tail -> decoder + heads -> loss, then the same way back to the camera
        parameters.  Every stage takes what it reads and returns what later stages read."""
        n = params.shape[0]
        flags = LF_EPI_LRELU | LF_EPI_PIXELNORM
        coefs, jac, cf20 = self._coefficients(params, intr, z_span, n)
        # wide blocks, ranking only (the released architecture under the cross-entropy search): the last block writes its output
        # depth-innermost, so that the factor projection K = D * C -> C2 is ONE row-major GEMM for the library
        # (128 renders: 32768 x 4096 x 256, 0.5 ms on hipBLASLt's fp32 MFMA kernel against 1.27 ms of lf_conv1x1_fwd's K slices)
        proj_gemm = self.PROJ_GEMM and self._wide_factor and not need_grad
        acts, norms, rode = self._blocks_fwd(self._resample(cf20, n), flags, proj_gemm)
        tail = self._tail_fwd(acts[-1], rode, flags, need_grad, proj_gemm, n)
        # the latent term on its own kernels (latent_kernel 'fused'): needs the projection's epilogue buffers
        fused_lat = zt is not None and self.latent_kernel == 'fused' and tail.pnorm is not None
        latent_grad = zt is not None and need_grad and not fused_lat
        explicit = self.dec is not None and not latent_grad
        if explicit:
            dacts, dnorms, logits = self._decoder_fwd(tail.zp, tail.pnorm, flags, n)
        else:
            logits = self._decoder_autograd(tail.feat, need_grad)
        if latent_grad:
            # the loss as an autograd node, joined by the cosine distance of the projected latent (what Photographer.forward
            # returns as its latent); autograd carries the objective back to the tail's leaf and the coefficients
            cf_leaf = coefs.detach().requires_grad_(True)
            with torch.enable_grad():
                total, losses = self._loss_autograd(logits, cf_leaf)
                lat = self._latent_distance(tail.feat, zt, n)
                total = total + self.w_latent * lat
                losses = losses.clone()
                losses[:, 5] = lat.detach()
                losses[:, 4] += self.w_latent * lat.detach()
                objective = self._objective(total)               # the optimised quantity (estimation.py:616-617)
            g_leaf, g_cf = torch.autograd.grad(objective, [tail.leaf, cf_leaf])
            gp = None
        else:
            # the optimised quantity is mean_n(total) (estimation.py:616-617): lf_pose_loss_fwd already leaves the sums'
            # gradients for exactly that, so the loss needs no autograd node -- logits -> loss -> d/d(logits, coefficients)
            # are two kernel calls, and autograd only carries d(logits) back through a generic decoder
            lg = ops.cl(logits.detach())                          # (n,2,h,w) channels-last == [n][h*w][2]
            losses, gsums, scratch = self._loss_fwd(lg, coefs, masked_depth)
            if fused_lat:
                # distance of all rows in one call; it fills losses[:, 5] and adds its weighted share to losses[:, 4]
                zt = zt.to(device=self.dev, dtype=torch.float32)
                lat_sums = ops.latent_cosine_fwd(tail.zp, zt, losses, self.w_latent)
                if need_grad:
                    tail = tail._replace(lat=(zt, lat_sums, self.w_latent / self._mean_rows(n)))
            if not need_grad:
                if zt is not None and not fused_lat:
                    # latent term of a ranking-only evaluation: cosine distance of the projected latent (estimation.py:112-116)
                    lat = self._latent_distance(tail.zp, zt, n)
                    losses[:, 5] = lat
                    losses[:, 4] += self.w_latent * lat
                return losses, None
            glogits = torch.empty_like(lg)
            # (lf_pose_loss_bwd writes entries 18..23; 0..17 come from the resampler's coefficient gradient below)
            g_cf = torch.empty(n, NCOEF, device=self.dev, dtype=torch.float32)
            self._loss_bwd(lg, coefs, gsums, glogits, g_cf, scratch)
            if explicit and fused_lat:
                # the decoder's backward stops at d/d(zp): _proj_pre_grad adds the latent term there and applies the epilogue
                gp, g_leaf = None, self._decoder_bwd(glogits, dacts, dnorms, flags, n, fold_first=False)
            elif explicit:
                gp, g_leaf = self._decoder_bwd(glogits, dacts, dnorms, flags, n), None
            else:
                gp, (g_leaf,) = None, torch.autograd.grad(logits, [tail.leaf], grad_outputs=[glogits])
        # ---- 3-D backward (data gradients only): ONE chain, entered where the tail's backward leaves off ----
        g, first, bounds = self._tail_bwd(tail, gp, g_leaf, acts, norms, flags, n)
        for i in range(first, -1, -1):
            g = self.plan.data_grad(i, g, acts, norms, flags, bounds)
        return self._finish_backward(g, g_cf, cf20, jac, n, grad_scale, losses)

    def _coefficients(self, params, intr, z_span, n):
        """(N,10) camera parameters -> coefficient blocks, their Jacobian, and the resampler's padded O2C block."""
        params = params.contiguous()
        intr = intr.contiguous()
        coefs = torch.empty(n, NCOEF, device=self.dev, dtype=torch.float32)
        jac = torch.empty(n, NCOEF, NPAR, device=self.dev, dtype=torch.float32)
        ops.launch('lf_camera_coefs', params.data_ptr(), intr.data_ptr(), float(self.cube), z_span, self.crop, self.crop,
                   coefs.data_ptr(), jac.data_ptr(), n)
        # O2C coefficient block padded to the resampler's stride (LF_MAP_COEFS = 20)
        # (the object->camera map reads 18 of the 20 floats of a block; the two pad floats are never read: no fill launch)
        cf20 = torch.empty(n, 20, device=self.dev, dtype=torch.float32)
        cf20[:, :18] = coefs[:, :18]
        return coefs, jac, cf20

    def _resample(self, cf20, n):
        S = self.S
        x0 = ops.empty_cl((n, self.C, S, S, S), self.dev)
        ops.launch('lf_resample3d_fwd', self.z.data_ptr(), 1, cf20.data_ptr(), LF_MAP_O2C, x0.data_ptr(), n, S, S, S, self.C,
                   tag='resample_fwd')
        return x0

    def _blocks_fwd(self, x0, flags, proj_gemm):
        """Camera blocks on the plan's kernels: (activations [x0, y_0, ..], PixelNorm factors, [zp, pnorm] if the factor projection
        rode in the last launch else [])."""
        acts, norms, rode = [x0], [], []
        last = self.nconv - 1
        for li in range(self.nconv):
            y, nrm, *rode = self.plan.forward(li, acts[-1], flags, depth_inner=proj_gemm and li == last)
            acts.append(y)
            norms.append(nrm)
        return acts, norms, rode

    # ---- the tail between the camera blocks and the 2-D decoder: three forms, each a forward / backward pair over a _Tail ----
    def _tail_fwd(self, act, rode, flags, need_grad, proj_gemm, n):
        if self.occ is not None:
            return self._occlusion_tail_fwd(act, flags, need_grad, n)
        if self.generic_tail:
            return self._module_tail_fwd(act, need_grad)
        return self._factor_fwd(act, rode, flags, need_grad, proj_gemm, n)

    def _tail_bwd(self, tail, gp, g_leaf, acts, norms, flags, n):
        """-> (g, first, bounds): the gradient entering camera-block layer `first` -- d/d(its pre-activation) where the plan's data
        gradients fold the previous epilogue (plan.folds_prev), else d/d(its output) -- and the plan's gradient bounds.
        gp: d/d(projection pre-activation) from the explicit decoder, else g_leaf: autograd's gradient at tail.leaf."""
        if self.occ is not None:
            return self._occlusion_tail_bwd(tail, gp, g_leaf, acts, norms, flags, n)
        if self.generic_tail:
            return self._module_tail_bwd(tail, g_leaf, acts, norms, flags)
        return self._factor_bwd(tail, gp, g_leaf, acts, norms, flags, n)

    def _proj_pre_grad(self, tail, gp, g_leaf, flags):
        """d/d(projection pre-activation): the explicit decoder's gp as it is, else the epilogue backward of the gradient at the
        projected latent -- joined there by the gradient of a fused latent term (tail.lat), in the same pass."""
        if tail.lat is not None:
            zt, lat_sums, gscale = tail.lat
            return ops.latent_cosine_bwd_epi(ops.cl(g_leaf), tail.zp, tail.pnorm, zt, lat_sums, gscale, flags)
        return gp if gp is not None else ops._epilogue_bwd(ops.cl(g_leaf), tail.zp, tail.pnorm, flags)

    def _factor_fwd(self, act, rode, flags, need_grad, proj_gemm, n):
        """The plain factor projection: ridden along in the last block's launch, the row-major GEMM of a ranking call on wide
        blocks (self.proj_kernel: the library's, or lf_rows_gemm_epi with the epilogue in its store), or its own launch."""
        pw, pb, phe, ppack, _ppack_t = self.proj
        cout, S, Cl = pw.shape[0], self.S, self.Cl
        if rode:
            zp, pnorm = rode
        elif proj_gemm and self.proj_kernel == 'mfma':
            rows, pnorm = ops.rows_gemm_epilogue(act.view(n * S * S, S * Cl), self.proj_rows_pack, pb, phe, cout, flags,
                                                 tag='factor_project_fwd')
            zp = rows.view(n, S, S, cout).permute(0, 3, 1, 2)                # channels-last (n, cout, S, S)
        elif proj_gemm:
            with ops._timed('factor_project_fwd'):
                x2 = act.view(n * S * S, S * Cl)
                if pb is not None:
                    rows = torch.addmm(pb.detach(), x2, self.proj_rows_t, alpha=phe)        # he * (x W^T) + b
                else:
                    rows = torch.mm(x2, self.proj_rows_t).mul_(phe)
                torch.nn.functional.leaky_relu_(rows, ops.SLOPE)
                pnorm = torch.empty(n * S * S, device=self.dev, dtype=torch.float32)
                ops.launch('lf_pixelnorm_fwd', rows.data_ptr(), rows.data_ptr(), pnorm.data_ptr(), n * S * S, cout, ops.PN_EPS)
            zp = rows.view(n, S, S, cout).permute(0, 3, 1, 2)                # channels-last (n, cout, S, S)
        else:
            zp = ops.empty_cl((n, cout, S, S), self.dev)
            with ops._timed('factor_project_fwd'):
                pnorm = ops._conv1x1_raw(act, ppack, pb, n, S * S, Cl, S, S * S * S * Cl, S * S * Cl, cout, zp, phe, flags)
        leaf = zp.detach().requires_grad_(need_grad)
        return _Tail(zp, pnorm, leaf, leaf, None)

    def _factor_bwd(self, tail, gp, g_leaf, acts, norms, flags, n):
        pw, _pb, phe, _ppack, ppack_t = self.proj
        cout, S, Cl, nconv = pw.shape[0], self.S, self.Cl, self.nconv
        gp = self._proj_pre_grad(tail, gp, g_leaf, flags)
        fused = self._proj_bwd_fused(gp, acts, norms, flags) if self.plan.folds_prev else None
        if fused is not None:
            return fused + (None,)
        g = ops.empty_cl((n, Cl, S, S, S), self.dev)
        bounds = self.plan.grad_bounds()
        if self.plan.folds_prev:
            # every data-gradient kernel also applies the LeakyReLU'/PixelNorm' of the layer feeding it,
            # so no separate epilogue-backward pass touches the (N,16,S,S,S) volumes
            ops.launch('lf_conv1x1_bwd_data', gp.data_ptr(), ppack_t.data_ptr(), g.data_ptr(), n, S * S, cout, S * Cl,
                       S * S * S * Cl, Cl, Cl, S * S * Cl, phe, acts[nconv].data_ptr(), norms[nconv - 1].data_ptr(), flags,
                       ops.SLOPE, bounds[nconv].data_ptr() if bounds is not None else None, tag='factor_project_bwd')
        else:
            ops._conv1x1_raw(gp, ppack_t, None, n, S * S, cout, 1, S * S * cout, 0, S * Cl, g, phe, 0,
                             yaddr=(S * S * S * Cl, Cl, Cl, S * S * Cl))
        return g, nconv - 1, bounds

    def _proj_bwd_fused(self, gp, acts, norms, flags):
        """Hook: (gradient after the LAST block's data-gradient convolution, index of the next layer to walk) when the projection
        backward is fused into that launch; None here (experimental.RenderLoopEngineX: lf_conv3d_c16_wino_projbwd)."""
        return None

    def _occlusion_tail_fwd(self, act, flags, need_grad, n):
        """Occlusion weights on explicit kernels, then the composite: the factor projection or the 'sum' as a depth-column op."""
        # (the projection as its own launch: the fused form reads the block's output, not the scaled one)
        zs, occ_saved = self._occlusion_fwd(act, flags)
        if self.proj is None:
            leaf = zs.detach().requires_grad_(need_grad)
            with torch.set_grad_enabled(need_grad):
                zp = ops.column_sum(leaf)
            return _Tail(zp, None, zp, leaf, occ_saved)
        pw, pb, phe, ppack, _ppack_t = self.proj
        cout, S, Cl = pw.shape[0], self.S, self.Cl
        zp = ops.empty_cl((n, cout, S, S), self.dev)
        with ops._timed('factor_project_fwd'):
            pnorm = ops._conv1x1_raw(act, ppack, pb, n, S * S, Cl, S, S * S * S * Cl, S * S * Cl, cout, zp, phe, flags,
                                     xscale=occ_saved[4])
        leaf = zp.detach().requires_grad_(need_grad)
        return _Tail(zp, pnorm, leaf, leaf, occ_saved)

    def _occlusion_tail_bwd(self, tail, gp, g_leaf, acts, norms, flags, n):
        """d/d(scaled volume), then the occlusion module's explicit backward onto the last camera block's pre-activation."""
        # (d/d(scaled volume): the projection's data gradient (factor) or autograd's column-sum gradient ('sum'))
        S, Cl, nconv = self.S, self.Cl, self.nconv
        proj_bwd = None
        if self.proj is None:
            g_zs = ops.cl(g_leaf)
        else:
            pw, _pb, phe, _ppack, ppack_t = self.proj
            cout = pw.shape[0]
            gp = self._proj_pre_grad(tail, gp, g_leaf, flags)
            with ops._timed('factor_project_bwd'):
                if Cl == 16 and cout == 16 and (S * S) % 16 == 0:
                    # the projection's data gradient is NOT stored: lf_occ_weight_grad sums g_zs * zc over the channels of every
                    # voxel -- the gradient of the occlusion weights, one read of zc instead of lf_column_scale_bwd's pass over
                    # two volumes -- and the input block's backward recomputes g_zs where it needs it (lf_occ_input_bwd_proj)
                    g_zs, proj_bwd = None, (gp, ppack_t, phe)
                else:
                    g_zs = ops.empty_cl((n, Cl, S, S, S), self.dev)
                    ops._conv1x1_raw(gp, ppack_t, None, n, S * S, cout, 1, S * S * cout, 0, S * Cl, g_zs, phe, 0,
                                     yaddr=(S * S * S * Cl, Cl, Cl, S * S * Cl))
        g = self._occlusion_bwd(g_zs, acts[-1], tail.occ_saved, flags, (acts[nconv], norms[nconv - 1], flags), proj_bwd)
        return g, nconv - 1, None

    def _module_tail_fwd(self, act, need_grad):
        """The tail as modules under autograd, differentiated up to the last camera block's output."""
        # occlusion weights (3-D U-Net logits -> softmax over the depth column -> scale) and / or the 'sum' composite
        # (reference recon/models.py:378-395,427-437), as in Photographer.forward
        from .recon.utils import get_normalized_voxel_depth
        leaf = act.detach().requires_grad_(need_grad)
        with torch.set_grad_enabled(need_grad):
            zt_ = leaf
            if self.ph.occlusion_module is not None:
                occ = self.ph.occlusion_module(torch.cat((zt_, get_normalized_voxel_depth(zt_)), dim=1))
                wocc = ops.column_softmax(occ)[0]
                if tuple(occ.shape[-3:]) != tuple(zt_.shape[-3:]):
                    wocc = ops.column_softmax(ops.resize_nearest_to(occ, zt_.size(-1)))[0]
                zt_ = ops.column_scale(zt_, wocc)
            zp = ops.column_sum(zt_) if self.ph.projection_type == 'sum' else self.ph.projection_block(zt_)
        return _Tail(zp, None, zp, leaf, None)

    def _module_tail_bwd(self, tail, g_leaf, acts, norms, flags):
        g = ops.cl(g_leaf)                                        # d/d(output of the last camera block)
        if self.plan.folds_prev:
            g = ops._epilogue_bwd(g, acts[self.nconv], norms[self.nconv - 1], flags)
        return g, self.nconv - 1, None

    # ---- 2-D decoder + heads ----
    def _decoder_fwd(self, zp, pnorm, flags, n):
        """Plain decoder, sequenced here: conv + He + bias + LeakyReLU + PixelNorm per launch, then the stacked heads.
        Returns (activations [zp, ..], PixelNorm factors [pnorm, ..], logits)."""
        dacts, dnorms = [zp], [pnorm]
        for (w2, b2, he2, pk2, _pkt2) in self.dec:
            y2, n2 = ops._conv3x3_raw(dacts[-1], pk2, b2, w2.shape[0], he2, flags, True)
            dacts.append(y2)
            dnorms.append(n2)
        hw, hb = self.heads
        hhe, hpk, _hpkt = self.heads_pack
        hh, ww = dacts[-1].shape[-2:]
        logits = ops.empty_cl((n, hw.shape[0], hh, ww), self.dev)
        ops._conv1x1_raw(dacts[-1], hpk, hb, n, hh * ww, hw.shape[1], 1, hh * ww * hw.shape[1], 0, hw.shape[0], logits, hhe, 0)
        return dacts, dnorms, logits

    def _decoder_bwd(self, glogits, dacts, dnorms, flags, n, fold_first=True):
        """d/d(logits) -> d/d(projection pre-activation): the heads, then the decoder's data gradients in reverse.
        fold_first=False stops one step short, at d/d(projected latent): the first layer's data gradient without the projection's
        epilogue backward (a fused latent term joins before it, _proj_pre_grad)."""
        # each launch folds in the LeakyReLU' / PixelNorm' of the activation it lands on (whole records of 16 / 32 / 64 channels;
        # otherwise a separate pass); dacts[0] is the projected latent itself
        hw = self.heads[0]
        cin_h = hw.shape[1]
        hh, ww = dacts[-1].shape[-2:]
        g2 = ops.empty_cl((n, cin_h, hh, ww), self.dev)
        fuse_h = cin_h == 16
        ops.launch('lf_conv1x1_bwd_data', glogits.data_ptr(), self.heads_pack[2].data_ptr(), g2.data_ptr(), n, hh * ww, hw.shape[0],
                   cin_h, hh * ww * cin_h, cin_h, cin_h if fuse_h else (1 << 30), 0, self.heads_pack[0],
                   dacts[-1].data_ptr() if fuse_h else None, dnorms[-1].data_ptr() if fuse_h else None, flags if fuse_h else 0,
                   ops.SLOPE, None)
        if not fuse_h:
            g2 = ops._epilogue_bwd(g2, dacts[-1], dnorms[-1], flags)
        for i in range(len(self.dec) - 1, -1, -1):
            w2, _b2, he2, _pk2, pkt2 = self.dec[i]
            cin2 = w2.shape[1]
            if i == 0 and not fold_first:
                g2 = ops.conv3x3_bwd_data(g2, pkt2, cin2, he2, None)
            elif cin2 in (16, 32, 64):
                g2 = ops.conv3x3_bwd_data(g2, pkt2, cin2, he2, (dacts[i], dnorms[i], flags))
            else:
                g2 = ops._epilogue_bwd(ops.conv3x3_bwd_data(g2, pkt2, cin2, he2, None), dacts[i], dnorms[i], flags)
        return g2

    def _decoder_autograd(self, feat, need_grad):
        """A generic decoder (or a plain one under the latent term) through the autograd ops; returns the logits."""
        # conv_mode 'f16x3': the decoder's wide 2-D convolutions on the split-precision Winograd GEMM where that was measured
        # faster (ops.WIDE2D_F16X3_ROUTE); each records its form for its own backward, so the autograd backward follows it
        # without the scope
        with torch.set_grad_enabled(need_grad), ops.wide2d_f16x3(self.conv_mode == 'f16x3'):
            yimg, rescale = self.ph.decode_features(feat)         # (a final nearest up-sampling is owed to the logits)
            if self.heads is not None:
                logits = ops.conv1x1(yimg, self.heads[0], self.heads[1])
            else:
                logits = torch.cat([ob(yimg) for ob in self.ph.output_blocks], dim=1)
            return rescale(logits) if rescale is not None else logits

    # ---- the pieces that see the target frame or partition a per-sample reduction by the batch
    #      (engine_multi.MultiTargetEngine replaces them with their several-target forms) ----
    def _loss_fwd(self, lg, coefs, masked_depth):
        """Fused pose loss of the logits lg [n][h*w][2] against the target frame: (losses, gsums, scratch)."""
        return _pose_loss_fwd(lg, coefs, self.tdepth, self.tmask, self.weights, self.H, self.W, 'masked' if masked_depth else 'logits')

    def _loss_bwd(self, lg, coefs, gsums, glogits, g_cf, scratch):
        """d/d(logits) and coefficient entries 18..23 of the loss formed by _loss_fwd."""
        _pose_loss_bwd(lg, coefs, self.tdepth, self.tmask, gsums, glogits, g_cf, scratch, self.H, self.W)

    def _loss_autograd(self, logits, coefs):
        """The fused loss as an autograd node (the latent-term path): (total (n,), components (n,8))."""
        return pose_loss(logits, coefs, self.tdepth, self.tmask, self.weights, self.H, self.W)

    def _objective(self, total):
        return total.mean()

    def _mean_rows(self, n):
        """Rows the optimised mean of a row's loss runs over (_objective): the scale of a fused latent term's gradient."""
        return n

    def _latent_distance(self, zp, zt, n):
        """Cosine distance of every hypothesis's projected latent to the target's latent code (estimation.py:112-116)."""
        return 1.0 - torch.cosine_similarity(zp.reshape(n, -1), zt.reshape(n, -1).to(zp.dtype), 1, 1e-8)

    def _bwd_coef(self, g, cf20, gcoef18, n):
        """d/d(O2C output) -> gcoef18 [n][18] (lf_resample3d_bwd_coef)."""
        L = _lib.lib()
        S = self.S
        nbytes = L.lf_resample3d_bwd_coef_scratch_bytes(n, S, S, S)
        scratch = torch.empty(nbytes // 4 + 1, device=self.dev, dtype=torch.float32)
        ops.launch('lf_resample3d_bwd_coef', g.data_ptr(), self.z.data_ptr(), 1, cf20.data_ptr(), gcoef18.data_ptr(),
                   scratch.data_ptr(), scratch.numel() * 4, n, S, S, S, self.C, tag='resample_bwd_coef')

    def _finish_backward(self, g, g_cf, cf20, jac, n, grad_scale, losses):
        """d/d(O2C output) -> coefficient gradient -> camera parameters (lf_resample3d_bwd_coef, lf_camera_coefs_bwd)."""
        dev = self.dev
        gcoef18 = torch.empty(n, 18, device=dev, dtype=torch.float32)
        self._bwd_coef(g, cf20, gcoef18, n)
        gcoefs = g_cf.contiguous()
        gcoefs[:, :18] = gcoef18
        gparams = torch.empty(n, NPAR, device=dev, dtype=torch.float32)
        ops.launch('lf_camera_coefs_bwd', gcoefs.data_ptr(), jac.data_ptr(), gparams.data_ptr(), n)
        if grad_scale != 1.0:
            gparams *= grad_scale
        return losses, gparams
