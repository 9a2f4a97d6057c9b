"""Operators of the TRAINING step (BASELINE cfg 5; reference tools/train/train_reconstruct.py:421-535) on top of ops.py:
weight / bias gradients, the 16 -> 16 layers and resampler under the bf16 autocast + storage policy, the per-gate ConvGRU / LSTM
functions, the fused lift (the ConvGRU fuser as one autograd node: gru_train.py).  Reached through `ops.<name>` (ops.__getattr__)
and through ops' dispatchers (conv3x3, conv1x1, resample_*, lift), which pick these forms when a gradient is wanted / the policy is on."""
import contextlib
import math  # noqa: F401

import torch

from . import _lib, ops
from ._lib import LF_EPI_LRELU, LF_EPI_PIXELNORM, LF_MAP_C2O, LF_MAP_COEFS, LF_MAP_O2C  # noqa: F401
from .ops import (PN_EPS, SLOPE, _ac_in, _cached, _conv1x1_raw, _dense_views, _f32, _lift_permute, _pk, _req, _timed, _wsrc, launch, autocast, cl, conv3d_c16_ring_bf16, conv3d_c16_ring_bf16_io, conv3d_c16_wino, empty_cl, empty_cl16, he_constant, pack_conv1x1, pack_conv3d_c16_ring_bf16, pack_conv3d_c16_wino, round_bf16, storage_bf16)  # noqa: F401


# Weight-gradient launches of the training step on a second HIP stream (round 5).  The 16 -> 16 kernels of the step are bound by
# latency at two resident workgroups per CU, not by HBM or the matrix pipe, and a CU has room for two weight-gradient
# workgroups (62 KB of LDS each) plus one ring-convolution workgroup (35 KB): the weight gradient of a layer -- nothing in the
# backward chain waits for it -- runs beside the data-gradient convolution of the same layer instead of in front of it.
WGRAD_STREAM = True
# ---- round-6 forms of the training step, each with its A/B switch (module attribute; LF_<NAME>=0/1 in the environment sets the
# default for a fresh process: tools/train_probe.py A/Bs, profiles/r06_*) --------------------------------------------------
import os as _os


def _env(name, default):
    return type(default)(int(_os.environ.get('LF_' + name, int(default))))


# the ConvGRU recurrence (gru_train.py) on the ring kernels with fused epilogues (csrc/conv_gru.hip); False: round 5's one-output
# kernels + stage kernels (kept: fp32 storage / no autocast take that path anyway)
GRU_RING = _env('GRU_RING', True)
# steps per multi-volume weight-gradient launch of the recurrence on the side stream (0: one launch over all steps, after the chain)
GRU_WGRAD_CHUNK = _env('GRU_WGRAD_CHUNK', 16)
RING_BLOCK_FWD = _env('RING_BLOCK_FWD', True)          # forward Block steps on ring_multi (LF_RING_EX_BLOCK, bit-identical)
RING_DGRAD = _env('RING_DGRAD', True)                  # data gradients of the 16 -> 16 layers on ring_multi (bit-identical)
CHAIN_EPILOGUE = _env('CHAIN_EPILOGUE', True)          # a Block's conv2 data gradient applies conv1's epilogue backward (LF_RING_EX_PREV)
LIFT_MFMA = _env('LIFT_MFMA', True)                    # the 16-channel lift as one MFMA kernel each way (csrc/lift_mfma.hip)
PW16 = _env('PW16', True)                              # 1x1x1 16 -> 16 layers on the pointwise MFMA kernels (csrc/pw16.hip), not on the centre tap of the ring kernels
WIDE_WGRAD = _env('WIDE_WGRAD', True)                  # weight gradients with Cin, Cout >= 64 on the LDS-staged MFMA kernel (csrc/wgrad_wide.hip)


class _SideWgrad:
    """Weight-gradient launches on the side stream beside the data-gradient chain of the current stream (`main`): the one place of
    the training step that makes events, waits across streams and calls record_stream.  On when WGRAD_STREAM is set, work is
    `wanted` and no KERNEL_TIMER runs (its events time the current stream); off, `run` launches inline and the rest does nothing.
    The allocator recycles a tensor by main's order alone: every tensor a side launch touches must be named to `begin` or `run`."""

    _streams = {}                                                 # device -> its side stream

    def __init__(self, device, wanted=True):
        self.main = torch.cuda.current_stream()
        self.on = bool(WGRAD_STREAM and wanted and ops.KERNEL_TIMER is None)
        if self.on and device not in self._streams:
            self._streams[device] = torch.cuda.Stream(device=device)
        self.side = self._streams[device] if self.on else None

    def begin(self, *long_lived):
        """The side stream waits for what main has enqueued (the allocation and zero fill of `long_lived`: what several runs touch)."""
        if self.on:
            self.side.wait_stream(self.main)
            for t in long_lived:
                t.record_stream(self.side)

    def run(self, fn, *keep, timed=None):
        """fn() on the side stream once what main has enqueued so far is complete, `keep` (what it touches beyond `begin`'s tensors)
        alive until it finishes; returns the completion event for `wait`.  Off: fn() here, inside _timed(*timed) if given; None."""
        if not self.on:
            with _timed(*timed) if timed else contextlib.nullcontext():
                fn()
            return None
        self.side.wait_stream(self.main)
        for t in keep:
            t.record_stream(self.side)
        with torch.cuda.stream(self.side):
            fn()
            done = torch.cuda.Event()
            done.record(self.side)
        return done

    def wait(self, done):
        """main waits for a `run`: before it reads what that wrote or rewrites what that read (None: nothing to wait for)."""
        if done is not None:
            self.main.wait_event(done)

    def join(self):
        if self.on:
            self.main.wait_stream(self.side)


class _SplitViews(torch.autograd.Function):
    """(1, V, C, D, H, W) -> V tensors (1, C, D, H, W), like `unbind(1)`, for the fusers' walk over the views.  The point is
    the backward: the V gradients are copied ONCE into a (V, C, D, H, W) channels-last block and handed back as its
    (1, V, ...) view -- `unbind` / `z[:, i]` give a standard-layout stack that the view reshape and the producing kernels'
    channels-last conversion then copy two more times (1 GB each at 8 x 128^3 x 16)."""

    @staticmethod
    def forward(ctx, z):
        ctx.shape = tuple(z.shape)
        return tuple(z[:, i] for i in range(z.shape[1]))

    @staticmethod
    def backward(ctx, *grads):
        B, V = ctx.shape[0], ctx.shape[1]
        ref = next(g for g in grads if g is not None)
        block = empty_cl((B * V,) + ctx.shape[2:], ref.device) if len(ctx.shape) == 6 else \
            torch.empty((B * V,) + ctx.shape[2:], device=ref.device, dtype=ref.dtype, memory_format=torch.channels_last)
        blk = block.view(B, V, *ctx.shape[2:])
        for i, g in enumerate(grads):
            if g is None:
                blk[:, i].zero_()
            else:
                blk[:, i].copy_(g)
        return blk


def split_views(z):
    """The views of a (B, V, C, [D,] H, W) stack as a tuple (autograd-friendly `unbind(1)`, see _SplitViews)."""
    if z.dim() in (5, 6) and z.is_cuda and z.shape[0] == 1 and torch.is_grad_enabled() and z.requires_grad:
        return _SplitViews.apply(z)
    return z.unbind(1)


class _ResampleAC(torch.autograd.Function):
    """The 16-channel resampler under the bf16 storage policy: source in fp32 or bf16, destination bf16; the volume gradient
    (deterministic fixed-point splat) comes back in the source's storage type.  No camera gradient (training path)."""

    @staticmethod
    def forward(ctx, vol, coef, kind):
        n = coef.shape[0]
        vol_n = 1 if (vol.shape[0] == 1 or vol.stride(0) == 0) else vol.shape[0]
        if vol_n not in (1, n):
            raise ValueError('batch dimension of the volume and the cameras must match')
        v = cl(vol[:1] if vol_n == 1 else vol)
        _, C, D, H, W = v.shape
        out = empty_cl16((n, 16, D, H, W), v.device, True)
        cf = torch.zeros(n, LF_MAP_COEFS, device=v.device, dtype=torch.float32)
        cf[:, :coef.shape[1]] = coef.detach().float()
        io = (1 if v.dtype == torch.bfloat16 else 0) | 2
        launch('lf_resample3d_fwd_io', v, vol_n, cf, kind, out, n, D, H, W, io, tag='resample_fwd', detail=f'{kind}:{n}:io{io}')
        ctx.save_for_backward(cf)
        ctx.meta = (kind, vol_n, tuple(vol.shape), vol.dtype)
        return out

    @staticmethod
    def backward(ctx, gout):
        L = _lib.lib()
        cf, = ctx.saved_tensors
        kind, vol_n, vshape, vdtype = ctx.meta
        if ctx.needs_input_grad[1]:
            raise NotImplementedError('camera gradients run on the fp32 resampler (the pose loop); not under the training storage policy')
        if not ctx.needs_input_grad[0]:
            return None, None, None
        g = cl(gout)
        n, C, D, H, W = g.shape
        gv = empty_cl16((vol_n, 16, D, H, W), g.device, vdtype == torch.bfloat16)
        nb = L.lf_resample3d_bwd_vol_det_io_scratch_bytes(vol_n, n, D, H, W)
        scr = torch.empty(nb // 8 + 1, device=g.device, dtype=torch.int64)
        io = (1 if g.dtype == torch.bfloat16 else 0) | (2 if gv.dtype == torch.bfloat16 else 0)
        launch('lf_resample3d_bwd_vol_det_io', g, cf, kind, gv, vol_n, scr.data_ptr(), scr.numel() * 8, n, D, H, W, io,
               tag='resample_bwd_vol', detail=f'{kind}:{n}:io{io}')
        if gv.shape[0] == vshape[0]:
            return gv, None, None
        gvol = torch.zeros(vshape, device=g.device, dtype=gv.dtype)     # expanded (stride-0) input: see _Resample.backward
        gvol[0] = gv[0]
        return gvol, None, None


def _resample_ac_ok(vol, coef):
    return (vol.dim() == 5 and vol.shape[1] == 16 and vol.is_cuda and not coef.requires_grad and ops.DETERMINISTIC_SPLAT
            and (vol.dtype == torch.bfloat16 or storage_bf16()) and vol.shape[2] * vol.shape[3] * vol.shape[4] * 64 < 0xffffffff
            and max(vol.shape[2:]) < 0x7fff)


def ring_multi_ok(D, H, W):
    """lf_conv3d_c16_ring_multi takes this volume: 32-bit byte offsets within a sample of 64 B records."""
    return D * H * W * 64 < 2 ** 31


def _geom(t, dims):
    """(N, D, H, W, C) of a channels-last (N,C,[D,]H,W) tensor, or of a plain [rows][C] matrix (rows as W) for dims = 0."""
    if dims == 0:
        return 1, 1, 1, t.shape[0], t.shape[1]
    D, H, W = t.shape[2:] if dims == 3 else (1,) + tuple(t.shape[2:])
    return t.shape[0], D, H, W, t.shape[1]


def _wgrad_bf16_ok(gp, dims, cin, cout):
    """Shapes lf_conv_bwd_weight_bf16(_io) takes: its scratch query is non-zero there (include/lf_hip.h states the domain;
    the rest stays on lf_conv_bwd_weight with pre-rounded operands)."""
    N, D, H, W, _ = _geom(gp, dims)
    return _lib.lib().lf_conv_bwd_weight_bf16_scratch_bytes(dims, N, D, H, W, cin, cout) != 0


def _wide_wgrad_ok(x, gp, dims, cin, cout):
    """Shapes routed to lf_conv_bwd_weight_wide (WIDE_WGRAD): Cin, Cout >= 64, 16-byte aligned channels-last operands."""
    return (WIDE_WGRAD and dims in (0, 2, 3) and cin >= 64 and cout >= 64 and x is not None
            and x.data_ptr() % 16 == 0 and gp.data_ptr() % 16 == 0)


class _Wgrad:
    """A weight-gradient launch planned once and made many times.  The shape fixes the route (`entry`): the wide kernel when
    the caller says the operands qualify (`wide`: _wide_wgrad_ok), the bf16 MFMA when both operands are bf16 values (`bf16`) and
    the shape is in its domain, else lf_conv_bwd_weight.  `scratch` is what that entry point's own query asks (with `bias`, or
    for cin = 0, also what the bias launch asks), allocated here and shared by every call: calls on one stream are in order."""
    WIDE, BF16, GENERIC = 'lf_conv_bwd_weight_wide', 'lf_conv_bwd_weight_bf16_io', 'lf_conv_bwd_weight'

    def __init__(self, dims, N, D, H, W, cin, cout, device, he, bf16=False, wide=False, bias=False):
        L = _lib.lib()
        self.dims, self.sp, self.cin, self.cout, self.he = dims, (D, H, W), cin, cout, he
        shape = (dims, N, D, H, W, cin, cout)
        self.entry, nbytes = None, 0
        if cin and wide:
            self.entry, nbytes = self.WIDE, L.lf_conv_bwd_weight_wide_scratch_bytes(*shape)
        elif cin:
            nbytes = L.lf_conv_bwd_weight_bf16_scratch_bytes(*shape) if bf16 else 0
            self.entry = self.BF16 if nbytes else self.GENERIC
            nbytes = nbytes or L.lf_conv_bwd_weight_scratch_bytes(*shape)
        if bias or not cin:
            nbytes = max(nbytes, L.lf_conv_bwd_weight_scratch_bytes(0, N, D, H, W, 0, cout))
        self.scratch = torch.empty(nbytes // 4 + 4, device=device, dtype=torch.float32)

    def _launch(self, entry, x, gp, out, dims, cin, he, *io):
        N = gp.shape[0] if self.dims else 1
        launch(entry, x, gp, out, self.scratch.data_ptr(), self.scratch.numel() * 4, dims, N, *self.sp, cin, self.cout, he, *io)

    def __call__(self, x, gp, out):
        """out [taps][cout][cin] = he * sum_v gp[v] x[v + tap] on the current stream.  The bf16 entry takes either operand in fp32
        or bf16 storage, and fewer samples than planned (its scratch does not depend on N); the others read fp32."""
        if self.entry == self.BF16:
            io = ((1 if x.dtype == torch.bfloat16 else 0) | (2 if gp.dtype == torch.bfloat16 else 0),)
        elif x.dtype != torch.float32 or gp.dtype != torch.float32:
            raise TypeError(f'{self.entry} reads fp32 operands')
        else:
            io = ()
        with _timed('wgrad_wide', f'{self.dims}:{self.cin}:{self.cout}') if self.entry == self.WIDE else contextlib.nullcontext():
            self._launch(self.entry, x, gp, out, self.dims, self.cin, self.he, *io)

    def bias(self, gp, gb):
        """gb [cout] = column sums of gp (lf_conv_bwd_weight with x == NULL) on the same scratch."""
        self._launch(self.GENERIC, None, gp, gb, 0, 0, 1.0)


def bias_grad(gp, dims):
    """Column sums of the pre-activation gradient = d(loss)/d(bias) (lf_conv_bwd_weight with x == NULL).
    gp: channels-last (N,C,[D,]H,W), or a plain [rows][C] matrix for dims = 0."""
    N, D, H, W, cout = _geom(gp, dims)
    gb = torch.empty(1, cout, 1, device=gp.device, dtype=torch.float32)
    _Wgrad(dims, N, D, H, W, 0, cout, gp.device, 1.0).bias(gp, gb)
    return gb.reshape(cout)


def conv_bwd_weight(x, gp, dims, cin, he, want_bias=True, bf16=None):
    """Weight and bias gradients of y = conv(x, W) * he + b from the pre-activation gradient `gp`
    (lf_conv_bwd_weight).  x, gp: channels-last (N,C,[D,]H,W), or plain [rows][C] matrices for dims = 0.
    Returns (gw [taps][Cout][Cin], gb [Cout] or None when want_bias is False).  bf16: both operands are bf16 values (None:
    the ambient autocast policy) -- 3-D 16 -> 16 layers then run on the bf16 MFMA (lf_conv_bwd_weight_bf16_io)."""
    if bf16 is None:
        bf16 = ops.AUTOCAST is not None
    if dims == 3 and gp.shape[1] == 16 and cin > 16:
        # the LDS-staged 16 -> 16 kernel is ~4x faster than the generic one even with the slice copies:
        # the weight gradient of a wider input is the concatenation of the gradients of its channel chunks
        parts, gb = [], None
        for c0 in range(0, cin, 16):
            c1 = min(c0 + 16, cin)
            if c1 - c0 < 16:
                # ragged last chunk (the 3 coordinate channels of the 35-channel GRU gates): zero-pad it to 16 so it
                # also takes the LDS-staged kernel (0.25 ms instead of 6.6 ms on the generic one at 128^3)
                xc = empty_cl((x.shape[0], 16) + tuple(x.shape[2:]), x.device).zero_()
                xc[:, :c1 - c0] = x[:, c0:c1]
                gw_c, gb_c = conv_bwd_weight(xc, gp, dims, 16, he, want_bias and c0 == 0, bf16)
                gw_c = gw_c[:, :, :c1 - c0]
            else:
                gw_c, gb_c = conv_bwd_weight(cl(x[:, c0:c1]), gp, dims, 16, he, want_bias and c0 == 0, bf16)
            gb = gb_c if c0 == 0 else gb                       # the bias gradient (column sums of gp) once, not per chunk
            parts.append(gw_c)
        return torch.cat(parts, dim=2), gb
    N, D, H, W, cout = _geom(gp, dims)
    gw = torch.empty({0: 1, 2: 9, 3: 27}[dims], cout, cin, device=gp.device, dtype=torch.float32)
    wg = _Wgrad(dims, N, D, H, W, cin, cout, gp.device, he, bf16=bf16, wide=_wide_wgrad_ok(x, gp, dims, cin, cout), bias=want_bias)
    wg(x, gp, gw)
    if not want_bias:
        return gw, None
    gb = torch.empty(1, cout, 1, device=gp.device, dtype=torch.float32)
    wg.bias(gp, gb)
    return gw, gb.reshape(cout)


def pack_center_tap(weight):
    """(16,16,1,1,1) -> (16,16,3,3,3) with the weights on the centre tap: a pointwise 16 -> 16 layer on the 3x3x3 kernels."""
    w3 = weight.new_zeros(16, 16, 3, 3, 3)
    w3[:, :, 1, 1, 1] = weight.reshape(16, 16)
    return w3


def epilogue_bwd_c16(gy, y, norm, flags, want_bias, out_bf16=True):
    """lf_epilogue_bwd_c16 on channels-last (N,16,D,H,W) tensors in fp32 / bf16 storage: (gp, gbias or None)."""
    L = _lib.lib()
    rows = gy.numel() // 16
    gp = torch.empty_like(gy, dtype=torch.bfloat16 if out_bf16 else torch.float32, memory_format=torch.preserve_format)
    gb = torch.empty(16, device=gy.device, dtype=torch.float32) if want_bias else None
    nb = L.lf_epilogue_bwd_c16_scratch_bytes(rows) if want_bias else 0
    scr = torch.empty(nb // 4 + 1, device=gy.device, dtype=torch.float32) if want_bias else None
    io = (1 if gy.dtype == torch.bfloat16 else 0) | (2 if (y is not None and y.dtype == torch.bfloat16) else 0) | (4 if out_bf16 else 0)
    launch('lf_epilogue_bwd_c16', gy, y, norm, gp, gb, scr.data_ptr() if scr is not None else None,
           scr.numel() * 4 if scr is not None else 0, rows, flags, SLOPE, io, tag='epilogue_bwd_c16', detail=f'{rows}:io{io}')
    return gp, gb


def _ex_prev_scratch_floats(device, _cache={}):
    """Size of LF_RING_EX_PREV's partial-sum buffer, 16 * (1 + 2 * #CUs) floats (include/lf_hip.h)."""
    n = _cache.get(device)
    if n is None:
        n = _cache[device] = 16 * (1 + 2 * torch.cuda.get_device_properties(device).multi_processor_count)
    return n


# The chained epilogue's hand-off (CHAIN_EPILOGUE).  A consumer that applied the producer's epilogue backward ARMS the
# producer's box with the data gradient `gx` it returned -- the producer's pre-activation gradient -- and the bias sums of
# that launch.  The producer takes the fused result only if the box was armed in the SAME backward pass, and it disarms the
# box.  Its incoming gradient is then either exactly `gx` (the usual case: nothing else consumed the activation), or `gx`
# plus post-activation gradients of other consumers, which still need the epilogue backward.  The box holds `gx` itself,
# not a copy: a tensor referenced elsewhere is never the target of autograd's in-place gradient accumulation, so `gx` keeps
# its values and the incoming gradient can be told apart from it (storage, version, shape).
def _chain_box():
    return {'gx': None, 'gb': None, 'task': None}


def _chain_take(box):
    """The box's (gx, gb) when it was armed in the running backward pass, else None."""
    if box['gx'] is None or box['task'] != torch._C._current_graph_task_id():
        return None
    return box['gx'], box['gb']


def _chain_arm(box, gx, gb):
    box['gx'], box['gb'], box['task'] = gx, gb, torch._C._current_graph_task_id()


def _chain_epilogue_bwd(ctx, gy, y, norm, want_b):
    """The producer's side of an armed box: (pre-activation gradient in bf16, bias gradient or None); disarms the box."""
    gx, gb = _chain_take(ctx.box)
    ctx.box.update(gx=None, gb=None, task=None)
    if (gy.data_ptr() == gx.data_ptr() and gy._version == gx._version and gy.shape == gx.shape
            and gy.stride() == gx.stride() and gy.dtype == gx.dtype):
        return gx, (gb if want_b else None)
    # other consumers added post-activation gradients into gy: their share still goes through this layer's epilogue backward
    rest = gy.float() - gx.float()
    gp_rest, gb_rest = epilogue_bwd_c16(cl(rest), y, norm, ctx.flags, want_b, out_bf16=False)
    gp = cl((gp_rest + gx.float()).to(torch.bfloat16))
    return gp, (gb + gb_rest if want_b else None)


class _Conv16AC(torch.autograd.Function):
    """A 3-D 16 -> 16 layer (3x3x3, or 1x1x1 on the centre tap) of the training step under the bf16 autocast + storage policy:
    x (fp32 or bf16 storage) -> epilogue(conv(x, W) * he + b) in bf16 storage on lf_conv3d_c16_ring_bf16_io.  Backward: one
    pass for LeakyReLU' / PixelNorm' and the bias gradient (lf_epilogue_bwd_c16), the data gradient on the ring kernel
    in the input's storage type, the weight gradient on lf_conv_bwd_weight_bf16_io -- every volume moves as bf16.

    chain (round 6): the caller states that x is the output of ANOTHER _Conv16AC layer with LeakyReLU + PixelNorm that nothing else
    consumes (the two convolutions of a Block, modules/blocks.py:152-158).  This layer's data gradient then applies that layer's
    epilogue backward in its store and sums its bias gradient (LF_RING_EX_PREV): the producer receives its PRE-activation
    gradient and skips its own lf_epilogue_bwd_c16 pass (1.28 ms and 4.3 GB per Block at 32 views)."""

    @staticmethod
    def forward(ctx, x, weight, bias, flags, chain=False):
        _req(weight, 'weight')
        link = getattr(x, '_lf_link', None) if (chain and CHAIN_EPILOGUE) else None
        x = cl(x)
        he = he_constant(weight)
        one = weight.shape[2] == 1
        w3 = (lambda t: pack_center_tap(t)) if one else (lambda t: t)
        ctx.pw = bool(one and PW16 and flags in (0, LF_EPI_LRELU))
        if ctx.pw:
            # (round 6) a pointwise layer is one MFMA per 16 voxels, streamed: same products, same roundings as the ring kernel
            wq = _pk(weight, 'p1f', lambda t: t.detach().reshape(16, 16).to(torch.bfloat16).contiguous())
            y = empty_cl16(tuple(x.shape), x.device, True)
            norm = None
            b_ = bias.detach() if bias is not None else None
            launch('lf_pw16_fwd', x, 1 if x.dtype == torch.bfloat16 else 0, wq, b_, he, flags, SLOPE, y, x.numel() // 16,
                   tag='pw16_fwd', detail=f'{x.shape[0]}:{x.dtype == torch.bfloat16}')
        elif RING_BLOCK_FWD and flags == (LF_EPI_LRELU | LF_EPI_PIXELNORM) and ring_multi_ok(*x.shape[2:]):
            # the same arithmetic on the one-group ring kernel with its epilogue at compile time (LF_RING_EX_BLOCK): bit-identical
            pack = _pk(weight, 'a3f', lambda t: pack_conv3d_c16_ring_bf16(w3(t)))
            y = empty_cl16(tuple(x.shape), x.device, True)
            norm = torch.empty(x.shape[0] * x.shape[2] * x.shape[3] * x.shape[4], device=x.device, dtype=torch.float32)
            ring_multi(x, pack.reshape(1, 14, 16, 32), he, [(y, None, True)], extra=_lib.LF_RING_EX_BLOCK,
                       e0=bias.detach() if bias is not None else None, o2=norm)
        else:
            pack = _pk(weight, 'a3f', lambda t: pack_conv3d_c16_ring_bf16(w3(t)))
            y, norm = conv3d_c16_ring_bf16_io(x, pack, bias.detach() if bias is not None else None, he, flags, 1, out_bf16=True)
        ctx.flags, ctx.he, ctx.one = flags, he, one
        need_w = weight.requires_grad or (bias is not None and bias.requires_grad)
        ctx.save_for_backward(y if flags else None, norm, weight, x if need_w else None)
        ctx.xdtype = x.dtype
        # the producer's side of the chain: what a consumer needs to run this layer's epilogue backward (its activation reaches
        # the consumer as that layer's input), and the box through which the consumer reports having done so
        ctx.box = None
        if CHAIN_EPILOGUE and flags == (LF_EPI_LRELU | LF_EPI_PIXELNORM) and not one:
            ctx.box = _chain_box()
            y._lf_link = (norm, ctx.box)
        ctx.link = None
        if link is not None and x.dtype == torch.bfloat16 and need_w and not one and ring_multi_ok(*x.shape[2:]):
            ctx.link = link                                       # (norm of the producer, its box)
        return y

    @staticmethod
    def backward(ctx, gy):
        y, norm, w, x_saved = ctx.saved_tensors
        gy = cl(gy)
        want_b = ctx.needs_input_grad[2]
        pw_bwd = ctx.pw and ctx.flags == 0 and gy.dtype == torch.bfloat16 and ctx.needs_input_grad[0]
        gp, gb = _Conv16AC._preact_grad(ctx, gy, y, norm, want_b, pw_bwd)
        gx = gw = None
        with autocast(True):
            # the weight gradient first, on the side stream (WGRAD_STREAM): it then runs beside the data gradient below
            wgrad = _Conv16AC._weight_grad_start(ctx, x_saved, gp) if ctx.needs_input_grad[1] else None
            if ctx.needs_input_grad[0]:
                gx, gb = _Conv16AC._data_grad(ctx, w, x_saved, gp, gb, pw_bwd and want_b)
            if ctx.needs_input_grad[1]:
                gw = _Conv16AC._weight_grad_finish(ctx, w, x_saved, gp, wgrad)
        return gx, gw, gb if want_b else None, None, None

    @staticmethod
    def _preact_grad(ctx, gy, y, norm, want_b, pw_bwd):
        """(pre-activation gradient in bf16, bias gradient or None)."""
        if pw_bwd:                                                # no activation: it IS gy; the bias sums ride in lf_pw16_bwd
            return gy, None
        if ctx.box is not None and _chain_take(ctx.box) is not None:
            return _chain_epilogue_bwd(ctx, gy, y, norm, want_b)  # the chained consumer ran this layer's epilogue backward
        if ctx.flags == 0 and not want_b and gy.dtype == torch.bfloat16:
            return gy, None
        return epilogue_bwd_c16(gy, y, norm, ctx.flags, want_b)

    @staticmethod
    def _weight_grad_start(ctx, x_saved, gp):
        """The bf16 weight gradient, launched: (side-stream helper, completion, gwt); None outside its domain (see _weight_grad_finish)."""
        if not _wgrad_bf16_ok(gp, 3, 16, 16):
            return None
        N, D, H, W, _ = _geom(gp, 3)
        gwt = torch.empty(27, 16, 16, device=gp.device, dtype=torch.float32)
        wg = _Wgrad(3, N, D, H, W, 16, 16, gp.device, ctx.he, bf16=True)
        io = (1 if x_saved.dtype == torch.bfloat16 else 0) | 2
        sw = _SideWgrad(gp.device)
        done = sw.run(lambda: wg(x_saved, gp, gwt), x_saved, gp, gwt, wg.scratch, timed=('wgrad3d_c16_bf16', f'{N}:io{io}'))
        return sw, done, gwt

    @staticmethod
    def _weight_grad_finish(ctx, w, x_saved, gp, started):
        if started is not None:
            sw, done, gwt = started
            sw.wait(done)
        else:                                                     # small volumes: the fp32-MFMA kernel on the same bf16 values
            xs = x_saved if x_saved.dtype == torch.bfloat16 else round_bf16(x_saved)
            gwt, _ = conv_bwd_weight(cl(xs.float()), cl(gp.float()), 3, 16, ctx.he, want_bias=False, bf16=False)
        if ctx.one:
            return round_bf16(gwt[13].reshape(w.shape).contiguous())
        return round_bf16(gwt.reshape(3, 3, 3, 16, 16).permute(3, 4, 0, 1, 2).contiguous())

    @staticmethod
    def _data_grad(ctx, w, x_saved, gp, gb, need_gb):
        """(gx in the input's storage type, bias gradient): pointwise / chained-producer / ring-multi / ring-io."""
        if ctx.pw and gp.dtype == torch.bfloat16:
            # pointwise data gradient (+ this layer's bias gradient when nothing ran before it): one streamed pass
            L = _lib.lib()
            wtq = _pk(w, 'p1b', lambda t: t.detach().reshape(16, 16).t().to(torch.bfloat16).contiguous())
            rows = gp.numel() // 16
            out16 = ctx.xdtype == torch.bfloat16
            gx = torch.empty_like(gp, dtype=torch.bfloat16 if out16 else torch.float32, memory_format=torch.preserve_format)
            if need_gb:
                gb = torch.empty(16, device=gp.device, dtype=torch.float32)
                nb = L.lf_pw16_bwd_scratch_bytes(rows)
                scr = torch.empty(nb // 4 + 4, device=gp.device, dtype=torch.float32)
            launch('lf_pw16_bwd', gp, wtq, ctx.he, gx, 1 if out16 else 0, gb if need_gb else None, scr.data_ptr() if need_gb else None,
                   scr.numel() * 4 if need_gb else 0, rows, tag='pw16_bwd', detail=f'{gp.shape[0]}:{out16}')
            return gx, gb
        w3 = (lambda t: pack_center_tap(t)) if ctx.one else (lambda t: t)
        pack_t = _pk(w, 'a3b', lambda t: pack_conv3d_c16_ring_bf16(w3(t), transpose=True))
        if ctx.link is not None and gp.dtype == torch.bfloat16 and _chain_take(ctx.link[1]) is None:
            pnorm, pbox = ctx.link                                # + the PRODUCER's epilogue backward and bias sums: x_saved is its activation
            gx = torch.empty_like(gp)
            gbuf = torch.zeros(_ex_prev_scratch_floats(gp.device), device=gp.device, dtype=torch.float32)
            ring_multi(gp, pack_t.reshape(1, 14, 16, 32), ctx.he, [(gx, None, True)], extra=_lib.LF_RING_EX_PREV, e0=x_saved, e1=pnorm,
                       o2=gbuf)
            _chain_arm(pbox, gx, gbuf[:16])
        elif RING_DGRAD and gp.dtype == torch.bfloat16 and ctx.xdtype == torch.bfloat16:
            # the same sums and roundings on the one-group ring kernel (csrc/conv_gru.hip): bit-identical, 32 instead of 53 us per 128^3
            gx = torch.empty_like(gp)
            ring_multi(gp, pack_t.reshape(1, 14, 16, 32), ctx.he, [(gx, None, True)])
        else:
            gx, _ = conv3d_c16_ring_bf16_io(gp, pack_t, None, ctx.he, 0, 1, out_bf16=ctx.xdtype == torch.bfloat16)
        return gx, gb


def _conv16_ac_ok(x, weight):
    return (storage_bf16() and x.dim() == 5 and weight.dim() == 5 and tuple(weight.shape[:2]) == (16, 16) and x.shape[1] == 16
            and weight.shape[2] in (1, 3) and x.is_cuda and ring_multi_ok(*x.shape[2:]))


class _Conv3x3Sum16(torch.autograd.Function):
    """sum_p conv3d(parts[p], W[:, c0_p : c0_p + w_p]) * he (+ b) (+ addend) for a 16-channel output: a convolution over a
    channel concatenation evaluated WITHOUT the concatenation, as a sum of 16 -> 16 convolutions (the addend form of
    lf_conv3d_c16_wino / lf_conv3d_c16_ring_bf16), one per part.  `parts` are channels-last (N,16,D,H,W) tensors; part p
    stands for the input channels cols[p] = (c0_p, w_p) of W (narrower parts -- the 3 coordinate channels of the ConvGRU
    gates -- are zero-padded to 16 by the caller).  The parts need not cover W: a part that is the same in every call (those
    coordinates) is convolved ONCE, bias included, and handed to the other calls as `addend`; autograd then sums its
    gradient over the calls, and its weight / bias gradients are one launch instead of one per call.  Backward: per-part
    data gradients on the same kernel, weight gradients on the LDS-staged 16 -> 16 kernels, no slice copies."""

    @staticmethod
    def forward(ctx, weight, bias, cols, addend, *parts):
        _req(weight, 'weight')
        assert weight.dim() == 5 and weight.shape[0] == 16 and len(cols) == len(parts) >= 1
        assert all(0 <= c0 and 0 < wdt <= 16 and c0 + wdt <= weight.shape[1] for c0, wdt in cols)
        he = he_constant(weight)

        ctx.ac = ops.AUTOCAST is not None
        # autocast: the bf16 ring kernel (and the bf16 weight-gradient kernel) round their operands while staging them; only
        # volumes the latter does not take keep the rounding pass in front
        ctx.pre_round = ctx.ac and not _wgrad_bf16_ok(parts[0], 3, 16, 16)
        parts = tuple((round_bf16(cl(p)) if ctx.pre_round else cl(p)) for p in parts)

        def make():
            wd, packs = _wsrc(weight).detach(), []
            pack = pack_conv3d_c16_ring_bf16 if ctx.ac else pack_conv3d_c16_wino
            for c0, wdt in cols:
                wp = wd.new_zeros(16, 16, 3, 3, 3)
                wp[:, :wdt] = wd[:, c0:c0 + wdt]
                packs.append((pack(wp), pack(wp, transpose=True)))
            return packs
        packs = _cached(weight, 'sum16_' + '_'.join(f'{c0}+{wdt}' for c0, wdt in cols) + ('@ac' if ctx.ac else ''), make)
        y = cl(addend) if addend is not None else None
        for i, (p, (pf, _pt)) in enumerate(zip(parts, packs)):
            _req(p, 'part')
            b = bias.detach() if (bias is not None and i == 0) else None
            if b is not None and y is not None:                  # (the addend forms take no bias: fold it in beforehand)
                y = y + b.view(1, -1, 1, 1, 1)
                b = None
            if ctx.ac:
                y, _ = conv3d_c16_ring_bf16(p, pf, b, he, 0, 0, addend=y)
            else:
                prev = None if y is None else (y, None, _lib.LF_EPI_ADD)
                y, _ = conv3d_c16_wino(p, pf, b, he, 0, prev=prev)
        ctx.he, ctx.cols, ctx.packs = he, cols, packs
        need_w = weight.requires_grad or (bias is not None and bias.requires_grad)
        ctx.save_for_backward(weight, *(parts if need_w else []))
        return y

    @staticmethod
    def backward(ctx, gy):
        gy = cl(gy)
        gy_full = gy
        w, *saved_parts = ctx.saved_tensors
        if ctx.pre_round:
            gy = round_bf16(gy)
        gparts = []
        for i, (_pf, pt) in enumerate(ctx.packs):
            if not ctx.needs_input_grad[4 + i]:
                gparts.append(None)
            elif ctx.ac:
                gparts.append(conv3d_c16_ring_bf16(gy, pt, None, ctx.he, 0, 1)[0])     # (rounded like autocast's conv backward)
            else:
                gparts.append(conv3d_c16_wino(gy, pt, None, ctx.he, 0)[0])
        gw = gb = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            gwt = torch.zeros(27, 16, w.shape[1], device=gy.device, dtype=torch.float32)      # columns of other calls stay zero
            for i, (p, (c0, wdt)) in enumerate(zip(saved_parts, ctx.cols)):
                g_i, gb_i = conv_bwd_weight(p, gy, 3, 16, ctx.he, want_bias=(i == 0 and ctx.needs_input_grad[1] and not ctx.ac), bf16=ctx.ac)
                gb = gb_i if i == 0 else gb
                gwt[:, :, c0:c0 + wdt] = g_i[:, :, :wdt]
            gw = gwt.reshape(3, 3, 3, 16, w.shape[1]).permute(3, 4, 0, 1, 2).contiguous()
            if ctx.ac:
                gw = round_bf16(gw)
                if ctx.needs_input_grad[1]:
                    gb = bias_grad(gy_full, 3)
        return (gw if ctx.needs_input_grad[0] else None, gb if ctx.needs_input_grad[1] else None, None,
                gy_full if ctx.needs_input_grad[3] else None, *gparts)


def ring_multi(x, wpacks, he, outs, extra=0, e0=None, e1=None, o2=None, addend_per_sample=True):
    """lf_conv3d_c16_ring_multi: ONE staged (N,16,D,H,W) channels-last volume `x` (bf16 or fp32 storage) convolved with 1 or 2
    ring-kernel weight packs.  wpacks: the packs back to back ((ngroups,14,16,32) bf16); outs: per group (y, addend or None, round)
    -- y / addend fp32 or bf16 channels-last volumes (their dtypes select the storage flags), round: bf16(bf16(conv) * he) instead
    of fma(conv, he, addend).  extra / e0 / e1 / o2: the fused element-wise stage (LF_RING_EX_*, include/lf_hip.h)."""
    N, _, D, H, W = x.shape
    ng = len(outs)
    assert wpacks.dtype == torch.bfloat16 and wpacks.numel() == ng * 14 * 512 and wpacks.is_contiguous()
    args = []
    for y, add, rnd in outs:
        fl = ((_lib.LF_RING_OUT_BF16 if y.dtype == torch.bfloat16 else 0) | (_lib.LF_RING_ROUND if rnd else 0)
              | (_lib.LF_RING_ADD_BF16 if (add is not None and add.dtype == torch.bfloat16) else 0))
        args += [y, add, fl]
    if ng == 1:
        args += [None, None, 0]
    fl0 = args[2] | (8 if outs[0][1] is not None else 0)           # group 0's epilogue form, as the kernel template sees it
    launch('lf_conv3d_c16_ring_multi', x, int(x.dtype == torch.bfloat16), wpacks, ng, *args, extra, e0, e1, o2, N, D, H, W, he,
           int(bool(addend_per_sample)), tag='conv3d_c16_ring_multi', detail=f'{ng}:{extra}:{N}:{fl0}:{x.element_size()}')


class _GruGates(torch.autograd.Function):
    """(upre, rpre, h) -> (u = sigmoid(upre), rh = h * sigmoid(rpre)); one kernel each way (lf_gru_stage_a[_bwd])
    instead of five element-wise passes over the volume (modules/gru.py:37-40)."""

    @staticmethod
    def forward(ctx, upre, rpre, h):
        upre, rpre, h = cl(upre), cl(rpre), cl(h)
        u, rh = torch.empty_like(h), torch.empty_like(h)
        C = h.shape[1]
        nvox = h.numel() // C
        launch('lf_gru_stage_a', upre, rpre, C, h, u, rh, nvox, C, C, 0)
        ctx.save_for_backward(u, rpre, h)
        return u, rh

    @staticmethod
    def backward(ctx, gu, grh):
        u, rpre, h = ctx.saved_tensors
        gu, grh = cl(gu), cl(grh)
        gupre, grpre, gh = torch.empty_like(h), torch.empty_like(h), torch.empty_like(h)
        launch('lf_gru_stage_a_bwd', gu, grh, u, rpre, h, gupre, grpre, gh, h.numel())
        return gupre, grpre, gh


class _GruBlend(torch.autograd.Function):
    """(h, u, cand) -> h (1 - u) + cand u  (modules/gru.py:42; lf_gru_stage_b[_bwd])."""

    @staticmethod
    def forward(ctx, h, u, cand):
        h, u, cand = cl(h), cl(u), cl(cand)
        out = torch.empty_like(h)
        C = h.shape[1]
        launch('lf_gru_stage_b', h, u, cand, out, None, h.numel() // C, C, C, 0)
        ctx.save_for_backward(h, u, cand)
        return out

    @staticmethod
    def backward(ctx, g):
        h, u, cand = ctx.saved_tensors
        g = cl(g)
        gh, gu, gc = torch.empty_like(h), torch.empty_like(h), torch.empty_like(h)
        launch('lf_gru_stage_b_bwd', g, h, u, cand, gh, gu, gc, h.numel())
        return gh, gu, gc


class _LstmCell(torch.autograd.Function):
    """(cc (N,4Ch,...), c) -> (h', c') of the ConvLSTM cell (modules/lstm.py:49-56; lf_lstm_cell_fwd/bwd): one kernel each
    way instead of four activations, three products and a split."""

    @staticmethod
    def forward(ctx, cc, c_cur):
        cc, c_cur = cl(_req(cc, 'cc')), cl(_req(c_cur, 'c'))
        Ch = c_cur.shape[1]
        if cc.shape[1] != 4 * Ch:
            raise ValueError('lstm_cell: cc must hold 4 x hidden channels')
        h, cn = torch.empty_like(c_cur), torch.empty_like(c_cur)
        launch('lf_lstm_cell_fwd', cc, c_cur, h, cn, c_cur.numel() // Ch, Ch)
        ctx.save_for_backward(cc, c_cur)
        ctx.set_materialize_grads(False)
        return h, cn

    @staticmethod
    def backward(ctx, gh, gcn):
        cc, c_cur = ctx.saved_tensors
        if gh is None and gcn is None:
            return None, None
        Ch = c_cur.shape[1]
        gh = cl(gh) if gh is not None else None
        gcn = cl(gcn) if gcn is not None else None
        gcc, gc = torch.empty_like(cc), torch.empty_like(c_cur)
        launch('lf_lstm_cell_bwd', cc, c_cur, gh, gcn, gcc, gc, c_cur.numel() // Ch, Ch)
        return gcc, gc


def lstm_cell(cc, c_cur):
    return _LstmCell.apply(cc, c_cur)


def gru_gates(upre, rpre, h):
    return _GruGates.apply(upre, rpre, h)


def gru_blend(h, u, cand):
    return _GruBlend.apply(h, u, cand)


def conv3x3_sum16(weight, bias, widths, parts, cols=None, addend=None):
    """See _Conv3x3Sum16.  `widths`: the parts cover W's input channels back to back; or `cols` = ((first, width), ...)."""
    if cols is None:
        cols, c0 = [], 0
        for wdt in widths:
            cols.append((c0, wdt))
            c0 += wdt
        assert c0 == weight.shape[1]
    return _Conv3x3Sum16.apply(weight, bias, tuple(tuple(c) for c in cols), addend, *parts)


class _LiftView(torch.autograd.Function):
    """(V, c0*S, H, W) channels-last, channel = c*S + d  ->  (V, c0, S, H, W) channels-last volume: the `.view` of
    FactorProjection2d3d (modules/geometry.py:728) as ONE permutation kernel each way (lf_lift_permute) instead of a
    strided ATen copy (1.9 ms per GB here; the kernel moves full lines both sides)."""

    @staticmethod
    def forward(ctx, y, c0, S):
        y = cl(y)
        V, cs, H, W = y.shape
        ctx.dims = (V, H, W, c0, S)
        return _lift_permute(y, V, H * W, c0, S, False, empty_cl((V, c0, S, H, W), y.device))

    @staticmethod
    def backward(ctx, g):
        V, H, W, c0, S = ctx.dims
        return _lift_permute(cl(g), V, H * W, c0, S, True, empty_cl((V, c0 * S, H, W), g.device)), None, None


def _lift_fused_ok(c0, S):
    return c0 % 4 == 0 and S % 4 == 0 and (2 * 4 * c0 * (S + 1) + 16) * 4 <= 150 * 1024


class _LiftFused(torch.autograd.Function):
    """FactorProjection2d3d with a gradient (training step), two passes each way: pointwise conv + LeakyReLU as rows, then
    lf_lift_norm_unfold (PixelNorm over all C0*S channels + the layout change into the channels-last volume, bf16 storage under
    the autocast storage policy); backward lf_lift_bwd (PixelNorm' / LeakyReLU' from the volume-layout gradient and the saved
    volume, written as rows) feeding the weight / data gradient products.  Replaces conv1x1 + PixelNorm pass + lift_permute
    (and their three backward passes): the (V, C0*S, H, W) activation is never stored."""

    @staticmethod
    def forward(ctx, x, weight, bias, S):
        _req(x, 'x'), _req(weight, 'weight')
        ctx.ac = ops.AUTOCAST is not None
        x = _ac_in(cl(x))
        V, cin, H, W = x.shape
        cs = weight.shape[0]
        c0 = cs // S
        P = H * W
        he = he_constant(weight)
        ctx.mfma = bool(LIFT_MFMA and ctx.ac and storage_bf16() and c0 == 16 and cin == 16 and S in (16, 32, 64, 128) and P % 16 == 0)
        if ctx.mfma:
            # round 6 (csrc/lift_mfma.hip): K = 16 -- the 16*S-channel row is recomputed by MFMA instead of stored as fp32 rows
            wtab = _pk(weight, 'l16f', lambda w: w.reshape(16, S, 16).permute(1, 0, 2).contiguous().to(torch.bfloat16))
            btab = bias.detach().reshape(16, S).t().contiguous() if bias is not None else None
            vol = empty_cl16((V, c0, S, H, W), x.device, True)
            norm = torch.empty(V * P, device=x.device, dtype=torch.float32)
            launch('lf_lift16_fwd', x, wtab, btab, vol, norm, V * P, P, S, he, SLOPE, PN_EPS, tag='lift16_fwd')
            ctx.dims, ctx.he = (V, cin, H, W, c0, S), he
            ctx.save_for_backward(vol, norm, weight, x)
            return vol
        wpack = _pk(weight, 'c1f', lambda w: pack_conv1x1(w.reshape(cs, cin)))
        tmp = torch.empty(V * P, cs, device=x.device, dtype=torch.float32)
        _conv1x1_raw(x, wpack, bias.detach() if bias is not None else None, V, P, cin, 1, P * cin, 0, cs, tmp, he, LF_EPI_LRELU)
        out16 = storage_bf16() and c0 == 16
        vol = empty_cl16((V, c0, S, H, W), x.device, out16)
        norm = torch.empty(V * P, device=x.device, dtype=torch.float32)
        launch('lf_lift_norm_unfold', tmp, vol, norm, V, P, c0, S, PN_EPS, int(out16), tag='lift_norm_unfold')
        del tmp
        ctx.dims, ctx.he = (V, cin, H, W, c0, S), he
        ctx.save_for_backward(vol, norm, weight, x)
        return vol

    @staticmethod
    def backward(ctx, g):
        L = _lib.lib()
        vol, norm, w, x = ctx.saved_tensors
        V, cin, H, W, c0, S = ctx.dims
        cs, P = c0 * S, H * W
        g = cl(g)
        if ctx.mfma and g.dtype == torch.bfloat16 and vol.dtype == torch.bfloat16:
            wtab_t = _pk(w, 'l16b', lambda t: t.reshape(16, S, 16).permute(1, 2, 0).contiguous().to(torch.bfloat16))
            gx = empty_cl((V, cin, H, W), g.device)
            gw = torch.empty(cs, cin, device=g.device, dtype=torch.float32)
            gb = torch.empty(cs, device=g.device, dtype=torch.float32)
            nb = L.lf_lift16_bwd_scratch_bytes(S)
            scr = torch.empty(nb // 4 + 4, device=g.device, dtype=torch.float32)
            launch('lf_lift16_bwd', g, vol, norm, x, wtab_t, gx, gw, gb, scr.data_ptr(), scr.numel() * 4, V * P, P, S, ctx.he,
                   SLOPE, 1, tag='lift16_bwd')
            return (gx if ctx.needs_input_grad[0] else None, _ac_in(gw.reshape(w.shape)) if ctx.needs_input_grad[1] else None,
                    gb if ctx.needs_input_grad[2] else None, None)
        gp = torch.empty(V * P, cs, device=g.device, dtype=torch.float32)
        io = (1 if g.dtype == torch.bfloat16 else 0) | (2 if vol.dtype == torch.bfloat16 else 0)
        launch('lf_lift_bwd', g, vol, norm, gp, V, P, c0, S, SLOPE, int(ctx.ac), io, tag='lift_bwd')
        gx = gw = gb = None
        with autocast(ctx.ac):
            if ctx.needs_input_grad[0]:
                wpack_t = _pk(w, 'c1b', lambda t: pack_conv1x1(t.reshape(cs, cin).t()))
                gx = empty_cl((V, cin, H, W), g.device)
                _conv1x1_raw(gp, wpack_t, None, V, P, cs, 1, P * cs, 0, cin, gx, ctx.he, 0)
                gx = _ac_in(gx)
            if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
                gwt, gb = conv_bwd_weight(x.permute(0, 2, 3, 1).reshape(V * P, cin), gp, 0, cin, ctx.he, want_bias=not ctx.ac)
                if ctx.ac and ctx.needs_input_grad[2]:
                    gb = bias_grad(gp, 0)              # (of the rounded rows: 5e5 roundings of 2^-9 average out far below fp32's own noise)
                gw = _ac_in(gwt.reshape(w.shape))
        return gx, gw if ctx.needs_input_grad[1] else None, gb if ctx.needs_input_grad[2] else None, None
