"""Device operators of the hot path: thin autograd wrappers over the C ABI (include/lf_hip.h).

Tensors keep the reference's LOGICAL shapes (N,C,D,H,W) / (N,C,H,W) but live in channels-last
memory (torch.channels_last_3d / torch.channels_last), which is exactly the [N][D][H][W][C]
layout the kernels use -- so the modules built on these ops are shape-compatible drop-ins for
the reference's nn.Modules without any transposes between layers.

There is no CPU or ATen fallback in this file: every op calls into liblf_hip.so.
"""
import math

import torch

from . import _lib
from ._lib import LF_EPI_LRELU, LF_EPI_PIXELNORM, LF_MAP_C2O, LF_MAP_COEFS, LF_MAP_O2C

SLOPE = 0.2
PN_EPS = 1e-8
# d(loss)/d(sampled volume) of the 3-D resamplers (training / encoder backward): True = fixed-point accumulation,
# bit-reproducible (lf_resample3d_bwd_vol_det); False = fp32 atomics (lf_resample3d_bwd_vol, order-dependent rounding)
DETERMINISTIC_SPLAT = True

# bf16 autocast policy of the training step (reference: `autocast(enabled=self.training)` around Sculptor / Photographer
# .forward, recon/models.py:199,405; tools/train/train_reconstruct.py:455).  Inside `with ops.autocast():` every
# convolution (3x3(x3), 1x1, factor projections, GRU gates) sees bf16-rounded inputs and weights with fp32 accumulation,
# its data / weight gradients likewise and rounded to bf16, exactly the tensors torch autocast hands to / takes from the
# convolution; everything else (bias, LeakyReLU, PixelNorm, resampling, losses, master weights, Adam) stays fp32.
# The 3-D 16 -> 16 blocks run on the bf16 MFMA (lf_conv3d_c16_bf16, forward and data gradient); the other layers round
# their operands (lf_round_bf16) and keep the fp32-MFMA kernels, which then compute what a bf16 MFMA would (bf16 x bf16
# products are exact in fp32).
AUTOCAST = None
# Storage policy under autocast (round 5): the 16-channel 3-D volumes that half-precision convolutions produce and consume
# -- block activations, their gradients, the resampled volumes between them, the per-view latent volumes -- are kept as
# bf16 channels-last tensors (32 B per voxel).  The convolutions round their inputs to bf16 while staging them anyway, so a
# volume that only convolutions read loses nothing; a volume that an fp32 stage also reads (PixelNorm' / LeakyReLU' of the
# epilogue backward, the trilinear resampler) is read rounded.  Halves the HBM bytes and the saved-activation memory of the
# training step.  False: fp32 storage everywhere (the round-2..4 behaviour), kept for A/B runs and tests.
BF16_STORAGE = True


def storage_bf16():
    return AUTOCAST is not None and BF16_STORAGE


def _f32(t):
    """An fp32 view of a tensor an op without a bf16-storage form was handed (a cast pass; the hot ops take bf16 natively)."""
    return t if t.dtype == torch.float32 else t.float()


class autocast:
    def __init__(self, enabled=True):
        self.enabled = enabled

    def __enter__(self):
        global AUTOCAST
        self.prev = AUTOCAST
        AUTOCAST = 'bf16' if self.enabled else None
        return self

    def __exit__(self, *exc):
        global AUTOCAST
        AUTOCAST = self.prev
        return False


def round_bf16(t):
    """bf16(t) in an fp32 container of the same layout (lf_round_bf16)."""
    _req(t, 'tensor')
    src = t if (t.is_contiguous() or t.is_contiguous(memory_format=torch.channels_last)
                or (t.dim() == 5 and t.is_contiguous(memory_format=torch.channels_last_3d))) else t.contiguous()
    out = torch.empty_like(src, memory_format=torch.preserve_format)
    launch('lf_round_bf16', src, out, src.numel())
    return out


def _ac_in(t):
    """An operand as the convolution sees it under the active policy."""
    return round_bf16(t) if AUTOCAST is not None else t

# Optional per-kernel timing with HIP events on the launch stream (used by bench.py for the
# roofline of the dominant kernel).  Set to a list to collect (name, start_event, end_event).
KERNEL_TIMER = None
# Restrict the events to these kernel tags (None = every tagged launch).  An event pair costs ~4-5 us of dispatch gap
# around its kernel: bench.py times only the kernels its roofline fields report.
KERNEL_TIMER_TAGS = None


class _Tag(str):
    """A kernel tag that compares like its name and carries a `detail` (form / batch / storage of the launch)."""
    detail = ''


class _timed:
    def __init__(self, name, detail=''):
        self.name = _Tag(name)
        self.name.detail = detail
        self.on = False

    def __enter__(self):
        self.on = KERNEL_TIMER is not None and (KERNEL_TIMER_TAGS is None or self.name in KERNEL_TIMER_TAGS)
        if self.on:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e1 = torch.cuda.Event(enable_timing=True)
            self.e0.record()                    # current stream == the stream the kernel is launched on
        return self

    def __exit__(self, *exc):
        if self.on and KERNEL_TIMER is not None:
            self.e1.record()
            KERNEL_TIMER.append((self.name, self.e0, self.e1))
        return False



def _T():
    """The training-step operators (ops_train.py), imported on first use: that module builds on this one."""
    from . import ops_train
    return ops_train


def __getattr__(name):
    """`ops.<name>` for the operators that live in ops_train.py (training step: weight gradients, bf16-storage layers, the
    fused ConvGRU recurrence / lift) and experimental.py (A/B and superseded kernels, include/lf_hip_experimental.h)."""
    import importlib
    if name.startswith('__'):                                 # (the import system probing `__path__`: not an operator, and the modules
        raise AttributeError(name)                            # below import names from this one while they load)
    for mod in ('ops_train', 'gru_train', 'experimental'):
        m = importlib.import_module('.' + mod, __package__)
        if name in m.__dict__:
            return m.__dict__[name]
    raise AttributeError(f'module {__name__!r} has no attribute {name!r}')

def _stream():
    return torch.cuda.current_stream().cuda_stream


def _req(t, name):
    if not t.is_cuda:
        raise _lib.LFHipError(f'{name} must be a device tensor: the HIP path has no CPU fallback')
    if t.dtype != torch.float32:
        raise TypeError(f'{name} must be float32')
    return t


def cl(t):
    """channels-last physical layout for a logical NC[D]HW tensor (no copy if already so)."""
    if t.dim() == 5:
        return t.contiguous(memory_format=torch.channels_last_3d)
    if t.dim() == 4:
        return t.contiguous(memory_format=torch.channels_last)
    raise ValueError('expected a 4-D or 5-D tensor')


def empty_cl(shape, device):
    fmt = torch.channels_last_3d if len(shape) == 5 else torch.channels_last
    return torch.empty(shape, device=device, dtype=torch.float32, memory_format=fmt)


def _ptr(t, scratch=False):
    if _lib.BYTE_LOG is not None:
        _lib.note_bytes(t, scratch)
    return t.data_ptr()


_Tensor = torch.Tensor
_LAUNCH_PLAN = {}          # entry point -> (arity with the stream, positions of its c_void_p arguments)


def launch(name, *args, tag=None, detail=''):
    """THE call of a library entry point `int lf_x(..., void* stream)` on the current stream: `args` are its C arguments
    without the stream.  At a void* position a tensor goes as its data_ptr() and is counted in the byte accounting as _ptr
    counts it (once per argument); None is NULL; anything else goes as it is, so an int there is an uncounted pointer (scratch
    buffers, pointer arithmetic).  A wrong argument count is a TypeError (ctypes would take surplus arguments silently), a
    non-zero return code an LFHipError naming the entry point.  tag: run inside _timed(tag, detail)."""
    plan = _LAUNCH_PLAN.get(name)
    if plan is None:
        res, argtypes = _lib.SIGNATURES.get(name) or _lib.EXPERIMENTAL_SIGNATURES[name]
        assert res is _lib.c_int and argtypes[-1] is _lib.P, f'{name} is not a launch: int lf_x(..., void* stream)'
        plan = _LAUNCH_PLAN[name] = (len(argtypes), tuple(i for i, t in enumerate(argtypes[:-1]) if t is _lib.P))
    if len(args) + 1 != plan[0]:
        raise TypeError(f'{name} takes {plan[0] - 1} arguments before the stream, got {len(args)}')
    a = list(args)
    for i in plan[1]:
        t = a[i]
        if t is not None and isinstance(t, _Tensor):
            a[i] = t.data_ptr()
    if _lib.BYTE_LOG is not None:                                 # (one branch per launch, not per pointer)
        for i in plan[1]:
            if isinstance(args[i], _Tensor):
                _lib.note_bytes(args[i])
    fn = getattr(_lib.lib(), name)
    if tag is None or KERNEL_TIMER is None:                       # (no timer: not even the _timed object)
        rc = fn(*a, _stream())
    else:
        with _timed(tag, detail):
            rc = fn(*a, _stream())
    _lib.check(rc, name)


def _prev(prev):
    """(y, norm, flags) of the layer whose epilogue backward a launch folds in -> its prev_y, prev_norm, prev_flags arguments."""
    return (prev[0], prev[1], prev[2]) if prev is not None else (None, None, 0)


def _norm_buf(flags, rows, device):
    """The per-row norms a PixelNorm epilogue saves for its backward (None without one)."""
    return torch.empty(rows, device=device, dtype=torch.float32) if flags & LF_EPI_PIXELNORM else None


# ---------------------------------------------------------------------------------------------
# weight packing (host side, cached per parameter version)
# ---------------------------------------------------------------------------------------------
_WEIGHT_EPOCH = 0


def invalidate_weight_packs():
    """Call after writing parameters through a raw pointer (e.g. lf_adam_step on a flat buffer): such writes
    do not bump torch's version counters, so the cached packs must be told."""
    global _WEIGHT_EPOCH
    _WEIGHT_EPOCH += 1


def _cached(key_tensor, tag, fn):
    """Memoises a packed layout ON the parameter object (so it dies with it and can never be
    confused with another tensor that later reuses the same device address); re-packs when the
    parameter is modified in place (version counter), moved, or when an optimiser that writes through
    raw pointers announced an update (invalidate_weight_packs)."""
    store = key_tensor.__dict__.setdefault('_lf_pack', {})
    stamp = (key_tensor._version, key_tensor.data_ptr(), _WEIGHT_EPOCH)
    hit = store.get(tag)
    if hit is None or hit[0] != stamp:
        hit = (stamp, fn())
        store[tag] = hit
    return hit[1]


def _wsrc(weight):
    """The weight tensor the kernels should see: the parameter itself, or its bf16 rounding under autocast."""
    if AUTOCAST is None:
        return weight
    return _cached(weight, 'ac_round', lambda: round_bf16(weight.detach()))


def _pk(weight, tag, fn):
    """Cached packed layout of `weight` (of its bf16 rounding under autocast) -- fn(tensor) builds it."""
    return _cached(weight, tag + ('@ac' if AUTOCAST is not None else ''), lambda: fn(_wsrc(weight)))


def _pad16(v):
    return (v + 15) // 16 * 16


def pack_conv3x3(weight, transpose=False):
    """[Cout,Cin,k..] -> [tap][CoutP][CinP] (lf_conv3x3_fwd layout).  transpose=True builds the
    data-gradient operator: taps flipped, in/out channels swapped."""
    L = _lib.lib()
    w = weight.detach()
    if transpose:
        w = w.transpose(0, 1).flip(dims=tuple(range(2, w.dim())))
    cout, cin = w.shape[0], w.shape[1]
    taps = w[0, 0].numel()
    coutp, cinp = L.lf_conv3x3_cout_padded(cout), _pad16(cin)
    out = torch.zeros(taps, coutp, cinp, device=w.device, dtype=torch.float32)
    out[:, :cout, :cin] = w.reshape(cout, cin, taps).permute(2, 0, 1)
    return out.contiguous()


def pack_conv1x1(weight2d):
    """[Cout,K] -> [CoutP][Kp] (lf_conv1x1_fwd layout)."""
    L = _lib.lib()
    cout, k = weight2d.shape
    out = torch.zeros(L.lf_conv1x1_cout_padded(cout), _pad16(k), device=weight2d.device, dtype=torch.float32)
    out[:cout, :k] = weight2d.detach()
    return out.contiguous()


def pack_rows_gemm(weight2d):
    """[Cout,K] -> [CoutP][K] row-major, rows Cout.. zero (lf_rows_gemm_epi layout; CoutP = lf_rows_gemm_cout_padded(Cout))."""
    L = _lib.lib()
    cout, k = weight2d.shape
    coutp = L.lf_rows_gemm_cout_padded(cout)
    if coutp == 0 or cout < 16 or cout % 4 or k < 4 or k % 4:
        raise ValueError(f'lf_rows_gemm_epi takes 16 <= Cout <= 256, Cout % 4 == 0, K >= 4, K % 4 == 0: got Cout {cout}, K {k}')
    out = torch.zeros(coutp, k, device=weight2d.device, dtype=torch.float32)
    out[:cout] = weight2d.detach()
    return out.contiguous()


def amax_buffer(value=None, device='cuda', rows=1):
    """Zeroed max-abs side-channel buffer(s) (rows x LF_AMAX_FLOATS); `value` (a tensor) pre-loads slot 0 of
    row 0, e.g. a maximum computed on the host side of the ABI."""
    buf = torch.zeros(rows, _lib.LF_AMAX_FLOATS, device=device, dtype=torch.float32)
    if value is not None:
        buf[0, 0] = value.reshape(()).to(device)
    return buf


_PAIR_TABLE = {}


def _pair_taps(w):
    """[16 cout][16 cin][3,3,3] -> [14 pairs][16 cout][32 = 2 taps x 16 cin] in the tap-pair order of the ring kernels
    (lf_conv3d_c16_split_pairs; a missing second tap = zeros): one gather, not 28 slice copies per pack -- the training
    step repacks every weight every iteration."""
    idx = _PAIR_TABLE.get(w.device)
    if idx is None:
        import ctypes
        table = (ctypes.c_int * 28)()
        _lib.lib().lf_conv3d_c16_split_pairs(table)
        idx = _PAIR_TABLE[w.device] = torch.tensor([t if t >= 0 else 27 for t in table], device=w.device)
    taps = torch.cat((w.reshape(16, 16, 27), w.new_zeros(16, 16, 1)), dim=2)       # tap 27 = zeros
    return taps[:, :, idx].reshape(16, 16, 14, 2).permute(2, 0, 3, 1).reshape(14, 16, 32)


def pack_conv3d_c16_split(weight, transpose=False):
    """[16,16,3,3,3] fp32 -> f16 hi/lo packs [14 pairs][hi,lo][16 cout][32 = 2 taps x 16 cin] for
    lf_conv3d_c16_split (the second tap of the last pair is zero)."""
    w = weight.detach().float()
    if transpose:
        w = w.transpose(0, 1).flip(dims=(2, 3, 4))
    assert tuple(w.shape) == (16, 16, 3, 3, 3)
    k = _pair_taps(w)                                              # [14 pairs][cout][tapsel*16 + cin]
    hi = k.half()
    lo = (k - hi.float()).half()
    return torch.stack((hi, lo), dim=1).contiguous()              # [14][2][16][32]


def conv3d_c16_split(x, wsplit, bias, he, flags, prev=None, amax_in=None, amax_out=None, want_norm=True):
    """Launch lf_conv3d_c16_split on a channels-last (N,16,D,H,W) tensor."""
    N, _, D, H, W = x.shape
    y = empty_cl((N, 16, D, H, W), x.device)
    norm = _norm_buf(flags, N * D * H * W, x.device)
    py, pn, pf = _prev(prev)
    launch('lf_conv3d_c16_split', x, wsplit, bias, y, norm, N, D, H, W, he, flags, SLOPE, PN_EPS, py, pn, pf, amax_in, amax_out,
           tag='conv3d_c16_split')
    return y, norm


def pack_conv3d_c16_ring_bf16(weight, transpose=False):
    """[16,16,3,3,3] -> bf16 [14 pairs][16 cout][32 = 2 taps x 16 cin] for lf_conv3d_c16_ring_bf16 (the tap pairs of
    lf_conv3d_c16_split_pairs; the second tap of the last pair is zero)."""
    w = weight.detach().float()
    if transpose:
        w = w.transpose(0, 1).flip(dims=(2, 3, 4))
    assert tuple(w.shape) == (16, 16, 3, 3, 3)
    k = _pair_taps(w)
    return k.to(torch.bfloat16).contiguous()


def conv3d_c16_ring_bf16(x, wpack, bias, he, flags, round_out, addend=None):
    """Launch lf_conv3d_c16_ring_bf16 on a channels-last (N,16,D,H,W) tensor (un-rounded input: the kernel rounds)."""
    N, _, D, H, W = x.shape
    y = empty_cl((N, 16, D, H, W), x.device)
    norm = _norm_buf(flags, N * D * H * W, x.device)
    launch('lf_conv3d_c16_ring_bf16', x, wpack, bias, y, norm, N, D, H, W, he, flags, SLOPE, PN_EPS, addend, round_out,
           tag='conv3d_c16_ring_bf16', detail=f"{'add' if addend is not None else 'fwd'}:{N}:io0")
    return y, norm


def empty_cl16(shape, device, bf16):
    """A channels-last (N,16,D,H,W) volume in fp32 or bf16 storage."""
    return torch.empty(shape, device=device, dtype=torch.bfloat16 if bf16 else torch.float32, memory_format=torch.channels_last_3d)


def conv3d_c16_ring_bf16_io(x, wpack, bias, he, flags, round_out, addend=None, out=None, out_bf16=False):
    """lf_conv3d_c16_ring_bf16_io: the bf16 ring convolution on volumes stored as fp32 OR bf16 channels-last records (the
    dtype of `x` / `addend` / `out` says which).  `out`: write into this (N,16,D,H,W) channels-last tensor (e.g. a slice of a
    gradient block) instead of a new one.  Returns (y, norm)."""
    N, _, D, H, W = x.shape
    y = out if out is not None else empty_cl16((N, 16, D, H, W), x.device, out_bf16)
    io = ((_lib.LF_IO_IN_BF16 if x.dtype == torch.bfloat16 else 0) | (_lib.LF_IO_OUT_BF16 if y.dtype == torch.bfloat16 else 0)
          | (_lib.LF_IO_ADDEND_BF16 if (addend is not None and addend.dtype == torch.bfloat16) else 0))
    norm = _norm_buf(flags, N * D * H * W, x.device)
    launch('lf_conv3d_c16_ring_bf16_io', x, wpack, bias, y, norm, N, D, H, W, he, flags, SLOPE, PN_EPS, addend, round_out, io,
           tag='conv3d_c16_ring_bf16', detail=f"{'add' if addend is not None else 'fwd'}:{N}:io{io}")
    return y, norm


_WINO_G = ((1.0, 0.0, 0.0), (0.5, 0.5, 0.5), (0.5, -0.5, 0.5), (0.0, 0.0, 1.0))


def pack_conv3d_c16_wino(weight, transpose=False):
    """[16,16,3,3,3] fp32 -> Winograd-domain pack [4 a][16 b*4+c][4 i][64 lanes] for lf_conv3d_c16_wino:
    U = (G x G x G) w evaluated in fp64, rounded once to fp32."""
    w = weight.detach()
    if transpose:
        w = w.transpose(0, 1).flip(dims=(2, 3, 4))
    assert tuple(w.shape) == (16, 16, 3, 3, 3)
    G = torch.tensor(_WINO_G, dtype=torch.float64, device=w.device)
    U = torch.einsum('ai,bj,ck,omijk->abcom', G, G, G, w.double())          # [a][b][c][cout][cin]
    U = U.reshape(4, 16, 16, 4, 4)                                          # [a][bc][cout][kg][i]
    U = U.permute(0, 1, 4, 3, 2).reshape(4, 16, 4, 64)                      # [a][bc][i][lane = kg*16 + cout]
    return U.float().contiguous()


def conv3d_c16_wino(x, upack, bias, he, flags, prev=None, amax_out=None, out=None):
    """Launch lf_conv3d_c16_wino on a channels-last (N,16,D,H,W) tensor (`out`: write into this tensor)."""
    N, _, D, H, W = x.shape
    y = out if out is not None else empty_cl((N, 16, D, H, W), x.device)
    norm = _norm_buf(flags, N * D * H * W, x.device)
    py, pn, pf = _prev(prev)
    launch('lf_conv3d_c16_wino', x, upack, bias, y, norm, N, D, H, W, he, flags, SLOPE, PN_EPS, py, pn, pf, amax_out,
           tag='conv3d_c16_wino')
    return y, norm


def pack_wino_proj(wp_dmajor, transpose=False):
    """Depth slices of the factor projection for the fused forms of lf_conv3d_c16_wino (include/lf_hip.h):
    wp_dmajor = the (16, D*16) matrix lf_conv1x1_fwd takes (K = d*16 + c) -> [D][64 lanes][4].
    transpose=False: A operands of the forward projection, [d][l][i] = Wp[l & 15][d*16 + (l >> 4)*4 + i];
    transpose=True : A operands of its data gradient,      [d][l][i] = Wp[(l >> 4)*4 + i][d*16 + (l & 15)]."""
    w = wp_dmajor.detach()
    cout, K = w.shape
    assert cout == 16 and K % 16 == 0
    D = K // 16
    if not transpose:
        out = w.reshape(16, D, 4, 4).permute(1, 2, 0, 3)          # [m][d][kg][i] -> [d][kg][m][i]
    else:
        out = w.reshape(4, 4, D, 16).permute(2, 0, 3, 1)          # [kg][i][d][m] -> [d][kg][m][i]
    return out.reshape(D, 64, 4).float().contiguous()


def conv3d_c16_wino_projfwd(x, upack, bias, he, flags, proj_wA, proj_bias, proj_he, proj_flags):
    """lf_conv3d_c16_wino_projfwd: the last camera block's convolution AND the factor projection behind it in one launch.
    Returns (y, norm, zp (N,16,H,W) channels-last, pnorm)."""
    N, _, D, H, W = x.shape
    y = empty_cl((N, 16, D, H, W), x.device)
    norm = _norm_buf(flags, N * D * H * W, x.device)
    zp = empty_cl((N, 16, H, W), x.device)
    pnorm = _norm_buf(proj_flags, N * H * W, x.device)
    launch('lf_conv3d_c16_wino_projfwd', x, upack, bias, y, norm, N, D, H, W, he, flags, SLOPE, PN_EPS, proj_wA, proj_bias, zp,
           pnorm, proj_he, proj_flags, tag='conv3d_c16_wino_projfwd')
    return y, norm, zp, pnorm


# 'fused' (default): input transform -> lf_wino_fused_gemm (this library's fp32-MFMA GEMM with the output transform and
# the epilogue folded in; the Winograd-domain products never reach memory).  'bmm': the three-stage form with the
# per-frequency products on the library GEMM (torch.bmm -> rocBLAS), kept for A/B measurements (tools/rel_probe.py).
WIDE_CONV_MODE = 'fused'


def _wino_weights(weight, transpose=False):
    """[Cout,Cin,3,3(,3)] -> the Winograd-domain weights U [64 | 16 f][Cout][Cin] = ((G x ..) w)[co][ci][f], evaluated in fp64;
    transpose=True: those of the data gradient (channels swapped, taps flipped)."""
    w = weight.detach()
    if transpose:
        w = w.transpose(0, 1).flip(dims=tuple(range(2, w.dim())))
    assert w.dim() in (4, 5) and tuple(w.shape[2:]) == (3,) * (w.dim() - 2)
    G = torch.tensor(_WINO_G, dtype=torch.float64, device=w.device)
    if w.dim() == 5:
        return torch.einsum('ai,bj,ck,omijk->abcom', G, G, G, w.double()).reshape(64, w.shape[0], w.shape[1])
    return torch.einsum('bj,ck,omjk->bcom', G, G, w.double()).reshape(16, w.shape[0], w.shape[1])


def pack_conv_wino_fused(weight, transpose=False):
    """[Cout,Cin,3,3(,3)] -> U2 [64 | 16 f][CoutP][Cin] (output-channel major, CoutP = lf_wino_fused_cout_padded(Cout),
    zero padded) for lf_wino_fused_gemm: U2[f][co][ci] = ((G x ..) w)[co][ci][f], evaluated in fp64."""
    U = _wino_weights(weight, transpose)
    F, cout, cin = U.shape
    out = torch.zeros(F, _lib.lib().lf_wino_fused_cout_padded(cout), cin, device=U.device, dtype=torch.float32)
    out[:, :cout] = U.float()
    return out.contiguous()


def _wino_conv_fused(x, cout, flags, depth_inner, v_shape, v_dtype, transform, nscr, gemm):
    """The launch sequence of the fused wide convolutions, written once: V, input transform, y (or the depth-inner y), scratch,
    GEMM, PixelNorm as a pass over the (small) output.  transform = (tag, f(V)) and gemm = (tag, f(V, y, scratch pointer or
    None, GEMM flags)); each f returns the (entry point, arguments...) of its launch, which runs under _timed(tag); nscr: the
    GEMM's scratch bytes (its own query).  Returns (y, norm or None)."""
    N, sp = x.shape[0], tuple(x.shape[2:])
    V = torch.empty(v_shape, device=x.device, dtype=v_dtype)
    launch(*transform[1](V), tag=transform[0])
    if depth_inner:
        assert len(sp) == 3
        y = torch.empty((N, sp[1], sp[2], sp[0], cout), device=x.device, dtype=torch.float32)
    else:
        y = empty_cl((N, cout) + sp, x.device)
    scr = torch.empty(nscr // 4, device=x.device, dtype=torch.float32) if nscr else None
    launch(*gemm[1](V, y, scr.data_ptr() if scr is not None else None,
                    (flags & LF_EPI_LRELU) | (_lib.LF_OUT_DEPTH_INNER if depth_inner else 0)), tag=gemm[0])
    del V
    norm = None
    if flags & LF_EPI_PIXELNORM:
        rows = N * math.prod(sp)
        norm = torch.empty(rows, device=x.device, dtype=torch.float32)
        launch('lf_pixelnorm_fwd', y, y, norm, rows, cout, PN_EPS)
    return y, norm


def conv_wino_fused(x, U2, cout, bias, he, flags, depth_inner=False, part_n=None):
    """Wide 2-D / 3-D conv: Winograd input transform, then ONE launch for the per-frequency fp32-MFMA products, the
    output transform, He scale, bias and LeakyReLU (lf_wino_fused_gemm); PixelNorm as a pass over the (small) output.
    depth_inner (3-D only): y comes back as a plain (N, H, W, D, cout) tensor (LF_OUT_DEPTH_INNER): the layout the factor
    projection that follows the last camera block wants.
    part_n: the N rows are N / part_n parts of part_n consecutive rows, and every part's output is bit-identical to this call
    on that part alone (lf_wino_fused_gemm_part: the part's frequency split, one launch for the batch); None: the batch's own
    plan.  Returns (y, norm or None)."""
    L = _lib.lib()
    dims = x.dim() - 2
    N, cin = x.shape[0], x.shape[1]
    D, H, W = (x.shape[2:] if dims == 3 else (1,) + tuple(x.shape[2:]))
    if part_n is not None:
        part_n = _part_rows(part_n)
        if N % part_n:
            raise ValueError(f'part_n = {part_n} does not divide the {N} rows')
    if dims == 3:
        T = L.lf_wino3d_tiles(N, D, H, W)
        transform = ('wino3d_input', lambda V: ('lf_wino3d_input_transform', x, V, N, D, H, W, cin))
    else:
        T = L.lf_wino2d_tiles(N, H, W)
        transform = ('wino2d_input', lambda V: ('lf_wino2d_input_transform', x, V, N, H, W, cin))
    if part_n is None:                                        # the scratch follows the query of the entry point that is called
        name, part = 'lf_wino_fused_gemm', ()
        nscr = L.lf_wino_fused_scratch_bytes(dims, N, D, H, W, cout)
    else:
        name, part = 'lf_wino_fused_gemm_part', (part_n,)
        nscr = L.lf_wino_fused_scratch_bytes_part(dims, N, D, H, W, cout, part_n)

    def gemm(V, y, scr, gflags):
        return (name, V, U2, bias, y, scr, nscr, dims, N, D, H, W, cin, cout, he, gflags, SLOPE) + part
    return _wino_conv_fused(x, cout, flags, depth_inner, (16 if dims == 2 else 64, T, cin), torch.float32, transform, nscr,
                            (f'wino{dims}d_fused', gemm))


def wide_conv(x, weight, bias, he, flags, transpose=False, depth_inner=False, part_n=None):
    """Dispatch of a wide (>= 64-channel) 3x3(x3) convolution or its data gradient (transpose=True) by WIDE_CONV_MODE.
    part_n: see conv_wino_fused ('fused' only)."""
    cout = weight.shape[1] if transpose else weight.shape[0]
    if WIDE_CONV_MODE == 'fused':
        U2 = _pk(weight, 'wfb' if transpose else 'wff', lambda w: pack_conv_wino_fused(w, transpose=transpose))
        return conv_wino_fused(x, U2, cout, bias, he, flags, depth_inner, part_n)
    if part_n is not None:
        raise NotImplementedError("part_n needs WIDE_CONV_MODE = 'fused': the library GEMM of 'bmm' picks its kernel by the batch")
    from . import experimental                     # 'bmm': the three-stage form on the library GEMM (A/B reference)
    U = _pk(weight, 'g3b' if transpose else 'g3f', lambda w: experimental.pack_conv3d_wino_gemm(w, transpose=transpose))
    return experimental.conv3d_wino_gemm(x, U, bias, he, flags)


# Scope of the per-part launch plan (MultiTargetEngine per_target_plan=True): inside `with ops.wide_parts(n):` the fp32 wide 2-D
# and 3-D convolutions of _Conv3x3 treat their batch as parts of n consecutive rows (wide_conv part_n = n), so each part's rows
# are bit-identical to the same convolution on that part alone.  The forward records n on ctx and the data gradient uses it
# whatever scope the backward runs in.  None: the batch's own plan.  Weight gradients are not affected, and neither are the
# split-precision forms (ops.wide2d_f16x3: their scales come from the whole batch).
WIDE_PARTS = None


def _part_rows(n):
    if isinstance(n, bool) or not isinstance(n, int) or n <= 0:
        raise ValueError(f'part rows must be a positive int, got {n!r}')
    return n


class wide_parts:
    def __init__(self, n):
        self.n = None if n is None else _part_rows(n)

    def __enter__(self):
        global WIDE_PARTS
        self.prev = WIDE_PARTS
        WIDE_PARTS = self.n
        return self

    def __exit__(self, *exc):
        global WIDE_PARTS
        WIDE_PARTS = self.prev
        return False


def pack_conv_wino_fused_f16x3(weight, transpose=False):
    """[Cout,Cin,3,3,3] or [Cout,Cin,3,3] -> (U2s, eU) for lf_wino_fused_f16x3_gemm / lf_wino_fused2d_f16x3_gemm:
    U2s [F][CoutP][CinP/32][2][32] f16 (F = 64 frequencies in 3-D, 16 in 2-D), the Winograd weights of pack_conv_wino_fused
    (fp64) times 2^eU, split into hi = f16(u) and lo = f16(u - hi) per 32-channel record (CoutP = lf_wino_fused_cout_padded(Cout),
    CinP = lf_wino_f16x3_cin_padded(Cin), zero padded); eU puts max|U| 2^eU in [2^11, 2^12)."""
    U = _wino_weights(weight, transpose)
    F, cout, cin = U.shape
    amax = U.abs().max().item()
    eU = 12 - math.frexp(amax)[1] if amax > 0 else 0
    coutp, cinp = (cout + 63) // 64 * 64, (cin + 31) // 32 * 32          # lf_wino_fused_cout_padded / lf_wino_f16x3_cin_padded
    Us = torch.zeros(F, coutp, cinp, dtype=torch.float64, device=U.device)
    Us[:, :cout, :cin] = torch.ldexp(U, torch.tensor(float(eU), dtype=torch.float64, device=U.device))
    hi = Us.half()
    lo = (Us - hi.double()).half()
    out = torch.stack((hi.reshape(F, coutp, cinp // 32, 32), lo.reshape(F, coutp, cinp // 32, 32)), dim=3)
    return out.contiguous(), eU


def wide_conv_f16x3(x, weight, bias, he, flags, transpose=False, depth_inner=False, amax_in=None, amax_out=None):
    """Wide 3-D 3x3x3 convolution (or its data gradient, transpose=True) with three-term f16 products
    (lf_wino3d_input_transform_f16x3 + lf_wino_fused_f16x3_gemm); PixelNorm as a pass over the output, as conv_wino_fused.
    A 4-D x: the 2-D 3x3 form (lf_wino2d_input_transform_f16x3 + lf_wino_fused2d_f16x3_gemm), whose input scale is chosen per
    Winograd tile by the transform itself (amax_in / amax_out / depth_inner do not apply).
    amax_in: max-abs buffer (amax_buffer) holding a bound of max|x| -- the input's power-of-two scale is derived from it on the
    device; None: measured here from x.  amax_out (zeroed amax_buffer, optional): receives max|y| before any PixelNorm.
    Returns (y, norm or None); depth_inner: y as a plain (N, H, W, D, cout) tensor (LF_OUT_DEPTH_INNER)."""
    L = _lib.lib()
    if x.dim() == 4:
        assert amax_in is None and amax_out is None and not depth_inner
        return _wide_conv2d_f16x3(x, weight, bias, he, flags, transpose)
    assert x.dim() == 5
    cout = weight.shape[1] if transpose else weight.shape[0]
    U2, eU = _pk(weight, 'wxb' if transpose else 'wxf', lambda w: pack_conv_wino_fused_f16x3(w, transpose=transpose))
    N, cin, D, H, W = x.shape
    if amax_in is None:
        amax_in = amax_buffer(x.detach().abs().amax(), x.device)
    T = L.lf_wino3d_tiles(N, D, H, W)
    nscr = L.lf_wino_fused_f16x3_scratch_bytes(N, D, H, W, cout)
    return _wino_conv_fused(
        x, cout, flags, depth_inner, (64, T, L.lf_wino_f16x3_cin_padded(cin) * 2), torch.float16,
        ('wino3d_input_f16x3', lambda V: ('lf_wino3d_input_transform_f16x3', x, amax_in, V, N, D, H, W, cin)), nscr,
        ('wino3d_fused_f16x3', lambda V, y, scr, gflags: ('lf_wino_fused_f16x3_gemm', V, U2, eU, amax_in, bias, y, amax_out, scr, nscr,
                                                          N, D, H, W, cin, cout, he, gflags, SLOPE)))


def _wide_conv2d_f16x3(x, weight, bias, he, flags, transpose=False):
    L = _lib.lib()
    cout = weight.shape[1] if transpose else weight.shape[0]
    U2, eU = _pk(weight, 'wxb' if transpose else 'wxf', lambda w: pack_conv_wino_fused_f16x3(w, transpose=transpose))
    N, cin, H, W = x.shape
    T = L.lf_wino2d_tiles(N, H, W)
    eV = torch.empty(T, device=x.device, dtype=torch.int32)
    nscr = L.lf_wino_fused2d_f16x3_scratch_bytes(N, H, W, cout)
    return _wino_conv_fused(
        x, cout, flags, False, (16, T, L.lf_wino_f16x3_cin_padded(cin) * 2), torch.float16,
        ('wino2d_input_f16x3', lambda V: ('lf_wino2d_input_transform_f16x3', x, V, eV, N, H, W, cin)), nscr,
        ('wino2d_fused_f16x3', lambda V, y, scr, gflags: ('lf_wino_fused2d_f16x3_gemm', V, eV, U2, eU, bias, y, scr, nscr, N, H, W,
                                                          cin, cout, he, gflags, SLOPE)))


# Scope of the split-precision 2-D decoder (RenderLoopEngine conv_mode='f16x3'): inside `with ops.wide2d_f16x3():` the wide 2-D
# convolutions of _Conv3x3 that WIDE2D_F16X3_ROUTE lists for their shape and batch run on lf_wino_fused2d_f16x3_gemm instead of
# the fp32 pair (lf_wino2d_input_transform + lf_wino_fused_gemm); the forward records the forms it chose, so the backward does
# not depend on the scope.  Autocast and the 3-D dispatch are not affected, and with WIDE_CONV_MODE = 'bmm' (the library-GEMM
# A/B form) nothing is routed: every wide convolution then keeps that form.
WIDE2D_F16X3 = False
# (Cin, Cout, H, W) of a convolution -- a layer's forward, or the data gradient of a layer (Cout, Cin, H, W) -- -> N_min: the
# smallest batch from which on f16x3 measured faster than the fp32 pair at every measured batch (N = 8, 16, 32, 128;
# tools/wide2d_f16x3_ab.py, profiles/r08_wide2d_f16x3_ab.jsonl).  Routed: the released architecture's decoder layers with
# >= 196 channels, 1.15-2.1x at N = 128.  Not routed: the 128 -> 128 / 128 -> 64 / 64 -> 64 layers on 64^2 and 128^2 (0.58-0.96x:
# the f16x3 GEMM is faster, but its input transform is 2.3-2.5x slower than the fp32 one -- one wave per tile leaves 48-56 of 64
# lanes idle at 64-128 channels, and it reads the patch twice) and the released-width model's 64-96-channel layers at N = 4
# (0.70-0.83x: launch-bound).
WIDE2D_F16X3_ROUTE = {
    (128, 196, 64, 64): 8, (196, 128, 64, 64): 8, (196, 196, 32, 32): 8, (196, 256, 32, 32): 8, (256, 196, 32, 32): 8,
    (256, 256, 16, 16): 16, (256, 512, 16, 16): 16, (512, 256, 16, 16): 8, (512, 512, 16, 16): 8, (512, 512, 8, 8): 16,
    (512, 1024, 8, 8): 8, (1024, 512, 8, 8): 16, (512, 512, 4, 4): 128}


class wide2d_f16x3:
    def __init__(self, enabled=True):
        self.enabled = enabled

    def __enter__(self):
        global WIDE2D_F16X3
        self.prev = WIDE2D_F16X3
        WIDE2D_F16X3 = bool(self.enabled)
        return self

    def __exit__(self, *exc):
        global WIDE2D_F16X3
        WIDE2D_F16X3 = self.prev
        return False


def _wide2d_f16x3_routed(cin, cout, H, W, N):
    n_min = WIDE2D_F16X3_ROUTE.get((cin, cout, H, W))
    return n_min is not None and N >= n_min


def _wide_part_n(N):
    """part_n of a wide convolution on N rows under the ops.wide_parts scope (None outside it)."""
    if WIDE_PARTS is None or WIDE_CONV_MODE != 'fused':
        return None
    if N % WIDE_PARTS:
        raise ValueError(f'ops.wide_parts({WIDE_PARTS}) does not divide a batch of {N} rows')
    return WIDE_PARTS


def epilogue_bwd_amax(gy, y, norm, flags, amax_out):
    """_epilogue_bwd (LeakyReLU' / PixelNorm' of a layer) that also publishes max|gp| into amax_out (lf_epilogue_bwd_amax)."""
    rows = gy.numel() // gy.shape[1]
    gp = torch.empty_like(gy, memory_format=torch.preserve_format)
    launch('lf_epilogue_bwd_amax', gy, y, norm, gp, rows, gy.shape[1], flags, SLOPE, amax_out)
    return gp


def _wino_gemm_ok(x, weight):
    """Wide 2-D / 3-D 3x3 convolutions where the transforms amortise over the channels."""
    return (x.dim() == weight.dim() and x.dim() in (4, 5) and weight.shape[0] >= 64 and weight.shape[1] >= 64
            and weight.shape[0] % 4 == 0 and weight.shape[1] % 4 == 0)


def he_constant(weight):
    """sqrt(2 / fan_in)  (modules/equalized.py:66-74)."""
    return math.sqrt(2.0 / weight[0].numel())


# ---------------------------------------------------------------------------------------------
# 3-D resampling
# ---------------------------------------------------------------------------------------------
def _resample_fwd(vol, coef, kind):
    n = coef.shape[0]
    vol_n = 1 if (vol.shape[0] == 1 or vol.stride(0) == 0) else vol.shape[0]
    if vol_n not in (1, n):
        raise ValueError('batch dimension of the volume and the cameras must match')
    v = cl(vol[:1] if vol_n == 1 else vol)
    _, C, D, H, W = v.shape
    out = empty_cl((n, C, D, H, W), v.device)
    cf = torch.zeros(n, LF_MAP_COEFS, device=v.device, dtype=torch.float32)
    cf[:, :coef.shape[1]] = coef
    launch('lf_resample3d_fwd', v, vol_n, cf, kind, out, n, D, H, W, C)
    return out, v, cf, vol_n


class _Resample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vol, coef, kind):
        vol = _f32(vol)
        _req(vol, 'vol'), _req(coef, 'coef')
        out, v, cf, vol_n = _resample_fwd(vol, coef.detach().float(), kind)
        ctx.save_for_backward(v, cf)
        ctx.kind, ctx.vol_n, ctx.vol_shape, ctx.ncoef = kind, vol_n, vol.shape, coef.shape[1]
        return out

    @staticmethod
    def backward(ctx, gout):
        L = _lib.lib()
        v, cf = ctx.saved_tensors
        g = cl(gout)
        n, C, D, H, W = g.shape
        gvol = gcoef = None
        if ctx.needs_input_grad[1]:
            if ctx.kind != LF_MAP_O2C:
                raise NotImplementedError('the reference C2O transform is not differentiable w.r.t. the camera '
                                          '(in-place division, modules/geometry.py:636)')
            gcoef = torch.empty(n, 18, device=g.device, dtype=torch.float32)
            nbytes = L.lf_resample3d_bwd_coef_scratch_bytes(n, D, H, W)
            scratch = torch.empty(max(nbytes, 4) // 4 + 1, device=g.device, dtype=torch.float32)
            launch('lf_resample3d_bwd_coef', g, v, ctx.vol_n, cf, gcoef, scratch.data_ptr(), scratch.numel() * 4, n, D, H, W, C)
        if ctx.needs_input_grad[0]:
            if DETERMINISTIC_SPLAT:
                gv = empty_cl((ctx.vol_n, C, D, H, W), g.device)
                nb = L.lf_resample3d_bwd_vol_det_scratch_bytes(ctx.vol_n, D, H, W, C)
                scr = torch.empty(nb // 8 + 1, device=g.device, dtype=torch.int64)
                launch('lf_resample3d_bwd_vol_det', g, cf, ctx.kind, gv, ctx.vol_n, scr.data_ptr(), scr.numel() * 8, n, D, H, W, C)
            else:
                gv = empty_cl((ctx.vol_n, C, D, H, W), g.device).zero_()
                launch('lf_resample3d_bwd_vol', g, cf, ctx.kind, gv, ctx.vol_n, n, D, H, W, C)
            if gv.shape[0] == ctx.vol_shape[0]:
                gvol = gv
            else:
                # expanded (stride-0) input: autograd sums over the expanded batch itself, so hand
                # back the accumulated volume once and zeros elsewhere
                gvol = torch.zeros(ctx.vol_shape, device=g.device, dtype=torch.float32)
                gvol[0] = gv[0]
        return gvol, gcoef, None


def resample_o2c(vol, coef):
    """ObjectToCameraTransform as an op: vol (1|N,C,S,S,S), coef (N,18) -> (N,C,S,S,S)."""
    if _T()._resample_ac_ok(vol, coef):
        return _T()._ResampleAC.apply(vol, coef, LF_MAP_O2C)
    return _Resample.apply(vol, coef, LF_MAP_O2C)


def resample_c2o(vol, coef):
    """CameraToObjectTransform as an op: vol (N,C,S,S,S), coef (N,16) -> (N,C,S,S,S)."""
    if _T()._resample_ac_ok(vol, coef):
        return _T()._ResampleAC.apply(vol, coef, LF_MAP_C2O)
    return _Resample.apply(vol, coef, LF_MAP_C2O)


def volume_table(indices, vol_n, device):
    """The `vol_idx` argument of the indexed resampler: row i of a batch reads volume indices[i] of vol_n.  The library cannot
    inspect a device table (its kernels clamp), so the range is checked here, on the host, before the table is uploaded."""
    idx = [int(i) for i in indices]
    if vol_n < 1 or not idx:
        raise ValueError(f'a volume table needs at least one row and one volume (got {len(idx)} rows, vol_n = {vol_n})')
    bad = [(r, i) for r, i in enumerate(idx) if not 0 <= i < vol_n]
    if bad:
        raise ValueError(f'volume table row {bad[0][0]} names volume {bad[0][1]}: outside [0, {vol_n})')
    return torch.tensor(idx, dtype=torch.int32).to(device)


def _indexed_args(vols, table, rows):
    _req(vols, 'vols')
    if vols.dim() != 5 or not vols.is_contiguous(memory_format=torch.channels_last_3d):
        raise ValueError('vols: (K,C,D,H,W) volumes in channels-last layout, back to back (ops.cl)')
    if table.dtype != torch.int32 or table.device != vols.device or table.dim() != 1 or not table.is_contiguous():
        raise ValueError('table: a contiguous int32 vector on the device of the volumes (ops.volume_table)')
    if table.numel() != rows:
        raise ValueError(f'the table has {table.numel()} rows, the batch {rows}')


def resample_fwd_indexed(vols, table, coef, kind=LF_MAP_O2C):
    """lf_resample3d_fwd_indexed: vols (K,C,D,H,W) channels-last, table (N,) from volume_table, coef (N,<=20) -> (N,C,D,H,W);
    row i is the resample of vols[table[i]] under coef[i].  Forward only (the pose loop's coefficient gradient is
    resample_bwd_coef_indexed)."""
    n = coef.shape[0]
    _indexed_args(vols, table, n)
    K, C, D, H, W = vols.shape
    out = empty_cl((n, C, D, H, W), vols.device)
    cf = torch.zeros(n, LF_MAP_COEFS, device=vols.device, dtype=torch.float32)
    cf[:, :coef.shape[1]] = coef
    launch('lf_resample3d_fwd_indexed', vols, K, table, cf, kind, out, n, D, H, W, C)
    return out


def resample_bwd_coef_indexed(gout, vols, table, coef, part_n):
    """lf_resample3d_bwd_coef_indexed: d(loss)/d(O2C coefficients) (N,18) of resample_fwd_indexed's rows, every row summed in
    the block partition of a launch of part_n rows (lf_resample3d_bwd_coef_part)."""
    L = _lib.lib()
    g = cl(_req(gout, 'gout'))
    n, C, D, H, W = g.shape
    _indexed_args(vols, table, n)
    if tuple(vols.shape[1:]) != (C, D, H, W):
        raise ValueError(f'gout rows {tuple(g.shape[1:])} and volumes {tuple(vols.shape[1:])} differ in shape')
    if part_n < 1:
        raise ValueError('part_n >= 1')
    cf = torch.zeros(n, LF_MAP_COEFS, device=g.device, dtype=torch.float32)
    cf[:, :coef.shape[1]] = coef
    gcoef = torch.empty(n, 18, device=g.device, dtype=torch.float32)
    nbytes = L.lf_resample3d_bwd_coef_indexed_scratch_bytes(n, part_n, D, H, W)
    scratch = torch.empty(nbytes // 4 + 1, device=g.device, dtype=torch.float32)
    launch('lf_resample3d_bwd_coef_indexed', g, vols, vols.shape[0], table, cf, gcoef, scratch.data_ptr(), scratch.numel() * 4, n,
           D, H, W, C, part_n)
    return gcoef


# ---------------------------------------------------------------------------------------------
# convolutions with fused epilogue
# ---------------------------------------------------------------------------------------------
def _conv3x3_raw(x, wpack, bias, cout, he, flags, want_norm):
    dims = x.dim() - 2
    if dims == 3:
        N, cin, D, H, W = x.shape
    else:
        N, cin, H, W = x.shape
        D = 1
    fuse_pn = bool(flags & LF_EPI_PIXELNORM) and cout <= 64
    kflags = flags if fuse_pn else (flags & ~LF_EPI_PIXELNORM)
    y = empty_cl((N, cout) + tuple(x.shape[2:]), x.device)
    norm = _norm_buf(flags, N * D * H * W, x.device)
    launch('lf_conv3x3_fwd', x, wpack, bias, y, norm if fuse_pn else None, dims, N, D, H, W, cin, cout,
           he, kflags, SLOPE, PN_EPS, tag=f'conv3x3_{dims}d_{cin}x{cout}')
    if (flags & LF_EPI_PIXELNORM) and not fuse_pn:
        launch('lf_pixelnorm_fwd', y, y, norm, N * D * H * W, cout, PN_EPS)
    return y, norm


def conv3x3_bwd_data(gy, wpack_t, cin, he, prev=None):
    """gx = conv^T(gy) * he; prev = (y_prev, norm_prev, flags_prev) folds the producing layer's
    epilogue backward into the store (16-channel records only)."""
    dims = gy.dim() - 2
    N, cout = gy.shape[0], gy.shape[1]
    D, H, W = (gy.shape[2:] if dims == 3 else (1,) + tuple(gy.shape[2:]))
    gx = empty_cl((N, cin) + tuple(gy.shape[2:]), gy.device)
    py, pn, pf = _prev(prev)
    launch('lf_conv3x3_bwd_data', gy, wpack_t, gx, dims, N, D, H, W, cout, cin, he, py, pn, pf, SLOPE,
           tag=f'conv3x3_{dims}d_{cout}x{cin}')
    return gx


def _epilogue_bwd(gy, y, norm, flags):
    if flags == 0:
        return gy
    rows = gy.numel() // gy.shape[1]
    gp = torch.empty_like(gy, memory_format=torch.preserve_format)
    launch('lf_epilogue_bwd', gy, y, norm, gp, rows, gy.shape[1], flags, SLOPE)
    return gp


def _latent_args(zp, zt):
    """(N, P, C, zt as the kernel reads it, its (n, pixel, channel) element strides) of the latent-term entry points: zp a
    channels-last (N,C,h,w) device tensor, zt (N or 1, C, h, w) in any layout whose pixels h*w sit at one stride (NCHW-contiguous
    and channels-last both do: no copy); anything else is made contiguous once."""
    _req(zp, 'zp')
    _req(zt, 'zt')
    if zp.dim() != 4 or zt.dim() != 4 or tuple(zt.shape[1:]) != tuple(zp.shape[1:]) or zt.shape[0] not in (1, zp.shape[0]):
        raise ValueError(f'zp {tuple(zp.shape)} / zt {tuple(zt.shape)}: expected (N,C,h,w) and (N or 1,C,h,w)')
    if not zp.is_contiguous(memory_format=torch.channels_last):
        raise ValueError('zp must be channels-last')
    N, C, h, w = zp.shape
    if not ((h == 1 or zt.stride(2) == w * zt.stride(3)) and min(zt.stride()) >= 0):
        zt = zt.contiguous()
    sp = zt.stride(3) if w > 1 else (zt.stride(2) if h > 1 else 1)
    return N, h * w, C, zt, (zt.stride(0), sp, zt.stride(1))


def latent_cosine_fwd(zp, zt, losses=None, w_latent=0.0):
    """Cosine distance of every row of the projected latent zp (N,C,h,w channels-last) to the target code zt (N or 1,C,h,w)
    (lf_latent_cosine_fwd): -> sums (N,4) = (dot, |zp|^2, |zt|^2, dist).  losses (N,8), when given, receives dist in column 5 and
    w_latent * dist on top of column 4, in place."""
    L = _lib.lib()
    N, P, C, zt, (sn, sp, sc) = _latent_args(zp, zt)
    if losses is not None:
        _req(losses, 'losses')
        if tuple(losses.shape) != (N, 8) or not losses.is_contiguous():
            raise ValueError('losses must be a contiguous (N,8) tensor')
    sums = torch.empty(N, 4, device=zp.device, dtype=torch.float32)
    nbytes = L.lf_latent_cosine_scratch_bytes(N, P, C)
    scratch = torch.empty(nbytes // 4 + 4, device=zp.device, dtype=torch.float32)
    launch('lf_latent_cosine_fwd', zp, zt, zt.shape[0], sn, sp, sc, sums, losses, w_latent, scratch.data_ptr(), scratch.numel() * 4,
           N, P, C, tag='latent_cosine_fwd', detail=f'{N}x{P}x{C}')
    return sums


def latent_cosine_bwd_epi(g_in, zp, norm, zt, sums, gscale, flags, out=None):
    """gp = Epi'(g_in + gscale * d(dist)/d(zp); zp, norm, flags) (lf_latent_cosine_bwd_epi): the latent term's gradient joins the
    decoder's gradient g_in (None: the addend alone) at the projected latent and the projection's LeakyReLU' / PixelNorm' is
    applied in the same pass.  out: None = a new tensor, or g_in itself for the in-place form."""
    N, P, C, zt, (sn, sp, sc) = _latent_args(zp, zt)
    _req(sums, 'sums')
    if tuple(sums.shape) != (N, 4) or not sums.is_contiguous():
        raise ValueError('sums must be the (N,4) output of latent_cosine_fwd')
    for t, name in ((g_in, 'g_in'), (out, 'out')):
        if t is not None:
            _req(t, name)
            if tuple(t.shape) != tuple(zp.shape) or not t.is_contiguous(memory_format=torch.channels_last):
                raise ValueError(f'{name} must be channels-last and shaped like zp')
    if norm is not None:
        _req(norm, 'norm')
        if norm.numel() != N * P or not norm.is_contiguous():
            raise ValueError('norm must hold N*h*w contiguous values')
    gp = out if out is not None else torch.empty_like(zp, memory_format=torch.preserve_format)
    launch('lf_latent_cosine_bwd_epi', g_in, zp, norm, zt, zt.shape[0], sn, sp, sc, sums, gscale, gp, N, P, C, flags, SLOPE,
           tag='latent_cosine_bwd_epi', detail=f'{N}x{P}x{C}')
    return gp


def _points_arg(t, name, last, dims):
    """A float32 device tensor of `dims` dimensions (one of them allowed) whose trailing shape is `last`, else ValueError."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f'{name} must be a device tensor: the HIP path has no CPU fallback')
    if t.dtype != torch.float32:
        raise ValueError(f'{name} must be float32')
    if t.dim() not in dims or tuple(t.shape[-len(last):]) != tuple(last) or t.numel() == 0:
        raise ValueError(f'{name} must be shaped (..., {", ".join(map(str, last))}), got {tuple(t.shape)}')
    return t


def _points_cloud(t, name, B):
    """(n,3) or (1,n,3): one cloud shared by the B batches (batch stride 0); (B,n,3): one per batch -> (tensor, stride)."""
    if t.dim() == 3 and t.shape[0] not in (1, B):
        raise ValueError(f'{name} has {t.shape[0]} batches, expected 1 or {B}')
    t = t.contiguous()
    return t, (t.shape[-2] * 3 if t.dim() == 3 and t.shape[0] == B and B > 1 else 0)


def nn_dist(x1, x2, T1=None, T2=None, want=('dist',)):
    """For every query x1[b][i] the distance to the nearest candidate T2_b x2[b][j] of T1_b x1[b][i] (lf_nn_dist): direct
    coordinate differences in fp32, the smallest index on ties.  x1 (M,3) or (B,M,3), x2 (Q,3) or (B,Q,3); a 2-D (or
    one-batch) cloud is shared by all batches.  T1 / T2: None or (B,3,4) affine maps.  want: any of 'dist' (B,M), 'idx' (B,M) int32
    and 'mean' (B,); -> a dict of them (without the batch dimension when no argument has one)."""
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or any(w not in ('dist', 'idx', 'mean') for w in want):
        raise ValueError("want must name some of 'dist', 'idx', 'mean'")
    _points_arg(x1, 'x1', (3,), (2, 3))
    _points_arg(x2, 'x2', (3,), (2, 3))
    for t, name in ((T1, 'T1'), (T2, 'T2')):
        if t is not None:
            _points_arg(t, name, (3, 4), (3,))
    tensors = [t for t in (x1, x2, T1, T2) if t is not None]
    if any(t.device != x1.device for t in tensors):
        raise ValueError('x1, x2, T1 and T2 must be on one device')
    batches = {t.shape[0] for t in tensors if t.dim() == 3 and t.shape[0] != 1}
    if len(batches) > 1:
        raise ValueError(f'batch sizes differ: {sorted(batches)}')
    batched = any(t.dim() == 3 for t in tensors)
    B = batches.pop() if batches else 1
    for t, name in ((T1, 'T1'), (T2, 'T2')):
        if t is not None and t.shape[0] != B:
            raise ValueError(f'{name} must hold one map per batch ({B})')
    x1, s1 = _points_cloud(x1, 'x1', B)
    x2, s2 = _points_cloud(x2, 'x2', B)
    M, Q = x1.shape[-2], x2.shape[-2]
    L = _lib.lib()
    T1 = T1.contiguous() if T1 is not None else None
    T2 = T2.contiguous() if T2 is not None else None
    dev = x1.device
    dist = torch.empty(B, M, device=dev, dtype=torch.float32) if 'dist' in want else None
    idx = torch.empty(B, M, device=dev, dtype=torch.int32) if 'idx' in want else None
    mean = torch.empty(B, device=dev, dtype=torch.float32) if 'mean' in want else None
    nbytes = L.lf_nn_dist_scratch_bytes(B, M, Q)
    scratch = torch.empty(nbytes // 4 + 4, device=dev, dtype=torch.float32)
    launch('lf_nn_dist', x1, s1, T1, x2, s2, T2, dist, idx, mean, scratch.data_ptr(), scratch.numel() * 4, B, M, Q, tag='nn_dist',
           detail=f'{B}x{M}x{Q}')
    out = {'dist': dist, 'idx': idx, 'mean': mean}
    return {k: (out[k] if batched else out[k][0]) for k in want}


def points_pair_dist(points, A, B):
    """Mean distance of the model points under two projective maps per row (lf_points_pair_dist): points (P,3) shared by all rows
    or (R,P,3); A, B (R,4,4) -> 3-D points after the division by the fourth component (ADD with obj_to_cam), or (R,3,4) -> 2-D
    points after the division by the third (proj2d with obj_to_image).  -> (R,) means."""
    _points_arg(points, 'points', (3,), (2, 3))
    if not isinstance(A, torch.Tensor) or A.dim() != 3 or tuple(A.shape[1:]) not in ((4, 4), (3, 4)):
        raise ValueError('A must be shaped (R,4,4) or (R,3,4)')
    _points_arg(A, 'A', tuple(A.shape[1:]), (3,))
    _points_arg(B, 'B', tuple(A.shape[1:]), (3,))
    if B.shape[0] != A.shape[0]:
        raise ValueError(f'A and B hold {A.shape[0]} and {B.shape[0]} rows')
    if points.device != A.device or points.device != B.device:
        raise ValueError('points, A and B must be on one device')
    R, rows = A.shape[0], A.shape[1]
    points, sr = _points_cloud(points, 'points', R)
    P = points.shape[-2]
    L = _lib.lib()
    A, B = A.contiguous(), B.contiguous()
    mean = torch.empty(R, device=points.device, dtype=torch.float32)
    nbytes = L.lf_points_pair_dist_scratch_bytes(R, P)
    scratch = torch.empty(nbytes // 4 + 4, device=points.device, dtype=torch.float32)
    launch('lf_points_pair_dist', points, sr, A, B, rows, mean, scratch.data_ptr(), scratch.numel() * 4, R, P,
           tag='points_pair_dist', detail=f'{R}x{P}x{rows}')
    return mean


def _frames_arg(t, name, dtypes):
    """(B,1,H,W) or (B,H,W) device tensor of one of `dtypes` -> its (B,H,W) view, else ValueError."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f'{name} must be a device tensor: the HIP path has no CPU fallback')
    if t.dtype not in dtypes:
        raise ValueError(f'{name} must be one of {", ".join(str(d) for d in dtypes)}, got {t.dtype}')
    if t.dim() not in (3, 4) or (t.dim() == 4 and t.shape[1] != 1) or t.numel() == 0:
        raise ValueError(f'{name} must be shaped (B,1,H,W) or (B,H,W), got {tuple(t.shape)}')
    return t[:, 0] if t.dim() == 4 else t


def _aligned4(t):
    """`t` contiguous and on a 4-byte boundary (a byte mask sliced at an odd offset is copied)."""
    t = t.contiguous()
    return t if t.device.type != 'cuda' or t.data_ptr() % 4 == 0 else t.clone()


def depth_init(depth, mask, intrinsic=None, m=3.0, erode_radius=0):
    """The estimators' initial translation for B frames in one call (lf_depth_init; pose/initialization.py): the centre of the
    mask's bounding box and the mid-range of the MAD-filtered masked depth, bit for bit what _masks_to_viewports,
    _reject_outliers_mad(m) and estimate_translation compute per frame on the host.  depth, mask: (B,1,H,W) or (B,H,W); depth
    float32, mask float32, bool or uint8 (foreground iff != 0); intrinsic: None or (B or 1, 3, >= 3) float32.  erode_radius = r > 0
    restricts the depths to the mask eroded by a disk of radius r (the frame's outside counts as foreground); the bounding box
    stays the un-eroded mask's.  -> {'trans': (B,3), only with intrinsic; 'stats': (B,8) = (z, median, mad, min_kept, max_kept,
    cu, cv, 0); 'counts': (B,8) int32 = (n_mask, n_valid, n_kept, xmin, ymin, xmax, ymax, 0)}.  Degenerate frames are reported
    (n_mask / n_valid / n_kept = 0 with NaN in their stats and trans rows), not raised: nothing here synchronises."""
    d3 = _frames_arg(depth, 'depth', (torch.float32,))
    k3 = _frames_arg(mask, 'mask', (torch.float32, torch.bool, torch.uint8))
    if tuple(d3.shape) != tuple(k3.shape):
        raise ValueError(f'depth and mask differ in shape: {tuple(depth.shape)} and {tuple(mask.shape)}')
    if k3.device != d3.device:
        raise ValueError('depth and mask must be on one device')
    B, H, W = d3.shape
    if B * H * W >= 2 ** 31:
        raise ValueError(f'{B} x {H} x {W} pixels: at most 2^31 - 1 per call')
    if isinstance(m, bool) or not isinstance(m, (int, float)) or not m > 0:
        raise ValueError(f'm must be a positive number, got {m!r}')
    if isinstance(erode_radius, bool) or not isinstance(erode_radius, int) or not 0 <= erode_radius <= 8:
        raise ValueError(f'erode_radius must be an integer in 0..8, got {erode_radius!r}')
    if intrinsic is not None:
        if not isinstance(intrinsic, torch.Tensor) or not intrinsic.is_cuda or intrinsic.device != d3.device:
            raise ValueError('intrinsic must be a device tensor on the device of depth')
        if intrinsic.dtype != torch.float32:
            raise ValueError('intrinsic must be float32')
        if intrinsic.dim() != 3 or intrinsic.shape[0] not in (1, B) or intrinsic.shape[1] != 3 or intrinsic.shape[2] < 3:
            raise ValueError(f'intrinsic must be shaped ({B} or 1, 3, >= 3), got {tuple(intrinsic.shape)}')
    L = _lib.lib()
    dev = d3.device
    d3 = _aligned4(d3)
    u8 = k3.dtype != torch.float32
    k3 = _aligned4(k3.view(torch.uint8) if k3.dtype == torch.bool else k3)
    intr = trans = None
    if intrinsic is not None:
        intr = torch.stack((intrinsic[:, 0, 0], intrinsic[:, 1, 1], intrinsic[:, 0, 2], intrinsic[:, 1, 2]), dim=-1).contiguous()
        trans = torch.empty(B, 3, device=dev, dtype=torch.float32)
    stats = torch.empty(B, 8, device=dev, dtype=torch.float32)
    counts = torch.empty(B, 8, device=dev, dtype=torch.int32)
    nbytes = L.lf_depth_init_scratch_bytes(B, H, W)
    scratch = torch.empty(nbytes // 4 + 4, device=dev, dtype=torch.float32)
    launch('lf_depth_init', d3, k3, int(u8), intr, intr.shape[0] if intr is not None else 1, float(m), erode_radius, trans, stats,
           counts, scratch.data_ptr(), scratch.numel() * 4, B, H, W, tag='depth_init', detail=f'{B}x{H}x{W}')
    out = {'stats': stats, 'counts': counts}
    if trans is not None:
        out['trans'] = trans
    return out


def pack_depth_cameras(camera):
    """Host packing of the camera records of `depth_points` (layout: include/lf_hip.h), one per view: viewport origin and
    extent, fu, fv, u0, v0, the 3x4 cam_to_obj and the 3x4 obj_to_image.  Everything is formed in fp64 from the Camera's state,
    view by view (a record does not depend on its batch mates), and rounded once to fp32, as pack_ibr_cameras does.  A camera on
    the device is read back for this (four small tensors); pack once and pass the records where that copy matters.
    -> (B, LF_DEPTH_CAM_FLOATS) float32 on the camera's device."""
    c = camera._map(lambda t: t.detach().to('cpu', torch.float64))
    n = len(c)
    rot, t = c.rotation_matrix[:, :3, :3], c.translation
    ext = torch.zeros(n, 4, 4, dtype=torch.float64)
    ext[:, :3, :3], ext[:, :3, 3], ext[:, 3, 3] = rot, t, 1.0                                   # obj_to_cam
    rec = torch.zeros(n, _lib.LF_DEPTH_CAM_FLOATS, dtype=torch.float64)
    rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3] = c.viewport[:, 0], c.viewport[:, 1], c.viewport_width, c.viewport_height
    rec[:, 4], rec[:, 5], rec[:, 6], rec[:, 7] = c.fu, c.fv, c.u0, c.v0
    inv = torch.cat((rot.transpose(1, 2), -sum(rot[:, k, :] * t[:, k, None] for k in range(3))[:, :, None]), dim=2)
    rec[:, 8:20] = inv.reshape(n, 12)                                                           # cam_to_obj
    rec[:, 20:32] = _mm4(c.intrinsic, ext).reshape(n, 12)                                       # obj_to_image
    return rec.to(torch.float32).to(camera.device)


DEPTH_FRAMES = ('object', 'camera')


def depth_points(depth, mask, camera, color=None, frame='object', segment=True, want_index=False):
    """Back-projection of B depth maps to points, segmentation by re-projection into the mask and ordered compaction in one
    call (lf_depth_points; Observation.pointcloud).  depth (B,1,H,W) or (B,H,W) float32; mask the same shape, float32, bool or
    uint8 (foreground iff != 0), None allowed without segment; camera: a Camera of B views or the records of
    pack_depth_cameras; color: None or (B,3,H,W) float32; frame: 'object' | 'camera' (the points' frame; the segmentation
    re-projects them with obj_to_image either way, as the reference does).  A pixel of depth exactly 0 is never kept under
    segment (the one departure from the reference, where its re-projection is rounding noise).
    -> {'points': (B*H*W, 3), 'counts': (B,) int32, 'colors': (B*H*W, 3) with color, 'index': (B*H*W,) int32 with want_index}:
    the kept points packed from row 0 in view-major, row-major order, sum(counts) rows valid, the rest unwritten.  Nothing here
    synchronises; the caller reads counts when it needs the total."""
    from .modules.geometry import Camera
    if frame not in DEPTH_FRAMES:
        raise ValueError(f'frame must be one of {DEPTH_FRAMES}, got {frame!r}')
    if not isinstance(segment, bool) or not isinstance(want_index, bool):
        raise ValueError('segment and want_index must be bool')
    d3 = _frames_arg(depth, 'depth', (torch.float32,))
    B, H, W = d3.shape
    k3 = None
    if mask is not None:
        k3 = _frames_arg(mask, 'mask', (torch.float32, torch.bool, torch.uint8))
        if tuple(k3.shape) != tuple(d3.shape):
            raise ValueError(f'depth and mask differ in shape: {tuple(depth.shape)} and {tuple(mask.shape)}')
        if k3.device != d3.device:
            raise ValueError('depth and mask must be on one device')
    elif segment:
        raise ValueError('segment=True needs a mask')
    if B * H * W >= 2 ** 31:
        raise ValueError(f'{B} x {H} x {W} pixels: at most 2^31 - 1 per call')
    if color is not None:
        if not isinstance(color, torch.Tensor) or not color.is_cuda or color.device != d3.device:
            raise ValueError('color must be a device tensor on the device of depth')
        if color.dtype != torch.float32 or tuple(color.shape) != (B, 3, H, W):
            raise ValueError(f'color must be float32 and shaped ({B}, 3, {H}, {W}), got {color.dtype} {tuple(color.shape)}')
    if isinstance(camera, Camera):
        if len(camera) != B:
            raise ValueError(f'camera holds {len(camera)} views, depth {B}')
        frame_w, frame_h = int(camera.width), int(camera.height)
        if segment and (frame_h, frame_w) != (H, W):
            raise ValueError(f'segment=True indexes the {H} x {W} mask with pixels of the {frame_h} x {frame_w} frame: the two '
                             f'must be equal')
        cams = pack_depth_cameras(camera).to(d3.device)
    else:
        cams = _points_arg(camera, 'camera', (B, _lib.LF_DEPTH_CAM_FLOATS), (2,))
        if cams.device != d3.device:
            raise ValueError('the camera records must be on the device of depth')
        frame_w, frame_h = W, H
    L = _lib.lib()
    dev = d3.device
    d3 = _aligned4(d3)
    u8 = k3 is not None and k3.dtype != torch.float32
    if k3 is not None:
        k3 = _aligned4(k3.view(torch.uint8) if k3.dtype == torch.bool else k3)
    cap = B * H * W
    points = torch.empty(cap, 3, device=dev, dtype=torch.float32)
    colors = torch.empty(cap, 3, device=dev, dtype=torch.float32) if color is not None else None
    index = torch.empty(cap, device=dev, dtype=torch.int32) if want_index else None
    counts = torch.empty(B, device=dev, dtype=torch.int32)
    nbytes = L.lf_depth_points_scratch_bytes(B, H, W)
    scratch = torch.empty(nbytes // 4 + 4, device=dev, dtype=torch.int32)
    launch('lf_depth_points', d3, k3, int(u8), color.contiguous() if color is not None else None, cams.contiguous(), points, colors,
           index, counts, scratch.data_ptr(), scratch.numel() * 4, B, H, W, frame_w, frame_h, int(frame == 'object'), int(segment),
           tag='depth_points', detail=f'{B}x{H}x{W}')
    out = {'points': points, 'counts': counts}
    if colors is not None:
        out['colors'] = colors
    if index is not None:
        out['index'] = index
    return out


FPS_FORMS = {'auto': 0, 'resident': 1, 'streamed': 2}


def farthest_points(points, k, want=('centers',), form='auto'):
    """Greedy farthest-point sampling of one cloud (N,3) or B clouds (B,N,3), device float32 (lf_farthest_points): pick 0 is
    row 0, pick j the smallest index among the rows farthest from picks 0..j-1, distances from direct coordinate differences in
    fp32 (not F.pairwise_distance's, which adds 1e-6 to every difference: the picks agree except at near-ties).  want: any of
    'centers' (B,k) int32, 'owner' (B,N) int32 -- the LAST pick that attains a row's minimum distance -- and 'nearest' (B,N),
    that distance; -> a dict of them (without the batch dimension for an (N,3) cloud).  form: 'auto' (by N alone) | 'resident'
    (one workgroup per cloud, one launch; N <= LF_FPS_RESIDENT_MAX) | 'streamed' (one launch per pick): the same bits."""
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or any(w not in ('centers', 'owner', 'nearest') for w in want):
        raise ValueError("want must name some of 'centers', 'owner', 'nearest'")
    if form not in FPS_FORMS:
        raise ValueError(f'form must be one of {tuple(FPS_FORMS)}, got {form!r}')
    _points_arg(points, 'points', (3,), (2, 3))
    batched = points.dim() == 3
    B, N = (points.shape[0], points.shape[1]) if batched else (1, points.shape[0])
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= N:
        raise ValueError(f'k must be an integer in 1..{N}, got {k!r}')
    if form == 'resident' and N > _lib.LF_FPS_RESIDENT_MAX:
        raise ValueError(f"form='resident' takes at most {_lib.LF_FPS_RESIDENT_MAX} points per cloud, got {N}")
    if B * N >= 2 ** 31:
        raise ValueError(f'{B} x {N} points: at most 2^31 - 1 per call')
    if batched and B > 1 and points.stride(0) == 0:               # an expanded cloud stays one cloud (batch stride 0)
        x, stride = points[0].contiguous(), 0
    else:
        x, stride = points.contiguous(), N * 3
    L = _lib.lib()
    dev = x.device
    centers = torch.empty(B, k, device=dev, dtype=torch.int32) if 'centers' in want else None
    owner = torch.empty(B, N, device=dev, dtype=torch.int32) if 'owner' in want else None
    nearest = torch.empty(B, N, device=dev, dtype=torch.float32) if 'nearest' in want else None
    nbytes = L.lf_farthest_points_scratch_bytes(B, N, k, FPS_FORMS[form])
    scratch = torch.empty(nbytes // 4 + 4, device=dev, dtype=torch.float32)
    launch('lf_farthest_points', x, stride, centers, owner, nearest, scratch.data_ptr(), scratch.numel() * 4, B, N, k,
           FPS_FORMS[form], tag='farthest_points', detail=f'{B}x{N}x{k}')
    out = {'centers': centers, 'owner': owner, 'nearest': nearest}
    return {w: (out[w] if batched else out[w][0]) for w in want}


OBS_STACKS = (None, 'color_mask', 'color_depth_mask')


def observation_prepare(color, depth, mask, boxes, target_size, zn=None, zf=None, prepare=False, normalize=False, stack=None):
    """Observation.zoom -> prepare -> normalize for B frames in one launch (lf_obs_prepare; observation.py, include/lf_hip.h for
    the arithmetic op by op).  color: (B,C,H,W) float32 or None (no colour planes); depth, mask: (B,1,H,W) or (B,H,W), depth
    float32, mask float32, bool or uint8 (a byte counts as its value); boxes: (B,4) float32 = (x0, y0, x1, y1) in frame pixels,
    the un-truncated viewport of Camera.zoom_viewport, ON THE DEVICE; target_size = T.  The crop always runs (colour bilinear,
    depth and mask nearest, zeros padding); prepare / normalize add the chains of Observation.prepare / normalize, the latter
    needs zn, zf: (B,) float32 = the camera's znear - 0.01 and zfar + 0.01.  stack: None, 'color_mask' or 'color_depth_mask'
    also writes the encoder input [colour | depth | mask * 2 - 1] (Sculptor.encode's concatenation).
    -> {'color': (B,C,T,T) or None, 'depth': (B,1,T,T), 'mask': (B,1,T,T), 'stack': (B,planes,T,T) when asked}.
    Every argument is checked before the library is touched, and nothing here synchronises."""
    d3 = _frames_arg(depth, 'depth', (torch.float32,))
    k3 = _frames_arg(mask, 'mask', (torch.float32, torch.bool, torch.uint8))
    if tuple(d3.shape) != tuple(k3.shape):
        raise ValueError(f'depth and mask differ in shape: {tuple(depth.shape)} and {tuple(mask.shape)}')
    dev = d3.device
    if k3.device != dev:
        raise ValueError('depth and mask must be on one device')
    B, H, W = d3.shape
    C = 0
    if color is not None:
        if not isinstance(color, torch.Tensor) or not color.is_cuda or color.device != dev:
            raise ValueError('color must be a device tensor on the device of depth (or None): the HIP path has no CPU fallback')
        if color.dtype != torch.float32:
            raise ValueError(f'color must be float32, got {color.dtype}')
        if color.dim() != 4 or color.shape[0] != B or tuple(color.shape[2:]) != (H, W):
            raise ValueError(f'color must be shaped ({B}, C, {H}, {W}), got {tuple(color.shape)}')
        C = color.shape[1]
    if isinstance(target_size, bool) or not isinstance(target_size, int) or target_size < 1:
        raise ValueError(f'target_size must be a positive integer, got {target_size!r}')
    T = target_size
    if B * max(C, 1) * H * W >= 2 ** 31 or B * (C + 2) * T * T >= 2 ** 31:
        raise ValueError(f'{B} frames of {max(C, 1)} x {H} x {W} -> {C + 2} x {T} x {T}: at most 2^31 - 1 values per call')
    if not isinstance(boxes, torch.Tensor) or not boxes.is_cuda or boxes.device != dev:
        raise ValueError('boxes must be a device tensor on the device of depth')
    if boxes.dtype != torch.float32 or tuple(boxes.shape) != (B, 4):
        raise ValueError(f'boxes must be float32 shaped ({B}, 4), got {boxes.dtype} {tuple(boxes.shape)}')
    for name, flag in (('prepare', prepare), ('normalize', normalize)):
        if not isinstance(flag, bool):
            raise ValueError(f'{name} must be a bool, got {flag!r}')
    for name, z in (('zn', zn), ('zf', zf)):
        if z is None:
            if normalize:
                raise ValueError(f'normalize needs {name}')
            continue
        if not isinstance(z, torch.Tensor) or not z.is_cuda or z.device != dev:
            raise ValueError(f'{name} must be a device tensor on the device of depth')
        if z.dtype != torch.float32 or tuple(z.shape) != (B,):
            raise ValueError(f'{name} must be float32 shaped ({B},), got {z.dtype} {tuple(z.shape)}')
    if isinstance(stack, (list, dict, set)) or stack not in OBS_STACKS:
        raise ValueError(f'stack {stack!r}: one of {OBS_STACKS}')
    d3 = _aligned4(d3)
    u8 = k3.dtype != torch.float32
    k3 = _aligned4(k3.view(torch.uint8) if k3.dtype == torch.bool else k3)
    color = _aligned4(color) if C > 0 else None
    boxes = _aligned4(boxes)
    zn, zf = (_aligned4(zn), _aligned4(zf)) if normalize else (None, None)
    color_out = torch.empty(B, C, T, T, device=dev, dtype=torch.float32) if C > 0 else None
    depth_out = torch.empty(B, 1, T, T, device=dev, dtype=torch.float32)
    mask_out = torch.empty(B, 1, T, T, device=dev, dtype=torch.float32)
    with_depth = stack == 'color_depth_mask'
    planes = C + 1 + int(with_depth)
    stacked = torch.empty(B, planes, T, T, device=dev, dtype=torch.float32) if stack is not None else None
    stages = (_lib.LF_OBS_PREPARE if prepare else 0) | (_lib.LF_OBS_NORMALIZE if normalize else 0)
    launch('lf_obs_prepare', color, d3, k3, int(u8), boxes, zn, zf, color_out, depth_out, mask_out, stacked, planes * T * T,
           int(with_depth), B, C, H, W, T, stages, tag='obs_prepare', detail=f'{B}x{C}x{H}x{W}->{T}')
    out = {'color': color_out, 'depth': depth_out, 'mask': mask_out}
    if stacked is not None:
        out['stack'] = stacked
    return out


RECON_BASES = ('l1', 'smooth_l1')


def _recon_args(x, y, base, k, mask_logits, mask_target, beta_param):
    """The argument rules of recon_losses / recon_losses_fwd; raises ValueError, touches neither the library nor the device."""
    if x is None and mask_logits is None:
        raise ValueError('recon_losses needs x / y, mask_logits / mask_target or both')
    dev = None
    if x is not None:
        for name, t in (('x', x), ('y', y)):
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise ValueError(f'{name} must be a device tensor: the HIP path has no CPU fallback (use the composed path)')
            if not t.is_floating_point():
                raise ValueError(f'{name} must be a floating-point tensor, got {t.dtype}')
        if x.dim() != 4 or tuple(x.shape) != tuple(y.shape) or x.numel() == 0:
            raise ValueError(f'x and y must be shaped (B,C,H,W) alike, got {tuple(x.shape)} and {tuple(y.shape)}')
        if y.device != x.device:
            raise ValueError('x and y must be on one device')
        dev = x.device
        B, C, H, W = x.shape
        if not 1 <= C <= 4:
            raise ValueError(f'{C} channels: 1 to 4')
        if H * W >= 2 ** 31 - 1 or B * H * W >= 2 ** 31 * 256:
            raise ValueError(f'{B} images of {H} x {W} pixels are too many for one call')
        if isinstance(base, (list, dict, set)) or base not in RECON_BASES:
            raise ValueError(f'base {base!r}: one of {RECON_BASES}')
        if isinstance(k, bool) or not isinstance(k, int) or not 0 <= k <= H * W:
            raise ValueError(f'k must be an integer in 0..{H * W} (0 = no mining), got {k!r}')
    elif y is not None:
        raise ValueError('y without x')
    if mask_logits is not None:
        for name, t in (('mask_logits', mask_logits), ('mask_target', mask_target)):
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise ValueError(f'{name} must be a device tensor: the HIP path has no CPU fallback (use the composed path)')
            if not t.is_floating_point():
                raise ValueError(f'{name} must be a floating-point tensor, got {t.dtype}')
        if tuple(mask_logits.shape) != tuple(mask_target.shape) or mask_logits.numel() == 0:
            raise ValueError(f'mask_logits and mask_target differ in shape or are empty: {tuple(mask_logits.shape)} and '
                             f'{tuple(mask_target.shape)}')
        if mask_target.device != mask_logits.device or (dev is not None and mask_logits.device != dev):
            raise ValueError('all tensors must be on one device')
        if mask_logits.numel() > 2 ** 40:
            raise ValueError('mask_logits is too large for one call')
        if isinstance(beta_param, bool) or not isinstance(beta_param, (int, float)) or not beta_param > 0:
            raise ValueError(f'beta_param must be a positive number, got {beta_param!r}')
    elif mask_target is not None:
        raise ValueError('mask_target without mask_logits')


def _recon_beta(beta_param):
    """(alpha, beta, log_beta) as the library takes them; the prior of the training step is symmetric."""
    if beta_param is None:
        return 1.0, 1.0, 0.0
    from . import losses
    return float(beta_param), float(beta_param), float(losses._log_beta(float(beta_param), float(beta_param)))


def recon_losses_fwd(x, y, base, k, mask_logits=None, mask_target=None, beta_param=None):
    """lf_recon_loss_fwd on prepared tensors (fp32, contiguous): -> {'terms': (4,) = (recon, mask_recon, mask_beta, 0), and with
    x: 'thresh': (B,), 'sel': (B,2) int32 = (n_gt, n_tie), 'img_sum': (B,)}.  Three launches, nothing synchronises."""
    _recon_args(x, y, base, k, mask_logits, mask_target, beta_param)
    L = _lib.lib()
    dev = x.device if x is not None else mask_logits.device
    B, C, H, W = x.shape if x is not None else (0, 0, 0, 0)
    Mn = mask_logits.numel() if mask_logits is not None else 0
    a, b, lb = _recon_beta(beta_param if mask_logits is not None else None)
    out = {'terms': torch.empty(4, device=dev, dtype=torch.float32)}
    if x is not None:
        out['thresh'] = torch.empty(B, device=dev, dtype=torch.float32)
        out['sel'] = torch.empty(B, 2, device=dev, dtype=torch.int32)
        out['img_sum'] = torch.empty(B, device=dev, dtype=torch.float32)
    nbytes = L.lf_recon_loss_scratch_bytes(B, C, H, W, Mn)
    scratch = torch.empty(nbytes // 8 + 1, device=dev, dtype=torch.float64)
    launch('lf_recon_loss_fwd', x, y, RECON_BASES.index(base) if x is not None else 0, k if x is not None else 0, mask_logits,
           mask_target, a, b, lb, out.get('thresh'), out.get('sel'), out.get('img_sum'), out['terms'], scratch.data_ptr(),
           scratch.numel() * 8, B, C, H, W, Mn, tag='recon_loss_fwd', detail=f'{B}x{C}x{H}x{W} k={k} Mn={Mn}')
    return out


def recon_losses_bwd(g_terms, x, y, base, k, thresh, sel, mask_logits=None, mask_target=None, beta_param=None):
    """lf_recon_loss_bwd: g_terms (>= 3,) fp32 ON THE DEVICE -> (gx or None, gmlogit or None).  One launch."""
    B, C, H, W = x.shape if x is not None else (0, 0, 0, 0)
    Mn = mask_logits.numel() if mask_logits is not None else 0
    a, b, lb = _recon_beta(beta_param if mask_logits is not None else None)
    gx = torch.empty_like(x) if x is not None else None
    gz = torch.empty_like(mask_logits) if mask_logits is not None else None
    launch('lf_recon_loss_bwd', g_terms, x, y, RECON_BASES.index(base) if x is not None else 0, k if x is not None else 0, thresh,
           sel, mask_logits, mask_target, a, b, lb, gx, gz, B, C, H, W, Mn, tag='recon_loss_bwd',
           detail=f'{B}x{C}x{H}x{W} k={k} Mn={Mn}')
    return gx, gz


class _ReconLosses(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, z, t, base, k, beta_param):
        out = recon_losses_fwd(x, y, base, k, z, t, beta_param)
        ctx.save_for_backward(x, y, z, t, out.get('thresh'), out.get('sel'))
        ctx.cfg = (base, k, beta_param)
        return out['terms']

    @staticmethod
    def backward(ctx, g):
        x, y, z, t, thresh, sel = ctx.saved_tensors
        base, k, beta_param = ctx.cfg
        gx, gz = recon_losses_bwd(g.float().contiguous(), x, y, base, k, thresh, sel, z, t, beta_param)
        return (gx if ctx.needs_input_grad[0] else None, None, gz if ctx.needs_input_grad[2] else None, None, None, None, None)


def recon_losses(x, y, base, k, mask_logits=None, mask_target=None, beta_param=None):
    """The loss tail of the generator's training step in one call (lf_recon_loss_fwd / _bwd; losses.py HardPixelLoss,
    beta_prior_loss, recon/training.py): -> terms (3,) on the device = (recon, mask_recon, mask_beta), differentiable w.r.t. x
    and mask_logits (y and mask_target are constants).  x, y: (B,C,H,W), C <= 4, or both None (mask terms alone); base: 'l1' or
    'smooth_l1' (beta 1); k = 0: the mean over all elements, 1 <= k <= H*W: the mean of every image's k largest per-pixel
    losses (mean over channels); of the pixels equal to an image's k-th largest loss those of lowest index carry the
    gradient.  mask_logits, mask_target: any shape alike, or both None; beta_param: the symmetric Beta prior's parameter, needed
    with the mask part.  The term of an absent part is 0.  Every argument is checked before the library is touched."""
    _recon_args(x, y, base, k, mask_logits, mask_target, beta_param)
    if x is not None:
        x, y = x.float().contiguous(), y.detach().float().contiguous()
    if mask_logits is not None:
        mask_logits, mask_target = mask_logits.float().contiguous(), mask_target.detach().float().contiguous()
    return _ReconLosses.apply(x, y, mask_logits, mask_target, base, k, beta_param)[:3]


def _wino_ok(x, weight):
    """The Winograd kernel serves 3-D 16 -> 16 convolutions on volumes of at least one 2x8x16 tile row."""
    return (x.dim() == 5 and tuple(weight.shape[:2]) == (16, 16) and x.shape[1] == 16
            and (x.shape[2] * x.shape[3] * x.shape[4]) * 64 < 2 ** 31)


class _Conv3x3(torch.autograd.Function):
    """x -> epilogue(conv3x3(x, W) * he + b).  The input is kept for the weight gradient only when the
    weight or bias asks for one (the pose loop never does)."""

    @staticmethod
    def forward(ctx, x, weight, bias, flags):
        _req(x, 'x'), _req(weight, 'weight')
        x = cl(x)
        he = he_constant(weight)
        b = bias.detach() if bias is not None else None
        ctx.ac = AUTOCAST is not None
        split2d = WIDE2D_F16X3 and not ctx.ac and WIDE_CONV_MODE == 'fused'
        ctx.f16x3 = (False, False)                            # (forward, data gradient) on the split-precision 2-D kernel
        ctx.part_n = None
        if ctx.ac and _wino_ok(x, weight):                    # autocast, 3-D 16 -> 16: direct conv on the bf16 MFMA
            y, norm = conv3d_c16_ring_bf16(x, _pk(weight, 'r3f', pack_conv3d_c16_ring_bf16), b, he, flags, 1)
            # (the input is saved un-rounded: the bf16 weight-gradient kernel rounds it while staging, like this one)
            if (weight.requires_grad or (bias is not None and bias.requires_grad)) and not _T()._wgrad_bf16_ok(x, 3, 16, 16):
                x = round_bf16(x)
        else:
            x = _ac_in(x)
            if _wino_ok(x, weight):                           # 3-D 16 -> 16: the all-fp32 Winograd kernel
                y, norm = conv3d_c16_wino(x, _pk(weight, 'w3f', pack_conv3d_c16_wino), b, he, flags)
            elif _wino_gemm_ok(x, weight):                    # wide 2-D / 3-D: Winograd with the fused fp32-MFMA GEMM
                if x.dim() == 4 and split2d:
                    N, cin, H, W = x.shape
                    ctx.f16x3 = (_wide2d_f16x3_routed(cin, weight.shape[0], H, W, N), _wide2d_f16x3_routed(weight.shape[0], cin, H, W, N))
                if ctx.f16x3[0]:                              # ... or its split-precision form (ops.wide2d_f16x3 scope)
                    y, norm = wide_conv_f16x3(x, weight, b, he, flags)
                else:
                    ctx.part_n = _wide_part_n(x.shape[0])     # ops.wide_parts scope; the data gradient follows it
                    y, norm = wide_conv(x, weight, b, he, flags, part_n=ctx.part_n)
            else:
                wpack = _pk(weight, 'c3f', pack_conv3x3)
                y, norm = _conv3x3_raw(x, wpack, b, weight.shape[0], he, flags, True)
        ctx.flags, ctx.he = flags, he
        need_w = weight.requires_grad or (bias is not None and bias.requires_grad)
        # everything the backward reads goes through save_for_backward (autograd's version check then catches
        # in-place edits between forward and backward); None slots are allowed
        ctx.save_for_backward(y, norm, weight, x if need_w else None)
        return y

    @staticmethod
    def backward(ctx, gy):
        y, norm, w, x_saved = ctx.saved_tensors
        gp = _epilogue_bwd(cl(gy), y, norm, ctx.flags)
        gx = gw = gb = None
        with autocast(ctx.ac):                                # the backward runs under the policy of its forward
            if ctx.needs_input_grad[0]:
                if ctx.ac and _wino_ok(gp, w):
                    gx, _ = conv3d_c16_ring_bf16(gp, _pk(w, 'r3b', lambda t: pack_conv3d_c16_ring_bf16(t, transpose=True)), None, ctx.he, 0, 1)
                else:
                    gpc = _ac_in(gp)
                    if _wino_ok(gpc, w):
                        gx, _ = conv3d_c16_wino(gpc, _pk(w, 'w3b', lambda t: pack_conv3d_c16_wino(t, transpose=True)), None, ctx.he, 0)
                    elif ctx.f16x3[1]:
                        gx, _ = wide_conv_f16x3(gpc, w, None, ctx.he, 0, transpose=True)
                    elif _wino_gemm_ok(gpc, w):
                        gx, _ = wide_conv(gpc, w, None, ctx.he, 0, transpose=True, part_n=ctx.part_n)
                    else:
                        wpack_t = _pk(w, 'c3b', lambda t: pack_conv3x3(t, transpose=True))
                        gx, _ = _conv3x3_raw(gpc, wpack_t, None, w.shape[1], ctx.he, 0, False)
                    gx = _ac_in(gx)
            if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
                dims = w.dim() - 2
                # (autocast: the weight gradient sees the half-precision gradient; the bias is added in fp32, so its
                # gradient is the column sum of the un-rounded one)
                in_kernel = ctx.ac and _T()._wgrad_bf16_ok(gp, dims, w.shape[1], w.shape[0])       # that kernel rounds its operands itself
                gwt, gb = _T().conv_bwd_weight(x_saved, gp if in_kernel else _ac_in(gp), dims, w.shape[1], ctx.he, want_bias=not ctx.ac)
                if ctx.ac and ctx.needs_input_grad[2]:
                    gb = _T().bias_grad(gp, dims)
                k = (3,) * dims
                gw = _ac_in(gwt.reshape(*k, w.shape[0], w.shape[1]).permute(dims, dims + 1, *range(dims)).contiguous())
        return gx, gw if ctx.needs_input_grad[1] else None, gb if ctx.needs_input_grad[2] else None, None


def conv3x3(x, weight, bias, lrelu=True, pixelnorm=True, chain=False):
    """chain: x is the output of the previous convolution of the same Block and has no other consumer (ops_train._Conv16AC)."""
    flags = (LF_EPI_LRELU if lrelu else 0) | (LF_EPI_PIXELNORM if pixelnorm else 0)
    if _T()._conv16_ac_ok(x, weight):
        return _T()._Conv16AC.apply(x, weight, bias, flags, chain)
    return _Conv3x3.apply(_f32(x), weight, bias, flags)


def _conv1x1_raw(x_ptr_tensor, wpack, bias, N, P, cin, ksl, xbs, xss, cout, y2d, he, flags, yaddr=None, xscale=None):
    """y2d: output buffer; yaddr = (batch_stride, row_stride, slice_channels, slice_stride) or None
    for plain [N*P][cout] rows.  xscale: a factor per (sample, slice, pixel) applied to the operand (lf_conv1x1_fwd_scaled).
    Returns norm or None."""
    ybs, yrs, ysc, yss = yaddr if yaddr is not None else (P * cout, cout, 1 << 30, 0)
    fuse_pn = bool(flags & LF_EPI_PIXELNORM) and cout <= 128
    kflags = flags if fuse_pn else (flags & ~LF_EPI_PIXELNORM)
    norm = _norm_buf(flags, N * P, y2d.device)
    if xscale is not None:
        assert xscale.numel() == N * ksl * P and xscale.dtype == torch.float32 and xscale.is_contiguous()
        launch('lf_conv1x1_fwd_scaled', x_ptr_tensor, xscale, wpack, bias, y2d,
               norm if fuse_pn else None, N, P, cin, ksl, xbs, xss, cout, ybs, yrs, ysc, yss, he,
               kflags, SLOPE, PN_EPS)
    else:
        launch('lf_conv1x1_fwd', x_ptr_tensor, wpack, bias, y2d, norm if fuse_pn else None, N, P, cin,
               ksl, xbs, xss, cout, ybs, yrs, ysc, yss, he, kflags, SLOPE, PN_EPS)
    if (flags & LF_EPI_PIXELNORM) and not fuse_pn:
        launch('lf_pixelnorm_fwd', y2d, y2d, norm, N * P, cout, PN_EPS)
    return norm


def rows_gemm_epilogue(x2, wpack, bias, he, cout, flags=LF_EPI_LRELU | LF_EPI_PIXELNORM, tag='rows_gemm_epi'):
    """y = epilogue(he * x2 @ W^T + bias) over the rows of x2 [M][K] in ONE launch (lf_rows_gemm_epi; wpack = pack_rows_gemm(W)):
    -> (y [M][cout], norm [M] or None without LF_EPI_PIXELNORM).  Forward only, no autograd: the ranking path's factor
    projection (engine.RenderLoopEngine, proj_kernel='mfma', which times it under its own stage `tag`)."""
    L = _lib.lib()
    _req(x2, 'x2')
    _req(wpack, 'wpack')
    if x2.dim() != 2 or not x2.is_contiguous():
        raise ValueError('x2 must be a contiguous [M][K] matrix')
    M, K = x2.shape
    if wpack.dim() != 2 or not wpack.is_contiguous() or tuple(wpack.shape) != (L.lf_rows_gemm_cout_padded(cout), K):
        raise ValueError(f'wpack {tuple(wpack.shape)} is not pack_rows_gemm of a [{cout}][{K}] weight')
    if bias is not None:
        bias = _req(bias.detach(), 'bias').contiguous()
        if bias.numel() != cout:
            raise ValueError('bias must hold Cout values')
    y = torch.empty(M, cout, device=x2.device, dtype=torch.float32)
    norm = _norm_buf(flags, M, x2.device)
    launch('lf_rows_gemm_epi', x2, wpack, bias, y, norm, M, K, cout, he, flags, SLOPE, PN_EPS, tag=tag, detail=f'{M}x{K}x{cout}')
    return y, norm


class _Conv1x1(torch.autograd.Function):
    """Pointwise conv on NC[D]HW (channels-last) tensors; weight [Cout,Cin,1,1[,1]]."""

    @staticmethod
    def forward(ctx, x, weight, bias, flags):
        _req(x, 'x'), _req(weight, 'weight')
        ctx.ac = AUTOCAST is not None
        x = _ac_in(cl(x))
        N, cin = x.shape[0], x.shape[1]
        P = x[0, 0].numel()
        cout = weight.shape[0]
        he = he_constant(weight)
        wpack = _pk(weight, 'c1f', lambda w: pack_conv1x1(w.reshape(cout, cin)))
        y = empty_cl((N, cout) + tuple(x.shape[2:]), x.device)
        norm = _conv1x1_raw(x, wpack, bias.detach() if bias is not None else None, N, P, cin, 1, P * cin, 0, cout, y, he, flags)
        ctx.flags, ctx.he = flags, he
        need_w = weight.requires_grad or (bias is not None and bias.requires_grad)
        ctx.save_for_backward(y, norm, weight, x if need_w else None)
        return y

    @staticmethod
    def backward(ctx, gy):
        y, norm, w, x_saved = ctx.saved_tensors
        gp = _epilogue_bwd(cl(gy), y, norm, ctx.flags)
        cout, cin = w.shape[0], w.shape[1]
        gx = gw = gb = None
        with autocast(ctx.ac):
            gp_full, gp = gp, _ac_in(gp)
            if ctx.needs_input_grad[0]:
                wpack_t = _pk(w, 'c1b', lambda t: pack_conv1x1(t.reshape(cout, cin).t()))
                N = gp.shape[0]
                P = gp[0, 0].numel()
                gx = empty_cl((N, cin) + tuple(gp.shape[2:]), gp.device)
                _conv1x1_raw(gp, wpack_t, None, N, P, cout, 1, P * cout, 0, cin, gx, ctx.he, 0)
                gx = _ac_in(gx)
            if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
                rows = gp.numel() // cout                                   # channels-last: plain [rows][C] matrices
                gwt, gb = _T().conv_bwd_weight(x_saved.permute(0, *range(2, x_saved.dim()), 1).reshape(rows, cin),
                                          gp.permute(0, *range(2, gp.dim()), 1).reshape(rows, cout), 0, cin, ctx.he,
                                          want_bias=not ctx.ac)
                if ctx.ac and ctx.needs_input_grad[2]:
                    gb = _T().bias_grad(gp_full.permute(0, *range(2, gp_full.dim()), 1).reshape(rows, cout), 0)
                gw = _ac_in(gwt.reshape(w.shape))
        return gx, gw if ctx.needs_input_grad[1] else None, gb if ctx.needs_input_grad[2] else None, None


def conv1x1(x, weight, bias, lrelu=False, pixelnorm=False):
    flags = (LF_EPI_LRELU if lrelu else 0) | (LF_EPI_PIXELNORM if pixelnorm else 0)
    if _T()._conv16_ac_ok(x, weight):                       # (the encoder's 16 -> 16 output layer: the ring kernel's centre tap)
        return _T()._Conv16AC.apply(x, weight, bias, flags, False)
    return _Conv1x1.apply(_f32(x), weight, bias, flags)


class _FactorProject(torch.autograd.Function):
    """FactorProjection3d2d (modules/geometry.py:731-749): folds the depth axis of a
    channels-last volume into the contraction dimension without copying it."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.x_bf16 = x.dtype == torch.bfloat16
        ctx.ac = AUTOCAST is not None
        ctx.mfma = bool(PROJ_MFMA and ctx.ac and ctx.x_bf16 and x.dim() == 5 and x.shape[1] == 16 and weight.shape[0] == 16
                        and x.shape[2] in (16, 32, 64, 128) and (x.shape[3] * x.shape[4]) % 16 == 0 and x.is_cuda)
        if ctx.mfma:
            # round 6 (csrc/lift_mfma.hip): the bf16 volume read as it lies, one MFMA per depth; no fp32 copy of the volume
            _req(weight, 'weight')
            x = cl(x)
            N, C, D, H, W = x.shape
            he = he_constant(weight)
            wtab = _pk(weight, 'p16f', lambda w: w.reshape(16, 16, D).permute(2, 0, 1).contiguous().to(torch.bfloat16))
            y = empty_cl((N, 16, H, W), x.device)
            norm = torch.empty(N * H * W, device=x.device, dtype=torch.float32)
            launch('lf_proj16_fwd', x, wtab, bias, y, norm, N * H * W, H * W, D, he, SLOPE, PN_EPS, tag='proj16_fwd')
            ctx.flags, ctx.he, ctx.xshape = LF_EPI_LRELU | LF_EPI_PIXELNORM, he, x.shape
            ctx.save_for_backward(y, norm, weight, x)
            return y
        x = _f32(x)
        _req(x, 'x'), _req(weight, 'weight')
        x = cl(x) if ctx.x_bf16 else _ac_in(cl(x))             # (a bf16-stored volume is already rounded)
        N, C, D, H, W = x.shape
        cout = weight.shape[0]
        he = he_constant(weight)                      # fan_in = C*D
        # reference K index = c*D + d; kernel K index = d*C + c
        wpack = _pk(weight, 'fpf', lambda w: pack_conv1x1(w.reshape(cout, C, D).permute(0, 2, 1).reshape(cout, D * C)))
        y = empty_cl((N, cout, H, W), x.device)
        flags = LF_EPI_LRELU | LF_EPI_PIXELNORM
        if C % 4:
            raise NotImplementedError('factor projection needs C % 4 == 0 on the HIP path')
        norm = _conv1x1_raw(x, wpack, bias.detach() if bias is not None else None, N, H * W, C, D,
                            D * H * W * C, H * W * C, cout, y, he, flags)
        ctx.flags, ctx.he, ctx.xshape = flags, he, x.shape
        need_w = weight.requires_grad or (bias is not None and bias.requires_grad)
        ctx.save_for_backward(y, norm, weight, x if need_w else None)
        return y

    @staticmethod
    def backward(ctx, gy):
        y, norm, w, x_saved = ctx.saved_tensors
        gp = _epilogue_bwd(cl(gy), y, norm, ctx.flags)
        N, C, D, H, W = ctx.xshape
        cout = w.shape[0]
        gw = gb = None
        if ctx.mfma:
            L = _lib.lib()
            wtab_t = _pk(w, 'p16b', lambda t: t.reshape(16, 16, D).permute(2, 1, 0).contiguous().to(torch.bfloat16))
            gx = empty_cl16((N, 16, D, H, W), gp.device, True)
            gwt = torch.empty(16, 16 * D, device=gp.device, dtype=torch.float32)
            nb = L.lf_proj16_bwd_scratch_bytes(D)
            scr = torch.empty(nb // 4 + 4, device=gp.device, dtype=torch.float32)
            launch('lf_proj16_bwd', gp, x_saved, wtab_t, gx, gwt, scr.data_ptr(), scr.numel() * 4, N * H * W, H * W, D, ctx.he,
                   tag='proj16_bwd')
            with autocast(True):
                if ctx.needs_input_grad[2]:
                    gb = _T().bias_grad(gp.permute(0, 2, 3, 1).reshape(N * H * W, cout), 0)
                gw = _ac_in(gwt.reshape(w.shape))
            return gx, gw if ctx.needs_input_grad[1] else None, gb if ctx.needs_input_grad[2] else None
        with autocast(ctx.ac):
            gp_full, gp = gp, _ac_in(gp)
            # gx[n,d,p,c] = he * sum_co gp[n,p,co] * W[co, c*D+d]  == pointwise conv with Cout' = D*C
            wt = _pk(w, 'fpb', lambda t: pack_conv1x1(t.reshape(cout, C, D).permute(2, 1, 0).reshape(D * C, cout)))
            # output channel d*C + c of pixel p goes straight to gx[n][d][p][c] (channels-last volume)
            gx = empty_cl((N, C, D, H, W), gp.device)
            _conv1x1_raw(gp, wt, None, N, H * W, cout, 1, H * W * cout, 0, D * C, gx, ctx.he, 0,
                         yaddr=(D * H * W * C, C, C, H * W * C))
            gx = _ac_in(gx)
            if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
                # rows = pixels, K = (c, d) in the reference's order c*D + d: one copy of the volume (training only)
                if _lift_ok(C, D):
                    xr = _lift_permute(x_saved, N, H * W, C, D, True, torch.empty(N * H * W, C * D, device=gp.device, dtype=torch.float32))
                else:
                    xr = x_saved.permute(0, 3, 4, 1, 2).reshape(N * H * W, C * D).contiguous()
                gwt, gb = _T().conv_bwd_weight(xr, gp.permute(0, 2, 3, 1).reshape(N * H * W, cout), 0, C * D, ctx.he,
                                          want_bias=not ctx.ac)
                if ctx.ac and ctx.needs_input_grad[2]:
                    gb = _T().bias_grad(gp_full.permute(0, 2, 3, 1).reshape(N * H * W, cout), 0)
                gw = _ac_in(gwt.reshape(w.shape))
        if ctx.x_bf16:
            gx = gx.to(torch.bfloat16)
        return gx, gw if ctx.needs_input_grad[1] else None, gb if ctx.needs_input_grad[2] else None


def factor_project(x, weight, bias):
    return _FactorProject.apply(x, weight, bias)


import os as _os
PROJ_MFMA = bool(int(_os.environ.get('LF_PROJ_MFMA', '1')))   # the training step's 3-D -> 2-D factor projection as one MFMA kernel each way (csrc/lift_mfma.hip)
LIFT_FUSED = True          # A/B switch of the fused training-path lift (_LiftFused); False: conv1x1 + PixelNorm + permutation


def _lift_permute(src, V, P, c0, S, fold, out):
    launch('lf_lift_permute', src, out, V, P, c0, S, 1 if fold else 0)
    return out


def _lift_ok(c0, S):
    return 4 * c0 * (S + 1) * 4 <= 64 * 1024


def lift(x, weight, bias, out_size):
    """FactorProjection2d3d (modules/geometry.py:711-728): 1x1 conv to C0*S channels, LeakyReLU,
    PixelNorm over ALL C0*S channels, viewed as (V,C0,S,H,W).  The fused unfold below is the inference path;
    when a gradient is wanted the same result is composed from the differentiable pointwise conv and a
    layout copy."""
    _req(x, 'x')
    x = cl(x)
    V, cin, H, W = x.shape
    cs = weight.shape[0]
    c0 = cs // out_size
    if torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad or (bias is not None and bias.requires_grad)):
        if LIFT_FUSED and _T()._lift_fused_ok(c0, out_size) and c0 * out_size == cs:
            return _T()._LiftFused.apply(x, weight, bias, out_size)
        y = conv1x1(x, weight, bias, lrelu=True, pixelnorm=True)            # (V, c0*S, H, W), channel = c*S + d
        if _lift_ok(c0, out_size):
            return _T()._LiftView.apply(y, c0, out_size)
        return cl(y.view(V, c0, out_size, H, W))
    he = he_constant(weight)
    wpack = _cached(weight, 'c1f', lambda: pack_conv1x1(weight.reshape(cs, cin)))
    P = H * W
    tmp = torch.empty(V * P, cs, device=x.device, dtype=torch.float32)
    norm = _conv1x1_raw(x, wpack, bias.detach() if bias is not None else None, V, P, cin, 1, P * cin, 0, cs, tmp, he,
                        LF_EPI_LRELU | (LF_EPI_PIXELNORM if cs <= 128 else 0))
    if cs > 128:
        norm = torch.empty(V * P, device=x.device, dtype=torch.float32)
        # norm only: normalisation itself is folded into the unfold pass below
        tmp2 = torch.empty_like(tmp)
        launch('lf_pixelnorm_fwd', tmp, tmp2, norm, V * P, cs, PN_EPS)
        tmp = tmp2
    out = empty_cl((V, c0, out_size, H, W), x.device)
    launch('lf_lift_unfold', tmp, None, out, V, P, c0, out_size)
    return out


# ---------------------------------------------------------------------------------------------
# depth-column composites (renderer) and view reductions (fusers)
# ---------------------------------------------------------------------------------------------
class _ColumnSum(torch.autograd.Function):
    """(N,C,D,H,W) -> (N,C,H,W), sum over the depth axis: the 'sum' projection (recon/models.py:436-437)."""

    @staticmethod
    def forward(ctx, x):
        x = cl(_req(_f32(x), 'x'))
        N, C, D, H, W = x.shape
        y = empty_cl((N, C, H, W), x.device)
        launch('lf_column_reduce_sum_fwd', x, y, N, D, H * W, C, tag='column_sum')
        ctx.xshape = tuple(x.shape)
        return y

    @staticmethod
    def backward(ctx, gy):
        N, C, D, H, W = ctx.xshape
        g = cl(gy)
        gx = empty_cl(ctx.xshape, g.device)
        launch('lf_column_reduce_sum_bwd', g, gx, N, D, H * W, C)
        return gx


def column_sum(x):
    return _ColumnSum.apply(x)


class _ColumnSoftmax(torch.autograd.Function):
    """Single-channel logits (N,1,D,H,W) -> (softmax over D (N,1,D,H,W), expected depth sum_d w * linspace(-1,1,D)
    (N,1,H,W)): Photographer._compute_depth_weights / _depth_from_weight (recon/models.py:378-395)."""

    @staticmethod
    def forward(ctx, logits):
        lg = _req(logits, 'logits').contiguous()
        N, one, D, H, W = lg.shape
        if one != 1:
            raise ValueError('column_softmax expects single-channel logits')
        w = torch.empty_like(lg)
        zd = torch.empty(N, 1, H, W, device=lg.device, dtype=torch.float32)
        launch('lf_column_softmax_fwd', lg, w, zd, N, D, H * W, tag='column_softmax')
        ctx.save_for_backward(w)
        ctx.set_materialize_grads(False)
        return w, zd

    @staticmethod
    def backward(ctx, gw, gzd):
        w, = ctx.saved_tensors
        N, _, D, H, W = w.shape
        if gw is None and gzd is None:
            return None
        gw = gw.contiguous() if gw is not None else None
        gzd = gzd.contiguous() if gzd is not None else None
        gl = torch.empty_like(w)
        launch('lf_column_softmax_bwd', w, gw, gzd, gl, N, D, H * W)
        return gl


def column_softmax(logits):
    return _ColumnSoftmax.apply(logits)


class _ColumnScale(torch.autograd.Function):
    """z (N,C,D,H,W) * w (N,1,D,H,W): the occlusion weighting z * depth_weights_resized (recon/models.py:427-430)."""

    @staticmethod
    def forward(ctx, z, w):
        z = cl(_req(_f32(z), 'z'))
        w = _req(w, 'w').contiguous()
        N, C, D, H, W = z.shape
        if tuple(w.shape) != (N, 1, D, H, W) or C % 4:
            raise ValueError('column_scale: w must be (N,1,D,H,W) and C a multiple of 4')
        out = empty_cl(z.shape, z.device)
        launch('lf_column_scale_fwd', z, w, out, N * D * H * W, C)
        ctx.save_for_backward(z, w)
        return out

    @staticmethod
    def backward(ctx, gout):
        z, w = ctx.saved_tensors
        N, C, D, H, W = z.shape
        g = cl(gout)
        gz = empty_cl(z.shape, z.device) if ctx.needs_input_grad[0] else None
        gw = torch.empty_like(w) if ctx.needs_input_grad[1] else None
        if gz is None and gw is None:
            return None, None
        launch('lf_column_scale_bwd', g, z, w, gz, gw, N * D * H * W, C)
        return gz, gw


def column_scale(z, w):
    return _ColumnScale.apply(z, w)


def _dense_views(z):
    """(B,V,...) -> (B*V,...) with every view dense in ONE common element order (channels-last when the per-view
    tensors are 4-/5-D, which is what the encoder produces: no copy then)."""
    zz = z.reshape(z.shape[0] * z.shape[1], *z.shape[2:])
    return cl(zz) if zz.dim() in (4, 5) else zz.contiguous()


def _dense_views_f32(z):
    return _dense_views(_f32(z))


FUSE_KINDS = {'mean': _lib.LF_FUSE_MEAN, 'max': _lib.LF_FUSE_MAX, 'abs_max': _lib.LF_FUSE_ABSMAX, 'median': _lib.LF_FUSE_MEDIAN}


class _FuseViews(torch.autograd.Function):
    """PoolFuser reductions over the view axis: z (B,V,...) -> (B,1,...)  (recon/fusion.py:45-57)."""

    @staticmethod
    def forward(ctx, z, kind):
        z = _f32(z)
        _req(z, 'z')
        B, V = z.shape[0], z.shape[1]
        zz = _dense_views(z)
        n = zz[0].numel()
        out = torch.empty_like(zz[:B])
        need_idx = kind != _lib.LF_FUSE_MEAN and ctx.needs_input_grad[0]
        idx = torch.empty(B, n, device=z.device, dtype=torch.int32) if need_idx else None
        with _timed('fuse_views'):
            for b in range(B):
                launch('lf_fuse_views_fwd', zz[b * V], out[b], idx[b] if idx is not None else None, kind, V, n, n)
        ctx.meta = (kind, B, V, n, tuple(zz.shape), tuple(z.shape))
        if idx is not None:
            ctx.save_for_backward(idx)
        return out.unsqueeze(1)

    @staticmethod
    def backward(ctx, g):
        kind, B, V, n, zshape, orig = ctx.meta
        idx = ctx.saved_tensors[0] if ctx.saved_tensors else None
        g = g.squeeze(1)
        g = cl(g) if g.dim() in (4, 5) else g.contiguous()
        gz = torch.empty(zshape, device=g.device, dtype=torch.float32,
                         memory_format=(torch.channels_last_3d if len(zshape) == 5 else torch.channels_last if len(zshape) == 4
                                        else torch.contiguous_format))
        for b in range(B):
            launch('lf_fuse_views_bwd', g[b], idx[b] if idx is not None else None, gz[b * V], kind, V, n, n)
        return gz.view(orig), None


def fuse_views(z, pool_type):
    if pool_type not in FUSE_KINDS:
        raise ValueError(f'Unknown pool_type value {pool_type}')
    return _FuseViews.apply(z, FUSE_KINDS[pool_type])


class _FuseBlend(torch.autograd.Function):
    """BlendFuser.forward (recon/fusion.py:139-148): z (B,V,C,D,H,W), logits (B,V,1,D,H,W) ->
    (sum_v z * softmax_v(logits) (B,1,C,D,H,W), weights (B,V,1,D,H,W))."""

    @staticmethod
    def forward(ctx, z, logits):
        z = _f32(z)
        _req(z, 'z'), _req(logits, 'logits')
        B, V, C = z.shape[:3]
        zz = _dense_views(z)                                    # (B*V,C,D,H,W) channels-last
        lg = logits.reshape(B * V, -1).contiguous()             # (B*V, rows)
        rows = lg.shape[1]
        if zz[0].numel() != rows * C or C % 4:
            raise ValueError('fuse_blend: shapes of z and logits do not match / C % 4 != 0')
        w = torch.empty_like(lg)
        out = torch.empty_like(zz[:B])
        with _timed('fuse_blend'):
            for b in range(B):
                launch('lf_fuse_blend_fwd', zz[b * V], lg[b * V], w[b * V], out[b], V, rows, C, rows * C, rows)
        ctx.save_for_backward(zz, w)
        ctx.meta = (B, V, C, rows, tuple(z.shape), tuple(logits.shape))
        ctx.mark_non_differentiable(w)
        return out.unsqueeze(1), w.view(logits.shape)

    @staticmethod
    def backward(ctx, g, _gw):
        zz, w = ctx.saved_tensors
        B, V, C, rows, zshape, lshape = ctx.meta
        g = cl(g.squeeze(1))
        gz = torch.empty_like(zz) if ctx.needs_input_grad[0] else None
        gl = torch.empty_like(w) if ctx.needs_input_grad[1] else None
        if gz is None and gl is None:
            return None, None
        for b in range(B):
            launch('lf_fuse_blend_bwd', g[b], zz[b * V], w[b * V], gz[b * V] if gz is not None else None,
                   gl[b * V] if gl is not None else None, V, rows, C, rows * C, rows)
        return (gz.view(zshape) if gz is not None else None), (gl.view(lshape) if gl is not None else None)


def fuse_blend(z, logits):
    return _FuseBlend.apply(z, logits)


# ---------------------------------------------------------------------------------------------
# 2-D grid sampling (image crops / uncrops / IBR warps)
# ---------------------------------------------------------------------------------------------
class _GridSample2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, grid, bilinear, border):
        _req(img, 'image')
        img, grid = img.float().contiguous(), grid.float().contiguous()
        N, C, H, W = img.shape
        Ho, Wo = grid.shape[1], grid.shape[2]
        if grid.shape[0] != N or grid.shape[3] != 2:
            raise ValueError('grid must be (N, Ho, Wo, 2)')
        out = torch.empty(N, C, Ho, Wo, device=img.device, dtype=torch.float32)
        launch('lf_grid_sample2d_fwd', img, grid, out, N, C, H, W, Ho, Wo, int(bilinear), int(border))
        ctx.save_for_backward(img, grid)
        ctx.mode = (int(bilinear), int(border))
        return out

    @staticmethod
    def backward(ctx, gout):
        img, grid = ctx.saved_tensors
        N, C, H, W = img.shape
        Ho, Wo = grid.shape[1], grid.shape[2]
        gimg = torch.zeros_like(img) if ctx.needs_input_grad[0] else None
        ggrid = torch.empty_like(grid) if ctx.needs_input_grad[1] else None
        if gimg is None and ggrid is None:
            return None, None, None, None
        launch('lf_grid_sample2d_bwd', img, grid, gout.float().contiguous(), gimg, ggrid, N, C, H, W, Ho, Wo, ctx.mode[0],
               ctx.mode[1])
        return gimg, ggrid, None, None


def grid_sample2d(img, grid, mode='bilinear', padding_mode='zeros'):
    """F.grid_sample(img, grid, mode, padding_mode, align_corners=False) for 4-D inputs on the HIP path."""
    if mode not in ('bilinear', 'nearest') or padding_mode not in ('zeros', 'border'):
        raise ValueError(f'unsupported mode {mode!r} / padding {padding_mode!r}')
    return _GridSample2d.apply(img, grid, mode == 'bilinear', padding_mode == 'border')


# ---------------------------------------------------------------------------------------------
# fused IBR reprojection (ibr.reproject_views as one launch for all objects, views and pixels)
# ---------------------------------------------------------------------------------------------
class IbrRecords:
    """Camera records of lf_ibr_reproject_* (layout: include/lf_hip.h): `pair` (B,V_o,V_i,32), `view_in` (B,V_i,16),
    `view_out` (B,V_o,16), fp32, slices of one buffer so that `to(device)` is one copy."""

    def __init__(self, flat, batch, n_out, n_in):
        self.flat, self.batch, self.n_out, self.n_in = flat, batch, n_out, n_in
        n_pair, n_vin = batch * n_out * n_in * _lib.LF_IBR_PAIR_FLOATS, batch * n_in * _lib.LF_IBR_VIEW_FLOATS
        self.pair = flat[:n_pair].view(batch, n_out, n_in, _lib.LF_IBR_PAIR_FLOATS)
        self.view_in = flat[n_pair:n_pair + n_vin].view(batch, n_in, _lib.LF_IBR_VIEW_FLOATS)
        self.view_out = flat[n_pair + n_vin:].view(batch, n_out, _lib.LF_IBR_VIEW_FLOATS)

    def to(self, device):
        return IbrRecords(self.flat.to(device), self.batch, self.n_out, self.n_in)


def _mm4(a, b):
    """(..., n, 4) @ (..., 4, m), written out term by term: every element is the same four products and three sums whatever
    the batch shape, which a library matmul does not promise."""
    return sum(a[..., :, k, None] * b[..., None, k, :] for k in range(4))


def pack_ibr_cameras(camera_in, camera_out, batch_size=1, depth_eps=0.01):
    """Host packing of the camera records of `ibr_reproject` for flat, object-major cameras (len = batch_size * views).

    Per pair (o, i): output camera -> object -> input image with the input viewport folded in, and input camera -> object ->
    z row of the output camera with the output camera's depth normalisation folded in; per view: the unprojection of the
    viewport lattice (and, for output views, the depth denormalisation).  Everything is formed in fp64 from the Camera
    properties, pair by pair (a record does not depend on its batch mates), and rounded once to fp32; the entries of the
    sampling-coordinate chain also carry the fp32 rounding of what that leaves (see the header).  Returns IbrRecords on the
    cameras' device."""
    dev = camera_in.device
    if camera_out.device != dev:
        raise ValueError('camera_in and camera_out must be on one device')
    n_in, n_out = len(camera_in) // batch_size, len(camera_out) // batch_size
    if n_in * batch_size != len(camera_in) or n_out * batch_size != len(camera_out) or n_in < 1 or n_out < 1:
        raise ValueError('the camera counts must be positive multiples of batch_size')

    def host(cam, n):
        c = cam._map(lambda t: t.detach().to('cpu', torch.float64))
        rot, t = c.rotation_matrix[:, :3, :3], c.translation
        ext = torch.zeros(len(c), 4, 4, dtype=torch.float64)
        inv = torch.zeros(len(c), 4, 4, dtype=torch.float64)
        ext[:, :3, :3], ext[:, :3, 3], ext[:, 3, 3] = rot, t, 1.0                           # obj_to_cam
        inv[:, :3, :3], inv[:, 3, 3] = rot.transpose(1, 2), 1.0                             # cam_to_obj
        inv[:, :3, 3] = -sum(rot[:, k, :] * t[:, k, None] for k in range(3))
        vp = c.viewport
        view = torch.zeros(len(c), _lib.LF_IBR_VIEW_FLOATS, dtype=torch.float64)
        view[:, 0], view[:, 1] = c.viewport_width / c.fu, (vp[:, 0] - c.u0) / c.fu
        view[:, 2], view[:, 3] = c.viewport_height / c.fv, (vp[:, 1] - c.v0) / c.fv
        zn, zf = c.znear - depth_eps, c.zfar + depth_eps
        view[:, 4], view[:, 5] = (zf - zn) / 2.0, (zf + zn) / 2.0
        bv = lambda x: x.view(batch_size, n, *x.shape[1:])                                   # noqa: E731
        return dict(K=bv(c.intrinsic), ext=bv(ext), inv=bv(inv), vp=bv(vp), view=bv(view), zn=bv(zn), zf=bv(zf))

    ci, co = host(camera_in, n_in), host(camera_out, n_out)
    # (B, V_o, V_i, ., .) by broadcasting: i on axis 2, o on axis 1
    to_img = _mm4(_mm4(ci['K'][:, None], ci['ext'][:, None]), co['inv'][:, :, None])         # 3x4
    vp_i = ci['vp'][:, None]
    n0 = (to_img[..., 0, :] - vp_i[..., 0, None] * to_img[..., 2, :]) / (vp_i[..., 2] - vp_i[..., 0])[..., None]
    n1 = (to_img[..., 1, :] - vp_i[..., 1, None] * to_img[..., 2, :]) / (vp_i[..., 3] - vp_i[..., 1])[..., None]
    zrow = _mm4(co['ext'][:, :, None, 2:3, :], ci['inv'][:, None])[..., 0, :].clone()         # 1x4
    zn, zf = co['zn'][:, :, None], co['zf'][:, :, None]
    zrow[..., 3] = zrow[..., 3] - zn
    zrow = zrow / (zf - zn)[..., None]
    def split(v, n, at):                                # entries [0, n): leading float at [k], float of the remainder at [at + k]
        lead = v.to(torch.float32)
        lead[..., at:at + n] = (v[..., :n] - lead[..., :n].double()).to(torch.float32)
        return lead

    pair = torch.zeros(*n0.shape[:-1], _lib.LF_IBR_PAIR_FLOATS, dtype=torch.float64)
    pair[..., 0:4], pair[..., 4:8], pair[..., 8:12], pair[..., 12:16] = n0, n1, to_img[..., 2, :], zrow
    view_in = ci['view'].clone()
    view_in[..., 4:] = 0.0
    flat = torch.cat((split(pair, 12, _lib.LF_IBR_PAIR_SPLIT).reshape(-1), view_in.to(torch.float32).reshape(-1),
                      split(co['view'], 6, _lib.LF_IBR_VIEW_SPLIT).reshape(-1)))
    return IbrRecords(flat.to(dev), batch_size, n_out, n_in)


def _ibr_shapes(image_in, depth_in, depth_out, mask_out, rec):
    if image_in.dim() != 5:
        raise ValueError('image_in must be (B, V_i, C, H, W)')
    B, Vi, C, H, W = image_in.shape
    Vo = rec.n_out
    if (rec.batch, rec.n_in) != (B, Vi):
        raise ValueError(f'records are for (B, V_i) = {(rec.batch, rec.n_in)}, image_in has {(B, Vi)}')
    for t, n, name in ((depth_in, Vi, 'depth_in'), (depth_out, Vo, 'depth_out'), (mask_out, Vo, 'mask_out')):
        if t is not None and (t.numel() != B * n * H * W or tuple(t.shape[:2]) != (B, n) or tuple(t.shape[-2:]) != (H, W)):
            raise ValueError(f'{name} must be (B, {n}, 1, H, W) = ({B}, {n}, 1, {H}, {W}), got {tuple(t.shape)}')
    return B, Vo, Vi, C, H, W


def _ibr_fwd(image_in, depth_in, depth_out, mask_out, rec, out):
    for t, name in ((image_in, 'image_in'), (depth_in, 'depth_in'), (depth_out, 'depth_out'), (rec.flat, 'records')):
        _req(t, name)
    B, Vo, Vi, C, H, W = _ibr_shapes(image_in, depth_in, depth_out, mask_out, rec)
    image_in, depth_in, depth_out = image_in.contiguous(), depth_in.contiguous(), depth_out.contiguous()
    if mask_out is not None:
        mask_out = _req(mask_out, 'mask_out').contiguous()
    if out is None:
        image_re = torch.empty(B, Vo, Vi, C, H, W, device=image_in.device, dtype=torch.float32)
        depth_re = torch.empty(B, Vo, Vi, 1, H, W, device=image_in.device, dtype=torch.float32)
        strides = (C * H * W, H * W)
    else:
        rows = out.view(B, Vo, Vi, C + 2, H, W)
        image_re, depth_re = rows[:, :, :, :C], rows[:, :, :, C:C + 1]
        strides = ((C + 2) * H * W, (C + 2) * H * W)
    launch('lf_ibr_reproject_fwd', image_in, depth_in, depth_out, mask_out, rec.pair.data_ptr(), rec.view_in.data_ptr(),
           rec.view_out.data_ptr(), image_re, depth_re, B, Vo, Vi, C, H, W, strides[0], strides[1])
    return (image_in, depth_in, depth_out, mask_out), (image_re, depth_re)


class _IbrReproject(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image_in, depth_in, depth_out, mask_out, rec):
        saved, outs = _ibr_fwd(image_in, depth_in, depth_out, mask_out, rec, None)
        ctx.save_for_backward(*saved)
        ctx.rec = rec
        return outs

    @staticmethod
    def backward(ctx, g_image, g_depth):
        image_in, depth_in, depth_out, mask_out = ctx.saved_tensors
        rec = ctx.rec
        B, Vo, Vi, C, H, W = _ibr_shapes(image_in, depth_in, depth_out, mask_out, rec)
        need = ctx.needs_input_grad
        if not any(need[:3]) or (g_image is None and g_depth is None):
            return None, None, None, None, None
        g_image = g_image.float().contiguous() if g_image is not None else None
        g_depth = g_depth.float().contiguous() if g_depth is not None else None
        gi = torch.zeros_like(image_in) if need[0] else None
        gdi = torch.zeros_like(depth_in) if need[1] else None
        gdo = torch.empty_like(depth_out) if need[2] else None
        launch('lf_ibr_reproject_bwd', image_in, depth_in, depth_out, mask_out, rec.pair.data_ptr(), rec.view_in.data_ptr(),
               rec.view_out.data_ptr(), g_image, g_depth, gi, gdi, gdo, B, Vo, Vi, C, H, W)
        return gi, gdi, gdo, None, None


def ibr_reproject(image_in, depth_in, depth_out, records, mask_out=None, out=None):
    """ibr.reproject_views for B objects in one launch (lf_ibr_reproject_fwd / _bwd): image_in (B,V_i,C,H,W), depth_in
    (B,V_i,1,H,W), depth_out (B,V_o,1,H,W), records = pack_ibr_cameras(...).  Returns (image_re, depth_re), shaped
    (B,V_o,V_i,C|1,H,W).  mask_out (B,V_o,1,H,W): the outputs are image_re * m and (depth_re + 1) * m - 1, bit for bit
    (a constant: a mask that requires grad is refused).  out: a contiguous (B*V_o, V_i, C+2, H, W) buffer the results are
    written into (channels [0, C) and C; channel C+1 is left alone); the returned tensors are views of it and carry no
    gradient, so inputs that require grad are refused with `out`.  Differentiable w.r.t. image_in, depth_in, depth_out."""
    if not isinstance(records, IbrRecords):
        raise TypeError('records must come from pack_ibr_cameras')
    grad = torch.is_grad_enabled()
    if mask_out is not None and grad and mask_out.requires_grad:
        raise NotImplementedError('ibr_reproject: mask_out is a constant of the fused kernel; apply a differentiable mask outside')
    if out is not None:
        if grad and any(t.requires_grad for t in (image_in, depth_in, depth_out)):
            raise NotImplementedError('ibr_reproject: results written into `out` carry no gradient')
        B, Vi, C, H, W = image_in.shape
        if not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous()
                and out.numel() == B * records.n_out * Vi * (C + 2) * H * W):
            raise ValueError('out must be a contiguous float32 device tensor of B*V_o*V_i*(C+2)*H*W elements')
        with torch.no_grad():
            return _ibr_fwd(image_in, depth_in, depth_out, mask_out, records, out)[1]
    return _IbrReproject.apply(image_in, depth_in, depth_out, mask_out, records)


# ---------------------------------------------------------------------------------------------
# standalone PixelNorm / rescale
# ---------------------------------------------------------------------------------------------
class _PixelNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        _req(x, 'x')
        x = cl(x)
        rows = x.numel() // x.shape[1]
        y = torch.empty_like(x, memory_format=torch.preserve_format)
        norm = torch.empty(rows, device=x.device, dtype=torch.float32)
        launch('lf_pixelnorm_fwd', x, y, norm, rows, x.shape[1], PN_EPS)
        ctx.save_for_backward(y, norm)
        return y

    @staticmethod
    def backward(ctx, gy):
        y, norm = ctx.saved_tensors
        return _epilogue_bwd(cl(gy), y, norm, LF_EPI_PIXELNORM)


def pixelnorm(x):
    return _PixelNorm.apply(x)


class _Resize(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, linear, up):
        _req(x, 'x')
        x = cl(x)
        dims = x.dim() - 2
        N, C = x.shape[0], x.shape[1]
        D, H, W = (x.shape[2:] if dims == 3 else (1,) + tuple(x.shape[2:]))
        out_sp = tuple((s * 2 if up else s // 2) for s in x.shape[2:])
        y = empty_cl((N, C) + out_sp, x.device)
        launch('lf_resize_fwd', x, y, dims, N, D, H, W, C, linear, up)
        ctx.meta = (dims, N, C, D, H, W, linear, up, tuple(x.shape))
        return y

    @staticmethod
    def backward(ctx, gy):
        dims, N, C, D, H, W, linear, up, xshape = ctx.meta
        g = cl(gy)
        gx = empty_cl(xshape, g.device)
        launch('lf_resize_bwd', g, gx, dims, N, D, H, W, C, linear, up)
        return gx, None, None


def interpolate(x, scale_factor, mode):
    """Block-end rescale (modules/__init__.py:18-36): x2 / x0.5, nearest or (bi|tri)linear with
    align_corners=False -- the only combinations the block grammar (I/U/D tokens) can produce."""
    if scale_factor not in (2.0, 0.5) or mode not in ('nearest', 'bilinear', 'trilinear'):
        raise NotImplementedError(f'rescale {scale_factor} / {mode} is not produced by the block grammar')
    return _Resize.apply(x, 0 if mode == 'nearest' else 1, 1 if scale_factor == 2.0 else 0)


def resize_nearest_to(x, size):
    """F.interpolate(x, size) (nearest) for cubic / square maps whose size ratio is a power of two -- what the occlusion
    U-Net's logits need when its resolution differs from the volume's (reference recon/models.py:385) -- on lf_resize_*."""
    cur = x.shape[-1]
    if any(d != cur for d in x.shape[2:]):
        raise NotImplementedError('resize_nearest_to expects equal spatial extents')
    while cur < size:
        x, cur = interpolate(x, 2.0, 'nearest'), cur * 2
    while cur > size:
        if cur % 2:
            break
        x, cur = interpolate(x, 0.5, 'nearest'), cur // 2
    if cur != size:
        raise NotImplementedError(f'resize from {x.shape[-1]} to {size} is not a power-of-two ratio')
    return x
