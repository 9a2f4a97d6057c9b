"""What tests/test_conv_direct_fp64_gpu.py, tests/test_rows_epilogue_fp64_gpu.py and tests/test_conv_direct_cases.py share: an
explicit restatement of the exact-fp32 convolutions of include/lf_hip.h (lf_conv3x3_fwd, lf_conv3x3_bwd_data, lf_conv1x1_fwd,
lf_conv1x1_fwd_scaled, lf_conv1x1_bwd_data) and of the row kernels (lf_pixelnorm_fwd, lf_epilogue_bwd(_amax)), evaluated in fp64
(the reference) and in fp32 (e32, and the stand-in for the kernel where there is no GPU); the host-side weight layouts as the
header words them; the cases; a Python restatement of the dispatch (which kernel form a call reaches); the bound; and the
misreadings the comparison has to reject.  Nothing here needs a GPU or the package.

THE RESTATEMENT is written out tap by tap on channels-last arrays [N][D][H][W][C] (dims = 2: D = 1):

    forward        v = (sum over taps t of x[voxel + t - 1] . W_t) * he + bias ; [v = v > 0 ? v : slope v] ;
                   [r = sqrt(mean_c(v^2) + eps), y = v / r]                       -> y, r
    data gradient  g = (sum over taps t of gy[voxel - (t - 1)] . W_t^T) * he, then, with the producing layer's saved output
                   y_prev, norm_prev and flags:   [g = (g - y_prev mean_c(g y_prev)) / norm_prev] ; [g = y_prev > 0 ? g : slope g]
                   or, LF_EPI_DOT: g as it is and dot[record] = sum_c g[c] y_prev[c] per 16-channel record
    pointwise      operand element (n, p, k = s Cin + c) = xbuf[n x_batch_stride + s x_slice_stride + p Cin + c]
                   [* xscale[(n ksl + s) P + p], the product rounded to fp32]; output channel co of pixel p of sample n at
                   ybuf[n y_batch_stride + (co / y_slice_channels) y_slice_stride + p y_row_stride + co % y_slice_channels]

y_prev and norm_prev are INPUTS (the fp64 forward of a producer layer, rounded to fp32), so both sides decide LeakyReLU' on
the same bits and no element is excluded.  One voxel of every fused-gradient case has an all-zero producer row: y_prev = 0 and
norm = sqrt(eps), a gradient 1e4 times the others.

THE BOUND is the project's standing form, per element |got - fp64| <= max(4 e32, 2e-6 + 2e-5 s): e32 the largest |fp32 - fp64|
of the same expressions over the case's output, s = |fp64| of the element for the forward outputs and the raw gradient, the
largest |fp64| of the element's record (the channels that share a norm) for the fused gradients, the largest |pre-normalisation
activation| of the row for the norms (the norm is their root mean square).  The zero-producer-row records carry an e32 of their
own: their values and errors are 1e4 times the others', and one scalar over both would loosen the bound of every ordinary
record by that factor.
"""
import functools
import math

import torch

LRELU, PIXELNORM, DOT = 1, 2, 8
SLOPE, EPS = 0.2, 1e-8
LF_EINVAL, LF_EALIGN = -1, -2
LF_AMAX_FLOATS = 2048
PLAIN = 1 << 30                                                   # y_slice_channels of plain channels-last rows
F64, F32 = torch.float64, torch.float32


def pad16(v):
    return (v + 15) // 16 * 16


def cout_padded3(cout):
    """lf_conv3x3_cout_padded: 16, 32, then multiples of 64."""
    c = pad16(cout)
    return c if c <= 32 else (c + 63) // 64 * 64


def cout_padded1(cout):
    """lf_conv1x1_cout_padded: 16, 32, 64, then multiples of 128."""
    c = pad16(cout)
    return c if c <= 32 else 64 if c <= 64 else (c + 127) // 128 * 128


def pack3(w):
    """[Cout][Cin][k..] -> [tap][CoutP][CinP], tap = (kz*3 + ky)*3 + kx, zero padded (lf_conv3x3_fwd's wpack)."""
    cout, cin, taps = w.shape[0], w.shape[1], w[0, 0].numel()
    out = torch.zeros(taps, cout_padded3(cout), pad16(cin), dtype=F32)
    out[:, :cout, :cin] = w.reshape(cout, cin, taps).permute(2, 0, 1)
    return out


def pack3_t(w):
    """The data-gradient operator of the same layer: taps flipped, in / out swapped."""
    return pack3(w.transpose(0, 1).flip(dims=tuple(range(2, w.dim()))))


def pack1(w2d):
    """[Cout][K] -> [CoutP][Kp] (lf_conv1x1_fwd's wpack)."""
    cout, k = w2d.shape
    out = torch.zeros(cout_padded1(cout), pad16(k), dtype=F32)
    out[:cout, :k] = w2d
    return out


# ---- the dispatch, restated ------------------------------------------------------------------------------------------------------
def form3x3(dims, shape, cin, cout, fused=False, bias_aligned=True, cus=256, N=1, slope=SLOPE):
    """The kernel conv3x3_launch picks, as a name; ' +prev' for a fused-backward launch, ' whole row' where the PixelNorm' sum
    runs over 2 or 4 tiles, ' walk' where the persistent kernel does two or more tiles per workgroup.  (The persistent kernel
    writes LeakyReLU as max(u, slope u), so the dispatch asks for 0 < slope < 1; every case here runs at SLOPE.)"""
    D, H, W = shape
    nvox = D * H * W
    tail = ' +prev' if fused else ''
    if cin == 16 and cout == 16 and dims == 3 and nvox >= 4096 and nvox * 64 < 0x7fffffff and 0.0 < slope < 1.0 and bias_aligned:
        return 'conv3d_c16_persistent_kernel' + tail + (' walk' if persistent_tiles_per_workgroup(shape, N, cus) >= 2 else '')
    if pad16(cin) == 16 and cout_padded3(cout) == 16:
        return f'conv3x3_c16_kernel<{dims}>' + tail
    nt = min(4, cout_padded3(cout) // 16)
    return f'conv3x3_kernel<{dims},{nt}>' + tail + (' whole row' if fused and nt > 1 else '')


def persistent_tiles(shape, N):
    D, H, W = shape
    return -(-W // 16) * -(-H // 8) * -(-D // 4) * N


def persistent_tiles_per_workgroup(shape, N, cus):
    """conv3d_c16_persistent_kernel: min(tiles, CUs) workgroups, ceil(tiles / workgroups) consecutive tiles each."""
    t = persistent_tiles(shape, N)
    return -(-t // min(t, cus))


def walk_batch(cus, shape=(10, 19, 40), tiles_per_wg=3):
    """The smallest N at which every workgroup of the persistent kernel walks `tiles_per_wg` tiles of `shape`."""
    per_sample = persistent_tiles(shape, 1)
    N = 1
    while -(-per_sample * N // cus) < tiles_per_wg:
        N += 1
    return N


def nt1x1(cout, fused=False):
    """Output tiles per workgroup of conv1x1_launch."""
    ntiles = cout_padded1(cout) // 16
    return (4 if (fused and ntiles >= 16) else 8) if ntiles >= 8 else ntiles


def form1x1(K, cout, fused=False, dot=False, vec_out=True):
    nt = nt1x1(cout, fused)
    chunks = pad16(K) // 16
    name = f'conv1x1_kernel<{nt}>'
    if nt == 1:
        name += f' chunks {chunks // 4 * 4}+{chunks % 4}'
    if cout_padded1(cout) // 16 > nt:
        name += f' groups {cout_padded1(cout) // 16 // nt}'
    if K % 4:
        name += ' scalar loads'
    if not vec_out:
        name += ' scalar stores'
    return name + (' +dot' if dot else ' +prev' if fused else '')


def form_rows(mode, rows, C, aligned=True):
    """launch_rows<MODE> of csrc/pointwise.hip: the vector form for C / 4 a power of two <= 64 and 16-byte aligned arrays."""
    q = C // 4
    vec = C % 4 == 0 and q > 0 and (q & (q - 1)) == 0 and q <= 64 and aligned
    if vec:
        second = rows > 16384 * (256 // q)
        return f'rows_vec4_kernel<{mode}>' + (' second iteration' if second else '')
    return f'rows_wave_kernel<{mode}>' + (' second iteration' if rows > 16384 * 4 else '')


# ---- the restatement -------------------------------------------------------------------------------------------------------------
def conv_taps(x, w, dims, transposed=False, flip=True):
    """x [N][D][H][W][Ci], w [Co][Ci][k..] of the FORWARD layer, in x's dtype.  Forward: out[v][co] = sum_t x[v + t - 1] . w_t[co];
    transposed (x is the output gradient, Co channels): out[v][ci] = sum_t x[v - (t - 1)] . w_t[:, ci].  flip = False is the
    misreading 'taps not flipped'.  Zero padding 1 on the 3 (2) spatial axes."""
    N, D, H, W, _ = x.shape
    if dims == 2:
        w = w.unsqueeze(2)
    KZ, pz = w.shape[2], (1 if dims == 3 else 0)
    xp = x.new_zeros(N, D + 2 * pz, H + 2, W + 2, x.shape[-1])
    xp[:, pz:pz + D, 1:1 + H, 1:1 + W] = x
    out = x.new_zeros(N * D * H * W, w.shape[1] if transposed else w.shape[0])         # one row per voxel
    for kz in range(KZ):
        for ky in range(3):
            for kx in range(3):
                m = w[:, :, kz, ky, kx]
                sz, sy, sx = (KZ - 1 - kz, 2 - ky, 2 - kx) if (transposed and flip) else (kz, ky, kx)
                out.addmm_(xp[:, sz:sz + D, sy:sy + H, sx:sx + W].reshape(N * D * H * W, -1), m if transposed else m.t())
    return out.reshape(N, D, H, W, -1)


def epilogue(raw, bias, he, flags, coutp=None, misread=None):
    """raw [..., Cout] conv sums -> (y, r, v): the stored output, the norm (None without PixelNorm), the pre-normalisation
    activation."""
    if bias is None:
        v = raw * he
    elif misread == 'he_after_bias':
        v = (raw + bias) * he
    else:
        v = raw * he + bias
    if flags & LRELU:
        v = torch.where(v > 0, v, SLOPE * v)
    if not flags & PIXELNORM:
        return v, None, v
    div = coutp if misread == 'mean_over_coutp' else raw.shape[-1]
    r = torch.sqrt((v * v).sum(-1) / div + EPS)
    return v / r[..., None], r, v


def epilogue_bwd(g, yp, nrm, flags, rec=None, dot_rec=None, misread=None):
    """g, yp [..., C]; nrm [..., C / rec]: one norm per record of `rec` channels (default: the row); the PixelNorm' mean runs
    over `dot_rec` channels (default rec; another value is a misreading)."""
    C = g.shape[-1]
    rec = rec or C
    dot_rec = dot_rec or rec
    if flags & PIXELNORM:
        gd, yd = g.reshape(*g.shape[:-1], C // dot_rec, dot_rec), yp.reshape(*g.shape[:-1], C // dot_rec, dot_rec)
        dot = ((gd * yd).sum(-1, keepdim=True) / dot_rec).expand_as(gd).reshape(g.shape)
        g = (g - yp * dot) / nrm.repeat_interleave(rec, dim=-1)
    if flags & LRELU:
        g = torch.where((g if misread == 'lrelu_sign_of_grad' else yp) > 0, g, SLOPE * g)
    return g


def record_max(t, rec=None):
    """The largest |t| of every record of `rec` channels (default: the row), broadcast back to t's shape."""
    C = t.shape[-1]
    rec = rec or C
    return t.abs().reshape(*t.shape[:-1], C // rec, rec).amax(-1, keepdim=True).expand(*t.shape[:-1], C // rec, rec).reshape(t.shape)


def pw_in_index(N, P, cin, ksl, xbs, xss):
    """[N][P][K] flat offsets into xbuf, k = s*Cin + c (slice-major)."""
    n = torch.arange(N).reshape(N, 1, 1, 1)
    p = torch.arange(P).reshape(1, P, 1, 1)
    s = torch.arange(ksl).reshape(1, 1, ksl, 1)
    c = torch.arange(cin).reshape(1, 1, 1, cin)
    return (n * xbs + s * xss + p * cin + c).reshape(N, P, ksl * cin)


def pw_out_index(N, P, cout, ybs, yrs, ysc, yss, misread=None):
    """[N][P][Cout] flat offsets into ybuf.  misread 'channel_major': co = c * slices + slice instead of slice * ysc + c."""
    co = torch.arange(cout)
    if misread == 'channel_major' and ysc < cout:
        nsl = cout // ysc
        sl, ch = co % nsl, co // nsl
    else:
        sl, ch = co // ysc, co % ysc
    n = torch.arange(N).reshape(N, 1, 1)
    p = torch.arange(P).reshape(1, P, 1)
    return n * ybs + sl.reshape(1, 1, -1) * yss + p * yrs + ch.reshape(1, 1, -1)


def _gen(*parts):
    seed = 0
    for v in parts:
        for ch in repr(v):
            seed = (seed * 131 + ord(ch)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def _randn(gen, *shape):
    return torch.randn(*shape, generator=gen, dtype=F32)


def _pick(t, alone):
    return t if alone is None or t is None else t[alone:alone + 1]


def _e32(a32, a64, mask=None):
    """Largest |fp32 - fp64|; with a boolean `mask` (broadcastable) one value per class, laid out per element."""
    err = (a32.double() - a64).abs()
    if mask is None:
        return err.max()
    mask = mask.expand_as(err)
    zero = torch.zeros((), dtype=err.dtype)
    return torch.where(mask, torch.where(mask, err, zero).max(), torch.where(mask, zero, err).max())


def ratio(got, want, e32, scale):
    """max over the elements of |got - want| / max(4 e32, 2e-6 + 2e-5 scale); inf for a non-finite output."""
    got = got.double()
    if got.shape != want.shape or not bool(torch.isfinite(got).all()):
        return float('inf')
    bound = torch.maximum(4 * torch.as_tensor(e32, dtype=F64), 2e-6 + 2e-5 * scale)
    return float(((got - want).abs() / bound).max())


# ---- 3x3 layers ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=64)
def layer3(dims, cin, cout, shape, B=3):
    """One forward layer on a batch of B: x [B][D][H][W][Cin], w, bias, he, and the conv sums in fp64 and fp32 (shared by every
    flag set; read-only)."""
    gen = _gen('layer3', dims, cin, cout, shape, B)
    D, H, W = shape
    x = _randn(gen, B, D, H, W, cin)
    w = _randn(gen, cout, cin, *([3] * dims))
    b = 0.1 * _randn(gen, cout)
    he = math.sqrt(2.0 / (cin * 3 ** dims))
    return {'x': x, 'w': w, 'b': b, 'he': he, 'raw64': conv_taps(x.double(), w.double(), dims), 'raw32': conv_taps(x, w, dims)}


def fwd3_expected(desc, misread=None):
    """desc = ('fwd3', dims, cin, cout, shape, B, alone, flags, with_bias).  -> {'y', 'norm'}: (fp64, fp32, scale) each."""
    _, dims, cin, cout, shape, B, alone, flags, with_bias = desc
    L = layer3(dims, cin, cout, shape, B)
    if misread == 'hw_swapped':                                    # the same flat buffer read as [N][D][W][H][C]
        D, H, W = shape
        raw = conv_taps(L['x'].double().reshape(B, D, W, H, cin), L['w'].double(), dims).reshape(B, D, H, W, cout)
    else:
        raw = L['raw64']
    bias = L['b'] if with_bias else None
    y64, r64, v64 = epilogue(_pick(raw, alone), bias.double() if with_bias else None, L['he'], flags, cout_padded3(cout), misread)
    y32, r32, _ = epilogue(_pick(L['raw32'], alone), bias, L['he'], flags)
    out = {'y': (y64, y32, y64.abs())}
    if flags & PIXELNORM:
        out['norm'] = (r64, r32, v64.abs().amax(-1))
    return out


@functools.lru_cache(maxsize=64)
def grad3(dims, cc, cp, shape, B=3):
    """One data-gradient problem: the consumer layer w [Cc][Cp][k..] (forward Cp -> Cc), its output gradient gy
    [B][D][H][W][Cc], and the producer of its input: a pointwise layer x0 [..][8] -> Cp channels without bias, whose row at
    voxel `zero` (the middle voxel of sample 1, or of sample 0 when B = 1) is all zero."""
    gen = _gen('grad3', dims, cc, cp, shape, B)
    D, H, W = shape
    gy = _randn(gen, B, D, H, W, cc)
    w = _randn(gen, cc, cp, *([3] * dims))
    x0 = _randn(gen, B, D, H, W, 8)
    w0 = _randn(gen, cp, 8)
    zero = (min(1, B - 1),) + tuple(s // 2 for s in shape)
    x0[zero] = 0.0
    he = math.sqrt(2.0 / (cp * 3 ** dims))
    pre = (x0.double() @ w0.double().t()) * math.sqrt(2.0 / 8)
    prev = {}
    for pf in (LRELU, PIXELNORM, LRELU | PIXELNORM):
        y, r, _ = epilogue(pre, None, 1.0, pf)
        prev[pf] = (y.float(), None if r is None else r.float())
    zmask = torch.zeros(B, D, H, W, 1, dtype=torch.bool)
    zmask[zero] = True
    return {'gy': gy, 'w': w, 'he': he, 'prev': prev, 'zmask': zmask, 'x0': x0, 'w0': w0, 'b_prev': 0.1 * _randn(gen, cp),
            'raw64': conv_taps(gy.double(), w.double(), dims, transposed=True), 'raw32': conv_taps(gy, w, dims, transposed=True)}


def bwd3_expected(desc, misread=None):
    """desc = ('bwd3', dims, cc, cp, shape, B, alone, prev_flags); prev_flags = 0: the raw gradient.  -> {'gx'}."""
    _, dims, cc, cp, shape, B, alone, pf = desc
    G = grad3(dims, cc, cp, shape, B)
    raw = G['raw64']
    if misread == 'taps_not_flipped':
        raw = conv_taps(G['gy'].double(), G['w'].double(), dims, transposed=True, flip=False)
    g64, g32 = _pick(raw, alone) * G['he'], _pick(G['raw32'], alone) * G['he']
    if misread == 'bias_in_gradient':
        g64 = g64 + G['b_prev'].double()
    if pf == 0:
        return {'gx': (g64, g32, g64.abs(), None)}
    yp, nrm = (_pick(t, alone) for t in G['prev'][pf])
    n64 = n32 = None
    if nrm is not None:
        n64, n32 = nrm.double()[..., None], nrm[..., None]
        if misread == 'norm_by_record':                           # norm[(voxel * Cout + c) / 16] (wrapped to stay inside the array)
            flat = nrm.double().reshape(-1)
            idx = (torch.arange(flat.numel() * cp) // 16) % flat.numel()
            n64 = flat[idx].reshape(*nrm.shape, cp)[..., ::16]
    if misread == 'norm_by_record':
        want = epilogue_bwd(g64, yp.double(), n64, pf, rec=16, dot_rec=cp)
    else:
        want = epilogue_bwd(g64, yp.double(), n64, pf, dot_rec=16 if misread == 'pn_per_tile' else None, misread=misread)
    g32 = epilogue_bwd(g32, yp, n32, pf)
    return {'gx': (want, g32, record_max(want), _pick(G['zmask'], alone))}


# ---- pointwise convolutions ------------------------------------------------------------------------------------------------------
def pw_spec(P=65, cin=16, ksl=1, cout=16, flags=0, bias=True, xscale=False, x_slice_pad=0, x_batch_pad=0, row_gap=0,
            unfold=0, y_batch_pad=0, alone=None, want_norm=True):
    """A forward pointwise call as a hashable tuple of (name, value) pairs; addressing derived from the paddings:
    x [n][s][p][Cin] with x_slice_stride = P Cin + x_slice_pad, x_batch_stride = ksl x_slice_stride + x_batch_pad;
    plain rows of Cout + row_gap floats, or (unfold = D > 0: Cout = 16 D) D slices [p][16] of a channels-last volume."""
    return ('pw',) + tuple(sorted(locals().items()))


def pw_addr(spec):
    a = dict(spec[1:])
    xss = a['P'] * a['cin'] + a['x_slice_pad']
    xbs = a['ksl'] * xss + a['x_batch_pad']
    if a['unfold']:
        assert a['cout'] == 16 * a['unfold'] and not a['row_gap']
        yrs, ysc, yss = 16, 16, a['P'] * 16
        ybs = a['unfold'] * yss + a['y_batch_pad']
    else:
        yrs, ysc, yss = a['cout'] + a['row_gap'], PLAIN, 0
        ybs = a['P'] * yrs + a['y_batch_pad']
    a.update(xss=xss, xbs=xbs, yrs=yrs, ysc=ysc, yss=yss, ybs=ybs, K=a['ksl'] * a['cin'], B=3,
             xlen=3 * xbs, ylen=3 * ybs)
    return a


@functools.lru_cache(maxsize=256)
def _pw_layer(P, cin, ksl, cout, xss, xbs, xscale):
    """Inputs of a batch of 3 and the sums in fp64 / fp32 (shared by flags, bias and output addressing; read-only)."""
    gen = _gen('pw', P, cin, ksl, cout, xss, xbs, xscale)
    K = ksl * cin
    xbuf = _randn(gen, 3 * xbs)
    w = _randn(gen, cout, K)
    b = 0.1 * _randn(gen, cout)
    xs = (0.5 + torch.rand(3 * ksl * P, generator=gen, dtype=F32)) if xscale else None
    idx = pw_in_index(3, P, cin, ksl, xbs, xss)
    X = xbuf[idx]
    if xscale:                                                      # the product rounded to fp32, as the header states
        X = (X.reshape(3, P, ksl, cin) * xs.reshape(3, ksl, P).permute(0, 2, 1)[..., None]).reshape(3, P, K)
    return {'xbuf': xbuf, 'w': w, 'b': b, 'xs': xs, 'he': math.sqrt(2.0 / K), 'raw64': X.double() @ w.double().t(), 'raw32': X @ w.t()}


def pw_layer(spec):
    a = pw_addr(spec)
    return _pw_layer(a['P'], a['cin'], a['ksl'], a['cout'], a['xss'], a['xbs'], a['xscale'])


def pw_expected(spec, misread=None):
    """-> {'y': (fp64 [N][P][Cout], fp32, scale), 'norm': ...}, in (n, p, co) order: pw_out_index says where each lies."""
    a, L = pw_addr(spec), pw_layer(spec)
    alone = a['alone']
    bias = L['b'] if a['bias'] else None
    y64, r64, v64 = epilogue(_pick(L['raw64'], alone), bias.double() if a['bias'] else None, L['he'], a['flags'],
                             cout_padded1(a['cout']), misread)
    y32, r32, _ = epilogue(_pick(L['raw32'], alone), bias, L['he'], a['flags'])
    if misread == 'channel_major':                                  # what lies where the true layout looks, had the kernel written so
        n = y64.shape[0]
        wrong = pw_out_index(n, a['P'], a['cout'], a['ybs'], a['yrs'], a['ysc'], a['yss'], misread)
        true = pw_out_index(n, a['P'], a['cout'], a['ybs'], a['yrs'], a['ysc'], a['yss'])
        flat = torch.zeros(n * a['ybs'], dtype=F64)
        flat[wrong.reshape(-1)] = y64.reshape(-1)
        y64 = flat[true]
    out = {'y': (y64, y32, y64.abs())}
    if a['flags'] & PIXELNORM:
        out['norm'] = (r64, r32, v64.abs().amax(-1))
    return out


def pwb_spec(P=65, cg=16, unfold=5, prev_flags=0, y_batch_pad=0, alone=None, store=True):
    """A pointwise data-gradient call into an unfolded volume: gy [3][P][cg] -> gx [n][d][p][16], d < unfold (Cout = 16 D),
    prev_flags 0 (raw), LRELU / PIXELNORM / both (16-channel records, the norm per record) or DOT (store = False: y NULL)."""
    return ('pwb',) + tuple(sorted(locals().items()))


def pwb_addr(spec):
    a = dict(spec[1:])
    a.update(cout=16 * a['unfold'], yrs=16, ysc=16, yss=a['P'] * 16)
    a['ybs'] = a['unfold'] * a['yss'] + a['y_batch_pad']
    a['ylen'] = 3 * a['ybs']
    return a


@functools.lru_cache(maxsize=128)
def _pwb_layer(P, cg, unfold, y_batch_pad):
    """The projection w [cg][K = 16 D] (k = d * 16 + c), its output gradient gy [3][P][cg] and the producer of its input volume:
    pointwise x0 [3][D][P][8] -> 16 channels per voxel; the voxel (sample 1, slice D / 2, pixel P / 2) has an all-zero row.
    prev buffers are laid out as the gradient is (batch stride padded alike): prev_y[offset], prev_norm[offset / 16]."""
    gen = _gen('pwb', P, cg, unfold, y_batch_pad)
    D = unfold
    gy = _randn(gen, 3, P, cg)
    w = _randn(gen, cg, 16 * D)
    x0 = _randn(gen, 3, D, P, 8)
    w0 = _randn(gen, 16, 8)
    x0[1, D // 2, P // 2] = 0.0
    pre = (x0.double() @ w0.double().t()) * math.sqrt(2.0 / 8)      # [3][D][P][16]
    prev = {}
    for pf in (LRELU, PIXELNORM, LRELU | PIXELNORM):
        y, r, _ = epilogue(pre, None, 1.0, pf)
        prev[pf] = (y.float(), None if r is None else r.float())
    prev[DOT] = (prev[LRELU | PIXELNORM][0], None)
    zmask = torch.zeros(3, D, P, 1, dtype=torch.bool)
    zmask[1, D // 2, P // 2] = True
    return {'gy': gy, 'w': w, 'he': math.sqrt(2.0 / (16 * D)), 'prev': prev, 'zmask': zmask, 'x0': x0, 'w0': w0,
            'raw64': gy.double() @ w.double(), 'raw32': gy @ w}


def pwb_layer(spec):
    a = pwb_addr(spec)
    return _pwb_layer(a['P'], a['cg'], a['unfold'], a['y_batch_pad'])


def pwb_expected(spec, misread=None):
    """-> {'gx': (fp64 [N][D][P][16], fp32, scale, zero-row mask)[, 'dot': ([N][D][P], ...)]} in volume order."""
    a, G = pwb_addr(spec), pwb_layer(spec)
    D, P, alone, pf = a['unfold'], a['P'], a['alone'], a['prev_flags']

    def vol(raw):                                                   # [n][P][D*16] -> [n][D][P][16]
        raw = _pick(raw, alone)
        return raw.reshape(raw.shape[0], P, D, 16).permute(0, 2, 1, 3)
    g64, g32 = vol(G['raw64']) * G['he'], vol(G['raw32']) * G['he']
    if pf == 0:
        return {'gx': (g64, g32, g64.abs(), None)}
    yp, nrm = (_pick(t, alone) for t in G['prev'][pf])
    zmask = _pick(G['zmask'], alone)
    if pf == DOT:
        d64, d32 = (g64 * yp.double()).sum(-1), (g32 * yp).sum(-1)
        return {'gx': (g64, g32, g64.abs(), None), 'dot': (d64, d32, (g64 * yp.double()).abs().amax(-1), zmask[..., 0])}
    n64 = n32 = None
    if nrm is not None:
        n64, n32 = nrm.double()[..., None], nrm[..., None]
        if misread == 'norm_by_row':                                # norm[n * P + p] of the same array
            flat = nrm.double().reshape(-1)
            n_ = torch.arange(nrm.shape[0]).reshape(-1, 1, 1)
            n64 = flat[(n_ * P + torch.arange(P).reshape(1, 1, P)).expand(nrm.shape)][..., None]
    if misread == 'pn_whole_row':                                   # the mean over the pixel's D * 16 channels
        rows = lambda t: t.permute(0, 2, 1, 3).reshape(t.shape[0], P, D * 16)   # noqa: E731
        want = epilogue_bwd(rows(g64), rows(yp.double()), n64[..., 0].permute(0, 2, 1), pf, rec=16, dot_rec=16 * D)
        want = want.reshape(-1, P, D, 16).permute(0, 2, 1, 3)
    else:
        want = epilogue_bwd(g64, yp.double(), n64, pf, misread=misread)
    return {'gx': (want, epilogue_bwd(g32, yp, n32, pf), record_max(want), zmask)}


# ---- row kernels -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=8)
def rows_inputs(rows, C):
    """x, gy [rows][C] fp32; row min(1, rows - 1) of x is all zero."""
    gen = _gen('rows', rows, C)
    x = _randn(gen, rows, C)
    x[min(1, rows - 1)] = 0.0
    return x, _randn(gen, rows, C)


def rows_prev(x, flags):
    """The saved output and norm (None without PixelNorm) of a layer with pre-activation x and epilogue `flags`: fp64, rounded."""
    y, r, _ = epilogue(x.double(), None, 1.0, flags)
    return y.float(), None if r is None else r.float()


def pixelnorm_expected(x, misread=None):
    """-> {'y', 'norm'}: (fp64, fp32, scale)."""
    def go(t):
        C = t.shape[-1]
        r = torch.sqrt((t * t).sum(-1) / (16 if (misread == 'mean_over_16' and t.dtype == F64) else C) + EPS)
        return t / r[..., None], r
    y64, r64 = go(x.double())
    y32, r32 = go(x)
    return {'y': (y64, y32, y64.abs()), 'norm': (r64, r32, x.double().abs().amax(-1))}


def rows_bwd_expected(gy, y, norm, flags, misread=None):
    """y, norm: the fp32 arrays the kernel is given.  -> {'gp': (fp64, fp32, scale, zero-row mask)}."""
    n64 = None if norm is None else norm.double()[..., None]
    if misread == 'norm_squared' and n64 is not None:
        n64 = n64 * n64
    want = epilogue_bwd(gy.double(), y.double(), n64, flags)
    g32 = epilogue_bwd(gy, y, None if norm is None else norm[..., None], flags)
    return {'gp': (want, g32, record_max(want), (y == 0).all(-1, keepdim=True))}


def ratios(expected, got):
    """{output: (err, e32, err / bound)} for the outputs present in `got`; e32 is always taken against expected's own fp64
    -- pass e32_from (the true expectation) through `with_true_e32` when `expected` is a misreading."""
    out = {}
    for k, g in got.items():
        want, a32, scale = expected[k][:3]
        mask = expected[k][3] if len(expected[k]) > 3 else None
        e32 = expected[k][4] if len(expected[k]) > 4 else _e32(a32, want, mask)
        out[k] = (float((g.double() - want).abs().max()) if g.shape == want.shape else float('inf'), float(torch.as_tensor(e32).max()),
                  ratio(g, want, e32, scale))
    return out


def with_true_e32(wrong, true):
    """A misread expectation carrying the TRUE expectation's e32 (a property of the inputs, not of the reference compared with)."""
    out = {}
    for k, v in wrong.items():
        t = true[k]
        mask = t[3] if len(t) > 3 else None
        out[k] = (v[0], v[1], v[2], mask, _e32(t[1], t[0], mask))
    return out


def stand_in(expected):
    """The fp32 chain's outputs, standing in for the kernel where there is no GPU."""
    return {k: v[1] for k, v in expected.items()}


# ---- the cases -------------------------------------------------------------------------------------------------------------------
FLAGSETS = (0, LRELU, PIXELNORM, LRELU | PIXELNORM)
PREV_FLAGS = (LRELU, PIXELNORM, LRELU | PIXELNORM)

C16_CHANNELS = [(16, 16), (5, 3), (12, 16), (16, 7)]
C16_SHAPES_3D = [(1, 1, 1), (4, 4, 16), (5, 6, 17), (2, 3, 33), (5, 9, 91)]
C16_SHAPES_2D = [(1, 1, 1), (1, 16, 16), (1, 17, 18), (1, 3, 33)]
GENERIC_CHANNELS = [(35, 16), (32, 10), (16, 32), (19, 24), (64, 64), (8, 48), (72, 132), (20, 66)]
GENERIC_SHAPES = {3: [(5, 6, 17), (1, 1, 1)], 2: [(1, 17, 18), (1, 1, 1)]}
# fused backward: (gy channels, producer channels = the launch's Cout)
FUSED_CHANNELS = [(16, 16), (40, 16), (16, 32), (24, 64)]
FUSED_SHAPES = {3: [(5, 6, 17), (1, 1, 1)], 2: [(1, 17, 18), (1, 1, 1)]}
PERSISTENT_SHAPES = [(8, 16, 32), (10, 19, 40), (4, 8, 128)]
WALK_SHAPE = (10, 19, 40)


def layers3():
    """(dims, cin, cout, shape) of every forward 3x3 layer outside the persistent kernel."""
    keys = []
    for cin, cout in C16_CHANNELS:
        keys += [(3, cin, cout, s) for s in C16_SHAPES_3D] + [(2, cin, cout, s) for s in C16_SHAPES_2D]
    for cin, cout in GENERIC_CHANNELS:
        for dims in (3, 2):
            keys += [(dims, cin, cout, s) for s in GENERIC_SHAPES[dims]]
    return keys


def fwd3_variants(cout):
    """(flags, with_bias, want_norm) of a forward layer: PixelNorm up to 64 channels; norm_out NULL with PixelNorm set."""
    out = []
    for flags in (FLAGSETS if cout <= 64 else (0, LRELU)):
        for with_bias in (True, False):
            out.append((flags, with_bias, True))
        if flags & PIXELNORM:
            out.append((flags, True, False))
    return out


def grads3():
    """(dims, cc, cp, shape) of every data-gradient problem outside the persistent kernel."""
    return [(dims, cc, cp, s) for cc, cp in FUSED_CHANNELS for dims in (3, 2) for s in FUSED_SHAPES[dims]]


PW_P = (1, 15, 63, 64, 65, 130)
# (Cin = K, Cout, PixelNorm allowed)
PW_CHANNELS = [(4, 16, True), (35, 16, True), (64, 16, True), (100, 16, True), (2048, 16, True),
               (20, 24, True), (20, 48, True), (20, 64, True), (20, 128, True), (20, 200, False), (20, 2, True)]
PW_UNFOLD = (1, 5, 16, 20)


def pw_form(spec):
    a = pw_addr(spec) if spec[0] == 'pw' else pwb_addr(spec)
    if spec[0] == 'pwb':
        pf = a['prev_flags']
        return form1x1(a['cg'], a['cout'], fused=pf != 0, dot=pf == DOT)
    vec_out = ((a['yrs'] | a['ysc']) & 3) == 0 and ((a['ybs'] | a['yss']) & 3) == 0
    return form1x1(a['K'], a['cout'], vec_out=vec_out)


def pw_specs():
    """Every forward pointwise case (batch of 3; the tests also run sample 1 alone)."""
    specs = []
    for P in PW_P:
        for cin, cout, pn in PW_CHANNELS:
            for flags in (FLAGSETS if pn else (0, LRELU)):
                for bias in (True, False):
                    specs.append(pw_spec(P=P, cin=cin, cout=cout, flags=flags, bias=bias))
            if pn:
                specs.append(pw_spec(P=P, cin=cin, cout=cout, flags=PIXELNORM | LRELU, want_norm=False))
        for ksl in (3, 16):                                         # folded depth, with and without the per-pixel factor
            for sp, bp in ((0, 0), (32, 0), (0, 64), (32, 64)):
                for xs in (False, True):
                    specs.append(pw_spec(P=P, cin=16, ksl=ksl, cout=16, flags=LRELU | PIXELNORM, xscale=xs, x_slice_pad=sp, x_batch_pad=bp))
        for gap in (4, 1):                                          # a row stride wider than Cout
            for cout in (16, 24):
                specs.append(pw_spec(P=P, cin=20, cout=cout, flags=LRELU | PIXELNORM, row_gap=gap))
        for D in PW_UNFOLD:                                         # unfolded into D slices; a padded batch stride
            for pad in (0, 48):
                specs.append(pw_spec(P=P, cin=16, cout=16 * D, flags=0, bias=False, unfold=D, y_batch_pad=pad))
        specs.append(pw_spec(P=P, cin=20, cout=24, flags=LRELU, y_batch_pad=8))
    return specs


def pwb_specs():
    specs = []
    for P in PW_P:
        for D in PW_UNFOLD:
            for pf in (0,) + PREV_FLAGS + (DOT,):
                specs.append(pwb_spec(P=P, unfold=D, prev_flags=pf))
            specs.append(pwb_spec(P=P, unfold=D, prev_flags=DOT, store=False))
            specs.append(pwb_spec(P=P, unfold=D, prev_flags=LRELU | PIXELNORM, y_batch_pad=48))
    return specs


ROWS_VEC_C = (4, 8, 16, 64, 256)
ROWS_WAVE_C = (1, 2, 3, 7, 12, 17, 65, 200, 512, 2048)
ROWS_COUNTS = (1, 3, 63, 65, 1027)
ROWS_LARGE = [(65536 + 5, 256), (65536 + 3, 3)]                   # the second grid-stride iteration of either form


def forms_reached(cus=256):
    """{form name} over every case above (the walk case at the batch a device of `cus` CUs needs)."""
    out = set()
    for dims, cin, cout, shape in layers3():
        out.add(form3x3(dims, shape, cin, cout))
    for dims, cc, cp, shape in grads3():
        out.add(form3x3(dims, shape, cc, cp))
        out.add(form3x3(dims, shape, cc, cp, fused=True))
    for shape in PERSISTENT_SHAPES:
        for N in (1, 3):
            out.add(form3x3(3, shape, 16, 16, N=N, cus=cus))
            out.add(form3x3(3, shape, 16, 16, fused=True, N=N, cus=cus))
    N = walk_batch(cus)
    out.add(form3x3(3, WALK_SHAPE, 16, 16, N=N, cus=cus))
    out.add(form3x3(3, WALK_SHAPE, 16, 16, fused=True, N=N, cus=cus))
    out.add(form3x3(3, (10, 19, 40), 16, 16, bias_aligned=False) + ' (misaligned bias)')
    for spec in pw_specs() + pwb_specs():
        out.add(pw_form(spec))
    for mode in (0, 1):
        for C in ROWS_VEC_C + ROWS_WAVE_C:
            out.add(form_rows(mode, 65, C))
        for rows, C in ROWS_LARGE:
            out.add(form_rows(mode, rows, C))
        out.add(form_rows(mode, 65, 16, aligned=False) + ' (misaligned)')
    return out


REQUIRED_FORMS = (
    ['conv3x3_c16_kernel<3>', 'conv3x3_c16_kernel<2>', 'conv3x3_c16_kernel<3> +prev', 'conv3x3_c16_kernel<2> +prev',
     'conv3d_c16_persistent_kernel', 'conv3d_c16_persistent_kernel +prev', 'conv3d_c16_persistent_kernel walk',
     'conv3d_c16_persistent_kernel +prev walk', 'conv3x3_c16_kernel<3> (misaligned bias)']
    + [f'conv3x3_kernel<{d},{nt}>' for d in (2, 3) for nt in (1, 2, 4)]
    + [f'conv3x3_kernel<{d},1> +prev' for d in (2, 3)]
    + [f'conv3x3_kernel<{d},{nt}> +prev whole row' for d in (2, 3) for nt in (2, 4)]
    + ['conv1x1_kernel<1> chunks 0+1', 'conv1x1_kernel<1> chunks 0+3 scalar loads', 'conv1x1_kernel<1> chunks 4+0',
       'conv1x1_kernel<1> chunks 4+3', 'conv1x1_kernel<1> chunks 128+0', 'conv1x1_kernel<2>', 'conv1x1_kernel<4>',
       'conv1x1_kernel<8>', 'conv1x1_kernel<8> groups 2', 'conv1x1_kernel<1> chunks 0+2 scalar stores',
       'conv1x1_kernel<1> chunks 0+1 +prev', 'conv1x1_kernel<8> +prev', 'conv1x1_kernel<4> groups 4 +prev',
       'conv1x1_kernel<4> groups 6 +prev', 'conv1x1_kernel<1> chunks 0+1 +dot', 'conv1x1_kernel<4> groups 4 +dot']
    + [f'rows_{k}_kernel<{m}>{s}' for k in ('vec4', 'wave') for m in (0, 1) for s in ('', ' second iteration')]
    + [f'rows_wave_kernel<{m}> (misaligned)' for m in (0, 1)])


# ---- misreadings: name -> (the case that reaches the form it is about, the output compared) ---------------------------------------
MISREADINGS = {
    'mean_over_coutp/8of16': (('fwd3', 3, 16, 8, (5, 6, 17), 3, None, LRELU | PIXELNORM, True), 'y'),
    'mean_over_coutp/48of64': (('fwd3', 2, 8, 48, (1, 17, 18), 3, None, LRELU | PIXELNORM, True), 'y'),
    'he_after_bias': (('fwd3', 3, 16, 16, (5, 6, 17), 3, None, 0, True), 'y'),
    'hw_swapped': (('fwd3', 3, 16, 16, (5, 6, 17), 3, None, 0, True), 'y'),
    'lrelu_sign_of_grad': (('bwd3', 3, 16, 16, (5, 6, 17), 3, None, LRELU), 'gx'),
    'pn_per_tile': (('bwd3', 2, 16, 32, (1, 17, 18), 3, None, PIXELNORM), 'gx'),
    'pn_whole_row': (pwb_spec(P=65, unfold=5, prev_flags=PIXELNORM), 'gx'),
    'taps_not_flipped': (('bwd3', 3, 16, 16, (5, 6, 17), 3, None, 0), 'gx'),
    'norm_by_record': (('bwd3', 3, 24, 64, (5, 6, 17), 3, None, LRELU | PIXELNORM), 'gx'),
    'norm_by_row': (pwb_spec(P=65, unfold=5, prev_flags=LRELU | PIXELNORM), 'gx'),
    'bias_in_gradient': (('bwd3', 3, 16, 16, (5, 6, 17), 3, None, 0), 'gx'),
    'channel_major': (pw_spec(P=65, cin=16, cout=80, flags=0, bias=False, unfold=5), 'y'),
}


def expected(desc, misread=None):
    misread = misread.split('/')[0] if misread else None
    return {'fwd3': fwd3_expected, 'bwd3': bwd3_expected, 'pw': pw_expected, 'pwb': pwb_expected}[desc[0]](desc, misread)


def misread_ratio(name, got):
    """How far `got` (the outputs of the misreading's case) is from the misread reference, in units of the bound that accepts
    it against the true one."""
    desc, key = MISREADINGS[name]
    wrong = with_true_e32(expected(desc, name), expected(desc))
    return ratios(wrong, {key: got[key]})[key][2]
