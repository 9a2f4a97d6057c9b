"""The wide weight gradient (lf_conv_bwd_weight_wide, csrc/wgrad_wide.hip) against a plain fp64 reference: every convolution
of the released architecture whose weight gradient it serves, at reduced batch and extent, plus a ragged extent, a problem
smaller than one voxel tile and one with the full 512 partial runs per output.

Reference: gw[tap][co][ci] = scale * sum_v gp[v][co] * x[v + tap][ci], written as an explicit per-tap sum over shifted views
of the zero-padded input, in fp64 on the CPU from the fp32 operands the kernel sees.

Metric (copied from tests/test_train_layers_fp64_gpu.py): e = |got - ref| / (|ref| + rms(ref)) per element; max(e) <= tau and
frac(e > 2^-8) <= f_max.  Each case also asserts that the bound rejects four wrong fp64 references (a transposed gw, the
flipped tap order, the last z-plane / row of x dropped, the last ragged Cin chunk zeroed) and, without any calibration, that
max(e) <= 2x the max(e) of lf_conv_bwd_weight on the same inputs.

Bounds: tau calibrated once on an MI355X as 2x the largest observed max(e), rounded up to a power of two; f_max = 0 (no
element above 2^-8 was seen).  Observed over the cases below: max(e) 1.05e-06 (wide, the 512-run case; 2.0e-07 - 5.9e-07
elsewhere), 1.19e-06 (lf_conv_bwd_weight)."""
import ctypes
import zlib

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ULP = 2.0 ** -8
TAU = 2.0 ** -18
FMAX = 0.0
LF_EINVAL, LF_EALIGN, LF_ENOSPC = -1, -2, -3


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def rel_err(got, ref):
    """e = |got - ref| / (|ref| + rms(ref)) per element (0 / 0 counts as 0, x / 0 as inf)."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    diff = (got - ref).abs()
    den = ref.abs() + ref.pow(2).mean().sqrt()
    return torch.where(den > 0, diff / den.clamp_min(1e-300), torch.where(diff > 0, float('inf'), 0.0))


def check(name, got, ref, bound, wrong=()):
    """Asserts max(e) <= tau and frac(e > 2^-8) <= f_max for the device result `got` against the fp64 reference, and that
    the same bound REJECTS `got` against every deliberately wrong reference in `wrong` ((label, tensor) pairs)."""
    tau, fmax = bound
    e = rel_err(got, ref)
    m, f = e.max().item(), (e > ULP).double().mean().item()
    assert m <= tau and f <= fmax, f'{name}: max e {m:.3g} (tau {tau:.3g}), frac(e > 2^-8) {f:.3g} (f_max {fmax:.3g})'
    for label, wref in wrong:
        ew = rel_err(got, wref)
        mw, fw = ew.max().item(), (ew > ULP).double().mean().item()
        assert mw > tau or fw > fmax, f'{name}: the bound does not reject the wrong reference "{label}" (max e {mw:.3g})'
    return m, f


def released_shapes():
    """(dims, Cin, Cout, k) of every convolution of build_released_model whose weight gradient ops_train routes to the wide
    kernel (Cin, Cout >= 64), found by walking the modules; k = 1 layers are pointwise (dims 0)."""
    from latentfusion_amd import synth
    from latentfusion_amd.recon import fusion
    from latentfusion_amd.recon.models import Photographer, Sculptor
    out = set()
    for mod in (Sculptor(**synth.RELEASED_SCULPTOR), fusion.get_fuser('gru', 256, 1.0), Photographer(**synth.RELEASED_PHOTOGRAPHER)):
        for name, p in mod.named_parameters():
            if not name.endswith('weight') or p.dim() not in (4, 5):
                continue
            cout, cin, k = p.shape[0], p.shape[1], p.shape[2]
            if cin >= 64 and cout >= 64:
                out.add((0 if k == 1 else p.dim() - 2, cin, cout, k))
    return sorted(out)


SHAPES = released_shapes()
EXTENT = {3: (1, 5, 6, 7), 2: (2, 1, 9, 13), 0: (1, 1, 1, 300)}       # (N, D, H, W); dims 0: rows = N*D*H*W
EXTRA = [
    ('ragged', 3, (2, 3, 5, 19), 259, 67),        # extent not a multiple of the 4 x 16 tile, Cin / Cout not multiples of 4
    ('subtile', 2, (1, 1, 2, 3), 96, 80),         # fewer voxels than one tile
    ('subtile0', 0, (1, 1, 1, 7), 515, 64),
    ('multirun', 0, (1, 1, 1, 524283), 64, 96),   # 8192 tiles -> 512 partial runs per output (2x the MI355X's 256 CUs)
]
CASES = [(f'd{d}_{ci}x{co}', d, EXTENT[d], ci, co) for d, ci, co, _ in SHAPES] + EXTRA


def _operands(dims, ext, cin, cout, key):
    g = torch.Generator().manual_seed(_seed(*key))
    N, D, H, W = ext
    if dims == 0:
        rows = N * D * H * W
        x, gp = torch.randn(rows, cin, generator=g), torch.randn(rows, cout, generator=g)
        return x, gp, x.to(DEV), gp.to(DEV)
    sp = (D, H, W) if dims == 3 else (H, W)
    mf = torch.channels_last_3d if dims == 3 else torch.channels_last
    x, gp = torch.randn((N, cin) + sp, generator=g), torch.randn((N, cout) + sp, generator=g)
    return x, gp, x.to(DEV).contiguous(memory_format=mf), gp.to(DEV).contiguous(memory_format=mf)


def ref_wgrad(x, gp, dims, scale):
    """fp64: gw[tap][co][ci] = scale * sum_v gp[v][co] * x[v + tap][ci], one explicit sum per tap over a shifted view of the
    zero-padded input.  x (N, Cin, [D,] H, W) / gp (N, Cout, ...), or [rows][C] matrices for dims 0."""
    x, gp = x.double(), gp.double()
    if dims == 0:
        return (scale * gp.t() @ x).unsqueeze(0)
    sp = x.shape[2:]
    xp = torch.nn.functional.pad(x, (1, 1) * len(sp))
    offs = [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)] if dims == 3 else \
        [(0, dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
    taps = []
    for dz, dy, dx in offs:
        if dims == 3:
            D, H, W = sp
            xs = xp[:, :, 1 + dz:1 + dz + D, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
        else:
            H, W = sp
            xs = xp[:, :, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
        taps.append(scale * torch.einsum('nk...,nc...->kc', gp, xs))
    return torch.stack(taps)


def _run(entry, x_dev, gp_dev, dims, ext, cin, cout, scale, scratch_fn):
    from latentfusion_amd import _lib
    L = _lib.lib()
    N, D, H, W = ext
    taps = {0: 1, 2: 9, 3: 27}[dims]
    nb = getattr(L, scratch_fn)(dims, N, D, H, W, cin, cout)
    assert nb > 0
    scr = torch.empty(nb // 4 + 4, device=DEV, dtype=torch.float32)
    gw = torch.empty(taps, cout, cin, device=DEV, dtype=torch.float32)
    rc = getattr(L, entry)(x_dev.data_ptr(), gp_dev.data_ptr(), gw.data_ptr(), scr.data_ptr(), scr.numel() * 4, dims, N, D, H, W,
                           cin, cout, ctypes.c_float(scale), None)
    assert rc == 0, (entry, rc)
    torch.cuda.synchronize()
    return gw


def wide(x_dev, gp_dev, dims, ext, cin, cout, scale):
    return _run('lf_conv_bwd_weight_wide', x_dev, gp_dev, dims, ext, cin, cout, scale, 'lf_conv_bwd_weight_wide_scratch_bytes')


def generic(x_dev, gp_dev, dims, ext, cin, cout, scale):
    return _run('lf_conv_bwd_weight', x_dev, gp_dev, dims, ext, cin, cout, scale, 'lf_conv_bwd_weight_scratch_bytes')


def test_shape_table_is_the_released_architecture():
    # 3-D camera blocks and encoder volume, 515 -> 256 ConvGRU gates, wide 2-D levels, K = 4096 factor projection
    assert (3, 256, 256, 3) in SHAPES and (3, 515, 256, 3) in SHAPES
    assert (2, 512, 512, 3) in SHAPES and (2, 1024, 512, 3) in SHAPES and (0, 4096, 256, 1) in SHAPES
    assert all(ci >= 64 and co >= 64 for _, ci, co, _ in SHAPES) and len(SHAPES) >= 15


@pytest.mark.parametrize('name,dims,ext,cin,cout', CASES, ids=[c[0] for c in CASES])
def test_wide_wgrad_against_fp64(name, dims, ext, cin, cout):
    scale = 0.0417
    x, gp, xd, gd = _operands(dims, ext, cin, cout, name)
    got = wide(xd, gd, dims, ext, cin, cout, scale)
    ref = ref_wgrad(x, gp, dims, scale)
    wrong = [('transposed gw', ref.transpose(1, 2).reshape(ref.shape))]
    if dims != 0:
        wrong.append(('convolution tap order', ref.flip(0)))
    xd_ = x.clone()
    if dims == 0:
        xd_[-1] = 0
    else:
        xd_[:, :, -1] = 0                                             # last z-plane (3-D) / row (2-D) of x dropped
    wrong.append(('halo: last plane / row dropped', ref_wgrad(xd_, gp, dims, scale)))
    xc = x.clone()
    xc[:, (cin - 1) // 64 * 64:] = 0
    wrong.append(('last Cin chunk zeroed', ref_wgrad(xc, gp, dims, scale)))
    m, _ = check(name, got, ref, (TAU, FMAX), wrong)
    m_gen = rel_err(generic(xd, gd, dims, ext, cin, cout, scale), ref).max().item()
    print(f'{name}: max e wide {m:.3g}, lf_conv_bwd_weight {m_gen:.3g}')
    assert m <= 2 * max(m_gen, 2.0 ** -24), (name, m, m_gen)


def test_wide_wgrad_is_deterministic():
    for name, dims, ext, cin, cout in (EXTRA[3], ('d3_mid', 3, (2, 12, 16, 16), 256, 256)):
        _, _, xd, gd = _operands(dims, ext, cin, cout, name)
        a = wide(xd, gd, dims, ext, cin, cout, 1.0)
        b = wide(xd, gd, dims, ext, cin, cout, 1.0)
        assert torch.equal(a, b), name


def test_wide_wgrad_abi_errors():
    from latentfusion_amd import _lib
    L = _lib.lib()
    dims, N, D, H, W, cin, cout = 3, 1, 4, 4, 4, 64, 64
    x = torch.randn(N * D * H * W * cin + 8, device=DEV)
    gp = torch.randn(N * D * H * W * cout + 8, device=DEV)
    nb = L.lf_conv_bwd_weight_wide_scratch_bytes(dims, N, D, H, W, cin, cout)
    scr = torch.empty(nb // 4 + 8, device=DEV)
    gw = torch.full((27 * cout * cin + 8,), 12345.0, device=DEV)
    p, q, s, o = x.data_ptr(), gp.data_ptr(), scr.data_ptr(), gw.data_ptr()
    f = ctypes.c_float(1.0)

    def call(xp, gpp, gwp, sp, sb, *shape):
        return L.lf_conv_bwd_weight_wide(xp, gpp, gwp, sp, sb, *(shape or (dims, N, D, H, W, cin, cout)), f, None)
    assert call(None, q, o, s, nb) == LF_EINVAL                       # x == NULL: the bias stays on lf_conv_bwd_weight
    assert call(p, None, o, s, nb) == LF_EINVAL
    assert call(p, q, None, s, nb) == LF_EINVAL
    assert call(p, q, o, None, nb) == LF_EINVAL
    assert call(p + 4, q, o, s, nb) == LF_EALIGN
    assert call(p, q + 4, o, s, nb) == LF_EALIGN
    assert call(p, q, o + 4, s, nb) == LF_EALIGN
    assert call(p, q, o, s, nb - 4) == LF_ENOSPC
    assert call(p, q, o, s, nb, dims, N, D, H, W, 15, cout) == LF_EINVAL
    assert call(p, q, o, s, nb, dims, N, D, H, W, cin, 8) == LF_EINVAL
    assert call(p, q, o, s, nb, 1, N, D, H, W, cin, cout) == LF_EINVAL
    assert call(p, q, o, s, nb, dims, 0, D, H, W, cin, cout) == LF_EINVAL
    assert L.lf_conv_bwd_weight_wide_scratch_bytes(dims, N, D, H, W, 15, cout) == 0
    torch.cuda.synchronize()
    assert bool((gw == 12345.0).all()), 'an error return wrote to gw'


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last_3d if t.dim() == 5 else torch.channels_last)


@pytest.fixture
def wide_switch():
    from latentfusion_amd import _lib, ops_train
    saved = ops_train.WIDE_WGRAD
    yield ops_train
    ops_train.WIDE_WGRAD = saved
    _lib.BYTE_LOG = None


def test_routing(wide_switch):
    from latentfusion_amd import _lib
    T = wide_switch
    g = torch.Generator().manual_seed(3)
    x = _cl(torch.randn(2, 256, 6, 5, 7, generator=g).to(DEV))
    gp = _cl(torch.randn(2, 128, 6, 5, 7, generator=g).to(DEV))
    T.WIDE_WGRAD = True
    _lib.BYTE_LOG = {}
    gw_w, _ = T.conv_bwd_weight(x, gp, 3, 256, 0.5, want_bias=False)
    log = dict(_lib.BYTE_LOG)
    assert log.get('lf_conv_bwd_weight_wide', [0])[0] == 1 and 'lf_conv_bwd_weight' not in log, log
    _lib.BYTE_LOG = {}
    _, gb = T.conv_bwd_weight(x, gp, 3, 256, 0.5, want_bias=True)
    log = dict(_lib.BYTE_LOG)
    assert log['lf_conv_bwd_weight_wide'][0] == 1 and log['lf_conv_bwd_weight'][0] == 1 and gb.shape == (128,), log   # bias only
    # a 16-channel layer (SYN) keeps its kernels
    x16 = _cl(torch.randn(2, 16, 9, 11, generator=g).to(DEV))
    gp16 = _cl(torch.randn(2, 16, 9, 11, generator=g).to(DEV))
    _lib.BYTE_LOG = {}
    T.conv_bwd_weight(x16, gp16, 2, 16, 0.5, want_bias=False)
    x64 = _cl(torch.randn(2, 64, 9, 11, generator=g).to(DEV))
    T.conv_bwd_weight(x64, gp16, 2, 64, 0.5, want_bias=False)
    log = dict(_lib.BYTE_LOG)
    assert 'lf_conv_bwd_weight_wide' not in log and log['lf_conv_bwd_weight'][0] == 2, log
    # switched off: the generic kernel
    T.WIDE_WGRAD = False
    _lib.BYTE_LOG = {}
    gw_g, _ = T.conv_bwd_weight(x, gp, 3, 256, 0.5, want_bias=False)
    log = dict(_lib.BYTE_LOG)
    assert 'lf_conv_bwd_weight_wide' not in log and log['lf_conv_bwd_weight'][0] == 1, log
    _lib.BYTE_LOG = None
    assert rel_err(gw_w, gw_g).max().item() < 2 ** -18
