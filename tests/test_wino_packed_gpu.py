"""The packed transforms next to the MFMAs of the fp32 Winograd 16-channel kernels (csrc/conv_wino.hip, wino_rows_packed;
lf_set_tuning key 7 = 1, the default) against the scalar form they replace (key 7 = 0): the same operations in the same
order and association, so every output must be the same bit pattern -- compared as int32, which also holds NaNs to
account (torch.equal on floats calls NaN != NaN)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'

# tile = 2 x 8 x 16 (z, y, x): exactly one tile; interior tiles plus tiles on the first and last rows and planes; sides
# that are no multiple of the tile (partial tiles on every axis)
SHAPES = [(2, 2, 8, 16), (2, 6, 24, 48), (2, 5, 9, 33)]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b, what, min_finite=0.5):
    assert torch.equal(_bits(a), _bits(b)), f'{what}: {(_bits(a) != _bits(b)).sum().item()} of {a.numel()} bit patterns differ'
    assert torch.isfinite(a).float().mean().item() >= min_finite, f'{what}: too few finite outputs for the comparison to mean much'


def _both(fn):
    """fn() under the scalar form, then under the packed form; the switch is restored."""
    from latentfusion_amd import _lib
    L = _lib.lib()
    prev = L.lf_set_tuning(7, 0)
    try:
        assert prev == 1, 'the packed form is the default'
        old = fn()
        assert L.lf_set_tuning(7, 1) == 0
        new = fn()
        torch.cuda.synchronize()
    finally:
        L.lf_set_tuning(7, prev)
    return old, new


def _problem(shape, seed, special):
    """PixelNorm-range data (unit RMS over the channels) with a few exact zeros; `special`: also NaNs and infinities of both
    signs in the data AND in the weights (one weight each: a NaN or an infinity there takes a whole output channel)."""
    from latentfusion_amd import ops
    N, D, H, W = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, 16, D, H, W, generator=g)
    x = x / torch.sqrt((x ** 2).mean(dim=1, keepdim=True) + 1e-8)
    w = torch.randn(16, 16, 3, 3, 3, generator=g)
    flat = x.view(-1)
    idx = torch.randperm(flat.numel(), generator=g)
    flat[idx[:9]] = 0.0
    w.view(-1)[torch.randperm(w.numel(), generator=g)[:5]] = 0.0
    if special:
        flat[idx[9]] = float('nan')
        flat[idx[10]] = float('inf')
        flat[idx[11]] = float('-inf')
        w[3, 5, 1, 2, 0] = float('nan')
        w[9, 2, 0, 1, 1] = float('-inf')
    b = torch.randn(16, generator=g) * 0.1
    wp = torch.randn(16, 16 * D, 1, 1, generator=g)
    pb = torch.randn(16, generator=g) * 0.1
    he = ops.he_constant(torch.randn(16, 16, 3, 3, 3, generator=g))          # (a finite He constant in either case)
    return ops.cl(x.to(DEV)), w.to(DEV), b.to(DEV), wp.to(DEV), pb.to(DEV), he


def _proj_matrix(wp, D):
    return wp.reshape(16, 16, D).permute(0, 2, 1).reshape(16, D * 16).contiguous()


@pytest.mark.parametrize('special', [False, True])
@pytest.mark.parametrize('shape', SHAPES)
def test_forward_and_data_gradient_bit_identical(shape, special):
    """Forward with the engine's epilogue (He, bias, LeakyReLU, PixelNorm) and the data gradient fused with the previous
    layer's LeakyReLU' / PixelNorm'.  With special values PixelNorm would spread one NaN over all 16 channels of its voxel's
    3 x 3 x 3 neighbourhood and a NaN weight over everything, so that case also runs without PixelNorm."""
    from latentfusion_amd import ops
    from latentfusion_amd._lib import LF_EPI_LRELU, LF_EPI_PIXELNORM
    x, w, b, _, _, he = _problem(shape, 3, special)
    up, upt = ops.pack_conv3d_c16_wino(w), ops.pack_conv3d_c16_wino(w, transpose=True)
    full = LF_EPI_LRELU | LF_EPI_PIXELNORM
    # a finite previous layer for the fused backward (its saved activation and norm)
    xf, wf, _, _, _, hef = _problem(shape, 4, False)
    act, nrm = ops.conv3d_c16_wino(xf, ops.pack_conv3d_c16_wino(wf), None, hef, full)

    def run():
        outs = []
        for flags in ((full, LF_EPI_LRELU) if special else (full,)):
            y, n = ops.conv3d_c16_wino(x, up, b, he, flags)
            outs += [y] + ([n] if n is not None else [])
        outs.append(ops.conv3d_c16_wino(x, upt, None, he, 0, prev=(act, nrm, full))[0])
        return outs

    old, new = _both(run)
    for i, (a, c) in enumerate(zip(old, new)):
        # (special: PixelNorm and its derivative take the NaN weight's channel to every channel; the LeakyReLU-only
        # forward, output 2, keeps the other channels finite)
        _same(c, a, f'output {i} of {shape}', min_finite=0.5 if (not special or i == 2) else 0.0)


@pytest.mark.parametrize('special', [False, True])
@pytest.mark.parametrize('shape', SHAPES)
def test_projfwd_bit_identical(shape, special):
    """The convolution with the factor projection riding on it: y, norm, the projected image zp and its PixelNorm denominators."""
    from latentfusion_amd import ops
    from latentfusion_amd._lib import LF_EPI_LRELU, LF_EPI_PIXELNORM
    N, D, H, W = shape
    x, w, b, wp, pb, he = _problem(shape, 5, special)
    up, wA, phe = ops.pack_conv3d_c16_wino(w), ops.pack_wino_proj(_proj_matrix(wp, D)), ops.he_constant(wp)
    flags = LF_EPI_LRELU | LF_EPI_PIXELNORM
    cflags = LF_EPI_LRELU if special else flags                    # (see above: keep most of the volume finite)
    old, new = _both(lambda: ops.conv3d_c16_wino_projfwd(x, up, b, he, cflags, wA, pb, phe, flags))
    for name, a, c in zip(('y', 'norm', 'zp', 'pnorm'), old, new):
        if a is None:
            assert c is None
            continue
        _same(c, a, f'{name} of {shape}', min_finite=0.0 if special else 0.5)
    if special:
        assert torch.isfinite(new[0]).float().mean().item() >= 0.5


@pytest.mark.parametrize('special', [False, True])
@pytest.mark.parametrize('shape', SHAPES)
def test_projbwd_bit_identical(shape, special):
    """The opt-in fused projection backward (its halo planes are formed on chip, then the same MFMA phase)."""
    from latentfusion_amd import experimental, ops
    from latentfusion_amd._lib import LF_EPI_LRELU, LF_EPI_PIXELNORM
    N, D, H, W = shape
    x, w, b, wp, _, he = _problem(shape, 7, False)
    flags = LF_EPI_LRELU | LF_EPI_PIXELNORM
    act1, nrm1 = ops.conv3d_c16_wino(x, ops.pack_conv3d_c16_wino(w), None, he, flags)
    act2, nrm2 = ops.conv3d_c16_wino(act1, ops.pack_conv3d_c16_wino(w), b, he, flags)
    g = torch.Generator().manual_seed(8)
    gp = torch.randn(N, 16, H, W, generator=g)
    gp.view(-1)[:3] = 0.0
    w2 = w.clone()
    if special:
        gp[0, 2, H // 2, W // 2] = float('nan')
        gp[N - 1, 7, 0, W - 1] = float('inf')
        w2[4, 11, 2, 0, 1] = float('nan')
    gp = ops.cl(gp.to(DEV))
    upt = ops.pack_conv3d_c16_wino(w2, transpose=True)
    wtA, phe = ops.pack_wino_proj(_proj_matrix(wp, D), transpose=True), ops.he_constant(wp)
    for prev in ((act1, nrm1, flags), None):
        old, new = _both(lambda: experimental.conv3d_c16_wino_projbwd(gp, wtA, phe, act2, nrm2, flags, upt, he, prev=prev))
        _same(new, old, f'projbwd of {shape}, prev {prev is not None}', min_finite=0.0 if special else 0.5)


def test_switch_reports_and_refuses():
    from latentfusion_amd import _lib
    L = _lib.lib()
    assert L.lf_set_tuning(7, 5) == 1 and L.lf_set_tuning(7, -1) == 1, 'an out-of-range value leaves the default in place'
    assert L.lf_set_tuning(7, 0) == 1 and L.lf_set_tuning(7, 1) == 0
