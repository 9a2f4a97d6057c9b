"""The z-staged halo of the fixed Winograd 16-channel forms (csrc/conv_wino.hip, ZST; lf_set_tuning key 8 = 4) against the same
forms on the raw-plane halo they were cut from (key 8 = 3) and against the generic kernels (key 8 = 0).  Staged, a lane combines
the four z planes of a halo point in registers (F0 = d0 - d2, F1 = d1 + d2, F2 = d2 - d1, F3 = d1 - d3) and writes the
frequency planes to LDS; unstaged, every overlapping tile reads two raw planes and combines them itself.  Same operations on the
same operands, so every output must be the same bit pattern -- compared as int32, which also holds the signs of zeros and the
signs and payloads of NaNs to account."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'

# tile = 2 x 8 x 16 (z, y, x), halo 4 x 10 x 18; a workgroup walks up a column of tiles
SHAPES = [
    (2, 6, 10, 20),    # three tiles up a column (slide twice, then a full fetch), two tiles in x and in y, a change of sample
    (1, 5, 9, 17),     # ragged in z, y and x: the out-of-range pieces must stage the same zeros
    (1, 2, 8, 16),     # one tile, no slide
    (3, 8, 16, 32),    # whole columns of four tiles (the projection form's ranges), three samples
]
CASES = ('plain', 'zeros', 'nan')
NAMES = ('forward y', 'forward norm_out', 'data gradient + previous layer', 'plain data gradient',
         'projfwd y', 'projfwd norm_out', 'projfwd zp', 'projfwd pnorm')
GENERIC, RAW, STAGED, DEFAULT = 0, 3, 4, 1


def _bits(t):
    return t.contiguous().view(torch.int32)


def _input(shape, case):
    N, D, H, W = shape
    g = torch.Generator().manual_seed(11)
    x = torch.randn(N, 16, D, H, W, generator=g)
    x = x / torch.sqrt((x ** 2).mean(dim=1, keepdim=True) + 1e-8)
    if case == 'zeros':
        # blocks that span z planes, tile borders and halo overlaps: +0 - +0, -0 - -0 (both +0) and -0 + -0 (-0) all occur
        x[:, :, : (D + 1) // 2, 1: H // 2 + 2, 2: W // 2 + 3] = 0.0
        x[:, :, D // 2:, H // 2:, W // 2 - 1:] = -0.0
        assert (x == 0).float().mean() > 0.2 and torch.signbit(x[x == 0]).any() and not torch.signbit(x[x == 0]).all()
    if case == 'nan':
        # one voxel, two payloads and both signs among its channels
        v = x[N - 1, :, D // 2, H // 2, W // 2].view(torch.int32)
        v[0::4] = 0x7FC00000
        v[1::4] = 0x7FC12345
        v[2::4] = 0xFFC00001 - (1 << 32)
        assert torch.isnan(x[N - 1, :, D // 2, H // 2, W // 2]).sum().item() == 12
    return x


@functools.lru_cache(maxsize=None)
def _outputs(shape, case, value):
    """The four launches of the render loop (forward block, data gradient with the previous layer, plain data gradient, forward
    block with the factor projection) under one value of key 8.  Computed once per (shape, case, value) and left unchanged."""
    from latentfusion_amd import _lib, ops
    from latentfusion_amd._lib import LF_EPI_LRELU, LF_EPI_PIXELNORM
    N, D, H, W = shape
    g = torch.Generator().manual_seed(12)
    w = torch.randn(16, 16, 3, 3, 3, generator=g).to(DEV)
    b = (torch.randn(16, generator=g) * 0.1).to(DEV)
    wp = torch.randn(16, D * 16, generator=g).to(DEV)
    pb = (torch.randn(16, generator=g) * 0.1).to(DEV)
    act = torch.randn(N, 16, D, H, W, generator=g)
    act = ops.cl((act / torch.sqrt((act ** 2).mean(dim=1, keepdim=True) + 1e-8)).to(DEV))
    nrm = (torch.rand(N * D * H * W, generator=g) + 0.5).to(DEV)
    x = ops.cl(_input(shape, case).to(DEV))
    he, phe = ops.he_constant(w), ops.he_constant(wp.view(16, D * 16, 1, 1))
    up, upt, wA = ops.pack_conv3d_c16_wino(w), ops.pack_conv3d_c16_wino(w, transpose=True), ops.pack_wino_proj(wp)
    full = LF_EPI_LRELU | LF_EPI_PIXELNORM
    L = _lib.lib()
    prev = L.lf_set_tuning(8, value)
    try:
        assert prev == DEFAULT, 'value 1 is the default'
        y, n = ops.conv3d_c16_wino(x, up, b, he, full)
        gprev = ops.conv3d_c16_wino(x, upt, None, he, 0, prev=(act, nrm, full))[0]
        gplain = ops.conv3d_c16_wino(x, upt, None, he, 0)[0]
        pf = ops.conv3d_c16_wino_projfwd(x, up, b, he, full, wA, pb, phe, full)
        torch.cuda.synchronize()
    finally:
        L.lf_set_tuning(8, prev)
    return (y, n, gprev, gplain) + tuple(pf)


@pytest.mark.parametrize('case', CASES)
@pytest.mark.parametrize('shape', SHAPES)
def test_staged_forms_bit_identical(shape, case):
    staged = _outputs(shape, case, STAGED)
    for other, what in ((RAW, 'the raw-plane halo (key 8 = 3)'), (GENERIC, 'the generic kernel (key 8 = 0)')):
        for name, a, c in zip(NAMES, _outputs(shape, case, other), staged):
            diff = (_bits(a) != _bits(c)).sum().item()
            assert diff == 0, f'{name} of {shape}, {case}: {diff} of {a.numel()} bit patterns differ from {what}'
    for name, c in zip(NAMES, staged):
        finite = torch.isfinite(c).float().mean().item()
        assert finite >= (0.3 if case == 'nan' else 1.0), f'{name} of {shape}, {case}: {finite:.2f} finite'
    if case == 'nan':
        assert torch.isnan(staged[3]).any() and torch.isnan(staged[6]).any(), 'the NaN voxel reached the outputs'


@pytest.mark.parametrize('shape', SHAPES[:2])
def test_default_is_one_of_the_two_stagings(shape):
    """Key 8 = 1 picks a staging per form; whichever it picks, the bits are those of every other value."""
    for name, a, c in zip(NAMES, _outputs(shape, 'plain', STAGED), _outputs(shape, 'plain', DEFAULT)):
        assert torch.equal(_bits(a), _bits(c)), f'{name} of {shape}'


def test_switch_takes_the_new_values():
    from latentfusion_amd import _lib
    L = _lib.lib()
    try:
        assert L.lf_set_tuning(8, RAW) == DEFAULT and L.lf_set_tuning(8, STAGED) == RAW and L.lf_set_tuning(8, 5) == STAGED
        assert L.lf_set_tuning(8, DEFAULT) == STAGED, 'an out-of-range value leaves the last one in place'
    finally:
        L.lf_set_tuning(8, DEFAULT)
