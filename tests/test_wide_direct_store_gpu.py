"""The fused wide Winograd GEMMs (lf_wino_fused_gemm, lf_wino_fused_f16x3_gemm) in their DIRECT-WRITE form: launches large
enough that no frequency split happens (*_scratch_bytes == 0), so the GEMM kernel's own epilogue -- tile decode, guards,
depth-inner addressing, scale / bias / LeakyReLU -- writes y.  The small shapes of test_ops_gpu.py / test_wide_f16x3_gpu.py reach
every GEMM only through its frequency-split form (raw partial sums + the finish kernel).

Both cases map 64 -> 512 channels, as a forward (weight (512, 64, 3, 3, 3)) and as a data gradient (transpose=True with a
weight (64, 512, 3, 3, 3): 64 gradient channels in, 512 out), so each launch has the same grid:
  16^3, N = 8:  T = 4096 tiles; the f16x3 grid is 64 x 4 and the fp32 grids 64 x 8 / 64 x 4 / 32 x 8: the XCD renumbering is active;
  14^3, N = 12: T = 4116 tiles, no multiple of 64 or 128: grid x = 65 / 33, renumbering off, the last tile block ragged.
The fp64 reference covers the first and the last sample only (the CPU convolution of all of them would take a minute)."""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CIN, COUT = 64, 512
CASES = [(16, 8), (14, 12)]                                              # (S, N)


@functools.lru_cache(maxsize=None)
def _case(S, N):
    """Operands on the device and the fp64 references of samples 0 and N-1, computed once per case and left unchanged."""
    from latentfusion_amd import ops
    F = torch.nn.functional
    g = torch.Generator().manual_seed(S * 100 + N)
    x = torch.randn((N, CIN) + (S,) * 3, generator=g)
    w = torch.randn((COUT, CIN, 3, 3, 3), generator=g)
    b = torch.randn(COUT, generator=g) * 0.1
    gin = torch.randn((N, CIN) + (S,) * 3, generator=g)
    wt = torch.randn((CIN, COUT, 3, 3, 3), generator=g)                   # data gradient of a 512 -> 64 layer: 64 -> 512 channels
    he, het = ops.he_constant(w), ops.he_constant(wt)
    ends = [0, N - 1]
    pre = F.conv3d(x[ends].double(), w.double(), None, 1, 1) * he + b.double().view(1, -1, 1, 1, 1)
    act = F.leaky_relu(pre, 0.2)
    want = act / torch.sqrt((act ** 2).mean(dim=1, keepdim=True) + 1e-8)
    gwant = F.conv_transpose3d(gin[ends].double(), wt.double(), None, 1, 1) * het
    dev = dict(x=ops.cl(x.to(DEV)), w=w.to(DEV), b=b.to(DEV), gin=ops.cl(gin.to(DEV)), wt=wt.to(DEV))
    return dev, he, het, ends, want, gwant


def _no_scratch(S, N, f16x3):
    from latentfusion_amd import _lib
    L = _lib.lib()
    if f16x3:
        return L.lf_wino_fused_f16x3_scratch_bytes(N, S, S, S, COUT) == 0
    return L.lf_wino_fused_scratch_bytes(3, N, S, S, S, COUT) == 0


def _run(conv, S, N):
    """(y, y depth-inner, gx, gx depth-inner) of one form; forward with bias + LeakyReLU + PixelNorm."""
    from latentfusion_amd._lib import LF_EPI_LRELU, LF_EPI_PIXELNORM
    d, he, het, _ends, _want, _gwant = _case(S, N)
    flags = LF_EPI_LRELU | LF_EPI_PIXELNORM
    y, nrm = conv(d['x'], d['w'], d['b'], he, flags)
    yi, _ = conv(d['x'], d['w'], d['b'], he, flags, depth_inner=True)
    gx, _ = conv(d['gin'], d['wt'], None, het, 0, transpose=True)
    gxi, _ = conv(d['gin'], d['wt'], None, het, 0, transpose=True, depth_inner=True)
    torch.cuda.synchronize()
    assert tuple(y.shape) == (N, COUT, S, S, S) and tuple(gx.shape) == (N, COUT, S, S, S) and nrm is not None
    return y, yi, gx, gxi


def _err(a, ends, ref):
    return (a[ends].double().cpu() - ref).abs().max().item()


@pytest.mark.parametrize('S,N', CASES)
def test_fp32_direct_store_matches_fp64(S, N):
    """Bars of test_wide_conv_fused_gemm: 2e-5 max(1, max|ref|) forward, 3e-5 max(1, max|ref|) data gradient; the depth-inner
    layout equals the permuted default layout bit for bit."""
    from latentfusion_amd import ops
    assert _no_scratch(S, N, f16x3=False)
    _d, _he, _het, ends, want, gwant = _case(S, N)
    y, yi, gx, gxi = _run(ops.wide_conv, S, N)
    e, ge = _err(y, ends, want), _err(gx, ends, gwant)
    print(f'fp32 {S}^3 x {N}: forward {e:.3e} (max|ref| {want.abs().max().item():.3e}), gradient {ge:.3e} (max|ref| {gwant.abs().max().item():.3e})')
    assert e < 2e-5 * max(1.0, want.abs().max().item()), e
    assert ge < 3e-5 * max(1.0, gwant.abs().max().item()), ge
    assert tuple(yi.shape) == (N, S, S, S, COUT)
    assert torch.equal(yi, y.permute(0, 3, 4, 2, 1)) and torch.equal(gxi, gx.permute(0, 3, 4, 2, 1))


@pytest.mark.parametrize('S,N', CASES)
def test_f16x3_direct_store_within_twice_the_fp32_kernel(S, N):
    """Bar of test_wide_f16x3_gpu: max error <= max(2 x the fp32 kernel's, 4e-6 max|ref|), forward and data gradient; the
    depth-inner layout equals the permuted default layout bit for bit."""
    from latentfusion_amd import ops
    assert _no_scratch(S, N, f16x3=True) and _no_scratch(S, N, f16x3=False)
    _d, _he, _het, ends, want, gwant = _case(S, N)
    y32, _yi, g32, _gi = _run(ops.wide_conv, S, N)
    y16, yi16, g16, gi16 = _run(ops.wide_conv_f16x3, S, N)
    e32, e16 = _err(y32, ends, want), _err(y16, ends, want)
    ge32, ge16 = _err(g32, ends, gwant), _err(g16, ends, gwant)
    print(f'f16x3 {S}^3 x {N}: forward {e16:.3e} (fp32 {e32:.3e}), gradient {ge16:.3e} (fp32 {ge32:.3e})')
    assert e16 <= max(2 * e32, 4e-6 * want.abs().max().item()), (e16, e32)
    assert ge16 <= max(2 * ge32, 4e-6 * gwant.abs().max().item()), (ge16, ge32)
    assert tuple(yi16.shape) == (N, S, S, S, COUT)
    assert torch.equal(yi16, y16.permute(0, 3, 4, 2, 1)) and torch.equal(gi16, g16.permute(0, 3, 4, 2, 1))


@pytest.mark.parametrize('S,N', CASES)
def test_fp32_direct_store_workgroup_shapes(S, N):
    """Every 3-D workgroup shape of lf_wino_fused_gemm (lf_set_tuning key 3: 64x64, 128x64, 64x128) launches these shapes
    unsplit (512 / 256 / 256 and 520 / 260 / 264 workgroups against the wanted 512 / 256 / 256) and gives the result of the
    default pick bit for bit, as test_wide_conv_fused_gemm_workgroup_shapes asserts for split launches."""
    from latentfusion_amd import _lib, ops
    L = _lib.lib()
    L.lf_set_tuning.restype = ctypes.c_int
    L.lf_set_tuning.argtypes = [ctypes.c_int, ctypes.c_int]
    assert _no_scratch(S, N, f16x3=False)
    ref = _run(ops.wide_conv, S, N)
    try:
        for cfg in (0, 1, 2):
            assert L.lf_set_tuning(3, cfg) >= -1
            got = _run(ops.wide_conv, S, N)
            assert all(torch.equal(a, b) for a, b in zip(got, ref)), cfg
    finally:
        L.lf_set_tuning(3, -1)
