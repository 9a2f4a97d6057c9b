"""lf_wino_fused_gemm_part / lf_wino_fused_scratch_bytes_part: ONE launch over N samples taken as parts of part_n consecutive
samples, each part's slice of y bit-identical to lf_wino_fused_gemm on that part alone (N = part_n).

What ties a sample's rounding to its batch in lf_wino_fused_gemm is the frequency split zs (wino_ring::Plan::split): it groups
the F = 64 (3-D) / 16 (2-D) frequency contributions into zs partial sums that the finish kernel adds in a fixed order.  The
shapes below are chosen so that the batch and the part pick DIFFERENT splits (derived by hand from Plan::split and
pick_fused_cfg; tiles per sample = ceil(D/2) ceil(H/2) ceil(W/2), 64 x 64 workgroups want 512, 8-wave shapes 256):
  3-D 64 -> 64,  8^3,  N = 16, part 1:   T = 1024 -> 16 workgroups -> zs 32;  part T = 64 -> 1 workgroup -> zs 64
  3-D 64 -> 64,  16^3, N = 8,  part 1/2: T = 4096 -> 64 workgroups -> zs 8;   part T = 512 / 1024 -> zs 64 / 32
  3-D 64 -> 128, 7 x 6 x 5, N = 6, part 3: ragged tiles (odd extents, a tile block that is not full)
  2-D 128 -> 128, 16^2, N = 64, part 1:  T = 4096 -> the 128 x 128 shape, 32 workgroups -> zs 8;  part T = 64 -> 64 x 64, zs 16
  2-D 64 -> 64,  13 x 9, N = 12, part 4: ragged tiles
The control test shows that at 16^3, N = 8 the plain batch launch does differ from the single-sample launch, i.e. that the
comparisons above would fail for an entry point that ignored part_n."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SLOPE = 0.2
LF_EINVAL, LF_EALIGN, LF_ENOSPC = -1, -2, -3

# name: (dims, cin, cout, (D, H, W), N)
SHAPES = {
    'c64_8': (3, 64, 64, (8, 8, 8), 16),
    'c64_16': (3, 64, 64, (16, 16, 16), 8),
    'c128_ragged': (3, 64, 128, (7, 6, 5), 6),
    'd128_16': (2, 128, 128, (1, 16, 16), 64),
    'd64_ragged': (2, 64, 64, (1, 13, 9), 12),
}


def _transform(L, x, dims, N, D, H, W, cin):
    """V [F][T][cin] of the channels-last x (N, cin, [D,] H, W)."""
    from latentfusion_amd._lib import check
    s = torch.cuda.current_stream().cuda_stream
    if dims == 3:
        T = L.lf_wino3d_tiles(N, D, H, W)
        V = torch.empty(64, T, cin, device=DEV, dtype=torch.float32)
        check(L.lf_wino3d_input_transform(x.data_ptr(), V.data_ptr(), N, D, H, W, cin, s), 'lf_wino3d_input_transform')
    else:
        T = L.lf_wino2d_tiles(N, H, W)
        V = torch.empty(16, T, cin, device=DEV, dtype=torch.float32)
        check(L.lf_wino2d_input_transform(x.data_ptr(), V.data_ptr(), N, H, W, cin, s), 'lf_wino2d_input_transform')
    return V


@functools.lru_cache(maxsize=None)
def _case(name, transpose=False):
    """Operands of a shape, built once and left unchanged: x (channels-last, random normal), its transform V, the packed
    weights U2 (ops.pack_conv_wino_fused; transpose: the data-gradient pack of a (cin, cout) layer), a bias."""
    from latentfusion_amd import _lib, ops
    L = _lib.lib()
    dims, cin, cout, (D, H, W), N = SHAPES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)) + transpose)
    sp = (D, H, W) if dims == 3 else (H, W)
    x = ops.cl(torch.randn((N, cin) + sp, generator=g).to(DEV))
    wshape = ((cin, cout) if transpose else (cout, cin)) + (3,) * dims
    w = torch.randn(wshape, generator=g).to(DEV)
    U2 = ops.pack_conv_wino_fused(w, transpose=transpose)
    bias = torch.randn(cout, generator=g).to(DEV)
    V = _transform(L, x, dims, N, D, H, W, cin)
    torch.cuda.synchronize()
    return x, V, U2, bias, ops.he_constant(w)


def _gemm(name, V, U2, bias, he, flags, N, part_n=None):
    """One call of lf_wino_fused_gemm (part_n None) or lf_wino_fused_gemm_part on N samples: y as a flat [N][rest] tensor."""
    from latentfusion_amd import _lib
    from latentfusion_amd._lib import check
    L = _lib.lib()
    dims, cin, cout, (D, H, W), _N = SHAPES[name]
    y = torch.full((N, D * H * W * cout), float('nan'), device=DEV, dtype=torch.float32)
    s = torch.cuda.current_stream().cuda_stream
    b = bias.data_ptr() if bias is not None else None
    if part_n is None:
        nscr = L.lf_wino_fused_scratch_bytes(dims, N, D, H, W, cout)
        scr = torch.empty(nscr // 4 + 4, device=DEV, dtype=torch.float32)
        check(L.lf_wino_fused_gemm(V.data_ptr(), U2.data_ptr(), b, y.data_ptr(), scr.data_ptr(), nscr, dims, N, D, H, W, cin, cout,
                                   he, flags, SLOPE, s), 'lf_wino_fused_gemm')
    else:
        nscr = L.lf_wino_fused_scratch_bytes_part(dims, N, D, H, W, cout, part_n)
        scr = torch.empty(nscr // 4 + 4, device=DEV, dtype=torch.float32)
        check(L.lf_wino_fused_gemm_part(V.data_ptr(), U2.data_ptr(), b, y.data_ptr(), scr.data_ptr(), nscr, dims, N, D, H, W, cin,
                                        cout, he, flags, SLOPE, part_n, s), 'lf_wino_fused_gemm_part')
    torch.cuda.synchronize()
    return y


def _part_V(name, x, p, part_n):
    from latentfusion_amd import _lib
    dims, cin, _cout, (D, H, W), _N = SHAPES[name]
    xs = x[p * part_n:(p + 1) * part_n]                    # (whole samples of a channels-last batch: contiguous memory)
    return _transform(_lib.lib(), xs, dims, part_n, D, H, W, cin)


def _check_parts(name, part_n, flags=0, with_bias=True, transpose=False):
    x, V, U2, bias, he = _case(name, transpose)
    N = SHAPES[name][4]
    b = bias if with_bias else None
    y = _gemm(name, V, U2, b, he, flags, N, part_n)
    assert torch.isfinite(y).all()
    for p in range(N // part_n):
        one = _gemm(name, _part_V(name, x, p, part_n), U2, b, he, flags, part_n)
        assert torch.equal(y[p * part_n:(p + 1) * part_n], one), (name, part_n, p)
    return y


@pytest.mark.parametrize('name,part_n', [('c64_8', 1), ('c64_16', 1), ('c64_16', 2), ('c128_ragged', 3), ('d128_16', 1),
                                         ('d64_ragged', 4)])
def test_each_part_equals_the_plain_call_on_that_part(name, part_n):
    from latentfusion_amd._lib import LF_EPI_LRELU
    _check_parts(name, part_n, LF_EPI_LRELU)


def test_depth_inner_output():
    from latentfusion_amd._lib import LF_EPI_LRELU, LF_OUT_DEPTH_INNER
    yi = _check_parts('c64_16', 2, LF_EPI_LRELU | LF_OUT_DEPTH_INNER)
    y = _check_parts('c64_16', 2, LF_EPI_LRELU)
    N, S, C = 8, 16, 64
    assert torch.equal(yi.view(N, S, S, S, C), y.view(N, S, S, S, C).permute(0, 2, 3, 1, 4))      # [N][H][W][D][C] of [N][D][H][W][C]


@pytest.mark.parametrize('name,part_n', [('c64_16', 2), ('d64_ragged', 4)])
@pytest.mark.parametrize('with_bias', [False, True])
@pytest.mark.parametrize('lrelu', [False, True])
def test_bias_and_lrelu_forms(name, part_n, with_bias, lrelu):
    from latentfusion_amd._lib import LF_EPI_LRELU
    _check_parts(name, part_n, LF_EPI_LRELU if lrelu else 0, with_bias)


def test_data_gradient_pack():
    _check_parts('c128_ragged', 3, 0, with_bias=False, transpose=True)
    _check_parts('d128_16', 1, 0, with_bias=False, transpose=True)


def test_control_plain_batch_differs_from_single_sample():
    """What makes the comparisons above mean something: the plain launch over the batch (zs 8) and over one sample (zs 64)
    do not agree bit for bit."""
    from latentfusion_amd._lib import LF_EPI_LRELU
    name = 'c64_16'
    x, V, U2, bias, he = _case(name)
    N = SHAPES[name][4]
    y = _gemm(name, V, U2, bias, he, LF_EPI_LRELU, N)
    differ = 0
    for p in range(N):
        one = _gemm(name, _part_V(name, x, p, 1), U2, bias, he, LF_EPI_LRELU, 1)
        differ += int((y[p:p + 1] != one).sum().item())
    print('elements of the plain batch launch that differ from the single-sample launch:', differ, 'of', y.numel())
    assert differ >= 1


@pytest.mark.parametrize('name', ['c64_16', 'c128_ragged', 'd128_16'])
def test_part_equal_to_batch_is_the_plain_call(name):
    from latentfusion_amd import _lib, ops
    from latentfusion_amd._lib import LF_EPI_LRELU
    L = _lib.lib()
    dims, cin, cout, (D, H, W), N = SHAPES[name]
    x, V, U2, bias, he = _case(name)
    assert torch.equal(_gemm(name, V, U2, bias, he, LF_EPI_LRELU, N, part_n=N), _gemm(name, V, U2, bias, he, LF_EPI_LRELU, N))
    assert L.lf_wino_fused_scratch_bytes_part(dims, N, D, H, W, cout, N) == L.lf_wino_fused_scratch_bytes(dims, N, D, H, W, cout)
    # the same sections and library calls through ops, with and without part_n = N
    seen = []
    for part in (None, N):
        ops.KERNEL_TIMER, _lib.BYTE_LOG = [], {}
        try:
            y, _ = ops.conv_wino_fused(x, U2, cout, bias, he, LF_EPI_LRELU, part_n=part)
            torch.cuda.synchronize()
            seen.append((y, [str(n) for n, _, _ in ops.KERNEL_TIMER], sorted(v[0] for v in _lib.BYTE_LOG.values())))
        finally:
            ops.KERNEL_TIMER, _lib.BYTE_LOG = None, None
    assert torch.equal(seen[0][0], seen[1][0])
    assert seen[0][1] == seen[1][1] and seen[0][2] == seen[1][2]


def test_scratch_query():
    from latentfusion_amd import _lib
    L = _lib.lib()
    for name, (dims, _cin, cout, (D, H, W), N) in SHAPES.items():
        plain = L.lf_wino_fused_scratch_bytes(dims, N, D, H, W, cout)
        for part_n in range(1, N + 1):
            if N % part_n:
                assert L.lf_wino_fused_scratch_bytes_part(dims, N, D, H, W, cout, part_n) == 0
                continue
            q = L.lf_wino_fused_scratch_bytes_part(dims, N, D, H, W, cout, part_n)
            assert q >= plain, (name, part_n)
            if part_n == N:
                assert q == plain
    assert L.lf_wino_fused_scratch_bytes_part(3, 8, 16, 16, 16, 64, 0) == 0
    assert L.lf_wino_fused_scratch_bytes_part(3, 8, 16, 16, 16, 64, -1) == 0


def test_abi_errors_leave_y_intact():
    from latentfusion_amd import _lib
    L = _lib.lib()
    name = 'c64_16'
    dims, cin, cout, (D, H, W), N = SHAPES[name]
    _x, V, U2, bias, he = _case(name)
    s = torch.cuda.current_stream().cuda_stream
    n_y = N * D * H * W * cout
    ybuf = torch.full((n_y + 4,), -7.5, device=DEV, dtype=torch.float32)
    nscr = L.lf_wino_fused_scratch_bytes_part(dims, N, D, H, W, cout, 1)
    assert nscr > 0
    scr = torch.empty(nscr // 4 + 4, device=DEV, dtype=torch.float32)

    def call(y_ptr, nbytes, part_n):
        rc = L.lf_wino_fused_gemm_part(V.data_ptr(), U2.data_ptr(), bias.data_ptr(), y_ptr, scr.data_ptr(), nbytes, dims, N, D, H, W,
                                       cin, cout, he, 0, SLOPE, part_n, s)
        torch.cuda.synchronize()
        assert bool((ybuf == -7.5).all()), 'y was written'
        return rc

    for part_n in (0, -1, 3):
        assert call(ybuf.data_ptr(), nscr, part_n) == LF_EINVAL, part_n
    assert call(ybuf.data_ptr(), nscr - 1, 1) == LF_ENOSPC
    assert call(ybuf.data_ptr() + 4, nscr, 1) == LF_EALIGN                 # (one float in: 4-byte aligned only)


@pytest.mark.parametrize('dims,ch,S,T,n', [(3, 64, 16, 4, 2), (2, 128, 16, 32, 2)])
def test_ops_wide_parts_scope(dims, ch, S, T, n):
    """Under ops.wide_parts(n) a wide _Conv3x3 forward and its input gradient on T * n rows equal, per part, the same call on
    the part's n rows outside the scope; the backward runs after the scope has exited.  (3-D 64 -> 64 on 16^3: zs 8 for the 8
    rows / 32 for 2; 2-D 128 -> 128 on 16^2: zs 8 for the 64 rows / 16 for 2.)"""
    from latentfusion_amd import ops
    from latentfusion_amd._lib import LF_EPI_LRELU, LF_EPI_PIXELNORM
    g = torch.Generator().manual_seed(dims * 7 + ch)
    flags = LF_EPI_LRELU | LF_EPI_PIXELNORM
    x = ops.cl(torch.randn((T * n, ch) + (S,) * dims, generator=g).to(DEV))
    w = torch.randn((ch, ch) + (3,) * dims, generator=g).to(DEV)
    b = (0.1 * torch.randn(ch, generator=g)).to(DEV)
    gy = ops.cl(torch.randn((T * n, ch) + (S,) * dims, generator=g).to(DEV))
    xb = x.clone().requires_grad_(True)
    with ops.wide_parts(n):
        y = ops._Conv3x3.apply(xb, w, b, flags)
    assert ops.WIDE_PARTS is None
    (gx,) = torch.autograd.grad(y, [xb], grad_outputs=[gy])
    torch.cuda.synchronize()
    for p in range(T):
        r = slice(p * n, (p + 1) * n)
        xp = ops.cl(x[r]).clone().requires_grad_(True)
        yp = ops._Conv3x3.apply(xp, w, b, flags)
        (gxp,) = torch.autograd.grad(yp, [xp], grad_outputs=[ops.cl(gy[r])])
        torch.cuda.synchronize()
        assert torch.equal(y[r], yp), p
        assert torch.equal(gx[r], gxp), p
