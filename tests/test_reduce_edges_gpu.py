"""Edge cases of the view reductions and depth-column composites (csrc/reduce.hip) against fp64 references: the same inputs cast
up, the tolerances of test_reduce_gpu.py unchanged.

  fuse_views      V = 1, 2, 3, 4, 5, 8, 9, 17 (both remainders of the four-at-a-time view loop, even V -> lower median), element
                  counts and view strides that take the scalar and the f32x4 instantiation, columns full of ties (values from
                  {-1, 0, 1}), and NaN / +inf / -inf in one view at a time for every kind (the pattern torch gives on the host:
                  a NaN in any view is the result, for the median too)
  fuse_blend,     logits of magnitude 80 and columns with one +80 among -80s (softmax saturates; weights and gradients stay
  column_softmax, finite), a column of -inf (NaN as torch), D = 1 .. 256 for the kernel that forms its logits on the way in and
  ..._head        D = 257 rejected on the host before anything is launched, P = 1, 15, 16, 17 columns; -inf logits in the head
                  kernel too, whose register slots use -inf as their filler
  column_sum,     C = 4, 12, 260 with row counts that leave the last workgroup partly empty, D = 1
  column_scale

Measured on an MI355X, largest |kernel - fp64| over all cases of a family (that of the fp32 torch expression on the same
inputs in brackets): fuse_views mean 1.3e-7 (1.2e-7), max / abs_max / median and every selection gradient exact; blend weights
6.2e-8 (6.2e-8), blend output 2.3e-7 (2.3e-7), its gradients 1.3e-7 (z) and 2.0e-7 (logits); column softmax weights 6.9e-8
(7.9e-8), expected depth 7.8e-8 (7.8e-8); head weights 1.4e-7, head expected depth 1.3e-7; column_sum 1.4e-6 (2.1e-6);
column_scale exact, its weight gradient 4.2e-6 (5.4e-6)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
LF_EINVAL = -1
KINDS = ('mean', 'max', 'abs_max', 'median')


def _s():
    return torch.cuda.current_stream().cuda_stream


def close(a, b, atol, rtol, what='', f32=None):
    """Kernel output (fp32, device) against an fp64 host reference; NaN only where the reference has NaN.  Prints the largest
    error (and, where given, that of the fp32 torch expression `f32` on the same inputs) for the table above."""
    a, b = a.detach().cpu().double().contiguous(), b.detach().cpu().double().contiguous()
    fin = torch.isfinite(b)
    err = float((a - b)[fin].abs().max()) if fin.any() else 0.0
    e32 = float((f32.detach().double() - b)[fin].abs().max()) if f32 is not None and fin.any() else float('nan')
    print(f'[reduce-edges] {what}: |hip - fp64| {err:.2e}  |fp32 torch - fp64| {e32:.2e}')
    torch.testing.assert_close(a, b, atol=atol, rtol=rtol, equal_nan=True, msg=lambda m: f'{what}: {m}')


def _pool_ref(t, kind):
    if kind == 'max':
        return t.max(dim=1, keepdim=True)[0]
    if kind == 'abs_max':
        idx = t.abs().max(dim=1, keepdim=True)[1]
        return torch.gather(t, 1, idx)
    if kind == 'mean':
        return t.mean(dim=1, keepdim=True)
    return t.median(dim=1, keepdim=True)[0]


def _depth_coord64(D):
    return torch.linspace(-1.0, 1.0, D, dtype=torch.float64).view(1, 1, -1, 1, 1)


# ---------------------------------------------------------------------------------------------------------------------------
# view reductions
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('V', [1, 2, 3, 4, 5, 8, 9, 17])
def test_fuse_views_view_counts_vs_fp64(kind, V):
    """Every remainder of the four-at-a-time view loop, on an element count that takes the f32x4 instantiation (256) and on
    one that takes the scalar one (105 = 3*5*7, not a multiple of 4)."""
    from latentfusion_amd import ops
    for inner in ((4, 4, 4, 4), (3, 5, 7)):
        g = torch.Generator().manual_seed(V * 131 + len(inner))
        z0 = torch.randn((2, V) + inner, generator=g)
        z = z0.to(DEV).requires_grad_(True)
        out = ops.fuse_views(z, kind)
        zr = z0.double().requires_grad_(True)
        ref = _pool_ref(zr, kind)
        assert out.shape == ref.shape
        close(out, ref, atol=1e-6 if kind == 'mean' else 0, rtol=1e-6 if kind == 'mean' else 0, what=f'{kind} V={V} {inner}',
              f32=_pool_ref(z0, kind))
        a = torch.randn(ref.shape, generator=g)
        (out * a.to(DEV)).sum().backward()
        (ref * a.double()).sum().backward()
        close(z.grad, zr.grad, atol=1e-7, rtol=1e-6, what=f'{kind} V={V} {inner} grad')


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('n,stride', [(64, 64), (64, 68), (64, 66), (63, 63), (63, 64), (1, 1), (5, 9)])
def test_fuse_views_strides_through_the_entry_point(kind, n, stride):
    """lf_fuse_views_fwd / _bwd with views `stride` floats apart: n and stride multiples of 4 -> f32x4 loads, anything else
    -> the scalar instantiation.  The floats between the views are never read (they hold NaN) or written."""
    from latentfusion_amd import _lib, ops
    L = _lib.lib()
    V = 5
    g = torch.Generator().manual_seed(n * 100 + stride)
    buf = torch.full((V, stride), float('nan'))
    buf[:, :n] = torch.randn(V, n, generator=g)
    zb = buf.to(DEV)
    out = torch.full((n,), 7.0, device=DEV)
    idx = torch.full((n,), -1, device=DEV, dtype=torch.int32)
    k = ops.FUSE_KINDS[kind]
    assert L.lf_fuse_views_fwd(zb.data_ptr(), out.data_ptr(), idx.data_ptr(), k, V, n, stride, _s()) == 0
    ref = _pool_ref(buf[:, :n].double().unsqueeze(0), kind).reshape(n)
    close(out, ref, atol=1e-6 if kind == 'mean' else 0, rtol=1e-6 if kind == 'mean' else 0, what=f'{kind} n={n} stride={stride}')
    gz = torch.full((V, stride), 7.0, device=DEV)
    gg = torch.randn(n, generator=g)
    ggd = gg.to(DEV)
    assert L.lf_fuse_views_bwd(ggd.data_ptr(), idx.data_ptr(), gz.data_ptr(), k, V, n, stride, _s()) == 0
    torch.cuda.synchronize()
    gz = gz.cpu()
    assert (gz[:, n:] == 7.0).all()
    if kind == 'mean':
        close(gz[:, :n], (gg.double() / V).expand(V, n), atol=1e-7, rtol=1e-6)
    else:
        sel = idx.cpu().long()
        assert ((sel >= 0) & (sel < V)).all()
        assert torch.equal(buf[:, :n].gather(0, sel.view(1, n)).reshape(n), out.cpu())
        want = torch.zeros(V, n).scatter_(0, sel.view(1, n), gg.view(1, n))
        assert torch.equal(gz[:, :n], want)


@pytest.mark.parametrize('kind', ['max', 'abs_max', 'median'])
@pytest.mark.parametrize('V', [2, 3, 4, 5, 8, 9])
def test_fuse_views_ties(kind, V):
    """Values from {-1, 0, 1}: most columns tie.  The value is torch's; the gradient is g on exactly ONE view, and that view
    holds the selected value (which of the tied views is not defined by torch on a device, so the index is not compared)."""
    from latentfusion_amd import ops
    for inner in ((4, 4, 4), (3, 7)):
        g = torch.Generator().manual_seed(V + 7 * len(inner))
        z0 = torch.randint(-1, 2, (2, V) + inner, generator=g).float()
        z = z0.to(DEV).requires_grad_(True)
        out = ops.fuse_views(z, kind)
        if kind == 'abs_max':
            # +1 and -1 tie in magnitude, and which of them torch's abs().max() index picks is not specified: the expected value
            # is the FIRST view of largest magnitude (torch.argmax documents first-occurrence; the kernel's rule, and what the
            # host path returns on the CPU)
            mag = z0.double().abs()
            first = (mag == mag.amax(dim=1, keepdim=True)).int().argmax(dim=1, keepdim=True)
            ref = torch.gather(z0.double(), 1, first)
            assert torch.equal(ref.abs(), _pool_ref(z0.double(), kind).abs())
        else:
            ref = _pool_ref(z0.double(), kind)
        assert torch.equal(out.detach().cpu().double(), ref)
        a = torch.rand(ref.shape, generator=g) + 0.5               # (never zero)
        (out * a.to(DEV)).sum().backward()
        gz = z.grad.cpu()
        hit = gz != 0
        assert (hit.sum(dim=1) == 1).all()
        assert torch.equal(gz.sum(dim=1, keepdim=True), a)
        assert torch.equal((z0 * hit).sum(dim=1, keepdim=True), out.detach().cpu())


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('V', [1, 2, 3, 4, 5, 9])
def test_fuse_views_nonfinite_pattern(kind, V):
    """NaN, +inf and -inf planted in one view at a time (one column per (view, value) pair, the other columns stay finite):
    the output is what torch returns on the host, NaN included -- for the median as for the other kinds."""
    from latentfusion_amd import ops
    vals = (float('nan'), float('inf'), float('-inf'))
    for inner in ((16, 4), (13, 5)):                              # 64 elements (f32x4) and 65 (scalar)
        g = torch.Generator().manual_seed(V)
        n = inner[0] * inner[1]
        z0 = torch.randn(1, V, n, generator=g)
        for v in range(V):
            for j, val in enumerate(vals):
                z0[0, v, (v * 3 + j) * 2 % n] = val
        z0 = z0.view((1, V) + inner)
        z = z0.to(DEV).requires_grad_(True)
        out = ops.fuse_views(z, kind)
        ref = _pool_ref(z0.double(), kind)
        assert torch.equal(torch.isnan(out.detach().cpu()), torch.isnan(ref)), (kind, V, inner)
        close(out, ref, atol=1e-6 if kind == 'mean' else 0, rtol=1e-6 if kind == 'mean' else 0, what=f'{kind} V={V} {inner}')
        if kind != 'mean':                                         # the selected view stays valid for the backward
            a = torch.rand(ref.shape, generator=g) + 0.5
            (out * a.to(DEV)).sum().backward()
            gz = z.grad.cpu()
            assert ((gz != 0).sum(dim=1) == 1).all() and torch.equal(gz.sum(dim=1, keepdim=True), a)
            picked = (torch.nan_to_num(z0, nan=12345.0) * (gz != 0)).sum(dim=1, keepdim=True)
            assert torch.equal(picked, torch.nan_to_num(out.detach().cpu(), nan=12345.0))


# ---------------------------------------------------------------------------------------------------------------------------
# softmax over views / over the depth column at saturating logits
# ---------------------------------------------------------------------------------------------------------------------------
def _saturating_logits(shape, dim, g):
    """+-80 with unit noise; every fourth column along `dim` is one +80 among -80s."""
    lg = 80.0 * (torch.randint(0, 2, shape, generator=g).float() * 2 - 1) + torch.randn(shape, generator=g)
    lg = lg.movedim(dim, -1).contiguous()
    flat = lg.view(-1, lg.shape[-1])
    flat[::4] = -80.0
    flat[::4, 0] = 80.0
    return lg.movedim(-1, dim).contiguous()


@pytest.mark.parametrize('shape', [(1, 1, 4, 1, 1, 1), (2, 2, 4, 1, 3, 5), (1, 5, 8, 2, 4, 2), (1, 3, 4, 1, 1, 17)])
def test_fuse_blend_saturated_vs_fp64(shape):
    from latentfusion_amd import ops
    B, V, C, D, H, W = shape
    g = torch.Generator().manual_seed(sum(shape))
    z0 = torch.randn(shape, generator=g)
    l0 = _saturating_logits((B, V, 1, D, H, W), 1, g)
    z, lg = z0.to(DEV).requires_grad_(True), l0.to(DEV).requires_grad_(True)
    out, w = ops.fuse_blend(z, lg)
    zr, lr = z0.double().requires_grad_(True), l0.double().requires_grad_(True)
    wr = torch.softmax(lr, dim=1)
    ref = torch.sum(zr * wr, dim=1, keepdim=True)
    w32 = torch.softmax(l0, dim=1)
    close(w, wr, atol=1e-6, rtol=1e-5, what='blend weights', f32=w32)
    close(out, ref, atol=2e-6, rtol=1e-5, what='blend out', f32=torch.sum(z0 * w32, dim=1, keepdim=True))
    a = torch.randn(ref.shape, generator=g)
    (out * a.to(DEV)).sum().backward()
    (ref * a.double()).sum().backward()
    assert torch.isfinite(z.grad).all() and torch.isfinite(lg.grad).all()
    close(z.grad, zr.grad, atol=1e-6, rtol=1e-5, what='gz')
    close(lg.grad, lr.grad, atol=5e-6, rtol=1e-4, what='glogits')


def test_fuse_blend_all_minus_inf_column_is_nan_as_torch():
    from latentfusion_amd import ops
    g = torch.Generator().manual_seed(5)
    z0 = torch.randn(1, 3, 4, 2, 3, 3, generator=g)
    l0 = torch.randn(1, 3, 1, 2, 3, 3, generator=g)
    l0[0, :, 0, 1, 2, 0] = float('-inf')                           # every view of one voxel
    l0[0, 1, 0, 0, 0, 0] = float('-inf')                           # one view of another: its weight is exactly 0
    out, w = ops.fuse_blend(z0.to(DEV), l0.to(DEV))
    wr = torch.softmax(l0.double(), dim=1)
    ref = torch.sum(z0.double() * wr, dim=1, keepdim=True)
    assert torch.isnan(wr[0, :, 0, 1, 2, 0]).all() and wr[0, 1, 0, 0, 0, 0] == 0
    assert torch.equal(torch.isnan(w.cpu()), torch.isnan(wr)) and torch.equal(torch.isnan(out.cpu()), torch.isnan(ref))
    close(w, wr, atol=1e-6, rtol=1e-5)
    close(out, ref, atol=2e-6, rtol=1e-5)


@pytest.mark.parametrize('D', [1, 2, 15, 16, 17, 33])
@pytest.mark.parametrize('hw', [(1, 1), (3, 5), (4, 4), (1, 17)])
def test_column_softmax_saturated_vs_fp64(D, hw):
    from latentfusion_amd import ops
    shape = (2, 1, D) + hw
    g = torch.Generator().manual_seed(D * 10 + hw[1])
    l0 = _saturating_logits(shape, 2, g)
    lg = l0.to(DEV).requires_grad_(True)
    w, zd = ops.column_softmax(lg)
    lr = l0.double().requires_grad_(True)
    wr = torch.softmax(lr, dim=2)
    zr = (_depth_coord64(D) * wr).sum(dim=2)
    w32 = torch.softmax(l0, dim=2)
    close(w, wr, atol=1e-6, rtol=1e-5, what='column softmax weights', f32=w32)
    close(zd, zr, atol=2e-6, rtol=1e-5, what='column softmax expected depth',
          f32=(torch.linspace(-1.0, 1.0, D).view(1, 1, -1, 1, 1) * w32).sum(dim=2))
    a, b = torch.randn(shape, generator=g), torch.randn(zr.shape, generator=g)
    ((w * a.to(DEV)).sum() + (zd * b.to(DEV)).sum()).backward()
    ((wr * a.double()).sum() + (zr * b.double()).sum()).backward()
    assert torch.isfinite(lg.grad).all()
    close(lg.grad, lr.grad, atol=2e-6, rtol=1e-4, what='glogits')


def test_column_softmax_all_minus_inf_column_is_nan_as_torch():
    from latentfusion_amd import ops
    g = torch.Generator().manual_seed(6)
    l0 = torch.randn(2, 1, 17, 3, 5, generator=g) * 3
    l0[1, 0, :, 2, 4] = float('-inf')
    l0[0, 0, 3, 0, 0] = float('-inf')
    w, zd = ops.column_softmax(l0.to(DEV))
    wr = torch.softmax(l0.double(), dim=2)
    zr = (_depth_coord64(17) * wr).sum(dim=2)
    assert torch.isnan(wr[1, 0, :, 2, 4]).all() and torch.isnan(zr[1, 0, 2, 4]) and wr[0, 0, 3, 0, 0] == 0
    assert torch.equal(torch.isnan(w.cpu()), torch.isnan(wr)) and torch.equal(torch.isnan(zd.cpu()), torch.isnan(zr))
    close(w, wr, atol=1e-6, rtol=1e-5)
    close(zd, zr, atol=2e-6, rtol=1e-5)


def _head_inputs(N, D, P, g):
    """Dyadic records, weights, scale and bias: every logit (sum_c y w) * he + b is exact in fp32 whatever the order of the sum,
    so the fp64 logits ARE the kernel's and only the softmax is compared.  Logits spread over about +-100."""
    y = torch.randint(-40, 41, (N, D, P, 16), generator=g).float()
    w16 = torch.tensor([1.0, -1.0, 0.5, -0.5] * 4)[torch.randperm(16, generator=g)].contiguous()
    return y, w16, torch.tensor([0.25]), 0.5


@pytest.mark.parametrize('D', [1, 2, 15, 16, 17, 255, 256])
@pytest.mark.parametrize('P', [1, 15, 16, 17])
def test_column_softmax_head_vs_fp64(D, P):
    from latentfusion_amd import _lib
    L = _lib.lib()
    N = 2
    g = torch.Generator().manual_seed(D * 100 + P)
    y, w16, bias, he = _head_inputs(N, D, P, g)
    if D > 1:
        y[0, :, 0] = 0.0                                           # one column with one +80 among -80s
        y[0, :, 0, 0] = -160.5 / float(w16[0])
        y[0, D // 2, 0, 0] = 159.5 / float(w16[0])
    logits = (y.double() * w16.double()).sum(-1) * he + bias.double()            # (N, D, P)
    if D > 1:
        assert logits[0, D // 2, 0] == 80.0 and logits[0, 0, 0] == -80.0 and float(logits.abs().max()) > 60
    wr = torch.softmax(logits, dim=1)
    zr = (torch.linspace(-1.0, 1.0, D, dtype=torch.float64).view(1, D, 1) * wr).sum(dim=1)
    yd, wd, bd = y.to(DEV), w16.to(DEV), bias.to(DEV)
    for with_bias in (True, False):
        w = torch.full((N, D, P), 7.0, device=DEV)
        zd = torch.full((N, P), 7.0, device=DEV)
        assert L.lf_column_softmax_head_fwd(yd.data_ptr(), wd.data_ptr(), bd.data_ptr() if with_bias else None, he, w.data_ptr(),
                                            zd.data_ptr(), N, D, P, _s()) == 0
        close(w, wr, atol=2e-6, rtol=1e-5, what=f'head weights D={D} P={P}')         # (a bias common to the column cancels)
        close(zd, zr, atol=2e-6, rtol=1e-5, what=f'head expected depth D={D} P={P}')
    # weights only / expected depth only
    w2 = torch.empty(N, D, P, device=DEV)
    assert L.lf_column_softmax_head_fwd(yd.data_ptr(), wd.data_ptr(), bd.data_ptr(), he, w2.data_ptr(), None, N, D, P, _s()) == 0
    assert torch.equal(w2, w)


@pytest.mark.parametrize('D', [1, 2, 17, 255, 256])
def test_column_softmax_head_minus_inf_logits_as_torch(D):
    """The kernel keeps its logits in registers and fills the unused slots (and starts the running maximum) with -inf, so -inf
    DATA meets the sentinel: a column whose logits are all -inf gives NaN weights and NaN expected depth as torch.softmax does,
    a single -inf logit weighs exactly 0, and the columns next to them are untouched.  A logit is -inf through one channel at
    -inf under a positive weight (zeros in the record's other channels), or through a bias of -inf for the whole call."""
    from latentfusion_amd import _lib
    L = _lib.lib()
    N, P = 2, 17
    g = torch.Generator().manual_seed(D)
    y, w16, bias, he = _head_inputs(N, D, P, g)
    c = int((w16 > 0).nonzero()[0])

    def minus_inf(n, d, p):
        y[n, d, p] = 0.0
        y[n, d, p, c] = float('-inf')
    for d in range(D):
        minus_inf(0, d, 3)                                         # whole columns: in the middle of a 16-column group,
        minus_inf(1, d, 16)                                        # and the lone column of the second group
    minus_inf(0, D // 2, 5)                                        # one logit of a column
    minus_inf(1, D - 1, 0)
    logits = (y.double() * w16.double()).sum(-1) * he + bias.double()
    assert (logits[0, :, 3] == float('-inf')).all() and logits[0, D // 2, 5] == float('-inf') and not torch.isnan(logits).any()
    wr = torch.softmax(logits, dim=1)
    zr = (torch.linspace(-1.0, 1.0, D, dtype=torch.float64).view(1, D, 1) * wr).sum(dim=1)
    assert torch.isnan(wr[0, :, 3]).all() and torch.isnan(zr[1, 16]) and (D == 1 or wr[0, D // 2, 5] == 0)
    yd, wd, bd = y.to(DEV), w16.to(DEV), bias.to(DEV)
    w = torch.full((N, D, P), 7.0, device=DEV)
    zd = torch.full((N, P), 7.0, device=DEV)
    assert L.lf_column_softmax_head_fwd(yd.data_ptr(), wd.data_ptr(), bd.data_ptr(), he, w.data_ptr(), zd.data_ptr(), N, D, P, _s()) == 0
    assert torch.equal(torch.isnan(w.cpu()), torch.isnan(wr)) and torch.equal(torch.isnan(zd.cpu()), torch.isnan(zr))
    assert D == 1 or (w[0, D // 2, 5] == 0 and w[1, D - 1, 0] == 0)
    close(w, wr, atol=2e-6, rtol=1e-5, what=f'head weights with -inf D={D}')
    close(zd, zr, atol=2e-6, rtol=1e-5, what=f'head expected depth with -inf D={D}')
    # a bias of -inf: every logit of the call is -inf
    binf = torch.tensor([float('-inf')], device=DEV)
    y2 = _head_inputs(N, D, P, g)[0].to(DEV)
    assert L.lf_column_softmax_head_fwd(y2.data_ptr(), wd.data_ptr(), binf.data_ptr(), he, w.data_ptr(), zd.data_ptr(), N, D, P, _s()) == 0
    assert torch.isnan(w).all() and torch.isnan(zd).all()


def test_column_softmax_head_rejects_depth_257_before_any_launch():
    """D > 256 does not fit the kernel's registers; the entry point returns LF_EINVAL from its argument check on the host
    (csrc/reduce.hip, lf_column_softmax_head_fwd: the check precedes the launch), so the outputs are untouched."""
    from latentfusion_amd import _lib
    L = _lib.lib()
    N, D, P = 1, 257, 16
    y = torch.zeros(N, D, P, 16, device=DEV)
    w16 = torch.ones(16, device=DEV)
    w = torch.full((N, D, P), 7.0, device=DEV)
    zd = torch.full((N, P), 7.0, device=DEV)
    assert L.lf_column_softmax_head_fwd(y.data_ptr(), w16.data_ptr(), None, 1.0, w.data_ptr(), zd.data_ptr(), N, D, P, _s()) == LF_EINVAL
    assert L.lf_column_softmax_head_fwd(y.data_ptr(), w16.data_ptr(), None, 1.0, None, None, N, 16, P, _s()) == LF_EINVAL
    torch.cuda.synchronize()
    assert (w == 7.0).all() and (zd == 7.0).all()
    assert L.lf_column_softmax_head_fwd(y.data_ptr(), w16.data_ptr(), None, 1.0, w.data_ptr(), zd.data_ptr(), N, 256, P, _s()) == 0
    torch.cuda.synchronize()
    assert (w[:, :256] == 1.0 / 256).all()


# ---------------------------------------------------------------------------------------------------------------------------
# column sum / scale
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(2, 4, 5, 3, 3), (1, 12, 7, 5, 5), (1, 260, 3, 3, 3), (2, 4, 1, 3, 5), (1, 5, 1, 3, 3), (3, 12, 1, 1, 1),
                                   (1, 4, 37, 9, 9)])
def test_column_sum_edges_vs_fp64(shape):
    from latentfusion_amd import ops
    g = torch.Generator().manual_seed(sum(shape))
    x0 = torch.randn(shape, generator=g)
    wgt = torch.randn(shape[0], shape[1], shape[3], shape[4], generator=g)
    x = x0.to(DEV).requires_grad_(True)
    y = ops.column_sum(x)
    xr = x0.double().requires_grad_(True)
    ref = xr.sum(dim=2)
    close(y, ref, atol=2e-5, rtol=1e-5, what='column_sum', f32=x0.sum(dim=2))
    (y * wgt.to(DEV)).sum().backward()
    (ref * wgt.double()).sum().backward()
    close(x.grad, xr.grad, atol=0, rtol=0)


@pytest.mark.parametrize('shape', [(1, 4, 1, 3, 3), (2, 12, 3, 5, 3), (1, 260, 2, 3, 5), (1, 260, 1, 1, 1), (3, 4, 1, 1, 1), (1, 12, 1, 13, 7)])
def test_column_scale_edges_vs_fp64(shape):
    from latentfusion_amd import ops
    g = torch.Generator().manual_seed(sum(shape))
    z0 = torch.randn(shape, generator=g)
    w0 = torch.rand(shape[0], 1, *shape[2:], generator=g)
    z, w = z0.to(DEV).requires_grad_(True), w0.to(DEV).requires_grad_(True)
    out = ops.column_scale(z, w)
    zr, wr = z0.double().requires_grad_(True), w0.double().requires_grad_(True)
    ref = zr * wr
    close(out, ref.float(), atol=0, rtol=0)                        # one fp32 product per element: the rounded fp64 product
    a = torch.randn(shape, generator=g)
    (out * a.to(DEV)).sum().backward()
    (ref * a.double()).sum().backward()
    close(z.grad, zr.grad.float(), atol=0, rtol=0)
    close(w.grad, wr.grad, atol=2e-5, rtol=1e-5, what='column_scale gw', f32=(z0 * a).sum(dim=1, keepdim=True))
