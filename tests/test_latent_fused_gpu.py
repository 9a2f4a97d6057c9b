"""The fused latent term on the GPU: lf_latent_cosine_fwd / lf_latent_cosine_bwd_epi against fp64, and the engines' option
latent_kernel='fused' against 'autograd' and the module path.

YARDSTICK.  dist = 1 - torch.cosine_similarity(zp, zt, eps = 1e-8) over a row's h*w*C values and its autograd gradient at zp,
evaluated in fp64, then gp = Epi'(g_in + gscale * d(dist)/d(zp); zp, norm) through an fp64 restatement of lf_epilogue_bwd's
forms (`_reference`).  BOUNDS, the convention of tests/test_pose_loss_fp64_gpu.py: e32 = the error of the same torch
expressions run in fp32 on the same inputs; forward, per row: |hip - fp64| <= max(4 e32, 2e-6 + 2e-5 |fp64|); gradient, per row:
max |hip - fp64| <= max(4 max e32, 2e-3 of the row's largest component).  The same helpers must REJECT plausible misreadings
(test_comparison_rejects_a_wrong_reference).

The installed torch clamps the two norms in place outside the graph, so below the clamp (0 < |zp| < eps) the norm's own
derivative zp / |zp| still flows; the kernel follows that (and 0 at |zp| = 0), see include/lf_hip.h.

Measured errors per case are printed (`[latent] ...`, run with -s) and recorded in COVERAGE.md."""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
EPS = 1e-8
LRELU, PIXELNORM = 1, 2
HW = {(4, 1): (1, 1), (16, 15): (3, 5), (16, 256): (16, 16), (20, 33): (3, 11), (256, 16): (4, 4)}
SENTINEL = -777.25


def close(a, b, atol=1e-5, rtol=1e-4):
    torch.testing.assert_close(a.detach().cpu().contiguous(), b.detach().cpu().contiguous(), atol=atol, rtol=rtol)


def prod_camera(d, device=DEV):
    from latentfusion_amd.modules.geometry import Camera
    return Camera(d['K'].to(device), None, d['z_span'], d['viewport'].to(device), width=d['width'],
                  height=d['height'], log_quaternion=d['log_q'].to(device), translation=d['t'].to(device))


# ---------------------------------------------------------------------------------------------------------------------------
# inputs, the fp64 restatement, the comparison
# ---------------------------------------------------------------------------------------------------------------------------
def _inputs(C, P, N, seed=0, scale=1.0):
    """zp (channels-last), a correlated target code per row, a decoder gradient of the addend's size, PixelNorm factors."""
    h, w = HW[(C, P)]
    g = torch.Generator().manual_seed(1000 * C + 10 * P + N + seed)
    zp = scale * torch.randn(N, C, h, w, generator=g)
    zt = 0.3 * zp + scale * torch.randn(N, C, h, w, generator=g)
    g_in = torch.randn(N, C, h, w, generator=g) * (0.03 / (scale * P * C))      # (the size of gscale * d(dist)/d(zp) below)
    norm = 0.5 + torch.rand(N * h * w, generator=g)
    cl = lambda t: t.to(DEV).contiguous(memory_format=torch.channels_last)      # noqa: E731
    return cl(zp), zt.to(DEV), cl(g_in), norm.to(DEV)


def _layout(zt, layout):
    return zt.contiguous() if layout == 'nchw' else zt.contiguous(memory_format=torch.channels_last)


def _reference(zp, zt, g_in, norm, gscale, flags, dtype, variant=None):
    """(dist (N,), gp (N,C,h,w)) of the torch expressions in `dtype`; variant: one of the misreadings that must fail."""
    from latentfusion_amd import ops
    N, C, h, w = zp.shape
    z = zp.detach().to(dtype).contiguous().requires_grad_(True)
    t = zt.detach().to(dtype)
    if variant == 'other_layout':                                  # the NCHW-contiguous words read as channels-last
        t = t.contiguous().view(t.shape[0], h, w, C).permute(0, 3, 1, 2)
    t = t.expand(N, -1, -1, -1)
    zf, tf = z.reshape(N, -1), t.reshape(N, -1)
    if variant == 'eps_on_product':
        cos = (zf * tf).sum(1) / (zf.norm(dim=1) * tf.norm(dim=1) + EPS)
    else:
        cos = torch.cosine_similarity(zf, tf, 1, EPS)
    dist = cos if variant == 'no_one_minus' else 1.0 - cos
    (dd,) = torch.autograd.grad(dist.sum(), z)
    if variant == 'no_zp_term':
        ab = zf.detach().norm(dim=1).clamp_min(EPS) * tf.norm(dim=1).clamp_min(EPS)
        dd = -(t / ab.view(N, 1, 1, 1))
    gi = g_in.to(dtype) if g_in is not None else torch.zeros_like(dd)
    y = z.detach()
    x = gi + gscale * dd
    if flags & PIXELNORM:
        m = ((gi + dd if variant == 'gscale_after_mean' else x) * y).mean(dim=1, keepdim=True)
        x = (x - y * m) / norm.to(dtype).view(N, 1, h, w)
    if flags & LRELU:
        x = torch.where(y > 0, x, x * ops.SLOPE)
    return dist.detach(), x.detach()


def _kernels(zp, zt, g_in, norm, gscale, flags, inplace=False):
    from latentfusion_amd import ops
    sums = ops.latent_cosine_fwd(zp, zt)
    gi = g_in.clone(memory_format=torch.preserve_format) if g_in is not None else None
    gp = ops.latent_cosine_bwd_epi(gi, zp, norm, zt, sums, gscale, flags, out=gi if inplace else None)
    if inplace:
        assert gp is gi
    elif gi is not None:
        assert torch.equal(gi, g_in)                                # the out-of-place form leaves g_in alone
    return sums, gp


def _fwd_mismatches(tag, got, ref64, ref32, stats=None):
    got, ref32 = got.double(), ref32.double()
    err, e32 = (got - ref64).abs(), (ref32 - ref64).abs()
    bound = torch.maximum(4 * e32, 2e-6 + 2e-5 * ref64.abs())
    if stats is not None:
        stats['fwd'] = max(stats.get('fwd', 0.0), float(err.max()))
        stats['fwd32'] = max(stats.get('fwd32', 0.0), float(e32.max()))
    bad = ~(err <= bound)                                          # (a NaN fails)
    return [f'{tag}[{n}]: hip {got[n]:.9g} fp64 {ref64[n]:.9g} fp32 {ref32[n]:.9g}' for n in bad.nonzero().flatten().tolist()]


def _grad_mismatches(tag, got, ref64, ref32, stats=None):
    N = ref64.shape[0]
    got, ref64, ref32 = got.double().reshape(N, -1), ref64.reshape(N, -1), ref32.double().reshape(N, -1)
    err, e32, scale = (got - ref64).abs().amax(1), (ref32 - ref64).abs().amax(1), ref64.abs().amax(1)
    bound = torch.maximum(4 * e32, 2e-3 * scale)
    nz = scale > 0
    if stats is not None and nz.any():
        stats['grad'] = max(stats.get('grad', 0.0), float((err[nz] / scale[nz]).max()))
        stats['grad32'] = max(stats.get('grad32', 0.0), float((e32[nz] / scale[nz]).max()))
        stats['needs_4e32'] = stats.get('needs_4e32', False) or bool(((err > 2e-3 * scale) & (err <= bound)).any())
    bad = ~(err <= bound)
    return [f'{tag}[{n}]: err {err[n]:.3e} bound {bound[n]:.3e} (largest component {scale[n]:.3e}, fp32 err {e32[n]:.3e})'
            for n in bad.nonzero().flatten().tolist()]


def _check(tag, zp, zt, g_in, norm, gscale, flags, inplace=False, stats=None):
    """Mismatches of the two kernels against the fp64 yardstick on these inputs (logical NCHW views: the layout of zt is the
    kernel's business, the logical values are the reference's)."""
    sums, gp = _kernels(zp, zt, g_in, norm, gscale, flags, inplace)
    d64, g64 = _reference(zp, zt, g_in, norm, gscale, flags, torch.float64)
    d32, g32 = _reference(zp, zt, g_in, norm, gscale, flags, torch.float32)
    N = zp.shape[0]
    t = zt.expand(N, -1, -1, -1).double().reshape(N, -1)
    z = zp.double().reshape(N, -1)
    bad = _fwd_mismatches(tag + ' dist', sums[:, 3], d64, d32, stats)
    for j, (name, want) in enumerate((('dot', (z * t).sum(1)), ('zz', (z * z).sum(1)), ('tt', (t * t).sum(1)))):
        err = (sums[:, j].double() - want).abs()
        # (worst case of the kernel's fixed order: <= 16 fp32 additions in a lane, 8 in the workgroup's tree, 2 over its waves,
        # one rounding of the result = 27 u relative to the sum of magnitudes, u = 6e-8; the slices are summed in fp64)
        ok = err <= 2e-6 * ((z.abs() * t.abs()).sum(1) if j == 0 else want) + 1e-30
        bad += [f'{tag} sums[{n}][{name}] {sums[n, j]:.9g} fp64 {want[n]:.9g}' for n in (~ok).nonzero().flatten().tolist()]
    return bad + _grad_mismatches(tag + ' gp', gp, g64, g32, stats)


# ---------------------------------------------------------------------------------------------------------------------------
# kernels against fp64
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', [1, 7])
@pytest.mark.parametrize('C,P', sorted(HW))
def test_kernels_match_fp64(C, P, N):
    """Every (zt rows, zt layout, flags, g_in form) of a shape: forward and gradient within the bounds above."""
    from latentfusion_amd import ops
    zp, zt_full, g_in, norm = _inputs(C, P, N)
    gscale = 0.2 / 7
    bad, stats = [], {}
    for zt_n, layout, flags, gmode in itertools.product(sorted({1, N}), ('nchw', 'cl'), (0, 1, 2, 3), ('none', 'out', 'inplace')):
        zt = _layout(zt_full[:zt_n], layout)
        if P > 1:                                                  # the two layouts are two stride triples
            strides = ops._latent_args(zp, zt)[4]
            assert strides[1:] == ((1, P) if layout == 'nchw' else (C, 1)), (layout, strides)
            assert ops._latent_args(zp, zt)[3] is zt               # and neither is copied
        bad += _check(f'C{C} P{P} N{N} zt_n{zt_n} {layout} flags{flags} {gmode}', zp, zt, None if gmode == 'none' else g_in, norm,
                      gscale, flags, inplace=gmode == 'inplace', stats=stats)
    print(f"[latent] C={C} P={P} N={N}: dist err hip {stats['fwd']:.2e} (fp32 {stats['fwd32']:.2e});  gradient rel. to the row's "
          f"largest component hip {stats.get('grad', 0.0):.2e} (fp32 {stats.get('grad32', 0.0):.2e}), "
          f"needs 4*e32: {stats.get('needs_4e32', False)}")
    assert not bad, '\n'.join(bad[:20])


VARIANTS = ('no_one_minus', 'eps_on_product', 'no_zp_term', 'gscale_after_mean', 'other_layout')


@pytest.mark.parametrize('variant', VARIANTS)
def test_comparison_rejects_a_wrong_reference(variant):
    """The bounds mean something: the helpers that accept the kernels against the fp64 restatement reject them against each
    plausible misreading (evaluated in fp64 and, for its e32, in fp32), on inputs that expose it: for the eps rule rows of norm
    ~1e-4, where an eps added to the PRODUCT of the norms (1e-8) doubles the denominator while the clamp of each norm is far
    away; for the others values of order one, as a PixelNorm output has them."""
    C, P, N = 16, 15, 7
    zp, zt_full, g_in, norm = _inputs(C, P, N, seed=5, scale=1e-4 / (C * P) ** 0.5 if variant == 'eps_on_product' else 1.0)
    zt = zt_full.contiguous()
    gscale, flags = 0.2 / 7, LRELU | PIXELNORM
    assert not _check('true reference', zp, zt, g_in, norm, gscale, flags)
    sums, gp = _kernels(zp, zt, g_in, norm, gscale, flags)
    d64, g64 = _reference(zp, zt, g_in, norm, gscale, flags, torch.float64, variant)
    d32, g32 = _reference(zp, zt, g_in, norm, gscale, flags, torch.float32, variant)
    if variant in ('no_one_minus', 'eps_on_product', 'other_layout'):
        assert _fwd_mismatches(variant, sums[:, 3], d64, d32), f'{variant} passes the forward bound of the true reference'
    if variant in ('no_zp_term', 'gscale_after_mean', 'other_layout'):
        assert _grad_mismatches(variant, gp, g64, g32), f'{variant} passes the gradient bound of the true reference'


# ---------------------------------------------------------------------------------------------------------------------------
# edges
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('layout', ['nchw', 'cl'])
def test_zero_rows_and_a_nan_row(layout):
    C, P, N = 16, 256, 7
    zp, zt_full, g_in, norm = _inputs(C, P, N, seed=2)
    gscale, flags = 0.2 / 7, LRELU | PIXELNORM
    zp[1] = 0.0                                                   # all-zero projected latent: dist = 1, a = eps
    zt_full[2] = 0.0                                              # all-zero target code: dist = 1, no addend
    zp[4] *= 1e-10 / float(zp[4].norm())                          # 0 < |zp| < eps: the clamp acts on the value only
    zt = _layout(zt_full, layout)
    sums, gp = _kernels(zp, zt, g_in, norm, gscale, flags)
    assert sums[1, 3] == 1.0 and sums[2, 3] == 1.0
    assert torch.isfinite(sums).all() and torch.isfinite(gp).all()
    assert not _check('zero rows', zp, zt, g_in, norm, gscale, flags)
    # (zero target row: the gradient is the decoder's alone -- the epilogue backward of g_in, to rounding of the same formula)
    from latentfusion_amd import ops
    close(gp[2:3], ops._epilogue_bwd(g_in[2:3].contiguous(memory_format=torch.channels_last), zp[2:3], norm[2 * P:3 * P], flags),
          atol=1e-6 * float(gp[2].abs().max()), rtol=1e-5)
    # a NaN in one row stays in that row: every other row keeps its bits
    zq = zp.clone(memory_format=torch.preserve_format)
    zq[3, 5, 2, 7] = float('nan')
    s2, g2 = _kernels(zq, zt, g_in, norm, gscale, flags)
    keep = [i for i in range(N) if i != 3]
    assert torch.equal(s2[keep], sums[keep]) and torch.equal(g2[keep], gp[keep])
    assert torch.isnan(s2[3, 3]) and torch.isnan(g2[3]).all()
    zq = zp.clone(memory_format=torch.preserve_format)
    tq = zt.clone(memory_format=torch.preserve_format)
    tq[5, 0, 0, 0] = float('nan')
    s3, g3 = _kernels(zq, tq, g_in, norm, gscale, flags)
    keep = [i for i in range(N) if i != 5]
    assert torch.equal(s3[keep], sums[keep]) and torch.equal(g3[keep], gp[keep]) and torch.isnan(s3[5, 3])


def _raw_fwd(L, zp, zt, zt_n, strides, sums, losses, w, scratch, scratch_bytes, N, P, C):
    ptr = lambda t: t if isinstance(t, int) or t is None else t.data_ptr()      # noqa: E731
    return L.lf_latent_cosine_fwd(ptr(zp), ptr(zt), zt_n, *strides, ptr(sums), ptr(losses), w, ptr(scratch), scratch_bytes, N, P, C,
                                  torch.cuda.current_stream().cuda_stream)


def _raw_bwd(L, g_in, zp, norm, zt, zt_n, strides, sums, gscale, gp, N, P, C, flags):
    from latentfusion_amd import ops
    ptr = lambda t: t if isinstance(t, int) or t is None else t.data_ptr()      # noqa: E731
    return L.lf_latent_cosine_bwd_epi(ptr(g_in), ptr(zp), ptr(norm), ptr(zt), zt_n, *strides, ptr(sums), gscale, ptr(gp), N, P, C,
                                      flags, ops.SLOPE, torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize('C,P', [(16, 15), (20, 33), (256, 16)])
def test_sentinels_behind_every_output_stay_intact(C, P):
    """Raw calls on buffers with guard words on both sides of sums, losses, the scratch buffer and gp."""
    from latentfusion_amd import _lib
    L = _lib.lib()
    N, G = 7, 8
    zp, zt_full, g_in, norm = _inputs(C, P, N, seed=3)
    zt = zt_full.contiguous()
    strides = (C * P, 1, P)
    nb = L.lf_latent_cosine_scratch_bytes(N, P, C)
    guard = lambda n: torch.full((n + 2 * G,), SENTINEL, device=DEV)            # noqa: E731
    sums, losses, scratch, gp = guard(N * 4), guard(N * 8), guard(nb // 4), guard(N * P * C)
    losses[G:G + N * 8] = 0.5
    assert _raw_fwd(L, zp, zt, N, strides, sums[G:], losses[G:], 0.25, scratch[G:], nb, N, P, C) == 0
    assert _raw_bwd(L, g_in, zp, norm, zt, N, strides, sums[G:], 0.1, gp[G:], N, P, C, 3) == 0
    torch.cuda.synchronize()
    for name, buf, n in (('sums', sums, N * 4), ('losses', losses, N * 8), ('scratch', scratch, nb // 4), ('gp', gp, N * P * C)):
        assert (buf[:G] == SENTINEL).all() and (buf[G + n:] == SENTINEL).all(), name
    want_s, want_g = _kernels(zp, zt, g_in, norm, 0.1, 3)
    assert torch.equal(sums[G:G + N * 4].view(N, 4), want_s)
    assert torch.equal(gp[G:G + N * P * C], want_g.permute(0, 2, 3, 1).reshape(-1))
    ls = losses[G:G + N * 8].view(N, 8)
    assert torch.equal(ls[:, 5], want_s[:, 3]) and torch.equal(ls[:, [0, 1, 2, 3, 6, 7]], torch.full((N, 6), 0.5, device=DEV))
    close(ls[:, 4], 0.5 + 0.25 * want_s[:, 3], atol=1e-7, rtol=1e-6)


# ---------------------------------------------------------------------------------------------------------------------------
# determinism: run to run, and a row's bits never follow the batch
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('zt_rows', ['one', 'per_row'])
@pytest.mark.parametrize('C,P', [(16, 256), (20, 33), (256, 16)])
def test_rows_are_bit_identical_alone_and_in_the_batch(C, P, zt_rows):
    N = 7
    zp, zt_full, g_in, norm = _inputs(C, P, N, seed=4)
    zt = zt_full[:1].contiguous() if zt_rows == 'one' else zt_full.contiguous()
    gscale, flags = 0.2 / 7, LRELU | PIXELNORM
    sums, gp = _kernels(zp, zt, g_in, norm, gscale, flags)
    again = _kernels(zp, zt, g_in, norm, gscale, flags)
    assert torch.equal(again[0], sums) and torch.equal(again[1], gp)
    sub = lambda t, r: t[r].contiguous(memory_format=torch.channels_last)       # noqa: E731
    for r in [slice(i, i + 1) for i in range(N)] + [slice(3, 6)]:
        zr = zt if zt_rows == 'one' else zt[r]
        s1, g1 = _kernels(sub(zp, r), zr, sub(g_in, r), norm[r.start * P:r.stop * P], gscale, flags)
        assert torch.equal(s1, sums[r]) and torch.equal(g1, gp[r]), r


# ---------------------------------------------------------------------------------------------------------------------------
# ABI: rejected arguments launch nothing and write nothing
# ---------------------------------------------------------------------------------------------------------------------------
def test_rejected_arguments_leave_the_outputs_untouched():
    from latentfusion_amd import _lib
    L = _lib.lib()
    EINVAL, EALIGN, ENOSPC = -1, -2, -3
    N, C, P = 3, 16, 15
    zp, zt_full, g_in, norm = _inputs(C, P, N, seed=6)
    zt = zt_full.contiguous()
    st = (C * P, 1, P)
    nb = L.lf_latent_cosine_scratch_bytes(N, P, C)
    assert nb == N * 16
    fresh = lambda n: torch.full((n,), SENTINEL, device=DEV)                    # noqa: E731
    sums, losses, scratch, gp = fresh(N * 4 + 4), fresh(N * 8), fresh(nb // 4 + 4), fresh(N * P * C + 4)
    good_sums = _kernels(zp, zt, g_in, norm, 0.1, 3)[0]
    fwd = dict(zp=zp, zt=zt, zt_n=N, strides=st, sums=sums, losses=losses, w=0.25, scratch=scratch, scratch_bytes=nb, N=N, P=P, C=C)
    fwd_cases = [
        (EINVAL, dict(N=0)), (EINVAL, dict(N=-1)), (EINVAL, dict(P=0)), (EINVAL, dict(C=0)), (EINVAL, dict(C=2)), (EINVAL, dict(C=260)),
        (EALIGN, dict(C=6)), (EALIGN, dict(C=18)), (EINVAL, dict(zt_n=2)), (EINVAL, dict(zt_n=0)),
        (EINVAL, dict(strides=(-1, 1, P))), (EINVAL, dict(strides=(C * P, -1, P))), (EINVAL, dict(strides=(C * P, 1, -P))),
        (EINVAL, dict(zp=None)), (EINVAL, dict(zt=None)), (EINVAL, dict(sums=None)),
        (EALIGN, dict(zp=zp.data_ptr() + 4)), (EALIGN, dict(sums=sums.data_ptr() + 4)), (EALIGN, dict(scratch=scratch.data_ptr() + 4)),
        (ENOSPC, dict(scratch_bytes=nb - 4)), (ENOSPC, dict(scratch_bytes=0)), (ENOSPC, dict(scratch=None)),
    ]
    for want, change in fwd_cases:
        assert _raw_fwd(L, **dict(fwd, **change)) == want, change
    bwd = dict(g_in=g_in, zp=zp, norm=norm, zt=zt, zt_n=N, strides=st, sums=good_sums, gscale=0.1, gp=gp, N=N, P=P, C=C, flags=3)
    bwd_cases = [
        (EINVAL, dict(N=0)), (EINVAL, dict(P=0)), (EINVAL, dict(C=0)), (EINVAL, dict(C=2)), (EINVAL, dict(C=260)), (EALIGN, dict(C=6)),
        (EINVAL, dict(zt_n=2)), (EINVAL, dict(strides=(C * P, 1, -P))), (EINVAL, dict(zp=None)), (EINVAL, dict(zt=None)),
        (EINVAL, dict(sums=None)), (EINVAL, dict(gp=None)), (EINVAL, dict(flags=4)), (EINVAL, dict(flags=8 | 3)),
        (EINVAL, dict(norm=None)), (EINVAL, dict(norm=None, flags=2)),
        (EALIGN, dict(zp=zp.data_ptr() + 4)), (EALIGN, dict(gp=gp.data_ptr() + 4)), (EALIGN, dict(g_in=g_in.data_ptr() + 4)),
        (EALIGN, dict(sums=good_sums.data_ptr() + 4)),
    ]
    for want, change in bwd_cases:
        assert _raw_bwd(L, **dict(bwd, **change)) == want, change
    torch.cuda.synchronize()
    for name, buf in (('sums', sums), ('losses', losses), ('scratch', scratch), ('gp', gp)):
        assert (buf == SENTINEL).all(), name
    # the controls: the unchanged argument sets are accepted (norm may be NULL without LF_EPI_PIXELNORM; zt may sit anywhere)
    assert _raw_fwd(L, **fwd) == 0 and _raw_bwd(L, **bwd) == 0
    assert _raw_bwd(L, **dict(bwd, norm=None, flags=1)) == 0 and _raw_bwd(L, **dict(bwd, g_in=None)) == 0
    torch.cuda.synchronize()
    assert torch.equal(sums[:N * 4].view(N, 4), good_sums)
    # the ops wrappers turn a refusal into an error
    from latentfusion_amd import ops
    with pytest.raises(ValueError):
        ops.latent_cosine_fwd(zp, zt[:2])
    with pytest.raises(_lib.LFHipError, match='LF_EALIGN'):
        ops.latent_cosine_fwd(zp[:, :6].contiguous(memory_format=torch.channels_last), zt[:, :6])


# ---------------------------------------------------------------------------------------------------------------------------
# the engines
# ---------------------------------------------------------------------------------------------------------------------------
def _aten_calls(fn):
    """Names of the ATen operators dispatched while fn() runs."""
    from torch.utils._python_dispatch import TorchDispatchMode
    names = []

    class Rec(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            names.append(str(func))
            return func(*args, **(kwargs or {}))
    with Rec():
        out = fn()
    return out, names


def _launches(fn):
    """{entry point: launches} of liblf_hip.so while fn() runs (counted by _lib.check)."""
    from latentfusion_amd import _lib
    _lib.BYTE_LOG = {}
    try:
        out = fn()
        torch.cuda.synchronize()
        return out, {k: v[0] for k, v in _lib.BYTE_LOG.items()}
    finally:
        _lib.BYTE_LOG = None


_G12 = {}


def _g12(golden):
    """The setup of tests/test_engine_gpu.py::test_engine_latent_term_matches_module_path and its module-path results,
    computed once for the tests below (nothing here is modified afterwards)."""
    if _G12:
        return _G12
    from latentfusion_amd.observation import Observation
    from latentfusion_amd.pose import estimation
    from latentfusion_amd.recon import fusion
    from latentfusion_amd.recon.inference import LatentFusionModel
    from latentfusion_amd.recon.models import Photographer, Sculptor
    g = golden('g12_latent_code')
    model = LatentFusionModel(Sculptor.from_checkpoint(g['sculptor']), fusion.from_checkpoint(g['fuser']),
                              Photographer.from_checkpoint(g['photographer']), g['camera_dist'], DEV)
    tg = g['target']
    target = Observation(tg['color_u8'].float() / 255.0, tg['depth'], tg['mask'].float(), prod_camera(tg['cam'], 'cpu')).to(DEV)
    z_obj = g['z_obj'].to(DEV)
    cam0 = prod_camera(g['cams'])
    weights = {'depth': 1.0, 'ov_depth': 0.3, 'iou': 0.0, 'mask': 0.0, 'latent': 0.2}
    kw = dict(model=model, learning_rate=0.01, num_samples=len(cam0), num_iters=3, ranking_size=len(cam0), converge_threshold=1e-9,
              converge_patience=100, optimizer='adam', loss_weights=weights, return_camera_history=True)
    ref = estimation.GradientPoseEstimator(use_engine=False, **kw)
    with model.frozen():
        st = ref.start(z_obj, target, cam0)
        with torch.no_grad():
            zt = model.compute_latent_code(target, st['cam'])
        ld, _, rank, _ = ref.loss_and_grad(z_obj, target, st['cam'], 0, zt)
        want_g = torch.cat((st['cam'].log_quaternion.grad, st['cam'].translation.grad, st['cam'].viewport.grad), dim=1)
    _G12.update(g=g, model=model, target=target, z_obj=z_obj, weights=weights, kw=kw, ref=ref, zt=zt.detach(),
                ld={k: v.detach() for k, v in ld.items()}, rank=rank.detach(), want_g=want_g.detach().clone())
    return _G12


def _g12_engine_call(S, latent_kernel, need_grad=True, **extra):
    """(engine, losses, gparams) of a GradientPoseEstimator's engine on the fixture's hypotheses."""
    from latentfusion_amd.pose import estimation
    kw = dict(S['kw'], **extra)
    if latent_kernel != 'absent':
        kw['latent_kernel'] = latent_kernel
    with S['model'].frozen():
        est = estimation.GradientPoseEstimator(**kw)
        st = est.start(S['z_obj'], S['target'], prod_camera(S['g']['cams']))
        assert 'engine' in st and st['engine'].w_latent == 0.2
        losses, gparams = st['engine'].forward_backward(st['cam'], need_grad=need_grad, z_target_latent=S['zt'])
    return st['engine'], st['cam'], losses, gparams


def _assert_follows(losses, gparams, ld, rank, want_g):
    """The assertions and bounds of test_engine_latent_term_matches_module_path."""
    for i, k in enumerate(('depth', 'ov_depth', 'iou', 'mask')):
        close(losses[:, i], ld[k], atol=5e-6, rtol=1e-4)
    close(losses[:, 5], ld['latent'], atol=2e-6, rtol=1e-4)
    close(losses[:, 4], rank, atol=5e-6, rtol=1e-4)
    rel = ((gparams - want_g).norm(dim=1) / want_g.norm(dim=1)).max().item()
    assert rel < 5e-3, rel
    return rel


def test_g12_engine_fused_matches_module_path_and_autograd(golden):
    S = _g12(golden)
    eng_f, _, lf, gf = _g12_engine_call(S, 'fused')
    eng_a, _, la, ga = _g12_engine_call(S, 'autograd')
    eng_0, _, l0, g0 = _g12_engine_call(S, 'absent')
    assert (eng_f.latent_kernel, eng_a.latent_kernel, eng_0.latent_kernel) == ('fused', 'autograd', 'autograd')
    # 'autograd' is what an engine constructed without the argument runs: bit for bit
    assert torch.equal(la, l0) and torch.equal(ga, g0)
    rel_mod = _assert_follows(lf, gf, S['ld'], S['rank'], S['want_g'])
    # 'fused' against 'autograd' on the same engine inputs, same bounds
    ld_a = {k: la[:, i] for i, k in enumerate(('depth', 'ov_depth', 'iou', 'mask'))}
    ld_a['latent'] = la[:, 5]
    rel_auto = _assert_follows(lf, gf, ld_a, la[:, 4], ga)
    print(f'[latent] g12 engine: camera-gradient rel-L2 fused vs module path {rel_mod:.2e}, fused vs autograd {rel_auto:.2e}')
    assert float(lf[:, 5].abs().min()) > 0 and torch.equal(lf[:, 6:], torch.zeros_like(lf[:, 6:]))
    # deterministic
    _, _, lf2, gf2 = _g12_engine_call(S, 'fused')
    assert torch.equal(lf2, lf) and torch.equal(gf2, gf)


def test_g12_fused_gradient_call_keeps_the_explicit_path(golden):
    """With 'fused' a gradient call with a latent term is the explicit iteration plus two entry points: the explicit decoder
    (no autograd graph on the logits), the two-launch loss, and no ATen cosine chain."""
    from latentfusion_amd import ops
    S = _g12(golden)
    eng, cam, _, _ = _g12_engine_call(S, 'fused')
    assert eng.dec is not None, 'the fixture has a plain 2-D decoder: the explicit path exists'
    seen = {}
    inner = eng._decoder_fwd

    def decoder_fwd(*a):
        out = inner(*a)
        seen['logits'] = out[2]
        return out

    def never(name):
        def f(*a, **k):
            raise AssertionError(f'{name} ran on the fused path')
        return f
    eng._decoder_fwd = decoder_fwd
    eng._decoder_autograd, eng._loss_autograd, eng._latent_distance = never('_decoder_autograd'), never('_loss_autograd'), never('_latent_distance')
    ops.KERNEL_TIMER = []
    try:
        with S['model'].frozen():
            ((out, names), counts) = _launches(lambda: _aten_calls(lambda: eng.forward_backward(cam, z_target_latent=S['zt'])))
        tags = [str(n) for n, _, _ in ops.KERNEL_TIMER]
    finally:
        ops.KERNEL_TIMER = None
    assert not seen['logits'].requires_grad and seen['logits'].grad_fn is None
    for tag in ('resample_fwd', 'resample_bwd_coef'):
        assert tag in tags, (tag, tags)
    assert [t for t in tags if t.startswith('conv3x3_2d_')], tags          # the explicit decoder's launches, forward and back
    assert tags.count('latent_cosine_fwd') == 1 and tags.count('latent_cosine_bwd_epi') == 1
    chain = lambda ns: [n for n in ns if 'cosine_similarity' in n or 'linalg_vector_norm' in n]      # noqa: E731
    assert not chain(names), chain(names)
    assert counts.get('lf_latent_cosine_fwd') == 1 and counts.get('lf_latent_cosine_bwd_epi') == 1
    assert counts.get('lf_pose_loss_fwd') == 1 and counts.get('lf_pose_loss_bwd') == 1
    # the same launches as the iteration WITHOUT a latent term (explicit decoder, fused epilogue backward) plus the two
    eng.set_weights(dict(S['weights'], latent=0.0))
    with S['model'].frozen():
        (_, plain) = _launches(lambda: eng.forward_backward(cam))
    eng.set_weights(S['weights'])
    assert 'lf_latent_cosine_fwd' not in plain
    assert {k: v for k, v in counts.items() if 'latent_cosine' not in k} == plain
    # the control: the recorder does see the chain on the 'autograd' engine, and that path builds a graph
    eng_a, cam_a, _, _ = _g12_engine_call(S, 'autograd')
    with S['model'].frozen():
        ((_, names_a), counts_a) = _launches(lambda: _aten_calls(lambda: eng_a.forward_backward(cam_a, z_target_latent=S['zt'])))
    assert chain(names_a) and 'lf_latent_cosine_fwd' not in counts_a
    # ranking call: the distance is the kernel's, no ATen chain either
    with S['model'].frozen(), torch.no_grad():
        ((lr, _), names_r), counts_r = _launches(lambda: _aten_calls(
            lambda: eng.forward_backward(cam, need_grad=False, z_target_latent=S['zt'])))
        la_r, _ = eng_a.forward_backward(cam_a, need_grad=False, z_target_latent=S['zt'])
    assert not chain(names_r) and counts_r.get('lf_latent_cosine_fwd') == 1 and 'lf_latent_cosine_bwd_epi' not in counts_r
    close(lr[:, 5], la_r[:, 5], atol=2e-6, rtol=1e-4)
    close(lr[:, 4], la_r[:, 4], atol=5e-6, rtol=1e-4)
    assert torch.equal(lr[:, :4], la_r[:, :4])


def test_g12_generic_decoder_branch_takes_the_fused_term(golden):
    """EXPLICIT_DECODER off (the route of a decoder the engine does not sequence, e.g. the released architecture): autograd only
    carries d(logits) back to the projected latent; the loss is the two launches and the latent term the two new kernels."""
    from latentfusion_amd.engine import RenderLoopEngine
    S = _g12(golden)
    old = RenderLoopEngine.EXPLICIT_DECODER
    RenderLoopEngine.EXPLICIT_DECODER = False
    try:
        eng, cam, lf, gf = _g12_engine_call(S, 'fused')
        assert eng.dec is None
        eng._loss_autograd = eng._latent_distance = None          # (calling either would raise)
        with S['model'].frozen():
            ((lf2, gf2), counts) = _launches(lambda: eng.forward_backward(cam, z_target_latent=S['zt']))
    finally:
        RenderLoopEngine.EXPLICIT_DECODER = old
    assert torch.equal(lf2, lf) and torch.equal(gf2, gf)
    assert counts.get('lf_latent_cosine_fwd') == 1 and counts.get('lf_latent_cosine_bwd_epi') == 1
    assert counts.get('lf_pose_loss_fwd') == 1 and counts.get('lf_pose_loss_bwd') == 1
    _assert_follows(lf, gf, S['ld'], S['rank'], S['want_g'])


def test_g12_estimators_with_the_fused_term(golden):
    from latentfusion_amd.pose import estimation
    S = _g12(golden)
    g, model, target, z_obj = S['g'], S['model'], S['target'], S['z_obj']
    a, ha = S['ref'].estimate(z_obj, target, camera=prod_camera(g['cams']))
    est = estimation.GradientPoseEstimator(latent_kernel='fused', **S['kw'])
    b, hb = est.estimate(z_obj, target, camera=prod_camera(g['cams']))
    la, lb = torch.stack([h[0] for h in ha]), torch.stack([h[0] for h in hb])
    close(lb[0], la[0], atol=5e-6, rtol=1e-4)
    close(lb, la, atol=0.0, rtol=2e-2)
    # ranking: CrossEntropyPoseEstimator.evaluate_samples with a latent weight, 'fused' against 'autograd'
    n = len(prod_camera(g['cams']))
    kw = dict(model=model, num_samples=n, num_elites=2, num_iters=1, num_gmm_components=2, learning_rate=0.9, sample_flipped=False,
              ranking_size=2, loss_weights=S['weights'])
    out = {}
    for k in ('fused', 'autograd'):
        ce = estimation.CrossEntropyPoseEstimator(latent_kernel=k, **kw)
        out[k] = ce.evaluate_samples(z_obj, target, prod_camera(g['cams']))[1]
        assert ce.last_scored_on_engine and ce._engine_cache[2].latent_kernel == k
    close(out['fused'], out['autograd'])
    assert torch.equal(torch.argsort(out['fused']), torch.argsort(out['autograd']))


def test_sum_tail_leaves_the_option_idle(golden):
    """A tail without a PixelNorm buffer (the 'sum' projection): 'fused' runs the existing path, bit for bit."""
    from latentfusion_amd.engine import RenderLoopEngine
    from latentfusion_amd.observation import Observation
    from latentfusion_amd.recon.models import Photographer
    r, t7 = golden('g5_decode')['sum'], golden('g7_adam_trace')
    ph = Photographer.from_checkpoint(r['ck']).to(DEV)
    for p in ph.parameters():
        p.requires_grad_(False)
    tg = t7['target']
    target = Observation(None, tg['depth'], tg['mask'].float(), prod_camera(tg['cam'], 'cpu')).to(DEV)
    weights = {'depth': 1.0, 'ov_depth': 0.3, 'iou': 0.2, 'mask': 0.4, 'latent': 0.3}
    cam0 = prod_camera(r['cam'])
    engs = {k: RenderLoopEngine(ph, r['z_obj'].to(DEV), target, weights, latent_kernel=k) for k in ('fused', 'autograd')}
    shape = {}
    inner = engs['fused']._tail_fwd

    def tail_fwd(*a):
        tail = inner(*a)
        shape['zp'], shape['pnorm'] = tuple(tail.zp.shape), tail.pnorm
        return tail
    engs['fused']._tail_fwd = tail_fwd
    with pytest.raises(ValueError):
        engs['fused'].forward_backward(cam0, need_grad=False)       # (a latent weight without a code is still an error)
    engs['fused'].set_weights(dict(weights, latent=0.0))
    engs['fused'].forward_backward(cam0, need_grad=False)           # (the shape of this tail's latent)
    engs['fused'].set_weights(weights)
    assert shape['pnorm'] is None
    zt = torch.randn(1, *shape['zp'][1:], generator=torch.Generator().manual_seed(3)).to(DEV)
    from latentfusion_amd import _lib
    for need_grad in (True, False):
        (lf, gf), counts = _launches(lambda: engs['fused'].forward_backward(cam0, need_grad=need_grad, z_target_latent=zt))
        la, ga = engs['autograd'].forward_backward(cam0, need_grad=need_grad, z_target_latent=zt)
        assert torch.equal(lf, la) and float(lf[:, 5].abs().min()) > 0
        assert (gf is None and ga is None) or torch.equal(gf, ga)
        assert not [k for k in counts if 'latent_cosine' in k]
    assert _lib.BYTE_LOG is None


# ---------------------------------------------------------------------------------------------------------------------------
# several targets
# ---------------------------------------------------------------------------------------------------------------------------
def _shifted(target, dy, dx):
    from latentfusion_amd.observation import Observation
    return Observation(torch.roll(target.color, (dy, dx), (-2, -1)).contiguous(),
                       torch.roll(target.depth, (dy, dx), (-2, -1)).contiguous(),
                       torch.roll(target.mask, (dy, dx), (-2, -1)).contiguous(), target.camera.clone())


def _syn(fuser='pool:mean'):
    from latentfusion_amd import synth
    from latentfusion_amd.pose import estimation, utils as pu
    model, _ = synth.build_model(32, 16, fuser, seed=4, device=DEV, bias_std=0.05)
    tg0 = synth.make_observation(1, 5, 'cpu')
    targets = [_shifted(tg0, 0, 0), _shifted(tg0, 9, -14), _shifted(tg0, -7, 11)]
    z_obj = torch.randn(1, 1, 16, 32, 32, 32, generator=torch.Generator().manual_seed(9)).to(DEV)
    cams = []
    for t, tg in enumerate(targets):
        c = pu.sample_cameras_with_estimate(4, estimation.PoseEstimator.initial_pose(tg))
        g = torch.Generator().manual_seed(70 + t)
        cams.append(c._like(log_quaternion=c.log_quaternion + 0.05 * torch.randn(c.log_quaternion.shape, generator=g)))
    return model, z_obj, targets, cams


@pytest.mark.parametrize('codes', ['per_target', 'per_row'])
def test_multi_target_engine_is_bit_identical_per_target(codes):
    """T = 3 targets x n = 4 hypotheses under 'fused': ONE lf_latent_cosine_fwd over the 12 rows, and per target the losses and
    camera gradients of RenderLoopEngine(latent_kernel='fused') on that target alone, bit for bit (gradient and ranking call)."""
    from latentfusion_amd.engine import RenderLoopEngine
    from latentfusion_amd.engine_multi import MultiTargetEngine
    from latentfusion_amd.modules.geometry import Camera
    model, z_obj, targets, cams = _syn()
    model.freeze()
    T, n = 3, 4
    weights = {'depth': 1.0, 'ov_depth': 0.3, 'iou': 0.2, 'mask': 0.4, 'latent': 0.2}
    dev_targets = [t.to(DEV) for t in targets]
    zoomed = [c.zoom(None, model.input_size, model.camera_dist).to(DEV) for c in cams]
    eng = MultiTargetEngine(model.photographer, z_obj, dev_targets, weights, latent_kernel='fused')
    assert eng.latent_kernel == 'fused' and eng.dec is not None
    cout, S = eng.proj[0].shape[0], eng.S
    rows = T if codes == 'per_target' else T * n
    zt = torch.randn(rows, cout, S, S, generator=torch.Generator().manual_seed(11)).to(DEV)
    allc = Camera.cat(zoomed)
    for need_grad in (True, False):
        (lm, gm), counts = _launches(lambda: eng.forward_backward(allc, n, need_grad=need_grad, z_target_latent=zt))
        assert counts.get('lf_latent_cosine_fwd') == 1 and counts.get('lf_latent_cosine_bwd_epi', 0) == int(need_grad)
        for t in range(T):
            one = RenderLoopEngine(model.photographer, z_obj, dev_targets[t], weights, latent_kernel='fused')
            z1 = zt[t:t + 1] if codes == 'per_target' else zt[t * n:(t + 1) * n]
            l1, g1 = one.forward_backward(zoomed[t], need_grad=need_grad, z_target_latent=z1)
            r = slice(t * n, (t + 1) * n)
            assert torch.equal(lm[r], l1), (t, need_grad)
            assert float(l1[:, 5].abs().min()) > 0
            if need_grad:
                assert torch.equal(gm[r], g1), t
        # against the per-target ATen chain of 'autograd': within the single-target bounds
        ea = MultiTargetEngine(model.photographer, z_obj, dev_targets, weights)
        la, ga = ea.forward_backward(allc, n, need_grad=need_grad, z_target_latent=zt)
        close(lm[:, 5], la[:, 5], atol=2e-6, rtol=1e-4)
        close(lm[:, 4], la[:, 4], atol=5e-6, rtol=1e-4)
        if need_grad:
            assert ((gm - ga).norm(dim=1) / ga.norm(dim=1)).max().item() < 5e-3


def test_estimate_batch_equals_sequential_estimates_with_the_fused_term():
    from latentfusion_amd.pose import estimation
    model, z_obj, targets, cams = _syn('gru')
    w = {'depth': 1.0, 'ov_depth': 0.3, 'iou': 0.0, 'mask': 0.0, 'latent': 0.2}
    est = estimation.GradientPoseEstimator(model=model, learning_rate=0.01, num_samples=4, num_iters=4, ranking_size=3,
                                           converge_threshold=-1.0, converge_patience=1, optimizer='adam', loss_weights=w,
                                           track_stats=True, return_camera_history=True, latent_kernel='fused')
    want = [est.estimate(z_obj, t, camera=c.clone()) for t, c in zip(targets, cams)]
    got = est.estimate_batch(z_obj, targets, cameras=[c.clone() for c in cams])
    assert 'latent_loss' in want[0][1]
    for (best_g, stats_g, hist_g), (best_w, stats_w, hist_w) in zip(got, want):
        for f in ('log_quaternion', 'translation', 'viewport', 'intrinsic'):
            assert torch.equal(getattr(best_g, f), getattr(best_w, f)), f
        assert set(stats_g) == set(stats_w)
        for k in stats_w:
            assert torch.equal(stats_g[k], stats_w[k]), k
        assert len(hist_g) == len(hist_w)
        for (rg, cg), (rw, cw) in zip(hist_g, hist_w):
            assert torch.equal(rg, rw)
            assert torch.equal(cg.log_quaternion, cw.log_quaternion) and torch.equal(cg.translation, cw.translation)
