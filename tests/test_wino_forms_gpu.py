"""The compile-time epilogue forms of the fp32 Winograd 16-channel kernels (csrc/conv_wino.hip, WF_*; lf_set_tuning key 8 = 1, the
default) against the generic kernels they were cut from (key 8 = 0).  The forms' epilogue arithmetic (wino_epi_*) spells out the
roundings the generic kernels are compiled to, operation for operation, so every output must be the same bit pattern --
compared as int32, which also holds the signs and payloads of NaNs to account.  Calls that match no
form must run the generic kernel under either value: the selector may never hand a call to a form that ignores one of its
arguments."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'

# tile = 2 x 8 x 16 (z, y, x): exactly one tile; interior tiles plus edge tiles, with the z slide and a change of column; sides
# that are no multiple of the tile (partial tiles on every axis)
SHAPES = [(2, 2, 8, 16), (2, 6, 24, 48), (2, 5, 9, 33)]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b, what, min_finite=0.5):
    assert torch.equal(_bits(a), _bits(b)), f'{what}: {(_bits(a) != _bits(b)).sum().item()} of {a.numel()} bit patterns differ'
    assert torch.isfinite(a).float().mean().item() >= min_finite, f'{what}: too few finite outputs for the comparison to mean much'


def _both(fn, key=8):
    """fn() under value 0 of the key, then under value 1 (the default of keys 7 and 8); the switch is restored."""
    from latentfusion_amd import _lib
    L = _lib.lib()
    prev = L.lf_set_tuning(key, 0)
    try:
        assert prev == 1, 'value 1 is the default'
        old = fn()
        assert L.lf_set_tuning(key, 1) == 0
        new = fn()
        torch.cuda.synchronize()
    finally:
        L.lf_set_tuning(key, prev)
    return old, new


def _problem(shape, seed, special):
    """The recipe of tests/test_wino_packed_gpu.py: PixelNorm-range data (unit RMS over the channels) with a few exact zeros;
    `special`: also NaNs and infinities of both signs in the data AND in the weights."""
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


def _prev_layer(shape):
    """A finite previous layer for the fused backward: its saved activation and PixelNorm denominators."""
    from latentfusion_amd import ops
    from latentfusion_amd._lib import LF_EPI_LRELU, LF_EPI_PIXELNORM
    xf, wf, _, _, _, hef = _problem(shape, 4, False)
    return ops.conv3d_c16_wino(xf, ops.pack_conv3d_c16_wino(wf), None, hef, LF_EPI_LRELU | LF_EPI_PIXELNORM)


def _three_forms(shape, special):
    """The three calls of the render loop, each of which matches a fixed form: forward block, data gradient with the previous
    layer's backward folded in, plain data gradient.  Returns a function that makes them and the names of its outputs."""
    from latentfusion_amd import ops
    from latentfusion_amd._lib import LF_EPI_LRELU, LF_EPI_PIXELNORM
    x, w, b, _, _, he = _problem(shape, 3, special)
    up, upt = ops.pack_conv3d_c16_wino(w), ops.pack_conv3d_c16_wino(w, transpose=True)
    full = LF_EPI_LRELU | LF_EPI_PIXELNORM
    act, nrm = _prev_layer(shape)

    def run():
        y, n = ops.conv3d_c16_wino(x, up, b, he, full)
        gprev = ops.conv3d_c16_wino(x, upt, None, he, 0, prev=(act, nrm, full))[0]
        gplain = ops.conv3d_c16_wino(x, upt, None, he, 0)[0]
        return y, n, gprev, gplain

    return run, ('forward y', 'forward norm_out', 'data gradient + previous layer', 'plain data gradient')


@pytest.mark.parametrize('special', [False, True])
@pytest.mark.parametrize('shape', SHAPES)
def test_three_forms_bit_identical(shape, special):
    """With special values PixelNorm and its derivative take the NaN weight's channel to every channel (no finite outputs
    left to count); the plain data gradient keeps the other 15 channels."""
    run, names = _three_forms(shape, special)
    old, new = _both(run)
    for name, a, c in zip(names, old, new):
        _same(c, a, f'{name} of {shape}', min_finite=0.5 if (not special or name == names[3]) else 0.0)


@pytest.mark.parametrize('special', [False, True])
@pytest.mark.parametrize('shape', SHAPES)
def test_projfwd_form_bit_identical(shape, special):
    """The forward block form with the factor projection riding on it: y, norm_out, the projected image zp and pnorm."""
    from latentfusion_amd import ops
    from latentfusion_amd._lib import LF_EPI_LRELU, LF_EPI_PIXELNORM
    N, D, H, W = shape
    x, w, b, wp, pb, he = _problem(shape, 5, special)
    up, wA, phe = ops.pack_conv3d_c16_wino(w), ops.pack_wino_proj(_proj_matrix(wp, D)), ops.he_constant(wp)
    flags = LF_EPI_LRELU | LF_EPI_PIXELNORM
    old, new = _both(lambda: ops.conv3d_c16_wino_projfwd(x, up, b, he, flags, wA, pb, phe, flags))
    for name, a, c in zip(('y', 'norm_out', 'zp', 'pnorm'), old, new):
        _same(c, a, f'{name} of {shape}', min_finite=0.0 if special else 0.5)


@pytest.mark.parametrize('shape', SHAPES)
def test_calls_outside_the_forms_run_the_generic_kernel(shape):
    """Calls that differ from every fixed form in ONE argument each.  A selector that looked at fewer arguments than a form
    pins would run the form, which ignores that argument, and the bits would differ from the generic kernel's."""
    from latentfusion_amd import ops
    from latentfusion_amd._lib import LF_EPI_ADD, LF_EPI_LRELU, LF_EPI_PIXELNORM
    N, D, H, W = shape
    x, w, b, wp, pb, he = _problem(shape, 6, False)
    up, upt = ops.pack_conv3d_c16_wino(w), ops.pack_conv3d_c16_wino(w, transpose=True)
    wA, phe = ops.pack_wino_proj(_proj_matrix(wp, D)), ops.he_constant(wp)
    full = LF_EPI_LRELU | LF_EPI_PIXELNORM
    act, nrm = _prev_layer(shape)

    def run():
        outs = {}
        outs['LReLU only'] = ops.conv3d_c16_wino(x, up, b, he, LF_EPI_LRELU)[0]
        outs['PixelNorm only'], outs['PixelNorm only: norm_out'] = ops.conv3d_c16_wino(x, up, b, he, LF_EPI_PIXELNORM)
        outs['add mode'], outs['add mode: norm_out'] = ops.conv3d_c16_wino(x, up, b, he, full, prev=(act, None, LF_EPI_ADD))
        outs['add mode, flags 0, no bias'] = ops.conv3d_c16_wino(x, up, None, he, 0, prev=(act, None, LF_EPI_ADD))[0]
        outs['no bias, flags set'], outs['no bias, flags set: norm_out'] = ops.conv3d_c16_wino(x, up, None, he, full)
        outs['bias, flags 0'] = ops.conv3d_c16_wino(x, up, b, he, 0)[0]
        outs['previous layer LReLU only'] = ops.conv3d_c16_wino(x, upt, None, he, 0, prev=(act, None, LF_EPI_LRELU))[0]
        for name, kw in (('forward', dict(bias=b, flags=full)), ('gradient + previous', dict(bias=None, flags=0, prev=(act, nrm, full))),
                         ('plain gradient', dict(bias=None, flags=0))):
            amax = ops.amax_buffer(device=DEV)
            res = ops.conv3d_c16_wino(x, upt, kw.pop('bias'), he, kw.pop('flags'), amax_out=amax, **kw)
            outs[f'amax_out set, {name}'], outs[f'amax_out set, {name}: amax'] = res[0], amax
            assert amax.abs().max().item() > 0.0, 'the max-abs side channel was written'
        pf = ops.conv3d_c16_wino_projfwd(x, up, b, he, LF_EPI_LRELU, wA, pb, phe, full)
        outs['projfwd, LReLU only'], outs['projfwd, LReLU only: zp'], outs['projfwd, LReLU only: pnorm'] = pf[0], pf[2], pf[3]
        pf = ops.conv3d_c16_wino_projfwd(x, up, None, he, full, wA, pb, phe, full)
        outs['projfwd, no bias'], outs['projfwd, no bias: norm_out'], outs['projfwd, no bias: zp'] = pf[0], pf[1], pf[2]
        return outs

    old, new = _both(run)
    assert old.keys() == new.keys()
    for name in old:
        _same(new[name], old[name], f'{name} of {shape}')
    # the arguments the forms would have ignored did matter: these outputs differ from the matching form's
    base = ops.conv3d_c16_wino(x, up, b, he, full)[0]
    for name in ('LReLU only', 'add mode', 'no bias, flags set'):
        assert not torch.equal(new[name], base), f'{name}: same as the full forward, the case checks nothing'


def test_scalar_transforms_run_the_generic_kernel():
    """Key 7 (packed / scalar transforms next to the MFMAs) under key 8 = 1.  The fixed forms exist for the packed transforms
    only: with key 7 = 0 every call is ROUTED TO THE GENERIC scalar kernel (the scalar form is the A/B baseline of the packing,
    not a product path, and is not specialised).  Both values must give the same bits as each other and as key 8 = 0."""
    from latentfusion_amd import _lib, ops
    from latentfusion_amd._lib import LF_EPI_LRELU, LF_EPI_PIXELNORM
    shape = SHAPES[1]
    N, D, H, W = shape
    run, names = _three_forms(shape, False)
    x, w, b, wp, pb, he = _problem(shape, 5, False)
    up, wA, phe = ops.pack_conv3d_c16_wino(w), ops.pack_wino_proj(_proj_matrix(wp, D)), ops.he_constant(wp)
    full = LF_EPI_LRELU | LF_EPI_PIXELNORM

    def run_all():
        return run() + ops.conv3d_c16_wino_projfwd(x, up, b, he, full, wA, pb, phe, full)

    names = names + ('projfwd y', 'projfwd norm_out', 'projfwd zp', 'projfwd pnorm')
    assert _lib.lib().lf_set_tuning(8, 1) == 1
    scalar, packed = _both(run_all, key=7)
    generic, _ = _both(run_all, key=8)
    for name, s, p, g in zip(names, scalar, packed, generic):
        _same(s, p, f'{name}: key 7 = 0 against key 7 = 1')
        _same(p, g, f'{name}: key 8 = 1 against key 8 = 0')


def test_forms_without_the_register_spending_bit_identical():
    """Key 8 = 2: the fixed forms with the optimiser fences and the per-tile bias read of the generic kernel (the A/B baseline of
    what the freed registers are spent on) against key 8 = 0."""
    from latentfusion_amd import _lib, ops
    from latentfusion_amd._lib import LF_EPI_LRELU, LF_EPI_PIXELNORM
    shape = SHAPES[1]
    N, D, H, W = shape
    run, names = _three_forms(shape, False)
    x, w, b, wp, pb, he = _problem(shape, 5, False)
    up, wA, phe = ops.pack_conv3d_c16_wino(w), ops.pack_wino_proj(_proj_matrix(wp, D)), ops.he_constant(wp)
    full = LF_EPI_LRELU | LF_EPI_PIXELNORM
    L = _lib.lib()
    outs = {}
    try:
        for value in (0, 2):
            L.lf_set_tuning(8, value)
            outs[value] = run() + ops.conv3d_c16_wino_projfwd(x, up, b, he, full, wA, pb, phe, full)
        torch.cuda.synchronize()
    finally:
        L.lf_set_tuning(8, 1)
    for name, a, c in zip(names + ('projfwd y', 'projfwd norm_out', 'projfwd zp', 'projfwd pnorm'), outs[0], outs[2]):
        _same(c, a, f'{name}: key 8 = 2 against key 8 = 0')


def test_switch_reports_and_refuses():
    from latentfusion_amd import _lib
    L = _lib.lib()
    assert L.lf_set_tuning(8, 9) == 1 and L.lf_set_tuning(8, -1) == 1, 'an out-of-range value leaves the default in place'
    assert L.lf_set_tuning(8, 0) == 1 and L.lf_set_tuning(8, 1) == 0
