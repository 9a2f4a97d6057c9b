"""Every kernel form behind lf_resample3d_fwd, lf_resample3d_bwd_coef and lf_resample3d_bwd_vol(_det) (csrc/resample.hip,
csrc/resample_gather.inc, csrc/splat.hip), called through the C ABI, against the explicit fp64 restatement of
tests/resample_cases.py -- not against another form of the same code.

Bounds (resample_cases.fwd_ratio / gcoef_ratio / gvol_ratio; a ratio is error / bound, accepted up to 1):
  lattice family (positions exact in fp32, so only the arithmetic behind them differs)
    forward       12 * 2^-24 * max|corner value| per element
    volume grad.  (12 + n) * 2^-24 * sum|contributions| per element, n contributions added in any order
                  (+ n * 2^-38 max|gout| for the fixed-point form, its documented quantum)
    coefficients  max(4 e32_j, 2e-5 A_j) per coefficient, A_j the sum of the absolute values of the terms of sum j
  general family  forward max(4 e32, 2e-6 + 2e-5 |fp64|); coefficients per sample max(4 max e32, 2e-3 of the largest component);
                  volume gradient max(4 e32, 2e-6 + 2e-5 sum|contributions|)
Every case runs with (N, vol_n) = (1, 1), (3, 1), (3, 3).  Every output is written into a buffer filled with NaN between two
runs of sentinels, which must survive.  `-s` prints one `[resample-fp64]` line per form, shape and channel count with the measured
error and e32 in the bound's own unit (COVERAGE.md, "Resampler against fp64").

Which case reaches which kernel form: FWD_FORMS, COEF_FORMS and VPB_CASES of tests/resample_cases.py."""
import pytest
import torch

import resample_cases as K
from resample_cases import O2C, C2O

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SENT, GUARD = 12345.0, 64
KINDS = [O2C, C2O]
_kid = lambda k: 'o2c' if k == O2C else 'c2o'  # noqa: E731


def _lib():
    from latentfusion_amd import _lib
    return _lib.lib()


@pytest.fixture(autouse=True)
def _restore_tuning():
    L = _lib()
    prev1 = L.lf_set_tuning(1, 3)
    prev2 = L.lf_set_tuning(2, 10)
    L.lf_set_tuning(1, prev1)
    L.lf_set_tuning(2, prev2)
    yield
    L.lf_set_tuning(1, prev1)
    L.lf_set_tuning(2, prev2)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def dev_in(x, offset=0):
    """x on the device, `offset` floats behind a 16-byte boundary."""
    flat = torch.zeros(x.numel() + offset + 4, device=DEV)
    view = flat[offset:offset + x.numel()]
    view.copy_(x.reshape(-1))
    assert view.data_ptr() % 16 == (4 * offset) % 16
    return view


def out_buf(n, fill=float('nan')):
    t = torch.full((GUARD + n + GUARD,), SENT, device=DEV)
    body = t[GUARD:GUARD + n]
    body.fill_(fill)
    return t, body


def check_guards(t, n):
    torch.cuda.synchronize()
    assert bool((t[:GUARD] == SENT).all()) and bool((t[GUARD + n:] == SENT).all()), 'written outside the output'


def run_fwd(vol, cf, kind, dims, variant=3, vol_off=0):
    L = _lib()
    D, H, W = dims
    vol_n, C, N = vol.shape[0], vol.shape[-1], cf.shape[0]
    L.lf_set_tuning(1, variant)
    v, c = dev_in(vol, vol_off), dev_in(cf)
    n = N * D * H * W * C
    t, body = out_buf(n)
    rc = L.lf_resample3d_fwd(v.data_ptr(), vol_n, c.data_ptr(), kind, body.data_ptr(), N, D, H, W, C, _stream())
    assert rc == 0, rc
    check_guards(t, n)
    return body.cpu().reshape(N, D, H, W, C)


def run_coef(gout, vol, cf, dims, key1=3, key2=10, gout_off=0, expect=0):
    L = _lib()
    D, H, W = dims
    vol_n, C, N = vol.shape[0], vol.shape[-1], cf.shape[0]
    L.lf_set_tuning(1, key1)
    L.lf_set_tuning(2, key2)
    g, v, c = dev_in(gout, gout_off), dev_in(vol), dev_in(cf)
    nb = L.lf_resample3d_bwd_coef_scratch_bytes(N, D, H, W)
    scratch = torch.empty(nb // 4 + 4, device=DEV)
    t, body = out_buf(18 * N)
    rc = L.lf_resample3d_bwd_coef(g.data_ptr(), v.data_ptr(), vol_n, c.data_ptr(), body.data_ptr(), scratch.data_ptr(),
                                  scratch.numel() * 4, N, D, H, W, C, _stream())
    assert rc == expect, rc
    check_guards(t, 18 * N)
    return body.cpu().reshape(N, 18)


def run_gvol(gout, cf, kind, dims, vol_n, det=False):
    L = _lib()
    D, H, W = dims
    C, N = gout.shape[-1], cf.shape[0]
    g, c = dev_in(gout), dev_in(cf)
    n = vol_n * D * H * W * C
    if det:
        t, body = out_buf(n)                                          # overwritten
        nb = L.lf_resample3d_bwd_vol_det_scratch_bytes(vol_n, D, H, W, C)
        scr = torch.empty(nb // 8 + 1, device=DEV, dtype=torch.int64)
        rc = L.lf_resample3d_bwd_vol_det(g.data_ptr(), c.data_ptr(), kind, body.data_ptr(), vol_n, scr.data_ptr(), scr.numel() * 8,
                                         N, D, H, W, C, _stream())
    else:
        t, body = out_buf(n, fill=0.0)                                # accumulated into: zeroed by the caller
        rc = L.lf_resample3d_bwd_vol(g.data_ptr(), c.data_ptr(), kind, body.data_ptr(), vol_n, N, D, H, W, C, _stream())
    assert rc == 0, rc
    check_guards(t, n)
    return body.cpu().reshape(vol_n, D, H, W, C)


def _units(err, unit):
    """Largest err / unit over the elements with a positive finite unit."""
    ok = torch.isfinite(unit) & (unit > 0) & torch.isfinite(err)
    return float((err[ok] / unit[ok]).max()) if bool(ok.any()) else 0.0


def report(what, form, dims, C, kind, worst):
    print(f'[resample-fp64] {what:5s} {form} | {"x".join(map(str, dims))} C={C} {_kid(kind)}: ' + ', '.join(f'{k} {v:.2e}' for k, v in worst.items()))


def check_fwd(got, c, family, worst):
    ref, r32 = c['ref'], c['r32']
    r = K.fwd_ratio(got, ref, family, r32)
    worst['err/max|corner|'] = max(worst.get('err/max|corner|', 0.0), _units((got.double() - ref['fwd']).abs(), ref['maxcorner']))
    worst['e32/max|corner|'] = max(worst.get('e32/max|corner|', 0.0), _units((r32['fwd'].double() - ref['fwd']).abs(), ref['maxcorner']))
    worst['err/bound'] = max(worst.get('err/bound', 0.0), r)
    if family == 'general':                                            # for the record: e32 taken at the same element (resample_cases.fwd_ratio)
        err, e32 = (got.double() - ref['fwd']).abs(), (r32['fwd'].double() - ref['fwd']).abs()
        worst['err/bound(e32 per element)'] = max(worst.get('err/bound(e32 per element)', 0.0),
                                                  float((err / torch.maximum(4 * e32, 2e-6 + 2e-5 * ref['fwd'].abs())).max()))
        worst['needs 4 e32'] = max(worst.get('needs 4 e32', 0.0), float((err > 2e-6 + 2e-5 * ref['fwd'].abs()).any()))
    assert r <= 1.0, r


def check_coef(got, c, family, worst):
    ref, r32 = c['ref'], c['r32']
    r = K.gcoef_ratio(got, ref, family, r32)
    err, e32 = (got.double() - ref['gcoef']).abs(), (r32['gcoef'].double() - ref['gcoef']).abs()
    worst['err/A'] = max(worst.get('err/A', 0.0), _units(err, ref['A']))
    worst['e32/A'] = max(worst.get('e32/A', 0.0), _units(e32, ref['A']))
    worst['err/bound'] = max(worst.get('err/bound', 0.0), r)
    if family != 'general':
        needs = ((err > 2e-5 * ref['A']) & (err <= 4 * e32)).any()
    else:
        needs = (err.amax(1) > 2e-3 * ref['gcoef'].abs().amax(1)).any()
    worst['needs 4 e32'] = max(worst.get('needs 4 e32', 0.0), float(needs))
    assert r <= 1.0, (r, err / ref['A'])


def check_gvol(got, c, family, worst, quantum=0.0, tag='err'):
    ref = c['ref']
    r = K.gvol_ratio(got, ref, family, c['r32'], quantum)
    worst[tag + '/sum|contrib|'] = max(worst.get(tag + '/sum|contrib|', 0.0), _units((got.double() - ref['gvol']).abs(), ref['gvol_abs']))
    worst[tag + '/bound'] = max(worst.get(tag + '/bound', 0.0), r)
    assert r <= 1.0, r


# ---- forward ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', KINDS, ids=_kid)
@pytest.mark.parametrize('variant,C,form', K.FWD_FORMS, ids=[f'tuning{v}-C{c}' for v, c, _ in K.FWD_FORMS])
def test_forward_forms(variant, C, form, kind):
    worst = {}
    for N, vol_n in K.NV:
        c = K.case('lattice', kind, K.BASE, C, N, vol_n)
        check_fwd(run_fwd(c['vol'], c['cf'], kind, K.BASE, variant), c, 'lattice', worst)
    report('fwd', f'tuning {variant}: {form}', K.BASE, C, kind, worst)


@pytest.mark.parametrize('kind', KINDS, ids=_kid)
@pytest.mark.parametrize('C', [16, 3])
@pytest.mark.parametrize('dims', K.LATTICE_SHAPES[1:], ids=lambda d: 'x'.join(map(str, d)))
def test_forward_shapes(dims, C, kind):
    worst = {}
    for N, vol_n in K.NV:
        c = K.case('lattice', kind, dims, C, N, vol_n)
        check_fwd(run_fwd(c['vol'], c['cf'], kind, dims), c, 'lattice', worst)
    report('fwd', 'resample_fwd_c16_kernel' if C == 16 else 'resample_fwd_kernel<KIND,1>', dims, C, kind, worst)


@pytest.mark.parametrize('kind', KINDS, ids=_kid)
def test_forward_misaligned_volume_takes_the_scalar_kernel(kind):
    """A volume pointer one float off a 16-byte boundary: fwd_plan picks resample_fwd_kernel<KIND,1> at C = 16, under every
    tuning.  Within the bound of fp64, hence within twice the bound of the aligned generic call (lf_set_tuning(1, 1):
    resample_fwd_kernel<KIND,4>, whose packed sum the compiler contracts in its own way); the default aligned call: next test."""
    worst = {}
    for N, vol_n in K.NV:
        c = K.case('lattice', kind, K.BASE, 16, N, vol_n)
        off = run_fwd(c['vol'], c['cf'], kind, K.BASE, 3, vol_off=1)
        check_fwd(off, c, 'lattice', worst)
        assert torch.equal(off, run_fwd(c['vol'], c['cf'], kind, K.BASE, 1, vol_off=1))
        for variant in (3, 1):
            aligned = run_fwd(c['vol'], c['cf'], kind, K.BASE, variant)
            key = f'|misaligned - aligned, tuning {variant}| / max|corner|'
            worst[key] = max(worst.get(key, 0.0), _units((off.double() - aligned.double()).abs(), c['ref']['maxcorner']))
            assert bool(((off.double() - aligned.double()).abs() <= 24 * K.U * c['ref']['maxcorner']).all())
    report('fwd', 'misaligned: resample_fwd_kernel<KIND,1>', K.BASE, 16, kind, worst)


@pytest.mark.parametrize('kind', KINDS, ids=_kid)
def test_forward_misaligned_volume_is_bit_identical_to_the_aligned_call(kind):
    """The same 16-channel data gives the same bits whether or not the volume is 16-byte aligned: resample_fwd_kernel<KIND,1>
    rounds the eight products as resample_fwd_c16_kernel's fmac chain does (first product rounded, the other seven fused in
    corner order).  Before the scalar kernel spelled that chain out, the compiler's contraction of `v000 * w000 + v001 * w001 + ...`
    fused the first product and rounded the second: 3043 (O2C) / 2671 (C2O) of 12240 outputs differed at N = 1, by one
    rounding (2.4e-7 at most).  Asserted where the positions are exact (lattice family), so that only this arithmetic is compared."""
    for N, vol_n in K.NV:
        c = K.case('lattice', kind, K.BASE, 16, N, vol_n)
        off = run_fwd(c['vol'], c['cf'], kind, K.BASE, 3, vol_off=1)
        aligned = run_fwd(c['vol'], c['cf'], kind, K.BASE, 3)
        assert torch.equal(off, aligned), (int((off != aligned).sum()), off.numel(), float((off - aligned).abs().max()))


@pytest.mark.parametrize('kind', KINDS, ids=_kid)
@pytest.mark.parametrize('C', [16, 3])
@pytest.mark.parametrize('dims', K.GENERAL_SHAPES, ids=lambda d: 'x'.join(map(str, d)))
def test_forward_general_family(dims, C, kind):
    worst = {}
    for N, vol_n in K.NV:
        c = K.case('general', kind, dims, C, N, vol_n)
        check_fwd(run_fwd(c['vol'], c['cf'], kind, dims), c, 'general', worst)
        if C == 16:
            check_fwd(run_fwd(c['vol'], c['cf'], kind, dims, 1), c, 'general', worst)
    report('fwd', 'general family', dims, C, kind, worst)


# ---- coefficient gradient ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C,form', K.COEF_FORMS, ids=[f'C{c}' for c, _ in K.COEF_FORMS])
def test_coefficient_gradient_forms(C, form):
    worst = {}
    for N, vol_n in K.NV:
        c = K.case('lattice', O2C, K.BASE, C, N, vol_n)
        got = run_coef(c['gout'], c['vol'], c['cf'], K.BASE)
        check_coef(got, c, 'lattice', worst)
    assert torch.equal(got, run_coef(c['gout'], c['vol'], c['cf'], K.BASE))          # fixed-order sums: run-to-run identical
    report('coef', form, K.BASE, C, O2C, worst)


@pytest.mark.parametrize('dims,C', [((17, 33, 9), 16), ((3, 2, 65), 16), ((17, 33, 9), 3), ((3, 2, 65), 3)],
                         ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else f'C{v}')
def test_coefficient_gradient_shapes(dims, C):
    worst = {}
    for N, vol_n in K.NV:
        c = K.case('lattice', O2C, dims, C, N, vol_n)
        check_coef(run_coef(c['gout'], c['vol'], c['cf'], dims), c, 'lattice', worst)
    report('coef', 'resample_bwd_coef_c16_kernel<8,1>' if C == 16 else 'resample_bwd_coef_kernel<1>', dims, C, O2C, worst)


@pytest.mark.parametrize('dims,N,vol_n,vpb,form', K.VPB_CASES, ids=[f'vpb{v[3]}' for v in K.VPB_CASES])
def test_coefficient_gradient_block_sizes(dims, N, vol_n, vpb, form):
    assert K.bwd_vox_per_block(dims[0] * dims[1] * dims[2], N) == vpb
    c = K.case('lattice', O2C, dims, 16, N, vol_n)
    worst = {}
    got = run_coef(c['gout'], c['vol'], c['cf'], dims)
    check_coef(got, c, 'lattice', worst)
    assert torch.equal(got, run_coef(c['gout'], c['vol'], c['cf'], dims))
    report('coef', f'vpb {vpb}: {form}', dims, 16, O2C, worst)


@pytest.mark.parametrize('key1,key2,form', [(1, 10, 'resample_bwd_coef_kernel<4>'), (4, 10, 'resample_bwd_coef_staged_kernel<16>'),
                                            (3, 1, 'resample_bwd_coef_c16_kernel<1,1>'),
                                            (3, 2, 'resample_bwd_coef_c16_kernel<1,2>'),
                                            (3, 6, 'resample_bwd_coef_c16_dedup_kernel<2,1>'),
                                            (3, 10, 'resample_bwd_coef_c16_dedup_kernel<2,1,true>')],
                         ids=lambda v: str(v) if isinstance(v, int) else None)
def test_coefficient_gradient_tuning_keys(key1, key2, form):
    dims, N, vol_n = K.VPB_CASES[2][:3]
    c = K.case('lattice', O2C, dims, 16, N, vol_n)
    worst = {}
    got = run_coef(c['gout'], c['vol'], c['cf'], dims, key1, key2)
    check_coef(got, c, 'lattice', worst)
    assert torch.equal(got, run_coef(c['gout'], c['vol'], c['cf'], dims, key1, key2))
    report('coef', f'tuning ({key1}, {key2}): {form}', dims, 16, O2C, worst)


def test_coefficient_gradient_misaligned_gout_c64():
    """gout one float off a 16-byte boundary: bwd_coef_plan takes resample_bwd_coef_kernel<1> with all 64 lanes of a voxel busy."""
    worst = {}
    for N, vol_n in K.NV:
        c = K.case('lattice', O2C, K.BASE, 64, N, vol_n)
        check_coef(run_coef(c['gout'], c['vol'], c['cf'], K.BASE, gout_off=1), c, 'lattice', worst)
    report('coef', 'misaligned: resample_bwd_coef_kernel<1>, lpv = 64', K.BASE, 64, O2C, worst)


@pytest.mark.parametrize('C,gout_off', [(65, 0), (260, 0), (128, 1)], ids=['C65', 'C260', 'C128-misaligned'])
def test_coefficient_gradient_channel_limit(C, gout_off):
    """More than 64 lanes per voxel (C > 64 scalar, C > 256 in groups of four): LF_EINVAL, nothing written."""
    gen = torch.Generator().manual_seed(C)
    vol = torch.randn(1, *K.BASE, C, generator=gen)
    gout = torch.randn(1, *K.BASE, C, generator=gen)
    cf = K.lattice_coefs(1, O2C, K.BASE, gen).float()
    got = run_coef(gout, vol, cf, K.BASE, gout_off=gout_off, expect=K.LF_EINVAL)
    assert bool(torch.isnan(got).all())                                # the poison the buffer was filled with


@pytest.mark.parametrize('C', [16, 3])
@pytest.mark.parametrize('dims', K.SIZE1_SHAPES, ids=lambda d: 'x'.join(map(str, d)))
def test_coefficient_gradient_size_one_axes(dims, C):
    """An axis of size 1 has no interior (mask 0) and its lattice coordinate is 0: its components and the rows of its basis
    functions are exactly 0."""
    D, H, W = dims
    worst = {}
    for N, vol_n in K.NV:
        c = K.case('lattice', O2C, dims, C, N, vol_n)
        got = run_coef(c['gout'], c['vol'], c['cf'], dims)
        check_coef(got, c, 'lattice', worst)
        g = got.reshape(N, 6, 3)
        for comp, S in enumerate((W, H, D)):
            if S == 1:
                assert bool((g[:, :, comp] == 0).all())
        rows = {0: (1, 4) if W == 1 else (), 1: (2, 5) if H == 1 else (), 2: (3, 4, 5) if D == 1 else ()}
        for js in rows.values():
            for j in js:
                assert bool((g[:, j, :] == 0).all()), (dims, j, g[:, j, :])
    report('coef', 'size-1 axes', dims, C, O2C, worst)


@pytest.mark.parametrize('C', [16, 3])
@pytest.mark.parametrize('dims', K.GENERAL_SHAPES, ids=lambda d: 'x'.join(map(str, d)))
def test_coefficient_gradient_general_family(dims, C):
    worst = {}
    for N, vol_n in K.NV:
        c = K.case('general', O2C, dims, C, N, vol_n)
        check_coef(run_coef(c['gout'], c['vol'], c['cf'], dims), c, 'general', worst)
    report('coef', 'general family', dims, C, O2C, worst)


# ---- volume gradient --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', KINDS, ids=_kid)
@pytest.mark.parametrize('C', [1, 3, 16, 20])
@pytest.mark.parametrize('dims', [K.BASE, K.SIZE1_SHAPES[0]], ids=lambda d: 'x'.join(map(str, d)))
def test_volume_gradient(dims, C, kind):
    worst = {}
    for N, vol_n in K.NV:
        c = K.case('lattice', kind, dims, C, N, vol_n)
        gv = run_gvol(c['gout'], c['cf'], kind, dims, vol_n)
        check_gvol(gv, c, 'lattice', worst)
        gvs = [gv]
        if C == 16:
            det = run_gvol(c['gout'], c['cf'], kind, dims, vol_n, det=True)
            check_gvol(det, c, 'lattice', worst, quantum=2.0 ** -38 * float(c['gout'].abs().max()), tag='det')
            gvs.append(det)
        # adjoint identity with the forward kernel tested above: <gout, fwd(vol)> = <bwd_vol(gout), vol>, both sums in fp64
        fwd = run_fwd(c['vol'], c['cf'], kind, dims).double()
        lhs, scale = (c['gout'].double() * fwd).sum(), (c['gout'].double() * fwd).abs().sum()
        for g in gvs:
            rhs = (g.double() * c['vol'].double()).sum()
            assert abs(float(lhs - rhs)) <= 2e-5 * float(scale), (float(lhs), float(rhs), float(scale))
            worst['adjoint/bound'] = max(worst.get('adjoint/bound', 0.0), abs(float(lhs - rhs)) / (2e-5 * float(scale)))
    report('gvol', 'resample_bwd_vol_kernel' + (' + lf_resample3d_bwd_vol_det' if C == 16 else ''), dims, C, kind, worst)


@pytest.mark.parametrize('kind', KINDS, ids=_kid)
@pytest.mark.parametrize('dims', K.GENERAL_SHAPES, ids=lambda d: 'x'.join(map(str, d)))
def test_volume_gradient_general_family(dims, kind):
    worst = {}
    for N, vol_n in K.NV:
        c = K.case('general', kind, dims, 16, N, vol_n)
        check_gvol(run_gvol(c['gout'], c['cf'], kind, dims, vol_n), c, 'general', worst)
        check_gvol(run_gvol(c['gout'], c['cf'], kind, dims, vol_n, det=True), c, 'general', worst, tag='det')
    report('gvol', 'general family', dims, 16, kind, worst)


# ---- non-finite and degenerate maps ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C', [16, 3])
@pytest.mark.parametrize('name', K.DEGENERATE)
def test_degenerate_maps(name, C):
    """NaN / infinite coefficients, a projective denominator that crosses zero, a map far outside, a constant map: the taps the
    header prescribes (tests/test_resample_cases.py spells them out on the reference), values within the lattice bounds, and
    coefficient gradients whose masked components are exactly 0 (`far_outside`: all of them, A = 0 leaves a bound of 0)."""
    c = K.degenerate_case(name, C)
    kind, worst = c['kind'], {}
    for variant in (3, 1):
        check_fwd(run_fwd(c['vol'], c['cf'], kind, K.BASE, variant), c, 'lattice', worst)
    if kind == O2C:
        got = run_coef(c['gout'], c['vol'], c['cf'], K.BASE)
        check_coef(got, c, 'lattice', worst)
        if name == 'far_outside':
            assert bool((got == 0).all())
    check_gvol(run_gvol(c['gout'], c['cf'], kind, K.BASE, 1), c, 'lattice', worst)
    report('degen', name, K.BASE, C, kind, worst)


@pytest.mark.parametrize('C', [16, 3])
def test_nan_in_the_volume_stays_in_the_outputs_that_touch_it(C):
    D, H, W = K.BASE
    c = K.case('lattice', O2C, K.BASE, C, 3, 1)
    vol = c['vol'].clone()
    counts = torch.bincount(c['ref']['taps'].reshape(-1), minlength=D * H * W)
    voxel = int(torch.where(counts > 0, (counts - 12).abs(), counts.max() + 12).argmin())   # a voxel that about a dozen taps read
    vol.reshape(-1, C)[voxel, C // 2] = float('nan')
    ref = K.reference(vol, c['cf'], O2C, K.BASE)
    touched = (ref['taps'] == voxel).any(-1).reshape(3, D, H, W)         # zero-weight taps included: 0 * NaN is NaN
    assert 0 < int(touched.sum()) < touched.numel()
    for variant in (3, 1):
        got = run_fwd(vol, c['cf'], O2C, K.BASE, variant)
        nan = torch.isnan(got)
        assert torch.equal(nan[..., C // 2], touched) and int(nan.sum()) == int(touched.sum())
        assert K.fwd_ratio(got, ref, 'lattice') <= 1.0


# ---- the comparison rejects misreadings --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', K.MISREADINGS)
def test_comparison_rejects_a_misread_reference(name):
    out, key = K.MISREAD_CASES[name]
    family, kind, dims, C, N, vol_n = key
    c = K.case(*key)
    got = run_fwd(c['vol'], c['cf'], kind, dims) if out == 'fwd' else run_coef(c['gout'], c['vol'], c['cf'], dims)
    true = K.fwd_ratio(got, c['ref'], family) if out == 'fwd' else K.gcoef_ratio(got, c['ref'], family, c['r32'])
    wrong = K.misread_ratio(name, got)
    print(f'[resample-fp64] misreading {name}: err/bound {wrong:.3g} against the misread reference, {true:.3g} against the true one')
    assert true <= 1.0 and wrong > 1.0, (true, wrong)
