"""Every kernel form behind lf_conv3x3_fwd, lf_conv3x3_bwd_data, lf_conv1x1_fwd, lf_conv1x1_fwd_scaled and lf_conv1x1_bwd_data
(csrc/conv.hip), called through the C ABI, against the explicit fp64 restatement of tests/conv_direct_cases.py -- not against
CPU fp32 and not against another kernel of the same file.  These are the kernels the Winograd, split-precision, f16x3 and
wide-GEMM tests take their e_ref and their fused-backward `want` from; this module is what bounds them.

Bound (conv_direct_cases.ratio; a ratio is error / bound, accepted up to 1): per element max(4 e32, 2e-6 + 2e-5 s), s = |fp64|
of the element (forward, raw gradient), the largest |fp64| of the element's record (fused gradients) or the row's largest
pre-normalisation activation (norms); e32 = the largest error of the same expressions in fp32 on the CPU.  No element is
excluded.

Every output is written into a NaN-filled buffer between two runs of sentinels, which must survive; x, prev_y, the bias and the
weight pack lie between NaN-filled guards and every output must come out finite (the persistent kernel's zero fill of the halo
relies on the buffer descriptor's range, not on what lies beside the sample).  Each sample alone must equal its row of the
batch bit for bit, two runs must be identical, and norm_out = NULL must change nothing in y.  `-s` prints one `[conv-fp64]` line
per form and case (COVERAGE.md, "Direct convolutions against fp64").

Which case reaches which kernel form: form3x3 / form1x1 of tests/conv_direct_cases.py, a restatement of conv3x3_launch and
conv1x1_launch that tests/test_conv_direct_cases.py checks for completeness."""
import pytest
import torch

import conv_direct_cases as K
from conv_direct_cases import DOT, EPS, LF_EALIGN, LF_EINVAL, LRELU, PIXELNORM, SLOPE

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SENT, GUARD = 12345.0, 64
NAN = float('nan')
BOTH = LRELU | PIXELNORM


def _lib():
    from latentfusion_amd import _lib
    return _lib.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def dev_in(x, offset=0):
    """x on the device between NaN guards, `offset` floats behind a 16-byte boundary."""
    n = x.numel()
    flat = torch.full((GUARD + offset + n + GUARD,), NAN, device=DEV)
    view = flat[GUARD + offset:GUARD + offset + n]
    view.copy_(x.reshape(-1))
    assert view.data_ptr() % 16 == (4 * offset) % 16
    return view


def out_buf(n, fill=NAN):
    t = torch.full((GUARD + n + GUARD,), SENT, device=DEV)
    body = t[GUARD:GUARD + n]
    body.fill_(fill)
    return t, body


def check_guards(t, n):
    torch.cuda.synchronize()
    assert bool((t[:GUARD] == SENT).all()) and bool((t[GUARD + n:] == SENT).all()), 'written outside the output'


def ptr(t):
    return None if t is None else t.data_ptr()


def _pick(t, alone):
    return t if alone is None or t is None else t[alone:alone + 1]


class Worst:
    """Per (form, case): the largest err, e32 and err / bound of every output over the variants run."""

    def __init__(self, what):
        self.what, self.rows = what, {}

    def add(self, form, case, ratios):
        row = self.rows.setdefault((form, case), {})
        for k, (err, e32, r) in ratios.items():
            o = row.get(k, (0.0, 0.0, 0.0))
            row[k] = (max(o[0], err), max(o[1], e32), max(o[2], r))
        bad = {k: v for k, v in ratios.items() if not v[2] <= 1.0}
        assert not bad, (form, case, bad)

    def report(self):
        for (form, case), row in self.rows.items():
            print(f'[conv-fp64] {self.what:4s} {form} | {case}: '
                  + '; '.join(f'{k} err {v[0]:.2e} (e32 {v[1]:.2e}) err/bound {v[2]:.2f}' for k, v in row.items()))


def _case3(dims, cin, cout, shape):
    return f'{dims}d {cin}->{cout} {"x".join(map(str, shape[3 - dims:]))}'


# ---- lf_conv3x3_fwd / lf_conv3x3_bwd_data ---------------------------------------------------------------------------------------
def run_fwd3(desc, want_norm=True, bias_off=0, expect=0, x_off=0, y_off=0, w_off=0):
    _, dims, cin, cout, shape, B, alone, flags, with_bias = desc
    L = K.layer3(dims, cin, cout, shape, B)
    D, H, W = shape
    x = _pick(L['x'], alone)
    N, nvox = x.shape[0], D * H * W
    xd, wd = dev_in(x, x_off), dev_in(K.pack3(L['w']), w_off)
    bd = dev_in(L['b'], bias_off) if with_bias else None
    t, body = out_buf(N * nvox * cout + y_off)
    tn, nbody = out_buf(N * nvox)
    rc = _lib().lf_conv3x3_fwd(ptr(xd), ptr(wd), ptr(bd), body.data_ptr() + 4 * y_off, ptr(nbody) if want_norm else None, dims, N, D, H, W,
                               cin, cout, L['he'], flags, SLOPE, EPS, _stream())
    assert rc == expect, rc
    check_guards(t, N * nvox * cout + y_off)
    check_guards(tn, N * nvox)
    if expect != 0:
        assert bool(torch.isnan(body).all()) and bool(torch.isnan(nbody).all()), 'a refused call wrote'
        return None
    out = {'y': body.cpu().reshape(N, D, H, W, cout)}
    if (flags & PIXELNORM) and want_norm:
        out['norm'] = nbody.cpu().reshape(N, D, H, W)
    else:
        assert bool(torch.isnan(nbody).all()), 'norm_out written without LF_EPI_PIXELNORM'
    return out


def run_bwd3(desc, expect=0, gy_off=0, prev_off=0, norm=True):
    _, dims, cc, cp, shape, B, alone, pf = desc
    G = K.grad3(dims, cc, cp, shape, B)
    D, H, W = shape
    gy = _pick(G['gy'], alone)
    N, nvox = gy.shape[0], D * H * W
    gd, wd = dev_in(gy, gy_off), dev_in(K.pack3_t(G['w']))
    yp = nr = None
    if pf:
        py, pn = G['prev'][pf]
        yp = dev_in(_pick(py, alone), prev_off)
        nr = dev_in(_pick(pn, alone)) if (pn is not None and norm) else None
    t, body = out_buf(N * nvox * cp)
    rc = _lib().lf_conv3x3_bwd_data(ptr(gd), ptr(wd), ptr(body), dims, N, D, H, W, cc, cp, G['he'], ptr(yp), ptr(nr), pf, SLOPE, _stream())
    assert rc == expect, rc
    check_guards(t, N * nvox * cp)
    if expect != 0:
        assert bool(torch.isnan(body).all()), 'a refused call wrote'
        return None
    return {'gx': body.cpu().reshape(N, D, H, W, cp)}


def _fwd3_layer(worst, dims, cin, cout, shape, B=3, alone=1, form=None, variants=None, repeat=True):
    """Every variant of one forward layer on the batch and on one sample alone, with the three properties."""
    form = form or K.form3x3(dims, shape, cin, cout, N=B, cus=_cus())
    case = _case3(dims, cin, cout, shape) + (f' N={B}' if B != 3 else '')
    first = repeat
    for flags, with_bias, want_norm in variants or K.fwd3_variants(cout):
        desc = ('fwd3', dims, cin, cout, shape, B, None, flags, with_bias)
        got = run_fwd3(desc, want_norm)
        worst.add(form, case, K.ratios(K.expected(desc), got))
        one = ('fwd3', dims, cin, cout, shape, B, alone, flags, with_bias)
        got1 = run_fwd3(one, want_norm)
        worst.add(K.form3x3(dims, shape, cin, cout, N=1, cus=_cus()), case + ' alone', K.ratios(K.expected(one), got1))
        for k in got1:                                               # the sample alone is its row of the batch
            assert torch.equal(got1[k], got[k][alone:alone + 1]), (desc, k)
        if first:                                                    # run to run
            again = run_fwd3(desc, want_norm)
            assert all(torch.equal(again[k], got[k]) for k in got), desc
            first = False
        if not want_norm:                                            # norm_out = NULL changes nothing in y
            assert torch.equal(run_fwd3(desc, True)['y'], got['y']), desc


def _bwd3_problem(worst, dims, cc, cp, shape, B=3, alone=1, repeat=(0, BOTH)):
    case = _case3(dims, cc, cp, shape) + (f' N={B}' if B != 3 else '')
    for pf in (0,) + K.PREV_FLAGS:
        form = K.form3x3(dims, shape, cc, cp, fused=pf != 0, N=B, cus=_cus())
        desc = ('bwd3', dims, cc, cp, shape, B, None, pf)
        got = run_bwd3(desc)
        worst.add(form, case + f' prev_flags {pf}', K.ratios(K.expected(desc), got))
        one = ('bwd3', dims, cc, cp, shape, B, alone, pf)
        got1 = run_bwd3(one)
        worst.add(K.form3x3(dims, shape, cc, cp, fused=pf != 0, N=1, cus=_cus()), case + f' prev_flags {pf} alone',
                  K.ratios(K.expected(one), got1))
        assert torch.equal(got1['gx'], got['gx'][alone:alone + 1]), desc
        if pf in repeat:
            assert torch.equal(run_bwd3(desc)['gx'], got['gx']), desc


_id3 = lambda k: f'{k[0]}d-{k[1]}to{k[2]}-{"x".join(map(str, k[3]))}'  # noqa: E731


def test_padded_channel_counts_are_the_librarys():
    L = _lib()
    for c in (1, 2, 3, 7, 10, 16, 17, 24, 32, 33, 48, 64, 65, 66, 80, 128, 129, 132, 200, 256, 320):
        assert L.lf_conv3x3_cout_padded(c) == K.cout_padded3(c) and L.lf_conv1x1_cout_padded(c) == K.cout_padded1(c), c


@pytest.mark.parametrize('key', K.layers3(), ids=_id3)
def test_conv3x3_forward_matches_fp64(key):
    worst = Worst('fwd')
    try:
        _fwd3_layer(worst, *key)
    finally:
        worst.report()


@pytest.mark.parametrize('key', K.grads3(), ids=_id3)
def test_conv3x3_data_gradient_matches_fp64(key):
    worst = Worst('bwd')
    try:
        _bwd3_problem(worst, *key)
    finally:
        worst.report()


@pytest.mark.parametrize('shape', K.PERSISTENT_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_persistent_kernel_matches_fp64(shape):
    assert K.form3x3(3, shape, 16, 16, N=3, cus=_cus()).startswith('conv3d_c16_persistent_kernel')
    worst = Worst('pers')
    try:
        _fwd3_layer(worst, 3, 16, 16, shape)
        _bwd3_problem(worst, 3, 16, 16, shape)
    finally:
        worst.report()


def test_persistent_kernel_walks_three_tiles_per_workgroup():
    """The double-buffered walk (issue_dma(t + 1, cur ^ 1)), the late epilogue of waves 4..7 and prefetch_prev with more tiles
    than workgroups: every workgroup that has work does per = ceil(tiles / CUs) >= 3 consecutive tiles (the last one the
    remainder; workgroups from ceil(tiles / per) on return at once -- 513 tiles on 256 CUs: 171 workgroups of three)."""
    cus = _cus()
    B = K.walk_batch(cus)
    tiles = K.persistent_tiles(K.WALK_SHAPE, B)
    per = K.persistent_tiles_per_workgroup(K.WALK_SHAPE, B, cus)
    assert tiles > 2 * cus and per >= 3, (cus, B, tiles, per)
    assert K.form3x3(3, K.WALK_SHAPE, 16, 16, N=B, cus=cus) == 'conv3d_c16_persistent_kernel walk'
    worst = Worst('walk')
    try:
        _fwd3_layer(worst, 3, 16, 16, K.WALK_SHAPE, B=B, alone=B - 1, variants=[(f, True, True) for f in K.FLAGSETS], repeat=False)
        _bwd3_problem(worst, 3, 16, 16, K.WALK_SHAPE, B=B, alone=B - 1, repeat=(BOTH,))
    finally:
        worst.report()
    print(f'[conv-fp64] walk {cus} CUs, N = {B}: {tiles} tiles, {per} per workgroup')


def test_misaligned_bias_falls_back_to_the_c16_kernel():
    """A bias 4 bytes behind a 16-byte boundary: the persistent kernel reads it as one float4 per lane, so conv3x3_launch sends
    the call to conv3x3_c16_kernel<3>, which must meet the same bound."""
    shape = (10, 19, 40)
    assert K.form3x3(3, shape, 16, 16, bias_aligned=False) == 'conv3x3_c16_kernel<3>'
    worst = Worst('fwd')
    try:
        for flags in K.FLAGSETS:
            desc = ('fwd3', 3, 16, 16, shape, 3, None, flags, True)
            got = run_fwd3(desc, bias_off=1)
            worst.add('conv3x3_c16_kernel<3> (misaligned bias)', _case3(3, 16, 16, shape), K.ratios(K.expected(desc), got))
            one = ('fwd3', 3, 16, 16, shape, 3, 1, flags, True)
            got1 = run_fwd3(one, bias_off=1)
            worst.add('conv3x3_c16_kernel<3> (misaligned bias)', _case3(3, 16, 16, shape) + ' alone', K.ratios(K.expected(one), got1))
            assert all(torch.equal(got1[k], got[k][1:2]) for k in got1), desc
            if flags & PIXELNORM:                                    # norm_out = NULL changes nothing in y
                assert torch.equal(run_fwd3(desc, want_norm=False, bias_off=1)['y'], got['y']), desc
    finally:
        worst.report()


def test_conv3x3_refused_arguments():
    """Every LF_EINVAL / LF_EALIGN of conv3x3_launch; the output stays as it was.  (prev_y with flags or a bias cannot be
    expressed through lf_conv3x3_bwd_data, which has neither argument.)"""
    L = _lib()
    s = _stream()
    D, H, W, C = 5, 6, 17, 16
    lay = K.layer3(3, C, C, (D, H, W))
    x, w, b = dev_in(lay['x']), dev_in(K.pack3(lay['w'])), dev_in(lay['b'])
    t, y = out_buf(3 * D * H * W * 80)
    tn, nrm = out_buf(3 * D * H * W)

    def fwd(xp=None, wp=None, yp=None, dims=3, N=3, D=D, H=H, W=W, cin=C, cout=C, flags=BOTH):
        return L.lf_conv3x3_fwd(xp or x.data_ptr(), wp or w.data_ptr(), b.data_ptr(), yp or y.data_ptr(), nrm.data_ptr(), dims, N, D, H, W,
                                cin, cout, lay['he'], flags, SLOPE, EPS, s)
    for kw in ({'N': 0}, {'N': -1}, {'D': 0}, {'H': 0}, {'W': 0}, {'W': -3}, {'cin': 0}, {'cout': 0}, {'cout': -16},
               {'dims': 1}, {'dims': 4}, {'dims': 0}, {'dims': 2}, {'dims': 2, 'D': 2}, {'cout': 65}, {'cout': 80, 'flags': PIXELNORM}):
        assert fwd(**kw) == LF_EINVAL, kw
    for kw in ({'xp': x.data_ptr() + 4}, {'yp': y.data_ptr() + 8}, {'wp': w.data_ptr() + 4}):
        assert fwd(**kw) == LF_EALIGN, kw
    check_guards(t, y.numel())
    check_guards(tn, nrm.numel())
    assert bool(torch.isnan(y).all()) and bool(torch.isnan(nrm).all())
    assert fwd(dims=2, D=1) == 0                                     # (dims = 2 with D = 1 is a valid call on the same buffers)
    # the fused backward: whole records of 16, 32 or 64 channels, a norm with PixelNorm', aligned prev_y
    for cp in (8, 48, 20, 128):
        G = K.grad3(3, 16, 16, (D, H, W))
        gy, wt = dev_in(G['gy']), dev_in(torch.zeros(27, K.cout_padded3(cp), 16))
        py, pn = dev_in(torch.zeros(3 * D * H * W * cp)), dev_in(torch.ones(3 * D * H * W))
        tg, gx = out_buf(3 * D * H * W * cp)
        assert L.lf_conv3x3_bwd_data(gy.data_ptr(), wt.data_ptr(), gx.data_ptr(), 3, 3, D, H, W, 16, cp, 1.0, py.data_ptr(), pn.data_ptr(),
                                     BOTH, SLOPE, s) == LF_EINVAL, cp
        check_guards(tg, gx.numel())
        assert bool(torch.isnan(gx).all())
    desc = ('bwd3', 3, 16, 16, (D, H, W), 3, None, BOTH)
    run_bwd3(desc, expect=LF_EINVAL, norm=False)                      # PixelNorm' without prev_norm
    run_bwd3(('bwd3', 3, 16, 16, (D, H, W), 3, None, PIXELNORM), expect=LF_EINVAL, norm=False)
    run_bwd3(desc, expect=LF_EINVAL, prev_off=1)                      # prev_y not 16-byte aligned (conv3x3_launch's code for it)
    run_bwd3(desc, expect=LF_EALIGN, gy_off=1)
    assert run_bwd3(('bwd3', 3, 16, 16, (D, H, W), 3, None, LRELU), norm=False) is not None     # LeakyReLU' alone needs no norm


# ---- lf_conv1x1_fwd, lf_conv1x1_fwd_scaled, lf_conv1x1_bwd_data -----------------------------------------------------------------
def run_pw(spec):
    a, lay = K.pw_addr(spec), K.pw_layer(spec)
    alone = a['alone']
    N = 3 if alone is None else 1
    first = 0 if alone is None else alone
    xbuf = lay['xbuf'][first * a['xbs']:(first + N) * a['xbs']]
    xd, wd = dev_in(xbuf), dev_in(K.pack1(lay['w']))
    bd = dev_in(lay['b']) if a['bias'] else None
    ylen = N * a['ybs']
    t, body = out_buf(ylen)
    tn, nbody = out_buf(N * a['P'])
    tail = (N, a['P'], a['cin'], a['ksl'], a['xbs'], a['xss'], a['cout'], a['ybs'], a['yrs'], a['ysc'], a['yss'], lay['he'], a['flags'],
            SLOPE, EPS, _stream())
    nptr = ptr(nbody) if a['want_norm'] else None
    if a['xscale']:
        per = a['ksl'] * a['P']
        xs = dev_in(lay['xs'][first * per:(first + N) * per])
        rc = _lib().lf_conv1x1_fwd_scaled(ptr(xd), ptr(xs), ptr(wd), ptr(bd), ptr(body), nptr, *tail)
    else:
        rc = _lib().lf_conv1x1_fwd(ptr(xd), ptr(wd), ptr(bd), ptr(body), nptr, *tail)
    assert rc == 0, (rc, spec)
    check_guards(t, ylen)
    check_guards(tn, N * a['P'])
    flat = body.cpu()
    idx = K.pw_out_index(N, a['P'], a['cout'], a['ybs'], a['yrs'], a['ysc'], a['yss'])
    gaps = torch.ones(ylen, dtype=torch.bool)
    gaps[idx.reshape(-1)] = False
    assert bool(torch.isnan(flat[gaps]).all()), ('written between the rows', spec)
    out = {'y': flat[idx]}
    if (a['flags'] & PIXELNORM) and a['want_norm']:
        out['norm'] = nbody.cpu().reshape(N, a['P'])
    else:
        assert bool(torch.isnan(nbody).all())
    return out, flat


def _scaled_in_two_launches(spec):
    """lf_column_scale_fwd into a buffer of the operand's own layout (one call per sample and slice: P dense rows of Cin each;
    the pads between slices and samples stay NaN), then lf_conv1x1_fwd with the same flags: what lf_conv1x1_fwd_scaled
    replaced.  -> (the whole output buffer, norm_out)."""
    a, lay = K.pw_addr(spec), K.pw_layer(spec)
    P, cin, ksl = a['P'], a['cin'], a['ksl']
    xd, xs, wd, bd = dev_in(lay['xbuf']), dev_in(lay['xs']), dev_in(K.pack1(lay['w'])), dev_in(lay['b'])
    z = dev_in(torch.full((3 * a['xbs'],), NAN))
    for n in range(3):
        for sl in range(ksl):
            off = n * a['xbs'] + sl * a['xss']
            assert _lib().lf_column_scale_fwd(xd.data_ptr() + 4 * off, xs.data_ptr() + 4 * (n * ksl + sl) * P, z.data_ptr() + 4 * off,
                                              P, cin, _stream()) == 0
    t, body = out_buf(3 * a['ybs'])
    tn, nbody = out_buf(3 * P)
    assert _lib().lf_conv1x1_fwd(ptr(z), ptr(wd), ptr(bd), ptr(body), ptr(nbody), 3, P, cin, ksl, a['xbs'], a['xss'], a['cout'],
                                 a['ybs'], a['yrs'], a['ysc'], a['yss'], lay['he'], a['flags'], SLOPE, EPS, _stream()) == 0
    check_guards(t, 3 * a['ybs'])
    check_guards(tn, 3 * P)
    return body.cpu(), nbody.cpu().reshape(3, P)


def _pw_case(a):
    s = f"P={a['P']} K={a['ksl']}x{a['cin']} Cout={a['cout']}"
    if a['xscale']:
        s += ' scaled'
    if a['x_slice_pad'] or a['x_batch_pad']:
        s += f" x pads {a['x_slice_pad']}/{a['x_batch_pad']}"
    if a['row_gap']:
        s += f" row stride +{a['row_gap']}"
    if a['unfold']:
        s += f" unfolded D={a['unfold']}"
    if a['y_batch_pad']:
        s += f" y batch +{a['y_batch_pad']}"
    return s


@pytest.mark.parametrize('P', K.PW_P)
def test_conv1x1_forward_matches_fp64(P):
    worst = Worst('pw')
    repeated = set()
    try:
        for spec in K.pw_specs():
            a = K.pw_addr(spec)
            if a['P'] != P:
                continue
            form, case = K.pw_form(spec), _pw_case(a)
            got, flat = run_pw(spec)
            worst.add(form, case, K.ratios(K.expected(spec), got))
            one = K.pw_spec(**{**dict(spec[1:]), 'alone': 1})
            got1, _ = run_pw(one)
            worst.add(form, case, K.ratios(K.expected(one), got1))
            for k in got1:
                assert torch.equal(got1[k], got[k][1:2]), (spec, k)
            if form not in repeated:                                 # run to run, once per form
                repeated.add(form)
                assert torch.equal(run_pw(spec)[0]['y'], got['y']), spec
            if not a['want_norm']:
                with_norm, _ = run_pw(K.pw_spec(**{**dict(spec[1:]), 'want_norm': True}))
                assert torch.equal(with_norm['y'], got['y']), spec
            if a['xscale']:                                          # y and norm_out, bit for bit, dense and padded strides
                assert a['flags'] == BOTH and a['want_norm']
                y2, n2 = _scaled_in_two_launches(spec)
                assert torch.equal(flat, y2) and torch.equal(got['norm'], n2), spec
    finally:
        worst.report()


def run_pwb(spec, amax=False):
    a, G = K.pwb_addr(spec), K.pwb_layer(spec)
    alone, pf, D, P = a['alone'], a['prev_flags'], a['unfold'], a['P']
    gy = _pick(G['gy'], alone)
    N = gy.shape[0]
    ylen, vol = N * a['ybs'], D * P * 16
    gd, wd = dev_in(gy), dev_in(K.pack1(G['w'].t()))
    yp = nr = am = None
    td = dbody = None
    if pf:
        py, pn = G['prev'][pf]
        pbuf = torch.full((ylen,), NAN)
        for n in range(N):
            pbuf[n * a['ybs']:n * a['ybs'] + vol] = _pick(py, alone)[n].reshape(-1)
        yp = dev_in(pbuf)
        if pf == DOT:
            td, dbody = out_buf(ylen // 16)
            nr = dbody
        elif pn is not None:
            nbuf = torch.full((ylen // 16,), NAN)
            for n in range(N):
                nbuf[n * a['ybs'] // 16:n * a['ybs'] // 16 + D * P] = _pick(pn, alone)[n].reshape(-1)
            nr = dev_in(nbuf)
    if amax:
        am = torch.zeros(K.LF_AMAX_FLOATS, device=DEV)
    t, body = out_buf(ylen)
    rc = _lib().lf_conv1x1_bwd_data(ptr(gd), ptr(wd), ptr(body) if a['store'] else None, N, P, a['cg'], a['cout'], a['ybs'], 16, 16, a['yss'],
                                    G['he'], ptr(yp), ptr(nr), pf, SLOPE, ptr(am), _stream())
    assert rc == 0, (rc, spec)
    check_guards(t, ylen)
    flat = body.cpu()
    out = {}
    if a['store']:
        out['gx'] = torch.stack([flat[n * a['ybs']:n * a['ybs'] + vol].reshape(D, P, 16) for n in range(N)])
        pad = torch.cat([flat[n * a['ybs'] + vol:(n + 1) * a['ybs']] for n in range(N)])
        assert bool(torch.isnan(pad).all()), ('written between the samples', spec)
    else:
        assert bool(torch.isnan(flat).all()), ('y = NULL, yet written', spec)
    if pf == DOT:
        check_guards(td, ylen // 16)
        dflat = dbody.cpu()
        out['dot'] = torch.stack([dflat[n * a['ybs'] // 16:n * a['ybs'] // 16 + D * P].reshape(D, P) for n in range(N)])
        pad = torch.cat([dflat[n * a['ybs'] // 16 + D * P:(n + 1) * a['ybs'] // 16] for n in range(N)])
        assert bool(torch.isnan(pad).all())
    if amax:
        torch.cuda.synchronize()
        assert am.max().item() == out['gx'].abs().max().item(), ('amax_out is not max|gx|', spec)
    return out


@pytest.mark.parametrize('P', K.PW_P)
def test_conv1x1_data_gradient_matches_fp64(P):
    worst = Worst('pwb')
    raw = {}
    try:
        for spec in K.pwb_specs():
            a = K.pwb_addr(spec)
            if a['P'] != P:
                continue
            pf = a['prev_flags']
            form = K.pw_form(spec)
            case = f"P={P} D={a['unfold']} prev_flags {pf}" + (' y NULL' if not a['store'] else '') + (f" y batch +{a['y_batch_pad']}" if a['y_batch_pad'] else '')
            got = run_pwb(spec, amax=pf in K.PREV_FLAGS)
            worst.add(form, case, K.ratios(K.expected(spec), got))
            one = K.pwb_spec(**{**dict(spec[1:]), 'alone': 1})
            got1 = run_pwb(one, amax=pf in K.PREV_FLAGS)
            worst.add(form, case, K.ratios(K.expected(one), got1))
            for k in got1:
                assert torch.equal(got1[k], got[k][1:2]), (spec, k)
            if pf == 0:
                raw[a['unfold']] = got['gx']
                assert torch.equal(run_pwb(spec)['gx'], got['gx']), spec
            if pf == DOT and a['store']:                              # the gradient is stored as the raw launch stores it
                assert torch.equal(got['gx'], raw[a['unfold']]), spec
    finally:
        worst.report()


def test_conv1x1_refused_arguments():
    """Every refused argument of conv1x1_launch; nothing is written.  (prev_y with flags or a bias cannot be expressed through
    lf_conv1x1_bwd_data.)"""
    L = _lib()
    s = _stream()
    P, C = 65, 16
    x, w, b = dev_in(torch.randn(3 * 3 * P * C)), dev_in(torch.zeros(256, 48)), dev_in(torch.zeros(256))
    xs = dev_in(torch.ones(3 * 3 * P))
    t, y = out_buf(3 * P * 256)
    tn, nrm = out_buf(3 * P)
    base = dict(N=3, P=P, cin=C, ksl=1, xbs=P * C, xss=0, cout=C, ybs=P * C, yrs=C, ysc=K.PLAIN, yss=0, flags=BOTH)

    def fwd(xp=None, wp=None, yp='y', scale=None, **kw):
        a = {**base, **kw}
        yp = y.data_ptr() if yp == 'y' else yp
        tail = (a['N'], a['P'], a['cin'], a['ksl'], a['xbs'], a['xss'], a['cout'], a['ybs'], a['yrs'], a['ysc'], a['yss'], 0.25, a['flags'],
                SLOPE, EPS, s)
        if scale is not None:
            return L.lf_conv1x1_fwd_scaled(xp or x.data_ptr(), scale or None, wp or w.data_ptr(), b.data_ptr(), yp, nrm.data_ptr(), *tail)
        return L.lf_conv1x1_fwd(xp or x.data_ptr(), wp or w.data_ptr(), b.data_ptr(), yp, nrm.data_ptr(), *tail)
    for kw in ({'N': 0}, {'P': 0}, {'P': -1}, {'cin': 0}, {'ksl': 0}, {'cout': 0}, {'ysc': 0}, {'ysc': -16},
               {'yrs': C - 1}, {'cout': 32, 'ysc': 16, 'yrs': 12, 'yss': P * 16}, {'cout': 129, 'yrs': 129, 'ybs': P * 129},
               {'yp': None}):
        assert fwd(**kw) == LF_EINVAL, kw
    assert fwd(scale=0) == LF_EINVAL                                  # lf_conv1x1_fwd_scaled without its factors
    for kw in ({'xp': x.data_ptr() + 4}, {'yp': y.data_ptr() + 4}, {'wp': w.data_ptr() + 8},
               {'cin': 6, 'ksl': 3, 'xss': P * 6, 'xbs': 3 * P * 6}, {'xbs': P * C + 2}, {'ksl': 3, 'xss': P * C + 1, 'xbs': 3 * P * C + 4},
               {'cin': 5, 'scale': xs.data_ptr(), 'xbs': P * 5}):
        assert fwd(**kw) == LF_EALIGN, kw
    # the data gradient with a fused producer: 16-channel records, strides in whole records, a norm where one is read
    D = 5
    gy, wt = dev_in(torch.randn(3 * P * C)), dev_in(torch.zeros(128, 16))
    py, pn = dev_in(torch.zeros(3 * D * P * 16 + 64)), dev_in(torch.ones(3 * D * P + 64))
    good = dict(cout=16 * D, ybs=D * P * 16, yrs=16, ysc=16, yss=P * 16, pf=BOTH, py=py.data_ptr(), pn=pn.data_ptr(), yp=y.data_ptr())

    def bwd(**kw):
        a = {**good, **kw}
        return L.lf_conv1x1_bwd_data(gy.data_ptr(), wt.data_ptr(), a['yp'], 3, P, C, a['cout'], a['ybs'], a['yrs'], a['ysc'], a['yss'], 0.25,
                                     a['py'], a['pn'], a['pf'], SLOPE, None, s)
    for kw in ({'ysc': 32}, {'yrs': 32}, {'cout': 16 * D + 4}, {'ybs': D * P * 16 + 8}, {'yss': P * 16 + 4}, {'py': py.data_ptr() + 4},
               {'pn': None}, {'pn': None, 'pf': PIXELNORM}, {'pf': DOT | LRELU}, {'pf': DOT, 'pn': None}, {'yp': None}):
        assert bwd(**kw) == LF_EINVAL, kw
    check_guards(t, y.numel())
    check_guards(tn, nrm.numel())
    assert bool(torch.isnan(y).all()) and bool(torch.isnan(nrm).all()), 'a refused call wrote'
    assert bool((pn[:3 * D * P] == 1).all())                          # (LF_EPI_DOT would have written here)
    assert bwd() == 0 and bwd(pf=LRELU, pn=None) == 0                 # the arguments they were derived from are accepted
    torch.cuda.synchronize()


# ---- the misreadings, on the device -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(K.MISREADINGS))
def test_misreadings_are_rejected_on_the_device(name):
    desc, key = K.MISREADINGS[name]
    if desc[0] == 'fwd3':
        got = run_fwd3(desc)
    elif desc[0] == 'bwd3':
        got = run_bwd3(desc)
    elif desc[0] == 'pw':
        got = run_pw(desc)[0]
    else:
        got = run_pwb(desc)
    true = K.ratios(K.expected(desc), got)[key][2]
    wrong = K.misread_ratio(name, got)
    print(f'[conv-fp64] misreading {name}: err/bound {true:.2f} against the restatement, {wrong:.1f} against the misreading')
    assert true <= 1.0 and wrong > 1.0, (true, wrong)
