"""tests/conv_direct_cases.py checked without a GPU: the tap-by-tap restatement of the direct convolutions, of their fused
data gradients and of the row kernels against the oracle's expressions (lf_oracle.nets: eq_conv, act_norm, pixel_norm) in fp64
and their fp64 autograd on the plain-layout cases; the fp32 chain inside its own bound at every case (finite, shapes agree);
every misreading rejected when the fp32 chain stands in for the kernel; the weight layouts; and the restated dispatch reaching
every kernel form the GPU module is about."""
import math

import pytest
import torch
import torch.nn.functional as F

import conv_direct_cases as K
from conv_direct_cases import DOT, LRELU, PIXELNORM
from lf_oracle import nets

BOTH = LRELU | PIXELNORM


def _ncdhw(t, dims):
    """channels-last [N][D][H][W][C] -> the oracle's NC[D]HW."""
    t = t.permute(0, 4, 1, 2, 3)
    return t[:, :, 0] if dims == 2 else t


def _act(pre, flags):
    if flags == BOTH:
        return nets.act_norm(pre)
    if flags == LRELU:
        return F.leaky_relu(pre, nets.SLOPE)
    return nets.pixel_norm(pre) if flags == PIXELNORM else pre


def test_constants_are_the_oracles():
    assert K.SLOPE == nets.SLOPE and K.EPS == 1e-8


@pytest.mark.parametrize('key', K.layers3(), ids=lambda k: f'{k[0]}d-{k[1]}to{k[2]}-{"x".join(map(str, k[3]))}')
def test_forward_restatement_is_the_oracle_in_fp64(key):
    dims, cin, cout, shape = key
    L = K.layer3(*key)
    sd = {'c.module.weight': L['w'].double(), 'c.bias': L['b'].double()}
    pre = nets.eq_conv(_ncdhw(L['x'].double(), dims), sd, 'c', 1)
    assert math.isclose(L['he'], math.sqrt(2.0 / L['w'][0].numel()))
    for flags, with_bias, _ in K.fwd3_variants(cout):
        if not with_bias:
            continue
        e = K.fwd3_expected(('fwd3', dims, cin, cout, shape, 3, None, flags, True))
        want = _act(pre, flags)
        got = _ncdhw(e['y'][0], dims)
        assert (got - want).abs().max().item() <= 1e-12 * (1 + want.abs().max().item())
        if flags & PIXELNORM:
            act = F.leaky_relu(pre, nets.SLOPE) if flags & LRELU else pre
            r = torch.sqrt((act ** 2).mean(1) + 1e-8)
            assert (_ncdhw(e['norm'][0][..., None], dims)[:, 0] - r).abs().max().item() <= 1e-12
        # sample 1 alone is sample 1 of the batch
        e1 = K.fwd3_expected(('fwd3', dims, cin, cout, shape, 3, 1, flags, True))
        assert torch.equal(e1['y'][0], e['y'][0][1:2])


@pytest.mark.parametrize('key', K.grads3() + [(3, 16, 16, (8, 16, 32))], ids=lambda k: f'{k[0]}d-{k[1]}to{k[2]}-{"x".join(map(str, k[3]))}')
def test_gradient_restatement_is_fp64_autograd_of_the_oracle(key):
    dims, cc, cp, shape = key
    G = K.grad3(*key)
    sd0 = {'p.module.weight': G['w0'].double().reshape(cp, 8, *([1] * dims)), 'p.bias': torch.zeros(cp, dtype=torch.float64)}
    sd = {'c.module.weight': G['w'].double(), 'c.bias': torch.zeros(cc, dtype=torch.float64)}
    gy = _ncdhw(G['gy'].double(), dims)
    for pf in (0,) + K.PREV_FLAGS:
        pre = nets.eq_conv(_ncdhw(G['x0'].double(), dims), sd0, 'p', 0).detach().requires_grad_(True)
        yprev = _act(pre, pf) if pf else pre
        (nets.eq_conv(yprev, sd, 'c', 1) * gy).sum().backward()
        e = K.bwd3_expected(('bwd3', dims, cc, cp, shape, 3, None, pf))
        got, want = _ncdhw(e['gx'][0], dims), pre.grad
        if pf:
            # the restatement is handed y_prev and norm ROUNDED TO FP32 (the kernel's inputs): 2^-24 relative on each
            tol = 4e-7 * K.record_max(e['gx'][0])
            assert torch.equal(G['prev'][pf][0].double(), yprev.detach().permute(0, *range(2, 2 + dims), 1).reshape(G['prev'][pf][0].shape).float().double())
            assert ((e['gx'][0] - want.permute(0, *range(2, 2 + dims), 1).reshape(e['gx'][0].shape)).abs() <= tol + 1e-12).all()
        else:
            assert (got - want).abs().max().item() <= 1e-12 * (1 + want.abs().max().item())
    # the all-zero producer row: y_prev = 0, norm = sqrt(eps)
    z = G['zmask'][..., 0]
    assert int(z.sum()) == 1
    assert (G['prev'][BOTH][0][z] == 0).all() and G['prev'][BOTH][1][z].item() == torch.tensor(1e-8, dtype=torch.float64).sqrt().float().item()


@pytest.mark.parametrize('P', [1, 65])
def test_pointwise_restatement_is_the_oracle_in_fp64(P):
    seen = 0
    for spec in K.pw_specs():
        a = K.pw_addr(spec)
        if a['P'] != P or a['xscale'] or not a['bias']:
            continue
        L = K.pw_layer(spec)
        X = L['xbuf'][K.pw_in_index(3, P, a['cin'], a['ksl'], a['xbs'], a['xss'])].double()          # [3][P][K]
        sd = {'c.module.weight': L['w'].double().reshape(a['cout'], a['K'], 1, 1), 'c.bias': L['b'].double()}
        want = _act(nets.eq_conv(X.permute(0, 2, 1)[..., None], sd, 'c', 0), a['flags'])[..., 0].permute(0, 2, 1)
        got = K.pw_expected(spec)['y'][0]
        assert (got - want).abs().max().item() <= 1e-12 * (1 + want.abs().max().item())
        seen += 1
    assert seen >= 40


def test_pointwise_addressing_restated():
    # folded depth: element (p, k = s*Cin + c) of sample n lies at n*xbs + s*xss + p*Cin + c
    idx = K.pw_in_index(2, 3, 4, 2, 100, 40)
    assert idx[1, 2, 1 * 4 + 3].item() == 100 + 40 + 2 * 4 + 3
    # unfolded output: channel co = d*16 + c of pixel p lies at n*ybs + d*yss + p*16 + c -- a channels-last volume [n][d][p][16]
    a = K.pw_addr(K.pw_spec(P=7, cin=16, cout=80, unfold=5, y_batch_pad=48))
    out = K.pw_out_index(3, 7, 80, a['ybs'], a['yrs'], a['ysc'], a['yss'])
    vol = (torch.arange(3).reshape(3, 1, 1, 1) * a['ybs'] + torch.arange(5 * 7 * 16).reshape(1, 5, 7, 16))
    assert torch.equal(out.reshape(3, 7, 5, 16).permute(0, 2, 1, 3), vol)
    # rows wider than Cout: the gap columns are no channel's address
    a = K.pw_addr(K.pw_spec(P=7, cin=20, cout=16, row_gap=4))
    out = K.pw_out_index(3, 7, 16, a['ybs'], a['yrs'], a['ysc'], a['yss'])
    assert out.unique().numel() == out.numel() and int(out.max()) == 3 * 7 * 20 - 5 and not bool(((out % 20) >= 16).any())


def test_pointwise_gradient_restatement_is_fp64_autograd_of_the_oracle():
    P, D = 65, 5
    G = K.pwb_layer(K.pwb_spec(P=P, unfold=D))
    w = G['w'].double()                                               # [cg][D*16], k = d*16 + c
    for pf in (0,) + K.PREV_FLAGS + (DOT,):
        pre = ((G['x0'].double() @ G['w0'].double().t()) * math.sqrt(2.0 / 8)).requires_grad_(True)   # [3][D][P][16]
        act = pf if pf in K.PREV_FLAGS else (BOTH if pf == DOT else 0)
        yprev = _act(pre.permute(0, 3, 1, 2), act).permute(0, 2, 3, 1) if act else pre
        scale = torch.ones(3, D, P, 1, dtype=torch.float64, requires_grad=True)     # LF_EPI_DOT: the gradient of a per-voxel factor
        X = (yprev.detach() * scale if pf == DOT else yprev).permute(0, 2, 1, 3).reshape(3, P, D * 16)
        ((X @ w.t()) * G['he'] * G['gy'].double()).sum().backward()
        e = K.pwb_expected(K.pwb_spec(P=P, unfold=D, prev_flags=pf))
        if pf == DOT:
            assert ((e['dot'][0] - scale.grad[..., 0]).abs() <= 4e-7 * e['dot'][2] + 1e-12).all()
        else:
            tol = (4e-7 if pf else 0.0) * K.record_max(e['gx'][0]) + 1e-12
            assert ((e['gx'][0] - pre.grad).abs() <= tol).all()


def test_row_restatements_are_the_oracle_in_fp64():
    for rows, C in ((65, 17), (3, 256)):
        x, gy = K.rows_inputs(rows, C)
        e = K.pixelnorm_expected(x)
        want = nets.pixel_norm(x.double().t()[None]).squeeze(0).t()
        assert (e['y'][0] - want).abs().max().item() <= 1e-12
        z = min(1, rows - 1)
        assert (e['y'][0][z] == 0).all() and e['norm'][0][z].item() == math.sqrt(1e-8)
        for flags in K.PREV_FLAGS:
            pre = x.double().clone().requires_grad_(True)
            y = _act(pre.t()[None], flags)[0].t()
            (y * gy.double()).sum().backward()
            y32 = y.detach().float()
            n32 = torch.sqrt((F.leaky_relu(x.double(), nets.SLOPE) if flags & LRELU else x.double()).pow(2).mean(1) + 1e-8).float()
            eb = K.rows_bwd_expected(gy, y32, n32 if flags & PIXELNORM else None, flags)
            assert ((eb['gp'][0] - pre.grad).abs() <= 4e-7 * eb['gp'][2] + 1e-12).all()


def _all_descs():
    for dims, cin, cout, shape in K.layers3():
        for flags, with_bias, _ in K.fwd3_variants(cout):
            for alone in (None, 1):
                yield ('fwd3', dims, cin, cout, shape, 3, alone, flags, with_bias)
    for dims, cc, cp, shape in K.grads3():
        for pf in (0,) + K.PREV_FLAGS:
            for alone in (None, 1):
                yield ('bwd3', dims, cc, cp, shape, 3, alone, pf)
    for spec in K.pw_specs() + K.pwb_specs():
        yield spec


def test_fp32_chain_is_inside_its_own_bound_at_every_case():
    n = 0
    for desc in _all_descs():
        e = K.expected(desc)
        for key, (err, e32, r) in K.ratios(e, K.stand_in(e)).items():
            assert r <= 1.0 and err <= e32, (desc, key, err, e32, r)
        n += 1
    assert n > 1000


@pytest.mark.parametrize('name', sorted(K.MISREADINGS))
def test_misreadings_are_rejected(name):
    desc, key = K.MISREADINGS[name]
    e = K.expected(desc)
    stand_in = K.stand_in(e)
    assert K.ratios(e, stand_in)[key][2] <= 1.0                       # accepted against the true reference
    r = K.misread_ratio(name, stand_in)
    assert r >= 10.0, r


def test_row_misreadings_are_rejected():
    x, gy = K.rows_inputs(65, 17)
    e = K.pixelnorm_expected(x)
    wrong = K.with_true_e32(K.pixelnorm_expected(x, 'mean_over_16'), e)
    assert K.ratios(wrong, K.stand_in(e))['y'][2] >= 10.0
    y, n = e['y'][0].float(), e['norm'][0].float()
    eb = K.rows_bwd_expected(gy, y, n, BOTH)
    wrong = K.with_true_e32(K.rows_bwd_expected(gy, y, n, BOTH, 'norm_squared'), eb)
    assert K.ratios(eb, K.stand_in(eb))['gp'][2] <= 1.0 and K.ratios(wrong, K.stand_in(eb))['gp'][2] >= 10.0


def test_weight_layouts_are_the_headers():
    g = torch.Generator().manual_seed(0)
    w = torch.randn(5, 3, 3, 3, 3, generator=g)
    p = K.pack3(w)
    assert p.shape == (27, 16, 16) and p[(2 * 3 + 0) * 3 + 1, 4, 2] == w[4, 2, 2, 0, 1] and p[:, 5:].abs().sum() == 0 and p[:, :, 3:].abs().sum() == 0
    pt = K.pack3_t(w)
    assert pt.shape == (27, 16, 16) and pt[(2 * 3 + 0) * 3 + 1, 2, 4] == w[4, 2, 0, 2, 1]
    w2 = torch.randn(48, 9, 3, 3, generator=g)
    assert K.pack3(w2).shape == (9, 64, 16) and K.pack3(torch.randn(132, 72, 3, 3, generator=g)).shape == (9, 192, 80)
    assert K.pack1(torch.randn(200, 35, generator=g)).shape == (256, 48)
    assert [K.cout_padded3(c) for c in (1, 16, 17, 32, 33, 64, 65, 132)] == [16, 16, 32, 32, 64, 64, 128, 192]
    assert [K.cout_padded1(c) for c in (2, 16, 24, 48, 64, 80, 128, 200, 320)] == [16, 16, 32, 64, 64, 128, 128, 256, 384]


def test_every_form_is_reached():
    reached = K.forms_reached()
    missing = [f for f in K.REQUIRED_FORMS if f not in reached]
    assert not missing, (missing, sorted(reached))
    # the thresholds the forms hang on
    assert K.form3x3(3, (5, 9, 91), 16, 16) == 'conv3x3_c16_kernel<3>' and 5 * 9 * 91 == 4095
    assert K.form3x3(3, (8, 16, 32), 16, 16) == 'conv3d_c16_persistent_kernel' and 8 * 16 * 32 == 4096
    assert K.walk_batch(256) == 19 and K.persistent_tiles(K.WALK_SHAPE, 19) == 513        # ceil(27 * 19 / 256) = 3, ceil(27 * 18 / 256) = 2
    assert K.persistent_tiles_per_workgroup(K.WALK_SHAPE, 19, 256) == 3
    assert K.persistent_tiles_per_workgroup((10, 19, 40), 3, 256) == 1            # what the cubic 16^3 / 20^3 tests ran
    assert K.nt1x1(256, fused=True) == 4 and K.nt1x1(256) == 8 and K.nt1x1(80, fused=True) == 8
