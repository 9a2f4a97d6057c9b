"""The autograd layers of the training step (BASELINE cfg 5, latentfusion_amd/ops_train.py) against the plain formula in
fp64, element by element: the 16 -> 16 layers (_Conv16AC), the two-layer Block with and without the chained epilogue
backward, the sum-of-parts convolution of the ConvGRU gates (_Conv3x3Sum16), the resampler under the storage policy
(_ResampleAC) and the fused ConvGRU recurrence (_GruFuse).

Reference: the oracle's expressions (lf_oracle.nets) evaluated in fp64 on the CPU and differentiated by fp64 autograd, on
operands rounded as the kernels see them: bf16 for the inputs and weights the kernels stage as bf16 under autocast, fp32
biases, and the upstream gradient rounded to bf16 where the layer receives it in bf16.

Metric (`check`), on the output and on every gradient returned: e = |got - ref| / (|ref| + rms(ref)) per element;
max(e) <= tau and the fraction of elements with e > 2^-8 <= f_max.  Every test also hands `check` deliberately wrong fp64
references (a LeakyReLU' of slope 1, a PixelNorm' without its projection term, the data gradient with its last z-plane
zeroed, the bias gradient summed over N - 1 samples, a transposed weight gradient, ...) and asserts that the same bound
rejects the device result against each of them: an error confined to one plane of tiles fails the test.

Bounds (BOUNDS below): calibrated once on an MI355X, tau = 2x the largest observed max(e) over the cases of its row,
rounded up to a power of two; f_max likewise from the largest observed fraction (0 where none was seen).  Under autocast
the reference forms each pre-activation as autocast does, bf16(bf16(conv) * he) + bias, so that LeakyReLU' takes the
kernel's branch where the exact value lies within a rounding of zero; the Block's stored activation is bf16.  Observed maxima (max e / fraction):

    conv16-ac         out 0.0061 / 2.5e-05  gx 0.015 / 0.019      gw 0.0069 / 0.016     gb 0.0026 / 0
    conv16-fp32       out 1.2e-06 / 0       gx 1.1e-06 / 0        gw 1.1e-06 / 0        gb 2.7e-07 / 0
    block             out 0.0077 / 0.00015  gx 0.11 / 0.17        gw 0.019 / 0.17       gb 0.0081 / 0.31
    sum16-ac          out 9.2e-07 / 0       gx 0.0077 / 0.0088    gw 0.0063 / 0.0036    gb 3.1e-07 / 0
    sum16-fp32        out 1e-06 / 0         gx 1.1e-06 / 0        gw 1.3e-06 / 0        gb 2.5e-07 / 0
    resample          out 0.003 / 0         gx 0.0037 / 0
    gru2-ac           out 0.0093 / 0.0032   gx 0.011 / 0.021      gw 0.013 / 0.097      gb 0.0049 / 0.19
    gru4-ac           out 0.014 / 0.011     gx 0.015 / 0.065      gw 0.021 / 0.17       gb 0.007 / 0.12
    gru2-fp32         out 1e-06 / 0         gx 1.2e-06 / 0        gw 9.8e-07 / 0        gb 4.7e-07 / 0
    gru4-fp32         out 1.1e-06 / 0       gx 1.5e-06 / 0        gw 1.5e-06 / 0        gb 6.5e-07 / 0
"""
import functools
import zlib

import pytest
import torch
import torch.nn.functional as F

from lf_oracle import nets

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SMALL = (1, 16, 5, 9, 13)          # 585 voxels: below _wgrad_bf16_ok's 8192, the fp32-MFMA weight gradient
MID = (3, 16, 7, 12, 10)           # three samples, 840 voxels each
LARGE = (2, 16, 33, 20, 17)        # 11220 voxels: the bf16 weight gradient on the side stream
ULP = 2.0 ** -8

# (tau_max, f_max) per (layer, precision, quantity); see the module docstring for the measurements behind them
BOUNDS = {
    ('conv16', True): {'out': (2 ** -6, 2 ** -14), 'gx': (2 ** -5, 2 ** -4), 'gw': (2 ** -6, 2 ** -5), 'gb': (2 ** -7, 0.0)},
    ('conv16', False): {'out': (2 ** -18, 0.0), 'gx': (2 ** -18, 0.0), 'gw': (2 ** -18, 0.0), 'gb': (2 ** -20, 0.0)},
    ('block', True): {'out': (2 ** -6, 2 ** -11), 'gx': (2 ** -2, 2 ** -1), 'gw': (2 ** -4, 2 ** -1), 'gb': (2 ** -5, 2 ** 0)},
    ('sum16', True): {'out': (2 ** -19, 0.0), 'gx': (2 ** -6, 2 ** -5), 'gw': (2 ** -6, 2 ** -7), 'gb': (2 ** -20, 0.0)},
    ('sum16', False): {'out': (2 ** -18, 0.0), 'gx': (2 ** -18, 0.0), 'gw': (2 ** -18, 0.0), 'gb': (2 ** -20, 0.0)},
    ('resample', True): {'out': (2 ** -7, 0.0), 'gx': (2 ** -7, 0.0)},
    ('gru2', True): {'out': (2 ** -5, 2 ** -7), 'gx': (2 ** -5, 2 ** -4), 'gw': (2 ** -5, 2 ** -2), 'gb': (2 ** -6, 2 ** -1)},
    ('gru4', True): {'out': (2 ** -5, 2 ** -5), 'gx': (2 ** -5, 2 ** -2), 'gw': (2 ** -4, 2 ** -1), 'gb': (2 ** -6, 2 ** -2)},
    ('gru2', False): {'out': (2 ** -18, 0.0), 'gx': (2 ** -18, 0.0), 'gw': (2 ** -18, 0.0), 'gb': (2 ** -20, 0.0)},
    ('gru4', False): {'out': (2 ** -18, 0.0), 'gx': (2 ** -18, 0.0), 'gw': (2 ** -18, 0.0), 'gb': (2 ** -19, 0.0)},
}


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def bf(t):
    return t.to(torch.bfloat16).float()


def rel_err(got, ref):
    """e = |got - ref| / (|ref| + rms(ref)) per element (0 / 0 counts as 0, x / 0 as inf)."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    diff = (got - ref).abs()
    den = ref.abs() + ref.pow(2).mean().sqrt()
    return torch.where(den > 0, diff / den.clamp_min(1e-300), torch.where(diff > 0, float('inf'), 0.0))


def check(name, got, ref, bound, wrong=()):
    """Asserts max(e) <= tau and frac(e > 2^-8) <= f_max for the device result `got` against the fp64 reference, and that
    the same bound REJECTS `got` against every deliberately wrong reference in `wrong` ((label, tensor) pairs)."""
    tau, fmax = bound
    e = rel_err(got, ref)
    m, f = e.max().item(), (e > ULP).double().mean().item()
    assert m <= tau and f <= fmax, f'{name}: max e {m:.3g} (tau {tau:.3g}), frac(e > 2^-8) {f:.3g} (f_max {fmax:.3g})'
    for label, wref in wrong:
        ew = rel_err(got, wref)
        mw, fw = ew.max().item(), (ew > ULP).double().mean().item()
        assert mw > tau or fw > fmax, f'{name}: the bound does not reject the wrong reference "{label}" (max e {mw:.3g})'
    return m, f


@pytest.fixture
def switches():
    """Saves and restores every module switch the tests below flip."""
    from latentfusion_amd import ops, ops_train
    names = ('RING_BLOCK_FWD', 'RING_DGRAD', 'CHAIN_EPILOGUE', 'PW16', 'GRU_RING', 'GRU_WGRAD_CHUNK', 'WGRAD_STREAM')
    saved = {n: getattr(ops_train, n) for n in names}
    storage = ops.BF16_STORAGE
    try:
        yield ops_train
    finally:
        for n, v in saved.items():
            setattr(ops_train, n, v)
        ops.BF16_STORAGE = storage


# ---- fp64 references --------------------------------------------------------------------------------------------------
def _act(pre, flags, slope_bwd=nets.SLOPE, pn_proj=True):
    """The layer's epilogue: nets.act_norm (LeakyReLU + PixelNorm), LeakyReLU alone or nothing; `slope_bwd` / `pn_proj`
    build the wrong references (same forward, a LeakyReLU' of another slope / a PixelNorm' without its projection)."""
    if not flags:
        return pre
    if slope_bwd == nets.SLOPE and pn_proj:
        return nets.act_norm(pre) if flags == 3 else F.leaky_relu(pre, nets.SLOPE)
    a = F.leaky_relu(pre, slope_bwd) + (F.leaky_relu(pre, nets.SLOPE) - F.leaky_relu(pre, slope_bwd)).detach()
    if flags == 3:
        nrm = torch.sqrt(torch.mean(a ** 2, dim=1, keepdim=True) + 1e-8)
        a = a / (nrm if pn_proj else nrm.detach())
    return a


def _leaf(t, grad):
    return t.detach().double().clone().requires_grad_(grad)


def _grads(out, gy, leaves):
    gs = torch.autograd.grad(out, [t for t in leaves if t.requires_grad], gy, allow_unused=True)
    it = iter(gs)
    return [next(it) if t.requires_grad else None for t in leaves]


def _pre(x, sd, prefix, ac):
    """nets.eq_conv in fp64.  ac: its value as autocast forms it, bf16(bf16(conv) * he) + bias in fp32 (the convolution's
    output is a bf16 tensor), passed straight through in the backward.  The branch LeakyReLU' takes depends on that
    rounded value wherever the exact one lies within a rounding of zero."""
    w = sd[prefix + '.module.weight']
    pre = nets.eq_conv(x, sd, prefix, w.shape[2] // 2)
    if not ac:
        return pre
    he = torch.tensor((2.0 / w[0].numel()) ** 0.5, dtype=torch.float32)
    acc = F.conv3d(x.detach(), w.detach(), None, 1, w.shape[2] // 2)
    rounded = bf(bf(acc.float()) * he) + sd[prefix + '.bias'].detach().float().view(1, -1, 1, 1, 1)
    return pre + (rounded.double() - pre).detach()


def ref_conv16(x, w, b, flags, gy, ac=True, **variant):
    """(y, gx, gw, gb, gp) of act(eq_conv(x, w, b)) in fp64; gp = the pre-activation gradient (per sample)."""
    x, w = _leaf(x, True), _leaf(w, True)
    b = _leaf(b if b is not None else torch.zeros(w.shape[0]), True)
    pre = _pre(x, {'c.module.weight': w, 'c.bias': b}, 'c', ac)
    y = _act(pre, flags, **variant)
    gx, gw, gb, gp = _grads(y, gy.double(), [x, w, b, pre])
    return y.detach(), gx, gw, gb, gp


def _plane_zeroed(t, plane=-1):
    t = t.clone()
    t[:, :, plane] = 0
    return t


def _heaviest_plane(t):
    return int(t.detach().double().pow(2).sum(dim=(0, 1, 3, 4)).argmax())


def _bias_over_first(gp, n):
    """The bias gradient summed over the first n samples only (a wrong reference)."""
    return gp[:n].sum(dim=(0, 2, 3, 4))


# ---- _Conv16AC through ops.conv3x3 / ops.conv1x1 ---------------------------------------------------------------------
# (kernel, flags, shape, x storage, variant): variants flip one condition of a branch in _Conv16AC.backward
CONV16_CASES = (
    [(3, fl, sh, xd, '') for fl in (3, 1, 0) for sh in (SMALL, LARGE) for xd in ('bf16', 'fp32')]
    + [(3, 3, MID, 'bf16', ''), (3, 1, MID, 'fp32', '')]
    + [(3, 3, LARGE, 'fp32', 'channels_first'), (3, 3, LARGE, 'bf16', 'no_bias'), (3, 0, LARGE, 'bf16', 'no_bias'),
       (3, 3, LARGE, 'bf16', 'bias_frozen'), (3, 0, SMALL, 'bf16', 'bias_frozen'), (3, 3, LARGE, 'bf16', 'weight_frozen'),
       (3, 3, SMALL, 'fp32', 'weight_frozen'), (3, 3, LARGE, 'bf16', 'x_frozen'), (3, 1, SMALL, 'bf16', 'x_frozen'),
       (3, 3, LARGE, 'bf16', 'ring_block_fwd_off'), (3, 3, SMALL, 'fp32', 'ring_block_fwd_off'),
       (3, 3, LARGE, 'bf16', 'ring_dgrad_off'), (3, 0, SMALL, 'bf16', 'ring_dgrad_off')]
    + [(1, fl, sh, xd, v) for fl in (0, 1) for sh in (SMALL, LARGE) for xd, v in (('bf16', ''), ('fp32', ''), ('bf16', 'pw16_off'))]
    + [(1, 3, sh, xd, '') for sh in (SMALL, LARGE) for xd in ('bf16', 'fp32')]
    + [(1, 0, MID, 'bf16', 'no_bias'), (1, 1, LARGE, 'bf16', 'bias_frozen'), (1, 0, LARGE, 'bf16', 'x_frozen'),
       (1, 1, SMALL, 'bf16', 'weight_frozen')]
)


def _conv16_case(k, flags, shape, xdtype, variant, autocast, switches):
    from latentfusion_amd import ops
    switches.RING_BLOCK_FWD = variant != 'ring_block_fwd_off'
    switches.RING_DGRAD = variant != 'ring_dgrad_off'
    switches.PW16 = variant != 'pw16_off'
    seed = _seed(k, flags, shape, xdtype, variant, autocast)
    g = torch.Generator().manual_seed(seed)
    x0 = torch.randn(shape, generator=g)
    w0 = torch.randn(16, 16, k, k, k, generator=g)
    b0 = torch.randn(16, generator=g) * 0.3
    gy0 = torch.randn(shape, generator=g)
    has_b, b_grad = variant != 'no_bias', variant not in ('no_bias', 'bias_frozen')
    w_grad, x_grad = variant != 'weight_frozen', variant != 'x_frozen'
    x = x0.to(DEV)
    if variant != 'channels_first':
        x = ops.cl(x)
    if xdtype == 'bf16':
        x = x.to(torch.bfloat16)
    x.requires_grad_(x_grad)
    w = w0.to(DEV).requires_grad_(w_grad)
    b = b0.to(DEV).requires_grad_(b_grad) if has_b else None
    with ops.autocast(autocast):
        y = (ops.conv3x3 if k == 3 else ops.conv1x1)(x, w, b, lrelu=bool(flags & 1), pixelnorm=bool(flags & 2))
    assert y.dtype == (torch.bfloat16 if autocast else torch.float32)
    y.backward(gy0.to(DEV).to(y.dtype))
    rnd = bf if autocast else (lambda t: t)
    args = (rnd(x0), rnd(w0), b0 if has_b else None, flags, rnd(gy0), autocast)
    ry, rgx, rgw, rgb, rgp = ref_conv16(*args)
    return (y, x.grad, w.grad, b.grad if b is not None else None), (ry, rgx, rgw, rgb, rgp), args


@pytest.mark.parametrize('k,flags,shape,xdtype,variant', CONV16_CASES)
def test_conv16_layer_vs_fp64(k, flags, shape, xdtype, variant, switches):
    """One 16 -> 16 layer under the bf16 autocast + storage policy, every backward branch of _Conv16AC on its own."""
    got, ref, args = _conv16_case(k, flags, shape, xdtype, variant, True, switches)
    _check_conv16(got, ref, args, BOUNDS[('conv16', True)], shape[0])


@pytest.mark.parametrize('k,flags,shape', [(3, 3, SMALL), (3, 1, LARGE), (3, 0, MID), (1, 3, MID), (1, 1, SMALL), (1, 0, LARGE)])
def test_conv16_layer_fp32_vs_fp64(k, flags, shape, switches):
    """The same layers without autocast (the fp32 kernels): fp32-sized bounds."""
    got, ref, args = _conv16_case(k, flags, shape, 'fp32', '', False, switches)
    _check_conv16(got, ref, args, BOUNDS[('conv16', False)], shape[0])


def _check_conv16(got, ref, args, bounds, n):
    y, gx, gw, gb = got
    ry, rgx, rgw, rgb, rgp = ref
    x0, w0, b0, flags, gy0, _ = args
    wrong_act = []
    if flags:
        wrong_act.append(('LeakyReLU\' slope 1', ref_conv16(*args, slope_bwd=1.0)))
    if flags == 3:
        wrong_act.append(('PixelNorm\' without projection', ref_conv16(*args, pn_proj=False)))
    check('out', y, ry, bounds['out'], [('output with its last z-plane zeroed', _plane_zeroed(ry))])
    if gx is not None:
        check('gx', gx, rgx, bounds['gx'], [('gx with its last z-plane zeroed', _plane_zeroed(rgx))]
              + [(lbl, r[1]) for lbl, r in wrong_act])
    if gw is not None:
        check('gw', gw, rgw, bounds['gw'], [('gw transposed', rgw.transpose(0, 1))] + [(lbl, r[2]) for lbl, r in wrong_act])
    if gb is not None:
        check('gb', gb, rgb, bounds['gb'], [(f'gb over {n - 1} of {n} samples', _bias_over_first(rgp, n - 1))]
              + [(lbl, r[3]) for lbl, r in wrong_act])


# ---- Block topologies (CHAIN_EPILOGUE on, and off as the control) ------------------------------------------------------
BLOCK_TOPOLOGIES = ('plain', 'no_bias', 'second_consumer', 'forward_hook', 'retain_graph', 'producer_frozen',
                    'consumer_frozen', 'grad_x_only')


def _ref_block(x0, sd, g2, g1, topology, variant=None):
    """fp64 Block (nets.eq_conv / nets.act_norm, the body of nets.block) and its gradients for the topology's loss;
    `variant` applies a wrong epilogue backward to conv1 (the producer)."""
    frozen = {'no_bias': ('b1.bias', 'b2.bias'), 'producer_frozen': ('b1.module.weight', 'b1.bias'),
              'consumer_frozen': ('b2.module.weight', 'b2.bias')}.get(topology, ())
    x = _leaf(x0, True)
    p = {k: _leaf(v, k not in frozen) for k, v in sd.items()}
    pre1 = _pre(x, p, 'b1', True)
    y1 = _act(pre1, 3, **(variant or {}))
    y1s = y1 + (bf(y1.detach()).double() - y1).detach()      # (stored in bf16: what conv2 stages and its input gradient sees)
    y2 = nets.act_norm(_pre(y1s, p, 'b2', True))
    if topology in ('second_consumer', 'forward_hook'):
        loss = (y2 * g2).sum() + (y1 * g1).sum()
    elif topology == 'retain_graph':
        loss = (y1 * g1).sum()                                   # the SECOND backward of the device run
    else:
        loss = (y2 * g2).sum()
    leaves = [x, p['b1.module.weight'], p['b1.bias'], p['b2.module.weight'], p['b2.bias'], pre1]
    return y2.detach(), dict(zip(('x', 'w1', 'b1', 'w2', 'b2', 'gp1'), _grads(loss, None, leaves)))


@pytest.mark.parametrize('chain', [True, False])
@pytest.mark.parametrize('shape', [MID, LARGE])
@pytest.mark.parametrize('topology', BLOCK_TOPOLOGIES)
def test_block_vs_fp64(topology, shape, chain, switches):
    """A Block of two 16 -> 16 layers with LeakyReLU + PixelNorm on a bf16 input: the chained epilogue backward (conv2's data
    gradient applies conv1's epilogue backward) must meet the fp64 bound in every topology of the autograd graph -- a second
    consumer of conv1's output (explicit or through a forward hook), a second backward through a retained graph that reaches
    conv1 only, a bias-free Block, one of the two layers frozen, a gradient of the input alone."""
    from latentfusion_amd import ops
    from latentfusion_amd.modules import EqualizedConv3d
    from latentfusion_amd.modules.blocks import Block
    switches.CHAIN_EPILOGUE = chain
    torch.manual_seed(7)
    conv = functools.partial(EqualizedConv3d, bias=False) if topology == 'no_bias' else EqualizedConv3d
    blk = Block(16, 16, conv_module=conv).to(DEV)
    with torch.no_grad():
        for c in (blk.conv1, blk.conv2):
            if c.bias is not None:
                c.bias.normal_(0.0, 0.3)
    if topology == 'producer_frozen':
        blk.conv1.requires_grad_(False)
    if topology == 'consumer_frozen':
        blk.conv2.requires_grad_(False)
    g = torch.Generator().manual_seed(_seed(topology, shape))
    x0 = bf(torch.randn(shape, generator=g))
    g2 = bf(torch.randn(shape, generator=g))
    g1 = bf(torch.randn(shape, generator=g) * 0.5)
    x = ops.cl(x0.to(DEV)).to(torch.bfloat16).requires_grad_(True)
    seen = []
    if topology in ('forward_hook', 'retain_graph'):
        blk.conv1.register_forward_hook(lambda mod, inp, out: seen.append(out))
    with ops.autocast(True):
        if topology == 'second_consumer':
            y1 = blk.conv1(x, fuse_act=True, fuse_norm=True)
            y2 = blk.conv2(y1, fuse_act=True, fuse_norm=True, chain=True)
        else:
            y2 = blk(x)
            y1 = seen[0] if seen else None
    loss2 = (y2.float() * g2.to(DEV)).sum()
    if topology in ('second_consumer', 'forward_hook'):
        (loss2 + (y1.float() * g1.to(DEV)).sum()).backward()
    elif topology == 'retain_graph':
        # the first backward runs the chained form; the second reaches conv1 alone
        loss2.backward(retain_graph=True)
        for t in [x] + list(blk.parameters()):
            t.grad = None
        (y1.float() * g1.to(DEV)).sum().backward()
    elif topology == 'grad_x_only':
        x.grad, = torch.autograd.grad(loss2, [x])
    else:
        loss2.backward()
    sd = {'b1.module.weight': bf(blk.conv1.module.weight.detach().cpu()),
          'b1.bias': blk.conv1.bias.detach().cpu() if blk.conv1.bias is not None else torch.zeros(16),
          'b2.module.weight': bf(blk.conv2.module.weight.detach().cpu()),
          'b2.bias': blk.conv2.bias.detach().cpu() if blk.conv2.bias is not None else torch.zeros(16)}
    ry, rg = _ref_block(x0, sd, g2.double(), g1.double(), topology)
    bounds = BOUNDS[('block', True)]
    wrong = {lbl: _ref_block(x0, sd, g2.double(), g1.double(), topology, v)[1]
             for lbl, v in (('conv1 LeakyReLU\' slope 1', {'slope_bwd': 1.0}), ('conv1 PixelNorm\' without projection', {'pn_proj': False}))}
    check('out', y2, ry, bounds['out'], [('output with its last z-plane zeroed', _plane_zeroed(ry))])
    got = {'x': x.grad, 'w1': blk.conv1.module.weight.grad, 'b1': blk.conv1.bias.grad if blk.conv1.bias is not None else None,
           'w2': blk.conv2.module.weight.grad, 'b2': blk.conv2.bias.grad if blk.conv2.bias is not None else None}
    if topology == 'grad_x_only':
        got = {'x': got['x']}
    for k, t in got.items():
        want = rg[k]
        assert (t is None) == (want is None), (k, t is None, want is None)
        if t is None:
            continue
        extra = [(lbl, w[k]) for lbl, w in wrong.items() if w[k] is not None and k in ('x', 'w1', 'b1')]
        if k == 'x':
            extra.append(('gx with its last z-plane zeroed', _plane_zeroed(want)))
        if k == 'b1':
            extra.append((f'conv1 gb over {shape[0] - 1} of {shape[0]} samples', _bias_over_first(rg['gp1'], shape[0] - 1)))
        if k in ('w1', 'w2'):
            extra.append(('gw transposed', want.transpose(0, 1)))
        if k == 'b2':
            extra.append(('conv2 gb negated', -want))
        check(k, t, want, bounds['gb' if k[0] == 'b' else 'gw' if k[0] == 'w' else 'gx'], extra)


# ---- _Conv3x3Sum16 through ops_train.conv3x3_sum16 ---------------------------------------------------------------------
# (input widths of the weight, the parts' columns or None = back to back, addend, which inputs want a gradient)
SUM16_CASES = [((16, 16), None, False, 'all'), ((16, 16, 3), None, False, 'all'), ((16, 3, 16), ((0, 16), (19, 16)), True, 'all'),
               ((16, 16, 3), None, False, 'parts'), ((16, 16), None, False, 'weight'), ((16, 16, 3), None, False, 'bias'),
               ((16, 3, 16), ((0, 16), (19, 16)), True, 'parts')]


@pytest.mark.parametrize('autocast', [True, False])
@pytest.mark.parametrize('shape', [SMALL, LARGE])
@pytest.mark.parametrize('widths,cols,addend,wants', SUM16_CASES)
def test_conv3x3_sum16_vs_fp64(widths, cols, addend, wants, shape, autocast, switches):
    """sum_p conv(parts[p], W[:, cols[p]]) * he + b (+ addend) against one fp64 convolution over the concatenation: the GRU
    gate shape (16, 16, 3) with its 3 channels zero-padded to 16, columns that do not cover W plus an addend, and each
    subset of gradients (parts only, weight only, bias only)."""
    from latentfusion_amd import ops, ops_train
    g = torch.Generator().manual_seed(_seed(widths, cols, addend, wants, shape, autocast))
    cin = sum(widths)
    if cols is None:
        cols_ = [(sum(widths[:i]), wdt) for i, wdt in enumerate(widths)]
    else:
        cols_ = list(cols)
    N, _, D, H, W = shape
    w0 = torch.randn(16, cin, 3, 3, 3, generator=g)
    b0 = torch.randn(16, generator=g) * 0.3
    parts0 = []
    for c0, wdt in cols_:
        p = torch.zeros(shape)
        p[:, :wdt] = torch.randn(N, wdt, D, H, W, generator=g)
        parts0.append(p)
    a0 = torch.randn(N, 16, D, H, W, generator=g) if addend else None
    gy0 = torch.randn(N, 16, D, H, W, generator=g)
    want_p, want_w, want_b = wants in ('all', 'parts'), wants in ('all', 'weight'), wants in ('all', 'bias')
    parts = [ops.cl(p.to(DEV)).requires_grad_(want_p) for p in parts0]
    w = w0.to(DEV).requires_grad_(want_w)
    b = None if addend else b0.to(DEV).requires_grad_(want_b)
    a = ops.cl(a0.to(DEV)).requires_grad_(True) if addend else None
    with ops.autocast(autocast):
        y = ops_train.conv3x3_sum16(w, b, None if cols else widths, parts, cols=cols, addend=a)
    y.backward(ops.cl(gy0.to(DEV)))
    # fp64: one convolution over the concatenation of the parts' real channels, on W's columns they stand for
    rnd = bf if autocast else (lambda t: t)
    xs = [_leaf(rnd(p[:, :wdt]), True) for p, (c0, wdt) in zip(parts0, cols_)]
    wr = _leaf(rnd(w0), True)
    br = _leaf(b0 if b is not None else torch.zeros(16), True)
    ar = _leaf(a0, True) if addend else None
    wsel = torch.cat([wr[:, c0:c0 + wdt] for c0, wdt in cols_], dim=1)
    # (the He constant is that of W's full fan-in, not of the columns taken)
    yr = nets.eq_conv(torch.cat(xs, dim=1), {'c.module.weight': wsel * (wsel[0].numel() / (cin * 27)) ** 0.5, 'c.bias': br}, 'c', 1)
    if ar is not None:
        yr = yr + ar
    gr = _grads(yr, gy0.double(), xs + [wr, br] + ([ar] if ar is not None else []))
    bounds = BOUNDS[('sum16', autocast)]
    check('out', y, yr, bounds['out'], [('output with its last z-plane zeroed', _plane_zeroed(yr.detach())),
                                        ('output without its last part', yr.detach() - _part_out(xs[-1], wr, cols_[-1], cin))])
    for i, (p, (c0, wdt)) in enumerate(zip(parts, cols_)):
        assert (p.grad is not None) == want_p
        if want_p:
            check(f'gpart{i}', p.grad[:, :wdt], gr[i], bounds['gx'], [('gx with its last z-plane zeroed', _plane_zeroed(gr[i])),
                                                                      ('gx of the transposed weight', _gx_transposed(gy0, wr, cols_[i], cin))])
    gw, gb = gr[len(xs)], gr[len(xs) + 1]
    assert (w.grad is not None) == want_w
    if want_w:
        covered = torch.zeros(cin, dtype=torch.bool)
        for c0, wdt in cols_:
            covered[c0:c0 + wdt] = True
        assert torch.all(w.grad[:, ~covered.to(DEV)] == 0)          # columns of other calls stay zero
        check('gw', w.grad, gw, bounds['gw'], [('gw transposed', _swap_in_out(gw)), ('gw without the last sample', _gw_first(xs, gy0, wr, cols_, cin, N - 1))])
    if b is not None:
        assert (b.grad is not None) == want_b
        if want_b:
            check('gb', b.grad, gb, bounds['gb'], [(f'gb over {N - 1} of {N} samples', gy0[:N - 1].double().sum(dim=(0, 2, 3, 4))),
                                                   ('gb negated', -gb)])
    if addend:
        check('gaddend', a.grad, gy0, bounds['out'], [('gaddend with its last z-plane zeroed', _plane_zeroed(gy0))])


def _part_out(x, w, col, cin):
    c0, wdt = col
    return F.conv3d(x.detach(), w.detach()[:, c0:c0 + wdt], None, 1, 1) * (2.0 / (cin * 27)) ** 0.5


def _gx_transposed(gy, w, col, cin):
    """The data gradient of the part through W^T's channel block in the wrong orientation (16 x 16 blocks only)."""
    c0, wdt = col
    wb = w.detach()[:, c0:c0 + wdt]
    if wdt == 16:
        wb = wb.transpose(0, 1).flip(2, 3, 4)
    else:
        wb = -wb
    return F.conv_transpose3d(gy.double(), wb, None, 1, 1) * (2.0 / (cin * 27)) ** 0.5


def _swap_in_out(gw):
    out = gw.clone()
    out[:, :16] = gw[:, :16].transpose(0, 1)
    return out


def _gw_first(xs, gy, w, cols, cin, n):
    """The weight gradient over the first n samples only (the columns the parts cover)."""
    gw = torch.zeros_like(w.detach())
    if n == 0:
        return gw
    x = torch.cat([t.detach()[:n] for t in xs], dim=1).requires_grad_(False)
    wsel = torch.cat([w.detach()[:, c0:c0 + wdt] for c0, wdt in cols], dim=1).requires_grad_(True)
    y = F.conv3d(x, wsel, None, 1, 1) * (2.0 / (cin * 27)) ** 0.5
    g, = torch.autograd.grad(y, [wsel], gy[:n].double())
    j = 0
    for c0, wdt in cols:
        gw[:, c0:c0 + wdt] = g[:, j:j + wdt]
        j += wdt
    return gw


# ---- _ResampleAC through ops.resample_o2c / resample_c2o ----------------------------------------------------------------
@pytest.mark.parametrize('leave', [False, True])
@pytest.mark.parametrize('src', ['fp32', 'bf16'])
@pytest.mark.parametrize('shared', [True, False])
@pytest.mark.parametrize('kind', ['o2c', 'c2o'])
def test_resample_vs_fp64(kind, shared, src, leave):
    """The resampler under the storage policy (bf16 destination, volume gradient in the source's storage) against the
    oracle's o2c / c2o in fp64: one volume shared by the cameras (expanded with stride 0) or one per camera, an fp32 or
    bf16 source, cameras whose samples stay inside the volume or leave it (the viewport shifted sideways)."""
    import lf_oracle as O
    from oracle_util import in_fp64
    from latentfusion_amd import ops
    from latentfusion_amd.modules.geometry import Camera, c2o_coefficients, o2c_coefficients
    S, N = 21, 3
    g = torch.Generator().manual_seed(_seed(kind, shared, src, leave))
    log_q = torch.randn(N, 3, generator=g) * 0.6
    t = torch.cat((torch.randn(N, 2, generator=g) * 0.05, 1.0 + 0.2 * torch.rand(N, 1, generator=g)), 1)
    K = torch.tensor([[615.1436, 0.0, 315.3623, 0.0], [0.0, 615.4991, 251.5415, 0.0], [0.0, 0.0, 1.0, 0.0]]).expand(N, -1, -1)
    ocam = O.Cam(K.clone(), log_q, t).zoom(None, S, 2.0)
    vp = ocam.viewport.detach().clone()
    if leave:
        vp[:, 0::2] += 0.6 * (vp[:, 2:3] - vp[:, 0:1])
    cam = Camera(ocam.K.to(DEV), None, 0.5, vp.to(DEV), width=640, height=480, log_quaternion=ocam.log_q.detach().to(DEV),
                 translation=ocam.t.detach().to(DEV))
    coef = (o2c_coefficients if kind == 'o2c' else c2o_coefficients)(cam, 1.0)
    vol0 = torch.randn(1 if shared else N, 16, S, S, S, generator=g)
    if src == 'bf16':
        vol0 = bf(vol0)
    gy0 = bf(torch.randn(N, 16, S, S, S, generator=g))
    vol = ops.cl(vol0.to(DEV))
    vol = (vol.to(torch.bfloat16) if src == 'bf16' else vol).requires_grad_(True)
    with ops.autocast(True):
        y = (ops.resample_o2c if kind == 'o2c' else ops.resample_c2o)(vol.expand(N, -1, -1, -1, -1) if shared else vol, coef)
    assert y.dtype == torch.bfloat16
    y.backward(gy0.to(DEV).to(torch.bfloat16))
    assert vol.grad.dtype == vol.dtype
    ocam64 = O.Cam(ocam.K.double(), ocam.log_q.detach().double(), ocam.t.detach().double(), viewport=vp.double())

    def ref(gy):
        v = _leaf(vol0, True)
        out = in_fp64(lambda: (nets.o2c if kind == 'o2c' else nets.c2o)(v.expand(N, -1, -1, -1, -1), ocam64))
        gv, = torch.autograd.grad(out, [v], gy.double())
        return out.detach(), gv
    ry, rg = ref(gy0)
    gy_wrong = gy0.clone()
    gy_wrong[-1] = 0
    bounds = BOUNDS[('resample', True)]
    check('out', y, ry, bounds['out'], [('output with its last z-plane zeroed', _plane_zeroed(ry)),
                                        ('output of the cameras in another order', ry.roll(1, 0))])
    check('gvol', vol.grad, rg, bounds['gx'], [('gvol with one z-plane zeroed', _plane_zeroed(rg, _heaviest_plane(rg))),
                                               ('gvol without the last camera', ref(gy_wrong)[1])])


# ---- _GruFuse through fusion.GRUFuser(16) ------------------------------------------------------------------------------
@pytest.mark.parametrize('V, mode', [(V, mode) for mode in ('autocast_ring', 'autocast', 'fp32') for V in (2, 4)]
                         + [(4, 'autocast_ring_chunk2')])
def test_gru_fuser_vs_fp64(V, mode, switches):
    """The fused ConvGRU recurrence (one autograd node; GRU_RING: the multi-output ring kernels) against nets.gru_step in
    fp64: output, gradient of the per-view volumes and of the six gate parameters.  The error grows with the number of
    views (the state is carried through V - 1 steps), so the bounds are per V.  autocast_ring_chunk2: the ring recurrence's
    weight gradients in two chunks of GRU_WGRAD_CHUNK = 2 steps (steps 3, 2 and step 1), the second one accumulating the gate
    gradients' sums (lf_sum_views_bf16 with `accumulate`) -- same bounds, same wrong references."""
    from latentfusion_amd import ops
    from latentfusion_amd.recon import fusion
    switches.GRU_RING = mode.startswith('autocast_ring')
    if mode == 'autocast_ring_chunk2':
        switches.GRU_WGRAD_CHUNK = 2
    ac = mode != 'fp32'
    torch.manual_seed(11)
    fu = fusion.GRUFuser(16).to(DEV)
    assert fu.fused_recurrence
    with torch.no_grad():
        for gate in (fu.gru.update_gate, fu.gru.reset_gate, fu.gru.out_gate):
            gate.bias.normal_(0.0, 0.3)
    D, H, W = 11, 20, 41                                     # 9020 voxels: the bf16 weight-gradient kernel
    g = torch.Generator().manual_seed(_seed(V, mode))
    rnd = bf if ac else (lambda t: t)
    z0 = rnd(torch.randn(1, V, 16, D, H, W, generator=g))
    gout = torch.randn(1, 1, 16, D, H, W, generator=g)
    z = z0.to(DEV).requires_grad_(True)
    with ops.autocast(ac):
        out, _ = fu(z, None, None, None)
    assert out.dtype == torch.float32
    (out * gout.to(DEV)).sum().backward()
    names = [f'gru.{gt}.{p}' for gt in ('update_gate', 'reset_gate', 'out_gate') for p in ('module.weight', 'bias')]
    params = dict(fu.named_parameters())
    coords = rnd(nets.voxel_coords_zyx(z0[:, 0]))

    def ref(steps=V):
        sd = {k: _leaf(rnd(v.detach().cpu()) if k.endswith('weight') else v.detach().cpu(), True) for k, v in params.items()}
        zr = _leaf(z0, True)
        h = zr[:, 0]
        for i in range(1, steps):
            h = nets.gru_step(sd, 'gru', torch.cat((zr[:, i], coords.double()), dim=1), h)
        grads = _grads(h, gout[:, 0].double(), [zr] + [sd[k] for k in names])
        return h.detach(), grads[0], dict(zip(names, grads[1:]))
    ry, rgz, rgp = ref()
    bounds = BOUNDS[(f'gru{V}', ac)]
    check('out', out[:, 0], ry, bounds['out'], [('output with its last z-plane zeroed', _plane_zeroed(ry)),
                                                ('output without the last view', ref(V - 1)[0])])
    check('gz', z.grad.reshape(V, 16, D, H, W), rgz.reshape(V, 16, D, H, W), bounds['gx'],
          [('gz with its last z-plane zeroed', _plane_zeroed(rgz.reshape(V, 16, D, H, W))),
           ('gz of the views in another order', rgz.reshape(V, 16, D, H, W).roll(1, 0))])
    swap = {'update_gate': 'reset_gate', 'reset_gate': 'update_gate', 'out_gate': 'update_gate'}
    for k in names:
        gate = k.split('.')[1]
        other = k.replace(gate, swap[gate])
        kind = 'gb' if k.endswith('bias') else 'gw'
        check(k, params[k].grad, rgp[k], bounds[kind], [(f'the gradient of {other}', rgp[other]), (f'{k} negated', -rgp[k])])


def test_gru_fuser_small_volume_takes_the_step_recurrence(switches):
    """A volume below the bf16 weight-gradient kernel's 8192 voxels (5 x 12 x 20, two views, autocast with bf16 storage,
    trainable gates): the ring recurrence stores its gate gradients in bf16 and has no weight-gradient kernel for them there, so
    GRU_RING leaves such a volume to the step recurrence -- output and every gradient are those of GRU_RING = False, bit for bit."""
    from latentfusion_amd import ops
    from latentfusion_amd.recon import fusion
    torch.manual_seed(12)
    fu = fusion.GRUFuser(16).to(DEV)
    with torch.no_grad():
        for gate in (fu.gru.update_gate, fu.gru.reset_gate, fu.gru.out_gate):
            gate.bias.normal_(0.0, 0.3)
    g = torch.Generator().manual_seed(_seed('gru-small'))
    z0 = torch.randn(1, 2, 16, 5, 12, 20, generator=g).to(DEV).to(torch.bfloat16)
    gout = torch.randn(1, 1, 16, 5, 12, 20, generator=g).to(DEV)

    def run(ring):
        switches.GRU_RING = ring
        z = z0.clone().requires_grad_(True)
        fu.zero_grad(set_to_none=True)
        with ops.autocast(True):
            out, _ = fu(z, None, None, None)
        (out * gout).sum().backward()
        return [out.detach(), z.grad] + [p.grad for p in fu.parameters()]
    on, off = run(True), run(False)
    assert len(on) == 8 and all(t is not None for t in on)
    for a, b in zip(on, off):
        assert a.dtype == b.dtype and torch.equal(a, b)
