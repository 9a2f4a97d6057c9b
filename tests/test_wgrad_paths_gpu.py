"""The weight-gradient routes of ops_train (one planned launch object, `_Wgrad`, behind conv_bwd_weight and the autograd
layers) and the scratch contract of the entry points they call.

Routes: what `_Wgrad` and `conv_bwd_weight` return is bit-identical to a direct ctypes call of the entry point the route
names (`_Wgrad.entry`), on that entry's own scratch query -- fp32 storage, the bf16 policy with operands pre-rounded to bf16
in all four storage variants (`io`), WIDE_WGRAD on and off.  Shapes: (1,16,9,20,50) -- 9000 voxels, just over the 8192
threshold of the tiled 16 -> 16 kernels and ragged against their 2 x 8 x 16 tile on every axis; (2,16,5,20,50) -- two samples
and an odd number of tile planes, so tile columns restart mid-range; (1,16,5,9,13) -- below the threshold, generic kernel;
35 input channels -- the chunked path with its ragged, zero-padded last chunk; 64 -> 64 at 8 x 8 in 2-D -- the wide route.

Every route is also compared with the fp64 contraction gw[tap][co][ci] = he * sum_v gp[v][co] * x[v + tap][ci] on the CPU,
with the bounds of the existing tests of the same entry points: the bf16 MFMA max |err| < 2e-6 * max |ref|
(test_autocast_gpu.test_weight_gradient_on_the_bf16_mfma), the fp32 kernels max(e) <= 2^-18 with no element above 2^-8,
e = |got - ref| / (|ref| + rms(ref)) (test_train_layers_fp64_gpu BOUNDS[('conv16', False)]['gw'], test_wide_wgrad_gpu TAU;
the bias sums 2^-20, BOUNDS[('conv16', False)]['gb']).

Scratch: an entry point returns LF_ENOSPC and writes nothing four bytes below its own query, and runs on exactly the query;
lf_conv_bwd_weight_scratch_bytes also covers the bf16 entries.  Domain: the bf16 query is non-zero exactly on the bf16
kernel's domain (host calls only), and ops_train._wgrad_bf16_ok says the same."""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
HE = 0.37
LF_ENOSPC = -3
TILED = (1, 16, 9, 20, 50)
TILED2 = (2, 16, 5, 20, 50)
SMALL = (1, 16, 5, 9, 13)
WIDE2D = (1, 64, 8, 8)
TAPS = {0: 1, 2: 9, 3: 27}


def bf(t):
    return t.to(torch.bfloat16).float()


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last_3d if t.dim() == 5 else torch.channels_last)


def operands(shape, cin=None, rounded=False):
    """(x, gp) on the CPU (fp32, made once, never modified): gp has `shape`, x has `cin` channels (default: as gp)."""
    return _operands(shape, cin, bool(rounded))


def reference(shape, cin=None, rounded=False):
    """fp64: gw[tap][co][ci] = HE * sum_v gp[v][co] * x[v + tap][ci], one explicit sum per tap over the zero-padded input;
    computed once per case."""
    return _reference(shape, cin, bool(rounded))


@functools.lru_cache(maxsize=None)
def _operands(shape, cin, rounded):
    g = torch.Generator().manual_seed(sum(shape) + (cin or 0))
    x = torch.randn((shape[0], cin or shape[1]) + shape[2:], generator=g)
    gp = torch.randn(shape, generator=g) * 1e-2
    return (bf(x), bf(gp)) if rounded else (x, gp)


@functools.lru_cache(maxsize=None)
def _reference(shape, cin, rounded):
    x, gp = (t.double() for t in operands(shape, cin, rounded))
    sp = shape[2:]
    xp = torch.nn.functional.pad(x, (1, 1) * len(sp))
    taps = []
    for tap in range(TAPS[len(sp)]):
        o = (tap // 9, (tap // 3) % 3, tap % 3)[3 - len(sp):]
        xs = xp[(slice(None), slice(None)) + tuple(slice(a, a + n) for a, n in zip(o, sp))]
        taps.append(HE * torch.einsum('nk...,nc...->kc', gp, xs))
    return torch.stack(taps)


def device_operands(shape, cin=None, rounded=False, io=0):
    x, gp = (_cl(t.to(DEV)) for t in operands(shape, cin, rounded))
    return (_cl(x.to(torch.bfloat16)) if io & 1 else x), (_cl(gp.to(torch.bfloat16)) if io & 2 else gp)


def geom(gp):
    dims = gp.dim() - 2
    return (dims, gp.shape[0]) + ((1,) if dims == 2 else ()) + tuple(gp.shape[2:])


def direct(entry, x, gp, cin, io=None):
    """The entry point called through ctypes on its own scratch query."""
    from latentfusion_amd import _lib
    L = _lib.lib()
    shape = geom(gp) + (cin, gp.shape[1])
    query = {'lf_conv_bwd_weight': 'lf_conv_bwd_weight_scratch_bytes', 'lf_conv_bwd_weight_bf16_io': 'lf_conv_bwd_weight_bf16_scratch_bytes',
             'lf_conv_bwd_weight_wide': 'lf_conv_bwd_weight_wide_scratch_bytes'}[entry]
    nb = getattr(L, query)(*shape)
    assert nb > 0 and nb % 4 == 0, (entry, nb)
    scr = torch.empty(nb // 4, device=DEV)
    gw = torch.empty(TAPS[shape[0]], gp.shape[1], cin, device=DEV)
    tail = (ctypes.c_float(HE),) + ((io,) if io is not None else ()) + (torch.cuda.current_stream().cuda_stream,)
    rc = getattr(L, entry)(x.data_ptr(), gp.data_ptr(), gw.data_ptr(), scr.data_ptr(), nb, *shape, *tail)
    assert rc == 0, (entry, rc)
    return gw


def planned(x, gp, cin, bf16):
    """(_Wgrad object, its result) for the operands, routed as conv_bwd_weight routes them."""
    from latentfusion_amd import ops_train as T
    dims, N, D, H, W = geom(gp)
    wg = T._Wgrad(dims, N, D, H, W, cin, gp.shape[1], gp.device, HE, bf16=bf16, wide=T._wide_wgrad_ok(x, gp, dims, cin, gp.shape[1]))
    gw = torch.empty(TAPS[dims], gp.shape[1], cin, device=DEV)
    wg(x, gp, gw)
    return wg, gw


def rel_err(got, ref):
    """e = |got - ref| / (|ref| + rms(ref)) per element (tests/test_train_layers_fp64_gpu.py)."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return (got - ref).abs() / (ref.abs() + ref.pow(2).mean().sqrt())


def assert_fp32_bound(name, got, ref, tau=2.0 ** -18):
    e = rel_err(got, ref)
    m, f = e.max().item(), (e > 2.0 ** -8).double().mean().item()
    print(f'{name}: max e {m:.3g}, frac(e > 2^-8) {f:.3g}')
    assert m <= tau and f <= 0.0, (name, m, f)


def assert_bf16_bound(name, got, ref):
    scale = ref.abs().max().item()
    m = (got.cpu().double() - ref).abs().max().item()
    print(f'{name}: max |err| {m:.3g} = {m / scale:.3g} max |ref|')
    assert m < 2e-6 * scale, (name, m, scale)


@pytest.mark.parametrize('shape,entry', [(TILED, 'lf_conv_bwd_weight'), (TILED2, 'lf_conv_bwd_weight'), (SMALL, 'lf_conv_bwd_weight')],
                         ids=['tiled', 'tiled2', 'small'])
def test_fp32_routes(shape, entry):
    from latentfusion_amd import ops_train as T
    x, gp = device_operands(shape)
    wg, gw = planned(x, gp, 16, bf16=False)
    assert wg.entry == entry
    want = direct(entry, x, gp, 16)
    assert torch.equal(gw, want)
    gw2, gb = T.conv_bwd_weight(x, gp, 3, 16, HE, want_bias=True, bf16=False)
    assert torch.equal(gw2, want)
    assert_fp32_bound(f'fp32 {shape}', gw, reference(shape))
    # the bias launch shares the object's scratch: column sums of gp
    ref_b = operands(shape)[1].double().sum(dim=(0, 2, 3, 4))
    assert_fp32_bound(f'bias {shape}', gb, ref_b, tau=2.0 ** -20)
    assert torch.equal(gb, T.bias_grad(gp, 3))


@pytest.mark.parametrize('shape', [TILED, TILED2], ids=['tiled', 'tiled2'])
def test_bf16_routes_all_storage_variants(shape):
    from latentfusion_amd import ops_train as T
    ref = reference(shape, None, True)
    outs = []
    for io in range(4):
        x, gp = device_operands(shape, None, True, io)
        wg, gw = planned(x, gp, 16, bf16=True)
        assert wg.entry == 'lf_conv_bwd_weight_bf16_io'
        assert torch.equal(gw, direct(wg.entry, x, gp, 16, io)), io
        gw2, gb = T.conv_bwd_weight(x, gp, 3, 16, HE, want_bias=False, bf16=True)
        assert gb is None and torch.equal(gw2, gw), io
        assert_bf16_bound(f'bf16 {shape} io{io}', gw, ref)
        outs.append(gw)
    assert all(torch.equal(o, outs[0]) for o in outs[1:])          # same values from either storage: same bits
    # the ambient policy selects the same route
    from latentfusion_amd import ops
    x, gp = device_operands(shape, None, True)
    with ops.autocast():
        gw3, _ = T.conv_bwd_weight(x, gp, 3, 16, HE, want_bias=False)
    assert torch.equal(gw3, outs[0])


def test_bf16_policy_below_the_threshold_stays_on_the_fp32_kernel():
    from latentfusion_amd import ops_train as T
    x, gp = device_operands(SMALL, None, True)
    wg, gw = planned(x, gp, 16, bf16=True)
    assert wg.entry == 'lf_conv_bwd_weight' and not T._wgrad_bf16_ok(gp, 3, 16, 16)
    assert torch.equal(gw, direct(wg.entry, x, gp, 16))
    gw2, _ = T.conv_bwd_weight(x, gp, 3, 16, HE, want_bias=False, bf16=True)
    assert torch.equal(gw2, gw)
    assert_fp32_bound('small, bf16 values', gw, reference(SMALL, None, True))
    with pytest.raises(TypeError):                                    # bf16 STORAGE is the bf16 entry's alone
        wg(_cl(x.to(torch.bfloat16)), gp, gw)


@pytest.mark.parametrize('bf16', [False, True], ids=['fp32', 'bf16'])
def test_chunked_ragged_input(bf16):
    """35 input channels (the ConvGRU gates: 16 + 3 + 16): chunks of 16, the last one zero-padded, each on the tiled kernels."""
    from latentfusion_amd import ops_train as T
    x, gp = device_operands(TILED, 35, bf16)
    gw, gb = T.conv_bwd_weight(x, gp, 3, 35, HE, want_bias=False, bf16=bf16)
    assert gb is None and gw.shape == (27, 16, 35)
    entry = 'lf_conv_bwd_weight_bf16_io' if bf16 else 'lf_conv_bwd_weight'
    parts = []
    for c0 in (0, 16, 32):
        xc = torch.zeros_like(gp)
        xc[:, :min(16, 35 - c0)] = x[:, c0:c0 + 16]
        parts.append(direct(entry, _cl(xc), gp, 16, 0 if bf16 else None)[:, :, :min(16, 35 - c0)])
    assert torch.equal(gw, torch.cat(parts, dim=2))
    (assert_bf16_bound if bf16 else assert_fp32_bound)(f'35 channels, bf16={bf16}', gw, reference(TILED, 35, bf16))


@pytest.fixture
def wide_switch():
    from latentfusion_amd import ops_train
    saved = ops_train.WIDE_WGRAD
    yield ops_train
    ops_train.WIDE_WGRAD = saved


@pytest.mark.parametrize('on', [True, False], ids=['wide_on', 'wide_off'])
def test_wide_route(wide_switch, on):
    T = wide_switch
    T.WIDE_WGRAD = on
    x, gp = device_operands(WIDE2D)
    wg, gw = planned(x, gp, 64, bf16=False)
    assert wg.entry == ('lf_conv_bwd_weight_wide' if on else 'lf_conv_bwd_weight')
    assert torch.equal(gw, direct(wg.entry, x, gp, 64))
    gw2, _ = T.conv_bwd_weight(x, gp, 2, 64, HE, want_bias=False)
    assert torch.equal(gw2, gw)
    assert_fp32_bound(f'64 -> 64 2-D, wide {on}', gw, reference(WIDE2D))


# ---- scratch contract ---------------------------------------------------------------------------------------------------
# (entry, query, gp shape, Cin): the tiled 16 -> 16 kernel, the generic kernel, the bias sums (x == NULL), the bf16 entry
SCRATCH_CASES = [
    ('lf_conv_bwd_weight', 'lf_conv_bwd_weight_scratch_bytes', TILED, 16),
    ('lf_conv_bwd_weight', 'lf_conv_bwd_weight_scratch_bytes', SMALL, 16),
    ('lf_conv_bwd_weight', 'lf_conv_bwd_weight_scratch_bytes', TILED, 0),
    ('lf_conv_bwd_weight_bf16_io', 'lf_conv_bwd_weight_bf16_scratch_bytes', TILED, 16),
]


@pytest.mark.parametrize('entry,query,shape,cin', SCRATCH_CASES, ids=['tiled', 'generic', 'bias', 'bf16_io'])
def test_scratch_contract(entry, query, shape, cin):
    from latentfusion_amd import _lib
    L = _lib.lib()
    x, gp = device_operands(shape)
    dims, N, D, H, W = (0, 1, 1, 1, gp.numel() // 16) if cin == 0 else geom(gp)     # (the bias: rows x 16, as bias_grad asks)
    nb = getattr(L, query)(dims, N, D, H, W, cin, 16)
    assert nb > 0 and nb % 4 == 0
    scr = torch.empty(nb // 4, device=DEV)
    gw = torch.full((TAPS[dims] * 16 * max(cin, 1),), 12345.0, device=DEV)
    tail = (ctypes.c_float(HE),) + ((0,) if entry.endswith('_io') else ()) + (None,)

    def call(nbytes):
        return getattr(L, entry)(x.data_ptr() if cin else None, gp.data_ptr(), gw.data_ptr(), scr.data_ptr(), nbytes, dims, N, D, H, W, cin, 16, *tail)
    assert call(nb - 4) == LF_ENOSPC
    torch.cuda.synchronize()
    assert bool((gw == 12345.0).all()), 'an error return wrote to gw'
    assert call(nb) == 0
    torch.cuda.synchronize()
    assert not bool((gw == 12345.0).any())


def test_fp32_query_covers_both_tiled_forms():
    from latentfusion_amd import _lib
    L = _lib.lib()
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    for shape in (TILED, TILED2, (32, 16, 128, 128, 128)):
        args = (3, shape[0]) + shape[2:] + (16, 16)
        nb = L.lf_conv_bwd_weight_scratch_bytes(*args)
        nb16 = L.lf_conv_bwd_weight_bf16_scratch_bytes(*args)
        assert nb16 > 0 and nb >= nb16                                # one buffer serves the bf16 entries too
        assert nb >= cus * 27 * 256 * 4                               # the fp32 kernel: one 27 x 256 block per CU
        assert nb16 % (cus * 27 * 256 * 4) == 0                       # whole blocks, a whole number of workgroups per CU


# ---- domain of the bf16 entry: host calls only, nothing allocated ---------------------------------------------------------
DOMAIN = [
    (3, (1, 16, 16, 32), 16, 16, True),           # 8192 voxels
    (3, (1, 7, 31, 37), 16, 16, False),           # 8029 voxels
    (3, (1, 16, 16, 32), 32, 16, False),          # Cin = 32
    (2, (1, 1, 128, 128), 16, 16, False),         # dims = 2
    (3, (1, 512, 256, 256), 16, 16, False),       # D*H*W*64 = 2^31
    (3, (1, 1, 4100, 4100), 16, 16, False),       # fails only the (D + 3) guard: D*H*W*64 < 2^31, (D+3)*H*W*64 > 2^32
]


@pytest.mark.parametrize('dims,ext,cin,cout,inside', DOMAIN, ids=['8192', '8029', 'cin32', 'dims2', '2^31', 'd+3'])
def test_bf16_domain(dims, ext, cin, cout, inside):
    from latentfusion_amd import _lib, ops_train as T
    N, D, H, W = ext
    nb = _lib.lib().lf_conv_bwd_weight_bf16_scratch_bytes(dims, N, D, H, W, cin, cout)
    assert (nb != 0) == inside, nb
    gp = torch.empty((N, cout) + ((D, H, W) if dims == 3 else (H, W)), device='meta')      # a shape, no memory
    assert T._wgrad_bf16_ok(gp, dims, cin, cout) == inside
