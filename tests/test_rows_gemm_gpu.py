"""lf_rows_gemm_epi on the GPU: the ranking path's factor projection 3-D -> 2-D as ONE in-tree fp32-MFMA launch
(y = epilogue(he * x W^T + b), epilogue = [LeakyReLU] ; [PixelNorm over all output channels]) -- against fp64, bit for bit
across batch sizes, at its edges, at its ABI, and behind RenderLoopEngine / MultiTargetEngine / the estimators as
proj_kernel='mfma' on the committed g20 / g25 fixtures.

BOUNDS.  |kernel - fp64| <= max(4 * e32, 2e-6 + 2e-5 * |fp64|) per element of y and of norm_out (the rule of
tests/test_pose_loss_fp64_gpu.py): fp64 = `_formula` in float64 on the same fp32 inputs, e32 = the distance from it of the
same formula in float32 torch (torch.mm, * he + b, leaky_relu, PixelNorm as the reference writes it) -- the yardstick is
the fp32 expressions, never this kernel.  The same helper rejects six misreadings of the formula run as fp64 references.

MEASURED on an MI355X (printed by every case as `[rows-gemm] ...`): max over the case's elements of |err| / max|fp64|, kernel
(fp32 expressions in brackets), and the worst err / bound of y; M = 300 unless stated, flags LRELU | PIXELNORM, with bias:

  (K, Cout)     y                    norm_out             worst err / bound
  (4, 16)       1.2e-7 (1.2e-7)      6.0e-8 (8.2e-8)      0.05
  (20, 100)     1.9e-7 (1.7e-7)      8.9e-8 (8.7e-8)      0.09
  (64, 64)      2.1e-7 (2.7e-7)      1.1e-7 (1.2e-7)      0.19
  (4096, 256)   2.5e-7 (9.0e-7)      1.7e-7 (1.6e-7)      0.55
  (4096, 256), M = 65, rows scaled by 2^+-20, no bias:   3.1e-7 (7.6e-7)   7.5e-8 (7.5e-8)   0.49
  (4096, 256), M = 65, flags 0:                          3.3e-7 (7.2e-7)                     0.52

Every case holds by the fixed member of the bound; none needs 4 * e32.  (With ONE running sum over K the kernel's y error at
K = 4096 was 2.3e-6 and up to 1.97 x the bound on 5 .. 20 elements of a case: the kernel adds the running sum of every 128 k
to a second-level sum.)  The six misreadings miss the bound by factors of 2.7e4 (PixelNorm before LeakyReLU) to 1.8e6
(channel-major K); after the PixelNorm `bias_before_he` and `no_he` are the same function (the overall scale cancels)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
LRELU, PIXELNORM = 1, 2
SENT = -12345.0                       # sentinel of the guard rows behind y / norm_out
GUARD = 8
MMAX = 300
SHAPES = [(4, 16), (20, 100), (64, 64), (4096, 256)]
MS = [1, 63, 64, 65, 129, 300]


def _ops():
    from latentfusion_amd import ops
    return ops


def _L():
    from latentfusion_amd import _lib
    return _lib.lib()


def _s():
    return torch.cuda.current_stream().cuda_stream


def _formula(x, w, b, he, flags, slope, eps, variant=None, dims=None):
    """The projection in x's dtype.  variant: one of the misreadings of VARIANTS (None: the formula of include/lf_hip.h)."""
    if variant == 'channel_major_k':                     # k read as c*D + d instead of d*C + c
        D, C = dims
        x = x.reshape(-1, D, C).transpose(1, 2).reshape(-1, D * C)
    s = torch.mm(x, w.t())
    if variant == 'no_he':
        he = 1.0
    if variant == 'bias_before_he':
        y = (s + (b if b is not None else 0.0)) * he
    else:
        y = s * he
        if b is not None:
            y = y + b
    if variant == 'slope_0p01':
        slope = 0.01
    if variant == 'no_eps':
        eps = 0.0

    def pn(v):
        r = torch.sqrt(torch.mean(v ** 2, dim=1, keepdim=True) + eps)
        return v / r, r[:, 0]
    norm = None
    if variant == 'pixelnorm_before_lrelu':
        if flags & PIXELNORM:
            y, norm = pn(y)
        if flags & LRELU:
            y = torch.nn.functional.leaky_relu(y, slope)
        return y, norm
    if flags & LRELU:
        y = torch.nn.functional.leaky_relu(y, slope)
    if flags & PIXELNORM:
        y, norm = pn(y)
    return y, norm


VARIANTS = ['no_he', 'slope_0p01', 'no_eps', 'pixelnorm_before_lrelu', 'channel_major_k', 'bias_before_he']

_CACHE = {}


def _inputs(K, cout, kind='normal'):
    """Seeded normal inputs of MMAX rows (computed once per shape and kind, never modified): x, w, bias, he, and the packed w.
    kind 'scaled': row 3 times 2^20, row 5 times 2^-20 (no bias: the small row's PixelNorm sum sits below eps);
    kind 'zero_row': row 7 all zero (no bias)."""
    key = (K, cout, kind)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(1000 * K + cout)
        x = torch.randn(MMAX, K, generator=g)
        w = torch.randn(cout, K, generator=g)
        b = 0.3 * torch.randn(cout, generator=g)
        if kind == 'scaled':
            x[3] *= 2.0 ** 20
            x[5] *= 2.0 ** -20
        if kind == 'zero_row':
            x[7] = 0.0
        he = math.sqrt(2.0 / K)
        x, w, b = x.to(DEV), w.to(DEV), b.to(DEV)
        _CACHE[key] = dict(x=x, w=w, b=b, he=he, wpack=_ops().pack_rows_gemm(w))
    return _CACHE[key]


_REFS = {}


def _references(K, cout, kind, flags, bias, variant=None):
    """(fp64 y, fp64 norm, fp32 y, fp32 norm) of the MMAX rows, computed once per configuration."""
    key = (K, cout, kind, flags, bias, variant)
    if key not in _REFS:
        ops, inp = _ops(), _inputs(K, cout, kind)
        dims = (16, K // 16) if K % 16 == 0 else None
        out = []
        for dt in (torch.float64, torch.float32):
            b = inp['b'].to(dt) if bias else None
            out += list(_formula(inp['x'].to(dt), inp['w'].to(dt), b, inp['he'], flags, ops.SLOPE, ops.PN_EPS, variant, dims))
        _REFS[key] = tuple(out)
    return _REFS[key]


def _run(x, wpack, b, he, cout, flags, M=None, want_norm=True):
    """The kernel on the first M rows of x through the C ABI, with guards: x is copied in front of 64 rows of NaN, y and
    norm_out carry GUARD sentinel rows behind row M, which must come back intact.  -> (y [M][cout], norm [M] or None)."""
    ops = _ops()
    M = x.shape[0] if M is None else M
    K = x.shape[1]
    xg = torch.full((M + 64, K), float('nan'), device=DEV)
    xg[:M] = x[:M]
    y = torch.full((M + GUARD, cout), SENT, device=DEV)
    norm = torch.full((M + GUARD,), SENT, device=DEV) if want_norm else None
    rc = _L().lf_rows_gemm_epi(xg.data_ptr(), wpack.data_ptr(), b.data_ptr() if b is not None else None, y.data_ptr(),
                               norm.data_ptr() if norm is not None else None, M, K, cout, he, flags, ops.SLOPE, ops.PN_EPS, _s())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert bool((y[M:] == SENT).all()), 'rows >= M of y were written'
    if norm is not None:
        assert bool((norm[M:] == SENT).all()), 'rows >= M of norm_out were written'
        if not (flags & PIXELNORM):
            assert bool((norm == SENT).all()), 'norm_out written without LF_EPI_PIXELNORM'
    return y[:M], (norm[:M] if (norm is not None and (flags & PIXELNORM)) else None)


def _mismatches(tag, got, ref64, ref32):
    """Elements of `got` outside max(4 * e32, 2e-6 + 2e-5 |fp64|); prints the measured figures first."""
    got, ref32 = got.double(), ref32.double()
    err, e32 = (got - ref64).abs(), (ref32 - ref64).abs()
    fixed = 2e-6 + 2e-5 * ref64.abs()
    bound = torch.maximum(4 * e32, fixed)
    scale = float(ref64.abs().max()) or 1.0
    print(f'[rows-gemm] {tag}: kernel err {float(err.max()) / scale:.2e}  fp32 expressions {float(e32.max()) / scale:.2e}'
          f'  worst err/bound {float((err / bound).max()):.3f}  needs 4*e32 {bool(((err > fixed) & (err <= bound)).any())}')
    bad = ~(err <= bound)
    return int(bad.sum())


def _check(tag, y, norm, refs, M):
    y64, n64, y32, n32 = refs
    bad = _mismatches(tag + ' y', y, y64[:M], y32[:M])
    if norm is not None:
        bad += _mismatches(tag + ' norm', norm, n64[:M], n32[:M])
    return bad


# ----------------------------------------------------------------------------------------------------------------------
# against fp64
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K,cout', SHAPES)
@pytest.mark.parametrize('M', MS)
def test_matches_fp64(M, K, cout):
    inp = _inputs(K, cout)
    flags = LRELU | PIXELNORM
    y, norm = _run(inp['x'], inp['wpack'], inp['b'], inp['he'], cout, flags, M)
    assert torch.isfinite(y).all() and torch.isfinite(norm).all()
    assert not _check(f'M {M} K {K} Cout {cout}', y, norm, _references(K, cout, 'normal', flags, True), M)


@pytest.mark.parametrize('M,K,cout', [(129, 64, 64), (65, 4096, 256)])
@pytest.mark.parametrize('flags', [0, LRELU, PIXELNORM, LRELU | PIXELNORM])
@pytest.mark.parametrize('bias', [True, False])
def test_every_flag_combination_with_and_without_bias(M, K, cout, flags, bias):
    inp = _inputs(K, cout)
    y, norm = _run(inp['x'], inp['wpack'], inp['b'] if bias else None, inp['he'], cout, flags, M)
    assert (norm is not None) == bool(flags & PIXELNORM)
    assert not _check(f'M {M} K {K} Cout {cout} flags {flags} bias {bias}', y, norm, _references(K, cout, 'normal', flags, bias), M)


@pytest.mark.parametrize('M,K,cout', [(129, 64, 64), (65, 4096, 256)])
def test_norm_out_may_be_null_with_pixelnorm_on(M, K, cout):
    inp = _inputs(K, cout)
    flags = LRELU | PIXELNORM
    y, _ = _run(inp['x'], inp['wpack'], inp['b'], inp['he'], cout, flags, M, want_norm=False)
    y2, _ = _run(inp['x'], inp['wpack'], inp['b'], inp['he'], cout, flags, M)
    assert torch.equal(y, y2)
    assert not _check(f'M {M} K {K} Cout {cout} norm_out NULL', y, None, _references(K, cout, 'normal', flags, True), M)


@pytest.mark.parametrize('K,cout', [(64, 64), (4096, 256)])
def test_rows_scaled_by_2_pow_20_up_and_down(K, cout):
    inp = _inputs(K, cout, 'scaled')
    flags = LRELU | PIXELNORM
    y, norm = _run(inp['x'], inp['wpack'], None, inp['he'], cout, flags, 65)
    assert torch.isfinite(y).all() and torch.isfinite(norm).all()
    assert float(norm[3]) > 1e4 and float(norm[5]) < 2e-4                  # the rows did reach both ends of the range
    assert not _check(f'scaled rows K {K} Cout {cout}', y, norm, _references(K, cout, 'scaled', flags, False), 65)


@pytest.mark.parametrize('K,cout', [(64, 64), (4096, 256)])
def test_all_zero_row_is_exactly_zero_over_sqrt_eps(K, cout):
    ops, inp = _ops(), _inputs(K, cout, 'zero_row')
    flags = LRELU | PIXELNORM
    y, norm = _run(inp['x'], inp['wpack'], None, inp['he'], cout, flags, 65)
    y64, n64, y32, n32 = _references(K, cout, 'zero_row', flags, False)
    assert bool((y32[7] == 0).all()) and abs(float(n32[7]) - math.sqrt(ops.PN_EPS)) < 1e-11      # sqrt(eps), rounded to fp32
    assert bool((y[7] == 0).all()), 'PixelNorm of an all-zero row: 0 / sqrt(eps) = 0 exactly'
    assert float(norm[7]) == float(n32[7]), 'norm_out of an all-zero row is sqrt(eps) as the fp32 expressions round it'
    assert not _check(f'zero row K {K} Cout {cout}', y, norm, (y64, n64, y32, n32), 65)


# ----------------------------------------------------------------------------------------------------------------------
# the bound means something: misreadings of the formula, as fp64 references, fail it
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('variant', VARIANTS)
def test_comparison_rejects_a_wrong_reference(variant):
    M, K, cout = 65, 4096, 256
    flags = LRELU | PIXELNORM
    # eps shows where the PixelNorm sum is small (the row scaled by 2^-20, no bias); the other misreadings on the plain case
    kind, bias = ('scaled', False) if variant == 'no_eps' else ('normal', True)
    inp = _inputs(K, cout, kind)
    y, norm = _run(inp['x'], inp['wpack'], inp['b'] if bias else None, inp['he'], cout, flags, M)
    assert not _check(f'{kind} true reference', y, norm, _references(K, cout, kind, flags, bias), M)
    wrong = _references(K, cout, kind, flags, bias, variant)        # its own fp32 evaluation is its e32
    assert _mismatches(f'{kind} vs {variant} y', y, wrong[0][:M], wrong[2][:M]), f'{variant} passes the bound of the true reference'
    assert _mismatches(f'{kind} vs {variant} norm', norm, wrong[1][:M], wrong[3][:M]), f'{variant}: norm_out passes the bound'


# ----------------------------------------------------------------------------------------------------------------------
# a row's result does not depend on the rows it is computed with; run-to-run identical
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K,cout', [(4096, 256), (20, 100)])
def test_rows_are_bit_identical_whatever_m(K, cout):
    ops, L, inp = _ops(), _L(), _inputs(K, cout)
    flags = LRELU | PIXELNORM
    y, norm = _run(inp['x'], inp['wpack'], inp['b'], inp['he'], cout, flags, MMAX)
    y_again, norm_again = _run(inp['x'], inp['wpack'], inp['b'], inp['he'], cout, flags, MMAX)
    assert torch.equal(y, y_again) and torch.equal(norm, norm_again), 'two runs of the same call differ'
    yb, nb = _run(inp['x'][64:129], inp['wpack'], inp['b'], inp['he'], cout, flags)
    assert torch.equal(yb, y[64:129]) and torch.equal(nb, norm[64:129]), 'rows 64..128 as their own call'
    y1 = torch.empty(MMAX, cout, device=DEV)
    n1 = torch.empty(MMAX, device=DEV)
    for i in range(MMAX):                                             # every row alone (M = 1)
        rc = L.lf_rows_gemm_epi(inp['x'][i:i + 1].data_ptr(), inp['wpack'].data_ptr(), inp['b'].data_ptr(), y1[i:i + 1].data_ptr(),
                                n1[i:i + 1].data_ptr(), 1, K, cout, inp['he'], flags, ops.SLOPE, ops.PN_EPS, _s())
        assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(y1, y) and torch.equal(n1, norm), 'a row computed alone differs from the row computed among 300'


# ----------------------------------------------------------------------------------------------------------------------
# nothing outside the operands is touched; a non-finite input stays in its row
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M', [1, 65, 129])
@pytest.mark.parametrize('K,cout', [(20, 100), (4096, 256)])
def test_rows_past_m_are_neither_read_nor_written(M, K, cout):
    inp = _inputs(K, cout)
    # _run puts 64 rows of NaN behind x and sentinel rows behind y / norm_out, and asserts the sentinels
    y, norm = _run(inp['x'], inp['wpack'], inp['b'], inp['he'], cout, LRELU | PIXELNORM, M)
    assert torch.isfinite(y).all() and torch.isfinite(norm).all()


@pytest.mark.parametrize('value', [float('nan'), float('inf'), float('-inf')])
@pytest.mark.parametrize('K,cout', [(20, 100), (4096, 256)])
def test_a_nonfinite_input_stays_in_its_row(value, K, cout):
    ops, inp = _ops(), _inputs(K, cout)
    flags = LRELU | PIXELNORM
    M, r = 129, 70
    clean_y, clean_n = _run(inp['x'], inp['wpack'], inp['b'], inp['he'], cout, flags, M)
    x = inp['x'][:M].clone()
    x[r, K // 2 + 1] = value
    y, norm = _run(x, inp['wpack'], inp['b'], inp['he'], cout, flags, M)
    others = [i for i in range(M) if i != r]
    assert torch.equal(y[others], clean_y[others]) and torch.equal(norm[others], clean_n[others])
    y32, n32 = _formula(x, inp['w'], inp['b'], inp['he'], flags, ops.SLOPE, ops.PN_EPS)
    assert not torch.isfinite(y32[r]).any() and not torch.isfinite(n32[r])           # the fp32 expressions lose the whole row
    assert torch.equal(torch.isnan(y[r]), torch.isnan(y32[r])) and torch.equal(torch.isinf(y[r]), torch.isinf(y32[r]))
    assert bool(torch.isnan(norm[r])) == bool(torch.isnan(n32[r])) and bool(torch.isinf(norm[r])) == bool(torch.isinf(n32[r]))
    if value != value:
        assert torch.isnan(y[r]).all() and torch.isnan(norm[r])


# ----------------------------------------------------------------------------------------------------------------------
# ABI errors: a negative code, nothing launched
# ----------------------------------------------------------------------------------------------------------------------
def test_abi_errors_leave_the_outputs_alone():
    ops, L = _ops(), _L()
    EINVAL, EALIGN = -1, -2
    M, K, cout = 40, 64, 64
    inp = _inputs(K, cout)
    x = inp['x'][:M + 1].contiguous()
    y = torch.full((M, 260), SENT, device=DEV)
    norm = torch.full((M,), SENT, device=DEV)
    good = dict(x=x.data_ptr(), wpack=inp['wpack'].data_ptr(), bias=inp['b'].data_ptr(), y=y.data_ptr(), norm=norm.data_ptr(),
                M=M, K=K, Cout=cout, flags=LRELU | PIXELNORM)

    def call(**kw):
        a = dict(good, **kw)
        rc = L.lf_rows_gemm_epi(a['x'], a['wpack'], a['bias'], a['y'], a['norm'], a['M'], a['K'], a['Cout'], inp['he'], a['flags'],
                                ops.SLOPE, ops.PN_EPS, _s())
        torch.cuda.synchronize()
        return rc

    cases = [('NULL x', dict(x=None), EINVAL), ('NULL wpack', dict(wpack=None), EINVAL), ('NULL y', dict(y=None), EINVAL),
             ('M = 0', dict(M=0), EINVAL), ('M < 0', dict(M=-3), EINVAL), ('M past the grid', dict(M=128 * (2 ** 31 - 1) + 1), EINVAL),
             ('K = 6', dict(K=6), EINVAL), ('K = 0', dict(K=0), EINVAL),
             ('Cout = 260', dict(Cout=260), EINVAL), ('Cout = 18', dict(Cout=18), EINVAL), ('Cout = 12', dict(Cout=12), EINVAL),
             ('unknown flag bit', dict(flags=LRELU | PIXELNORM | 4), EINVAL), ('depth-inner bit', dict(flags=0x100 | LRELU), EINVAL),
             ('x + 4 bytes', dict(x=x.data_ptr() + 4), EALIGN), ('wpack + 4 bytes', dict(wpack=inp['wpack'].data_ptr() + 4), EALIGN),
             ('y + 8 bytes', dict(y=y.data_ptr() + 8), EALIGN)]
    for name, kw, want in cases:
        assert call(**kw) == want, name
        assert bool((y == SENT).all()) and bool((norm == SENT).all()), f'{name}: an output buffer was written'
    assert call() == 0                                                 # and the same arguments, unbroken, run
    assert bool((y.view(-1)[:M * cout] != SENT).all()) and bool((norm != SENT).all())
    # the Python wrapper raises for the same
    from latentfusion_amd._lib import LFHipError
    with pytest.raises(ValueError):
        ops.rows_gemm_epilogue(x, inp['wpack'][:, :32].contiguous(), None, inp['he'], cout)
    with pytest.raises(ValueError):
        ops.rows_gemm_epilogue(x.t(), inp['wpack'], None, inp['he'], cout)
    with pytest.raises(LFHipError):
        ops.rows_gemm_epilogue(x, inp['wpack'], None, inp['he'], cout, flags=4)
    with pytest.raises(LFHipError):
        ops.rows_gemm_epilogue(x.cpu(), inp['wpack'], None, inp['he'], cout)


def test_ops_wrapper_matches_the_abi_call_and_is_timed():
    ops, inp = _ops(), _inputs(4096, 256)
    flags = LRELU | PIXELNORM
    y, norm = _run(inp['x'], inp['wpack'], inp['b'], inp['he'], 256, flags, 129)
    ops.KERNEL_TIMER = []
    try:
        y2, norm2 = ops.rows_gemm_epilogue(inp['x'][:129], inp['wpack'], inp['b'], inp['he'], 256)
        y3, norm3 = ops.rows_gemm_epilogue(inp['x'][:129], inp['wpack'], None, inp['he'], 256, flags=LRELU)
        torch.cuda.synchronize()
        tags = [str(n) for n, _, _ in ops.KERNEL_TIMER]
    finally:
        ops.KERNEL_TIMER = None
    assert tags == ['rows_gemm_epi', 'rows_gemm_epi']
    assert torch.equal(y2, y) and torch.equal(norm2, norm) and norm3 is None and not y2.requires_grad
    assert not _check('wrapper LRELU no bias', y3, None, _references(4096, 256, 'normal', LRELU, False), 129)


# ----------------------------------------------------------------------------------------------------------------------
# engine and estimator on the committed fixtures
# ----------------------------------------------------------------------------------------------------------------------
def close(a, b, atol=1e-4, rtol=1e-3):
    torch.testing.assert_close(a.detach().cpu().contiguous(), b.detach().cpu().contiguous(), atol=atol, rtol=rtol)


def prod_camera(d, device=DEV):
    from latentfusion_amd.modules.geometry import Camera
    return Camera(d['K'].to(device), None, d['z_span'], d['viewport'].to(device), width=d['width'],
                  height=d['height'], log_quaternion=d['log_q'].to(device), translation=d['t'].to(device))


def same_order_up_to_ties(loss, ref_loss, tol):
    """The HIP losses sort like the reference's wherever the reference separates two samples by more than tol."""
    loss, ref_loss = loss.detach().cpu(), ref_loss.detach().cpu()
    order = torch.argsort(ref_loss)
    return all(not (ref_loss[b] - ref_loss[a] > tol) or bool(loss[a] < loss[b]) for a, b in zip(order[:-1].tolist(), order[1:].tolist()))


def _g20_model(g):
    from latentfusion_amd.recon import fusion
    from latentfusion_amd.recon.inference import LatentFusionModel
    from latentfusion_amd.recon.models import Photographer, Sculptor
    return LatentFusionModel(Sculptor.from_checkpoint(g['sculptor']), fusion.from_checkpoint(g['fuser']),
                             Photographer.from_checkpoint(g['photographer']), g['camera_dist'], DEV)


def _g7_target(t7, device=DEV):
    from latentfusion_amd.observation import Observation
    tg = t7['target']
    return Observation(None, tg['depth'], tg['mask'].float(), prod_camera(tg['cam'], 'cpu')).to(device)


def _observation(d, device=DEV):
    from latentfusion_amd.modules.geometry import Camera
    from latentfusion_amd.observation import Observation
    return Observation(d['color'], d['depth'], d['mask'], Camera(d['intrinsic'], d['extrinsic'], width=d['width'],
                                                                  height=d['height'])).to(device)


def _shifted_targets(target, shifts):
    from latentfusion_amd.observation import Observation
    return [Observation(None, torch.roll(target.depth, (dy, dx), (-2, -1)).contiguous(),
                        torch.roll(target.mask, (dy, dx), (-2, -1)).contiguous(), target.camera) for dy, dx in shifts]


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
    """{entry point: launches} of liblf_hip.so while fn() runs (counted by _lib.check, as the engine tests count them)."""
    from latentfusion_amd import _lib
    _lib.BYTE_LOG = {}
    try:
        out = fn()
        torch.cuda.synchronize()
        return out, {k: v[0] for k, v in _lib.BYTE_LOG.items()}
    finally:
        _lib.BYTE_LOG = None


def test_g20_ranking_engine_mfma_one_launch_no_library_gemm(golden):
    """RenderLoopEngine(proj_kernel='mfma') on the 64-channel fixture: a ranking call's projection is ONE lf_rows_gemm_epi under
    ONE factor_project_fwd section, with no addmm / mm / leaky_relu dispatched; its losses equal the library trio's within the
    bound tests/test_released_width_gpu.py uses between the library GEMM and the K-sliced form; the gradient path is untouched."""
    from latentfusion_amd import ops
    from latentfusion_amd.engine import RenderLoopEngine
    g, t7 = golden('g20_released_width'), golden('g7_adam_trace')
    model = _g20_model(g)
    Lg = g['loss']
    target = _g7_target(t7)
    zc = prod_camera(Lg['zoomed'])
    engs = {k: RenderLoopEngine(model.photographer, g['z_obj'].to(DEV), target, Lg['weights'], proj_kernel=k) for k in ('mfma', 'library', None)}
    assert engs['mfma'].proj_kernel == 'mfma' and engs['library'].proj_kernel == 'library' and engs[None].proj_kernel == 'library'
    assert engs['mfma'].proj_rows_pack is not None and engs['library'].proj_rows_pack is None
    out, names, tags, counts = {}, {}, {}, {}
    for k in ('mfma', 'library'):
        ops.KERNEL_TIMER = []
        try:
            with torch.no_grad():
                ((out[k], names[k]), counts[k]) = _launches(lambda: _aten_calls(
                    lambda: engs[k].forward_backward(zc, need_grad=False, masked_depth=True)[0]))
            tags[k] = [str(n) for n, _, _ in ops.KERNEL_TIMER]
        finally:
            ops.KERNEL_TIMER = None
    assert tags['mfma'].count('factor_project_fwd') == 1 and tags['library'].count('factor_project_fwd') == 1
    gemm = lambda ns: [n for n in ns if 'addmm' in n or 'aten.mm' in n or 'leaky_relu' in n]      # noqa: E731
    assert not gemm(names['mfma']), gemm(names['mfma'])
    assert len(gemm(names['library'])) == 2, gemm(names['library'])            # (the control: the recorder does see them)
    assert counts['mfma'].get('lf_rows_gemm_epi') == 1 and 'lf_rows_gemm_epi' not in counts['library']
    assert counts['mfma'].get('lf_pixelnorm_fwd', 0) == counts['library']['lf_pixelnorm_fwd'] - 1
    assert torch.isfinite(out['mfma']).all()
    close(out['mfma'], out['library'], atol=2e-6, rtol=2e-5)
    # need_grad=True keeps lf_conv1x1_fwd: the same kernels, so the same losses and gradients, whatever proj_kernel says
    (l1, g1), (l2, g2) = (engs[k].forward_backward(zc) for k in ('mfma', 'library'))
    assert torch.equal(l1, l2)
    close(g1, g2, atol=1e-6 * float(g2.abs().max()), rtol=1e-6)
    for i, k in enumerate(engs['mfma'].LOSS_KEYS):
        close(l1[:, i], Lg['components'][k], atol=2e-5, rtol=1e-3)


def test_g20_cross_entropy_evaluation_mfma(golden):
    """CrossEntropyPoseEstimator(proj_kernel='mfma')._score_samples through evaluate_samples at released width: the
    assertions of tests/test_released_width_gpu.py::test_g20_cross_entropy_evaluation against the reference's recorded losses
    and loss order, and its bound between 'mfma' and 'library'."""
    from latentfusion_amd.pose import estimation
    g, t7 = golden('g20_released_width'), golden('g7_adam_trace')
    model = _g20_model(g)
    ce = g['ce']
    loss = {}
    for k in ('mfma', 'library'):
        est = estimation.CrossEntropyPoseEstimator(model=model, num_samples=24, num_elites=8, num_iters=1, num_gmm_components=2,
                                                   learning_rate=0.9, sample_flipped=True, ranking_size=4,
                                                   loss_weights=ce['weights'], proj_kernel=k)
        cams, loss[k] = est.evaluate_samples(g['z_obj'].to(DEV), _g7_target(t7), prod_camera(ce['cams']))
        assert est.last_scored_on_engine and est._engine_cache[2].proj_kernel == k
        close(cams.log_quaternion, ce['all_cams']['log_q'], atol=1e-5)
        close(loss[k], ce['loss'], atol=2e-5, rtol=1e-3)
        assert same_order_up_to_ties(loss[k], ce['loss'], 2e-5) and int(torch.argmin(loss[k])) == int(ce['order'][0])
        close(torch.sort(loss[k])[0][:8], ce['elite_loss'], atol=2e-5, rtol=1e-3)
    close(loss['mfma'], loss['library'], atol=2e-6, rtol=2e-5)


def test_g20_ranking_latent_term_reads_the_mfma_projection(golden):
    """With a 'latent' weight the ranking call's cosine term reads zp of the new kernel as it read the library trio's."""
    from latentfusion_amd.engine import RenderLoopEngine
    g, t7 = golden('g20_released_width'), golden('g7_adam_trace')
    model = _g20_model(g)
    Lg = g['loss']
    target = _g7_target(t7)
    zc = prod_camera(Lg['zoomed'])
    w = dict(Lg['weights'], latent=0.5)
    out, zps = {}, {}
    for k in ('mfma', 'library'):
        eng = RenderLoopEngine(model.photographer, g['z_obj'].to(DEV), target, w, proj_kernel=k)
        inner = eng._factor_fwd

        def hooked(*a, _inner=inner, _k=k):
            tail = _inner(*a)
            zps[_k] = (tail.zp, tail.pnorm)
            return tail
        eng._factor_fwd = hooked
        cout, S = eng.proj[0].shape[0], eng.S
        zt = torch.randn(1, cout, S, S, generator=torch.Generator().manual_seed(3)).to(DEV)
        with torch.no_grad():
            out[k] = eng.forward_backward(zc, need_grad=False, z_target_latent=zt, masked_depth=True)[0]
        n = out[k].shape[0]
        want = 1.0 - torch.cosine_similarity(zps[k][0].reshape(n, -1), zt.expand(n, -1, -1, -1).reshape(n, -1), 1, 1e-8)
        assert torch.equal(out[k][:, 5], want) and float(want.abs().min()) > 0
    close(zps['mfma'][0], zps['library'][0], atol=2e-6, rtol=2e-5)
    close(zps['mfma'][1], zps['library'][1], atol=2e-6, rtol=2e-5)
    close(out['mfma'], out['library'], atol=2e-6, rtol=2e-5)


def test_g20_multi_target_projection_is_bit_identical_per_target(golden):
    """MultiTargetEngine(proj_kernel='mfma'), two targets x 4 hypotheses: the projection stage of target t's rows is bit-identical
    to the single-target engine's kernel call on the same activations (the camera blocks in front of it are documented as not
    batch-invariant on wide renderers, so the comparison is made at the stage, on the multi-target call's own activations);
    the losses stay within the single-target tolerance of tests/test_multi_target_engine_gpu.py."""
    from latentfusion_amd import ops
    from latentfusion_amd.engine import RenderLoopEngine
    from latentfusion_amd.engine_multi import MultiTargetEngine
    from latentfusion_amd.modules.geometry import Camera
    g, t7 = golden('g20_released_width'), golden('g7_adam_trace')
    model = _g20_model(g)
    weights = g['loss']['weights']
    targets = _shifted_targets(_g7_target(t7), [(0, 0), (10, 12)])
    zc = prod_camera(g['loss']['zoomed'])
    n = 4
    assert zc.translation.shape[0] >= n
    gen = torch.Generator().manual_seed(61)
    cams = [zc[:n], zc[:n]._like(translation=zc[:n].translation + 0.005 * torch.randn(n, 3, generator=gen).to(DEV))]
    with model.frozen():
        eng = MultiTargetEngine(model.photographer, g['z_obj'].to(DEV), targets, weights, proj_kernel='mfma')
        assert eng.proj_kernel == 'mfma'
        seen = []
        inner = eng._factor_fwd

        def hooked(act, *a):
            tail = inner(act, *a)
            seen.append((act, tail.zp, tail.pnorm))
            return tail
        eng._factor_fwd = hooked
        with torch.no_grad():
            lm, _ = eng.forward_backward(Camera.cat(cams), n, need_grad=False, masked_depth=True)
        assert len(seen) == 1
        act, zp, pnorm = seen[0]
        S, cout = eng.S, eng.proj[0].shape[0]
        rows = act.view(2 * n * S * S, S * eng.Cl)
        zp_rows = zp.permute(0, 2, 3, 1).reshape(2 * n * S * S, cout)
        for t in range(2):
            one = RenderLoopEngine(model.photographer, g['z_obj'].to(DEV), targets[t], weights, proj_kernel='mfma')
            r = slice(t * n * S * S, (t + 1) * n * S * S)
            y1, n1 = ops.rows_gemm_epilogue(rows[r], one.proj_rows_pack, one.proj[1], one.proj[2], cout)
            assert torch.equal(y1, zp_rows[r]) and torch.equal(n1, pnorm[r]), t
            with torch.no_grad():
                l1, _ = one.forward_backward(cams[t], need_grad=False, masked_depth=True)
            close(lm[t * n:(t + 1) * n], l1, atol=1e-5, rtol=1e-4)


def test_cfg3_released_architecture_mfma_vs_reference(golden):
    """The released 256-channel architecture (golden g25, K = 4096 -> 256: the shape the kernel was built for) scored by
    CrossEntropyPoseEstimator(proj_kernel='mfma'): the ranking-path assertions of tests/test_fullshape_gpu.py::
    test_cfg3_released_architecture_vs_reference against the reference's losses and order, and 'mfma' against 'library'."""
    from latentfusion_amd import synth
    from latentfusion_amd.pose import estimation
    g = golden('g25_released_arch')
    seed = g['seed']
    model, cks = synth.build_released_model(DEV, seed, 0.1)
    ref = _observation(synth.make_observation_data(g['views'], seed + 10))
    target = _observation(synth.make_observation_data(1, seed + 20))
    z_obj = model.build_latent_object(ref)
    loss = {}
    for k in ('mfma', 'library'):
        est = estimation.CrossEntropyPoseEstimator(model=model, num_samples=16, num_elites=6, num_iters=1, num_gmm_components=2,
                                                   learning_rate=0.9, sample_flipped=True, ranking_size=4, loss_weights=g['weights'],
                                                   proj_kernel=k)
        cams, loss[k] = est.evaluate_samples(z_obj, target, prod_camera(g['cams']))
        eng = est._engine_cache[2]
        assert eng.proj_kernel == k and eng._wide_factor and (eng.S * eng.Cl, eng.proj[0].shape[0]) == (4096, 256)
        close(cams.log_quaternion, g['all_cams']['log_q'], atol=1e-5)
        close(loss[k], g['loss'], atol=2e-5, rtol=1e-3)
        assert same_order_up_to_ties(loss[k], g['loss'], 2e-5) and int(torch.argmin(loss[k])) == int(g['order'][0])
    close(loss['mfma'], loss['library'], atol=2e-6, rtol=2e-5)
