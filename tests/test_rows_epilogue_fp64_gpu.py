"""lf_pixelnorm_fwd, lf_epilogue_bwd and lf_epilogue_bwd_amax (csrc/pointwise.hip: rows_vec4_kernel for C / 4 a power of two
<= 64 on 16-byte aligned arrays, rows_wave_kernel for everything else), through the C ABI, against the fp64 restatement of
tests/conv_direct_cases.py under its bound max(4 e32, 2e-6 + 2e-5 s) (s = |fp64| of the element for y, the row's largest |x| for
the norm, the row's largest |fp64| for the gradient).  Row counts on both sides of a block, in place and out of place, the
three flag sets, a misaligned array at C = 16 (which must take the wave form and meet the same bound), an all-zero row
(y = 0, norm = sqrt(eps) exactly), max|gp| of lf_epilogue_bwd_amax, and -- what the whole-volume passes of the workload run and
no test did -- the second grid-stride iteration of either form.  Outputs lie in NaN-filled buffers between sentinels.
`-s` prints one `[conv-fp64] rows` line per form and channel count."""
import math

import pytest
import torch

import conv_direct_cases as K
from conv_direct_cases import EPS, LF_EINVAL, LRELU, PIXELNORM, SLOPE
from test_conv_direct_fp64_gpu import DEV, Worst, _lib, _stream, check_guards, dev_in, out_buf, ptr

pytestmark = pytest.mark.gpu
BOTH = LRELU | PIXELNORM
# sqrt of the fp32 eps, correctly rounded to fp32 (through fp64: 29 spare bits; not through a vectorised fp32 sqrt of the host)
SQRT_EPS = torch.tensor(math.sqrt(torch.tensor(EPS, dtype=torch.float32).item()), dtype=torch.float32).item()


def run_pixelnorm(x, in_place=False, x_off=0, want_norm=True):
    rows, C = x.shape
    xd = dev_in(x, x_off)
    if in_place:
        t = body = None
        y = xd
    else:
        t, body = out_buf(rows * C)
        y = body
    tn, nbody = out_buf(rows)
    rc = _lib().lf_pixelnorm_fwd(ptr(xd), ptr(y), ptr(nbody) if want_norm else None, rows, C, EPS, _stream())
    assert rc == 0, rc
    if t is not None:
        check_guards(t, rows * C)
    check_guards(tn, rows)
    return {'y': y.cpu().reshape(rows, C), 'norm': nbody.cpu()}


def run_bwd(gy, y, norm, flags, in_place=False, gy_off=0, amax=False):
    rows, C = gy.shape
    gd, yd = dev_in(gy, gy_off), dev_in(y)
    nd = dev_in(norm) if norm is not None else None
    if in_place:
        t = None
        gp = gd
    else:
        t, gp = out_buf(rows * C)
    if amax:
        am = torch.zeros(K.LF_AMAX_FLOATS, device=DEV)
        rc = _lib().lf_epilogue_bwd_amax(ptr(gd), ptr(yd), ptr(nd), ptr(gp), rows, C, flags, SLOPE, ptr(am), _stream())
    else:
        rc = _lib().lf_epilogue_bwd(ptr(gd), ptr(yd), ptr(nd), ptr(gp), rows, C, flags, SLOPE, _stream())
    assert rc == 0, rc
    if t is not None:
        check_guards(t, rows * C)
    torch.cuda.synchronize()
    out = gp.cpu().reshape(rows, C)
    if amax:
        assert am.max().item() == out.abs().max().item(), 'amax_out is not max|gp|'
    return {'gp': out}


def _check_rows(worst, rows, C, x_off=0, places=(False, True)):
    x, gy = K.rows_inputs(rows, C)
    aligned = x_off == 0
    tag = '' if aligned else ' (misaligned)'
    case = f'C={C}'
    e = K.pixelnorm_expected(x)
    z = min(1, rows - 1)
    for in_place in places:
        got = run_pixelnorm(x, in_place, x_off)
        worst.add(K.form_rows(0, rows, C, aligned) + tag, case, K.ratios(e, got))
        assert bool((got['y'][z] == 0).all()) and got['norm'][z].item() == SQRT_EPS, 'the all-zero row'
    assert torch.equal(run_pixelnorm(x, False, x_off, want_norm=False)['y'], got['y'])         # norm_out = NULL; in place = out of place
    for flags in K.PREV_FLAGS:
        y, n = K.rows_prev(x, flags)
        eb = K.rows_bwd_expected(gy, y, n, flags)
        for in_place in places:
            got = run_bwd(gy, y, n, flags, in_place, x_off, amax=in_place)
            worst.add(K.form_rows(1, rows, C, aligned) + tag, case, K.ratios(eb, got))


@pytest.mark.parametrize('rows', K.ROWS_COUNTS)
def test_row_kernels_match_fp64(rows):
    worst = Worst(f'rows {rows}')
    try:
        for C in K.ROWS_VEC_C + K.ROWS_WAVE_C:
            _check_rows(worst, rows, C)
        _check_rows(worst, rows, 16, x_off=1)                        # 4 bytes off: the vector form is not eligible
    finally:
        worst.report()
    forms = {f for f, _ in worst.rows}
    assert forms == {f'rows_{k}_kernel<{m}>' for k in ('vec4', 'wave') for m in (0, 1)} | {f'rows_wave_kernel<{m}> (misaligned)' for m in (0, 1)}


@pytest.mark.parametrize('rows,C', K.ROWS_LARGE, ids=lambda v: str(v))
def test_second_grid_stride_iteration(rows, C):
    """More rows than 16384 blocks cover in one pass: forward and backward of one case each form."""
    assert K.form_rows(0, rows, C).endswith('second iteration') and K.form_rows(1, rows, C).endswith('second iteration')
    assert not K.form_rows(0, rows - 6, C).endswith('second iteration')
    worst = Worst(f'rows {rows}')
    x, gy = K.rows_inputs(rows, C)
    try:
        got = run_pixelnorm(x)
        worst.add(K.form_rows(0, rows, C), f'C={C}', K.ratios(K.pixelnorm_expected(x), got))
        y, n = K.rows_prev(x, BOTH)
        worst.add(K.form_rows(1, rows, C), f'C={C}', K.ratios(K.rows_bwd_expected(gy, y, n, BOTH), run_bwd(gy, y, n, BOTH, amax=True)))
    finally:
        worst.report()


def test_row_misreadings_are_rejected_on_the_device():
    x, gy = K.rows_inputs(65, 17)
    e = K.pixelnorm_expected(x)
    got = run_pixelnorm(x)
    wrong = K.with_true_e32(K.pixelnorm_expected(x, 'mean_over_16'), e)
    assert K.ratios(e, got)['y'][2] <= 1.0 and K.ratios(wrong, {'y': got['y']})['y'][2] > 1.0
    y, n = K.rows_prev(x, BOTH)
    eb = K.rows_bwd_expected(gy, y, n, BOTH)
    got = run_bwd(gy, y, n, BOTH)
    wrong = K.with_true_e32(K.rows_bwd_expected(gy, y, n, BOTH, 'norm_squared'), eb)
    assert K.ratios(eb, got)['gp'][2] <= 1.0 and K.ratios(wrong, got)['gp'][2] > 1.0


def test_row_kernels_refuse_bad_arguments():
    L, s = _lib(), _stream()
    x = dev_in(torch.randn(8 * 16))
    t, y = out_buf(8 * 16)
    assert L.lf_pixelnorm_fwd(ptr(x), ptr(y), None, 0, 16, EPS, s) == LF_EINVAL
    assert L.lf_pixelnorm_fwd(ptr(x), ptr(y), None, 8, 0, EPS, s) == LF_EINVAL
    assert L.lf_epilogue_bwd(ptr(x), ptr(x), None, ptr(y), 8, 16, PIXELNORM, SLOPE, s) == LF_EINVAL       # PixelNorm' without the norm
    assert L.lf_epilogue_bwd_amax(ptr(x), ptr(x), None, ptr(y), 8, 16, LRELU, SLOPE, None, s) == LF_EINVAL  # no amax_out
    check_guards(t, 8 * 16)
    assert bool(torch.isnan(y).all())
