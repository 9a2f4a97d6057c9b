"""The fused pose-loss kernels (csrc/image.hip: lf_pose_loss_fwd / _bwd, _fwd_masked, _fwd_depth / _bwd_depth and the _mt
forms) against an fp64 restatement of the loss, at the viewports, crops and frames where the sampling and its separable adjoint
can go wrong, at the clamps of the finish kernel, and on non-finite input.

REFERENCE.  `_reference` below restates pose/loss.py `_pose_loss_expressions` plus the three front ends in one dtype-generic
function (run in fp64 as the yardstick, in fp32 where an fp32 figure of an intermediate is needed):

    depth mode    channel 0 of the crop is the metric depth crop                                   (lf_pose_loss_fwd_depth)
    logits mode   depth = ((tanh(dl) + 1) * (sigmoid(ml) > 0.5) - 1) * (z_span + 0.01) + t_z           (lf_pose_loss_fwd)
    masked mode   that depth times sigmoid(ml) of the same crop pixel, forward only             (lf_pose_loss_fwd_masked)

Sampling positions px = clamp((x - xmin) * w / vw - 0.5, 0, w - 1), written as clamp(ax * x + bx) with ax = w / vw,
bx = -xmin * ax - 0.5 so that the gradient of the six coefficients (gcoefs[18..23] of the ABI) can be read off; depth by round
half to even, mask logit bilinear with the upper corner clamped to w - 1; torch autograd w.r.t. crop, viewport and t_z.

BOUNDS.  |hip - fp64| <= max(4 * e32, fixed member), e32 = the distance of the project's fp32 expressions
(`_pose_loss_expressions` on the host) from fp64 on the same inputs; for `sums` and gcoefs[18..23], which those expressions do
not expose, e32 is that of `_reference` run in fp32.  Fixed member: forward atol 2e-6 + rtol 2e-5 * |fp64| (the tolerance of
test_fused_pose_loss_matches_module_loss); gradients, per sample, 2e-3 of that sample's largest component.

PRECONDITIONS on the inputs (asserted, never used to exclude anything): outside the exact-tie case every sampling position that
is not clamped lies >= 1e-4 pixels from a .5 boundary and from an integer (fp32 evaluates positions to ~1.5e-5 at worst); in
the tie case every quantity is dyadic; |ml| >= 1e-3; target mask values are 0 or >= 0.2 (case `faint_rim` adds a ring of 0.05:
away from the 0.1 threshold on the other side, it is what makes `mask > 0` and `mask > 0.1` differ); the sign of pd - td is
the same in fp32 and fp64 at every valid pixel; no sum lies within 1 % of a clamp threshold.

The border clip of a sampling position passes a gradient strictly inside (0, size - 1) only (ATen's grid_sample, and the
kernels); torch.clamp would also pass it AT the ends, which only the exact-tie case reaches.

MEASURED on an MI355X (largest error over modes, weightings and samples; the fp32 expressions' own error in brackets).  Forward:
relative to |fp64| over terms, total and sums; gradients: relative to the sample's largest component.

    case                   forward            glogits            gcoefs[18..23]     viewport           t_z
    typical32              2.5e-7 (2.0e-7)    3.3e-6 (2.3e-4)    1.7e-4 (1.9e-4)    7.3e-5 (6.8e-5)    7.7e-8 (3.0e-5)
    typical128             4.8e-7 (2.1e-7)    5.6e-6 (2.5e-4)    8.2e-4 (7.7e-4)    6.8e-4 (5.9e-4)    1.1e-7 (4.1e-5)
    overhang_left_top      4.3e-7 (4.3e-7)    7.4e-6 (5.7e-4)    3.6e-5 (1.7e-4)    1.9e-5 (8.9e-5)    1.2e-7 (5.3e-5)
    overhang_right_bottom  4.3e-7 (2.0e-7)    3.4e-5 (1.0e-2)    4.6e-5 (5.4e-5)    7.7e-5 (1.7e-5)    6.4e-8 (1.9e-4)
    magnified              1.3e-6 (5.5e-7)    2.4e-5 (1.9e-3)    6.6e-4 (3.9e-4)    5.5e-4 (9.0e-6)    4.7e-5 (5.2e-4)
    minified               6.4e-7 (4.2e-7)    6.4e-7 (5.1e-6)    8.9e-6 (2.8e-5)    3.4e-6 (1.3e-5)    1.4e-7 (1.0e-6)
    ties                   6.5e-7 (3.2e-7)    7.3e-6 (7.3e-4)    2.4e-6 (4.2e-4)    1.0e-6 (8.7e-7)    1.1e-7 (4.4e-4)
    frame540x720           5.9e-7 (2.1e-7)    3.5e-6 (3.3e-4)    1.7e-4 (4.0e-4)    7.3e-5 (7.9e-5)    1.0e-7 (3.6e-5)
    frame97x131            5.3e-7 (3.3e-7)    1.9e-6 (1.0e-5)    6.3e-5 (6.9e-5)    3.4e-5 (5.9e-5)    5.8e-8 (2.3e-6)
    crop2x2                4.5e-7 (3.7e-7)    8.5e-6 (6.3e-4)    3.2e-6 (1.2e-5)    2.3e-6 (9.0e-7)    1.2e-6 (4.7e-4)
    n1                     2.0e-7 (2.8e-7)    3.2e-6 (2.6e-4)    1.3e-4 (1.3e-4)    8.3e-5 (2.7e-5)    3.2e-8 (4.5e-5)
    n128 (8 rows)          1.0e-6 (4.4e-7)    3.9e-6 (2.6e-4)    5.2e-4 (5.6e-4)    2.0e-4 (1.4e-4)    1.1e-7 (6.8e-5)
    faint_rim              7.9e-7 (2.9e-7)    3.7e-6 (2.5e-4)    2.9e-4 (3.0e-4)    7.7e-5 (5.6e-5)    5.9e-8 (2.2e-5)
    empty_mask             9.6e-8 (1.6e-7)    2.4e-6 (1.8e-4)    7.8e-5 (9.7e-5)    5.2e-5 (5.2e-5)    6.7e-8 (3.1e-5)
    full_mask              4.2e-7 (4.2e-7)    2.9e-6 (2.7e-4)    1.7e-4 (1.7e-4)    1.5e-4 (3.4e-5)    2.4e-7 (4.7e-4)
    all_invalid            1.6e-7 (1.5e-7)    2.9e-6 (2.5e-4)    3.1e-5 (3.2e-5)    1.9e-5 (6.7e-6)    3.4e-8 (4.1e-5)
    pred_empty             1.0e-7 (3.2e-7)    2.4e-6 (2.6e-4)    9.4e-8 (9.0e-5)    0 (0)              9.4e-8 (9.0e-5)
    pred_full              7.3e-7 (2.1e-7)    see below          6.9e-8 (6.2e-5)    0 (0)              1.0e-7 (6.2e-5)
    empty_both             1e-7, see below    3.0e-6 (2.4e-4)    1.0e-7 (5.8e-5)    0 (0)              1.0e-7 (5.8e-5)

Every comparison holds by the fixed member except one, which needs 4 * e32: glogits of `pred_full` with the iou term alone.
That gradient is sig * (1 - sig) * dsig ~ 1e-13 of a mask logit of +30, and 1 - sigmoid(30) is exactly 0 in fp32: the kernel
and the fp32 expressions both return 0 where fp64 has 1e-13 (relative error 1 of a gradient of no consequence).  `empty_both`:
the BCE sum S6 is 2.9e-8 in fp64 and 0 in fp32 (-30 + 9e-14 rounds to -30), inside the atol of 2e-6.
"""
import functools
import types

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = 'cuda'
Z_SPAN = 0.5
TERMS = ('depth', 'ov_depth', 'iou', 'mask')
MIXED = (1.0, 0.3, 0.7, 0.5)
WEIGHTINGS = (MIXED, (1.0, 0.0, 0.0, 0.0), (0.0, 1.0, 0.0, 0.0), (0.0, 0.0, 1.0, 0.0), (0.0, 0.0, 0.0, 1.0))
MARGIN = 1e-4

# frame (H, W), crop (h, w), base viewport (xmin, ymin, xmax, ymax), N
CASES = {
    'typical32': dict(frame=(480, 640), crop=(32, 32), vp=(180.31, 111.15, 460.54, 391.75), N=3),
    'typical128': dict(frame=(480, 640), crop=(128, 128), vp=(180.11, 110.62, 461.23, 391.21), N=3),
    'overhang_left_top': dict(frame=(480, 640), crop=(24, 40), vp=(-59.95, -40.32, 300.39, 320.98), N=3),
    'overhang_right_bottom': dict(frame=(480, 640), crop=(24, 40), vp=(400.3, 250.2, 760.8, 610.6), N=3),
    'magnified': dict(frame=(480, 640), crop=(64, 48), vp=(300.2, 200.1, 330.7, 236.4), N=3),
    'minified': dict(frame=(480, 640), crop=(16, 16), vp=(-180.4, -260.3, 820.1, 740.6), N=3),
    'ties': dict(frame=(480, 640), crop=(32, 32), vp=(200.0, 150.0, 264.0, 214.0), N=3, ties=True),
    'frame540x720': dict(frame=(540, 720), crop=(32, 32), vp=(200.3, 150.2, 520.7, 470.9), N=3),
    'frame97x131': dict(frame=(97, 131), crop=(24, 40), vp=(20.76, 10.42, 90.74, 80.68), N=3),
    'crop2x2': dict(frame=(480, 640), crop=(2, 2), vp=(179.96, 111.17, 460.92, 390.92), N=3),
    'n1': dict(frame=(480, 640), crop=(32, 32), vp=(180.31, 111.15, 460.54, 391.75), N=1),
    'n128': dict(frame=(480, 640), crop=(32, 32), vp=(180.31, 111.15, 460.54, 391.75), N=128, ref_rows=tuple(range(0, 128, 16))),
    'faint_rim': dict(frame=(480, 640), crop=(32, 32), vp=(180.31, 111.15, 460.54, 391.75), N=3, target='faint_rim'),
    # degenerate targets / predictions, one each
    'empty_mask': dict(frame=(480, 640), crop=(32, 32), vp=(180.31, 111.15, 460.54, 391.75), N=3, target='empty'),
    'full_mask': dict(frame=(480, 640), crop=(32, 32), vp=(180.31, 111.15, 460.54, 391.75), N=3, target='full'),
    'all_invalid': dict(frame=(480, 640), crop=(32, 32), vp=(180.31, 111.15, 460.54, 391.75), N=3, target='all_invalid'),
    'pred_empty': dict(frame=(480, 640), crop=(32, 32), vp=(180.31, 111.15, 460.54, 391.75), N=3, ml_const=-30.0),
    'pred_full': dict(frame=(480, 640), crop=(32, 32), vp=(180.31, 111.15, 460.54, 391.75), N=3, ml_const=30.0),
    'empty_both': dict(frame=(480, 640), crop=(32, 32), vp=(180.31, 111.15, 460.54, 391.75), N=3, target='empty', ml_const=-30.0),
}
GEOMETRY_CASES = ('typical32', 'typical128', 'overhang_left_top', 'overhang_right_bottom', 'magnified', 'minified', 'ties',
                  'frame540x720', 'frame97x131', 'crop2x2', 'n1', 'n128', 'faint_rim')
DEGENERATE_CASES = ('empty_mask', 'full_mask', 'all_invalid', 'pred_empty', 'pred_full', 'empty_both')
REPEAT_CASES = ('overhang_left_top', 'overhang_right_bottom', 'n128')


def _s():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------------
def _coefs6(vp, tz, h, w):
    """(ax, bx, ay, by, a_depth, b_depth): crop position of frame pixel (x, y) = (ax x + bx, ay y + by); z = a d + b."""
    ax = w / (vp[:, 2] - vp[:, 0])
    ay = h / (vp[:, 3] - vp[:, 1])
    return torch.stack((ax, -vp[:, 0] * ax - 0.5, ay, -vp[:, 1] * ay - 0.5, torch.full_like(tz, Z_SPAN + 0.01), tz), dim=1)


def _pick(img, iy, ix):
    """img (N, a, b), iy (N, H), ix (N, W) -> img[n, iy[n, :, None], ix[n, None, :]]  (N, H, W)."""
    n = torch.arange(img.shape[0]).view(-1, 1, 1)
    return img[n, iy[:, :, None], ix[:, None, :]]


def _nearest(img, ux, uy, zeros_pad, half_up):
    h, w = img.shape[-2:]
    rnd = (lambda p: torch.floor(p + 0.5)) if half_up else torch.round          # torch.round: half to even
    if zeros_pad:
        ix, iy = rnd(ux), rnd(uy)
        ok = ((iy >= 0) & (iy <= h - 1))[:, :, None] & ((ix >= 0) & (ix <= w - 1))[:, None, :]
        return _pick(img, iy.clamp(0, h - 1).long(), ix.clamp(0, w - 1).long()) * ok
    return _pick(img, rnd(uy.clamp(0, h - 1)).long(), rnd(ux.clamp(0, w - 1)).long())


def _axis_weights(u, size, zeros_pad):
    """Corner indices and weights of a 1-D linear sample at positions u (border: clamp the position, upper corner clamped to
    size - 1; zeros: corners outside the image weigh nothing)."""
    # (the border clip passes a gradient strictly inside (0, size - 1) only, as ATen's grid_sample does; torch.clamp would also
    # pass it AT the two ends, which the exact-tie case reaches)
    p = u if zeros_pad else torch.where((u > 0) & (u < size - 1), u, u.detach().clamp(0, size - 1))
    f = torch.floor(p)
    w1 = p - f
    w0 = 1 - w1
    i0, i1 = f.long(), f.long() + 1
    if zeros_pad:
        w0 = w0 * ((i0 >= 0) & (i0 <= size - 1))
        w1 = w1 * ((i1 >= 0) & (i1 <= size - 1))
    return i0.clamp(0, size - 1), i1.clamp(0, size - 1), w0, w1


def _bilinear(img, ux, uy, zeros_pad):
    N, h, w = img.shape
    x0, x1, wx0, wx1 = _axis_weights(ux, w, zeros_pad)
    y0, y1, wy0, wy1 = _axis_weights(uy, h, zeros_pad)
    n, r = torch.arange(N).view(-1, 1, 1), torch.arange(h).view(1, -1, 1)
    rows = img[n, r, x0[:, None, :]] * wx0[:, None, :] + img[n, r, x1[:, None, :]] * wx1[:, None, :]          # (N, h, W)
    c = torch.arange(rows.shape[2]).view(1, 1, -1)
    return rows[n, y0[:, :, None], c] * wy0[:, :, None] + rows[n, y1[:, :, None], c] * wy1[:, :, None]


VARIANTS = ('round_half_up', 'depth_bilinear', 'align_corners', 'zeros_padding', 'invalid_mask_gt_0', 's5_without_valid',
            'bce_over_mask')


def _reference(crop, cf6, td, tm, mode, variant=None):
    """crop (N, 2, h, w), cf6 (N, 6), td / tm (H, W), all of one dtype -> dict(terms (N, 4), sums (N, 7), diff, valid)."""
    assert variant is None or variant in VARIANTS
    N, _, h, w = crop.shape
    H, W = td.shape
    dt = crop.dtype
    ux = cf6[:, 0:1] * torch.arange(W, dtype=dt) + cf6[:, 1:2]                  # (N, W)
    uy = cf6[:, 2:3] * torch.arange(H, dtype=dt) + cf6[:, 3:4]                  # (N, H)
    dl, ml = crop[:, 0], crop[:, 1]
    if mode == 'depth':
        dcrop = dl
    else:
        dcrop = ((torch.tanh(dl) + 1) * (torch.sigmoid(ml) > 0.5) - 1) * cf6[:, 4].view(-1, 1, 1) + cf6[:, 5].view(-1, 1, 1)
        if mode == 'masked':
            dcrop = dcrop * torch.sigmoid(ml)
    zeros_pad = variant == 'zeros_padding'
    if variant == 'depth_bilinear':
        dhat = _bilinear(dcrop, ux, uy, zeros_pad)
    else:
        dhat = _nearest(dcrop, ux, uy, zeros_pad, variant == 'round_half_up')
    lx, ly = ux, uy
    if variant == 'align_corners':                                             # position = (x - xmin) / vw * (w - 1)
        lx, ly = (ux + 0.5) * ((w - 1) / w), (uy + 0.5) * ((h - 1) / h)
    logit = _bilinear(ml, lx, ly, zeros_pad)
    sig = torch.sigmoid(logit)
    pd = dhat * sig
    invalid = (td == 0) & (tm > (0.0 if variant == 'invalid_mask_gt_0' else 0.1))
    valid = (~invalid).to(dt)
    diff = pd - td * tm
    l1 = diff.abs() * valid
    bce = F.binary_cross_entropy_with_logits(logit, tm.expand_as(logit), reduction='none')
    s5 = tm if variant == 's5_without_valid' else tm * valid
    S = [l1.sum((1, 2)), (l1 * (sig * tm)).sum((1, 2)), (sig * tm).sum((1, 2)), sig.sum((1, 2)), (sig * (tm * valid)).sum((1, 2)),
         s5.sum().expand(N), bce.sum((1, 2))]
    uni = S[3] + S[5] - S[4]
    mask_term = (bce * tm).sum((1, 2)) / tm.sum() if variant == 'bce_over_mask' else S[6] / (H * W)
    terms = torch.stack((S[0] / (H * W), S[1].clamp(min=1e-5) / S[2].clamp(min=1e-4),
                         torch.log(uni.clamp(min=1e-4)) - torch.log(S[4].clamp(min=1e-4)), mask_term), dim=1)
    return dict(terms=terms, sums=torch.stack(S, dim=1), diff=diff.detach(), valid=valid, ux=ux.detach(), uy=uy.detach())


def _reference_with_grads(crop, vp, tz, td, tm, mode, dtype):
    """Forward and, for the differentiable modes, the gradient of every term (summed over samples: rows are independent)
    w.r.t. crop, the six coefficients, the viewport and t_z."""
    crop, vp, tz = (t.detach().to(dtype).requires_grad_(True) for t in (crop, vp, tz))
    cf6 = _coefs6(vp, tz, crop.shape[2], crop.shape[3])
    out = _reference(crop, cf6, td.to(dtype), tm.to(dtype), mode)
    res = dict(terms=out['terms'].detach(), sums=out['sums'].detach(), diff=out['diff'], valid=out['valid'], ux=out['ux'], uy=out['uy'])
    if mode != 'masked':
        res['grads'] = []
        for k in range(4):
            g = torch.autograd.grad(out['terms'][:, k].sum(), (crop, cf6, vp, tz), retain_graph=True, allow_unused=True)
            res['grads'].append([torch.zeros_like(x) if gi is None else gi for gi, x in zip(g, (crop, cf6, vp, tz))])
    return res


def _camera(vp, tz, H, W, device):
    from latentfusion_amd.modules.geometry import Camera
    N = vp.shape[0]
    K = torch.tensor([[500.0, 0.0, W / 2.0], [0.0, 500.0, H / 2.0], [0.0, 0.0, 1.0]], device=device).expand(N, -1, -1).contiguous()
    t = torch.cat((torch.zeros(N, 2, device=device), tz.view(N, 1)), dim=1)
    return Camera(K, None, Z_SPAN, vp, width=W, height=H, log_quaternion=torch.zeros(N, 3, device=device), translation=t)


def _expressions32(crop, vp, tz, td, tm, mode):
    """The project's fp32 expressions on the host with the front end of `mode`: terms (N, 4) and their gradients."""
    from latentfusion_amd.pose.loss import _pose_loss_expressions
    crop, vp, tz = (t.detach().float().requires_grad_(True) for t in (crop, vp, tz))
    H, W = td.shape
    cam = _camera(vp, tz, H, W, 'cpu')
    dl, ml = crop[:, :1], crop[:, 1:2]
    if mode == 'depth':
        depth = dl
    else:
        depth = cam.denormalize_depth((torch.tanh(dl) + 1) * (torch.sigmoid(ml) > 0.5) - 1)
        if mode == 'masked':
            depth = depth * torch.sigmoid(ml)
    ld = _pose_loss_expressions(types.SimpleNamespace(depth=td.view(1, 1, H, W), mask=tm.view(1, 1, H, W)), depth, ml, cam)
    terms = torch.stack([ld[k] for k in TERMS], dim=1)
    res = dict(terms=terms.detach())
    if mode != 'masked':
        res['grads'] = []
        for k in range(4):
            g = torch.autograd.grad(terms[:, k].sum(), (crop, vp, tz), retain_graph=True, allow_unused=True)
            res['grads'].append([torch.zeros_like(x) if gi is None else gi for gi, x in zip(g, (crop, vp, tz))])
    return res


# ---------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------
def _position_margin(vp_row, h, w, H, W):
    """Smallest distance (fp64, from the fp32 viewport) of a sampling position to a decision boundary: to an integer for the
    positions within a quarter pixel of the clamp range (kink of the bilinear sample, the clamp itself at 0 and size - 1), to a
    .5 boundary for those inside it (the nearest pick)."""
    m = float('inf')
    for lo, hi, size, n in ((vp_row[0], vp_row[2], w, W), (vp_row[1], vp_row[3], h, H)):
        a = size / (hi - lo)
        p = a * torch.arange(n, dtype=torch.float64) + (-lo * a - 0.5)
        near = p[(p > -0.25) & (p < size - 0.75)]
        inner = p[(p > 0) & (p < size - 1)]
        if near.numel():
            m = min(m, float((near - near.round()).abs().min()))
        if inner.numel():
            m = min(m, float(((inner - inner.floor()) - 0.5).abs().min()))
    return m


def _nudged(v, h, w, H, W, gen):
    """Viewport v (fp64, two decimals) moved by at most +-0.5 pixel per try until, rounded to fp32, it satisfies
    `_position_margin`; fails if 20 tries do not get there."""
    for _ in range(20):
        if _position_margin(v.float().double(), h, w, H, W) >= MARGIN:
            return v.float()
        v = v + ((torch.rand(4, generator=gen).double() - 0.5) * 100).round() / 100
    raise AssertionError(f'no viewport near {v.tolist()} keeps every sampling position {MARGIN} off a decision boundary')


def _viewports(case, gen):
    """(N, 4) fp32: the case's viewport for sample 0, shifted copies for the others; each nudged by at most +-0.5 pixel per try
    (two decimals) with `_nudged`.  The tie case shifts by whole pixels and doubles every other width."""
    c = CASES[case]
    (h, w), (H, W) = c['crop'], c['frame']
    base = torch.tensor(c['vp'], dtype=torch.float64)
    rows = []
    for n in range(c['N']):
        if c.get('ties'):
            off = torch.randint(-8, 9, (2,), generator=gen).double() if n else torch.zeros(2, dtype=torch.float64)
            scale = 2.0 if n % 2 else 1.0
            v = torch.stack((base[0] + off[0], base[1] + off[1], base[0] + off[0] + (base[2] - base[0]) * scale,
                             base[1] + off[1] + (base[3] - base[1]) * scale))
            rows.append(v.float())
            continue
        v = base.clone()
        if n:
            v = v + ((torch.rand(4, generator=gen).double() * 8 - 4) * 100).round() / 100
        rows.append(_nudged(v, h, w, H, W, gen))
    return torch.stack(rows)


def _target(H, W, kind, gen):
    """Target frame: box mask with a soft rim (0.3 .. 0.7), depth 0.8 .. 1.2 everywhere except a hole of depth == 0 that lies
    inside the mask and crosses its rim (the `invalid` pixels)."""
    y0, y1, x0, x1 = int(0.25 * H), int(0.70 * H), int(0.30 * W), int(0.72 * W)
    tm = torch.zeros(H, W)
    tm[y0:y1, x0:x1] = 0.3 + 0.4 * torch.rand(y1 - y0, x1 - x0, generator=gen)
    tm[y0 + 3:y1 - 3, x0 + 3:x1 - 3] = 1.0
    if kind == 'faint_rim':
        faint = torch.zeros(H, W)
        faint[y0 - 4:y1 + 4, x0 - 4:x1 + 4] = 0.05
        tm = torch.where(tm > 0, tm, faint)
    elif kind == 'empty':
        tm.zero_()
    elif kind == 'full':
        tm.fill_(1.0)
    td = 0.8 + 0.4 * torch.rand(H, W, generator=gen)
    td[int(0.45 * H):int(0.55 * H), int(0.45 * W):int(0.75 * W)] = 0.0          # crosses the right rim and leaves the box
    if kind == 'all_invalid':
        td[tm > 0] = 0.0
    return td, tm


@functools.lru_cache(maxsize=None)
def _inputs(case):
    c = CASES[case]
    (h, w), (H, W), N = c['crop'], c['frame'], c['N']
    gen = torch.Generator().manual_seed(sum(map(ord, case)))
    vp = _viewports(case, gen)
    tz = (1.0 + 0.05 * torch.randn(N, generator=gen)).float()
    ml = torch.randn(N, h, w, generator=gen) * 2
    ml = ml + torch.where(ml >= 0, 0.01, -0.01)                                # the (> 0.5) gate: stay off 0
    if 'ml_const' in c:
        ml = torch.full_like(ml, c['ml_const'])
    dl = torch.randn(N, h, w, generator=gen) * 1.5
    crops = {'logits': torch.stack((dl, ml), dim=1), 'depth': torch.stack((1.0 + 0.15 * torch.randn(N, h, w, generator=gen), ml), dim=1)}
    crops['masked'] = crops['logits']
    td, tm = _target(H, W, c.get('target', 'box'), gen)
    rows = list(c.get('ref_rows', range(N)))
    # keep the |pd - td| kink of every referenced row away from zero: move the target depth of a pixel whose difference is
    # below 1e-4 in any mode by 2e-3 (valid pixels only, so `invalid` is untouched); the precondition is asserted afterwards
    for _ in range(5):
        moved = torch.zeros(H, W, dtype=torch.bool)
        for mode, crop in crops.items():
            r = _reference(crop[rows].double(), _coefs6(vp[rows].double(), tz[rows].double(), h, w), td.double(), tm.double(), mode)
            moved |= ((r['diff'].abs() < 1e-4) & (r['valid'] > 0)).any(dim=0) & (tm > 0)
        if not moved.any():
            break
        td = torch.where(moved, td + 2e-3, td)
    return dict(vp=vp, tz=tz, crops=crops, td=td, tm=tm, rows=rows, h=h, w=w, H=H, W=W, N=N)


def _assert_preconditions(case, inp, ref64, ref32, mode):
    c = CASES[case]
    vp, h, w, H, W = inp['vp'], inp['h'], inp['w'], inp['H'], inp['W']
    if c.get('ties'):
        ratio = torch.cat(((vp[:, 2] - vp[:, 0]) / w, (vp[:, 3] - vp[:, 1]) / h)).double()
        assert torch.equal(vp, vp.round()) and torch.equal(torch.log2(ratio), torch.log2(ratio).round()), 'tie case must be dyadic'
        frac = ref64['ux'] - ref64['ux'].floor()
        assert (frac[(ref64['ux'] > 0) & (ref64['ux'] < w - 1)] == 0.5).any(), 'tie case without a tie'
    else:
        for n in inp['rows']:
            m = _position_margin(vp[n].double(), h, w, H, W)
            assert m >= MARGIN, f'{case} sample {n}: a sampling position lies {m:.2e} pixels from a decision boundary'
    tm, ml = inp['tm'], inp['crops'][mode][:, 1]
    assert (ml.abs() >= 1e-3).all()
    if c.get('target') == 'faint_rim':
        assert ((tm == 0) | (tm == 0.05) | (tm >= 0.2)).all() and (tm == 0.05).any()
    else:
        assert ((tm == 0) | (tm >= 0.2)).all()
    v = (ref64['valid'] > 0).expand_as(ref64['diff'])
    assert torch.equal(torch.sign(ref64['diff'])[v], torch.sign(ref32['diff'].double())[v]), 'sign of pd - td differs between fp32 and fp64'
    S = ref64['sums']
    for val, thr in ((S[:, 1], 1e-5), (S[:, 2], 1e-4), (S[:, 4], 1e-4), (S[:, 3] + S[:, 5] - S[:, 4], 1e-4)):
        assert ((val / thr - 1).abs() > 0.01).all(), 'a sum lies within 1 % of its clamp threshold'


# ---------------------------------------------------------------------------------------------------------------------------
# the kernels
# ---------------------------------------------------------------------------------------------------------------------------
def _hip_forward(mode, crop, coefs, td, tm, weights, mt=None):
    """sums, losses, gsums (N, 8) of one forward call; mt = (T, n) takes the several-target entry points."""
    from latentfusion_amd import _lib, ops
    L = _lib.lib()
    lg = ops.cl(crop)
    N, _, h, w = lg.shape
    H, W = td.shape[-2:]
    nb = L.lf_pose_loss_scratch_bytes(N, h, w, H, W)
    sc = torch.empty(nb // 4 + 1, device=DEV)
    sums, losses, gsums = (torch.full((N, 8), float('nan'), device=DEV) for _ in range(3))
    wv = torch.tensor(weights, device=DEV)
    dims = (N, h, w, H, W) if mt is None else (N,) + tuple(mt) + (h, w, H, W)
    head = (lg.data_ptr(), coefs.data_ptr(), td.data_ptr(), tm.data_ptr(), wv.data_ptr(), sums.data_ptr(), losses.data_ptr())
    if mode == 'masked':
        fn = L.lf_pose_loss_fwd_masked if mt is None else L.lf_pose_loss_fwd_masked_mt
        rc = fn(*head, sc.data_ptr(), nb, *dims, _s())
        gsums = None
    else:
        fn = {'depth': L.lf_pose_loss_fwd_depth, 'logits': L.lf_pose_loss_fwd if mt is None else L.lf_pose_loss_fwd_mt}[mode]
        rc = fn(*head, gsums.data_ptr(), sc.data_ptr(), nb, *dims, _s())
    assert rc == 0, rc
    return sums, losses, gsums


def _hip_backward(mode, crop, coefs, td, tm, gsums, mt=None):
    """glogits (N, 2, h, w) and gcoefs (N, 24) of one backward call."""
    from latentfusion_amd import _lib, ops
    L = _lib.lib()
    lg = ops.cl(crop)
    N, _, h, w = lg.shape
    H, W = td.shape[-2:]
    nb = L.lf_pose_loss_scratch_bytes(N, h, w, H, W)
    sc = torch.empty(nb // 4 + 1, device=DEV)
    glogits = torch.full_like(lg, float('nan'))
    gcoefs = torch.zeros(N, 24, device=DEV)
    dims = (N, h, w, H, W) if mt is None else (N,) + tuple(mt) + (h, w, H, W)
    fn = {'depth': L.lf_pose_loss_bwd_depth, 'logits': L.lf_pose_loss_bwd if mt is None else L.lf_pose_loss_bwd_mt}[mode]
    rc = fn(lg.data_ptr(), coefs.data_ptr(), td.data_ptr(), tm.data_ptr(), gsums.data_ptr(), glogits.data_ptr(), gcoefs.data_ptr(),
            sc.data_ptr(), nb, *dims, _s())
    assert rc == 0, rc
    return glogits, gcoefs


def _hip_run(inp, mode, weightings, rows=None):
    """Every output of the kernels for one mode: forward once per weighting, backward likewise (gradients of the MEAN over
    the call's samples of the weighted total), viewport / t_z gradients through engine.camera_coefs."""
    from latentfusion_amd.engine import camera_coefs
    sel = slice(None) if rows is None else rows
    crop = inp['crops'][mode][sel].to(DEV)
    td, tm = inp['td'].to(DEV).contiguous(), inp['tm'].to(DEV).contiguous()
    vp = inp['vp'][sel].to(DEV).requires_grad_(True)
    tz = inp['tz'][sel].to(DEV).requires_grad_(True)
    coefs = camera_coefs(_camera(vp, tz, inp['H'], inp['W'], DEV), 1.0, inp['h'], inp['w'])
    cf = coefs.detach().contiguous()
    out = dict(by_weight={})
    for wts in weightings:
        sums, losses, gsums = _hip_forward(mode, crop, cf, td, tm, wts)
        r = dict(sums=sums.cpu(), losses=losses.cpu(), gsums=None if gsums is None else gsums.cpu())
        if mode != 'masked':
            glogits, gcoefs = _hip_backward(mode, crop, cf, td, tm, gsums)
            gvp, gtz = torch.autograd.grad(coefs, (vp, tz), grad_outputs=gcoefs, retain_graph=True)
            r.update(glogits=glogits.cpu().contiguous(), gcoefs=gcoefs.cpu(), gvp=gvp.cpu(), gtz=gtz.cpu())
        out['by_weight'][wts] = r
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the comparison
# ---------------------------------------------------------------------------------------------------------------------------
def _fwd_mismatches(tag, got, ref64, ref32):
    """Element-wise: |got - fp64| <= max(4 |fp32 - fp64|, 2e-6 + 2e-5 |fp64|).  Returns the violations."""
    got, ref32 = got.double(), ref32.double()
    err, e32 = (got - ref64).abs(), (ref32 - ref64).abs()
    bound = torch.maximum(4 * e32, 2e-6 + 2e-5 * ref64.abs())
    scale = ref64.abs().clamp(min=1e-30)
    print(f'[pose-loss] {tag}: rel err hip {float((err / scale).max()):.2e}  fp32 {float((e32 / scale).max()):.2e}'
          f'  worst err/bound {float((err / bound).max()):.3f}  needs 4*e32 {bool(((err > 2e-6 + 2e-5 * ref64.abs()) & (err <= bound)).any())}')
    bad = ~(err <= bound)                                          # (a NaN fails)
    return [f'{tag}{list(i)}: hip {got[tuple(i)]:.9g} fp64 {ref64[tuple(i)]:.9g} fp32 {ref32[tuple(i)]:.9g}' for i in bad.nonzero().tolist()]


def _grad_mismatches(tag, got, ref64, ref32):
    """Per sample, relative to the sample's largest component: max |got - fp64| <= max(4 max |fp32 - fp64|, 2e-3 max |fp64|)."""
    N = ref64.shape[0]
    got, ref64, ref32 = got.double().reshape(N, -1), ref64.reshape(N, -1), ref32.double().reshape(N, -1)
    err, e32, scale = (got - ref64).abs().amax(1), (ref32 - ref64).abs().amax(1), ref64.abs().amax(1)
    bound = torch.maximum(4 * e32, 2e-3 * scale)
    nz = scale > 0
    if nz.any():
        print(f'[pose-loss] {tag}: rel err hip {float((err[nz] / scale[nz]).max()):.2e}  fp32 {float((e32[nz] / scale[nz]).max()):.2e}'
              f'  needs 4*e32 {bool(((err > 2e-3 * scale) & (err <= bound)).any())}')
    bad = ~(err <= bound)
    return [f'{tag}[{n}]: err {err[n]:.3e} bound {bound[n]:.3e} (largest component {scale[n]:.3e}, fp32 err {e32[n]:.3e})'
            for n in bad.nonzero().flatten().tolist()]


def _combine(grads, wts, N, which):
    return sum(wk * grads[k][which] for k, wk in enumerate(wts)) / N


def _compare(tag, hip, wts, ref64, ref32, expr32, N, forward_only=False):
    """Every output of one (mode, weighting) against the references; N = the number of samples of the kernel call (the mean)."""
    bad = []
    w64 = torch.tensor(wts, dtype=torch.float64)
    bad += _fwd_mismatches(f'{tag} terms', hip['losses'][:, :4], ref64['terms'], expr32['terms'])
    bad += _fwd_mismatches(f'{tag} total', hip['losses'][:, 4], ref64['terms'] @ w64, expr32['terms'] @ w64.float())
    bad += _fwd_mismatches(f'{tag} sums', hip['sums'][:, :7], ref64['sums'], ref32['sums'])
    if forward_only or 'grads' not in ref64:
        return bad
    bad += _grad_mismatches(f'{tag} glogits', hip['glogits'], _combine(ref64['grads'], wts, N, 0), _combine(expr32['grads'], wts, N, 0))
    bad += _grad_mismatches(f'{tag} gcoefs', hip['gcoefs'][:, 18:], _combine(ref64['grads'], wts, N, 1), _combine(ref32['grads'], wts, N, 1))
    bad += _grad_mismatches(f'{tag} gviewport', hip['gvp'], _combine(ref64['grads'], wts, N, 2), _combine(expr32['grads'], wts, N, 1))
    bad += _grad_mismatches(f'{tag} gtz', hip['gtz'], _combine(ref64['grads'], wts, N, 3), _combine(expr32['grads'], wts, N, 2))
    if not (hip['gcoefs'][:, :18] == 0).all():
        bad.append(f'{tag}: gcoefs[0..17] written')
    return bad


@functools.lru_cache(maxsize=None)
def _references(case, mode):
    inp = _inputs(case)
    rows = inp['rows']
    args = (inp['crops'][mode][rows], inp['vp'][rows], inp['tz'][rows], inp['td'], inp['tm'], mode)
    ref64 = _reference_with_grads(*args, torch.float64)
    ref32 = _reference_with_grads(*args, torch.float32)
    expr32 = _expressions32(*args)
    _assert_preconditions(case, inp, ref64, ref32, mode)
    del ref64['diff'], ref32['diff']                               # frame-sized; not needed once the precondition is checked
    return ref64, ref32, expr32


@functools.lru_cache(maxsize=None)
def _kernel_outputs(case, mode):
    weightings = WEIGHTINGS if mode != 'masked' else (MIXED,)
    return _hip_run(_inputs(case), mode, weightings)


def _rows_of(hip, rows):
    return {k: (v[rows] if v is not None else None) for k, v in hip.items()}


def _check_case(case, mode):
    inp = _inputs(case)
    ref64, ref32, expr32 = _references(case, mode)
    out = _kernel_outputs(case, mode)
    bad = []
    for wts, hip in out['by_weight'].items():
        bad += _compare(f'{case} {mode} w={wts}', _rows_of(hip, inp['rows']), wts, ref64, ref32, expr32, inp['N'])
        for k, v in hip.items():
            assert v is None or torch.isfinite(v[:, :7] if k in ('sums', 'losses', 'gsums') else v).all(), (case, mode, wts, k)
    assert not bad, '\n'.join(bad)
    return out


def _unsampled(ref64, h, w):
    """(n, h, w) bool: crop pixels that no frame pixel picks as its nearest."""
    hit_x = torch.zeros(ref64['ux'].shape[0], w, dtype=torch.bool)
    hit_y = torch.zeros(ref64['uy'].shape[0], h, dtype=torch.bool)
    hit_x.scatter_(1, torch.round(ref64['ux'].clamp(0, w - 1)).long(), True)
    hit_y.scatter_(1, torch.round(ref64['uy'].clamp(0, h - 1)).long(), True)
    return ~(hit_y[:, :, None] & hit_x[:, None, :])


# ---------------------------------------------------------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module', autouse=True)
def _per_module_results():
    """`_inputs`, `_references` and `_kernel_outputs` memoise per (case, mode), each filled on demand by whichever test asks
    first (so any test runs alone and in any order, and a case's kernels are launched once); nothing is kept past this module."""
    yield
    for fn in (_inputs, _references, _kernel_outputs):
        fn.cache_clear()


@pytest.mark.parametrize('mode', ['depth', 'logits', 'masked'])
@pytest.mark.parametrize('case', GEOMETRY_CASES)
def test_pose_loss_matches_fp64(case, mode):
    """Forward (terms, total, sums) in all three modes; in the differentiable ones glogits, gcoefs[18..23] and the viewport /
    t_z gradients for the mixed weights and for every term alone; crop pixels that no frame pixel samples get exactly 0."""
    inp = _inputs(case)
    out = _check_case(case, mode)
    if mode == 'masked':
        return
    ref64 = _references(case, mode)[0]
    dead = _unsampled(ref64, inp['h'], inp['w'])
    if case == 'magnified':
        assert dead.float().mean() > 0.5                           # most crop pixels are sampled by no frame pixel
    assert all((ref64['grads'][k][0][:, 0][dead] == 0).all() for k in range(4))
    for wts, hip in out['by_weight'].items():
        assert (hip['glogits'][inp['rows'], 0][dead] == 0).all(), (case, mode, wts)


def test_n128_equals_sixteen_calls_of_eight():
    """The fp64 reference of case n128 covers rows 0, 16, .. 112; the other rows are held by this comparison: the N = 128 call
    against 16 calls of N = 8 on the same rows -- sums and losses bit for bit, gradients after the exact factor 16 that the
    mean over N introduces (a power of two: the scaled values are the same floats)."""
    inp = _inputs('n128')
    for mode in ('depth', 'logits'):
        whole = _kernel_outputs('n128', mode)['by_weight'][MIXED]
        for c in range(16):
            rows = list(range(8 * c, 8 * c + 8))
            part = _hip_run(inp, mode, (MIXED,), rows=rows)['by_weight'][MIXED]
            for k in ('sums', 'losses'):
                assert torch.equal(whole[k][rows], part[k]), (mode, c, k)
            for k in ('gsums', 'glogits', 'gcoefs', 'gvp', 'gtz'):
                assert torch.equal(whole[k][rows] * 16, part[k]), (mode, c, k)
    wholem = _kernel_outputs('n128', 'masked')['by_weight'][MIXED]
    partm = _hip_run(inp, 'masked', (MIXED,), rows=list(range(40, 48)))['by_weight'][MIXED]
    assert torch.equal(wholem['losses'][40:48], partm['losses']) and torch.equal(wholem['sums'][40:48], partm['sums'])


@pytest.mark.parametrize('case', REPEAT_CASES)
def test_pose_loss_is_run_to_run_identical(case):
    inp = _inputs(case)
    for mode in ('depth', 'logits', 'masked'):
        first = _kernel_outputs(case, mode)['by_weight'][MIXED]
        again = _hip_run(inp, mode, (MIXED,))['by_weight'][MIXED]
        for k, v in first.items():
            assert v is None or torch.equal(v, again[k]), (case, mode, k)


@pytest.mark.parametrize('mode', ['depth', 'logits', 'masked'])
@pytest.mark.parametrize('case', DEGENERATE_CASES)
def test_pose_loss_degenerate_targets_and_predictions(case, mode):
    """Empty / full / all-invalid target masks, empty / full predictions: everything finite, values and gradients equal the
    fp64 expressions through the same clamps, and a term whose clamp is active passes exactly nothing."""
    inp = _inputs(case)
    out = _check_case(case, mode)
    S = _references(case, mode)[0]['sums']
    uni = S[:, 3] + S[:, 5] - S[:, 4]
    expect = {'empty_mask': (True, True, True, False), 'all_invalid': (True, False, True, False), 'pred_empty': (True, True, True, False),
              'empty_both': (True, True, True, True), 'full_mask': (False,) * 4, 'pred_full': (False,) * 4}[case]
    active = ((S[:, 1] < 1e-5).all(), (S[:, 2] < 1e-4).all(), (S[:, 4] < 1e-4).all(), (uni < 1e-4).all())
    assert tuple(bool(a) for a in active) == expect, (case, active)
    if mode == 'masked':
        return
    for wts, hip in out['by_weight'].items():
        g = hip['gsums']
        if expect[0]:
            assert (g[:, 1] == 0).all()
        if expect[1]:
            assert (g[:, 2] == 0).all()
        if expect[2]:
            assert torch.equal(g[:, 4], -g[:, 3])                  # no 1 / S4 part
        if expect[3]:
            assert (g[:, 3] == 0).all() and (g[:, 4] == 0).all()
        if inp['crops'][mode][:, 1].max() < 0 and mode == 'logits':
            assert (hip['glogits'][:, 0] == 0).all()               # closed mask everywhere: no depth-logit gradient at all


def test_mt_entry_points_match_fp64_and_single_target_calls():
    """T = 3 targets with different masks, n = 2 hypotheses each, through lf_pose_loss_fwd_mt / _fwd_masked_mt / _bwd_mt:
    bit-identical to the single-target calls on each target's rows, and those rows right against fp64."""
    from latentfusion_amd.engine import camera_coefs
    T, n, H, W, h, w = 3, 2, 120, 160, 24, 40
    N = T * n
    gen = torch.Generator().manual_seed(77)
    frames = [_target(H, W, kind, gen) for kind in ('box', 'faint_rim', 'full')]
    base = torch.tensor([30.27, 20.63, 110.81, 95.38], dtype=torch.float64)
    vps = []
    for i in range(N):
        v = base + ((torch.rand(4, generator=gen).double() * 6 - 3) * 100).round() / 100
        vps.append(_nudged(v, h, w, H, W, gen))
    vp = torch.stack(vps)
    tz = (1.0 + 0.05 * torch.randn(N, generator=gen)).float()
    ml = torch.randn(N, h, w, generator=gen) * 2
    crop = torch.stack((torch.randn(N, h, w, generator=gen) * 1.5, ml + torch.where(ml >= 0, 0.01, -0.01)), dim=1)
    cf = camera_coefs(_camera(vp.to(DEV), tz.to(DEV), H, W, DEV), 1.0, h, w).detach().contiguous()
    td = torch.stack([f[0] for f in frames]).to(DEV).contiguous()
    tm = torch.stack([f[1] for f in frames]).to(DEV).contiguous()
    cd = crop.to(DEV)
    sums, losses, gsums = _hip_forward('logits', cd, cf, td, tm, MIXED, mt=(T, n))
    msums, mlosses, _ = _hip_forward('masked', cd, cf, td, tm, MIXED, mt=(T, n))
    glogits, gcoefs = _hip_backward('logits', cd, cf, td, tm, gsums, mt=(T, n))
    bad = []
    for t in range(T):
        r = slice(t * n, (t + 1) * n)
        s1, l1, g1 = _hip_forward('logits', cd[r], cf[r].contiguous(), td[t], tm[t], MIXED)
        ms1, ml1, _ = _hip_forward('masked', cd[r], cf[r].contiguous(), td[t], tm[t], MIXED)
        gl1, gc1 = _hip_backward('logits', cd[r], cf[r].contiguous(), td[t], tm[t], g1)
        for a, b in ((sums[r], s1), (losses[r], l1), (gsums[r], g1), (msums[r], ms1), (mlosses[r], ml1), (glogits[r], gl1), (gcoefs[r], gc1)):
            assert torch.equal(a, b), t
        for mode, hs, hl in (('logits', sums, losses), ('masked', msums, mlosses)):
            args = (crop[r], vp[r], tz[r], frames[t][0], frames[t][1], mode)
            ref64, ref32, expr32 = _reference_with_grads(*args, torch.float64), _reference_with_grads(*args, torch.float32), _expressions32(*args)
            v = (ref64['valid'] > 0).expand_as(ref64['diff'])
            assert torch.equal(torch.sign(ref64['diff'])[v], torch.sign(ref32['diff'].double())[v])
            hip = dict(sums=hs[r].cpu(), losses=hl[r].cpu())
            if mode == 'logits':
                hip.update(glogits=glogits[r].cpu().contiguous(), gcoefs=gcoefs[r].cpu(), gvp=None, gtz=None)
                bad += _grad_mismatches(f'mt target {t} glogits', hip['glogits'], _combine(ref64['grads'], MIXED, n, 0),
                                        _combine(expr32['grads'], MIXED, n, 0))
                bad += _grad_mismatches(f'mt target {t} gcoefs', hip['gcoefs'][:, 18:], _combine(ref64['grads'], MIXED, n, 1),
                                        _combine(ref32['grads'], MIXED, n, 1))
            bad += _compare(f'mt target {t} {mode}', hip, MIXED, ref64, ref32, expr32, n, forward_only=True)
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('value', [float('nan'), float('inf')])
@pytest.mark.parametrize('where', ['depth_logit_under_closed_mask', 'mask_logit', 'target_depth'])
def test_nonfinite_pattern_is_that_of_the_fp32_expressions(where, value):
    """A NaN (or +inf) in one depth logit under a closed mask, in one mask logit, in one target depth pixel: the non-finite
    entries of losses[:, :5] are those of the fp32 expressions -- (tanh(nan) + 1) * 0 - 1 is NaN, and clamp(min=) keeps a NaN
    sum NaN -- and the rows that do not read the planted value stay bit-identical to the clean run."""
    from latentfusion_amd.engine import camera_coefs
    inp = _inputs('typical32')
    h, w, H, W = inp['h'], inp['w'], inp['H'], inp['W']
    crop, td = inp['crops']['logits'].clone(), inp['td'].clone()
    if where == 'depth_logit_under_closed_mask':
        crop[1, 1, 15, 16] = -1.5
        crop[1, 0, 15, 16] = value
    elif where == 'mask_logit':
        crop[1, 1, 15, 16] = value
    else:
        assert inp['tm'][200, 300] == 1.0
        td[200, 300] = value
    cf = camera_coefs(_camera(inp['vp'].to(DEV), inp['tz'].to(DEV), H, W, DEV), 1.0, h, w).detach().contiguous()
    w4 = torch.tensor(MIXED)
    for mode in ('logits', 'masked'):
        _, losses, _ = _hip_forward(mode, crop.to(DEV), cf, td.to(DEV), inp['tm'].to(DEV), MIXED)
        e = _expressions32(crop, inp['vp'], inp['tz'], td, inp['tm'], mode)['terms']
        want = torch.cat((e, (e * w4).sum(1, keepdim=True)), dim=1)
        got = losses[:, :5].cpu()
        print(f'[pose-loss] nonfinite {where} {value} {mode}: hip {(~torch.isfinite(got)).int().tolist()} fp32 {(~torch.isfinite(want)).int().tolist()}')
        assert torch.equal(torch.isfinite(got), torch.isfinite(want)), (where, value, mode)
        if where != 'target_depth':
            clean = _kernel_outputs('typical32', mode)['by_weight'][MIXED]['losses']
            assert torch.equal(got[[0, 2]], clean[[0, 2], :5])
    if where == 'depth_logit_under_closed_mask' and value != value:
        # the planted logit's own gradient entry is NaN too, as autograd through (tanh(nan) + 1) * 0 - 1 gives; samples 0 and 2
        # keep finite gradients
        _, _, gsums = _hip_forward('logits', crop.to(DEV), cf, td.to(DEV), inp['tm'].to(DEV), MIXED)
        glogits, _ = _hip_backward('logits', crop.to(DEV), cf, td.to(DEV), inp['tm'].to(DEV), gsums)
        g32 = _expressions32(crop, inp['vp'], inp['tz'], td, inp['tm'], 'logits')['grads']
        assert torch.isnan(_combine(g32, MIXED, 3, 0)[1, 0, 15, 16]) and torch.isnan(glogits[1, 0, 15, 16])
        assert torch.isfinite(glogits[[0, 2]]).all()


VARIANT_CASE = {'round_half_up': 'ties', 'depth_bilinear': 'typical32', 'align_corners': 'typical32', 'zeros_padding': 'overhang_left_top',
                'invalid_mask_gt_0': 'faint_rim', 's5_without_valid': 'typical32', 'bce_over_mask': 'typical32'}


@pytest.mark.parametrize('variant', VARIANTS)
def test_comparison_rejects_a_wrong_reference(variant):
    """The bounds mean something: the same helper that accepts the kernels' forward outputs against the fp64 restatement
    rejects them against each plausible misreading of the loss (fp64 as well), on the case that exposes it."""
    case = VARIANT_CASE[variant]
    inp = _inputs(case)
    for mode in ('depth', 'logits'):
        ref64, ref32, expr32 = _references(case, mode)
        hip = _kernel_outputs(case, mode)['by_weight'][MIXED]
        rows = inp['rows']
        assert not _compare(f'{case} {mode}', _rows_of(hip, rows), MIXED, ref64, ref32, expr32, inp['N'], forward_only=True)
        wrong = {}
        for dt in (torch.float64, torch.float32):                  # e32 of the variant = the variant's own fp32 evaluation
            crop, vp, tz = (t[rows].to(dt) for t in (inp['crops'][mode], inp['vp'], inp['tz']))
            wrong[dt] = _reference(crop, _coefs6(vp, tz, inp['h'], inp['w']), inp['td'].to(dt), inp['tm'].to(dt), mode, variant)
        bad = _compare(f'{case} {mode} vs {variant}', _rows_of(hip, rows), MIXED, wrong[torch.float64], wrong[torch.float32],
                       wrong[torch.float32], inp['N'], forward_only=True)
        assert bad, f'{variant} on {case} ({mode}) passes the same bounds as the true reference'
