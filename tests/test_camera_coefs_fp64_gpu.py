"""lf_camera_coefs / lf_camera_coefs_bwd (csrc/image.hip: fp64 dual numbers, one thread per camera x parameter) over the
parameter space, against modules.geometry.o2c_coefficients plus the uncrop / depth block evaluated in fp64 with torch autograd:

  rotation     |log_quaternion| = 0 (exactly), 1e-9, 1e-6, 1e-3, 1, pi - 1e-3, pi, 4: both sides of the clamp(min=1e-8) inside qexp,
               the norm's sub-gradient at 0, the half turn
  viewports    8 .. 2000 pixels wide, partly negative; crop_h != crop_w; z_span 0.25 / 0.5; cube_size 1 / 0.7
  N            1, 6, 7 (60 / 70 threads: the edge of the 64-thread block), 128
  Jacobian     all 24 x 10 entries: one backward per one-hot gcoefs column, not one random weighting

Bounds (those of test_camera_coefs_and_jacobian): values atol 1e-6 / rtol 1e-5 (uncrop block atol 1e-5), Jacobian entries to
1e-4 of the largest entry of their row (one coefficient's ten derivatives).  The kernel computes in fp64 and rounds once, and
o2c_coefficients itself returns its fp64 result rounded to fp32, so both sit within an fp32 ulp of each other.
Measured on an MI355X: values within 1.2e-7 relative (one fp32 ulp), Jacobian entries within 7.6e-8 of their row's largest."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NORMS = (0.0, 1e-9, 1e-6, 1e-3, 1.0, math.pi - 1e-3, math.pi, 4.0)


def _params(N, gen):
    """fp32 camera parameters: rotation norms cycling through NORMS (random axes), t_z around 1, viewports 8 .. 2000 wide."""
    axis = torch.randn(N, 3, generator=gen).double()
    axis = axis / axis.norm(dim=1, keepdim=True)
    norms = torch.tensor([NORMS[i % len(NORMS)] for i in range(N)], dtype=torch.float64)
    log_q = (axis * norms[:, None]).float()
    t = torch.cat((0.1 * torch.randn(N, 2, generator=gen), 1.0 + 0.2 * torch.rand(N, 1, generator=gen)), dim=1)
    widths = torch.tensor([8.0, 30.5, 280.25, 640.0, 1000.75, 2000.0])[torch.arange(N) % 6]
    heights = widths * (0.6 + 0.8 * torch.rand(N, generator=gen))
    x0 = -0.4 * widths + 300 * torch.rand(N, generator=gen)                     # negative for the wide ones
    y0 = -0.4 * heights + 200 * torch.rand(N, generator=gen)
    vp = torch.stack((x0, y0, x0 + widths, y0 + heights), dim=1)
    K = torch.tensor([[572.4, 0.0, 325.3], [0.0, 573.6, 242.0], [0.0, 0.0, 1.0]]).expand(N, -1, -1).contiguous()
    return log_q, t, vp, K, norms


def _camera(log_q, t, vp, K, z_span):
    from latentfusion_amd.modules.geometry import Camera
    return Camera(K, None, z_span, vp, width=640, height=480, log_quaternion=log_q, translation=t)


def _jacobian(coefs, leaves):
    """(N, 24, 10): row j = the derivatives of coefficient j, from one backward with the one-hot gcoefs column j."""
    rows = []
    for j in range(coefs.shape[1]):
        e = torch.zeros_like(coefs)
        e[:, j] = 1.0
        g = torch.autograd.grad(coefs, leaves, grad_outputs=e, retain_graph=True, allow_unused=True)
        rows.append(torch.cat([torch.zeros_like(x) if gi is None else gi for gi, x in zip(g, leaves)], dim=1))
    return torch.stack(rows, dim=1)


def _check(N, crop_h, crop_w, z_span, cube, seed, take=None):
    from latentfusion_amd.engine import camera_coefs
    from latentfusion_amd.modules.geometry import o2c_coefficients
    gen = torch.Generator().manual_seed(seed)
    log_q, t, vp, K, norms = (x[:take] for x in _params(N, gen))      # take: the first rows of the same batch
    # fp64 reference on the same fp32 parameters
    leaves64 = [x.double().requires_grad_(True) for x in (log_q, t, vp)]
    cam64 = _camera(*leaves64, K.double(), z_span)
    vw, vh = leaves64[2][:, 2] - leaves64[2][:, 0], leaves64[2][:, 3] - leaves64[2][:, 1]
    extra = torch.stack((crop_w / vw, -leaves64[2][:, 0] * crop_w / vw - 0.5, crop_h / vh, -leaves64[2][:, 1] * crop_h / vh - 0.5,
                         torch.full_like(vw, z_span + 0.01), leaves64[1][:, 2]), dim=1)
    want = torch.cat((o2c_coefficients(cam64, cube).double(), extra), dim=1)
    J64 = _jacobian(want, leaves64)
    # the kernels
    leaves = [x.to(DEV).requires_grad_(True) for x in (log_q, t, vp)]
    got = camera_coefs(_camera(*leaves, K.to(DEV), z_span), cube, crop_h, crop_w)
    J = _jacobian(got, leaves).cpu().double()
    got = got.detach().cpu().double()
    assert torch.isfinite(got).all() and torch.isfinite(J).all()
    torch.testing.assert_close(got[:, :18], want[:, :18].detach(), atol=1e-6, rtol=1e-5)
    torch.testing.assert_close(got[:, 18:], want[:, 18:].detach(), atol=1e-5, rtol=1e-5)
    row_max = J64.abs().amax(dim=2, keepdim=True)
    err = (J - J64).abs()
    rel_v = float(((got - want.detach()).abs() / want.detach().abs().clamp(min=1e-3)).max())
    rel_j = float((err / row_max.clamp(min=1e-30))[row_max.expand_as(err) > 0].max())
    print(f'[camera-coefs] N={log_q.shape[0]} crop={crop_h}x{crop_w} z_span={z_span} cube={cube}: values rel {rel_v:.2e}  jacobian/row max {rel_j:.2e}')
    assert (err <= 1e-4 * row_max).all(), (err / row_max.clamp(min=1e-30)).max()
    # at |log_q| = 0 exactly the reference's own gradient is zero (sub-gradient of the norm, sin(0) / 1e-8): so is the kernel's
    zero = norms == 0
    assert zero.any() and (J64[zero][:, :, :3] == 0).all() and (J[zero][:, :, :3] == 0).all()
    return got, J


@pytest.mark.parametrize('crop', [(16, 16), (24, 40), (128, 96)])
@pytest.mark.parametrize('z_span,cube', [(0.5, 1.0), (0.25, 0.7)])
def test_camera_coefs_and_full_jacobian_vs_fp64(crop, z_span, cube):
    _check(48, crop[0], crop[1], z_span, cube, seed=crop[0] + crop[1])


@pytest.mark.parametrize('N', [1, 6, 7, 128])
def test_camera_coefs_block_edges(N):
    """N * 10 threads in blocks of 64: 10, 60 (four short of a block), 70 (six into the second block), 1280."""
    got, J = _check(N, 24, 40, 0.5, 1.0, seed=N)
    if N > 1:                                                      # a row does not depend on the batch it is computed in
        got1, J1 = _check(N, 24, 40, 0.5, 1.0, seed=N, take=1)
        assert torch.equal(got[:1], got1) and torch.equal(J[:1], J1)
