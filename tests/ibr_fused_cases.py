"""Shared by tests/test_ibr_fused_gpu.py and tests/test_ibr_fused_args.py: seeded cameras and inputs for the fused IBR
reprojection, the composed code evaluated in fp64 / fp32 on the host (computed once per case and cached), a parametrised
re-statement of the composed arithmetic from which the deliberately WRONG references are made, and the bounds."""
import functools

import torch

from oracle_util import in_fp64

FRAME_W, FRAME_H = 640, 480


def make_cameras(n_in, n_out, batch=1, dtype=torch.float32, device='cpu'):
    """Flat object-major cameras on a 480 x 640 frame.  Rotations 0.15-0.4 rad apart between every (output, input) pair,
    slightly different translations around t_z = 1, distinct viewports that are not the full frame: input view 1 overhangs
    the left frame edge, input view 2 / output view 1 have viewport_height != viewport_width.  No output camera equals an
    input camera."""
    from latentfusion_amd.modules.geometry import Camera
    # log quaternion = axis * angle / 2
    lq_in = torch.tensor([[0.010, 0.000, 0.005], [0.000, 0.150, -0.010], [0.012, -0.125, 0.000]], dtype=torch.float64)
    lq_out = torch.tensor([[-0.025, 0.070, 0.000], [0.075, -0.025, 0.010]], dtype=torch.float64)
    t_in = torch.tensor([[0.010, -0.020, 1.000], [-0.030, 0.015, 1.030], [0.025, 0.020, 0.980]], dtype=torch.float64)
    t_out = torch.tensor([[-0.015, 0.010, 1.010], [0.020, -0.010, 0.990]], dtype=torch.float64)
    vp_in = torch.tensor([[215.0, 140.0, 425.0, 350.0], [-20.0, 120.0, 215.0, 355.0], [230.0, 110.0, 440.0, 370.0]],
                         dtype=torch.float64)
    vp_out = torch.tensor([[205.0, 134.5, 430.0, 360.0], [222.0, 128.0, 418.0, 372.0]], dtype=torch.float64)
    K = torch.tensor([[600.0, 0.0, 320.0], [0.0, 590.0, 240.0], [0.0, 0.0, 1.0]], dtype=torch.float64)

    def build(lq, t, vp, n):
        rows = []
        for b in range(batch):                                  # each object gets its own small perturbation
            k = torch.arange(n) % len(lq)
            rows.append((lq[k] + 0.004 * b, t[k] + 0.006 * b, vp[k] + 3.0 * b))
        lq_, t_, vp_ = (torch.cat([r[j] for r in rows]).to(dtype).to(device) for j in range(3))
        return Camera(K.to(dtype).to(device).expand(len(lq_), -1, -1).clone(), None, 0.5, vp_, width=FRAME_W, height=FRAME_H,
                      log_quaternion=lq_, translation=t_)

    t_in = t_in.clone()
    t_in[1, 0] = -0.36                                          # projects the object to u ~ 104: inside the overhanging viewport
    return build(lq_in, t_in, vp_in, n_in), build(lq_out, t_out, vp_out, n_out)


def make_inputs(batch, n_in, n_out, C, H, W, clamped=False):
    """Smooth fp64 fields: image_in (B,V_i,C,H,W), depth_in (B,V_i,1,H,W) around t_z, depth_out (B,V_o,1,H,W) within
    +-0.5.  clamped: the top tenth of the rows of depth_in is pushed 0.7 behind, which drives the normalised transformed
    depth of those taps into its upper clamp."""
    y = torch.linspace(0, 1, H, dtype=torch.float64).view(1, 1, 1, H, 1)
    x = torch.linspace(0, 1, W, dtype=torch.float64).view(1, 1, 1, 1, W)
    b = torch.arange(batch, dtype=torch.float64).view(batch, 1, 1, 1, 1)
    vi = torch.arange(n_in, dtype=torch.float64).view(1, n_in, 1, 1, 1)
    vo = torch.arange(n_out, dtype=torch.float64).view(1, n_out, 1, 1, 1)
    c = torch.arange(C, dtype=torch.float64).view(1, 1, C, 1, 1)
    image_in = torch.sin(3.1 * x + 0.7 * c + 0.9 * vi + 0.4 * b) * torch.cos(2.3 * y - 0.5 * c + 0.3 * vi) + 0.2 * c
    depth_in = 1.0 + 0.05 * torch.sin(2.9 * x + 1.7 * y + 0.8 * vi + 0.5 * b)
    depth_out = 0.42 * torch.sin(2.1 * x + 0.6 * vo + 0.3 * b) * torch.cos(1.9 * y + 0.4 * vo)
    if clamped:
        depth_in = depth_in + 0.7 * (y < 0.1).to(torch.float64)
    return image_in, depth_in, depth_out


def directions(shape_image, shape_depth, seed=11):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape_image, generator=g, dtype=torch.float64), torch.randn(shape_depth, generator=g, dtype=torch.float64))


def cast_camera(cam, dtype, device='cpu'):
    return cam._map(lambda t: t.detach().to(device=device, dtype=dtype))


def slice_cameras(cam, b, n):
    return cam[b * n:(b + 1) * n]


# ---- a re-statement of reproject_views from which the wrong references are made ----------------------------------------
def restated(image_in, depth_in, depth_out, cam_in, cam_out, swap_hw=False, denorm_in=False, eps=0.01, padding='zeros',
             align_corners=False, in_bounds=False, clamp=True, return_coords=False):
    """reproject_views of one object written out ((V_i,C,H,W), (V_i,1,H,W), (V_o,1,H,W) -> (V_o,V_i,C|1,H,W)); every
    keyword switches ONE of the mirrored quirks to the plausible wrong choice."""
    import torch.nn.functional as F
    dt = image_in.dtype
    H, W = image_in.shape[-2:]
    v_i, v_o = len(cam_in), len(cam_out)

    def lattice(cam):
        lv, lu = torch.linspace(0, 1, H, dtype=dt), torch.linspace(0, 1, W, dtype=dt)
        if swap_hw:                                             # the lattice steps taken from the other dimension
            lv, lu = torch.arange(H, dtype=dt) / (W - 1), torch.arange(W, dtype=dt) / (H - 1)
        v, u = torch.meshgrid(lv, lu, indexing='ij')
        u = u[None] * cam.viewport_width.view(-1, 1, 1) + cam.viewport[:, 0].view(-1, 1, 1)
        v = v[None] * cam.viewport_height.view(-1, 1, 1) + cam.viewport[:, 1].view(-1, 1, 1)
        return u, v

    def points(cam, z):                                         # camera-space points of the lattice, homogeneous (V,H,W,4)
        u, v = lattice(cam)
        x = (u - cam.u0.view(-1, 1, 1)) / cam.fu.view(-1, 1, 1) * z
        y = (v - cam.v0.view(-1, 1, 1)) / cam.fv.view(-1, 1, 1) * z
        return torch.stack((x, y, z, torch.ones_like(z)), dim=-1)

    def bounds(cam):
        return cam.znear - eps, cam.zfar + eps

    zn_o, zf_o = bounds(cam_out)
    z_out = (depth_out[:, 0] / 2 + 0.5) * (zf_o - zn_o).view(-1, 1, 1) + zn_o.view(-1, 1, 1)
    obj = torch.einsum('vij,vhwj->vhwi', cam_out.cam_to_obj, points(cam_out, z_out))                     # (V_o,H,W,4)
    pix = torch.einsum('iaj,ohwj->oihwa', cam_in.obj_to_image, obj)                                      # (V_o,V_i,H,W,3)
    px, py = pix[..., 0] / pix[..., 2], pix[..., 1] / pix[..., 2]
    vp = cam_in.viewport
    gx = (px - vp[:, 0].view(1, -1, 1, 1)) / (vp[:, 2] - vp[:, 0]).view(1, -1, 1, 1) * 2 - 1
    gy = (py - vp[:, 1].view(1, -1, 1, 1)) / (vp[:, 3] - vp[:, 1]).view(1, -1, 1, 1) * 2 - 1
    grid = torch.stack((gx, gy), dim=-1).reshape(v_o * v_i, H, W, 2)
    z_in = depth_in[:, 0]
    if denorm_in:
        zn_i, zf_i = bounds(cam_in)
        z_in = (z_in / 2 + 0.5) * (zf_i - zn_i).view(-1, 1, 1) + zn_i.view(-1, 1, 1)
    obj_in = torch.einsum('vij,vhwj->vhwi', cam_in.cam_to_obj, points(cam_in, z_in))                     # (V_i,H,W,4)
    z_tf = torch.einsum('oj,ihwj->oihw', cam_out.obj_to_cam[:, 2], obj_in)                               # (V_o,V_i,H,W)
    zn, zf = bounds(cam_in) if in_bounds else (zn_o, zf_o)
    zn, zf = (zn.view(1, -1, 1, 1), zf.view(1, -1, 1, 1)) if in_bounds else (zn.view(-1, 1, 1, 1), zf.view(-1, 1, 1, 1))
    d = (z_tf - zn) / (zf - zn)
    if clamp:
        d = d.clamp(0, 1)
    d = d * 2 - 1
    image = image_in[None].expand(v_o, -1, -1, -1, -1).reshape(v_o * v_i, -1, H, W)
    image_re = F.grid_sample(image, grid, mode='bilinear', padding_mode=padding, align_corners=align_corners)
    depth_re = F.grid_sample(d.reshape(v_o * v_i, 1, H, W), grid, mode='bilinear', padding_mode=padding,
                             align_corners=align_corners)
    out = image_re.view(v_o, v_i, -1, H, W), depth_re.view(v_o, v_i, 1, H, W)
    if return_coords:
        sx = ((gx + 1) * W - 1) / 2
        sy = ((gy + 1) * H - 1) / 2
        return out + (sx, sy, d)
    return out


WRONG = {
    'lattice_hw_swapped': dict(swap_hw=True),
    'depth_in_denormalised': dict(denorm_in=True),
    'depth_bounds_eps_dropped': dict(eps=0.0),
    'border_padding': dict(padding='border'),
    'align_corners': dict(align_corners=True),
    'input_camera_bounds': dict(in_bounds=True),
}


def emulate(rec, image_in, depth_in, depth_out):
    """The arithmetic lf_ibr_reproject_fwd is specified to do with the packed records (include/lf_hip.h), in the records'
    dtype on the host, for one object: pair (V_o,V_i,32), view_in (V_i,16), view_out (V_o,16); the two floats of a
    coordinate entry are summed first."""
    import torch.nn.functional as F
    pair, vin, vout = (r.clone() for r in rec)
    pair[..., :12] += pair[..., 16:28]
    vout[..., :6] += vout[..., 8:14]
    dt = pair.dtype
    H, W = image_in.shape[-2:]
    v_o, v_i = pair.shape[:2]
    ly, lx = torch.meshgrid(torch.linspace(0, 1, H, dtype=dt), torch.linspace(0, 1, W, dtype=dt), indexing='ij')

    def rays(v):
        return lx[None] * v[:, 0].view(-1, 1, 1) + v[:, 1].view(-1, 1, 1), ly[None] * v[:, 2].view(-1, 1, 1) + v[:, 3].view(-1, 1, 1)

    xn, yn = rays(vout)
    z = depth_out[:, 0] * vout[:, 4].view(-1, 1, 1) + vout[:, 5].view(-1, 1, 1)
    P = torch.stack((xn * z, yn * z, z, torch.ones_like(z)), dim=-1)                                     # (V_o,H,W,4)
    p = torch.einsum('oiaj,ohwj->oihwa', pair[..., :12].reshape(v_o, v_i, 3, 4), P)
    sx, sy = p[..., 0] / p[..., 2] * W - 0.5, p[..., 1] / p[..., 2] * H - 0.5
    grid = torch.stack(((2 * sx + 1) / W - 1, (2 * sy + 1) / H - 1), dim=-1).reshape(v_o * v_i, H, W, 2)
    xi, yi = rays(vin)
    zi = depth_in[:, 0]
    Pi = torch.stack((xi * zi, yi * zi, zi, torch.ones_like(zi)), dim=-1)                                # (V_i,H,W,4)
    d = torch.einsum('oij,ihwj->oihw', pair[..., 12:16], Pi).clamp(0, 1) * 2 - 1
    image = image_in[None].expand(v_o, -1, -1, -1, -1).reshape(v_o * v_i, -1, H, W)
    image_re = F.grid_sample(image, grid, mode='bilinear', padding_mode='zeros', align_corners=False)
    depth_re = F.grid_sample(d.reshape(v_o * v_i, 1, H, W), grid, mode='bilinear', padding_mode='zeros', align_corners=False)
    return image_re.view(v_o, v_i, -1, H, W), depth_re.view(v_o, v_i, 1, H, W)


# ---- the reference, once per case -------------------------------------------------------------------------------------
def _run(fn, dtype, batch, n_in, n_out, tensors, cam_in, cam_out, dirs):
    """fn per object in `dtype` on the host with gradients along `dirs` -> dict of (B,...) fp64 tensors."""
    image_in, depth_in, depth_out = (t.to(dtype).clone().requires_grad_(True) for t in tensors)
    ci, co = cast_camera(cam_in, dtype), cast_camera(cam_out, dtype)
    imgs, deps = [], []
    for b in range(batch):
        a, d = fn(image_in[b], depth_in[b], depth_out[b], slice_cameras(ci, b, n_in), slice_cameras(co, b, n_out))
        imgs.append(a)
        deps.append(d)
    image_re, depth_re = torch.stack(imgs), torch.stack(deps)
    out = {'image_re': image_re.detach().double(), 'depth_re': depth_re.detach().double()}
    if dirs is not None:
        ((image_re * dirs[0].to(dtype)).sum() + (depth_re * dirs[1].to(dtype)).sum()).backward()
        out.update(g_image_in=image_in.grad.double(), g_depth_in=depth_in.grad.double(), g_depth_out=depth_out.grad.double())
    return out


@functools.lru_cache(maxsize=None)
def case(batch, n_in, n_out, C, H, W, clamped=False):
    """Inputs, cameras, directions, the composed code in fp64 (`ref`) and in fp32 (`e32` = |fp32 - fp64|), the mask of
    (b, o, i, pixel) whose fp64 sampling coordinate is within 1e-4 of an integer (gradient comparisons leave them out:
    the directions are zero there), and the share of clamped taps.  Cached: tests share it and must not modify it."""
    from latentfusion_amd import ibr
    # every input is an fp32 value held in fp64: the fp64 reference, the fp32 yardstick and the kernel see the same numbers
    cam_in, cam_out = (cast_camera(cast_camera(c, torch.float32), torch.float64) for c in make_cameras(n_in, n_out, batch, torch.float64))
    tensors = tuple(t.float().double() for t in make_inputs(batch, n_in, n_out, C, H, W, clamped))

    def composed(*a):
        return ibr.reproject_views(*a, kernel='composed')

    # sampling coordinates of the fp64 evaluation -> what the gradient comparisons leave out
    near, taps_clamped = [], []
    for b in range(batch):
        _, _, sx, sy, d = in_fp64(lambda: restated(tensors[0][b], tensors[1][b], tensors[2][b], slice_cameras(cam_in, b, n_in),
                                                   slice_cameras(cam_out, b, n_out), return_coords=True))
        near.append(((sx - sx.round()).abs() < 1e-4) | ((sy - sy.round()).abs() < 1e-4))
        taps_clamped.append(d.abs() >= 1.0)
    near = torch.stack(near)                                                       # (B,V_o,V_i,H,W)
    taps_clamped = torch.stack(taps_clamped)                                       # (B,V_o,V_i,H,W) of INPUT pixels
    dirs = directions((batch, n_out, n_in, C, H, W), (batch, n_out, n_in, 1, H, W))
    keep = (~near).unsqueeze(3).to(torch.float64)
    dirs = tuple((d * keep).float().double() for d in dirs)
    ref = in_fp64(lambda: _run(composed, torch.float64, batch, n_in, n_out, tensors, cam_in, cam_out, dirs))
    f32 = _run(composed, torch.float32, batch, n_in, n_out, tensors, cam_in, cam_out, dirs)
    e32 = {k: (f32[k] - ref[k]).abs() for k in ref}
    return dict(cam_in=cam_in, cam_out=cam_out, tensors=tensors, dirs=dirs, ref=ref, e32=e32, near=near,
                taps_clamped=taps_clamped, dims=(batch, n_in, n_out, C, H, W))


def wrong_reference(cs, name):
    """Forward outputs of the composed arithmetic with one quirk switched (fp64)."""
    batch, n_in, n_out = cs['dims'][:3]
    kw = dict(clamp=False) if name == 'clamp_omitted' else WRONG[name]
    return in_fp64(lambda: _run(lambda *a: restated(*a, **kw), torch.float64, batch, n_in, n_out, cs['tensors'], cs['cam_in'],
                                cs['cam_out'], None))


# ---- the bounds (tests/test_pose_loss_fp64_gpu.py's rule) ------------------------------------------------------------------
def forward_excess(got, ref, e32):
    """max over elements of |got - ref| - max(4 e32, 2e-6 + 2e-5 |ref|): <= 0 passes.  NaN counts as +inf."""
    err = (got.double().cpu() - ref).abs()
    ex = err - torch.maximum(4 * e32, 2e-6 + 2e-5 * ref.abs())
    return torch.nan_to_num(ex, nan=float('inf')).max().item(), err.max().item()


def gradient_excess(got, ref, e32, keep=None):
    err = (got.double().cpu() - ref).abs()
    ex = err - torch.maximum(4 * e32, torch.full_like(ref, 2e-3 * ref.abs().max().item()))
    if keep is not None:
        ex, err = ex[keep], err[keep]
    return torch.nan_to_num(ex, nan=float('inf')).max().item(), err.max().item()
