"""lf_ibr_reproject_fwd / _bwd (ops.ibr_reproject, kernel='fused' of latentfusion_amd.ibr) on the GPU.

The reference in every case is ibr.reproject_views ('composed') evaluated in fp64 on the host; e32 is the same composed
code in fp32 on the same inputs (tests/ibr_fused_cases.py computes both once per case).  Bounds, the project's rule from
tests/test_pose_loss_fp64_gpu.py:
  forward    |kernel - ref| <= max(4 e32, 2e-6 + 2e-5 |ref|) per element;
  gradients  |kernel - ref| <= max(4 e32, 2e-3 of the largest component of that gradient tensor), with every (o, i, pixel)
             whose fp64 sampling coordinate is within 1e-4 of an integer left out (the sampler's gradient jumps there), a
             g_depth_out pixel if any of its i is; at most 1 % may be left out.
Each test prints its figures before it asserts."""
import pytest
import torch

import ibr_fused_cases as K

pytestmark = pytest.mark.gpu
DEV = 'cuda'

MAIN = (2, 3, 2, 3, 24, 32)                        # B, V_i, V_o, C, H, W
CASES = [MAIN, (1, 1, 1, 1, 5, 7), (1, 3, 2, 4, 33, 65), (2, 1, 2, 1, 33, 65), (1, 3, 1, 4, 5, 7)]


def _device(cs, grad=False):
    from latentfusion_amd import ops
    B = cs['dims'][0]
    t = [x.float().to(DEV).requires_grad_(grad) for x in cs['tensors']]
    rec = ops.pack_ibr_cameras(K.cast_camera(cs['cam_in'], torch.float32, DEV), K.cast_camera(cs['cam_out'], torch.float32, DEV),
                               batch_size=B)
    return t, rec


def _fused(cs, grad=True):
    from latentfusion_amd import ops
    t, rec = _device(cs, grad)
    image_re, depth_re = ops.ibr_reproject(t[0], t[1], t[2], rec)
    out = {'image_re': image_re.detach(), 'depth_re': depth_re.detach()}
    if grad:
        ((image_re * cs['dirs'][0].float().to(DEV)).sum() + (depth_re * cs['dirs'][1].float().to(DEV)).sum()).backward()
        out.update(g_image_in=t[0].grad, g_depth_in=t[1].grad, g_depth_out=t[2].grad)
    return out


def _check(cs, got, label):
    near = cs['near']
    share = near.double().mean().item()
    print(f'{label}: excluded share {share:.3e}, clamped taps {cs["taps_clamped"].double().mean().item():.3e}')
    assert share <= 0.01
    bad = []
    for k in ('image_re', 'depth_re'):
        ex, err = K.forward_excess(got[k], cs['ref'][k], cs['e32'][k])
        print(f'  {k}: max err {err:.3e} (e32 max {cs["e32"][k].max().item():.3e}, |ref| max {cs["ref"][k].abs().max().item():.3e}), excess {ex:.3e}')
        bad += [k] if ex > 0 else []
    keep_out = ~near.any(dim=2).unsqueeze(2)                                        # (B,V_o,1,H,W)
    for k, keep in (('g_image_in', None), ('g_depth_in', None), ('g_depth_out', keep_out)):
        ex, err = K.gradient_excess(got[k], cs['ref'][k], cs['e32'][k], keep)
        print(f'  {k}: max err {err:.3e} (e32 max {cs["e32"][k].max().item():.3e}, |ref| max {cs["ref"][k].abs().max().item():.3e}), excess {ex:.3e}')
        bad += [k] if ex > 0 else []
    assert not bad, bad


@pytest.mark.parametrize('dims', CASES, ids=lambda d: 'B%d_Vi%d_Vo%d_C%d_%dx%d' % d)
def test_forward_and_gradients_against_fp64(dims):
    cs = K.case(*dims)
    assert not cs['taps_clamped'].any()                                              # the smooth depths stay off the clamp
    _check(cs, _fused(cs), str(dims))


def test_clamped_taps_pass_no_gradient():
    """A tenth of the taps of depth_in in the clamp of the normalised depth: values and gradients within the bounds, and
    g_depth_in exactly 0 at every input pixel that every output camera sees clamped."""
    cs = K.case(*MAIN, clamped=True)
    share = cs['taps_clamped'].double().mean().item()
    assert 0.05 <= share <= 0.2, share
    got = _fused(cs)
    _check(cs, got, 'clamped')
    dead = cs['taps_clamped'].all(dim=1).unsqueeze(2)                                # (B,V_i,1,H,W)
    assert dead.any()
    assert (got['g_depth_in'].cpu()[dead] == 0).all()
    assert (cs['ref']['g_depth_in'][dead] == 0).all()


@pytest.mark.parametrize('name', list(K.WRONG) + ['clamp_omitted'])
def test_wrong_references_are_rejected(name):
    """The forward bound that accepts the kernel rejects the composed arithmetic with one quirk switched."""
    cs = K.case(*MAIN, clamped=(name == 'clamp_omitted'))
    got = _fused(cs, grad=False)
    wrong = K.wrong_reference(cs, name)
    ex = {k: K.forward_excess(got[k], wrong[k], cs['e32'][k])[0] for k in ('image_re', 'depth_re')}
    right = {k: K.forward_excess(got[k], cs['ref'][k], cs['e32'][k])[0] for k in ('image_re', 'depth_re')}
    print(name, 'excess against the wrong reference', ex, 'against the right one', right)
    assert max(right.values()) <= 0
    assert max(ex.values()) > 0


# ---------------------------------------------------------------------------------------------------------------------
# bit for bit
# ---------------------------------------------------------------------------------------------------------------------
def _sub_records(cs, b=None, o=None, i=None):
    """Records of object b alone, or of the single pair (o, i) of object b."""
    from latentfusion_amd import ops
    _, n_in, n_out = cs['dims'][:3]
    ci = K.slice_cameras(K.cast_camera(cs['cam_in'], torch.float32, DEV), b, n_in)
    co = K.slice_cameras(K.cast_camera(cs['cam_out'], torch.float32, DEV), b, n_out)
    if o is not None:
        ci, co = ci[i], co[o]
    return ops.pack_ibr_cameras(ci, co, batch_size=1)


def test_batch_and_rows_are_independent():
    """A B = 2 call equals two B = 1 calls, and row (o, i) of a V_o = 2, V_i = 3 call equals the V_o = V_i = 1 call on that
    pair -- forward and all three gradients' deterministic part (g_depth_out needs all i, so it is compared per object)."""
    from latentfusion_amd import ops
    cs = K.case(*MAIN)
    whole = _fused(cs)
    t, _ = _device(cs)
    for b in range(2):
        tb = [x[b:b + 1].clone().requires_grad_(True) for x in t]
        image_re, depth_re = ops.ibr_reproject(tb[0], tb[1], tb[2], _sub_records(cs, b))
        assert torch.equal(image_re, whole['image_re'][b:b + 1]) and torch.equal(depth_re, whole['depth_re'][b:b + 1])
        ((image_re * cs['dirs'][0][b:b + 1].float().to(DEV)).sum() + (depth_re * cs['dirs'][1][b:b + 1].float().to(DEV)).sum()).backward()
        assert torch.equal(tb[2].grad, whole['g_depth_out'][b:b + 1])
        for o in range(2):
            for i in range(3):
                a, d = ops.ibr_reproject(t[0][b:b + 1, i:i + 1], t[1][b:b + 1, i:i + 1], t[2][b:b + 1, o:o + 1],
                                         _sub_records(cs, b, o, i))
                assert torch.equal(a[0, 0, 0], whole['image_re'][b, o, i]), (b, o, i)
                assert torch.equal(d[0, 0, 0], whole['depth_re'][b, o, i]), (b, o, i)


def test_mask_in_the_store_equals_the_torch_expressions():
    from latentfusion_amd import ops
    cs = K.case(*MAIN)
    t, rec = _device(cs)
    B, _, n_out, _, H, W = cs['dims']
    g = torch.Generator().manual_seed(5)
    mask = torch.rand(B, n_out, 1, H, W, generator=g).to(DEV)                        # soft mask: products that round
    mask[:, :, :, :3] = 0.0
    mask[:, :, :, 3:6] = 1.0
    image_re, depth_re = ops.ibr_reproject(t[0], t[1], t[2], rec)
    image_m, depth_m = ops.ibr_reproject(t[0], t[1], t[2], rec, mask_out=mask)
    assert torch.equal(image_m, image_re * mask.unsqueeze(2))
    assert torch.equal(depth_m, (depth_re + 1.0) * mask.unsqueeze(2) - 1.0)
    # and its gradient: the directions are the gradients of the masked outputs
    tg = [x.clone().requires_grad_(True) for x in t]
    a, d = ops.ibr_reproject(tg[0], tg[1], tg[2], rec, mask_out=mask)
    gi, gd = cs['dirs'][0].float().to(DEV), cs['dirs'][1].float().to(DEV)
    ((a * gi).sum() + (d * gd).sum()).backward()
    tu = [x.clone().requires_grad_(True) for x in t]
    a, d = ops.ibr_reproject(tu[0], tu[1], tu[2], rec)
    ((a * mask.unsqueeze(2) * gi).sum() + (((d + 1.0) * mask.unsqueeze(2) - 1.0) * gd).sum()).backward()
    assert torch.equal(tg[2].grad, tu[2].grad)                                       # deterministic, same products
    for x, y in zip(tg[:2], tu[:2]):                                                 # atomics: last bits may differ
        torch.testing.assert_close(x.grad, y.grad, atol=1e-5 * y.grad.abs().max().item(), rtol=0)
    with pytest.raises(NotImplementedError):
        ops.ibr_reproject(t[0], t[1], t[2], rec, mask_out=mask.clone().requires_grad_(True))


def test_strided_output_lands_in_the_generator_stack():
    from latentfusion_amd import ops
    cs = K.case(*MAIN)
    t, rec = _device(cs)
    B, n_in, n_out, C, H, W = cs['dims']
    image_re, depth_re = ops.ibr_reproject(t[0], t[1], t[2], rec)
    SENT = -12345.0
    buf = torch.full((B * n_out * n_in * (C + 2) * H * W + 2 * H * W,), SENT, device=DEV)
    stack = buf[H * W:-H * W].view(B * n_out, n_in, C + 2, H, W)                        # guard planes before and after
    a, d = ops.ibr_reproject(t[0], t[1], t[2], rec, out=stack)
    assert a.data_ptr() == stack.data_ptr() and a.shape == image_re.shape and d.shape == depth_re.shape
    assert torch.equal(a, image_re) and torch.equal(d, depth_re)
    assert torch.equal(stack[:, :, :C], image_re.flatten(0, 1)) and torch.equal(stack[:, :, C:C + 1], depth_re.flatten(0, 1))
    assert (stack[:, :, C + 1] == SENT).all() and (buf[:H * W] == SENT).all() and (buf[-H * W:] == SENT).all()
    with pytest.raises(NotImplementedError):
        ops.ibr_reproject(t[0].clone().requires_grad_(True), t[1], t[2], rec, out=stack)
    with pytest.raises(ValueError):
        ops.ibr_reproject(t[0], t[1], t[2], rec, out=stack[:, :, :C + 1])


def test_row_stride_past_2_to_the_31_elements():
    """The output row offset is 64-bit: with a row stride of 2^31 + 64 floats the second row (input view 1) lands 8 GiB past
    the first, with the values of the packed call, and nothing is written where a 32-bit offset would have put it."""
    from latentfusion_amd import _lib, ops
    L = _lib.lib()
    cs = K.case(1, 3, 1, 4, 5, 7)
    t, rec = _device(cs)
    B, n_in, n_out, C, H, W = cs['dims']
    image_re, depth_re = ops.ibr_reproject(t[0], t[1], t[2], rec)
    stride = 2 ** 31 + 64
    row = (C + 1) * H * W
    buf = torch.empty(2 * stride + row, device=DEV)                                  # rows 0, 1, 2 at 0, stride, 2 * stride
    SENT = -7.0
    heads = [buf[k * stride:k * stride + row] for k in range(3)]
    guard = buf[row:row + 256]                          # rows 1 and 2 would start at 64 and 128 with offsets taken mod 2^31 floats
    for x in heads + [guard]:
        x.fill_(SENT)
    rc = L.lf_ibr_reproject_fwd(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), None, rec.pair.data_ptr(),
                                rec.view_in.data_ptr(), rec.view_out.data_ptr(), buf.data_ptr(), buf[C * H * W:].data_ptr(),
                                B, n_out, n_in, C, H, W, stride, stride, None)
    torch.cuda.synchronize()
    assert rc == 0
    for i in range(n_in):
        assert torch.equal(heads[i][:C * H * W].view(C, H, W), image_re[0, 0, i]), i
        assert torch.equal(heads[i][C * H * W:].view(1, H, W), depth_re[0, 0, i]), i
    assert (guard == SENT).all()


def test_forward_and_depth_out_gradient_are_run_to_run_identical():
    cs = K.case(*MAIN)
    runs = [_fused(cs) for _ in range(3)]
    for r in runs[1:]:
        for k in ('image_re', 'depth_re', 'g_depth_out'):
            assert torch.equal(r[k], runs[0][k]), k


# ---------------------------------------------------------------------------------------------------------------------
# non-finite inputs
# ---------------------------------------------------------------------------------------------------------------------
def test_non_finite_depths_follow_the_composed_path():
    """NaN / +inf / -inf at a few pixels of depth_out and NaN at a few pixels of depth_in: the fused output has the
    non-finite and the zero pattern of the composed path run on the device; everything else stays within the bound."""
    from latentfusion_amd import ibr, ops
    cs = K.case(*MAIN)
    t, rec = _device(cs)
    B, n_in, n_out, C, H, W = cs['dims']
    image_in, depth_in, depth_out = (x.clone() for x in t)
    depth_out[0, 0, 0, 3, 4], depth_out[0, 1, 0, 10, 20], depth_out[1, 0, 0, 17, 9] = float('nan'), float('inf'), float('-inf')
    depth_out[1, 1, 0, 23, 31], depth_out[1, 1, 0, 0, 0] = float('nan'), float('inf')
    depth_in[0, 0, 0, 12, 16], depth_in[0, 2, 0, 6, 25], depth_in[1, 1, 0, 18, 7] = float('nan'), float('nan'), float('nan')
    image_re, depth_re = ops.ibr_reproject(image_in, depth_in, depth_out, rec)
    ci, co = K.cast_camera(cs['cam_in'], torch.float32, DEV), K.cast_camera(cs['cam_out'], torch.float32, DEV)
    comp = [ibr.reproject_views(image_in[b], depth_in[b], depth_out[b], K.slice_cameras(ci, b, n_in), K.slice_cameras(co, b, n_out),
                                kernel='composed') for b in range(B)]
    for got, want, k in ((image_re, torch.stack([c[0] for c in comp]), 'image_re'),
                         (depth_re, torch.stack([c[1] for c in comp]), 'depth_re')):
        print(k, 'NaN', got.isnan().sum().item(), want.isnan().sum().item(), 'inf', got.isinf().sum().item(),
              want.isinf().sum().item(), 'zero', (got == 0).sum().item(), (want == 0).sum().item())
        assert want.isnan().any()
        assert torch.equal(got.isnan(), want.isnan()), k
        assert torch.equal(got.isinf(), want.isinf()), k
        assert torch.equal(got == 0, want == 0), k
        fin = got.isfinite().cpu()
        err = (got.double().cpu() - cs['ref'][k]).abs()
        ex = (err - torch.maximum(4 * cs['e32'][k], 2e-6 + 2e-5 * cs['ref'][k].abs()))[fin].max().item()
        print(k, 'finite elements: excess', ex)
        assert ex <= 0


# ---------------------------------------------------------------------------------------------------------------------
# ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_abi_rejects_bad_arguments_and_launches_nothing():
    from latentfusion_amd import _lib
    L = _lib.lib()
    cs = K.case(1, 1, 1, 1, 5, 7)
    t, rec = _device(cs)
    B, n_in, n_out, C, H, W = cs['dims']
    SENT = 777.0
    image_re = torch.full((B, n_out, n_in, C, H, W), SENT, device=DEV)
    depth_re = torch.full((B, n_out, n_in, 1, H, W), SENT, device=DEV)
    grads = [torch.full_like(x, SENT) for x in t]
    gi, gd = torch.ones_like(image_re), torch.ones_like(depth_re)
    ptrs = [t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), None, rec.pair.data_ptr(), rec.view_in.data_ptr(),
            rec.view_out.data_ptr()]
    sizes = [B, n_out, n_in, C, H, W]

    def fwd(p=ptrs, outs=None, s=sizes, strides=(C * H * W, H * W)):
        outs = (image_re.data_ptr(), depth_re.data_ptr()) if outs is None else outs
        return L.lf_ibr_reproject_fwd(*p, *outs, *s, *strides, None)

    def bwd(p=ptrs, g=None, s=sizes):
        g = (gi.data_ptr(), gd.data_ptr()) if g is None else g
        return L.lf_ibr_reproject_bwd(*p, *g, *[x.data_ptr() for x in grads], *s, None)

    codes = []
    for k in (0, 1, 2, 4, 5, 6):                                                     # (mask_out, index 3, may be NULL)
        bad = list(ptrs)
        bad[k] = None
        codes += [fwd(p=bad), bwd(p=bad)]
    codes += [fwd(outs=(None, depth_re.data_ptr())), fwd(outs=(image_re.data_ptr(), None)), bwd(g=(None, None))]
    for k in range(6):
        for v in (0, -1):
            bad = list(sizes)
            bad[k] = v
            codes += [fwd(s=bad), bwd(s=bad)]
    codes += [fwd(strides=(C * H * W - 1, H * W)), fwd(strides=(C * H * W, H * W - 1)), fwd(strides=(0, 0))]
    torch.cuda.synchronize()
    assert codes and all(c == -1 for c in codes), codes                               # LF_EINVAL
    for x in [image_re, depth_re] + grads:
        assert (x == SENT).all()
    assert fwd() == 0 and bwd(g=(gi.data_ptr(), None)) == 0
    torch.cuda.synchronize()
    assert not (image_re == SENT).any() and not (depth_re == SENT).any()
    with pytest.raises(ValueError):
        from latentfusion_amd import ops
        ops.ibr_reproject(t[0], t[1], t[2][:, :, :, :-1], rec)


# ---------------------------------------------------------------------------------------------------------------------
# the switch and the fixtures with kernel='fused'
# ---------------------------------------------------------------------------------------------------------------------
def close(a, b, atol=1e-4, rtol=1e-3):
    torch.testing.assert_close(a.detach().cpu().contiguous(), b.detach().cpu().contiguous(), atol=atol, rtol=rtol)


def prod_camera(d, device=DEV):
    from latentfusion_amd.modules.geometry import Camera
    return Camera(d['K'].to(device), None, d['z_span'], d['viewport'].to(device), width=d['width'],
                  height=d['height'], log_quaternion=d['log_q'].to(device), translation=d['t'].to(device))


def _launches(fn):
    """{entry point: launches} of liblf_hip.so while fn() runs (counted by _lib.check, as tests/test_rows_gemm_gpu.py does)."""
    from latentfusion_amd import _lib
    _lib.BYTE_LOG = {}
    try:
        out = fn()
        return out, {k: v[0] for k, v in _lib.BYTE_LOG.items()}
    finally:
        _lib.BYTE_LOG = None


def _parent_reproject_views(image_in, depth_in, depth_out, camera_in, camera_out):
    """The composition reproject_views was before it had a `kernel` argument, from the module's own pieces."""
    from latentfusion_amd import ibr, image_ops, three
    from latentfusion_amd.three.batchview import b2bv, bv2b
    grid = bv2b(ibr.depth_to_warp_field(camera_in, camera_out, depth_out))
    v_i, v_o = len(camera_in), len(camera_out)
    image = bv2b(image_in.unsqueeze(0).expand(v_o, -1, -1, -1, -1))
    obj = bv2b(ibr.depth_object_coords(camera_in, depth_in).unsqueeze(0).expand(v_o, -1, -1, -1, -1))
    cam_rep = camera_out.repeat_interleave(v_i)
    depth_tf = cam_rep.normalize_depth(three.transform_coord_grid(obj, cam_rep.obj_to_cam)[..., 2].unsqueeze(1))
    return (b2bv(image_ops._sample(image, grid, 'bilinear', 'zeros'), v_i),
            b2bv(image_ops._sample(depth_tf, grid, 'bilinear', 'zeros'), v_i))


def test_g9_ibr_fused(golden):
    """g9 (render_latent_ibr2, reproject_views) with kernel='fused', the tolerances of test_g9_ibr_on_hip; with KERNEL at its
    default the outputs are those of the parent's composition bit for bit (the switch is idle)."""
    from latentfusion_amd import ibr
    from latentfusion_amd.recon.models import Photographer
    g = golden('g9_ibr')
    ph = Photographer.from_checkpoint(g['ck']).to(DEV)
    cam_in, cam_out = prod_camera(g['cam_in']), prod_camera(g['cam_out'])
    y, z = ibr.render_latent_ibr2(ph, g['z_obj'].to(DEV), cam_in, cam_out, g['image_in'].to(DEV), p=0.5,
                                  weight_type='cam_dist', apply_mask=True, kernel='fused')
    close(y['depth'], g['depth'], atol=2e-4, rtol=2e-3)
    close(y['color'], g['color'], atol=2e-3, rtol=1e-2)
    with torch.no_grad():
        y_in, _, _ = ph.decode(g['z_obj'].to(DEV), cam_in, apply_mask=True)
        y_out, _, _ = ph.decode(g['z_obj'].to(DEV), cam_out, apply_mask=True)
        args = (g['image_in'][0].to(DEV), y_in['depth'][0], y_out['depth'][0], cam_in, cam_out)
        (img_re, dep_re), counts = _launches(lambda: ibr.reproject_views(*args, kernel='fused'))
        assert counts == {'lf_ibr_reproject_fwd': 1}, counts
        close(img_re, g['image_reproj'], atol=2e-3, rtol=1e-2)
        assert ibr.KERNEL == 'composed'
        default, counts = _launches(lambda: ibr.reproject_views(*args))
        assert counts == {'lf_grid_sample2d_fwd': 2}, counts
        parent = _parent_reproject_views(*args)
        for a, b, c in zip(default, parent, ibr.reproject_views(*args, kernel='composed')):
            assert torch.equal(a, b) and torch.equal(a, c)
        close(dep_re, default[1], atol=2e-3, rtol=1e-2)


def _g23_model(golden, ibr_kernel):
    from latentfusion_amd.modules.unet import UNet2d
    from latentfusion_amd.observation import Observation
    from latentfusion_amd.recon import fusion
    from latentfusion_amd.recon.inference import LatentFusionModel
    from latentfusion_amd.recon.models import Photographer, Sculptor
    g = golden('g23_ibr_generator')
    e = golden('g10_encode_pool_mean')
    model = LatentFusionModel(Sculptor.from_checkpoint(e['sculptor']), fusion.from_checkpoint(e['fuser']),
                              Photographer.from_checkpoint(g['photographer']), g['camera_dist'], DEV,
                              generator=UNet2d.from_checkpoint(g['generator']), ibr_kernel=ibr_kernel)
    obs = Observation(g['color_in'], g['depth_in'], g['mask_in'], prod_camera(g['cam_in'], 'cpu'), is_zoomed=True,
                      is_prepared=True, is_normalized=True).to(DEV)
    return g, model, obs


def test_g23_ibr_generator_fused(golden):
    """g23 (render_ibr with the generator, _render_reprojections, reproject_views_batch, render_latent_ibr) with
    ibr_kernel / kernel = 'fused', the tolerances of test_g23_ibr_generator_on_hip; one reprojection launch per call and no
    lf_grid_sample2d_fwd for it (render_ibr keeps the one of warp_blend_logits)."""
    from latentfusion_amd import ibr
    g, model, obs = _g23_model(golden, 'fused')
    cam_in, cam_out = prod_camera(g['cam_in']), prod_camera(g['cam_out'])
    z_obj = g['z_obj'].to(DEV)
    with torch.no_grad():
        (y, z_out), n_ibr = _launches(lambda: model.render_ibr(z_obj, obs, cam_out))
        rp, n_rp = _launches(lambda: model._render_reprojections(z_obj, obs.color, cam_in, cam_out))
        _, _, img_re, dep_re, _, _, dist_r, dist_t = rp
        lat, n_lat = _launches(lambda: ibr.render_latent_ibr(model.photographer, z_obj, cam_in, cam_out, obs.color.unsqueeze(0),
                                                             p=0.5, kernel='fused'))
        col, d_out, m_out, reproj = lat
    assert n_ibr.get('lf_ibr_reproject_fwd') == 1 and n_ibr.get('lf_grid_sample2d_fwd') == 1, n_ibr
    assert n_rp.get('lf_ibr_reproject_fwd') == 1 and 'lf_grid_sample2d_fwd' not in n_rp, n_rp
    assert n_lat.get('lf_ibr_reproject_fwd') == 1 and 'lf_grid_sample2d_fwd' not in n_lat, n_lat
    for k in ('depth', 'mask', 'depth_logits', 'mask_logits'):
        close(y[k], g['y'][k], atol=2e-4, rtol=2e-3)
    close(img_re, g['image_reproj'], atol=2e-3, rtol=1e-2)
    close(dep_re, g['depth_reproj'], atol=2e-3, rtol=1e-2)
    close(dist_r, g['cam_dist_r'], atol=1e-5, rtol=1e-4)
    close(dist_t, g['cam_dist_t'], atol=1e-5, rtol=1e-4)
    close(y['color'], g['y']['color'], atol=3e-3, rtol=1e-2)
    close(z_out, g['z_out'], atol=3e-4, rtol=3e-3)
    close(col, g['latent_ibr']['color'], atol=2e-3, rtol=1e-2)
    close(d_out, g['latent_ibr']['depth'], atol=2e-4, rtol=2e-3)
    close(reproj, g['latent_ibr']['reproj'], atol=2e-3, rtol=1e-2)


def test_g23_switch_is_idle_and_fused_backpropagates_to_the_latent(golden):
    """ibr_kernel=None (KERNEL at its default) gives the explicit 'composed' outputs bit for bit; render_latent_ibr with
    kernel='fused' back-propagates to z_obj and agrees with the composed path's gradient within 2e-3 of its largest
    component (the gradient bound; there is no fp64 evaluation of the renderer to take an e32 from)."""
    from latentfusion_amd import ibr
    g, model, obs = _g23_model(golden, None)
    _, explicit, _ = _g23_model(golden, 'composed')
    cam_in, cam_out = prod_camera(g['cam_in']), prod_camera(g['cam_out'])
    z_obj = g['z_obj'].to(DEV)
    assert ibr.KERNEL == 'composed'
    with torch.no_grad():
        (ya, za), counts = _launches(lambda: model.render_ibr(z_obj, obs, cam_out))
        yb, zb = explicit.render_ibr(z_obj, obs, cam_out)
    assert 'lf_ibr_reproject_fwd' not in counts and counts.get('lf_grid_sample2d_fwd') == 3, counts
    assert torch.equal(za, zb) and all(torch.equal(ya[k], yb[k]) for k in ya)
    grads = {}
    w = torch.randn(g['latent_ibr']['color'].shape, generator=torch.Generator().manual_seed(3)).to(DEV)
    for kernel in ('composed', 'fused'):
        z = z_obj.clone().requires_grad_(True)
        col, _, _, _ = ibr.render_latent_ibr(model.photographer, z, cam_in, cam_out, obs.color.unsqueeze(0), p=0.5, kernel=kernel)
        (col * w).sum().backward()
        grads[kernel] = z.grad
    top = grads['composed'].abs().max().item()
    err = (grads['fused'] - grads['composed']).abs().max().item()
    print('d colour / d z_obj: largest component', top, 'fused - composed', err)
    assert top > 0 and err <= 2e-3 * top
