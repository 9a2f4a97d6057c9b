"""Host side of the fused IBR reprojection: the camera records of ops.pack_ibr_cameras against the Camera properties in
fp64, the rules of the `kernel` argument of latentfusion_amd.ibr, and the ibr_kernel plumbing of LatentFusionModel."""
import pytest
import torch

import ibr_fused_cases as K
from oracle_util import in_fp64


def _properties_fp64(cam_in, cam_out, b, n_in, n_out):
    """The record entries of object b from the Camera properties (library matmuls), fp64."""
    ci, co = K.slice_cameras(cam_in, b, n_in), K.slice_cameras(cam_out, b, n_out)
    eps = 0.01
    pair = torch.zeros(n_out, n_in, 32, dtype=torch.float64)
    for o in range(n_out):
        for i in range(n_in):
            m = ci.obj_to_image[i] @ co.cam_to_obj[o]                               # output camera -> object -> input image
            vp = ci.viewport[i]
            pair[o, i, 0:4] = (m[0] - vp[0] * m[2]) / ci.viewport_width[i]
            pair[o, i, 4:8] = (m[1] - vp[1] * m[2]) / ci.viewport_height[i]
            pair[o, i, 8:12] = m[2]
            zrow = (co.obj_to_cam[o] @ ci.cam_to_obj[i])[2].clone()                 # input camera -> object -> z of camera o
            zn, zf = co.znear[o] - eps, co.zfar[o] + eps
            zrow[3] -= zn
            pair[o, i, 12:16] = zrow / (zf - zn)

    def view(c, out):
        v = torch.zeros(len(c), 16, dtype=torch.float64)
        v[:, 0], v[:, 1] = c.viewport_width / c.fu, (c.viewport[:, 0] - c.u0) / c.fu
        v[:, 2], v[:, 3] = c.viewport_height / c.fv, (c.viewport[:, 1] - c.v0) / c.fv
        if out:
            zn, zf = c.znear - eps, c.zfar + eps
            v[:, 4], v[:, 5] = (zf - zn) / 2, (zf + zn) / 2
        return v
    return pair, view(ci, False), view(co, True)


def test_pack_ibr_cameras_against_the_camera_properties():
    from latentfusion_amd import _lib, ops
    B, n_in, n_out = 2, 3, 2
    cam_in, cam_out = K.make_cameras(n_in, n_out, B, torch.float64)
    rec = ops.pack_ibr_cameras(cam_in, cam_out, batch_size=B)
    assert rec.flat.dtype == torch.float32 and rec.flat.dim() == 1
    assert rec.pair.shape == (B, n_out, n_in, _lib.LF_IBR_PAIR_FLOATS) and rec.view_in.shape == (B, n_in, _lib.LF_IBR_VIEW_FLOATS)
    assert rec.view_out.shape == (B, n_out, _lib.LF_IBR_VIEW_FLOATS)
    assert rec.flat.numel() == rec.pair.numel() + rec.view_in.numel() + rec.view_out.numel()
    for b in range(B):
        want = in_fp64(lambda: _properties_fp64(cam_in, cam_out, b, n_in, n_out))
        for got, w, n, at in zip((rec.pair[b], rec.view_in[b], rec.view_out[b]), want, (12, 0, 6), (16, 8, 8)):
            got = got.double()
            # formed in fp64, rounded ONCE: half an ulp of fp32 (the two fp64 evaluations differ by ~1e-16 relative) ...
            assert ((got[..., :at] - w[..., :at]).abs() <= 2.0 ** -24 * w[..., :at].abs() * (1 + 1e-6) + 1e-300).all()
            # ... and the entries of the coordinate chain with the float of the remainder: 2^-48 relative, plus the
            # difference between the two fp64 evaluations (cancellation inside an entry: absolute, against the row's size)
            if not n:
                assert (got[..., 4:] == 0).all()                 # input views: singly rounded, the rest padding
                continue
            two = got[..., :n] + got[..., at:at + n]
            assert ((two - w[..., :n]).abs() <= 2.0 ** -47 * w[..., :n].abs() + 1e-14 * w[..., :n].abs().max()).all()
            assert (got[..., at + n:] == 0).all() and (w[..., at:] == 0).all()
    # a record does not depend on its batch mates or on the other views
    for b in range(B):
        alone = ops.pack_ibr_cameras(K.slice_cameras(cam_in, b, n_in), K.slice_cameras(cam_out, b, n_out))
        assert torch.equal(alone.pair[0], rec.pair[b]) and torch.equal(alone.view_in[0], rec.view_in[b])
        assert torch.equal(alone.view_out[0], rec.view_out[b])
        one = ops.pack_ibr_cameras(K.slice_cameras(cam_in, b, n_in)[2], K.slice_cameras(cam_out, b, n_out)[1])
        assert torch.equal(one.pair[0, 0, 0], rec.pair[b, 1, 2])
    with pytest.raises(ValueError):
        ops.pack_ibr_cameras(cam_in, cam_out, batch_size=4)
    # fp32 cameras are read as they are (no second rounding of the inputs)
    c32i, c32o = K.cast_camera(cam_in, torch.float32), K.cast_camera(cam_out, torch.float32)
    again = ops.pack_ibr_cameras(K.cast_camera(c32i, torch.float64), K.cast_camera(c32o, torch.float64), batch_size=B)
    assert torch.equal(ops.pack_ibr_cameras(c32i, c32o, batch_size=B).flat, again.flat)


def test_record_arithmetic_reproduces_the_composed_path():
    """The arithmetic the header specifies for the records, carried out on the host in fp64 with the fp32 records, stays
    inside the forward bound against the composed code in fp64 -- and the re-statement the wrong references are made from
    IS the composed code."""
    from latentfusion_amd import ops
    cs = K.case(2, 3, 2, 3, 24, 32)
    B, n_in, n_out = cs['dims'][:3]
    rec = ops.pack_ibr_cameras(cs['cam_in'], cs['cam_out'], batch_size=B)
    for b in range(B):
        r = (rec.pair[b].double(), rec.view_in[b].double(), rec.view_out[b].double())
        t = [x[b] for x in cs['tensors']]
        image_re, depth_re = in_fp64(lambda: K.emulate(r, *t))
        for got, k in ((image_re, 'image_re'), (depth_re, 'depth_re')):
            ex, err = K.forward_excess(got, cs['ref'][k][b], cs['e32'][k][b])
            assert ex <= 0, (k, ex, err)
        a, d = in_fp64(lambda: K.restated(*t, K.slice_cameras(cs['cam_in'], b, n_in), K.slice_cameras(cs['cam_out'], b, n_out)))
        assert (a - cs['ref']['image_re'][b]).abs().max() < 1e-11 and (d - cs['ref']['depth_re'][b]).abs().max() < 1e-11
    assert cs['near'].double().mean().item() <= 0.01 and not cs['taps_clamped'].any()


def test_kernel_argument_rules(monkeypatch):
    from latentfusion_amd import ibr
    assert ibr.KERNEL == 'composed'
    cs = K.case(1, 1, 1, 1, 5, 7)
    cam_in, cam_out = K.cast_camera(cs['cam_in'], torch.float32), K.cast_camera(cs['cam_out'], torch.float32)
    image_in, depth_in, depth_out = (x[0].float() for x in cs['tensors'])
    a = ibr.reproject_views(image_in, depth_in, depth_out, cam_in, cam_out)
    b = ibr.reproject_views(image_in, depth_in, depth_out, cam_in, cam_out, kernel='composed')
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for fn, args in ((ibr.reproject_views, (image_in, depth_in, depth_out)),
                     (ibr.reproject_views_batch, (image_in[None], depth_in[None], depth_out[None]))):
        with pytest.raises(ValueError, match='Unknown IBR kernel'):
            fn(*args, cam_in, cam_out, kernel='triton')
        with pytest.raises(ValueError, match='device tensors'):                      # 'fused' on host tensors
            fn(*args, cam_in, cam_out, kernel='fused')
    with pytest.raises(ValueError, match='device tensors'):
        ibr.render_ibr(cam_in, cam_out, image_in[None], depth_in[None], depth_out[None], kernel='fused')
    with pytest.raises(ValueError, match="kernel='fused'"):
        ibr.reproject_views_batch(image_in[None], depth_in[None], depth_out[None], cam_in, cam_out, mask_out=depth_out[None])
    # None reads the module's KERNEL at call time
    monkeypatch.setattr(ibr, 'KERNEL', 'fused')
    with pytest.raises(ValueError, match='device tensors'):
        ibr.reproject_views(image_in, depth_in, depth_out, cam_in, cam_out)
    monkeypatch.setattr(ibr, 'KERNEL', 'composed')
    # a camera that requires grad: the fused kernel has no camera gradient (checked first, so also for host tensors)
    cam_g = cam_out.clone()
    cam_g.translation.requires_grad_(True)

    args = (image_in, depth_in, depth_out)
    with pytest.raises(NotImplementedError, match='constants'):
        ibr.reproject_views(*args, cam_in, cam_g, kernel='fused')
    with pytest.raises(NotImplementedError, match='constants'):
        ibr.reproject_views_batch(*(x[None] for x in args), cam_g, cam_out, kernel='fused')
    with torch.no_grad():                                     # nothing asks for the gradient: only the host tensors are refused
        with pytest.raises(ValueError, match='device tensors'):
            ibr.reproject_views(*args, cam_in, cam_g, kernel='fused')


def test_model_hands_ibr_kernel_down(monkeypatch):
    """LatentFusionModel(ibr_kernel=...) reaches render_latent_ibr2 (render_ibr_basic) and reproject_views_batch
    (_render_reprojections, render_ibr), with the mask and the stacked output on 'fused' only."""
    from latentfusion_amd import ibr
    from latentfusion_amd.recon.inference import LatentFusionModel
    H = W = 4
    calls = []

    class Photographer:
        def decode(self, z_obj, camera, return_latent=False, apply_mask=False):
            n = len(camera)
            y = {'depth': torch.zeros(1, n, 1, H, W), 'mask': torch.ones(1, n, 1, H, W)}
            return y, torch.zeros(1, n, 2), None

    def batch_stub(image_in, depth_in, depth_out, camera_in, camera_out, kernel=None, mask_out=None, out=None):
        calls.append(('batch', kernel, mask_out is not None, out is not None))
        n_out, n_in = depth_out.shape[1], image_in.shape[1]
        if out is not None:
            rows = out.view(1, n_out, n_in, -1, H, W)
            rows.zero_()
            img, dep = rows[:, :, :, :3], rows[:, :, :, 3:4]
        else:
            img, dep = torch.zeros(1, n_out, n_in, 3, H, W), torch.zeros(1, n_out, n_in, 1, H, W)
        return img, dep, torch.zeros(1, n_out, n_in), torch.full((1, n_out, n_in), 0.25)

    def ibr2_stub(photographer, z_obj, camera_in, camera_out, image_in, kernel=None, **kw):
        calls.append(('ibr2', kernel))
        return {'color': torch.zeros(1, len(camera_out), 3, H, W)}, torch.zeros(1, len(camera_out), 2)

    monkeypatch.setattr(ibr, 'reproject_views_batch', batch_stub)
    monkeypatch.setattr(ibr, 'render_latent_ibr2', ibr2_stub)
    cam_in, cam_out = K.make_cameras(3, 2)

    class Obs:
        meta = {'is_zoomed': True, 'is_prepared': True, 'is_normalized': True}
        color = torch.zeros(3, 3, H, W)
        camera = cam_in

    seen = {}

    def generator(x):
        seen['x'] = x
        return torch.zeros(x.shape[0], 9, H, W)

    for kernel in (None, 'composed', 'fused'):
        model = LatentFusionModel.__new__(LatentFusionModel)
        model.photographer, model.generator, model.device, model.ibr_kernel = Photographer(), generator, 'cpu', kernel
        model.camera_dist, model.input_size = 1.0, H
        calls.clear()
        model.render_ibr_basic(None, Obs, cam_out)
        out = model._render_reprojections(None, Obs.color, cam_in, cam_out)
        assert out[2].shape == (2, 3, 3, H, W) and out[3].shape == (2, 3, 1, H, W)
        model.render_ibr(None, Obs, cam_out)
        fused = kernel == 'fused'
        want = 'fused' if fused else 'composed'
        assert calls == [('ibr2', kernel), ('batch', want, fused, False), ('batch', want, fused, fused)], (kernel, calls)
        # the generator's input: (V_o, 1 + V_i * (C + 2), H, W), the similarity plane 1 - 2 * 0.25 after every view's depth
        x = seen['x']
        assert x.shape == (2, 1 + 3 * 5, H, W)
        assert (x[:, 1:].reshape(2, 3, 5, H, W)[:, :, 4] == 0.5).all() and (x[:, 1:].reshape(2, 3, 5, H, W)[:, :, :4] == 0).all()
    assert 'ibr_kernel' in LatentFusionModel.__init__.__code__.co_varnames
    assert 'ibr_kernel' in LatentFusionModel.from_checkpoint.__func__.__code__.co_varnames
