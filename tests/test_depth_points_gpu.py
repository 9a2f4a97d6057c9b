"""lf_depth_points (csrc/depth_points.hip, ops.depth_points, Observation.pointcloud(kernel='fused')) on the cases of
tests/eval_cloud_cases.py: `index` and `counts` torch.equal to the composed path on CPU copies (tests/test_eval_cloud_cases.py
proves that the cases keep exactly their own-pixel mask, far from every truncation boundary), `points` against the fp64
restatement of the contract within the project's bound max(4 e32, 2e-6 + 2e-5 |fp64|), e32 the composed CPU path's own error at
the same element; colours are copies and compared exactly.

Every call of the entry point goes through `_run`, which hands it NaN-poisoned outputs and scratch with sentinels behind each
of them, checks the sentinels and that no row past sum(counts) was written."""
import pytest
import torch

import eval_cloud_cases as K

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SENT, ISENT, GUARD = -777.25, -424242, 64
LF_EINVAL, LF_EALIGN, LF_ENOSPC = -1, -2, -3
CASES = [(h, w, b) for (h, w) in K.OBS_FRAMES for b in K.OBS_BATCHES]


def _L():
    from latentfusion_amd import _lib
    return _lib.lib()


def _s():
    return torch.cuda.current_stream().cuda_stream


def _guarded(n, dtype):
    """n elements (all bytes 0xff: NaN / -1) followed by GUARD sentinels -> (whole buffer, view of the n elements)."""
    buf = torch.empty(n + GUARD, device=DEV, dtype=dtype)
    buf.view(torch.uint8)[:n * buf.element_size()] = 0xff
    buf[n:] = SENT if dtype.is_floating_point else ISENT
    return buf, buf[:n]


def _intact(buf, n):
    return bool((buf[n:] == (SENT if buf.dtype.is_floating_point else ISENT)).all())


def _untouched(view):
    return bool((view.contiguous().view(torch.uint8) == 0xff).all())


def _records(camera):
    from latentfusion_amd import ops
    return ops.pack_depth_cameras(camera)


def _call(depth, mask, color, cams, to_object=1, segment=1, want_index=True, frame_wh=None, over=None):
    """One call of the entry point on CPU inputs (depth (B,H,W), mask (B,H,W) fp32 / uint8 / bool or None, color (B,3,H,W) or
    None, cams (B,32)).  over: a function that edits the argument list (the ABI-error cases).
    -> (rc, dict of the guarded output views, whether every sentinel is intact)."""
    L = _L()
    B, H, W = depth.shape
    cap = B * H * W
    d = depth.to(DEV).contiguous()
    mk = None
    u8 = 0
    if mask is not None:
        mk = mask.to(DEV).contiguous()
        u8 = int(mk.dtype != torch.float32)
        mk = mk.view(torch.uint8) if mk.dtype == torch.bool else mk
    col = color.to(DEV).contiguous() if color is not None else None
    cm = cams.to(DEV).contiguous()
    pb, points = _guarded(cap * 3, torch.float32)
    cb, colors = _guarded(cap * 3, torch.float32)
    ib, index = _guarded(cap, torch.int32)
    nb, counts = _guarded(B, torch.int32)
    nbytes = L.lf_depth_points_scratch_bytes(B, H, W)
    assert nbytes == B * ((H * W + 1023) // 1024) * 4
    xb, _ = _guarded(nbytes // 4, torch.int32)
    fw, fh = frame_wh if frame_wh is not None else (W, H)
    args = [d.data_ptr(), mk.data_ptr() if mk is not None else None, u8, col.data_ptr() if col is not None else None, cm.data_ptr(),
            points.data_ptr(), colors.data_ptr() if col is not None else None, index.data_ptr() if want_index else None,
            counts.data_ptr(), xb.data_ptr(), nbytes, B, H, W, fw, fh, to_object, segment, _s()]
    if over is not None:
        over(args)
    rc = L.lf_depth_points(*args)
    torch.cuda.synchronize()
    ok = _intact(pb, cap * 3) and _intact(cb, cap * 3) and _intact(ib, cap) and _intact(nb, B) and _intact(xb, nbytes // 4)
    return rc, dict(points=points.view(cap, 3), colors=colors.view(cap, 3), index=index, counts=counts), ok


def _run(obs, frame='object', segment=True, mask=None, color=True, want_index=True, cams=None):
    """lf_depth_points on a CPU observation -> dict(points (n,3), colors (n,3) or None, index (n,) or None, counts (B,)) on the
    CPU.  mask: another (B,H,W) tensor than the observation's (any of the three storages)."""
    B, _, H, W = obs.depth.shape
    mk = (obs.mask[:, 0] if mask is None else mask) if segment else None
    rc, out, ok = _call(obs.depth[:, 0], mk, obs.color if color else None, _records(obs.camera) if cams is None else cams,
                        to_object=int(frame == 'object'), segment=int(segment), want_index=want_index)
    assert rc == 0, rc
    assert ok
    counts = out['counts'].cpu()
    n = int(counts.sum())
    assert _untouched(out['points'][n:]) and _untouched(out['index'][n if want_index else 0:])
    assert _untouched(out['colors'][n if color else 0:])
    return dict(points=out['points'][:n].cpu(), colors=out['colors'][:n].cpu() if color else None,
                index=out['index'][:n].cpu() if want_index else None, counts=counts)


def _against_fp64(obs, got, frame, segment):
    """index / counts equal to the composed path, points within the bound, colours equal.  -> (worst excess, largest error)."""
    points, colors, index, counts = K.composed(obs, frame=frame, segment=segment)
    assert torch.equal(got['counts'], counts), (got['counts'], counts)
    assert torch.equal(got['index'], index)
    r = K.restate64(obs, frame=frame)
    flat = index.long()
    ref = r['points'].reshape(-1, 3)[flat]
    e32 = (points.double() - ref).abs()
    ex, err = K.excess(got['points'], ref, e32)
    print(f'depth_points {tuple(obs.depth.shape)} {frame} segment={segment}: max |err| {err:.3e}, composed e32 max '
          f'{float(e32.max()) if e32.numel() else 0.0:.3e}, worst excess over the bound {ex:.3e}')
    assert ex <= 0.0, (ex, err)
    if got['colors'] is not None:
        assert torch.equal(got['colors'], colors)
    return ex, err


@pytest.mark.parametrize('H,W,B', CASES)
def test_cases_against_the_composed_path_and_fp64(H, W, B):
    obs = K.obs_case(H, W, B)
    _against_fp64(obs, _run(obs), 'object', True)


@pytest.mark.parametrize('H,W,B', [(2, 2, 3), (33, 65, 3), (97, 131, 1)])
@pytest.mark.parametrize('frame', ['object', 'camera'])
def test_segment_0_writes_every_row_in_order(H, W, B, frame):
    obs = K.obs_case(H, W, B)
    got = _run(obs, frame=frame, segment=False)
    assert torch.equal(got['index'], torch.arange(B * H * W, dtype=torch.int32))
    assert got['counts'].tolist() == [H * W] * B
    _against_fp64(obs, got, frame, False)
    lean = _run(obs, frame=frame, segment=False, color=False, want_index=False)
    assert torch.equal(lean['points'], got['points'])


@pytest.mark.parametrize('H,W,B', [(5, 7, 3), (97, 131, 3)])
def test_camera_frame_with_segment_projects_with_obj_to_image_all_the_same(H, W, B):
    """The reference's quirk: the camera-frame points go through obj_to_image.  Their re-projections fall anywhere, so the kept
    set is compared with the composed path's where the fp64 re-projection is at least 1e-3 px from an integer on both axes
    (fp32 error of the quotient: a few 1e-4 px at these sizes); nearer than that either decision is a rounding."""
    obs = K.obs_case(H, W, B)
    got = _run(obs, frame='camera')
    r = K.restate64(obs, frame='camera')
    safe = (K.pix_margin(r['pix']) >= 1e-3).reshape(-1)
    keep = K.keep64(obs, r['pix']).reshape(-1)
    mine = torch.zeros(B * H * W, dtype=torch.bool)
    mine[got['index'].long()] = True
    assert torch.equal(mine[safe], keep[safe]) and int(safe.sum()) > 0.9 * safe.numel()
    wrong = K.keep64(obs, K.restate64(obs, frame='camera', project='intrinsic')['pix']).reshape(-1)
    assert not torch.equal(mine[safe], wrong[safe])
    ref = r['points'].reshape(-1, 3)[got['index'].long()]
    host = torch.stack(obs.camera.depth_camera_coords(obs.depth), dim=-1).reshape(-1, 3)[got['index'].long()]
    assert K.excess(got['points'], ref, (host.double() - ref).abs())[0] <= 0.0


def test_zero_depth_pixels_are_never_kept():
    obs = K.make_observation(33, 65, 3, seed=5)
    fg = obs.mask[:, 0] != 0
    zero = fg & (torch.rand(fg.shape, generator=torch.Generator().manual_seed(9)) < 0.5)
    assert 0 < int(zero.sum()) < int(fg.sum())
    obs.depth[:, 0][zero] = 0.0
    got = _run(obs)
    hit = torch.zeros(fg.numel(), dtype=torch.bool)
    hit[got['index'].long()] = True
    assert not bool(hit[zero.reshape(-1)].any())
    assert torch.equal(hit, (fg & ~zero).reshape(-1))
    cleared = _run(obs, mask=(fg & ~zero).float())                  # the same call with those pixels' mask cleared
    for k in ('points', 'colors', 'index', 'counts'):
        assert torch.equal(got[k], cleared[k]), k


@pytest.mark.parametrize('H,W,B', [(5, 7, 1), (97, 131, 3)])
def test_mask_storage(H, W, B):
    obs = K.obs_case(H, W, B)
    a = _run(obs)
    scaled = obs.mask[:, 0] * -3.5                                   # any non-zero value is foreground
    for mask in (obs.mask[:, 0].to(torch.uint8), obs.mask[:, 0].bool(), scaled, (obs.mask[:, 0] * 200).to(torch.uint8)):
        b = _run(obs, mask=mask)
        for k in ('points', 'colors', 'index', 'counts'):
            assert torch.equal(a[k], b[k]), (k, mask.dtype)


def test_views_do_not_depend_on_their_batch_and_runs_repeat():
    obs = K.obs_case(97, 131, 3)
    whole = _run(obs)
    again = _run(obs)
    for k in ('points', 'colors', 'index', 'counts'):
        assert torch.equal(whole[k], again[k]), k
    at = 0
    for b in range(3):
        alone = _run(obs[b])
        n = int(whole['counts'][b])
        assert alone['counts'].tolist() == [n]
        assert torch.equal(alone['points'], whole['points'][at:at + n])
        assert torch.equal(alone['colors'], whole['colors'][at:at + n])
        assert torch.equal(alone['index'] + b * 97 * 131, whole['index'][at:at + n])
        at += n


def _centred(H, W, B, seed):
    """An observation whose lattice samples the pixel centres (viewport (0.5, 0.5, W - 0.5, H - 0.5)): every pixel, the last row
    and column too, re-projects half a pixel from every integer, so any mask is kept exactly."""
    return K.make_observation(H, W, B, seed=seed, viewport=(0.5, 0.5, W - 0.5, H - 0.5))


def test_compaction_with_empty_single_and_full_chunks():
    H, W = 97, 131
    obs = _centred(H, W, 4, seed=2)
    obs.mask[0] = 1.0                                                # every chunk full (the last one of the view: partly filled)
    obs.mask[1] = 0.0                                                # every chunk empty
    obs.mask[2] = 0.0
    obs.mask[2, 0, 40, 17] = 1.0                                     # one chunk holds one pixel
    obs.mask[2, 0, H - 1, W - 1] = 1.0                               # and the view's last pixel
    got = _run(obs)                                                  # view 3: the random 40 %
    assert got['counts'].tolist() == [H * W, 0, 2, int(obs.mask[3].sum())]
    assert got['index'][:H * W].tolist() == list(range(H * W))
    assert got['index'][H * W:H * W + 2].tolist() == [2 * H * W + 40 * W + 17, 3 * H * W - 1]
    _against_fp64(obs, got, 'object', True)


def test_wrong_restatements_are_rejected():
    H, W, B = 33, 65, 3
    obs = K.obs_case(H, W, B)
    got = _run(obs)
    own = K.own_pixel_keep(obs).reshape(B, H, W)
    assert torch.equal(got['index'].long(), torch.nonzero(own.reshape(-1))[:, 0])
    shifted = torch.roll(own, 1, dims=2)                             # the mask of the pixel to the left
    assert not torch.equal(got['index'].long(), torch.nonzero(shifted.reshape(-1))[:, 0])
    pixel_major = torch.nonzero(own.reshape(B, -1).t().reshape(-1))[:, 0]        # (pixel, view) order
    pixel_major = (pixel_major % B) * H * W + pixel_major // B
    assert sorted(pixel_major.tolist()) == got['index'].tolist() and not torch.equal(pixel_major, got['index'].long())
    # floor instead of trunc: a viewport that starts at -0.5 puts row 0 and column 0 at -0.5, which truncation reads at pixel 0
    # and floor would drop; every sample is half a pixel from the integers
    low = K.make_observation(H, W, B, seed=3, viewport=(-0.5, -0.5, W - 1.5, H - 1.5))
    low.mask[:] = (torch.rand(B, 1, H, W, generator=torch.Generator().manual_seed(4)) < 0.5).float()
    g = _run(low)
    _against_fp64(low, g, 'object', True)
    pix = K.restate64(low)['pix']
    floor_keep = (pix[..., 0] >= 0) & (pix[..., 1] >= 0) & K.keep64(low, pix)
    mine = torch.zeros(B * H * W, dtype=torch.bool)
    mine[g['index'].long()] = True
    assert not torch.equal(mine, floor_keep.reshape(-1)) and bool(mine.reshape(B, H, W)[:, 0, :].any())


def test_abi_errors_leave_the_outputs_intact():
    obs = K.obs_case(5, 7, 3)
    depth, mask, cams = obs.depth[:, 0], obs.mask[:, 0], _records(obs.camera)

    def bad(expect, segment=1, mask_arg=mask, frame_wh=None, **edits):
        def over(args):
            for pos, fn in edits.items():
                args[int(pos[1:])] = fn(args[int(pos[1:])])
        rc, out, ok = _call(depth, mask_arg, obs.color, cams, segment=segment, frame_wh=frame_wh, over=over)
        assert rc == expect, (rc, expect, edits)
        assert ok and all(_untouched(v) for v in out.values()), edits

    bad(LF_EINVAL, a0=lambda p: None)                                # depth
    bad(LF_EINVAL, a4=lambda p: None)                                # cams
    bad(LF_EINVAL, a5=lambda p: None)                                # points
    bad(LF_EINVAL, a8=lambda p: None)                                # counts
    bad(LF_EINVAL, a1=lambda p: None)                                # segment without a mask
    bad(LF_EINVAL, a6=lambda p: None)                                # color without colors
    bad(LF_EINVAL, a3=lambda p: None)                                # colors without color
    bad(LF_EINVAL, a11=lambda v: 0)                                  # B
    bad(LF_EINVAL, a12=lambda v: -1)                                 # H
    bad(LF_EINVAL, a2=lambda v: 2)                                   # mask_u8
    bad(LF_EINVAL, a16=lambda v: 2)                                  # to_object
    bad(LF_EINVAL, a17=lambda v: -1)                                 # segment
    bad(LF_EINVAL, frame_wh=(8, 5))                                  # the frame is not the mask's size
    bad(LF_EINVAL, frame_wh=(7, 6))
    bad(LF_EINVAL, a12=lambda v: 1 << 16, a13=lambda v: 1 << 15)     # B * H * W = 3 * 2^31
    bad(LF_EALIGN, a0=lambda p: p + 2)
    bad(LF_EALIGN, a5=lambda p: p + 1)
    bad(LF_EALIGN, a7=lambda p: p + 2)
    bad(LF_EALIGN, a9=lambda p: p + 2)
    bad(LF_ENOSPC, a10=lambda v: v - 1)
    bad(LF_ENOSPC, a9=lambda p: None)
    assert _L().lf_depth_points_scratch_bytes(3, 1 << 16, 1 << 15) == 0


def test_python_wrappers():
    from latentfusion_amd import ops
    obs = K.obs_case(33, 65, 3)
    dev = obs.to(DEV)
    host = K.composed(obs)
    out = ops.depth_points(dev.depth, dev.mask, dev.camera, color=dev.color, want_index=True)
    n = int(out['counts'].sum())
    assert out['points'].shape == (3 * 33 * 65, 3) and torch.equal(out['index'][:n].cpu(), host[2])
    assert torch.equal(out['counts'].cpu(), host[3]) and torch.equal(out['colors'][:n].cpu(), host[1])
    rec = ops.pack_depth_cameras(obs.camera).to(DEV)                 # prepacked records, a bool mask, (B,H,W) shapes
    out2 = ops.depth_points(dev.depth[:, 0], dev.mask[:, 0].bool(), rec)
    assert sorted(out2) == ['counts', 'points'] and torch.equal(out2['points'][:n], out['points'][:n])
    points, colors = dev.pointcloud(return_colors=True, kernel='fused')
    assert points.is_cuda and torch.equal(points, out['points'][:n]) and torch.equal(colors, out['colors'][:n])
    assert torch.equal(dev.pointcloud(kernel='fused'), points)
    cam_pts = dev.pointcloud(frame='camera', segment=False, kernel='fused')
    assert cam_pts.shape == (3 * 33 * 65, 3)
    from latentfusion_amd import observation
    assert observation.KERNEL == 'composed'
    assert float((dev.pointcloud().cpu() - host[0]).abs().max()) < 1e-5          # the default stays the composed path
    with pytest.raises(ValueError, match='device tensors'):
        obs.pointcloud(kernel='fused')
    with pytest.raises(ValueError, match='differ in shape'):
        ops.depth_points(dev.depth, dev.mask[:, :, :-1], dev.camera)
    with pytest.raises(ValueError, match='needs a mask'):
        ops.depth_points(dev.depth, None, dev.camera)
    with pytest.raises(ValueError, match='camera holds'):
        ops.depth_points(dev.depth, dev.mask, dev.camera[:2])
    with pytest.raises(ValueError, match='color must be'):
        ops.depth_points(dev.depth, dev.mask, dev.camera, color=dev.color[:, :2])
    small = obs.camera._like()
    small.width = 64
    with pytest.raises(ValueError, match='must be equal'):
        ops.depth_points(dev.depth, dev.mask, small)
