"""tests/eval_cloud_cases.py checked without a GPU: the FPS clouds satisfy the condition under which the kernel may be compared
with the composed path, the observation cases keep exactly their own-pixel mask, the composed Observation.pointcloud agrees
with the fp64 restatement of the contract, and the wrappers' argument rules hold before any library call."""
import pytest
import torch
import torch.nn.functional as F

import eval_cloud_cases as K


# ---- farthest-point sampling ---------------------------------------------------------------------------------------------------
def test_fps_clouds_meet_the_condition_and_the_two_large_ones_do_not():
    """Measured (minimum pick gap, owner near-tie share) of the six clouds, in the order of FPS_SIZES: printed below."""
    rows = []
    for i, (x, k) in enumerate(K.fps_clouds()):
        gap, share, _ = K.fps_gaps64(x, k)
        rows.append((tuple(x.shape), k, gap, share))
        print(f'fps cloud {tuple(x.shape)} K={k}: min pick gap {gap:.3e}, owner near-tie share {share:.3e}')
        if i < K.FPS_CONDITIONED:
            assert gap >= K.FPS_MARGIN and share == 0.0, rows[-1]
        else:
            assert gap < K.FPS_MARGIN or share > 0.0, rows[-1]


@pytest.mark.parametrize('i', range(K.FPS_CONDITIONED))
def test_fps_restatement_equals_the_composed_path_on_the_conditioned_clouds(i):
    x, k = K.fps_clouds()[i]
    centers, owner, nearest = K.fps_expected(i)
    c_centers, c_owner, c_nearest = K.fps_composed(x, k)
    assert c_centers.dtype == torch.long and c_owner.dtype == torch.long
    assert torch.equal(centers.long(), c_centers) and int(centers[0]) == 0
    assert torch.equal(owner.long(), c_owner)
    assert float((nearest - c_nearest).abs().max()) <= 4e-6


def test_fps_restatement_ties_and_wrong_readings():
    # duplicated points and a lattice: maxima and minima tie exactly
    for x, k in K.fps_tie_clouds():
        centers, owner, nearest = K.fps_restate(x, k)
        assert centers[0] == 0
        wrong_c = K.fps_restate(x, k, tie='largest')[0]
        wrong_o = K.fps_restate(x, k, owner_rule='first')[1]
        assert not torch.equal(wrong_c, centers) and not torch.equal(wrong_o, owner)
    dup, k = K.fps_tie_clouds()[0]
    centers, owner, nearest = K.fps_restate(dup, k)
    assert torch.equal(owner[:20], owner[20:40])                    # a duplicate belongs to its twin's centre
    # after the 20 distinct rows every running minimum is 0: the maxima tie everywhere, row 0 is picked again and takes its
    # twins over as the LAST centre at distance 0
    assert centers[20:].tolist() == [0] * (k - 20) and owner[0] == k - 1 and owner[40] == k - 1 and not bool(nearest.any())


def test_rounded_sqrt_is_the_correctly_rounded_root():
    import numpy as np
    v = torch.cat((torch.rand(50000, generator=torch.Generator().manual_seed(1)) * 64, K.fps_expected(3)[2] ** 2, torch.zeros(3)))
    assert torch.equal(K.rounded_sqrt(v), torch.from_numpy(np.sqrt(v.numpy())))
    exact = torch.sqrt(v.double())
    r = K.rounded_sqrt(v)
    up, down = torch.nextafter(r, torch.full_like(r, 1e9)), torch.nextafter(r, torch.full_like(r, -1e9))
    err = (r.double() - exact).abs()
    assert bool((err <= (up.double() - exact).abs()).all()) and bool((err <= (down.double() - exact).abs()).all())


def test_composed_farthest_points_early_return_and_kernel_argument():
    from latentfusion_amd.three.utils import farthest_points
    x = K.fps_clouds()[0][0]
    ids, centers = farthest_points(x, 7, F.pairwise_distance, return_center_indexes=True)
    assert torch.equal(ids, torch.arange(7)) and torch.equal(centers, torch.arange(7))
    assert torch.equal(farthest_points(x, 3, F.pairwise_distance, kernel='composed'), farthest_points(x, 3, F.pairwise_distance))
    with pytest.raises(ValueError, match='Unknown farthest_points kernel'):
        farthest_points(x, 3, F.pairwise_distance, kernel='hip')
    with pytest.raises(ValueError, match='dist_func'):
        farthest_points(x, 3, lambda a, b: (a - b).abs().sum(-1), kernel='fused')


# ---- observations ----------------------------------------------------------------------------------------------------------------
CASES = [(h, w, b) for (h, w) in K.OBS_FRAMES for b in K.OBS_BATCHES]


@pytest.mark.parametrize('H,W,B', CASES)
def test_composed_set_is_the_own_pixel_mask(H, W, B):
    obs = K.obs_case(H, W, B)
    assert bool((obs.depth > 0).all())
    assert not bool(obs.mask[:, :, -1, :].any()) and not bool(obs.mask[:, :, :, -1].any())
    own = K.own_pixel_keep(obs)
    points, colors, index, counts = K.composed(obs)
    assert torch.equal(index.long(), torch.nonzero(own.reshape(-1))[:, 0])
    assert torch.equal(counts, own.sum(dim=1).to(torch.int32))
    r = K.restate64(obs)
    assert torch.equal(K.keep64(obs, r['pix']), own)
    # every kept pixel's re-projection is far from the integers it could flip at (pixel 0 sits ON 0, where trunc is flat)
    pix = r['pix'][own]
    off = (pix - pix.round()).abs()
    risky = off[(pix.round() > 0.5)]
    if risky.numel():
        assert float(risky.min()) >= 0.5 / max(H - 1, W - 1, 1), float(risky.min())


@pytest.mark.parametrize('H,W,B', [(5, 7, 3), (33, 65, 1), (97, 131, 3)])
@pytest.mark.parametrize('frame', ['object', 'camera'])
@pytest.mark.parametrize('segment', [True, False])
def test_composed_pointcloud_against_the_restatement(H, W, B, frame, segment):
    obs = K.obs_case(H, W, B)
    r = K.restate64(obs, frame=frame)
    points, colors, index, counts = K.composed(obs, frame=frame, segment=segment)
    only = obs.pointcloud(frame=frame, segment=segment)
    assert torch.equal(only, points) and points.dtype == torch.float32 and points.shape == (int(counts.sum()), 3)
    assert colors.shape == points.shape
    if segment:
        keep = K.keep64(obs, r['pix'])
        got = torch.zeros(B * H * W, dtype=torch.bool)
        got[index.long()] = True
        safe = (K.pix_margin(r['pix']) >= 1e-3).reshape(-1)         # fp32 re-projection error: a few 1e-4 px at these sizes
        assert torch.equal(got[safe], keep.reshape(-1)[safe])
        if frame == 'object':
            assert torch.equal(got, keep.reshape(-1))                 # (column / row 0 sit ON an integer, where trunc is flat)
        else:                                                         # the quirk: camera-frame points through obj_to_image
            assert not torch.equal(got, K.own_pixel_keep(obs).reshape(-1))
    flat = index.long()
    ref_p, ref_c = r['points'].reshape(-1, 3)[flat], r['colors'].reshape(-1, 3)[flat]
    if flat.numel():                                                   # (the quirk can send every point of a view off the frame)
        assert float((points.double() - ref_p).abs().max()) <= 5e-6    # ~20 fp32 operations on coordinates of magnitude <= 1.3
    assert torch.equal(colors.double(), ref_c)
    # view-major, then row-major: the source indices ascend
    assert bool((flat[1:] > flat[:-1]).all())


def test_restatement_misreadings_differ():
    obs = K.obs_case(33, 65, 1)
    r = K.restate64(obs)
    assert float((K.restate64(obs, lattice='centres')['points'] - r['points']).abs().max()) > 1e-3
    rc = K.restate64(obs, frame='camera')
    assert float((K.restate64(obs, frame='camera', project='intrinsic')['pix'] - rc['pix']).abs().max()) > 1.0


def test_project_pointcloud_truncates_and_compute_point_mask_bounds():
    from latentfusion_amd.modules.geometry import Camera
    from latentfusion_amd.pointcloud import compute_point_mask, project_pointcloud
    cam = Camera(torch.tensor([[10.0, 0, 0], [0, 10.0, 0], [0, 0, 1.0]]), torch.eye(4), width=4, height=3)
    pts = torch.tensor([[[-0.05, -0.05, 1.0], [0.39, 0.29, 1.0], [0.4, 0.1, 1.0], [0.1, 0.3, 1.0], [-0.1, 0.0, 1.0],
                         [0.0, 0.0, 0.0], [0.15, 0.25, 1.0]]])
    pix = project_pointcloud(cam, pts)
    assert pix.dtype == torch.long and pix[0, 0].tolist() == [0, 0] and pix[0, 1].tolist() == [3, 2]
    mask = torch.ones(1, 1, 3, 4)
    mask[0, 0, 2, 1] = 0.0
    keep = compute_point_mask(cam, mask, pts)
    #        -0.5 -> pixel 0   inside     x = width  y = height  x = -1   0/0     masked out
    assert keep[0].tolist() == [True, True, False, False, False, False, False]
    with pytest.raises(IndexError):
        compute_point_mask(cam, torch.ones(1, 1, 2, 4), pts)          # (3, 2) is in the frame and outside the mask


def test_pointcloud_rejects_unknown_kernel_and_fused_needs_a_gpu():
    from latentfusion_amd import pointcloud
    obs = K.obs_case(5, 7, 1)
    with pytest.raises(ValueError, match='Unknown observation kernel'):
        obs.pointcloud(kernel='hip')
    with pytest.raises(ValueError, match='Unknown observation kernel'):
        pointcloud.eval_points(obs, 4, kernel='hip')
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="needs a GPU"):
            obs.pointcloud(kernel='fused')
        with pytest.raises(RuntimeError, match="needs a GPU"):
            pointcloud.eval_points(obs, 4, kernel='fused')
        from latentfusion_amd.three.utils import farthest_points
        with pytest.raises(RuntimeError, match="needs a GPU"):
            farthest_points(torch.zeros(5, 3), 2, F.pairwise_distance, kernel='fused')
    else:
        with pytest.raises(ValueError, match='device tensors'):
            obs.pointcloud(kernel='fused')


def test_eval_points_composed():
    from latentfusion_amd import pointcloud
    obs = K.obs_case(33, 65, 3)
    cloud = obs.pointcloud()
    pts = pointcloud.eval_points(obs, 50)
    centers = K.fps_composed(cloud, 50)[0]
    assert torch.equal(pts, cloud[centers]) and pts.shape == (50, 3)
    assert torch.equal(pointcloud.eval_points(obs, 10 ** 6), cloud)      # fewer points than asked for: all of them


# ---- the wrappers' argument rules, before any library call -------------------------------------------------------------------
def test_wrapper_argument_rules(monkeypatch):
    from latentfusion_amd import _lib, ops

    def no_library():
        raise AssertionError('the library was reached')
    monkeypatch.setattr(_lib, 'lib', no_library)
    host = torch.zeros(2, 1, 4, 5)
    cam = K.obs_case(5, 7, 1).camera
    with pytest.raises(ValueError, match='frame must be'):
        ops.depth_points(host, host, cam, frame='world')
    with pytest.raises(ValueError, match='must be bool'):
        ops.depth_points(host, host, cam, segment=1)
    with pytest.raises(ValueError, match='device tensor'):
        ops.depth_points(host, host, cam)
    with pytest.raises(ValueError, match='want must name'):
        ops.farthest_points(torch.zeros(5, 3), 2, want=('dist',))
    with pytest.raises(ValueError, match='want must name'):
        ops.farthest_points(torch.zeros(5, 3), 2, want=())
    with pytest.raises(ValueError, match='form must be'):
        ops.farthest_points(torch.zeros(5, 3), 2, form='cooperative')
    with pytest.raises(ValueError, match='device tensor'):
        ops.farthest_points(torch.zeros(5, 3), 2)


def test_binding_table_entries():
    from latentfusion_amd import _lib
    from latentfusion_amd.csrc import build
    for name in ('lf_depth_points', 'lf_depth_points_scratch_bytes', 'lf_farthest_points', 'lf_farthest_points_scratch_bytes'):
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES['lf_depth_points'][1]) == 19 and len(_lib.SIGNATURES['lf_farthest_points'][1]) == 12
    assert 'depth_points.hip' in build.SOURCES and 'fps.hip' in build.SOURCES
    assert _lib.LF_DEPTH_CAM_FLOATS == 32 and _lib.LF_FPS_RESIDENT_MAX == (160 * 1024 - 256) // 16
    L = _lib.lib()                                                   # loads without a GPU
    assert L.lf_depth_points_scratch_bytes(3, 97, 131) == 3 * 13 * 4 and L.lf_depth_points_scratch_bytes(0, 4, 4) == 0
    assert L.lf_farthest_points_scratch_bytes(2, 2000, 5, 0) == 0 and L.lf_farthest_points_scratch_bytes(2, 2000, 5, 1) == 0
    assert L.lf_farthest_points_scratch_bytes(2, 2000, 5, 2) == (2 * 2000 + 4 * 2 * 2) * 4
    assert L.lf_farthest_points_scratch_bytes(1, 20000, 5, 0) == (20000 + 4 * 20) * 4
    assert L.lf_farthest_points_scratch_bytes(1, 20000, 5, 1) == 0 and L.lf_farthest_points_scratch_bytes(1, 5, 6, 0) == 0
    # the entry points reject bad arguments before they touch the device
    assert L.lf_depth_points(None, None, 0, None, None, None, None, None, None, None, 0, 1, 4, 4, 4, 4, 1, 1, None) == -1
    assert L.lf_farthest_points(None, 0, None, None, None, None, 0, 1, 4, 2, 0, None) == -1


def test_pack_depth_cameras_matches_the_camera_properties():
    from latentfusion_amd import ops
    cam = K.obs_case(33, 65, 3).camera
    rec = ops.pack_depth_cameras(cam)
    assert rec.shape == (3, 32) and rec.dtype == torch.float32
    assert torch.equal(rec[:, 0:2], cam.viewport[:, :2]) and torch.equal(rec[:, 2], cam.viewport_width)
    assert torch.equal(rec[:, 4], cam.fu) and torch.equal(rec[:, 7], cam.v0)
    assert float((rec[:, 8:20].reshape(3, 3, 4) - cam.cam_to_obj[:, :3]).abs().max()) < 1e-6
    assert float((rec[:, 20:32].reshape(3, 3, 4) - cam.obj_to_image).abs().max()) < 1e-4
    assert torch.equal(ops.pack_depth_cameras(cam[1:2]), rec[1:2])       # a record does not depend on its batch mates
