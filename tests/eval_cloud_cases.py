"""Cases, restatements and bounds of the evaluation point-cloud tests (tests/test_eval_cloud_cases.py proves on the CPU what
tests/test_depth_points_gpu.py and tests/test_fps_gpu.py lean on).  Everything here runs on the CPU; nothing is changed after
it is made (the lru_caches hand out the same objects: treat them as read-only).

FPS clouds: randn(n,3).clamp(-4,4) from ONE generator seeded 3, drawn in the order of FPS_SIZES.  The first four are compared
with the composed path (three.utils.farthest_points over F.pairwise_distance on the CPU) as well: they satisfy, in fp64,
  - at every pick after the first the largest and the second-largest running minimum distance differ by >= FPS_MARGIN = 2e-5,
  - no point's two nearest centres are closer than FPS_MARGIN to each other in distance.
Why 2e-5: F.pairwise_distance adds 1e-6 to every coordinate difference, which moves a distance by at most sqrt(3) * 1e-6 and two
distances against each other by at most 3.6e-6; fp32 rounding of a distance at |x| <= 4 (differences <= 8, d <= 14) is about
2e-6 for the pair.  Together under 6e-6: the margin is three times that.  The last two clouds fail the condition and are compared
with the bit-exact restatement only.

Observations: frames OBS_FRAMES, B in OBS_BATCHES, un-zoomed cameras whose frame is the image (viewport (0, 0, W, H)), depth
t_z +- 0.15 (positive everywhere), a random 40 % mask with the last row and the last column cleared.  The viewport lattice is
u_j = W j / (W - 1): its last sample sits exactly on u = W, where the frame test flips with rounding (hence the cleared row and
column); sample 0 sits on 0, where truncation toward zero maps either sign of the rounding noise to pixel 0; every other
sample is j + j / (W - 1), at least 1 / (W - 1) px from an integer, against a re-projection error of a few 1e-4 px.  So the kept
set of the composed path is the own-pixel mask, which tests/test_eval_cloud_cases.py asserts for every case."""
import functools
import math

import torch
import torch.nn.functional as F

FPS_SIZES = [(7, 3), (65, 64), (257, 40), (1025, 128), (4099, 512), (20000, 1024)]
FPS_CONDITIONED = 4                        # the first four
FPS_MARGIN = 2e-5
FPS_START = 1e14                           # the running minimum's start on d^2 (1e7 squared)
OBS_FRAMES = [(1, 1), (2, 2), (5, 7), (33, 65), (97, 131)]
OBS_BATCHES = [1, 3]
T_Z = 1.0


# ----------------------------------------------------------------------------------------------------------------------------
# farthest-point sampling
# ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fps_clouds():
    """[(x (n,3) float32, K)] in the order of FPS_SIZES."""
    g = torch.Generator().manual_seed(3)
    return [(torch.randn(n, 3, generator=g).clamp(-4, 4), k) for n, k in FPS_SIZES]


def rounded_sqrt(v):
    """The correctly rounded fp32 root: torch.sqrt in fp64, rounded once (53 bits are more than the 2 * 24 + 2 that make the
    second rounding harmless).  torch.sqrt on a float32 CPU tensor is NOT it: its AVX-512 form is one ulp off for about 0.6 % of
    the values (it differs from numpy's root and from the fp64 one; 30 of cloud 2's 257 distances, measured), while the
    kernel's sqrtf and torch.sqrt on the device are correctly rounded.  tests/test_eval_cloud_cases.py holds this against numpy."""
    return torch.sqrt(v.double()).float()


def fps_restate(x, K, tie='smallest', owner_rule='last'):
    """The contract of lf_farthest_points in fp32 on the CPU, one elementwise torch operation per contract operation (eager ops
    are not fused) and rounded_sqrt: -> (centers (K,) int32, owner (n,) int32, nearest (n,) float32).  tie / owner_rule other
    than the defaults are deliberate misreadings (largest index among the maxima; the FIRST centre that attains the minimum)."""
    x = x.float()
    n = x.shape[0]
    mins = torch.full((n,), FPS_START, dtype=torch.float32)
    owner = torch.full((n,), -1, dtype=torch.int32)
    centers = []
    for k in range(K):
        if tie == 'smallest':
            c = int(torch.argmax(mins))                                            # the first of the maxima
        else:
            c = n - 1 - int(torch.argmax(mins.flip(0)))
        centers.append(c)
        dx, dy, dz = x[:, 0] - x[c, 0], x[:, 1] - x[c, 1], x[:, 2] - x[c, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        hit = d2 <= mins if owner_rule == 'last' else d2 < mins
        owner[hit] = k
        mins = torch.minimum(mins, d2)
    return torch.tensor(centers, dtype=torch.int32), owner, rounded_sqrt(mins)


@functools.lru_cache(maxsize=None)
def fps_tie_clouds():
    """[(x, K)] where maxima and minima tie exactly: 20 random rows twice and five of them a third time, with more picks than
    distinct rows; a 4 x 4 x 3 integer lattice."""
    base = torch.randn(20, 3, generator=torch.Generator().manual_seed(11))
    lat = torch.stack(torch.meshgrid(torch.arange(4.), torch.arange(4.), torch.arange(3.), indexing='ij'), dim=-1).reshape(-1, 3)
    return [(torch.cat((base, base, base[:5])), 23), (lat, 12)]


@functools.lru_cache(maxsize=None)
def fps_expected(i):
    """fps_restate of cloud i, computed once."""
    x, k = fps_clouds()[i]
    return fps_restate(x, k)


def fps_gaps64(x, K):
    """In fp64 with exact distances: (the smallest gap over picks 1..K-1 between the largest and second-largest running minimum
    distance, the share of points whose two nearest centres are closer than FPS_MARGIN to each other in distance, the picks)."""
    x = x.double()
    n = x.shape[0]
    mins = torch.full((n,), 1e7, dtype=torch.float64)
    gap = math.inf
    centers = []
    for k in range(K):
        if k > 0:
            top = torch.topk(mins, 2).values
            gap = min(gap, float(top[0] - top[1]))
        centers.append(int(torch.argmax(mins)))
        mins = torch.minimum(mins, (x - x[centers[-1]]).norm(dim=1))
    if K < 2:
        return gap, 0.0, centers
    two = torch.topk(torch.cdist(x, x[centers]), 2, dim=1, largest=False).values
    return gap, float(((two[:, 1] - two[:, 0]) < FPS_MARGIN).float().mean()), centers


def fps_composed(x, K):
    """The composed path on the CPU: (centers int64, owner int64, nearest float32)."""
    from latentfusion_amd.three.utils import farthest_points
    owner, centers, nearest = farthest_points(x, K, F.pairwise_distance, return_center_indexes=True, return_distances=True)
    return centers, owner, nearest


# ----------------------------------------------------------------------------------------------------------------------------
# observations
# ----------------------------------------------------------------------------------------------------------------------------
def _rotations(B, gen):
    """B proper rotations (3,3) float32, about 0.5 rad from the identity."""
    from latentfusion_amd.three import quaternion as quat
    axis = F.normalize(torch.randn(B, 3, generator=gen), dim=-1)
    angle = 0.2 + 0.5 * torch.rand(B, 1, generator=gen)
    q = torch.cat((torch.cos(angle / 2), axis * torch.sin(angle / 2)), dim=-1)
    return quat.quat_to_mat(q)[:, :3, :3]


def make_observation(H, W, B, seed=0, zero_extrinsic=False, viewport=None):
    """An Observation on the CPU as the module docstring describes it.  zero_extrinsic: identity rotation and t = 0 (object
    frame = camera frame); viewport: (xmin, ymin, xmax, ymax) instead of the whole frame."""
    from latentfusion_amd.modules.geometry import Camera
    from latentfusion_amd.observation import Observation
    gen = torch.Generator().manual_seed(1000 * seed + 7 * H + W + 31 * B)
    f = 1.3 * max(H, W, 4)
    intrinsic = torch.tensor([[f, 0.0, W / 2.0 + 0.3], [0.0, 1.1 * f, H / 2.0 - 0.2], [0.0, 0.0, 1.0]]).expand(B, -1, -1).clone()
    extrinsic = torch.eye(4).expand(B, -1, -1).clone()
    if not zero_extrinsic:
        extrinsic[:, :3, :3] = _rotations(B, gen)
        extrinsic[:, :3, 3] = torch.cat((0.1 * (torch.rand(B, 2, generator=gen) - 0.5), torch.full((B, 1), T_Z)), dim=-1)
    vp = None if viewport is None else torch.tensor(viewport, dtype=torch.float32).expand(B, -1).clone()
    camera = Camera(intrinsic, extrinsic, width=W, height=H, viewport=vp)
    depth = T_Z + 0.3 * (torch.rand(B, 1, H, W, generator=gen) - 0.5)
    mask = (torch.rand(B, 1, H, W, generator=gen) < 0.4).float()
    mask[:, :, -1, :] = 0.0
    mask[:, :, :, -1] = 0.0
    color = torch.rand(B, 3, H, W, generator=gen)
    return Observation(color, depth, mask, camera)


@functools.lru_cache(maxsize=None)
def obs_case(H, W, B):
    return make_observation(H, W, B)


def restate64(obs, frame='object', lattice='linear', project='obj_to_image'):
    """The contract of lf_depth_points in fp64, from the camera's fp32 state widened to fp64: -> dict(points (B,HW,3), pix
    (B,HW,2) the re-projected pixel before truncation, colors (B,HW,3)).  lattice / project other than the defaults are
    deliberate misreadings: 'centres' samples pixel centres, 'intrinsic' projects camera-frame points without the extrinsic."""
    cam = obs.camera._map(lambda t: t.detach().double())
    B, _, H, W = obs.depth.shape
    vp = cam.viewport
    sx = torch.arange(W, dtype=torch.float64) / (W - 1) if W > 1 else torch.zeros(1, dtype=torch.float64)
    sy = torch.arange(H, dtype=torch.float64) / (H - 1) if H > 1 else torch.zeros(1, dtype=torch.float64)
    if lattice == 'centres':
        sx, sy = (torch.arange(W, dtype=torch.float64) + 0.5) / W, (torch.arange(H, dtype=torch.float64) + 0.5) / H
    u = (vp[:, 0, None, None] + (vp[:, 2] - vp[:, 0])[:, None, None] * sx[None, None, :]).expand(B, H, W)
    v = (vp[:, 1, None, None] + (vp[:, 3] - vp[:, 1])[:, None, None] * sy[None, :, None]).expand(B, H, W)
    z = obs.depth[:, 0].double()
    K = cam.intrinsic
    x = (u - K[:, 0, 2, None, None]) / K[:, 0, 0, None, None] * z
    y = (v - K[:, 1, 2, None, None]) / K[:, 1, 1, None, None] * z
    p = torch.stack((x, y, z), dim=-1).reshape(B, H * W, 3)
    R, t = cam.rotation_matrix[:, :3, :3], cam.translation
    if frame == 'object':
        p = (p - t[:, None, :]) @ R                                                # R^T (p - t), as rows
    q = p @ R.transpose(1, 2) + t[:, None, :] if project == 'obj_to_image' else p    # obj_to_cam of whatever p is
    h = q @ K[:, :, :3].transpose(1, 2) + K[:, None, :, 3]
    pix = h[..., :2] / h[..., 2:]
    return dict(points=p, pix=pix, colors=obs.color.double().permute(0, 2, 3, 1).reshape(B, H * W, 3))


def own_pixel_keep(obs):
    """(B, HW) bool: the pixel's own mask entry."""
    return obs.mask[:, 0].reshape(len(obs), -1) != 0


def keep64(obs, pix):
    """(B, HW) bool: the keep rule of the contract applied to fp64 re-projections `pix` (B,HW,2)."""
    B, _, H, W = obs.mask.shape
    pu, pv = pix[..., 0], pix[..., 1]
    ok = torch.isfinite(pu) & torch.isfinite(pv) & (pu > -1) & (pu < W) & (pv > -1) & (pv < H) & (obs.depth[:, 0].reshape(B, -1) != 0)
    zero = torch.zeros_like(pu)
    at = torch.where(ok, pv, zero).trunc().long() * W + torch.where(ok, pu, zero).trunc().long()
    return ok & (torch.gather(obs.mask[:, 0].reshape(B, -1), 1, at) != 0)


def pix_margin(pix):
    """(B, HW): distance of the re-projected pixel to the nearest integer on either axis (0 for non-finite ones)."""
    d = (pix - pix.round()).abs().amin(dim=-1)
    return torch.where(torch.isfinite(d), d, torch.zeros_like(d))


def composed(obs, frame='object', segment=True):
    """The composed path on the CPU: (points (n,3), colors (n,3), index (n,) int32, counts (B,) int32)."""
    from latentfusion_amd.pointcloud import compute_point_mask
    B, _, H, W = obs.depth.shape
    points, colors = obs.pointcloud(frame=frame, return_colors=True, segment=segment, kernel='composed')
    if not segment:
        return points, colors, torch.arange(B * H * W, dtype=torch.int32), torch.full((B,), H * W, dtype=torch.int32)
    lattice = obs.camera.depth_object_coords if frame == 'object' else obs.camera.depth_camera_coords
    keep = compute_point_mask(obs.camera, obs.mask, torch.stack(lattice(obs.depth), dim=-1).reshape(B, -1, 3))
    return points, colors, torch.nonzero(keep.reshape(-1))[:, 0].to(torch.int32), keep.sum(dim=1).to(torch.int32)


def excess(got, ref, e32):
    """max over elements of |got - ref| - max(4 e32, 2e-6 + 2e-5 |ref|): <= 0 passes (the project's forward bound).  NaN counts
    as +inf; an empty comparison passes."""
    if ref.numel() == 0:
        return -math.inf, 0.0
    err = (got.double() - ref).abs()
    ex = err - torch.maximum(4 * e32, 2e-6 + 2e-5 * ref.abs())
    ex = torch.where(torch.isnan(ex), torch.full_like(ex, math.inf), ex)
    return float(ex.max()), float(err.max())
