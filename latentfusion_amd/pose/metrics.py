"""Pose-accuracy metrics of the reference's evaluation code: rotation / translation distance, ADD,
ADD-S, ADD with the z-180 symmetry, 2-D projection error (latentfusion/pose/metrics.py:11-109).

Same names, argument order and return types as the reference.  ADD-S's nearest-neighbour search runs
in row blocks of `batch_size` like the reference's `best_distance`, so the peak memory is
batch_size x P instead of P x P."""
import collections
import math

import torch

from .. import three


def camera_rotation_dist(camera1, camera2):
    return three.quaternion.angular_distance(camera1.quaternion, camera2.quaternion)


def camera_translation_dist(camera1, camera2):
    return torch.norm(camera1.translation - camera2.translation, dim=-1)


def compute_point_add(extrinsic_gt, extrinsic_eval, points):
    """Mean distance between the model points under the two poses (metrics.py:76-80)."""
    p_gt = three.transform_coords(points, extrinsic_gt)
    p_ev = three.transform_coords(points, extrinsic_eval)
    return torch.mean(torch.norm(p_gt - p_ev, dim=-1))


def best_distance(x1, x2, batch_size: int = 1000):
    """For every row of x1 the distance to its nearest row of x2 (metrics.py:90-99)."""
    out = []
    for i in range(0, x1.shape[0], batch_size):
        out.append(torch.cdist(x1[i:i + batch_size], x2).min(dim=1).values)
    return torch.cat(out, dim=0) if out else x1.new_zeros(0)


def compute_point_add_s(extrinsic_gt, extrinsic_eval, points):
    """ADD-S: mean closest-point distance (metrics.py:83-87)."""
    p_gt = three.transform_coords(points, extrinsic_gt)
    p_ev = three.transform_coords(points, extrinsic_eval)
    if p_gt.dim() == 3:                                   # (1,P,3) from a batched extrinsic
        p_gt, p_ev = p_gt.reshape(-1, 3), p_ev.reshape(-1, 3)
    return torch.mean(best_distance(p_gt, p_ev))


def compute_point_add_sym(extrinsic_gt, extrinsic_eval, points):
    """min(ADD, ADD with the ground truth turned 180 degrees about z) (metrics.py:64-73)."""
    z_axis = torch.tensor([[0.0, 0.0, 1.0]], dtype=torch.float32)
    rot = three.rotation_to_4x4(three.quaternion.quat_to_mat(three.quaternion.from_axis_angle(z_axis, math.pi)))
    a0 = compute_point_add(extrinsic_gt, extrinsic_eval, points)
    a1 = compute_point_add(extrinsic_gt @ rot.to(extrinsic_gt), extrinsic_eval, points)
    return torch.min(a0, a1)


def compute_point_proj2d(proj_gt, proj_eval, points):
    """Mean image-plane distance of the projected model points (metrics.py:102-106)."""
    p_gt = three.transform_coords(points, proj_gt)
    p_ev = three.transform_coords(points, proj_eval)
    return torch.mean(torch.norm(p_gt - p_ev, dim=-1))


def camera_metrics(camera_gt, camera_eval, points, scale_to_meters, use_add=True, use_add_sym=True, use_add_s=True,
                   use_proj2d=True, **kwargs):
    """Dictionary of metrics for one camera pair, a list of them for batched cameras (metrics.py:19-61;
    like the reference, the per-pair recursion uses the default switches)."""
    if len(camera_gt) > 1:
        return [camera_metrics(c1, c2, points, scale_to_meters) for c1, c2 in zip(camera_gt, camera_eval)]
    camera_gt, camera_eval = camera_gt.clone().cpu(), camera_eval.clone().cpu()
    metrics = {
        'rotation_dist': camera_rotation_dist(camera_gt, camera_eval).squeeze().item(),
        'translation_dist': (camera_translation_dist(camera_gt, camera_eval) * scale_to_meters).squeeze().item(),
    }
    if points is not None:
        if use_add:
            metrics['add'] = compute_point_add(camera_gt.obj_to_cam, camera_eval.obj_to_cam, points) * scale_to_meters
        if use_add_s:
            metrics['add_s'] = compute_point_add_s(camera_gt.obj_to_cam, camera_eval.obj_to_cam, points) * scale_to_meters
        if use_add_sym:
            metrics['add_sym'] = (compute_point_add_sym(camera_gt.obj_to_cam, camera_eval.obj_to_cam, points)
                                  * scale_to_meters)
        if use_proj2d:
            metrics['proj2d'] = compute_point_proj2d(camera_gt.obj_to_image, camera_eval.obj_to_image, points)
    return metrics


def concat_camera_metrics(metrics_list):
    out = collections.defaultdict(list)
    for key in metrics_list[0].keys():
        for m in metrics_list:
            out[key].append(m[key])
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# batched scoring on the device (csrc/points.hip): additions, the functions above are unchanged
# ---------------------------------------------------------------------------------------------------------------------------
def best_distance_device(x1, x2, return_index=False):
    """`best_distance` on device tensors, batched: x1 (M,3) / x2 (Q,3), or (B,M,3) / (B,Q,3) -> dist (M,) or (B,M), with
    return_index=True also the nearest row's index (int32, the smallest on ties).  One lf_nn_dist launch; distances are direct
    coordinate differences in fp32 (closer to fp64 than `best_distance`, whose torch.cdist takes the Gram form)."""
    from .. import ops
    out = ops.nn_dist(x1, x2, want=('dist', 'idx') if return_index else ('dist',))
    return (out['dist'], out['idx']) if return_index else out['dist']


def _rot_z180(like):
    z_axis = torch.tensor([[0.0, 0.0, 1.0]], dtype=torch.float32)
    rot = three.rotation_to_4x4(three.quaternion.quat_to_mat(three.quaternion.from_axis_angle(z_axis, math.pi)))
    return rot.to(like)


def camera_metrics_batch(camera_gt, camera_eval, points, scale_to_meters, use_add=True, use_add_sym=True, use_add_s=True,
                         use_proj2d=True, device=None):
    """`camera_metrics` for B camera pairs at once -> a dict of (B,) float32 tensors on the compute device: 'rotation_dist',
    'translation_dist' and, with points, the selected ones of 'add', 'add_s', 'add_sym', 'proj2d' (units as in
    `camera_metrics`; {k: v.tolist()} has the layout of `concat_camera_metrics`).

    len(camera_gt) is len(camera_eval), or 1: one ground truth against B hypotheses (the ranking an estimator returns).
    Unlike the per-pair recursion of `camera_metrics` (which, like the reference, drops them), the use_* switches hold for
    every pair.  device: where to compute, default camera_eval's.  On a GPU the cameras stay there and one call issues one
    lf_nn_dist launch (ADD-S) and at most two lf_points_pair_dist launches (ADD with the z-180 member of ADD-sym as rows of
    one, proj2d as the other) whatever B is; the library is required there.  On the CPU the per-pair functions above run and
    their results are stacked."""
    n_gt, B = len(camera_gt), len(camera_eval)
    if B < 1 or n_gt not in (1, B):
        raise ValueError(f'camera_gt must hold 1 or {B} cameras (one per camera_eval), got {n_gt}')
    device = torch.device(device) if device is not None else camera_eval.device
    if device.type != 'cuda':
        per_pair = [camera_metrics(camera_gt[i if n_gt > 1 else 0], camera_eval[i], points, scale_to_meters, use_add=use_add,
                                   use_add_sym=use_add_sym, use_add_s=use_add_s, use_proj2d=use_proj2d) for i in range(B)]
        return {k: torch.stack([torch.as_tensor(m[k], dtype=torch.float32).reshape(()) for m in per_pair]).to(device)
                for k in per_pair[0]}
    from .. import ops
    camera_gt, camera_eval = camera_gt.to(device), camera_eval.to(device)
    # angular_distance pair by pair (its (N1,N2) table would grow with B squared)
    q_gt, q_ev = three.quaternion.normalize(camera_gt.quaternion), three.quaternion.normalize(camera_eval.quaternion)
    metrics = {
        'rotation_dist': (2 * torch.acos((q_gt * q_ev).sum(dim=-1).abs().clamp(-1.0 + 1e-7, 1.0 - 1e-7))).expand(B),
        'translation_dist': (camera_translation_dist(camera_gt, camera_eval) * scale_to_meters).expand(B),
    }
    if points is None:
        return metrics
    points = points.to(device=device, dtype=torch.float32).reshape(-1, 3)
    e_gt, e_ev = camera_gt.obj_to_cam.expand(B, 4, 4), camera_eval.obj_to_cam
    if use_add or use_add_sym:
        a = [e_gt] + ([e_gt @ _rot_z180(e_gt)] if use_add_sym else [])    # ADD itself is ADD-sym's first member
        means = ops.points_pair_dist(points, torch.cat(a), torch.cat([e_ev] * len(a))).view(len(a), B)
        if use_add:
            metrics['add'] = means[0] * scale_to_meters
    if use_add_s:
        metrics['add_s'] = ops.nn_dist(points, points, e_gt[:, :3], e_ev[:, :3], want=('mean',))['mean'] * scale_to_meters
    if use_add_sym:
        metrics['add_sym'] = torch.min(means[0], means[1]) * scale_to_meters
    if use_proj2d:
        # obj_to_image = intrinsic @ obj_to_cam as the camera forms it, from the poses already at hand
        metrics['proj2d'] = ops.points_pair_dist(points, (camera_gt.intrinsic @ e_gt[:n_gt]).expand(B, 3, 4),
                                                 camera_eval.intrinsic @ e_ev)
    return metrics
