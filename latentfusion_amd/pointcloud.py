"""Point clouds of observations: which pixel a point falls on, which points of a view lie on its segmentation mask (the
project_pointcloud / compute_point_mask pair of the reference's pointcloud module, same semantics, written for this package
without the per-view host loop), and the evaluation cloud built from them: Observation.pointcloud, then greedy farthest-point
sampling.  PLY IO, the outlier filters and the plane segmentation of that module are out of scope (plyfile, scikit-learn, PCL)."""
import torch
import torch.nn.functional as F

from . import three
from .three import utils as three_utils


def project_pointcloud(camera, points):
    """(B,n,3) object-frame points -> (B,n,2) long pixels (x, y) under camera.obj_to_image, truncated toward zero: -0.5 is
    pixel 0.  On the CPU the conversion turns a NaN or infinite quotient into the most negative integer, which no frame holds."""
    return three.transform_coords(points, camera.obj_to_image).long()


def compute_point_mask(camera, mask, points):
    """(B,n) bool: point i of view b projects inside the camera.width x camera.height frame and onto a non-zero pixel of
    mask (B,1,H,W) or (B,H,W).  A pixel of the frame that the mask does not hold is an IndexError (the mask is indexed with
    frame pixels: it has to be frame-sized)."""
    fg = (mask[:, 0] if mask.dim() == 4 else mask) != 0
    rows, cols = fg.shape[-2:]
    px, py = project_pointcloud(camera, points).unbind(-1)
    inside = (px >= 0) & (px < camera.width) & (py >= 0) & (py < camera.height)
    if bool((inside & ((px >= cols) | (py >= rows))).any()):
        raise IndexError(f'a point projects to a pixel of the {camera.height} x {camera.width} frame outside the '
                         f'{rows} x {cols} mask')
    zero = torch.zeros_like(px)
    at = torch.where(inside, py * cols + px, zero)                   # (pixels outside the frame read element 0 and are dropped)
    return inside & torch.gather(fg.reshape(fg.shape[0], -1), 1, at)


def eval_points(observation, n_points=4096, frame='object', kernel=None):
    """The evaluation cloud of an observation: observation.pointcloud(frame, segment=True), farthest-point sampled down to
    n_points (all of them when the cloud has no more) -> (n,3), ready for pose.metrics.camera_metrics_batch.  kernel: None
    (observation.KERNEL) | 'composed' | 'fused' (lf_depth_points and lf_farthest_points: device tensors only; the one
    device-to-host copy is the point count)."""
    from .observation import _resolve_kernel
    kernel = _resolve_kernel(kernel)
    points = observation.pointcloud(frame=frame, segment=True, kernel=kernel)
    _, centers = three_utils.farthest_points(points, n_points, F.pairwise_distance, return_center_indexes=True, kernel=kernel)
    return points[centers.to(points.device)]
