"""Greedy farthest-point sampling / clustering (latentfusion/three/utils.py:4-49)."""
import torch

KERNELS = ('composed', 'fused')


def _farthest_points_fused(data, n_clusters, dist_func, return_center_indexes, return_distances):
    """The tuple forms of farthest_points from ops.farthest_points (lf_farthest_points): long tensors on the data's device."""
    import torch.nn.functional as F
    if dist_func is not None and dist_func is not F.pairwise_distance:
        raise ValueError("kernel='fused' computes Euclidean distances: dist_func must be F.pairwise_distance or None")
    if not isinstance(data, torch.Tensor) or not data.is_cuda:
        if not torch.cuda.is_available():
            raise RuntimeError("kernel 'fused' needs a GPU: the sampling HIP kernel has no CPU form (use kernel='composed')")
        raise ValueError("kernel='fused' needs a device tensor (the composed path serves host tensors)")
    if data.dtype != torch.float32 or data.dim() != 2 or data.shape[1] != 3:
        raise ValueError(f"kernel='fused' needs a float32 (N,3) tensor, got {data.dtype} {tuple(data.shape)}")
    count = data.shape[0]
    if n_clusters >= count:                                  # every row is its own centre
        ids = torch.arange(count, dtype=torch.long, device=data.device)
        return (ids, ids.clone()) if return_center_indexes else ids
    from .. import ops
    want = ('owner',) + (('centers',) if return_center_indexes else ()) + (('nearest',) if return_distances else ())
    out = ops.farthest_points(data, int(n_clusters), want=want)
    owner = out['owner'].long()
    if not return_center_indexes:
        return owner
    centers = out['centers'].long()
    return (owner, centers, out['nearest']) if return_distances else (owner, centers)


def farthest_points(data, n_clusters: int, dist_func, return_center_indexes=False, return_distances=False, verbose=False,
                    kernel=None):
    """Picks `n_clusters` rows of `data`, each the farthest from those already picked (the first is row 0, the
    arg-max of the constant initial distances), and assigns every row to the LAST centre that attains its
    minimum distance.  Returns cluster ids [, centre indices [, distances to the nearest centre]].
    kernel: None | 'composed' (this host loop, on the tensors' device) | 'fused' (one lf_farthest_points call for a device
    float32 (N,3) cloud and Euclidean distances; direct coordinate differences, so it agrees with F.pairwise_distance's picks
    except at near-ties)."""
    if kernel is not None and kernel not in KERNELS:
        raise ValueError(f'Unknown farthest_points kernel {kernel!r} (one of {KERNELS})')
    if kernel == 'fused':
        return _farthest_points_fused(data, n_clusters, dist_func, return_center_indexes, return_distances)
    count = data.shape[0]
    dev = data.device
    if n_clusters >= count:                                  # every row is its own centre
        ids = torch.arange(count, dtype=torch.long, device=dev)
        return (ids, ids.clone()) if return_center_indexes else ids
    owner = torch.full((count,), -1, dtype=torch.long, device=dev)
    nearest = torch.full((count,), 1e7, dtype=torch.float32, device=dev)
    picked = []
    for k in range(n_clusters):
        picked.append(int(torch.argmax(nearest)))
        to_new = dist_func(data[picked[-1]].unsqueeze(0).expand(count, -1), data)
        nearest = torch.minimum(nearest, to_new)
        owner[nearest == to_new] = k
        if verbose:
            print('farthest points max distance : {}'.format(nearest.max()))
    centers = torch.tensor(picked, dtype=torch.long, device=dev)
    if not return_center_indexes:
        return owner
    return (owner, centers, nearest) if return_distances else (owner, centers)
