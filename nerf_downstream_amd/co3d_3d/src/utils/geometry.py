"""Correspondence helpers of the registration stack (counterpart of the reference's co3d_3d/src/utils/geometry.py), on torch
tensors.  The names and argument lists are the reference's; the nearest-neighbour searches run as one launch of
`minkowski.graph.knn_cross` (csrc/graph.hip mink_knn_cross), which streams the candidates through LDS and never forms an
N0 x N1 matrix, instead of the reference's chunked `pdist` + row minimum with a host copy per chunk.

Deviations, on purpose:
  * `find_nn_gpu` returns its indices (int64) and distances on the inputs' device, not on the CPU: the reference's `.cpu()` per
    chunk is a host synchronisation per chunk.  `nn_max_n` is accepted and ignored (there are no chunks).
  * `get_matching_indices` takes [n, 3] arrays or tensors instead of open3d point clouds, and returns an int64 [m, 2] tensor
    instead of a list of tuples; open3d's KD-tree radius search is `knn_cross` on the transformed source with C = 3.
  * `make_open3d_point_cloud` is not here: it needs open3d."""
import numpy as np
import torch
from scipy.linalg import expm, norm

from nerf_downstream_amd.minkowski.graph import MAX_K, knn_cross


def M(axis, theta):
    """Rotation matrix about `axis` by the angle `theta` (the matrix exponential of the cross-product matrix)."""
    return expm(np.cross(np.eye(3), axis / norm(axis) * theta))


def sample_random_trans(pcd, randg, rotation_range=360):
    """A 4 x 4 rigid transform: a random rotation (axis `randg.rand(3) - 0.5`, then angle from `randg.rand(1)`: the reference's
    draws in the reference's order) that also moves the centroid of `pcd` [n, 3] to the origin."""
    pcd = pcd.detach().cpu().numpy() if torch.is_tensor(pcd) else np.asarray(pcd)
    T = np.eye(4)
    R = M(randg.rand(3) - 0.5, rotation_range * np.pi / 180.0 * (randg.rand(1) - 0.5))
    T[:3, :3] = R
    T[:3, 3] = R.dot(-np.mean(pcd, axis=0))
    return T


def pdist(A, B, dist_type="L2"):
    """The full [len(A), len(B)] distance matrix in plain torch, for small inputs: it FORMS the matrix (and a
    [len(A), len(B), C] difference tensor on the way).  "L2" is sqrt(d2 + 1e-7), "SquareL2" is d2."""
    if dist_type == "L2":
        D2 = torch.sum((A.unsqueeze(1) - B.unsqueeze(0)).pow(2), 2)
        return torch.sqrt(D2 + 1e-7)
    elif dist_type == "SquareL2":
        return torch.sum((A.unsqueeze(1) - B.unsqueeze(0)).pow(2), 2)
    else:
        raise NotImplementedError("Not implemented")


def corr_dist(est, gth, xyz0, xyz1, weight=None, max_dist=1):
    """Mean distance, clamped at `max_dist`, between xyz0 moved by the estimated and by the ground-truth 4 x 4 transform."""
    xyz0_est = xyz0 @ est[:3, :3].t() + est[:3, 3]
    xyz0_gth = xyz0 @ gth[:3, :3].t() + gth[:3, 3]
    dists = torch.clamp(torch.sqrt(((xyz0_est - xyz0_gth).pow(2)).sum(1)), max=max_dist)
    if weight is not None:
        dists = weight * dists
    return dists.mean()


def find_corr(xyz0, xyz1, F0, F1, subsample_size=-1, nn_max_n=500):
    """(xyz0', xyz1'): for every (sub-sampled, through np.random.choice as in the reference) row of F0 its nearest row of F1 in
    feature space, as matched coordinates; the indexing stays on the device."""
    subsample = len(F0) > subsample_size
    if subsample_size > 0 and subsample:
        N0 = min(len(F0), subsample_size)
        N1 = min(len(F1), subsample_size)
        inds0 = torch.as_tensor(np.random.choice(len(F0), N0, replace=False), device=F0.device)
        inds1 = torch.as_tensor(np.random.choice(len(F1), N1, replace=False), device=F1.device)
        F0, F1 = F0[inds0], F1[inds1]

    nn_inds = find_nn_gpu(F0, F1, nn_max_n=nn_max_n)
    if subsample_size > 0 and subsample:
        return xyz0[inds0.to(xyz0.device)], xyz1[inds1[nn_inds].to(xyz1.device)]
    else:
        return xyz0, xyz1[nn_inds.to(xyz1.device)]


def find_nn_gpu(F0, F1, nn_max_n=-1, return_distance=False, dist_type="SquareL2"):
    """inds int64 [N0] on the inputs' device: the row of F1 nearest to every row of F0 (ties to the lower row); with
    `return_distance` also dists [N0, 1], "SquareL2" = the squared distance of the chosen pair, "L2" = sqrt(d2 + 1e-7) as
    `pdist` defines it.  One `knn_cross(..., k=1)` launch; `nn_max_n` is accepted and ignored.  F1 must not be empty."""
    if dist_type not in ("L2", "SquareL2"):
        raise NotImplementedError("Not implemented")
    if len(F1) == 0:
        raise ValueError("find_nn_gpu: F1 is empty")
    if not return_distance:
        return knn_cross(F0, F1, k=1)[:, 0].long()
    idx, d2 = knn_cross(F0, F1, k=1, return_distance=True)
    return idx[:, 0].long(), (torch.sqrt(d2 + 1e-7) if dist_type == "L2" else d2)


_RADIUS_K = MAX_K  # slots of the radius search


def _xyz(a, device=None):
    a = a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))
    assert a.dim() == 2 and a.shape[1] == 3, "get_matching_indices: [n, 3] points"
    return a.to(device=device, dtype=torch.float32) if device is not None else a.float()


def get_matching_indices(source, target, trans, search_voxel_size, K=None):
    """int64 [m, 2]: the pairs (i, j) with |trans(source_i) - target_j| <= search_voxel_size, i ascending and, per i, distance
    ascending (the order of the reference's loop over a KD-tree radius search), at most K per source point.  source, target:
    [n, 3] arrays or tensors (target's device decides where the search runs: it must be the GPU); trans: 4 x 4.
    The candidates are the `knn_cross` neighbours of the transformed source (K slots, 64 for K=None); a pair is kept when its
    recomputed squared distance is at most search_voxel_size ** 2.  K=None means all inside the radius: if some point has all
    64 slots inside it the answer would be truncated, and a ValueError is raised.  K > 64 is a ValueError."""
    if K is not None and not 1 <= int(K) <= _RADIUS_K:
        raise ValueError(f"get_matching_indices: K = {K} outside 1..{_RADIUS_K} (K=None: all inside the radius, at most {_RADIUS_K})")
    target = _xyz(target)
    source = _xyz(source, target.device)
    trans = torch.as_tensor(np.asarray(trans) if not torch.is_tensor(trans) else trans).to(device=target.device, dtype=torch.float32)
    moved = source @ trans[:3, :3].t() + trans[:3, 3]
    k = _RADIUS_K if K is None else int(K)
    idx, d2 = knn_cross(moved, target, k=k, return_distance=True)
    inside = d2 <= float(search_voxel_size) ** 2  # (+inf at the -1 slots: never inside)
    if K is None and bool(inside.all(1).any()):
        raise ValueError(f"get_matching_indices: a point has {_RADIUS_K} or more neighbours inside the radius; pass K <= {_RADIUS_K}")
    # per source point distance ascending, equal distances in slot (= row) order; the slots already follow the ranking score
    order = torch.argsort(torch.where(inside, d2, torch.full_like(d2, float("inf"))), dim=1, stable=True)
    idx, inside = idx.gather(1, order), inside.gather(1, order)
    rows = torch.arange(idx.shape[0], device=idx.device).unsqueeze(1).expand_as(idx)
    return torch.stack([rows[inside], idx[inside].long()], 1)
