"""The reference's src/utils/icp.py on the device (csrc/icp.hip through ``ops.icp``), for 3-D points.

    best_fit_transform(A, B) -> (T, R, t)                                           icp.py:5-47
    nearest_neighbor(src, dst) -> (distances, indices)                              icp.py:50-66
    icp(A, B, init_pose=None, max_iterations=20, tolerance=0.001) -> (T, distances, i)   icp.py:69-121

``nearest_neighbor`` and ``icp`` take ``method='brute'`` (the default) or ``'tree'``: the octree of csrc/point_tree.hip where the reference
has sklearn's kd-tree, with results equal to the brute force's bit for bit.

numpy arrays in give float64 numpy arrays out (indices int64, ``i`` a Python int); they are moved to the current HIP device for the
work.  Device tensors in give device tensors out (indices int32, ``i`` a 0-dim int32 tensor: nothing waits for the device).  Batches
[B,N,3] give T [B,4,4], R [B,3,3], t [B,3], distances [B,N] and i [B].  There is no host path: without a HIP device every call raises.

Two differences from the reference, both relaxations: ``nearest_neighbor`` and ``icp`` accept sets of different sizes (the reference's
asserts are stricter than its arithmetic; ``best_fit_transform`` still needs equal shapes), and equal distances go to the lowest index
(the kd-tree's choice is unspecified).  ``max_iterations < 1``, where the reference dies with an unbound name, raises VtError; so does
any point dimension other than 3.
"""
import numpy as np
import torch

from .._lib import VtError


def _device_points(what, *sets):
    """The sets as device tensors, and whether they came as numpy arrays."""
    host = not any(torch.is_tensor(s) for s in sets)
    out = []
    for s in sets:
        if not torch.is_tensor(s):
            s = np.asarray(s)
            if s.dtype != np.float32:
                s = s.astype(np.float64)
        if s.ndim not in (2, 3):
            raise VtError(f"{what}: expected points [N,3] or [B,N,3] (got shape {tuple(s.shape)})")
        if s.shape[-1] != 3:
            raise VtError(f"{what}: only 3-D points are built (got m = {s.shape[-1]})")
        if not torch.is_tensor(s):
            if not torch.cuda.is_available():
                raise VtError(f"{what}: no HIP device to move the points to; vtaco_amd has no CPU path")
            s = torch.from_numpy(np.ascontiguousarray(s)).to(torch.device("cuda", torch.cuda.current_device()))
        out.append(s)
    return out, host


def best_fit_transform(A, B):
    """The least-squares rigid transform that maps the corresponding points A onto B: (T [4,4], R [3,3], t [3])."""
    (a, b), host = _device_points("best_fit_transform", A, B)
    if tuple(a.shape) != tuple(b.shape):
        raise VtError(f"best_fit_transform: A and B must have one shape (got {tuple(a.shape)} and {tuple(b.shape)})")
    from .. import ops
    T = ops.icp.icp_fit(a, b)
    R, t = T[..., :3, :3], T[..., :3, 3]
    if host:
        T = T.cpu().numpy()
        return T, T[..., :3, :3].copy(), T[..., :3, 3].copy()
    return T, R.contiguous(), t.contiguous()


def nearest_neighbor(src, dst, method="brute"):
    """(distances, indices): the Euclidean distance from every point of src to its nearest point of dst, and that point's index.
    ``method='tree'`` searches an octree over dst (``ops.icp.point_tree_build``): the same bits."""
    (s, d), host = _device_points("nearest_neighbor", src, dst)
    from .. import ops
    d2, idx = ops.icp.nn_points(s, d, method=method)
    dist = torch.sqrt(d2)
    if host:
        return dist.cpu().numpy(), idx.cpu().numpy().astype(np.int64)
    return dist, idx


def icp(A, B, init_pose=None, max_iterations=20, tolerance=0.001, method="brute"):
    """Iterative closest point: (T, distances, i) -- the transform that maps A onto B, the last iteration's neighbour distances and the
    0-based index of the last executed iteration.  ``method='tree'`` searches an octree over B in every iteration: the same bits."""
    (a, b), host = _device_points("icp", A, B)
    if init_pose is not None and not torch.is_tensor(init_pose):
        init_pose = torch.from_numpy(np.ascontiguousarray(np.asarray(init_pose, dtype=np.float64))).to(a.device)
    from .. import ops
    out = ops.icp.icp(a, b, init_pose=init_pose, max_iterations=max_iterations, tolerance=tolerance, method=method)
    if host:
        its = out.iterations.cpu().numpy()
        return out.T.cpu().numpy(), out.distances.cpu().numpy(), (int(its) if its.ndim == 0 else its.astype(np.int64))
    return out.T, out.distances, out.iterations
