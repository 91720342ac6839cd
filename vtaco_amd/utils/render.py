"""Depth rendering of a mesh from the tactile sensors' poses, on the device (ops.rays: csrc/ray_mesh.hip): the way back from a mesh to the
depth images the tactile side consumes (``vt_contact_scan`` / ``vt_contact_points``, ``vt_depth_cloud``, the ``Inferencer``).  The reference
takes those images from a simulator outside its tree; a ``trimesh.Trimesh`` would offer ``mesh.ray.intersects_first``.

The camera is the inverse of ``ops.contact_points``' unprojection, built from the same pose records (``common.sensor_pose_inverse``: the
sample rotation + [-pi/2, 0, pi/2] and the reference's pc_cam_to_world matrices; ``common.cloud_norm``), so a rendered depth image fed to
``contact_scan`` + ``contact_points`` gives back the points the rays hit.  The mesh is in the normalised frame, as generated meshes are."""
import numpy as np
import torch

from .. import ops
from ..common import cloud_norm, sensor_pose_inverse
from .voxels import _mesh_tensors


def pose_records(cam_pos, cam_rot, pc_ply=None, centroid=None, scale=None):
    """float64 [n,16] on the host: per sensor pose the record ``ops.contact_points`` reads -- ``sensor_pose_inverse``'s 3 x 3 and translation,
    then the normalisation: ``cloud_norm(pc_ply)``, or ``centroid`` / ``scale`` (0 / 1 by default: poses given in the mesh's own frame)."""
    cam_pos = np.asarray(cam_pos.detach().cpu() if torch.is_tensor(cam_pos) else cam_pos, dtype=np.float64).reshape(-1, 3)
    cam_rot = np.asarray(cam_rot.detach().cpu() if torch.is_tensor(cam_rot) else cam_rot, dtype=np.float64).reshape(-1, 3)
    if cam_pos.shape != cam_rot.shape:
        raise ValueError(f"pose_records: cam_pos {cam_pos.shape} and cam_rot {cam_rot.shape} differ")
    if pc_ply is not None:
        if centroid is not None or scale is not None:
            raise ValueError("pose_records: give pc_ply or centroid / scale, not both")
        centroid, scale = cloud_norm(pc_ply.detach().cpu().numpy() if torch.is_tensor(pc_ply) else pc_ply)
    pose = np.zeros((len(cam_pos), 16))
    for i in range(len(cam_pos)):
        m_inv, trans = sensor_pose_inverse(cam_pos[i], cam_rot[i])
        pose[i, :9], pose[i, 9:12] = m_inv.reshape(-1), trans
    pose[:, 12:15] = 0.0 if centroid is None else np.asarray(centroid, dtype=np.float64).reshape(3)
    pose[:, 15] = 1.0 if scale is None else float(scale)
    return pose


def _cast(mesh, pose, height, width, fov, method):
    v, f = _mesh_tensors(mesh)
    pose = torch.as_tensor(pose, dtype=torch.float64).reshape(-1, 16).to(v.device)
    origins, dirs = ops.rays.camera_rays(pose, width, height, fov)
    n = pose.shape[0]
    s, face = ops.rays.ray_mesh(v, f, origins, dirs.view(-1, 3), method=method, rays_per_origin=height * width)
    return s.view(n, height * width), face.view(n, height * width)


def render_depth(mesh, cam_pos, cam_rot, height=240, width=320, fov=60.0, pc_ply=None, centroid=None, scale=None, method='tree'):
    """(depth f32 [n,H,W], face i32 [n,H,W]) of the mesh seen from n sensor poses: per pixel the planar depth of the first face its ray
    hits -- the number ``contact_points`` and ``depth_cloud`` unproject -- and that face; +inf and -1 where the ray hits nothing.
    ``cam_pos`` / ``cam_rot`` [n,3] are what ``Generator3D.generate_tactile_pc`` takes; ``pc_ply`` (the scene's object cloud) or
    ``centroid`` / ``scale`` say how the mesh's frame was normalised (default: not at all).  ``method``: ``ops.rays.ray_mesh``'s; the rays of an
    image are coherent and the tree wins at every mesh size measured, its build included (profiles/ray_mesh_bench.json: five 320 x 240 images
    0.43 against 0.69 ms at 576 faces, 1.9 against 944 ms at 976 125)."""
    pose = pose_records(cam_pos, cam_rot, pc_ply, centroid, scale)
    s, face = _cast(mesh, pose, int(height), int(width), fov, method)
    depth = ops.rays.depth_from_hits(s)
    return depth.view(-1, int(height), int(width)), face.view(-1, int(height), int(width))


def _origin(depth_origin, n_pixels, dev):
    if isinstance(depth_origin, str):
        depth_origin = np.loadtxt(depth_origin)
    o = torch.as_tensor(depth_origin.detach().cpu() if torch.is_tensor(depth_origin) else np.asarray(depth_origin, dtype=np.float64), dtype=torch.float64)
    if o.numel() != n_pixels:
        raise ValueError(f"simulate_touch: depth_origin has {o.numel()} readings for a sensor image of {n_pixels} pixels")
    return o.reshape(-1).to(dev)


def simulate_touch(mesh, cam_pos, cam_rot, depth_origin, near=0.019, threshold=1e-4, height=240, width=320, fov=60.0, pc_ply=None, centroid=None,
                   scale=None, method='tree'):
    """(depth f32 [n, H*W], touch_success bool [n]) of n sensors pressed against the mesh, shaped like ``inputs.depth``: per pixel
    ``min(hit depth, depth_origin)`` clamped below at ``near``, the sensor's flat reading ``depth_origin`` (array or path, as ``Generator3D``
    accepts it) where the ray hits nothing or hits beyond it.  A sensor touched when some pixel departs from the flat reading by more than
    ``threshold`` (``ops.contact_scan``'s rule): the result can be fed to ``contact_scan`` / ``contact_points`` and the ``Inferencer``."""
    pose = pose_records(cam_pos, cam_rot, pc_ply, centroid, scale)
    s, _ = _cast(mesh, pose, int(height), int(width), fov, method)
    origin = _origin(depth_origin, int(height) * int(width), s.device)
    depth = ops.rays.depth_from_hits(s, origin, near)
    _, count = ops.contact_scan(depth, origin, None, threshold)
    return depth, count > 0


def visible_points(mesh, points, eye, slack=None, method=None):
    """bool [N]: whether each of ``points`` [N,3] is seen from ``eye`` [3] -- one ray ``eye + s (point - eye)`` per point, the point at
    s = 1; visible when no face is hit at s < 1 - slack.  ``slack`` defaults to the walk's own, ``ops.rays.SLACK`` times the size of the
    scene about the eye over the ray's length: a point ON the mesh is not hidden by its own face.  Points that lie off the surface by more
    (float32 samples, say) need a ``slack`` of their own."""
    v, f = _mesh_tensors(mesh)
    p = torch.as_tensor(points).to(v.device)
    p = (p if p.dtype == torch.float64 else p.float()).reshape(-1, 3)
    e = torch.as_tensor(eye).to(v.device).to(torch.float64).reshape(1, 3)
    if slack is None:
        lo, hi = v.min(0).values.double().cpu().numpy(), v.max(0).values.double().cpu().numpy()
        pe = p.double().cpu().numpy() - e.cpu().numpy()
        size = np.maximum(np.abs(lo - e.cpu().numpy()), np.abs(hi - e.cpu().numpy())).sum()
        reach = np.abs(pe).max(axis=1) if len(pe) else np.ones(0)
        slack = float((ops.rays.SLACK * size / np.maximum(reach, np.finfo(np.float64).tiny)).max()) if len(pe) else 0.0
    dirs = p.double() - e
    s, _ = ops.rays.ray_mesh(v, f, e, dirs, t_min=0.0, t_max=1.0 - float(slack), method=method)
    return torch.isinf(s)
