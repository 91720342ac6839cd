"""Ray casting on a mesh and the sensor camera (vt_ray_mesh, vt_ray_tree_query, vt_camera_rays, vt_depth_from_hits: csrc/ray_mesh.hip).  A
submodule only: callers write ``ops.rays.ray_mesh``, ``ops.rays.ray_tree_query``, ``ops.rays.camera_rays``, ``ops.rays.depth_from_hits``.

Rays are ``o + s d`` in float64; ``d`` is not normalised and ``s`` is in units of ``d``.  A miss is ``s = +inf``, ``face = -1``, NaN weights.
``method='brute'`` tests every face and is the definition; ``method='tree'`` walks the face octree (``ops.metrics.ClosestTree``: the tree of
the fast winding number with the closest point's boxes) and gives the same bits.  ``TREE_MIN_FACES`` is chosen from
profiles/ray_mesh_bench.json (README, "ray_mesh.hip")."""
import ctypes
import math

import torch

from ._base import _lib, VtError, check, dev_ptr, stream_ptr, I32, _c
from . import metrics

F64 = torch.float64
TREE_MIN_FACES = 8192         # method=None: the tree from this many faces on.  profiles/ray_mesh_bench.json: 100 000 scattered rays, build included,
                              # 1.75 against 1.35 ms at 4 096 faces, 1.89 against 4.66 ms at 16 384; coherent image rays win at every size
SLACK = 2.0 ** -40            # the walk grows every box by SLACK * S ("ray_mesh.hip")


def _rays(what, origins, dirs, dev):
    """(origins f64 [N or 1, 3], dirs f64 [N,3], rays per origin): f32 or f64 in, converted exactly."""
    if not (torch.is_tensor(origins) and torch.is_tensor(dirs)):
        raise VtError(f"{what}: origins and dirs must be tensors")
    if origins.device != dev or dirs.device != dev or not dirs.is_cuda:
        raise VtError(f"{what}: origins and dirs must live on the mesh's HIP device (got {origins.device}, {dirs.device}); vtaco_amd has no CPU path")
    if origins.dtype not in (torch.float32, F64) or dirs.dtype not in (torch.float32, F64):
        raise VtError(f"{what}: origins and dirs must be float32 or float64 (got {origins.dtype}, {dirs.dtype})")
    if dirs.dim() != 2 or dirs.shape[1] != 3 or origins.dim() != 2 or origins.shape[1] != 3 or origins.shape[0] not in (1, dirs.shape[0]):
        raise VtError(f"{what}: expected dirs [N,3] and origins [N,3] or [1,3] (got {tuple(dirs.shape)} and {tuple(origins.shape)})")
    N = dirs.shape[0]
    return _c(origins.to(F64)), _c(dirs.to(F64)), (1 if origins.shape[0] == N else max(N, 1))


def _outputs(N, dev, bary, stats=False):
    s = torch.empty((N,), dtype=F64, device=dev)
    face = torch.empty((N,), dtype=I32, device=dev)
    w = torch.empty((N, 3), dtype=F64, device=dev) if bary else None
    st = torch.empty((N, 2), dtype=I32, device=dev) if stats else None
    return s, face, w, st


def ray_tree_query(ctree, origins, dirs, t_min=0.0, t_max=math.inf, bary=False, stats=False, strict=True, rays_per_origin=None):
    """``ray_mesh``'s (s f64 [N], face i32 [N][, bary f64 [N,3]]) against a ClosestTree (``ops.metrics.closest_point_tree_build``; a tree
    built for distance or winding is reused), bit for bit (vt_ray_tree_query: a walk that skips every cell whose box the ray's remaining
    segment misses; reads nothing back).  With ``stats`` also int32 [N,2]: the boxes and the faces tested per ray.  A tree whose mesh has a
    face index outside [0, V) raises VtError as the brute-force call does; ``strict=False`` answers from the other faces.
    ``rays_per_origin``: origins [N / rays_per_origin, 3], one per block of that many consecutive rays (camera images)."""
    what = "ray_tree_query"
    if not isinstance(ctree, metrics.ClosestTree):
        raise VtError(f"{what}: expected a ClosestTree (ops.metrics.closest_point_tree_build)")
    t = ctree.tree
    origins, dirs, per = _per_origin(what, origins, dirs, t.device, rays_per_origin)
    if strict and ctree.status & 1:
        raise VtError(f"{what}: a face index lies outside [0, V) (found on the device by the build; that face was not read)")
    N = dirs.shape[0]
    s, face, w, st = _outputs(N, t.device, bary, stats)
    check(_lib.load().vt_ray_tree_query(ctypes.c_void_p(t.buf.data_ptr()), t.buf.numel() * 8, ctypes.c_void_p(ctree.side.data_ptr()),
                                        ctree.side.numel() * 8, t.n_faces, t.depth, t._state, dev_ptr(origins, "origins", F64) if N else None, per,
                                        dev_ptr(dirs, "dirs", F64) if N else None, N, float(t_min), float(t_max),
                                        dev_ptr(s, "s", F64) if N else None, dev_ptr(face, "face", I32) if N else None,
                                        dev_ptr(w, "bary", F64) if bary and N else None, dev_ptr(st, "stats", I32) if stats and N else None,
                                        stream_ptr()), "vt_ray_tree_query")
    out = (s, face, w) if bary else (s, face)
    return out + (st,) if stats else out


def _per_origin(what, origins, dirs, dev, rays_per_origin):
    if rays_per_origin is None:
        return _rays(what, origins, dirs, dev)
    per = int(rays_per_origin)
    if not (torch.is_tensor(origins) and torch.is_tensor(dirs)) or dirs.dim() != 2 or origins.dim() != 2 or per < 1 or \
            origins.shape[0] * per != dirs.shape[0]:
        raise VtError(f"{what}: rays_per_origin={rays_per_origin} needs origins [N / rays_per_origin, 3] and dirs [N, 3]")
    o, d, _ = _rays(what, origins[:1], dirs, dev)
    return _c(origins.to(F64)), d, per


def ray_mesh(verts, faces, origins, dirs, t_min=0.0, t_max=math.inf, method=None, tree=None, bary=False, rays_per_origin=None):
    """What every ray ``origins + s dirs`` hits first on the mesh (verts [V,3] f32, faces [F,3] i32 / i64 on the device): (s f64 [N], face
    i32 [N][, bary f64 [N,3]]) -- the smallest s in [t_min, t_max], its face (the lowest index among equal s) and the weights of that
    face's corners; a miss is (+inf, -1, NaN).  The watertight rule of csrc/ray_face.h in float64, two-sided: what trimesh's
    ``mesh.ray.intersects_first`` / ``intersects_location`` answer.  ``origins`` [N,3] or [1,3], f32 or f64 (converted exactly).
    ``method='brute'`` (vt_ray_mesh) tests every face; ``'tree'`` (vt_ray_tree_query) walks the face octree -- ``tree``: a ClosestTree of
    this mesh, built when not given -- to the same bits; None picks the tree from ``TREE_MIN_FACES`` faces on, or when a tree is given.
    A mesh without vertices or faces, or a face index outside [0, V), raises VtError."""
    what = "ray_mesh"
    if method is None:
        method = 'tree' if tree is not None or (torch.is_tensor(faces) and faces.shape[0] >= TREE_MIN_FACES) else 'brute'
    if method not in ('brute', 'tree'):
        raise VtError(f"{what}: method must be 'brute', 'tree' or None (got {method!r})")
    if not (torch.is_tensor(verts) and torch.is_tensor(faces)) or not (verts.is_cuda and faces.is_cuda) or verts.device != faces.device:
        raise VtError(f"{what}: verts and faces must be tensors on one HIP device; vtaco_amd has no CPU path")
    if verts.dim() != 2 or verts.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise VtError(f"{what}: expected verts [V,3] and faces [F,3] (got {tuple(verts.shape)} and {tuple(faces.shape)})")
    if verts.dtype != torch.float32 or faces.dtype not in (torch.int32, torch.int64):
        raise VtError(f"{what}: verts must be float32 and faces int32 or int64 (got {verts.dtype}, {faces.dtype})")
    verts, faces = _c(verts), _c(faces.to(I32))
    V, F = verts.shape[0], faces.shape[0]
    if V == 0 or F == 0:
        raise VtError(f"{what}: a mesh without vertices or faces has nothing to hit")
    if method == 'tree':
        if tree is None:
            tree = metrics.closest_point_tree_build(verts, faces)
        elif not isinstance(tree, metrics.ClosestTree) or tree.tree.n_faces != F or tree.tree.device != verts.device:
            raise VtError(f"{what}: the tree given is not a ClosestTree of this mesh")
        return ray_tree_query(tree, origins, dirs, t_min, t_max, bary=bary, rays_per_origin=rays_per_origin)
    origins, dirs, per = _per_origin(what, origins, dirs, verts.device, rays_per_origin)
    N, dev = dirs.shape[0], verts.device
    s, face, w, _ = _outputs(N, dev, bary)
    lib = _lib.load()
    ws = torch.empty((max(lib.vt_ray_mesh_workspace_bytes(F, N), 8) // 4,), dtype=I32, device=dev)
    check(lib.vt_ray_mesh(dev_ptr(verts, "verts"), V, dev_ptr(faces, "faces", I32), F, dev_ptr(origins, "origins", F64) if N else None, per,
                          dev_ptr(dirs, "dirs", F64) if N else None, N, float(t_min), float(t_max), dev_ptr(s, "s", F64) if N else None,
                          dev_ptr(face, "face", I32) if N else None, dev_ptr(w, "bary", F64) if bary and N else None,
                          ctypes.c_void_p(ws.data_ptr()), ws.numel() * 4, stream_ptr()), "vt_ray_mesh")
    if N and int(ws[0].item()) & 1:
        raise VtError(f"{what}: a face index lies outside [0, V) (found on the device by the prepare pass; that face was not read)")
    return (s, face, w) if bary else (s, face)


def camera_rays(pose, width, height, fov=60.0):
    """(origins f64 [n,3], dirs f64 [n, height * width, 3]) of the sensor cameras (vt_camera_rays): ``pose`` [n,16] f64 on the device, the
    records ``contact_points`` and ``depth_cloud`` read (inverse pose 3 x 3, translation, cloud centroid, scale).  The inverse of their
    unprojection: pixel (u, v) of image i at planar depth z is the point ``origins[i] + z dirs[i, v * width + u]``, so the ``s`` of a hit
    is the depth those two consume."""
    if not torch.is_tensor(pose) or pose.dim() != 2 or pose.shape[1] != 16 or pose.dtype != F64 or not pose.is_cuda:
        raise VtError(f"camera_rays: pose must be a float64 [n,16] device tensor (got {tuple(pose.shape) if torch.is_tensor(pose) else pose})")
    pose = _c(pose)
    n, W, H = pose.shape[0], int(width), int(height)
    if W <= 0 or H <= 0:
        raise VtError(f"camera_rays: width and height must be positive (got {width}, {height})")
    origins = torch.empty((n, 3), dtype=F64, device=pose.device)
    dirs = torch.empty((n, H * W, 3), dtype=F64, device=pose.device)
    check(_lib.load().vt_camera_rays(dev_ptr(pose, "pose", F64) if n else None, n, W, H, float(fov), dev_ptr(origins, "origins", F64) if n else None,
                                     dev_ptr(dirs, "dirs", F64) if n else None, stream_ptr()), "vt_camera_rays")
    return origins, dirs


def depth_from_hits(s, depth_origin=None, near=0.0):
    """float32 depth of the hit parameters ``s`` f64 [..., n_pixels] (vt_depth_from_hits): ``min(s, depth_origin)`` clamped below at
    ``near``; a miss gives the sensor's flat reading ``depth_origin`` (f64 [n_pixels]), or +inf without one."""
    if not torch.is_tensor(s) or s.dtype != F64 or not s.is_cuda or s.dim() < 1:
        raise VtError("depth_from_hits: s must be a float64 device tensor [..., n_pixels]")
    s = _c(s)
    npix, N = max(int(s.shape[-1]), 1), s.numel()
    if depth_origin is not None:
        if not torch.is_tensor(depth_origin) or depth_origin.dtype != F64 or depth_origin.device != s.device or depth_origin.numel() != s.shape[-1]:
            raise VtError(f"depth_from_hits: depth_origin must be a float64 tensor of {s.shape[-1]} readings on the device of s")
        depth_origin = _c(depth_origin.reshape(-1))
    depth = torch.empty(s.shape, dtype=torch.float32, device=s.device)
    check(_lib.load().vt_depth_from_hits(dev_ptr(s, "s", F64) if N else None, dev_ptr(depth_origin, "depth_origin", F64) if N else None, npix, N,
                                         float(near), dev_ptr(depth, "depth") if N else None, stream_ptr()), "vt_depth_from_hits")
    return depth
