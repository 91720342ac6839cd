"""Evaluation metrics of the reference (src/common.py:11-175): the host functions as the reference writes them, the device
forms of the two the visualise block calls (chamfer_distance_device, earth_mover_distance_device: HIP kernels), the kd-tree Chamfer
distance on the point octree (chamfer_distance_kdtree, chamfer_distance), and the hand-object
geometry of its eval_step (training.py:393-419) on vt_closest_point_mesh and vt_winding_number: signed_distance, penetration_depth,
mesh_distances."""
from __future__ import annotations

import numpy as np
import torch


def compute_iou(occ1, occ2, threshold=None):
    """IoU of two occupancy sets (common.py:11-43).  As in the reference the ``threshold`` argument is
    IGNORED: both sets are binarised at mean(occ2)."""
    occ1, occ2 = np.asarray(occ1), np.asarray(occ2)
    if occ1.ndim >= 2:
        occ1 = occ1.reshape(occ1.shape[0], -1)
    if occ2.ndim >= 2:
        occ2 = occ2.reshape(occ2.shape[0], -1)
    thr = np.mean(occ2)
    a, b = occ1 >= thr, occ2 >= thr
    union = (a | b).astype(np.float32).sum(axis=-1)
    inter = (a & b).astype(np.float32).sum(axis=-1)
    return inter / union


def chamfer_distance_naive(points1, points2):
    """Squared-distance Chamfer of two [B,T,3] tensors (common.py:62-83); runs on whatever device they live on."""
    if points2.size(1) < 2048:
        points1 = points1[:, :points2.size(1), :]
    assert points1.size() == points2.size()
    d = (points1.unsqueeze(2) - points2.unsqueeze(1)).pow(2).sum(-1)
    return d.min(dim=1)[0].mean(dim=1) + d.min(dim=2)[0].mean(dim=1)


def earth_mover_distance(points1, points2):
    """EMD by optimal assignment (common.py:45-51)."""
    from scipy.optimize import linear_sum_assignment
    from scipy.spatial import distance
    d = distance.cdist(points1, points2)
    rows, cols = linear_sum_assignment(d)
    return d[rows, cols].sum() / len(d)


def chamfer_distance_device(points1, points2, give_id=False):
    """``chamfer_distance(points1, points2, use_kdtree=False)`` (common.py:69-91) on the device: [B,T,3] f32 HIP tensors -> [B]
    (f32, on the device): mean over points2 of the squared distance to the nearest point of points1, plus the same the other way
    (vt_chamfer_nn: the minima are numpy's f32 restatement bit for bit).  The reference's truncation rule holds: when points2 has
    fewer than 2048 points, points1 is cut to that many, and the two sizes must then agree (VtError otherwise).  ``give_id``:
    also the nearest indices, (chamfer, idx_12 [B,T] of points2 for each point1, idx_21 [B,T] of points1 for each point2) as
    int64, like the kd-tree variant returns them."""
    from . import ops
    from ._lib import VtError
    if points1.dim() != 3 or points2.dim() != 3:
        raise VtError(f"chamfer_distance_device: expected [B,T,3] point sets (got {tuple(points1.shape)}, {tuple(points2.shape)})")
    if points2.size(1) < 2048:
        points1 = points1[:, :points2.size(1), :]
    if points1.size() != points2.size():
        raise VtError(f"chamfer_distance_device: point sets of different sizes {tuple(points1.size())} and {tuple(points2.size())}")
    d_12, i_12, d_21, i_21 = ops.chamfer_nn(points1, points2)
    chamfer = d_21.mean(dim=1) + d_12.mean(dim=1)
    if give_id:
        return chamfer, i_12.long(), i_21.long()
    return chamfer


def chamfer_distance_kdtree(points1, points2, give_id=False):
    """``chamfer_distance_kdtree`` (common.py:94-140) on the device: [B,T1,3] and [B,T2,3] HIP tensors of any two sizes, no truncation
    rule -> chamfer1 + chamfer2 [B]: the mean over points1 of the squared distance to the nearest point of points2, plus the same the
    other way.  Where the reference asks pykdtree, each side's octree answers (``ops.icp.point_tree_build`` / ``point_tree_query``:
    float64, the lowest index among equal minima); the means are ``torch.mean`` over those float64 distances and the result is cast to
    the inputs' dtype.  ``give_id``: the reference's tuple (chamfer1, chamfer2, idx_nn_12 [B,T1], idx_nn_21 [B,T2]), indices int64."""
    from . import ops
    from ._lib import VtError
    if not (torch.is_tensor(points1) and torch.is_tensor(points2)) or points1.dim() != 3 or points2.dim() != 3:
        raise VtError("chamfer_distance_kdtree: expected [B,T,3] point sets")
    if points1.dtype != points2.dtype:
        raise VtError(f"chamfer_distance_kdtree: point sets of two dtypes ({points1.dtype}, {points2.dtype})")
    p1, p2 = points1.detach(), points2.detach()
    d_12, i_12 = ops.icp.point_tree_query(ops.icp.point_tree_build(p2), p1)
    d_21, i_21 = ops.icp.point_tree_query(ops.icp.point_tree_build(p1), p2)
    chamfer1, chamfer2 = torch.mean(d_12, dim=1), torch.mean(d_21, dim=1)
    if give_id:
        return chamfer1.to(points1.dtype), chamfer2.to(points1.dtype), i_12.long(), i_21.long()
    return (chamfer1 + chamfer2).to(points1.dtype)


def chamfer_distance(points1, points2, use_kdtree=True, give_id=False):
    """``chamfer_distance`` (common.py:54-66) on the device: ``chamfer_distance_kdtree`` by default, ``chamfer_distance_device`` (the
    reference's naive form, its truncation rule included) with ``use_kdtree=False``; ``give_id`` goes to the tree form only, as there."""
    if use_kdtree:
        return chamfer_distance_kdtree(points1, points2, give_id=give_id)
    return chamfer_distance_device(points1, points2)


def earth_mover_distance_device(points1, points2, return_assignment=False):
    """``EarthMoverDistance(points1, points2)`` (common.py:45-51: cdist, linear_sum_assignment, sum / len(d)) on the device:
    points1 [N,3], points2 [M,3] (or batches [B,N,3], [B,M,3]) -> the mean matched distance as a float (a float64 array [B] for
    batches).  The assignment is the epsilon-scaling auction of ops.emd_assignment (exact for N != M: the smaller side is padded
    with zero-cost dummies; cost within max(N, M) * eps / N of the optimum, eps = ops.EMD_EPS_FINAL * 2^floor(log2(cost range)),
    the cost range being the diagonal of the clouds' common bounding box), its cost is evaluated in float64 as cdist does.  A NaN or
    infinite coordinate raises VtError.  Inputs are taken as float32 and moved to the current HIP device when they are elsewhere.
    ``return_assignment``: also the ops.EmdResult (assign [.., max(N, M)] i32: row i of points1 -> row assign[i] of points2, >= M = left unmatched)."""
    from . import ops
    from ._lib import VtError
    dev = torch.device("cuda", torch.cuda.current_device())

    def dev_f32(p):
        t = p if torch.is_tensor(p) else torch.from_numpy(np.asarray(p))
        return t.to(dev if not t.is_cuda else t.device, torch.float32)
    a, b = dev_f32(points1), dev_f32(points2)
    single = a.dim() == 2
    if single:
        a, b = a.unsqueeze(0), b.unsqueeze(0)
    if a.dim() != 3 or b.dim() != 3:
        raise VtError(f"earth_mover_distance_device: expected [N,3] / [B,N,3] point sets (got {tuple(a.shape)}, {tuple(b.shape)})")
    res = ops.emd_assignment(a, b)
    emd = float(res.emd[0]) if single else res.emd
    return (emd, res) if return_assignment else emd


def hand_joint_error(joints_gt, joints_pred):
    """Mean over the joints of the L2 distance between ground-truth and predicted joints (common.py:142-154), per scene:
    [B,J,3] (or [J,3]) tensors or arrays -> float64 [B] (a float for one scene, as the reference returns it)."""
    def host(j):
        return (j.detach().cpu().numpy() if torch.is_tensor(j) else np.asarray(j)).astype(np.float64)
    gt, pred = host(joints_gt), host(joints_pred)
    if gt.shape != pred.shape or gt.ndim not in (2, 3) or gt.shape[-1] != 3:
        from ._lib import VtError
        raise VtError(f"hand_joint_error: expected two [B,J,3] joint sets (got {gt.shape}, {pred.shape})")
    err = np.mean(np.linalg.norm(gt - pred, axis=-1), axis=-1)
    return float(err) if gt.ndim == 2 else err


def _inside_depth(d2, winding):
    """Per row: the largest surface distance among the points whose winding number exceeds 0.5, 0 where none is inside."""
    dist = torch.sqrt(d2) * (winding > 0.5).to(d2.dtype)
    return dist.max(dim=-1)[0]


def _winding(winding, verts, faces, pts):
    """The winding numbers of pts by the exact kernel or by the tree of ``ops.winding`` (built for this call)."""
    from . import ops
    if winding == 'exact':
        return ops.winding_number(verts, faces, pts)
    if winding == 'fast':
        return ops.winding.fast(verts, faces, pts)
    raise ValueError("winding must be 'exact' or 'fast'")


def _distance2(distance, verts, faces, pts, tree=None):
    """vt_closest_point_mesh's d2 of pts [N,3] by the brute-force kernel or through the face octree (built for this call, on ``tree`` when
    one is given): equal bits."""
    from . import ops
    if distance == 'brute':
        return ops.metrics.closest_point_mesh(verts.float(), faces, pts, want_point=False).d2
    if distance == 'tree':
        return ops.metrics.closest_point_tree_query(ops.metrics.closest_point_tree_build(verts.float(), faces, tree=tree), pts, want_point=False).d2
    raise ValueError("distance must be 'brute' or 'tree'")


def signed_distance(pts, verts, faces, winding='exact', distance='brute'):
    """Distance from every query point pts [N,3] to the mesh (verts [V,3] f32, faces [F,3] int; device tensors), float64 [N]: the square
    root of vt_closest_point_mesh's minimum, negative where the winding number (vt_winding_number) exceeds 0.5 -- inside a closed,
    outward-oriented mesh.  ``winding='fast'`` takes the sign from the hierarchical approximation (vt_winding_tree_query) instead.
    ``distance='tree'`` finds the same minimum by walking the face octree (vt_closest_tree_query: equal bits); with ``winding='fast'``
    one octree serves both halves."""
    from . import ops
    pts = pts.float().contiguous()
    if winding == 'fast' and distance == 'tree':
        tree = ops.winding.build(verts.float(), faces)
        d2 = _distance2(distance, verts, faces, pts, tree=tree)
        inside = ops.winding.query(tree, pts) > 0.5
        dist = torch.sqrt(d2)
        return torch.where(inside, -dist, dist)
    d2 = _distance2(distance, verts, faces, pts)
    inside = _winding(winding, verts, faces, pts) > 0.5
    dist = torch.sqrt(d2)
    return torch.where(inside, -dist, dist)


_HAND_UPSAMPLE = (0, 1, 2)
_upsample_layer = None


def upsample_hand(hand_verts, hand_faces, levels):
    """The hand's vertices after ``levels`` (0, 1 or 2) midpoint subdivisions of ``hand_faces`` -- the reference's ``UpSampleLayer``
    (encoder/manopth/upsample_layer.py, csrc/mesh_subdivide.hip): 778 MANO vertices become 3 093, then 12 337, and sample the contact
    region 4x and 16x as densely.  hand_verts [K,3] or [B,K,3] on the device, hand_faces [Fh,3] int; one connectivity, cached, serves
    every hand.  ``levels`` 0 returns ``hand_verts`` and launches nothing."""
    global _upsample_layer
    if levels not in _HAND_UPSAMPLE or isinstance(levels, bool):
        raise ValueError(f"hand_upsample must be one of {_HAND_UPSAMPLE} (got {levels!r})")
    if levels == 0:
        return hand_verts
    if hand_faces is None:
        raise ValueError("hand_upsample > 0 needs hand_faces, the hand's triangles ([Fh,3]; the MANO layer's th_faces)")
    if _upsample_layer is None:
        from .encoder.manopth import UpSampleLayer
        _upsample_layer = UpSampleLayer()
    v = hand_verts if hand_verts.dim() == 3 else hand_verts.unsqueeze(0)
    v = v.float().contiguous()
    f = hand_faces.to(v.device).unsqueeze(0).expand(v.shape[0], -1, -1)
    for _ in range(levels):
        v, f = _upsample_layer(v, f)
    return v if hand_verts.dim() == 3 else v[0]


def penetration_depth(hand_verts, verts, faces, scale, winding='exact', distance='brute', hand_upsample=0, hand_faces=None):
    """Penetration depth of a hand into an object mesh as the reference's eval_step measures it (training.py:406-419): 0 when no hand
    vertex has a winding number above 0.5; otherwise the largest distance to the surface (trimesh.proximity.closest_point there,
    vt_closest_point_mesh here) among the vertices that have, times ``scale`` -- the reference passes max ||pc_ply|| of the uncentred
    object cloud.  hand_verts [K,3] in the mesh's frame, verts [V,3] f32, faces [F,3] int on the device -> float.  ``winding``: 'exact'
    (vt_winding_number) or 'fast' (vt_winding_tree_query); ``distance``: 'brute' (vt_closest_point_mesh) or 'tree' (vt_closest_tree_query:
    equal bits).  ``hand_upsample`` 1 or 2 probes the hand after that many midpoint subdivisions of ``hand_faces`` (``upsample_hand``:
    K + E vertices, 4x and 16x as dense); 0 (the default) probes the K vertices given and launches what it always did."""
    pts = upsample_hand(hand_verts, hand_faces, hand_upsample).float().contiguous()
    d2 = _distance2(distance, verts, faces, pts)
    return float(_inside_depth(d2, _winding(winding, verts, faces, pts))) * float(scale)


def penetration_depth_scenes(hand_verts, meshes, scales, winding='exact', trees=None, distance='brute', ctrees=None, hand_upsample=0,
                             hand_faces=None):
    """``penetration_depth`` for a batch in one launch sequence each (vt_closest_point_mesh_scenes, vt_winding_number_scenes):
    hand_verts [B,K,3] on the device, meshes = [(verts f32 [V,3], faces i32 [F,3])] per scene, scales [B] -> float64 array [B].
    ``winding='fast'`` queries one tree per scene (``trees``: those of ``ops.winding.build``, built here when not given).
    ``distance='tree'`` walks one face octree per scene (``ctrees``: those of ``ops.metrics.closest_point_tree_build``, built here -- on
    ``trees`` where given -- when not): equal bits.  ``hand_upsample`` / ``hand_faces``: as in ``penetration_depth``."""
    from . import ops
    pts = upsample_hand(hand_verts, hand_faces, hand_upsample).float().contiguous()
    if distance == 'brute':
        d2 = ops.metrics.closest_point_mesh_scenes(meshes, pts, want_point=False).d2
    elif distance == 'tree':
        if ctrees is None:
            ctrees = [ops.metrics.closest_point_tree_build(v, f, tree=None if trees is None else trees[b]) for b, (v, f) in enumerate(meshes)]
        if winding == 'fast' and trees is None:
            trees = [c.tree for c in ctrees]
        d2 = ops.metrics.closest_point_tree_query_scenes(ctrees, pts, want_point=False).d2
    else:
        raise ValueError("distance must be 'brute' or 'tree'")
    if winding == 'exact':
        w = ops.winding_number_scenes(meshes, pts)
    elif winding == 'fast':
        w = ops.winding.query_scenes(trees if trees is not None else [ops.winding.build(v, f) for v, f in meshes], pts)
    else:
        raise ValueError("winding must be 'exact' or 'fast'")
    depth = _inside_depth(d2, w)
    return depth.cpu().numpy() * np.asarray(scales, dtype=np.float64)


def sample_mesh_surface(verts, faces, n, generator=None):
    """n area-weighted samples of a mesh's surface with torch ops on the mesh's device: the face by searchsorted on the cumulative
    areas, the point by square-root barycentrics (1 - sqrt(r1), sqrt(r1) (1 - r2), sqrt(r1) r2).  float64 arithmetic; returns
    (points [n,3] f32, face [n] int64).  ``generator``: a torch.Generator on that device (the default generator otherwise)."""
    v = verts.double()
    f = faces.long()
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    area = 0.5 * torch.linalg.cross(b - a, c - a).norm(dim=1)
    cum = torch.cumsum(area, dim=0)
    r = torch.rand((n, 3), dtype=torch.float64, device=v.device, generator=generator)
    face = torch.searchsorted(cum, r[:, 0] * cum[-1], right=True).clamp(max=f.shape[0] - 1)
    s = torch.sqrt(r[:, 1])
    w0, w1, w2 = (1 - s).unsqueeze(1), (s * (1 - r[:, 2])).unsqueeze(1), (s * r[:, 2]).unsqueeze(1)
    return (a[face] * w0 + b[face] * w1 + c[face] * w2).float(), face


def _closest_face(distance, verts, faces, pts):
    """(d2, face) of ``_distance2``'s call: the same kernels, the same bits, with the index of the closest face kept."""
    from . import ops
    if distance == 'brute':
        cp = ops.metrics.closest_point_mesh(verts.float(), faces, pts, want_point=False)
    elif distance == 'tree':
        cp = ops.metrics.closest_point_tree_query(ops.metrics.closest_point_tree_build(verts.float(), faces), pts, want_point=False)
    else:
        raise ValueError("distance must be 'brute' or 'tree'")
    return cp.d2, cp.face


def _face_normals(verts, faces):
    from . import ops
    return ops.mesh.normals(verts.float().contiguous(), faces.int().contiguous(), vertex=False).face_normals.double()


def mesh_distances(pred_mesh, gt_mesh, n, generator=None, threshold=0.01, distance='brute', normals=False):
    """Surface-to-surface distances of two meshes, each (verts [V,3] f32, faces [F,3] int) on the device: ``n`` area-weighted samples
    per mesh (``sample_mesh_surface``), every sample's distance to the OTHER mesh's surface (vt_closest_point_mesh) -- not to its
    vertices, so a dense mesh is not favoured.  Returns floats: 'accuracy' (mean distance of the predicted samples to the ground-truth
    mesh), 'completeness' (the other way), 'chamfer_l1' (their mean), 'f_score' (harmonic mean of the shares of samples within
    ``threshold``, precision and recall; 0 when both are 0).  ``distance='tree'`` takes the same distances from a walk of each mesh's face
    octree (vt_closest_tree_query: equal bits, far fewer faces per sample on a large mesh).

    ``normals=True`` adds the normal consistency of the ConvONet evaluation, from the same samples: 'normals_accuracy', the mean of
    |n_sample . n_closest| over the predicted samples -- n_sample the unit normal of the sampled face, n_closest that of the face of the
    other mesh the closest point lies on (vt_mesh_normals; a degenerate face counts as 0) --, 'normals_completeness', the same the
    other way round, and 'normals_consistency', their mean.  The absolute value makes it blind to the orientation of either mesh.  The
    four other keys are what the default call returns from the same generator state, bit for bit."""
    (pv, pf), (gv, gf) = pred_mesh, gt_mesh
    sp, fp = sample_mesh_surface(pv, pf, n, generator)
    sg, fg = sample_mesh_surface(gv, gf, n, generator)
    if normals:
        (d2_acc, near_g), (d2_comp, near_p) = _closest_face(distance, gv, gf, sp), _closest_face(distance, pv, pf, sg)
    else:
        d2_acc, d2_comp = _distance2(distance, gv, gf, sp), _distance2(distance, pv, pf, sg)
    acc = torch.sqrt(d2_acc)
    comp = torch.sqrt(d2_comp)
    precision, recall = float((acc <= threshold).double().mean()), float((comp <= threshold).double().mean())
    accuracy, completeness = float(acc.mean()), float(comp.mean())
    f_score = 2 * precision * recall / (precision + recall) if precision + recall > 0 else 0.0
    out = {'accuracy': accuracy, 'completeness': completeness, 'chamfer_l1': 0.5 * (accuracy + completeness), 'f_score': f_score}
    if normals:
        np_, ng = _face_normals(pv, pf), _face_normals(gv, gf)
        n_acc = float((np_[fp] * ng[near_g.long()]).sum(dim=1).abs().mean())
        n_comp = float((ng[fg] * np_[near_p.long()]).sum(dim=1).abs().mean())
        out.update({'normals_accuracy': n_acc, 'normals_completeness': n_comp, 'normals_consistency': 0.5 * (n_acc + n_comp)})
    return out


def mesh_distances_aligned(pred_mesh, gt_mesh, n, generator=None, threshold=0.01, max_iterations=20, tolerance=1e-3, distance='brute',
                           registration='brute', normals=False):
    """``mesh_distances`` after a rigid registration of the predicted mesh onto the ground truth, so that a pose offset of the prediction
    does not read as shape error.  Both surfaces are sampled exactly as ``mesh_distances`` samples them; ``ops.icp.icp`` maps the
    predicted samples onto the ground-truth samples (vt_icp, float64); its T moves the predicted vertices, per component
    ((T00 x + T01 y) + T02 z) + T03 in float64, rounded to float32.  Returns ``mesh_distances`` of the moved mesh against the ground truth
    from the same random draws (the generator is put back to where the sampling began, so it ends where one ``mesh_distances`` call
    leaves it), plus 'transform' (4x4 float64 numpy array) and 'icp_iterations' (int, the 0-based index of the last executed iteration).
    ``distance`` is ``mesh_distances``'; ``registration='tree'`` searches the loop's neighbours in an octree over the ground-truth
    samples (vt_icp_tree): the same transform, bit for bit.  ``normals`` is ``mesh_distances``': the sample normals are those of the moved
    mesh, that is, rotated with T."""
    from . import ops
    from ._lib import VtError
    if registration not in ('brute', 'tree'):
        raise VtError(f"mesh_distances_aligned: registration must be 'brute' or 'tree' (got {registration!r})")
    (pv, pf), (gv, gf) = pred_mesh, gt_mesh
    state = generator.get_state() if generator is not None else torch.cuda.get_rng_state(pv.device)
    sp, _ = sample_mesh_surface(pv, pf, n, generator)
    sg, _ = sample_mesh_surface(gv, gf, n, generator)
    fit = ops.icp.icp(sp, sg, max_iterations=max_iterations, tolerance=tolerance, method=registration)
    T, v = fit.T, pv.double()
    moved = torch.stack([((T[r, 0] * v[:, 0] + T[r, 1] * v[:, 1]) + T[r, 2] * v[:, 2]) + T[r, 3] for r in range(3)], dim=1).float()
    if generator is not None:
        generator.set_state(state)
    else:
        torch.cuda.set_rng_state(state, pv.device)
    out = mesh_distances((moved, pf), gt_mesh, n, generator, threshold, distance=distance, normals=normals)
    out['transform'] = T.cpu().numpy()
    out['icp_iterations'] = int(fit.iterations)
    return out
