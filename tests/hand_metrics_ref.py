"""The hand terms of the reference's eval_step (src/conv_onet/training.py:393-419) restated in numpy, in the reference's own operation
order, at a chosen arithmetic ``dtype`` (float64: the reference for the tests; float32: the same run in single precision, whose distance
from the float64 run is the scale of the float32-level gate).

  chamfer_distance   chamfer_distance(pc_hand, pc_pred, use_kdtree=False): the naive form (common.py:69-91), pc_hand cut to the prediction's
                     point count
  hand_joints_error  np.mean(np.linalg.norm(j_gt - j_pred, axis=1)) (common.py:142-154)
  penetration_depth  the predicted vertices out of the MANO frame and the wrist rotation, plus the wrist position, norm_pc_1; winding
                     numbers against the object mesh (the exact sum igl.fast_winding_number_for_meshes approximates, fed float32 points as
                     there); 0 when none exceeds 0.5, otherwise the largest closest-point distance of those vertices (the float64
                     restatement of tests/closest_point_ref.py where the reference calls trimesh.proximity.closest_point) times
                     max ||pc_ply||
"""
import numpy as np

import closest_point_ref as C


def r_from_pyr(roll, pitch, yaw):
    """R_from_PYR (common.py:591-604)."""
    cr, sr, cp, sp, cy, sy = np.cos(roll), np.sin(roll), np.cos(pitch), np.sin(pitch), np.cos(yaw), np.sin(yaw)
    about_z = np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]])
    about_x_t = np.array([[1, 0, 0], [0, cp, sp], [0, -sp, cp]])
    about_y_t = np.array([[cy, 0, -sy], [0, 1, 0], [sy, 0, cy]])
    return about_x_t @ about_y_t @ about_z


def chamfer_naive(points1, points2, dtype=np.float64):
    """common.py:69-91 for one scene: [T1,3], [T,3] -> the Chamfer distance in ``dtype``."""
    p1, p2 = np.asarray(points1).astype(dtype), np.asarray(points2).astype(dtype)
    if p2.shape[0] < 2048:
        p1 = p1[:p2.shape[0]]
    assert p1.shape == p2.shape
    d = ((p1[:, None, :] - p2[None, :, :]) ** 2).sum(-1)
    return d.min(axis=0).mean(dtype=dtype) + d.min(axis=1).mean(dtype=dtype)


def hand_joint_error(joints_gt, joints_pred, dtype=np.float64):
    return np.mean(np.linalg.norm(np.asarray(joints_gt).astype(dtype) - np.asarray(joints_pred).astype(dtype), axis=1), dtype=dtype)


def hand_to_object_frame(verts, wrist_pos, wrist_euler, pc_ply, dtype=np.float64):
    """training.py:399-404: rows times the transposed inverses, one rotation after the other, then norm_pc_1 (common.py:606-612)."""
    v = np.asarray(verts, dtype=np.float32) - np.array([0.11, 0.005, 0], dtype=np.float32)
    v = np.dot(v.astype(dtype), np.linalg.inv(r_from_pyr(-np.pi / 2, np.pi / 2, 0)).T.astype(dtype))
    v = np.dot(v, np.linalg.inv(r_from_pyr(*np.asarray(wrist_euler))).T.astype(dtype))     # (the angles in the loader's dtype, as R_from_PYR gets them)
    v = v + np.asarray(wrist_pos).astype(dtype)
    cloud = np.asarray(pc_ply)                          # norm_pc_1 runs in the cloud's own dtype (float32 from the loader)
    centroid = np.mean(cloud, axis=0)
    m = np.max(np.sqrt(np.sum((cloud - centroid) ** 2, axis=1)))
    return ((v - centroid) / (2 * m)).astype(dtype)


def winding_number(verts, faces, pts, dtype=np.float64):
    """w(q) = 1 / (4 pi) sum_f Omega_f(q), Van Oosterom-Strackee solid angles."""
    v = np.asarray(verts, dtype=np.float32).astype(dtype)
    f = np.asarray(faces).astype(np.int64)
    p = np.asarray(pts).astype(dtype)[:, None, :]
    a, b, c = v[f[:, 0]][None] - p, v[f[:, 1]][None] - p, v[f[:, 2]][None] - p
    la, lb, lc = np.linalg.norm(a, axis=-1), np.linalg.norm(b, axis=-1), np.linalg.norm(c, axis=-1)
    num = (a * np.cross(b, c)).sum(-1)
    den = la * lb * lc + (a * b).sum(-1) * lc + (b * c).sum(-1) * la + (c * a).sum(-1) * lb
    return (2.0 * np.arctan2(num, den)).sum(-1) / dtype(4.0 * np.pi)


def penetration_depth(hand_verts, mesh_v, mesh_f, scale, dtype=np.float64):
    """training.py:406-419 on hand vertices already in the mesh's frame."""
    pts = np.asarray(hand_verts).astype(dtype)
    inside = winding_number(mesh_v, mesh_f, pts.astype(np.float32), dtype) > 0.5
    if not inside.any():
        return dtype(0.0)
    d2, _, _ = C.by_parts(mesh_v, mesh_f, pts[inside], dtype=dtype)
    return dtype(np.sqrt(d2.astype(dtype)).max() * dtype(scale))


def hand_metrics(pc_hand, mano_verts, joints_gt, joints_pred, wrist_pos, wrist_euler, pc_ply, meshes, dtype=np.float64):
    """The three eval_step terms, each the mean over the batch's scenes; ``meshes`` = [(verts, faces)] per scene."""
    B = len(meshes)
    chamfer, joints, depth = [], [], []
    for b in range(B):
        chamfer.append(chamfer_naive(pc_hand[b], mano_verts[b], dtype))
        joints.append(hand_joint_error(joints_gt[b], joints_pred[b], dtype))
        verts = hand_to_object_frame(mano_verts[b], wrist_pos[b], wrist_euler[b], pc_ply[b], dtype)
        scale = np.max(np.sqrt(np.sum(np.asarray(pc_ply[b]) ** 2, axis=1)))
        depth.append(penetration_depth(verts, meshes[b][0], meshes[b][1], scale, dtype))
    return {"chamfer_distance": float(np.mean(chamfer)), "hand_joints_error": float(np.mean(joints)), "penetration_depth": float(np.mean(depth)),
            "per_scene_depth": [float(x) for x in depth]}
