"""The scenes tests/test_ray_mesh_ref_cpu.py and tests/test_render_depth_gpu.py render: the torus of the closest-point tests seen from five
seeded sensor poses that look at it (the camera axis of pose i passes through a point of the tube's centre circle), and one that looks away."""
import numpy as np

import closest_point_tree_ref as C

SIZES = ((24, 32), (5, 7))          # (height, width)


def aimed_poses(n, seed, away=False):
    """(cam_pos, cam_rot) [n,3]: seeded rotations; the position puts the camera 0.9 .. 1.3 axis lengths from its target, on the axis."""
    from vtaco_amd.common import sensor_pose_inverse
    rng = np.random.RandomState(seed)
    rot = rng.uniform(-np.pi, np.pi, size=(n, 3))
    ang = rng.uniform(0.0, 2.0 * np.pi, size=n)
    target = np.stack([0.30 * np.cos(ang), 0.30 * np.sin(ang), np.zeros(n)], axis=1)
    pos = np.zeros((n, 3))
    for i in range(n):
        axis = sensor_pose_inverse(np.zeros(3), rot[i])[0][:, 0]         # the direction of the centre pixel's ray
        pos[i] = target[i] - (-1.0 if away else 1.0) * rng.uniform(0.9, 1.3) * axis
    return pos, rot


def torus_scene(away=False):
    """(verts, faces, pose records [5,16]) in the mesh's own frame (centroid 0, scale 1)."""
    from vtaco_amd.utils import render
    verts, faces = C.grid_mesh("torus")
    pos, rot = aimed_poses(5, 2024, away)
    return verts, faces, render.pose_records(pos, rot)
