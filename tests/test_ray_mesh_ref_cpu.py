"""CPU: tests/ray_mesh_ref.py, the numpy restatement of csrc/ray_face.h and csrc/ray_mesh.hip, held to itself and to an independent formula.
tests/test_ray_mesh_gpu.py and tests/test_render_depth_gpu.py hold the kernels to the restatement bit for bit on the same inputs.

  * the tree walk equals the brute-force search bit for bit (s, face, weights), for both walks, on every input the GPU tests use
  * float64 Moller-Trumbore picks the same face and an s within the bound derived below
  * no ray shot from inside a closed mesh, or along an axis exactly through one of its vertices or edges, misses
  * ``camera_rays`` inverts the unprojection tests/tactile_pc_rule.py restates from the reference (pinned by g24_tactile_pc.npz)
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import closest_point_ref as R
import closest_point_tree_ref as C
import ray_mesh_ref as M

U = 2.0 ** -53
INPUTS = {name: rest for name, *rest in M.named_inputs()}


def _same_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape
    return np.array_equal(got.view(np.uint8), want.view(np.uint8))


@pytest.mark.parametrize("name", sorted(INPUTS))
def test_tree_equals_brute_bit_for_bit(name):
    verts, faces, o, d, depth = INPUTS[name]
    s, face, bary = M.brute(verts, faces, o, d)
    t = C.build(verts, faces, depth)
    for order in (True, False):
        ts, tface, tbary, stats = M.tree_query(t, verts, faces, o, d, order=order)
        assert _same_bits(ts, s) and _same_bits(tface, face) and _same_bits(tbary, bary), (name, order)
        assert (stats[:, 1] <= len(faces)).all()
    assert np.isinf(s[face < 0]).all() and np.isnan(bary[face < 0]).all() and not np.isnan(s).any()
    assert np.isfinite(bary[face >= 0]).all()


def test_segment_limits_tree_and_brute():
    verts, faces, o, d, cases = M.segment_case()
    for t_min, t_max, want_s, want_face in cases:
        for depth in (1, 2):
            s, face, _ = M.brute(verts, faces, o, d, t_min, t_max)
            ts, tface, _, _ = M.tree(verts, faces, o, d, depth, t_min=t_min, t_max=t_max)
            assert s[0] == want_s and face[0] == want_face, (t_min, t_max, s, face)
            assert _same_bits(ts, s) and _same_bits(tface, face)
    verts, faces, o, d = M.behind_case()
    assert M.brute(verts, faces, o, d)[1][0] == -1 and M.tree(verts, faces, o, d, 1)[1][0] == -1


@pytest.mark.parametrize("swap", [False, True])
def test_equal_s_in_different_leaves_gives_the_lowest_face(swap):
    verts, faces, o, d, (i, j) = M.tie_pair(swap)
    t = C.build(verts, faces, 2)
    assert t.codes[i] != t.codes[j]                                     # the two faces lie in different leaves
    a, b, c, valid = M.corners(verts, faces)
    S = M.pairs(M.setup(o, d), a, b, c, valid)
    assert S[0, i] == 0.75 and S[0, j] == 0.75
    for order in (True, False):
        s, face, _, _ = M.tree_query(t, verts, faces, o, d, order=order)
        assert s[0] == 0.75 and face[0] == i


def test_degenerate_faces_are_never_hit():
    for kind in ("repeated", "collinear"):
        verts, faces, o, d, _ = INPUTS[f"degenerate-{kind}-False"]
        s, face, _ = M.brute(verts, faces, o, d)
        assert (face == -1).all() and np.isinf(s).all()
        verts, faces, o, d, _ = INPUTS[f"degenerate-{kind}-True"]
        s, face, _ = M.brute(verts, faces, o, d)
        n_bad = 3 if kind == "repeated" else 2
        assert not ((face >= 150) & (face < 150 + n_bad)).any() and (face >= 0).any() and not np.isnan(s).any()


def test_bad_rays_and_bad_indices():
    verts, faces, o, d, _ = INPUTS["bad-rays"]
    s, face, _ = M.brute(verts, faces, o, d)
    assert (face[:8] == -1).all() and np.isinf(s[:8]).all() and (face[8:] >= 0).any()
    verts, faces, o, d, _ = INPUTS["bad-index"]
    s, face, _ = M.brute(verts, faces, o, d)
    assert not np.isin(face, [9, 40]).any() and (face >= 0).any()
    keep = np.setdiff1d(np.arange(len(faces)), [9, 40])
    s2, face2, _ = M.brute(verts, faces[keep], o, d)
    assert _same_bits(s, s2) and np.array_equal(face, np.where(face2 >= 0, keep[np.maximum(face2, 0)], -1))


@pytest.mark.parametrize("F", M.GRID_F + ("torus",))
def test_moller_trumbore_agrees(F):
    """The same face, and |s - s_MT| <= 256 u K.  Both formulas are s = (n . (a - o)) / (n . d), n the face's normal, in other operation
    orders.  With M = |a - o| + |s| |d| + the face's longest edge (everything either formula subtracts is below it), e = |ab| + |ac|:
      Moller-Trumbore  two cross products and two dots of vectors below M, e and |d|: numerator and denominator each carry at most
                       ~30 u M e^2 and ~30 u |d| e^2 (3 terms per dot, 2 products per cross component, the rounded edges), so
                       |ds| <= 60 u M e^2 / |n . d|
      the rule         ("ray_mesh.hip") s = sum w_i z_i + 9 u M / max|d_a|, and the computed weights differ from the exact ones
                       by 3 (4 u R^2 + 24 u R M) / |det| with R <= 2 e the sheared corners' distance from the ray, det = (n . d) / d_kz,
                       times the spread of the z_i, <= e / |d_kz|: |ds| <= 168 u M e^2 / |n . d| + 9 u M / max|d_a|
    so K = M (e^2 / |n . d| + 1 / max|d_a|) and 60 + 168 + 9 < 256.  Rays whose smallest weight is below 1e-9 (a hit on an edge: the two
    formulas may take either neighbour) are left out, at most 1 % of the case's rays."""
    verts, faces = M.grid_mesh(F)
    o, d = M.grid_rays(F, verts, faces)
    s, face, bary = M.brute(verts, faces, o, d)
    ms, mface, mweight = M.moller_trumbore(verts, faces, o, d)
    with np.errstate(invalid="ignore"):
        edge = ((face >= 0) & (np.nanmin(np.where(np.isnan(bary), np.inf, bary), axis=1) < 1e-9)) | ((mface >= 0) & (mweight < 1e-9))
    assert edge.sum() <= 0.01 * len(d), edge.sum()
    keep = ~edge
    assert np.array_equal(face[keep] >= 0, mface[keep] >= 0)
    hit = keep & (face >= 0)
    corner_sets = np.sort(np.asarray(faces), axis=1)                    # (a soup repeats a triangle at two indices: either index is that face)
    assert np.array_equal(corner_sets[face[hit]], corner_sets[mface[hit]])
    assert hit.sum() >= len(d) // 3
    v = verts.astype(np.float64)
    a, b, c = (v[faces[face[hit]][:, k]] for k in range(3))
    nrm = np.cross(b - a, c - a)
    e = np.linalg.norm(b - a, axis=1) + np.linalg.norm(c - a, axis=1)
    dd = d[hit]
    reach = np.linalg.norm(a - o[hit], axis=1) + np.abs(s[hit]) * np.linalg.norm(dd, axis=1) + e
    K = reach * (e * e / np.abs((nrm * dd).sum(1)) + 1.0 / np.abs(dd).max(axis=1))
    ratio = np.abs(s[hit] - ms[hit]) / (U * K)
    print(f"F={F}: {int(hit.sum())} hits, {int(edge.sum())} left out, max |ds| / (u K) = {ratio.max():.3g}")
    assert (ratio <= 256.0).all(), ratio.max()


LEAKS = ("leak-torus", "leak-box", "axis-torus", "axis-box")


@pytest.mark.parametrize("name", LEAKS)
def test_no_ray_leaks_through_a_closed_mesh(name):
    """From points inside the closed torus and the closed box of 12 triangles: at every vertex, at every edge midpoint, along the three axes
    both ways and 2 000 seeded random directions; and axis-parallel lines exactly through every vertex and every exactly representable
    edge midpoint.  Every ray hits: zero misses."""
    verts, faces, o, d, _ = INPUTS[name]
    s, face, _ = M.brute(verts, faces, o, d)
    assert len(d) > 100 and (face >= 0).all(), np.nonzero(face < 0)[0][:10]
    assert (s > 0).all() and np.isfinite(s).all()


def test_the_box_is_hit_on_edges_and_corners_exactly():
    """Exact arithmetic: from the centre of the box along the axes (through the faces' diagonals) and at the corners."""
    verts, faces = M.box12()
    o = np.zeros((1, 3))
    d = np.concatenate([np.eye(3), -np.eye(3), verts.astype(np.float64)])
    s, face, bary = M.brute(verts, faces, o, d)
    assert (face >= 0).all()
    assert np.array_equal(s[:6], np.abs(verts.astype(np.float64)).max(0)[[0, 1, 2, 0, 1, 2]]) and (s[6:] == 1.0).all()
    assert (np.sort(bary[6:], axis=1) == np.array([0.0, 0.0, 1.0])).all()                 # a corner: one weight is 1


@pytest.mark.parametrize("height,width", [(240, 320), (5, 7)])
def test_camera_rays_invert_the_reference_unprojection(height, width):
    """pixel (u, v) at depth z: tactile_pc_rule.tactile_pc's point equals origin + z dir to 1e-12 of the scene's size."""
    import tactile_pc_rule as TP
    from vtaco_amd.utils import render
    rng = np.random.RandomState(240 + height)
    n = 5
    pred = rng.rand(n, height * width).astype(np.float32)
    cam_pos, cam_rot = rng.uniform(-0.3, 0.3, size=(n, 3)), rng.uniform(-np.pi, np.pi, size=(n, 3))
    pc_ply = (rng.rand(500, 3).astype(np.float32) - np.float32(0.5)) * np.float32(0.2)
    want = TP.tactile_pc(pred, height, width, cam_pos, cam_rot, pc_ply)
    pose = render.pose_records(cam_pos, cam_rot, pc_ply)
    origins, dirs = M.camera_rays(pose, width, height, float(TP.FOV))
    depth = (pred * np.float32(0.005) + np.float32(0.019)).astype(np.float64)
    got = origins[:, None, :] + depth[:, :, None] * dirs
    size = np.abs(want).max()
    assert np.abs(got - want).max() <= 1e-12 * size, (np.abs(got - want).max(), size)


def test_depth_from_hits_rule():
    s = np.array([0.5, np.inf, 0.01, 0.02, 0.3])
    origin = np.array([0.02, 0.02, 0.02, 0.02, 0.25])
    assert np.array_equal(M.depth_from_hits(s, origin, 0.019), np.array([0.02, 0.02, 0.019, 0.02, 0.25], dtype=np.float32))
    assert np.array_equal(M.depth_from_hits(s), np.array([0.5, np.inf, 0.01, 0.02, 0.3], dtype=np.float32))


def test_rendered_hit_points_lie_on_the_mesh():
    """The precondition of tests/test_render_depth_gpu.py's hit-point check, on the restatement: o + s d lies within the walk's slack E of
    the face that was hit (closest_point_ref.by_regions in float64)."""
    import render_cases as RC
    for height, width in RC.SIZES:
        verts, faces, pose = RC.torus_scene()
        s, face, origins, dirs = M.render(verts, faces, pose, width, height)
        hit = face >= 0
        assert hit.any() and not hit.all()
        pts = (origins[:, None, :] + s[:, :, None] * dirs)[hit]
        d2 = R.by_regions(verts, faces, pts)[0]
        E = np.repeat(M.slack(C.build(verts, faces), origins), height * width).reshape(hit.shape)[hit]
        assert (d2 <= E * E).all(), (np.sqrt(d2.max()), E.min())
