"""GPU: utils/render.py (render_depth, simulate_touch, visible_points) and the Mesh methods on them, against tests/ray_mesh_ref.py's
camera and brute-force search.  The scenes are tests/render_cases.py's: the torus from five seeded sensor poses that look at it, at 24 x 32
and 5 x 7 pixels.  tests/test_ray_mesh_ref_cpu.py ties the restated camera to the reference's unprojection and checks the hit points of the
restatement on the CPU."""
import numpy as np
import pytest
import torch

import closest_point_ref as R
import closest_point_tree_ref as C
import ray_mesh_ref as M
import render_cases as RC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_scene = {}


def D(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _same_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape
    return np.array_equal(got.view(np.uint8), want.view(np.uint8))


def scene(height, width):
    """The torus, its poses and the restatement's render, computed once per size and left unchanged."""
    if (height, width) not in _scene:
        verts, faces = C.grid_mesh("torus")
        pos, rot = RC.aimed_poses(5, 2024)
        _, _, pose = RC.torus_scene()
        _scene[height, width] = (verts, faces, pos, rot, pose) + M.render(verts, faces, pose, width, height)
    return _scene[height, width]


@pytest.mark.parametrize("method", ["brute", "tree", None])
@pytest.mark.parametrize("height,width", RC.SIZES)
def test_torus_render_equals_the_restatement(height, width, method):
    from vtaco_amd.utils import render
    verts, faces, pos, rot, pose, s, face, _, _ = scene(height, width)
    depth, fmap = render.render_depth((D(verts), D(faces)), pos, rot, height=height, width=width, method=method)
    assert depth.shape == (5, height, width) and depth.dtype == torch.float32 and fmap.dtype == torch.int32
    assert np.array_equal(fmap.cpu().numpy().reshape(5, -1), face)
    assert _same_bits(depth.cpu().numpy().reshape(5, -1), M.depth_from_hits(s))
    hit = face >= 0
    assert hit.any(axis=1).all() and not hit.all()                     # every sensor sees the torus, and sky beside it


def test_camera_rays_equal_the_restatement():
    from vtaco_amd import ops
    for height, width in RC.SIZES + ((3, 300),):                        # 900 pixels: more than one block of 256
        _, _, pose = RC.torus_scene()
        pose[:, 12:15], pose[:, 15] = [0.01, -0.02, 0.03], 0.75         # a normalisation that is not the identity
        o, d = ops.rays.camera_rays(D(pose), width, height, 50.0)
        wo, wd = M.camera_rays(pose, width, height, 50.0)
        assert _same_bits(o.cpu().numpy(), wo) and _same_bits(d.cpu().numpy(), wd)


@pytest.mark.parametrize("height,width", RC.SIZES)
def test_hit_points_lie_on_the_mesh(height, width):
    """o + s d (float64, on the host, from the kernel's s) lies within the walk's slack E = 2^-40 S of the mesh: by_regions in float64 gives
    d2 <= E^2 (the bound tests/test_ray_mesh_ref_cpu.py meets on the restatement; S is the scene's size about the origin, the walk's own).
    ``closest_point_mesh`` takes float32 queries: the hit point rounded to float32 moved by r = |p - f32(p)|, which the host knows exactly,
    so the kernel's distance is held to E + r."""
    from vtaco_amd import ops
    verts, faces, pos, rot, pose, ws, wface, origins, dirs = scene(height, width)
    o, d = ops.rays.camera_rays(D(pose), width, height)
    s, face = ops.rays.ray_mesh(D(verts), D(faces), o, d.view(-1, 3), method='tree', rays_per_origin=height * width)
    s, face = s.cpu().numpy().reshape(5, -1), face.cpu().numpy().reshape(5, -1)
    assert _same_bits(s, ws) and np.array_equal(face, wface)
    hit = face >= 0
    pts = (origins[:, None, :] + s[:, :, None] * dirs)[hit]
    E = np.repeat(M.slack(C.build(verts, faces), origins), height * width).reshape(hit.shape)[hit]
    d2 = R.by_regions(verts, faces, pts)[0]
    assert (d2 <= E * E).all(), (np.sqrt(d2.max()), E.min())
    p32 = pts.astype(np.float32)
    r = np.sqrt(((pts - p32.astype(np.float64)) ** 2).sum(1))
    cp = ops.metrics.closest_point_mesh(D(verts), D(faces), D(p32), want_point=False)
    dist = np.sqrt(cp.d2.cpu().numpy())
    print(f"{height}x{width}: {int(hit.sum())} hits, max f64 distance {np.sqrt(d2.max()):.3g} (E {E.min():.3g}), max f32-query distance {dist.max():.3g}")
    assert (dist <= E + r).all(), (dist - r).max()


@pytest.mark.parametrize("height,width", RC.SIZES)
def test_round_trip_through_contact_scan_and_contact_points(height, width):
    """simulate_touch -> contact_scan -> contact_points gives back the hit points.  Per component a, with z = f32(s) the stored depth:
      * the depth's rounding moves the point by |d_a| |z - s| <= 2^-24 s |d_a|
      * vt_contact_points evaluates M cam z + t, the normalisation and the pinhole factors in float64, a dozen roundings of terms below
        |o_a| + s |d_a|: 2^-45 of that covers them (2^-45 = 256 u)
      * the row is stored as float32: 2^-24 |p_a| more
    so |row_a - p_a| <= 2^-24 (s |d_a| + |p_a|) + 2^-45 (|o_a| + s |d_a|), first order; the flat reading is 3.0 (beyond every hit) and
    near = 0, so every hit pixel is a touched pixel and none is clamped."""
    from vtaco_amd import ops
    from vtaco_amd.utils import render
    verts, faces, pos, rot, pose, s, face, origins, dirs = scene(height, width)
    npix = height * width
    flat = np.full(npix, 3.0)
    depth, touched = render.simulate_touch((D(verts), D(faces)), pos, rot, flat, near=0.0, height=height, width=width)
    assert depth.shape == (5, npix) and depth.dtype == torch.float32 and touched.dtype == torch.bool and touched.cpu().numpy().all()
    assert _same_bits(depth.cpu().numpy(), M.depth_from_hits(s, flat, 0.0))
    hit = face >= 0
    assert s[hit].max() < 2.9
    index, count = ops.contact_scan(depth, D(flat), None, 1e-4)
    cnt = count.cpu().numpy()
    assert np.array_equal(cnt, hit.sum(1))
    row0 = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.int32)
    total = int(cnt.sum())
    rows = torch.zeros((1, total, 3), dtype=torch.float32, device=DEV)
    ops.contact_points(depth, index, None, count, D(row0), D(pose), width, height, 60.0, npix, rows)
    got = rows.cpu().numpy()[0].astype(np.float64)
    want = (origins[:, None, :] + s[:, :, None] * dirs)[hit]             # image by image, pixels ascending: the rows' order
    reach = (s[:, :, None] * np.abs(dirs))[hit]
    tol = 2.0 ** -24 * (reach + np.abs(want)) + 2.0 ** -45 * (np.abs(np.repeat(origins[:, None, :], npix, axis=1))[hit] + reach)
    print(f"{height}x{width}: {total} rows, max |row - p| / tol = {(np.abs(got - want) / tol).max():.3g}")
    assert (np.abs(got - want) <= tol).all()


def test_touch_fails_for_a_sensor_that_faces_away_and_depths_stay_in_range():
    from vtaco_amd.utils import render
    verts, faces = C.grid_mesh("torus")
    height, width = RC.SIZES[0]
    flat = np.full(height * width, 1.25)
    flat[::7] = 1.0                                                     # a reading that differs from pixel to pixel
    pos, rot = RC.aimed_poses(5, 2024, away=True)
    depth, touched = render.simulate_touch((D(verts), D(faces)), pos, rot, flat, near=0.9, height=height, width=width)
    assert not touched.cpu().numpy().any() and np.array_equal(depth.cpu().numpy(), np.tile(flat.astype(np.float32), (5, 1)))
    pos, rot = RC.aimed_poses(5, 2024)
    pos[4], rot[4] = RC.aimed_poses(5, 2024, away=True)[0][4], RC.aimed_poses(5, 2024, away=True)[1][4]
    depth, touched = render.simulate_touch((D(verts), D(faces)), pos, rot, flat, near=0.9, height=height, width=width)
    z = depth.cpu().numpy()
    assert touched.cpu().numpy().tolist() == [True, True, True, True, False]
    assert (z >= np.float32(0.9)).all() and (z <= flat.astype(np.float32)[None, :]).all()
    assert (z == np.float32(0.9)).any() and ((z > np.float32(0.9)) & (z < flat.astype(np.float32)[None, :])).any()
    _, _, _, _, _, s, _, _, _ = scene(height, width)
    assert _same_bits(z[:4], M.depth_from_hits(s[:4], flat, 0.9))


def test_visible_points_on_the_torus():
    """Seen from (2, 0, 0.5): the vertices of the outer equator that face the eye are visible; the inner-equator vertices across the tube
    from them are hidden by the tube."""
    from vtaco_amd.utils import render
    verts, faces = C.grid_mesh("torus")
    v = verts.astype(np.float64)
    rad, ang = np.hypot(v[:, 0], v[:, 1]), np.arctan2(v[:, 1], v[:, 0])
    front = (np.abs(v[:, 2]) < 1e-6) & (np.abs(ang) < 1.0)
    outer, inner = front & (rad > 0.41), front & (rad < 0.19)
    assert outer.sum() >= 5 and outer.sum() == inner.sum()
    eye = np.array([2.0, 0.0, 0.5])
    for method in ("brute", "tree"):
        assert render.visible_points((D(verts), D(faces)), v[outer], eye, method=method).cpu().numpy().all()
        assert not render.visible_points((D(verts), D(faces)), v[inner], eye, method=method).cpu().numpy().any()
    assert render.visible_points((D(verts), D(faces)), verts[outer], eye).cpu().numpy().all()      # float32 points, converted exactly


def test_mesh_methods_return_what_the_functions_return():
    from vtaco_amd import ops
    from vtaco_amd.conv_onet.generation import Mesh
    from vtaco_amd.utils import render
    verts, faces, pos, rot, pose, s, face, _, _ = scene(5, 7)
    mesh = Mesh(D(verts), D(faces))
    o, d = M.grid_rays("torus", verts, faces, 70)
    got, want = mesh.ray_cast(D(o), D(d), bary=True), ops.rays.ray_mesh(D(verts), D(faces), D(o), D(d), bary=True)
    assert all(_same_bits(x.cpu().numpy(), y.cpu().numpy()) for x, y in zip(got, want))
    assert _same_bits(got[0].cpu().numpy(), M.brute(verts, faces, o, d)[0])
    got, want = mesh.render_depth(pos, rot, height=5, width=7), render.render_depth(mesh, pos, rot, height=5, width=7)
    assert all(_same_bits(x.cpu().numpy(), y.cpu().numpy()) for x, y in zip(got, want))
    flat = np.full(35, 2.0)
    got = mesh.simulate_touch(pos, rot, flat, near=0.5, height=5, width=7)
    want = render.simulate_touch(mesh, pos, rot, flat, near=0.5, height=5, width=7)
    assert all(_same_bits(x.cpu().numpy(), y.cpu().numpy()) for x, y in zip(got, want))
    assert _same_bits(got[0].cpu().numpy(), M.depth_from_hits(s, flat, 0.5))
