"""GPU: vt_ray_mesh / vt_ray_tree_query through ``ops.rays`` against tests/ray_mesh_ref.py (the numpy restatement of the rule, the brute-force
search and the walk).

s, face, the weights and the two statistics (boxes tested, faces tested) are compared with the restatement for EQUAL BITS, no element left
out; s, face and the weights of the tree kernel also with the brute-force kernel on the same inputs: both call one rf_face, and the walk skips
a cell only when the ray's remaining segment misses its grown box.  tests/test_ray_mesh_ref_cpu.py holds the restatement's walk to its
brute-force search, and that to Moller-Trumbore, on the same inputs."""
import math

import numpy as np
import pytest
import torch

import ray_mesh_ref as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INPUTS = {name: rest for name, *rest in M.named_inputs()}


def D(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _same_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape
    return np.array_equal(got.view(np.uint8), want.view(np.uint8))


def _host(out):
    return tuple(x.cpu().numpy() for x in out)


def _tree_run(verts, faces, o, d, depth=None, strict=True, **kw):
    from vtaco_amd import ops
    ct = ops.metrics.closest_point_tree_build(D(verts), D(faces), depth)
    return _host(ops.rays.ray_tree_query(ct, D(o), D(d), bary=True, stats=True, strict=strict, **kw)), ct


def _brute_run(verts, faces, o, d, **kw):
    from vtaco_amd import ops
    return _host(ops.rays.ray_mesh(D(verts), D(faces), D(o), D(d), method='brute', bary=True, **kw))


def _check(verts, faces, o, d, depth=None, order=True, **kw):
    """The tree kernel against the restatement (statistics included) and against the brute-force kernel; that against its restatement."""
    (s, face, bary, stats), ct = _tree_run(verts, faces, o, d, depth, **kw)
    want = M.tree(verts, faces, o, d, depth, order=order, **kw)
    assert np.array_equal(face, want[1])
    assert _same_bits(s, want[0]) and _same_bits(bary, want[2])
    assert np.array_equal(stats, want[3]), (stats.sum(0), want[3].sum(0))
    b = _brute_run(verts, faces, o, d, **kw)
    assert _same_bits(s, b[0]) and _same_bits(face, b[1]) and _same_bits(bary, b[2])
    wb = M.brute(verts, faces, o, d, **kw)
    assert _same_bits(b[0], wb[0]) and _same_bits(b[1], wb[1]) and _same_bits(b[2], wb[2])
    return (s, face, bary, stats), ct


@pytest.mark.parametrize("depth", M.GRID_DEPTH)
@pytest.mark.parametrize("F", M.GRID_F + ("torus",))
def test_grid_of_sizes_equals_the_restatement_and_the_brute_force_kernel(F, depth):
    verts, faces, o, d, _ = INPUTS[f"grid-{F}-{depth}"]
    (s, face, _, _), _ = _check(verts, faces, o, d, depth)
    assert (face >= 0).sum() >= 100 and (face < 0).sum() >= 50


@pytest.mark.parametrize("name", ["leak-torus", "leak-box", "axis-torus", "axis-box"])
def test_no_ray_leaks_through_a_closed_mesh(name):
    verts, faces, o, d, depth = INPUTS[name]
    (s, face, _, _), _ = _check(verts, faces, o, d, depth)
    assert (face >= 0).all() and np.isfinite(s).all()                  # from both kernels: _check holds them equal


@pytest.mark.parametrize("swap", [False, True])
def test_equal_s_in_different_leaves_gives_the_lowest_face(swap):
    verts, faces, o, d, (i, j) = M.tie_pair(swap)
    (s, face, _, _), ct = _check(verts, faces, o, d, 2)
    assert s[0] == 0.75 and face[0] == i
    one = _brute_run(verts, faces[[i, j]], o, d)
    assert one[0][0] == 0.75 and one[1][0] == 0
    assert _brute_run(verts, faces[[j]], o, d)[0][0] == 0.75           # the higher face gives the same s on its own


def test_segment_limits():
    verts, faces, o, d, cases = M.segment_case()
    for t_min, t_max, want_s, want_face in cases:
        (s, face, _, _), _ = _check(verts, faces, o, d, 2, t_min=t_min, t_max=t_max)
        assert s[0] == want_s and face[0] == want_face, (t_min, t_max)
    verts, faces, o, d = M.behind_case()
    (s, face, _, _), _ = _check(verts, faces, o, d, 1)
    assert face[0] == -1 and s[0] == np.inf


def test_bad_rays_miss_and_the_launch_returns():
    verts, faces, o, d, depth = INPUTS["bad-rays"]
    (s, face, bary, stats), _ = _check(verts, faces, o, d, depth)
    assert (face[:8] == -1).all() and np.isinf(s[:8]).all() and np.isnan(bary[:8]).all() and (face[8:] >= 0).any()
    assert (stats[[0, 1, 2, 3, 4, 7]] == 0).all()                     # an invalid ray walks nothing


@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("kind", ["repeated", "collinear"])
def test_degenerate_faces_are_never_hit(kind, mixed):
    verts, faces, o, d, depth = INPUTS[f"degenerate-{kind}-{mixed}"]
    (s, face, _, _), _ = _check(verts, faces, o, d, depth)
    assert not np.isnan(s).any()
    if mixed:
        n_bad = 3 if kind == "repeated" else 2
        assert not ((face >= 150) & (face < 150 + n_bad)).any() and (face >= 0).any()
    else:
        assert (face == -1).all()


def test_a_face_with_a_bad_index_is_skipped_and_reported():
    from vtaco_amd import ops
    verts, faces, o, d, _ = INPUTS["bad-index"]
    with pytest.raises(ops.VtError, match="outside"):
        ops.rays.ray_mesh(D(verts), D(faces), D(o), D(d), method='brute')
    ct = ops.metrics.closest_point_tree_build(D(verts), D(faces))
    assert ct.status & 1
    with pytest.raises(ops.VtError, match="outside"):
        ops.rays.ray_tree_query(ct, D(o), D(d))
    s, face, bary, stats = _host(ops.rays.ray_tree_query(ct, D(o), D(d), bary=True, stats=True, strict=False))
    want = M.tree(verts, faces, o, d)
    assert _same_bits(s, want[0]) and _same_bits(face, want[1]) and _same_bits(bary, want[2]) and np.array_equal(stats, want[3])
    assert not np.isin(face, [9, 40]).any() and (face >= 0).any()
    # the brute-force kernel skips them too: its results are there behind the error
    lib = ops._lib.load()
    N, F = len(d), len(faces)
    ws = torch.zeros(lib.vt_ray_mesh_workspace_bytes(F, N) // 4, dtype=torch.int32, device=DEV)
    bs, bf = torch.empty(N, dtype=torch.float64, device=DEV), torch.empty(N, dtype=torch.int32, device=DEV)
    vd, fd, od, dd = D(verts), D(faces), D(o), D(d)
    assert lib.vt_ray_mesh(vd.data_ptr(), len(verts), fd.data_ptr(), F, od.data_ptr(), 1, dd.data_ptr(), N, 0.0, math.inf, bs.data_ptr(),
                           bf.data_ptr(), None, ws.data_ptr(), ws.numel() * 4, None) == 0
    torch.cuda.synchronize()
    assert int(ws[0].item()) == 1 and _same_bits(bs.cpu().numpy(), s) and _same_bits(bf.cpu().numpy(), face)


def test_one_leaf_holding_every_face():
    verts, faces, o, d, depth = INPUTS["one-leaf"]
    (_, face, _, stats), ct = _check(verts, faces, o, d, depth)
    assert ct.tree.counts[depth] == 1 and (face >= 0).any()
    assert np.isin(stats[:, 1], [0, len(faces)]).all()


def test_sparse_deep_tree():
    """65 faces at depth 7: a pyramid of 2 396 745 cells with at most 65 occupied leaves, long climbs between them."""
    verts, faces, o, d, depth = INPUTS["sparse-deep"]
    _, ct = _check(verts, faces, o, d, depth)
    assert ct.tree.depth == 7 and ct.tree.counts[7] <= 65


def test_two_runs_and_both_walks_give_equal_bits(monkeypatch):
    verts, faces, o, d, _ = INPUTS["grid-torus-None"]
    first, _ = _check(verts, faces, o, d)
    again, _ = _tree_run(verts, faces, o, d)
    assert all(_same_bits(x, y) for x, y in zip(first, again))
    b1, b2 = _brute_run(verts, faces, o, d), _brute_run(verts, faces, o, d)
    assert all(_same_bits(x, y) for x, y in zip(b1, b2))
    monkeypatch.setenv("VTACO_RAY_TREE_WALK", "plain")
    plain, _ = _check(verts, faces, o, d, order=False)
    assert all(_same_bits(x, y) for x, y in zip(first[:3], plain[:3]))
    assert plain[3][:, 0].sum() > first[3][:, 0].sum()                 # near children first tests fewer boxes
    monkeypatch.setenv("VTACO_RAY_TREE_WALK", "sideways")
    from vtaco_amd import ops
    with pytest.raises(ops.VtError, match="VTACO_RAY_TREE_WALK"):
        _tree_run(verts, faces, o, d)


def test_origins_may_be_shared_and_float32():
    from vtaco_amd import ops
    verts, faces = M.grid_mesh("torus")
    _, d = M.grid_rays("torus", verts, faces)
    o1 = np.array([[0.3, 0.0, 0.0]], dtype=np.float32)
    d32 = d.astype(np.float32)
    want = M.brute(verts, faces, o1.astype(np.float64), d32.astype(np.float64))
    for method in ('brute', 'tree'):
        s, face = _host(ops.rays.ray_mesh(D(verts), D(faces), D(o1), D(d32), method=method))
        assert _same_bits(s, want[0]) and _same_bits(face, want[1])
    assert (want[1] >= 0).all()                                         # the origin is inside the tube
    # blocks of rays per origin: 3 origins x 100 rays
    o3 = M.torus_inside()
    want = M.brute(verts, faces, np.repeat(o3, 100, axis=0), d)
    for method in ('brute', 'tree'):
        s, face = _host(ops.rays.ray_mesh(D(verts), D(faces), D(o3), D(d), method=method, rays_per_origin=100))
        assert _same_bits(s, want[0]) and _same_bits(face, want[1])


def test_a_tree_built_by_the_winding_number_is_reused():
    from vtaco_amd import ops
    verts, faces, o, d, _ = INPUTS["grid-torus-None"]
    wt = ops.winding.build(D(verts), D(faces))
    ct = ops.metrics.closest_point_tree_build(D(verts), D(faces), tree=wt)
    assert ct.tree is wt
    s, face = _host(ops.rays.ray_mesh(D(verts), D(faces), D(o), D(d), tree=ct))
    want = M.brute(verts, faces, o, d)
    assert _same_bits(s, want[0]) and _same_bits(face, want[1])
    # the closest point and the winding number still answer from the same buffers
    pts = D(verts[:16])
    assert ops.metrics.closest_point_tree_query(ct, pts).d2.max().item() == 0.0
    assert ops.winding.query(wt, D(M.torus_inside().astype(np.float32))).min().item() > 0.9


def test_empty_rays_and_bad_arguments():
    from vtaco_amd import ops
    lib = ops._lib.load()
    verts, faces = M.grid_mesh(65)
    vd, fd = D(verts), D(faces)
    e = torch.empty((0, 3), dtype=torch.float64, device=DEV)
    for method in ('brute', 'tree'):
        s, face, bary = ops.rays.ray_mesh(vd, fd, e, e, method=method, bary=True)
        assert s.shape == (0,) and face.shape == (0,) and bary.shape == (0, 3)
    ct = ops.metrics.closest_point_tree_build(vd, fd)
    t = ct.tree
    o, d = M.grid_rays(65, verts, faces, 8)
    od, dd = D(o), D(d)
    s, f = torch.empty(8, dtype=torch.float64, device=DEV), torch.empty(8, dtype=torch.int32, device=DEV)
    ws = torch.empty(lib.vt_ray_mesh_workspace_bytes(65, 8) // 4, dtype=torch.int32, device=DEV)
    INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3                      # VT_ERR_INVALID, VT_ERR_UNSUPPORTED, VT_ERR_WORKSPACE
    assert lib.vt_ray_mesh(None, 1, None, 1, None, 1, None, 0, 0.0, 1.0, None, None, None, None, 0, None) == INVALID

    def brute(V=len(verts), F=65, per=1, N=8, o_=od, s_=s, ws_bytes=ws.numel() * 4):
        return lib.vt_ray_mesh(vd.data_ptr(), V, fd.data_ptr(), F, o_.data_ptr() if o_ is not None else None, per, dd.data_ptr(), N, 0.0, math.inf,
                               s_.data_ptr() if s_ is not None else None, f.data_ptr(), None, ws.data_ptr(), ws_bytes, None)
    assert brute() == 0
    assert brute(V=0) == INVALID and brute(F=0) == INVALID and brute(N=-1) == INVALID and brute(per=0) == INVALID
    assert brute(o_=None) == INVALID and brute(s_=None) == INVALID
    assert brute(ws_bytes=64) == WORKSPACE
    assert lib.vt_ray_mesh_workspace_bytes(0, 8) == 0 and lib.vt_ray_mesh_workspace_bytes(65, -1) == 0

    def walk(depth=t.depth, F=65, per=1, N=8, tree_bytes=t.buf.numel() * 8, side_bytes=ct.side.numel() * 8, tree=t.buf.data_ptr(), d_=dd):
        return lib.vt_ray_tree_query(tree, tree_bytes, ct.side.data_ptr(), side_bytes, F, depth, t._state, od.data_ptr(), per,
                                     d_.data_ptr() if d_ is not None else None, N, 0.0, math.inf, s.data_ptr(), f.data_ptr(), None, None, None)
    assert walk() == 0
    assert walk(tree=None) == INVALID and walk(F=0) == INVALID and walk(N=-1) == INVALID and walk(per=0) == INVALID and walk(d_=None) == INVALID
    assert walk(depth=0) == UNSUPPORTED and walk(depth=8) == UNSUPPORTED
    assert walk(tree_bytes=64) == WORKSPACE and walk(side_bytes=64) == WORKSPACE
    assert walk(N=0, d_=None) == 0

    pose = torch.zeros((2, 16), dtype=torch.float64, device=DEV)
    pose[:, 15] = 1.0
    co, cd = torch.empty((2, 3), dtype=torch.float64, device=DEV), torch.empty((2, 12, 3), dtype=torch.float64, device=DEV)

    def cam(n=2, W=4, H=3, fov=60.0, p=pose.data_ptr(), o_=co.data_ptr()):
        return lib.vt_camera_rays(p, n, W, H, fov, o_, cd.data_ptr(), None)
    assert cam() == 0 and cam(n=0, p=None, o_=None) == 0
    assert cam(n=-1) == INVALID and cam(W=0) == INVALID and cam(H=-3) == INVALID and cam(fov=0.0) == INVALID and cam(fov=180.0) == INVALID
    assert cam(p=None) == INVALID and cam(o_=None) == INVALID
    assert lib.vt_depth_from_hits(None, None, 12, 4, 0.0, None, None) == INVALID and lib.vt_depth_from_hits(None, None, 0, 0, 0.0, None, None) == INVALID
    assert lib.vt_depth_from_hits(None, None, 12, 0, 0.0, None, None) == 0
    torch.cuda.synchronize()
    # the Python layer: wrong devices, shapes, dtypes, methods
    for bad in (lambda: ops.rays.ray_mesh(vd, fd, od.cpu(), dd), lambda: ops.rays.ray_mesh(vd, fd, od[:3], dd), lambda: ops.rays.ray_mesh(vd, fd, od, dd.int()),
                lambda: ops.rays.ray_mesh(vd, fd, od, dd, method='bvh'), lambda: ops.rays.ray_mesh(vd[:0], fd, od, dd), lambda: ops.rays.ray_tree_query(t, od, dd),
                lambda: ops.rays.ray_mesh(vd, fd[:10], od, dd, tree=ct), lambda: ops.rays.camera_rays(pose.float(), 4, 3)):
        with pytest.raises(ops.VtError):
            bad()
