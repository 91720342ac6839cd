"""CPU: the definition of the edge-collapse decimation (tests/mesh_collapse_ref.py) alone: closed meshes stay closed, oriented manifolds
with their Euler numbers and components and land on the count; what must not move does not; the row-wise solve is mesh_simplify_ref's;
and the names the device side adds are bound."""
import inspect
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mesh_collapse_ref as C  # noqa: E402
import mesh_simplify_ref as S  # noqa: E402
import mesh_topo_ref as T  # noqa: E402


def _two_tori():
    v, f = T.torus(16, 32)
    return C.together(T.torus(8, 16), (v + np.float32(4.0), f))


CLOSED = {"torus8x16": (lambda: T.torus(8, 16), 100), "torus16x32": (lambda: T.torus(16, 32), 300), "two_tori": (_two_tori, 201),
          "octahedron": (C.octahedron, 6)}


def _no_shared_face(faces, u, v):
    """The hook: no face holds an end of two selected edges."""
    owner = np.full(int(faces.max()) + 1, -1)
    owner[u] = np.arange(u.shape[0])
    owner[v] = np.arange(v.shape[0])
    assert np.unique(np.concatenate([u, v])).shape[0] == 2 * u.shape[0]
    o = owner[faces]
    for a, b in ((0, 1), (1, 2), (0, 2)):
        assert not ((o[:, a] >= 0) & (o[:, b] >= 0) & (o[:, a] != o[:, b])).any()


@pytest.mark.parametrize("name", sorted(CLOSED))
@pytest.mark.parametrize("placement", C.PLACEMENTS)
def test_closed_meshes_stay_closed_manifolds_and_land_on_the_count(name, placement):
    make, nfaces = CLOSED[name]
    v, f = make()
    out = C.collapse(v, f, nfaces, placement=placement, hook=_no_shared_face)
    before, after = T.topo(v, f), T.topo(out["vertices"], out["faces"])
    assert not out["stalled"] and out["rounds"] >= 1
    assert out["faces"].shape[0] == nfaces - nfaces % 2 and out["faces"].dtype == np.int32 and out["vertices"].dtype == v.dtype
    assert after["oriented"].all() and (after["n_boundary"] == 0).all() and (after["n_nonmanifold"] == 0).all() and (after["n_misoriented"] == 0).all()
    assert after["n_components"] == before["n_components"] and np.array_equal(np.sort(after["euler"]), np.sort(before["euler"]))
    # vertex_map: onto the output vertices, and a survivor keeps its place in ascending order
    vmap, K = out["vertex_map"], out["vertices"].shape[0]
    assert vmap.dtype == np.int32 and vmap.min() >= 0 and np.array_equal(np.unique(vmap), np.arange(K))
    survivors = np.array([np.nonzero(vmap == k)[0].min() for k in range(K)])
    assert (np.diff(survivors) > 0).all()
    if placement == "midpoint":                     # every merged vertex is a midpoint of midpoints: inside the hull of its sources
        for k in range(K):
            src = v[vmap == k].astype(np.float64)
            assert (out["vertices"][k] >= src.min(0) - 1e-6).all() and (out["vertices"][k] <= src.max(0) + 1e-6).all()


def test_midpoint_positions_of_one_round_are_the_exact_midpoints():
    v, f = T.torus(8, 16)
    v = v.astype(np.float64)
    out = C.collapse(v, f, 100, placement="midpoint", max_rounds=1)
    assert out["rounds"] == 1
    vmap = out["vertex_map"]
    merged = 0
    for k in range(out["vertices"].shape[0]):
        src = np.nonzero(vmap == k)[0]
        assert src.shape[0] in (1, 2)
        if src.shape[0] == 2:
            c = 0.5 * v.min(0) + 0.5 * v.max(0)
            want = c + ((v[src[0]] - c) + (v[src[1]] - c)) * 0.5
            assert out["vertices"][k].tobytes() == want.tobytes()
            assert np.abs(out["vertices"][k] - 0.5 * (v[src[0]] + v[src[1]])).max() <= 2.0 ** -50
            merged += 1
        else:
            assert out["vertices"][k].tobytes() == v[src[0]].tobytes()
    assert merged == (f.shape[0] - out["faces"].shape[0]) // 2 >= 1


def test_max_rounds_bounds_the_rounds_and_the_rounds_are_a_prefix():
    v, f = T.torus(8, 16)
    one, two, full = (C.collapse(v, f, 100, max_rounds=r) for r in (1, 2, None))
    assert (one["rounds"], two["rounds"]) == (1, 2) and full["rounds"] > 2
    assert f.shape[0] > one["faces"].shape[0] > two["faces"].shape[0] > full["faces"].shape[0] == 100
    # what is merged after one round stays merged
    assert all(np.unique(two["vertex_map"][one["vertex_map"] == k]).shape[0] == 1 for k in range(one["vertices"].shape[0]))


def test_tetrahedron_stalls_unchanged():
    v, f = T.tetrahedron()
    out = C.collapse(v, f, 2)
    assert out["stalled"] and out["rounds"] == 0 and np.array_equal(out["faces"], f) and out["vertices"].tobytes() == v.tobytes()


@pytest.mark.parametrize("n", [2, 64, 257])
def test_a_strip_is_all_boundary_and_stalls_unchanged(n):
    v, f = T.grid_strip(n)
    out = C.collapse(v, f, 1)
    assert out["stalled"] and out["rounds"] == 0 and np.array_equal(out["faces"], f)
    assert out["vertices"].tobytes() == v[:out["vertices"].shape[0]].tobytes()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_open_patch_keeps_its_boundary_vertex_for_vertex(dtype):
    v, f = C.quad_patch(12, dtype)
    n = 13
    i, j = np.divmod(np.arange(n * n), n)
    rim = np.nonzero((i == 0) | (i == n - 1) | (j == 0) | (j == n - 1))[0]
    out = C.collapse(v, f, 100)
    assert out["faces"].shape[0] == 100 and not out["stalled"]
    at = out["vertex_map"][rim]
    assert (np.diff(at) > 0).all() and out["vertices"][at].tobytes() == v[rim].tobytes()
    assert all((out["vertex_map"] == k).sum() == 1 for k in at)          # nothing merged into the rim
    after = T.topo(out["vertices"], out["faces"])
    assert after["n_boundary"][0] == 48 and after["euler"][0] == 1 and after["n_nonmanifold"][0] == 0
    assert out["vertices"].shape[0] < v.shape[0]


def test_the_ends_of_a_fin_never_merge():
    v, f, (a, b) = C.fin_mesh()
    out = C.collapse(v, f, 30)
    vmap = out["vertex_map"]
    assert out["rounds"] >= 1 and vmap[a] != vmap[b]
    assert (vmap == vmap[a]).sum() == 1 and (vmap == vmap[b]).sum() == 1 and out["vertices"][vmap[a]].tobytes() == v[a].tobytes()
    assert T.topo(out["vertices"], out["faces"])["n_nonmanifold"][0] == 1


def test_a_zero_area_face_beside_the_surface_does_not_block_its_neighbours():
    v, f = T.torus(8, 16)
    extra = np.array([[5, 5, 40], [7, 60, 60]], dtype=np.int32)                     # two equal corners each: no edge, no vote
    out = C.collapse(v, np.concatenate([f[:50], extra, f[50:]]), 102)
    assert not out["stalled"] and out["faces"].shape[0] == 102
    proper = C.proper_faces(out["faces"].astype(np.int64))
    assert (~proper).sum() == 2
    closed = T.topo(out["vertices"], out["faces"][proper])
    assert closed["oriented"].all() and closed["euler"][0] == 0


def test_a_face_without_area_has_no_say_on_flips():
    """A proper face with n_old = (0, 0, 0) in a closed mesh: with a vote its dot product, 0, would refuse every collapse that moves
    one of its corners and leaves it alive.  Such edges are candidates in round 1, and the mesh ends as the others do."""
    v, f, corners = C.sliver_torus()
    P = v.astype(np.float64)
    assert all(float(np.abs(n[0])) == 0.0 for n in C.face_normals_raw(P[f[:1, 0]], P[f[:1, 1]], P[f[:1, 2]]))
    assert C.proper_faces(f.astype(np.int64))[0] and np.unique(P[list(corners)], axis=0).shape[0] == 3
    lo, hi = P.min(0), P.max(0)
    c = 0.5 * lo + 0.5 * hi
    for placement in C.PLACEMENTS:
        cand = C.select(P, C.initial_quadrics(P, f.astype(np.int64), c), c, f.astype(np.int64), 1, placement)["candidates"]
        one_end = np.isin(cand, corners).sum(1) == 1            # the face survives these and has one corner moved
        assert one_end.sum() >= 3, (placement, int(one_end.sum()))
    out = C.collapse(v, f, 60, hook=_no_shared_face)
    after = T.topo(out["vertices"], out["faces"])
    assert not out["stalled"] and out["faces"].shape[0] == 60 and after["oriented"].all() and after["euler"][0] == 0
    assert np.isfinite(out["vertices"]).all()


def test_unreferenced_vertices_and_bad_input():
    v, f = T.torus(8, 16)
    v2 = np.concatenate([[[9, 9, 9]], v, [[np.nan, 0, 0]]]).astype(np.float32)
    out = C.collapse(v2, f + 1, 100)
    assert out["vertex_map"][0] == -1 and out["vertex_map"][-1] == -1 and (out["vertex_map"][1:-1] >= 0).all()
    assert out["faces"].shape[0] == 100 and np.isfinite(out["vertices"]).all()          # (the hash sees the indices: another mesh than f's)
    bad = f.copy()
    bad[3, 1] = v.shape[0]
    with pytest.raises(ValueError, match="outside"):
        C.collapse(v, bad, 100)
    nan = v.copy()
    nan[7, 2] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        C.collapse(nan, f, 100)
    for kw in (dict(nfaces=0), dict(nfaces=100, placement="best"), dict(nfaces=100, max_rounds=0)):
        with pytest.raises(ValueError):
            C.collapse(v, f, **kw)


def test_solve_rows_is_mesh_simplify_refs_solve_and_the_hash_is_uint32():
    v, f = T.torus(8, 16)
    P = v.astype(np.float64)
    Q = C.initial_quadrics(P, f.astype(np.int64), np.zeros(3))
    q = np.concatenate([Q[f[:, 0]] + Q[f[:, 1]], np.zeros((1, 10)), np.eye(10)[[0, 4, 7]]])
    x0 = np.concatenate([(P[f[:, 0]] + P[f[:, 1]]) * 0.5, np.ones((4, 3))])
    xs = C.solve_rows(q, x0)
    for i in range(q.shape[0]):
        assert np.array(S.solve([float(t) for t in q[i]], [float(t) for t in x0[i]])).tobytes() == xs[i].tobytes(), i
    es = C.energy_rows(q, xs)
    assert all(es[i] == S.energy(q[i], xs[i]) for i in range(0, q.shape[0], 17))
    u, w, r = 123456, 2 ** 31 - 5, 7
    h = (u * 0x9E3779B1 ^ w * 0x85EBCA77 ^ r * 0xC2B2AE3D) & 0xFFFFFFFF
    h ^= h >> 15
    h = h * 0x2C1B3C6D & 0xFFFFFFFF
    h ^= h >> 12
    assert int(C.edge_hash([u], [w], r)[0]) == h >> 12 < 2 ** 20
    key = C.edge_keys(np.array([1.0, -1.0, np.inf]), np.array([u] * 3), np.array([w] * 3), r, np.array([5, 6, 7]))
    assert [int(k) >> 52 for k in key] == [0x3F8, 0, 0x7F8] and [int(k) & 0xFFFFFFFF for k in key] == [5, 6, 7]


def test_the_definition_is_quick_enough():
    import time
    v, f = T.torus(32, 64)
    t = time.time()
    out = C.collapse(v, f, 3000)
    assert out["faces"].shape[0] == 3000 and time.time() - t < 5.0


def test_abi_names_are_bound_and_the_python_surface_is_there():
    from vtaco_amd import _lib, ops
    from vtaco_amd._lib import VtError
    from vtaco_amd.conv_onet import config
    from vtaco_amd.conv_onet.generation import Generator3D, Mesh
    from vtaco_amd.utils import mesh_clean
    names = {"vt_mesh_collapse_workspace_bytes", "vt_mesh_collapse"}
    assert names <= set(_lib.SIGNATURES)
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vtaco_hip.h")).read()
    assert all(n + "(" in text for n in names)
    assert ops.mesh.Collapsed._fields == ("vertices", "faces", "vertex_map", "rounds", "stalled") and not hasattr(ops, "collapse")
    assert str(inspect.signature(ops.mesh.collapse)) == "(vertices, faces, nfaces, placement='optimal', max_rounds=None)"
    assert str(inspect.signature(mesh_clean.decimate)) == "(mesh, nfaces, placement='optimal')"
    assert callable(Mesh.decimate) and callable(Mesh.decimate_report) and callable(mesh_clean.decimate_report)
    # the default is vertex clustering; the config key reaches configure_simplify only when it is there
    assert Generator3D.simplify_method == "cluster"
    g = Generator3D.__new__(Generator3D)
    assert g.configure_simplify("collapse") is g and g.simplify_method == "collapse" and g.configure_simplify().simplify_method == "cluster"
    for bad in ("quadric", None, 1):
        with pytest.raises(VtError, match="method"):
            g.configure_simplify(bad)
    seen = {}

    class Stub:
        def __init__(self, model, **kw):
            seen["kw"] = kw

        def configure_subdivide(self, *a, **kw):
            return self

        def configure_simplify(self, method):
            seen["method"] = method
            return self

    saved, config.Generator3D = config.Generator3D, Stub
    try:
        cfg = {"generation": {"resolution_0": 16, "upsampling_steps": 1, "simplify_nfaces": 500}, "test": {"threshold": 0.5},
               "data": {"input_type": "pointcloud", "padding": 0.1}, "model": {}}
        config.get_generator(None, cfg, None)
        assert "method" not in seen and "simplify_method" not in seen["kw"] and seen["kw"]["simplify_nfaces"] == 500
        cfg["generation"]["simplify_method"] = "collapse"
        config.get_generator(None, cfg, None)
        assert seen["method"] == "collapse" and "simplify_method" not in seen["kw"]
    finally:
        config.Generator3D = saved
