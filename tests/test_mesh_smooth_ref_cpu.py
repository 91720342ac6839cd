"""CPU: the definition in tests/mesh_smooth_ref.py against things it did not come from -- the adjacency by Python sets, the uniform row mean
by a scipy.sparse operator, the closed form of one Laplacian pass on a regular icosahedron, the exact fixed points of an integer planar
grid -- and what the filters are for, on a marching-cubes sphere with the staircase of its lattice (inequalities between measured
quantities only; RATIO lines go to the file VTACO_RATIO_LOG names: profiles/mesh_smooth_f64_ratios.txt).  Then the argument checks of
ops.mesh.smooth, Generator3D(smooth=...) and the config keys, none of which needs a device."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mesh_smooth_ref as R  # noqa: E402

NAMES = sorted(R.FIXTURES)


@pytest.fixture(scope="module")
def spheres():
    from oracle import mc
    out = {}
    for key, radius in (("closed", R.CLOSED_RADIUS), ("cut", R.CUT_RADIUS)):
        v, f, _ = mc.marching_cubes(R.sphere_volume(radius), 0.0)
        v, f = np.ascontiguousarray(v, dtype=np.float32), np.ascontiguousarray(f, dtype=np.int32)
        out[key] = (v, f, R.adjacency(f, v.shape[0]))
    return out


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _check_adjacency(v, f):
    adj = R.adjacency(f, v.shape[0])
    rows, boundary = R.adjacency_by_sets(f, v.shape[0])
    off = adj["offsets"]
    assert off.dtype == np.int32 and off[0] == 0 and off[-1] == adj["neighbors"].shape[0] == sum(len(r) for r in rows)
    for i, want in enumerate(rows):
        got = adj["neighbors"][off[i]:off[i + 1]].tolist()
        assert got == want, i
        be = adj["boundary_edge"][off[i]:off[i + 1]].tolist()
        assert be == [int((min(i, j), max(i, j)) in boundary) for j in want], i
        assert int(adj["boundary_vertex"][i]) == int(any(be)), i
    return adj


@pytest.mark.parametrize("name", NAMES)
def test_adjacency_is_the_set_construction(name):
    v, f = R.fixture(name)
    adj = _check_adjacency(v, f)
    deg = np.diff(adj["offsets"])
    if name == "fan300":
        assert deg[0] == 300 and set(deg[1:].tolist()) == {3} and adj["boundary_vertex"].tolist() == [0] + [1] * 300
    if name == "odd":
        assert deg[[0, 7, 12]].tolist() == [0, 0, 0] and deg[4] == 2 and adj["neighbors"].shape[0] <= 6 * f.shape[0]
    if name == "empty":
        assert adj["offsets"].tolist() == [0, 0] and adj["neighbors"].shape[0] == 0
    if name == "icosahedron":
        assert set(deg.tolist()) == {5} and not adj["boundary_vertex"].any()
    with pytest.raises(ValueError):
        R.adjacency(np.array([[0, 1, v.shape[0]]]), v.shape[0])


def test_adjacency_of_the_spheres(spheres):
    for key, (nv, nf, nbv, dmax) in (("closed", (1296, 2588, 0, 8)), ("cut", (1968, 3560, 384, 9))):
        v, f, adj = spheres[key]
        _check_adjacency(v, f)
        assert (v.shape[0], f.shape[0], int(adj["boundary_vertex"].sum()), int(np.diff(adj["offsets"]).max())) == (nv, nf, nbv, dmax), key
        # neither the order of the faces nor their orientation is in it
        rng = np.random.RandomState(3)
        for other in (f[rng.permutation(f.shape[0])], f[:, ::-1], np.roll(f, 1, axis=1)):
            again = R.adjacency(other, v.shape[0])
            assert all(np.array_equal(adj[k], again[k]) for k in adj), key


def test_uniform_mean_is_the_sparse_operator(spheres):
    import scipy.sparse as sp
    for key in ("closed", "cut"):
        v, _, adj = spheres[key]
        x = v.astype(np.float64)
        V, nnz = v.shape[0], adj["neighbors"].shape[0]
        deg = np.diff(adj["offsets"]).astype(np.float64)
        A = sp.csr_matrix((np.ones(nnz), adj["neighbors"], adj["offsets"]), shape=(V, V))
        want = (A @ x) / deg[:, None]
        got, moves = R.row_mean(x, adj, R.weights(v, adj, "uniform"), "free")
        assert moves.all()
        gate = deg.max() * 2.0 ** -52 * np.abs(x).max()
        err = float(np.abs(got - want).max())
        R.log_line(f"RATIO cpu mc_sphere {key} uniform mean vs scipy.sparse: max |diff| = {err:.3e}, gate deg_max 2^-52 max|x| = {gate:.3e}")
        assert err <= gate, (key, err, gate)


def test_icosahedron_closed_form():
    v, f = R.fixture("icosahedron")
    adj = R.adjacency(f, 12)
    out = R.smooth(v, adj, "laplacian", 1, lam=0.5)
    want = 1.0 - 0.5 + 0.5 / np.sqrt(5.0)
    ratio = np.linalg.norm(out, axis=1) / np.linalg.norm(v, axis=1)
    err = float(np.abs(ratio - want).max())
    R.log_line(f"RATIO cpu icosahedron one laplacian pass: radius ratio {ratio[0]:.17g}, closed form {want:.17g}, "
               f"max |diff| = {err / 2.0 ** -52:.2f} x 2^-52 (gate 4)")
    assert abs(want - 0.7236067977499789) < 1e-15 and err <= 4 * 2.0 ** -52
    assert np.abs(out[v != 0] / v[v != 0] - want).max() <= 4 * 2.0 ** -52   # the direction of every vertex stays
    assert np.array_equal(out[v == 0], v[v == 0])


def test_planar_integer_grid():
    v, f = R.fixture("grid9")
    adj = R.adjacency(f, v.shape[0])
    n = 9
    side = np.zeros((n, n), dtype=bool)
    side[0, :] = side[-1, :] = side[:, 0] = side[:, -1] = True
    assert np.array_equal(adj["boundary_vertex"].astype(bool), side.reshape(-1))
    m, moves = R.row_mean(v.astype(np.float64), adj, R.weights(v, adj, "uniform"), "free")
    assert moves.all() and np.array_equal(m[~side.reshape(-1)], v[~side.reshape(-1)].astype(np.float64))    # exact fixed points
    for method in R.METHODS:
        assert _bits(R.smooth(v, adj, method, 7, boundary="pin")) == _bits(v), method
    corners = np.zeros((n, n), dtype=bool)
    corners[0, 0] = corners[0, -1] = corners[-1, 0] = corners[-1, -1] = True
    out = R.smooth(v, adj, "laplacian", 1, boundary="loop")
    moved = (out != v).any(axis=1)
    assert np.array_equal(moved, corners.reshape(-1))                     # the straight sides stay, the corners are cut
    for method in R.METHODS:                                              # the cut stays in its plane, whatever moves within it
        out = R.smooth(v, adj, method, 5, boundary="loop")
        assert np.array_equal(out[:, 2], v[:, 2]) and (out != v).any(), method


def test_what_the_filters_are_for(spheres):
    v, f, adj = spheres["closed"]
    tb, lp = R.smooth(v, adj, "taubin", 10), R.smooth(v, adj, "laplacian", 10, lam=0.5)
    hc = R.smooth(v, adj, "humphrey", 10)
    s0, s_tb, s_lp, s_hc = (R.radial_std(x) for x in (v, tb, lp, hc))
    vol = [abs(R.signed_volume(x, f)) for x in (v, tb, lp, hc)]
    R.log_line(f"RATIO cpu mc_sphere closed (R {R.CLOSED_RADIUS}, {v.shape[0]} vertices): radial std input {s0:.4f}, taubin {s_tb:.4f}, "
               f"laplacian {s_lp:.4f}, humphrey {s_hc:.4f}")
    R.log_line(f"RATIO cpu mc_sphere closed: volume input {vol[0]:.1f}, taubin {vol[1]:.1f}, laplacian {vol[2]:.1f}, humphrey {vol[3]:.1f}")
    assert s_tb < s0
    assert abs(vol[1] - vol[0]) < abs(vol[2] - vol[0])
    v, f, adj = spheres["cut"]
    bv = adj["boundary_vertex"].astype(bool)
    assert int(bv.sum()) == 384
    tb, lp = R.smooth(v, adj, "taubin", 10, boundary="pin"), R.smooth(v, adj, "laplacian", 10, lam=0.5, boundary="pin")
    hc = R.smooth(v, adj, "humphrey", 10, boundary="pin")
    s0, s_tb, s_lp, s_hc = (R.radial_std(x) for x in (v, tb, lp, hc))
    R.log_line(f"RATIO cpu mc_sphere cut (R {R.CUT_RADIUS}, {v.shape[0]} vertices, 384 pinned): radial std input {s0:.4f}, taubin {s_tb:.4f}, "
               f"laplacian {s_lp:.4f}, humphrey {s_hc:.4f}")
    assert s_tb < s0
    for out in (tb, lp, hc):
        assert _bits(out[bv]) == _bits(v[bv]) and (out[~bv] != v[~bv]).any()
    # 'loop' keeps every cut in the side of the box it lies in
    out = R.smooth(v, adj, "taubin", 10, boundary="loop")
    for axis in range(3):
        for wall in (0.0, 23.0):
            on = bv & (v[:, axis] == wall)
            assert on.any() and (out[on, axis] == wall).all(), (axis, wall)


def test_inverse_distance_weights_and_coincident_neighbours():
    v, f = R.fixture("coincident")
    adj = R.adjacency(f, v.shape[0])
    w = R.weights(v, adj, "inverse_distance")
    off, nb = adj["offsets"], adj["neighbors"]
    assert np.isfinite(w).all() and w[off[1]:off[2]][nb[off[1]:off[2]] == 2] == 0.0 and (w[off[5]:off[8]] == 0).all()
    assert w[off[0]:off[1]].tolist() == [1.0, 1.0, 1.0, 1.0]
    for method in R.METHODS:
        out = R.smooth(v, adj, method, 3, weights_scheme="inverse_distance", boundary="free")
        assert np.isfinite(out).all() and _bits(out[5:]) == _bits(v[5:]), method           # all weights 0: the vertex stays
        assert (out[:5] != v[:5]).any()


def test_iterations_zero_and_the_empty_mesh():
    v, f = R.fixture("tetrahedron")
    adj = R.adjacency(f, 4)
    assert _bits(R.smooth(v, adj, "taubin", 0)) == _bits(v)
    v, f = R.fixture("empty")
    assert _bits(R.smooth(v, R.adjacency(f, 1), "humphrey", 4)) == _bits(v)


def test_arguments_without_a_device():
    import inspect
    import torch
    from vtaco_amd import _lib, ops
    from vtaco_amd._lib import VtError
    from vtaco_amd.conv_onet import config
    from vtaco_amd.conv_onet.generation import Generator3D, Mesh
    m = ops.mesh
    adj = m.MeshAdjacency(*(torch.zeros(n, dtype=t) for n, t in ((4, torch.int32), (0, torch.int32), (0, torch.uint8), (3, torch.uint8))))
    x = torch.zeros(3, 3)
    for kw, word in ((dict(method="cotangent"), "method"), (dict(weights="cotangent"), "weights"), (dict(boundary="slide"), "boundary"),
                     (dict(iterations=-1), "iterations"), (dict(iterations=2.5), "iterations"), (dict(iterations=True), "iterations"),
                     (dict(lam=0.0), "lam"), (dict(lam=float("nan")), "lam"), (dict(lam="0.5"), "lam"), (dict(mu=-0.5), "mu < -lam"),
                     (dict(mu=0.3), "mu < -lam"), (dict(lam=0.6, mu=-0.53), "mu < -lam"), (dict(method="humphrey", alpha=1.5), "alpha"),
                     (dict(method="humphrey", beta=-0.1), "alpha and beta")):
        with pytest.raises(VtError, match=word):
            m.smooth(x, adj, **kw)
    with pytest.raises(VtError, match="HIP device"):                    # good arguments get as far as the device check, and no further
        m.smooth(x, adj)
    with pytest.raises(VtError, match="HIP device"):
        m.smooth(x, adj, method="laplacian", mu=0.3)                        # mu is taubin's alone
    with pytest.raises(VtError, match="HIP device"):
        m.vertex_adjacency(torch.zeros((1, 3), dtype=torch.int32), 3)
    mesh = Mesh(x, torch.zeros((1, 3), dtype=torch.int32))
    with pytest.raises(VtError, match="method"):
        mesh.smooth("cotangent")
    with pytest.raises(VtError, match="HIP device"):
        mesh.smooth()
    with pytest.raises(VtError, match="HIP device"):
        mesh.vertex_neighbors()
    # the launcher names the 6 F bound before it touches anything
    lib = _lib.load()
    assert m.MAX_ADJACENCY_FACES == 357913941 and lib.vt_mesh_adjacency_workspace_bytes(4, m.MAX_ADJACENCY_FACES + 1) == 0
    assert lib.vt_mesh_adjacency_count(None, m.MAX_ADJACENCY_FACES + 1, 4, None, None, None, 0, None) != 0
    assert "357913941" in lib.vt_last_error().decode() and "6 F" in lib.vt_last_error().decode()
    model = torch.nn.Linear(1, 1)
    for bad in ("nonsense", True, 0, 1.5):
        with pytest.raises(VtError, match="smooth"):
            Generator3D(model, device="cpu", smooth=bad)
    for bad in (-1, 4.0, True, "8"):
        with pytest.raises(VtError, match="smooth_iterations"):
            Generator3D(model, device="cpu", smooth="taubin", smooth_iterations=bad)
    gen = Generator3D(model, device="cpu")
    assert gen.smooth is None and gen.smooth_iterations == 10
    assert gen._clean(mesh) is mesh                                        # the default launches nothing
    gen = Generator3D(model, device="cpu", smooth="humphrey", smooth_iterations=np.int64(3))
    assert (gen.smooth, gen.smooth_iterations) == ("humphrey", 3) and isinstance(gen.smooth_iterations, int)
    with pytest.raises(VtError, match="Mesh.smooth"):
        Generator3D(model, device="cpu", smooth="taubin").generate_obj_mesh_sharded({})
    # test_mesh_fill_ref_cpu.py fixes the constructor's last three names, so the new ones stand just before them; every argument up
    # to min_component_faces keeps its position
    names = list(inspect.signature(Generator3D.__init__).parameters)
    assert names[-6:] == ["min_component_faces", "smooth", "smooth_iterations", "refine_sampler", "fill_holes", "fill_holes_max_edges"]
    assert names.index("min_component_faces") == 23
    cfg = {"generation": {"resolution_0": 8, "upsampling_steps": 0, "smooth": "taubin", "smooth_iterations": 4},
           "test": {"threshold": 0.5}, "data": {"input_type": "pointcloud", "padding": 0.1}, "model": {}}
    gen = config.get_generator(model, cfg, "cpu")
    assert (gen.smooth, gen.smooth_iterations) == ("taubin", 4)
    del cfg["generation"]["smooth"], cfg["generation"]["smooth_iterations"]
    gen = config.get_generator(model, cfg, "cpu")
    assert (gen.smooth, gen.smooth_iterations) == (None, 10)
