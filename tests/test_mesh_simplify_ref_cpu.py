"""CPU: the numpy restatement of csrc/mesh_simplify.hip (tests/mesh_simplify_ref.py) on meshes whose answers are known: the quadrics
put a simplified cube's vertices back on the cube, the solve never raises a cluster's error above the mean's, the search meets its
contract at pinned resolutions, the fallback fires, welding undoes a doubling; and the generator's argument check without a device."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mesh_simplify_ref as S  # noqa: E402
import mesh_topo_ref as T  # noqa: E402


def _same_mesh(a, b):
    return a[0].dtype == b[0].dtype and a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1])


@pytest.fixture(scope="module")
def cube():
    v, f = S.cube_grid(12)
    assert v.shape == (866, 3) and f.shape == (1728, 3) and v.dtype == np.float32
    t = T.topo(v, f)
    assert t["n_components"] == 1 and bool(t["oriented"][0]) and t["volume"][0] == pytest.approx(1.0, abs=1e-12)
    return v, f


@pytest.mark.parametrize("resolution", [2, 3, 4, 5, 6, 7])
def test_quadrics_put_the_cube_back_on_its_surface(cube, resolution):
    """The test that shows the quadrics are real: every vertex of the result on the cube's surface, the result one watertight oriented
    component of volume 1.  (The restatement gave distances <= 4e-17 and |volume - 1| = 0 at every resolution.)"""
    v, f = cube
    out = S.simplify(v, f, resolution=resolution)
    assert out["vertices"].dtype == np.float32 and out["vertices"].shape == (out["K"], 3) and out["faces"].max() == out["K"] - 1
    dist = S.surface_distance_unit_cube(out["vertices"])
    t = T.topo(out["vertices"], out["faces"])
    print(f"cube R={resolution}: K={out['K']} F={out['faces'].shape[0]} fallbacks={out['fallbacks']} max distance {dist.max():.3e} "
          f"volume - 1 = {t['volume'][0] - 1.0:.3e}")
    assert dist.max() <= 1e-12
    assert t["n_components"] == 1 and bool(t["watertight"][0]) and bool(t["oriented"][0])
    assert abs(t["volume"][0] - 1.0) <= 1e-12
    assert out["faces"].shape[0] < f.shape[0]


def test_mean_placement_shrinks_the_cube(cube):
    v, f = cube
    out = S.simplify(v, f, resolution=4, placement="mean")
    t = T.topo(out["vertices"], out["faces"])
    assert t["n_components"] == 1 and t["volume"][0] < 0.8
    assert np.array_equal(out["faces"], S.simplify(v, f, resolution=4)["faces"])        # the placement moves vertices only


@pytest.fixture(scope="module")
def torus():
    return T.torus(32, 64)


@pytest.fixture(scope="module")
def blob():
    from oracle import mc
    v, f, _ = mc.marching_cubes(T.blob_volume(33), 0.0)
    v, f = np.ascontiguousarray(v, dtype=np.float32), np.ascontiguousarray(f, dtype=np.int32)
    assert f.shape[0] == 2968 and T.topo(v, f)["n_components"] == 3
    return v, f


@pytest.mark.parametrize("resolution", [5, 12, 23])
def test_the_solve_never_raises_a_clusters_error(torus, resolution):
    """Per cluster E(x*) <= E(x0) + gate (mesh_simplify_ref.energy_gate)."""
    v, f = torus
    out = S.simplify(v, f, resolution=resolution)
    worst, lowered = 0.0, 0
    for k in range(out["K"]):
        ea, eb = S.energy(out["q"][k], out["x"][k]), S.energy(out["q"][k], out["x0"][k])
        gate = S.energy_gate(out["q"][k], out["x"][k], out["x0"][k])
        assert ea <= eb + gate, (k, ea, eb, gate)
        worst = max(worst, (ea - eb) / gate if gate > 0 else 0.0)
        lowered += ea < eb
    print(f"torus R={resolution}: worst (E(x*) - E(x0)) / gate = {worst:.3e}, lowered in {lowered} of {out['K']} clusters")
    assert lowered > out["K"] // 2


SEARCH = {("torus", 300): (8, 208), ("torus", 1000): (15, 944), ("torus", 2000): (23, 1984),
          ("blob", 300): (9, 254), ("blob", 1000): (18, 968), ("blob", 2000): (33, 1854)}


@pytest.mark.parametrize("name,target", sorted(SEARCH))
def test_search_meets_its_target(torus, blob, name, target):
    v, f = torus if name == "torus" else blob
    out = S.simplify(v, f, nfaces=target)
    n = out["faces"].shape[0]
    print(f"{name} target {target}: {n} faces at R = {out['R']} after {out['probes']} probes")
    assert target / 2 <= n <= target
    assert (out["R"], n) == SEARCH[(name, target)] and 7 <= out["probes"] <= 11
    again = S.simplify(v, f, resolution=out["R"])
    assert S.count_at(v, f, out["R"]) == n and _same_mesh((out["vertices"], out["faces"]), (again["vertices"], again["faces"]))


def test_a_target_at_or_above_f_returns_the_input(torus):
    v, f = torus
    for target in (f.shape[0], f.shape[0] + 1):
        out = S.simplify(v, f, nfaces=target)
        assert out["vertices"] is v and out["faces"] is f and out["unchanged"] and out["probes"] == 0
    with pytest.raises(ValueError):
        S.simplify(v, f)
    with pytest.raises(ValueError):
        S.simplify(v, f, nfaces=10, resolution=3)


def test_the_count_is_not_monotone_in_the_resolution(torus):
    """Why the contract is "at most nfaces at the resolution the search finds" and not "the finest grid"."""
    v, f = torus
    counts = [S.count_at(v, f, r) for r in range(2, 40)]
    assert any(b < a for a, b in zip(counts, counts[1:]))


def test_the_fallback_fires(torus):
    v, f = torus
    out = S.simplify(v, f, resolution=12)
    assert (out["K"], out["fallbacks"]) == (264, 32)
    fell = np.nonzero((out["x"] == out["x0"]).all(1))[0]
    assert fell.shape[0] >= 32
    assert S.simplify(v, f, resolution=12, placement="mean")["fallbacks"] == 0
    # a fallen cluster sits at its mean, every other one inside its cell
    bound = np.array(S.cell_bound(S.cluster(v, f, 12)["lo"], float(S.cluster(v, f, 12)["L"]), float(out["h"])))
    assert (np.abs(out["x"]) <= bound).all()


def test_nothing_merges_on_a_fine_grid(torus):
    v, f = torus
    out = S.simplify(v, f, resolution=64)
    assert out["K"] == v.shape[0] and np.array_equal(out["faces"], f) and out["cluster_of_vertex"].tolist() == list(range(v.shape[0]))
    assert np.abs(out["vertices"].astype(np.float64) - v).max() <= 2.0 ** -23 * 1.3     # one vertex per cluster: the quadric has it on all its planes


def test_rules_among_equals_and_edge_cases():
    v, f = T.concatenated()
    c = S.cluster(v, f, 3)
    cov, rep = c["cluster_of_vertex"], c["rep"]
    assert (cov < 0).sum() == 1                                                      # the spare vertex of two_cubes_and_a_spare
    assert (np.diff(rep) > 0).all() and all(cov[r] == k for k, r in enumerate(rep.tolist()))
    for k, r in enumerate(rep.tolist()):
        assert r == np.nonzero(cov == k)[0][0]                                       # the representative is the lowest index
    # an out-of-range face takes no part
    bad = np.concatenate([f, [[0, 1, v.shape[0]]]]).astype(np.int32)
    assert np.array_equal(S.cluster(v, bad, 3)["cluster_of_vertex"], cov)
    # L = 0: one cluster, no faces
    p = np.ones((3, 3), dtype=np.float32)
    out = S.simplify(p, np.array([[0, 1, 2]], dtype=np.int32), resolution=5)
    assert out["K"] == 1 and out["faces"].shape == (0, 3) and out["vertices"].tolist() == [[1.0, 1.0, 1.0]]
    with pytest.raises(ValueError, match="non-finite"):
        S.simplify(np.array([[0, 0, 0], [1, 0, 0], [0, np.nan, 0]], dtype=np.float32), np.array([[0, 1, 2]], dtype=np.int32), resolution=2)
    # integer coordinates, R = the extent: every vertex on a cell boundary, the last row on the box's upper faces
    v, f = S.lattice_mesh(4)
    c = S.cluster(v, f, 4)
    assert c["h"] == 1.0 and c["cell"][:, 0].tolist() == [min(i, 3) for i in range(5) for _ in range(5)]
    # of two faces with one unordered triple the first survives, with its own corner order
    ids = np.array([0, 1, 2, 3], dtype=np.int32)
    out = S.cluster_faces(np.array([[2, 1, 0], [0, 1, 2], [1, 1, 3], [0, 3, 2]], dtype=np.int32), ids, 4)
    assert out.tolist() == [[2, 1, 0], [0, 3, 2]]
    assert S.cluster_faces(np.array([[2, 1, 0], [0, 1, 2], [1, 1, 3]], dtype=np.int32), ids, 4, unique=False).tolist() == [[2, 1, 0], [0, 1, 2]]


def test_fixed_point_sums_equal_the_topology_restatement():
    rng = np.random.RandomState(1)
    terms = rng.randn(500) * 10.0 ** rng.randint(-8, 8, 500)
    owner = rng.randint(0, 7, 500)
    big = np.zeros(7)
    np.maximum.at(big, owner, np.abs(terms))
    got = S.fixed_sums(terms, owner, 7, S.exponent_of(big))
    for k in range(7):
        assert got[k] == T.fixed_point_sum(terms[owner == k])


def test_weld_undoes_a_doubling():
    v, f = T.torus(8, 16)
    v2, f2 = S.doubled(v, f, seed=2)
    wv, wf, cov = S.weld(v2, f2, unique_faces=True)
    assert wv.shape == v.shape and wf.shape == f.shape
    assert sorted(map(tuple, wv.tolist())) == sorted(map(tuple, v.tolist()))
    t = T.topo(wv, wf)
    assert t["n_components"] == 1 and bool(t["oriented"][0]) and int(t["euler"][0]) == 0
    wv, wf, _ = S.weld(v2, f2)                                                       # the copies' faces stay without unique_faces
    assert wv.shape == v.shape and wf.shape[0] == 2 * f.shape[0]
    # survivors are the lowest indices, in their order, with their own coordinates
    rep = np.array([np.nonzero(cov == k)[0][0] for k in range(v.shape[0])])
    assert (np.diff(rep) > 0).all() and wv.tobytes() == v2[rep].tobytes()


def test_weld_zero_signs_nan_and_tolerance():
    v = np.array([[0.0, 1, 2], [-0.0, 1, 2], [np.nan, 0, 0], [np.nan, 0, 0], [5, 5, 5], [5, 5, 5.04], [9, 9, 9]], dtype=np.float64)
    f = np.array([[0, 4, 2], [1, 5, 3], [0, 1, 4]], dtype=np.int32)
    wv, wf, cov = S.weld(v, f)
    assert cov.tolist() == [0, 0, 1, 2, 3, 4, -1]                                    # -0.0 = +0.0; NaN with nothing; [9,9,9] unreferenced
    assert wf.tolist() == [[0, 3, 1], [0, 4, 2]] and wv.shape == (5, 3) and np.signbit(wv[0, 0]) == np.signbit(v[0, 0])
    wv, wf, cov = S.weld(v, f, tol=0.1)
    assert cov.tolist() == [0, 0, 1, 2, 3, 3, -1] and wv[3].tolist() == [5, 5, 5]
    wv, wf, cov = S.weld(v, f, tol=0.01)
    assert cov.tolist() == [0, 0, 1, 2, 3, 4, -1]
    with pytest.raises(ValueError, match="int64"):
        S.weld(v, f, tol=1e-300)
    dup = np.array([[0, 4, 2], [4, 0, 2], [0, 4, 5]], dtype=np.int32)
    assert S.weld(v, dup, tol=0.1, unique_faces=True)[1].shape[0] == 1 and S.weld(v, dup, tol=0.1)[1].shape[0] == 2


def test_generator_argument_without_a_device():
    import torch
    from vtaco_amd._lib import VtError
    from vtaco_amd.conv_onet.generation import Generator3D, Mesh
    model = torch.nn.Linear(1, 1)
    for bad in (0, -5, 2.5, "100", True):
        with pytest.raises(VtError, match="simplify_nfaces"):
            Generator3D(model, device="cpu", simplify_nfaces=bad)
    assert Generator3D(model, device="cpu").simplify_nfaces is None
    gen = Generator3D(model, device="cpu", simplify_nfaces=np.int64(500))
    assert gen.simplify_nfaces == 500 and isinstance(gen.simplify_nfaces, int)
    with pytest.raises(VtError, match="Mesh.simplify"):
        gen.generate_obj_mesh_sharded({})
    mesh = Mesh(torch.zeros(3, 3), torch.zeros((1, 3), dtype=torch.int32))
    assert gen._clean(mesh) is mesh                                                  # at most N faces already: nothing is launched
    with pytest.raises(VtError, match="HIP device"):
        mesh.simplify(resolution=4)
    with pytest.raises(VtError, match="HIP device"):
        mesh.merge_vertices()
    for kw in ({}, {"nfaces": 10, "resolution": 4}):
        with pytest.raises(VtError, match="exactly one"):
            mesh.simplify(**kw)
