"""GPU: csrc/mesh_simplify.hip through ops.mesh and utils/mesh_clean against the numpy restatement (tests/mesh_simplify_ref.py):
cluster_of_vertex, K, the faces, the fallback count, the resolution the search finds and its probe count are equal, the positions are
equal byte for byte; everything runs twice and the two runs are equal bit for bit.  RATIO lines (appended to the file VTACO_RATIO_LOG
names) give the share of the energy gate the placement used."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mesh_simplify_ref as S  # noqa: E402
import mesh_topo_ref as T  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _dev(v, f):
    return torch.from_numpy(np.ascontiguousarray(v)).to(DEV), torch.from_numpy(np.ascontiguousarray(f)).to(DEV)


def _gate_share(ref):
    worst = 0.0
    for k in range(ref["K"]):
        ea, eb = S.energy(ref["q"][k], ref["x"][k]), S.energy(ref["q"][k], ref["x0"][k])
        gate = S.energy_gate(ref["q"][k], ref["x"][k], ref["x0"][k])
        worst = max(worst, (ea - eb) / gate if gate > 0 else (0.0 if ea <= eb else float("inf")))
    return worst


def _check(name, v, f, placement="quadric", **how):
    """simplify_report of the mesh, twice, against the restatement; returns (mesh, report, restatement)."""
    from vtaco_amd.utils import mesh_clean
    tv, tf = _dev(v, f)
    (got, rep), (again, rep2) = (mesh_clean.simplify_report((tv, tf), placement=placement, **how) for _ in range(2))
    ref = S.simplify(v, f, placement=placement, **how)
    assert torch.equal(got.vertices, again.vertices) and torch.equal(got.faces, again.faces) and rep[:4] == rep2[:4], name
    assert torch.equal(rep.cluster_of_vertex, rep2.cluster_of_vertex), name
    cov = rep.cluster_of_vertex.cpu().numpy()
    assert cov.dtype == np.int32 and np.array_equal(cov, ref["cluster_of_vertex"]), name
    assert (rep.n_clusters, rep.resolution, rep.probes) == (ref["K"], ref["R"], ref["probes"]), (name, rep[:4], ref["K"], ref["R"], ref["probes"])
    faces = got.faces.cpu().numpy()
    assert faces.dtype == np.int32 and faces.shape == ref["faces"].shape and np.array_equal(faces, ref["faces"]), name
    assert rep.fallbacks == ref["fallbacks"], (name, rep.fallbacks, ref["fallbacks"])
    pos = got.vertices.cpu().numpy()
    assert pos.dtype == v.dtype and pos.shape == (ref["K"], 3)
    differ = np.nonzero((pos.view(np.uint8).reshape(ref["K"], -1) != ref["vertices"].view(np.uint8).reshape(ref["K"], -1)).any(1))[0]
    assert differ.size == 0, (name, differ[:8], pos[differ[:4]], ref["vertices"][differ[:4]])
    if placement == "quadric":
        share = _gate_share(ref)
        T.log_line(f"RATIO gpu {name} {how}: E(x*) - E(x0) at most {share:.3e} of the gate, {ref['K']} clusters, {ref['fallbacks']} fallbacks")
        assert share <= 1.0, name
    return got, rep, ref


@pytest.mark.parametrize("n_faces", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_grid_strip(n_faces):
    v, f = T.grid_strip(n_faces)
    for R in (1, 2, 7):
        got, rep, ref = _check(f"strip{n_faces}", v, f, resolution=R)
        if R == 1:
            assert rep.n_clusters == 1 and got.faces.shape[0] == 0


def test_float64_vertices():
    v, f = T.torus(8, 16)
    v = v.astype(np.float64) + 1e-9 * np.random.RandomState(2).randn(*v.shape)
    for R in (3, 5, 40):
        got, rep, ref = _check("torus_f64", v, f, resolution=R)
        assert got.vertices.dtype == torch.float64
    _check("torus_f64", v, f, placement="mean", resolution=5)


@pytest.fixture(scope="module")
def torus():
    return T.torus(32, 64)


@pytest.mark.parametrize("R", [12, 23, 64])
def test_torus(torus, R):
    v, f = torus
    got, rep, ref = _check("torus", v, f, resolution=R)
    if R == 12:
        assert (rep.n_clusters, rep.fallbacks) == (264, 32)
    if R == 64:                                              # nothing merges: the output is the input
        assert rep.n_clusters == v.shape[0] and np.array_equal(got.faces.cpu().numpy(), f)
    _check("torus", v, f, placement="mean", resolution=R)


def test_cube_through_the_device_components():
    from vtaco_amd.utils import mesh_clean
    v, f = S.cube_grid(12)
    for R in range(2, 8):
        got, rep, ref = _check("cube", v, f, resolution=R)
        assert S.surface_distance_unit_cube(got.vertices.cpu().numpy()).max() <= 1e-12
        comps = mesh_clean.components(got)
        assert comps.n_components == 1 and bool(comps.watertight[0]) and bool(comps.oriented[0])
        assert abs(float(comps.volume[0]) - 1.0) <= 1e-12
    mean, _, _ = _check("cube", v, f, placement="mean", resolution=4)
    assert float(mesh_clean.components(mean).volume[0]) < 0.8


def test_hand_meshes_interleaved():
    v, f = T.concatenated()
    for R in (1, 3, 8, 50):
        _check("concatenated", v, f, resolution=R)


def test_thousands_of_clusters():
    v, f = T.triangles_and_spares(2000, 100)
    got, rep, ref = _check("triangles", v, f, resolution=512)
    assert rep.n_clusters > 5000 and int((rep.cluster_of_vertex < 0).sum()) == 100
    _check("triangles", v, f, resolution=4)


def test_vertices_on_cell_boundaries():
    for n in (4, 9):
        v, f = S.lattice_mesh(n)
        got, rep, ref = _check(f"lattice{n}", v, f, resolution=n)
        assert rep.n_clusters == n * n + 1                   # the last row and column share the last cells; the lifted corner has its own


def test_a_box_without_extent():
    v = np.full((5, 3), 2.5, dtype=np.float32)
    f = np.array([[0, 1, 2], [2, 3, 4]], dtype=np.int32)
    got, rep, ref = _check("point", v, f, resolution=9)
    assert rep.n_clusters == 1 and tuple(got.faces.shape) == (0, 3) and got.vertices.tolist() == [[2.5, 2.5, 2.5]]


@pytest.fixture(scope="module")
def blob_mesh():
    from vtaco_amd import ops
    vol = torch.from_numpy(T.blob_volume(33)).to(DEV)
    verts, faces, _ = ops.marching_cubes(vol, level=0.0)
    return verts.cpu().numpy(), faces.cpu().numpy()


@pytest.mark.parametrize("target", [300, 1000, 2000])
def test_search_on_the_torus(torus, target):
    v, f = torus
    got, rep, ref = _check("torus", v, f, nfaces=target)
    assert target / 2 <= got.faces.shape[0] <= target and 7 <= rep.probes <= 11


@pytest.mark.parametrize("target", [300, 1000, 2000])
def test_search_on_the_marching_cubes_mesh(blob_mesh, target):
    v, f = blob_mesh
    assert f.shape[0] == 2968
    got, rep, ref = _check("marching_cubes", v, f, nfaces=target)
    assert target / 2 <= got.faces.shape[0] <= target
    assert rep.resolution == {300: 9, 1000: 18, 2000: 33}[target]


def test_a_target_at_or_above_f_launches_nothing(torus):
    from vtaco_amd.conv_onet.generation import Mesh
    mesh = Mesh(*_dev(*torus))
    for target in (4096, 5000):
        out, rep = mesh.simplify_report(nfaces=target)
        assert out is mesh and rep.resolution is None and rep.probes == 0
    assert mesh.simplify(nfaces=4096) is mesh
    out = mesh.simplify(nfaces=1000)
    assert isinstance(out, Mesh) and out.faces.shape[0] == 944 and torch.equal(out.faces, mesh.simplify(resolution=15).faces)


def test_refusals(torus):
    from vtaco_amd import ops
    from vtaco_amd._lib import VtError
    from vtaco_amd.utils import mesh_clean
    v, f = torus
    tv, tf = _dev(v, f)
    with pytest.raises(VtError, match="HIP device"):
        mesh_clean.simplify((tv.cpu(), tf.cpu()), resolution=4)
    with pytest.raises(VtError, match="HIP device"):
        ops.mesh.cluster(tv.cpu(), tf, 4)
    for kw in ({}, {"nfaces": 100, "resolution": 4}):
        with pytest.raises(VtError, match="exactly one"):
            mesh_clean.simplify((tv, tf), **kw)
    for R in (0, -1, (1 << 20) + 1, 2.5):
        with pytest.raises(VtError, match="resolution"):
            mesh_clean.simplify((tv, tf), resolution=R)
    for n in (0, -3, 1.5):
        with pytest.raises(VtError, match="nfaces"):
            mesh_clean.simplify((tv, tf), nfaces=n)
    with pytest.raises(VtError, match="placement"):
        mesh_clean.simplify((tv, tf), resolution=4, placement="median")
    nan = tv.clone()
    nan[17, 1] = float("nan")
    with pytest.raises(VtError, match="non-finite"):
        mesh_clean.simplify((nan, tf), resolution=4)
    inf = tv.clone()
    inf[99, 2] = float("inf")
    with pytest.raises(VtError, match="non-finite"):
        mesh_clean.simplify((inf, tf), nfaces=500)
    with pytest.raises(VtError, match="float32 or float64"):
        mesh_clean.simplify((tv.half(), tf), resolution=4)


def test_a_face_index_out_of_range(torus):
    """The asynchronous call reports it in the status word and leaves the face out; the call that reads the state raises."""
    from vtaco_amd import ops
    from vtaco_amd._lib import VtError
    v, f = torus
    bad = f.copy()
    bad[100, 1] = v.shape[0]
    bad[3000, 0] = -1
    tv, tf = _dev(v, bad)
    c = ops.mesh.cluster(tv, tf, 6)
    state = c.state.cpu().numpy()
    want = S.cluster(v, bad, 6)
    assert state[ops.mesh.STATE_BAD] == 1 and state[ops.mesh.STATE_K] == want["K"]
    assert np.array_equal(c.cluster_of_vertex.cpu().numpy(), want["cluster_of_vertex"])
    assert np.array_equal(c.cluster_rep[:want["K"]].cpu().numpy(), want["rep"])
    with pytest.raises(VtError, match=r"outside \[0, V\)"):
        ops.mesh.cluster_faces(tf, c)
    good = ops.mesh.cluster(tv, torch.from_numpy(f).to(DEV), 6)
    assert int(good.state[ops.mesh.STATE_BAD]) == 0


def test_the_cluster_limit_is_named():
    """2^21 clusters or more: the face key has 21 bits per corner.  700 000 disjoint random triangles at the finest grid."""
    from vtaco_amd._lib import VtError
    from vtaco_amd.utils import mesh_clean
    g = torch.Generator(device=DEV).manual_seed(11)
    tv = torch.rand((2_100_000, 3), generator=g, device=DEV, dtype=torch.float64)
    tf = torch.arange(2_100_000, device=DEV, dtype=torch.int32).view(-1, 3)
    with pytest.raises(VtError, match="2097152"):
        mesh_clean.simplify((tv, tf), resolution=1 << 20)


# ---- welding -----------------------------------------------------------------------------------------------------------------------------
def _check_weld(name, v, f, **how):
    from vtaco_amd.utils import mesh_clean
    tv, tf = _dev(v, f)
    got, again = mesh_clean.merge_vertices((tv, tf), **how), mesh_clean.merge_vertices((tv, tf), **how)
    wv, wf, _ = S.weld(v, f, **how)
    assert torch.equal(got.faces, again.faces) and got.vertices.cpu().numpy().tobytes() == again.vertices.cpu().numpy().tobytes(), name
    assert got.faces.dtype == torch.int32 and np.array_equal(got.faces.cpu().numpy(), wf), name
    assert got.vertices.cpu().numpy().dtype == v.dtype and got.vertices.cpu().numpy().tobytes() == wv.tobytes(), name
    return got


def test_weld_undoes_a_doubling(torus):
    for name, (v, f) in (("torus8", T.torus(8, 16)), ("torus32", torus), ("concatenated", T.concatenated())):
        v2, f2 = S.doubled(v, f, seed=2)
        got = _check_weld(name, v2, f2, unique_faces=True)
        _check_weld(name, v2, f2)
        if name != "concatenated":
            assert tuple(got.vertices.shape) == v.shape and tuple(got.faces.shape) == f.shape
            comps = got.components()
            assert comps.n_components == 1 and bool(comps.oriented[0]) and int(comps.euler[0]) == 0
    v, f = T.triangles_and_spares(2000, 100)
    got = _check_weld("triangles", v, f)
    assert got.vertices.shape[0] == 6000 and got.faces.shape[0] == 2000


def test_weld_zero_signs_nan_and_tolerance():
    from vtaco_amd import ops
    from vtaco_amd._lib import VtError
    from vtaco_amd.utils import mesh_clean
    v = np.array([[0.0, 1, 2], [-0.0, 1, 2], [np.nan, 0, 0], [np.nan, 0, 0], [5, 5, 5], [5, 5, 5.04], [9, 9, 9]], dtype=np.float64)
    f = np.array([[0, 4, 2], [1, 5, 3], [0, 1, 4]], dtype=np.int32)
    for dtype in (np.float64, np.float32):
        for how in ({}, {"tol": 0.1}, {"tol": 0.01}, {"tol": 0.1, "unique_faces": True}):
            _check_weld("signs", v.astype(dtype), f, **how)
        tv, tf = _dev(v.astype(dtype), f)
        assert ops.mesh.weld(tv, tf).cluster_of_vertex.tolist() == [0, 0, 1, 2, 3, 4, -1]
        assert ops.mesh.weld(tv, tf, 0.1).cluster_of_vertex.tolist() == [0, 0, 1, 2, 3, 3, -1]
    dup = np.array([[0, 4, 2], [4, 0, 2], [0, 4, 5]], dtype=np.int32)
    assert _check_weld("dup", v, dup, tol=0.1, unique_faces=True).faces.shape[0] == 1
    assert _check_weld("dup", v, dup, tol=0.1).faces.shape[0] == 2
    tv, tf = _dev(v, f)
    with pytest.raises(VtError, match="int64"):
        mesh_clean.merge_vertices((tv, tf), tol=1e-300)
    for tol in (-1.0, float("inf"), float("nan")):
        with pytest.raises(VtError, match="tol"):
            mesh_clean.merge_vertices((tv, tf), tol=tol)
    with pytest.raises(VtError, match="HIP device"):
        mesh_clean.merge_vertices((tv.cpu(), tf.cpu()))
