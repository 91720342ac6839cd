"""GPU: csrc/mesh_fill.hip through ops.mesh and utils/mesh_clean against the definition (tests/mesh_fill_ref.py).  Every output is equal:
the loops' offsets, vertices and half-edges, every count, the output faces, the copied vertices, and the centroid vertices bit for bit;
everything runs twice and the two runs are equal bit for bit.  One functional test on marching-cubes output: a sphere that leaves its
volume through all six sides is watertight once filled, and its exact float64 winding number is an integer at every cell centre to
within 8 x what the same kernel leaves on a closed torus (RATIO lines, appended to the file VTACO_RATIO_LOG names)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mesh_fill_ref as R  # noqa: E402
import mesh_topo_ref as T  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAMES = sorted(R.FIXTURES)
COUNTS = ("n_loops", "n_filled", "n_new_faces", "n_new_vertices", "n_irregular")


def _dev(v, f):
    return torch.from_numpy(np.ascontiguousarray(v)).to(DEV), torch.from_numpy(np.ascontiguousarray(f)).to(DEV)


def _variants(name):
    """The fixture in float32 and float64 (the f64 one is its own fixture name where the definition needs it cached)."""
    v, f = R.fixture(name)
    yield name, v, f
    if v.dtype == np.float32:
        yield name + ":f64", v.astype(np.float64), f


def _reference(tag, v, f, method, max_edges=None):
    if ":" not in tag:
        return R.reference(tag, method, max_edges)
    key = (tag, method, max_edges)
    if key not in R._ref_cache:
        R._ref_cache[key] = R.fill_holes(v, f, method, max_edges)
    return R._ref_cache[key]


@pytest.mark.parametrize("name", NAMES)
def test_boundary_loops(name):
    from vtaco_amd import ops
    from vtaco_amd.utils import mesh_clean
    v, f = R.fixture(name)
    ref = R.boundary_loops(f, v.shape[0])
    tv, tf = _dev(v, f)
    got, again = ops.mesh.boundary_loops(tf, v.shape[0]), ops.mesh.boundary_loops(tf, v.shape[0])
    for k in ("offsets", "vertices", "half_edges"):
        g = getattr(got, k).cpu().numpy()
        assert g.dtype == np.int32 and np.array_equal(g, ref[k]), (name, k)
        assert torch.equal(getattr(got, k), getattr(again, k)), (name, k)
    assert (got.n_boundary, got.n_irregular) == (ref["n_boundary"], ref["n_irregular"]) == (again.n_boundary, again.n_irregular), name
    _, lengths, n_irregular = R.FIXTURES[name]
    if lengths is not None:
        assert np.diff(got.offsets.cpu().numpy()).tolist() == lengths
    if f.shape[0]:
        assert got.n_boundary == int(mesh_clean.components((tv, tf)).n_boundary.sum()), name
    if name == "annulus":
        T.log_line(f"ROUNDS gpu annulus: NB {got.n_boundary}, {int(np.ceil(np.log2(got.n_boundary)))} doubling rounds per pass")


@pytest.mark.parametrize("method", ["fan", "centroid"])
@pytest.mark.parametrize("name", NAMES)
def test_fill_holes(name, method):
    from vtaco_amd import ops
    from vtaco_amd.utils import mesh_clean
    for tag, v, f in _variants(name):
        ref = _reference(tag, v, f, method)
        tv, tf = _dev(v, f)
        got, again = ops.mesh.fill_holes(tv, tf, method=method), ops.mesh.fill_holes(tv, tf, method=method)
        for k in COUNTS:
            assert getattr(got, k) == ref[k] == getattr(again, k), (tag, k)
        gf, gv = got.faces.cpu().numpy(), got.vertices.cpu().numpy()
        assert gf.dtype == np.int32 and np.array_equal(gf, ref["faces"]), tag
        assert gv.dtype == v.dtype and gv[:v.shape[0]].tobytes() == v.tobytes(), tag
        assert gv.tobytes() == ref["vertices"].tobytes(), tag                      # the centroids, bit for bit
        assert torch.equal(got.faces, again.faces) and got.vertices.cpu().numpy().tobytes() == again.vertices.cpu().numpy().tobytes(), tag
        if ref["n_new_faces"] == 0:
            assert got.vertices.data_ptr() == tv.data_ptr() and got.faces.data_ptr() == tf.data_ptr(), tag       # the inputs' own storage
        elif ref["n_irregular"] == 0 and name != "fan_on_one_edge":
            comps = mesh_clean.components((got.vertices, got.faces))
            assert bool(comps.watertight.all()) and bool(comps.oriented.all()), tag


def test_more_than_256_scan_blocks():
    """87 382 disjoint triangles: the 3 F flags, and the NB = 262 146 boundary half-edges after them, each take 257 blocks of the scan, so
    the one workgroup that scans the block sums goes round its loop twice and carries a sum over -- in the int32 scan of the flags and in
    the 64-bit scan of the loop heads.  Every triangle is a loop of 3 and gets one face."""
    from vtaco_amd import ops
    n = 87382
    f = np.arange(3 * n, dtype=np.int32).reshape(n, 3)
    v = (np.arange(9 * n) % 97).astype(np.float32).reshape(3 * n, 3)
    assert -(-3 * n // 1024) == 257
    ref = R.fill_holes(v, f, "fan")
    loops = ref["loops"]
    assert (loops["n_loops"], loops["n_boundary"], loops["n_irregular"], ref["n_new_faces"]) == (n, 3 * n, 0, n)
    tv, tf = _dev(v, f)
    got, again = ops.mesh.boundary_loops(tf, 3 * n), ops.mesh.boundary_loops(tf, 3 * n)
    for k in ("offsets", "vertices", "half_edges"):
        assert np.array_equal(getattr(got, k).cpu().numpy(), loops[k]) and torch.equal(getattr(got, k), getattr(again, k)), k
    assert (got.n_boundary, got.n_irregular) == (3 * n, 0) == (again.n_boundary, again.n_irregular)
    got, again = ops.mesh.fill_holes(tv, tf, method="fan"), ops.mesh.fill_holes(tv, tf, method="fan")
    for k in COUNTS:
        assert getattr(got, k) == ref[k] == getattr(again, k), k
    assert np.array_equal(got.faces.cpu().numpy(), ref["faces"]) and torch.equal(got.faces, again.faces)
    assert got.vertices.cpu().numpy().tobytes() == v.tobytes() == again.vertices.cpu().numpy().tobytes()


def test_max_edges_and_report():
    from vtaco_amd.conv_onet.generation import Mesh
    from vtaco_amd.utils import mesh_clean
    v, f = R.fixture("torus_with_holes")
    tv, tf = _dev(v, f)
    for method in ("fan", "centroid"):
        ref = R.reference("torus_with_holes", method, 5)                  # between the loops of 3 and the loop of 8
        mesh, rep = mesh_clean.fill_report(Mesh(tv, tf), method=method, max_edges=5)
        assert (rep.n_loops, rep.n_filled, rep.n_new_faces, rep.n_new_vertices, rep.n_irregular) == (5, 4, 4, 0, 0)
        assert rep.n_boundary == 20 and np.array_equal(mesh.faces.cpu().numpy(), ref["faces"])
        assert not bool(mesh.components().watertight.all())
    v, f = R.fixture("torus_with_bowtie")
    mesh, rep = Mesh(*_dev(v, f)).fill_report("centroid")
    assert (rep.n_loops, rep.n_filled, rep.n_new_vertices, rep.n_irregular) == (3, 3, 1, 6)
    assert mesh.vertices.shape[0] == v.shape[0] + 1


def test_closed_mesh_comes_back_as_itself_and_bad_input_is_refused():
    from vtaco_amd import ops
    from vtaco_amd._lib import VtError
    from vtaco_amd.conv_onet.generation import Mesh, NormalMesh
    from vtaco_amd.utils import mesh_clean
    tv, tf = _dev(*T.torus(8, 16))
    mesh = Mesh(tv, tf)
    assert mesh.fill_holes() is mesh and mesh_clean.fill_holes(mesh, "centroid") is mesh
    assert mesh.boundary_loops().n_boundary == 0 and mesh.boundary_loops().offsets.tolist() == [0]
    empty = Mesh(tv, tf[:0])
    assert empty.fill_holes() is empty
    bad = tf.clone()
    bad[5, 1] = tv.shape[0]
    with pytest.raises(VtError, match=r"outside \[0, V\)"):
        ops.mesh.boundary_loops(bad, tv.shape[0])
    bad[5, 1] = -1
    with pytest.raises(VtError, match=r"outside \[0, V\)"):
        ops.mesh.fill_holes(tv, bad)
    with pytest.raises(VtError, match="int32"):
        ops.mesh.boundary_loops(tf.long(), tv.shape[0])
    with pytest.raises(VtError, match="method"):
        ops.mesh.fill_holes(tv, tf, method="ear")
    with pytest.raises(VtError, match="max_edges"):
        ops.mesh.fill_holes(tv, tf, max_edges=2)
    # a NormalMesh: 'fan' keeps its normals and values, 'centroid' names the two ways on
    ov, of = _dev(*R.fixture("open_cube"))
    nm = NormalMesh(ov, of, vertex_normals=torch.ones_like(ov), values=torch.arange(8.0, device=DEV), normals_source="marching_cubes")
    out = nm.fill_holes("fan")
    assert isinstance(out, NormalMesh) and out.vertex_normals is nm.vertex_normals and out.values is nm.values
    assert out.normals_source == "marching_cubes" and out.faces.shape[0] == of.shape[0] + 2
    with pytest.raises(VtError, match=r"'fan'.*with_vertex_normals\(\)"):
        nm.fill_holes("centroid")


# ---- marching-cubes output -------------------------------------------------------------------------------------------------------------
N = 24


@pytest.fixture(scope="module")
def sphere():
    from vtaco_amd import ops
    verts, faces, _ = ops.marching_cubes(torch.from_numpy(R.sphere_volume(N)).to(DEV), level=0.0)
    c = (torch.arange(N - 1, device=DEV, dtype=torch.float32) + 0.5)
    centres = torch.stack(torch.meshgrid(c, c, c, indexing="ij"), -1).reshape(-1, 3).contiguous()
    return verts, faces, centres


def _deviation(v, f, pts):
    """max |w - round(w)| of the exact float64 winding number (every face summed: no cell of the tree is accepted)."""
    from vtaco_amd import ops
    w, stats = ops.winding.fast(v, f, pts, accuracy=1e30, dtype=torch.float64, stats=True)
    assert w.dtype == torch.float64 and int(stats[:, 0].max()) == 0 and int(stats[:, 1].min()) == f.shape[0]
    return float((w - w.round()).abs().max())


def test_marching_cubes_sphere(sphere):
    from vtaco_amd.conv_onet.generation import Mesh
    verts, faces, centres = sphere
    mesh = Mesh(verts, faces)
    loops = mesh.boundary_loops()
    L = loops.offsets.shape[0] - 1
    assert L == 6 and loops.n_irregular == 0, (L, loops.n_irregular)
    lv, off = loops.vertices.long(), loops.offsets.tolist()
    for l in range(6):                                                    # each loop lies in one side of the volume
        ring = verts[lv[off[l]:off[l + 1]]]
        spread = ring.max(0).values - ring.min(0).values
        assert int((spread == 0).sum()) == 1, l
    tv, tf = _dev(*T.torus(8, 16))
    tv = tv * 8.0 + (N - 1) / 2.0
    assert float(tv.min()) > 0 and float(tv.max()) < N - 1
    base = _deviation(tv, tf, centres)
    gate = 8.0 * base
    open_dev = _deviation(verts, faces, centres)
    T.log_line(f"RATIO gpu mc_sphere{N} open: max |w - round(w)| = {open_dev:.3e} over {centres.shape[0]} cell centres, {faces.shape[0]} faces")
    T.log_line(f"RATIO gpu torus(8,16) closed: max |w - round(w)| = {base:.3e}; the gate is 8 x that = {gate:.3e}")
    assert open_dev > 0.25                                                # the unfilled mesh leaves w fractional: the feature shows, not the gate
    for method in ("fan", "centroid"):
        filled, rep = mesh.fill_report(method)
        assert (rep.n_loops, rep.n_filled, rep.n_irregular) == (6, 6, 0)
        comps = filled.components()
        assert comps.n_components == 1 and bool(comps.watertight[0]) and bool(comps.oriented[0]) and int(comps.euler[0]) == 2, method
        dev = _deviation(filled.vertices, filled.faces, centres)
        T.log_line(f"RATIO gpu mc_sphere{N} {method}: max |w - round(w)| = {dev:.3e}, {dev / gate:.3e} of the gate, {filled.faces.shape[0]} faces")
        assert dev <= gate, (method, dev, gate)
