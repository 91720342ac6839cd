"""GPU: csrc/mesh_topo.hip through ops.mesh and utils/mesh_clean against the numpy restatement (tests/mesh_topo_ref.py).  Every integer
output is equal; filtered vertices and bbox are equal bit for bit; area and volume lie inside the rounding gate
|got - ref| <= (n_faces_c + 16) 2^-52 sum_f M_f (RATIO lines, appended to the file VTACO_RATIO_LOG names: the share of the gate that was used); everything runs twice and
the two runs are equal bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mesh_topo_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
INT_FIELDS = ("labels", "comp_of_vertex", "comp_of_face", "n_faces", "n_vertices", "n_edges", "n_boundary", "n_nonmanifold", "n_misoriented",
              "euler")


def _dev(v, f):
    return torch.from_numpy(np.ascontiguousarray(v)).to(DEV), torch.from_numpy(np.ascontiguousarray(f)).to(DEV)


def _check(name, v, f):
    """components() of the mesh, twice, against the restatement; returns (record, restatement)."""
    from vtaco_amd.utils import mesh_clean
    tv, tf = _dev(v, f)
    got, again = mesh_clean.components((tv, tf)), mesh_clean.components((tv, tf))
    ref = R.topo(v, f)
    assert got.n_components == ref["n_components"] == again.n_components, name
    for k in INT_FIELDS:
        g = getattr(got, k).cpu().numpy()
        assert g.dtype == np.int32 and np.array_equal(g, ref[k]), (name, k)
        assert torch.equal(getattr(got, k), getattr(again, k)), (name, k)
    for k in ("watertight", "oriented"):
        assert np.array_equal(getattr(got, k).cpu().numpy(), ref[k]), (name, k)
    bbox = got.bbox.cpu().numpy()
    assert bbox.dtype == v.dtype and bbox.tobytes() == ref["bbox"].tobytes(), name
    m_area, m_vol = R.term_bounds(v, f)
    for k, bounds in (("area", m_area), ("volume", m_vol)):
        g = getattr(got, k).cpu().numpy()
        assert g.dtype == np.float64 and g.tobytes() == getattr(again, k).cpu().numpy().tobytes(), (name, k)
        worst = 0.0
        for c in range(ref["n_components"]):
            sel = ref["comp_of_face"] == c
            gate = R.sum_gate(int(sel.sum()), bounds[sel].tolist())
            err = abs(float(g[c]) - float(ref[k][c]))
            worst = max(worst, err / gate if gate > 0 else (0.0 if err == 0 else float("inf")))
        R.log_line(f"RATIO gpu {name} {k}: {worst:.3e} of the gate, {ref['n_components']} components")
        assert worst <= 1.0, (name, k, worst)
    assert got.rounds >= 1
    return got, ref


@pytest.mark.parametrize("n_faces", [1, 63, 64, 65, 257, 1000])
def test_grid_strip(n_faces):
    v, f = R.grid_strip(n_faces)
    got, ref = _check(f"strip{n_faces}", v, f)
    assert got.n_components == 1


def test_float64_vertices():
    v, f = R.torus(8, 16)
    rng = np.random.RandomState(2)
    v = v.astype(np.float64) + 1e-9 * rng.randn(*v.shape)
    got, ref = _check("torus_f64", v, f)
    assert got.bbox.dtype == torch.float64 and int(got.euler[0]) == 0


def test_permuted_strip_of_20000_vertices():
    """One component of maximal diameter over many workgroups: what a capped round count or a stale plain load breaks."""
    v, f = R.permuted_strip(20000, seed=3)
    got, ref = _check("permuted_strip", v, f)
    assert got.n_components == 1 and int(got.labels.max()) == 0
    R.log_line(f"ROUNDS gpu permuted_strip: {got.rounds} hooking rounds")


def test_disjoint_triangles_and_unreferenced_vertices():
    v, f = R.triangles_and_spares(2000, 100)
    got, ref = _check("triangles", v, f)
    assert got.n_components == 2000 and int((got.comp_of_vertex < 0).sum()) == 100


def test_hand_meshes_interleaved():
    v, f = R.concatenated()
    got, ref = _check("concatenated", v, f)
    assert got.n_components == 8
    rep = got.report()
    assert rep["n_nonmanifold"][0] == 3 and rep["euler"] == ref["euler"].tolist() and rep["oriented"] == ref["oriented"].tolist()
    assert rep["area"] == got.area.cpu().tolist() and rep["n_components"] == 8


@pytest.fixture(scope="module")
def blob_mesh():
    from vtaco_amd import ops
    vol = torch.from_numpy(R.blob_volume(33)).to(DEV)
    verts, faces, _ = ops.marching_cubes(vol, level=0.0)
    assert faces.dtype == torch.int32 and verts.dtype == torch.float32
    return verts, faces, verts.cpu().numpy(), faces.cpu().numpy()


def test_marching_cubes_mesh(blob_mesh):
    from vtaco_amd.conv_onet.generation import Mesh
    from vtaco_amd.utils import mesh_clean
    tv, tf, v, f = blob_mesh
    got, ref = _check("marching_cubes", v, f)
    assert got.n_components == 3
    small = int(np.argmin(ref["n_faces"]))
    mesh = Mesh(tv, tf)
    for by in ("faces", "area", "volume"):
        want_v, want_f, _ = R.filter_mesh(v, f, ref, R.largest(ref, by))
        out = mesh.keep_largest(by=by)
        assert np.array_equal(out.faces.cpu().numpy(), want_f) and out.vertices.cpu().numpy().tobytes() == want_v.tobytes(), by
    keep = np.ones(3, dtype=bool)
    keep[small] = False
    want_v, want_f, _ = R.filter_mesh(v, f, ref, keep)
    out = mesh.remove_small(min_faces=int(ref["n_faces"][small]) + 1)
    assert np.array_equal(out.faces.cpu().numpy(), want_f) and out.vertices.cpu().numpy().tobytes() == want_v.tobytes()
    assert out.faces.shape[0] == f.shape[0] - int(ref["n_faces"][small])
    same = mesh.remove_small()
    assert torch.equal(same.faces, tf) and torch.equal(same.vertices, tv)
    assert out.faces.shape[0] == mesh.remove_small(min_area_fraction=0.05).faces.shape[0]
    parts = mesh.split()
    assert [p.faces.shape[0] for p in parts] == ref["n_faces"].tolist() and all(isinstance(p, Mesh) for p in parts)
    assert sum(p.vertices.shape[0] for p in parts) == v.shape[0]
    assert mesh_clean.split(Mesh(tv, tf[:0])) == []


def test_filter_masks():
    from vtaco_amd import ops
    v, f = R.concatenated(seed=4)
    # component 1 (the torus) gets vertices that are not contiguous in index: renumber with a seeded permutation of all vertices
    perm = np.random.RandomState(8).permutation(v.shape[0]).astype(np.int32)
    v2 = np.empty_like(v)
    v2[perm] = v
    f2 = perm[f]
    ref = R.topo(v2, f2)
    tv, tf = _dev(v2, f2)
    labels = ops.mesh.components(tf, tv.shape[0])
    table = ops.mesh.component_table(tf, labels)
    C = table.n_components
    assert C == ref["n_components"] == 8
    masks = {"all": np.ones(C, bool), "none": np.zeros(C, bool), "alternating": np.arange(C) % 2 == 0}
    big = int(np.argmax(ref["n_vertices"]))
    assert np.any(np.diff(np.nonzero(ref["comp_of_vertex"] == big)[0]) > 1)       # its vertices are scattered through the index range
    masks["scattered"] = np.arange(C) == big
    for name, keep in masks.items():
        want_v, want_f, want_map = R.filter_mesh(v2, f2, ref, keep)
        for kd in (torch.from_numpy(keep).to(DEV), torch.from_numpy(keep.astype(np.uint8)).to(DEV)):
            out = ops.mesh.filter_components(tv, tf, table, kd)
            assert out.faces.dtype == torch.int32 and tuple(out.faces.shape) == want_f.shape, name
            assert np.array_equal(out.faces.cpu().numpy(), want_f) and np.array_equal(out.vertex_map.cpu().numpy(), want_map), name
            assert out.vertices.cpu().numpy().tobytes() == want_v.tobytes() and out.vertices.shape[0] == want_v.shape[0], name
    none = ops.mesh.filter_components(tv, tf, table, torch.zeros(C, dtype=torch.uint8, device=DEV))
    assert tuple(none.vertices.shape) == (0, 3) and tuple(none.faces.shape) == (0, 3)


def test_bad_input_is_refused():
    from vtaco_amd import ops
    from vtaco_amd._lib import VtError
    v, f = R.tetrahedron()
    tv, tf = _dev(v, f)
    with pytest.raises(VtError, match="HIP device"):
        ops.mesh.components(tf.cpu(), 4)
    with pytest.raises(VtError, match="int32"):
        ops.mesh.components(tf.long(), 4)                   # int64 faces are refused, not converted
    with pytest.raises(VtError, match="F = 0"):
        ops.mesh.components(tf[:0], 4)
    with pytest.raises(VtError, match=r"outside \[0, V\)"):
        ops.mesh.components(tf, 3)                          # index 3 >= V: found on the device, never dereferenced
    bad = tf.clone()
    bad[2, 1] = -1
    with pytest.raises(VtError, match=r"outside \[0, V\)"):
        ops.mesh.components(bad, 4)
    labels = ops.mesh.components(tf, 4)
    assert labels.tolist() == [0, 0, 0, 0]
    with pytest.raises(VtError, match=r"outside \[0, V\)"):
        ops.mesh.component_table(bad, labels)
    table = ops.mesh.component_table(tf, labels)
    with pytest.raises(VtError, match="float32 or float64"):
        ops.mesh.component_stats(tv.half(), tf, table)
    with pytest.raises(VtError, match="keep"):
        ops.mesh.filter_components(tv, tf, table, torch.ones(2, dtype=torch.uint8, device=DEV))
    with pytest.raises(VtError, match=r"outside \[0, V\)"):
        ops.mesh.filter_components(tv, bad, table, torch.ones(1, dtype=torch.uint8, device=DEV))
