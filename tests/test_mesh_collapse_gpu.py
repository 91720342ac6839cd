"""GPU: csrc/mesh_collapse.hip through ops.mesh.collapse and utils/mesh_clean.decimate_report against the numpy definition
(tests/mesh_collapse_ref.py): the faces, the vertices byte for byte, vertex_map, rounds and stalled are equal; every case runs twice and the
two runs are equal bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mesh_collapse_ref as C  # noqa: E402
import mesh_topo_ref as T  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _dev(v, f):
    return torch.from_numpy(np.ascontiguousarray(v)).to(DEV), torch.from_numpy(np.ascontiguousarray(f)).to(DEV)


def _check(name, v, f, nfaces, **how):
    """ops.mesh.collapse of the mesh, twice, against the definition; returns (result, definition)."""
    from vtaco_amd import ops
    tv, tf = _dev(v, f)
    got, again = (ops.mesh.collapse(tv, tf, nfaces, **how) for _ in range(2))
    ref = C.collapse(v, f, nfaces, **how)
    assert torch.equal(got.vertices, again.vertices) and torch.equal(got.faces, again.faces) and torch.equal(got.vertex_map, again.vertex_map), name
    assert got[3:] == again[3:] == (ref["rounds"], ref["stalled"]), (name, got[3:], again[3:], ref["rounds"], ref["stalled"])
    faces = got.faces.cpu().numpy()
    assert faces.dtype == np.int32 and faces.shape == ref["faces"].shape and np.array_equal(faces, ref["faces"]), name
    vmap = got.vertex_map.cpu().numpy()
    assert vmap.dtype == np.int32 and np.array_equal(vmap, ref["vertex_map"]), name
    pos = got.vertices.cpu().numpy()
    K = ref["vertices"].shape[0]
    assert pos.dtype == v.dtype and pos.shape == (K, 3), name
    differ = np.nonzero((pos.view(np.uint8).reshape(K, -1) != ref["vertices"].view(np.uint8).reshape(K, -1)).any(1))[0]
    assert differ.size == 0, (name, differ[:8], pos[differ[:4]], ref["vertices"][differ[:4]])
    return got, ref


def _two_tori():
    v, f = T.torus(16, 32)
    return C.together(T.torus(8, 16), (v + np.float32(4.0), f))


def test_tetrahedron_stalls_and_octahedron_loses_one_edge():
    got, _ = _check("tetrahedron", *T.tetrahedron(), 2)
    assert got.stalled and got.rounds == 0 and got.faces.shape[0] == 4
    got, _ = _check("octahedron", *C.octahedron(), 6)
    assert not got.stalled and got.rounds == 1 and got.faces.shape[0] == 6 and got.vertices.shape[0] == 5


@pytest.mark.parametrize("n_faces", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_grid_strip_has_nothing_to_collapse(n_faces):
    from vtaco_amd import ops
    v, f = T.grid_strip(n_faces)
    if n_faces == 1:                                 # no target lies below one face: the same tensors come back
        tv, tf = _dev(v, f)
        got = ops.mesh.collapse(tv, tf, 1)
        assert got.vertices is tv and got.faces is tf and got[2:] == (None, 0, False)
        return
    got, _ = _check(f"strip{n_faces}", v, f, 1)
    assert got.stalled and got.rounds == 0 and np.array_equal(got.faces.cpu().numpy(), f)
    assert got.vertices.cpu().numpy().tobytes() == v[:got.vertices.shape[0]].tobytes()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_open_patch(dtype):
    v, f = C.quad_patch(12, dtype)
    got, _ = _check("patch", v, f, 100)
    assert got.faces.shape[0] == 100 and not got.stalled


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("placement", C.PLACEMENTS)
def test_torus_8x16(dtype, placement):
    v, f = T.torus(8, 16)
    v = v.astype(dtype)
    if dtype == np.float64:
        v = v + 1e-9 * np.random.RandomState(2).randn(*v.shape)
    got, _ = _check("torus8x16", v, f, 100, placement=placement)
    assert got.faces.shape[0] == 100 and not got.stalled


def test_torus_16x32_and_an_odd_count():
    got, _ = _check("torus16x32", *T.torus(16, 32), 300)
    assert got.faces.shape[0] == 300
    got, _ = _check("torus16x32 odd", *T.torus(16, 32), 701)
    assert got.faces.shape[0] == 700 and not got.stalled


def test_torus_32x64_tables_and_scans_span_many_blocks():
    got, ref = _check("torus32x64", *T.torus(32, 64), 3000)
    assert got.faces.shape[0] == 3000 and 1 <= got.rounds <= 16
    from vtaco_amd.utils import mesh_clean
    comps = mesh_clean.components((got.vertices, got.faces)).report()
    assert comps["oriented"] == [True] and comps["euler"] == [0]


def test_two_tori():
    v, f = _two_tori()
    got, _ = _check("two tori", v, f, 200)
    assert got.faces.shape[0] == 200


def test_fin():
    v, f, (a, b) = C.fin_mesh()
    got, _ = _check("fin", v, f, 30)
    vmap = got.vertex_map.cpu().numpy()
    assert vmap[a] != vmap[b] and got.rounds >= 1


def test_a_face_with_two_equal_corners_rides_along():
    v, f = T.torus(8, 16)
    extra = np.array([[5, 5, 40], [7, 60, 60]], dtype=np.int32)
    got, _ = _check("degenerate", v, np.concatenate([f[:50], extra, f[50:]]), 102)
    assert got.faces.shape[0] == 102 and not got.stalled


def test_a_face_without_area_has_no_say_on_flips():
    v, f, corners = C.sliver_torus()
    got, _ = _check("sliver", v, f, 60)
    assert got.faces.shape[0] == 60 and not got.stalled
    got, _ = _check("sliver f64", v.astype(np.float64), f, 100, placement="midpoint")
    assert got.faces.shape[0] == 100


def test_one_round_is_the_definitions_first_round():
    v, f = T.torus(16, 32)
    got, ref = _check("one round", v, f, 300, max_rounds=1)
    assert got.rounds == 1 and 300 < got.faces.shape[0] < f.shape[0]
    got3, _ = _check("three rounds", v, f, 300, max_rounds=3)           # (a batch of four rounds holds the fourth back)
    assert got3.rounds == 3 and got3.faces.shape[0] < got.faces.shape[0]
    got5, _ = _check("five rounds", v, f, 300, max_rounds=5)            # (the bound falls inside the second batch)
    assert got5.rounds == 5


def test_at_most_nfaces_already_returns_the_same_objects():
    from vtaco_amd import ops
    from vtaco_amd.conv_onet.generation import Mesh
    from vtaco_amd.utils import mesh_clean
    tv, tf = _dev(*T.torus(8, 16))
    for n in (256, 257, 10 ** 6):
        got = ops.mesh.collapse(tv, tf, n)
        assert got.vertices is tv and got.faces is tf and got[2:] == (None, 0, False)
    mesh = Mesh(tv, tf)
    same, rep = mesh_clean.decimate_report(mesh, 256)
    assert same is mesh and rep == (0, False, None) and mesh.decimate(300) is mesh


def test_decimate_report_and_mesh_methods():
    from vtaco_amd.conv_onet.generation import Mesh, NormalMesh
    from vtaco_amd.utils import mesh_clean
    v, f = T.torus(8, 16)
    ref = C.collapse(v, f, 101)
    tv, tf = _dev(v, f)
    mesh = Mesh(tv, tf)
    got, rep = mesh.decimate_report(101)
    assert isinstance(got, Mesh) and (rep.rounds, rep.stalled) == (ref["rounds"], ref["stalled"])
    assert np.array_equal(got.faces.cpu().numpy(), ref["faces"]) and got.vertices.cpu().numpy().tobytes() == ref["vertices"].tobytes()
    assert np.array_equal(rep.vertex_map.cpu().numpy(), ref["vertex_map"])
    again = mesh_clean.decimate((tv, tf.long()), 101)                  # (int64 faces are converted, as everywhere in mesh_clean)
    assert torch.equal(again.faces, got.faces) and torch.equal(again.vertices, got.vertices)
    normal = mesh_clean.with_vertex_normals(mesh)
    out = normal.decimate(101, placement="midpoint")
    assert isinstance(out, NormalMesh) and out.normals_source == "geometry" and out.vertex_normals.shape == out.vertices.shape
    assert torch.equal(out.vertex_normals, mesh_clean.vertex_normals(Mesh(out.vertices, out.faces)))
    c = got.components().report()
    assert c["oriented"] == [True] and c["euler"] == [0] and c["n_faces"] == [100]


def test_unreferenced_vertices_map_to_minus_one():
    v, f = T.torus(8, 16)
    v2 = np.concatenate([[[9, 9, 9]], v, [[np.nan, 0, 0]]]).astype(np.float32)
    got, _ = _check("spares", v2, f + 1, 100)
    vmap = got.vertex_map.cpu().numpy()
    assert vmap[0] == -1 and vmap[-1] == -1 and (vmap[1:-1] >= 0).all()


def test_bad_input_raises_and_a_valid_call_afterwards_passes():
    from vtaco_amd import ops
    from vtaco_amd._lib import VtError
    v, f = T.torus(8, 16)
    bad = f.copy()
    bad[3, 1] = v.shape[0]
    with pytest.raises(VtError, match="outside"):
        ops.mesh.collapse(*_dev(v, bad), 100)
    bad[3, 1] = -1
    with pytest.raises(VtError, match="outside"):
        ops.mesh.collapse(*_dev(v, bad), 100)
    nan = v.copy()
    nan[7, 2] = np.nan
    with pytest.raises(VtError, match="non-finite"):
        ops.mesh.collapse(*_dev(nan, f), 100)
    tv, tf = _dev(v, f)
    for kw in (dict(nfaces=0), dict(nfaces=1.5), dict(nfaces=100, placement="best"), dict(nfaces=100, max_rounds=0)):
        with pytest.raises(VtError):
            ops.mesh.collapse(tv, tf, **kw)
    with pytest.raises(VtError, match="int32"):
        ops.mesh.collapse(tv, tf.long(), 100)
    lib = ops._lib.load()
    assert lib.vt_mesh_collapse_workspace_bytes(0, 5) == 0 and lib.vt_mesh_collapse_workspace_bytes(200, 300) > 0
    _check("after the errors", v, f, 100)
