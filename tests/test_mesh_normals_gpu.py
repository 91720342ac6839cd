"""GPU: csrc/mesh_normals.hip through ops.mesh.normals, utils/mesh_clean and the Mesh methods against the numpy float64 restatement
(tests/mesh_normals_ref.py).  Every component of a face or vertex normal lies within 2 roundings of the restatement (2 * 2^-24 for float32
outputs; 2 * 2^-53 for float64 outputs with weight='area', float32's gate with 'angle': see the restatement's docstring), a second run
gives equal bits, and so does a random permutation of the faces."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mesh_normals_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GATE32, GATE64 = 2 * 2.0 ** -24, 2 * 2.0 ** -53


def _dev(v, f):
    return torch.from_numpy(np.ascontiguousarray(v)).to(DEV), torch.from_numpy(np.ascontiguousarray(f)).to(DEV)


def _check(name, v, f, weight, gate):
    from vtaco_amd import ops
    tv, tf = _dev(v, f)
    got, again = ops.mesh.normals(tv, tf, weight=weight), ops.mesh.normals(tv, tf, weight=weight)
    ref_fn, ref_vn = R.normals(v, f, weight)
    for k, ref in (("face_normals", ref_fn), ("vertex_normals", ref_vn)):
        g = getattr(got, k).cpu().numpy()
        assert g.dtype == v.dtype and g.shape == ref.shape, (name, k)
        assert g.tobytes() == getattr(again, k).cpu().numpy().tobytes(), (name, k)
        err = float(np.abs(g.astype(np.float64) - ref).max())
        print(f"ERR gpu {name} {weight} {k}: {err:.3e} (gate {gate:.3e})")
        assert np.all(np.isfinite(g)) and err <= gate, (name, weight, k, err)
        assert np.array_equal(np.all(g == 0, axis=1), np.all(ref == 0, axis=1)), (name, k)
    # the faces in another order: the same vertex normals bit for bit, the face normals moved with their faces
    perm = np.random.RandomState(11).permutation(len(f))
    shuffled = ops.mesh.normals(tv, tf[torch.from_numpy(perm).to(DEV)].contiguous(), weight=weight)
    assert torch.equal(shuffled.vertex_normals, got.vertex_normals), (name, weight)
    assert torch.equal(shuffled.face_normals, got.face_normals[torch.from_numpy(perm).to(DEV)]), (name, weight)
    # one output at a time gives the same bits
    only_f = ops.mesh.normals(tv, tf, weight=weight, vertex=False)
    only_v = ops.mesh.normals(tv, tf, weight=weight, face=False)
    assert only_f.vertex_normals is None and only_v.face_normals is None
    assert torch.equal(only_f.face_normals, got.face_normals) and torch.equal(only_v.vertex_normals, got.vertex_normals)
    return got


@pytest.mark.parametrize("weight", R.WEIGHTS)
@pytest.mark.parametrize("name", sorted(R.MESHES))
def test_float32(name, weight):
    v, f = R.MESHES[name]()
    got = _check(name, v, f, weight, GATE32)
    if name == "cube_degenerate_spare":
        assert not got.face_normals[12:].any() and not got.vertex_normals[8:].any()
    if name == "fan1000":
        assert torch.bincount(torch.from_numpy(f).reshape(-1))[0] == 1000


@pytest.mark.parametrize("name", ["torus16x8", "fan1000", "cube_degenerate_spare"])
def test_float64_area(name):
    v, f = R.MESHES[name]()
    v = v.astype(np.float64) + 1e-9 * np.random.RandomState(2).randn(*v.shape)
    if name == "cube_degenerate_spare":
        v[9] = v[0]                                              # (the perturbation took it off the edge: put it on a corner)
    _check(name + "_f64", v, f, "area", GATE64)


def test_float64_angle():
    v, f = R.torus()
    v = v.astype(np.float64) + 1e-9 * np.random.RandomState(3).randn(*v.shape)
    _check("torus_f64", v, f, "angle", GATE32)


def test_more_than_one_block_and_ragged_tail():
    v, f = R.torus(41, 19)                                       # 1558 faces: seven workgroups, the last one partly filled
    assert len(f) % 256 != 0 and len(f) > 1024
    _check("torus41x19", v, f, "area", GATE32)
    _check("torus41x19", v, f, "angle", GATE32)


def test_mesh_methods_and_mesh_clean():
    from vtaco_amd import ops
    from vtaco_amd.conv_onet.generation import Mesh, NormalMesh
    from vtaco_amd.utils import mesh_clean
    v, f = R.torus()
    tv, tf = _dev(v, f)
    mesh = Mesh(tv, tf)
    both = ops.mesh.normals(tv, tf)
    assert torch.equal(mesh.face_normals(), both.face_normals) and torch.equal(mesh.vertex_normals(), both.vertex_normals)
    assert torch.equal(mesh_clean.face_normals((tv, tf.long())), both.face_normals)
    assert torch.equal(mesh_clean.vertex_normals(mesh, weight="angle"), ops.mesh.normals(tv, tf, weight="angle").vertex_normals)
    nm = mesh.with_vertex_normals()
    assert isinstance(nm, NormalMesh) and nm.normals_source == "geometry" and nm.values is None
    assert torch.equal(nm.vertex_normals, both.vertex_normals) and nm.vertices is tv
    assert torch.equal(nm.geometric_vertex_normals(), both.vertex_normals)
    empty = Mesh(tv, tf[:0])
    assert tuple(empty.face_normals().shape) == (0, 3) and not empty.vertex_normals().any()
    assert tuple(empty.vertex_normals().shape) == tuple(tv.shape)


def test_refused_inputs():
    from vtaco_amd import ops
    from vtaco_amd._lib import VtError
    from vtaco_amd.utils import mesh_clean
    v, f = R.tetrahedron()
    tv, tf = _dev(v, f)
    bad = tf.clone()
    bad[2, 1] = 4                                                # one past the last vertex
    with pytest.raises(VtError, match="outside"):
        ops.mesh.normals(tv, bad)
    bad[2, 1] = -1
    with pytest.raises(VtError, match="outside"):
        ops.mesh.normals(tv, bad, vertex=False)
    with pytest.raises(VtError):
        ops.mesh.normals(tv, tf.long())
    with pytest.raises(VtError):
        ops.mesh.normals(tv.cpu(), tf)
    with pytest.raises(VtError):
        ops.mesh.normals(tv.half(), tf)
    with pytest.raises(VtError):
        ops.mesh.normals(tv, tf, weight="uniform")
    with pytest.raises(VtError):
        ops.mesh.normals(tv, tf, face=False, vertex=False)
    with pytest.raises(VtError):
        ops.mesh.normals(tv, tf[:0])
    with pytest.raises(VtError):
        mesh_clean.vertex_normals((tv, tf), weight="uniform")
    # the device is as it was: the next call answers
    assert torch.isfinite(ops.mesh.normals(tv, tf).vertex_normals).all()
