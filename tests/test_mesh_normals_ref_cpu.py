"""CPU: the restatement of csrc/mesh_normals.hip (tests/mesh_normals_ref.py) against itself -- its two-limb integer sums against
math.fsum, known normals of simple meshes, independence of the order of the faces -- and NormalMesh / Mesh.export, which need no device."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mesh_normals_ref as R  # noqa: E402


@pytest.mark.parametrize("weight", R.WEIGHTS)
@pytest.mark.parametrize("name", sorted(R.MESHES))
def test_fixed_point_sums_equal_fsum(name, weight):
    v, f = R.MESHES[name]()
    fn, vn = R.normals(v, f, weight)
    ref = R.vertex_normals_fsum(v, f, weight)
    # the integer sums are exact to 2^-62 of the largest term; both sides then square, add, take a root and divide in float64
    assert np.abs(vn - ref).max() <= 4 * 2.0 ** -53, (name, weight, np.abs(vn - ref).max())
    length = np.linalg.norm(vn, axis=1)
    assert np.all((np.abs(length - 1) < 1e-15) | (length == 0))
    flen = np.linalg.norm(fn, axis=1)
    assert np.all((np.abs(flen - 1) < 1e-15) | (flen == 0))


@pytest.mark.parametrize("weight", R.WEIGHTS)
def test_permuted_faces_equal_bits(weight):
    v, f = R.fan()
    perm = np.random.RandomState(0).permutation(len(f))
    fn, vn = R.normals(v, f, weight)
    fn2, vn2 = R.normals(v, f[perm], weight)
    assert vn.tobytes() == vn2.tobytes() and fn[perm].tobytes() == fn2.tobytes()


def test_known_normals():
    v, f = R.tetrahedron()
    fn, vn = R.normals(v, f)
    s = 1 / np.sqrt(3.0)
    assert np.allclose(fn, [[0, 0, -1], [0, -1, 0], [s, s, s], [-1, 0, 0]], atol=1e-15)
    assert np.allclose(vn[0], [-s, -s, -s], atol=1e-15)                     # three unit right triangles meet in the origin
    v, f = R.cube_degenerate_spare()
    for weight in R.WEIGHTS:
        fn, vn = R.normals(v, f, weight)
        assert np.array_equal(fn[12:], np.zeros((2, 3)))                       # the two degenerate faces
        assert np.array_equal(vn[8], np.zeros(3)) and np.array_equal(vn[9], np.zeros(3))     # unreferenced; on a degenerate face only
        c = v[:8].astype(np.float64) - v[:8].astype(np.float64).mean(0)
        assert np.allclose(vn[:8], c / np.linalg.norm(c, axis=1, keepdims=True), atol=1e-6 if weight == "angle" else 0.5)
    # area and angle weights differ where the faces around a vertex differ: the cube's corners split 1 or 2 triangles per side
    assert np.abs(R.normals(v, f, "area")[1][:8] - R.normals(v, f, "angle")[1][:8]).max() > 0.05


def _read_ply(path):
    lines = open(path).read().split("\n")
    end = lines.index("end_header")
    props = [l.split()[2] for l in lines[:end] if l.startswith("property") and "list" not in l]
    nv = int([l for l in lines[:end] if l.startswith("element vertex")][0].split()[2])
    rows = np.array([[float(x) for x in l.split()] for l in lines[end + 1:end + 1 + nv]])
    return props, rows


def test_normal_mesh_and_export(tmp_path):
    from vtaco_amd._lib import VtError
    from vtaco_amd.conv_onet.generation import Mesh, NormalMesh
    v, f = R.torus()
    _, vn = R.normals(v, f)
    vn32 = vn.astype(np.float32)
    m = NormalMesh(v, f, vertex_normals=vn32)
    plain = Mesh(v, f)
    a, b = m
    assert a is v and b is f and len(m) == 2 and m.vertices is v and m.faces is f
    assert isinstance(m, Mesh) and m.normals_source == "geometry" and m.values is None and m.vertex_normals is vn32
    assert tuple.__eq__(m, plain)
    with pytest.raises(VtError):
        NormalMesh(v, f)
    with pytest.raises(VtError):
        NormalMesh(v, f, vertex_normals=vn32[:-1])
    with pytest.raises(VtError):
        NormalMesh(v, f, vertex_normals=vn32, normals_source="guess")
    # a plain Mesh writes the bytes it wrote before; OFF is the same for both
    for ext in ("ply", "obj", "off"):
        plain.export(str(tmp_path / f"plain.{ext}"))
        m.export(str(tmp_path / f"normal.{ext}"))
    assert open(tmp_path / "plain.off").read() == open(tmp_path / "normal.off").read()
    head = open(tmp_path / "plain.ply").read().split("end_header")[0]
    assert "nx" not in head and "vn " not in open(tmp_path / "plain.obj").read()
    props, rows = _read_ply(tmp_path / "normal.ply")
    assert props == ["x", "y", "z", "nx", "ny", "nz"]
    assert rows[:, :3].astype(np.float32).tobytes() == v.tobytes() and rows[:, 3:].astype(np.float32).tobytes() == vn32.tobytes()
    obj = open(tmp_path / "normal.obj").read().split("\n")
    got_v = np.array([[float(x) for x in l.split()[1:]] for l in obj if l.startswith("v ")], dtype=np.float32)
    got_n = np.array([[float(x) for x in l.split()[1:]] for l in obj if l.startswith("vn ")], dtype=np.float32)
    got_f = np.array([[[int(x) for x in c.split("//")] for c in l.split()[1:]] for l in obj if l.startswith("f ")])
    assert got_v.tobytes() == v.tobytes() and got_n.tobytes() == vn32.tobytes()
    assert np.array_equal(got_f[:, :, 0] - 1, f) and np.array_equal(got_f[:, :, 0], got_f[:, :, 1])
