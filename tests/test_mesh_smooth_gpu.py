"""GPU: csrc/mesh_smooth.hip through ops.mesh and utils/mesh_clean against the definition (tests/mesh_smooth_ref.py).  Everything is equal
bit for bit -- offsets, neighbours, both flag arrays, the weights and the smoothed positions, in float32 and float64 -- and every call is
made twice with equal results.  The fixtures are the places the kernels can go wrong: the smallest closed mesh, no faces at all, a row of
300 entries, unreferenced vertices, repeated faces and indices, an edge with three faces, coincident neighbours, and marching-cubes spheres
of several workgroups with a ragged tail, closed and cut by their box."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mesh_smooth_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAMES = sorted(R.FIXTURES)
KEYS = ("offsets", "neighbors", "boundary_edge", "boundary_vertex")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return (a.cpu().numpy() if torch.is_tensor(a) else np.ascontiguousarray(a)).tobytes()


def _f64(name, v):
    """The fixture's float64 version: values that no float32 holds, except on the integer grid (whose fixed points are exact)."""
    v64 = v.astype(np.float64)
    return v64 if name == "grid9" else v64 * 1.0000000123


def _adjacency(f, V):
    """(device adjacency, the definition's), compared with each other and with a second call."""
    from vtaco_amd import ops
    ref = R.adjacency(f, V)
    tf = _t(f)
    got, again = ops.mesh.vertex_adjacency(tf, V), ops.mesh.vertex_adjacency(tf, V)
    for k in KEYS:
        g = getattr(got, k)
        assert g.dtype == (torch.int32 if k in KEYS[:2] else torch.uint8) and g.cpu().numpy().dtype == ref[k].dtype, k
        assert np.array_equal(g.cpu().numpy(), ref[k]), k
        assert torch.equal(g, getattr(again, k)), k
    return got, ref


def _smooth(v, adj, ref, **kw):
    """ops.mesh.smooth twice, equal to each other and to the definition bit for bit; returns the result."""
    from vtaco_amd import ops
    rkw = dict(kw)
    if "weights" in rkw:
        rkw["weights_scheme"] = rkw.pop("weights")
    want = R.smooth(v, ref, **rkw)
    tv = _t(v)
    got, again = ops.mesh.smooth(tv, adj, **kw), ops.mesh.smooth(tv, adj, **kw)
    assert got.dtype == tv.dtype and got.data_ptr() != tv.data_ptr() and _bits(tv) == _bits(v)
    assert _bits(got) == _bits(again), kw
    assert _bits(got) == _bits(want), (kw, float(np.abs(got.cpu().numpy().astype(np.float64) - want.astype(np.float64)).max()))
    # one launch per pass, and every pass in one workgroup where the mesh fits: equal bits
    forms = ("launches", "workgroup") if v.shape[0] <= ops.mesh.SMOOTH_WORKGROUP_MAX_V else ("launches",)
    for form in forms:
        a, b = ops.mesh.smooth(tv, adj, form=form, **kw), ops.mesh.smooth(tv, adj, form=form, **kw)
        assert _bits(a) == _bits(b) == _bits(want), (form, kw)
    return got


@pytest.fixture(scope="module")
def spheres():
    from vtaco_amd import ops
    out = {}
    for key, radius, counts in (("closed", R.CLOSED_RADIUS, (1296, 2588)), ("cut", R.CUT_RADIUS, (1968, 3560))):
        verts, faces, _ = ops.marching_cubes(_t(R.sphere_volume(radius)), level=0.0)
        v, f = verts.cpu().numpy(), faces.cpu().numpy()
        assert (v.shape[0], f.shape[0]) == counts and v.dtype == np.float32
        adj, ref = _adjacency(f, v.shape[0])
        out[key] = (v, f, adj, ref)
    assert int(out["cut"][3]["boundary_vertex"].sum()) == 384 and not out["closed"][3]["boundary_vertex"].any()
    return out


@pytest.mark.parametrize("name", NAMES)
def test_fixture(name):
    v, f = R.fixture(name)
    adj, ref = _adjacency(f, v.shape[0])
    rules = R.BOUNDARIES if name == "grid9" else ("pin", "free")
    for x in (v.astype(np.float32), _f64(name, v)):
        for method, boundary in itertools.product(R.METHODS, rules):
            got = _smooth(x, adj, ref, method=method, iterations=2, boundary=boundary)
            if name == "empty":
                assert _bits(got) == _bits(x)                              # F = 0: the input comes back
            if name == "grid9" and boundary == "pin":
                assert _bits(got) == _bits(x)                              # interior vertices are exact fixed points
        if name in ("coincident", "fan300", "tetrahedron"):
            for method in R.METHODS:
                got = _smooth(x, adj, ref, method=method, iterations=3, weights="inverse_distance", boundary="free")
                assert bool(torch.isfinite(got).all())
                if name == "coincident":
                    assert _bits(got[5:]) == _bits(x[5:])                  # every weight 0: the vertex stays


@pytest.mark.parametrize("V", [1022, 1023, 1024])
def test_offsets_at_the_scan_chunk(V):
    """The scan that writes offsets, in the caller's array and in the workspace, runs over V + 1 = 1023, 1024 and 1025 elements: below, on
    and above its 1 024-element chunk.  The strip has 1 004 vertices; the ones past it are unreferenced and their rows are empty."""
    v, f = R.T.grid_strip(1000)
    assert v.shape[0] == 1004
    got, ref = _adjacency(f, V)
    assert got.offsets.numel() == V + 1 and int(got.offsets[-1]) == ref["neighbors"].shape[0]


def test_more_than_256_scan_blocks():
    """87 382 disjoint triangles: the V + 1 = 262 147 offsets take 257 blocks of the scan, so the one workgroup that scans the block sums
    goes round its loop twice and carries a sum over."""
    n = 87382
    f = np.arange(3 * n, dtype=np.int32).reshape(n, 3)
    assert -(-(3 * n + 1) // 1024) == 257
    got, ref = _adjacency(f, 3 * n)
    assert got.neighbors.numel() == ref["neighbors"].shape[0] == 524292


def test_weights_are_the_definitions(spheres):
    from vtaco_amd import ops
    cases = [(n,) + R.fixture(n) for n in ("coincident", "fan300", "odd")] + [("cut",) + spheres["cut"][:2]]
    for name, v, f in cases:
        adj = ops.mesh.vertex_adjacency(_t(f), v.shape[0])
        ref = R.adjacency(f, v.shape[0])
        for x in (v.astype(np.float32), _f64(name, v)):
            for scheme in R.WEIGHTS:
                got, again = ops.mesh.smooth_weights(_t(x), adj, scheme), ops.mesh.smooth_weights(_t(x), adj, scheme)
                assert got.dtype == torch.float64 and bool(torch.isfinite(got).all())
                assert _bits(got) == _bits(again) == _bits(R.weights(x, ref, scheme)), (name, scheme, x.dtype)


@pytest.mark.parametrize("method", R.METHODS)
def test_iteration_counts(spheres, method):
    v, f, adj, ref = spheres["cut"]
    tv, tf = R.fixture("tetrahedron")
    tadj, tref = _adjacency(tf, 4)
    for n in (0, 1, 2, 3, 7):                                              # both parities of the buffers, and none
        got = _smooth(v, adj, ref, method=method, iterations=n)
        assert (_bits(got) == _bits(v)) == (n == 0)
        _smooth(v.astype(np.float64) * 1.0000000123, adj, ref, method=method, iterations=n, boundary="free")
        _smooth(tv, tadj, tref, method=method, iterations=n)


@pytest.mark.parametrize("weights", R.WEIGHTS)
@pytest.mark.parametrize("boundary", R.BOUNDARIES)
@pytest.mark.parametrize("method", R.METHODS)
def test_every_combination_on_the_cut_sphere(spheres, method, boundary, weights):
    v, f, adj, ref = spheres["cut"]
    bv = ref["boundary_vertex"].astype(bool)
    for x in (v, v.astype(np.float64) * 1.0000000123):
        got = _smooth(x, adj, ref, method=method, iterations=3, weights=weights, boundary=boundary).cpu().numpy()
        if boundary == "pin":
            assert _bits(got[bv]) == _bits(x[bv])
        else:
            assert (got[bv] != x[bv]).any()
        assert (got[~bv] != x[~bv]).any()
    _smooth(spheres["closed"][0], spheres["closed"][2], spheres["closed"][3], method=method, weights=weights, boundary=boundary)    # the defaults


@pytest.mark.parametrize("extra", [0, 1])
def test_where_the_form_changes(extra):
    """2 048 vertices are the most one workgroup holds (three float64 buffers in LDS); one more goes by launches."""
    from vtaco_amd import ops
    from vtaco_amd._lib import VtError
    import mesh_topo_ref as T
    v, f = T.torus(32, 64)
    assert v.shape[0] == ops.mesh.SMOOTH_WORKGROUP_MAX_V == 2048
    v = np.concatenate([v, np.ones((extra, 3), dtype=np.float32)])
    adj, ref = _adjacency(f, v.shape[0])
    for method in R.METHODS:
        for x in (v, v.astype(np.float64) * 1.0000000123):
            _smooth(x, adj, ref, method=method, iterations=3, weights="inverse_distance", boundary="free")
    if extra:
        with pytest.raises(VtError, match="2048"):
            ops.mesh.smooth(_t(v), adj, form="workgroup")
    with pytest.raises(VtError, match="form"):
        ops.mesh.smooth(_t(v), adj, form="lds")


def test_faces_permuted_and_flipped(spheres):
    from vtaco_amd import ops
    rng = np.random.RandomState(7)
    for key in ("closed", "cut"):
        v, f, adj, ref = spheres[key]
        want = ops.mesh.smooth(_t(v), adj, "taubin", 4, boundary="loop", weights="inverse_distance")
        for other in (f[rng.permutation(f.shape[0])], np.ascontiguousarray(f[:, ::-1]), np.roll(f, 1, axis=1)):
            again = ops.mesh.vertex_adjacency(_t(other), v.shape[0])
            assert all(torch.equal(getattr(adj, k), getattr(again, k)) for k in KEYS), key
            assert torch.equal(ops.mesh.smooth(_t(v), again, "taubin", 4, boundary="loop", weights="inverse_distance"), want), key


def test_mesh_methods_and_report(spheres):
    from vtaco_amd import ops
    from vtaco_amd.conv_onet.generation import Mesh, NormalMesh
    from vtaco_amd.utils import mesh_clean
    v, f, adj, ref = spheres["cut"]
    mesh = Mesh(_t(v), _t(f))
    nb = mesh.vertex_neighbors()
    assert all(torch.equal(getattr(nb, k), getattr(adj, k)) for k in KEYS)
    assert np.array_equal(mesh.vertex_degree().cpu().numpy(), np.diff(ref["offsets"])) and int(mesh.boundary_vertices().sum()) == 384
    out, rep = mesh.smooth_report("taubin", 10)
    assert isinstance(out, Mesh) and out.faces is mesh.faces and _bits(out.vertices) == _bits(R.smooth(v, ref, "taubin", 10))
    assert torch.equal(mesh.smooth("taubin", 10, adjacency=adj).vertices, out.vertices)
    assert torch.equal(mesh_clean.smooth((mesh.vertices, mesh.faces.long())).vertices, out.vertices)       # int64 faces are converted here
    for m, area, volume in ((mesh, rep.area_before, rep.volume_before), (out, rep.area_after, rep.volume_after)):
        comps = m.components()
        assert area == float(comps.area.sum()) and volume == float(comps.volume.sum())
    d = np.linalg.norm(out.vertices.cpu().numpy().astype(np.float64) - v.astype(np.float64), axis=1)
    assert rep.n_pinned == 384 and rep.max_displacement == pytest.approx(d.max(), rel=1e-12)
    assert rep.rms_displacement == pytest.approx(np.sqrt((d * d).mean()), rel=1e-12) and 0 < rep.rms_displacement < rep.max_displacement
    assert mesh.smooth_report("humphrey", 2, boundary="free")[1].n_pinned == 0
    # a NormalMesh comes back with the normals of the new geometry
    nm = NormalMesh(mesh.vertices, mesh.faces, vertex_normals=torch.ones_like(mesh.vertices), values=torch.zeros(v.shape[0], device=DEV),
                    normals_source="marching_cubes")
    sm = nm.smooth("humphrey", 3)
    assert isinstance(sm, NormalMesh) and sm.normals_source == "geometry" and sm.values is None
    assert torch.equal(sm.vertices, mesh.smooth("humphrey", 3).vertices)
    assert torch.equal(sm.vertex_normals, ops.mesh.normals(sm.vertices, sm.faces, face=False).vertex_normals)


def test_bad_input_is_refused(spheres):
    from vtaco_amd import ops
    from vtaco_amd._lib import VtError
    v, f, adj, _ = spheres["closed"]
    tv, tf = _t(v), _t(f)
    bad = tf.clone()
    bad[5, 1] = v.shape[0]
    with pytest.raises(VtError, match=r"outside \[0, V\)"):
        ops.mesh.vertex_adjacency(bad, v.shape[0])
    bad[5, 1] = -1
    with pytest.raises(VtError, match=r"outside \[0, V\)"):
        ops.mesh.vertex_adjacency(bad, v.shape[0])
    with pytest.raises(VtError, match="int32"):
        ops.mesh.vertex_adjacency(tf.long(), v.shape[0])
    with pytest.raises(VtError, match="offsets"):
        ops.mesh.smooth(tv[:-1], adj)                                      # an adjacency of another mesh
    with pytest.raises(VtError, match="MeshAdjacency"):
        ops.mesh.smooth(tv, tuple(adj))
    with pytest.raises(VtError, match="float32 or float64"):
        ops.mesh.smooth(tv.half(), adj)
    with pytest.raises(VtError, match="mu < -lam"):
        ops.mesh.smooth(tv, adj, mu=-0.4)
