"""GPU: csrc/mesh_subdivide.hip through ops.mesh, utils/mesh_clean and UpSampleLayer against the definition (tests/mesh_subdivide_ref.py)
and the real reference layer's outputs (tests/golden/g31_subdivide.npz).  Everything is equal bit for bit -- vertices, faces, edge pairs,
face parents and counts, in float32 and float64, under every marking rule and both schemes -- and every call is made twice with equal
results.  The fixtures are the places the kernels can go wrong: no faces, one face, the smallest closed mesh, a vertex of degree 300, an
unreferenced vertex, a repeated face, an edge with four faces and a flipped face, half-edge counts one below, at and one above a multiple
of the scan chunk, and marching-cubes spheres of several workgroups with a ragged tail, closed and cut by their box."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mesh_smooth_ref as S  # noqa: E402
import mesh_subdivide_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAMES = sorted(R.FIXTURES)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g31_subdivide.npz")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return (a.cpu().numpy() if torch.is_tensor(a) else np.ascontiguousarray(a)).tobytes()


def _f64(name, v):
    """The fixture's float64 version: values that no float32 holds, except on the integer grids (whose fixed points are exact)."""
    v64 = v.astype(np.float64)
    return v64 if name in R.INTEGER_GRIDS else v64 * 1.0000000123


def _check(v, f, scheme="midpoint", **kw):
    """ops.mesh.subdivide twice, equal to each other and to the definition bit for bit; returns the definition's info."""
    from vtaco_amd import ops
    want_v, want_f, info = R.subdivide(v, f, scheme, **kw)
    tv, tf = _t(v), _t(f)
    tkw = {k: (_t(x) if k == "face_mask" else x) for k, x in kw.items()}
    outs = [ops.mesh.subdivide(tv, tf, scheme, **tkw) for _ in range(2)]
    for gv, gf, gi in outs:
        assert gv.dtype == tv.dtype and gf.dtype == torch.int32 and gi.edge_verts.dtype == torch.int32 and gi.face_parent.dtype == torch.int32
        assert (gi.n_marked, gi.n_irregular if gi.n_marked else 0) == (info["n_marked"], info["n_irregular"] if info["n_marked"] else 0), (scheme, kw)
        assert tuple(gv.shape) == want_v.shape and tuple(gf.shape) == want_f.shape
        assert np.array_equal(gf.cpu().numpy(), want_f), (scheme, kw)
        assert np.array_equal(gi.edge_verts.cpu().numpy(), info["edge_verts"]) and np.array_equal(gi.face_parent.cpu().numpy(), info["face_parent"])
        assert _bits(gv) == _bits(want_v), (scheme, kw, float(np.abs(gv.cpu().numpy().astype(np.float64) - want_v.astype(np.float64)).max()))
    assert _bits(tv) == _bits(v) and _bits(tf) == _bits(f)
    assert ops.mesh.subdivide_count(tv, tf, **tkw)[:2] == (info["n_marked"], want_f.shape[0])
    return info


def _modes(v, f):
    out = [dict()]
    if f.shape[0]:
        out.append(dict(max_edge=float(np.sqrt(np.median(R.edge_lengths2(v, f))))))
        one = np.zeros(f.shape[0], dtype=np.uint8)
        one[f.shape[0] // 2] = 1
        out += [dict(face_mask=one), dict(face_mask=1 - one)]
    return out


@pytest.fixture(scope="module")
def spheres():
    from vtaco_amd import ops
    out = {}
    for key, radius, counts in (("closed", S.CLOSED_RADIUS, (1296, 2588)), ("cut", S.CUT_RADIUS, (1968, 3560))):
        verts, faces, _ = ops.marching_cubes(_t(S.sphere_volume(radius)), level=0.0)
        v, f = verts.cpu().numpy(), faces.cpu().numpy()
        assert (v.shape[0], f.shape[0]) == counts and v.dtype == np.float32
        out[key] = (v, f)
    assert int(S.adjacency(out["cut"][1], 1968)["boundary_vertex"].sum()) == 384
    return out


@pytest.mark.parametrize("name", NAMES)
def test_fixture(name):
    v, f = R.fixture(name)
    for x in (v.astype(np.float32), _f64(name, v)):
        for kw in _modes(x, f):
            _check(x, f, "midpoint", **kw)
        info = _check(x, f, "loop")
        if name == "odd":
            assert info["n_irregular"] == 6
    if name == "empty":
        from vtaco_amd import ops
        tv, tf = _t(v), _t(f)
        gv, gf, gi = ops.mesh.subdivide(tv, tf)
        assert gv.data_ptr() == tv.data_ptr() and tuple(gf.shape) == (0, 3) and gi.n_marked == 0 and tuple(gi.edge_verts.shape) == (0, 2) and gi.face_parent.numel() == 0


def test_chunk_fixtures_sit_on_the_scan_chunk():
    assert [3 * R.fixture(n)[1].shape[0] - k * R.MT_CHUNK for n, k in (("chunk_below", 1), ("chunk_at", 3), ("chunk_above", 2))] == [-1, 0, 1]


def test_more_than_256_scan_blocks():
    """87 382 disjoint triangles: the 3 F = 262 146 first-use flags take 257 blocks of the scan, so the one workgroup that scans the block
    sums goes round its loop twice and carries a sum over.  Every edge is marked: 4 F faces."""
    n = 87382
    f = np.arange(3 * n, dtype=np.int32).reshape(n, 3)
    v = (np.arange(9 * n) % 97).astype(np.float32).reshape(3 * n, 3)
    assert -(-3 * n // R.MT_CHUNK) == 257
    info = _check(v, f)
    assert info["n_marked"] == 3 * n and info["face_parent"].shape[0] == 349528


def test_loop_leaves_the_ends_of_irregular_edges_in_place():
    from vtaco_amd import ops
    v, f = R.fixture("odd")
    tab = R.edge_table(f, v.shape[0])
    bad = (tab["fwd"] > 1) | (tab["bwd"] > 1)
    ends = np.unique(np.concatenate([tab["lo"][bad], tab["hi"][bad]]))
    gv, _, gi = ops.mesh.subdivide(_t(v), _t(f), "loop")
    assert gi.n_irregular == int(bad.sum()) == 6
    assert _bits(gv[torch.from_numpy(ends).to(DEV)]) == _bits(v[ends]) and _bits(gv[0]) == _bits(v[0])


@pytest.mark.parametrize("key", ["closed", "cut"])
def test_spheres(spheres, key):
    v, f = spheres[key]
    for x in (v, v.astype(np.float64) * 1.0000000123):
        for kw in _modes(x, f):
            _check(x, f, "midpoint", **kw)
        assert _check(x, f, "loop")["n_irregular"] == 0


def test_all_four_face_cases(spheres):
    v, f = R.fixture("stretched_torus")
    info = _check(v, f, max_edge=R.FOUR_CASES_MAX_EDGE)
    assert np.bincount(info["marks_per_face"], minlength=4).tolist() == [64, 64, 96, 32]
    v, f = spheres["cut"]
    m = float(np.sqrt(np.quantile(R.edge_lengths2(v, f), 0.6)))
    info = _check(v, f, max_edge=m)
    assert (np.bincount(info["marks_per_face"], minlength=4) > 0).all()
    _check(v.astype(np.float64) * 1.0000000123, f, max_edge=m)


def test_bad_faces_are_refused():
    from vtaco_amd import ops
    from vtaco_amd._lib import VtError
    v, f = R.fixture("tetrahedron")
    tv = _t(v)
    for row in ([0, 1, 4], [0, -1, 2], [0, 1, 1], [3, 1, 3]):
        bad = f.copy()
        bad[2] = row
        for scheme in R.SCHEMES:
            with pytest.raises(VtError, match="outside|repeated"):
                ops.mesh.subdivide(tv, _t(bad), scheme)
        with pytest.raises(VtError, match="outside|repeated"):
            ops.mesh.subdivide_count(tv, _t(bad))
    _check(v, f)                                                                   # and the next call is untouched by them
    for kw in (dict(scheme="sqrt3"), dict(scheme="loop", max_edge=1.0), dict(max_edge=0.0), dict(max_edge=1.0, face_mask=_t(np.ones(4, np.uint8))),
               dict(face_mask=_t(np.ones(3, np.uint8)))):
        with pytest.raises(VtError):
            ops.mesh.subdivide(tv, _t(f), **kw)
    with pytest.raises(VtError, match="int32"):
        ops.mesh.subdivide(tv, _t(f).long())


def test_mesh_clean(spheres):
    from vtaco_amd._lib import VtError
    from vtaco_amd.conv_onet.generation import Mesh, NormalMesh
    from vtaco_amd.utils import mesh_clean
    v, f = spheres["cut"]
    mesh = Mesh(_t(v), _t(f))
    v1, f1, i1 = R.subdivide(v, f)
    v2, f2, i2 = R.subdivide(v1, f1)
    got, rep = mesh.subdivide_report(iterations=2)
    assert _bits(got.vertices) == _bits(v2) and np.array_equal(got.faces.cpu().numpy(), f2)
    assert (rep.rounds, rep.n_vertices, rep.n_faces, rep.n_marked) == (2, [v1.shape[0], v2.shape[0]], [f1.shape[0], f2.shape[0]],
                                                                     [i1["n_marked"], i2["n_marked"]])
    assert np.array_equal(rep.face_parent.cpu().numpy(), i1["face_parent"][i2["face_parent"]])
    assert mesh.subdivide(0) is mesh
    lv, lf, _ = R.subdivide(v, f, "loop")
    loop = mesh_clean.subdivide_loop((mesh.vertices, mesh.faces))
    assert _bits(loop.vertices) == _bits(lv) and np.array_equal(loop.faces.cpu().numpy(), lf)
    # face_index: the selected faces in four, and in four again in the second round; their neighbours conform
    idx = [5, 6, 700]
    mask = np.zeros(f.shape[0], dtype=np.uint8)
    mask[idx] = 1
    a_v, a_f, a_i = R.subdivide(v, f, face_mask=mask)
    b_v, b_f, _ = R.subdivide(a_v, a_f, face_mask=mask[a_i["face_parent"]])
    got = mesh.subdivide(2, face_index=idx)
    assert _bits(got.vertices) == _bits(b_v) and np.array_equal(got.faces.cpu().numpy(), b_f)
    assert _bits(mesh.subdivide(1, face_index=_t(mask).bool()).vertices) == _bits(a_v)
    # subdivide_to_size
    edge = float(np.sqrt(R.edge_lengths2(v, f).max())) * 0.45
    want_v, want_f, rounds = R.subdivide_to_size(v, f, edge)
    got, rep = mesh.subdivide_report(max_edge=edge)
    assert rounds >= 2 and rep.rounds == rounds and _bits(got.vertices) == _bits(want_v) and np.array_equal(got.faces.cpu().numpy(), want_f)
    assert float(R.edge_lengths2(want_v, want_f).max()) <= edge * edge
    again = mesh.subdivide_to_size(edge)
    assert _bits(again.vertices) == _bits(want_v) and got.subdivide_to_size(edge) is got
    with pytest.raises(VtError, match=r"\d+ edges are still longer"):
        mesh.subdivide_to_size(edge, max_iter=1)
    # a NormalMesh comes back with geometric normals
    nm = mesh.with_vertex_normals().subdivide()
    assert isinstance(nm, NormalMesh) and nm.normals_source == "geometry" and nm.values is None and _bits(nm.vertices) == _bits(v1)
    assert tuple(nm.vertex_normals.shape) == (v1.shape[0], 3)


# ---- UpSampleLayer ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["tetra", "batch2", "ball", "strip"])
def test_upsample_layer_equals_the_reference(case):
    from vtaco_amd.encoder.manopth import UpSampleLayer
    g = np.load(GOLDEN)
    layer = UpSampleLayer()
    v, f = _t(g[case + "_verts"]), _t(g[case + "_faces"]).long()
    for _ in range(2):
        nv, nf = layer(v, f)
        assert nf.dtype == torch.int64 and nv.dtype == torch.float32
        assert _bits(nv) == _bits(g[case + "_new_verts"]) and np.array_equal(nf.cpu().numpy(), g[case + "_new_faces"])
    assert (layer.misses, layer.hits) == (1, 1)
    f[0, 0] = f[0, 0].roll(1)                                                       # an in-place write misses
    layer(v, f)
    assert layer.misses == 2


def test_upsample_layer_two_levels(spheres):
    from vtaco_amd.encoder.manopth import UpSampleLayer
    v, f = spheres["closed"]
    B, layer = 3, UpSampleLayer()
    rng = np.random.RandomState(2)
    vb = np.stack([v, v * 1.5, (v + rng.randn(*v.shape) * 0.01)]).astype(np.float32)
    tv, tf = _t(vb), _t(f).long().unsqueeze(0).expand(B, -1, -1)
    V, F = v.shape[0], f.shape[0]
    E = 3 * F // 2
    v1, f1 = layer(tv, tf)
    assert tuple(v1.shape) == (B, V + E, 3) and tuple(f1.shape) == (B, 4 * F, 3)
    v2, f2 = layer(v1, f1)
    assert tuple(v2.shape) == (B, V + E + (2 * E + 3 * F), 3) and tuple(f2.shape) == (B, 16 * F, 3)
    layer(tv, tf), layer(v1, f1)
    assert (layer.misses, layer.hits) == (2, 2)                                     # computed once per level for the whole batch
    for b in range(B):
        w1, g1, _ = R.subdivide(vb[b], f)
        w2, g2, _ = R.subdivide(w1, g1)
        assert _bits(v2[b]) == _bits(w2) and np.array_equal(f2[b].cpu().numpy(), g2)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_upsample_layer_backward(spheres, dtype):
    from vtaco_amd import ops
    from vtaco_amd.encoder.manopth import UpSampleLayer
    layer = UpSampleLayer()
    rng = np.random.RandomState(4)
    for name in ("fan300", "cut", "tetrahedron"):
        v, f = spheres[name] if name in spheres else R.fixture(name)
        _, _, info = R.subdivide(v, f)
        V, E = v.shape[0], info["n_marked"]
        g = (rng.randn(2, V + E, 3) * np.exp(rng.randn(2, V + E, 3) * 3)).astype(dtype)       # terms of very different sizes
        tv = _t(np.stack([v, v]).astype(dtype)).requires_grad_(True)
        out, _ = layer(tv, _t(f).long().unsqueeze(0).expand(2, -1, -1))
        grads = []
        for _ in range(2):
            tv.grad = None
            out.backward(_t(g), retain_graph=True)
            grads.append(tv.grad.clone())
        assert grads[0].dtype == tv.dtype and _bits(grads[0]) == _bits(grads[1])
        assert _bits(ops.mesh.subdivide_backward(_t(g), _t(info["edge_verts"]), V)) == _bits(grads[0])
        for b in range(2):
            want, mag, n = R.backward(info["edge_verts"], V, g[b].astype(np.float64))
            err = np.abs(grads[0][b].cpu().numpy().astype(np.float64) - want)
            # float64: one rounding per partial sum at the most; float32: the sum is exact and rounded once, 2^-24 of at most sum |terms|
            bound = n[:, None] * 2.0 ** -53 * mag if dtype == np.float64 else 2.0 ** -23 * mag
            print(f"RATIO subdivide_bwd {name} {np.dtype(dtype).name} item {b}: max err / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3g}")
            assert (err <= bound).all(), (name, float((err / np.maximum(bound, 1e-300)).max()))


def test_upsample_layer_gradcheck():
    from vtaco_amd.encoder.manopth import UpSampleLayer
    v, f = R.fixture("tetrahedron")
    layer = UpSampleLayer()
    tv = _t(np.stack([v, v * 2 + 0.25]).astype(np.float64)).requires_grad_(True)
    tf = _t(f).long().unsqueeze(0).expand(2, -1, -1)
    assert torch.autograd.gradcheck(lambda x: layer(x, tf)[0], (tv,))
    tf2 = torch.stack([_t(f).long(), _t(f[[1, 2, 3, 0]]).long()])                   # items with faces of their own
    assert torch.autograd.gradcheck(lambda x: layer(x, tf2)[0], (tv,))


def test_hand_upsample_changes_the_probe_count(monkeypatch):
    from vtaco_amd import eval as E
    hv, hf = S.icosahedron()
    hv = (hv * 0.2 + 0.5).astype(np.float32)                                        # a small "hand" inside the unit cube
    import mesh_topo_ref as T
    cv, cf = T.cube()
    thv, thf, tcv, tcf = _t(hv), _t(hf).long(), _t(cv), _t(cf)
    plain = E.penetration_depth(thv, tcv, tcf, 2.0)
    seen = []
    real = E._distance2
    monkeypatch.setattr(E, "_distance2", lambda distance, verts, faces, pts: (seen.append(pts.shape[0]), real(distance, verts, faces, pts))[1])
    assert E.penetration_depth(thv, tcv, tcf, 2.0, hand_upsample=0) == plain > 0 and E.penetration_depth(thv, tcv, tcf, 2.0, hand_upsample=0, hand_faces=thf) == plain
    w1, f1, _ = R.subdivide(hv, hf)
    w2, _, _ = R.subdivide(w1, f1)
    one = E.penetration_depth(thv, tcv, tcf, 2.0, hand_upsample=1, hand_faces=thf)
    two = E.penetration_depth(thv, tcv, tcf, 2.0, hand_upsample=2, hand_faces=thf)
    assert seen == [12, 12, 12 + 30, 42 + 120]
    monkeypatch.undo()
    assert one == E.penetration_depth(_t(w1), tcv, tcf, 2.0) and two == E.penetration_depth(_t(w2), tcv, tcf, 2.0)
    scenes = E.penetration_depth_scenes(torch.stack([thv, thv]), [(tcv, tcf), (tcv, tcf)], [2.0, 3.0], hand_upsample=1, hand_faces=thf)
    assert np.array_equal(scenes, E.penetration_depth_scenes(torch.stack([_t(w1), _t(w1)]), [(tcv, tcf), (tcv, tcf)], [2.0, 3.0])) and scenes[0] > 0
    with pytest.raises(ValueError):
        E.penetration_depth(thv, tcv, tcf, 2.0, hand_upsample=1)
    with pytest.raises(ValueError):
        E.penetration_depth(thv, tcv, tcf, 2.0, hand_upsample=3, hand_faces=thf)
