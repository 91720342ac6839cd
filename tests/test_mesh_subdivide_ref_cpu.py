"""CPU: the definition of mesh subdivision (tests/mesh_subdivide_ref.py) against the real reference's UpSampleLayer (tests/golden/
g31_subdivide.npz, made by tests/golden/make_subdivide_goldens.py), the invariants a subdivision has to keep, and the plumbing around
csrc/mesh_subdivide.hip that needs no GPU: the ABI names, the ops namespace, Generator3D's pinned constructor and the config keys."""
import inspect
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mesh_subdivide_ref as R  # noqa: E402
import mesh_topo_ref as T  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g31_subdivide.npz")
NAMES = sorted(R.FIXTURES)
# Generator3D.__init__ as the parent commit has it
PARENT_PARAMETERS = ["self", "model", "points_batch_size", "threshold", "refinement_step", "device", "resolution0", "upsampling_steps", "with_normals",
                     "padding", "sample", "input_type", "vol_info", "vol_bound", "simplify_nfaces", "alpha", "with_img", "encode_t2d",
                     "decode_precision", "depth_origin", "reference_returns", "extraction", "components", "min_component_faces", "smooth",
                     "smooth_iterations", "refine_sampler", "fill_holes", "fill_holes_max_edges"]


def _normals(v, f):
    x = np.asarray(v, dtype=np.float64)
    return np.cross(x[f[:, 1]] - x[f[:, 0]], x[f[:, 2]] - x[f[:, 0]])


def _keeps_orientation(v, f, ov, of, parent):
    """Every child of a face with area points the way its parent does."""
    n0, n1 = _normals(v, f)[parent], _normals(ov, of)
    dots = (n0 * n1).sum(1)
    live = (n0 * n0).sum(1) > 0
    return bool((dots[live] > 0).all())


def _modes(name, v, f):
    """The marking rules tried on a fixture: every edge, an edge length about the median, one face, all faces but one."""
    out = [dict()]
    if f.shape[0]:
        out.append(dict(max_edge=float(np.sqrt(np.median(R.edge_lengths2(v, f))))))
        one = np.zeros(f.shape[0], dtype=np.uint8)
        one[f.shape[0] // 2] = 1
        out += [dict(face_mask=one), dict(face_mask=1 - one)]
    return out


@pytest.mark.parametrize("case", ["tetra", "batch2", "ball", "strip"])
def test_definition_equals_the_reference_layer(case):
    g = np.load(GOLDEN)
    for b in range(g[case + "_verts"].shape[0]):
        v, f = g[case + "_verts"][b], g[case + "_faces"][b]
        ov, of, info = R.subdivide(v, f)
        assert ov.dtype == np.float32 and ov.tobytes() == g[case + "_new_verts"][b].tobytes()
        assert np.array_equal(of, g[case + "_new_faces"][b]) and np.array_equal(info["edge_verts"], g[case + "_pairs"][b])
        assert np.array_equal(info["face_parent"], np.repeat(np.arange(f.shape[0]), 4))
    if case == "tetra":
        assert info["edge_verts"].tolist() == [[0, 1], [1, 2], [0, 2], [2, 3], [0, 3], [1, 3]]
        assert of[:4].tolist() == [[4, 5, 6], [0, 4, 6], [1, 5, 4], [2, 6, 5]]


@pytest.mark.parametrize("name", NAMES)
def test_orientation_area_and_counts(name):
    v, f = R.fixture(name)
    for kw in _modes(name, v, f):
        ov, of, info = R.subdivide(v, f, "midpoint", **kw)
        F, E = f.shape[0], info["n_marked"]
        assert ov.shape[0] == v.shape[0] + E and of.shape[0] == F + int(info["marks_per_face"].sum()) == info["face_parent"].shape[0]
        assert ov[:v.shape[0]].tobytes() == v.tobytes()
        assert _keeps_orientation(v, f, ov, of, info["face_parent"]), kw
        if name in R.INTEGER_GRIDS:
            assert R.total_area(ov, of) == R.total_area(v, f), kw            # halves of small integers: every term is exact
        if not kw:
            assert of.shape[0] == 4 * F and E == np.unique(np.sort(f[:, [0, 1, 1, 2, 2, 0]].reshape(-1, 2), 1), axis=0).shape[0]
        if name in R.CLOSED:
            t0, t1 = T.topo(v, f), T.topo(ov, of)
            assert t1["euler"].tolist() == t0["euler"].tolist() and t1["watertight"].all() and t1["oriented"].all(), kw
            if not kw:
                assert int(t1["n_edges"].sum()) == 2 * int(t0["n_edges"].sum()) + 3 * F and int(t1["n_faces"].sum()) == 4 * F
    if f.shape[0]:
        lv, lf, linfo = R.subdivide(v, f, "loop")
        assert np.array_equal(lf, R.subdivide(v, f)[1]) and lv.dtype == v.dtype and lv.shape == (v.shape[0] + linfo["n_marked"], 3)
        if name in R.INTEGER_GRIDS or name in R.CLOSED:                             # (Loop may fold a face of a wild mesh over)
            assert _keeps_orientation(v, f, lv, lf, linfo["face_parent"])


def test_all_four_face_cases_occur_and_conform():
    v, f = R.fixture("stretched_torus")
    ov, of, info = R.subdivide(v, f, max_edge=R.FOUR_CASES_MAX_EDGE)
    assert np.bincount(info["marks_per_face"], minlength=4).tolist() == [64, 64, 96, 32]
    assert _keeps_orientation(v, f, ov, of, info["face_parent"])
    t = T.topo(ov, of)
    assert t["watertight"].all() and t["oriented"].all() and t["euler"].tolist() == [0]


@pytest.mark.parametrize("name,max_edge", [("torus", 0.2), ("voxel_ball", 0.4), ("tetrahedron", 0.3), ("grid9", 0.6), ("strip10", 0.45)])
def test_subdivide_to_size(name, max_edge):
    v, f = R.fixture(name)
    ov, of, rounds = R.subdivide_to_size(v, f, max_edge)
    assert rounds >= 1 and float(R.edge_lengths2(ov, of).max()) <= max_edge * max_edge
    t = T.topo(ov, of)
    assert int(t["n_nonmanifold"].sum()) == 0 and int(t["n_misoriented"].sum()) == 0
    if name in R.CLOSED:
        assert t["watertight"].all() and t["euler"].tolist() == T.topo(v, f)["euler"].tolist()      # every edge has exactly two faces
    if name == "grid9":
        # an open mesh: a T-junction would be a boundary edge inside the square; every boundary edge lies on its outline instead
        tab = R.edge_table(of, ov.shape[0])
        on = lambda p: (p[:, 0] == 0) | (p[:, 0] == 8) | (p[:, 1] == 0) | (p[:, 1] == 8)
        b = tab["fwd"] + tab["bwd"] == 1
        mid = (ov[tab["lo"][b]].astype(np.float64) + ov[tab["hi"][b]]) * 0.5
        assert b.sum() > 0 and on(ov[tab["lo"][b]]).all() and on(ov[tab["hi"][b]]).all() and on(mid).all()
        assert R.total_area(ov, of) == 64.0
    with pytest.raises(RuntimeError, match="edges are still longer"):
        R.subdivide_to_size(v, f, max_edge / 64, max_iter=1)


def test_loop_fixed_points_on_the_regular_grid():
    v, f = R.fixture("regular7")
    for x in (v, v.astype(np.float64)):
        ov, of, info = R.subdivide(x, f, "loop")
        assert info["n_irregular"] == 0 and (ov[:, 2] == 2).all()                  # the grid stays in its plane exactly
        interior = np.array([a * 7 + b for a in range(1, 6) for b in range(1, 6)])
        assert ov[interior].tobytes() == x[interior].tobytes()                      # valence 6, symmetric neighbours: a fixed point
        corner = ov[0]
        assert corner.tolist() == [0.125, 0.125, 2.0]                               # 0.75 (0,0) + 0.125 ((1,0) + (0,1))


def test_loop_irregular_edges_keep_their_ends():
    v, f = R.fixture("odd")
    ov, of, info = R.subdivide(v, f, "loop")
    tab = R.edge_table(f, v.shape[0])
    bad = (tab["fwd"] > 1) | (tab["bwd"] > 1)
    assert info["n_irregular"] == int(bad.sum()) == 6
    ends = np.unique(np.concatenate([tab["lo"][bad], tab["hi"][bad]]))
    assert ov[ends].tobytes() == v[ends].tobytes() and ov[0].tobytes() == v[0].tobytes()      # and the unreferenced vertex


def test_bad_faces_are_refused():
    v, _ = R.fixture("tetrahedron")
    for f in ([[0, 1, 4]], [[0, 1, -1]], [[0, 1, 1]], [[2, 1, 2]]):
        with pytest.raises(ValueError):
            R.subdivide(v, np.array(f, dtype=np.int32))


def test_backward_is_the_transpose():
    v, f = R.fixture("voxel_ball")
    ov, of, info = R.subdivide(v.astype(np.float64), f)
    g = np.random.RandomState(3).randn(*ov.shape)
    gv, mag, n = R.backward(info["edge_verts"], v.shape[0], g)
    dense = np.zeros((ov.shape[0], v.shape[0]))
    dense[np.arange(v.shape[0]), np.arange(v.shape[0])] = 1.0
    for e, (a, b) in enumerate(info["edge_verts"].tolist()):
        dense[v.shape[0] + e, [a, b]] = 0.5
    assert np.abs(gv - dense.T @ g).max() <= 2.0 ** -50 * mag.max() and (n >= 4).all()


def test_abi_names_are_bound_and_ops_gained_no_name():
    from vtaco_amd import _lib, ops
    names = {"vt_mesh_subdivide_workspace_bytes", "vt_mesh_subdivide_count", "vt_mesh_subdivide_emit", "vt_mesh_subdivide_midpoints",
             "vt_mesh_subdivide_bwd_workspace_bytes", "vt_mesh_subdivide_bwd"}
    assert names <= set(_lib.SIGNATURES)
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vtaco_hip.h")).read()
    assert all(n + "(" in text for n in names)
    for n in ("subdivide", "subdivide_backward", "subdivide_midpoints", "subdivide_count", "SubdivideInfo"):
        assert hasattr(ops.mesh, n) and not hasattr(ops, n)
    assert ops.mesh.SubdivideInfo._fields == ("edge_verts", "face_parent", "n_marked", "n_irregular")


def test_generator_constructor_is_the_parents_and_the_config_reaches_configure_subdivide(monkeypatch):
    from vtaco_amd._lib import VtError
    from vtaco_amd.conv_onet import config
    from vtaco_amd.conv_onet.generation import Generator3D, Mesh
    assert list(inspect.signature(Generator3D.__init__).parameters) == PARENT_PARAMETERS
    assert (Generator3D.subdivide, Generator3D.subdivide_iterations, Generator3D.subdivide_max_edge) == (None, 1, None)
    for m in ("subdivide", "subdivide_loop", "subdivide_to_size", "subdivide_report"):
        assert callable(getattr(Mesh, m))
    seen = {}

    class Stub:
        def __init__(self, model, **kw):
            seen["kw"] = kw

        def configure_subdivide(self, scheme=None, iterations=1, max_edge=None):
            seen["subdivide"] = (scheme, iterations, max_edge)
            return self

    monkeypatch.setattr(config, "Generator3D", Stub)
    cfg = {"generation": {"resolution_0": 16, "upsampling_steps": 1, "subdivide": "loop", "subdivide_iterations": 2},
           "test": {"threshold": 0.5}, "data": {"input_type": "pointcloud", "padding": 0.1}, "model": {}}
    assert isinstance(config.get_generator(None, cfg, None), Stub) and seen["subdivide"] == ("loop", 2, None)
    cfg["generation"] = {"resolution_0": 16, "upsampling_steps": 1, "subdivide": "midpoint", "subdivide_max_edge": 0.05}
    config.get_generator(None, cfg, None)
    assert seen["subdivide"] == ("midpoint", 1, 0.05)
    cfg["generation"] = {"resolution_0": 16, "upsampling_steps": 1}
    config.get_generator(None, cfg, None)
    assert seen["subdivide"] == (None, 1, None) and "subdivide" not in seen["kw"]
    # the checks of the method itself need no device
    g = Generator3D.__new__(Generator3D)
    assert g.configure_subdivide("midpoint", 2) is g and (g.subdivide, g.subdivide_iterations, g.subdivide_max_edge) == ("midpoint", 2, None)
    assert g.configure_subdivide().subdivide is None
    for bad in (dict(scheme="sqrt3"), dict(scheme="midpoint", iterations=-1), dict(scheme="loop", max_edge=0.1), dict(scheme="midpoint", max_edge=0.0)):
        with pytest.raises(VtError):
            g.configure_subdivide(**bad)
    g.configure_subdivide("loop")
    with pytest.raises(VtError, match="sharded"):
        g.refinement_step, g.with_normals, g.simplify_nfaces, g.fill_holes, g.smooth = 0, False, None, None, None
        g.generate_obj_mesh_sharded({})
