"""GPU: vt_closest_tree_build / vt_closest_tree_query through ``ops.metrics`` against tests/closest_point_tree_ref.py (the numpy restatement of
the walk) and against vt_closest_point_mesh, the brute-force kernel.

d2, face, closest and the two statistics (boxes tested, faces tested) are compared with the restatement for EQUAL BITS, no element left out;
d2, face and closest also with ``ops.metrics.closest_point_mesh`` on the same inputs: both kernels call one cp_face, and the walk skips a
cell only when its box cannot hold the answer.  tests/test_closest_point_tree_ref_cpu.py ties the restatement to by_regions on the same inputs."""
import ctypes

import numpy as np
import pytest
import torch

import closest_point_ref as R
import closest_point_tree_ref as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WALKS = {"seed+order": (True, True), "seed": (True, False), "order": (False, True), "plain": (False, False)}


def D(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _same_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape
    return np.array_equal(got.view(np.uint8), want.view(np.uint8))


def _host(out):
    return out.d2.cpu().numpy(), out.face.cpu().numpy(), None if out.closest is None else out.closest.cpu().numpy()


def _tree_run(verts, faces, pts, depth=None, strict=True):
    from vtaco_amd import ops
    ct = ops.metrics.closest_point_tree_build(D(verts), D(faces), depth)
    out, stats = ops.metrics.closest_point_tree_query(ct, D(pts), stats=True, strict=strict)
    return _host(out) + (stats.cpu().numpy(),), ct


def _brute_run(verts, faces, pts):
    from vtaco_amd import ops
    return _host(ops.metrics.closest_point_mesh(D(verts), D(faces), D(pts)))


def _check(verts, faces, pts, depth=None, walk="seed+order"):
    """The kernel against the restatement (statistics included) and against the brute-force kernel."""
    (d2, face, q, stats), ct = _tree_run(verts, faces, pts, depth)
    want = T.tree(verts, faces, pts, depth, *WALKS[walk])
    assert np.array_equal(face, want[1])
    assert _same_bits(d2, want[0]) and _same_bits(q, want[2])
    assert np.array_equal(stats, want[3]), (stats.sum(0), want[3].sum(0))
    b = _brute_run(verts, faces, pts)
    assert _same_bits(d2, b[0]) and _same_bits(face, b[1]) and _same_bits(q, b[2])
    return (d2, face, q, stats), ct


@pytest.mark.parametrize("depth", T.GRID_DEPTH)
@pytest.mark.parametrize("F", T.GRID_F + ("torus",))
def test_grid_of_sizes_equals_the_restatement_and_the_brute_force_kernel(F, depth):
    verts, faces = T.grid_mesh(F)
    for N in T.GRID_N:
        _check(verts, faces, T.grid_queries(F, N, verts, faces), depth)


def test_sparse_deep_tree():
    """65 faces at depth 7: a pyramid of 2 396 745 cells with at most 65 occupied leaves, long climbs between them."""
    verts, faces = T.grid_mesh(65)
    _, ct = _check(verts, faces, T.grid_queries(65, 65, verts, faces), 7)
    assert ct.tree.depth == 7 and ct.tree.counts[7] <= 65


def test_boxes_and_records_equal_the_restatement():
    from vtaco_amd import ops
    verts, faces = T.grid_mesh("torus")
    ct = ops.metrics.closest_point_tree_build(D(verts), D(faces))
    t = T.build(verts, faces)
    assert ct.status == 0 and ct.tree.depth == t.depth
    for l in range(t.depth + 1):
        assert _same_bits(ct.boxes(l).cpu().numpy(), t.boxes[l])
    rec = ct.records.cpu().numpy()
    v = verts.astype(np.float64)[faces[t.lists]]
    assert _same_bits(rec[:, 0:3], v[:, 0]) and _same_bits(rec[:, 3:6], v[:, 1] - v[:, 0]) and _same_bits(rec[:, 6:9], v[:, 2] - v[:, 0])
    assert (rec[:, 12] == 0).all() and (rec[:, 13] == 0).all()


@pytest.mark.parametrize("swap", [False, True])
def test_equal_minima_in_different_leaves_give_the_lowest_face(swap):
    verts, faces, pts, (i, j) = T.mirrored_pair(swap)
    (d2, face, _, _), ct = _check(verts, faces, pts)
    leaf_of = {}
    off, lists = ct.tree.list_offsets.cpu().numpy(), ct.tree.lists.cpu().numpy()
    for k in range(len(off) - 1):
        leaf_of.update({int(f): k for f in lists[off[k]:off[k + 1]]})
    assert leaf_of[i] != leaf_of[j] and leaf_of[3] == leaf_of[31]
    assert (face == i).all()                                               # face j is as near, bit for bit (the CPU test shows it)


def test_far_and_nan_queries():
    verts, faces = T.grid_mesh(65)
    for depth in (2, 7):
        (d2, _, q, _), _ = _check(verts, faces, T.far_queries(), depth)
        assert np.isfinite(d2).all() and np.isfinite(q).all() and d2[3] > 0.9e12
    pts = T.nan_queries(verts, faces)
    (d2, face, q, stats), ct = _check(verts, faces, pts)                   # ends, and equals the brute-force kernel's output
    bad = np.isnan(pts).any(axis=1)
    assert (face[bad] == -1).all() and np.isinf(d2[bad]).all() and np.isnan(q[bad]).all() and np.isfinite(d2[~bad]).all()
    assert (stats[bad, 0] == sum(ct.tree.counts)).all() and (stats[bad, 1] == len(faces)).all()


def test_one_leaf_holds_every_face():
    verts, faces = T.one_leaf()
    for depth in (1, 3):
        (_, _, _, stats), ct = _check(verts, faces, R.queries(65, 3, verts, faces), depth)
        assert ct.tree.counts[depth] == 1 and (stats[:, 1] == len(faces)).all()


@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("kind", ["repeated", "collinear"])
def test_degenerate_faces(kind, mixed):
    _check(*T.degenerate(kind, mixed))


def test_a_face_with_a_bad_index_is_skipped_and_reported():
    from vtaco_amd import ops
    from vtaco_amd._lib import VtError
    verts, faces = T.bad_index_mesh()
    pts = R.queries(65, 5)
    (d2, face, q, stats), ct = _tree_run(verts, faces, pts, strict=False)
    assert ct.status == 1
    want, brute = T.tree(verts, faces, pts), T.brute(verts, faces, pts)
    assert _same_bits(d2, want[0]) and np.array_equal(face, want[1]) and _same_bits(q, want[2]) and np.array_equal(stats, want[3])
    assert _same_bits(d2, brute[0]) and np.array_equal(face, brute[1]) and _same_bits(q, brute[2])      # the other faces are unaffected
    with pytest.raises(VtError, match="face index"):                       # reported as closest_point_mesh reports it
        ops.metrics.closest_point_tree_query(ct, D(pts))
    with pytest.raises(VtError, match="face index"):
        ops.metrics.closest_point_mesh(D(verts), D(faces), D(pts), method="tree")
    with pytest.raises(VtError, match="face index"):
        ops.metrics.closest_point_mesh(D(verts), D(faces), D(pts))
    alone = np.array([[0, 1, 2], [3, 4, 99]], dtype=np.int32)              # a leaf of one bad face: an empty box
    far = verts[:5].copy()
    far[3:] += 4.0
    (d2, face, _, _), ct = _tree_run(far, alone, pts, 1, strict=False)
    boxes = ct.boxes(1).cpu().numpy()
    assert ct.tree.counts[1] == 2 and sorted(np.isinf(boxes).all(axis=1)) == [False, True]
    assert (face == 0).all() and _same_bits(d2, R.by_regions(far, alone[:1], pts)[0])


def test_two_runs_and_every_walk_give_equal_bits(monkeypatch):
    from vtaco_amd import ops
    from vtaco_amd._lib import VtError
    monkeypatch.delenv("VTACO_CLOSEST_TREE_WALK", raising=False)
    verts, faces = T.grid_mesh("torus")
    pts = T.grid_queries("torus", 778, verts, faces)
    first, ct = _tree_run(verts, faces, pts)
    second, _ = _tree_run(verts, faces, pts)
    for a, b in zip(first, second):
        assert _same_bits(a, b)
    out = ops.metrics.closest_point_tree_query(ct, D(pts), want_point=False)
    assert out.closest is None and _same_bits(out.d2.cpu().numpy(), first[0]) and _same_bits(out.face.cpu().numpy(), first[1])
    i64 = ops.metrics.closest_point_tree_query(ops.metrics.closest_point_tree_build(D(verts), D(faces.astype(np.int64))), D(pts))
    assert _same_bits(i64.d2.cpu().numpy(), first[0]) and _same_bits(i64.closest.cpu().numpy(), first[2])
    t = T.build(verts, faces)
    for walk, (seed, order) in WALKS.items():                              # seed and order change what is skipped, never a result
        monkeypatch.setenv("VTACO_CLOSEST_TREE_WALK", walk)
        out, stats = ops.metrics.closest_point_tree_query(ct, D(pts), stats=True)
        got = _host(out)
        assert _same_bits(got[0], first[0]) and _same_bits(got[1], first[1]) and _same_bits(got[2], first[2])
        assert np.array_equal(stats.cpu().numpy(), T.query(t, verts, faces, pts, seed, order)[3])
        assert 0 < int(stats[:, 1].sum()) < len(pts) * len(faces)
    monkeypatch.setenv("VTACO_CLOSEST_TREE_WALK", "random")
    with pytest.raises(VtError, match="VTACO_CLOSEST_TREE_WALK"):
        ops.metrics.closest_point_tree_query(ct, D(pts))


def test_scenes_equal_their_single_calls():
    from vtaco_amd import ops
    cases = [T.grid_mesh(65), R.torus(24, 12, seed=2), T.grid_mesh(1000)]
    N = 130
    pts = np.stack([R.queries(N, 20 + b, *cases[b]) for b in range(3)])
    cts = [ops.metrics.closest_point_tree_build(D(v), D(f)) for v, f in cases]
    out, stats = ops.metrics.closest_point_tree_query_scenes(cts, D(pts), stats=True)
    assert tuple(out.d2.shape) == (3, N) and tuple(out.closest.shape) == (3, N, 3) and tuple(stats.shape) == (3, N, 2)
    batch = ops.metrics.closest_point_mesh_scenes([(D(v), D(f)) for v, f in cases], D(pts))
    for b in range(3):
        one, st = ops.metrics.closest_point_tree_query(cts[b], D(pts[b]), stats=True)
        for got, want, brute in zip(_host(ClosestRow(out, b)), _host(one), _host(ClosestRow(batch, b))):
            assert _same_bits(got, want) and _same_bits(got, brute)
        assert torch.equal(stats[b], st)
    plain = ops.metrics.closest_point_tree_query_scenes(cts, D(pts), want_point=False)
    assert plain.closest is None and torch.equal(plain.d2, out.d2)


class ClosestRow:
    """Scene b of a batched ClosestPoint."""

    def __init__(self, cp, b):
        self.d2, self.face, self.closest = cp.d2[b], cp.face[b], cp.closest[b]


def test_empty_queries_and_bad_arguments():
    from vtaco_amd import _lib, ops
    from vtaco_amd._lib import VtError
    lib = _lib.load()
    verts, faces = T.grid_mesh(9)
    v, f = D(verts), D(faces)
    ct = ops.metrics.closest_point_tree_build(v, f)
    out, stats = ops.metrics.closest_point_tree_query(ct, torch.zeros((0, 3), device=DEV), stats=True)
    assert tuple(out.d2.shape) == (0,) and tuple(out.face.shape) == (0,) and tuple(out.closest.shape) == (0, 3) and tuple(stats.shape) == (0, 2)
    empty = ops.metrics.closest_point_mesh(v, f, torch.zeros((0, 3), device=DEV), method="tree")
    assert tuple(empty.d2.shape) == (0,) and empty.d2.dtype == torch.float64 and empty.face.dtype == torch.int32
    none = ops.metrics.closest_point_tree_query_scenes([], torch.zeros((0, 4, 3), device=DEV))
    assert tuple(none.d2.shape) == (0, 4)
    for bad_v, bad_f in ((v, f[:0]), (v[:0], f)):                          # as the brute-force call: a mesh needs vertices and faces
        with pytest.raises(VtError):
            ops.metrics.closest_point_tree_build(bad_v, bad_f)
        with pytest.raises(VtError):
            ops.metrics.closest_point_mesh(bad_v, bad_f, torch.zeros((4, 3), device=DEV), method="tree")
    with pytest.raises(VtError, match="method"):
        ops.metrics.closest_point_mesh(v, f, torch.zeros((4, 3), device=DEV), method="kdtree")
    with pytest.raises(VtError):
        ops.metrics.closest_point_tree_build(v.cpu(), f.cpu())
    with pytest.raises(VtError):
        ops.metrics.closest_point_tree_build(v.double(), f)
    with pytest.raises(VtError):
        ops.metrics.closest_point_tree_query(ct, torch.zeros((4, 3), dtype=torch.float64, device=DEV))
    with pytest.raises(VtError):
        ops.metrics.closest_point_tree_query(ct.tree, torch.zeros((4, 3), device=DEV))
    with pytest.raises(VtError, match="2 trees|1 trees"):
        ops.metrics.closest_point_tree_query_scenes([ct], torch.zeros((2, 4, 3), device=DEV))
    with pytest.raises(VtError, match="not one of this mesh"):
        ops.metrics.closest_point_tree_build(v, f[:5], tree=ct.tree)
    # the C entry points: every refusal comes before any launch
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    pts = torch.zeros((4, 3), device=DEV)
    d2 = torch.full((4,), 7.0, dtype=torch.float64, device=DEV)
    face = torch.full((4,), 7, dtype=torch.int32, device=DEV)
    tr, state, F, L = ct.tree, ct.tree._state, len(faces), ct.tree.depth
    offsets = (ctypes.c_size_t * 3)()
    assert lib.vt_closest_tree_layout(F, L, state, offsets) == 0 and 256 <= offsets[0] < offsets[1] < offsets[2] <= ct.side.numel() * 8
    assert lib.vt_closest_tree_layout(0, L, state, offsets) == -1 and lib.vt_closest_tree_layout(F, 0, state, offsets) == -2
    assert lib.vt_closest_tree_layout(F, L, None, offsets) == -1

    def query(F=F, L=L, side_bytes=ct.side.numel() * 8, pts_p=P(pts)):
        return lib.vt_closest_tree_query(P(tr.buf), tr.buf.numel() * 8, P(ct.side), side_bytes, F, L, state, pts_p, 4, P(d2), P(face), None, None, None)
    assert query(F=0) == -1 and query(L=8) == -2 and query(side_bytes=64) == -3 and query(pts_p=None) == -1
    assert lib.vt_closest_tree_build(P(v), 0, P(f), F, L, state, P(tr.buf), tr.buf.numel() * 8, P(ct.side), ct.side.numel() * 8, None) == -1
    assert lib.vt_closest_tree_build(P(v), len(verts), P(f), F, L, state, P(tr.buf), 64, P(ct.side), ct.side.numel() * 8, None) == -3
    torch.cuda.synchronize()
    assert (d2 == 7.0).all() and (face == 7).all()                         # nothing was launched
    assert query() == 0
    torch.cuda.synchronize()
    assert _same_bits(d2.cpu().numpy(), R.by_regions(verts, faces, np.zeros((4, 3), dtype=np.float32))[0])


def test_a_tree_built_for_the_winding_number_is_reused():
    from vtaco_amd import ops
    verts, faces = T.grid_mesh("torus")
    pts = D(T.grid_queries("torus", 778, verts, faces))
    v, f = D(verts), D(faces)
    tree = ops.winding.build(v, f)
    shared = ops.metrics.closest_point_tree_build(v, f, tree=tree)
    fresh = ops.metrics.closest_point_tree_build(v, f)
    assert shared.tree is tree and torch.equal(shared.records, fresh.records)
    assert all(torch.equal(shared.boxes(l), fresh.boxes(l)) for l in range(tree.depth + 1))
    a, b = ops.metrics.closest_point_tree_query(shared, pts), ops.metrics.closest_point_tree_query(fresh, pts)
    for x, y in zip(_host(a), _host(b)):
        assert _same_bits(x, y)
    via = ops.metrics.closest_point_mesh(v, f, pts, method="tree")
    assert _same_bits(via.d2.cpu().numpy(), a.d2.cpu().numpy()) and torch.equal(via.face, a.face) and torch.equal(via.closest, a.closest)
    assert torch.equal(ops.winding.query(tree, pts), ops.winding.fast(v, f, pts))                 # the tree is left as it was


def test_eval_callers_with_the_tree_equal_brute_force():
    from vtaco_amd import eval as E
    tv, tf = R.torus(24, 12, seed=4)
    v, f = D(tv), D(tf)
    rng = np.random.RandomState(3)
    pts = D((rng.rand(778, 3).astype(np.float32) - np.float32(0.5)))
    for winding in ("exact", "fast"):
        brute = E.signed_distance(pts, v, f, winding=winding)
        tree = E.signed_distance(pts, v, f, winding=winding, distance="tree")
        assert brute.dtype == torch.float64 and torch.equal(brute, tree) and bool((brute < 0).any()) and bool((brute > 0).any())
        assert E.penetration_depth(pts, v, f, 2.0, winding=winding) == E.penetration_depth(pts, v, f, 2.0, winding=winding, distance="tree") > 0
    cv, cf = D(R.CUBE_V), D(R.CUBE_F)
    hands = torch.stack([pts[:300], pts[300:600]])
    for winding in ("exact", "fast"):
        brute = E.penetration_depth_scenes(hands, [(v, f), (cv, cf)], [2.0, 3.0], winding=winding)
        assert (brute > 0).all()
        assert np.array_equal(brute, E.penetration_depth_scenes(hands, [(v, f), (cv, cf)], [2.0, 3.0], winding=winding, distance="tree"))
    with pytest.raises(ValueError, match="distance"):
        E.signed_distance(pts, v, f, distance="kdtree")
    with pytest.raises(ValueError, match="distance"):
        E.penetration_depth_scenes(hands, [(v, f), (cv, cf)], [2.0, 3.0], distance="kdtree")
    moved = D(tv + np.array([0.01, -0.02, 0.005], dtype=np.float32))
    for fn, kw in ((E.mesh_distances, {}), (E.mesh_distances_aligned, {"max_iterations": 5})):
        res = []
        for distance in ("brute", "tree"):
            gen = torch.Generator(device=DEV).manual_seed(1)
            res.append(fn((moved, f), (v, f), 2000, gen, distance=distance, **kw))
        assert sorted(res[0]) == sorted(res[1])
        for key in res[0]:
            assert np.array_equal(res[0][key], res[1][key]), key
        assert res[0]["accuracy"] > 0


def test_signed_distance_field_of_the_torus():
    from vtaco_amd import eval as E
    from vtaco_amd.conv_onet.generation import Mesh
    from vtaco_amd.utils import voxels
    tv, tf = T.grid_mesh("torus")
    v, f = D(tv), D(tf)
    res = 16
    sdf = voxels.signed_distance_field((v, f), res, loc=(0.0, 0.0, 0.0), scale=1.0)
    assert sdf.dtype == torch.float64 and tuple(sdf.shape) == (res, res, res) and sdf.is_cuda
    centres = voxels._centres(res, (0.0, 0.0, 0.0), 1.0, v.device).reshape(-1, 3)
    for winding, distance in (("fast", "tree"), ("fast", "brute"), ("exact", "brute")):
        want = E.signed_distance(centres, v, f, winding=winding, distance=distance).reshape(res, res, res)
        assert torch.equal(voxels.signed_distance_field((v, f), res, (0.0, 0.0, 0.0), 1.0, winding=winding, distance=distance), want)
        if winding == "fast":
            assert torch.equal(sdf, want)
    inside = voxels.voxelize_interior((v, f), res, rule="fast_winding")
    assert torch.equal(sdf < 0, inside) and 0 < int(inside.sum()) < res ** 3
    # from_mesh's conventions: by default the grid is centred on the bounds and the mesh fills [-0.45, 0.45]^3 of it
    auto = Mesh(v, f).signed_distance_field(res)
    lo, hi = tv.astype(np.float64).min(0), tv.astype(np.float64).max(0)
    assert torch.equal(auto, voxels.signed_distance_field((tv, tf), res, loc=(lo + hi) / 2, scale=(hi - lo).max() / 0.9))
    assert float(auto.max()) < 0.75 * (hi - lo).max() and float(auto.min()) < 0
    with pytest.raises(ValueError):
        voxels.signed_distance_field((v, f[:0]), res)


def test_vtaco_closest_point_knob_reaches_eval_step(tmp_path, monkeypatch):
    """VTACO_CLOSEST_POINT unset / 'brute': the hand metrics as before; 'tree': the same penetration depth from the walk, on trees that are
    built once per mesh object; anything else is refused."""
    from test_hand_metrics_gpu import _trainer_and_batch
    from vtaco_amd import ops
    from vtaco_amd._lib import VtError
    from vtaco_amd.common import hand_in_object_frame
    model, trainer, batch = _trainer_and_batch(tmp_path)
    names = list(batch["points.name"])
    mano_gt = batch["points.mano"].float()
    model.eval()
    with torch.no_grad():
        mano_verts = model.encode_hand_inputs(batch["inputs"].to(DEV))["mano_verts"].cpu().numpy()
    hand = hand_in_object_frame(mano_verts, mano_gt.numpy()[:, :3], batch["points.wrist"].numpy(), batch["inputs.pc_ply"].numpy())
    vf = {}
    for b in range(2):                                                      # a cube round the centre of each hand: part of it is inside
        centre, extent = hand[b].mean(0), float(np.ptp(hand[b], axis=0).max())
        vf[names[b]] = {"v": (R.CUBE_V.astype(np.float64) * extent + centre).astype(np.float32), "f": R.CUBE_F}
    calls = {"build": 0, "query": 0}
    build, query = ops.metrics.closest_point_tree_build, ops.metrics.closest_point_tree_query_scenes

    def counted_build(*a, **kw):
        calls["build"] += 1
        return build(*a, **kw)

    def counted_query(*a, **kw):
        calls["query"] += 1
        return query(*a, **kw)
    monkeypatch.setattr(ops.metrics, "closest_point_tree_build", counted_build)
    monkeypatch.setattr(ops.metrics, "closest_point_tree_query_scenes", counted_query)
    monkeypatch.delenv("VTACO_CLOSEST_POINT", raising=False)
    monkeypatch.delenv("VTACO_WINDING", raising=False)
    plain = trainer.eval_step(batch, vf, hand_metrics=True)
    monkeypatch.setenv("VTACO_CLOSEST_POINT", "brute")
    assert trainer.eval_step(batch, vf, hand_metrics=True) == plain and calls == {"build": 0, "query": 0}
    assert plain["penetration_depth"] > 0
    monkeypatch.setenv("VTACO_CLOSEST_POINT", "tree")
    assert trainer.eval_step(batch, vf, hand_metrics=True) == plain and calls == {"build": 2, "query": 1}
    assert trainer.eval_step(batch, vf, hand_metrics=True) == plain and calls == {"build": 2, "query": 2}      # the trees are cached
    monkeypatch.setenv("VTACO_WINDING", "fast")
    fast = trainer.eval_step(batch, vf, hand_metrics=True)
    monkeypatch.setenv("VTACO_CLOSEST_POINT", "brute")
    assert trainer.eval_step(batch, vf, hand_metrics=True) == fast and calls == {"build": 2, "query": 3}
    monkeypatch.setenv("VTACO_CLOSEST_POINT", "rtree")
    with pytest.raises(VtError, match="VTACO_CLOSEST_POINT"):
        trainer.eval_step(batch, vf, hand_metrics=True)
