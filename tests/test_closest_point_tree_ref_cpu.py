"""CPU: the walk of csrc/closest_point_tree.hip, restated in numpy by tests/closest_point_tree_ref.py, loses nothing.

On every mesh and query set the GPU test names, the restatement -- boxes, the slack delta, the seed and the child order as the kernel has
them -- returns closest_point_ref.by_regions' d2, face and closest, EQUAL BITS, no element left out: a cell the walk skips never held the
answer, and the explicit tie rule gives the lowest face whatever order the leaves are met in.  The boxes are checked for what the bound
relies on: every face inside its leaf's box, every child box inside its parent's."""
import os

import numpy as np
import pytest

import closest_point_ref as R
import closest_point_tree_ref as T

WALKS = [(True, True), (True, False), (False, True), (False, False)]          # (seed, order): the kernel's default first


def _same_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape
    return np.array_equal(got.view(np.uint8), want.view(np.uint8))


def _check(verts, faces, pts, depth=None, walks=WALKS, want=None):
    want = R.by_regions(verts, faces, pts) if want is None else want
    t = T.build(verts, faces, depth)
    out = None
    for seed, order in walks:
        d2, face, q, stats = T.query(t, verts, faces, pts, seed, order)
        assert np.array_equal(face, want[1]), (seed, order)
        assert _same_bits(d2, want[0]) and _same_bits(q, want[2]), (seed, order)
        assert (stats[:, 0] >= 1).all() and (stats[:, 1] <= (2 if seed else 1) * len(faces)).all()
        out = out or (t, stats)
    return out


@pytest.mark.parametrize("depth", T.GRID_DEPTH)
@pytest.mark.parametrize("F", T.GRID_F + ("torus",))
def test_grid_equals_by_regions(F, depth):
    verts, faces = T.grid_mesh(F)
    for N in T.GRID_N:
        _check(verts, faces, T.grid_queries(F, N, verts, faces), depth, walks=WALKS if N == 65 else WALKS[:1])


def test_sparse_deep_tree():
    """65 faces at depth 7: a pyramid of 2 396 745 cells with 65 occupied leaves, long climbs between them."""
    verts, faces = T.grid_mesh(65)
    t, _ = _check(verts, faces, T.grid_queries(65, 65, verts, faces), 7)
    assert t.depth == 7 and len(t.boxes[7]) <= 65


@pytest.mark.parametrize("swap", [False, True])
def test_equal_minima_in_different_leaves_give_the_lowest_face(swap):
    verts, faces, pts, (i, j) = T.mirrored_pair(swap)
    t = T.build(verts, faces)
    assert t.codes[i] != t.codes[j] and t.codes[3] == t.codes[31]                  # the mirrored faces in two leaves, the repeated one in one
    D, _ = T.pairs(verts, faces, pts, t.valid)
    assert _same_bits(D[:, i], D[:, j]) and (D[:, i] == D.min(axis=1)).all()        # the tie is real and it is the minimum
    for seed, order in WALKS:
        assert (T.query(t, verts, faces, pts, seed, order)[1] == i).all()
    _check(verts, faces, pts)
    on_repeated = verts[faces[3]].astype(np.float64).mean(axis=0, keepdims=True).astype(np.float32)
    assert T.tree(verts, faces, on_repeated)[1][0] == R.by_regions(verts, faces, on_repeated)[1][0] <= 3


def test_far_and_nan_queries():
    verts, faces = T.grid_mesh(65)
    for depth in (2, 7):
        t, stats = _check(verts, faces, T.far_queries(), depth)
        assert np.isfinite(T.slack(t, T.far_queries().astype(np.float64))).all()
    pts = T.nan_queries(verts, faces)
    t, stats = _check(verts, faces, pts)
    bad = np.isnan(pts).any(axis=1)
    cells = sum(len(b) for b in t.boxes)
    assert (stats[bad, 0] == cells).all() and (stats[bad, 1] == len(faces)).all()   # nothing is skipped, and the walk ends


def test_one_leaf_holds_every_face():
    verts, faces = T.one_leaf()
    for depth in (1, 3):
        t, stats = _check(verts, faces, R.queries(65, 3, verts, faces), depth)
        assert len(t.boxes[depth]) == 1 and (stats[:, 1] == len(faces)).all()


@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("kind", ["repeated", "collinear"])
def test_degenerate_faces(kind, mixed):
    _check(*T.degenerate(kind, mixed))


def test_a_face_with_a_bad_index_is_in_no_box():
    verts, faces = T.bad_index_mesh()
    pts = R.queries(65, 5)
    t, _ = _check(verts, faces, pts, want=T.brute(verts, faces, pts))
    assert (~t.valid).sum() == 2
    alone = np.array([[0, 1, 2], [3, 4, 99]], dtype=np.int32)                       # a leaf of one bad face: an empty box
    far = verts[:5].copy()
    far[3:] += 4.0                                                                   # (binned by its clamped indices: a leaf of its own)
    t = T.build(far, alone, 1)
    empty = [b for b in t.boxes[1] if np.isinf(b).any()]
    assert len(empty) == 1 and (empty[0][:3] == np.inf).all() and (empty[0][3:] == -np.inf).all()
    d2, face, _, _ = T.query(t, far, alone, pts)
    assert (face == 0).all() and _same_bits(d2, R.by_regions(far, alone[:1], pts)[0])


@pytest.mark.parametrize("case", ["torus", "soup", "deep", "bad"])
def test_boxes_hold_their_faces_and_children(case):
    verts, faces = {"torus": T.grid_mesh("torus"), "soup": T.grid_mesh(1000), "deep": T.grid_mesh(65), "bad": T.bad_index_mesh()}[case]
    t = T.build(verts, faces, 7 if case == "deep" else None)
    L = t.depth
    v = verts.astype(np.float64)
    for f in np.nonzero(t.valid)[0]:
        box = t.boxes[L][t.pyramid[L][t.codes[f]]]
        assert (v[faces[f]] >= box[:3]).all() and (v[faces[f]] <= box[3:]).all()
    for l in range(L):
        cells = np.nonzero(t.pyramid[l + 1] >= 0)[0]
        child, parent = t.boxes[l + 1][t.pyramid[l + 1][cells]], t.boxes[l][t.pyramid[l][cells >> 3]]
        assert (child[:, :3] >= parent[:, :3]).all() and (child[:, 3:] <= parent[:, 3:]).all()
    assert _same_bits(t.boxes[0][0], np.concatenate([v[faces[t.valid]].reshape(-1, 3).min(0), v[faces[t.valid]].reshape(-1, 3).max(0)]))


def test_the_walk_prunes_on_the_torus():
    """Fewer faces tested than N F, and the recorded shares (profiles/closest_point_tree_f64_ratios.txt) are this restatement's."""
    verts, faces = T.grid_mesh("torus")
    pts = T.grid_queries("torus", 778, verts, faces)
    t = T.build(verts, faces)
    pairs = len(pts) * len(faces)
    shares = {}
    for seed, order in WALKS:
        stats = T.query(t, verts, faces, pts, seed, order)[3]
        assert 0 < stats[:, 1].sum() < pairs
        shares[(seed, order)] = (int(stats[:, 0].sum()), int(stats[:, 1].sum()))
    path = os.path.join(os.path.dirname(__file__), "..", "profiles", "closest_point_tree_f64_ratios.txt")
    recorded = {}
    for line in open(path):
        w = line.split()
        if len(w) >= 5 and w[0] == "torus(24,12)":
            recorded[w[1]] = (int(w[2]), int(w[3]))
    names = {(True, True): "seed+order", (True, False): "seed", (False, True): "order", (False, False): "plain"}
    assert recorded == {names[k]: v for k, v in shares.items()}
