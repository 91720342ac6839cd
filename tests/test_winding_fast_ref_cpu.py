"""CPU: the numpy restatement of the fast winding number (tests/winding_fast_ref.py, what csrc/winding_fast.hip follows operation by
operation) against the independent truth, the exact float64 sum of tests/voxelize_ref.py::winding_number.  The restatement is never
its own judge: tree invariants are recomputed from the faces, errors are taken against the exact sum."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mesh_topo_ref as T  # noqa: E402
import voxelize_ref as VR  # noqa: E402
import winding_fast_ref as W  # noqa: E402

U = 2.0 ** -53


def named_torus():
    v, f = VR.torus(64, 32, 0.30, 0.12)
    pts = ((np.random.RandomState(0).rand(400, 3) - 0.5) * (1, 1, 0.4)).astype(np.float32)
    return v.astype(np.float32), f.astype(np.int32), pts


def soup(n, seed):
    rs = np.random.RandomState(seed)
    base = rs.rand(n, 1, 3) - 0.5
    v = (base + 0.08 * (rs.rand(n, 3, 3) - 0.5)).reshape(-1, 3).astype(np.float32)
    return v, np.arange(3 * n, dtype=np.int32).reshape(n, 3)


def meshes():
    bv, bf = VR.box()
    tv, tf = VR.torus(16, 8)
    return {"cube": (bv.astype(np.float32), bf.astype(np.int32), True), "torus": (tv.astype(np.float32), tf.astype(np.int32), True),
            "soup": soup(150, 3) + (False,)}


def direct_record(tri, idx, p):
    """(N0, M1, M2) of the faces idx about p, straight from the definitions (vectorised, another order than the restatement's)."""
    t = tri[idx]
    nv, area, cen = W.face_terms(t)
    n0 = nv.sum(0)
    m1 = np.einsum("tj,ti->ji", cen - p, nv)
    mids = np.stack([0.5 * (t[:, 0] + t[:, 1]), 0.5 * (t[:, 1] + t[:, 2]), 0.5 * (t[:, 2] + t[:, 0])], 1) - p
    c = np.einsum("tmj,tmk->tjk", mids, mids) / 3.0
    m2 = np.einsum("tjk,ti->jki", c, nv)
    return n0, m1, np.stack([m2[j, k] for j, k in W.PAIRS])


@pytest.mark.parametrize("depth", [1, 2, 3, 4])
@pytest.mark.parametrize("name", ["cube", "torus", "soup"])
def test_tree_invariants(name, depth):
    v, f, closed = meshes()[name]
    t = W.build(v, f, depth)
    F, L = len(f), depth
    assert np.array_equal(np.sort(t.lists), np.arange(F))                       # every face in exactly one list
    assert t.list_offsets[0] == 0 and t.list_offsets[-1] == F and np.all(np.diff(t.list_offsets) > 0)
    leaf_of_face = np.empty(F, dtype=np.int64)
    for k in range(len(t.list_offsets) - 1):
        lst = t.lists[t.list_offsets[k]:t.list_offsets[k + 1]]
        assert np.all(np.diff(lst) > 0)                                          # ascending
        leaf_of_face[lst] = k
    assert np.array_equal(t.pyramid[L][t.codes], leaf_of_face)                  # the list is the centroid's leaf
    scale = np.abs(t.records[L][:, 4:7]).sum() + 1e-300
    for l in range(L + 1):
        assert len(t.records[l]) == int((t.pyramid[l] >= 0).sum())
        assert t.records[l][:, 35].sum() == F                                    # counts sum to F
        assert np.abs(t.records[l][:, 4:7].sum(0) - t.records[0][0, 4:7]).max() <= 64 * F * U * scale
    if closed:
        assert np.abs(t.records[0][0, 4:7]).max() <= 64 * F * U * scale
    size = np.abs(t.tri).max()
    for l in range(L + 1):
        cells = t.codes >> (3 * (L - l))
        for m in np.unique(cells):
            idx = np.nonzero(cells == m)[0]
            rec = t.records[l][t.pyramid[l][m]]
            reach = np.sqrt(((t.tri[idx] - rec[0:3]) ** 2).sum(-1)).max()
            assert reach <= rec[3] * (1 + 1e-12) + 1e-300, (l, m)               # every vertex within r of p
            n0, m1, m2 = direct_record(t.tri, idx, rec[0:3])
            area = W.face_terms(t.tri[idx])[1].sum()
            tol = 256 * len(idx) * U * max(area, 1e-300)                         # terms are at most area x size^k
            assert np.abs(rec[4:7] - n0).max() <= tol
            assert np.abs(rec[7:16].reshape(3, 3) - m1).max() <= tol * size * (L + 1)
            assert np.abs(rec[16:34].reshape(6, 3) - m2).max() <= tol * size * size * (L + 1)
            assert abs(rec[34] - area) <= tol


def test_convergence_order_of_one_cell():
    """The expansion's error against the exact sum over the cell's own faces at 4r, 8r and 16r: orders 0, 1, 2 fall by at least 4x, 8x
    and 16x per doubling (the first neglected terms fall 8x, 16x and 32x)."""
    v, f, _ = named_torus()
    t = W.build(v, f, 3)
    k = int(np.argmax(t.records[3][:, 35]))
    rec = t.records[3][k]
    faces = f[t.lists[t.list_offsets[k]:t.list_offsets[k + 1]]]
    dirs = np.random.RandomState(5).randn(8, 3)
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    err = np.zeros((3, 3))
    for a, mult in enumerate((4.0, 8.0, 16.0)):
        q = (rec[0:3] + mult * rec[3] * dirs).astype(np.float32)
        truth = VR.winding_number(v, faces, q)
        for order in range(3):
            got = W.expansion(np.repeat(rec[None], len(q), 0), q.astype(np.float64), order) / W.FOUR_PI
            err[order, a] = np.abs(got - truth).max()
    for order, need in enumerate((4.0, 8.0, 16.0)):
        print(f"order {order}: errors {err[order]}, ratios {err[order, 0] / err[order, 1]:.1f} {err[order, 1] / err[order, 2]:.1f}")
        assert err[order, 0] >= need * err[order, 1] and err[order, 1] >= need * err[order, 2], (order, err[order])
    assert np.all(err[2] < err[1]) and np.all(err[1] < err[0])


def test_accuracy_1e30_is_the_exact_sum():
    v, f, pts = named_torus()
    w, stats = W.query(W.build(v, f, 3), pts, accuracy=1e30)[:2]
    truth = VR.winding_number(v, f, pts)
    tri = W.corners(v, f)
    weight = np.array([np.abs(W.solid_angle(tri, np.repeat(q[None].astype(np.float64), len(tri), 0))).sum() for q in pts]) / W.FOUR_PI
    # both sides: F roundings of a running sum of weight at most `weight`, and one atan2 and a dozen products per term
    bound = 2 * (len(f) + 32) * U * weight * 2
    assert np.all(np.abs(w - truth) <= bound), np.abs((w - truth) / bound).max()
    assert np.array_equal(stats, np.repeat([[0, len(f)]], len(pts), 0))


def test_approximation_error_on_the_named_torus():
    """accuracy 2, order 2: max |fast - exact| <= 1e-2 at depth 3 and 4 (the issue's prototype: 3.4e-3 and 3.2e-3, the cap 3x that since
    the method has no closed-form bound); no label differs; accuracy 4 is at least 4x closer (the cell terms scale as beta^-3)."""
    v, f, pts = named_torus()
    truth = VR.winding_number(v, f, pts)
    for depth in (3, 4):
        t = W.build(v, f, depth)
        e2 = np.abs(W.query(t, pts, 2.0)[0] - truth).max()
        e4 = np.abs(W.query(t, pts, 4.0)[0] - truth).max()
        T.log_line(f"RATIO cpu torus 4096 faces depth {depth}: max |fast - exact| {e2:.3e} at accuracy 2 ({e2 / 1e-2:.3f} of the cap), "
                   f"{e4:.3e} at accuracy 4 (a {e2 / e4:.1f}th)")
        assert e2 <= 1e-2
        assert np.array_equal(W.query(t, pts, 2.0)[0] > 0.5, truth > 0.5)
        assert e4 <= e2 / 4


def test_degenerate_input():
    # zero-area faces among proper ones; a cell whose faces all have zero area; every face in one leaf
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [.25, .25, .25], [4, 4, 4]], dtype=np.float32)
    f = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3], [4, 4, 4], [0, 1, 1], [5, 5, 5], [5, 5, 5]], dtype=np.int32)
    q = np.array([[.1, .1, .1], [2, 2, 2], [0, 0, 0], [1, 0, 0], [4, 4, 4], [.25, .25, .25], [-3, 0, 1]], dtype=np.float32)
    truth = VR.winding_number(v, f, q)
    assert np.all(np.isfinite(truth))
    for depth in (1, 3):
        t = W.build(v, f, depth)
        assert all(np.all(np.isfinite(r)) for r in t.records)
        zero = t.records[depth][t.pyramid[depth][t.codes[6]]]
        assert zero[34] == 0.0 and zero[3] == 0.0 and np.all(zero[0:3] == 4.0)  # the mean of the centroids stands in
        for acc in (2.0, 1e30):
            w = W.query(t, q, acc)[0]
            assert np.all(np.isfinite(w))
            assert np.abs(w - truth).max() <= (1e-2 if acc == 2.0 else 1e-14)
        at_p = t.records[0][0, 0:3].astype(np.float32)                           # a query at a cell's centre is never accepted there
        w = W.query(t, at_p[None], 2.0)[0]
        assert np.isfinite(w[0]) and abs(w[0] - VR.winding_number(v, f, at_p[None])[0]) <= 1e-2
    one = W.build(v[:4] * 1e-3 + np.float32(0.5), f[:4], 2)                      # (far vertex dropped: one small tetrahedron)
    one_leaf = W.build(np.vstack([v[:4] * np.float32(1e-3), [[1, 1, 1]]]).astype(np.float32), f[:4], 2)
    assert len(one_leaf.records[2]) == 1 and one_leaf.records[2][0, 35] == 4
    assert np.isfinite(W.query(one, q, 2.0)[0]).all()
    empty = W.build(v, np.zeros((0, 3), dtype=np.int32), 2)
    assert np.array_equal(W.query(empty, q)[0], np.zeros(len(q)))
