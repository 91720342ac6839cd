"""GPU: csrc/knn.hip (vt_knn_points, vt_point_tree_knn, vt_knn_normals) through ``ops.knn``, ``vtaco_amd.utils.pointcloud`` and
``vtaco_amd.common`` against tests/knn_ref.py (the kernels' operations in the kernels' order) and brute force against tree.

d2 and idx are compared for EQUAL BITS and equal integers, no element left out: the list rule is a total order and the walk's skip rule
has no slack term ("knn.hip"), so nothing weaker than equality is the right test.  The normals are held to gates from the
float64 unit roundoff u = 2^-53: residual and Rayleigh quotient within 8 (k + 8) u |C|_F, length within 4 u, angle to numpy's eigh
within 8 (k + 8) u lambda_2 / (lambda_1 - lambda_0); every ratio (error / gate) is printed and, with VTACO_RATIO_LOG naming a file,
appended to it (profiles/knn_f64_ratios.txt is made so)."""
import numpy as np
import pytest
import torch

import icp_ref as R
import knn_ref as K
import point_tree_ref as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def host(*ts):
    return tuple(t.cpu().numpy() for t in ts)


def same(got, want):
    """d2 equal bit for bit and idx equal, shapes and types included."""
    (gd, gi), (wd, wi) = got[:2], want[:2]
    assert gd.dtype == wd.dtype == np.float64 and gi.dtype == wi.dtype == np.int32 and gd.shape == wd.shape and gi.shape == wi.shape
    return np.array_equal(np.ascontiguousarray(gd).view(np.uint64), np.ascontiguousarray(wd).view(np.uint64)) and np.array_equal(gi, wi)


def check_case(tag, src, dst, k, T=None, depth=None, lanes=("morton",), want=None, slabs=(None,)):
    """Device brute force == restatement == device tree (every lane order, stats against the restatement's walk); returns the lists."""
    from vtaco_amd import ops
    want = K.brute(src, dst, k, T) if want is None else want
    for slab in slabs:
        got = host(*ops.knn.knn_points(dev(src), dev(dst), k, T=dev(T), slab=slab))
        assert same(got, want), (tag, k, "brute", slab)
    tree = ops.icp.point_tree_build(dev(dst), depth)
    ref = P.build(dst, depth)
    w_tree = K.tree(ref, src, k, T)
    assert same(w_tree, want), (tag, k, "restated tree")
    for order in lanes:
        d2, idx, stats = host(*ops.knn.knn_points(dev(src), dev(dst), k, T=dev(T), method="tree", tree=tree, lanes=order, stats=True))
        assert same((d2, idx), want), (tag, k, "tree", order)
        assert np.array_equal(stats, w_tree[2]), (tag, k, "stats", order)
    return want


def test_k1_is_nn_points_bit_for_bit():
    from vtaco_amd import ops
    src, dst, T = K.k1_case()
    n_d2, n_idx = host(*ops.icp.nn_points(dev(src), dev(dst), T=dev(T)))
    for method in ("brute", "tree"):
        d2, idx = host(*ops.knn.knn_points(dev(src), dev(dst), 1, T=dev(T), method=method))
        assert d2.shape == (2, 257, 1) and same((d2[..., 0], idx[..., 0]), (n_d2, n_idx)), method
    for b in range(2):
        assert same((n_d2[b, :, None], n_idx[b, :, None]), K.brute(src[b], dst[b], 1, T[b]))


def test_lists_shorter_than_k_keep_the_tail():
    for src, dst, k in K.short_cases():
        d2, idx = check_case(f"short M {len(dst)}", src, dst, k)
        assert (idx[:, len(dst):] == -1).all() and np.isinf(d2[:, len(dst):]).all() and (idx[:, :min(k, len(dst))] >= 0).all()


@pytest.mark.parametrize("k", [8, 16, 32])
def test_ties_on_a_doubled_lattice(k):
    src, dst = K.tie_case()
    want = K.brute(src, dst, k)
    for depth in (1, 2, None):
        check_case(f"ties depth {depth}", src, dst, k, depth=depth, lanes=("query", "morton"), want=want)


@pytest.mark.parametrize("N", [1, 255, 256, 257])
def test_tile_and_slab_edges(N):
    from vtaco_amd import ops
    src, dst = K.edge_case(N)
    slab = ops.knn.knn_slab_points(N, len(dst))
    assert slab == K.slab_points(N, len(dst)) and len(dst) == 2 * slab + 1
    for k in (8, 32):
        _, idx = check_case(f"edges N {N}", src, dst, k, slabs=(None, 256, slab, 4 * slab))
        assert (idx[0] < slab).any() and (idx[0] >= slab).any()


def test_one_cell_of_coincident_points():
    src, dst = K.one_cell_case()
    d2, idx = check_case("one cell", src, dst, 8)
    assert (idx[:2] == np.arange(8)).all() and (d2[:2] == d2[:2, :1]).all()


def test_nan_rows_and_a_batch_answered_from_its_own_targets():
    from vtaco_amd import ops
    src, dst = K.batch_case()
    tree = ops.icp.point_tree_build(dev(dst))
    got = [host(*ops.knn.knn_points(dev(src), dev(dst), 4)), host(*ops.knn.knn_points(dev(src), dev(dst), 4, method="tree", tree=tree))]
    for b in range(3):
        want = K.brute(src[b], dst[b], 4)
        bad = ~np.isfinite(src[b]).all(1)
        assert (want[1][bad] == -1).all() and np.isinf(want[0][bad]).all() and bad.sum() == 1
        for d2, idx in got:
            assert same((d2[b], idx[b]), want), b


@pytest.mark.parametrize("k", [8, 32])
def test_pruning_on_20000_uniform_points(k):
    from vtaco_amd import ops
    cloud = K.pruning_cloud()
    w_d2, w_idx, w_stats = K.pruning_ref(k)
    assert float(w_stats[:, 1].mean()) < len(cloud) / 4                      # the cap holds for the restatement's own count
    pts = dev(cloud)
    b_d2, b_idx = host(*ops.knn.knn_points(pts, pts, k))
    d2, idx, stats = host(*ops.knn.knn_points(pts, pts, k, method="tree", stats=True))
    assert same((d2, idx), (b_d2, b_idx)) and same((d2, idx), (w_d2, w_idx))
    assert np.array_equal(stats, w_stats)
    mean = float(stats[:, 1].mean())
    R.ratio(f"knn pruning k {k}: mean points tested per query / (M / 4)", mean, len(cloud) / 4)
    assert mean < len(cloud) / 4


def test_every_walk_gives_the_same_lists(monkeypatch):
    from vtaco_amd import ops
    src, dst = K.edge_case(257)
    want = K.brute(src, dst, 16)
    tree, ref = ops.icp.point_tree_build(dev(dst)), P.build(dst)
    for walk in P.WALKS:
        monkeypatch.setenv("VTACO_POINT_TREE_WALK", walk)
        d2, idx, stats = host(*ops.knn.knn_points(dev(src), dev(dst), 16, method="tree", tree=tree, stats=True))
        assert same((d2, idx), want), walk
        assert np.array_equal(stats, K.tree(ref, src, 16, None, *P.WALKS[walk])[2]), walk


def test_arguments_are_checked():
    from vtaco_amd import ops
    from vtaco_amd._lib import VtError
    a, b = dev(np.zeros((4, 3))), dev(np.ones((9, 3)))
    tree = ops.icp.point_tree_build(b)
    for bad in (lambda: ops.knn.knn_points(a, b, 0), lambda: ops.knn.knn_points(a, b, 33), lambda: ops.knn.knn_points(a.cpu(), b.cpu(), 2),
                lambda: ops.knn.knn_points(a, b, 2, tree=tree), lambda: ops.knn.knn_points(a, a, 2, method="tree", tree=tree),
                lambda: ops.knn.knn_points(a, b, 2, slab=100), lambda: ops.knn.knn_points(a, b, 2, method="kd")):
        with pytest.raises(VtError):
            bad()


# ---- normals ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [8, 16, 32])
@pytest.mark.parametrize("name", ["plane", "sphere"])
def test_normals_meet_the_float64_gates(name, k):
    from vtaco_amd import ops
    cloud = K.normal_clouds()[name]
    pts = dev(cloud)
    _, idx = ops.knn.knn_points(pts, pts, k)
    n, lam = host(*ops.knn.normals(pts, idx))
    idx = idx.cpu().numpy()
    assert np.array_equal(idx, K.brute(cloud, cloud, k)[1])
    C, _ = K.covariance(cloud, idx)
    w, v = np.linalg.eigh(C)
    gap = (w[:, 1] - w[:, 0]) / w[:, 2]
    assert float(gap.min()) >= K.GAPS[k]
    ratios = np.array([K.normal_gates(C[j], n[j], lam[j, 0], k) for j in range(len(cloud))])          # no point is excluded
    sin = np.linalg.norm(np.cross(n, v[:, :, 0]), axis=1)
    angle = sin / (8.0 * (k + 8) * K.U / gap)
    worst = [R.ratio(f"knn normals {name} k {k} {what}", float(x.max()), 1.0)
             for what, x in (("residual", ratios[:, 0]), ("rayleigh", ratios[:, 1]), ("length", ratios[:, 2]), ("angle to eigh", angle))]
    assert max(worst) <= 1.0, worst
    assert (np.diff(lam, axis=1) >= 0).all()
    r_n, r_lam = K.normals(cloud, idx)
    R.ratio(f"knn normals {name} k {k} |normal - restatement| / u", float(np.abs(n - r_n).max()), K.U)
    big = np.abs(n).argmax(1)
    assert (n[np.arange(len(n)), big] > 0).all()                              # without a view: the largest component is positive
    if name == "sphere":
        inward, _ = host(*ops.knn.normals(pts, dev(idx), view=dev(np.zeros(3))))
        assert ((inward * cloud).sum(1) < 0).all()                           # towards the centre
        assert np.array_equal(np.abs(inward), np.abs(n))
        per_point, _ = host(*ops.knn.normals(pts, dev(idx), view=dev(2.0 * cloud)))
        assert ((per_point * cloud).sum(1) > 0).all()


def test_degenerate_neighbourhoods():
    from vtaco_amd import ops
    rng = np.random.default_rng(51)
    t = rng.random(16)
    direction = np.array([1.0, 2.0, -0.5]) / np.linalg.norm([1.0, 2.0, -0.5])
    pts = np.concatenate([np.tile([[0.3, -0.7, 0.11]], (16, 1)), np.array([0.2, 0.1, -0.3]) + t[:, None] * direction])
    idx = np.stack([np.arange(16), np.arange(16), np.arange(16, 32), np.arange(16)]).astype(np.int32)
    idx[1, 2:] = -1                                                          # two valid neighbours
    idx[3, 5:] = 40                                                          # coincident, the rest outside [0, M)
    n, lam = host(*ops.knn.normals(dev(pts), dev(idx)))
    assert np.isfinite(n).all() and np.isfinite(lam).all()
    for row in (0, 1, 3):
        assert (n[row] == 0).all() and (lam[row] == 0).all(), row
    C, _ = K.covariance(pts, idx)
    res, ray, length = K.normal_gates(C[2], n[2], lam[2, 0], 16)
    R.ratio("knn normals collinear residual", res, 1.0)
    assert res <= 1.0 and length <= 1.0
    assert abs(float(n[2] @ direction)) <= 8.0 * 24 * K.U * np.sqrt((C[2] * C[2]).sum()) / lam[2, 2]     # the residual gate over the line's eigenvalue


# ---- what is built on them ---------------------------------------------------------------------------------------------------------------
def test_statistical_outlier_mask_drops_exactly_the_planted_points():
    from vtaco_amd.utils import pointcloud
    pts, planted = K.outlier_cloud()
    want, stat, thr = K.outlier_mask(pts)
    assert np.abs(stat / thr - 1.0).min() > 1e-9                             # no point near the threshold: rounding cannot change the mask
    mask = pointcloud.statistical_outlier_mask(dev(pts))
    assert mask.dtype == torch.bool and mask.is_cuda
    assert np.array_equal(mask.cpu().numpy(), want) and np.array_equal(np.nonzero(~want)[0], planted)
    kept, m2 = pointcloud.remove_statistical_outliers(dev(pts)[None].repeat(2, 1, 1))
    assert len(kept) == 2 and kept[0].shape == (len(pts) - 20, 3) and np.array_equal(m2[1].cpu().numpy(), want)
    dist, idx = pointcloud.knn(dev(pts), 4)
    assert (idx[:, 0].cpu().numpy() == np.arange(len(pts))).all() and (dist[:, 0] == 0).all()
    nrm, eig = pointcloud.estimate_normals(dev(pts), k=16)
    assert nrm.shape == eig.shape == (len(pts), 3) and float(pointcloud.surface_variation(eig).max()) <= 1.0 / 3.0 + 1e-12


@pytest.mark.parametrize("k", [1, 4])
def test_neighbour_batch_on_the_device_equals_the_restatement(k):
    from vtaco_amd import common
    src, dst, _ = K.k1_case()
    for method in ("brute", "tree"):
        idx, dist = common.get_nearest_neighbors_indices_batch(src, dst, k=k, method=method)
        for b in range(2):
            d2, want = K.brute(src[b], dst[b], k)
            assert idx[b].shape == ((257,) if k == 1 else (257, k))
            assert np.array_equal(idx[b].reshape(257, k), want) and np.array_equal(dist[b].reshape(257, k), np.sqrt(d2))
    idx, dist = common.get_nearest_neighbors_indices_batch([src[0], src[1][:100]], [dst[0][:50], dst[1]], k=k)
    assert np.array_equal(idx[1].reshape(100, k), K.brute(src[1][:100], dst[1], k)[1])
