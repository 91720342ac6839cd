"""CPU: tests/knn_ref.py (the numpy restatement of csrc/knn.hip) against itself and against scipy, and the host-side code that ships
with it: utils/io.py and common.get_nearest_neighbors_indices_batch (through a stub in place of the device).

The walk of the tree and the brute force are compared for EQUAL BITS on every input tests/test_knn_gpu.py uses: the skip rule has no
slack, so nothing weaker is the right test."""
import numpy as np
import pytest

import knn_ref as K
import point_tree_ref as P


def same(a, b):
    return np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64)) and np.array_equal(a[1], b[1])


def tree_is_brute(src, dst, k, T=None, depth=None, walks=("seed+order",)):
    want = K.brute(src, dst, k, T)
    ref = P.build(dst, depth)
    for walk in walks:
        got = K.tree(ref, src, k, T, *P.WALKS[walk])
        assert same(got[:2], want), (k, depth, walk)
    return want


def test_tree_equals_brute_on_the_k1_batch_and_k1_is_the_nearest_neighbour():
    src, dst, T = K.k1_case()
    for b in range(2):
        d2, idx = tree_is_brute(src[b], dst[b], 1, T[b], walks=tuple(P.WALKS))
        n_d2, n_idx = P.brute(src[b], dst[b], T[b])
        assert same((d2[:, 0], idx[:, 0]), (n_d2, n_idx))


def test_short_lists_keep_a_tail_of_inf_and_minus_one():
    for src, dst, k in K.short_cases():
        d2, idx = tree_is_brute(src, dst, k)
        M = len(dst)
        assert (idx[:, :min(k, M)] >= 0).all() and (idx[:, M:] == -1).all() and np.isinf(d2[:, M:]).all()
        assert all(sorted(row[:M]) == list(range(M)) for row in idx.tolist()) if M <= k else True


@pytest.mark.parametrize("k", [8, 16, 32])
def test_ties_go_to_the_lowest_index(k):
    src, dst = K.tie_case()
    for depth in (1, 2, None):
        d2, idx = tree_is_brute(src, dst, k, depth=depth)
    assert (np.diff(d2, axis=1) >= 0).all()
    tie = np.diff(d2, axis=1) == 0
    assert tie.any() and (np.diff(idx, axis=1)[tie] > 0).all()
    assert (idx[:64, 0] == np.arange(64)).all() and (idx[:64, 1] == np.arange(64) + 64).all()     # a lattice point: itself, then its copy


@pytest.mark.parametrize("N", [1, 255, 256, 257])
def test_tile_and_slab_edges(N):
    src, dst = K.edge_case(N)
    slab = K.slab_points(N, len(dst))
    assert len(dst) == 2 * slab + 1
    for k in (8, 32):
        _, idx = tree_is_brute(src, dst, k)
        assert (idx[0] < slab).any() and (idx[0] >= slab).any()              # the first query's neighbours lie on both sides of the edge
    if N == 257:
        tree_is_brute(src, dst, 16, walks=tuple(P.WALKS))                    # the input of the GPU test of the four walks


def test_one_cell_and_bad_queries():
    src, dst = K.one_cell_case()
    d2, idx = tree_is_brute(src, dst, 8)
    assert (idx[:2] == np.arange(8)).all() and (d2[:2] == d2[:2, :1]).all() and d2[0, 0] == 0.0
    src, dst = K.batch_case()
    for b in range(3):
        d2, idx = tree_is_brute(src[b], dst[b], 4)
        bad = ~np.isfinite(src[b]).all(1)
        assert bad.sum() == 1 and (idx[bad] == -1).all() and np.isinf(d2[bad]).all() and (idx[~bad] >= 0).all()


def test_pruning_case_tree_equals_brute_and_tests_few_points():
    cloud = K.pruning_cloud()
    want = K.brute(cloud, cloud, 32)
    for k in (8, 32):
        d2, idx, stats = K.pruning_ref(k)
        assert same((d2, idx), (want[0][:, :k].copy(), want[1][:, :k].copy()))
        mean = float(stats[:, 1].mean())
        print(f"knn pruning k {k}: mean points tested per query {mean:.1f} of {len(cloud)} (cap {len(cloud) / 4:.0f})")
        assert mean < len(cloud) / 4
    assert (want[1][:, 0] == np.arange(len(cloud))).all() and (want[0][:, 0] == 0.0).all()       # a self-query finds itself first


def test_restatement_against_scipy_on_tie_free_clouds():
    spatial = pytest.importorskip("scipy.spatial")
    rng = np.random.default_rng(175)
    for N, M, k in ((300, 1000, 1), (257, 600, 8), (64, 2000, 32)):
        src, dst = rng.random((N, 3)) - 0.5, rng.random((M, 3)) - 0.5
        d2, idx = K.brute(src, dst, k)
        assert (np.diff(d2, axis=1) > 0).all()                               # tie-free: the order is the distances' alone
        dist, at = spatial.cKDTree(dst).query(src, k=k)
        dist, at = dist.reshape(N, k), at.reshape(N, k)
        assert np.array_equal(at, idx)
        want = np.sqrt(d2)
        assert (np.abs(dist - want) <= 2 * np.spacing(want)).all()


def test_normal_clouds_have_the_stated_gaps_and_the_restatement_meets_the_gates():
    for name, cloud in K.normal_clouds().items():
        for k in (8, 16, 32):
            _, idx = K.brute(cloud, cloud, k)
            C, _ = K.covariance(cloud, idx)
            w, v = np.linalg.eigh(C)
            assert float(((w[:, 1] - w[:, 0]) / w[:, 2]).min()) >= K.GAPS[k], (name, k)
            n, lam = K.normals(cloud, idx)
            worst = np.max([K.normal_gates(C[j], n[j], lam[j, 0], k) for j in range(len(cloud))], axis=0)
            assert (worst <= 1.0).all(), (name, k, worst)
            big = np.abs(n).argmax(1)
            assert (n[np.arange(len(n)), big] > 0).all()


def test_tree_equals_brute_on_the_clouds_of_the_normals_and_the_outlier_rule():
    for cloud in K.normal_clouds().values():
        for k in (8, 16, 32):
            tree_is_brute(cloud, cloud, k)
    pts, _ = K.outlier_cloud()
    for k in (4, 16, 20):
        tree_is_brute(pts, pts, k)


def test_outlier_rule_drops_exactly_the_planted_points():
    pts, planted = K.outlier_cloud()
    mask, stat, thr = K.outlier_mask(pts)
    assert np.array_equal(np.nonzero(~mask)[0], planted)
    assert np.abs(stat / thr - 1.0).min() > 1e-9


# ---- utils/io.py -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("as_text", [True, False])
@pytest.mark.parametrize("with_normals", [False, True])
def test_pointcloud_round_trip(tmp_path, as_text, with_normals):
    from vtaco_amd.utils import io
    rng = np.random.default_rng(6)
    v = (rng.standard_normal((37, 3)) * 10.0).astype(np.float32)
    n = rng.standard_normal((37, 3)).astype(np.float32)
    path = str(tmp_path / "cloud.ply")
    io.export_pointcloud(v.astype(np.float64), path, as_text=as_text, normals=n if with_normals else None)
    head = open(path, "rb").read(64)
    assert head.startswith(b"ply\nformat ascii 1.0\n" if as_text else b"ply\nformat binary_little_endian 1.0\n")
    got = io.load_pointcloud(path)
    assert got.dtype == np.float32 and np.array_equal(got, v)
    got_v, got_n = io.load_pointcloud(path, with_normals=True)
    assert np.array_equal(got_v, v)
    assert np.array_equal(got_n, n) if with_normals else got_n is None


def test_load_pointcloud_reads_what_mesh_export_writes(tmp_path):
    import torch
    from vtaco_amd.conv_onet.generation import Mesh
    from vtaco_amd.utils import io
    v = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.1, 0.2, 0.3]], dtype=torch.float32)
    f = torch.tensor([[0, 1, 2], [1, 3, 2]])
    path = str(tmp_path / "mesh.ply")
    Mesh(v, f).export(path)
    assert np.array_equal(io.load_pointcloud(path), v.numpy())
    off = str(tmp_path / "mesh.off")
    Mesh(v, f).export(off)
    vs, fs = io.read_off(off)
    assert isinstance(vs, list) and isinstance(fs, list) and np.array_equal(np.array(vs, dtype=np.float32), v.numpy())
    assert fs == [[3, 0, 1, 2], [3, 1, 3, 2]]


def test_read_off_takes_both_header_forms(tmp_path):
    from vtaco_amd._lib import VtError
    from vtaco_amd.utils import io
    body = "0 0 0\n1 0 0\n0 1.5 0\n3 0 1 2\n"
    a, b = tmp_path / "a.off", tmp_path / "b.off"
    a.write_text("OFF\n3 1 0\n" + body)
    b.write_text("OFF3 1 0\n" + body)
    assert io.read_off(str(a)) == io.read_off(str(b)) == ([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.5, 0.0]], [[3, 0, 1, 2]])
    bad = tmp_path / "c.off"
    bad.write_text("PLY\n")
    with pytest.raises(VtError):
        io.read_off(str(bad))


# ---- common.get_nearest_neighbors_indices_batch ---------------------------------------------------------------------------------------
def test_neighbour_batch_shapes_and_types_through_a_stub(monkeypatch):
    import torch
    from vtaco_amd import common
    from vtaco_amd._lib import VtError
    calls = []

    def stub(src, dst, k, method):
        calls.append((src.shape, dst.shape, k, method))
        out = [K.brute(s, d, k) for s, d in zip(src, dst)]
        return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])

    monkeypatch.setattr(common, "_knn_device", stub)
    rng = np.random.default_rng(4)
    src, dst = rng.random((2, 50, 3)), rng.random((2, 70, 3))
    for k in (1, 4):
        idx, dist = common.get_nearest_neighbors_indices_batch(src, torch.from_numpy(dst), k=k)
        assert isinstance(idx, list) and isinstance(dist, list) and len(idx) == len(dist) == 2
        for b in range(2):
            assert idx[b].shape == dist[b].shape == ((50,) if k == 1 else (50, 4))
            assert idx[b].dtype == np.int64 and dist[b].dtype == np.float64
            d2, want = K.brute(src[b], dst[b], k)
            assert np.array_equal(idx[b].reshape(50, k), want) and np.array_equal(dist[b].reshape(50, k), np.sqrt(d2))
    assert calls == [((2, 50, 3), (2, 70, 3), 1, "brute"), ((2, 50, 3), (2, 70, 3), 4, "brute")]
    del calls[:]
    idx, dist = common.get_nearest_neighbors_indices_batch([src[0], src[1][:20]], [dst[0], dst[1]], k=4, method="tree")
    assert [c[0] for c in calls] == [(1, 50, 3), (1, 20, 3)] and idx[1].shape == (20, 4)
    with pytest.raises(VtError, match="32"):
        common.get_nearest_neighbors_indices_batch(src, dst, k=33)
