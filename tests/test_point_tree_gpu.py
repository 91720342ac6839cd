"""GPU: csrc/point_tree.hip (vt_point_tree_*) and vt_icp_tree through ``ops.icp``, ``vtaco_amd.utils.icp`` and ``vtaco_amd.eval`` against
tests/point_tree_ref.py (the kernel's operations in the kernel's order, stats included) and against ``ops.icp.nn_points(method='brute')``.

d2, idx, stats, the tree's arrays, and T, distances, idx and iterations of the loop are compared for EQUAL BITS, no element left out: the
walk's skip rule has no slack term ("point_tree.hip"), so nothing weaker than equality is the right test."""
import os

import numpy as np
import pytest
import torch

import closest_point_ref as CP
import icp_ref as R
import point_tree_ref as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def same_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    return np.array_equal(got.view(np.uint8), want.view(np.uint8))


def log(line):
    print(line)
    if os.environ.get("VTACO_RATIO_LOG"):
        with open(os.environ["VTACO_RATIO_LOG"], "a") as fh:
            fh.write(line + "\n")


@pytest.fixture(scope="module")
def clouds():
    return P.clouds()


@pytest.fixture(scope="module")
def g28():
    return np.load(R.GOLDEN)


def set_walk(monkeypatch, walk):
    if walk is None:
        monkeypatch.delenv("VTACO_POINT_TREE_WALK", raising=False)
    else:
        monkeypatch.setenv("VTACO_POINT_TREE_WALK", walk)


def check_case(tag, src, dst, T=None, depth=None, walks=("seed+order",), monkeypatch=None):
    """Device tree query == restatement (d2, idx, stats) == device brute force, bit for bit; returns the device tree."""
    from vtaco_amd import ops
    tree = ops.icp.point_tree_build(dev(dst), depth)
    ref = P.build(dst, depth)
    assert tree.depth == ref["depth"] and tree.counts == ref["counts"] and tree.status == 0
    b_d2, b_idx = ops.icp.nn_points(dev(src), dev(dst), T=dev(T), method="brute")
    b_d2, b_idx = b_d2.cpu().numpy(), b_idx.cpu().numpy()
    most = 0.0
    for walk in walks:
        if monkeypatch is not None:
            set_walk(monkeypatch, walk)
        d2, idx, stats = ops.icp.point_tree_query(tree, dev(src), T=dev(T), stats=True)
        d2, idx, stats = d2.cpu().numpy(), idx.cpu().numpy(), stats.cpu().numpy()
        w_d2, w_idx, w_stats = P.query(ref, src, T, *P.WALKS[walk])
        assert np.array_equal(idx, w_idx) and same_bits(d2, w_d2), (tag, walk)
        assert np.array_equal(stats, w_stats), (tag, walk)
        assert np.array_equal(idx, b_idx) and same_bits(d2, b_d2), (tag, walk)
        most = max(most, float(stats[:, 1].mean()) / len(dst))
    log(f"EQUAL BITS point_tree {tag}: d2, idx, stats ({len(src)} x {len(dst)}, depth {tree.depth}, {'/'.join(walks)}); "
        f"points tested per query / M at most {most:.3e}")
    return tree, ref


# ---- the size grid -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", P.SIZES)
@pytest.mark.parametrize("N", P.SIZES)
def test_grid_of_sizes_equals_the_restatement_and_brute_force(clouds, N, M):
    src, dst = clouds[("src", N)], clouds[("dst", M)]
    check_case(f"grid {N}x{M}", src, dst)
    check_case(f"grid {N}x{M} pose", src, dst, P.pose_of(N * 10000 + M))


@pytest.mark.parametrize("depth", [1, 2, 3, None])
def test_depths_and_all_four_walks(clouds, monkeypatch, depth):
    check_case(f"walks depth {depth}", clouds[("src", 257)], clouds[("dst", 1025)], depth=depth, walks=tuple(P.WALKS), monkeypatch=monkeypatch)


def test_tree_arrays_equal_the_definition_byte_for_byte(clouds):
    from vtaco_amd import ops
    dst = clouds[("dst", 1025)]
    tree, ref = ops.icp.point_tree_build(dev(dst)), P.build(dst)
    assert tree.depth == ref["depth"] and tree.counts == ref["counts"]
    frame = tree.frame().cpu().numpy()
    assert same_bits(frame[:3], ref["lo"]) and frame[3] == ref["side"]
    for l in range(tree.depth + 1):
        assert np.array_equal(tree.pyramid(l).cpu().numpy(), ref["pyramids"][l]), l
        assert same_bits(tree.boxes(l).cpu().numpy(), ref["boxes"][l]), l
    assert np.array_equal(tree.list_offsets().cpu().numpy(), ref["offsets"])
    assert np.array_equal(tree.lists().cpu().numpy(), ref["lists"])
    assert same_bits(tree.points().cpu().numpy(), ref["points"])
    log("EQUAL BITS point_tree build 1025: pyramids, offsets, lists, boxes, points")


def test_a_minimum_of_minus_zero_is_stored_as_plus_zero(clouds):
    """The point tree adds + 0.0 to the frame's minimum corner (the face tree does not): the sign bit of a zero is part of the bytes."""
    from vtaco_amd import ops
    dst = clouds[("dst", 64)].copy()
    dst[:, 1] -= dst[:, 1].min()
    dst[dst[:, 1] == 0, 1] = -0.0                                   # y is -0.0 or positive: no +0.0 for the minimum to tie with
    assert np.signbit(dst[:, 1].min()) and (dst[:, 1] == 0).sum() == 1
    tree, ref = ops.icp.point_tree_build(dev(dst), 2), P.build(dst, 2)
    assert not np.signbit(ref["lo"][1]) and ref["lo"][1] == 0.0
    assert tree.frame().cpu().numpy().tobytes() == np.append(ref["lo"], ref["side"]).tobytes()
    assert tree.counts == ref["counts"]
    for l in range(tree.depth + 1):
        assert np.array_equal(tree.pyramid(l).cpu().numpy(), ref["pyramids"][l]), l
        assert same_bits(tree.boxes(l).cpu().numpy(), ref["boxes"][l]), l
    assert np.array_equal(tree.list_offsets().cpu().numpy(), ref["offsets"])
    assert np.array_equal(tree.lists().cpu().numpy(), ref["lists"])
    assert same_bits(tree.points().cpu().numpy(), ref["points"])


# ---- degenerate sets and awkward queries ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(P.special_cases()))
def test_special_cases(monkeypatch, name):
    src, dst, depth = P.special_cases()[name]
    tree, ref = check_case(name, src, dst, depth=depth, walks=("plain", "seed+order"), monkeypatch=monkeypatch)
    set_walk(monkeypatch, None)
    from vtaco_amd import ops
    d2, idx = (t.cpu().numpy() for t in ops.icp.point_tree_query(tree, dev(src)))
    if name == "sparse_deep":
        assert tree.depth == 7 and tree.counts[7] <= 65
    if name == "all_equal":
        assert tree.frame().cpu().numpy()[3] == 1.0 and (idx == 0).all()
    if name == "duplicates":                                          # dst = [reversed, plain, first 100]: the winner is in the reversed copy
        assert (idx < 600).all() and same_bits(dst[idx], dst[600:1200][599 - idx])
    if name == "lattice_twice":
        assert (idx < 729).all() and not d2[:729].any()
    if name == "on_targets":
        assert not d2.any() and np.array_equal(idx, np.arange(0, 1025, 3))
    if name == "nonfinite_queries":
        assert np.isposinf(d2[:6]).all() and (idx[:6] == -1).all() and np.isfinite(d2[6:]).all()


def test_float32_inputs_and_a_batch_of_three(clouds):
    from vtaco_amd import ops
    s32, d32 = clouds[("src", 257)].astype(np.float32), clouds[("dst", 600)].astype(np.float32)
    d2, idx = ops.icp.nn_points(dev(s32), dev(d32), method="tree")
    w_d2, w_idx = R.kernel_order.nn(s32.astype(np.float64), d32.astype(np.float64))
    assert d2.dtype == torch.float64 and np.array_equal(idx.cpu().numpy(), w_idx) and same_bits(d2.cpu().numpy(), w_d2)
    src, dst, T = P.batch_of_three()
    flat = dst.copy()
    flat[1, :, 2] = flat[1, 0, 2]                                     # depth 1: problem 0 fills 8 leaves, problem 1 (a plane) 4, problem 2 3
    for depth, dst in ((None, dst), (1, flat)):
        tree = ops.icp.point_tree_build(dev(dst), depth)
        assert tree.depth == (3 if depth is None else depth)
        d2, idx, stats = ops.icp.point_tree_query(tree, dev(src), T=dev(T), stats=True)
        b_d2, b_idx = ops.icp.nn_points(dev(src), dev(dst), T=dev(T))
        assert same_bits(d2.cpu().numpy(), b_d2.cpu().numpy()) and np.array_equal(idx.cpu().numpy(), b_idx.cpu().numpy())
        assert len({tuple(c) for c in tree.counts}) == 3              # different occupancies share one layout
        for b in range(3):
            ref = P.build(dst[b], depth)
            w_d2, w_idx, w_stats = P.query(ref, src[b], T[b])
            assert same_bits(d2[b].cpu().numpy(), w_d2) and np.array_equal(idx[b].cpu().numpy(), w_idx), (depth, b)
            assert np.array_equal(stats[b].cpu().numpy(), w_stats), (depth, b)
            assert tree.counts[b] == ref["counts"]
            for l in range(tree.depth + 1):
                assert np.array_equal(tree.pyramid(l, b).cpu().numpy(), ref["pyramids"][l]), (depth, b, l)
                assert same_bits(tree.boxes(l, b).cpu().numpy(), ref["boxes"][l]), (depth, b, l)
            assert np.array_equal(tree.lists(b).cpu().numpy(), ref["lists"]) and same_bits(tree.points(b).cpu().numpy(), ref["points"])
            assert np.array_equal(tree.list_offsets(b).cpu().numpy(), ref["offsets"])
    log("EQUAL BITS point_tree batch of 3: d2, idx, stats, boxes, lists, points per problem")


# ---- lane order: which lane answers a query, never a result ------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", ["query", "morton"])
def test_lane_order_changes_no_bit(clouds, g28, lanes):
    from vtaco_amd import ops
    for depth in (1, None, 7):
        src, dst = clouds[("src", 1025)], clouds[("dst", 1025)]
        tree, ref = ops.icp.point_tree_build(dev(dst), depth), P.build(dst, depth)
        T = P.pose_of(7)
        d2, idx, stats = ops.icp.point_tree_query(tree, dev(src), T=dev(T), stats=True, lanes=lanes)
        w_d2, w_idx, w_stats = P.query(ref, src, T)
        assert same_bits(d2.cpu().numpy(), w_d2) and np.array_equal(idx.cpu().numpy(), w_idx) and np.array_equal(stats.cpu().numpy(), w_stats)
    src, dst, T = P.batch_of_three()
    tree = ops.icp.point_tree_build(dev(dst))
    got = ops.icp.point_tree_query(tree, dev(src), T=dev(T), stats=True, lanes=lanes)
    for b in range(3):
        want = P.query(P.build(dst[b]), src[b], T[b])
        assert same_bits(got[0][b].cpu().numpy(), want[0]) and np.array_equal(got[1][b].cpu().numpy(), want[1])
        assert np.array_equal(got[2][b].cpu().numpy(), want[2])
    A = np.stack([g28[n + ".A"] for n in R.BATCH_CASES])                   # the loop: the order is taken once, frozen problems stay frozen
    B = np.stack([g28[n + ".B"] for n in R.BATCH_CASES])
    iters, tol = int(g28["batch0.max_iterations"]), float(g28["batch0.tolerance"])
    brute = ops.icp.icp(dev(A), dev(B), max_iterations=iters, tolerance=tol)
    loop = ops.icp.icp(dev(A), dev(B), max_iterations=iters, tolerance=tol, method="tree", lanes=lanes)
    for g, w in zip(loop, brute):
        assert same_bits(g.cpu().numpy(), w.cpu().numpy())
    log(f"EQUAL BITS point_tree lanes={lanes}: d2, idx, stats at depths 1, 3 and 7 and a batch of three; the batched loop against brute")


# ---- the loop ----------------------------------------------------------------------------------------------------------------------------
def loop_pair(g28, name, **kw):
    from vtaco_amd import ops
    A, B, pose, iters, tol = R.case_of(g28, name)
    brute = ops.icp.icp(dev(A), dev(B), init_pose=dev(pose), max_iterations=iters, tolerance=tol)
    tree = ops.icp.icp(dev(A), dev(B), init_pose=dev(pose), max_iterations=iters, tolerance=tol, method="tree", **kw)
    return tuple(t.cpu().numpy() for t in brute), tuple(t.cpu().numpy() for t in tree)


@pytest.mark.parametrize("name", R.LOOP_CASES + R.BATCH_CASES)
def test_loop_on_a_tree_equals_the_brute_loop(g28, name):
    (b_T, b_d, b_idx, b_its), (T, distances, idx, its) = loop_pair(g28, name)
    assert int(its) == int(b_its) and np.array_equal(idx, b_idx)
    assert same_bits(T, b_T) and same_bits(distances, b_d)
    R.check_loop_against_fixture(g28, name, "gpu tree", T, distances, its, idx)
    log(f"EQUAL BITS icp tree {name}: T, distances, idx, iterations ({int(its) + 1} iterations)")


def test_batch_of_three_on_trees_freezes_finished_problems(g28):
    from vtaco_amd import ops
    A = np.stack([g28[n + ".A"] for n in R.BATCH_CASES])
    B = np.stack([g28[n + ".B"] for n in R.BATCH_CASES])
    iters, tol = int(g28["batch0.max_iterations"]), float(g28["batch0.tolerance"])
    brute = ops.icp.icp(dev(A), dev(B), max_iterations=iters, tolerance=tol)
    tree = ops.icp.point_tree_build(dev(B))
    got = ops.icp.icp(dev(A), dev(B), max_iterations=iters, tolerance=tol, method="tree", tree=tree)
    fresh = ops.icp.icp(dev(A), dev(B), max_iterations=iters, tolerance=tol, method="tree")
    T, distances, idx, its = (t.cpu().numpy() for t in got)
    assert len(set(its.tolist())) == 3
    for g, w in zip(got, brute):
        assert same_bits(g.cpu().numpy(), w.cpu().numpy())
    for g, w in zip(got, fresh):                                        # a reused tree and a fresh one
        assert same_bits(g.cpu().numpy(), w.cpu().numpy())
    for b, name in enumerate(R.BATCH_CASES):
        assert int(its[b]) == int(g28[name + ".i"]), name
        R.check_loop_against_fixture(g28, name, "gpu tree batch", T[b], distances[b], its[b], idx[b])


def test_utils_call_forms(g28):
    from vtaco_amd.utils import icp as U
    A, B, pose, iters, tol = R.case_of(g28, "pose")
    w_T, w_d, w_i = U.icp(A, B, init_pose=pose, max_iterations=iters, tolerance=tol)
    n_T, n_d, n_i = U.icp(A, B, init_pose=pose, max_iterations=iters, tolerance=tol, method="tree")
    assert isinstance(n_T, np.ndarray) and isinstance(n_i, int) and n_i == w_i and same_bits(n_T, w_T) and same_bits(n_d, w_d)
    t_T, t_d, t_i = U.icp(dev(A), dev(B), init_pose=dev(pose), max_iterations=iters, tolerance=tol, method="tree")
    assert t_T.is_cuda and t_d.is_cuda and t_i.is_cuda
    assert same_bits(t_T.cpu().numpy(), w_T) and same_bits(t_d.cpu().numpy(), w_d) and int(t_i) == w_i
    dist, ind = U.nearest_neighbor(A, B[:250], method="tree")
    w_d2, w_idx = R.kernel_order.nn(A, B[:250])
    assert ind.dtype == np.int64 and np.array_equal(ind, w_idx) and same_bits(dist, np.sqrt(w_d2))
    dist, ind = U.nearest_neighbor(dev(A), dev(B[:250]), method="tree")
    assert dist.is_cuda and np.array_equal(ind.cpu().numpy(), w_idx) and same_bits(dist.cpu().numpy(), np.sqrt(w_d2))


# ---- Chamfer distance --------------------------------------------------------------------------------------------------------------------
def test_chamfer_kdtree_equals_the_restatement():
    from vtaco_amd import eval as E
    p1, p2 = P.chamfer_clouds()
    c1, c2, i12, i21 = E.chamfer_distance_kdtree(dev(p1), dev(p2), give_id=True)
    both = E.chamfer_distance_kdtree(dev(p1), dev(p2))
    via = E.chamfer_distance(dev(p1), dev(p2))
    assert i12.dtype == torch.int64 and i21.dtype == torch.int64 and c1.dtype == torch.float32 and both.shape == (2,)
    for b in range(2):
        a64, b64 = p1[b].astype(np.float64), p2[b].astype(np.float64)
        d12, w12 = R.kernel_order.nn(a64, b64)
        d21, w21 = R.kernel_order.nn(b64, a64)
        assert np.array_equal(i12[b].cpu().numpy(), w12) and np.array_equal(i21[b].cpu().numpy(), w21)
    d12 = np.stack([R.kernel_order.nn(p1[b].astype(np.float64), p2[b].astype(np.float64))[0] for b in range(2)])
    d21 = np.stack([R.kernel_order.nn(p2[b].astype(np.float64), p1[b].astype(np.float64))[0] for b in range(2)])
    m1, m2 = torch.mean(dev(d12), dim=1), torch.mean(dev(d21), dim=1)   # the restatement's distances through the function's own reduction
    assert same_bits(c1.cpu().numpy(), m1.float().cpu().numpy()) and same_bits(c2.cpu().numpy(), m2.float().cpu().numpy())
    assert same_bits(both.cpu().numpy(), (m1 + m2).float().cpu().numpy())
    for b in range(2):
        assert float(via[b]) == float(both[b])


def test_chamfer_kdtree_against_the_naive_form_and_dispatch():
    """Equal sizes of 2048 points, float32 values given to the tree form as float64 exactly.  The naive form works in float32, u = 2^-24:
    a difference a_k - b_k rounds once, its square once more (relative 3 u on the square, to first order), the sum of the three
    non-negative squares twice: every pair's squared distance is within 5 u relative.  A minimum of values each within 5 u relative is
    within 5 u relative of the true minimum.  The float32 mean of n = 2048 non-negative minima is within (n - 1) u relative in ANY
    summation order, the division by n adds u, the sum of the two means u: (5 + 2047 + 1 + 1) u = 2054 * 2^-24 relative.  The tree
    form's float64 error (below 2^-40 relative) is not worth a term."""
    from vtaco_amd import eval as E
    p1, p2 = P.chamfer_clouds_2048()
    c1, c2, _, _ = E.chamfer_distance_kdtree(dev(p1).double(), dev(p2).double(), give_id=True)
    naive = E.chamfer_distance_naive(dev(p1), dev(p2))
    tree = (c1 + c2)
    bound = 2054 * 2.0 ** -24
    for b in range(2):
        err = abs(float(naive[b]) - float(tree[b])) / float(tree[b])
        log(f"RATIO chamfer kdtree vs naive [{b}]: {err / bound:.3e} (gate {bound:.3e})")
        assert err <= bound
    same = E.chamfer_distance(dev(p1), dev(p2), use_kdtree=False)
    assert same_bits(same.cpu().numpy(), E.chamfer_distance_device(dev(p1), dev(p2)).cpu().numpy())


# ---- aligned mesh distances --------------------------------------------------------------------------------------------------------------
def test_mesh_distances_aligned_with_a_tree_registration():
    from vtaco_amd import eval as E
    gv, gf = CP.torus(24, 12, seed=3)
    Tm = np.identity(4)
    Tm[:3, :3] = R.rodrigues(np.array([0.3, -1.0, 0.5]), 0.1)
    Tm[:3, 3] = 0.03 * np.array([2.0, -1.0, 2.0]) / 3.0
    pv = (gv.astype(np.float64) @ Tm[:3, :3].T + Tm[:3, 3]).astype(np.float32)
    gt, pred = (dev(gv), dev(gf)), (dev(pv), dev(gf))

    def gen():
        return torch.Generator(device=DEV).manual_seed(11)
    want = E.mesh_distances_aligned(pred, gt, 2000, generator=gen(), registration="brute")
    got = E.mesh_distances_aligned(pred, gt, 2000, generator=gen(), registration="tree")
    assert sorted(got) == sorted(want)
    for key in want:
        if key == "transform":
            assert same_bits(got[key], want[key])
        else:
            assert got[key] == want[key], (key, got[key], want[key])


# ---- refusals and reproducibility ------------------------------------------------------------------------------------------------------
def test_refusals():
    from vtaco_amd import ops
    from vtaco_amd._lib import VtError
    a = torch.rand(5, 3, dtype=torch.float64, device=DEV)
    b = torch.rand(6, 3, dtype=torch.float64, device=DEV)
    for bad in (float("nan"), float("inf")):
        c = b.clone()
        c[2, 1] = bad
        with pytest.raises(VtError, match="not finite"):
            ops.icp.point_tree_build(c)
        with pytest.raises(VtError, match="not finite"):
            ops.icp.icp(a, c, method="tree")
    with pytest.raises(VtError, match="empty"):
        ops.icp.point_tree_build(b[:0])
    with pytest.raises(VtError, match="depth"):
        ops.icp.point_tree_build(b, depth=0)
    with pytest.raises(VtError, match="depth"):
        ops.icp.point_tree_build(b, depth=8)
    tree = ops.icp.point_tree_build(b)
    with pytest.raises(VtError, match="built for"):
        ops.icp.icp(a, b[:5], method="tree", tree=tree)
    with pytest.raises(VtError, match="HIP device"):
        ops.icp.point_tree_build(b.cpu())
    with pytest.raises(VtError, match="HIP device"):
        ops.icp.point_tree_query(tree, a.cpu())
    with pytest.raises(VtError, match="PointTree"):
        ops.icp.point_tree_query(b, a)
    with pytest.raises(VtError, match="method"):
        ops.icp.nn_points(a, b, method="kd")
    with pytest.raises(VtError, match="tree="):
        ops.icp.icp(a, b, tree=tree)
    with pytest.raises(VtError, match="lanes"):
        ops.icp.point_tree_query(tree, a, lanes="hilbert")
    from vtaco_amd import eval as E
    with pytest.raises(VtError, match="registration"):
        E.mesh_distances_aligned((a.float(), None), (b.float(), None), 10, registration="kd")


def test_two_builds_and_two_queries_give_equal_bytes(clouds):
    from vtaco_amd import ops
    src, dst = dev(clouds[("src", 1025)]), dev(clouds[("dst", 1025)])
    t1, t2 = ops.icp.point_tree_build(dst), ops.icp.point_tree_build(dst)
    assert t1.counts == t2.counts
    for l in range(t1.depth + 1):
        assert same_bits(t1.boxes(l).cpu().numpy(), t2.boxes(l).cpu().numpy())
        assert np.array_equal(t1.pyramid(l).cpu().numpy(), t2.pyramid(l).cpu().numpy())
    assert np.array_equal(t1.lists().cpu().numpy(), t2.lists().cpu().numpy()) and same_bits(t1.points().cpu().numpy(), t2.points().cpu().numpy())
    q1, q2 = ops.icp.point_tree_query(t1, src, stats=True), ops.icp.point_tree_query(t2, src, stats=True)
    for x, y in zip(q1, q2):
        assert same_bits(x.cpu().numpy(), y.cpu().numpy())
