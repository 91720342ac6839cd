"""CPU: tests/point_tree_ref.py (the numpy definition of csrc/point_tree.hip) against the brute-force definition, against scipy's kd-tree,
the pruning condition, and the two host-only entry points of the built library.

The restatement must return icp_ref.kernel_order.nn's d2 and idx bit for bit on every input the GPU tests use, for all four walks: the
skip rule lb > best has no slack term ("point_tree.hip", gives the argument), so one differing bit is a wrong rule."""
import ctypes

import numpy as np
import pytest

import icp_ref as R
import point_tree_ref as P


def same_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    return np.array_equal(got.view(np.uint8), want.view(np.uint8))


@pytest.fixture(scope="module")
def clouds():
    return P.clouds()


def check_all_walks(src, dst, T=None, depth=None):
    tree = P.build(dst, depth)
    w_d2, w_idx = P.brute(src, dst, T)
    for name, (seed, order) in P.WALKS.items():
        d2, idx, stats = P.query(tree, src, T, seed, order)
        assert np.array_equal(idx, w_idx), name
        assert same_bits(d2, w_d2), name
        assert (stats[:, 0] >= 1).all() and (stats[:, 1] <= 2 * len(dst)).all(), name
    return tree


@pytest.mark.parametrize("M", P.SIZES)
@pytest.mark.parametrize("N", P.SIZES)
def test_grid_of_sizes_equals_the_definition(clouds, N, M):
    src, dst = clouds[("src", N)], clouds[("dst", M)]
    check_all_walks(src, dst)
    check_all_walks(src, dst, P.pose_of(N * 10000 + M))


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_depths_equal_the_definition(clouds, depth):
    check_all_walks(clouds[("src", 257)], clouds[("dst", 1025)], depth=depth)


@pytest.mark.parametrize("name", sorted(P.special_cases()))
def test_special_cases_equal_the_definition(name):
    src, dst, depth = P.special_cases()[name]
    check_all_walks(src, dst, depth=depth)
    if name == "nonfinite_queries":
        d2, idx, _ = P.query(P.build(dst, depth), src)
        assert np.isposinf(d2[:6]).all() and (idx[:6] == -1).all() and np.isfinite(d2[6:]).all()
    if name == "lattice_twice":
        d2, idx, _ = P.query(P.build(dst, depth), src)
        assert (idx < 729).all() and not d2[:729].any()                # the first copy wins; lattice queries sit on their targets
    if name == "sparse_deep":
        assert P.build(dst, depth)["counts"][7] <= 65


def test_float32_inputs_and_the_batch_of_three(clouds):
    s32, d32 = clouds[("src", 257)].astype(np.float32), clouds[("dst", 600)].astype(np.float32)
    check_all_walks(s32.astype(np.float64), d32.astype(np.float64))
    src, dst, T = P.batch_of_three()
    for b in range(3):
        check_all_walks(src[b], dst[b], T[b])
    assert len({tuple(P.build(dst[b])["counts"]) for b in range(3)}) == 3


@pytest.mark.parametrize("name", R.LOOP_CASES + R.BATCH_CASES)
def test_loop_clouds_equal_the_definition(name):
    A, B, pose, _, _ = R.case_of(np.load(R.GOLDEN), name)
    check_all_walks(A, B, pose)


def test_chamfer_clouds_equal_the_definition():
    for p1, p2 in (P.chamfer_clouds(), P.chamfer_clouds_2048()):
        for b in range(2):
            a64, b64 = p1[b].astype(np.float64), p2[b].astype(np.float64)
            check_all_walks(a64, b64)
            check_all_walks(b64, a64)


def test_build_arrays_are_consistent(clouds):
    dst = clouds[("dst", 1025)]
    t = P.build(dst)
    assert t["depth"] == P.default_depth(1025) == 3
    assert sorted(t["lists"].tolist()) == list(range(1025)) and same_bits(t["points"], dst[t["lists"]])
    for a, b in zip(t["offsets"][:-1], t["offsets"][1:]):
        assert a < b and (np.diff(t["lists"][a:b]) > 0).all()             # ascending inside a leaf, no empty leaf
    assert np.array_equal(t["boxes"][0][0], np.concatenate([dst.min(0), dst.max(0)]))
    for l in range(t["depth"] + 1):
        assert (t["pyramids"][l] >= 0).sum() == t["counts"][l] == len(t["boxes"][l])


def test_indices_equal_scipys_kd_tree_where_the_margin_allows(clouds):
    from scipy.spatial import cKDTree
    cases = [(clouds[("src", n)], clouds[("dst", m)], None) for n in (65, 1025) for m in (64, 1025)]
    cases += [v for k, v in P.special_cases().items() if k not in ("nonfinite_queries",)]
    checked = 0
    for src, dst, depth in cases:
        d2, idx, _ = P.query(P.build(dst, depth), src)
        k = min(2, len(dst))
        dist, ind = cKDTree(dst).query(src, k=k)
        if k == 1:
            dist, ind = dist[:, None], ind[:, None]
            clear = np.ones(len(src), dtype=bool)
        else:
            clear = dist[:, 1] - dist[:, 0] > 1e-9
        assert np.array_equal(idx[clear], ind[clear, 0])
        checked += int(clear.sum())
    assert checked > 3000


@pytest.mark.parametrize("M", [1025, 4097])
def test_pruning_stays_inside_its_caps(M):
    """A condition that keeps pruning honest, not a measurement: uniform targets, default depth; the plain walk tests on average at most
    M / 8 points per query, the ordered walk at most M / 32, inside the cloud and far outside it.  (This definition: 54.2 / 47.1 plain and
    5.7 / 14.5 ordered at M = 1025; 73.8 / 76.9 and 4.0 / 11.1 at M = 4097.)"""
    inside, far, dst = P.pruning_case(M)
    tree = P.build(dst)
    for tag, src in (("inside", inside), ("far", far)):
        plain = P.query(tree, src, None, False, False)[2][:, 1].mean()
        ordered = P.query(tree, src, None, False, True)[2][:, 1].mean()
        both = P.query(tree, src, None, True, True)[2][:, 1].mean()
        print(f"points tested per query, M = {M}, {tag}: plain {plain:.1f}, order {ordered:.1f}, seed+order {both:.1f}")
        assert plain <= M / 8 and ordered <= M / 32 and both <= M / 32, (tag, plain, ordered, both)


def test_host_only_abi_agrees_with_the_definition():
    from vtaco_amd import _lib
    lib = _lib.load()
    for M in (1, 64, 65, 4096, 4097, 10 ** 6):
        assert lib.vt_point_tree_default_depth(M) == P.default_depth(M), M
    assert [P.default_depth(M) for M in (1, 64, 65, 4096, 4097, 10 ** 6)] == [1, 1, 2, 3, 4, 6]
    rng = np.random.default_rng(5)
    for M in (1, 64, 65, 4096, 4097, 10 ** 6):
        trees = [P.build(rng.random((M, 3)) - 0.5) for _ in range(2)]
        L = trees[0]["depth"]
        state = (ctypes.c_int32 * 32)()
        for b, t in enumerate(trees):
            for l in range(L + 1):
                state[16 * b + 1 + l] = t["counts"][l]
        off = (ctypes.c_size_t * 7)()
        assert lib.vt_point_tree_layout(M, L, 2, state, off) == 0
        caps = [max(t["counts"][l] for t in trees) for l in range(L + 1)]
        up = lambda x: (x + 255) // 256 * 256
        want = [256]
        want.append(want[-1] + up(4 * ((8 ** (L + 1) - 1) // 7)))
        want.append(want[-1] + up(48 * sum(caps)))
        want.append(want[-1] + up(4 * (caps[L] + 1)))
        want.append(want[-1] + up(4 * M))
        want.append(want[-1] + up(24 * M))
        assert list(off) == want + [2 * want[-1]], (M, list(off), want)
    state = (ctypes.c_int32 * 16)()
    off = (ctypes.c_size_t * 7)()
    assert lib.vt_point_tree_layout(65, 2, 1, state, off) != 0          # counts of zero: no tree has them
    assert lib.vt_point_tree_layout(65, 8, 1, state, off) != 0 and lib.vt_point_tree_layout(0, 2, 1, state, off) != 0
    assert lib.vt_point_tree_workspace_bytes(65, 1, 0) == 0 and lib.vt_point_tree_workspace_bytes(65, 1, 2) > 0
