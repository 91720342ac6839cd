"""CPU: tests/icp_ref.py against the reference's recorded results (tests/golden/g28_icp.npz, from the real src/utils/icp.py), the fixture's
margin conditions, and the refusals of ``vtaco_amd.utils.icp`` / ``ops.icp`` that need no device.

reference_order and kernel_order both run every fixture case: ``i`` and the indices of the last iteration must EQUAL the reference's (the
fixture's margins make them independent of float64 rounding); T and the distances must lie within the derived bound -- not equal bits,
because LAPACK builds differ between machines.

The bound (icp_ref.fit_bound, from the fixture's points alone): with identical correspondences one fit's rotation error is at most
2 |dH|_F / (sigma_2 + s sigma_3), s = sign det H (the reflection case is governed by sigma_2 - sigma_3), with
|dH|_F <= N 2^-53 sum |a_i - abar| |b_i - bbar|.  The gate on T is that bound times (executed iterations + 1) times 8 -- the project's
usual factor over a rounding estimate; it covers the Jacobi solve and the point updates -- and the gate on the distances is the gate on T
times (1 + max |p|).  Every comparison prints ``RATIO <tag>: error / gate``; with VTACO_RATIO_LOG naming a file the lines are appended
to it (profiles/icp_f64_ratios.txt was written that way)."""
import os

import numpy as np
import pytest
import torch

import icp_ref as R

GOLDEN = R.GOLDEN
ALL_CASES = R.LOOP_CASES + R.BATCH_CASES


@pytest.fixture(scope="module")
def g28():
    return np.load(GOLDEN)


@pytest.mark.parametrize("form", ["reference_order", "kernel_order"])
@pytest.mark.parametrize("name", ALL_CASES)
def test_both_forms_reproduce_the_reference(g28, name, form):
    A, B, pose, iters, tol = R.case_of(g28, name)
    T, distances, i, idx = getattr(R, form).icp(A, B, pose, iters, tol)
    R.check_loop_against_fixture(g28, name, f"cpu {form}", T, distances, i, idx)


@pytest.mark.parametrize("form", ["reference_order", "kernel_order"])
def test_mirrored_cloud_takes_the_reflection_branch(g28, form):
    A, B = g28["mirror.A"], g28["mirror.B"]
    H = (A - A.mean(0)).T @ (B - B.mean(0))
    assert np.linalg.det(H) < 0
    T = getattr(R, form).fit(A, B)
    assert np.linalg.det(T[:3, :3]) > 0
    assert R.ratio(f"cpu {form} mirror T", float(np.abs(T - g28["mirror.T"]).max()), 8.0 * R.fit_bound(A, B)) <= 1.0


def test_fixture_margins_and_iteration_counts(g28):
    """The conditions that make indices and i independent of rounding, recomputed here from the inputs (not read from the fixture alone)."""
    for name in ALL_CASES:
        A, B, pose, iters, tol = R.case_of(g28, name)
        trace = []
        _, _, i, _ = R.reference_order.icp(A, B, pose, iters, tol, trace=trace)
        assert i == int(g28[name + ".i"]) and len(trace) == i + 1
        assert np.array_equal(np.stack([t[0] for t in trace]), g28[name + ".idx"].astype(np.int64)), name
        margin, gap = min(t[1] for t in trace), min(t[2] for t in trace)
        assert margin >= R.MIN_MARGIN and gap >= R.MIN_MARGIN, (name, margin, gap)
        assert float(g28[name + ".min_margin"]) >= R.MIN_MARGIN and float(g28[name + ".min_gap"]) >= R.MIN_MARGIN, name
    assert int(g28["cap.i"]) == int(g28["cap.max_iterations"]) - 1 == 4
    assert len({int(g28[n + ".i"]) for n in R.BATCH_CASES}) == 3
    for (name, seed, N, angle, tr, noise, tol, iters) in R.CASES:          # the inputs are the issue's recipe
        A, B = R.make_case(seed, N, angle, tr, noise)
        assert np.array_equal(A, g28[name + ".A"]) and np.array_equal(B, g28[name + ".B"]), name


def test_kernel_order_pieces():
    """Ties go to the lowest index; H == 0 gives R = I; rank-deficient H still gives a proper rotation."""
    dst = np.array([[1.0, 0, 0], [0, 1.0, 0], [1.0, 0, 0], [0, 1.0, 0]])
    d2, idx = R.kernel_order.nn(np.array([[1.0, 0, 0], [0, 1.0, 0], [0.5, 0.5, 0]]), dst)
    assert idx.tolist() == [0, 1, 0] and d2.tolist() == [0.0, 0.0, 0.5]
    one = R.kernel_order.fit(np.array([[0.3, -0.2, 0.1]]), np.array([[1.0, 2.0, 3.0]]))
    assert np.array_equal(one[:3, :3], np.identity(3)) and np.array_equal(one[:3, 3], np.array([1.0, 2.0, 3.0]) - np.array([0.3, -0.2, 0.1]))
    same = R.kernel_order.fit(np.full((257, 3), 0.25), np.full((257, 3), -0.5))            # dyadic: the centroids are exact, H == 0
    assert np.array_equal(same[:3, :3], np.identity(3)) and np.array_equal(same[:3, 3], np.full(3, -0.75))
    rng = np.random.default_rng(7)
    for a, b in ((rng.random((2, 3)), rng.random((2, 3))),                                  # rank 1
                 (np.c_[rng.random((40, 2)), np.zeros(40)], np.c_[rng.random((40, 2)), np.zeros(40)])):   # planar: rank 2
        Rm = R.kernel_order.fit(a, b)[:3, :3]
        tol = 128 * 2.0 ** -53                                                        # tests/test_icp_gpu.py, check_rotation
        assert np.abs(Rm @ Rm.T - np.identity(3)).max() <= tol and abs(np.linalg.det(Rm) - 1.0) <= tol


def test_api_refusals_need_no_device():
    from vtaco_amd import ops
    from vtaco_amd._lib import VtError
    from vtaco_amd.utils import icp as U
    a, b = torch.zeros(5, 3, dtype=torch.float64), torch.zeros(5, 3, dtype=torch.float64)
    for call in (lambda: ops.icp.nn_points(a, b), lambda: ops.icp.icp_fit(a, b), lambda: ops.icp.icp(a, b),
                 lambda: U.nearest_neighbor(a, b), lambda: U.best_fit_transform(a, b), lambda: U.icp(a, b)):
        with pytest.raises(VtError, match="HIP device"):
            call()
    with pytest.raises(VtError, match="tensors"):
        ops.icp.icp(np.zeros((5, 3)), np.zeros((5, 3)))
    # the remaining checks come after the device check in ops.icp: shapes and dimensions are refused by utils.icp before any transfer
    for m in (2, 4):
        for call in (U.nearest_neighbor, U.best_fit_transform, U.icp):
            with pytest.raises(VtError, match="3-D"):
                call(np.zeros((5, m)), np.zeros((5, m)))
    with pytest.raises(VtError, match=r"\[N,3\]"):
        U.icp(np.zeros(3), np.zeros(3))
    with pytest.raises(VtError, match="one shape"):
        U.best_fit_transform(torch.zeros(5, 3), torch.zeros(6, 3))


def test_ops_icp_is_a_submodule_only():
    from vtaco_amd import ops
    assert ops.icp.icp.__module__ == "vtaco_amd.ops.icp"
    for name in ("nn_points", "icp_fit", "IcpResult", "nn_slab_points"):
        assert hasattr(ops.icp, name) and not hasattr(ops, name), name
