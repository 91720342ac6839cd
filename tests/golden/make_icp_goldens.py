#!/usr/bin/env python3
"""Generate tests/golden/g28_icp.npz.

    python tests/golden/make_icp_goldens.py

From the REAL reference (needs it mounted read-only where make_goldens.py expects it, and scikit-learn for its kd-tree): src/utils/icp.py
is loaded through importlib and run unmodified.  Per loop case of tests/icp_ref.py (CASES, "pose" = "mid" with an initial pose, and three
N = 257 problems whose iteration counts differ from one another, found by walking a fixed list of angles and noise levels): the inputs,
the reference's T, distances and i; and from icp_ref.reference_order -- the same arithmetic with a brute-force neighbour search, checked
here against the reference's outputs -- the indices of every iteration, the smallest neighbour margin (second-nearest minus nearest
distance) and the smallest | |prev - mean| - tolerance | of any iteration.  Every case must keep both at or above icp_ref.MIN_MARGIN, which
makes the indices and i independent of float64 rounding; the generator refuses to write a fixture that does not.  "mirror": a cloud and
its reflection, best_fit_transform alone (the det R < 0 branch).
No reference code is stored: arrays and numbers only.
"""
import importlib.util
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_goldens as mg  # noqa: E402
import icp_ref as R  # noqa: E402


def _load_reference():
    spec = importlib.util.spec_from_file_location("ref_icp", os.path.join(mg.REF, "src", "utils", "icp.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run_case(ref, out, name, A, B, tolerance, max_iterations, init_pose=None):
    T, distances, i = ref.icp(A, B, init_pose=init_pose, max_iterations=max_iterations, tolerance=tolerance)
    trace = []
    T2, d2, i2, idx2 = R.reference_order.icp(A, B, init_pose, max_iterations, tolerance, trace=trace)
    assert i2 == i and len(trace) == i + 1, (name, i, i2)
    dT, dd = float(np.abs(T2 - T).max()), float(np.abs(d2 - distances).max())
    assert dT <= 1e-12 and dd <= 1e-12, (name, dT, dd)
    margin, gap = min(t[1] for t in trace), min(t[2] for t in trace)
    assert margin >= R.MIN_MARGIN and gap >= R.MIN_MARGIN, (name, margin, gap)
    assert A.shape[0] < 32768
    out.update({f"{name}.A": A, f"{name}.B": B, f"{name}.T": T, f"{name}.distances": distances, f"{name}.i": np.int64(i),
                f"{name}.idx": np.stack([t[0] for t in trace]).astype(np.int16), f"{name}.min_margin": np.float64(margin),
                f"{name}.min_gap": np.float64(gap), f"{name}.tolerance": np.float64(tolerance),
                f"{name}.max_iterations": np.int64(max_iterations)})
    if init_pose is not None:
        out[f"{name}.init_pose"] = init_pose
    print(f"{name}: N {A.shape[0]} i {i} min margin {margin:.2e} min gap {gap:.2e} |T - reference_order| {dT:.1e} |d - reference_order| {dd:.1e}")
    return i


def main():
    ref = _load_reference()
    out = {}
    for name, seed, N, angle, tr, noise, tol, iters in R.CASES:
        A, B = R.make_case(seed, N, angle, tr, noise)
        run_case(ref, out, name, A, B, tol, iters)
    assert int(out["cap.i"]) == 4
    # "mid" from a non-trivial initial pose: a rotation of 0.1 rad about (1, 2, 3) and a shift
    pose = np.identity(4)
    pose[:3, :3] = R.rodrigues(np.array([1.0, 2.0, 3.0]), 0.1)
    pose[:3, 3] = [0.02, -0.03, 0.01]
    name, seed, N, angle, tr, noise, tol, iters = R.CASES[1]
    A, B = R.make_case(seed, N, angle, tr, noise)
    run_case(ref, out, "pose", A, B, tol, iters, init_pose=pose)
    # three N = 257 problems with iteration counts that differ from one another
    found = {}
    seed = 10
    for angle in (0.1, 0.2, 0.3, 0.4, 0.5):
        for noise in (0.001, 0.002, 0.004):
            if len(found) == 3:
                break
            seed += 1
            A, B = R.make_case(seed, 257, angle, 0.05, noise)
            trial = {}
            try:
                i = run_case(ref, trial, f"batch{len(found)}", A, B, 1e-5, 20)
            except AssertionError:
                continue
            if i not in found and i < 19:
                found[i] = trial
                out.update(trial)
    assert len(found) == 3, sorted(found)
    assert len({int(out[f"{n}.i"]) for n in R.BATCH_CASES}) == 3
    # a cloud and its mirror image: best_fit_transform's reflection branch
    rng = np.random.default_rng(5)
    A = rng.random((65, 3)) - 0.5
    B = A * np.array([-1.0, 1.0, 1.0])
    T, Rm, t = ref.best_fit_transform(A, B)
    H = (A - A.mean(0)).T @ (B - B.mean(0))
    assert np.linalg.det(H) < 0 and np.linalg.det(Rm) > 0
    out.update({"mirror.A": A, "mirror.B": B, "mirror.T": T})
    path = os.path.join(HERE, "g28_icp.npz")
    np.savez(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
