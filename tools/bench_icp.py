#!/usr/bin/env python3
"""Time of ``ops.icp.icp`` (csrc/icp.hip: the whole loop enqueued, no host synchronisation inside) against a torch formulation of the same
algorithm on the same device: per iteration ``torch.cdist`` (float64, queries in chunks of --pairs pairs) + ``argmin``, the fit through
``torch.linalg.svd``, the update, and one host check of the mean error -- the reference's loop (src/utils/icp.py:102-121) moved to device
tensors as it stands.  Cases: area-weighted surface samples of a 64 x 32 torus and of its copy moved by 0.1 rad and 0.03 (independent
samples, so the neighbour distances do not go to zero), at

  visualise   2 048 points a side (the visualise block's cloud size)
  surface     100 000 points a side (a mesh evaluation's sample count): 10^10 pairs per iteration

Per case: host-clock ms around the call, which ends synchronised, as the median over --rounds rounds that time both candidates once each,
alternately, in one process, with the spread (max - min) between rounds; the iterations both took and the largest |T difference|.  Nothing
is gated on these times.  Prints one JSON object; --out also writes it.

    python tools/bench_icp.py [--rounds 5] [--out profiles/icp_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def torch_fit(a, b):
    ca, cb = a.mean(0), b.mean(0)
    H = (a - ca).T @ (b - cb)
    U, S, Vt = torch.linalg.svd(H)
    R = Vt.T @ U.T
    if torch.linalg.det(R) < 0:
        Vt = Vt.clone()
        Vt[2] = -Vt[2]
        R = Vt.T @ U.T
    T = torch.eye(4, dtype=a.dtype, device=a.device)
    T[:3, :3] = R
    T[:3, 3] = cb - R @ ca
    return T


def torch_nn(src, dst, pairs):
    step = max(1, int(pairs) // dst.shape[0])
    dist, idx = [], []
    for n0 in range(0, src.shape[0], step):
        d, i = torch.cdist(src[n0:n0 + step], dst).min(dim=1)
        dist.append(d)
        idx.append(i)
    return torch.cat(dist), torch.cat(idx)


def torch_icp(A, B, max_iterations, tolerance, pairs):
    """(T, distances, i): icp.py:69-121 on device tensors, one host check per iteration."""
    src = A.clone()
    prev_error = 0.0
    for i in range(max_iterations):
        distances, idx = torch_nn(src, B, pairs)
        T = torch_fit(src, B[idx])
        src = src @ T[:3, :3].T + T[:3, 3]
        mean_error = float(distances.mean())
        if abs(prev_error - mean_error) < tolerance:
            break
        prev_error = mean_error
    return torch_fit(A, src), distances, i


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--pairs", type=float, default=2e8, help="(query, target) pairs per cdist chunk of the torch formulation")
    ap.add_argument("--cases", default="visualise,surface")
    ap.add_argument("--max-iterations", type=int, default=20)
    ap.add_argument("--tolerance", type=float, default=1e-5)
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_icp: no HIP device")
    import closest_point_ref as CP
    import icp_ref as R
    from vtaco_amd import eval as E, ops
    dev = torch.device("cuda:0")
    tv, tf = CP.torus(64, 32, seed=5)
    Tm = np.identity(4)
    Tm[:3, :3] = R.rodrigues(np.array([0.3, -1.0, 0.5]), 0.1)
    Tm[:3, 3] = 0.03 * np.array([2.0, -1.0, 2.0]) / 3.0
    pv = (tv.astype(np.float64) @ Tm[:3, :3].T + Tm[:3, 3]).astype(np.float32)
    gt = (torch.from_numpy(tv).to(dev), torch.from_numpy(tf).to(dev))
    pred = (torch.from_numpy(pv).to(dev), gt[1])
    sizes = {"visualise": 2048, "surface": 100000}
    result = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "torch_pairs_per_chunk": args.pairs,
              "max_iterations": args.max_iterations, "tolerance": args.tolerance,
              "method": "candidates alternately in one process; host clock around a call that ends synchronised; per figure the median over "
                        "rounds and the spread (max - min) between rounds", "cases": []}
    for name in args.cases.split(","):
        n = sizes[name]
        gen = torch.Generator(device=dev).manual_seed(n)
        A = E.sample_mesh_surface(pred[0], pred[1], n, gen)[0].double()
        B = E.sample_mesh_surface(gt[0], gt[1], n, gen)[0].double()
        cands = {"kernel": lambda: ops.icp.icp(A, B, max_iterations=args.max_iterations, tolerance=args.tolerance),
                 "torch": lambda: torch_icp(A, B, args.max_iterations, args.tolerance, args.pairs)}
        out = {k: fn() for k, fn in cands.items()}                             # warm-up: every shape once
        times = {k: [] for k in cands}
        for _ in range(args.rounds):
            for k, fn in cands.items():                                       # alternating: one round times every candidate once
                times[k].append(timed(fn)[0])
        its_k, its_t = int(out["kernel"].iterations), int(out["torch"][2])
        case = {"case": name, "points": n, "pairs_per_iteration": n * n, "slab_points": ops.icp.nn_slab_points(n, n),
                "kernel_iterations": its_k, "torch_iterations": its_t}
        for k in cands:
            case[k + "_ms"] = round(statistics.median(times[k]), 4)
            case[k + "_spread_ms"] = round(max(times[k]) - min(times[k]), 4)
        case["kernel_gpairs_per_s"] = round(case["pairs_per_iteration"] * (its_k + 1) / case["kernel_ms"] / 1e6, 2)
        case["torch_over_kernel_time"] = round(case["torch_ms"] / case["kernel_ms"], 2)
        case["max_abs_T_difference"] = float((out["kernel"].T - out["torch"][0]).abs().max())
        case["max_abs_distance_difference"] = float((out["kernel"].distances - out["torch"][1]).abs().max()) if its_k == its_t else None
        result["cases"].append(case)
        print(json.dumps(case), file=sys.stderr, flush=True)
        del out
        torch.cuda.empty_cache()
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
