#!/usr/bin/env python3
"""Time of the k nearest neighbours (csrc/knn.hip) three ways in one process: brute force (vt_knn_points), the walk of the point octree
(vt_point_tree_knn; its build timed too) and torch's ``cdist`` + ``topk`` (float64, in chunks of rows that keep the distance matrix
under 2 GB), with what is built on them.

  knn_<n>_k<k>      independent area-weighted surface samples of the 4 096-face torus, n = 2 048, 16 384, 100 000 points a side,
                    k = 1, 8, 16, 32; at k = 1 also ``ops.icp.nn_points`` both ways.  Equal bits of brute and tree are asserted; torch's
                    indices are compared and the share of equal ones recorded (its distances round differently)
  tactile_k<k>      the self-query of a cloud shaped like ``generate_tactile_pc``'s: five 320 x 240 image grids (384 000 points) on
                    gently curved patches, the fifth laid over a part of the first so that a fifth of its pixels are exact
                    duplicates.  Dense image grids and duplicated pixels are the tree's hard case: the leaves are full, every lane
                    scans its leaf serially and equal points cannot be split.  torch runs at k = 16 only, one round
  normals, outliers ``utils.pointcloud.estimate_normals(k=16)`` and ``statistical_outlier_mask(k=20)`` on that cloud, with either search

Per figure: host-clock ms around a call that ends synchronised, the median over --rounds rounds that time every candidate once each,
alternately, with the spread (max - min) between rounds.  Nothing is gated on these times.  Prints one JSON object; --out also writes
it.  ``--wnf LABEL`` instead prints one JSON line with the time of generate_obj_mesh_wnf at 128^3 with the defaults in the tree the
script lies in (profiles/knn_wnf_parent.jsonl: this commit and its parent, alternately).

    python tools/bench_knn.py [--rounds 5] [--out profiles/knn_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_point_tree import bits, put, race      # noqa: E402

KS = (1, 8, 16, 32)


def torch_knn(src, dst, k):
    """cdist + topk in float64, rows in chunks that keep the distance matrix under 2 GB."""
    rows = max(1, (1 << 28) // dst.shape[0])
    d, i = [], []
    for r0 in range(0, src.shape[0], rows):
        dd, ii = torch.cdist(src[r0:r0 + rows], dst).topk(k, dim=1, largest=False)
        d.append(dd)
        i.append(ii)
    return torch.cat(d), torch.cat(i)


def tactile_cloud(dev):
    """float64 [384000, 3]: five 320 x 240 grids on curved patches; a fifth of the last grid's pixels lie exactly on the first's."""
    v, u = torch.meshgrid(torch.arange(320, dtype=torch.float64, device=dev), torch.arange(240, dtype=torch.float64, device=dev), indexing="ij")
    u, v = u.reshape(-1) / 240.0, v.reshape(-1) / 320.0
    grids = []
    for t in range(5):
        z = 0.02 * torch.sin(6.0 * u + t) * torch.cos(5.0 * v - t)
        grids.append(torch.stack([0.06 * u + 0.07 * t, 0.08 * v, z], dim=1))
    grids[4][:76800 // 5] = grids[0][:76800 // 5]
    return torch.cat(grids).contiguous()


def knn_case(name, A, B, k, rounds, with_torch=True, torch_rounds=None):
    from vtaco_amd import ops
    tree = ops.icp.point_tree_build(B)
    case = {"case": name, "queries": int(A.shape[0]), "targets": int(B.shape[0]), "k": k, "depth": tree.depth, "leaves": tree.counts[tree.depth]}
    cands = {"brute": lambda: ops.knn.knn_points(A, B, k), "tree_build": lambda: ops.icp.point_tree_build(B),
             "tree_query": lambda: ops.knn.knn_points(A, B, k, method="tree", tree=tree),
             "tree_total": lambda: ops.knn.knn_points(A, B, k, method="tree")}
    if k == 1:
        cands["nn_points_brute"] = lambda: ops.icp.nn_points(A, B)
        cands["nn_points_tree_query"] = lambda: ops.icp.point_tree_query(tree, A)
    if with_torch and torch_rounds is None:
        cands["torch_cdist_topk"] = lambda: torch_knn(A, B, k)
    res, out = race(cands, rounds)
    put(case, res)
    if with_torch and torch_rounds is not None:
        r, o = race({"torch_cdist_topk": lambda: torch_knn(A, B, k)}, torch_rounds)
        put(case, r)
        case["torch_rounds"] = torch_rounds
        out.update(o)
    case["equal_bits"] = bits(out["brute"][0], out["tree_total"][0]) and bool(torch.equal(out["brute"][1], out["tree_total"][1]))
    assert case["equal_bits"], name
    if "torch_cdist_topk" in out:
        case["torch_equal_indices"] = round(float((out["torch_cdist_topk"][1] == out["brute"][1]).double().mean()), 6)
    st = ops.knn.knn_points(A, B, k, method="tree", tree=tree, stats=True)[2].double().mean(0)
    case["boxes_per_query"], case["points_per_query"] = round(float(st[0]), 1), round(float(st[1]), 1)
    case["brute_over_tree_query"] = round(case["brute_ms"] / case["tree_query_ms"], 2)
    case["brute_over_tree_total"] = round(case["brute_ms"] / case["tree_total_ms"], 2)
    print(json.dumps(case), file=sys.stderr, flush=True)
    return case


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cases", default="knn,tactile,normals,outliers")
    ap.add_argument("--out")
    ap.add_argument("--wnf", metavar="LABEL")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_knn: no HIP device")
    if args.wnf:
        from bench_mesh_simplify import wnf_line
        return wnf_line(args.wnf, args.rounds)
    import closest_point_ref as CP
    from vtaco_amd import eval as E
    from vtaco_amd.utils import pointcloud
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds,
              "method": "candidates alternately in one process; host clock around a call that ends synchronised; per figure the median over "
                        "rounds and the spread (max - min) between rounds", "cases": []}
    cases = args.cases.split(",")
    if "knn" in cases:
        tv, tf = CP.torus(64, 32, seed=5)
        tv, tf = torch.from_numpy(tv).to(dev), torch.from_numpy(tf).to(dev)
        for n in (2048, 16384, 100000):
            gen = torch.Generator(device=dev).manual_seed(n)
            A = E.sample_mesh_surface(tv, tf, n, gen)[0].double()
            B = E.sample_mesh_surface(tv, tf, n, gen)[0].double()
            for k in KS:
                result["cases"].append(knn_case(f"knn_{n}_k{k}", A, B, k, args.rounds))
    cloud = tactile_cloud(dev) if any(c in cases for c in ("tactile", "normals", "outliers")) else None
    if "tactile" in cases:
        for k in KS:
            result["cases"].append(knn_case(f"tactile_k{k}", cloud, cloud, k, args.rounds, with_torch=k == 16, torch_rounds=1))
    for what, fn in (("normals", lambda m: pointcloud.estimate_normals(cloud, k=16, method=m)),
                     ("outliers", lambda m: pointcloud.statistical_outlier_mask(cloud, k=20, method=m))):
        if what in cases:
            res, out = race({m: (lambda m=m: fn(m)) for m in ("brute", "tree")}, args.rounds)
            case = {"case": f"{what}_tactile", "points": int(cloud.shape[0])}
            put(case, res)
            a, b = out["brute"], out["tree"]
            case["equal_results"] = bool(torch.equal(a, b)) if torch.is_tensor(a) else all(bits(x, y) for x, y in zip(a, b))
            assert case["equal_results"], what
            if what == "outliers":
                case["kept"] = int(a.sum())
            case["brute_over_tree"] = round(case["brute_ms"] / case["tree_ms"], 2)
            result["cases"].append(case)
            print(json.dumps(case), file=sys.stderr, flush=True)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
