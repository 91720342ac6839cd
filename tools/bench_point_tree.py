#!/usr/bin/env python3
"""Time of the point octree (csrc/point_tree.hip, vt_icp_tree) against the brute-force neighbour search it equals bit for bit
(csrc/icp.hip: vt_nn_points, vt_icp), both through ``ops.icp`` in one process.  Clouds are area-weighted surface samples of a mesh and
of its moved copy (independent samples): the marching-cubes mesh of the shipped scene (129^3 lattice) and the 4 096-face torus.

  nn_<mesh>_<n>     ``nn_points`` at n = 2 048, 16 384, 100 000 points a side: brute, the tree's build, its query, both; the four walks
                    (VTACO_POINT_TREE_WALK) with the boxes and points tested per query
  icp_<n>           the loop at 2 048 and 100 000 (torus): vt_icp, vt_icp_tree with a fresh tree, and with a built one; equal iteration
                    counts and equal bits of T are asserted
  aligned           ``eval.mesh_distances_aligned(n = 100 000, distance='tree')`` of the scene mesh with both registrations
  chamfer           ``eval.chamfer_distance_kdtree`` at 100 000 x 30 000 against the same sums from two brute ``nn_points`` calls
  training          16 problems x 2 048 points: one batched call each way
  ab                queries handed to lanes in query order or in Morton order of the tree's leaves (the permutation's launches inside
                    the timed call), on a built tree and in the loop; equal bits asserted (--ab-out profiles/point_tree_ab.json)

Per figure: host-clock ms around a call that ends synchronised, the median over --rounds rounds that time every candidate once each,
alternately, with the spread (max - min) between rounds.  Nothing is gated on these times.  Prints one JSON object; --out also writes it.

    python tools/bench_point_tree.py [--rounds 5] [--out profiles/point_tree_bench.json]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

WALKS = ("plain", "seed", "order", "seed+order")
ENV = "VTACO_POINT_TREE_WALK"


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def race(cands, rounds):
    """{name: (median ms, spread ms)} and the warm-up outputs: every candidate once per round, alternately."""
    out = {k: fn() for k, fn in cands.items()}
    times = {k: [] for k in cands}
    for _ in range(rounds):
        for k, fn in cands.items():
            times[k].append(timed(fn)[0])
    return {k: (round(statistics.median(t), 4), round(max(t) - min(t), 4)) for k, t in times.items()}, out


def put(case, res):
    for k, (ms, spread) in res.items():
        case[k + "_ms"], case[k + "_spread_ms"] = ms, spread


def bits(a, b):
    return bool(torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64)))


def nn_case(name, A, B, rounds):
    from vtaco_amd import ops
    I = ops.icp
    os.environ.pop(ENV, None)
    tree = I.point_tree_build(B)
    counts = tree.counts if tree.single else tree.counts[0]
    case = {"case": name, "problems": 1 if A.dim() == 2 else int(A.shape[0]), "points": int(A.shape[-2]), "depth": tree.depth,
            "leaves": counts[tree.depth]}
    res, out = race({"brute": lambda: I.nn_points(A, B), "tree_build": lambda: I.point_tree_build(B),
                     "tree_query": lambda: I.point_tree_query(tree, A),
                     "tree_total": lambda: I.nn_points(A, B, method="tree")}, rounds)
    put(case, res)
    case["equal_bits"] = bits(out["brute"][0], out["tree_total"][0]) and bool(torch.equal(out["brute"][1], out["tree_total"][1]))
    assert case["equal_bits"], name
    case["brute_over_tree_query"] = round(case["brute_ms"] / case["tree_query_ms"], 2)
    case["brute_over_tree_total"] = round(case["brute_ms"] / case["tree_total_ms"], 2)

    def with_walk(w):                                                      # (the environment is read at every launch: set it per call)
        def run():
            os.environ[ENV] = w
            return I.point_tree_query(tree, A)
        return run
    res, _ = race({w: with_walk(w) for w in WALKS}, rounds)
    case["walks"] = {}
    for w in WALKS:
        os.environ[ENV] = w
        st = I.point_tree_query(tree, A, stats=True)[2].double().reshape(-1, 2).mean(0)
        case["walks"][w] = {"query_ms": res[w][0], "spread_ms": res[w][1], "boxes_per_query": round(float(st[0]), 1),
                            "points_per_query": round(float(st[1]), 1)}
    os.environ.pop(ENV, None)
    print(json.dumps(case), file=sys.stderr, flush=True)
    return case


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cases", default="nn_torus,nn_scene,icp,aligned,chamfer,training,ab")
    ap.add_argument("--max-iterations", type=int, default=20)
    ap.add_argument("--tolerance", type=float, default=1e-5)
    ap.add_argument("--out")
    ap.add_argument("--ab-out", help="where the 'ab' case writes its own JSON object (profiles/point_tree_ab.json)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_point_tree: no HIP device")
    import closest_point_ref as CP
    import icp_ref as R
    from vtaco_amd import eval as E, ops
    dev = torch.device("cuda:0")
    Tm = np.identity(4)
    Tm[:3, :3] = R.rodrigues(np.array([0.3, -1.0, 0.5]), 0.1)
    Tm[:3, 3] = 0.03 * np.array([2.0, -1.0, 2.0]) / 3.0

    def moved(v):
        return (v.double() @ torch.from_numpy(Tm[:3, :3].T).to(dev) + torch.from_numpy(Tm[:3, 3]).to(dev)).float().contiguous()

    def samples(mesh, n):
        gen = torch.Generator(device=dev).manual_seed(n)
        A = E.sample_mesh_surface(moved(mesh[0]), mesh[1], n, gen)[0].double()
        B = E.sample_mesh_surface(mesh[0], mesh[1], n, gen)[0].double()
        return A, B
    tv, tf = CP.torus(64, 32, seed=5)
    torus = (torch.from_numpy(tv).to(dev), torch.from_numpy(tf).to(dev))
    scene = None
    if any(c in args.cases for c in ("nn_scene", "aligned", "ab")):
        from bench_closest_point import scene_mesh
        scene = scene_mesh(dev)
    result = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "max_iterations": args.max_iterations,
              "tolerance": args.tolerance,
              "method": "candidates alternately in one process; host clock around a call that ends synchronised; per figure the median over "
                        "rounds and the spread (max - min) between rounds", "cases": []}
    cases = args.cases.split(",")
    for mesh_name, mesh in (("torus", torus), ("scene", scene)):
        if "nn_" + mesh_name in cases:
            for n in (2048, 16384, 100000):
                A, B = samples(mesh, n)
                result["cases"].append(nn_case(f"nn_{mesh_name}_{n}", A, B, args.rounds))
    if "icp" in cases:
        for n in (2048, 100000):
            A, B = samples(torus, n)
            kw = dict(max_iterations=args.max_iterations, tolerance=args.tolerance)
            tree = ops.icp.point_tree_build(B)
            res, out = race({"brute": lambda: ops.icp.icp(A, B, **kw), "tree": lambda: ops.icp.icp(A, B, method="tree", **kw),
                             "tree_reused": lambda: ops.icp.icp(A, B, method="tree", tree=tree, **kw)}, args.rounds)
            case = {"case": f"icp_{n}", "points": n, "iterations": int(out["brute"].iterations) + 1, "depth": tree.depth}
            put(case, res)
            for k in ("tree", "tree_reused"):
                assert int(out[k].iterations) == int(out["brute"].iterations) and bits(out[k].T, out["brute"].T), (n, k)
                assert bits(out[k].distances, out["brute"].distances) and torch.equal(out[k].idx, out["brute"].idx), (n, k)
            case["equal_iterations_and_bits"] = True
            case["brute_over_tree"] = round(case["brute_ms"] / case["tree_ms"], 2)
            result["cases"].append(case)
            print(json.dumps(case), file=sys.stderr, flush=True)
    if "aligned" in cases:
        v, f = scene
        n = 100000
        pv = moved(v)

        def run(registration):
            gen = torch.Generator(device=dev).manual_seed(1)
            return E.mesh_distances_aligned((pv, f), (v, f), n, gen, distance="tree", registration=registration)
        res, out = race({"registration_brute": lambda: run("brute"), "registration_tree": lambda: run("tree")}, args.rounds)
        case = {"case": "aligned", "samples_per_side": n, "faces": int(f.shape[0]), "icp_iterations": out["registration_tree"]["icp_iterations"] + 1}
        put(case, res)
        a, b = out["registration_brute"], out["registration_tree"]
        case["equal_results"] = all(np.array_equal(a[k], b[k]) if k == "transform" else a[k] == b[k] for k in a)
        assert case["equal_results"]
        case["brute_over_tree"] = round(case["registration_brute_ms"] / case["registration_tree_ms"], 2)
        result["cases"].append(case)
        print(json.dumps(case), file=sys.stderr, flush=True)
    if "chamfer" in cases:
        A, _ = samples(torus, 100000)
        _, B = samples(torus, 30000)
        p1, p2 = A.float()[None].contiguous(), B.float()[None].contiguous()

        def brute():
            d12, _ = ops.icp.nn_points(p1, p2)
            d21, _ = ops.icp.nn_points(p2, p1)
            return (torch.mean(d12, dim=1) + torch.mean(d21, dim=1)).float()
        res, out = race({"brute": brute, "kdtree": lambda: E.chamfer_distance_kdtree(p1, p2)}, args.rounds)
        case = {"case": "chamfer", "points1": 100000, "points2": 30000, "equal_value": bool(torch.equal(out["brute"], out["kdtree"])),
                "value": float(out["kdtree"][0])}
        assert case["equal_value"]
        put(case, res)
        case["brute_over_kdtree"] = round(case["brute_ms"] / case["kdtree_ms"], 2)
        result["cases"].append(case)
        print(json.dumps(case), file=sys.stderr, flush=True)
    if "ab" in cases:
        # which lane answers a query: query order, or Morton order of the tree's leaves (the permutation's launches are inside the
        # timed call).  Results are equal by construction and checked.
        ab = {"device": result["device"], "rounds": args.rounds, "method": result["method"],
              "candidate": "lanes = query | morton (ops.icp.point_tree_query(lanes=), ops.icp.icp(method='tree', lanes=))", "cases": []}
        for mesh_name, mesh, n in (("scene", scene, 100000), ("torus", torus, 100000), ("scene", scene, 16384), ("torus", torus, 2048)):
            A, B = samples(mesh, n)
            tree = ops.icp.point_tree_build(B)
            res, out = race({lanes: (lambda lanes=lanes: ops.icp.point_tree_query(tree, A, lanes=lanes)) for lanes in ("query", "morton")}, args.rounds)
            case = {"case": f"ab_query_{mesh_name}_{n}", "points": n, "depth": tree.depth}
            put(case, res)
            assert bits(out["query"][0], out["morton"][0]) and torch.equal(out["query"][1], out["morton"][1])
            case["equal_bits"] = True
            ab["cases"].append(case)
            print(json.dumps(case), file=sys.stderr, flush=True)
        for n in (2048, 100000):
            A, B = samples(torus, n)
            tree = ops.icp.point_tree_build(B)
            kw = dict(max_iterations=args.max_iterations, tolerance=args.tolerance, method="tree", tree=tree)
            res, out = race({lanes: (lambda lanes=lanes: ops.icp.icp(A, B, lanes=lanes, **kw)) for lanes in ("query", "morton")}, args.rounds)
            case = {"case": f"ab_loop_torus_{n}", "points": n, "iterations": int(out["query"].iterations) + 1}
            put(case, res)
            assert bits(out["query"].T, out["morton"].T) and int(out["query"].iterations) == int(out["morton"].iterations)
            case["equal_bits"] = True
            ab["cases"].append(case)
            print(json.dumps(case), file=sys.stderr, flush=True)
        if args.ab_out:
            with open(args.ab_out, "w") as fh:
                fh.write(json.dumps(ab) + "\n")
    if "training" in cases:
        A = torch.stack([samples(torus, 2048 + b)[0][:2048] for b in range(16)]).contiguous()
        B = torch.stack([samples(torus, 2048 + b)[1][:2048] for b in range(16)]).contiguous()
        result["cases"].append(nn_case("training_16x2048", A, B, args.rounds))
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
