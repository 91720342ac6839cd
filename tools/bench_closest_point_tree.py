#!/usr/bin/env python3
"""Time of the closest point through the face octree (csrc/closest_point_tree.hip: ``ops.metrics.closest_point_tree_build`` /
``closest_point_tree_query``) against the brute-force kernel (``ops.metrics.closest_point_mesh``, csrc/closest_point.hip) on the meshes of
tools/bench_closest_point.py:

  hand_scene      778 queries against the marching-cubes mesh of the shipped scene (129^3 lattice): few queries, many faces
  cloud_torus     100 000 queries against a 64 x 32 torus, 4 096 faces: many queries, few faces
  mesh_distances  ``eval.mesh_distances`` with 100 000 samples a side, the scene mesh against its translate
  sdf_scene_R     ``utils.voxels.signed_distance_field`` of the scene mesh at R^3 (32, 64, 128); brute force runs only below --brute-pairs
                  (query, face) pairs and is marked skipped, with the pair count, otherwise
  training        16 scenes x 778 points against 576-face meshes: ``closest_point_mesh_scenes`` against ``closest_point_tree_query_scenes``
  sweep           tori of 576 .. 262 144 faces x 778 and 100 000 queries: where the tree starts to win

Per candidate: host-clock ms around the call, which ends synchronised, as the median over --rounds rounds that time every candidate once
each, alternately, in one process, with the spread (max - min) between rounds.  The tree's build (the octree and the side buffer, with their
host reads) and its query are timed separately; ``tree_total`` is a call that does both.  Per query case also the mean boxes and faces
tested per query, and the query under each walk (VTACO_CLOSEST_TREE_WALK: plain, seed, order, seed+order).  Every tree result is compared
with the brute-force one for equal bits where that ran.  Nothing is gated on these times.  Prints one JSON object; --out also writes it.

    python tools/bench_closest_point_tree.py [--rounds 5] [--out profiles/closest_point_tree_bench.json]
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


def query_case(name, v, f, q, rounds, brute_pairs, depth=None):
    """One mesh, one query set: brute force, the tree's build, query and both, the statistics and the walks."""
    from vtaco_amd import ops
    M = ops.metrics
    pairs = int(q.shape[0]) * int(f.shape[0])
    case = {"case": name, "queries": int(q.shape[0]), "faces": int(f.shape[0]), "pairs": pairs}
    ct = M.closest_point_tree_build(v, f, depth)
    case["depth"], case["leaves"] = ct.tree.depth, ct.tree.counts[ct.tree.depth]
    os.environ.pop("VTACO_CLOSEST_TREE_WALK", None)
    cands = {"tree_build": lambda: M.closest_point_tree_build(v, f, depth),
             "tree_query": lambda: M.closest_point_tree_query(ct, q, want_point=False),
             "tree_query_with_point": lambda: M.closest_point_tree_query(ct, q),
             "tree_total": lambda: M.closest_point_tree_query(M.closest_point_tree_build(v, f, depth), q, want_point=False)}
    if pairs <= brute_pairs:
        cands["brute"] = lambda: M.closest_point_mesh(v, f, q, want_point=False)
    else:
        case["brute"] = f"skipped: {pairs:.3g} pairs"
    res, out = race(cands, rounds)
    put(case, res)
    if "brute" in cands:
        full = M.closest_point_mesh(v, f, q)
        tree = out["tree_query_with_point"]
        case["equal_bits"] = bool(torch.equal(full.d2.view(torch.int64), tree.d2.view(torch.int64)) and torch.equal(full.face, tree.face)
                                  and torch.equal(full.closest.view(torch.int64), tree.closest.view(torch.int64)))
        case["brute_over_tree_query"] = round(case["brute_ms"] / case["tree_query_ms"], 2)
        case["brute_over_tree_total"] = round(case["brute_ms"] / case["tree_total_ms"], 2)
    def with_walk(w):                                                      # (the environment is read at every launch: set it per call)
        def run():
            os.environ["VTACO_CLOSEST_TREE_WALK"] = w
            return M.closest_point_tree_query(ct, q, want_point=False)
        return run
    res, _ = race({w: with_walk(w) for w in WALKS}, rounds)
    case["walks"] = {}
    for w in WALKS:
        os.environ["VTACO_CLOSEST_TREE_WALK"] = w
        st = M.closest_point_tree_query(ct, q, want_point=False, stats=True)[1].double().mean(0)
        case["walks"][w] = {"query_ms": res[w][0], "spread_ms": res[w][1], "boxes_per_query": round(float(st[0]), 1),
                            "faces_per_query": round(float(st[1]), 1)}
    os.environ.pop("VTACO_CLOSEST_TREE_WALK", None)
    print(json.dumps(case), file=sys.stderr, flush=True)
    return case


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--brute-pairs", type=float, default=1e11, help="brute force runs only up to this many (query, face) pairs")
    ap.add_argument("--cases", default="hand_scene,cloud_torus,mesh_distances,sdf,training,sweep")
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_closest_point_tree: no HIP device")
    import closest_point_ref as R
    from vtaco_amd import eval as E
    from vtaco_amd import ops
    from vtaco_amd.utils import voxels
    M = ops.metrics
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(0)
    result = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "brute_pairs_limit": args.brute_pairs,
              "method": "candidates alternately in one process; host clock around a call that ends synchronised; per figure the median over "
                        "rounds and the spread (max - min) between rounds", "cases": []}
    scene = None
    if any(c in args.cases for c in ("hand_scene", "mesh_distances", "sdf")):
        from bench_closest_point import scene_mesh
        scene = scene_mesh(dev)
    if "hand_scene" in args.cases:
        v, f = scene
        lo, hi = v.min(0).values.cpu().numpy(), v.max(0).values.cpu().numpy()
        q = torch.from_numpy((lo + (hi - lo) * (0.4 + 0.2 * rng.rand(778, 3))).astype(np.float32)).to(dev)
        result["cases"].append(query_case("hand_scene", v, f, q, args.rounds, args.brute_pairs))
        result["cases"].append(query_case("hand_scene_depth7", v, f, q, args.rounds, args.brute_pairs, depth=7))
    if "cloud_torus" in args.cases:
        tv, tf = R.torus(64, 32, seed=5)
        q = torch.from_numpy((1.2 * rng.rand(100000, 3) - 0.6).astype(np.float32)).to(dev)
        result["cases"].append(query_case("cloud_torus", torch.from_numpy(tv).to(dev), torch.from_numpy(tf).to(dev), q, args.rounds, args.brute_pairs))
    if "mesh_distances" in args.cases:
        v, f = scene
        moved = (v + torch.tensor([0.004, -0.003, 0.002], device=dev)).contiguous()
        n = 100000
        case = {"case": "mesh_distances", "samples_per_side": n, "faces": int(f.shape[0]), "pairs": 2 * n * int(f.shape[0])}

        def run(distance):
            gen = torch.Generator(device=dev).manual_seed(1)
            return E.mesh_distances((moved, f), (v, f), n, gen, distance=distance)
        cands = {"tree": lambda: run("tree")}
        if case["pairs"] <= 4 * args.brute_pairs:                              # (2e11 pairs: about a second and a half; still worth a figure)
            cands["brute"] = lambda: run("brute")
        else:
            case["brute"] = f"skipped: {case['pairs']:.3g} pairs"
        res, out = race(cands, args.rounds)
        put(case, res)
        if "brute" in cands:
            case["equal_results"] = out["tree"] == out["brute"]
            case["brute_over_tree"] = round(case["brute_ms"] / case["tree_ms"], 2)
        case["chamfer_l1"] = out["tree"]["chamfer_l1"]
        result["cases"].append(case)
        print(json.dumps(case), file=sys.stderr, flush=True)
    if "sdf" in args.cases:
        v, f = scene
        for res_ in (32, 64, 128):
            pairs = res_ ** 3 * int(f.shape[0])
            case = {"case": f"sdf_scene_{res_}", "voxels": res_ ** 3, "faces": int(f.shape[0]), "pairs": pairs}
            cands = {"tree": lambda: voxels.signed_distance_field((v, f), res_)}
            if pairs <= args.brute_pairs:
                cands["brute"] = lambda: voxels.signed_distance_field((v, f), res_, distance="brute")
            else:
                case["brute"] = f"skipped: {pairs:.3g} pairs"
            res, out = race(cands, args.rounds)
            put(case, res)
            if "brute" in cands:
                case["equal_bits"] = bool(torch.equal(out["tree"].view(torch.int64), out["brute"].view(torch.int64)))
                case["brute_over_tree"] = round(case["brute_ms"] / case["tree_ms"], 2)
            case["inside_voxels"] = int((out["tree"] < 0).sum())
            result["cases"].append(case)
            print(json.dumps(case), file=sys.stderr, flush=True)
            del out
            torch.cuda.empty_cache()
    if "training" in args.cases:
        B, N = 16, 778
        meshes = []
        for b in range(B):
            tv, tf = R.torus(24, 12, seed=b)
            meshes.append((torch.from_numpy(tv).to(dev), torch.from_numpy(tf).to(dev)))
        q = torch.from_numpy((rng.rand(B, N, 3).astype(np.float32) - np.float32(0.5))).to(dev)
        cts = [M.closest_point_tree_build(v, f) for v, f in meshes]
        case = {"case": "training", "scenes": B, "queries": N, "faces": 576}
        res, out = race({"brute": lambda: M.closest_point_mesh_scenes(meshes, q, want_point=False),
                         "tree_query": lambda: M.closest_point_tree_query_scenes(cts, q, want_point=False),
                         "tree_build": lambda: [M.closest_point_tree_build(v, f) for v, f in meshes]}, args.rounds)
        put(case, res)
        case["equal_bits"] = bool(torch.equal(out["brute"].d2.view(torch.int64), out["tree_query"].d2.view(torch.int64)))
        case["brute_over_tree_query"] = round(case["brute_ms"] / case["tree_query_ms"], 2)
        result["cases"].append(case)
        print(json.dumps(case), file=sys.stderr, flush=True)
    if "sweep" in args.cases:
        sweep = []
        for nu, nv in ((24, 12), (64, 32), (128, 64), (256, 128), (512, 256)):
            tv, tf = R.torus(nu, nv, seed=5)
            v, f = torch.from_numpy(tv).to(dev), torch.from_numpy(tf).to(dev)
            for N in (778, 100000):
                q = torch.from_numpy((1.2 * rng.rand(N, 3) - 0.6).astype(np.float32)).to(dev)
                ct = M.closest_point_tree_build(v, f)
                res, out = race({"brute": lambda: M.closest_point_mesh(v, f, q, want_point=False),
                                 "tree_query": lambda: M.closest_point_tree_query(ct, q, want_point=False),
                                 "tree_build": lambda: M.closest_point_tree_build(v, f)}, args.rounds)
                row = {"faces": int(f.shape[0]), "queries": N, "depth": ct.tree.depth}
                put(row, res)
                row["equal_bits"] = bool(torch.equal(out["brute"].d2.view(torch.int64), out["tree_query"].d2.view(torch.int64))
                                         and torch.equal(out["brute"].face, out["tree_query"].face))
                sweep.append(row)
                print(json.dumps(row), file=sys.stderr, flush=True)
        result["cases"].append({"case": "sweep", "mesh": "torus(nu, nu / 2), queries uniform in [-0.6, 0.6]^3", "rows": sweep})
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
