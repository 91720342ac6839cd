#!/usr/bin/env python3
"""Time of the fast winding number (``ops.winding``: csrc/winding_fast.hip, accuracy 2, order 2, default depth) against the exact sum
(``ops.winding_number``: csrc/winding.hip) in the same process and alternately, on

  torus     a 64 x 32 torus, 4 096 faces (tests/voxelize_ref.py), at the centres of a 64^3 and a 128^3 lattice
  scene     the marching-cubes mesh of the shipped scene as tools/bench_voxelize.py builds it (about 976 k faces), in its unit frame: at
            64^3, at 128^3 (2e12 pairs: the exact sum is skipped above --exact-max pairs and written as null) and for 778 queries, a
            hand's vertex count, drawn near the surface
  training  16 scenes x 2 048 points, each scene its own 576-face torus (24 x 12, rotated by its seed): the size of the meshes the
            trainer's tests label against; exact is the single vt_winding_number_scenes launch, fast one query per cached tree

Per case: the tree's build (host clock around ``ops.winding.build``, which contains its one host read and is synchronised after), the
query and the exact sum (device time between two events on the stream), as the median over --rounds rounds that time every candidate
once, with the spread (max - min); build + query; the labels (w > 0.5) on which fast and exact differ; the largest |fast - exact|; the
mean cells accepted and faces summed exactly per query.  ``query_skip_walk_ms`` is the same query with the walk that reads a
cell's eight child words at once and never visits an empty child (VTACO_WINDING_WALK=skip; equal results).  Prints one JSON object; --out also writes it.

    python tools/bench_winding.py [--rounds 5] [--out profiles/winding_fast_bench.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d D -o wf -- python tools/bench_winding.py --profile-run
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


def host_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def device_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def lattice(res, dev):
    c = (torch.arange(res, dtype=torch.float64, device=dev) + 0.5) / res - 0.5
    return torch.stack(torch.meshgrid(c, c, c, indexing="ij"), dim=-1).reshape(-1, 3).float().contiguous()


def unit_frame(v):
    lo, hi = v.double().min(0).values, v.double().max(0).values
    return ((v.double() - (lo + hi) / 2) / ((hi - lo).max() / 0.9)).float().contiguous()


def med(xs):
    return round(statistics.median(xs), 4), round(max(xs) - min(xs), 4)


def run_case(name, label, build, query, exact, rounds, faces, n_queries):
    """build() -> trees; query(trees) -> (w, stats); exact() -> w or None when skipped."""
    trees = build()                                                             # warm-up: every candidate once
    w, st = query(trees)
    we = exact() if exact else None
    t = {"build": [], "query": [], "skip": [], "exact": []}
    for _ in range(rounds):                                                     # alternating: one round times every candidate once
        ms, trees = host_ms(build)
        t["build"].append(ms)
        t["query"].append(device_ms(lambda: query(trees))[0])
        os.environ["VTACO_WINDING_WALK"] = "skip"                             # the walk that never visits an empty child
        t["skip"].append(device_ms(lambda: query(trees))[0])
        del os.environ["VTACO_WINDING_WALK"]
        if exact:
            t["exact"].append(device_ms(exact)[0])
    case = {"case": name, "queries": label, "faces": faces, "n_queries": n_queries}
    (case["build_ms"], case["build_spread_ms"]), (case["query_ms"], case["query_spread_ms"]) = med(t["build"]), med(t["query"])
    case["query_skip_walk_ms"], case["query_skip_walk_spread_ms"] = med(t["skip"])
    case["build_plus_query_ms"] = round(case["build_ms"] + case["query_ms"], 4)
    case["exact_ms"], case["exact_spread_ms"] = med(t["exact"]) if exact else (None, None)
    case["exact_over_query"] = round(case["exact_ms"] / case["query_ms"], 2) if exact else None
    case["exact_over_build_plus_query"] = round(case["exact_ms"] / case["build_plus_query_ms"], 2) if exact else None
    case["label_mismatches"] = int(((w > 0.5) != (we > 0.5)).sum()) if exact else None
    case["max_abs_difference"] = float((w.double() - we.double()).abs().max()) if exact else None
    case["inside"] = int((w > 0.5).sum())
    mean = st.reshape(-1, 2).double().mean(0)
    case["mean_cells_accepted"], case["mean_faces_exact"] = round(float(mean[0]), 2), round(float(mean[1]), 2)
    print(json.dumps(case), file=sys.stderr, flush=True)
    return case


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--exact-max", type=float, default=3e11, help="skip the exact sum above this many query x face pairs")
    ap.add_argument("--cases", default="torus,scene,training")
    ap.add_argument("--profile-run", action="store_true", help="one round of every case, for a kernel trace")
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_winding: no HIP device")
    if args.profile_run:
        args.rounds = 1
    import voxelize_ref as R
    from vtaco_amd import ops
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "exact_max_pairs": args.exact_max, "accuracy": 2.0, "order": 2,
              "method": "candidates alternately in one process after one warm-up of each; build: host clock around a call that is synchronised "
                        "after (it contains the build's host read); query and exact: device time between two stream events; per figure the "
                        "median over rounds and the spread (max - min) between rounds", "cases": []}

    def single(name, label, v, f, pts):
        depth = ops.winding.default_depth(f.shape[0])
        exact = (lambda: ops.winding_number(v, f, pts)) if float(pts.shape[0]) * f.shape[0] <= args.exact_max else None
        case = run_case(name, label, lambda: ops.winding.build(v, f), lambda t: ops.winding.query(t, pts, stats=True), exact, args.rounds,
                        int(f.shape[0]), int(pts.shape[0]))
        case["depth"] = depth
        tree = ops.winding.build(v, f)
        case["records_per_level"], case["tree_mib"] = tree.counts, round(tree.buf.numel() * 8 / 2 ** 20, 2)
        result["cases"].append(case)

    if "torus" in args.cases:
        v, f = R.torus(64, 32)
        v, f = torch.from_numpy(R.rotate(v, 5)).to(dev), torch.from_numpy(f.astype(np.int32)).to(dev)
        for res in (64, 128):
            single("torus", f"{res}^3 lattice", v, f, lattice(res, dev))
    if "scene" in args.cases:
        from bench_voxelize import scene_mesh
        v, f = scene_mesh(dev)
        v, f = unit_frame(v), f.to(torch.int32).contiguous()
        for res in (64, 128):
            single("scene", f"{res}^3 lattice", v, f, lattice(res, dev))
        g = torch.Generator(device="cpu").manual_seed(0)
        at = v[f[torch.randint(f.shape[0], (778,), generator=g).to(dev)].long()].mean(1)
        hand = (at + 0.02 * torch.randn(778, 3, generator=g).to(dev)).contiguous()
        single("scene", "778 points near the surface", v, f, hand)
    if "training" in args.cases:
        B, N = 16, 2048
        meshes = []
        for b in range(B):
            v, f = R.torus(24, 12)
            meshes.append((torch.from_numpy(R.rotate(v, b)).to(dev).contiguous(), torch.from_numpy(f.astype(np.int32)).to(dev).contiguous()))
        g = torch.Generator(device="cpu").manual_seed(1)
        pts = ((torch.rand(B, N, 3, generator=g) - 0.5) * 1.1).to(dev).contiguous()
        case = run_case("training", f"{B} scenes x {N} points, one {meshes[0][1].shape[0]}-face mesh each",
                        lambda: [ops.winding.build(v, f) for v, f in meshes], lambda ts: ops.winding.query_scenes(ts, pts, stats=True),
                        lambda: ops.winding_number_scenes(meshes, pts), args.rounds, int(meshes[0][1].shape[0]), B * N)
        case["depth"] = ops.winding.default_depth(meshes[0][1].shape[0])
        case["note"] = "build_ms is all 16 trees; the trainer builds a mesh's tree once and keeps it"
        result["cases"].append(case)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
