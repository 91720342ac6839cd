#!/usr/bin/env python3
"""Multiresolution isosurface extraction (Generator3D extraction="mise") against the dense lattice at the same n, on the shipped
scene (BASELINE config 2: tests/config2_case.py), visual branch, decode_precision "f16x3", encode excluded:

  (r0, S) in (32,2) (64,2) (32,4) (64,3): n = r0 * 2^S + 1 = 129, 129, 513, 513

Per case: points decoded per level and in total (dense: n^3), device ms of the field (MISE: mise.extract -- refine passes, decodes,
scatters and its one count read per level; dense: Generator3D.eval_lattice at n) and of marching cubes at level 0 (ops.marching_cubes,
its own count read included), host reads per level, and the meshes' face counts.  Device ms: median over --reps of device events
around the call.  Also the f16x3 lattice-vs-point difference at odd n (eval_lattice against the point path on the same n^3 points).
With --kernel-stats <rocprofv3 kernel_stats.csv> (from a separate `rocprofv3 --kernel-trace --stats` run of this script), the rows
of the MISE kernels are added.  Prints one JSON object; --out also writes it.

    python tools/bench_mise.py [--reps 5] [--out profiles/mise_bench.json] [--kernel-stats <csv>]
"""
import argparse
import csv
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = ((32, 2), (64, 2), (32, 4), (64, 3))
BOX = 1.1


def device_ms(fn, reps):
    out, res = [], None
    for _ in range(reps):
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        res = fn()
        e.record()
        e.synchronize()
        out.append(s.elapsed_time(e))
    return statistics.median(out), res


def kernel_rows(path):
    rows = []
    with open(path) as fh:
        for r in csv.DictReader(fh):
            if "mise" in r.get("Name", "").lower():
                rows.append({k: r[k] for k in ("Name", "Calls", "TotalDurationNs", "AverageNs", "MinNs", "MaxNs") if k in r})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    ap.add_argument("--kernel-stats")
    args = ap.parse_args()
    import config2_case as c2
    from vtaco_amd import mise, ops
    from vtaco_amd.common import make_3d_grid
    from vtaco_amd.conv_onet.generation import Generator3D
    from vtaco_amd.conv_onet.models import ConvolutionalOccupancyNetwork
    dev = torch.device("cuda:0")
    z = c2.fixture()
    enc, dec = c2.models(z)
    model = ConvolutionalOccupancyNetwork(dec, enc, device=dev).eval()
    cloud = torch.from_numpy(z["cloud"]).float().to(dev)
    reads = [0]
    plain_read = mise._read_count

    def counted_read(count):
        reads[0] += 1
        return plain_read(count)
    mise._read_count = counted_read
    result = {"scene": "config 2 (tests/config2_case.py), visual branch", "decode_precision": "f16x3", "reps": args.reps,
              "device": torch.cuda.get_device_name(0), "cases": []}
    with torch.no_grad():
        c = model.encode_inputs(cloud)
        torch.cuda.synchronize()
        for r0, steps in CASES:
            gen = Generator3D(model, device=dev, resolution0=r0, upsampling_steps=steps, extraction="mise", decode_precision="f16x3")
            n = mise.size(r0, steps)
            evaluate = gen.mise_evaluator(c)
            mise.extract(evaluate, r0, steps, 0.0, BOX, dev)                 # warm-up (caches, capacity guess)
            reads[0] = 0
            t_mise, (values, known, per_level) = device_ms(lambda: mise.extract(evaluate, r0, steps, 0.0, BOX, dev), args.reps)
            mise_reads = reads[0] / args.reps
            rescale = ((n - 1) / 2, BOX / (n - 1))
            ops.marching_cubes(values, 0.0, rescale=rescale)
            t_mc_mise, m_mesh = device_ms(lambda: ops.marching_cubes(values, 0.0, rescale=rescale), args.reps)
            del values, known
            gen.eval_lattice(c, n)
            t_dense, dense = device_ms(lambda: gen.eval_lattice(c, n), args.reps)
            vol = dense.reshape(n, n, n)
            ops.marching_cubes(vol, 0.0, rescale=rescale)
            t_mc_dense, d_mesh = device_ms(lambda: ops.marching_cubes(vol, 0.0, rescale=rescale), args.reps)
            case = {"r0": r0, "steps": steps, "n": n,
                    "mise": {"points_per_level": per_level, "points": sum(per_level), "decode_ms": round(t_mise, 4),
                             "mc_ms": round(t_mc_mise, 4), "total_ms": round(t_mise + t_mc_mise, 4),
                             "host_reads_per_refinement_level": mise_reads / max(steps, 1) if steps else 0, "host_reads_mc": 1,
                             "faces": int(m_mesh[1].shape[0])},
                    "dense": {"points": n ** 3, "decode_ms": round(t_dense, 4), "mc_ms": round(t_mc_dense, 4),
                              "total_ms": round(t_dense + t_mc_dense, 4), "host_reads_mc": 1, "faces": int(d_mesh[1].shape[0])}}
            case["points_ratio"] = round(n ** 3 / sum(per_level), 2)
            case["speedup_decode_plus_mc"] = round((t_dense + t_mc_dense) / (t_mise + t_mc_mise), 2)
            if n <= 257:                       # f16x3: the lattice kernel against the point path on the same odd-n points
                pts = (BOX * make_3d_grid((-0.5,) * 3, (0.5,) * 3, (n,) * 3)).to(dev)
                point = evaluate(None, pts)
                diff = (point - dense).abs()
                case["f16x3_lattice_vs_point"] = {"bit_identical": bool(torch.equal(point.view(torch.int32), dense.view(torch.int32))),
                                                  "max_abs": float(diff.max()), "points_differing": int((diff > 0).sum())}
                del pts, point
            del dense, vol, m_mesh, d_mesh
            torch.cuda.empty_cache()
            result["cases"].append(case)
            print(json.dumps(case), flush=True)
        for n in (257,):
            pts = (BOX * make_3d_grid((-0.5,) * 3, (0.5,) * 3, (n,) * 3)).to(dev)
            gen = Generator3D(model, device=dev, extraction="mise", decode_precision="f16x3")
            point, lat = gen.mise_evaluator(c)(None, pts), gen.eval_lattice(c, n)
            diff = (point - lat).abs()
            result["f16x3_lattice_vs_point_257"] = {"bit_identical": bool(torch.equal(point.view(torch.int32), lat.view(torch.int32))),
                                                    "max_abs": float(diff.max()), "points_differing": int((diff > 0).sum())}
    if args.kernel_stats:
        result["kernel_stats"] = kernel_rows(args.kernel_stats)
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
