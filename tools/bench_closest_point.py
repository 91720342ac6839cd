#!/usr/bin/env python3
"""Time of ``ops.metrics.closest_point_mesh`` (csrc/closest_point.hip) against a brute-force torch formulation of the same float64 region
algorithm on the same device (every (query, face) pair through torch ops, faces in chunks of --pairs pairs, running minimum), on

  hand_scene   778 queries (a hand's vertex count) against the marching-cubes mesh of the shipped scene (BASELINE config 2:
               tests/config2_case.py, 129^3 lattice = 128^3 cells, decode "f16x3"): few queries, many faces
  cloud_torus  100 000 queries against a 64 x 32 torus, 4 096 faces: many queries, few faces

Per case: host-clock ms around the call, which ends synchronised, as the median over --rounds rounds that time both candidates once each,
alternately, in one process, with the spread (max - min) between rounds; the largest |d2 difference| and the number of differing faces
between the two (regular faces: the torch form has no degenerate-face branch).  Nothing is gated on these times.  Prints one JSON
object; --out also writes it.

    python tools/bench_closest_point.py [--rounds 5] [--out profiles/closest_point_bench.json]
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


def scene_mesh(dev):
    import config2_case as c2
    from vtaco_amd import ops
    from vtaco_amd.conv_onet.generation import Generator3D
    from vtaco_amd.conv_onet.models import ConvolutionalOccupancyNetwork
    z = c2.fixture()
    enc, dec = c2.models(z)
    model = ConvolutionalOccupancyNetwork(dec, enc, device=dev).eval()
    n, box = 129, 1.1
    with torch.no_grad():
        c = model.encode_inputs(torch.from_numpy(z["cloud"]).float().to(dev))
        gen = Generator3D(model, device=dev, decode_precision="f16x3")
        vol = gen.eval_lattice(c, n).reshape(n, n, n)
        mesh = ops.marching_cubes(vol, 0.0, rescale=((n - 1) / 2, box / (n - 1)))
    return mesh[0].float().contiguous(), mesh[1].int().contiguous()


def _dot(u, w):
    return (u[..., 0] * w[..., 0] + u[..., 1] * w[..., 1]) + u[..., 2] * w[..., 2]


def torch_brute(verts, faces, pts, pairs):
    """(d2 [N] f64, face [N] i64): the kernel's region algorithm on every pair with torch ops, faces in chunks, first among equal minima."""
    v, p = verts.double(), pts.double()[:, None, :]
    f = faces.long()
    N, F = pts.shape[0], f.shape[0]
    chunk = max(1, int(pairs) // max(N, 1))
    best = torch.full((N,), float("inf"), dtype=torch.float64, device=pts.device)
    best_f = torch.full((N,), -1, dtype=torch.int64, device=pts.device)
    for f0 in range(0, F, chunk):
        fc = f[f0:f0 + chunk]
        a = v[fc[:, 0]][None]
        ab, ac = v[fc[:, 1]][None] - a, v[fc[:, 2]][None] - a
        d00, d01, d11 = _dot(ab, ab), _dot(ab, ac), _dot(ac, ac)
        ap = p - a
        d1, d2 = _dot(ab, ap), _dot(ac, ap)
        d3, d4, d5, d6 = d1 - d00, d2 - d01, d1 - d01, d2 - d11
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        e43, e56 = d4 - d3, d5 - d6
        zero, one = torch.zeros_like(d1), torch.ones_like(d1)
        nv, nw, den = vb, vc, (va + vb) + vc
        on_bc = (va <= 0) & (e43 >= 0) & (e56 >= 0)
        nv, nw, den = torch.where(on_bc, zero, nv), torch.where(on_bc, e43, nw), torch.where(on_bc, e43 + e56, den)
        for cond, nv_new, nw_new, den_new in (((vb <= 0) & (d2 >= 0) & (d6 <= 0), zero, d2, d2 - d6), ((d6 >= 0) & (d5 <= d6), zero, one, one),
                                              ((vc <= 0) & (d1 >= 0) & (d3 <= 0), d1, zero, d1 - d3), ((d3 >= 0) & (d4 <= d3), one, zero, one),
                                              ((d1 <= 0) & (d2 <= 0), zero, zero, one)):
            nv, nw, den = torch.where(cond, nv_new, nv), torch.where(cond, nw_new, nw), torch.where(cond, den_new, den)
            on_bc = on_bc & ~cond
        bad = ~(den > 0)
        nv, nw, den, on_bc = torch.where(bad, zero, nv), torch.where(bad, zero, nw), torch.where(bad, one, den), on_bc & ~bad
        w = nw / den
        vv = torch.where(on_bc, 1.0 - w, nv / den)
        q = (a + ab * vv[..., None]) + ac * w[..., None]
        d = p - q
        dist = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        m, j = dist.min(dim=1)
        take = m < best
        best, best_f = torch.where(take, m, best), torch.where(take, j + f0, best_f)
    return best, best_f


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--pairs", type=float, default=4e6, help="(query, face) pairs per chunk of the torch formulation")
    ap.add_argument("--cases", default="hand_scene,cloud_torus")
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_closest_point: no HIP device")
    import closest_point_ref as R
    from vtaco_amd import ops
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(0)
    cases = {}
    if "hand_scene" in args.cases:
        v, f = scene_mesh(dev)
        lo, hi = v.min(0).values.cpu().numpy(), v.max(0).values.cpu().numpy()
        # a hand-sized cloud (a fifth of the mesh's box) in the middle of the mesh's bounding box
        q = (lo + (hi - lo) * (0.4 + 0.2 * rng.rand(778, 3))).astype(np.float32)
        cases["hand_scene"] = (v, f, torch.from_numpy(q).to(dev))
    if "cloud_torus" in args.cases:
        tv, tf = R.torus(64, 32, seed=5)
        cases["cloud_torus"] = (torch.from_numpy(tv).to(dev), torch.from_numpy(tf).to(dev),
                                torch.from_numpy((1.2 * rng.rand(100000, 3) - 0.6).astype(np.float32)).to(dev))
    result = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "torch_pairs_per_chunk": args.pairs,
              "method": "candidates alternately in one process; host clock around a call that ends synchronised; per figure the median over "
                        "rounds and the spread (max - min) between rounds", "cases": []}
    for name, (v, f, q) in cases.items():
        cands = {"kernel": lambda: ops.metrics.closest_point_mesh(v, f, q, want_point=False)[:2],
                 "kernel_with_point": lambda: ops.metrics.closest_point_mesh(v, f, q)[:2],
                 "torch": lambda: torch_brute(v, f, q, args.pairs)}
        out = {k: fn() for k, fn in cands.items()}                             # warm-up: every shape once
        times = {k: [] for k in cands}
        for _ in range(args.rounds):
            for k, fn in cands.items():                                       # alternating: one round times every candidate once
                times[k].append(timed(fn)[0])
        case = {"case": name, "queries": int(q.shape[0]), "faces": int(f.shape[0]), "vertices": int(v.shape[0]),
                "pairs": int(q.shape[0]) * int(f.shape[0]), "slab_faces": ops.metrics.closest_point_slab_faces(f.shape[0], q.shape[0])}
        for k in cands:
            case[k + "_ms"] = round(statistics.median(times[k]), 4)
            case[k + "_spread_ms"] = round(max(times[k]) - min(times[k]), 4)
        case["kernel_gpairs_per_s"] = round(case["pairs"] / case["kernel_ms"] / 1e6, 2)
        case["torch_over_kernel_time"] = round(case["torch_ms"] / case["kernel_ms"], 2)
        case["max_abs_d2_difference"] = float((out["kernel"][0] - out["torch"][0]).abs().max())
        case["faces_differing"] = int((out["kernel"][1].long() != out["torch"][1]).sum())
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
