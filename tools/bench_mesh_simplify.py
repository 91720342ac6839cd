#!/usr/bin/env python3
"""Time of mesh simplification (csrc/mesh_simplify.hip through ``utils.mesh_clean.simplify``) against a plain torch formulation of the
same clustering on the same device: cells by float64 arithmetic, clusters by ``unique`` on 64-bit cell keys (renumbered by their lowest
vertex index with ``scatter_reduce(amin)``), quadrics by ``index_add_`` (whose float atomics the kernels avoid), placement by batched
``linalg.eigh``, faces by ``unique`` on the sorted triples' keys.  Both are checked to give the same faces; the positions differ by
rounding (the torch sums have no fixed order) and the largest difference is reported.  Cases:

  (a) the shipped scene's (BASELINE config 2: tests/config2_case.py) marching-cubes mesh at 128^3 and 256^3 to 10 000 and 100 000 faces
      (the search included, on both sides)
  (b) one ``resolution=`` call without the search, on the 256^3 mesh
  (c) ``closest_point_mesh`` for 778 queries against the full 256^3 mesh and against its simplification to 10 000 faces
  (d) merge_vertices of the 128^3 mesh concatenated with a copy of itself

Per figure: host-clock ms around a call that ends synchronised, the median over --rounds rounds that time every candidate once each,
alternately, in one process, with the spread (max - min) between rounds.  Nothing is gated on these times.  Prints one JSON object;
--out also writes it.  ``--wnf LABEL`` instead prints one JSON line with the time of generate_obj_mesh_wnf at 128^3 with the defaults
in the tree the script lies in (profiles/mesh_simplify_wnf_parent.jsonl: this commit and its parent, alternately).

    python tools/bench_mesh_simplify.py [--rounds 5] [--out profiles/mesh_simplify_bench.json]
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

EIG_REL = 1e-3


def torch_clusters(verts, faces, R):
    """(cluster_of_vertex, K, centre [V,3], h): unique on cell keys, the groups renumbered by ascending lowest vertex index."""
    V = verts.shape[0]
    f = faces.long()
    ref = torch.zeros(V, dtype=torch.bool, device=verts.device)
    ref[f.reshape(-1)] = True
    p = verts.double()
    lo, hi = p[ref].amin(0), p[ref].amax(0)
    h = (hi - lo).max() / R
    cell = torch.floor((p - lo) / h).clamp_(0, R - 1).long()
    key = (cell[:, 0] * R + cell[:, 1]) * R + cell[:, 2]
    idx = torch.nonzero(ref)[:, 0]
    _, inverse = torch.unique(key[idx], return_inverse=True)
    G = int(inverse.max()) + 1
    rep = torch.full((G,), V, dtype=torch.long, device=verts.device).scatter_reduce(0, inverse, idx, "amin")
    rank = torch.empty(G, dtype=torch.long, device=verts.device)
    rank[torch.argsort(rep)] = torch.arange(G, device=verts.device)
    cov = torch.full((V,), -1, dtype=torch.long, device=verts.device)
    cov[idx] = rank[inverse]
    return cov, G, lo + (cell.double() + 0.5) * h, h


def torch_faces(faces, cov):
    ids = cov[faces.long()]
    at = torch.nonzero((ids[:, 0] != ids[:, 1]) & (ids[:, 1] != ids[:, 2]) & (ids[:, 0] != ids[:, 2]))[:, 0]
    ids = ids[at]
    s, _ = torch.sort(ids, dim=1)
    key = (s[:, 0] << 42) | (s[:, 1] << 21) | s[:, 2]
    uniq, inverse = torch.unique(key, return_inverse=True)
    first = torch.full((uniq.shape[0],), ids.shape[0], dtype=torch.long, device=faces.device).scatter_reduce(
        0, inverse, torch.arange(ids.shape[0], device=faces.device), "amin")
    return ids[torch.sort(first)[0]].int()


def torch_simplify(verts, faces, R):
    cov, K, centre, h = torch_clusters(verts, faces, R)
    out_faces = torch_faces(faces, cov)
    f = faces.long()
    p = verts.double()
    n = torch.linalg.cross(p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]])
    ids = cov[f]
    Q = torch.zeros((K, 4, 4), dtype=torch.float64, device=verts.device)
    for k in range(3):
        first = torch.ones(f.shape[0], dtype=torch.bool, device=verts.device)
        for j in range(k):
            first &= ids[:, j] != ids[:, k]
        q = p[f[:, k]] - centre[f[:, k]]
        plane = torch.cat([n, -(n * q).sum(1, keepdim=True)], 1)[first]
        Q.index_add_(0, ids[first, k], plane[:, :, None] * plane[:, None, :])
    member = cov >= 0
    s = torch.zeros((K, 3), dtype=torch.float64, device=verts.device).index_add_(0, cov[member], (p - centre)[member])
    x0 = s / torch.bincount(cov[member], minlength=K)[:, None].double()
    A, b = Q[:, :3, :3], Q[:, :3, 3]
    lam, vec = torch.linalg.eigh(A)
    g = -b - (A @ x0[:, :, None])[:, :, 0]
    inv = torch.where(lam > EIG_REL * lam.amax(1, keepdim=True), 1.0 / lam, torch.zeros_like(lam))
    x = x0 + (vec @ (inv * (vec.transpose(1, 2) @ g[:, :, None])[:, :, 0])[:, :, None])[:, :, 0]
    x = torch.where(((x.abs() <= 0.5 * h * (1 + 1e-9)).all(1))[:, None], x, x0)
    rep_centre = torch.zeros((K, 3), dtype=torch.float64, device=verts.device)
    rep_centre[cov[member]] = centre[member]
    return (rep_centre + x).to(verts.dtype), out_faces


def torch_search(verts, faces, nfaces, max_r=1 << 20):
    count = lambda r: torch_faces(faces, torch_clusters(verts, faces, r)[0]).shape[0]
    lo, hi = 1, 2
    while hi <= max_r and count(hi) <= nfaces:
        lo, hi = hi, 2 * hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if count(mid) <= nfaces:
            lo = mid
        else:
            hi = mid
    return torch_simplify(verts, faces, lo)


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def alternately(cands, rounds):
    """{name: (median ms, spread ms)} and the warm-up outputs: every candidate once per round, in turn."""
    out = {k: fn() for k, fn in cands.items()}
    times = {k: [] for k in cands}
    for _ in range(rounds):
        for k, fn in cands.items():
            times[k].append(timed(fn)[0])
    return {k: (round(statistics.median(v), 4), round(max(v) - min(v), 4)) for k, v in times.items()}, out


def simplify_case(name, mesh, rounds, **how):
    from vtaco_amd.utils import mesh_clean
    v, f = mesh.vertices, mesh.faces
    torch_fn = (lambda: torch_search(v, f, how["nfaces"])) if "nfaces" in how else (lambda: torch_simplify(v, f, how["resolution"]))
    t, out = alternately({"kernel": lambda: mesh_clean.simplify(mesh, **how), "torch": torch_fn}, rounds)
    _, rep = mesh_clean.simplify_report(mesh, **how)
    k, (tv, tf) = out["kernel"], out["torch"]
    same = tuple(k.faces.shape) == tuple(tf.shape) and torch.equal(k.faces, tf)
    case = {"case": name, "vertices": int(v.shape[0]), "faces": int(f.shape[0]), **how, "out_faces": int(k.faces.shape[0]),
            "out_vertices": int(k.vertices.shape[0]), "resolution_used": rep.resolution, "probes": rep.probes, "fallbacks": rep.fallbacks,
            "kernel_ms": t["kernel"][0], "kernel_spread_ms": t["kernel"][1], "torch_ms": t["torch"][0], "torch_spread_ms": t["torch"][1],
            "torch_over_kernel_time": round(t["torch"][0] / t["kernel"][0], 2), "faces_equal": bool(same),
            "max_position_difference": float((k.vertices.double() - tv.double()).abs().max()) if same else None}
    print(json.dumps(case), file=sys.stderr, flush=True)
    return case


def scene(dev):
    import config2_case as c2
    from vtaco_amd.conv_onet.models import ConvolutionalOccupancyNetwork
    z = c2.fixture()
    enc, dec = c2.models(z)
    return ConvolutionalOccupancyNetwork(dec, enc, device=dev).eval(), torch.from_numpy(z["cloud"]).float().to(dev)


def wnf_line(label, rounds):
    from vtaco_amd.conv_onet.generation import Generator3D
    dev = torch.device("cuda:0")
    model, cloud = scene(dev)
    gen = Generator3D(model, device=dev, resolution0=32)
    data = {"inputs": cloud}
    for _ in range(3):
        mesh = gen.generate_obj_mesh_wnf(data)
    times = [timed(lambda: gen.generate_obj_mesh_wnf(data))[0] for _ in range(max(rounds, 20))]
    print(json.dumps({"tree": label, "median_ms": round(statistics.median(times), 4), "min_ms": round(min(times), 4),
                      "max_ms": round(max(times), 4), "faces": int(mesh.faces.shape[0])}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cases", default="a,b,c,d")
    ap.add_argument("--out")
    ap.add_argument("--wnf", metavar="LABEL")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_mesh_simplify: no HIP device")
    if args.wnf:
        return wnf_line(args.wnf, args.rounds)
    from vtaco_amd import ops
    from vtaco_amd.conv_onet.generation import Generator3D, Mesh
    from vtaco_amd.utils import mesh_clean
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds,
              "method": "candidates alternately in one process; host clock around a call that ends synchronised; per figure the median over "
                        "rounds and the spread (max - min) between rounds", "cases": []}
    wanted = args.cases.split(",")
    model, cloud = scene(dev)
    meshes = {4 * r0: Generator3D(model, device=dev, resolution0=r0).generate_obj_mesh_wnf({"inputs": cloud}) for r0 in (32, 64)}
    torch.cuda.empty_cache()
    if "a" in wanted:
        for nx, mesh in meshes.items():
            for target in (10000, 100000):
                result["cases"].append(simplify_case(f"a: shipped scene at {nx}^3 to {target} faces", mesh, args.rounds, nfaces=target))
    if "b" in wanted:
        result["cases"].append(simplify_case("b: shipped scene at 256^3, resolution=64, no search", meshes[256], args.rounds, resolution=64))
    if "c" in wanted:
        full = meshes[256]
        small = full.simplify(nfaces=10000)
        lo, hi = full.vertices.amin(0), full.vertices.amax(0)
        rng = np.random.RandomState(0)
        q = lo + (hi - lo) * torch.from_numpy((0.4 + 0.2 * rng.rand(778, 3)).astype(np.float32)).to(dev)
        t, out = alternately({"full": lambda: ops.metrics.closest_point_mesh(full.vertices, full.faces, q),
                              "simplified": lambda: ops.metrics.closest_point_mesh(small.vertices, small.faces, q)}, args.rounds)
        d_full, d_small = out["full"].d2.sqrt(), out["simplified"].d2.sqrt()
        case = {"case": "c: closest_point_mesh, 778 queries, the 256^3 mesh against its simplification to 10 000 faces",
                "full_faces": int(full.faces.shape[0]), "simplified_faces": int(small.faces.shape[0]),
                "full_ms": t["full"][0], "full_spread_ms": t["full"][1], "simplified_ms": t["simplified"][0],
                "simplified_spread_ms": t["simplified"][1], "max_distance_difference": float((d_full - d_small).abs().max()),
                "box_diagonal": float((hi - lo).norm())}
        print(json.dumps(case), file=sys.stderr, flush=True)
        result["cases"].append(case)
    if "d" in wanted:
        m = meshes[128]
        V = m.vertices.shape[0]
        double = Mesh(torch.cat([m.vertices, m.vertices]), torch.cat([m.faces, m.faces + V]))

        def torch_weld():
            uniq, inverse = torch.unique(double.vertices, dim=0, return_inverse=True)
            return uniq, inverse[double.faces.long()]
        t, out = alternately({"kernel": lambda: mesh_clean.merge_vertices(double, unique_faces=True), "torch": torch_weld}, args.rounds)
        case = {"case": "d: merge_vertices of the 128^3 mesh doubled", "vertices": 2 * V, "faces": int(double.faces.shape[0]),
                "out_vertices": int(out["kernel"].vertices.shape[0]), "out_faces": int(out["kernel"].faces.shape[0]),
                "kernel_ms": t["kernel"][0], "kernel_spread_ms": t["kernel"][1], "torch_unique_rows_ms": t["torch"][0],
                "torch_spread_ms": t["torch"][1], "undone": bool(out["kernel"].vertices.shape[0] == V and torch.equal(out["kernel"].faces, m.faces)),
                "note": "the torch side is unique(dim=0) and the face gather only: sorted vertex order, no face dedup"}
        print(json.dumps(case), file=sys.stderr, flush=True)
        result["cases"].append(case)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
