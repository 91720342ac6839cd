#!/usr/bin/env python3
"""Time of the mesh-topology kernels (csrc/mesh_topo.hip through ``utils.mesh_clean.components``: labels, table, per-component
measures, edge statistics) against a plain torch formulation of the same results on the same device: labels by repeated
``scatter_reduce(amin)`` over the directed edges plus a gather (pointer jumping) to a fixed point, one host check per round; edges by
``sort`` / ``unique_consecutive`` of 64-bit keys; sums by ``index_add_`` (whose float atomics the kernels avoid).  Cases:

  (a) the shipped scene's (BASELINE config 2: tests/config2_case.py) marching-cubes mesh at 128^3 and 256^3
  (b) a synthetic mesh of 2 000 small closed components (tetrahedra), face order shuffled
  (c) generate_obj_mesh_wnf at 128^3 with components='all' against 'largest', alternately

Per figure: host-clock ms around a call that ends synchronised, the median over --rounds rounds that time every candidate once each,
alternately, in one process, with the spread (max - min) between rounds.  Also the hooking rounds each mesh needed (kernel and torch).
Nothing is gated on these times.  Prints one JSON object; --out also writes it.

    python tools/bench_mesh_topo.py [--rounds 5] [--out profiles/mesh_topo_bench.json]
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


def torch_labels(faces, V):
    """(labels, rounds): min-label propagation over the edges and pointer jumping until a round changes nothing."""
    f = faces.long()
    src = torch.cat([f[:, 0], f[:, 1], f[:, 1], f[:, 2]])
    dst = torch.cat([f[:, 1], f[:, 0], f[:, 2], f[:, 1]])
    labels = torch.arange(V, device=faces.device)
    rounds = 0
    while True:
        rounds += 1
        new = labels.scatter_reduce(0, dst, labels[src], "amin", include_self=True)
        new = new[new]
        if bool((new == labels).all()):
            return labels, rounds
        labels = new


def torch_topo(verts, faces):
    """The results of utils.mesh_clean.components in torch ops (labels, ranks, counts, bbox, area, volume, edge statistics)."""
    V = verts.shape[0]
    labels, rounds = torch_labels(faces, V)
    f = faces.long()
    ref = torch.zeros(V, dtype=torch.bool, device=verts.device)
    ref[f.reshape(-1)] = True
    is_root = ref & (labels == torch.arange(V, device=verts.device))
    rank = torch.cumsum(is_root, 0) - 1
    C = int(is_root.sum())
    cov = torch.where(ref, rank[labels], -1)
    cof = cov[f[:, 0]]
    n_faces = torch.bincount(cof, minlength=C)
    n_vertices = torch.bincount(cov[ref], minlength=C)
    p = verts.double()
    p0, p1, p2 = p[f[:, 0]], p[f[:, 1]], p[f[:, 2]]
    area = torch.zeros(C, dtype=torch.float64, device=verts.device).index_add_(0, cof, 0.5 * torch.linalg.cross(p1 - p0, p2 - p0).norm(dim=1))
    volume = torch.zeros(C, dtype=torch.float64, device=verts.device).index_add_(0, cof, (p0 * torch.linalg.cross(p1, p2)).sum(1) / 6.0)
    idx = cov[ref][:, None].expand(-1, 3)
    lo = torch.full((C, 3), float("inf"), dtype=verts.dtype, device=verts.device).scatter_reduce(0, idx, verts[ref], "amin")
    hi = torch.full((C, 3), float("-inf"), dtype=verts.dtype, device=verts.device).scatter_reduce(0, idx, verts[ref], "amax")
    a = torch.cat([f[:, 0], f[:, 1], f[:, 2]])
    b = torch.cat([f[:, 1], f[:, 2], f[:, 0]])
    keep = a != b
    a, b = a[keep], b[keep]
    key = (torch.minimum(a, b) << 32) | torch.maximum(a, b)
    key, order = torch.sort(key)
    fwd = (a < b)[order].long()
    uniq, inverse, counts = torch.unique_consecutive(key, return_inverse=True, return_counts=True)
    n_fwd = torch.zeros_like(counts).index_add_(0, inverse, fwd)
    ec = cov[uniq >> 32]
    n_edges = torch.bincount(ec, minlength=C)
    n_boundary = torch.bincount(ec[counts == 1], minlength=C)
    n_nonmanifold = torch.bincount(ec[counts >= 3], minlength=C)
    n_misoriented = torch.bincount(ec[(counts == 2) & (n_fwd != 1)], minlength=C)
    return dict(labels=labels, rounds=rounds, n_components=C, comp_of_vertex=cov, comp_of_face=cof, n_faces=n_faces, n_vertices=n_vertices,
                area=area, volume=volume, bbox=torch.stack([lo, hi], 1), n_edges=n_edges, n_boundary=n_boundary, n_nonmanifold=n_nonmanifold,
                n_misoriented=n_misoriented)


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


def topo_case(name, verts, faces, rounds):
    from vtaco_amd.utils import mesh_clean
    t, out = alternately({"kernel": lambda: mesh_clean.components((verts, faces)), "torch": lambda: torch_topo(verts, faces)}, rounds)
    k, r = out["kernel"], out["torch"]
    same = all(torch.equal(getattr(k, n).long(), r[n].long()) for n in ("labels", "comp_of_vertex", "comp_of_face", "n_faces", "n_vertices",
                                                                         "n_edges", "n_boundary", "n_nonmanifold", "n_misoriented"))
    case = {"case": name, "vertices": int(verts.shape[0]), "faces": int(faces.shape[0]), "components": k.n_components,
            "kernel_ms": t["kernel"][0], "kernel_spread_ms": t["kernel"][1], "torch_ms": t["torch"][0], "torch_spread_ms": t["torch"][1],
            "torch_over_kernel_time": round(t["torch"][0] / t["kernel"][0], 2), "kernel_hook_rounds": k.rounds, "torch_rounds": r["rounds"],
            "integer_results_equal": bool(same and k.n_components == r["n_components"]),
            "max_rel_area_difference": float(((k.area - r["area"]).abs() / r["area"].abs().clamp_min(1e-300)).max()),
            "watertight_components": int(k.watertight.sum()), "largest_component_faces": int(k.n_faces.max())}
    print(json.dumps(case), file=sys.stderr, flush=True)
    return case


def tetrahedra(n, seed=0):
    import mesh_topo_ref as R
    rng = np.random.RandomState(seed)
    v0, f0 = R.tetrahedron()
    v = np.concatenate([0.01 * v0 + rng.rand(1, 3).astype(np.float32) for _ in range(n)])
    f = np.concatenate([f0 + 4 * k for k in range(n)])
    return v.astype(np.float32), f[rng.permutation(f.shape[0])].astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cases", default="a,b,c")
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_mesh_topo: no HIP device")
    import config2_case as c2
    from vtaco_amd.conv_onet.generation import Generator3D
    from vtaco_amd.conv_onet.models import ConvolutionalOccupancyNetwork
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds,
              "method": "candidates alternately in one process; host clock around a call that ends synchronised; per figure the median over "
                        "rounds and the spread (max - min) between rounds", "cases": []}
    wanted = args.cases.split(",")
    if "a" in wanted or "c" in wanted:
        z = c2.fixture()
        enc, dec = c2.models(z)
        model = ConvolutionalOccupancyNetwork(dec, enc, device=dev).eval()
        cloud = torch.from_numpy(z["cloud"]).float().to(dev)
    if "a" in wanted:
        for r0 in (32, 64):
            mesh = Generator3D(model, device=dev, resolution0=r0).generate_obj_mesh_wnf({"inputs": cloud})
            result["cases"].append(topo_case(f"a: shipped scene, marching cubes at {4 * r0}^3", mesh.vertices, mesh.faces, args.rounds))
            torch.cuda.empty_cache()
    if "b" in wanted:
        v, f = tetrahedra(2000)
        result["cases"].append(topo_case("b: 2000 tetrahedra, faces shuffled", torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev), args.rounds))
    if "c" in wanted:
        gens = {name: Generator3D(model, device=dev, resolution0=32, components=name) for name in ("all", "largest")}
        data = {"inputs": cloud}
        for g in gens.values():                                                  # every shape twice: the second call captures the scene graph
            g.generate_obj_mesh_wnf(data)
            g.generate_obj_mesh_wnf(data)
        t, out = alternately({k: (lambda g=g: g.generate_obj_mesh_wnf(data)) for k, g in gens.items()}, args.rounds)
        case = {"case": "c: generate_obj_mesh_wnf at 128^3, components='all' against 'largest'",
                "all_ms": t["all"][0], "all_spread_ms": t["all"][1], "largest_ms": t["largest"][0], "largest_spread_ms": t["largest"][1],
                "all_faces": int(out["all"].faces.shape[0]), "largest_faces": int(out["largest"].faces.shape[0]),
                "components": out["all"].components().n_components}
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
