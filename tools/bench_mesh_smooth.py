#!/usr/bin/env python3
"""Time of the adjacency and smoothing kernels (csrc/mesh_smooth.hip through ``ops.mesh.vertex_adjacency`` and ``ops.mesh.smooth``)
against a plain torch formulation on the same device: the directed edges by ``unique`` over 64-bit keys, the row sums by ``index_add_``
in float64.  ``index_add_`` adds with float atomics in no fixed order, so the two are compared to a tolerance and the largest difference
is reported, not asserted equal; the kernel path is run twice and its two results are asserted equal bit for bit.  Cases:

  (a) the shipped scene's (BASELINE config 2: tests/config2_case.py) marching-cubes mesh at 128^3 and 256^3
  (b) the 4 096-face torus (tests/mesh_topo_ref.py: torus(32, 64))
  (c) the 778-vertex hand (the synthetic MANO asset's template and faces)
  (d) generate_obj_mesh_wnf at 128^3 with smooth=None against 'taubin', alternately

Per mesh: the adjacency build alone, 10 taubin pairs alone, 10 humphrey iterations alone (both on a ready adjacency) and the whole
``Mesh.smooth`` call (adjacency + 10 taubin pairs).  For one gather pass the time is taken as (40 passes - 20 passes) / 20, which leaves
out the two conversion launches, and set against the pass's algorithmic bytes -- rows (offsets and neighbours), the neighbours' float64
positions and one float64 write.

Per figure: host-clock ms around a call that ends synchronised, the median over --rounds rounds that time every candidate once each,
alternately, in one process, with the spread (max - min) between rounds.  Nothing is gated on these times.  Prints one JSON object;
--out also writes it.  ``--wnf LABEL`` instead prints one JSON line with the time of generate_obj_mesh_wnf at 128^3 with the defaults
in the tree the script lies in (profiles/mesh_smooth_wnf_parent.jsonl: this commit and its parent, alternately).

    python tools/bench_mesh_smooth.py [--rounds 5] [--out profiles/mesh_smooth_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def torch_adjacency(faces, V):
    """(row, col int64 [nnz], degree float64 [V], boundary_vertex bool [V]): the directed edges, each undirected edge once per direction."""
    f = faces.long()
    a, b = f.reshape(-1), f[:, [1, 2, 0]].reshape(-1)
    live = a != b
    key, counts = torch.unique((torch.minimum(a, b)[live] << 32) | torch.maximum(a, b)[live], return_counts=True)
    lo, hi = key >> 32, key & 0xffffffff
    row, col = torch.cat([lo, hi]), torch.cat([hi, lo])
    deg = torch.bincount(row, minlength=V).double()
    bv = torch.zeros(V, dtype=torch.bool, device=faces.device)
    alone = counts == 1
    bv[lo[alone]] = True
    bv[hi[alone]] = True
    return row, col, deg, bv


def _mean(x, row, col, deg):
    return torch.zeros_like(x).index_add_(0, row, x[col]) / deg[:, None]


def torch_taubin(verts, adj, n=10, lam=0.5, mu=-0.53):
    row, col, deg, bv = adj
    moves = ((deg > 0) & ~bv)[:, None]
    deg = deg.clamp_min(1.0)
    x = verts.double()
    for k in range(2 * n):
        x = torch.where(moves, x + (mu if k % 2 else lam) * (_mean(x, row, col, deg) - x), x)
    return x.to(verts.dtype)


def torch_humphrey(verts, adj, n=10, alpha=0.1, beta=0.5):
    row, col, deg, bv = adj
    moves = ((deg > 0) & ~bv)[:, None]
    deg = deg.clamp_min(1.0)
    o = verts.double()
    x = o
    for _ in range(n):
        q = x
        x = torch.where(moves, _mean(q, row, col, deg), q)
        b = x - (alpha * o + (1.0 - alpha) * q)
        x = torch.where(moves, x - (beta * b + (1.0 - beta) * _mean(b, row, col, deg)), x)
    return x.to(verts.dtype)


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


def smooth_case(name, verts, faces, rounds):
    from vtaco_amd import ops
    from vtaco_amd.conv_onet.generation import Mesh
    m = ops.mesh
    V = verts.shape[0]
    adj, tadj = m.vertex_adjacency(faces, V), torch_adjacency(faces, V)
    mesh = Mesh(verts, faces)
    cands = {
        "adjacency": lambda: m.vertex_adjacency(faces, V),
        "torch_adjacency": lambda: torch_adjacency(faces, V),
        "taubin10": lambda: m.smooth(verts, adj, "taubin", 10),
        "torch_taubin10": lambda: torch_taubin(verts, tadj),
        "humphrey10": lambda: m.smooth(verts, adj, "humphrey", 10),
        "torch_humphrey10": lambda: torch_humphrey(verts, tadj),
        "mesh_smooth": lambda: mesh.smooth("taubin", 10),
        "torch_mesh_smooth": lambda: torch_taubin(verts, torch_adjacency(faces, V)),
        "laplacian20": lambda: m.smooth(verts, adj, "laplacian", 20, form="launches"),
        "laplacian40": lambda: m.smooth(verts, adj, "laplacian", 40, form="launches"),
    }
    fits = V <= m.SMOOTH_WORKGROUP_MAX_V                                  # the two forms of the filter, where there is a choice
    if fits:
        for method in ("taubin", "humphrey"):
            for form in ("launches", "workgroup"):
                cands[f"{method}10_{form}"] = lambda method=method, form=form: m.smooth(verts, adj, method, 10, form=form)
    t, out = alternately(cands, rounds)
    # the kernel path is deterministic: a second run has equal bits; the torch form agrees to rounding
    assert torch.equal(out["taubin10"], m.smooth(verts, adj, "taubin", 10)) and torch.equal(out["humphrey10"], m.smooth(verts, adj, "humphrey", 10))
    assert torch.equal(out["mesh_smooth"].vertices, out["taubin10"])
    row, col, deg, bv = tadj
    assert int(adj.offsets[-1]) == row.shape[0] and torch.equal(adj.boundary_vertex.bool(), bv)
    assert torch.equal((adj.offsets[1:] - adj.offsets[:-1]).double(), deg)
    scale = float(verts.abs().max())
    diff = {k: float((out[k].double() - out["torch_" + k].double()).abs().max()) for k in ("taubin10", "humphrey10")}
    # both carry float64 whose sums differ in their last bits (the order of the atomics), so after the one rounding to the vertices' type
    # they differ by an ulp of the largest coordinate at the most; four are allowed
    tol = 4 * scale * (2.0 ** -23 if verts.dtype == torch.float32 else 2.0 ** -44)
    assert all(d <= tol for d in diff.values()), (name, diff, tol)
    nnz = row.shape[0]
    pass_ms = (t["laplacian40"][0] - t["laplacian20"][0]) / 20.0
    pass_bytes = 4 * (V + 1) + 4 * nnz + 24 * nnz + 24 * V
    case = {"case": name, "vertices": int(V), "faces": int(faces.shape[0]), "nnz": int(nnz), "max_degree": int(deg.max()),
            "boundary_vertices": int(bv.sum()), "dtype": str(verts.dtype).replace("torch.", "")}
    for k in ("adjacency", "taubin10", "humphrey10", "mesh_smooth"):
        case[k + "_ms"], case[k + "_spread_ms"] = t[k]
        case["torch_" + k + "_ms"], case["torch_" + k + "_spread_ms"] = t["torch_" + k]
        case[k + "_torch_over_kernel_time"] = round(t["torch_" + k][0] / t[k][0], 2)
    case.update({"taubin10_max_abs_diff_to_torch": diff["taubin10"], "humphrey10_max_abs_diff_to_torch": diff["humphrey10"],
                 "kernel_runs_equal_bits": True})
    if not V <= m.SMOOTH_WORKGROUP_MAX_V:                                 # (a small mesh's pass is a launch boundary: its bytes say nothing)
        case.update({"laplacian20_ms": t["laplacian20"][0], "laplacian40_ms": t["laplacian40"][0], "pass_ms": round(pass_ms, 5),
                     "pass_algorithmic_bytes": pass_bytes, "pass_GB_per_s": round(pass_bytes / (pass_ms * 1e-3) / 1e9, 1) if pass_ms > 0 else None})
    if fits:
        for method in ("taubin", "humphrey"):
            a, b = f"{method}10_launches", f"{method}10_workgroup"
            assert torch.equal(out[a], out[b]) and torch.equal(out[a], out[method + "10"])
            case.update({a + "_ms": t[a][0], a + "_spread_ms": t[a][1], b + "_ms": t[b][0], b + "_spread_ms": t[b][1],
                         f"{method}10_launches_over_workgroup_time": round(t[a][0] / t[b][0], 2)})
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
        sys.exit("bench_mesh_smooth: no HIP device")
    if args.wnf:
        return wnf_line(args.wnf, args.rounds)
    import mesh_topo_ref as T
    from vtaco_amd import synth_mano
    from vtaco_amd.conv_onet.generation import Generator3D
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds,
              "method": "candidates alternately in one process; host clock around a call that ends synchronised; per figure the median over "
                        "rounds and the spread (max - min) between rounds; pass_ms = (40 laplacian passes - 20) / 20", "cases": []}
    wanted = args.cases.split(",")
    if "a" in wanted or "d" in wanted:
        model, cloud = scene(dev)
    if "a" in wanted:
        for r0 in (32, 64):
            mesh = Generator3D(model, device=dev, resolution0=r0).generate_obj_mesh_wnf({"inputs": cloud})
            result["cases"].append(smooth_case(f"a: shipped scene, marching cubes at {4 * r0}^3", mesh.vertices, mesh.faces, args.rounds))
            torch.cuda.empty_cache()
    if "b" in wanted:
        v, f = T.torus(32, 64)
        result["cases"].append(smooth_case("b: torus of 4096 faces", torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev), args.rounds))
    if "c" in wanted:
        import numpy as np
        asset = synth_mano.make_asset(0)
        v, f = torch.from_numpy(asset["v_template"].astype(np.float32)).to(dev), torch.from_numpy(asset["f"].astype(np.int32)).to(dev)
        result["cases"].append(smooth_case("c: the 778-vertex hand (synthetic MANO template)", v, f, args.rounds))
    if "d" in wanted:
        gens = {str(name): Generator3D(model, device=dev, resolution0=32, smooth=name) for name in (None, "taubin")}
        data = {"inputs": cloud}
        for g in gens.values():                                                  # every shape twice: the second call captures the scene graph
            g.generate_obj_mesh_wnf(data)
            g.generate_obj_mesh_wnf(data)
        t, out = alternately({k: (lambda g=g: g.generate_obj_mesh_wnf(data)) for k, g in gens.items()}, max(args.rounds, 20))
        case = {"case": "d: generate_obj_mesh_wnf at 128^3, smooth=None against 'taubin' (10 pairs)",
                "none_ms": t["None"][0], "none_spread_ms": t["None"][1], "taubin_ms": t["taubin"][0], "taubin_spread_ms": t["taubin"][1],
                "faces": int(out["None"].faces.shape[0]), "same_faces": bool(torch.equal(out["None"].faces, out["taubin"].faces)),
                "max_displacement": float((out["taubin"].vertices - out["None"].vertices).norm(dim=1).max())}
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
