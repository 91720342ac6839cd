#!/usr/bin/env python3
"""Time and quality of edge-collapse decimation (csrc/mesh_collapse.hip through ``utils.mesh_clean.decimate``) against vertex clustering
(csrc/mesh_simplify.hip through ``utils.mesh_clean.simplify``) at equal ``nfaces``.  Meshes: the shipped scene's (BASELINE config 2:
tests/config2_case.py) marching-cubes mesh at 128^3 and 256^3, each to 10 000 and 100 000 faces, and the 4 096-face torus of
tests/mesh_topo_ref.py to 1 000.  Per case: the time of both, the rounds and whether the decimation stalled, the faces both reached, and
the quality of both results against the input mesh -- ``eval.mesh_distances`` Chamfer-L1 with 100 000 samples (``distance='tree'``, one
seeded generator per measurement), the relative error of the summed signed volume, and the non-manifold and boundary edge counts of
``Mesh.components()``.

Per time: host-clock ms around a call that ends synchronised, the median over --rounds rounds that time every candidate once each,
alternately, in one process, with the spread (max - min) between rounds.  Nothing is gated on these figures.  Prints one JSON object;
--out also writes it.  ``--wnf LABEL`` instead prints one JSON line with the time of generate_obj_mesh_wnf at 128^3 with the defaults
in the tree the script lies in (profiles/mesh_collapse_wnf_parent.jsonl: this commit and its parent, alternately).

    python tools/bench_mesh_collapse.py [--rounds 5] [--out profiles/mesh_collapse_bench.json]
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

SAMPLES = 100000


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


def quality(mesh, source, source_volume):
    from vtaco_amd import eval as ev
    g = torch.Generator(device=mesh.vertices.device).manual_seed(0)
    d = ev.mesh_distances((mesh.vertices.float(), mesh.faces), (source.vertices.float(), source.faces), SAMPLES, generator=g, distance="tree")
    c = mesh.components().report()
    volume = sum(c["volume"])
    return {"faces": int(mesh.faces.shape[0]), "vertices": int(mesh.vertices.shape[0]), "chamfer_l1": d["chamfer_l1"], "accuracy": d["accuracy"],
            "completeness": d["completeness"], "relative_volume_error": abs(volume - source_volume) / abs(source_volume),
            "n_components": c["n_components"], "nonmanifold_edges": int(sum(c["n_nonmanifold"])), "boundary_edges": int(sum(c["n_boundary"])),
            "euler": c["euler"][:8]}


def decimate_case(name, mesh, nfaces, rounds):
    from vtaco_amd.utils import mesh_clean
    t, out = alternately({"collapse": lambda: mesh_clean.decimate(mesh, nfaces), "cluster": lambda: mesh_clean.simplify(mesh, nfaces=nfaces)}, rounds)
    _, rep = mesh_clean.decimate_report(mesh, nfaces)
    src = mesh.components().report()
    source_volume = sum(src["volume"])
    case = {"case": name, "vertices": int(mesh.vertices.shape[0]), "faces": int(mesh.faces.shape[0]), "nfaces": nfaces,
            "source": {"n_components": src["n_components"], "nonmanifold_edges": int(sum(src["n_nonmanifold"])),
                       "boundary_edges": int(sum(src["n_boundary"])), "euler": src["euler"][:8], "volume": source_volume},
            "rounds": rep.rounds, "stalled": rep.stalled,
            "collapse_ms": t["collapse"][0], "collapse_spread_ms": t["collapse"][1], "cluster_ms": t["cluster"][0],
            "cluster_spread_ms": t["cluster"][1], "collapse_over_cluster_time": round(t["collapse"][0] / t["cluster"][0], 2),
            "collapse": quality(out["collapse"], mesh, source_volume), "cluster": quality(out["cluster"], mesh, source_volume)}
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
    ap.add_argument("--cases", default="scene,torus")
    ap.add_argument("--out")
    ap.add_argument("--wnf", metavar="LABEL")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_mesh_collapse: no HIP device")
    if args.wnf:
        return wnf_line(args.wnf, args.rounds)
    import mesh_topo_ref as T
    from vtaco_amd.conv_onet.generation import Generator3D, Mesh
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "samples": SAMPLES,
              "method": "candidates alternately in one process; host clock around a call that ends synchronised; per time the median over "
                        "rounds and the spread (max - min) between rounds; quality against the input mesh", "cases": []}
    wanted = args.cases.split(",")
    if "scene" in wanted:
        model, cloud = scene(dev)
        for r0 in (32, 64):
            mesh = Generator3D(model, device=dev, resolution0=r0).generate_obj_mesh_wnf({"inputs": cloud})
            torch.cuda.empty_cache()
            for target in (10000, 100000):
                result["cases"].append(decimate_case(f"shipped scene at {4 * r0}^3 to {target} faces", mesh, target, args.rounds))
    if "torus" in wanted:
        v, f = T.torus(32, 64)
        mesh = Mesh(torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev))
        result["cases"].append(decimate_case("torus 32 x 64 (4 096 faces) to 1 000 faces", mesh, 1000, args.rounds))
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
