#!/usr/bin/env python3
"""What normals cost (csrc/mc_normals.hip, csrc/mesh_normals.hip), on the shipped scene (BASELINE config 2: tests/config2_case.py):

  (a) generate_obj_mesh_wnf at 128^3 and 256^3 with ``with_normals`` off and on: the extra cost, and the share of it that is the
      vt_mc_emit_normals kernel itself (device events around that one launch on a workspace a count and an emit filled); the rest is
      the two output allocations and the launch
  (b) ``vertex_normals`` (area weights) of the 128^3 and 256^3 meshes against a torch formulation on the same device: cross products,
      three ``index_add_`` (float atomics: the bits change from run to run), a normalisation.  The largest difference is reported.

Per figure: host-clock ms around a call that ends synchronised, the median over --rounds rounds that time every candidate once each,
alternately, in one process, with the spread (max - min) between rounds.  Nothing is gated on these times.  Prints one JSON object;
--out also writes it.  ``--wnf LABEL`` instead prints one JSON line with the time of generate_obj_mesh_wnf at 128^3 with the defaults
in the tree the script lies in (profiles/mc_normals_wnf_parent.jsonl: this commit and its parent, alternately; the parent, which has
no such script, is timed by tools/bench_mesh_simplify.py --wnf, the same measurement).

    python tools/bench_mc_normals.py [--rounds 5] [--out profiles/mc_normals_bench.json]
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


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def alternately(cands, rounds, warmup=3):
    """{name: (median ms, spread ms)} and the warm-up outputs: every candidate once per round, in turn."""
    out = {}
    for _ in range(warmup):
        out = {k: fn() for k, fn in cands.items()}
    times = {k: [] for k in cands}
    for _ in range(rounds):
        for k, fn in cands.items():
            times[k].append(timed(fn)[0])
    return {k: (round(statistics.median(v), 4), round(max(v) - min(v), 4)) for k, v in times.items()}, out


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


def kernel_ms(model, cloud, nx, rounds):
    """Device time of the vt_mc_emit_normals launch alone on the scene's logits: median and spread over ``rounds`` launches."""
    from vtaco_amd import ops
    from vtaco_amd.conv_onet.generation import Generator3D
    gen = Generator3D(model, device=cloud.device, resolution0=nx // 4)
    with torch.no_grad():
        vol = gen.eval_lattice(model.encode_inputs(cloud), nx).reshape(nx, nx, nx).contiguous()
    verts, faces, _ = ops.marching_cubes(vol)
    ws = ops.mc.mc_count(vol)
    ops.mc.mc_emit(vol, ws, capacity=(verts.shape[0], faces.shape[0]))
    ts = []
    for i in range(rounds + 3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ops.mc.mc_emit_normals(vol, ws, verts.shape[0])
        b.record()
        torch.cuda.synchronize()
        if i >= 3:
            ts.append(a.elapsed_time(b))
    return round(statistics.median(ts), 4), round(max(ts) - min(ts), 4)


def torch_vertex_normals(v, f):
    p, f = v.double(), f.long()
    n = torch.linalg.cross(p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]])
    s = torch.zeros_like(p)
    for k in range(3):
        s.index_add_(0, f[:, k], n)
    length = s.norm(dim=1, keepdim=True)
    return torch.where(length > 0, s / length.clamp_min(1e-300), torch.zeros_like(s)).to(v.dtype)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out")
    ap.add_argument("--wnf", metavar="LABEL")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_mc_normals: no HIP device")
    if args.wnf:
        return wnf_line(args.wnf, args.rounds)
    from vtaco_amd.conv_onet.generation import Generator3D
    from vtaco_amd.utils import mesh_clean
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds,
              "method": "candidates alternately in one process; host clock around a call that ends synchronised; per figure the median over "
                        "rounds and the spread (max - min) between rounds; kernel_ms by device events around the one launch", "cases": []}
    model, cloud = scene(dev)
    data = {"inputs": cloud}
    for r0 in (32, 64):
        nx = 4 * r0
        off, on = Generator3D(model, device=dev, resolution0=r0), Generator3D(model, device=dev, resolution0=r0, with_normals=True)
        t, out = alternately({"off": lambda: off.generate_obj_mesh_wnf(data), "on": lambda: on.generate_obj_mesh_wnf(data)}, args.rounds)
        k_ms, k_spread = kernel_ms(model, cloud, nx, args.rounds)
        extra = round(t["on"][0] - t["off"][0], 4)
        case = {"case": f"a: generate_obj_mesh_wnf at {nx}^3, with_normals off / on", "vertices": int(out["on"].vertices.shape[0]),
                "faces": int(out["on"].faces.shape[0]), "off_ms": t["off"][0], "off_spread_ms": t["off"][1], "on_ms": t["on"][0],
                "on_spread_ms": t["on"][1], "extra_ms": extra, "kernel_ms": k_ms, "kernel_spread_ms": k_spread,
                "kernel_share_of_extra": round(k_ms / extra, 3) if extra > 0 else None,
                "same_mesh": bool(torch.equal(out["on"].vertices, out["off"].vertices) and torch.equal(out["on"].faces, out["off"].faces))}
        print(json.dumps(case), file=sys.stderr, flush=True)
        result["cases"].append(case)
        mesh = out["off"]
        v, f = mesh.vertices.clone(), mesh.faces.clone()
        t, o = alternately({"kernel": lambda: mesh_clean.vertex_normals((v, f)), "torch": lambda: torch_vertex_normals(v, f)}, args.rounds)
        case = {"case": f"b: vertex_normals (area) of the {nx}^3 mesh against torch index_add_", "vertices": int(v.shape[0]), "faces": int(f.shape[0]),
                "kernel_ms": t["kernel"][0], "kernel_spread_ms": t["kernel"][1], "torch_ms": t["torch"][0], "torch_spread_ms": t["torch"][1],
                "torch_over_kernel_time": round(t["torch"][0] / t["kernel"][0], 2),
                "max_difference": float((o["kernel"].double() - o["torch"].double()).abs().max()),
                "kernel_bits_repeat": bool(torch.equal(o["kernel"], mesh_clean.vertex_normals((v, f))))}
        print(json.dumps(case), file=sys.stderr, flush=True)
        result["cases"].append(case)
        del off, on
        torch.cuda.empty_cache()
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
