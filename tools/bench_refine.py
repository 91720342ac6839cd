#!/usr/bin/env python3
"""What mesh refinement costs (csrc/field_jet.hip, csrc/refine.hip), on the shipped scene (BASELINE config 2: tests/config2_case.py):
its meshes at 128^3 and 256^3 and a 4 096-face torus (launch-bound).  Three candidates for the field jet at the face points:

  fused      vt_decode_jet: one kernel
  composed   vt_decode_jet_composed: vt_decode_fwd (save) + vt_decode_bwd_dc + the gather kernel
  torch      what a user would write today: the decoder in torch ops on the same device under autograd with create_graph=True, one
             more grad per Hessian row (tests/refine_ref.py in float32; its corner-gather sampler, because torch has no double
             backward for grid_sample)

and for a whole iteration (sample -> jet -> face gradient -> RMSprop step): ops.refine over 30 steps / 30 with either jet, and the torch
loss + autograd + update.  Then generate_obj_mesh_wnf at 128^3 with refinement_step 0 and 30.

Per figure: host-clock ms around a call that ends synchronised, the median over --rounds rounds that time every candidate once each,
alternately, in one process, with the spread (max - min) between rounds.  Nothing is gated on these times.  Prints one JSON object;
--out also writes it.  ``--wnf LABEL`` instead prints one JSON line with the time of generate_obj_mesh_wnf at 128^3 with the defaults.

    python tools/bench_refine.py [--rounds 5] [--out profiles/refine_bench.json]
"""
import argparse
import json
import math
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


def alternately(cands, rounds, warmup=2):
    """{name: (median ms, spread ms)}: every candidate once per round, in turn."""
    for _ in range(warmup):
        for fn in cands.values():
            fn()
    times = {k: [] for k in cands}
    for _ in range(rounds):
        for k, fn in cands.items():
            times[k].append(timed(fn)[0])
    return {k: (round(statistics.median(v), 4), round(max(v) - min(v), 4)) for k, v in times.items()}


def scene(dev):
    import config2_case as c2
    from vtaco_amd.conv_onet.models import ConvolutionalOccupancyNetwork
    z = c2.fixture()
    enc, dec = c2.models(z)
    return ConvolutionalOccupancyNetwork(dec, enc, device=dev).eval(), torch.from_numpy(z["cloud"]).float().to(dev)


def torus(n_u=64, n_v=32, dev="cuda:0"):
    """2 n_u n_v faces (4 096) of a torus inside the box."""
    u = torch.arange(n_u, dtype=torch.float64) * (2 * math.pi / n_u)
    v = torch.arange(n_v, dtype=torch.float64) * (2 * math.pi / n_v)
    uu, vv = torch.meshgrid(u, v, indexing="ij")
    verts = torch.stack([(0.3 + 0.1 * vv.cos()) * uu.cos(), (0.3 + 0.1 * vv.cos()) * uu.sin(), 0.1 * vv.sin()], -1).reshape(-1, 3)
    i, j = torch.meshgrid(torch.arange(n_u), torch.arange(n_v), indexing="ij")
    a, b = i * n_v + j, ((i + 1) % n_u) * n_v + j
    c, d = ((i + 1) % n_u) * n_v + (j + 1) % n_v, i * n_v + (j + 1) % n_v
    faces = torch.cat([torch.stack([a, b, c], -1).reshape(-1, 3), torch.stack([a, c, d], -1).reshape(-1, 3)])
    return verts.float().to(dev), faces.int().to(dev)


def wnf_line(label, rounds):
    from vtaco_amd.conv_onet.generation import Generator3D
    dev = "cuda:0"
    model, cloud = scene(dev)
    gen = Generator3D(model, device=dev, resolution0=32, padding=0.1)
    res = alternately({"wnf": lambda: gen.generate_obj_mesh_wnf({"inputs": cloud})}, rounds, warmup=4)
    print(json.dumps({"label": label, "wnf_128_ms": res["wnf"][0], "spread_ms": res["wnf"][1], "rounds": rounds}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--wnf", default=None, metavar="LABEL")
    ap.add_argument("--sizes", default="32,64", help="resolution0 of the scene's meshes (lattice = 4 x)")
    args = ap.parse_args()
    if args.wnf is not None:
        return wnf_line(args.wnf, args.rounds)
    import refine_ref as rr
    from vtaco_amd import ops
    from vtaco_amd.conv_onet.generation import Generator3D
    dev = "cuda:0"
    model, cloud = scene(dev)
    dec = model.decoder
    blob, blob_t = ops.refine.refine_blobs(dec)
    sd = {k: v.detach() for k, v in dec.state_dict().items()}
    data = {"inputs": cloud}
    with torch.no_grad():
        grid = model.encode_inputs(cloud)["grid"].float().clone()
    grid_cf = grid.contiguous()                                     # the torch candidate indexes a plain [1,C,R,R,R] tensor
    meshes = {}
    for r0 in [int(x) for x in args.sizes.split(",")]:
        m = Generator3D(model, device=dev, resolution0=r0, padding=0.1).generate_obj_mesh_wnf(data)
        meshes[f"scene_{4 * r0}^3"] = (m.vertices.float().contiguous(), m.faces.contiguous())
    meshes["torus"] = torus(dev=dev)
    report = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "cases": {}}
    for name, (verts, faces) in meshes.items():
        F = faces.shape[0]
        _, pts = ops.refine.refine_sample(verts, faces, seed=1)
        p1 = pts.unsqueeze(0)

        def torch_iteration():
            eps, _ = ops.refine.refine_sample(verts, faces, seed=1)
            _, _, _, g = rr.refine_loss(sd, grid_cf, verts, faces, eps, 0.5, dtype=torch.float32)
            return rr.rmsprop_step(verts, g, torch.zeros_like(verts))[0]
        jet = alternately({"fused": lambda: ops.refine.decode_jet(grid, blob, blob_t, p1, form="fused"),
                           "composed": lambda: ops.refine.decode_jet(grid, blob, blob_t, p1, form="composed"),
                           "torch": lambda: rr.jet_autograd(sd, grid_cf, pts, dtype=torch.float32)[0]}, args.rounds)
        it = alternately({"fused": lambda: ops.refine.refine(verts, faces, grid, dec, 30, 0.5, dec.padding, form="fused"),
                          "composed": lambda: ops.refine.refine(verts, faces, grid, dec, 30, 0.5, dec.padding, form="composed"),
                          "torch": torch_iteration}, args.rounds)
        ref = ops.refine.decode_jet(grid, blob, blob_t, p1, form="fused")[0, :, :7]
        tj = rr.jet_autograd(sd, grid_cf, pts, dtype=torch.float32)[0]
        report["cases"][name] = {
            "faces": F, "vertices": int(verts.shape[0]),
            "jet_ms": {k: v[0] for k, v in jet.items()}, "jet_spread_ms": {k: v[1] for k, v in jet.items()},
            "iteration_ms": {"fused": round(it["fused"][0] / 30, 4), "composed": round(it["composed"][0] / 30, 4), "torch": it["torch"][0]},
            "iteration_spread_ms": {"fused": round(it["fused"][1] / 30, 4), "composed": round(it["composed"][1] / 30, 4), "torch": it["torch"][1]},
            "fused_equals_composed": bool(torch.equal(ops.refine.decode_jet(grid, blob, blob_t, p1, form="fused"),
                                                      ops.refine.decode_jet(grid, blob, blob_t, p1, form="composed"))),
            "median_abs_jet_difference_fused_vs_torch_f32": float((ref - tj).abs().median())}
    g0 = Generator3D(model, device=dev, resolution0=32, padding=0.1)
    g30 = Generator3D(model, device=dev, resolution0=32, padding=0.1, refinement_step=30)
    wnf = alternately({"refinement_step_0": lambda: g0.generate_obj_mesh_wnf(data), "refinement_step_30": lambda: g30.generate_obj_mesh_wnf(data)},
                      args.rounds, warmup=4)
    report["generate_obj_mesh_wnf_128_ms"] = {k: v[0] for k, v in wnf.items()}
    report["generate_obj_mesh_wnf_128_spread_ms"] = {k: v[1] for k, v in wnf.items()}
    text = json.dumps(report, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
