#!/usr/bin/env python3
"""Time of the hole-filling kernels (csrc/mesh_fill.hip through ``ops.mesh.boundary_loops`` and ``ops.mesh.fill_holes``, method 'fan')
against a plain torch formulation of the same definition on the same device: the boundary by ``sort`` / ``unique_consecutive`` of 64-bit
edge keys, succ by ``bincount`` and a ``scatter_reduce(amin)``, the loops' heads and positions by pointer doubling with gathers (the same
2 ceil(log2 NB) rounds, no host read per round), the fan by ``repeat_interleave``.  Equal outputs are asserted.  Cases:

  (a) the shipped scene's (BASELINE config 2: tests/config2_case.py) marching-cubes mesh at 128^3 and 256^3, with NB, L and the longest loop
  (b) 2 000 shuffled tetrahedra each missing a face (tests/mesh_fill_ref.py: open_tetrahedra)
  (c) the annulus of 20 000 vertices: two loops of 10 000 edges (tests/mesh_fill_ref.py: annulus)
  (d) generate_obj_mesh_wnf at 128^3 with fill_holes=None against 'fan', alternately
  (e) a marching-cubes sphere that leaves its 256^3 volume through all six sides: six planar loops, the box cut the feature is for

Per figure: host-clock ms around a call that ends synchronised, the median over --rounds rounds that time every candidate once each,
alternately, in one process, with the spread (max - min) between rounds.  Nothing is gated on these times.  Prints one JSON object;
--out also writes it.  ``--wnf LABEL`` instead prints one JSON line with the time of generate_obj_mesh_wnf at 128^3 with the defaults
in the tree the script lies in (profiles/mesh_fill_wnf_parent.jsonl: this commit and its parent, alternately).

    python tools/bench_mesh_fill.py [--rounds 5] [--out profiles/mesh_fill_bench.json]
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


def torch_fill(verts, faces):
    """(offsets, loop vertices, loop half-edges, n_irregular, filled faces) of the definition, method 'fan', in torch ops."""
    dev = faces.device
    f = faces.long()
    F = f.shape[0]
    a, b = f.reshape(-1), f[:, [1, 2, 0]].reshape(-1)                  # tail and head of half-edge h = 3 f + k
    h = torch.arange(3 * F, device=dev)
    live = a != b
    key = (torch.minimum(a, b) << 32) | torch.maximum(a, b)
    key, order = torch.sort(torch.where(live, key, -1 - h))            # dead half-edges get keys of their own, below every live one
    _, inverse, counts = torch.unique_consecutive(key, return_inverse=True, return_counts=True)
    alone = (counts[inverse] == 1) & live[order]
    bhe = torch.sort(h[order][alone]).values                            # half-edge order
    NB = bhe.shape[0]
    empty = torch.zeros(0, dtype=torch.int32, device=dev)
    if NB == 0:
        return torch.zeros(1, dtype=torch.int32, device=dev), empty, empty, 0, faces
    tail, head = a[bhe], b[bhe]
    V = verts.shape[0]
    idx = torch.arange(NB, device=dev)
    vout, vin = torch.bincount(tail, minlength=V), torch.bincount(head, minlength=V)
    vfirst = torch.full((V,), NB, dtype=torch.long, device=dev).scatter_reduce(0, tail, idx, "amin")
    succ = torch.where((vout[head] == 1) & (vin[head] == 1), vfirst[head], -1)
    rounds = max(0, (NB - 1).bit_length())

    def double(nxt, val, op):
        for _ in range(rounds):
            ok = nxt >= 0
            j = nxt.clamp_min(0)
            val = torch.where(ok, op(val, val[j]), val)
            nxt = torch.where(ok, nxt[j], nxt)
        return nxt, val

    nxt, mn = double(succ, idx, torch.minimum)
    in_loop = nxt >= 0
    is_head = in_loop & (mn == idx)
    cut = torch.where(in_loop & ~is_head[succ.clamp_min(0)], succ, -1)
    _, d = double(cut, (cut >= 0).long(), torch.add)
    lens = (d + 1)[is_head]
    L = lens.shape[0]
    offsets = torch.zeros(L + 1, dtype=torch.long, device=dev)
    offsets[1:] = torch.cumsum(lens, 0)
    loop_no = torch.cumsum(is_head, 0) - 1
    hd = mn[in_loop]
    at = offsets[loop_no[hd]] + d[hd] - d[in_loop]
    n_in = int(offsets[-1])                                             # (the one host read: the outputs' size)
    lh = torch.empty(n_in, dtype=torch.long, device=dev)
    lv = torch.empty(n_in, dtype=torch.long, device=dev)
    lh[at] = bhe[in_loop]
    lv[at] = tail[in_loop]
    per = (lens - 2).clamp_min(0)
    which = torch.repeat_interleave(torch.arange(L, device=dev), per)
    first = torch.cumsum(per, 0) - per
    i = torch.arange(which.shape[0], device=dev) - first[which] + 1
    o = offsets[which]
    fan = torch.stack([lv[o], lv[o + i + 1], lv[o + i]], 1)
    return offsets.int(), lv.int(), lh.int(), NB - n_in, torch.cat([faces, fan.int()])


def kernel_fill(verts, faces):
    from vtaco_amd import ops
    loops = ops.mesh.boundary_loops(faces, verts.shape[0])
    return loops, ops.mesh.fill_holes(verts, faces, method="fan", loops=loops)


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


def fill_case(name, verts, faces, rounds):
    t, out = alternately({"kernel": lambda: kernel_fill(verts, faces), "torch": lambda: torch_fill(verts, faces)}, rounds)
    (loops, filled), (off, lv, lh, n_irr, tfaces) = out["kernel"], out["torch"]
    same = (torch.equal(loops.offsets, off) and torch.equal(loops.vertices, lv) and torch.equal(loops.half_edges, lh)
            and loops.n_irregular == n_irr and tuple(filled.faces.shape) == tuple(tfaces.shape) and torch.equal(filled.faces, tfaces))
    assert same, f"{name}: the kernel path and the torch formulation differ"
    lens = (loops.offsets[1:] - loops.offsets[:-1])
    case = {"case": name, "vertices": int(verts.shape[0]), "faces": int(faces.shape[0]), "n_boundary": loops.n_boundary,
            "n_loops": filled.n_loops, "n_irregular": loops.n_irregular, "longest_loop": int(lens.max()) if lens.numel() else 0,
            "new_faces": filled.n_new_faces, "doubling_rounds_per_pass": (loops.n_boundary - 1).bit_length() if loops.n_boundary else 0,
            "kernel_ms": t["kernel"][0], "kernel_spread_ms": t["kernel"][1], "torch_ms": t["torch"][0], "torch_spread_ms": t["torch"][1],
            "torch_over_kernel_time": round(t["torch"][0] / t["kernel"][0], 2), "outputs_equal": bool(same)}
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
    ap.add_argument("--cases", default="a,b,c,d,e")
    ap.add_argument("--out")
    ap.add_argument("--wnf", metavar="LABEL")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_mesh_fill: no HIP device")
    if args.wnf:
        return wnf_line(args.wnf, args.rounds)
    import mesh_fill_ref as R
    from vtaco_amd.conv_onet.generation import Generator3D
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds,
              "method": "candidates alternately in one process; host clock around a call that ends synchronised; per figure the median over "
                        "rounds and the spread (max - min) between rounds", "cases": []}
    wanted = args.cases.split(",")
    to_dev = lambda v, f: (torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev))
    if "a" in wanted or "d" in wanted:
        model, cloud = scene(dev)
    if "a" in wanted:
        for r0 in (32, 64):
            mesh = Generator3D(model, device=dev, resolution0=r0).generate_obj_mesh_wnf({"inputs": cloud})
            result["cases"].append(fill_case(f"a: shipped scene, marching cubes at {4 * r0}^3", mesh.vertices, mesh.faces, args.rounds))
            torch.cuda.empty_cache()
    if "b" in wanted:
        result["cases"].append(fill_case("b: 2000 open tetrahedra, faces shuffled", *to_dev(*R.open_tetrahedra(2000)), args.rounds))
    if "c" in wanted:
        result["cases"].append(fill_case("c: annulus of 20000 vertices, two loops of 10000 edges", *to_dev(*R.annulus(20000)), args.rounds))
    if "d" in wanted:
        gens = {str(name): Generator3D(model, device=dev, resolution0=32, fill_holes=name) for name in (None, "fan")}
        data = {"inputs": cloud}
        for g in gens.values():                                                  # every shape twice: the second call captures the scene graph
            g.generate_obj_mesh_wnf(data)
            g.generate_obj_mesh_wnf(data)
        t, out = alternately({k: (lambda g=g: g.generate_obj_mesh_wnf(data)) for k, g in gens.items()}, max(args.rounds, 20))
        comps = out["fan"].components()
        case = {"case": "d: generate_obj_mesh_wnf at 128^3, fill_holes=None against 'fan'",
                "none_ms": t["None"][0], "none_spread_ms": t["None"][1], "fan_ms": t["fan"][0], "fan_spread_ms": t["fan"][1],
                "none_faces": int(out["None"].faces.shape[0]), "fan_faces": int(out["fan"].faces.shape[0]),
                "fan_watertight_components": int(comps.watertight.sum()), "fan_components": comps.n_components}
        print(json.dumps(case), file=sys.stderr, flush=True)
        result["cases"].append(case)
    if "e" in wanted:
        from vtaco_amd import ops
        verts, faces, _ = ops.marching_cubes(torch.from_numpy(R.sphere_volume(256, 150.0)).to(dev), level=0.0)
        result["cases"].append(fill_case("e: marching-cubes sphere of radius 150 cut by its 256^3 box", verts, faces, args.rounds))
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
