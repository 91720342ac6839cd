#!/usr/bin/env python3
"""Time of the subdivision kernels (csrc/mesh_subdivide.hip through ``ops.mesh.subdivide``, ``utils/mesh_clean`` and ``UpSampleLayer``)
against a plain torch formulation on the same device: the edges by ``unique`` over 64-bit keys, the first-seen numbering by
``scatter_reduce(amin)`` of the half-edge index and an ``argsort``, the vertices and faces by gathers.  The midpoint form is compared bit
for bit; the Loop form's even vertices are ``index_add_`` sums (float atomics in no fixed order) and are compared to a tolerance.  Cases:

  (a) a stand-in of the 778-vertex hand's size and topology (``hand_stand_in``: 769 vertices, 1 520 faces, a disk), 1 and 2 levels, and
      ``UpSampleLayer`` on a batch of 8 of them with its connectivity cache on and off
  (b) the shipped scene's (BASELINE config 2: tests/config2_case.py) marching-cubes mesh at 128^3, one midpoint level
  (c) ``subdivide_to_size`` on the 4 096-face torus (tests/mesh_topo_ref.py: torus(32, 64)) to half its longest edge
  (d) Loop on the 128^3 mesh

Per figure: host-clock ms around a call that ends synchronised, the median over --rounds rounds that time every candidate once each,
alternately, in one process, with the spread (max - min) between rounds.  Nothing is gated on these times.  Prints one JSON object;
--out also writes it.  ``--wnf LABEL`` instead prints one JSON line with the time of generate_obj_mesh_wnf at 128^3 with the defaults
in the tree the script lies in (profiles/mesh_subdivide_wnf_parent.jsonl: this commit and its parent, in turn).

    python tools/bench_mesh_subdivide.py [--rounds 5] [--out profiles/mesh_subdivide_bench.json]
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


def torch_edges(faces):
    """(lo, hi int64 [E] in first-seen order, edge of every half-edge int64 [3F], fwd, bwd counts [E])."""
    f = faces.long()
    a, b = f.reshape(-1), f[:, [1, 2, 0]].reshape(-1)
    key, inv = torch.unique((torch.minimum(a, b) << 32) | torch.maximum(a, b), return_inverse=True)
    n = key.shape[0]
    h = torch.arange(a.shape[0], device=f.device)
    minh = torch.full((n,), a.shape[0], dtype=torch.int64, device=f.device).scatter_reduce(0, inv, h, "amin")
    order = torch.argsort(minh)
    rank = torch.empty_like(order)
    rank[order] = torch.arange(n, device=f.device)
    up = a < b
    fwd = torch.bincount(inv[up], minlength=n)[order]
    bwd = torch.bincount(inv[~up], minlength=n)[order]
    return (key >> 32)[order], (key & 0xffffffff)[order], rank[inv], fwd, bwd


def torch_children(faces, eid, V):
    f = faces.long()
    m = (V + eid).reshape(-1, 3)
    a, b, c, x, y, z = f[:, 0], f[:, 1], f[:, 2], m[:, 0], m[:, 1], m[:, 2]
    kids = torch.stack([torch.stack([x, y, z], 1), torch.stack([a, x, z], 1), torch.stack([b, y, x], 1), torch.stack([c, z, y], 1)], 1)
    return kids.reshape(-1, 3).int()


def torch_midpoint(verts, faces):
    lo, hi, eid, _, _ = torch_edges(faces)
    return torch.cat([verts, (verts[lo] + verts[hi]) * 0.5]), torch_children(faces, eid, verts.shape[0])


def torch_loop(verts, faces):
    V = verts.shape[0]
    lo, hi, eid, fwd, bwd = torch_edges(faces)
    f = faces.long()
    a, b = f.reshape(-1), f[:, [1, 2, 0]].reshape(-1)
    opp, up = f[:, [2, 0, 1]].reshape(-1), a < b
    c = torch.zeros_like(lo).scatter(0, eid[up], opp[up])
    d = torch.zeros_like(lo).scatter(0, eid[~up], opp[~up])
    x = verts.double()
    interior = ((fwd == 1) & (bwd == 1))[:, None]
    odd = torch.where(interior, 0.375 * (x[lo] + x[hi]) + 0.125 * (x[c] + x[d]), (x[lo] + x[hi]) * 0.5)
    row, col = torch.cat([lo, hi]), torch.cat([hi, lo])
    n = torch.bincount(row, minlength=V).double()
    s = torch.zeros_like(x).index_add_(0, row, x[col])
    beta = torch.where(n == 3, torch.full_like(n, 0.1875), 3.0 / (8.0 * n.clamp_min(1.0)))
    even = (1.0 - n * beta)[:, None] * x + beta[:, None] * s
    edge_b = (fwd + bwd) == 1
    rb, cb = torch.cat([lo[edge_b], hi[edge_b]]), torch.cat([hi[edge_b], lo[edge_b]])
    nb = torch.bincount(rb, minlength=V)
    sb = torch.zeros_like(x).index_add_(0, rb, x[cb])
    even = torch.where((nb == 2)[:, None], 0.75 * x + 0.125 * sb, even)
    bad = ~((fwd <= 1) & (bwd <= 1))
    keep = (n == 0) | ((nb > 0) & (nb != 2))
    keep[lo[bad]] = True
    keep[hi[bad]] = True
    even = torch.where(keep[:, None], x, even)
    return torch.cat([even, odd]).to(verts.dtype), torch_children(faces, eid, V)


def hand_stand_in(rings=48, around=16):
    """A mesh of the MANO hand's size and topology -- a disk, open at the wrist: a tube of 48 rings of 16 vertices closed by one apex
    vertex, 769 vertices and 1 520 faces against the hand's 778 and 1 538.  (The synthetic MANO asset's faces are random triples, some
    with a repeated index, which a subdivision refuses.)"""
    import numpy as np
    rng = np.random.RandomState(0)
    k, a = np.meshgrid(np.arange(rings), np.arange(around), indexing="ij")
    r = 0.02 + 0.01 * np.sin(k / 5.0)
    v = np.stack([r * np.cos(2 * np.pi * a / around), r * np.sin(2 * np.pi * a / around), 0.004 * k], -1).reshape(-1, 3)
    v = np.concatenate([v, [[0.0, 0.0, 0.004 * rings]]]) + rng.randn(rings * around + 1, 3) * 2e-4
    idx = lambda i, j: i * around + j % around
    f = []
    for i in range(rings - 1):
        for j in range(around):
            f += [[idx(i, j), idx(i, j + 1), idx(i + 1, j + 1)], [idx(i, j), idx(i + 1, j + 1), idx(i + 1, j)]]
    f += [[idx(rings - 1, j), idx(rings - 1, j + 1), rings * around] for j in range(around)]
    return v.astype(np.float32), np.array(f, dtype=np.int32)


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


def _record(case, t, pairs):
    for k, tk in pairs:
        case[k + "_ms"], case[k + "_spread_ms"] = t[k]
        if tk is not None:
            case[tk + "_ms"], case[tk + "_spread_ms"] = t[tk]
            case[k + "_torch_over_kernel_time"] = round(t[tk][0] / t[k][0], 2)


def midpoint_case(name, verts, faces, rounds, levels=(1,)):
    from vtaco_amd import ops
    from vtaco_amd.conv_onet.generation import Mesh
    mesh = Mesh(verts, faces)

    def torch_levels(n):
        v, f = verts, faces
        for _ in range(n):
            v, f = torch_midpoint(v, f)
        return v, f
    cands = {}
    for n in levels:
        cands[f"subdivide{n}"] = lambda n=n: mesh.subdivide(n)
        cands[f"torch_subdivide{n}"] = lambda n=n: torch_levels(n)
    t, out = alternately(cands, rounds)
    case = {"case": name, "vertices": int(verts.shape[0]), "faces": int(faces.shape[0]), "dtype": str(verts.dtype).replace("torch.", "")}
    for n in levels:
        got, (tv, tf) = out[f"subdivide{n}"], out[f"torch_subdivide{n}"]
        assert torch.equal(got.vertices, tv) and torch.equal(got.faces, tf)          # the same numbering, the same bits
        again = mesh.subdivide(n)
        assert torch.equal(got.vertices, again.vertices) and torch.equal(got.faces, again.faces)
        case[f"vertices_after_{n}"], case[f"faces_after_{n}"] = int(tv.shape[0]), int(tf.shape[0])
    _record(case, t, [(f"subdivide{n}", f"torch_subdivide{n}") for n in levels])
    case["equal_to_torch_bit_for_bit"] = True
    print(json.dumps(case), file=sys.stderr, flush=True)
    return case


def layer_case(verts, faces, rounds, B=8):
    """UpSampleLayer on a batch of hands: the connectivity cached against rebuilt on every call, and the torch form both ways."""
    from vtaco_amd.encoder.manopth import UpSampleLayer
    vb = torch.stack([verts * (1.0 + 0.01 * b) for b in range(B)]).contiguous()
    fb = faces.long().unsqueeze(0).expand(B, -1, -1)
    cached, rebuilt = UpSampleLayer(), UpSampleLayer(cache_size=0)

    def levels(layer, n):
        v, f = vb, fb
        for _ in range(n):
            v, f = layer(v, f)
        return v, f
    lo1, hi1, eid1, _, _ = torch_edges(faces)
    f1 = torch_children(faces, eid1, verts.shape[0])

    def torch_cached():
        return torch.cat([vb, (vb[:, lo1] + vb[:, hi1]) * 0.5], 1), f1

    def torch_rebuilt():
        lo, hi, eid, _, _ = torch_edges(faces)
        return torch.cat([vb, (vb[:, lo] + vb[:, hi]) * 0.5], 1), torch_children(faces, eid, verts.shape[0])
    cands = {"layer1_cached": lambda: levels(cached, 1), "layer1_rebuilt": lambda: levels(rebuilt, 1), "layer2_cached": lambda: levels(cached, 2),
             "layer2_rebuilt": lambda: levels(rebuilt, 2), "torch_layer1_cached": torch_cached, "torch_layer1_rebuilt": torch_rebuilt}
    t, out = alternately(cands, rounds)
    assert torch.equal(out["layer1_cached"][0], out["torch_layer1_rebuilt"][0]) and torch.equal(out["layer1_cached"][0], out["layer1_rebuilt"][0])
    assert torch.equal(out["layer1_cached"][1][0].int(), out["torch_layer1_rebuilt"][1])
    case = {"case": f"a: UpSampleLayer on a batch of {B} hands", "vertices": int(verts.shape[0]), "faces": int(faces.shape[0]),
            "vertices_after_1": int(out["layer1_cached"][0].shape[1]), "vertices_after_2": int(out["layer2_cached"][0].shape[1])}
    _record(case, t, [("layer1_cached", "torch_layer1_cached"), ("layer1_rebuilt", "torch_layer1_rebuilt"), ("layer2_cached", None),
                      ("layer2_rebuilt", None)])
    case["layer1_rebuilt_over_cached_time"] = round(t["layer1_rebuilt"][0] / t["layer1_cached"][0], 2)
    case["layer2_rebuilt_over_cached_time"] = round(t["layer2_rebuilt"][0] / t["layer2_cached"][0], 2)
    print(json.dumps(case), file=sys.stderr, flush=True)
    return case


def to_size_case(verts, faces, rounds):
    from vtaco_amd.conv_onet.generation import Mesh
    mesh = Mesh(verts, faces)
    f = faces.long()
    longest = max(float((verts[f[:, k]] - verts[f[:, (k + 1) % 3]]).norm(dim=1).max()) for k in range(3))
    edge = 0.5 * longest
    t, out = alternately({"subdivide_to_size": lambda: mesh.subdivide_report(max_edge=edge)}, rounds)
    got, rep = out["subdivide_to_size"]
    g = got.faces.long()
    after = max(float((got.vertices[g[:, k]] - got.vertices[g[:, (k + 1) % 3]]).norm(dim=1).max()) for k in range(3))
    assert after <= edge
    case = {"case": "c: subdivide_to_size on the torus of 4096 faces, max_edge = half the longest edge", "vertices": int(verts.shape[0]),
            "faces": int(faces.shape[0]), "max_edge": edge, "rounds_run": rep.rounds, "edges_split_per_round": rep.n_marked,
            "vertices_after": int(got.vertices.shape[0]), "faces_after": int(got.faces.shape[0]), "longest_edge_after": after,
            "torch_form": "not written: the adaptive split has no torch formulation here, so this case has no comparison"}
    _record(case, t, [("subdivide_to_size", None)])
    print(json.dumps(case), file=sys.stderr, flush=True)
    return case


def loop_case(verts, faces, rounds):
    from vtaco_amd.conv_onet.generation import Mesh
    mesh = Mesh(verts, faces)
    t, out = alternately({"subdivide_loop": lambda: mesh.subdivide_loop(), "torch_subdivide_loop": lambda: torch_loop(verts, faces)}, rounds)
    got, (tv, tf) = out["subdivide_loop"], out["torch_subdivide_loop"]
    again = mesh.subdivide_loop()
    assert torch.equal(got.faces, tf) and torch.equal(got.vertices, again.vertices)
    diff = float((got.vertices.double() - tv.double()).abs().max())
    tol = 4 * float(verts.abs().max()) * (2.0 ** -23 if verts.dtype == torch.float32 else 2.0 ** -44)
    assert diff <= tol, (diff, tol)
    case = {"case": "d: Loop on the shipped scene's mesh at 128^3", "vertices": int(verts.shape[0]), "faces": int(faces.shape[0]),
            "vertices_after": int(tv.shape[0]), "faces_after": int(tf.shape[0]), "max_abs_diff_to_torch": diff, "kernel_runs_equal_bits": True}
    _record(case, t, [("subdivide_loop", "torch_subdivide_loop")])
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
        sys.exit("bench_mesh_subdivide: no HIP device")
    if args.wnf:
        return wnf_line(args.wnf, args.rounds)
    import mesh_topo_ref as T
    from vtaco_amd.conv_onet.generation import Generator3D
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds,
              "method": "candidates alternately in one process; host clock around a call that ends synchronised; per figure the median over "
                        "rounds and the spread (max - min) between rounds", "cases": []}
    wanted = args.cases.split(",")
    if "a" in wanted:
        v, f = (torch.from_numpy(x).to(dev) for x in hand_stand_in())
        result["cases"].append(midpoint_case("a: the hand stand-in (769 vertices, 1520 faces, a disk), 1 and 2 levels", v, f, args.rounds, levels=(1, 2)))
        result["cases"].append(layer_case(v, f, args.rounds))
    if "b" in wanted or "d" in wanted:
        model, cloud = scene(dev)
        mesh = Generator3D(model, device=dev, resolution0=32).generate_obj_mesh_wnf({"inputs": cloud})
        if "b" in wanted:
            result["cases"].append(midpoint_case("b: shipped scene, marching cubes at 128^3, one level", mesh.vertices, mesh.faces, args.rounds))
        if "d" in wanted:
            result["cases"].append(loop_case(mesh.vertices, mesh.faces, args.rounds))
    if "c" in wanted:
        v, f = T.torus(32, 64)
        result["cases"].append(to_size_case(torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev), args.rounds))
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
