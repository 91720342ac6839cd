#!/usr/bin/env python3
"""Time of ray casting through the face octree (csrc/ray_mesh.hip: ``ops.rays.ray_tree_query`` over ``ops.metrics.closest_point_tree_build``)
against the brute-force kernel (``ops.rays.ray_mesh(method='brute')``) on the meshes of tools/bench_closest_point.py:

  images_scene    five 320 x 240 sensor images (384 000 coherent rays) against the marching-cubes mesh of the shipped scene (129^3 lattice)
  images_torus    the same five images against a 64 x 32 torus, 4 096 faces
  scattered_*     100 000 rays with random origins in the frame and random directions against both meshes
  training        five 320 x 240 images against a 24 x 12 torus, 576 faces: the size of a training-time mesh
  render_depth    ``utils.render.render_depth`` end to end (pose records on the host, camera, query, depth) on the torus, both methods
  sweep           tori of 576 .. 262 144 faces x the five images and x 100 000 scattered rays: where the tree starts to win

Per candidate: host-clock ms around the call, which ends synchronised, as the median over --rounds rounds that time every candidate once
each, alternately, in one process, with the spread (max - min) between rounds.  The tree's build (the octree and the side buffer, with their
host reads) and its query are timed separately; ``tree_total`` is a call that does both.  Per case also the mean boxes and faces tested per
ray, and the query under each walk (VTACO_RAY_TREE_WALK: plain, order).  Every tree result is compared with the brute-force one for equal
bits where that ran.  Nothing is gated on these times.  Prints one JSON object; --out also writes it.

    python tools/bench_ray_mesh.py [--rounds 5] [--out profiles/ray_mesh_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_closest_point_tree import put, race          # noqa: E402

WALKS = ("plain", "order")
H, W = 240, 320


def aimed_poses(v, n, seed):
    """n sensor poses (cam_pos, cam_rot) whose camera axis passes through a vertex of the mesh, 0.6 .. 0.9 of its extent away."""
    from vtaco_amd.common import sensor_pose_inverse
    rng = np.random.RandomState(seed)
    lo, hi = v.min(0).values.cpu().numpy().astype(np.float64), v.max(0).values.cpu().numpy().astype(np.float64)
    rot = rng.uniform(-np.pi, np.pi, size=(n, 3))
    target = v[torch.from_numpy(rng.randint(v.shape[0], size=n)).to(v.device)].cpu().numpy().astype(np.float64)
    pos = np.zeros((n, 3))
    for i in range(n):
        axis = sensor_pose_inverse(np.zeros(3), rot[i])[0][:, 0]
        pos[i] = target[i] - rng.uniform(0.6, 0.9) * (hi - lo).max() * axis / np.linalg.norm(axis)
    return pos, rot


def image_rays(v, seed=3):
    from vtaco_amd import ops
    from vtaco_amd.utils import render
    pos, rot = aimed_poses(v, 5, seed)
    o, d = ops.rays.camera_rays(torch.from_numpy(render.pose_records(pos, rot)).to(v.device), W, H)
    return o, d.view(-1, 3).contiguous(), H * W


def scattered_rays(v, n, seed):
    rng = np.random.RandomState(seed)
    lo, hi = v.min(0).values.cpu().numpy().astype(np.float64), v.max(0).values.cpu().numpy().astype(np.float64)
    o = lo - 0.1 * (hi - lo) + 1.2 * (hi - lo) * rng.rand(n, 3)
    return torch.from_numpy(o).to(v.device), torch.from_numpy(rng.randn(n, 3)).to(v.device), None


def ray_case(name, v, f, rays, rounds, brute_pairs, walks=True):
    from vtaco_amd import ops
    o, d, per = rays
    N, F = int(d.shape[0]), int(f.shape[0])
    case = {"case": name, "rays": N, "faces": F, "pairs": N * F}
    ct = ops.metrics.closest_point_tree_build(v, f)
    case["depth"], case["leaves"] = ct.tree.depth, ct.tree.counts[ct.tree.depth]
    os.environ.pop("VTACO_RAY_TREE_WALK", None)
    cands = {"tree_build": lambda: ops.metrics.closest_point_tree_build(v, f),
             "tree_query": lambda: ops.rays.ray_tree_query(ct, o, d, rays_per_origin=per),
             "tree_total": lambda: ops.rays.ray_mesh(v, f, o, d, method='tree', rays_per_origin=per)}
    if N * F <= brute_pairs:
        cands["brute"] = lambda: ops.rays.ray_mesh(v, f, o, d, method='brute', rays_per_origin=per)
    else:
        case["brute"] = f"skipped: {N * F:.3g} pairs"
    res, out = race(cands, rounds)
    put(case, res)
    case["hits"] = int((out["tree_query"][1] >= 0).sum())
    if "brute" in cands:
        case["equal_bits"] = bool(torch.equal(out["brute"][0].view(torch.int64), out["tree_query"][0].view(torch.int64))
                                  and torch.equal(out["brute"][1], out["tree_query"][1]))
        case["brute_over_tree_query"] = round(case["brute_ms"] / case["tree_query_ms"], 2)
        case["brute_over_tree_total"] = round(case["brute_ms"] / case["tree_total_ms"], 2)
    if walks:
        def with_walk(w):                                                  # (the environment is read at every launch: set it per call)
            def run():
                os.environ["VTACO_RAY_TREE_WALK"] = w
                return ops.rays.ray_tree_query(ct, o, d, rays_per_origin=per)
            return run
        res, _ = race({w: with_walk(w) for w in WALKS}, rounds)
        case["walks"] = {}
        for w in WALKS:
            os.environ["VTACO_RAY_TREE_WALK"] = w
            st = ops.rays.ray_tree_query(ct, o, d, rays_per_origin=per, stats=True)[2].double().mean(0)
            case["walks"][w] = {"query_ms": res[w][0], "spread_ms": res[w][1], "boxes_per_ray": round(float(st[0]), 1),
                                "faces_per_ray": round(float(st[1]), 1)}
        os.environ.pop("VTACO_RAY_TREE_WALK", None)
    print(json.dumps(case), file=sys.stderr, flush=True)
    return case


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--brute-pairs", type=float, default=1e12, help="brute force runs only up to this many (ray, face) pairs")
    ap.add_argument("--cases", default="images_scene,images_torus,scattered,training,render_depth,sweep")
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_ray_mesh: no HIP device")
    import closest_point_ref as R
    from vtaco_amd.utils import render
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "brute_pairs_limit": args.brute_pairs,
              "method": "candidates alternately in one process; host clock around a call that ends synchronised; per figure the median over "
                        "rounds and the spread (max - min) between rounds", "cases": []}

    def torus(nu, nv):
        tv, tf = R.torus(nu, nv, seed=5)
        return torch.from_numpy(tv).to(dev), torch.from_numpy(tf).to(dev)
    scene = None
    if "images_scene" in args.cases or "scattered" in args.cases:
        from bench_closest_point import scene_mesh
        scene = scene_mesh(dev)
    if "images_scene" in args.cases:
        result["cases"].append(ray_case("images_scene", *scene, image_rays(scene[0]), args.rounds, args.brute_pairs))
    if "images_torus" in args.cases:
        v, f = torus(64, 32)
        result["cases"].append(ray_case("images_torus", v, f, image_rays(v), args.rounds, args.brute_pairs))
    if "scattered" in args.cases:
        v, f = torus(64, 32)
        result["cases"].append(ray_case("scattered_scene", *scene, scattered_rays(scene[0], 100000, 1), args.rounds, args.brute_pairs))
        result["cases"].append(ray_case("scattered_torus", v, f, scattered_rays(v, 100000, 2), args.rounds, args.brute_pairs))
    if "training" in args.cases:
        v, f = torus(24, 12)
        result["cases"].append(ray_case("training", v, f, image_rays(v), args.rounds, args.brute_pairs))
    if "render_depth" in args.cases:
        v, f = torus(64, 32)
        pos, rot = aimed_poses(v, 5, 3)
        case = {"case": "render_depth", "faces": int(f.shape[0]), "images": 5, "height": H, "width": W}
        res, out = race({m: (lambda m=m: render.render_depth((v, f), pos, rot, method=m)) for m in ("brute", "tree")}, args.rounds)
        put(case, res)
        case["equal_bits"] = bool(torch.equal(out["brute"][0].view(torch.int32), out["tree"][0].view(torch.int32)) and torch.equal(out["brute"][1], out["tree"][1]))
        result["cases"].append(case)
        print(json.dumps(case), file=sys.stderr, flush=True)
    if "sweep" in args.cases:
        rows = []
        for nu, nv in ((24, 12), (32, 16), (48, 24), (64, 32), (128, 64), (256, 128), (512, 256)):
            v, f = torus(nu, nv)
            for kind, rays in (("images", image_rays(v)), ("scattered", scattered_rays(v, 100000, 4))):
                row = ray_case(f"sweep_{kind}_{2 * nu * nv}", v, f, rays, args.rounds, args.brute_pairs, walks=False)
                rows.append(row)
        result["cases"].append({"case": "sweep", "mesh": "torus(nu, nu / 2)", "rows": rows})
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
