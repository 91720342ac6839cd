#!/usr/bin/env python3
"""Time of ``VoxelGrid.from_mesh`` (vtaco_amd/utils/voxels.py on csrc/voxelize.hip) for method 'ray' and 'fill' at 64^3, 128^3 and 256^3,
against ``voxelize_interior(rule='winding')`` (the exact winding number, O(voxels x faces)) in the same process and alternately, on

  torus   a 64 x 32 torus, 4 096 faces, watertight (tests/voxelize_ref.py)
  scene   the marching-cubes mesh of the shipped scene (BASELINE config 2: tests/config2_case.py, 129^3 lattice, decode "f16x3"); the
          isosurface of seeded weights is open where it meets the lattice's boundary, so parity and winding need not agree on it

Per (mesh, resolution): host-clock ms around the call, which ends synchronised (from_mesh reads the bounds and the fill's flag back), as
the median over --rounds rounds that time every candidate once, with the spread (max - min); the occupied counts; the voxels on which
parity and winding disagree; the parity / winding time ratio.  The winding number is skipped where voxels x faces exceeds
--winding-max (it is written as null).  Prints one JSON object; --out also writes it.

    python tools/bench_voxelize.py [--rounds 5] [--out profiles/voxelize_bench.json]
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

RESOLUTIONS = (64, 128, 256)


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
    return mesh[0].float().contiguous(), mesh[1].contiguous()


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--winding-max", type=float, default=3e11, help="skip the winding number above this many voxel x face pairs")
    ap.add_argument("--meshes", default="torus,scene")
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_voxelize: no HIP device")
    import voxelize_ref as R
    from vtaco_amd.utils import voxels
    from vtaco_amd.utils.voxels import VoxelGrid
    dev = torch.device("cuda:0")
    meshes = {}
    if "torus" in args.meshes:
        v, f = R.torus(64, 32)
        meshes["torus"] = (torch.from_numpy(R.rotate(v, 5)).to(dev), torch.from_numpy(f).to(dev))
    if "scene" in args.meshes:
        meshes["scene"] = scene_mesh(dev)
    result = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "winding_max_pairs": args.winding_max,
              "method": "candidates alternately in one process; host clock around a call that ends synchronised; per figure the median over "
                        "rounds and the spread (max - min) between rounds", "cases": []}
    for name, (v, f) in meshes.items():
        # the frame from_mesh would choose, applied once, so that the winding rule sees the same unit-frame mesh
        lo, hi = v.double().min(0).values, v.double().max(0).values
        unit = (((v.double() - (lo + hi) / 2) / ((hi - lo).max() / 0.9)).float().contiguous(), f)
        for res in RESOLUTIONS:
            cands = {"ray": lambda: VoxelGrid.from_mesh((v, f), res, method="ray").data,
                     "fill": lambda: VoxelGrid.from_mesh((v, f), res, method="fill").data,
                     "parity_interior": lambda: voxels.voxelize_interior(unit, res),
                     "surface": lambda: voxels.voxelize_surface(unit, res)}
            if float(res) ** 3 * f.shape[0] <= args.winding_max:
                cands["winding_interior"] = lambda: voxels.voxelize_interior(unit, res, rule="winding")
            out = {k: fn() for k, fn in cands.items()}                       # warm-up: every shape once
            times = {k: [] for k in cands}
            for _ in range(args.rounds):
                for k, fn in cands.items():                                 # alternating: one round times every candidate once
                    times[k].append(timed(fn)[0])
            case = {"mesh": name, "faces": int(f.shape[0]), "vertices": int(v.shape[0]), "res": res,
                    "occupied": {k: int(o.sum()) for k, o in out.items()}}
            for k in ("ray", "fill", "parity_interior", "surface", "winding_interior"):
                case[k + "_ms"] = round(statistics.median(times[k]), 4) if k in times else None
                case[k + "_spread_ms"] = round(max(times[k]) - min(times[k]), 4) if k in times else None
            if "winding_interior" in out:
                case["parity_winding_mismatch"] = int((out["parity_interior"] != out["winding_interior"]).sum())
                case["parity_over_winding_time"] = round(case["parity_interior_ms"] / case["winding_interior_ms"], 5)
                case["winding_over_parity_time"] = round(case["winding_interior_ms"] / case["parity_interior_ms"], 2)
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
