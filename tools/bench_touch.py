#!/usr/bin/env python3
"""Multi-touch session (conv_onet.inferencing.Inferencer) on the shipped tactile model sections (bench_util.build_tactile_scene:
VTacO / t2d and VTacOH), lattices 128^3 and 256^3, decode_precision "f16x3", a sequence of --touches touches of one object (the
scene's sample with the sensors / the wrist moved a little per touch, so later touches overlap earlier ones).

Per route and lattice: host wall time per ``add_touch`` (device drained before and after: a touch contains host reads), p50 over
--reps sequences after two warm-up sequences (graphs captured), for touch 0 and for the later touches, incremental and
``incremental=False``; the changed-point count of every later touch; and, measured in the same process right next to them, the
yardstick: ``Generator3D.generate_obj_mesh_wnf`` on the first touch's sample (the single-scene call a session replaces; unchanged
code) alone and followed by ``generate_hand_mesh`` (a touch returns both meshes).  Prints one JSON object; --out also writes it.

    python tools/bench_touch.py [--reps 7] [--touches 4] [--out profiles/touch_bench.json]
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


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def touches_of(data, variant, n):
    g = torch.Generator().manual_seed(9)
    out = []
    for k in range(n):
        d = dict(data)
        if variant == "vtaco":
            d["points.cam_pos"] = data["points.cam_pos"] + (0.004 * k) * torch.randn(1, 5, 3, generator=g).double()
            d["points.cam_rot"] = data["points.cam_rot"] + (0.02 * k) * torch.randn(1, 5, 3, generator=g).double()
        else:
            d["points.mano"] = data["points.mano"].clone()
            d["points.mano"][0, :3] += 0.02 * k * torch.tensor([1.0, 0.5, -0.5])
        out.append(d)
    return out


def p50(xs):
    return round(statistics.median(xs), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--touches", type=int, default=4)
    ap.add_argument("--out")
    args = ap.parse_args()
    from vtaco_amd.bench_util import build_tactile_scene
    from vtaco_amd.conv_onet.generation import Generator3D
    from vtaco_amd.conv_onet.inferencing import Inferencer
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "decode_precision": "f16x3", "reps": args.reps, "touches": args.touches,
              "timing": "host wall ms per call, device drained before and after; p50", "cases": []}
    for variant in ("vtaco", "vtacoh"):
        model, data, depth_origin = build_tactile_scene(dev, variant=variant)
        seq = touches_of(data, variant, args.touches)
        for r0 in (32, 64):
            gen = Generator3D(model, device=dev, resolution0=r0, padding=0.1, with_img=True, encode_t2d=variant == "vtaco",
                              depth_origin=depth_origin)
            case = {"route": variant, "nx": r0 * 4, "points": (r0 * 4) ** 3}
            for name, incremental in (("incremental", True), ("whole_lattice", False)):
                inf = Inferencer(model, None, gen, device=dev, with_img=True, encode_t2d=variant == "vtaco", incremental=incremental)
                first, later = [], []
                for rep in range(args.reps + 2):
                    np.random.seed(3)
                    inf.reset()
                    for k, d in enumerate(seq):
                        ms, _ = wall_ms(lambda: inf.add_touch(d))
                        if rep >= 2:
                            (first if k == 0 else later).append(ms)
                case[name] = {"touch0_ms": p50(first), "later_touch_ms": p50(later), "later_touch_min_ms": round(min(later), 4)}
                if incremental:
                    case["changed_points_per_touch"] = inf.changed_points[1:]
            own, both = [], []
            for rep in range(args.reps + 2):
                np.random.seed(3)
                ms, _ = wall_ms(lambda: gen.generate_obj_mesh_wnf(seq[0]))
                ms2, _ = wall_ms(lambda: gen.generate_hand_mesh(seq[0]))
                if rep >= 2:
                    own.append(ms)
                    both.append(ms + ms2)
            case["single_scene_generate_obj_mesh_wnf_ms"] = p50(own)
            case["single_scene_obj_plus_hand_mesh_ms"] = p50(both)
            case["later_touch_vs_single_scene"] = round(case["single_scene_obj_plus_hand_mesh_ms"] / case["incremental"]["later_touch_ms"], 2)
            result["cases"].append(case)
            print(json.dumps(case), flush=True)
            del gen
            torch.cuda.empty_cache()
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
