"""The voxel encoder's front end (conv_in + ReLU + scatter-mean) on the fused HIP kernels (csrc/voxel_encoder.hip) against the host
composition (nn.Conv3d through MIOpen + the point encoders' sort and scatter-mean kernels on the generated voxel coordinates), both in
ONE process and alternately, so that box-to-box and run-to-run drift falls on both alike.

    python tools/bench_voxel_encoder.py [--rounds 5] [--out profiles/voxel_encoder_bench.json]

What is timed, C = 32, one scene, no U-Net behind it (the U-Nets are the same launches on either side):
  grid      a 32^3 volume -> the 32^3 feature grid         LocalVoxelEncoder.forward, inference
  planes    a 64^3 volume -> the xz, xy, yz planes at 64^2  LocalVoxelEncoder.forward, inference
  train     the same two with forward + backward to conv_in's gradients under autograd
Device time by events over 20 calls after 3 warm-up calls, taken ``--rounds`` times per path, host and hip in turn; reported: the
median over rounds and the spread (max - min).  ``default``: the side that is faster by more than the spread on both inference
shapes; VTACO_VOXEL_ENCODER's default in vtaco_amd/encoder/voxels.py follows this file's committed run."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _event_ms(fn, n=20, warm=3):
    import torch
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def _summary(vals):
    return {"median_ms": statistics.median(vals), "spread_ms": max(vals) - min(vals), "rounds": [round(v, 5) for v in vals]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxel_encoder_bench.json"))
    args = ap.parse_args()
    import torch
    from vtaco_amd.encoder import encoder_dict
    dev = torch.device("cuda:0")
    rounds = max(5, args.rounds)
    paths = ("host", "hip")
    res = {"device": torch.cuda.get_device_name(0), "rounds_per_path": rounds, "c_dim": 32,
           "method": "host and hip alternately in one process; device time by events over 20 calls; per figure the median over rounds "
                     "and the spread (max - min) between rounds"}
    shapes = {"grid_32_to_32": (32, dict(plane_type="grid", grid_resolution=32)),
              "planes_64_to_3x64": (64, dict(plane_type=["xz", "xy", "yz"], plane_resolution=64))}
    for name, (D, kw) in shapes.items():
        torch.manual_seed(0)
        enc = encoder_dict["voxel_simple_local"](c_dim=32, **kw).to(dev).eval()
        x = (torch.rand(1, D, D, D, generator=torch.Generator().manual_seed(1)) < 0.3).float().to(dev)

        def infer():
            with torch.no_grad():
                enc(x)

        def train():
            enc.zero_grad(set_to_none=True)
            sum(v.sum() for v in enc(x).values()).backward()
        for what, fn in (("inference", infer), ("train", train)):
            vals = {p: [] for p in paths}
            for _ in range(rounds):
                for p in paths:
                    enc.voxel_encoder = p
                    vals[p].append(_event_ms(fn))
            res[f"{name}_{what}_device_ms"] = {p: _summary(v) for p, v in vals.items()}
    wins = {"hip": 0, "host": 0}
    for name in shapes:
        r = res[f"{name}_inference_device_ms"]
        spread = max(r["host"]["spread_ms"], r["hip"]["spread_ms"])
        if r["hip"]["median_ms"] < r["host"]["median_ms"] - spread:
            wins["hip"] += 1
        elif r["host"]["median_ms"] < r["hip"]["median_ms"] - spread:
            wins["host"] += 1
    res["default"] = "hip" if wins["hip"] == len(shapes) else "host" if wins["host"] == len(shapes) else "undecided"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
