"""The tactile depth estimator (U-Net depth 3, 32 start filters, five 320 x 240 images per scene) on the HIP kernels (csrc/unet2d.hip)
against the nn modules (MIOpen), both in ONE process and alternately, so that box-to-box and run-to-run drift falls on both alike.

    python tools/bench_tactile_unet.py [--rounds 5] [--out profiles/tactile_unet_bench.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d out/tactile_unet_prof -o r -- python tools/bench_tactile_unet.py --profile-run

What is timed:
  stage       ``model.encode_t2d(inputs, imgs)`` of the shipped VTacO (t2d) model section in eval mode under no_grad, the way bench.py's
              generate_obj_mesh_wnf_t2d.encode_t2d_forward_ms takes it (wall clock, median of 5 after 2 warm-up calls per round); it
              includes the digit-pose encoder, which is the same work on both paths
  unet        the U-Net alone on 5 and on 40 images: eager calls timed by device events over 20 calls
  tactile_pc  ``Generator3D.generate_tactile_pc`` for one scene, end to end with the copy of the [1, 5, 76 800, 3] float64 result
Every figure is taken ``--rounds`` times per path, host and hip in turn; reported: the median over rounds and the spread (max - min).
FLOPs come from the layer shapes (work_per_image below), not from a counter."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KNOB = "VTACO_TACTILE_UNET"


def work_per_image(depth, sf, cin, classes, H, W):
    """[(layer, multiply-adds)] per image from the shapes."""
    rows = []
    for i in range(depth):
        c, px = sf << i, (H >> i) * (W >> i)
        rows.append((f"down{i}.conv1", px * c * (cin if i == 0 else c // 2) * 9))
        rows.append((f"down{i}.conv2", px * c * c * 9))
    for i in range(depth - 2, -1, -1):
        c, px = sf << i, (H >> i) * (W >> i)
        rows.append((f"up{i}.upconv", px * c * 2 * c))
        rows.append((f"up{i}.conv1", px * c * 2 * c * 9))
        rows.append((f"up{i}.conv2", px * c * c * 9))
    rows.append(("conv_final", H * W * classes * sf))
    return rows


def _median_ms(fn, n=5, warm=2):
    import torch
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return sorted(ts)[len(ts) // 2]


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tactile_unet_bench.json"))
    ap.add_argument("--profile-run", action="store_true", help="20 eager HIP forwards at the shipped shape and nothing else (for rocprofv3)")
    args = ap.parse_args()
    import torch
    from vtaco_amd.bench_util import build_tactile_scene
    from vtaco_amd.conv_onet.generation import Generator3D
    from vtaco_amd.conv_onet.models import ConvolutionalOccupancyNetwork
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    model, data, _ = build_tactile_scene(dev, "vtaco", "simple_local")
    model.eval()
    imgs, inputs = data["inputs.img"].to(dev), data["inputs"].to(dev)
    unet = model.encoder_t2d.encoder_img
    if args.profile_run:
        os.environ[KNOB] = "hip"
        for _ in range(20):
            unet(imgs[0])
        torch.cuda.synchronize()
        return
    rounds = max(5, args.rounds)
    paths = ("host", "hip")
    res = {"device": torch.cuda.get_device_name(0), "rounds_per_path": rounds, "shape": list(imgs.shape[1:]),
           "method": "host and hip alternately in one process; per figure the median over rounds and the spread (max - min) between rounds"}

    def each(fn):
        vals = {p: [] for p in paths}
        for _ in range(rounds):
            for p in paths:
                os.environ[KNOB] = p
                vals[p].append(fn())
        return {p: _summary(v) for p, v in vals.items()}

    res["stage_encode_t2d_5x320x240"] = each(lambda: _median_ms(lambda: model.encode_t2d(inputs, imgs)))
    x5 = imgs[0].contiguous()
    x40 = torch.rand(40, *x5.shape[1:], device=dev)
    res["unet_5_images_device_ms"] = each(lambda: _event_ms(lambda: unet(x5)))
    res["unet_40_images_device_ms"] = each(lambda: _event_ms(lambda: unet(x40)))
    # ---- generate_tactile_pc for one scene --------------------------------------------------------------------------------------------
    g = torch.Generator().manual_seed(3)
    pc_model = ConvolutionalOccupancyNetwork(None, None, None, unet, None, device=dev).eval()
    gen = Generator3D(pc_model, device=dev, with_img=True)
    scene = {"inputs.img": imgs, "inputs.pc_ply": torch.randn(1, 400, 3, generator=g) * 0.15, "points.name": ["scene"],
             "points.cam_pos": torch.randn(1, 5, 3, generator=g) * 0.12, "points.cam_rot": torch.randn(1, 5, 3, generator=g) * 0.8}
    res["generate_tactile_pc_one_scene"] = each(lambda: _median_ms(lambda: gen.generate_tactile_pc(scene)))
    # ---- work from the shapes -----------------------------------------------------------------------------------------------------
    rows = work_per_image(unet.depth, unet.start_filts, unet.in_channels, unet.num_classes, x5.shape[2], x5.shape[3])
    macs = sum(r[1] for r in rows)
    res["work"] = {"multiply_adds_per_image": macs, "gflop_per_scene": 2 * 5 * macs * 1e-9, "per_layer_multiply_adds": dict(rows),
                   "f32_matrix_peak_tflops": 157.0, "floor_ms_exact_f32": 2 * 5 * macs / 157e12 * 1e3}
    res["work"]["share_of_f32_matrix_peak_whole_forward"] = res["work"]["floor_ms_exact_f32"] / res["unet_5_images_device_ms"]["hip"]["median_ms"]
    st = res["stage_encode_t2d_5x320x240"]
    spread = max(st["host"]["spread_ms"], st["hip"]["spread_ms"])
    res["gate"] = {"stage_hip_below_host_by_more_than_spread": st["hip"]["median_ms"] < st["host"]["median_ms"] - spread,
                   "stage_host_minus_hip_ms": st["host"]["median_ms"] - st["hip"]["median_ms"], "spread_ms": spread}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
