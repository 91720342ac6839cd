"""The tactile feature encoder (Resnet18, five 320 x 240 images per scene) on the HIP kernels (csrc/resnet2d.hip) against the nn modules
(MIOpen), both in ONE process and alternately, so that box-to-box and run-to-run drift falls on both alike.

    python tools/bench_resnet.py [--rounds 5] [--out profiles/resnet_bench.json]
    rocprofv3 --kernel-trace --stats -d out/resnet_prof -o r -- python tools/bench_resnet.py --profile-run     (per-kernel times)

What is timed:
  stage      ``gen._replay("encode_img", [imgs], model.encode_img_inputs)`` of the shipped VTacOH model section, the way bench.py's
             config5.setup_stage_ms.resnet18_tactile_features takes it (a graph replay; median of 7 after 2 warm-up calls per round)
  40 images  the config-4 batch (8 scenes x 5), and Resnet34 at 5 images: eager module calls timed by device events over 20 calls
  routes     generate_obj_mesh_wnf end to end, config 3 (VTacO, encode_t2d, 128^3) and config 5 (VTacOH, 256^3)
Every figure is taken ``--rounds`` times per path, host and hip in turn; reported: the median over rounds and the spread (max - min).
FLOPs and bytes come from the layer shapes (work_per_image below), not from a counter."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def work_per_image(blocks, H, W, classes=32):
    """[(layer, multiply-adds, bytes read + written)] per image from the shapes: stem, every 3x3 conv (+ its 1x1 projection), tail."""
    up = lambda v: (v - 1) // 2 + 1
    hs, ws = up(H), up(W)
    h, w = up(hs), up(ws)
    rows = [("stem", hs * ws * 64 * 147, 4 * (3 * H * W + 64 * 147 + h * w * 64))]
    cin = 64
    for s, nb in enumerate(blocks):
        c = 64 << s
        for b in range(nb):
            if s > 0 and b == 0:
                h, w = up(h), up(w)
            px = h * w
            proj = s > 0 and b == 0
            rows.append((f"layer{s + 1}.{b}.conv1", px * c * (cin * 9 + (cin if proj else 0)),
                         4 * (px * (4 if proj else 1) * cin + c * cin * (10 if proj else 9) + px * c * (2 if proj else 1))))
            rows.append((f"layer{s + 1}.{b}.conv2", px * c * c * 9, 4 * (px * c + c * c * 9 + 2 * px * c)))
            cin = c
    rows.append(("tail", h * w * 512 + 512 * 100 + 100 * classes, 4 * (h * w * 512 + 512 * 100 + 100 * classes)))
    return rows


def _median_ms(fn, n=7, warm=2):
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resnet_bench.json"))
    ap.add_argument("--profile-run", action="store_true", help="20 eager HIP forwards at the shipped shape and nothing else (for rocprofv3)")
    ap.add_argument("--no-routes", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    from vtaco_amd.bench_util import build_tactile_scene
    from vtaco_amd.conv_onet.generation import Generator3D
    from vtaco_amd.encoder import encoder_dict
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    model, data, _ = build_tactile_scene(dev, "vtacoh", "simple_local")
    model.eval()
    imgs = data["inputs.img"].to(dev)
    if args.profile_run:
        os.environ["VTACO_TACTILE_RESNET"] = "hip"
        for _ in range(20):
            model.encode_img_inputs(imgs)
        torch.cuda.synchronize()
        return
    rounds = max(5, args.rounds)
    paths = ("host", "hip")
    res = {"device": torch.cuda.get_device_name(0), "rounds_per_path": rounds, "shape": list(imgs.shape[1:]),
           "method": "host and hip alternately in one process; per figure the median over rounds and the spread (max - min) between rounds"}

    def each(make):
        """make(path) -> a timing closure, built once per path with the knob set; then the paths in turn, `rounds` times."""
        fns = {}
        for p in paths:
            os.environ["VTACO_TACTILE_RESNET"] = p
            fns[p] = make(p)
        vals = {p: [] for p in paths}
        for _ in range(rounds):
            for p in paths:
                os.environ["VTACO_TACTILE_RESNET"] = p
                vals[p].append(fns[p]())
        return {p: _summary(v) for p, v in vals.items()}

    # ---- the stage, as bench.py takes it -------------------------------------------------------------------------------------------
    def stage(path):
        gen = Generator3D(model, device=dev, resolution0=64, padding=0.1, with_img=True, encode_t2d=False)
        return lambda: _median_ms(lambda: gen._replay("encode_img", [data["inputs.img"]], model.encode_img_inputs))
    res["stage_5x320x240_graph_replay"] = each(stage)
    # ---- eager, device time: 5 and 40 images, Resnet34 ------------------------------------------------------------------------------
    x40 = torch.rand(8, 5, 3, 320, 240, device=dev)
    res["eager_5_images_device_ms"] = each(lambda p: (lambda: _event_ms(lambda: model.encode_img_inputs(imgs))))
    res["eager_40_images_device_ms"] = each(lambda p: (lambda: _event_ms(lambda: model.encode_img_inputs(x40))))
    r34 = encoder_dict["Resnet34"](num_classes=32).to(dev).eval()
    res["resnet34_5_images_device_ms"] = each(lambda p: (lambda: _event_ms(lambda: r34(imgs[0]))))
    # ---- work from the shapes ---------------------------------------------------------------------------------------------------
    rows = work_per_image((2, 2, 2, 2), 320, 240)
    macs = sum(r[1] for r in rows)
    res["work"] = {"multiply_adds_per_image": macs, "gflop_per_scene": 2 * 5 * macs * 1e-9,
                   "bytes_per_scene_min": 5 * sum(r[2] for r in rows),
                   "per_layer_multiply_adds": {r[0]: r[1] for r in rows},
                   "f32_matrix_peak_tflops": 157.0,
                   "floor_ms_exact_f32": 2 * 5 * macs / 157e12 * 1e3}
    hip_ms = res["eager_5_images_device_ms"]["hip"]["median_ms"]
    res["work"]["share_of_f32_matrix_peak_whole_forward"] = res["work"]["floor_ms_exact_f32"] / hip_ms
    # ---- the routes end to end ------------------------------------------------------------------------------------------------------
    if not args.no_routes:
        def route(variant, nx):
            m, d, origin = build_tactile_scene(dev, variant, "simple_local")

            def make(path):
                gen = Generator3D(m, device=dev, resolution0=nx // 4, padding=0.1, with_img=True, encode_t2d=variant == "vtaco",
                                  depth_origin=origin)

                def call():
                    np.random.seed(11)
                    gen.generate_obj_mesh_wnf(d)
                return lambda: _median_ms(call)
            return each(make)
        res["config3_vtaco_t2d_128_end_to_end"] = route("vtaco", 128)
        res["config5_vtacoh_256_end_to_end"] = route("vtacoh", 256)
    st = res["stage_5x320x240_graph_replay"]
    spread = max(st["host"]["spread_ms"], st["hip"]["spread_ms"])
    res["gate"] = {"stage_hip_below_host_by_more_than_spread": st["hip"]["median_ms"] < st["host"]["median_ms"] - spread}
    for k in ("config3_vtaco_t2d_128_end_to_end", "config5_vtacoh_256_end_to_end"):
        if k in res:
            sp = max(res[k]["host"]["spread_ms"], res[k]["hip"]["spread_ms"])
            res["gate"][k + "_not_above_host_by_more_than_spread"] = res[k]["hip"]["median_ms"] <= res[k]["host"]["median_ms"] + sp
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
