"""The Bottleneck tactile encoders (Resnet50 / Resnet101, 320 x 240 images) on the HIP kernels (csrc/resnet2d_bneck.hip) against the nn
modules (MIOpen), both in ONE process and alternately, so that box-to-box and run-to-run drift falls on both alike.

    python tools/bench_resnet_bneck.py [--rounds 5] [--out profiles/resnet_bneck_bench.json]
    rocprofv3 --kernel-trace --stats -d out/resnet_bneck_prof -o r -- python tools/bench_resnet_bneck.py --profile-run

What is timed:
  stage      ``gen._replay("encode_img", [imgs], model.encode_img_inputs)`` of the VTacOH model section with ``encoder_img`` a Resnet50 (a
             graph replay; median of 7 after 2 warm-up calls per round)
  eager      device time of an eager module call by device events over 20 calls: Resnet50 at 5 and at 40 images, Resnet101 at 5
Every figure is taken ``--rounds`` times per path, host and hip in turn; reported: the median over rounds and the spread (max - min).
FLOPs come from the layer shapes (work_per_image below), not from a counter."""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_resnet import _event_ms, _median_ms, _summary          # noqa: E402

KNOB = "VTACO_TACTILE_BOTTLENECK"
PEAK_SPEC_TFLOPS, PEAK_MEASURED_TFLOPS = 157.3, 155.0             # exact-f32 matrix rate of the MI355X: data sheet, and as measured


def work_per_image(blocks, H, W, classes=32):
    """[(layer, multiply-adds)] per image from the shapes: stem, conv1 / conv2 / conv3 (+ projection) of every block, tail."""
    up = lambda v: (v - 1) // 2 + 1
    hs, ws = up(H), up(W)
    h, w = up(hs), up(ws)
    rows = [("stem", hs * ws * 64 * 147)]
    cin = 64
    for s, nb in enumerate(blocks):
        c = 64 << s
        for b in range(nb):
            name = f"layer{s + 1}.{b}"
            rows.append((name + ".conv1", h * w * c * cin))
            if s > 0 and b == 0:
                h, w = up(h), up(w)
            rows.append((name + ".conv2", h * w * c * c * 9))
            rows.append((name + ".conv3", h * w * 4 * c * (c + (cin if b == 0 else 0))))
            cin = 4 * c
    rows.append(("tail", h * w * 2048 + 2048 * 100 + 100 * classes))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resnet_bneck_bench.json"))
    ap.add_argument("--profile-run", action="store_true", help="20 eager HIP forwards of Resnet50 at five images and nothing else (for rocprofv3)")
    args = ap.parse_args()
    import torch
    from vtaco_amd import layers
    from vtaco_amd.bench_util import build_tactile_scene
    from vtaco_amd.conv_onet.generation import Generator3D
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    model, data, _ = build_tactile_scene(dev, "vtacoh", "simple_local")
    torch.manual_seed(0)
    model.encoder_img = layers.Resnet50(num_classes=32).to(dev)
    model.eval()
    imgs = data["inputs.img"].to(dev)
    if args.profile_run:
        os.environ[KNOB] = "hip"
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
            os.environ[KNOB] = p
            fns[p] = make(p)
        vals = {p: [] for p in paths}
        for _ in range(rounds):
            for p in paths:
                os.environ[KNOB] = p
                vals[p].append(fns[p]())
        return {p: _summary(v) for p, v in vals.items()}

    def stage(path):
        gen = Generator3D(model, device=dev, resolution0=64, padding=0.1, with_img=True, encode_t2d=False)
        return lambda: _median_ms(lambda: gen._replay("encode_img", [data["inputs.img"]], model.encode_img_inputs))
    res["resnet50_stage_5x320x240_graph_replay"] = each(stage)
    x40 = torch.rand(8, 5, 3, 320, 240, device=dev)
    r50, r101 = model.encoder_img, layers.Resnet101(num_classes=32).to(dev).eval()
    res["resnet50_eager_5_images_device_ms"] = each(lambda p: (lambda: _event_ms(lambda: r50(imgs[0]))))
    res["resnet50_eager_40_images_device_ms"] = each(lambda p: (lambda: _event_ms(lambda: r50(x40.view(40, 3, 320, 240)))))
    res["resnet101_eager_5_images_device_ms"] = each(lambda p: (lambda: _event_ms(lambda: r101(imgs[0]))))
    res["work"] = {"f32_matrix_peak_tflops_spec": PEAK_SPEC_TFLOPS, "f32_matrix_peak_tflops_measured": PEAK_MEASURED_TFLOPS}
    for key, blocks, n in (("resnet50_eager_5_images_device_ms", (3, 4, 6, 3), 5), ("resnet50_eager_40_images_device_ms", (3, 4, 6, 3), 40),
                           ("resnet101_eager_5_images_device_ms", (3, 4, 23, 3), 5)):
        flop = 2 * n * sum(r[1] for r in work_per_image(blocks, 320, 240))
        hip_ms = res[key]["hip"]["median_ms"]
        res["work"][key] = {"gflop": flop * 1e-9, "hip_tflops": flop / hip_ms * 1e-9,
                            "share_of_spec_peak": flop / hip_ms * 1e-9 / PEAK_SPEC_TFLOPS,
                            "share_of_measured_peak": flop / hip_ms * 1e-9 / PEAK_MEASURED_TFLOPS,
                            "hip_over_host": hip_ms / res[key]["host"]["median_ms"]}
    st = res["resnet50_stage_5x320x240_graph_replay"]
    spread = max(st["host"]["spread_ms"], st["hip"]["spread_ms"])
    res["default"] = {"knob": KNOB, "hip_beats_host_at_five_images": st["hip"]["median_ms"] < st["host"]["median_ms"],
                      "by_more_than_spread": st["hip"]["median_ms"] < st["host"]["median_ms"] - spread}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
