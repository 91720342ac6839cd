"""The tactile feature encoder's TRAINING step (Resnet18, five 320 x 240 images per scene) on the HIP kernels (csrc/resnet2d_train.hip)
against the nn modules (MIOpen), both in ONE process and alternately, so that box-to-box and run-to-run drift falls on both alike.

    python tools/bench_resnet_train.py [--rounds 5] [--out profiles/resnet_train_bench.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d out/resnet_train_prof -o r -- python tools/bench_resnet_train.py --profile-run

What is timed:
  resnet      forward + backward + Adam of the Resnet18 alone (L1 against a fixed target through ``forward_scenes``) at S = 8 and S = 1
              scenes (wall clock, median of 5 after 2 warm-up calls per round)
  train_step  the step ``bench.py --full`` reports as ``train_step.ms_per_step`` (``bench_util.build_train_case``: the shipped VTacO
              model, 8 scenes x 2048 points, Adam), 8 steps after 3 warm-up steps per round
Every figure is taken ``--rounds`` times per path, host and hip in turn; reported: the median over rounds and the spread (max - min).
Also written: the largest difference between the two paths' losses and parameter gradients after one step at S = 8, the HIP path's
workspace bytes, and ``sources``: the hash of the kernel sources the numbers belong to (``bench.source_hash``).  ``gate`` applies the
rule for the knob's default: hip only if the S = 8 step of the Resnet18 on hip is below host by more than three times the larger
spread."""
from __future__ import annotations

import argparse
import copy
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KNOB = "VTACO_TACTILE_RESNET_TRAIN"
H, W, FN = 320, 240, 5
SOURCES = ("resnet2d_train.hip", "resnet2d_conv.h", "resnet2d.hip", "decode_common.h", "vt_common.h", "Makefile")


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


def _summary(vals):
    return {"median_ms": statistics.median(vals), "spread_ms": max(vals) - min(vals), "rounds": [round(v, 5) for v in vals]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resnet_train_bench.json"))
    ap.add_argument("--no-train-step", action="store_true", help="skip the whole VTacO training step")
    ap.add_argument("--profile-run", action="store_true", help="3 HIP training steps of the Resnet18 alone at S = 8 and nothing else (for rocprofv3)")
    args = ap.parse_args()
    import numpy as np
    import torch
    from torch.nn import functional as F
    import bench
    from vtaco_amd import _lib
    from vtaco_amd.encoder import encoder_dict
    dev = torch.device("cuda:0")
    torch.manual_seed(1)
    seed_net = encoder_dict["Resnet18"](num_classes=32).to(dev).train()

    def resnet_step(S):
        net = copy.deepcopy(seed_net)
        opt = torch.optim.Adam(net.parameters(), lr=1e-4)
        g = torch.Generator().manual_seed(5)
        imgs, target = torch.rand(S, FN, 3, H, W, generator=g).to(dev), torch.randn(S, FN, 32, generator=g).to(dev)

        def step():
            opt.zero_grad(set_to_none=True)
            F.l1_loss(net.forward_scenes(imgs), target).backward()
            opt.step()
        return step

    if args.profile_run:
        os.environ[KNOB] = "hip"
        step = resnet_step(8)
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        return
    rounds = max(5, args.rounds)
    paths = ("host", "hip")
    res = {"device": torch.cuda.get_device_name(0), "rounds_per_path": rounds, "shape": [FN, 3, H, W], "sources": bench.source_hash(SOURCES),
           "method": "host and hip alternately in one process; per figure the median over rounds and the spread (max - min) between rounds"}

    def each(fn):
        vals = {p: [] for p in paths}
        for _ in range(rounds):
            for p in paths:
                os.environ[KNOB] = p
                vals[p].append(fn())
        return {p: _summary(v) for p, v in vals.items()}

    for S in (8, 1):
        step = resnet_step(S)
        res[f"resnet18_fwd_bwd_adam_S{S}"] = each(lambda: _median_ms(step))
        del step
        torch.cuda.empty_cache()
    # ---- the two paths after one step from the same state (S = 8) ----------------------------------------------------------------------
    g = torch.Generator().manual_seed(5)
    imgs, target = torch.rand(8, FN, 3, H, W, generator=g).to(dev), torch.randn(8, FN, 32, generator=g).to(dev)
    out = {}
    for p in paths:
        os.environ[KNOB] = p
        net = copy.deepcopy(seed_net)
        loss = F.l1_loss(net.forward_scenes(imgs), target)
        loss.backward()
        out[p] = (float(loss.detach()), {n: q.grad.clone() for n, q in net.named_parameters()})
    res["hip_against_host_S8"] = {
        "loss_host": out["host"][0], "loss_hip": out["hip"][0], "loss_abs_diff": abs(out["host"][0] - out["hip"][0]),
        "grad_max_rel_l2_diff": max(float((out["hip"][1][n] - gr).norm() / gr.norm()) for n, gr in out["host"][1].items())}
    del imgs, target, out
    torch.cuda.empty_cache()
    lib = _lib.load()
    blocks = (ctypes.c_int32 * 4)(2, 2, 2, 2)
    res["workspace_bytes"] = {f"S{S}": int(lib.vt_resnet_train_workspace_bytes(blocks, 32, S * FN, S, H, W)) for S in (1, 8)}
    if not args.no_train_step:
        from vtaco_amd.bench_util import build_train_case
        model, trainer, batch, vf = build_train_case(dev, 0, scenes=8, pretrained_t2d=True)
        np.random.seed(1234)

        def steps(n=8, warm=3):
            for _ in range(warm):
                trainer.train_step(batch, vf)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                trainer.train_step(batch, vf)
            torch.cuda.synchronize()
            return 1e3 * (time.perf_counter() - t0) / n
        res["train_step_ms_per_step"] = each(steps)
    st = res["resnet18_fwd_bwd_adam_S8"]
    spread = max(st["host"]["spread_ms"], st["hip"]["spread_ms"])
    res["gate"] = {"S8_step_hip_below_host_by_more_than_3_spreads": st["hip"]["median_ms"] < st["host"]["median_ms"] - 3 * spread,
                   "S8_step_host_minus_hip_ms": st["host"]["median_ms"] - st["hip"]["median_ms"], "larger_spread_ms": spread}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
