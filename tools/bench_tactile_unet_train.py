"""The tactile depth estimator's TRAINING step (U-Net depth 3, 32 start filters, five 320 x 240 images per scene; the reference's
train_depth.py) on the HIP kernels (csrc/unet2d_train.hip) against the nn modules (MIOpen), both in ONE process and alternately, so
that box-to-box and run-to-run drift falls on both alike.

    python tools/bench_tactile_unet_train.py [--rounds 5] [--out profiles/tactile_unet_train_bench.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d out/tactile_unet_train_prof -o r -- python tools/bench_tactile_unet_train.py --profile-run

What is timed:
  step        one ``Trainer(train_tactile=True).train_step`` (forward, L1 loss, backward, Adam), the U-Net alone and with the digit-pose
              encoder, at S = 1 and S = 12 scenes (wall clock, median of 3 after 1 warm-up call per round)
  unet        the U-Net's forward + backward alone (L1 against a fixed target), timed by device events
Every figure is taken ``--rounds`` times per path, host and hip in turn; reported: the median over rounds and the spread (max - min).
Also written: the largest difference between the two paths' losses and parameter gradients after one step at the shipped shape, and the
HIP path's workspace bytes.  ``gate`` applies the rule for the knob's default: hip only if the S = 12 step on hip is below host by more
than three times the larger spread."""
from __future__ import annotations

import argparse
import copy
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KNOB = "VTACO_TACTILE_UNET_TRAIN"
H, W, FN = 320, 240, 5


def _median_ms(fn, n=3, warm=1):
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


def _event_ms(fn, n=3, warm=1):
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


def _scene_data(S, seed):
    import torch
    g = torch.Generator().manual_seed(seed)
    return {"inputs": torch.randn(S, 300, 3, generator=g) * 0.2, "inputs.img": torch.rand(S, FN, 3, H, W, generator=g),
            "inputs.depth": 0.019 + 0.003 * torch.rand(S, FN, H * W, generator=g), "points.cam_pos": torch.randn(S, FN, 3, generator=g) * 0.1,
            "points.cam_rot": torch.randn(S, FN, 3, generator=g)}


def _model(dev, with_digits):
    import torch
    from vtaco_amd.conv_onet.models import ConvolutionalOccupancyNetwork
    from vtaco_amd.encoder import encoder_dict
    torch.manual_seed(1)
    unet = encoder_dict["UNet"](num_classes=1, in_channels=3, depth=3, start_filts=32)
    digits = None
    if with_digits:
        digits = encoder_dict["pointnet_local_pool"](dim=3, c_dim=16, padding=0.1, hidden_dim=32, plane_type=["xz", "xy", "yz"],
                                                     plane_resolution=32, unet=False, out_mano=True, out_dim=30)
    return ConvolutionalOccupancyNetwork(None, None, digits, unet, None, device=dev).train()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tactile_unet_train_bench.json"))
    ap.add_argument("--profile-run", action="store_true", help="3 HIP training steps of the U-Net alone at S = 12 and nothing else (for rocprofv3)")
    args = ap.parse_args()
    import torch
    from torch.nn import functional as F
    from vtaco_amd import _lib
    from vtaco_amd.conv_onet.training import Trainer
    dev = torch.device("cuda:0")

    def trainer(S, with_digits):
        model = _model(dev, with_digits)
        data = {k: v.to(dev) for k, v in _scene_data(S, 2).items()}
        tr = Trainer(model, torch.optim.Adam(model.parameters(), lr=1e-4), device=dev, train_tactile=True)
        return lambda: tr.train_step(data)

    if args.profile_run:
        os.environ[KNOB] = "hip"
        step = trainer(12, False)
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        return
    rounds = max(5, args.rounds)
    paths = ("host", "hip")
    res = {"device": torch.cuda.get_device_name(0), "rounds_per_path": rounds, "shape": [FN, 3, H, W],
           "method": "host and hip alternately in one process; per figure the median over rounds and the spread (max - min) between rounds"}

    def each(fn):
        vals = {p: [] for p in paths}
        for _ in range(rounds):
            for p in paths:
                os.environ[KNOB] = p
                vals[p].append(fn())
        return {p: _summary(v) for p, v in vals.items()}

    for S in (1, 12):
        for with_digits in (False, True):
            step = trainer(S, with_digits)
            res[f"train_step_S{S}_{'unet_and_digit_pose' if with_digits else 'unet_only'}"] = each(lambda: _median_ms(step))
            del step
            torch.cuda.empty_cache()
    unet = _model(dev, False).encoder_img
    for S in (1, 12):
        g = torch.Generator().manual_seed(5)
        x, target = torch.rand(S * FN, 3, H, W, generator=g).to(dev), torch.rand(S * FN, 1, H, W, generator=g).to(dev)

        def fwd_bwd():
            unet.zero_grad(set_to_none=True)
            F.l1_loss(unet(x, scenes=S), target).backward()
        res[f"unet_fwd_bwd_S{S}_device_ms"] = each(lambda: _event_ms(fwd_bwd))
    # ---- the two paths after one step from the same state (S = 12) ---------------------------------------------------------------------
    out = {}
    for p in paths:
        os.environ[KNOB] = p
        net = copy.deepcopy(unet)
        net.zero_grad(set_to_none=True)
        loss = F.l1_loss(net(x, scenes=12), target)
        loss.backward()
        out[p] = (float(loss.detach()), {n: q.grad.clone() for n, q in net.named_parameters()})
    res["hip_against_host_S12"] = {
        "loss_host": out["host"][0], "loss_hip": out["hip"][0], "loss_abs_diff": abs(out["host"][0] - out["hip"][0]),
        "grad_max_abs_diff": max(float((out["hip"][1][n] - g).abs().max()) for n, g in out["host"][1].items()),
        "grad_max_rel_l2_diff": max(float((out["hip"][1][n] - g).norm() / g.norm()) for n, g in out["host"][1].items() if not n.endswith("conv1.bias") and not n.endswith("conv2.bias")),
        "note": "conv1.bias / conv2.bias (in front of a train-mode BatchNorm: a gradient of rounding noise) are left out of the relative figure"}
    lib = _lib.load()
    res["workspace_bytes"] = {f"S{S}": int(lib.vt_tactile_unet_train_workspace_bytes(3, 32, 3, 1, S * FN, FN, H, W)) for S in (1, 12)}
    st = res["train_step_S12_unet_only"]
    spread = max(st["host"]["spread_ms"], st["hip"]["spread_ms"])
    res["gate"] = {"S12_step_hip_below_host_by_more_than_3_spreads": st["hip"]["median_ms"] < st["host"]["median_ms"] - 3 * spread,
                   "S12_step_host_minus_hip_ms": st["host"]["median_ms"] - st["hip"]["median_ms"], "larger_spread_ms": spread}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
