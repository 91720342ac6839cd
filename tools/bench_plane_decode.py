#!/usr/bin/env python3
"""Times the plane route of the dense decode on one GPU and writes profiles/plane_decode_bench.json.

Shape: a 128^3 lattice, three 64^2 planes, c_dim 32, hidden 32 (one scene).  Measured, each as the median of ROUNDS rounds that alternate
the candidates inside one process, every timing a pair of device events around REPS back-to-back calls:
  - the sampler in table form and in point form on the materialised lattice points (the comparison that decides the lattice path),
    and the point kernel on coordinates generated in the kernel;
  - the conditioned MLP on the lattice's given features (f16x3 and f32);
  - the grid-only decode_lattice of the same widths (64^3 volume), from the same run.
The lattice goes through in slabs of LATTICE_SLAB_POINTS, as LocalDecoder.decode_lattice runs it.

    python tools/bench_plane_decode.py [--out profiles/plane_decode_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NX, R, C, BOX, ROUNDS, REPS = 128, 64, 32, 1.1, 5, 3


def timed(fn):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / REPS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "plane_decode_bench.json"))
    args = ap.parse_args()
    from vtaco_amd import ops
    from vtaco_amd.common import make_3d_grid
    from vtaco_amd.conv_onet.models import decoder as decmod
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    dec = decmod.LocalDecoder(dim=3, c_dim=C, hidden_size=32, n_blocks=5, padding=0.1).to(dev).eval()
    planes = {k: torch.randn(1, C, R, R, device=dev) for k in ("xz", "xy", "yz")}
    grid = torch.randn(1, C, 64, 64, 64, device=dev)
    total, slab = NX ** 3, decmod.LATTICE_SLAB_POINTS
    slabs = [(lo, min(slab, total - lo)) for lo in range(0, total, slab)]
    pts = (BOX * make_3d_grid((-0.5,) * 3, (0.5,) * 3, (NX,) * 3)).to(dev).unsqueeze(0)
    feat = torch.randn(1, slab, C, device=dev)

    def sampler(form):
        def run():
            for lo, n in slabs:
                if form == "points_materialised":
                    ops.planes.sample_planes(planes, pts[:, lo:lo + n], 0.1)
                else:
                    ops.planes.sample_planes(planes, None, 0.1, lattice=(NX, BOX, lo, n), lattice_form=form)
        return run

    def mlp(prec):
        blob = dec._blob(precision=prec)
        def run():
            for lo, n in slabs:
                ops.planes.decode_mlp_lattice(feat[:, :n], blob, (NX, BOX, lo, n), precision=prec)
        return run

    def whole(c, prec):
        return lambda: dec.decode_lattice(c, NX, box=BOX, precision=prec)

    with torch.no_grad():
        cands = {"sampler_table_ms": sampler("table"), "sampler_points_materialised_ms": sampler("points_materialised"),
                 "sampler_points_generated_ms": sampler("points"), "mlp_f16x3_ms": mlp("f16x3"), "mlp_f32_ms": mlp("f32"),
                 "plane_decode_lattice_f16x3_ms": whole(planes, "f16x3"), "grid_decode_lattice_f16x3_ms": whole(grid, "f16x3"),
                 "plane_decode_lattice_f32_ms": whole(planes, "f32"), "grid_decode_lattice_f32_ms": whole(grid, "f32")}
        # the two sampler forms give the same bits
        a = ops.planes.sample_planes(planes, None, 0.1, lattice=(NX, BOX, 5, 100000), lattice_form="table")
        assert torch.equal(a, ops.planes.sample_planes(planes, pts[:, 5:100005], 0.1))
        for fn in cands.values():                       # warm up every shape
            fn()
        rounds = {k: [] for k in cands}
        for _ in range(ROUNDS):
            for k, fn in cands.items():                 # alternating: one round times every candidate once
                rounds[k].append(timed(fn))
    res = {k: round(statistics.median(v), 4) for k, v in rounds.items()}
    res["spread"] = {k: [round(min(v), 4), round(max(v), 4)] for k, v in rounds.items()}
    chosen = "table" if res["sampler_table_ms"] <= res["sampler_points_materialised_ms"] else "points"
    round_trip_mb = 2 * total * C * 4 / 1e6
    res.update({"shape": {"lattice": NX, "planes": 3, "plane_resolution": R, "c_dim": C, "hidden": 32, "slab_points": slab},
                "device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "reps_per_timing": REPS,
                "chosen_lattice_form": chosen, "shipped_lattice_form": ops.planes.LATTICE_FORM,
                "feature_round_trip_mb": round(round_trip_mb, 1),
                "sampler_table_write_gbps": round(total * C * 4 / 1e6 / res["sampler_table_ms"], 1)})
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
