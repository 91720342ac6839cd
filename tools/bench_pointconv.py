"""The PointConv baseline (pointnet_plus_plus encoder + simple_local_point decoder) on the HIP kernels of csrc/pointnetpp.hip and
csrc/point_sample.hip against their torch-op restatement (vtaco_amd/pointconv_host.py, what VTACO_POINTCONV=host runs), both in ONE
process and alternately, so that box-to-box and run-to-run drift falls on both alike.

    python tools/bench_pointconv.py [--rounds 5] [--out profiles/pointconv_bench.json]

What is timed, one scene with a 3 000-point cloud, at c_dim / hidden_size 32 / 32 and at the class defaults 128 / 256:
  stages    fps 3000 -> 512 and 512 -> 128, the two ball queries, the 3-NN weights of fp1 (3000 targets, 512 sources), the sampler on
            2 048 queries forward and forward + backward, the sampler on the 128^3 lattice, the conditioned MLP on 2 048 queries
  train     encoder + decoder, forward and backward, 2 048 queries
  mesh      Generator3D.generate_obj_mesh_wnf on the 128^3 lattice (resolution_0 32)
Device-synchronised time by events over ``n`` calls after warm-up, taken ``--rounds`` times per path, host and hip in turn;
reported: the median over rounds and the spread (max - min).  ``default_form``: per stage "hip" where its median is below host's by
more than the larger of the two spreads at every shape timed for it, "host" otherwise (the sampler counts as two stages: the point
form on 2 048 queries and the lattice form) -- vtaco_amd/pointconv_host.py's DEFAULT_FORM follows this file's
committed run.  ``sampler_share_of_f32_matrix_peak``: 2 * 128^3 * 3000 * c_dim FLOP over the lattice sampler's time, against
the 157.3 TFLOP/s of the exact-f32 matrix instruction -- the share of that peak, not a rate of the whole decode."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
F32_MATRIX_PEAK = 157.3e12


def _event_ms(fn, n=10, warm=2):
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pointconv_bench.json"))
    ap.add_argument("--only", default=None, help="hip or host: run one path only (a profiler run of its own)")
    args = ap.parse_args()
    import torch
    from vtaco_amd import ops, pointconv_host as host
    from vtaco_amd.conv_onet.generation import Generator3D
    from vtaco_amd.conv_onet.models import ConvolutionalOccupancyNetwork, decoder_dict
    from vtaco_amd.encoder import encoder_dict, pointnetpp
    dev = torch.device("cuda:0")
    rounds = max(5, args.rounds) if args.only is None else 1
    paths = ("host", "hip") if args.only is None else (args.only,)
    N, M, NX = 3000, 2048, 128
    g = torch.Generator().manual_seed(0)
    cloud = (torch.rand(1, N, 3, generator=g) - 0.5).to(dev)
    q = ((torch.rand(1, M, 3, generator=g) - 0.5) * 1.1).to(dev)
    occ = (torch.rand(1, M, generator=g) < 0.5).float().to(dev)
    start = torch.zeros(1, dtype=torch.long)
    res = {"device": torch.cuda.get_device_name(0), "rounds_per_path": rounds, "cloud_points": N, "train_queries": M, "lattice": NX,
           "method": "host and hip alternately in one process; device-synchronised time by events over n calls after warm-up; per "
                     "figure the median over rounds and the spread (max - min) between rounds"}

    def set_form(p):
        host.FORM.update({s: p for s in host.STAGES})

    def timed(key, fns, n=10, warm=2):
        """fns: {path: callable}; alternate the paths, ``rounds`` times."""
        vals = {p: [] for p in paths}
        for _ in range(rounds):
            for p in paths:
                set_form(p)
                vals[p].append(_event_ms(fns[p] if isinstance(fns, dict) else fns, n, warm))
        res[key] = {p: _summary(v) for p, v in vals.items()}

    # ---- the geometric stages (no widths in them) ---------------------------------------------------------------------------------
    set_form("hip")
    c1 = pointnetpp.index_points(cloud, pointnetpp.fps(cloud, 512, start))
    c2 = pointnetpp.index_points(c1, pointnetpp.fps(c1, 128, start))
    with torch.no_grad():
        timed("fps_3000_512_ms", lambda: pointnetpp.fps(cloud, 512, start))
        timed("fps_512_128_ms", lambda: pointnetpp.fps(c1, 128, start))
        timed("ball_query_3000_512_ms", lambda: pointnetpp.ball_query(cloud, c1, 0.2, 32))
        timed("ball_query_512_128_ms", lambda: pointnetpp.ball_query(c1, c2, 0.4, 64))
        timed("three_nn_3000_512_ms", lambda: pointnetpp.three_nn(cloud, c1))

    for c_dim, hidden in ((32, 32), (128, 256)):
        tag = f"c{c_dim}_h{hidden}"
        torch.manual_seed(0)
        enc = encoder_dict["pointnet_plus_plus"](dim=3, c_dim=c_dim).to(dev)
        dec = decoder_dict["simple_local_point"](dim=3, c_dim=c_dim, hidden_size=hidden, sample_mode="gaussian", gaussian_val=0.1).to(dev)
        model = ConvolutionalOccupancyNetwork(dec, enc, device=dev)
        fea = torch.randn(1, N, c_dim, generator=torch.Generator().manual_seed(1)).to(dev)
        grad_c = torch.randn(1, M, c_dim, generator=torch.Generator().manual_seed(2)).to(dev)

        def sample(pts=None, lattice=None):
            return dec._sample_points(cloud, fea, pts, lattice)

        def sample_fb():
            f = fea.clone().requires_grad_(True)
            if host.form("sample") == "hip":
                from vtaco_amd.conv_onet.models.decoder import _PointSampleFn
                c = _PointSampleFn.apply(cloud, f, q, "gaussian", 0.1)
            else:
                c = host.point_sample(cloud, f, pts=q, sample_mode="gaussian", gaussian_val=0.1)
            c.backward(grad_c)

        def sample_lattice():
            step = 1 << 20
            for lo in range(0, NX ** 3, step):
                sample(lattice=(NX, 1.1, lo, min(step, NX ** 3 - lo)))

        def train():
            model.train()
            model.zero_grad(set_to_none=True)
            torch.nn.functional.l1_loss(model.decode(q, model.encode_inputs(cloud)).logits, occ).backward()

        gen = Generator3D(model, device=dev, resolution0=NX // 4, padding=0.1)

        def mesh():
            gen.generate_obj_mesh_wnf({"inputs": cloud})
        with torch.no_grad():
            timed(f"{tag}_sampler_fwd_{M}_ms", lambda: sample(q))
            timed(f"{tag}_sampler_lattice_{NX}_ms", sample_lattice, n=2, warm=1)
            c = sample(q)
            timed(f"{tag}_mlp_fwd_{M}_ms", lambda: dec._mlp_given(c, q))
        timed(f"{tag}_sampler_fwd_bwd_{M}_ms", sample_fb)
        timed(f"{tag}_train_fwd_bwd_{M}_ms", train, n=5, warm=2)
        model.eval()
        timed(f"{tag}_mesh_{NX}_ms", mesh, n=2, warm=1)
        if "hip" in paths:
            t = res[f"{tag}_sampler_lattice_{NX}_ms"]["hip"]["median_ms"] * 1e-3
            res[f"{tag}_sampler_share_of_f32_matrix_peak"] = 2.0 * NX ** 3 * N * c_dim / t / F32_MATRIX_PEAK

    if args.only is None:
        def verdict(keys):
            wins = 0
            for k in keys:
                r = res[k]
                wins += r["hip"]["median_ms"] < r["host"]["median_ms"] - max(r["host"]["spread_ms"], r["hip"]["spread_ms"])
            return "hip" if wins == len(keys) else "host"
        res["default_form"] = {
            "fps": verdict(["fps_3000_512_ms", "fps_512_128_ms"]),
            "ball_query": verdict(["ball_query_3000_512_ms", "ball_query_512_128_ms"]),
            "three_nn": verdict(["three_nn_3000_512_ms"]),
            "sample": verdict([k for k in res if "_sampler_fwd_" in k and k.endswith("_ms")]),
            "sample_lattice": verdict([k for k in res if "_sampler_lattice_" in k and k.endswith("_ms")])}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
