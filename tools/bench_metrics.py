#!/usr/bin/env python3
"""Device time of the visualise block's metrics against the host forms the reference uses, on the same box:

  chamfer_nn      vt_chamfer_nn (both directions, one launch) vs the reference's naive Chamfer in torch on the host CPU
  emd_assignment  vt_emd_auction (one workgroup per problem)  vs scipy cdist + linear_sum_assignment on the host CPU

for a close pair (the second cloud = the first plus 0.01-sigma noise) and a dissimilar pair (a 0.1-sigma Gaussian against a
uniform cube, what an early-training mesh looks like), 2048 x 2048 each, plus a batch of 8 dissimilar pairs in one launch.
Device times: median of device events around the call (the emd call ends in its status read, so it is synchronous).
Prints one JSON object; --out also writes it to a file.

    python tools/bench_metrics.py [--reps 5] [--scipy-reps 1] [--out profiles/metrics_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def pairs(n=2048):
    rng = np.random.RandomState(2100)
    g = (rng.randn(n, 3) * 0.1).astype(np.float32)
    yield "close", g, (g + rng.randn(n, 3) * 0.01).astype(np.float32)
    yield "dissimilar", (rng.randn(n, 3) * 0.1).astype(np.float32), rng.uniform(-0.5, 0.5, (n, 3)).astype(np.float32)


def device_ms(fn, reps):
    fn()                                                   # warm-up (library load, first launch)
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        out.append(s.elapsed_time(e))
    return statistics.median(out)


def host_ms(fn, reps):
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scipy-reps", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_metrics: no HIP device")
    from scipy.optimize import linear_sum_assignment
    from scipy.spatial import distance
    from vtaco_amd import eval as veval, ops
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "host_threads": torch.get_num_threads(), "eps_final": ops.EMD_EPS_FINAL}
    for name, a, b in pairs():
        ta, tb = torch.from_numpy(a)[None].to(dev), torch.from_numpy(b)[None].to(dev)
        ca, cb = torch.from_numpy(a)[None], torch.from_numpy(b)[None]
        r = {}
        r["chamfer_nn_device_ms"] = device_ms(lambda: ops.chamfer_nn(ta, tb), args.reps)
        r["chamfer_torch_host_ms"] = host_ms(lambda: veval.chamfer_distance_naive(ca, cb), args.reps)
        r["emd_device_ms"] = device_ms(lambda: ops.emd_assignment(ta, tb), args.reps)
        st = ops.emd_assignment(ta, tb)
        r.update(emd_device=float(st.emd[0]), rounds=int(st.rounds[0]), bids=int(st.bids[0]), phases=int(st.phases[0]))

        def scipy_emd():
            d = distance.cdist(a, b)
            return d[linear_sum_assignment(d)].sum() / len(d)
        r["emd_scipy_host_ms"] = host_ms(scipy_emd, args.scipy_reps)
        r["emd_scipy"] = float(scipy_emd())
        r["emd_speedup_vs_scipy"] = r["emd_scipy_host_ms"] / r["emd_device_ms"]
        r["chamfer_speedup_vs_torch_host"] = r["chamfer_torch_host_ms"] / r["chamfer_nn_device_ms"]
        res[name] = r
        print(name, json.dumps(r), file=sys.stderr)
    # a batch of 8 dissimilar pairs in one launch (8 workgroups)
    rng = np.random.RandomState(2108)
    a8 = torch.from_numpy((rng.randn(8, 2048, 3) * 0.1).astype(np.float32)).to(dev)
    b8 = torch.from_numpy(rng.uniform(-0.5, 0.5, (8, 2048, 3)).astype(np.float32)).to(dev)
    st = ops.emd_assignment(a8, b8)
    res["dissimilar_batch8"] = {"chamfer_nn_device_ms": device_ms(lambda: ops.chamfer_nn(a8, b8), args.reps),
                                "emd_device_ms": device_ms(lambda: ops.emd_assignment(a8, b8), args.reps),
                                "rounds": st.rounds.tolist(), "bids": st.bids.tolist()}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
