#!/usr/bin/env python3
"""Golden vectors for LocalDecoder on plane features (tests/golden/g21_plane_decode.npz), from the REAL reference:
LocalDecoder.forward (src/conv_onet/models/decoder.py:135-161) with sample_plane_feature (:55-60) at

    A: c_dim 32, hidden_size 32, n_blocks 5, bilinear, c_plane = {xz, xy, yz} at R = 9
    B: c_dim 32, hidden_size 64, n_blocks 5, leaky,    c_plane = {grid (R = 6), yz, xz, xy at R = 7}, given in that shuffled order

both with B = 2 scenes of N = 67 points, 8 of them per scene at |p| >= 0.56 on every axis (both clamps of normalize_coordinate), and
the gradients of logits.sum() under the reference's own autograd: to every plane and the grid in full, per parameter the
gradient's sum, abs-sum and 64 sampled entries (as g20 does).

Eval mode.  Runs only in the build container (/root/reference).  Weights and features are rounded to f16-representable values so that
the fixture stores them in half the bytes without changing the arithmetic.

    python tests/golden/make_plane_decode_goldens.py
"""
import importlib
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_goldens import _install_stubs, _randomise, _save  # noqa: E402
from make_attn_wide_goldens import sample_index  # noqa: E402

CASES = (("A", 32, 32, False, ("xz", "xy", "yz"), 9, None, 210),
         ("B", 32, 64, True, ("grid", "yz", "xz", "xy"), 7, 6, 211))


def points(g, B=2, N=67, far=8):
    p = (torch.rand(B, N, 3, generator=g) - 0.5) * (2 * 0.549)
    sign = torch.where(torch.rand(B, far, 3, generator=g) < 0.5, -1.0, 1.0)
    p[:, :far] = sign * (0.56 + 0.2 * torch.rand(B, far, 3, generator=g))
    p[:, 0, :] = p[:, 0, :].abs()                       # at least one point beyond each clamp on every axis
    p[:, 1, :] = -p[:, 1, :].abs()
    return p


def main():
    _install_stubs()
    decoder = importlib.import_module("src.conv_onet.models.decoder")
    torch.set_num_threads(8)
    out = {}
    for tag, c_dim, hidden, leaky, keys, R, Rg, seed in CASES:
        torch.manual_seed(seed)
        dec = decoder.LocalDecoder(dim=3, c_dim=c_dim, hidden_size=hidden, n_blocks=5, leaky=leaky, padding=0.1).eval()
        _randomise(dec, seed + 10)
        with torch.no_grad():
            for prm in dec.parameters():
                prm.copy_(prm.half().float())
        g = torch.Generator().manual_seed(seed + 20)
        c_plane = {}
        for k in keys:
            shape = (2, c_dim, Rg, Rg, Rg) if k == "grid" else (2, c_dim, R, R)
            c_plane[k] = torch.randn(*shape, generator=g).half().float().requires_grad_(True)
        p = points(g)
        logits = dec(p, c_plane)
        logits.sum().backward()
        out[f"{tag}.p"], out[f"{tag}.logits"] = p.numpy(), logits.detach().numpy()
        out[f"{tag}.keys"] = np.array(",".join(keys))
        for k in keys:
            out[f"{tag}.c.{k}"] = c_plane[k].detach().numpy().astype(np.float16)
            out[f"{tag}.grad.{k}"] = c_plane[k].grad.numpy()
        for name, prm in dec.state_dict().items():
            out[f"{tag}.sd.{name}"] = prm.numpy().astype(np.float16)
        for name, prm in dec.named_parameters():
            if prm.grad is None:                        # fc_p_img: not on forward's path
                continue
            gr = prm.grad.reshape(-1)
            out[f"{tag}.pgrad.{name}.sum"] = np.array([float(gr.double().sum()), float(gr.double().abs().sum())])
            out[f"{tag}.pgrad.{name}.samples"] = gr[sample_index(name, gr.numel())].numpy()
    _save("g21_plane_decode.npz", **out)


if __name__ == "__main__":
    main()
