#!/usr/bin/env python3
"""Golden vectors for the PointConv baseline (tests/golden/g26_pointconv.npz), from the REAL reference: src/encoder/pointnetpp.py
(PointNetPlusPlus) and src/conv_onet/models/decoder.py:427-515 (LocalPointDecoder) on a seeded [2,600,3] cloud, c_dim 32,
hidden_size 32.  Parameters come from tests/pointconv_ref.fill (seeded_fill + BatchNorm scales 1 + 0.1 r), so the file stores
inputs, outputs, gradients and the state_dict key lists only:

    enc.eval / enc.train   the encoder's features under torch.manual_seed(SEED_EVAL / SEED_TRAIN) (its farthest-point start
                           indices are two torch.randint draws from the global generator; stored as enc.*.starts)
    dec.<mode>.logits      the decoder on 300 queries and the eval features, 'gaussian' (gaussian_val 0.1) and 'inverse'
    dec.<mode>.grad.*      parameter gradients and the feature gradient of an L1 loss against a seeded target
Runs only where the reference is mounted (make_goldens.REF).

    python tests/golden/make_pointconv_goldens.py
"""
import importlib
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_goldens import _install_stubs, _save  # noqa: E402
from pointconv_ref import fill  # noqa: E402
from seeded_fill import keys_of  # noqa: E402

SEED_ENC, SEED_DEC, SEED_EVAL, SEED_TRAIN = 2601, 2602, 2611, 2612
MODES = (("gaussian", dict(sample_mode="gaussian", gaussian_val=0.1)), ("inverse", dict(sample_mode="inverse")))


def cloud():
    g = torch.Generator().manual_seed(2600)
    return (torch.rand(2, 600, 3, generator=g) - 0.5) * torch.tensor([1.0, 0.8, 0.9])


def queries():
    g = torch.Generator().manual_seed(2603)
    q = (torch.rand(2, 300, 3, generator=g) - 0.5) * 1.1
    q[:, :4] = cloud()[:, :4]                       # queries that are cloud points exactly
    return q, torch.rand(2, 300, generator=g)


def starts(seed, N=600, B=2):
    """The two draws farthest_point_sample makes under torch.manual_seed(seed): sa1 on the cloud, sa2 on its 512 centres."""
    torch.manual_seed(seed)
    return torch.randint(0, N, (B,), dtype=torch.long), torch.randint(0, 512, (B,), dtype=torch.long)


def main():
    _install_stubs()
    pointnetpp = importlib.import_module("src.encoder.pointnetpp")
    decoder = importlib.import_module("src.conv_onet.models.decoder")
    torch.set_num_threads(8)
    x = cloud()
    q, occ = queries()
    out = {"cloud": x.numpy(), "queries": q.numpy(), "occ": occ.numpy()}
    enc = fill(pointnetpp.PointNetPlusPlus(dim=3, c_dim=32, padding=0.1), SEED_ENC)
    out["enc.keys"] = np.array(keys_of(enc))
    for tag, seed in (("eval", SEED_EVAL), ("train", SEED_TRAIN)):
        enc.train(tag == "train")
        s = starts(seed)
        torch.manual_seed(seed)
        with torch.no_grad():
            xyz, fea = enc(x)
        assert torch.equal(xyz, x)
        out[f"enc.{tag}.fea"] = fea.numpy().astype(np.float32)
        out[f"enc.{tag}.starts"] = torch.stack(s).numpy()
    fea = torch.from_numpy(out["enc.eval.fea"])
    for tag, kw in MODES:
        dec = fill(decoder.LocalPointDecoder(dim=3, c_dim=32, hidden_size=32, **kw), SEED_DEC)
        out[f"dec.{tag}.keys"] = np.array(keys_of(dec))
        f = fea.clone().requires_grad_(True)
        logits = dec(q, (x, f))
        torch.nn.functional.l1_loss(logits, occ).backward()
        out[f"dec.{tag}.logits"] = logits.detach().numpy().astype(np.float32)
        out[f"dec.{tag}.grad.fea"] = f.grad.numpy().copy()
        for name, prm in dec.named_parameters():
            out[f"dec.{tag}.grad.{name}"] = prm.grad.numpy().copy()
    _save("g26_pointconv.npz", **out)


if __name__ == "__main__":
    main()
