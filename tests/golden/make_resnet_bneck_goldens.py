#!/usr/bin/env python3
"""Golden vector for the Bottleneck tactile encoders (g29_resnet_bneck.npz) from the REAL reference ``Resnet50`` (src/layers.py:86-207).
Build container only.  The 24 M parameters are not stored: both sides fill them with ``bottleneck_fill`` (seeded values in state_dict
order), so the fixture holds an input, the outputs and the list of parameter names / shapes.

    python tests/golden/make_resnet_bneck_goldens.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_goldens as mg          # noqa: E402


def bottleneck_fill(module, seed):
    """Overwrite every parameter and buffer, in state_dict order, with seeded values: EVERY BatchNorm weight (bn1, bn2, bn3, downsample.1)
    is 1 + 0.1 r, so conv3 speaks as loudly as the skip (make_resnet_goldens.deterministic_fill gives bn3.weight 0.1 r, which nearly
    silences it); variances 0.5 + |r|; conv and linear weights r / sqrt(fan_in); every other vector 0.1 r."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, t in module.state_dict().items():
            if "num_batches_tracked" in name:
                continue
            r = torch.randn(t.shape, generator=g)
            leaf = name.rsplit(".", 2)[-2:]                       # (module, tensor)
            batchnorm = leaf[0] in ("bn1", "bn2", "bn3") or (leaf[0] == "1" and "downsample" in name)
            if name.endswith("running_var"):
                t.copy_(0.5 + r.abs())
            elif batchnorm and leaf[1] == "weight":
                t.copy_(1.0 + 0.1 * r)
            elif t.dim() >= 2:
                t.copy_(r * (1.0 / max(1, t[0].numel())) ** 0.5)
            else:
                t.copy_(0.1 * r)


def make_resnet_bneck_golden():
    """g29_resnet_bneck.npz: the reference Resnet50 on a seeded input in eval and in train mode."""
    mg._install_stubs()
    from src.layers import Resnet50
    net = Resnet50(num_classes=32)
    bottleneck_fill(net, 90)
    x = torch.rand(2, 3, 64, 48, generator=torch.Generator().manual_seed(91))
    net.eval()
    with torch.no_grad():
        y_eval = net(x)
    net.train()
    with torch.no_grad():
        y_train = net(x)
    keys = [f"{k}:{tuple(v.shape)}" for k, v in net.state_dict().items() if "num_batches_tracked" not in k]
    mg._save("g29_resnet_bneck.npz", x=x.numpy(), y_eval=y_eval.numpy(), y_train=y_train.numpy(), keys=np.array(keys))


if __name__ == "__main__":
    make_resnet_bneck_golden()
