"""Shared by tests/test_tactile_unet_gpu.py and tests/test_tactile_pc_gpu.py: the guard that makes the framework's conv / norm / pool /
sigmoid operators raise under the HIP tactile U-Net, the JSON report, and a seeded U-Net.  Test infrastructure."""
import json
import os

import torch
from torch.nn import functional as F

from seeded_fill import seeded_fill

_PATCHED_F = ("conv2d", "conv_transpose2d", "batch_norm", "max_pool2d", "sigmoid")


class no_framework_ops:
    """``with no_framework_ops():`` -- the functional ops the nn modules of the U-Net go through raise."""

    def __enter__(self):
        self.saved = {n: getattr(F, n) for n in _PATCHED_F}
        self.sigmoid = torch.sigmoid

        def boom(*a, **k):
            raise AssertionError("a framework operator ran under the HIP tactile U-Net")
        for n in _PATCHED_F:
            setattr(F, n, boom)
        torch.sigmoid = boom
        return self

    def __exit__(self, *exc):
        for n, f in self.saved.items():
            setattr(F, n, f)
        torch.sigmoid = self.sigmoid
        return False


def report(name, rep):
    out = os.environ.get("VTACO_REPORT_DIR") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "out")
    try:
        os.makedirs(out, exist_ok=True)
        path = os.path.join(out, "tactile_unet_gpu.json")
        cur = json.load(open(path)) if os.path.exists(path) else {}
        cur[name] = rep
        json.dump(cur, open(path, "w"), indent=1, sort_keys=True)
    except (OSError, ValueError):
        pass


def seeded_unet(depth=3, sf=32, cin=3, classes=1, seed=90):
    """A seeded U-Net, running statistics included (tests/seeded_fill.py; gain 1.4 keeps the activations O(1) through every level, so
    the sigmoid's argument spreads over a few units instead of collapsing to 0)."""
    from vtaco_amd.encoder import encoder_dict
    return seeded_fill(encoder_dict["UNet"](num_classes=classes, in_channels=cin, depth=depth, start_filts=sf), seed, gain=1.4).eval()
