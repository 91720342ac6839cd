#!/usr/bin/env python3
"""Golden vectors for ``Generator3D.generate_tactile_pc`` (generation.py:286-333) from the REAL reference (g24_tactile_pc.npz): the
five predicted depth images of two scenes as world-space point clouds, normalised by the object's cloud.

Build container only.  The reference generator and the reference ``UNet`` (depth 3, 32 start filters: the tactile config's) run
unmodified on the CPU inside the reference's own ``ConvolutionalOccupancyNetwork`` (decoder and encoder None, as the tactile config
builds it); only the hand encoder is a stand-in that returns zeros (the reference calls it and uses nothing of the result).  The
0.47 M weights and the images are seeds (``tests/seeded_fill.py``, ``torch.rand``); stored are the poses, the object clouds, and of
``pred_depth`` and the result every 97th pixel of each sensor plus the per-sensor min / max / mean of the whole result.

    python tests/golden/make_tactile_pc_goldens.py
"""
import importlib
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_goldens as mg          # noqa: E402
from seeded_fill import keys_of, seeded_fill          # noqa: E402

W, H = 240, 320
WEIGHT_SEED, IMAGE_SEED, POSE_SEED, STRIDE = 240, 241, 242, 97


def main():
    mg._install_stubs()
    for name in ("trimesh", "skimage", "skimage.measure"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["skimage"].measure = sys.modules["skimage.measure"]
    loadtxt = np.loadtxt
    np.loadtxt = lambda *a, **k: np.zeros(W * H)        # generation.py reads ./data/VTacO_mesh/depth_origin.txt at import
    try:
        generation = importlib.import_module("src.conv_onet.generation")
    finally:
        np.loadtxt = loadtxt
    from src.layers import UNet
    torch.set_num_threads(8)
    net = seeded_fill(UNet(num_classes=1, in_channels=3, depth=3, start_filts=32), WEIGHT_SEED).eval()
    B = 2
    imgs = torch.rand(B, 5, 3, H, W, generator=torch.Generator().manual_seed(IMAGE_SEED))
    g = torch.Generator().manual_seed(POSE_SEED)
    pc_ply = torch.randn(B, 400, 3, generator=g) * 0.15 + 0.02
    cam_pos = torch.randn(B, 5, 3, generator=g) * 0.12
    cam_rot = torch.randn(B, 5, 3, generator=g) * 0.8
    seen = {}

    class NoHand(torch.nn.Module):
        """The hand encoder's place: generate_tactile_pc reads ``mano_param`` from its result and uses nothing of it."""

        def forward(self, inputs):
            return {"mano_param": torch.zeros(inputs.size(0), 30)}

    # the reference's own model class (models/__init__.py; mg's stub package stands at its import name, so the file is loaded by path)
    spec = importlib.util.spec_from_file_location("ref_conv_onet_models", os.path.join(mg.REF, "src", "conv_onet", "models", "__init__.py"))
    ref_models = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref_models)
    model = ref_models.ConvolutionalOccupancyNetwork(None, None, NoHand(), net, None, device="cpu").eval()
    net.register_forward_hook(lambda m, a, y: seen.setdefault("pred", []).append(y.detach().reshape(1, y.shape[0], -1).numpy().copy()))
    data = {"points": torch.zeros(B, 8, 3), "points.name": ["scene_a", "scene_b"], "inputs": torch.zeros(B, 16, 3), "inputs.pc_ply": pc_ply,
            "inputs.img": imgs, "inputs.depth": torch.zeros(B, 5, W * H), "points.cam_pos": cam_pos, "points.cam_rot": cam_rot}
    gen = generation.Generator3D(model, device="cpu")
    out, names = gen.generate_tactile_pc(data)
    assert out.shape == (B, 5, W * H, 3) and out.dtype == np.float64 and list(names) == ["scene_a", "scene_b"]
    pred = np.concatenate(seen["pred"], axis=0)
    print("pred range", float(pred.min()), float(pred.max()), "fraction in (0.05, 0.95):", float(((pred > 0.05) & (pred < 0.95)).mean()))
    mg._save("g24_tactile_pc.npz", weight_seed=np.array(WEIGHT_SEED), image_seed=np.array(IMAGE_SEED), stride=np.array(STRIDE),
             keys=np.array(keys_of(net)), pc_ply=pc_ply.numpy(), cam_pos=cam_pos.numpy(), cam_rot=cam_rot.numpy(),
             pred=pred[:, :, ::STRIDE].copy(), out=out[:, :, ::STRIDE].copy(),
             out_min=out.min(axis=2), out_max=out.max(axis=2), out_mean=out.mean(axis=2))


if __name__ == "__main__":
    main()
