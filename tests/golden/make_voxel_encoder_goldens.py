#!/usr/bin/env python3
"""Golden vectors for the voxel-input encoder (tests/golden/g25_voxel_encoder.npz, tests/golden/g25_model.binvox), from the REAL
reference: src/encoder/voxels.py:10-119 (LocalVoxelEncoder: conv_in, ReLU, torch_scatter.scatter_mean onto the grid / the planes, the
optional UNet3D) on a seeded non-cubic [2,6,5,7] volume, about 30 % occupied with a few non-binary values, in four forms --

    grid        grid_resolution 8, no UNet3D         outputs + conv_in gradients under a seeded upstream gradient
    planes      xz / xy / yz at resolution 8, no U-Net   the same
    grid_unet   grid_resolution 8 with a two-level UNet3D (pins the state_dict keys and the wiring)
    k1          kernel_size 1, grid_resolution 8

-- and src/utils/binvox_rw.py: a seeded 8x8x8 occupancy array written by ``write`` and what ``read_as_3d_array`` gives back.
Runs only where the reference is mounted (make_goldens.REF); torch_scatter is not installed: make_goldens.py's stand-in.

    python tests/golden/make_voxel_encoder_goldens.py
"""
import importlib
import importlib.util
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_goldens import OUT, REF, _install_stubs, _save, _sd  # noqa: E402

FORMS = (("grid", dict(grid_resolution=8, plane_type="grid")),
         ("planes", dict(plane_resolution=8, plane_type=["xz", "xy", "yz"])),
         ("grid_unet", dict(grid_resolution=8, plane_type="grid", unet3d=True,
                            unet3d_kwargs=dict(num_levels=2, f_maps=8, in_channels=32, out_channels=32))),
         ("k1", dict(grid_resolution=8, plane_type="grid", kernel_size=1)))


def volume():
    g = torch.Generator().manual_seed(251)
    x = (torch.rand(2, 6, 5, 7, generator=g) < 0.3).float()
    soft = torch.rand(2, 6, 5, 7, generator=g) < 0.05                # a few non-binary values
    return torch.where(soft, torch.rand(2, 6, 5, 7, generator=g), x)


def main():
    _install_stubs()
    voxels = importlib.import_module("src.encoder.voxels")
    torch.set_num_threads(8)
    out = {"x": volume().numpy()}
    x = volume()
    for i, (tag, kw) in enumerate(FORMS):
        torch.manual_seed(252 + i)
        enc = voxels.LocalVoxelEncoder(dim=3, c_dim=32, padding=0.1, **kw)
        with torch.no_grad():                                         # a bias of either sign: both sides of the ReLU
            enc.conv_in.bias.add_(0.05 * torch.randn(32, generator=torch.Generator().manual_seed(260 + i)))
        fea = enc(x)
        for k, v in fea.items():
            out[f"{tag}.fea.{k}"] = v.detach().numpy().astype(np.float32)
        if tag in ("grid", "planes"):
            g = torch.Generator().manual_seed(270 + i)
            up = {k: torch.randn(v.shape, generator=g) for k, v in fea.items()}
            sum((fea[k] * up[k]).sum() for k in fea).backward()
            for k, v in up.items():
                out[f"{tag}.up.{k}"] = v.numpy()
            out[f"{tag}.grad.weight"] = enc.conv_in.weight.grad.numpy().copy()
            out[f"{tag}.grad.bias"] = enc.conv_in.bias.grad.numpy().copy()
        out.update(_sd(enc, f"sd.{tag}."))

    # ---- binvox: the reference's writer and reader on a seeded 8^3 array --------------------------------------------------------
    if not hasattr(np, "bool"):
        np.bool = bool                                               # binvox_rw.py:145 predates numpy 1.24
    spec = importlib.util.spec_from_file_location("binvox_rw", os.path.join(REF, "src", "utils", "binvox_rw.py"))
    binvox_rw = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(binvox_rw)
    occ = (np.random.RandomState(253).rand(8, 8, 8) < 0.35).astype(np.uint8)
    path = os.path.join(OUT, "g25_model.binvox")
    # the writer emits str (header) and chr(byte) (runs): a latin-1 text file without newline translation is the byte stream
    with open(path, "w", encoding="latin-1", newline="") as f:
        binvox_rw.write(binvox_rw.Voxels(occ, [8, 8, 8], [0.0, 0.0, 0.0], 1.0, "xyz"), f)
    with open(path, "rb") as f:
        back = binvox_rw.read_as_3d_array(f)
    assert np.array_equal(back.data, occ.astype(bool))
    out["binvox.array"] = back.data.astype(np.uint8)
    print(f"g25_model.binvox: {os.path.getsize(path)} bytes")
    _save("g25_voxel_encoder.npz", **out)


if __name__ == "__main__":
    main()
