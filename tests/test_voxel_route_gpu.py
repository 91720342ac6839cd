"""GPU: a voxel-input Convolutional Occupancy Network built by get_model (``encoder: voxel_simple_local``), on the feature grid with
a UNet3D and on three planes with the plane U-Net -- one training step, eval_step's iou_voxels, and dense / MISE generation from a
[1,D,D,D] input."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BOX = 1.1
ENCODERS = {"grid": {"plane_type": "grid", "grid_resolution": 16, "unet3d": True,
                     "unet3d_kwargs": {"num_levels": 2, "f_maps": 32, "in_channels": 32, "out_channels": 32}},
            "planes": {"plane_type": ["xz", "xy", "yz"], "plane_resolution": 16, "unet": True,
                       "unet_kwargs": {"depth": 3, "merge_mode": "concat", "start_filts": 32}}}


def _cfg(kind):
    return {"data": {"dim": 3, "padding": 0.1, "input_type": "voxels"},
            "model": {"decoder": "simple_local", "encoder": "voxel_simple_local", "c_dim": 32,
                      "decoder_kwargs": {"sample_mode": "bilinear", "hidden_size": 32}, "encoder_kwargs": ENCODERS[kind]},
            "test": {"threshold": 0.5}, "generation": {"resolution_0": 8, "upsampling_steps": 0}}


def _volumes(B, D=16):
    """Solid balls of different radii as occupancy volumes [B,D,D,D]."""
    ax = torch.linspace(-0.5, 0.5, D)
    r = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), dim=-1).norm(dim=-1)
    return torch.stack([(r < 0.3 + 0.05 * b).float() for b in range(B)])


def _model(kind):
    from vtaco_amd.conv_onet import config as cfgmod
    from vtaco_amd.encoder.voxels import LocalVoxelEncoder
    cfg = _cfg(kind)
    torch.manual_seed(1)
    model = cfgmod.get_model(cfg, device=DEV)
    for blk in model.decoder.blocks:
        torch.nn.init.normal_(blk.fc_1.weight, 0, 0.1)                # (zero-initialised by the reference: let the field move)
    assert isinstance(model.encoder, LocalVoxelEncoder) and model.encoder.planes == (["grid"] if kind == "grid" else ["xz", "xy", "yz"])
    assert (model.encoder.unet3d is not None) == (kind == "grid") and (model.encoder.unet is not None) == (kind == "planes")
    return cfg, model


def _batch(B):
    g = torch.Generator().manual_seed(6)
    p = torch.rand(B, 256, 3, generator=g) - 0.5
    return {"inputs": _volumes(B), "points": p, "points.occ": (p.norm(dim=-1) < 0.3).float(), "voxels": _volumes(B)}


@pytest.mark.parametrize("kind", ["grid", "planes"])
def test_train_step_and_iou_voxels(kind):
    from vtaco_amd.common import make_3d_grid
    from vtaco_amd.conv_onet import config as cfgmod
    cfg, model = _model(kind)
    opt = torch.optim.Adam(model.parameters(), lr=1e-4)
    trainer = cfgmod.get_trainer(model, opt, cfg, DEV)
    data = _batch(2)
    model.train()
    loss, _, _ = trainer.compute_loss(data)
    assert math.isfinite(float(loss.detach()))
    opt.zero_grad()
    loss.backward()
    conv = model.encoder.conv_in
    for prm in (conv.weight, conv.bias):
        assert prm.grad is not None and bool(torch.isfinite(prm.grad).all()) and float(prm.grad.abs().max()) > 0
    assert math.isfinite(trainer.train_step(data)[0])
    # eval_step: iou_voxels from the logits at the voxel centres (training.py:374-390), recomputed in numpy
    model.eval()
    vox = data["voxels"]
    pts = make_3d_grid((-0.5 + 1 / 64,) * 3, (0.5 - 1 / 64,) * 3, tuple(vox.shape[1:])).unsqueeze(0).expand(2, -1, -1).contiguous()
    with torch.no_grad():
        probs = torch.sigmoid(model.decode(pts.to(DEV), model.encode_inputs(data["inputs"].to(DEV))).logits).cpu().numpy()
    trainer.threshold = float(np.median(probs))                       # a random field: cut it where both classes exist
    out = trainer.eval_step(data)
    assert set(out) == {"loss", "iou_voxels"} and math.isfinite(out["loss"])
    hat = probs >= trainer.threshold
    occ = (vox.numpy() >= 0.5).reshape(2, -1)
    assert hat.any() and not hat.all()
    want = float(np.mean((hat & occ).sum(-1) / (hat | occ).sum(-1)))
    assert abs(out["iou_voxels"] - want) <= 1e-6 and 0.0 < want < 1.0
    assert "iou_voxels" not in trainer.eval_step({k: v for k, v in data.items() if k != "voxels"})


@pytest.mark.parametrize("kind", ["grid", "planes"])
def test_dense_and_mise_generation_from_a_volume(kind):
    """generate_obj_mesh_wnf on [1,D,D,D] inputs (the eager route: a 4-D input is never captured): the dense mesh is the extraction of
    the point decode of the 32^3 lattice; without upsampling MISE is the dense extraction of its own lattice, the same vertices and
    faces; with one upsampling step its known entries are the point decode."""
    from vtaco_amd import mise, ops
    from vtaco_amd.common import make_3d_grid
    from vtaco_amd.conv_onet.generation import Generator3D
    _, model = _model(kind)
    model.eval()
    vol = _volumes(1)
    lattice = lambda n: (BOX * make_3d_grid((-0.5,) * 3, (0.5,) * 3, (n,) * 3)).to(DEV)
    with torch.no_grad():
        c = model.encode_inputs(vol.to(DEV))
        assert set(c) == ({"grid"} if kind == "grid" else {"xz", "xy", "yz"})
        dense32 = model.decode(lattice(32).unsqueeze(0), c).logits.reshape(32, 32, 32)
        dense9 = model.decode(lattice(9).unsqueeze(0), c).logits.reshape(9, 9, 9)
        dense17 = model.decode(lattice(17).unsqueeze(0), c).logits.reshape(17, 17, 17)
    threshold = 1.0 / (1.0 + math.exp(-float(dense32.median())))       # the level where the field crosses
    gen = Generator3D(model, device=DEV, resolution0=8, decode_precision="f32", threshold=threshold)
    mesh = gen.generate_obj_mesh_wnf({"inputs": vol})
    again = gen.generate_obj_mesh_wnf({"inputs": vol})                # a shape seen twice still runs eagerly
    assert not getattr(gen, "_graphs", None)
    own = gen.extract_mesh(dense32)                                   # (the dense route's level is the middle of the field's range)
    assert mesh.faces.shape[0] > 0
    for m in (mesh, again):
        assert torch.equal(m.vertices, own.vertices) and torch.equal(m.faces, own.faces)
    flat = Generator3D(model, device=DEV, resolution0=8, upsampling_steps=0, extraction="mise", decode_precision="f32", threshold=threshold)
    got = flat.generate_obj_mesh_wnf({"inputs": vol})
    want = ops.marching_cubes(dense9, flat.mise_level(), rescale=(4.0, BOX / 8))
    assert flat.mise_points_per_level == [9 ** 3] and got.faces.shape[0] > 0
    assert torch.equal(got.faces, want[1]) and torch.equal(got.vertices, want[0])
    fine = Generator3D(model, device=DEV, resolution0=8, upsampling_steps=1, extraction="mise", decode_precision="f32", threshold=threshold)
    assert fine.generate_obj_mesh_wnf({"inputs": vol}).faces.shape[0] > 0
    with torch.no_grad():
        values, known, per_level = mise.extract(fine.mise_evaluator(c), 8, 1, fine.mise_level(), BOX, DEV)
    k = known.bool()
    assert per_level == fine.mise_points_per_level and int(k.sum()) >= 9 ** 3 and torch.equal(values[k], dense17[k])
