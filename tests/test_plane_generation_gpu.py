"""GPU: a three-plane Convolutional Occupancy Network built by get_model -- dense and MISE generation against the point decode bit
for bit, and one training step whose gradients reach the encoder's U-Net with F.grid_sample never called."""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BOX = 1.1


def _cfg():
    return {"data": {"dim": 3, "padding": 0.1, "input_type": "pointcloud"},
            "model": {"decoder": "simple_local", "encoder": "pointnet_local_pool", "c_dim": 32,
                      "decoder_kwargs": {"sample_mode": "bilinear", "hidden_size": 32},
                      "encoder_kwargs": {"hidden_dim": 32, "plane_type": ["xz", "xy", "yz"], "plane_resolution": 32, "unet": True,
                                         "unet_kwargs": {"depth": 4, "merge_mode": "concat", "start_filts": 32}}},
            "test": {"threshold": 0.5}, "generation": {"resolution_0": 8, "upsampling_steps": 0}}


def _cloud(n, seed, B=1):
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(B, n, 3, generator=g)
    return 0.35 * v / v.norm(dim=-1, keepdim=True) + 0.01 * torch.randn(B, n, 3, generator=g)      # a noisy sphere shell


@pytest.fixture(scope="module")
def scene():
    """The seeded model recipe of tests/test_mise_gpu.py (get_model under torch.manual_seed(1), wider fc_1 so the field moves)."""
    from vtaco_amd.conv_onet import config as cfgmod
    torch.manual_seed(1)
    model = cfgmod.get_model(_cfg(), device=DEV)
    for blk in list(model.decoder.blocks) + list(model.encoder.blocks):
        torch.nn.init.normal_(blk.fc_1.weight, 0, 0.1)
    assert model.encoder.planes == ["xz", "xy", "yz"] and model.encoder.unet is not None
    return model.eval(), _cloud(300, 2)


def _lattice(n):
    from vtaco_amd.common import make_3d_grid
    return (BOX * make_3d_grid((-0.5,) * 3, (0.5,) * 3, (n,) * 3)).to(DEV)


def test_dense_generation_is_the_point_decode(scene):
    from vtaco_amd.conv_onet.generation import Generator3D
    model, cloud = scene
    gen = Generator3D(model, device=DEV, resolution0=8, decode_precision="f32")
    nx = 32
    with torch.no_grad():
        c = model.encode_inputs(cloud.to(DEV))
        assert set(c) == {"xz", "xy", "yz"}
        lat = gen.eval_lattice(c, nx)
        pts = model.decode(_lattice(nx).unsqueeze(0), c).logits.reshape(-1)
        part = gen.eval_lattice(c, nx, first=nx * nx + 3, count=2 * nx * nx + 7)
    assert torch.equal(lat, pts) and torch.equal(part, pts[nx * nx + 3:3 * nx * nx + 10])
    mesh = gen.generate_obj_mesh_wnf({"inputs": cloud})
    own = gen.extract_mesh(pts.reshape(nx, nx, nx))
    assert mesh.vertices.shape[0] > 0 and mesh.faces.shape[0] > 0
    assert torch.equal(mesh.vertices, own.vertices) and torch.equal(mesh.faces, own.faces)


def test_mise_generation_known_entries_are_the_point_decode(scene):
    from vtaco_amd import mise
    from vtaco_amd.conv_onet.generation import Generator3D
    model, cloud = scene
    n = 33
    with torch.no_grad():
        c = model.encode_inputs(cloud.to(DEV))
        dense = model.decode(_lattice(n).unsqueeze(0), c).logits.reshape(n, n, n)
    # the level is the logit of the threshold: put it at the field's median so that the field crosses it
    threshold = 1.0 / (1.0 + math.exp(-float(dense.median())))
    gen = Generator3D(model, device=DEV, resolution0=16, upsampling_steps=1, extraction="mise", decode_precision="f32", threshold=threshold)
    mesh = gen.generate_obj_mesh_wnf({"inputs": cloud})
    assert mesh.vertices.shape[0] > 0 and mesh.faces.shape[0] > 0
    with torch.no_grad():
        values, known, per_level = mise.extract(gen.mise_evaluator(c), 16, 1, gen.mise_level(), BOX, DEV)
    assert per_level == gen.mise_points_per_level and values.shape == (n, n, n)
    k = known.bool()
    assert int(k.sum()) > 17 ** 3 and torch.equal(values[k], dense[k])


def test_refused_generator_routes(scene):
    from vtaco_amd._lib import VtError
    from vtaco_amd.conv_onet.generation import Generator3D
    from vtaco_amd.conv_onet.inferencing import Inferencer
    model, cloud = scene
    gen = Generator3D(model, device=DEV, resolution0=8)
    with pytest.raises(VtError, match="plane features"):
        gen.generate_mesh_graphed(cloud)
    with pytest.raises(VtError, match="plane features"):
        gen.generate_obj_mesh_sharded({"inputs": cloud})
    with pytest.raises(VtError, match="plane features"):
        Generator3D(model, device=DEV, resolution0=8, with_img=True).generate_obj_mesh_wnf({"inputs": cloud})
    with pytest.raises(VtError, match="plane features"):
        Inferencer(model, None, Generator3D(model, device=DEV, resolution0=8, with_img=True), device=DEV, with_img=True)


def test_one_train_step_reaches_the_unet(monkeypatch):
    from vtaco_amd.conv_onet import config as cfgmod
    cfg = _cfg()
    torch.manual_seed(1)
    model = cfgmod.get_model(cfg, device=DEV)
    opt = torch.optim.Adam(model.parameters(), lr=1e-4)
    trainer = cfgmod.get_trainer(model, opt, cfg, DEV)
    g = torch.Generator().manual_seed(6)
    B = 2
    p = torch.rand(B, 256, 3, generator=g) - 0.5
    data = {"inputs": _cloud(300, 7, B), "points": p, "points.occ": (p.norm(dim=-1) < 0.35).float()}
    calls = []
    monkeypatch.setattr(F, "grid_sample", lambda *a, **k: calls.append(1) or (_ for _ in ()).throw(AssertionError("F.grid_sample called")))
    model.train()
    loss, _, _ = trainer.compute_loss(data)
    assert math.isfinite(float(loss.detach()))
    opt.zero_grad()
    loss.backward()
    used = {n: q for n, q in model.named_parameters() if not n.startswith("decoder.fc_p_img")}
    for n, q in used.items():
        assert q.grad is not None and bool(torch.isfinite(q.grad).all()), n
    assert any(float(q.grad.abs().max()) > 0 for n, q in used.items() if n.startswith("encoder.unet.") and n.endswith("weight"))
    out = trainer.train_step(data)
    assert math.isfinite(out[0]) and not calls
