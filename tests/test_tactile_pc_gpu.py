"""GPU: vt_depth_cloud against the float64 rule (tests/tactile_pc_rule.py, pinned to the reference by tests/test_tactile_pc_cpu.py), and
``Generator3D.generate_tactile_pc`` on a model built from the tactile configuration against the reference-made golden g24_tactile_pc.npz.
Under the HIP path the framework's conv / norm / pool / sigmoid operators raise."""
import math
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

import tactile_pc_rule as rule
from tactile_unet_util import no_framework_ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W = 320, 240


@pytest.fixture(scope="module")
def g24():
    return np.load(os.path.join(GOLDEN, "g24_tactile_pc.npz"))


@pytest.mark.parametrize("n,h,w", [(5, 8, 6), (10, 320, 240), (1, 2, 2)], ids=["5x8x6", "10x320x240", "1x2x2"])
def test_depth_cloud_against_the_rule(n, h, w, g24):
    """The same arithmetic in the same precision: only the last-bit order of the 3 x 3 product is free (1e-12 relative)."""
    from vtaco_amd import ops
    from vtaco_amd.common import sensor_pose_records
    rs = np.random.RandomState(100 + n)
    pred = rs.rand(n, h * w).astype(np.float32)
    B = (n + 4) // 5
    cam_pos, cam_rot = (rs.randn(B, 5, 3) * 0.12).astype(np.float32), (rs.randn(B, 5, 3) * 0.8).astype(np.float32)
    pc_ply = g24["pc_ply"][np.arange(B) % 2]
    pose = sensor_pose_records(cam_pos, cam_rot, pc_ply)[:n]
    got = ops.depth_cloud(torch.from_numpy(pred).to(DEV), torch.from_numpy(pose).to(DEV), w, h)
    assert got.dtype == torch.float64 and got.shape == (n, h * w, 3)
    ref = np.concatenate([rule.tactile_pc(pred[5 * b:5 * b + 5], h, w, cam_pos[b], cam_rot[b], pc_ply[b]) for b in range(B)])
    err, size = float(np.abs(got.cpu().numpy() - ref).max()), float(np.abs(ref).max())
    print({"max_abs_err": err, "size": size})
    assert err <= 1e-12 * size
    # the float32 output: the float64 result rounded once
    got32 = ops.depth_cloud(torch.from_numpy(pred).to(DEV), torch.from_numpy(pose).to(DEV), w, h, dtype=torch.float32)
    assert torch.equal(got32, got.float())


TACTILE_TEST_SHAPED_YAML = """
# the model section of the reference's configs/tactile/tactile_test.yaml key for key and value for value (decoder and encoder False, the
# depth U-Net as encoder_img, the digit-pose regressor with its MANO layer as encoder_hand), over the entries its loader inherits from
# the default config (dim, padding, c_dim, threshold, resolution_0); mano_root points at a synthetic asset.  Written by this test.
method: vtaco
data:
  input_type: pointcloud
  dim: 3
  padding: 0.1
  num_sample: 2048
model:
  train_tactile: True
  with_img: True
  with_contact: False
  encoder: False
  encoder_hand: pointnet_local_pool
  encoder_hand_kwargs:
    hidden_dim: 32
    plane_type: ['xz', 'xy', 'yz']
    plane_resolution: 64
    unet: True
    unet_kwargs: {{depth: 4, merge_mode: concat, start_filts: 32}}
    out_mano: True
    out_dim: 30
    manolayer_kwargs:
      center_idx: 9
      flat_hand_mean: False
      ncomps: 45
      side: right
      mano_root: {mano}
      use_pca: False
      root_rot_mode: axisang
      joint_rot_mode: axisang
      robust_rot: False
      return_transf: False
      return_full_pose: True
  encoder_img: UNet
  encoder_img_kwargs: {{num_classes: 1, in_channel: 3, start_filts: 32, depth: 3}}
  encoder_t2d: False
  encoder_t2d_kwargs: False
  decoder: False
  c_dim: 32
test: {{threshold: 0.5}}
generation: {{resolution_0: 32, upsampling_steps: 0}}
"""


@pytest.fixture(scope="module")
def tactile_generator(g24, tmp_path_factory):
    import yaml
    import synth_mano
    from vtaco_amd.conv_onet import config
    mano = tmp_path_factory.mktemp("mano")
    synth_mano.write_pkl(synth_mano.make_asset(0), str(mano))
    cfg = yaml.safe_load(TACTILE_TEST_SHAPED_YAML.format(mano=str(mano)))
    torch.manual_seed(0)
    model = config.get_model(cfg, device=torch.device(DEV))
    assert model.decoder is None and model.encoder is None and model.encoder_hand is not None and model.encoder_t2d is None
    rule.fill_like_the_golden(model.encoder_img, g24)
    return model, config.get_generator(model, cfg, torch.device(DEV))


@pytest.mark.parametrize("B", [1, 2])
def test_generate_tactile_pc_against_the_reference_golden(B, g24, tactile_generator, monkeypatch):
    from vtaco_amd import ops
    from vtaco_amd.common import sensor_pose_records
    monkeypatch.setenv("VTACO_TACTILE_UNET", "hip")
    model, gen = tactile_generator
    imgs = torch.rand(2, 5, 3, H, W, generator=torch.Generator().manual_seed(int(g24["image_seed"])))[:B]
    names = ["scene_a", "scene_b"][:B]
    data = {"points": torch.zeros(B, 8, 3), "points.name": names, "inputs": torch.zeros(B, 16, 3), "inputs.img": imgs,
            "inputs.pc_ply": torch.from_numpy(g24["pc_ply"][:B]), "points.cam_pos": torch.from_numpy(g24["cam_pos"][:B]),
            "points.cam_rot": torch.from_numpy(g24["cam_rot"][:B]).reshape(B, 15)}
    hand = model.encoder_hand.forward
    model.encoder_hand.forward = lambda *a, **k: (_ for _ in ()).throw(AssertionError("generate_tactile_pc ran the hand encoder"))
    try:
        with no_framework_ops():
            out, got_names = gen.generate_tactile_pc(data)
            with torch.no_grad():
                pred = model.encode_img_inputs(imgs.to(DEV))
    finally:
        model.encoder_hand.forward = hand
    assert isinstance(out, np.ndarray) and out.dtype == np.float64 and out.shape == (B, 5, H * W, 3)
    assert list(got_names) == names
    # the reference's predicted depth at the stored pixels: the bound of the g6 test
    stride = int(g24["stride"])
    depth_err = float(np.abs(pred.cpu().numpy()[:, :, ::stride] - g24["pred"][:B]).max())
    assert depth_err <= 1e-4, depth_err
    # the tolerance is derived, not measured: a depth error of 1e-4 (the bound above) times 0.005 (pred -> metres) times 1.2 (the largest
    # |direction| of a pixel ray (1, -x / f, -y / f) at fov 60) divided by the golden's normalisation scale
    for b in range(B):
        cloud = g24["pc_ply"][b]
        scale = 2 * float(np.max(np.sqrt(np.sum((cloud - cloud.mean(axis=0)) ** 2, axis=1))))
        tol = 1e-4 * 0.005 * 1.2 / scale
        err = float(np.abs(out[b][:, ::stride] - g24["out"][b]).max())
        print({"scene": b, "max_abs_err": err, "tol": tol, "depth_err": depth_err})
        assert err <= tol, (err, tol)
        assert float(np.abs(out[b].min(axis=1) - g24["out_min"][b]).max()) <= tol
        assert float(np.abs(out[b].max(axis=1) - g24["out_max"][b]).max()) <= tol
        assert float(np.abs(out[b].mean(axis=1) - g24["out_mean"][b]).max()) <= tol
    # it IS depth_cloud(encode_img_inputs(imgs)) with the sample's pose records
    pose = torch.from_numpy(sensor_pose_records(g24["cam_pos"][:B], g24["cam_rot"][:B], g24["pc_ply"][:B])).to(DEV)
    again = ops.depth_cloud(pred.reshape(B * 5, H * W), pose, W, H).view(B, 5, H * W, 3).cpu().numpy()
    assert np.array_equal(out, again)
    # scene 0 of a batch of two is the batch of one, bit for bit (the depth estimator is batch-invariant)
    if B == 2:
        one = dict(data)
        for k in ("points", "inputs", "inputs.img", "inputs.pc_ply", "points.cam_pos", "points.cam_rot"):
            one[k] = data[k][:1]
        one["points.name"] = names[:1]
        with no_framework_ops():
            assert np.array_equal(gen.generate_tactile_pc(one)[0][0], out[0])
