"""CPU: the float64 restatement of generate_tactile_pc's per-pixel path (tests/tactile_pc_rule.py) against the golden made by the REAL
reference's ``Generator3D.generate_tactile_pc`` (g24_tactile_pc.npz, tests/golden/make_tactile_pc_goldens.py), and the host-side pieces of
the public method: the pose records, the dispatch rules that need no GPU, the factory on the tactile configuration."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

import tactile_pc_rule as rule

H, W = 320, 240


@pytest.fixture(scope="module")
def g24():
    return np.load(os.path.join(GOLDEN, "g24_tactile_pc.npz"))


def test_rule_reproduces_the_reference_golden(g24):
    """The golden keeps every 97th pixel of pred_depth and of the result: the rule on an image that holds those predictions (zeros
    elsewhere; a pixel's point depends on its own depth alone) gives the reference's points there.  The same float64 operations in the
    same order: equal to the last bits of the 3 x 3 product (1e-12 relative to the coordinates' size)."""
    stride = int(g24["stride"])
    idx = np.arange(0, H * W, stride)
    assert g24["pred"].shape == (2, 5, idx.size) and g24["out"].shape == (2, 5, idx.size, 3)
    for b in range(2):
        pred = np.zeros((5, H * W), dtype=np.float32)
        pred[:, idx] = g24["pred"][b]
        got = rule.tactile_pc(pred, H, W, g24["cam_pos"][b], g24["cam_rot"][b], g24["pc_ply"][b])[:, idx]
        ref = g24["out"][b]
        assert got.dtype == np.float64
        assert float(np.abs(got - ref).max()) <= 1e-12 * float(np.abs(ref).max())


def test_rule_camera_cloud_is_the_oracles():
    """The any-size unprojection of the rule is the oracle's function, bit for bit, at the one size the oracle's is written for."""
    from oracle import vtaco_oracle as orc
    depth = (0.019 + 0.003 * np.random.RandomState(3).rand(H, W)).astype(np.float32)
    assert np.array_equal(rule._camera_cloud_any(depth), orc.depth_to_camera_cloud(depth))


def test_pose_records_carry_the_rules_pose_and_norm(g24):
    """``sensor_pose_records`` (what vt_depth_cloud reads): applying a record by hand gives the rule's point."""
    from vtaco_amd.common import sensor_pose_records
    pose = sensor_pose_records(g24["cam_pos"], g24["cam_rot"], g24["pc_ply"])
    assert pose.shape == (10, 16) and pose.dtype == np.float64
    pred = np.random.RandomState(4).rand(5, 8 * 6).astype(np.float32)
    ref = rule.tactile_pc(pred, 8, 6, g24["cam_pos"][1], g24["cam_rot"][1], g24["pc_ply"][1])
    for t in range(5):
        rec = pose[5 + t]
        cam = rule.camera_cloud(pred[t].reshape(8, 6) * 0.005 + 0.019)
        got = ((rec[:9].reshape(3, 3) @ cam.T).T + rec[9:12] - rec[12:15]) / rec[15]
        assert float(np.abs(got - ref[t]).max()) <= 1e-12 * float(np.abs(ref[t]).max())


def test_unet_dispatch_without_a_gpu(monkeypatch):
    """CPU tensors never take the HIP path; the knob is validated at call time; state_dict keys are the golden's."""
    from vtaco_amd.encoder import encoder_dict
    net = encoder_dict["UNet"](num_classes=1, in_channels=3, depth=3, start_filts=8).eval()
    x = torch.rand(1, 3, 8, 8)
    for mode in ("hip", "host"):
        monkeypatch.setenv("VTACO_TACTILE_UNET", mode)
        assert not net.hip_supported(x)
    with torch.no_grad():
        assert torch.equal(net(x), net.forward_modules(x))
    monkeypatch.setenv("VTACO_TACTILE_UNET", "fast")
    with pytest.raises(ValueError):
        net.hip_supported(x)


def test_seeded_weights_reproduce_the_goldens_network(g24):
    """The golden stores seeds, not weights: vtaco_amd's U-Net filled in the golden's key order, run by its nn modules on the CPU on
    scene 0's first image, gives the reference's pred_depth at the stored pixels (1e-4, the bound of tests/test_host_modules_gpu.py)."""
    from vtaco_amd.encoder import encoder_dict
    net = rule.fill_like_the_golden(encoder_dict["UNet"](num_classes=1, in_channels=3, depth=3, start_filts=32), g24).eval()
    imgs = torch.rand(2, 5, 3, H, W, generator=torch.Generator().manual_seed(int(g24["image_seed"])))
    with torch.no_grad():
        y = net(imgs[0, :1]).reshape(-1)[::int(g24["stride"])].numpy()
    assert float(np.abs(y - g24["pred"][0, 0]).max()) <= 1e-4


def test_supported_shapes_host_query():
    from vtaco_amd import _lib
    lib = _lib.load()
    ok = lambda *a: bool(lib.vt_tactile_unet_supported(*a))
    assert ok(3, 32, 3, 1, 5, 320, 240) and ok(3, 8, 3, 1, 2, 64, 48) and ok(1, 16, 1, 1, 1, 15, 17) and ok(5, 64, 4, 4, 1, 32, 32)
    assert not ok(3, 32, 3, 1, 5, 322, 240) and not ok(3, 12, 3, 1, 1, 8, 8) and not ok(6, 8, 3, 1, 1, 32, 32) and not ok(3, 72, 3, 1, 1, 8, 8)
    assert not ok(3, 32, 5, 1, 1, 8, 8) and not ok(3, 32, 3, 5, 1, 8, 8) and not ok(3, 32, 3, 1, 1025, 8, 8) and not ok(3, 32, 3, 1, 1, 4096, 8)
    assert not ok(3, 64, 3, 1, 1024, 2048, 2048)                                  # a tensor of 2^31 elements or more
    assert lib.vt_tactile_unet_blob_bytes(3, 32, 3, 1) > 4 * 460_000 and lib.vt_tactile_unet_blob_bytes(3, 12, 3, 1) == 0
    assert lib.vt_tactile_unet_workspace_bytes(3, 32, 3, 1, 5, 322, 240) == 0
