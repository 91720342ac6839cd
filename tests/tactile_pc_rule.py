"""The reference's per-pixel path of ``generate_tactile_pc`` (generation.py:325-331) restated on the CPU in float64 from the functions
the oracle already has: ``depth_to_camera_cloud`` (RFUniverseCamera.depth_2_camera_pointcloud, the unfiltered cloud),
``cam_to_world`` (pc_cam_to_world) and norm_pc_1.  Test infrastructure: tests/test_tactile_pc_cpu.py pins it to the reference-made
golden g24_tactile_pc.npz, tests/test_tactile_pc_gpu.py holds vt_depth_cloud to it."""
import math

import numpy as np

from oracle import vtaco_oracle as orc

FOV = 60


def camera_cloud(depth):
    """``orc.depth_to_camera_cloud`` for an image of any size [H, W] (the oracle's is written for the sensor's 320 x 240; at that size
    this IS the oracle's function, at the others the same expressions -- test_rule_camera_cloud_is_the_oracles holds the two together)."""
    h, w = depth.shape
    if (h, w) == (orc.T2D_H, orc.T2D_W):
        return orc.depth_to_camera_cloud(depth)
    return _camera_cloud_any(depth)


def _camera_cloud_any(depth):
    h, w = depth.shape
    f = h / (2 * math.tan(math.radians(FOV / 2)))
    xmap, ymap = np.meshgrid(np.arange(w), np.arange(h))
    x = (xmap - w / 2) * depth / f
    y = (ymap - h / 2) * depth / f
    return np.stack([depth, -x, -y], axis=-1).reshape(-1, 3)


def tactile_pc(pred, height, width, cam_pos, cam_rot, pc_ply):
    """pred [n, height * width] float32 (the depth estimator's output), cam_pos / cam_rot [n, 3], pc_ply [T, 3] (float32, the scene's
    object cloud) -> [n, height * width, 3] float64, as the reference's loop body computes it."""
    pred = np.asarray(pred, dtype=np.float32)
    pc_ply = np.asarray(pc_ply)
    centroid = np.mean(pc_ply, axis=0)
    m = np.max(np.sqrt(np.sum((pc_ply - centroid) ** 2, axis=1)))
    out = np.zeros((pred.shape[0], height * width, 3))
    for t in range(pred.shape[0]):
        depth = pred[t].reshape(height, width) * 0.005 + 0.019                       # float32, as numpy keeps a float32 array
        world = orc.cam_to_world(camera_cloud(depth), np.asarray(cam_rot[t]) + np.array([-np.pi / 2, 0, np.pi / 2]), cam_pos[t])
        out[t] = (world - centroid) / (2 * m)
    return out


class _InKeyOrder:
    """A module's state_dict in a given key order (``seeded_fill`` draws in state_dict order, and the reference's UpConv registers its
    transposed conv BEFORE conv1 / conv2 / bn where vtaco_amd's registers it after them: same keys, another order)."""

    def __init__(self, module, keys):
        self.module, self.names = module, [k.rsplit(":", 1)[0] for k in keys]

    def state_dict(self):
        sd = self.module.state_dict()
        return {k: sd[k] for k in self.names}


def fill_like_the_golden(net, golden):
    """The weights the golden's reference network had: ``seeded_fill`` with the golden's seed in the golden's key order."""
    from seeded_fill import keys_of, seeded_fill
    keys = [str(k) for k in golden["keys"]]
    assert sorted(keys_of(net)) == sorted(keys)
    seeded_fill(_InKeyOrder(net, keys), int(golden["weight_seed"]))
    return net
