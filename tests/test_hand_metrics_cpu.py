"""CPU: the host side of the hand metrics (vtaco_amd.common.hand_in_object_frame, vtaco_amd.eval.hand_joint_error) and the numpy
restatement of the reference's eval_step terms (tests/hand_metrics_ref.py) that the GPU tests compare against."""
import numpy as np
import pytest
import torch

import closest_point_ref as C
import hand_metrics_ref as H


def _scene(seed, B=3, K=21):
    rng = np.random.RandomState(seed)
    return (rng.randn(B, K, 3).astype(np.float32) * 0.1, rng.randn(B, 3).astype(np.float32) * 0.2, rng.randn(B, 3).astype(np.float32),
            rng.randn(B, 100, 3).astype(np.float32) * 0.3)


@pytest.mark.parametrize("K", [21, 778])
def test_hand_in_object_frame_is_the_fingertip_transform(K):
    from vtaco_amd.common import fingertips_in_object_frame, hand_in_object_frame
    pts, wrist_pos, wrist_euler, pc_ply = _scene(4, K=K)
    whole = hand_in_object_frame(pts, wrist_pos, wrist_euler, pc_ply)
    assert whole.dtype == np.float64 and whole.shape == (3, K, 3)
    tips = fingertips_in_object_frame(pts[:, :21], wrist_pos, wrist_euler, pc_ply)
    assert np.array_equal(whole[:, [4, 8, 12, 16, 20]].view(np.uint8), tips.view(np.uint8))           # bit for bit
    # the reference's eval_step writes the same transform as rows times transposed inverses (training.py:399-404)
    for b in range(3):
        ref = H.hand_to_object_frame(pts[b], wrist_pos[b], wrist_euler[b], pc_ply[b])
        assert np.abs(whole[b] - ref).max() <= 64 * 2.0 ** -53 * max(1.0, np.abs(ref).max())


def test_hand_joint_error_of_a_hand_computed_case():
    from vtaco_amd._lib import VtError
    from vtaco_amd.eval import hand_joint_error
    gt = np.zeros((2, 4, 3), dtype=np.float32)
    pred = np.zeros((2, 4, 3), dtype=np.float32)
    pred[0, :, 0] = [3, 0, 0, 6]
    pred[0, :, 1] = [4, 0, 8, 0]                       # distances 5, 0, 8, 6 -> mean 4.75
    pred[1, 2] = [1, 2, 2]                             # 0, 0, 3, 0 -> 0.75
    err = hand_joint_error(torch.from_numpy(gt), torch.from_numpy(pred))
    assert err.dtype == np.float64 and np.array_equal(err, [4.75, 0.75])
    assert hand_joint_error(gt[0], pred[0]) == 4.75 and isinstance(hand_joint_error(gt[0], pred[0]), float)
    assert H.hand_joint_error(gt[0], pred[0]) == 4.75
    with pytest.raises(VtError):
        hand_joint_error(gt, pred[:, :3])


def test_reference_penetration_depth_on_a_cube():
    """A 0.5 cube: a point 1/16 under the +x face is inside at depth 1/16; points outside count for nothing."""
    hand = np.array([[0.25 - 0.0625, 0.03125, -0.0625], [0.5, 0, 0], [0.25 - 0.03125, 0.1, 0.1], [0, 0, 1]], dtype=np.float32)
    w = H.winding_number(C.CUBE_V, C.CUBE_F, hand)
    assert np.allclose(w, [1, 0, 1, 0], atol=1e-12)
    assert H.penetration_depth(hand, C.CUBE_V, C.CUBE_F, 3.0) == 3.0 * 0.0625
    assert H.penetration_depth(hand[[1, 3]], C.CUBE_V, C.CUBE_F, 3.0) == 0.0
    assert abs(float(H.penetration_depth(hand, C.CUBE_V, C.CUBE_F, 3.0, dtype=np.float32)) - 0.1875) <= 1e-6


def test_reference_chamfer_cuts_the_first_set():
    rng = np.random.RandomState(1)
    a, b = rng.randn(30, 3), rng.randn(20, 3)
    d = ((a[:20, None] - b[None]) ** 2).sum(-1)
    assert np.isclose(H.chamfer_naive(a, b), d.min(0).mean() + d.min(1).mean(), rtol=1e-15)
