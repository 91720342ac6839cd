"""GPU: the hand-object evaluation of vtaco_amd.eval (signed_distance, penetration_depth, mesh_distances: vt_closest_point_mesh and
vt_winding_number) and Trainer.eval_step(hand_metrics=True) against tests/hand_metrics_ref.py, the numpy restatement of the reference's
eval_step (training.py:393-419).

eval_step's gate is float32-level in the project's way (tests/test_decode_train_f64_gpu.py): |got - ref64| <= 8 max(e32, 2^-24 bound),
ref64 the restatement in float64 fed with the model's own mano_verts / mano_joints, e32 the distance of the same restatement run in float32,
bound the magnitude the value is built from: the value itself for the Chamfer distance and the joint error (sums of positive terms), the
scale times the largest coordinate 1-norm of hand and mesh for the penetration depth (a coordinate rounded to float32 moves a distance by
that much).  Every comparison prints `RATIO <key>: err / gate-base`."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import closest_point_ref as C
import hand_metrics_ref as H
import synth_mano

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GATE = 8.0
MANO_KW = dict(center_idx=9, flat_hand_mean=False, ncomps=45, side="right", use_pca=False,
               root_rot_mode="axisang", joint_rot_mode="axisang", robust_rot=False, return_transf=False)
T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def test_signed_distance_sign_matches_containment():
    from vtaco_amd.eval import signed_distance
    rng = np.random.RandomState(3)
    pts = (rng.rand(500, 3) - 0.5).astype(np.float32)                      # the cube is [-0.25, 0.25]^3
    pts = pts[np.abs(np.abs(pts).max(1) - 0.25) > 1e-3]                    # (none on the surface: the sign there is the winding number's)
    sd = signed_distance(T(pts), T(C.CUBE_V), T(C.CUBE_F)).cpu().numpy()
    inside = np.abs(pts).max(1) < 0.25
    assert sd.dtype == np.float64 and 50 < inside.sum() < 450
    assert np.array_equal(sd < 0, inside)
    # inside, the distance to the surface of an axis-aligned cube is 0.25 - the largest |coordinate|
    want = 0.25 - np.abs(pts[inside].astype(np.float64)).max(1)
    assert np.abs(-sd[inside] - want).max() <= 4 * 2.0 ** -53
    d2, _, _ = C.by_regions(C.CUBE_V, C.CUBE_F, pts)
    assert (np.abs(np.abs(sd) - np.sqrt(d2)) <= 2.0 ** -52 * np.sqrt(d2)).all()


def test_penetration_depth_of_a_hand_outside_and_pushed_inside():
    from vtaco_amd.eval import penetration_depth, penetration_depth_scenes
    rng = np.random.RandomState(5)
    hand = (rng.rand(778, 3).astype(np.float32) * 0.25 + np.float32(0.5))  # all outside: [0.5, 0.75]^3
    v, f = T(C.CUBE_V), T(C.CUBE_F)
    assert penetration_depth(T(hand), v, f, 3.0) == 0.0
    # one vertex pushed 1/16 under the +x face, one 1/32 under the -z face: dyadic coordinates, the depth is exact
    hand[7] = [0.25 - 0.0625, 0.03125, -0.0625]
    hand[400] = [0.0625, -0.125, -0.25 + 0.03125]
    for scale in (3.0, 1.7):                                               # to float64 rounding
        assert abs(penetration_depth(T(hand), v, f, scale) - 0.0625 * scale) <= 4 * 2.0 ** -53 * 0.0625 * scale
        assert abs(H.penetration_depth(hand, C.CUBE_V, C.CUBE_F, scale) - 0.0625 * scale) <= 4 * 2.0 ** -53 * 0.0625 * scale
    tv, tf = C.torus(24, 12, seed=2)
    both = penetration_depth_scenes(T(np.stack([hand, hand])), [(v, f), (T(tv), T(tf))], [3.0, 2.0])
    assert both.dtype == np.float64 and abs(both[0] - 0.1875) <= 4 * 2.0 ** -53 * 0.1875
    assert abs(both[1] - H.penetration_depth(hand, tv, tf, 2.0)) <= 1e-14
    clear = penetration_depth_scenes(T(np.stack([hand[8:300], hand[8:300]])), [(T(tv), T(tf)), (v, f)], [2.0, 3.0])
    assert np.array_equal(clear, [0.0, 0.0])                               # neither mesh reaches [0.5, 0.75]^3


def test_mesh_distances_of_a_mesh_against_itself_and_its_translate():
    from vtaco_amd.eval import mesh_distances, sample_mesh_surface
    tv, tf = C.torus(24, 12, seed=4)
    v, f = T(tv), T(tf)
    gen = torch.Generator(device=DEV).manual_seed(1)
    pts, face = sample_mesh_surface(v, f, 4000, gen)
    assert pts.dtype == torch.float32 and tuple(pts.shape) == (4000, 3) and int(face.min()) >= 0 and int(face.max()) < len(tf)
    # area-weighted: the share of samples on the outer half of the torus' faces matches those faces' share of the area
    a, b, c = (tv[tf[:, k]].astype(np.float64) for k in range(3))
    area = 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1)
    big = area > np.median(area)
    share = float(big[face.cpu().numpy()].mean())
    assert abs(share - area[big].sum() / area.sum()) <= 4 * np.sqrt(0.25 / 4000)
    same = mesh_distances((v, f), (v, f), 2000, gen, threshold=1e-6)
    # a sample is a float32 rounding of a point of the surface (coordinates below 0.5: 2^-25 per axis) plus float64 rounding
    assert 0 <= same["accuracy"] <= 2.0 ** -24 and 0 <= same["completeness"] <= 2.0 ** -24
    assert same["f_score"] == 1.0 and same["chamfer_l1"] == 0.5 * (same["accuracy"] + same["completeness"])
    t = np.array([0.01, -0.02, 0.005], dtype=np.float32)
    moved = mesh_distances((T(tv + t), f), (v, f), 2000, gen, threshold=0.5 * float(np.linalg.norm(t)))
    limit = float(np.linalg.norm(t.astype(np.float64))) + 2.0 ** -22
    assert 0 < moved["accuracy"] <= limit and 0 < moved["completeness"] <= limit and 0 <= moved["f_score"] < 1.0
    far = mesh_distances((T(tv + np.float32(5.0)), f), (v, f), 500, gen, threshold=0.01)
    assert far["f_score"] == 0.0 and far["accuracy"] > 4.0


def _trainer_and_batch(tmp_path):
    from synth_dataset import make_cfg, make_synthetic_dataset
    from vtaco_amd import data
    from vtaco_amd.config import get_dataset
    from vtaco_amd.conv_onet import config as cfgmod
    dev = torch.device(DEV)
    os.makedirs(tmp_path / "ds")
    make_synthetic_dataset(str(tmp_path / "ds"), seed=5)
    synth_mano.write_pkl(synth_mano.make_asset(0), str(tmp_path / "mano"))
    cfg = make_cfg(str(tmp_path / "ds"), points_subsample=128)
    cfg["model"] = {"decoder": "simple_local", "encoder": "pointnet_local_pool", "c_dim": 32,
                    "decoder_kwargs": {"sample_mode": "bilinear", "hidden_size": 32},
                    "encoder_kwargs": {"hidden_dim": 32, "plane_type": "grid", "grid_resolution": 32, "unet3d": True,
                                       "unet3d_kwargs": {"num_levels": 3, "f_maps": 32, "in_channels": 32, "out_channels": 32}},
                    "encoder_hand": "pointnet_local_pool",
                    "encoder_hand_kwargs": {"hidden_dim": 32, "plane_type": ["xz", "xy", "yz"], "plane_resolution": 32,
                                            "unet": True, "unet_kwargs": {"depth": 3, "merge_mode": "concat", "start_filts": 16},
                                            "out_mano": True, "out_dim": 51,
                                            "manolayer_kwargs": dict(MANO_KW, mano_root=str(tmp_path / "mano"))}}
    cfg["test"] = {"threshold": 0.5}
    torch.manual_seed(0)
    model = cfgmod.get_model(cfg, device=dev)
    trainer = cfgmod.get_trainer(model, torch.optim.Adam(model.parameters(), lr=1e-3), cfg, dev)
    np.random.seed(0)
    batch = next(iter(torch.utils.data.DataLoader(get_dataset("train", cfg), batch_size=2, collate_fn=data.collate_remove_none)))
    return model, trainer, batch


def test_eval_step_hand_metrics_on_the_synthetic_dataset(tmp_path):
    from vtaco_amd._lib import VtError
    from vtaco_amd.common import hand_in_object_frame
    model, trainer, batch = _trainer_and_batch(tmp_path)
    names = list(batch["points.name"])
    assert len(names) == 2 and names[0] != names[1]
    mano_gt = batch["points.mano"].float()
    model.eval()
    with torch.no_grad():
        c_hand = model.encode_hand_inputs(batch["inputs"].to(DEV))
        joints_gt = model.encode_hand_mano(torch.cat((torch.zeros(2, 3), mano_gt[:, 6:]), dim=1).to(DEV))["mano_joints"].cpu().numpy()
    mano_verts, joints_pred = c_hand["mano_verts"].cpu().numpy(), c_hand["mano_joints"].cpu().numpy()
    wrist_pos, wrist_euler, pc_ply = mano_gt.numpy()[:, :3], batch["points.wrist"].numpy(), batch["inputs.pc_ply"].numpy()
    # scene 0: a cube round the centre of where the predicted hand lands, as wide as half the hand's extent (part of it is inside);
    # scene 1: a torus well away from its hand (depth 0) -- meshes of different sizes, both paths of the depth
    hand = hand_in_object_frame(mano_verts, wrist_pos, wrist_euler, pc_ply)
    centre, extent = hand[0].mean(0), float(np.ptp(hand[0], axis=0).max())
    cube_v = (C.CUBE_V.astype(np.float64) * extent + centre).astype(np.float32)
    tv, tf = C.torus(24, 12, seed=2)
    tv = (tv + (hand[1].max(0) + 1.0)).astype(np.float32)
    vf = {names[0]: {"v": cube_v, "f": C.CUBE_F}, names[1]: {"v": tv, "f": tf}}
    meshes = [(cube_v, C.CUBE_F), (tv, tf)]

    plain = trainer.eval_step(batch)
    today = ["loss"] + (["iou"] if "points_iou" in batch else [])           # (no voxels in this dataset)
    assert sorted(plain) == sorted(today)
    out = trainer.eval_step(batch, vf, hand_metrics=True)
    assert sorted(out) == sorted(today + ["chamfer_distance", "hand_joints_error", "penetration_depth"])
    assert all(out[k] == plain[k] for k in today) and trainer.eval_step(batch, vf) == plain

    args = (batch["points.pc_hand"].numpy(), mano_verts, joints_gt, joints_pred, wrist_pos, wrist_euler, pc_ply, meshes)
    r64, r32 = H.hand_metrics(*args, dtype=np.float64), H.hand_metrics(*args, dtype=np.float32)
    assert r64["per_scene_depth"][0] > 0 and r64["per_scene_depth"][1] == 0
    scale0 = float(np.max(np.sqrt(np.sum(pc_ply[0].astype(np.float64) ** 2, axis=1))))
    bound = {"chamfer_distance": abs(r64["chamfer_distance"]), "hand_joints_error": abs(r64["hand_joints_error"]),
             # (the mean over two scenes, one of depth 0)
             "penetration_depth": 0.5 * scale0 * float(np.abs(hand[0]).sum(1).max() + np.abs(cube_v.astype(np.float64)).sum(1).max())}
    for key in ("chamfer_distance", "hand_joints_error", "penetration_depth"):
        e32 = abs(r32[key] - r64[key])
        base = max(e32, 2.0 ** -24 * bound[key])
        ratio = abs(out[key] - r64[key]) / base
        print(f"RATIO {key}: {ratio:.3f} (got {out[key]:.9g}, ref64 {r64[key]:.9g}, e32 {e32:.3e}, 2^-24 bound {2.0 ** -24 * bound[key]:.3e})")
        assert ratio <= GATE, f"{key}: |got - ref64| is {ratio:.3f} x max(e32, 2^-24 bound), above {GATE}"

    mean = trainer.evaluate([batch, batch], vf, hand_metrics=True)
    assert sorted(mean) == sorted(out) and all(abs(mean[k] - out[k]) <= 1e-12 * max(1.0, abs(out[k])) for k in out)
    assert sorted(trainer.evaluate([batch])) == sorted(today)

    # every input the flag needs is named when it is missing
    with pytest.raises(VtError, match="vf_dict"):
        trainer.eval_step(batch, None, hand_metrics=True)
    for key in ("points.mano", "points.pc_hand", "points.wrist", "inputs.pc_ply", "points.name"):
        with pytest.raises(VtError, match=key.replace(".", r"\.")):
            trainer.eval_step({k: v for k, v in batch.items() if k != key}, vf, hand_metrics=True)
    with pytest.raises(VtError, match=names[1]):
        trainer.eval_step(batch, {names[0]: vf[names[0]]}, hand_metrics=True)
    hand_encoder, model.encoder_hand = model.encoder_hand, None
    try:
        with pytest.raises(VtError, match="hand encoder"):
            trainer.eval_step(batch, vf, hand_metrics=True)
    finally:
        model.encoder_hand = hand_encoder
