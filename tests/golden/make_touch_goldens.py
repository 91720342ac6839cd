#!/usr/bin/env python3
"""Golden vectors for the multi-touch Inferencer (g23_touch.npz) from the REAL reference: ``Inferencer.inference_step``
(src/conv_onet/inferencing.py) walks four touches of one object on both routes (VTacOH: inference_img, VTacO: inference_img_t2d)
and the per-point tactile tensor ``c_img_all`` it carries from touch to touch is recorded after every touch.

Build container only (needs the reference checkout).  The reference runs on a stand-in model: ``encode_img_inputs`` returns the
constant rows ``5 k + t + 1`` (touch k, finger t), so the dense c_img_all it hands to eval_points reads back as one table row per
lattice point; ``encode_hand_inputs`` returns seeded joints per touch; ``generator.eval_points`` is replaced by the recorder.
inferencing.py imports trimesh / skimage (not installed) and reads ./data/VTacO_mesh/depth_origin.txt at import: stand-ins for the
modules (marching_cubes_lewiner returns one triangle), and np.loadtxt answers that one read with THIS script's synthetic array.

Stored small: the depth images as the shared flat reading plus the pixels that differ, the id lattices as (index, row) pairs of
the occupied points.

    python tests/golden/make_touch_goldens.py
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_goldens as mg          # noqa: E402

W, H = 240, 320                    # inferencing.py:19-20 (w, h)
TOUCHES = 4
NX = 128                           # resolution0 32: the reference's t2d route is hard-wired to 8 x 64^3 points
SEED = 654


class Trimesh(object):
    def __init__(self, vertices, faces):
        self.vertices, self.faces = np.asarray(vertices), np.asarray(faces)


def _stub_modules():
    tm = types.ModuleType("trimesh")
    tm.Trimesh = Trimesh
    sk, skm = types.ModuleType("skimage"), types.ModuleType("skimage.measure")
    sk.measure = skm
    skm.marching_cubes_lewiner = lambda vol, **kw: (np.zeros((3, 3), dtype=np.float32), np.zeros((1, 3), dtype=np.int64), None, None)
    sys.modules.update({"trimesh": tm, "skimage": sk, "skimage.measure": skm})
    for name in ("matplotlib", "matplotlib.pyplot", "mpl_toolkits", "mpl_toolkits.mplot3d"):
        try:
            importlib.import_module(name)
        except ImportError:
            m = types.ModuleType(name)
            m.Axes3D = object
            sys.modules[name] = m
    if "matplotlib" in sys.modules and not hasattr(sys.modules["matplotlib"], "pyplot"):
        sys.modules["matplotlib"].pyplot = sys.modules["matplotlib.pyplot"]


class FakeGenerator(object):
    resolution0, padding = NX // 4, 0.1

    def __init__(self):
        self.rows = []

    def eval_points(self, p, c=None, c_img_all=None, **kw):
        self.rows.append(c_img_all[0, :, 0].round().to(torch.uint8).numpy().copy())
        return torch.zeros(p.shape[0])


class FakeModel(object):
    """encode_img_inputs: the rows 5 k + t + 1 of touch k; encode_hand_inputs: touch k's joints.  Both are called once per touch."""

    def __init__(self, joints):
        self.joints, self.k_img, self.k_hand = joints, 0, 0

    def eval(self):
        return self

    def encode_inputs(self, inputs):
        return "c"

    def encode_t2d(self, inputs, imgs):
        return torch.zeros(1, 5, W * H), {"mano_param": torch.zeros(1, 30)}

    def encode_hand_inputs(self, inputs):
        k, self.k_hand = self.k_hand, self.k_hand + 1
        return {"mano_param": torch.zeros(1, 51), "mano_verts": torch.zeros(1, 778, 3), "mano_faces": torch.zeros(1538, 3, dtype=torch.int64),
                "mano_joints": torch.from_numpy(self.joints[k])[None]}

    def encode_img_inputs(self, imgs):
        k, self.k_img = self.k_img, self.k_img + 1
        return (5 * k + torch.arange(5).float() + 1).view(1, 5, 1)


def _pairs(rows):
    """(index int32, row u8) of the occupied points; the recorder's 0 = no row, r + 1 = row r."""
    idx = np.nonzero(rows)[0].astype(np.int32)
    return idx, (rows[idx] - 1).astype(np.uint8)


def main():
    mg._install_stubs()
    _stub_modules()
    rs = np.random.RandomState(60)
    # the flat sensor reading: seven distinct values (compresses; the t2d rule only compares against it)
    depth_origin = 0.0215 + 1e-5 * rs.randint(-3, 4, size=W * H).astype(np.float64)
    loadtxt = np.loadtxt
    np.loadtxt = lambda *a, **k: depth_origin.copy()
    try:
        inferencing = importlib.import_module("src.conv_onet.inferencing")
    finally:
        np.loadtxt = loadtxt

    g = torch.Generator().manual_seed(61)
    pc_ply = torch.randn(1, 500, 3, generator=g) * 0.15 + 0.02
    cloud = pc_ply[0].numpy()
    centroid = cloud.mean(0)
    base = {"inputs": torch.zeros(1, 16, 3), "inputs.img": torch.zeros(1, 5, 3, 8, 6), "inputs.pc_ply": pc_ply,
            "points.points_obj": torch.zeros(1, 8, 3)}
    out = {"nx": np.array(NX), "pc_ply": pc_ply.numpy(), "seed": np.array(SEED)}

    # ---- VTacOH: fingertips from the joints; the hand drifts a few centimetres per touch, so later touches overlap earlier ones
    joints = (np.array([0.11, 0.005, 0.0]) + 0.06 * rs.randn(TOUCHES, 21, 3)).astype(np.float32)
    joints[1:] = joints[0] + (0.012 * rs.randn(TOUCHES - 1, 21, 3)).astype(np.float32)
    mano = np.zeros((TOUCHES, 51), dtype=np.float32)
    mano[:, :3] = centroid + np.array([0.12, -0.05, 0.08]) + np.cumsum(0.03 * rs.randn(TOUCHES, 3), axis=0)
    wrist = (np.array([0.4, -0.7, 1.1]) + 0.05 * rs.randn(TOUCHES, 3)).astype(np.float32)
    touch_h = np.array([[1, 1, 1, 0, 1], [1, 0, 1, 1, 1], [1, 1, 0, 1, 1], [1, 1, 1, 1, 1]], dtype=bool)
    seq = [{"data": dict(base, **{"inputs.touch_success": torch.from_numpy(touch_h[k:k + 1]), "points.mano": torch.from_numpy(mano[k:k + 1]),
                                  "points.wrist": torch.from_numpy(wrist[k:k + 1])})} for k in range(TOUCHES)]
    gen = FakeGenerator()
    inf = inferencing.Inferencer(FakeModel(joints), None, gen, device="cpu", with_img=True, encode_t2d=False)
    objs, hands = inf.inference_step(seq)
    assert len(objs) == len(hands) == len(gen.rows) == TOUCHES
    out.update({"h.joints": joints, "h.mano": mano, "h.wrist": wrist, "h.touch": touch_h})
    prev = np.zeros(NX ** 3, dtype=np.uint8)
    for k, rows in enumerate(gen.rows):
        out[f"h.idx_{k}"], out[f"h.row_{k}"] = _pairs(rows)
        print(f"VTacOH touch {k}: {int((rows != prev).sum())} points changed, {int((rows != 0).sum())} occupied")
        prev = rows
    print("VTacOH rows in the final lattice:", sorted(set((gen.rows[-1][gen.rows[-1] != 0] - 1).tolist())))

    # ---- VTacO (t2d): contact clouds from the depth images; the sensors move a little per touch
    yy, xx = np.mgrid[0:H, 0:W]
    flat = depth_origin.astype(np.float32)
    depths = np.repeat(flat[None, None, :], TOUCHES, axis=0).repeat(5, axis=1)
    for k in range(TOUCHES):
        for t in range(5):
            cy, cx, rad = rs.randint(40, H - 40), rs.randint(40, W - 40), (30, 5, 14, 8, 20)[(t + k) % 5]
            blob = (((yy - cy) ** 2 + (xx - cx) ** 2) < rad ** 2).reshape(-1)
            depths[k, t, blob] -= (0.0004 + 0.001 * rs.rand(int(blob.sum()))).astype(np.float32)
    d = rs.randn(5, 3)
    cam_pos0 = 0.18 * d / np.linalg.norm(d, axis=1, keepdims=True)
    cam_rot0 = 0.8 * rs.randn(5, 3)
    cam_pos = (cam_pos0[None] + 0.004 * rs.randn(TOUCHES, 5, 3)).astype(np.float32)
    cam_rot = (cam_rot0[None] + 0.02 * rs.randn(TOUCHES, 5, 3)).astype(np.float32)
    touch_d = np.array([[1, 1, 1, 0, 1], [1, 1, 0, 1, 1], [0, 1, 1, 1, 1], [1, 1, 1, 1, 1]], dtype=bool)
    seq = [{"data": dict(base, **{"inputs.depth": torch.from_numpy(depths[k:k + 1]), "inputs.touch_success": torch.from_numpy(touch_d[k:k + 1]),
                                  "points.mano": torch.zeros(1, 51), "points.wrist": torch.zeros(1, 3),
                                  "points.cam_pos": torch.from_numpy(cam_pos[k:k + 1]), "points.cam_rot": torch.from_numpy(cam_rot[k:k + 1])})}
           for k in range(TOUCHES)]
    gen = FakeGenerator()
    inf = inferencing.Inferencer(FakeModel(joints), None, gen, device="cpu", with_img=True, encode_t2d=True)
    np.random.seed(SEED)                                             # ONE seed: the randint draws run on through the sequence
    objs, hands = inf.inference_step(seq)
    assert len(objs) == len(hands) == len(gen.rows) == TOUCHES
    out.update({"d.depth_origin": depth_origin, "d.cam_pos": cam_pos, "d.cam_rot": cam_rot, "d.touch": touch_d})
    prev = np.zeros(NX ** 3, dtype=np.uint8)
    for k, rows in enumerate(gen.rows):
        diff = np.nonzero(depths[k].reshape(-1) != np.tile(flat, 5))[0].astype(np.int32)
        out[f"d.dep_idx_{k}"], out[f"d.dep_val_{k}"] = diff, depths[k].reshape(-1)[diff]
        out[f"d.idx_{k}"], out[f"d.row_{k}"] = _pairs(rows)
        print(f"VTacO touch {k}: {int((rows != prev).sum())} points changed, {int((rows != 0).sum())} occupied")
        prev = rows
    print("VTacO rows in the final lattice:", sorted(set((gen.rows[-1][gen.rows[-1] != 0] - 1).tolist())))
    mg._save("g23_touch.npz", **out)


if __name__ == "__main__":
    main()
