"""numpy restatement of the touch session's accumulation rule (reference src/conv_onet/inferencing.py:155-170, 274-313) and the
readers of its fixture g23_touch.npz, shared by tests/test_touch_cpu.py and tests/test_touch_gpu.py.

The id lattice holds one table row per point (255 = none); touch k owns rows 5 k .. 5 k + 4.  A touch assigns fingers by the rule
of vt_tactile_assign (anchors rounded to float32, distances in float64 like scipy's cdist: VTacOH = the nearest fingertip within
0.05 if its touch succeeded, VTacO = within 0.015 of a finger's contact points, later fingers overwrite) and writes its rows where
a finger was named; everything else keeps the earlier touches' rows."""
import os

import numpy as np
import torch

from conftest import GOLDEN

BOX = 1.1
W, H = 240, 320
ROUTES = {"h": ("nearest", 0.05), "d": ("within", 0.015)}


def fixture():
    return np.load(os.path.join(GOLDEN, "g23_touch.npz"))


def touches(z):
    return int(z["h.touch"].shape[0])


def lattice_axis(nx, box=BOX):
    """box * linspace(-0.5, 0.5, nx) in float32 (make_3d_grid's axis), as float64."""
    return (box * torch.linspace(-0.5, 0.5, nx)).numpy().astype(np.float64)


def assign(nx, anchors, count, success, mode, radius, box=BOX):
    """Finger per lattice point (uint8 [nx^3], 255 = none) of one touch.  anchors [F,K,3] (used as float32), count [F], success [F].
    Only the block of the lattice within ``radius`` of the anchors' bounds is evaluated: a point outside it is further than the
    radius from every anchor along one axis."""
    ax = lattice_axis(nx, box)
    anchors = np.asarray(anchors, dtype=np.float32).astype(np.float64)
    ids = np.full((nx, nx, nx), 255, dtype=np.uint8)
    F = anchors.shape[0]

    def block(pts):
        lo, hi = pts.min(0) - radius * (1 + 1e-9), pts.max(0) + radius * (1 + 1e-9)
        sl = []
        for c in range(3):
            inside = np.nonzero((ax >= lo[c]) & (ax <= hi[c]))[0]
            if inside.size == 0:
                return None
            sl.append(slice(int(inside[0]), int(inside[-1]) + 1))
        gx, gy, gz = np.meshgrid(ax[sl[0]], ax[sl[1]], ax[sl[2]], indexing="ij")
        return tuple(sl), np.stack([gx, gy, gz], axis=-1).reshape(-1, 3)

    if mode == "nearest":
        ok = [f for f in range(F) if success[f]]
        if not ok:
            return ids.reshape(-1)
        got = block(anchors[ok, 0])
        if got is None:
            return ids.reshape(-1)
        sl, p = got
        d = np.sqrt(((p[:, None, :] - anchors[None, :, 0, :]) ** 2).sum(-1))
        arg, best = d.argmin(1), d.min(1)                          # first minimum
        hit = (best < radius) & np.asarray(success, dtype=bool)[arg]
        sub = np.where(hit, arg, 255).astype(np.uint8)
        ids[sl] = sub.reshape(ids[sl].shape)
        return ids.reshape(-1)
    for f in range(F):                                              # ascending: later fingers overwrite
        n = int(count[f])
        if not success[f] or n == 0:
            continue
        got = block(anchors[f, :n])
        if got is None:
            continue
        sl, p = got
        d = np.sqrt(((anchors[f, :n][:, None, :] - p[None, :, :]) ** 2).sum(-1))
        hit = (d < radius).any(0).reshape(ids[sl].shape)
        ids[sl][hit] = f
    return ids.reshape(-1)


def merge(ids, fingers, row_base):
    """The session's lattice after one more touch (a new array) and the ascending list of the points it changed."""
    hit = fingers != 255
    out = ids.copy()
    out[hit] = (row_base + fingers[hit]).astype(np.uint8)
    return out, np.nonzero(hit)[0].astype(np.int32)


def expected(z, route, k):
    """The reference's id lattice after touch k (uint8 [nx^3], 255 = none)."""
    nx = int(z["nx"])
    ids = np.full(nx ** 3, 255, dtype=np.uint8)
    ids[z[f"{route}.idx_{k}"]] = z[f"{route}.row_{k}"]
    return ids


def depths_of(z, k):
    """Touch k's five depth images [5, H*W] float32: the flat reading plus the stored pixels."""
    d = np.tile(z["d.depth_origin"].astype(np.float32), 5)
    d[z[f"d.dep_idx_{k}"]] = z[f"d.dep_val_{k}"]
    return d.reshape(5, W * H)


def sample(z, route, k):
    """Touch k as the sample dictionary the Inferencer reads (no images: the tests' encoders take what they are given)."""
    data = {"inputs.pc_ply": torch.from_numpy(z["pc_ply"]), "inputs.touch_success": torch.from_numpy(z[f"{route}.touch"][k:k + 1])}
    if route == "h":
        data.update({"points.mano": torch.from_numpy(z["h.mano"][k:k + 1]), "points.wrist": torch.from_numpy(z["h.wrist"][k:k + 1])})
    else:
        data.update({"inputs.depth": torch.from_numpy(depths_of(z, k))[None], "points.cam_pos": torch.from_numpy(z["d.cam_pos"][k:k + 1]),
                     "points.cam_rot": torch.from_numpy(z["d.cam_rot"][k:k + 1]), "points.mano": torch.zeros(1, 51),
                     "points.wrist": torch.zeros(1, 3)})
    return data


def anchors_of(z, route, k):
    """(anchors float32 [5,K,3], count int32 [5], success uint8 [5]) of touch k through the project's host functions (the t2d route
    draws from numpy's global generator: seed once with z['seed'] and call for k = 0, 1, ... in order)."""
    from vtaco_amd.common import contact_clouds_from_depth, fingertips_in_object_frame
    touch = z[f"{route}.touch"][k]
    if route == "h":
        tips = fingertips_in_object_frame(z["h.joints"][k:k + 1], z["h.mano"][k:k + 1, :3], z["h.wrist"][k:k + 1], z["pc_ply"])
        return tips[0].astype(np.float32)[:, None, :], np.ones(5, dtype=np.int32), touch.astype(np.uint8)
    anchors, count = contact_clouds_from_depth(depths_of(z, k), z["d.depth_origin"], z["d.cam_pos"][k], z["d.cam_rot"][k], z["pc_ply"][0], touch)
    return anchors.astype(np.float32), count.astype(np.int32), (count > 0).astype(np.uint8)


def walk(z, route, order=None):
    """Per touch of ``order`` (default 0 .. T-1): (anchors, count, success, lattice after the touch, changed list) by the numpy rule.
    Row base of the i-th touch fed is 5 i."""
    nx = int(z["nx"])
    mode, radius = ROUTES[route]
    order = list(range(touches(z))) if order is None else list(order)
    state = np.random.get_state()
    try:
        np.random.seed(int(z["seed"]))
        setups = {}
        for k in sorted(set(order)):                                # the draws of the fixture's own sequence, in its order
            setups[k] = anchors_of(z, route, k)
    finally:
        np.random.set_state(state)
    ids = np.full(nx ** 3, 255, dtype=np.uint8)
    out = []
    for i, k in enumerate(order):
        anchors, count, success = setups[k]
        ids, changed = merge(ids, assign(nx, anchors, count, success, mode, radius), 5 * i)
        out.append((anchors, count, success, ids, changed))
    return out
