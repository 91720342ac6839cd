"""The MANO hand layer (vt_mano_*)."""
import torch

from ._base import _lib, check, dev_ptr, stream_ptr, _c


MANO_BLOB_FLOATS = 330240


def mano_pack(v_template, shapedirs, betas, posedirs, j_regressor, weights, hands_mean, left=False):
    """Model arrays (f32, on the device) -> the blob vt_mano_fwd reads (vt_mano_pack_side; ``left``: a MANO_LEFT model)."""
    dev = v_template.device
    want = {"v_template": (v_template, (778, 3)), "posedirs": (posedirs, (778, 3, 135)),
            "j_regressor": (j_regressor, (16, 778)), "weights": (weights, (778, 16)), "hands_mean": (hands_mean, (45,))}
    if betas is not None:
        want["shapedirs"], want["betas"] = (shapedirs, (778, 3, 10)), (betas, (10,))
    arrs = {}
    for name, (t, shape) in want.items():
        if tuple(t.shape) != shape:
            raise _lib.VtError(f"mano_pack: {name} has shape {tuple(t.shape)}, expected {shape}")
        arrs[name] = _c(t.float())
    blob = torch.empty(MANO_BLOB_FLOATS, dtype=torch.float32, device=dev)
    check(_lib.load().vt_mano_pack_side(dev_ptr(arrs["v_template"], "v_template"), dev_ptr(arrs.get("shapedirs"), "shapedirs"),
                                        dev_ptr(arrs.get("betas"), "betas"), dev_ptr(arrs["posedirs"], "posedirs"),
                                        dev_ptr(arrs["j_regressor"], "j_regressor"), dev_ptr(arrs["weights"], "weights"),
                                        dev_ptr(arrs["hands_mean"], "hands_mean"), int(bool(left)), dev_ptr(blob, "blob"), stream_ptr()),
          "vt_mano_pack_side")
    return blob


def mano_fwd(pose, blob, center_idx=9):
    """pose [B,48] -> (verts [B,778,3], joints [B,21,3]) (vt_mano_fwd)."""
    pose = _c(pose.float())
    if pose.dim() != 2 or pose.shape[1] != 48:
        raise _lib.VtError(f"mano_fwd: pose must be [B,48] (root axis-angle + 45 joint angles), got {tuple(pose.shape)}")
    B = pose.shape[0]
    verts = torch.empty((B, 778, 3), dtype=torch.float32, device=pose.device)
    joints = torch.empty((B, 21, 3), dtype=torch.float32, device=pose.device)
    check(_lib.load().vt_mano_fwd(dev_ptr(pose, "pose"), B, dev_ptr(blob, "blob"),
                                  -1 if center_idx is None else int(center_idx),
                                  dev_ptr(verts, "verts"), dev_ptr(joints, "joints"), stream_ptr()), "vt_mano_fwd")
    return verts, joints


def mano_bwd(pose, blob, center_idx, dverts, djoints):
    """d pose [B,48] of mano_fwd from d verts [B,778,3] and d joints [B,21,3] (vt_mano_bwd)."""
    pose = _c(pose.float())
    B = pose.shape[0]
    dverts = _c(dverts.float()) if dverts is not None else torch.zeros((B, 778, 3), dtype=torch.float32, device=pose.device)
    djoints = _c(djoints.float()) if djoints is not None else torch.zeros((B, 21, 3), dtype=torch.float32, device=pose.device)
    dpose = torch.empty((B, 48), dtype=torch.float32, device=pose.device)
    check(_lib.load().vt_mano_bwd(dev_ptr(pose, "pose"), B, dev_ptr(blob, "blob"), -1 if center_idx is None else int(center_idx),
                                  dev_ptr(dverts, "dverts"), dev_ptr(djoints, "djoints"), dev_ptr(dpose, "dpose"), stream_ptr()), "vt_mano_bwd")
    return dpose
