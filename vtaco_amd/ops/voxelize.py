"""Mesh -> occupancy volume (vt_voxelize_surface, vt_voxelize_interior, vt_voxel_fill): the launchers behind
``vtaco_amd.utils.voxels`` (src/utils/voxels.py).  A submodule only: callers write ``ops.voxelize.surface``."""
import ctypes

import torch

from ._base import _lib, VtError, check, dev_ptr, stream_ptr, I32, U8, _c


MAX_RES = 512                 # VT_VOXELIZE_MAX_RES
FILL_ROUNDS_PER_RES = 4       # vt_voxel_fill rounds before `fill` gives up: 4 * res


def _mesh(verts, faces, res, loc, scale, what):
    if not (torch.is_tensor(verts) and torch.is_tensor(faces)):
        raise VtError(f"{what}: verts and faces must be tensors")
    if not (verts.is_cuda and faces.is_cuda) or verts.device != faces.device:
        raise VtError(f"{what}: verts and faces must live on one HIP device (got {verts.device}, {faces.device}); vtaco_amd has no CPU path")
    res = int(res)
    if not 1 <= res <= MAX_RES:
        raise VtError(f"{what}: resolution {res} is outside 1..{MAX_RES}")
    if verts.dim() != 2 or verts.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise VtError(f"{what}: expected verts [V,3] and faces [F,3] (got {tuple(verts.shape)} and {tuple(faces.shape)})")
    if verts.dtype != torch.float32 or faces.dtype not in (torch.int32, torch.int64):
        raise VtError(f"{what}: verts must be float32 and faces int32 or int64 (got {verts.dtype}, {faces.dtype})")
    scale = float(scale)
    if not scale > 0:
        raise VtError(f"{what}: scale must be > 0 (got {scale})")
    V, F = verts.shape[0], faces.shape[0]
    if F > 0:
        lo, hi = int(faces.min()), int(faces.max())
        if lo < 0 or hi >= V:
            raise VtError(f"{what}: face indices span {lo}..{hi}, the mesh has {V} vertices")
    loc3 = (ctypes.c_double * 3)(*[float(x) for x in loc])
    return _c(verts), _c(faces.to(I32)), V, F, loc3, scale, res


def surface(verts, faces, res, loc=(0.0, 0.0, 0.0), scale=1.0):
    """u8 [res, res, res] ([x][y][z]): 1 where the voxel's closed box overlaps a triangle (13-axis separating-axis test in float64 on
    g = ((v - loc) / scale + 0.5) * res).  verts [V,3] f32, faces [F,3] i32 / i64 on the device; an empty mesh gives an empty volume."""
    verts, faces, V, F, loc3, scale, res = _mesh(verts, faces, res, loc, scale, "voxelize.surface")
    occ = torch.zeros((res, res, res), dtype=U8, device=verts.device)
    check(_lib.load().vt_voxelize_surface(dev_ptr(verts, "verts") if V else None, V, dev_ptr(faces, "faces", I32) if F else None, F, loc3, scale, res,
                                          dev_ptr(occ, "occ", U8), stream_ptr()), "vt_voxelize_surface")
    return occ


def interior(verts, faces, res, loc=(0.0, 0.0, 0.0), scale=1.0):
    """i32 [res, res, ceil(res / 32)] bit masks (bit k % 32 of word k // 32 = voxel [x][y][k]): parity of the crossings of the +z ray
    from every voxel centre; bit-reproducible (integer XOR)."""
    verts, faces, V, F, loc3, scale, res = _mesh(verts, faces, res, loc, scale, "voxelize.interior")
    bits = torch.zeros((res, res, (res + 31) // 32), dtype=I32, device=verts.device)
    check(_lib.load().vt_voxelize_interior(dev_ptr(verts, "verts") if V else None, V, dev_ptr(faces, "faces", I32) if F else None, F, loc3, scale, res,
                                           dev_ptr(bits, "bits", I32), stream_ptr()), "vt_voxelize_interior")
    return bits


def fill(occ, max_rounds=None):
    """(outside u8 [res]^3, rounds): the unoccupied voxels connected to the grid's boundary through unoccupied voxels (6-connectivity);
    scipy.ndimage.binary_fill_holes(occ) is ``outside == 0``.  Rounds of six line sweeps until one changes nothing; more than
    ``max_rounds`` (default 4 * res) raises VtError."""
    if not torch.is_tensor(occ) or occ.dim() != 3 or not (occ.shape[0] == occ.shape[1] == occ.shape[2]):
        raise VtError("voxelize.fill: occ must be a cubic u8 volume")
    res = occ.shape[0]
    if not 1 <= res <= MAX_RES:
        raise VtError(f"voxelize.fill: resolution {res} is outside 1..{MAX_RES}")
    occ = _c(occ)
    cap = FILL_ROUNDS_PER_RES * res if max_rounds is None else int(max_rounds)
    outside = torch.zeros_like(occ)
    changed = torch.zeros((1,), dtype=I32, device=occ.device)
    lib = _lib.load()
    rounds = 0
    while True:
        if rounds >= cap:
            raise VtError(f"voxelize.fill: the fill did not finish within {cap} rounds at resolution {res}")
        changed.zero_()
        check(lib.vt_voxel_fill(dev_ptr(occ, "occ", U8), res, dev_ptr(outside, "outside", U8), dev_ptr(changed, "changed", I32), stream_ptr()),
              "vt_voxel_fill")
        rounds += 1
        if int(changed.item()) == 0:
            return outside, rounds
