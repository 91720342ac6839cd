"""Point -> voxel / plane indices and the pooling and scatter-mean kernels over them (vt_voxel_*, vt_plane_*)."""
import ctypes

import torch

from ._base import _lib, check, dev_ptr, stream_ptr, I32, _c, _ptr_array


class VoxelIndex:
    """Per-forward voxel bookkeeping of a point cloud [B,T,3] (vt_voxel_build).  ``clear``: a contiguous float tensor the same
    launch zero-fills with the workgroups the sort leaves idle (vt_voxel_build_clear: the mean grid, without a fill launch)."""

    def __init__(self, pts, reso, padding=0.1, clear=None, want_tile_flags=False):
        pts = _c(pts.float())
        B, T, _ = pts.shape
        self.B, self.T, self.R = B, T, reso
        dev = pts.device
        self.idx = torch.empty((B, T), dtype=I32, device=dev)
        self.order = torch.empty((B, T), dtype=I32, device=dev)
        self.seg_lo = torch.empty((B, T), dtype=I32, device=dev)
        self.seg_hi = torch.empty((B, T), dtype=I32, device=dev)
        # ``want_tile_flags``: uint8 [B, (reso/8)^3], 1 where no point lies in the 10^3 halo of that 8^3 block (voxel_tile_flags),
        # marked by the same launch (vt_voxel_build_clear_flags); None where the resolution is not covered
        self.tile_flags = None
        if want_tile_flags and reso % 8 == 0 and 8 <= reso <= 128:
            self.tile_flags = torch.empty((B, (reso // 8) ** 3), dtype=torch.uint8, device=dev)
            check(_lib.load().vt_voxel_build_clear_flags(dev_ptr(pts, "pts"), B, T, reso, float(padding),
                                                         dev_ptr(self.idx, "idx", I32), dev_ptr(self.order, "order", I32),
                                                         dev_ptr(self.seg_lo, "seg_lo", I32), dev_ptr(self.seg_hi, "seg_hi", I32),
                                                         dev_ptr(clear, "clear") if clear is not None else None,
                                                         clear.numel() * clear.element_size() if clear is not None else 0,
                                                         dev_ptr(self.tile_flags, "tile_flags", torch.uint8), stream_ptr()),
                  "vt_voxel_build_clear_flags")
            return
        if clear is not None:
            check(_lib.load().vt_voxel_build_clear(dev_ptr(pts, "pts"), B, T, reso, float(padding),
                                                   dev_ptr(self.idx, "idx", I32), dev_ptr(self.order, "order", I32),
                                                   dev_ptr(self.seg_lo, "seg_lo", I32), dev_ptr(self.seg_hi, "seg_hi", I32),
                                                   dev_ptr(clear, "clear"), clear.numel() * clear.element_size(), stream_ptr()),
                  "vt_voxel_build_clear")
            return
        check(_lib.load().vt_voxel_build(dev_ptr(pts, "pts"), B, T, reso, float(padding),
                                         dev_ptr(self.idx, "idx", I32), dev_ptr(self.order, "order", I32),
                                         dev_ptr(self.seg_lo, "seg_lo", I32), dev_ptr(self.seg_hi, "seg_hi", I32),
                                         stream_ptr()), "vt_voxel_build")


def voxel_tile_flags(vi):
    """uint8 [B, (R/8)^3]: 1 where no point of the scene lies in the 10^3 halo of that 8^3 voxel block (vt_voxel_tile_flags) -- the
    mean grid is zero over everything a 3x3x3 conv of the block reads, so the UNet3D's first layer can skip the block's taps
    (unet3d_fwd(tile_flags=...)).  None where the resolution is not covered (not a multiple of 8, or above 128)."""
    if vi.R % 8 or vi.R < 8 or vi.R > 128:
        return None
    flags = torch.empty((vi.B, (vi.R // 8) ** 3), dtype=torch.uint8, device=vi.idx.device)
    check(_lib.load().vt_voxel_tile_flags(dev_ptr(vi.idx, "idx", I32), vi.B, vi.T, vi.R, dev_ptr(flags, "flags", torch.uint8), stream_ptr()),
          "vt_voxel_tile_flags")
    return flags


def voxel_pool_max_fwd(feat, vi, want_argmax=True):
    feat = _c(feat)
    B, T, C = feat.shape
    out = torch.empty_like(feat)
    arg = torch.empty((B, T, C), dtype=I32, device=feat.device) if want_argmax else None
    check(_lib.load().vt_voxel_pool_max_fwd(dev_ptr(feat, "feat"), dev_ptr(vi.order, "order", I32),
                                            dev_ptr(vi.seg_lo, "seg_lo", I32), dev_ptr(vi.seg_hi, "seg_hi", I32),
                                            B, T, C, dev_ptr(out, "out"), dev_ptr(arg, "argmax", I32), stream_ptr()),
          "vt_voxel_pool_max_fwd")
    return out, arg


def voxel_pool_max_sum_fwd(feat, vis, want_argmax=True):
    """Sum over the index sets ``vis`` of the per-cell channel max, gathered back to the points (vt_voxel_pool_max_sum_fwd): one launch
    for the hand encoder's three planes.  Returns (out [B,T,C], list of arg-max tensors or None)."""
    feat = _c(feat)
    B, T, C = feat.shape
    K = len(vis)
    out = torch.empty_like(feat)
    args = [torch.empty((B, T, C), dtype=I32, device=feat.device) for _ in range(K)] if want_argmax else None
    check(_lib.load().vt_voxel_pool_max_sum_fwd(dev_ptr(feat, "feat"), K, _ptr_array([v.order for v in vis], "order"),
                                                _ptr_array([v.seg_lo for v in vis], "seg_lo"), _ptr_array([v.seg_hi for v in vis], "seg_hi"),
                                                B, T, C, dev_ptr(out, "out"), _ptr_array(args, "argmax") if args else None, stream_ptr()),
          "vt_voxel_pool_max_sum_fwd")
    return out, args


def voxel_pool_max_sum_bwd(grad_out, args, vis):
    grad_out = _c(grad_out)
    B, T, C = grad_out.shape
    g = torch.empty_like(grad_out)
    check(_lib.load().vt_voxel_pool_max_sum_bwd(dev_ptr(grad_out, "grad_out"), len(vis), _ptr_array(args, "argmax"),
                                                _ptr_array([v.order for v in vis], "order"), _ptr_array([v.seg_lo for v in vis], "seg_lo"),
                                                _ptr_array([v.seg_hi for v in vis], "seg_hi"), B, T, C, dev_ptr(g, "grad_feat"), stream_ptr()),
          "vt_voxel_pool_max_sum_bwd")
    return g


def voxel_pool_mean(feat, vi):
    """pool_local with scatter_type='mean' (vt_voxel_pool_mean): every point gets the mean of the features of its cell; its
    backward is the same call on the gradient."""
    feat = _c(feat.float())
    B, T, C = feat.shape
    out = torch.empty_like(feat)
    check(_lib.load().vt_voxel_pool_mean(dev_ptr(feat, "feat"), dev_ptr(vi.order, "order", I32), dev_ptr(vi.seg_lo, "seg_lo", I32),
                                         dev_ptr(vi.seg_hi, "seg_hi", I32), B, T, C, dev_ptr(out, "out"), stream_ptr()), "vt_voxel_pool_mean")
    return out


def voxel_pool_max_bwd(grad_out, argmax, vi):
    grad_out = _c(grad_out)
    B, T, C = grad_out.shape
    g = torch.empty_like(grad_out)
    check(_lib.load().vt_voxel_pool_max_bwd(dev_ptr(grad_out, "grad_out"), dev_ptr(argmax, "argmax", I32),
                                            dev_ptr(vi.order, "order", I32), dev_ptr(vi.seg_lo, "seg_lo", I32),
                                            dev_ptr(vi.seg_hi, "seg_hi", I32), B, T, C, dev_ptr(g, "grad_feat"), stream_ptr()),
          "vt_voxel_pool_max_bwd")
    return g


def voxel_scatter_mean_fwd(feat, vi):
    feat = _c(feat)
    B, T, C = feat.shape
    R = vi.R
    grid = torch.empty((B, C, R, R, R), dtype=torch.float32, device=feat.device)
    check(_lib.load().vt_voxel_scatter_mean_fwd(dev_ptr(feat, "feat"), dev_ptr(vi.idx, "idx", I32),
                                                dev_ptr(vi.order, "order", I32), dev_ptr(vi.seg_lo, "seg_lo", I32),
                                                dev_ptr(vi.seg_hi, "seg_hi", I32), B, T, C, R, dev_ptr(grid, "grid"),
                                                stream_ptr()), "vt_voxel_scatter_mean_fwd")
    return grid


def voxel_scatter_mean_bwd(grad_grid, vi, C):
    grad_grid = _c(grad_grid)
    B, T = vi.B, vi.T
    g = torch.empty((B, T, C), dtype=torch.float32, device=grad_grid.device)
    check(_lib.load().vt_voxel_scatter_mean_bwd(dev_ptr(grad_grid, "grad_grid"), dev_ptr(vi.idx, "idx", I32),
                                                dev_ptr(vi.seg_lo, "seg_lo", I32), dev_ptr(vi.seg_hi, "seg_hi", I32),
                                                B, T, C, vi.R, dev_ptr(g, "grad_feat"), stream_ptr()),
          "vt_voxel_scatter_mean_bwd")
    return g


PLANES = {"xz": 0, "xy": 1, "yz": 2}


class PlaneIndex(VoxelIndex):
    """VoxelIndex of one canonical plane (vt_plane_build): same fields, R^2 cells, so the
    voxel_pool_max_* wrappers take it unchanged."""

    def __init__(self, pts, reso, padding=0.1, plane="xz"):
        if plane not in PLANES:
            raise _lib.VtError(f"PlaneIndex: unknown plane {plane!r} (one of {sorted(PLANES)})")
        pts = _c(pts.float())
        B, T, _ = pts.shape
        self.B, self.T, self.R, self.plane = B, T, reso, plane
        dev = pts.device
        self.idx, self.order, self.seg_lo, self.seg_hi = (torch.empty((B, T), dtype=I32, device=dev) for _ in range(4))
        check(_lib.load().vt_plane_build(dev_ptr(pts, "pts"), B, T, reso, float(padding), PLANES[plane],
                                         dev_ptr(self.idx, "idx", I32), dev_ptr(self.order, "order", I32),
                                         dev_ptr(self.seg_lo, "seg_lo", I32), dev_ptr(self.seg_hi, "seg_hi", I32),
                                         stream_ptr()), "vt_plane_build")


def plane_indices(pts, reso, padding=0.1, planes=("xz", "xy", "yz")):
    """[PlaneIndex(pts, reso, padding, k) for k in planes] from ONE launch (vt_plane_build_multi): the planes' sorts run side by side."""
    for k in planes:
        if k not in PLANES:
            raise _lib.VtError(f"PlaneIndex: unknown plane {k!r} (one of {sorted(PLANES)})")
    if not 1 <= len(planes) <= 3:
        return [PlaneIndex(pts, reso, padding, k) for k in planes]
    pts = _c(pts.float())
    B, T, _ = pts.shape
    n = len(planes)
    buf = torch.empty((4, n, B, T), dtype=I32, device=pts.device)
    ids = (ctypes.c_int * n)(*[PLANES[k] for k in planes])
    check(_lib.load().vt_plane_build_multi(dev_ptr(pts, "pts"), B, T, reso, float(padding), n, ids, dev_ptr(buf[0], "idx", I32),
                                           dev_ptr(buf[1], "order", I32), dev_ptr(buf[2], "seg_lo", I32), dev_ptr(buf[3], "seg_hi", I32),
                                           stream_ptr()), "vt_plane_build_multi")
    out = []
    for i, k in enumerate(planes):
        pi = PlaneIndex.__new__(PlaneIndex)
        pi.B, pi.T, pi.R, pi.plane, pi.tile_flags = B, T, reso, k, None
        pi.idx, pi.order, pi.seg_lo, pi.seg_hi = buf[0, i], buf[1, i], buf[2, i], buf[3, i]
        pi.group = (buf, i, n)                                      # the planes' arrays side by side: the *_multi entries take them whole
        out.append(pi)
    return out


def plane_group(pis):
    """The shared [4, n, B, T] index buffer of ``pis`` if they are exactly the planes of one plane_indices call, in order; else None."""
    g = getattr(pis[0], "group", None)
    if g is None or g[2] != len(pis) or any(getattr(p, "group", (None,))[0] is not g[0] or p.group[1] != i for i, p in enumerate(pis)):
        return None
    return g[0]


def plane_scatter_mean_multi_fwd(feat, pis):
    """generate_plane_features for the planes of one plane_indices call in one launch (vt_plane_scatter_mean_multi_fwd): [n * B, C, R, R],
    the planes one after the other (= torch.cat of the per-plane tensors)."""
    buf = plane_group(pis)
    feat = _c(feat)
    B, T, C = feat.shape
    n, R = len(pis), pis[0].R
    planes = torch.empty((n * B, C, R, R), dtype=torch.float32, device=feat.device)
    check(_lib.load().vt_plane_scatter_mean_multi_fwd(dev_ptr(feat, "feat"), n, dev_ptr(buf[0], "idx", I32), dev_ptr(buf[1], "order", I32),
                                                      dev_ptr(buf[2], "seg_lo", I32), dev_ptr(buf[3], "seg_hi", I32), B, T, C, R,
                                                      dev_ptr(planes, "planes"), stream_ptr()), "vt_plane_scatter_mean_multi_fwd")
    return planes


def plane_scatter_mean_multi_bwd(grad_planes, pis, C):
    buf = plane_group(pis)
    grad_planes = _c(grad_planes)
    B, T, n, R = pis[0].B, pis[0].T, len(pis), pis[0].R
    g = torch.empty((B, T, C), dtype=torch.float32, device=grad_planes.device)
    check(_lib.load().vt_plane_scatter_mean_multi_bwd(dev_ptr(grad_planes, "grad_planes"), n, dev_ptr(buf[0], "idx", I32),
                                                      dev_ptr(buf[2], "seg_lo", I32), dev_ptr(buf[3], "seg_hi", I32), B, T, C, R,
                                                      dev_ptr(g, "grad_feat"), stream_ptr()), "vt_plane_scatter_mean_multi_bwd")
    return g


def plane_scatter_mean_fwd(feat, pi):
    feat = _c(feat)
    B, T, C = feat.shape
    plane = torch.empty((B, C, pi.R, pi.R), dtype=torch.float32, device=feat.device)
    check(_lib.load().vt_plane_scatter_mean_fwd(dev_ptr(feat, "feat"), dev_ptr(pi.idx, "idx", I32),
                                                dev_ptr(pi.order, "order", I32), dev_ptr(pi.seg_lo, "seg_lo", I32),
                                                dev_ptr(pi.seg_hi, "seg_hi", I32), B, T, C, pi.R, dev_ptr(plane, "plane"),
                                                stream_ptr()), "vt_plane_scatter_mean_fwd")
    return plane


def plane_scatter_mean_bwd(grad_plane, pi, C):
    grad_plane = _c(grad_plane)
    g = torch.empty((pi.B, pi.T, C), dtype=torch.float32, device=grad_plane.device)
    check(_lib.load().vt_plane_scatter_mean_bwd(dev_ptr(grad_plane, "grad_plane"), dev_ptr(pi.idx, "idx", I32),
                                                dev_ptr(pi.seg_lo, "seg_lo", I32), dev_ptr(pi.seg_hi, "seg_hi", I32),
                                                pi.B, pi.T, C, pi.R, dev_ptr(g, "grad_feat"), stream_ptr()),
          "vt_plane_scatter_mean_bwd")
    return g


def voxel_scatter_mean_cl_fwd(feat, vi):
    """Scatter-mean into a channels-last grid [B,R,R,R,C]."""
    feat = _c(feat)
    B, T, C = feat.shape
    R = vi.R
    grid = torch.empty((B, R, R, R, C), dtype=torch.float32, device=feat.device)
    check(_lib.load().vt_voxel_scatter_mean_cl_fwd(dev_ptr(feat, "feat"), dev_ptr(vi.idx, "idx", I32),
                                                   dev_ptr(vi.order, "order", I32), dev_ptr(vi.seg_lo, "seg_lo", I32),
                                                   dev_ptr(vi.seg_hi, "seg_hi", I32), B, T, C, R, dev_ptr(grid, "grid"),
                                                   stream_ptr()), "vt_voxel_scatter_mean_cl_fwd")
    return grid


def voxel_scatter_mean_cl_bwd(grad_grid_cl, vi, C):
    """grad of voxel_scatter_mean_cl_fwd: grad_grid_cl [B,R,R,R,C] contiguous -> [B,T,C]."""
    g = torch.empty((vi.B, vi.T, C), dtype=torch.float32, device=grad_grid_cl.device)
    check(_lib.load().vt_voxel_scatter_mean_cl_bwd(dev_ptr(_c(grad_grid_cl), "grad_grid"), dev_ptr(vi.idx, "idx", I32),
                                                   dev_ptr(vi.seg_lo, "seg_lo", I32), dev_ptr(vi.seg_hi, "seg_hi", I32),
                                                   vi.B, vi.T, C, vi.R, dev_ptr(g, "grad_feat"), stream_ptr()),
          "vt_voxel_scatter_mean_cl_bwd")
    return g
