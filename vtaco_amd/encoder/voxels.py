"""Voxel-input local encoder -> feature grid or canonical planes (drop-in for reference src/encoder/voxels.py:10-119,
``voxel_simple_local``): same constructor arguments, attribute names and state_dict keys (conv_in.*, unet.*, unet3d.*).

conv_in, ReLU and the scatter-mean onto the grid / planes are one HIP launch (vt_voxel_encode_grid / _planes: a voxel's cell follows
from the volume's shape alone, so the scatter is a gather over a box of voxels); under autograd the launch is wrapped in a Function
whose backward is vt_voxel_encode_bwd.  ``VTACO_VOXEL_ENCODER=host`` keeps nn.Conv3d and the point encoders' scatter-means on the
generated voxel coordinates: the comparator the timing tool measures against.
"""
from __future__ import annotations

import os

import torch
import torch.nn.functional as F
from torch import nn

from .. import ops
from .._lib import VtError
from .pointnet import _ScatterMeanCL, _ScatterMeanPlane, _ScatterMeanPlanes
from .unet import UNet
from .unet3d import UNet3D


class _EncodeGridFn(torch.autograd.Function):
    """x, conv weight, conv bias -> channels-last mean grid [B,R,R,R,C]; the volume is data and gets no gradient."""

    @staticmethod
    def forward(ctx, x, weight, bias, reso, padding):
        ctx.save_for_backward(x, weight, bias)
        ctx.padding = padding
        return ops.voxel_encoder.encode_grid(x, weight, bias, reso, padding)

    @staticmethod
    def backward(ctx, grad):
        x, weight, bias = ctx.saved_tensors
        dw, db = ops.voxel_encoder.encode_bwd(x, weight, bias, ctx.padding, grad_grid=grad)
        return None, dw, db, None, None


class _EncodePlanesFn(torch.autograd.Function):
    """x, conv weight, conv bias -> the planes stacked [P B,C,R,R]."""

    @staticmethod
    def forward(ctx, x, weight, bias, reso, padding, planes):
        ctx.save_for_backward(x, weight, bias)
        ctx.padding, ctx.planes = padding, planes
        return ops.voxel_encoder.encode_planes(x, weight, bias, reso, padding, planes)

    @staticmethod
    def backward(ctx, grad):
        x, weight, bias = ctx.saved_tensors
        dw, db = ops.voxel_encoder.encode_bwd(x, weight, bias, ctx.padding, grad_planes=grad, planes=ctx.planes)
        return None, dw, db, None, None, None


class LocalVoxelEncoder(nn.Module):
    """Args as the reference (voxels.py:13-27).  'grid' in ``plane_type`` takes precedence over the planes (voxels.py:110-118)."""

    def __init__(self, dim=3, c_dim=128, unet=False, unet_kwargs=None, unet3d=False, unet3d_kwargs=None,
                 plane_resolution=512, grid_resolution=None, plane_type='xz', kernel_size=3, padding=0.1):
        super().__init__()
        self.actvn = F.relu
        self.conv_in = nn.Conv3d(1, c_dim, 1) if kernel_size == 1 else nn.Conv3d(1, c_dim, kernel_size, padding=1)
        self.unet = UNet(c_dim, in_channels=c_dim, **(unet_kwargs or {})) if unet else None
        self.unet3d = UNet3D(**unet3d_kwargs) if unet3d else None
        self.c_dim = c_dim
        self.reso_plane, self.reso_grid = plane_resolution, grid_resolution
        self.plane_type, self.padding = plane_type, padding
        names = [plane_type] if isinstance(plane_type, str) else list(plane_type)
        # the keys forward returns, in the reference's fixed order; Generator3D reads ``planes`` to tell a plane model from a grid model
        self.planes = ['grid'] if 'grid' in names else [k for k in ('xz', 'xy', 'yz') if k in names]
        if not self.planes:
            raise VtError(f"LocalVoxelEncoder: plane_type {plane_type!r} names none of 'grid','xz','xy','yz'")
        if self.planes == ['grid'] and grid_resolution is None:
            raise VtError("LocalVoxelEncoder: grid_resolution is required")
        # "hip": the fused kernels; "host": nn.Conv3d + the point encoders' scatter-means on the voxel coordinates
        self.voxel_encoder = os.environ.get("VTACO_VOXEL_ENCODER", "hip")
        if self.voxel_encoder not in ("hip", "host"):
            raise VtError(f"VTACO_VOXEL_ENCODER must be 'hip' or 'host' (got {self.voxel_encoder!r})")
        # UNet3D under autograd, as LocalPoolPointnet: "hip" = the vt_* forward and backward kernels, "host" = PyTorch-ROCm autograd
        self.train_unet3d = os.environ.get("VTACO_TRAIN_UNET3D", "hip")

    def _hip_fits(self):
        """The knob alone decides: a shape the kernels do not cover (C, kernel size) is a VtError from ops, not another route."""
        return self.voxel_encoder == "hip"

    @staticmethod
    def voxel_coordinates(x):
        """p [B, D1 D2 D3, 3]: every voxel's coordinate, linspace(-0.5, 0.5, D) per axis (voxels.py:94-102)."""
        axes = [torch.linspace(-0.5, 0.5, x.size(k + 1)).to(x.device) for k in range(3)]
        shape = [(1, -1, 1, 1), (1, 1, -1, 1), (1, 1, 1, -1)]
        p = torch.stack([a.view(s).expand_as(x) for a, s in zip(axes, shape)], dim=4)
        return p.reshape(x.size(0), -1, 3)

    def voxel_features(self, x):
        """relu(conv_in(x)) by voxel, [B, D1 D2 D3, C] (voxels.py:105-107): the host route's first half."""
        c = self.actvn(self.conv_in(x.unsqueeze(1))).view(x.size(0), self.c_dim, -1)
        return c.permute(0, 2, 1).contiguous()

    # -- grid ---------------------------------------------------------------------------------------------------------
    def _mean_grid_cl(self, x):
        """The mean grid, [B,C,R,R,R]-shaped with channels-last strides."""
        if self._hip_fits():
            w, b = self.conv_in.weight, self.conv_in.bias
            if torch.is_grad_enabled() and (w.requires_grad or b.requires_grad):
                grid = _EncodeGridFn.apply(x, w, b, self.reso_grid, self.padding)
            else:
                grid = ops.voxel_encoder.encode_grid(x, w, b, self.reso_grid, self.padding)
            return grid.permute(0, 4, 1, 2, 3)
        vi = ops.VoxelIndex(self.voxel_coordinates(x), self.reso_grid, self.padding)
        feat = self.voxel_features(x)
        if torch.is_grad_enabled():
            return _ScatterMeanCL.apply(feat, vi)
        return ops.voxel_scatter_mean_cl_fwd(feat, vi).permute(0, 4, 1, 2, 3)

    def forward_grid(self, x):
        grid = self._mean_grid_cl(x)
        net = self.unet3d
        if net is None:
            return {'grid': grid}
        if not net.hip_supported():
            return {'grid': net(grid)}
        cl = grid.permute(0, 2, 3, 4, 1)
        if not torch.is_grad_enabled():
            return {'grid': net.forward_channels_last(cl).permute(0, 4, 1, 2, 3)}
        if self.train_unet3d == "hip":
            return {'grid': net.forward_channels_last_train(cl.contiguous()).permute(0, 4, 1, 2, 3)}
        return {'grid': net(grid)}

    # -- planes -------------------------------------------------------------------------------------------------------
    def forward_planes(self, x):
        B = x.shape[0]
        if self._hip_fits():
            w, b = self.conv_in.weight, self.conv_in.bias
            if torch.is_grad_enabled() and (w.requires_grad or b.requires_grad):
                stacked = _EncodePlanesFn.apply(x, w, b, self.reso_plane, self.padding, tuple(self.planes))
            else:
                stacked = ops.voxel_encoder.encode_planes(x, w, b, self.reso_plane, self.padding, self.planes)
        else:
            pis = ops.plane_indices(self.voxel_coordinates(x), self.reso_plane, self.padding, self.planes)
            feat = self.voxel_features(x)
            if len(pis) > 1 and ops.plane_group(pis) is not None:
                stacked = _ScatterMeanPlanes.apply(feat, pis)
            else:
                stacked = torch.cat([_ScatterMeanPlane.apply(feat, pi) for pi in pis], dim=0)
        if self.unet is not None:
            # one U-Net pass over the planes stacked on the batch axis, as LocalPoolPointnet.forward_planes
            stacked = self.unet(stacked)
        return dict(zip(self.planes, stacked.split(B, dim=0)))

    def forward(self, x):
        if not x.is_cuda:
            raise VtError(f"LocalVoxelEncoder: inputs must live on a HIP device (got {x.device})")
        if x.dim() != 4:
            raise VtError(f"LocalVoxelEncoder: inputs must be a voxel volume [B,D1,D2,D3] (got {tuple(x.shape)})")
        x = x.float()
        return self.forward_grid(x) if self.planes == ['grid'] else self.forward_planes(x)
