"""1-to-4 midpoint subdivision of a batch of meshes (drop-in for reference src/encoder/manopth/upsample_layer.py:46-105, ``UpSampleLayer``:
the MANO hand from 778 to 3 093 to 12 337 vertices).

    new_verts [B, V + E, 3], new_faces [B, 4 F, 3] int64 = UpSampleLayer()(vertices [B, V, 3], faces [B, F, 3])

The reference numbers the edges in a Python dict filled face by face on the host, once per call and per batch item.  Here the
connectivity comes from ``ops.mesh.subdivide`` (csrc/mesh_subdivide.hip: the same numbering, from a scan over the half-edges) and is
kept per faces tensor; the vertices go through ``vt_mesh_subdivide_midpoints`` and are differentiable through ``vt_mesh_subdivide_bwd``
(the reference's ``# TODO check the gradient``: g_v[i] = g[i] + 0.5 sum of g[V + e] over the edges at i, summed exactly, so the gradient
has equal bits from run to run).

Cache policy.  An entry is keyed by the faces tensor's storage address, version counter, shape, strides and dtype, and holds that
tensor, so the address cannot be handed to other data while the entry lives; an in-place write bumps the version and misses.  A batch
whose items share their faces -- B = 1, a batch stride of 0 as ``th_faces.unsqueeze(0).expand(B, -1, -1)`` has it, or equal contents (one
host read, on a miss only) -- is computed once; the faces this layer returns for such a batch are themselves an expanded view, so the
next level hits the same way.  ``cache_size`` entries (default 8: two levels of both hands and room to spare), least recently used
first out; 0 builds the connectivity on every call.
"""
from collections import OrderedDict

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from ... import ops
from ..._lib import VtError


class _Midpoints(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vertices, edge_verts):
        ctx.edge_verts, ctx.n_vertices = edge_verts, vertices.shape[-2]
        return ops.mesh.subdivide_midpoints(vertices, edge_verts)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        return ops.mesh.subdivide_backward(grad_out.contiguous(), ctx.edge_verts, ctx.n_vertices), None


class UpSampleLayer(nn.Module):
    def __init__(self, cache_size=8):
        super().__init__()
        if isinstance(cache_size, bool) or int(cache_size) != cache_size or cache_size < 0:
            raise VtError(f"UpSampleLayer: cache_size must be an integer >= 0 (got {cache_size!r})")
        self.cache_size = int(cache_size)
        self._cache = OrderedDict()
        self.hits = self.misses = 0

    @staticmethod
    def _key(faces, n_vertices):
        return (faces.data_ptr(), faces._version, tuple(faces.shape), tuple(faces.stride()), faces.dtype, str(faces.device), n_vertices)

    @staticmethod
    def _connectivity(faces, n_vertices):
        """(shared, edge_verts, new_faces int64): one [E,2] / [4F,3] pair when every item has the same faces, [B,...] stacks otherwise."""
        B = faces.shape[0]
        shared = B == 1 or faces.stride(0) == 0 or bool(torch.equal(faces, faces[:1].expand_as(faces)))
        items = []
        for b in range(1 if shared else B):
            probe = torch.zeros((n_vertices, 3), dtype=torch.float32, device=faces.device)
            _, nf, info = ops.mesh.subdivide(probe, faces[b].int().contiguous())
            items.append((info.edge_verts, nf.long()))
        if shared:
            return True, items[0][0], items[0][1]
        if len({ev.shape[0] for ev, _ in items}) != 1:
            raise VtError("UpSampleLayer: the batch items have different edge counts (" + ", ".join(str(ev.shape[0]) for ev, _ in items)
                          + "); one tensor cannot hold their vertices")
        return False, torch.stack([ev for ev, _ in items]), torch.stack([nf for _, nf in items])

    def forward(self, vertices, faces):
        what = "UpSampleLayer"
        if not torch.is_tensor(vertices) or not torch.is_tensor(faces) or not vertices.is_cuda or faces.device != vertices.device:
            raise VtError(f"{what}: vertices and faces must be tensors on one HIP device; vtaco_amd has no CPU path")
        if vertices.dim() != 3 or vertices.shape[-1] != 3 or vertices.dtype not in (torch.float32, torch.float64):
            raise VtError(f"{what}: vertices must be float32 or float64 [B,V,3] (got {vertices.dtype} {tuple(vertices.shape)})")
        if faces.dim() != 3 or faces.shape[-1] != 3 or faces.shape[0] != vertices.shape[0] or faces.dtype not in (torch.int32, torch.int64):
            raise VtError(f"{what}: faces must be int32 or int64 [B,F,3] with the vertices' B (got {faces.dtype} {tuple(faces.shape)})")
        B, V = vertices.shape[0], vertices.shape[1]
        key = self._key(faces, V)
        entry = self._cache.get(key)
        if entry is None:
            self.misses += 1
            entry = (faces,) + self._connectivity(faces, V)
            if self.cache_size:
                self._cache[key] = entry
                while len(self._cache) > self.cache_size:
                    self._cache.popitem(last=False)
        else:
            self.hits += 1
            self._cache.move_to_end(key)
        _, shared, edge_verts, new_faces = entry
        if shared:
            return _Midpoints.apply(vertices, edge_verts), new_faces.unsqueeze(0).expand(B, -1, -1)
        return torch.stack([_Midpoints.apply(vertices[b], edge_verts[b]) for b in range(B)]), new_faces
