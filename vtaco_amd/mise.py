"""Multiresolution isosurface extraction (MISE, Occupancy Networks) on the device.

The reference configures it (``generation.resolution_0`` / ``upsampling_steps``; its Generator3D docstring calls them the MISE
settings) and keeps the algorithm as numpy code that nothing calls (src/utils/mesh.py:7-84 ``MultiGridExtractor``).  Here level 0
evaluates the (r0+1)^3 lattice, and every further level doubles the resolution: the device classifies the voxels the surface
crosses, upsamples the value grid, compacts the unknown corners of the children of those voxels into a query list
(vtaco_amd/csrc/mise.hip), ``evaluate`` decodes the list and the logits are scattered into the fine grid.  The points decoded grow
with the surface (~n^2), not with the volume (n^3).

One deliberate difference from the reference: a voxel is active when its corners do not all satisfy the same side of marching
cubes' own predicate ``(double)v - level > 0``, where the reference asks ``v < threshold``.  The two rules differ only where a value
equals the level exactly; with the marching-cubes rule a voxel MISE leaves unrefined can never emit a triangle.
"""
from __future__ import annotations

import torch

from . import ops
from ._lib import VtError

MAX_N = ops.MISE_MAX_N
_capacity_guess = {}            # (device, nc) -> query-list length that covered the last step from nc


def size(resolution0, upsampling_steps):
    """Points per axis of the finest level: r0 * 2^S + 1."""
    return int(resolution0) * 2 ** int(upsampling_steps) + 1


def _read_count(count):
    """The query count of the step just queued: one host read, through a page-locked word."""
    slot = torch.empty(1, dtype=torch.int32, pin_memory=True)
    slot.copy_(count, non_blocking=True)
    done = torch.cuda.Event()
    done.record()
    done.synchronize()
    return int(slot[0])


def extract(evaluate, resolution0, upsampling_steps, level, box, device):
    """MISE from ``resolution0`` with ``upsampling_steps`` refinements of the field ``evaluate``.

    ``evaluate(ids, pts) -> logits [M]``: lattice ids (int32 [M], x-major ids of the current level's n^3 lattice) and their
    coordinates (f32 [M,3], ``box * linspace(-0.5, 0.5, n)`` per axis, as the decode kernels' lattice computes them; coarse point i and
    fine point 2i are the same floats).  Level 0 is the whole (r0+1)^3 lattice, given to ``evaluate`` in id order.

    Returns ``(values [n,n,n] f32, known [n,n,n] u8, points_per_level)`` with n = r0 * 2^S + 1: the known entries (the points some
    level decoded) hold the field, the others the nearest-coarse fill (``upsample3d_nn(...)[:-1,:-1,:-1]`` as the reference); ``points_per_level`` lists how many
    points each level decoded.  Host reads: one per refinement level (the query count, to size the decode), a second one only when
    the list outgrew its guessed capacity.  The order of a level's query list may vary from run to run; the sets, the values and
    therefore the mesh do not."""
    r0, steps = int(resolution0), int(upsampling_steps)
    if r0 < 1 or steps < 0:
        raise VtError(f"mise.extract: resolution0 >= 1 and upsampling_steps >= 0 needed (got {r0}, {steps})")
    n = size(r0, steps)
    if n > MAX_N:
        raise VtError(f"mise.extract: {n}^3 is beyond the {MAX_N}^3 this extraction is verified for (resolution0 * 2^steps <= {MAX_N - 1})")
    device = torch.device(device)
    nc = r0 + 1
    with torch.no_grad():
        ids, pts = ops.mise_lattice(nc, box, device)
        values = _logits(evaluate(ids, pts), nc ** 3).reshape(nc, nc, nc)
        known = torch.ones((nc, nc, nc), dtype=torch.uint8, device=device)
        per_level = [nc ** 3]
        count = torch.empty(1, dtype=torch.int32, device=device)
        for _ in range(steps):
            nf = 2 * nc - 1
            worst = nf ** 3 - nc ** 3
            key = (device, nc)
            cap = min(worst, _capacity_guess.get(key, 64 * nf * nf))
            fine, fk, qids, qpts, _ = ops.mise_refine(values, level, box, cap, coarse_known=known, count=count)
            m = _read_count(count)
            if m > cap:                          # the list outgrew the guess: the step again with room for all of it
                cap = m
                fine, fk, qids, qpts, _ = ops.mise_refine(values, level, box, cap, coarse_known=known, fine=fine, known=fk, count=count)
            _capacity_guess[key] = min(worst, m + m // 4 + 4096)
            if m:
                ops.mise_scatter(fine, qids[:m], _logits(evaluate(qids[:m], qpts[:m]), m), known=fk)
            known = fk
            values, nc = fine, nf
            per_level.append(m)
    return values, known, per_level


def _logits(vals, m):
    vals = vals.detach().reshape(-1)
    if vals.numel() != m or vals.dtype != torch.float32:
        raise VtError(f"mise.extract: evaluate must return {m} float32 logits (got {vals.numel()} {vals.dtype})")
    return vals.contiguous()
