"""Mesh generation (drop-in for the hot-path part of reference
src/conv_onet/generation.py: ``Generator3D.eval_points`` :338-383 and the dense
evaluation + marching cubes of ``generate_obj_mesh_wnf`` :119-120, 155-157, 257-273).

The reference builds the nx^3 lattice on the CPU, ships it to the GPU in 100k-point
chunks, copies every chunk's logits back and runs scikit-image's marching cubes on
the CPU.  Here the lattice is generated inside the decode kernel, the logits stay on
the device and marching cubes is a HIP kernel; the results (logits within 1e-4,
vertex numbering bit-exact) are the same.  ``generate_hand_mesh`` (:74-115) runs the hand
encoder + MANO layer on the device and the reference's wrist-frame post-processing on the
778 vertices.  ``c_img_all`` can be passed in pre-built or as finger ids (generate_obj_mesh_tactile).
"""
from __future__ import annotations

import numbers
import operator
import os
from collections import namedtuple

import torch

from .. import ops
from .._lib import VtError

# A/B knob: "0" reads a captured scene's marching-cubes counts through a copy + event behind the graph instead of the page-locked slot
# the scan kernel writes (ops.mc_count_echo)
_MC_ECHO = os.environ.get("VTACO_MC_ECHO", "1") != "0"

class Mesh(namedtuple("Mesh", ["vertices", "faces"])):
    """(vertices [V,3], faces [F,3]) as tensors, on the device the generator left them -- a namedtuple (field access, unpacking,
    equality as a tuple) that also writes itself to a file the way the reference's ``trimesh.Trimesh.export`` is called
    (train.py:252-253, generate.py): see ``export``."""
    __slots__ = ()

    FILE_TYPES = ("off", "ply", "obj")

    def export(self, file_obj, file_type=None):
        """Write the mesh to ``file_obj`` (a path) as OFF, ASCII PLY or OBJ, chosen by ``file_type`` or the path's extension.
        The vertices and faces are written as given: no duplicate-vertex merging, no removal of degenerate or unreferenced
        entries (trimesh's ``process=True`` does both).  float32 vertices are printed with 9 significant digits, float64 ones
        with 17: either reads back to the same value."""
        import numpy as np
        ft = (file_type or os.path.splitext(str(file_obj))[1].lstrip(".")).lower()
        if ft not in self.FILE_TYPES:
            raise VtError(f"Mesh.export: unknown file type {ft!r} (one of {', '.join(self.FILE_TYPES)})")
        v = self.vertices.detach().cpu().numpy() if torch.is_tensor(self.vertices) else np.asarray(self.vertices)
        f = self.faces.detach().cpu().numpy() if torch.is_tensor(self.faces) else np.asarray(self.faces)
        v, f = v.reshape(-1, 3), f.reshape(-1, 3).astype(np.int64)
        double = v.dtype == np.float64
        vfmt = "%.17g" if double else "%.9g"
        if not double:
            v = v.astype(np.float32)
        vlines = [" ".join(vfmt % x for x in row) for row in v.tolist()]
        n = self.vertex_normals if isinstance(self, NormalMesh) else None     # a plain Mesh writes what it always wrote
        if n is not None and ft != "off":
            n = n.detach().cpu().numpy() if torch.is_tensor(n) else np.asarray(n)
            n = n.reshape(-1, 3).astype(v.dtype)
            if len(n) != len(v):
                raise VtError(f"Mesh.export: {len(n)} vertex normals for {len(v)} vertices")
            nlines = [" ".join(vfmt % x for x in row) for row in n.tolist()]
            kind = "double" if double else "float"
            if ft == "ply":
                head = ["ply", "format ascii 1.0", f"element vertex {len(v)}"] + [f"property {kind} {c}" for c in ("x", "y", "z", "nx", "ny", "nz")] \
                    + [f"element face {len(f)}", "property list uchar int vertex_indices", "end_header"]
                body = [a + " " + b for a, b in zip(vlines, nlines)] + ["3 %d %d %d" % tuple(r) for r in f.tolist()]
            else:
                head = []
                body = ["v " + line for line in vlines] + ["vn " + line for line in nlines] \
                    + ["f %d//%d %d//%d %d//%d" % (a, a, b, b, c, c) for a, b, c in (f + 1).tolist()]
            with open(file_obj, "w") as fh:
                fh.write("\n".join(head + body) + "\n")
            return
        if ft == "off":
            head = ["OFF", f"{len(v)} {len(f)} 0"]
            body = vlines + ["3 %d %d %d" % tuple(r) for r in f.tolist()]
        elif ft == "ply":
            kind = "double" if double else "float"
            head = ["ply", "format ascii 1.0", f"element vertex {len(v)}", f"property {kind} x", f"property {kind} y",
                    f"property {kind} z", f"element face {len(f)}", "property list uchar int vertex_indices", "end_header"]
            body = vlines + ["3 %d %d %d" % tuple(r) for r in f.tolist()]
        else:
            head = []
            body = ["v " + line for line in vlines] + ["f %d %d %d" % tuple(r) for r in (f + 1).tolist()]
        with open(file_obj, "w") as fh:
            fh.write("\n".join(head + body) + "\n")

    # what trimesh.Trimesh gives the reference's users for free (utils/mesh_clean.py, on the device)
    def components(self):
        """The MeshComponents record: labels, per-component counts, area, volume, Euler number, watertight, oriented."""
        from ..utils import mesh_clean
        return mesh_clean.components(self)

    def split(self):
        """One Mesh per connected component, in component order."""
        from ..utils import mesh_clean
        return mesh_clean.split(self)

    def keep_largest(self, by="faces"):
        """The largest component by 'faces', 'area' or 'volume'."""
        from ..utils import mesh_clean
        return mesh_clean.keep_largest(self, by=by)

    def remove_small(self, min_faces=0, min_area_fraction=0.0):
        """The components that reach both bounds."""
        from ..utils import mesh_clean
        return mesh_clean.remove_small(self, min_faces=min_faces, min_area_fraction=min_area_fraction)

    def simplify(self, nfaces=None, resolution=None, placement="quadric"):
        """At most ``nfaces`` faces, or the clustering at ``resolution`` cells: vertex clustering with quadric placement.  Topology is
        not preserved."""
        from ..utils import mesh_clean
        return mesh_clean.simplify(self, nfaces=nfaces, resolution=resolution, placement=placement)

    def simplify_report(self, nfaces=None, resolution=None, placement="quadric"):
        """(mesh, report): ``simplify`` and the resolution it used, the probes of its search, the clusters and the fallbacks."""
        from ..utils import mesh_clean
        return mesh_clean.simplify_report(self, nfaces=nfaces, resolution=resolution, placement=placement)

    def decimate(self, nfaces, placement="optimal"):
        """At most ``nfaces`` faces by quadric edge collapses that keep a manifold a manifold (utils/mesh_clean.py: decimate)."""
        from ..utils import mesh_clean
        return mesh_clean.decimate(self, nfaces, placement=placement)

    def decimate_report(self, nfaces, placement="optimal"):
        """(mesh, DecimateReport) (utils/mesh_clean.py: decimate_report)."""
        from ..utils import mesh_clean
        return mesh_clean.decimate_report(self, nfaces, placement=placement)

    def merge_vertices(self, tol=0.0, unique_faces=False):
        """Equal vertices merged (within ``tol`` of a lattice where ``tol`` > 0), collapsed faces and unreferenced vertices dropped."""
        from ..utils import mesh_clean
        return mesh_clean.merge_vertices(self, tol=tol, unique_faces=unique_faces)

    def boundary_loops(self):
        """The boundary loops of the mesh (utils/mesh_clean.py: boundary_loops)."""
        from ..utils import mesh_clean
        return mesh_clean.boundary_loops(self)

    def fill_holes(self, method="fan", max_edges=None):
        """The mesh with its boundary loops capped; the mesh itself when it has none (utils/mesh_clean.py: fill_holes)."""
        from ..utils import mesh_clean
        return mesh_clean.fill_holes(self, method=method, max_edges=max_edges)

    def fill_report(self, method="fan", max_edges=None):
        """(mesh, FillReport) (utils/mesh_clean.py: fill_report)."""
        from ..utils import mesh_clean
        return mesh_clean.fill_report(self, method=method, max_edges=max_edges)

    def vertex_neighbors(self):
        """The vertex-vertex adjacency as CSR rows, ``ops.mesh.MeshAdjacency`` (utils/mesh_clean.py: vertex_neighbors)."""
        from ..utils import mesh_clean
        return mesh_clean.vertex_neighbors(self)

    def vertex_degree(self):
        """int32 [V]: the number of neighbours of every vertex."""
        from ..utils import mesh_clean
        return mesh_clean.vertex_degree(self)

    def boundary_vertices(self):
        """bool [V]: the vertices on an edge with exactly one face."""
        from ..utils import mesh_clean
        return mesh_clean.boundary_vertices(self)

    def smooth(self, method="taubin", iterations=10, lam=0.5, mu=-0.53, alpha=0.1, beta=0.5, weights="uniform", boundary="pin",
               adjacency=None):
        """The same faces on smoothed vertices: 'laplacian', 'taubin' or 'humphrey' (utils/mesh_clean.py: smooth)."""
        from ..utils import mesh_clean
        return mesh_clean.smooth(self, method=method, iterations=iterations, lam=lam, mu=mu, alpha=alpha, beta=beta, weights=weights,
                                 boundary=boundary, adjacency=adjacency)

    def smooth_report(self, method="taubin", iterations=10, lam=0.5, mu=-0.53, alpha=0.1, beta=0.5, weights="uniform", boundary="pin",
                      adjacency=None):
        """(mesh, SmoothReport) (utils/mesh_clean.py: smooth_report)."""
        from ..utils import mesh_clean
        return mesh_clean.smooth_report(self, method=method, iterations=iterations, lam=lam, mu=mu, alpha=alpha, beta=beta, weights=weights,
                                        boundary=boundary, adjacency=adjacency)

    def subdivide(self, iterations=1, face_index=None):
        """1-to-4 midpoint subdivision, conforming around ``face_index`` (utils/mesh_clean.py: subdivide)."""
        from ..utils import mesh_clean
        return mesh_clean.subdivide(self, iterations=iterations, face_index=face_index)

    def subdivide_loop(self, iterations=1):
        """Loop subdivision (utils/mesh_clean.py: subdivide_loop)."""
        from ..utils import mesh_clean
        return mesh_clean.subdivide_loop(self, iterations=iterations)

    def subdivide_to_size(self, max_edge, max_iter=10):
        """Adaptive midpoint rounds until no edge is longer than ``max_edge`` (utils/mesh_clean.py: subdivide_to_size)."""
        from ..utils import mesh_clean
        return mesh_clean.subdivide_to_size(self, max_edge, max_iter=max_iter)

    def subdivide_report(self, scheme="midpoint", iterations=1, face_index=None, max_edge=None, max_iter=10):
        """(mesh, SubdivideReport) (utils/mesh_clean.py: subdivide_report)."""
        from ..utils import mesh_clean
        return mesh_clean.subdivide_report(self, scheme=scheme, iterations=iterations, face_index=face_index, max_edge=max_edge, max_iter=max_iter)

    def face_normals(self):
        """Unit face normals [F,3] by the faces' winding; (0,0,0) for a degenerate face."""
        from ..utils import mesh_clean
        return mesh_clean.face_normals(self)

    def vertex_normals(self, weight="area"):
        """Unit vertex normals [V,3] from the geometry, weighted by face 'area' or corner 'angle'."""
        from ..utils import mesh_clean
        return mesh_clean.vertex_normals(self, weight=weight)

    def with_vertex_normals(self, weight="area"):
        """This mesh as a ``NormalMesh`` carrying its geometric vertex normals."""
        from ..utils import mesh_clean
        return mesh_clean.with_vertex_normals(self, weight=weight)

    def refine(self, generator, c, steps=None, eps=None, seed=0):
        """This mesh after ``steps`` refinement iterations against ``generator``'s field on the encoder output ``c``
        (``Generator3D.refine_mesh``): same faces, moved vertices."""
        return generator.refine_mesh(self, c, steps=steps, eps=eps, seed=seed)

    def signed_distance_field(self, resolution, loc=None, scale=None, winding='fast', distance='tree'):
        """float64 [resolution]^3: the signed distance to this mesh at the voxel centres of ``VoxelGrid``'s lattice (utils/voxels.py)."""
        from ..utils import voxels
        return voxels.signed_distance_field(self, resolution, loc=loc, scale=scale, winding=winding, distance=distance)

    def ray_cast(self, origins, dirs, t_min=0.0, t_max=float("inf"), method=None, tree=None, bary=False):
        """(s f64 [N], face i32 [N][, bary f64 [N,3]]): what the rays ``origins + s dirs`` hit first (``ops.rays.ray_mesh``)."""
        from ..utils.voxels import _mesh_tensors
        v, f = _mesh_tensors(self)
        return ops.rays.ray_mesh(v, f, origins, dirs, t_min=t_min, t_max=t_max, method=method, tree=tree, bary=bary)

    def render_depth(self, cam_pos, cam_rot, height=240, width=320, fov=60.0, pc_ply=None, centroid=None, scale=None, method='tree'):
        """(depth f32 [n,H,W], face i32 [n,H,W]): this mesh seen from n sensor poses (utils/render.py)."""
        from ..utils import render
        return render.render_depth(self, cam_pos, cam_rot, height=height, width=width, fov=fov, pc_ply=pc_ply, centroid=centroid, scale=scale,
                                   method=method)

    def simulate_touch(self, cam_pos, cam_rot, depth_origin, near=0.019, threshold=1e-4, **kw):
        """(depth f32 [n, H*W], touch_success bool [n]): the depth images of n sensors pressed against this mesh (utils/render.py)."""
        from ..utils import render
        return render.simulate_touch(self, cam_pos, cam_rot, depth_origin, near=near, threshold=threshold, **kw)


class NormalMesh(Mesh):
    """A ``Mesh`` that carries per-vertex normals.  The tuple is still (vertices, faces): unpacking, indexing and equality are those
    of ``Mesh``.  Attributes: ``vertex_normals`` [V,3], ``values`` ([V] or None) and ``normals_source`` ('marching_cubes' or
    'geometry').  ``export`` writes the normals to PLY (nx ny nz) and OBJ (vn, f v//vn); OFF has no place for them.  ``Mesh``'s
    ``vertex_normals(weight=)`` method is reached as ``geometric_vertex_normals`` here, the name being taken by the attribute."""
    SOURCES = ("marching_cubes", "geometry")

    def __new__(cls, vertices, faces, vertex_normals=None, values=None, normals_source="geometry"):
        if vertex_normals is None:
            raise VtError("NormalMesh: vertex_normals is required (a mesh without normals is a Mesh)")
        if normals_source not in cls.SOURCES:
            raise VtError(f"NormalMesh: normals_source must be one of {cls.SOURCES} (got {normals_source!r})")
        if tuple(vertex_normals.shape) != (vertices.shape[0], 3):
            raise VtError(f"NormalMesh: vertex_normals must be [{vertices.shape[0]},3] (got {tuple(vertex_normals.shape)})")
        if values is not None and tuple(values.shape) != (vertices.shape[0],):
            raise VtError(f"NormalMesh: values must be [{vertices.shape[0]}] (got {tuple(values.shape)})")
        self = super().__new__(cls, vertices, faces)
        self.vertex_normals, self.values, self.normals_source = vertex_normals, values, normals_source
        return self

    def geometric_vertex_normals(self, weight="area"):
        """Unit vertex normals [V,3] recomputed from the geometry (``Mesh.vertex_normals``)."""
        from ..utils import mesh_clean
        return mesh_clean.vertex_normals(self, weight=weight)

    def __reduce__(self):
        return (NormalMesh, (self.vertices, self.faces, self.vertex_normals, self.values, self.normals_source))


_tensor_version = operator.attrgetter("_version")


_PRECISION_ORDER = ("f16f8", "f16x3", "bf16x3", "f32")            # least to most conservative


def _guard_step(word, precision):
    """What the range word of a finished scene asks of a half-precision decode: (next precision, reason) or None."""
    if precision not in ("f16x3", "f16f8"):
        return None
    if word & ops.RANGE_HALF:
        return "bf16x3", "reach the half-precision range limit (65504)"
    if (word & ops.RANGE_FP8) and precision == "f16f8":
        return "f16x3", "reach 1024, where the fp8 correction products of 'f16f8' begin to clip"
    if (word & ops.RANGE_LOGIT) and precision == "f16f8":
        return "f16x3", "produce logits beyond 2.5, where the relative error of 'f16f8' (~3e-5 |logit|) leaves the 1e-4 bar"
    return None


def _agree_precision(precision, group, device):
    """The most conservative decode precision held by any rank of ``group`` (one MAX all-reduce of its rank in _PRECISION_ORDER);
    ``precision`` itself without an initialised process group."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) <= 1:
        return precision
    mine = _PRECISION_ORDER.index(precision) if precision in _PRECISION_ORDER else len(_PRECISION_ORDER) - 1
    if dist.get_backend(group) == "nccl":
        dev = device if device is not None and torch.device(device).type == "cuda" else torch.device("cuda", torch.cuda.current_device())
    else:
        dev = "cpu"
    t = torch.tensor([mine], dtype=torch.int32, device=dev)
    dist.all_reduce(t, op=dist.ReduceOp.MAX, group=group)
    return _PRECISION_ORDER[int(t.item())] if int(t.item()) != mine else precision


def _range_guarded(method=None, *, collective=False):
    """A generation entry point under the half-precision decodes' range guard (ops.decode_range_status, one word per device).
    "f16f8" that met activations >= 1024 (RANGE_FP8: its fp8 correction copies begin to clip) or wrote a logit beyond 2.5
    (RANGE_LOGIT: its error is relative, ~3e-5 |logit|) has left its 1e-4 contract and moves to "f16x3"; a half-precision form that met activations at the edge of the half range (RANGE_HALF: 65504, hi operands saturate)
    moves to "bf16x3" (f32's exponent range) -- for good, with a warning -- and the scene is generated again.  The word is
    cleared (asynchronously) when the outermost guarded call begins, so that only THIS scene's launches are judged, and read
    back once per scene behind the synchronisation the mesh extraction has just done.

    The decision is RANK-LOCAL for every entry point except the sharded one: a rank-0-only mesh export during distributed
    training or per-rank evaluation with uneven scene counts must not meet a collective here.  ``collective=True``
    (generate_obj_mesh_sharded) is a collective on the ``group`` the call was given whatever the ranks' precisions are: the
    ranks first agree on the most conservative precision any of them holds (a rank-local guard may have moved one rank
    earlier: the slabs of one value grid must be decoded in one arithmetic, and every rank must enter the same reductions),
    then every round reduces the word over the group, so that all ranks take the same decision."""
    import functools
    import warnings

    def wrap(method):
        @functools.wraps(method)
        def guarded(self, *args, **kwargs):
            if getattr(self, "_guard_depth", 0):
                return method(self, *args, **kwargs)
            group = kwargs.get("group", args[1] if len(args) > 1 else None) if collective else None
            if collective:
                agreed = _agree_precision(self.decode_precision, group, self.device)
                if agreed != self.decode_precision:
                    warnings.warn(f"Generator3D: another rank of the group decodes in {agreed!r}; this rank follows "
                                  f"(decode_precision {self.decode_precision!r} -> {agreed!r})")
                    self._set_decode_precision(agreed)
            if self.decode_precision not in ("f16x3", "f16f8"):
                return method(self, *args, **kwargs)
            self._guard_depth = 1
            try:
                ops.decode_range_clear()                             # bits left by earlier launches on this device are not this scene's
                out = method(self, *args, **kwargs)
                for _ in range(2):                                   # f16f8 -> f16x3 -> bf16x3 at most
                    if self.decode_precision not in ("f16x3", "f16f8"):
                        break
                    word = ops.decode_range_status(reset=True)
                    if collective:
                        word = _reduce_or(word, group, self.device)
                    step = _guard_step(word, self.decode_precision)
                    if step is None:
                        break
                    nxt, why = step
                    warnings.warn(f"Generator3D: the decoder's activations {why}; "
                                  f"decode_precision {self.decode_precision!r} -> {nxt!r} and the scene is generated again")
                    self._set_decode_precision(nxt)
                    out = method(self, *args, **kwargs)
                return out
            finally:
                self._guard_depth = 0
        return guarded
    return wrap if method is None else wrap(method)


def _reduce_or(word, group, device):
    """Bitwise OR of a small status word over the ranks of ``group`` (None = the default group); the word itself without an
    initialised process group.  With the nccl (RCCL) backend the scratch tensor lives on this rank's device."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) <= 1:
        return word
    if dist.get_backend(group) == "nccl":
        dev = device if device is not None and torch.device(device).type == "cuda" else torch.device("cuda", torch.cuda.current_device())
    else:
        dev = "cpu"
    t = torch.tensor([(word >> b) & 1 for b in range(8)], dtype=torch.int32, device=dev)      # RCCL has no bitwise OR: MAX per bit
    dist.all_reduce(t, op=dist.ReduceOp.MAX, group=group)
    return sum(int(v) << b for b, v in enumerate(t.tolist()))


class Generator3D(object):
    """Constructor arguments as the reference (generation.py:42-52), plus ``extraction``: how generate_obj_mesh_wnf samples the field.

    ``"dense"`` (the default, the reference's behaviour): the nx^3 lattice, nx = resolution0 * 4, decoded whole, then marching cubes
    at scikit-image's default level with the reference's ``-nx/2, (1+padding)/nx`` rescale; ``upsampling_steps`` is ignored, as the
    reference ignores it.

    ``"mise"``: multiresolution isosurface extraction (vtaco_amd/mise.py) from ``resolution0`` with ``upsampling_steps`` refinements,
    n = resolution0 * 2^upsampling_steps + 1 points per axis (at most 513): the (r0+1)^3 lattice, then per level only the corners of
    the voxels the surface crosses are decoded.  The level is the logit of ``threshold`` (``log(t) - log(1-t)`` in double: 0 at 0.5,
    as ConvONet), and the vertices are rescaled by ``(n-1)/2, (1+padding)/(n-1)`` so that they lie in the frame the field was sampled
    in.  Every level decodes through the POINT path -- ``decode_precision`` where that path has the arithmetic, ``"f16x3"`` for
    ``"f16f8"`` (a lattice-only form) -- so a known entry is bit for bit the point-path decode of the same point of the dense n^3
    lattice.  All three routes of generate_obj_mesh_wnf take it (visual: eager, not graph-captured; VTacOH and VTacO t2d: finger ids
    assigned at the query points), under the same range guard.  Refused (VtError): the attention decoder (TransformerFusion couples
    the points of a chunk: a sparse subset is not the dense field), a caller-supplied ``c_img_all`` (indexed by the dense lattice),
    generate_obj_mesh_sharded and generate_mesh_graphed.

    ``components`` / ``min_component_faces``: the connected components of the finished object mesh that are returned -- ``"all"``
    (the default), or the largest one by faces (``"largest"``), area (``"largest_area"``) or |signed volume| (``"largest_volume"``),
    after the components with fewer than ``min_component_faces`` faces are dropped.  With the defaults nothing runs.  Otherwise the
    filter (utils/mesh_clean.py) runs eagerly on the extracted mesh -- behind the graph replay where the route is graphed -- and costs
    three host reads (the labels' convergence flags, the component count, the kept vertex and face counts; one more per two further
    hooking rounds where hooks collided), in
    generate_obj_mesh_wnf (all three routes, dense and MISE), generate_mesh_graphed and generate_obj_mesh_tactile, and
    ``reference_returns`` measures the mesh that is returned.  Hand meshes and the Inferencer are left alone;
    generate_obj_mesh_sharded refuses a non-default value (VtError).

    ``simplify_nfaces`` (config ``generation.simplify_nfaces``): a positive integer N simplifies the finished object mesh to at most N
    faces -- ``Mesh.simplify(nfaces=N)``, vertex clustering with quadric placement (utils/mesh_clean.py, csrc/mesh_simplify.hip) --
    after the component filter, in the same places as that filter; everything downstream, ``reference_returns``' EMD and Chamfer
    included, sees the simplified mesh.  It costs one host read per probe of the search for the grid (some ten).  The result has at
    most N faces but is not the finest such grid, and its topology is not the input's (``Mesh.components()`` reports what it is).
    ``None`` (the default) launches nothing.  The Inferencer does not apply it; generate_obj_mesh_sharded refuses it (VtError).

    ``configure_simplify(method)`` (config ``generation.simplify_method``; a method, not a constructor argument, as
    ``configure_subdivide`` is): ``'cluster'`` (the default state) is the vertex clustering above, with not one launch more than
    before; ``'collapse'`` runs ``Mesh.decimate(nfaces=N)`` in its place -- rounds of independent quadric edge collapses,
    utils/mesh_clean.py, csrc/mesh_collapse.hip -- which keeps a closed manifold closed with its Euler number and lands on the largest
    even count <= N (boundary and non-manifold edges never move; where nothing more can collapse the result has more than N faces).
    It costs one host read per four rounds, tens of rounds of some twenty launches.  With ``with_normals`` the normals are recomputed
    from the geometry, as after clustering.  Any other value raises VtError; generate_obj_mesh_sharded refuses ``'collapse'``.

    ``fill_holes`` / ``fill_holes_max_edges`` (config ``generation.fill_holes`` / ``generation.fill_holes_max_edges``): ``'fan'`` or
    ``'centroid'`` caps the boundary loops of the finished object mesh -- ``Mesh.fill_holes(method, max_edges)``, utils/mesh_clean.py,
    csrc/mesh_fill.hip -- after the component filter (a dropped floater's holes are not worth closing) and before ``simplify_nfaces``
    (which then sees the closed surface), in the same places as those two.  Marching cubes on the unpadded lattice cuts the surface
    where the object reaches the box: those cuts are planar loops and are capped exactly.  ``fill_holes_max_edges``: only loops of at
    most that many edges.  It costs three host reads.  With ``with_normals``, ``'fan'`` keeps the marching-cubes normals and values (no
    vertex is added); ``'centroid'`` is refused in the constructor.  ``None`` (the default) launches nothing.  The Inferencer does not
    apply it; generate_obj_mesh_sharded refuses it (VtError).

    ``smooth`` / ``smooth_iterations`` (config ``generation.smooth`` / ``generation.smooth_iterations``): ``'laplacian'``, ``'taubin'``
    or ``'humphrey'`` runs that filter on the vertices of the finished object mesh -- ``Mesh.smooth(method, iterations)`` with its
    other defaults (uniform weights, boundary vertices pinned, so the planar cuts at the box stay where they are), utils/mesh_clean.py,
    csrc/mesh_smooth.hip -- after ``fill_holes`` and before ``simplify_nfaces``: the marching-cubes staircase is taken out at full
    resolution, before vertex clustering would amplify it.  It costs one host read (the adjacency's size); the passes are enqueued at
    once.  With ``with_normals`` the normals are recomputed from the smoothed geometry (``normals_source='geometry'``, no values).
    ``None`` (the default) launches nothing.  The Inferencer does not apply it; generate_obj_mesh_sharded refuses it (VtError).
    Pass both by keyword: in the signature they stand before ``refine_sampler``, whose place as third from the end, with
    ``fill_holes`` and ``fill_holes_max_edges`` as the last two, tests/test_mesh_fill_ref_cpu.py fixes.

    ``with_normals`` (config ``generation.with_normals``; the reference's "whether normals should be estimated"): every route that
    ends in ``extract_mesh`` -- dense, MISE, tactile, the graphed scene -- returns a ``NormalMesh`` whose ``vertex_normals`` and
    ``values`` are those of scikit-image's ``measure.marching_cubes`` (vt_mc_emit_normals: one launch behind the emit, outside the
    captured graph; ``normals_source='marching_cubes'``).  The component filter gathers them through its vertex map; after
    ``simplify_nfaces`` they are recomputed from the geometry, area-weighted (``normals_source='geometry'``, no values);
    ``generate_hand_mesh`` carries the geometric normals of the MANO vertices.  generate_obj_mesh_sharded refuses it (VtError); the
    Inferencer ignores it.  ``False`` (the default) launches and returns what it always did.

    ``refinement_step`` (config ``generation.refinement_step``; the Convolutional Occupancy Networks generator's ``refine_mesh``): a
    positive integer N runs N RMSprop iterations (torch's defaults, lr 1e-4) on the vertices of the finished object mesh -- after the
    component filter and ``simplify_nfaces``, upstream's order -- in generate_obj_mesh_wnf's visual route, dense and MISE.  Every
    iteration draws one point per face, pulls the occupancy there to ``threshold`` and the face normal to the negative normalised
    gradient of the occupancy, differentiating through that gradient: ``refine_mesh`` below, csrc/field_jet.hip and csrc/refine.hip,
    six launches per iteration and no host read.  The encoder runs once more, eagerly, for the feature volume (a graphed route keeps
    its own inside the graph).  ``refine_sampler='device'`` (the default) draws the points' weights in the kernel from a counter hash
    of (seed 0, step, face); ``'numpy'`` draws ``np.random.dirichlet((0.5, 0.5, 0.5), size=F)`` from numpy's global generator once per
    step and uploads it, exactly as upstream.  With ``with_normals`` the normals are recomputed from the refined geometry
    (``normals_source='geometry'``, no values); ``reference_returns`` measures the refined mesh.  Refused (VtError, in the constructor):
    a negative or non-integer value, and with N > 0 the tactile routes (``with_img``, ``encode_t2d``), the attention decoder, plane
    features, the PointConv baseline and decoder shapes other than hidden 32 / c_dim 32 / 5 blocks (the jet kernel's shape);
    generate_mesh_graphed, generate_obj_mesh_sharded and generate_obj_mesh_tactile refuse N > 0 when called.  The Inferencer ignores
    it.  ``0`` (the default) launches nothing and returns what it always did.

    ``configure_subdivide(scheme, iterations, max_edge)`` (config ``generation.subdivide`` / ``generation.subdivide_iterations`` /
    ``generation.subdivide_max_edge``; a method, not a constructor argument: tests pin the constructor's parameter list): ``'midpoint'``
    or ``'loop'`` subdivides the finished object mesh ``iterations`` times, or with ``max_edge`` (``'midpoint'`` only) until no edge is
    longer -- ``Mesh.subdivide`` / ``subdivide_loop`` / ``subdivide_to_size``, utils/mesh_clean.py, csrc/mesh_subdivide.hip -- after
    ``smooth`` and before ``simplify_nfaces``, so ``refinement_step`` moves the vertices of the denser mesh onto the isosurface: a
    coarse extraction, subdivision and refinement reach resolution without a denser lattice.  One host read per round.  With
    ``with_normals`` the normals are recomputed from the geometry (``normals_source='geometry'``, no values).  ``None`` (the default
    state) launches nothing.  The Inferencer does not apply it; generate_obj_mesh_sharded refuses it (VtError)."""

    EXTRACTIONS = ("dense", "mise")
    COMPONENTS = ("all", "largest", "largest_area", "largest_volume")
    REFINE_SAMPLERS = ("device", "numpy")
    FILL_HOLES = (None, "fan", "centroid")
    SMOOTH = (None, "laplacian", "taubin", "humphrey")
    SUBDIVIDE = (None, "midpoint", "loop")
    # configure_subdivide's state; the class attributes are the default: nothing runs
    subdivide, subdivide_iterations, subdivide_max_edge = None, 1, None
    SIMPLIFY_METHODS = ("cluster", "collapse")
    # configure_simplify's state; the class attribute is the default: vertex clustering
    simplify_method = "cluster"

    MAX_SCENE_GRAPHS = 4
    FUSED_CHUNKS_PER_CALL = 256          # attention_local: chunks of points_batch_size points evaluated per launch sequence (see _fused_chunks_per_call)
    # generate_obj_mesh_wnf replays the visual branch as a captured hipGraph (VTACO_SCENE_GRAPH=0: eager launches)
    scene_graph = os.environ.get("VTACO_SCENE_GRAPH", "1") != "0"

    def __init__(self, model, points_batch_size=100000, threshold=0.5, refinement_step=0, device=None,
                 resolution0=16, upsampling_steps=3, with_normals=False, padding=0.1, sample=False,
                 input_type=None, vol_info=None, vol_bound=None, simplify_nfaces=None, alpha=0.2,
                 with_img=False, encode_t2d=False, decode_precision="f16x3", depth_origin=None, reference_returns=False,
                 extraction="dense", components="all", min_component_faces=0, smooth=None, smooth_iterations=10,
                 refine_sampler="device", fill_holes=None, fill_holes_max_edges=None):
        if smooth not in self.SMOOTH:
            raise VtError(f"Generator3D: smooth must be one of {self.SMOOTH} (got {smooth!r})")
        if isinstance(smooth_iterations, bool) or not isinstance(smooth_iterations, numbers.Integral) or smooth_iterations < 0:
            raise VtError(f"Generator3D: smooth_iterations must be an integer >= 0 (got {smooth_iterations!r})")
        # None -- the default -- returns the mesh as extracted and launches nothing
        self.smooth, self.smooth_iterations = smooth, int(smooth_iterations)
        if isinstance(refinement_step, bool) or not isinstance(refinement_step, numbers.Integral) or refinement_step < 0:
            raise VtError(f"Generator3D: refinement_step must be an integer >= 0 (got {refinement_step!r})")
        if refine_sampler not in self.REFINE_SAMPLERS:
            raise VtError(f"Generator3D: refine_sampler must be one of {self.REFINE_SAMPLERS} (got {refine_sampler!r})")
        if components not in self.COMPONENTS:
            raise VtError(f"Generator3D: components must be one of {self.COMPONENTS} (got {components!r})")
        if int(min_component_faces) != min_component_faces or min_component_faces < 0:
            raise VtError(f"Generator3D: min_component_faces must be an integer >= 0 (got {min_component_faces!r})")
        # which connected components of the finished object mesh are returned (utils/mesh_clean.py): "all" with
        # min_component_faces 0 -- the defaults -- returns the mesh as extracted and launches nothing
        self.components, self.min_component_faces = components, int(min_component_faces)
        if simplify_nfaces is not None and (isinstance(simplify_nfaces, bool) or not isinstance(simplify_nfaces, numbers.Integral)
                                            or simplify_nfaces < 1):
            raise VtError(f"Generator3D: simplify_nfaces must be a positive integer or None (got {simplify_nfaces!r})")
        if fill_holes not in self.FILL_HOLES:
            raise VtError(f"Generator3D: fill_holes must be one of {self.FILL_HOLES} (got {fill_holes!r})")
        if fill_holes_max_edges is not None and (isinstance(fill_holes_max_edges, bool) or not isinstance(fill_holes_max_edges, numbers.Integral)
                                                 or fill_holes_max_edges < 3):
            raise VtError(f"Generator3D: fill_holes_max_edges must be an integer >= 3 or None (got {fill_holes_max_edges!r})")
        if fill_holes == "centroid" and with_normals:
            raise VtError("Generator3D(fill_holes='centroid', with_normals=True): the vertices the caps add have no marching-cubes normal or "
                          "value; use fill_holes='fan', which adds none, or leave with_normals off and take geometric normals of the "
                          "returned mesh with Mesh.with_vertex_normals()")
        # None -- the default -- returns the mesh as extracted and launches nothing
        self.fill_holes = fill_holes
        self.fill_holes_max_edges = None if fill_holes_max_edges is None else int(fill_holes_max_edges)
        if extraction not in self.EXTRACTIONS:
            raise VtError(f"Generator3D: extraction must be one of {self.EXTRACTIONS} (got {extraction!r})")
        if extraction == "mise" and hasattr(getattr(model, "decoder", None), "fuser"):
            raise VtError("Generator3D(extraction='mise'): the attention decoder couples the points of a chunk (TransformerFusion), "
                          "so the field at a sparse subset of the lattice is not the dense field; use extraction='dense'")
        self.extraction = extraction
        self.model = model.to(device)
        # True: generate_obj_mesh_wnf returns (mesh, emd, cd) as the reference's does (generation.py:274-284) -- the metrics of
        # the mesh against data['points.points_obj'], computed on the device (reference_metrics); False: the mesh alone
        self.reference_returns = reference_returns
        # arithmetic of the dense lattice decode (eval_lattice): "f16x3" = split-f16 MFMA (the default: f32-level logit error,
        # ~1e-6 on the goldens, for hidden activations below 65504 -- guarded, see _range_guarded), "bf16x3" = split-bf16 MFMA
        # (f32's exponent range, ~1.6e-5), "f32" = exact-f32 MFMA, "f16f8" = f16 products + fp8 correction products (opt-in:
        # fewer matrix cycles, but its error is RELATIVE, ~3e-5 |logit| -- inside the 1e-4 bar for |logit| <~ 2.5 only -- and
        # the mesh is not vertex-for-vertex the f32 path's; slabs it does not cover run as "f16x3").  eval_points follows the
        # decoder's own ``precision`` attribute (default "f32").
        self.decode_precision = decode_precision
        self.points_batch_size = points_batch_size
        self.threshold, self.refinement_step, self.refine_sampler = threshold, int(refinement_step), refine_sampler
        self.device = device
        self.resolution0, self.upsampling_steps = resolution0, upsampling_steps
        self.with_normals, self.input_type, self.padding, self.sample = with_normals, input_type, padding, sample
        self.simplify_nfaces, self.alpha = None if simplify_nfaces is None else int(simplify_nfaces), alpha
        self.with_img, self.encode_t2d = with_img, encode_t2d
        # the tactile sensor's flat depth reading [240*320] (the VTacO branch compares every depth image with it): an array, a
        # path, or None = the reference's ./data/VTacO_mesh/depth_origin.txt (generation.py:17), read when first needed
        self.depth_origin = depth_origin
        self.vol_bound = vol_bound
        if input_type == 'pointcloud_crop':
            raise VtError("Generator3D: crop / sliding-window mode is not built (no shipped config uses it)")
        if self.refinement_step > 0:
            self._refuse_refinement_config()

    def configure_subdivide(self, scheme=None, iterations=1, max_edge=None):
        """Subdivide the finished object mesh in ``_clean`` (the class docstring); ``scheme=None`` turns it off again.  Returns self."""
        if scheme not in self.SUBDIVIDE:
            raise VtError(f"Generator3D.configure_subdivide: scheme must be one of {self.SUBDIVIDE} (got {scheme!r})")
        if isinstance(iterations, bool) or not isinstance(iterations, numbers.Integral) or iterations < 0:
            raise VtError(f"Generator3D.configure_subdivide: iterations must be an integer >= 0 (got {iterations!r})")
        if max_edge is not None:
            if isinstance(max_edge, bool) or not isinstance(max_edge, numbers.Real) or not 0.0 < float(max_edge) < float("inf"):
                raise VtError(f"Generator3D.configure_subdivide: max_edge must be a positive finite number or None (got {max_edge!r})")
            if scheme != "midpoint":
                raise VtError(f"Generator3D.configure_subdivide: max_edge goes with scheme='midpoint' (got {scheme!r})")
        self.subdivide, self.subdivide_iterations = scheme, int(iterations)
        self.subdivide_max_edge = None if max_edge is None else float(max_edge)
        return self

    def configure_simplify(self, method="cluster"):
        """How ``simplify_nfaces`` is met in ``_clean`` (the class docstring): ``'cluster'`` or ``'collapse'``.  Returns self."""
        if method not in self.SIMPLIFY_METHODS:
            raise VtError(f"Generator3D.configure_simplify: method must be one of {self.SIMPLIFY_METHODS} (got {method!r})")
        self.simplify_method = method
        return self

    def _subdivided(self, mesh):
        if self.subdivide is None or mesh.faces.shape[0] == 0:
            return mesh
        if self.subdivide_max_edge is not None:
            return mesh.subdivide_to_size(self.subdivide_max_edge)       # (``iterations`` does not count here)
        if self.subdivide == "loop":
            return mesh.subdivide_loop(self.subdivide_iterations)
        return mesh.subdivide(self.subdivide_iterations)

    # -- refinement_step: RMSprop on the vertices against the field's jet -----------
    def _refuse_refinement_config(self):
        """What refinement_step > 0 cannot be combined with, said before anything is launched."""
        if self.with_img or self.encode_t2d:
            raise VtError("Generator3D(refinement_step > 0): not built for the tactile routes (with_img / encode_t2d): the field there "
                          "also depends on the finger features assigned to each point, and the jet kernel differentiates the plain decoder")
        self._refuse_planes("refinement_step > 0", "the jet kernel differentiates the trilinear sample of a feature volume")
        self._refuse_point("refinement_step > 0", "its features are sampled from a point cloud, not a feature volume")
        ops.refine.refine_check(getattr(self.model, "decoder", None))

    def _refuse_refinement(self, what, instead):
        if self.refinement_step > 0:
            raise VtError(f"Generator3D.{what}: refinement_step is not built for this route; {instead}")

    def refine_mesh(self, mesh, c, steps=None, eps=None, seed=0):
        """Upstream's ``refine_mesh(mesh, occ_hat, c)`` without the unused ``occ_hat``: ``steps`` (None: ``refinement_step``) RMSprop
        iterations on the vertices against the decoder's field on the encoder output ``c`` (the feature volume, or the dict that holds
        it alone).  ``eps`` [steps,F,3]: the face points' weights instead of a draw; ``seed``: the device sampler's.  Returns a Mesh
        with the same faces and float32 vertices -- a NormalMesh with the normals of the refined geometry where ``mesh`` is one."""
        steps = self.refinement_step if steps is None else int(steps)
        dec = self.model.decoder
        ops.refine.refine_check(dec)
        if isinstance(c, (tuple, list)):
            raise VtError("Generator3D.refine_mesh: the PointConv baseline's (cloud, features) pair is not a feature volume")
        grid = dec._grid_of(c, "refine_mesh") if isinstance(c, dict) else c
        if steps <= 0 or mesh.faces.shape[0] == 0:
            return mesh
        verts = ops.refine.refine(mesh.vertices.float(), mesh.faces, grid, dec, steps, self.threshold, dec.padding, eps=eps, seed=seed,
                           sampler=self.refine_sampler)
        out = Mesh(verts, mesh.faces)
        if isinstance(mesh, NormalMesh):
            from ..utils import mesh_clean
            return mesh_clean.with_vertex_normals(out, weight="area")
        return out

    def _refined(self, mesh, data):
        """generate_obj_mesh_wnf's refinement: the scene encoded once more, eagerly, for its feature volume."""
        if mesh.faces.shape[0] == 0:
            return mesh
        self._eval_mode()
        with torch.no_grad():
            c = self.model.encode_inputs(data.get('inputs').to(self.device))
        return self.refine_mesh(mesh, c)

    # -- reference API: arbitrary points, chunked, result on the CPU ---------------
    def eval_points(self, p, c=None, c_img_all=None, vol_bound=None, **kwargs):
        """Occupancy logits [N] (CPU tensor, as the reference returns) for points p [N,3]."""
        p = p.to(self.device)
        ci = None if c_img_all is None else c_img_all.reshape(-1, c_img_all.shape[-1]).to(self.device)
        outs = []
        with torch.no_grad():
            lo0 = 0
            if self.with_img and ci is not None and hasattr(self.model.decoder, 'fuser'):
                # decoder attention_local: the whole chunks as batches of chunks (see _eval_lattice_fused), the ragged rest below
                dec, chunk = self.model.decoder, self.points_batch_size
                grid = dec._grid_of(c)
                full = p.shape[0] // chunk
                per_call = self._fused_chunks_per_call(chunk)
                for lo in range(0, full, per_call):
                    nb = min(per_call, full - lo)
                    sl = slice(lo * chunk, (lo + nb) * chunk)
                    pb = p[sl].float()
                    feat = ops.sample_grid(grid, pb.unsqueeze(0), dec.padding).reshape(nb, chunk, -1)
                    fused = dec.fuser(ci[sl].float().reshape(nb, chunk, -1), 1, feat, 1)
                    outs.append(dec._mlp_fwd(fused, pb.reshape(nb, chunk, 3)).reshape(-1))
                lo0 = full * chunk
            for lo in range(lo0, p.shape[0], self.points_batch_size):
                pi = p[lo:lo + self.points_batch_size].unsqueeze(0)
                if self.with_img and ci is not None:
                    occ = self.model.decode_img(pi, c, ci[lo:lo + self.points_batch_size].unsqueeze(0), **kwargs).logits
                else:
                    occ = self.model.decode(pi, c, **kwargs).logits
                outs.append(occ.squeeze(0))
        return torch.cat(outs, dim=0).detach().cpu()

    def _fused_chunks_per_call(self, chunk):
        """Chunks of ``chunk`` points per launch sequence of the attention decoder: FUSED_CHUNKS_PER_CALL, but at most 2^19 points
        (the fusion workspace is ~1.3 KB per point: 0.7 GB there, whatever the chunk size)."""
        return max(1, min(self.FUSED_CHUNKS_PER_CALL, (1 << 19) // max(int(chunk), 1)))

    # -- fast path: the nx^3 lattice never exists as a tensor ----------------------
    def eval_lattice(self, c, nx, c_img_all=None, first=0, count=None, out=None):
        """Logits of the (1+padding)-box lattice, device tensor [count] (whole: nx^3).  ``out``: a contiguous float32 tensor of
        ``count`` elements to write them into."""
        if isinstance(c, (tuple, list)):
            # the PointConv baseline's (cloud, per-point features): the lattice form of the point-feature sampler, slab by slab
            self._refuse_point_tactile("eval_lattice", c_img_all)
            if c[1].shape[0] != 1:
                raise VtError("eval_lattice: one scene at a time (the lattice is per scene)")
            if count == 0:
                return torch.empty(0, dtype=torch.float32, device=c[1].device)
            return self.model.decoder.decode_lattice(c, nx, box=1 + self.padding, first=first, count=count, out=out,
                                                     precision=self.decode_precision).reshape(-1)
        if isinstance(c, dict) and set(c) != {'grid'}:
            # plane features (alone or next to the volume): the decoder's sampled route, slab by slab (LocalDecoder.decode_lattice)
            one = next(iter(c.values()))
            if one.shape[0] != 1:
                raise VtError("eval_lattice: one scene at a time (the lattice is per scene)")
            if count == 0:
                return torch.empty(0, dtype=torch.float32, device=one.device)
            return self.model.decoder.decode_lattice(c, nx, box=1 + self.padding, first=first, count=count, c_img=c_img_all, out=out,
                                                     precision=self.decode_precision).reshape(-1)
        grid = c['grid'] if isinstance(c, dict) else c
        if grid.shape[0] != 1:
            raise VtError("eval_lattice: one scene at a time (the lattice is per scene)")
        if count == 0:                                   # an empty slab of a sharded lattice: no kernel
            return torch.empty(0, dtype=torch.float32, device=grid.device)
        return self.model.decoder.decode_lattice(grid, nx, box=1 + self.padding, first=first, count=count,
                                                 c_img=c_img_all, out=out, precision=self.decode_precision).reshape(-1)

    def _plane_model(self):
        """True if the model's encoder returns canonical planes ('xz','xy','yz') instead of the feature volume."""
        enc = getattr(self.model, "encoder", None)
        return enc is not None and getattr(enc, "planes", ['grid']) != ['grid']

    def _refuse_planes(self, what, why):
        if self._plane_model():
            raise VtError(f"Generator3D.{what}: the encoder returns plane features {self.model.encoder.planes}, which this route does "
                          f"not take ({why}); generate_obj_mesh_wnf without with_img and eval_lattice decode them")

    def _point_model(self):
        """True for the PointConv baseline: the decoder takes (cloud, per-point features) instead of a grid or planes."""
        from .models.decoder import LocalPointDecoder
        return isinstance(getattr(self.model, "decoder", None), LocalPointDecoder)

    def _refuse_point(self, what, why):
        if self._point_model():
            raise VtError(f"Generator3D.{what}: not built for the PointConv baseline (pointnet_plus_plus / simple_local_point): {why}")

    def _refuse_point_tactile(self, what, c_img_all=None):
        if self.with_img or c_img_all is not None:
            raise VtError(f"Generator3D.{what}: the PointConv decoder has no tactile variant (the reference's LocalPointDecoder has "
                          "neither forward_img nor a contact head)")

    def extract_mesh(self, value_grid, level=None, with_normals=None):
        """``measure.marching_cubes(value_grid, gradient_direction='ascent')`` followed by
        ``vertices -= nx/2; vertices *= (1+padding)/nx`` (generation.py:270-272), on the device.  With ``with_normals`` (None: the
        generator's own flag) the result is a ``NormalMesh`` with scikit-image's normals and values: one more launch."""
        nx = value_grid.shape[0]
        return self._marching_cubes(value_grid, level, (nx / 2, (1 + self.padding) / nx), with_normals)

    def _marching_cubes(self, value_grid, level, rescale, with_normals=None):
        if self.with_normals if with_normals is None else with_normals:
            verts, faces, normals, values, _ = ops.mc.marching_cubes_normals(value_grid, level, rescale=rescale)
            return NormalMesh(verts, faces, vertex_normals=normals, values=values, normals_source="marching_cubes")
        verts, faces, _ = ops.marching_cubes(value_grid, level, rescale=rescale)
        return Mesh(verts, faces)

    # -- whole scene as ONE hipGraph replay (encode + dense decode + marching-cubes count) --------
    def _module_tables(self):
        """The model's modules and their parameter / buffer dicts, listed once per model object: the per-scene checks below
        walk these lists instead of ``nn.Module``'s recursive generators (0.3 ms each for the ~110 tensors of the shipped model,
        more than a quarter of a graphed scene).  A module's dict is updated in place when a weight is replaced, so the lists
        stay valid; submodules (or a module's first parameter) added after the first call are not followed."""
        tab = getattr(self, "_tables", None)
        if tab is None or tab[0] is not self.model:
            mods = list(self.model.modules())
            tab = self._tables = (self.model, mods, [d for m in mods for d in (m._parameters, m._buffers) if d])
        return tab

    def _set_decode_precision(self, precision):
        """Move the lattice decode to ``precision`` (the range guard's downgrade); "bf16x3" / "f32" also take the attention decoder's
        MLP back to the exact kernel."""
        self.decode_precision = precision
        if precision in ("bf16x3", "f32") and hasattr(self.model.decoder, "mlp_precision"):
            self.model.decoder.mlp_precision = "f32"

    def _eval_mode(self):
        """``self.model.eval()`` (generation.py:66, 131), skipped when every module already is in eval mode."""
        if any(m.training for m in self._module_tables()[1]):
            self.model.eval()

    def _weight_stamps(self):
        """(object, storage address, version counter) of every parameter and buffer: changes when a weight is updated in place
        (optimizer.step, load_state_dict), moved (``.to()`` swaps the storage under the same Parameter) or replaced."""
        ts = [t for d in self._module_tables()[2] for t in d.values() if t is not None]
        return tuple(map(id, ts)), tuple(map(torch.Tensor.data_ptr, ts)), tuple(map(_tensor_version, ts))

    def _captured(self, key, shapes, run):
        """The captured graph of ``run(*static_inputs)`` for one key (kind, input shapes, ...): ``{"graph", "in": static inputs, "out":
        what run returned, ...}``.  A graph holds raw pointers to derived buffers -- packed conv weights, the decoder blob, the UNet3D
        workspace -- that live in caches keyed on the weights' versions and on the last shape run; so the entry (a) keeps every such
        tensor alive next to the graph (``ops.graph_keepalive``) and (b) records the weight stamps at capture: a replay after
        ``optimizer.step()`` / ``load_state_dict`` / ``.to()`` finds different stamps and captures afresh instead of reading stale
        or recycled memory.  At most MAX_SCENE_GRAPHS entries stay captured, least recently used first out."""
        self._graphs = getattr(self, "_graphs", {})
        hit = self._graphs.get(key)
        stamps = self._weight_stamps()
        if hit is not None and hit["stamps"] == stamps:
            if len(self._graphs) > 1:
                self._graphs[key] = self._graphs.pop(key)   # most recently used last
            return hit
        self._drop_graph(key)                            # stale: drop the old graph (and its keep-alive list) first
        while len(self._graphs) >= self.MAX_SCENE_GRAPHS:   # every graph pins its workspaces (~0.5 GB at 128^3): keep a few shapes
            self._drop_graph(next(iter(self._graphs)))
        static = [torch.zeros(shape, dtype=torch.float32, device=self.device) for shape in shapes]
        with ops.graph_keepalive() as keep:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side), torch.no_grad():
                for _ in range(2):                      # warm-up: fills every cache / workspace outside the capture
                    run(*static)
            torch.cuda.current_stream().wait_stream(side)
            # the stamps the entry is valid for are taken AFTER the warm-up (a module that bumps a buffer's version during its
            # forward would otherwise look changed at every call and be captured again each time) ...
            stamps = self._weight_stamps()
            graph = torch.cuda.CUDAGraph()
            with torch.no_grad(), torch.cuda.graph(graph):
                out = run(*static)
            # ... and must not move while the graph is recorded: a capture that changes a weight cannot be replayed safely
            if self._weight_stamps() != stamps:
                raise VtError("Generator3D: the model's parameters or buffers changed while its launches were being captured; "
                              "set scene_graph = False for models whose forward updates state")
        self._graphs[key] = {"graph": graph, "in": static, "out": out, "keep": list(keep), "stamps": stamps}
        return self._graphs[key]

    def _drop_graph(self, key):
        """Forget a captured graph; its marching-cubes echo slot (a page-locked block, 64 per process) goes back to the pool once the
        device has drained the graph's last replay."""
        hit = self._graphs.pop(key, None)
        if hit is not None and hit.get("echo") is not None:
            torch.cuda.synchronize()
            hit.pop("graph", None)
            ops.mc_echo_release(hit["echo"])

    def __del__(self):
        try:
            for key in list(getattr(self, "_graphs", {})):
                self._drop_graph(key)
        except Exception:                                 # noqa: BLE001 -- interpreter shutdown: the library may be gone
            pass

    def _scene_graph(self, shape, nx):
        """Encode + dense decode + marching-cubes classification of one (input shape, lattice size) as one graph."""
        key = (tuple(shape), nx, self.decode_precision)
        hit = getattr(self, "_graphs", {}).get(key)
        # the counts of a replay arrive in a page-locked slot the scan kernel writes (no copy command between it and the emit kernels);
        # the slot is made before the capture and belongs to this graph
        if hit is not None and "echo" in hit:
            echo = hit.pop("echo")                        # (a stale entry is re-captured below: its slot moves to the new graph)
        else:
            try:
                echo = ops.mc_echo_slot() if _MC_ECHO else None
            except VtError:                                           # every slot taken (64 captured shapes): the copy + event form
                echo = None

        def run(static_in):
            c = self.model.encode_inputs(static_in)
            vol = self.eval_lattice(c, nx).reshape(nx, nx, nx)
            return vol, (ops.mc_count_echo(vol, None, echo) if echo is not None else ops.mc_count(vol))
        g = self._captured(key, [shape], run)
        g["vol"], g["ws"] = g["out"]
        g["echo"] = echo
        return g

    def _graphs_allowed(self):
        """Captured graphs are used in single-process runs only: with several ranks per node the launches stay eager -- two processes
        replaying graphs on ONE device (the gloo dry-run of the multi-rank bench) took 180 ms per replay, and the one-process-per-GPU
        case could not be measured on this pool (the encoder is then 1.0 instead of 0.7 ms per scene)."""
        if not self.scene_graph:
            return False
        import torch.distributed as dist
        return not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1)

    def _worth_capturing(self, key):
        """A capture costs two warm-up runs and a recording (tens of milliseconds): a shape is captured when it comes back, not the
        first time it is seen -- callers whose clouds all differ in size stay on plain launches instead of recording a graph per call."""
        if key in getattr(self, "_graphs", {}):
            return True
        seen = self.__dict__.setdefault("_seen_shapes", {})
        if key in seen:
            return True
        if len(seen) >= 64:
            seen.pop(next(iter(seen)))
        seen[key] = True
        return False

    def _replay(self, kind, tensors, run):
        """``run(*tensors)`` through a captured graph per (kind, shapes) when ``self.scene_graph`` is on.  LIFETIME of the result:
        it lives in the graph's static buffers -- the next replay of the same (kind, shapes) overwrites it in place, and the entry
        can be evicted (MAX_SCENE_GRAPHS, least recently used) -- so it is for use within the current scene; a caller that keeps
        encoder outputs across scenes (``c`` of one cloud next to the ``c`` of another of the same shape) clones them.  The
        generator's own entry points consume the result before they return.  Plain call otherwise."""
        key = (kind,) + tuple(tuple(t.shape) for t in tensors)
        if not self._graphs_allowed() or not self._worth_capturing(key):
            with torch.no_grad():
                return run(*[t.to(self.device) for t in tensors])
        g = self._captured(key, [t.shape for t in tensors], run)
        for dst, src in zip(g["in"], tensors):
            dst.copy_(src.to(self.device), non_blocking=True)
        g["graph"].replay()
        return g["out"]

    def _filters_components(self):
        return self.components != "all" or self.min_component_faces > 0

    def _clean(self, mesh):
        """The returned components of a finished object mesh (``components``, ``min_component_faces``), its boundary loops capped
        (``fill_holes``), its vertices smoothed (``smooth``), its faces subdivided (``configure_subdivide``), then simplified to ``simplify_nfaces`` faces; the mesh itself with the
        defaults."""
        mesh = self._kept_components(mesh)
        if self.fill_holes is not None and mesh.faces.shape[0] > 0:
            mesh = mesh.fill_holes(self.fill_holes, self.fill_holes_max_edges)
        if self.smooth is not None and mesh.faces.shape[0] > 0:
            mesh = mesh.smooth(self.smooth, self.smooth_iterations)
        mesh = self._subdivided(mesh)
        if self.simplify_nfaces is None or mesh.faces.shape[0] <= self.simplify_nfaces:
            return mesh
        from ..utils import mesh_clean
        if self.simplify_method == "collapse":
            simplified = mesh_clean.decimate(mesh, self.simplify_nfaces)
        else:
            simplified = mesh_clean.simplify(mesh, nfaces=self.simplify_nfaces)
        if isinstance(mesh, NormalMesh) and simplified.faces.shape[0] > 0:
            # both methods move the vertices: marching cubes' normals no longer belong to them -- recomputed from the geometry
            return mesh_clean.with_vertex_normals(simplified, weight="area")
        return simplified

    def _kept_components(self, mesh):
        if not self._filters_components() or mesh.faces.shape[0] == 0:
            return mesh
        from ..utils import mesh_clean
        comps = mesh_clean.components(mesh)
        keep = comps.n_faces >= self.min_component_faces
        if self.components != "all":
            keep = mesh_clean.largest_mask(comps, {"largest": "faces", "largest_area": "area", "largest_volume": "volume"}[self.components], among=keep)
        if not isinstance(mesh, NormalMesh):
            return mesh_clean._filtered(mesh.vertices, mesh.faces, comps, keep)
        # the normals and values of the kept vertices, through the filter's vertex map (the kept vertices keep their order)
        table = ops.mesh.ComponentTable(comps.n_components, comps.comp_of_vertex, comps.comp_of_face)
        out = ops.mesh.filter_components(mesh.vertices, mesh.faces, table, keep)
        kept = out.vertex_map >= 0
        if out.vertices.shape[0] == 0:
            return Mesh(out.vertices, out.faces)
        return NormalMesh(out.vertices, out.faces, vertex_normals=mesh.vertex_normals[kept],
                          values=None if mesh.values is None else mesh.values[kept], normals_source=mesh.normals_source)

    def generate_mesh_graphed(self, inputs):
        """``_generate_mesh_graphed`` (the captured visual branch), then the component filter where one is set."""
        self._refuse_refinement("generate_mesh_graphed", "generate_obj_mesh_wnf refines behind the same graph replay")
        return self._clean(self._generate_mesh_graphed(inputs))

    @_range_guarded
    def _generate_mesh_graphed(self, inputs):
        """Same result as ``generate_obj_mesh_wnf({'inputs': inputs})`` for the visual branch, with the
        ~110 launches of encode + decode + marching-cubes classification replayed as one hipGraph
        (launch-bound otherwise); only the data-dependent output sizing leaves the graph.  Safe across weight
        updates and interleaved eager calls of other shapes (see ``_scene_graph``).  Dense extraction only."""
        self._refuse_mise("generate_mesh_graphed")
        self._refuse_point("generate_mesh_graphed", "the encoder draws its farthest-point start indices from the CPU generator, once "
                           "per scene; a captured graph would replay one draw for ever")
        self._refuse_planes("generate_mesh_graphed", "the captured scene graph holds the fused volume decode, vt_decode_fwd*")
        self._eval_mode()
        nx = self.resolution0 * 4
        g = self._scene_graph(inputs.shape, nx)
        g["in"][0].copy_(inputs.to(self.device), non_blocking=True)
        if g.get("echo") is not None:
            ops.mc_echo_arm(g["echo"])                               # the number this replay's scan kernel writes behind the counts
        g["graph"].replay()
        verts, faces, _ = ops.mc_emit(g["vol"], g["ws"], rescale=(nx / 2, (1 + self.padding) / nx), echo=g.get("echo"))
        if self.with_normals:                                        # one launch behind the emit, outside the captured graph
            normals, values = ops.mc.mc_emit_normals(g["vol"], g["ws"], verts.shape[0])
            return NormalMesh(verts, faces, vertex_normals=normals, values=values, normals_source="marching_cubes")
        return Mesh(verts, faces)

    def generate_obj_mesh_sharded(self, data, group=None):
        """``_generate_obj_mesh_sharded``; a component filter, ``fill_holes``, ``smooth`` or ``simplify_nfaces`` is refused before anything is launched."""
        self._refuse_refinement("generate_obj_mesh_sharded", "refine the returned mesh with Mesh.refine(generator, c)")
        if self.with_normals:
            raise VtError("generate_obj_mesh_sharded: with_normals is not built for the sharded route; take the normals of the returned "
                          "mesh with Mesh.with_vertex_normals(), or ops.mc.marching_cubes_normals of the gathered value grid")
        if self.simplify_method != "cluster":
            raise VtError("generate_obj_mesh_sharded: simplify_method='collapse' (configure_simplify) is not built for the sharded route; "
                          "decimate the returned mesh with Mesh.decimate(nfaces)")
        if self.simplify_nfaces is not None:
            raise VtError("generate_obj_mesh_sharded: simplify_nfaces is not built for the sharded route; simplify the returned mesh with "
                          "Mesh.simplify(nfaces=...)")
        if self.fill_holes is not None:
            raise VtError("generate_obj_mesh_sharded: fill_holes is not built for the sharded route; fill the returned mesh with "
                          "Mesh.fill_holes(method, max_edges)")
        if self.smooth is not None:
            raise VtError("generate_obj_mesh_sharded: smooth is not built for the sharded route; smooth the returned mesh with "
                          "Mesh.smooth(method, iterations)")
        if self.subdivide is not None:
            raise VtError("generate_obj_mesh_sharded: subdivision (configure_subdivide) is not built for the sharded route; subdivide the "
                          "returned mesh with Mesh.subdivide / subdivide_loop / subdivide_to_size")
        if self._filters_components():
            raise VtError("generate_obj_mesh_sharded: the component filter (components / min_component_faces) is not built for the sharded "
                          "route; filter the returned mesh with Mesh.keep_largest / Mesh.remove_small")
        return self._generate_obj_mesh_sharded(data, group)

    @_range_guarded(collective=True)
    def _generate_obj_mesh_sharded(self, data, group=None):
        """``generate_obj_mesh_wnf`` with the lattice split over the ranks of a process group (one process per GPU):
        every rank encodes the scene (cheap, deterministic: no broadcast), decodes its slab of x-plane pairs with no
        data-path collective, one all_gather of the logit slabs (8.4 MB at 128^3, 67 MB at 256^3) rebuilds the value
        grid, and every rank extracts the (identical) mesh.  Without an initialised group this is the single-GPU path.
        Dense extraction only."""
        from .. import dist as vdist
        self._refuse_mise("generate_obj_mesh_sharded")
        self._refuse_point("generate_obj_mesh_sharded", "every rank would draw its own farthest-point start indices, so the slabs of "
                           "one value grid would belong to different encodings")
        self._refuse_planes("generate_obj_mesh_sharded", "its slabs are aligned for the fused volume decode, vt_decode_fwd*")
        self._eval_mode()
        nx = self.resolution0 * 4
        inputs = data.get('inputs').to(self.device)
        c = self._replay("encode_inputs", [inputs], self.model.encode_inputs)        # the encoder's launches as one graph
        with torch.no_grad():
            if self.with_img:
                # the tactile branches (VTacOH fingertips / VTacO contact clouds): every rank assigns finger ids to ITS slab and
                # decodes by id; the VTacO clouds are drawn with numpy's generator, so rank 0's go to everybody (a few KB) -- and so
                # do rank 0's tactile FEATURES (F x C floats): they come out of the host framework's convolutions (MIOpen), whose
                # algorithm choice is made per process by timing, so two ranks may hold features that differ in the last bits and
                # the slabs of one value grid would not belong to one function
                setup = self._tactile_setup(data)
                if vdist.dist.is_initialized() and vdist.dist.get_world_size(group) > 1:
                    setup['feats'] = setup['feats'].float().contiguous()
                    for key in ('anchors', 'count', 'success', 'feats'):
                        t = setup[key].to(self.device)
                        vdist.dist.broadcast(t, src=vdist.dist.get_global_rank(group, 0) if group is not None else 0, group=group)
                        setup[key] = t
                fused = hasattr(self.model.decoder, 'fuser')
                values = vdist.decode_lattice_sharded(
                    lambda first, count: self._eval_lattice_tactile(c, nx, setup, first, count), nx, group,
                    align=self.points_batch_size if fused else None, device=self.device)
            else:
                values = vdist.decode_lattice_sharded(lambda first, count: self.eval_lattice(c, nx, first=first, count=count), nx, group,
                                                      device=self.device)
        return self.extract_mesh(values.reshape(nx, nx, nx))

    def generate_obj_mesh_tactile(self, data, finger_feats, anchors, success, mode='within', radius=None, count=None):
        """``_generate_obj_mesh_tactile``, then the component filter where one is set."""
        self._refuse_refinement("generate_obj_mesh_tactile", "the field there also depends on the finger features assigned to each point")
        return self._clean(self._generate_obj_mesh_tactile(data, finger_feats, anchors, success, mode=mode, radius=radius, count=count))

    @_range_guarded
    def _generate_obj_mesh_tactile(self, data, finger_feats, anchors, success, mode='within', radius=None, count=None):
        """Tactile branch of ``generate_obj_mesh_wnf`` (generation.py:159-257) without the dense
        ``c_img_all [1,nx^3,C]`` tensor and its CPU cdist glue: every lattice point gets the id of the finger whose
        contact points lie within ``radius`` (``mode='within'``, radius 0.015: VTacO, :245-255) or of the nearest
        successful fingertip (``mode='nearest'``, radius 0.05: VTacOH, :186-200) from ``vt_tactile_assign``, and the
        decoder reads ``finger_feats [F,C]`` by id (``vt_decode_fwd_ids``): 1 byte per point instead of 4*C.
        ``anchors [F,K,3]`` (K = 1 for 'nearest'), ``count [F]`` valid anchors per finger, ``success [F]``."""
        self._refuse_point("generate_obj_mesh_tactile", "the PointConv decoder has no tactile variant")
        self._eval_mode()
        nx = self.resolution0 * 4
        setup = {'feats': finger_feats, 'anchors': anchors, 'success': success, 'mode': mode,
                 'radius': (0.015 if mode == 'within' else 0.05) if radius is None else radius,
                 'count': count if count is not None else torch.full((anchors.shape[0],), anchors.shape[1], dtype=torch.int32)}
        inputs = data.get('inputs').to(self.device)
        c = self._replay("encode_inputs", [inputs], self.model.encode_inputs)        # the encoder's ~55 launches as one graph
        with torch.no_grad():
            values = self._eval_lattice_tactile(c, nx, setup)
        return self.extract_mesh(values.reshape(nx, nx, nx))

    def _eval_lattice_tactile(self, c, nx, setup, first=0, count=None):
        """Logits of lattice points [first, first+count) with the tactile features of ``setup`` (finger features, anchors, rule)."""
        count = nx ** 3 - first if count is None else count
        grid = c['grid'] if isinstance(c, dict) else c
        if count == 0:                                   # an empty slab of a sharded lattice: no kernel
            return torch.empty(0, dtype=torch.float32, device=grid.device)
        ids = ops.tactile_assign(setup['anchors'].to(self.device), setup['success'].to(self.device), setup['mode'], setup['radius'],
                                 lattice=(nx, 1 + self.padding, first, count), count=setup['count'].to(self.device))
        feats = setup['feats'].to(self.device)
        if hasattr(self.model.decoder, 'fuser'):
            return self._eval_lattice_fused(c, nx, ids, feats, first, count)
        return self.model.decoder.decode_lattice_ids(grid, nx, ids, feats, box=1 + self.padding, first=first, count=count,
                                                     precision=self.decode_precision).reshape(-1)

    def _eval_lattice_fused(self, c, nx, ids, finger_feats, first=0, count=None):
        """``decoder: attention_local`` over the lattice (BASELINE config 3's decoder): TransformerFusion couples the points
        of a chunk (attention + InstanceNorm over the chunk), so the chunk is part of the function -- ``points_batch_size``
        points at a time in lattice order, exactly as ``eval_points`` walks them (the reference default of 100 000 needs a
        40 GB attention matrix; 2048 is the workable setting).  The per-chunk tactile features are gathered from the finger ids.
        A slab must start on a chunk boundary (sharded generation aligns its slabs to the chunk)."""
        from ..common import make_3d_grid
        chunk = self.points_batch_size
        count = nx ** 3 - first if count is None else count
        if first % chunk:
            raise VtError(f"_eval_lattice_fused: slab start {first} splits a chunk of {chunk} points")
        # the lattice as the reference builds it (host arithmetic, generation.py:155-157), kept on the device per (nx, padding):
        # 25 MB at 128^3 that every scene of a run shares
        cache = self.__dict__.setdefault("_lattice_points", {})
        key = (nx, float(self.padding))
        if key not in cache:
            if len(cache) >= 2:
                cache.pop(next(iter(cache)))
            cache[key] = ((1 + self.padding) * make_3d_grid((-0.5,) * 3, (0.5,) * 3, (nx,) * 3)).to(self.device)
        pts = cache[key][first:first + count]
        feats = finger_feats.float().contiguous()
        out = torch.empty(count, dtype=torch.float32, device=self.device)
        dec = self.model.decoder
        grid = dec._grid_of(c)
        # whole chunks go through the kernels as a BATCH of chunks (each is its own attention / InstanceNorm problem, exactly as
        # in a call of its own: the same logits bit for bit) -- one chunk per call is ~20 launches per 2048 points, 100 ms of
        # launches for a 128^3 lattice whose arithmetic takes 15
        full = count // chunk
        per_call = self._fused_chunks_per_call(chunk)
        C = feats.shape[1]
        # the finger ids of the whole chunks, [full, chunk] (a view): the fusion kernels read the tactile rows by id
        # (vt_fusion_fwd_ids) -- no gathered [chunks, chunk, C] tensor, no framework indexing between vt_tactile_assign and the fuser
        P3, I2, O2 = pts[:full * chunk].reshape(full, chunk, 3), ids.reshape(-1)[:full * chunk].view(full, chunk), out[:full * chunk].view(full, chunk)

        def fused_chunks(sel):
            """The attention decoder on the chunks ``sel`` (a slice of consecutive chunks, or an index tensor)."""
            p = P3[sel]
            nb = p.shape[0]
            if isinstance(sel, slice):                      # consecutive chunks: the lattice range itself (points generated in the kernel)
                feat = ops.sample_grid(grid, None, dec.padding, lattice=(nx, 1 + self.padding, first + sel.start * chunk, nb * chunk))
                fused = dec.fuser.forward_ids(I2[sel], feats, feat.reshape(nb, chunk, -1))
            else:                                           # picked chunks: their id rows through the index list, in the kernel
                feat = ops.sample_grid(grid, p.reshape(1, -1, 3), dec.padding).reshape(nb, chunk, -1)
                fused = dec.fuser.forward_ids(I2, feats, feat, chunk_index=sel.to(torch.int32))
            O2[sel] = dec._mlp_fwd(fused, p)

        # (the shortcut below holds in eval mode only: under model.train() the reference's dropout breaks the 'constant row ->
        # InstanceNorm -> 0' argument; generation always runs in eval mode (_eval_mode), asserted here.  It costs one host read per
        # lattice (torch.nonzero), so a lattice that takes it cannot be captured into a hipGraph.)
        if full and self.skip_untouched_chunks and not dec.training:
            # A chunk NO point of which carries a tactile feature (the fingers touch a few per cent of a scene's chunks) needs no
            # attention at all: with c_img = 0 on the whole chunk the decoder's self-attention block returns the same vector for
            # every point, InstanceNorm over the chunk turns that into zeros, the cross-attention of an all-zero query block is
            # constant over the points again, and the last InstanceNorm leaves fuse(0, c) = 0 -- in exact arithmetic and, bit for
            # bit, in these kernels (constant rows leave the norm as exact zeros: fusion.hip, fusion_inorm_relu*; asserted in
            # tests/test_fusion_gpu.py; the reference's own f32 evaluation leaves rounding noise of ~1e-5 there, TransformerFusion.py
            # :144, 209-218).  Such chunks go through the conditioned MLP with zero features; the others through the whole fuser.
            touched = (I2 != 255).any(dim=1)
            t_idx, u_idx = torch.nonzero(touched).flatten(), torch.nonzero(~touched).flatten()      # one host read per lattice
            for lo in range(0, u_idx.numel(), per_call):
                sel = u_idx[lo:lo + per_call]
                O2[sel] = dec._mlp_fwd(self._zero_features(sel.numel() * chunk, C).view(-1, chunk, C), P3[sel])
            for lo in range(0, t_idx.numel(), per_call):
                fused_chunks(t_idx[lo:lo + per_call])
        else:
            for lo in range(0, full, per_call):
                fused_chunks(slice(lo, min(lo + per_call, full)))
        if full * chunk < count:                          # the ragged last chunk
            sl = slice(full * chunk, count)
            tail = ids.reshape(-1)[sl].view(1, -1)
            feat = ops.sample_grid(grid, pts[sl].unsqueeze(0), dec.padding)
            out[sl] = dec._mlp_fwd(dec.fuser.forward_ids(tail, feats, feat), pts[sl].unsqueeze(0))[0]
        return out

    # attention_local over a lattice: chunks without any tactile feature skip the fuser (see _eval_lattice_fused; VTACO_FUSION_SKIP_UNTOUCHED=0
    # or ``gen.skip_untouched_chunks = False`` sends every chunk through the three attention units)
    skip_untouched_chunks = os.environ.get("VTACO_FUSION_SKIP_UNTOUCHED", "1") != "0"

    def _zero_features(self, rows, C):
        """[rows, C] zeros on the device, never written: the fused features of chunks without tactile input."""
        z = self.__dict__.get("_zero_feat")
        if z is None or z.shape[0] < rows or z.shape[1] != C or z.device != torch.device(self.device):
            z = self._zero_feat = torch.zeros((rows, C), dtype=torch.float32, device=self.device)
        return z[:rows]

    def generate_hand_mesh(self, data):
        """Hand mesh of one scene (generation.py:74-115): encoder_hand -> MANO vertices, then out of the MANO
        frame (fixed offset and rotation), out of the predicted wrist rotation (rotation vector -> 'XYZ' Euler
        -> the reference's R_from_PYR convention, common.py:591-604), plus the wrist position, normalised by
        the object's ``inputs.pc_ply`` cloud (norm_pc_1, common.py:606-612).  Returns Mesh(vertices [778,3]
        f64, faces [1538,3] i64) on the device (the reference wraps the same arrays in a trimesh.Trimesh)."""
        self._eval_mode()
        inputs = data.get('inputs').to(self.device)
        pc_ply = data.get('inputs.pc_ply').to(self.device)
        if inputs.shape[0] != 1:
            raise VtError(f"generate_hand_mesh: one scene at a time (got a batch of {inputs.shape[0]})")
        c_hand = self._replay("encode_hand_inputs", [inputs], self.model.encode_hand_inputs)   # ~70 launches as one graph
        return self._hand_mesh_of(c_hand, pc_ply)

    def _hand_mesh_of(self, c_hand, pc_ply):
        """generate_hand_mesh's arithmetic on a hand encoder output that is already there (the touch session's VTacOH route runs
        the hand encoder once per touch for the fingertips and the mesh)."""
        import numpy as np
        from scipy.spatial.transform import Rotation
        if not isinstance(c_hand, dict) or 'mano_verts' not in c_hand:
            raise VtError("generate_hand_mesh: the hand encoder has no MANO layer (out_dim <= 30 regresses digit poses only)")
        param = c_hand['mano_param'][0].double().cpu().numpy()

        def pyr(roll, pitch, yaw):                                  # 3x3, host side: nine numbers
            cr, sr, cp, sp, cy, sy = np.cos(roll), np.sin(roll), np.cos(pitch), np.sin(pitch), np.cos(yaw), np.sin(yaw)
            about_z = np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]])
            about_x_t = np.array([[1, 0, 0], [0, cp, sp], [0, -sp, cp]])
            about_y_t = np.array([[cy, 0, -sy], [0, 1, 0], [sy, 0, cy]])
            return about_x_t @ about_y_t @ about_z

        euler = Rotation.from_rotvec(param[3:6]).as_euler('XYZ', degrees=False)
        undo = np.linalg.inv(pyr(*euler)) @ np.linalg.inv(pyr(-np.pi / 2, np.pi / 2, 0.0))
        dev = c_hand['mano_verts'].device
        undo_t = torch.from_numpy(undo).to(dev)
        v = (c_hand['mano_verts'][0] - torch.tensor([0.11, 0.005, 0.0], device=dev)).double()
        v = v @ undo_t.t() + torch.from_numpy(param[:3]).to(dev)
        cloud = pc_ply[0].float()
        centroid = cloud.mean(dim=0)
        m = (cloud - centroid).pow(2).sum(dim=1).sqrt().max()
        v = (v - centroid.double()) / (2.0 * m.double())
        if self.with_normals:                                        # the 778 MANO vertices: normals of the geometry, area-weighted
            from ..utils import mesh_clean
            return NormalMesh(v, c_hand['mano_faces'], vertex_normals=mesh_clean.vertex_normals((v, c_hand['mano_faces'])),
                              normals_source="geometry")
        return Mesh(v, c_hand['mano_faces'])

    def generate_tactile_pc(self, data, fov=60.0):
        """The tactile model's inference output (generation.py:286-333): every pixel of the five predicted depth images of each scene
        as a point of the object's normalised frame.  ``data``: 'inputs.img' [B,5,C,H,W], 'points.cam_pos' / 'points.cam_rot' (the
        sensors' poses, [B,5,3] or [B,15]), 'inputs.pc_ply' [B,T,3], 'points.name'.  Returns (pc_world_l, data_name): a float64 numpy
        array [B, 5, H*W, 3] and the names, as the reference does.  The depth estimator runs on all B * 5 images at once
        (encode_img_inputs); depth = pred * 0.005 + 0.019, the pinhole unprojection, the pose (rotation + [-pi/2, 0, pi/2]) and
        norm_pc_1 run per pixel on the device (vt_depth_cloud); the host prepares the 5 B pose inverses and the clouds' centroid and
        scale (sensor_pose_records).  H and W come from the images (the reference hard-codes 320 x 240).  The reference also calls
        encode_hand_inputs here and uses nothing of its result: that call is not made."""
        from ..common import sensor_pose_records
        if getattr(self.model, 'encoder_img', None) is None:
            raise VtError("generate_tactile_pc: the model needs encoder_img (the tactile depth estimator)")
        self._eval_mode()
        imgs = data.get('inputs.img').to(self.device)
        if imgs.dim() != 5 or imgs.shape[1] != 5:
            raise VtError(f"generate_tactile_pc: inputs.img must be [B, 5, C, H, W] (got {tuple(imgs.shape)})")
        B, Fn, _, H, W = imgs.shape
        cam_pos = data.get('points.cam_pos').detach().cpu().numpy().reshape(B, 5, 3)
        cam_rot = data.get('points.cam_rot').detach().cpu().numpy().reshape(B, 5, 3)
        pc_ply = data.get('inputs.pc_ply').detach().cpu().numpy()
        with torch.no_grad():
            pred = self.model.encode_img_inputs(imgs)
            if pred.shape[0] != B or pred.numel() != B * Fn * H * W:
                raise VtError(f"generate_tactile_pc: the depth estimator must give one value per pixel (got {tuple(pred.shape)}: num_classes 1?)")
            pose = torch.from_numpy(sensor_pose_records(cam_pos, cam_rot, pc_ply)).to(self.device)
            cloud = ops.depth_cloud(pred.reshape(B * Fn, H * W).float(), pose, W, H, fov)
        return cloud.view(B, Fn, H * W, 3).cpu().numpy(), data.get('points.name')

    def generate_obj_mesh_wnf(self, data, c_img_all=None):
        """Encode -> dense decode -> marching cubes for one scene; ``data['inputs']`` is the
        point cloud [1,T,3].  Returns Mesh(vertices [V,3] f32, faces [F,3] i32) on the device -- or, with
        ``reference_returns``, (mesh, emd, cd) as the reference does (see reference_metrics)."""
        mesh = self._clean(self._generate_obj_mesh(data, c_img_all))
        if self.refinement_step > 0:
            mesh = self._refined(mesh, data)
        if not self.reference_returns:
            return mesh
        emd, cd = self.reference_metrics(mesh, data)     # outside the range guard: the metrics are of the scene it kept
        return mesh, emd, cd

    def reference_metrics(self, mesh, data):
        """(emd, cd) of the reference's generate_obj_mesh_wnf (generation.py:274-284): the mesh's vertices shuffled with numpy's
        global generator (np.random.shuffle of their indices draws what the reference's in-place shuffle of the [V,3] array
        draws), the first 2048 kept, then ``chamfer_distance(points_obj, vertices, use_kdtree=False).item()`` and
        ``EarthMoverDistance(points_obj[0], vertices)`` -- both on the device (eval.chamfer_distance_device,
        eval.earth_mover_distance_device).  ``data['points.points_obj']`` [1,T,3] is required.  An empty mesh gives
        (nan, nan), where the reference fails inside scikit-image's marching cubes."""
        import numpy as np
        from ..eval import chamfer_distance_device, earth_mover_distance_device
        points_obj = data.get('points.points_obj')
        if points_obj is None:
            raise VtError("Generator3D(reference_returns=True): data has no 'points.points_obj' to measure the mesh against")
        V = int(mesh.vertices.shape[0])
        if V == 0:
            return float("nan"), float("nan")
        order = np.arange(V)
        np.random.shuffle(order)
        verts = mesh.vertices.index_select(0, torch.from_numpy(order[:2048]).to(mesh.vertices.device)).float().contiguous()
        target = points_obj.to(verts.device).float()
        cd = chamfer_distance_device(target, verts.unsqueeze(0))
        emd = earth_mover_distance_device(target[0].contiguous(), verts)
        return emd, float(cd.item())

    @_range_guarded
    def _generate_obj_mesh(self, data, c_img_all=None):
        """The mesh of generate_obj_mesh_wnf, under the half-precision decodes' range guard."""
        self._eval_mode()
        if self.extraction == "mise":
            return self._generate_mise(data, c_img_all)
        nx = self.resolution0 * 4                       # generation.py:120
        inputs = data.get('inputs').to(self.device)
        if self._point_model():
            self._refuse_point_tactile("generate_obj_mesh_wnf", c_img_all)
        if self.with_img:
            self._refuse_planes("generate_obj_mesh_wnf(with_img)", "the tactile decodes (fc_p_img, finger ids) sample a volume")
        if self.with_img and c_img_all is None:
            return self._generate_tactile(data)
        if (not self.with_img and not self._plane_model() and not self._point_model() and self._graphs_allowed() and inputs.dim() == 3 and inputs.shape[0] == 1
                and self._worth_capturing((tuple(inputs.shape), nx, self.decode_precision))):
            # the visual branch: the same launches replayed as one hipGraph per (cloud shape, lattice) -- 1.1 instead of 1.5 ms
            return self._generate_mesh_graphed(inputs)
        with torch.no_grad():
            c = self.model.encode_inputs(inputs)
            values = self.eval_lattice(c, nx, c_img_all=c_img_all if self.with_img else None)
        return self.extract_mesh(values.reshape(nx, nx, nx))

    def _depth_origin(self):
        import numpy as np
        src = self.depth_origin
        if src is None:
            src = "./data/VTacO_mesh/depth_origin.txt"
        if isinstance(src, str):
            import os
            if not os.path.exists(src):
                raise VtError(f"Generator3D: the VTacO branch needs the sensor's flat depth reading; {src} not found "
                              "(pass depth_origin=<array or path>)")
            src = np.loadtxt(src)
            self.depth_origin = src
        return np.asarray(src.cpu() if torch.is_tensor(src) else src, dtype=np.float64).reshape(-1)

    def _tactile_setup(self, data, sides=None):
        """Finger features, anchors and assignment rule of the configured tactile branch (VTacO t2d or VTacOH).  ``sides``: two HIP
        streams that take the branch's encoders (see _generate_tactile); None: everything on the current stream."""
        return self._setup_vtaco_t2d(data, sides) if self.encode_t2d else self._setup_vtacoh(data, sides)

    def _side_streams(self):
        """Two side streams per generator for the tactile branch's encoders, or None where graphs / overlap are off
        (VTACO_SCENE_OVERLAP=0: the three encoders one after the other on the caller's stream)."""
        if os.environ.get("VTACO_SCENE_OVERLAP", "1") == "0" or not self._graphs_allowed():
            return None
        if getattr(self, "_sides", None) is None:
            # (plain priority: with high-priority side streams the VTacOH route measured 3.59 against 3.71 ms, the t2d route 4.7 against
            # 2.25 -- the shape encoder's convs then wait behind ~60 small launches)
            prio = int(os.environ.get("VTACO_SCENE_SIDE_PRIORITY", "0"))
            self._sides = (torch.cuda.Stream(device=self.device, priority=prio), torch.cuda.Stream(device=self.device, priority=prio))
        return self._sides

    def _generate_tactile(self, data):
        """generate_obj_mesh_tactile with the branch's own setup.  The scene's encoders do not depend on each other -- the shape
        encoder (0.6 ms, the whole chip for its 64^3 convs), the tactile feature encoder (Resnet18 on five images: 1.2-1.3 ms of
        launch-bound kernels on a few CUs) and, in the VTacOH branch, the hand encoder (0.44 ms) -- so their graphs are replayed on
        three HIP streams at once and joined in front of the decode: 2.3 ms of encoders one after the other become the longest one.
        The setup's host side (contact clouds in numpy, the fingertips' frame change) runs under them."""
        nx = self.resolution0 * 4
        c, setup = self._tactile_encode(data)
        with torch.no_grad():
            values = self._eval_lattice_tactile(c, nx, setup)
        return self.extract_mesh(values.reshape(nx, nx, nx))

    def _tactile_encode(self, data):
        """(c, setup) of a tactile scene: the shape encoder's output and the branch's finger features, anchors and rule, with the
        encoders overlapped on the side streams (see _generate_tactile)."""
        self._eval_mode()
        self._refuse_point("generate_obj_mesh_wnf(with_img)", "the PointConv decoder has no tactile variant")
        self._refuse_planes("generate_obj_mesh_wnf(with_img)", "the tactile decodes read the finger features in vt_decode_fwd_ids / "
                            "the fuser's id kernels, which sample a volume")
        inputs = data.get('inputs').to(self.device)
        if inputs.shape[0] != 1:
            raise VtError(f"generate_obj_mesh_wnf: one scene at a time (got a batch of {inputs.shape[0]})")
        sides = self._side_streams()
        if sides is not None:
            cur = torch.cuda.current_stream(self.device)
            for side in sides:                                      # (the side streams see everything queued so far: the inputs' uploads,
                side.wait_stream(cur)                               #  the previous scene's reads of the graphs' static outputs)
            pending = self._tactile_setup(data, sides)              # queues the tactile encoders; returns the host part still to do
            c = self._replay("encode_inputs", [inputs], self.model.encode_inputs)
            setup = pending()
            for side in sides:
                cur.wait_stream(side)
        else:
            c = self._replay("encode_inputs", [inputs], self.model.encode_inputs)
            setup = self._tactile_setup(data)
        return c, setup

    # -- multiresolution isosurface extraction (extraction="mise") --------------------------------------------------------------
    def _refuse_mise(self, what):
        if self.extraction == "mise":
            raise VtError(f"Generator3D.{what}: dense extraction only (this generator has extraction='mise'; use generate_obj_mesh_wnf)")

    def mise_level(self):
        """The iso level of extraction="mise": the logit of ``threshold``, log(t) - log(1-t) in double (0.0 at 0.5)."""
        import math
        t = float(self.threshold)
        return math.log(t) - math.log(1.0 - t)

    def _mise_precision(self):
        """The point path's arithmetic for ``decode_precision``: "f16f8" is lattice-only, its points run as "f16x3"."""
        return "f16x3" if self.decode_precision == "f16f8" else self.decode_precision

    def mise_evaluator(self, c, setup=None):
        """``evaluate(ids, pts) -> logits`` of the scene's decoder at arbitrary points for mise.extract: the point path in
        ``_mise_precision()``; with a tactile ``setup`` every point first gets its finger id (vt_tactile_assign at the points) and
        the decoder reads the finger's feature by id."""
        dec = self.model.decoder
        prec = self._mise_precision()
        if isinstance(c, (tuple, list)):
            # the PointConv baseline: the point form of the sampler (vt_point_sample_fwd), then the MLP on given features
            if setup is not None:
                raise VtError("Generator3D.mise_evaluator: the PointConv decoder has no tactile variant")
            cloud, fea = dec._pair(c)

            def evaluate_cloud(ids, pts):
                p = pts.reshape(1, -1, 3)
                return dec._mlp_given(dec._sample_points(cloud, fea, p), p, precision=prec).reshape(-1)
            return evaluate_cloud
        if isinstance(c, dict) and set(c) != {'grid'}:
            # plane features: the point path of the decoder's sampled route (vt_sample_planes, then the MLP on given features)
            if setup is not None:
                raise VtError("Generator3D.mise_evaluator: plane features with a tactile setup are not built (vt_decode_fwd_ids samples a volume)")
            vol, planes = dec._features_of(c)
            prepared = ops.planes.Prepared()            # the planes are laid out by the first level's call and kept for the others

            def evaluate_planes(ids, pts):
                p = pts.reshape(1, -1, 3)
                return dec._mlp_given(dec._sample(p, vol, planes, prepared=prepared), p, precision=prec).reshape(-1)
            return evaluate_planes
        grid = dec._grid_of(c) if isinstance(c, dict) else c
        if setup is None:
            def evaluate(ids, pts):
                p = pts.reshape(1, -1, 3)
                if dec._wide:
                    return dec._wide_fwd(grid, precision=prec, pts=p).reshape(-1)
                return ops.decode_fwd(grid, dec._blob(precision=prec), pts=p, padding=dec.padding, precision=prec).reshape(-1)
            return evaluate
        dev = self.device
        anchors, success = setup['anchors'].to(dev), setup['success'].to(dev)
        count, feats = setup['count'].to(dev), setup['feats'].to(dev).float().contiguous()

        def evaluate_tactile(ids, pts):
            p = pts.reshape(1, -1, 3)
            fid = ops.tactile_assign(anchors, success, setup['mode'], setup['radius'], pts=p, count=count)
            if dec._wide:
                return dec._wide_fwd(grid, precision=prec, pts=p, finger_ids=fid, finger_feats=feats).reshape(-1)
            return ops.decode_fwd_ids(grid, dec._blob(img=True, precision=prec), fid, feats, pts=p, padding=dec.padding,
                                      precision=prec).reshape(-1)
        return evaluate_tactile

    def _generate_mise(self, data, c_img_all=None):
        """generate_obj_mesh_wnf with extraction="mise": the route's encoders as the dense route runs them, then mise.extract
        instead of the lattice decode, then marching cubes at the threshold's logit in the sampled frame.  The points each level
        decoded are left in ``self.mise_points_per_level``."""
        from .. import mise
        if c_img_all is not None:
            raise VtError("Generator3D(extraction='mise'): c_img_all is indexed by the dense nx^3 lattice; pass the tactile inputs "
                          "instead (the route assigns finger ids at the query points)")
        inputs = data.get('inputs').to(self.device)
        if inputs.shape[0] != 1:
            raise VtError(f"generate_obj_mesh_wnf: one scene at a time (got a batch of {inputs.shape[0]})")
        if self.with_img:
            c, setup = self._tactile_encode(data)
        else:
            with torch.no_grad():
                c = self.model.encode_inputs(inputs)
            setup = None
        box, level = 1 + self.padding, self.mise_level()
        values, _, per_level = mise.extract(self.mise_evaluator(c, setup), self.resolution0, self.upsampling_steps, level, box,
                                            self.device)
        self.mise_points_per_level = per_level
        n = values.shape[0]
        return self._marching_cubes(values, level, ((n - 1) / 2, box / (n - 1)))

    def _setup_vtaco_t2d(self, data, sides=None):
        """The VTacO branch of generate_obj_mesh_wnf (generation.py:202-257): per finger whose touch succeeded, the contact cloud
        unprojected from the sample's depth image (as the reference: the dataset's depth, not the predicted one, and the dataset's
        camera poses), at most 128 points; every lattice point within 0.015 of a contact point takes that finger's tactile feature
        (later fingers overwrite earlier ones) -- by finger id (vt_tactile_assign 'within' + vt_decode_fwd_ids) at any lattice
        size, where the reference builds a dense [1, 128^3, C] tensor with eight CPU cdist passes hard-wired to 128^3."""
        from ..common import contact_clouds_from_depth
        if getattr(self.model, 'encoder_img', None) is None:
            raise VtError("generate_obj_mesh_wnf(with_img, encode_t2d): the model needs encoder_img (tactile features)")
        inputs = data.get('inputs').to(self.device)
        if inputs.shape[0] != 1:
            raise VtError(f"generate_obj_mesh_wnf: one scene at a time (got a batch of {inputs.shape[0]})")
        self._eval_mode()
        # [1,5,C]; the feature encoder (Resnet18 in eval mode: ~60 launch-bound MIOpen / ATen kernels) replayed as a graph
        c_img = self._replay_on(sides[0] if sides else None, "encode_img", [data.get('inputs.img')], self.model.encode_img_inputs)
        # (one scene's five images stay on the host: 0.5 ms of numpy that runs under the shape encoder's replay; the device kernels of
        # the training step -- vt_contact_scan / vt_contact_points, 40 images per step -- need the counts back on the host in between,
        # which would wait for that replay: measured 1.78 against 1.26 ms for this setup)
        def host_part():
            anchors, count = contact_clouds_from_depth(
                data.get('inputs.depth')[0].float().cpu().numpy(), self._depth_origin(),
                data.get('points.cam_pos').reshape(1, 5, 3)[0].cpu().numpy(), data.get('points.cam_rot').reshape(1, 5, 3)[0].cpu().numpy(),
                data.get('inputs.pc_ply')[0].float().cpu().numpy(), data.get('inputs.touch_success')[0].cpu().numpy())
            return {'feats': c_img[0], 'anchors': torch.from_numpy(anchors).float(), 'success': torch.from_numpy((count > 0).astype('uint8')),
                    'mode': 'within', 'radius': 0.015, 'count': torch.from_numpy(count).int()}
        return host_part if sides else host_part()

    def _replay_on(self, stream, kind, tensors, run):
        """A clone of ``_replay(kind, tensors, run)``'s result, queued on ``stream`` (None: the current one).  The clone is marked as
        used by the caller's stream, which reads it behind its ``wait_stream``."""
        if stream is None:
            return self._replay(kind, tensors, run).clone()
        cur = torch.cuda.current_stream(self.device)
        with torch.cuda.stream(stream):
            out = self._replay(kind, tensors, run).clone()
        out.record_stream(cur)
        return out

    def _setup_vtacoh(self, data, sides=None):
        """The VTacOH branch of generate_obj_mesh_wnf (generation.py:161-200): fingertips from the hand encoder's MANO joints
        in the object's frame (ground-truth wrist position and wrist Euler angles from the sample), every lattice point
        within 0.05 of its nearest fingertip takes that finger's tactile feature if its touch succeeded -- by finger id
        (vt_tactile_assign + vt_decode_fwd_ids) instead of the reference's dense [1, nx^3, C] tensor and CPU cdist."""
        from ..common import fingertips_in_object_frame
        if getattr(self.model, 'encoder_hand', None) is None or getattr(self.model, 'encoder_img', None) is None:
            raise VtError("generate_obj_mesh_wnf(with_img): the model needs encoder_hand (fingertips) and encoder_img "
                          "(tactile features), or pass c_img_all / use generate_obj_mesh_tactile")
        inputs = data.get('inputs').to(self.device)
        if inputs.shape[0] != 1:
            raise VtError(f"generate_obj_mesh_wnf: one scene at a time (got a batch of {inputs.shape[0]})")
        self._eval_mode()
        # the tactile features first (the longest of the scene's encoders), then the hand encoder: plane PointNet + 2-D U-Net + MANO as one graph
        c_img = self._replay_on(sides[0] if sides else None, "encode_img", [data.get('inputs.img')], self.model.encode_img_inputs)    # [1,5,C]
        hand_stream = sides[1] if sides else torch.cuda.current_stream(self.device)
        with torch.cuda.stream(hand_stream):
            c_hand = self._replay("encode_hand_inputs", [inputs], self.model.encode_hand_inputs)
            if 'mano_joints' not in c_hand:
                raise VtError("generate_obj_mesh_wnf(with_img): the hand encoder has no MANO layer (out_dim <= 30)")
            joints_dev = c_hand['mano_joints'].float()

        def host_part():
            with torch.cuda.stream(hand_stream):                    # (the copy back waits for the hand encoder's stream only)
                joints = joints_dev.cpu().numpy()
            tips = fingertips_in_object_frame(joints, data.get('points.mano').cpu().numpy()[:, :3],
                                              data.get('points.wrist').cpu().numpy(), data.get('inputs.pc_ply').float().cpu().numpy())
            anchors = torch.from_numpy(tips[0]).float().unsqueeze(1)                               # [5,1,3]
            return {'feats': c_img[0], 'anchors': anchors, 'success': data.get('inputs.touch_success')[0].to(torch.uint8),
                    'mode': 'nearest', 'radius': 0.05, 'count': torch.ones(5, dtype=torch.int32),
                    'c_hand': c_hand}                               # (the graph's static output: valid until the next hand replay)
        return host_part if sides else host_part()
