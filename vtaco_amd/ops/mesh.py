"""Topology of a triangle mesh (vt_mesh_components, vt_mesh_component_table, vt_mesh_component_stats, vt_mesh_edge_stats, vt_mesh_filter:
csrc/mesh_topo.hip), its normals (vt_mesh_normals: csrc/mesh_normals.hip; ``ops.mesh.normals``) and, at the end of the file, its simplification and welding (vt_mesh_cluster, vt_mesh_weld, vt_mesh_cluster_faces,
vt_mesh_cluster_place: csrc/mesh_simplify.hip; vt_mesh_collapse: csrc/mesh_collapse.hip, ``ops.mesh.collapse``), and behind those its hole filling (vt_mesh_boundary, vt_mesh_boundary_loops, vt_mesh_fill_count,
vt_mesh_fill_emit: csrc/mesh_fill.hip; ``ops.mesh.boundary_loops``, ``ops.mesh.fill_holes``), and last its vertex adjacency and smoothing (vt_mesh_adjacency_count, vt_mesh_adjacency_fill, vt_mesh_smooth_weights,
vt_mesh_smooth: csrc/mesh_smooth.hip; ``ops.mesh.vertex_adjacency``, ``ops.mesh.smooth``), and its subdivision (vt_mesh_subdivide_count, vt_mesh_subdivide_emit, vt_mesh_subdivide_midpoints, vt_mesh_subdivide_bwd: csrc/mesh_subdivide.hip; ``ops.mesh.subdivide``, ``ops.mesh.subdivide_backward``); those three families alone take F = 0.  A submodule only: callers write ``ops.mesh.components``, ``ops.mesh.component_table``, ``ops.mesh.component_stats``,
``ops.mesh.edge_stats``, ``ops.mesh.filter_components``.  faces are int32 [F,3] and vertices float32 or float64 [V,3] device tensors, as
``ops.marching_cubes`` returns them; int64 faces are refused, not converted (a conversion would be a torch computation here: the caller
writes ``faces.int()``).  F >= 1.  A face index outside [0, V) is found on the device by the calls that read a count back anyway
(``components``, ``component_table``, ``filter_components``), which raise; no kernel dereferences such an index."""
from collections import namedtuple
import ctypes
import numbers

import torch

from ._base import _lib, VtError, check, dev_ptr, stream_ptr, I32, U8, _c
from ._octree import _ws  # noqa: F401  (ops/refine.py takes it from here)


F64 = torch.float64
ComponentTable = namedtuple("ComponentTable", ["n_components", "comp_of_vertex", "comp_of_face"])
ComponentStats = namedtuple("ComponentStats", ["n_faces", "n_vertices", "bbox", "area", "volume"])
EdgeStats = namedtuple("EdgeStats", ["n_edges", "n_boundary", "n_nonmanifold", "n_misoriented"])
FilteredMesh = namedtuple("FilteredMesh", ["vertices", "faces", "vertex_map"])


def _faces(what, faces, *others):
    if not torch.is_tensor(faces) or any(not torch.is_tensor(t) for t in others):
        raise VtError(f"{what}: expected tensors")
    if not faces.is_cuda or any(t.device != faces.device for t in others):
        raise VtError(f"{what}: every tensor must live on one HIP device (got {', '.join(str(t.device) for t in (faces,) + others)}); "
                      "vtaco_amd has no CPU path")
    if faces.dtype != I32:
        raise VtError(f"{what}: faces must be int32, as ops.marching_cubes returns them (got {faces.dtype}); convert with faces.int()")
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise VtError(f"{what}: faces must be [F,3] (got {tuple(faces.shape)})")
    if faces.shape[0] < 1:
        raise VtError(f"{what}: a mesh without faces has no components (F = 0)")
    return _c(faces)


def _count(what, n, name="V"):
    if int(n) != n or int(n) < 1:
        raise VtError(f"{what}: {name} must be an integer >= 1 (got {n})")
    return int(n)


def _vertices(what, vertices):
    if vertices.dtype not in (torch.float32, F64):
        raise VtError(f"{what}: vertices must be float32 or float64 (got {vertices.dtype})")
    if vertices.dim() != 2 or vertices.shape[1] != 3 or vertices.shape[0] < 1:
        raise VtError(f"{what}: vertices must be [V,3] with V >= 1 (got {tuple(vertices.shape)})")
    return _c(vertices)


def _i32(what, t, n, name):
    if t.dtype != I32 or tuple(t.shape) != (n,):
        raise VtError(f"{what}: {name} must be int32 [{n}] (got {t.dtype} {tuple(t.shape)})")
    return _c(t)


def components(faces, n_vertices, return_rounds=False):
    """labels int32 [V]: the smallest vertex index of each vertex's connected component (vt_mesh_components); an unreferenced vertex
    keeps its own index.  Converged when it returns: the launcher repeats hooking rounds until one changes nothing, reading their flags
    once per two rounds.  ``return_rounds``: (labels, rounds), rounds = the hooking rounds run, the one that changed nothing included."""
    what = "mesh.components"
    faces = _faces(what, faces)
    V, F = _count(what, n_vertices), faces.shape[0]
    labels = torch.empty(V, dtype=I32, device=faces.device)
    lib = _lib.load()
    ws = _ws(lib.vt_mesh_components_workspace_bytes(V, F), faces.device)
    rounds = ctypes.c_int(0)
    check(lib.vt_mesh_components(dev_ptr(faces, "faces", I32), F, V, dev_ptr(labels, "labels", I32), ctypes.byref(rounds),
                                 ctypes.c_void_p(ws.data_ptr()), ws.numel() * 8, stream_ptr()), "vt_mesh_components")
    return (labels, rounds.value) if return_rounds else labels


def component_table(faces, labels):
    """ComponentTable(n_components, comp_of_vertex int32 [V], comp_of_face int32 [F]) from ``components``' labels: components are
    numbered by ascending root index over the roots that own a face; unreferenced vertices get -1 (vt_mesh_component_table)."""
    what = "mesh.component_table"
    faces = _faces(what, faces, labels)
    if labels.dtype != I32 or labels.dim() != 1 or labels.shape[0] < 1:
        raise VtError(f"{what}: labels must be int32 [V] (got {labels.dtype} {tuple(labels.shape)})")
    labels = _c(labels)
    V, F, dev = labels.shape[0], faces.shape[0], faces.device
    cov = torch.empty(V, dtype=I32, device=dev)
    cof = torch.empty(F, dtype=I32, device=dev)
    lib = _lib.load()
    ws = _ws(lib.vt_mesh_component_table_workspace_bytes(V, F), dev)
    n = ctypes.c_int(0)
    check(lib.vt_mesh_component_table(dev_ptr(faces, "faces", I32), F, V, dev_ptr(labels, "labels", I32), dev_ptr(cov, "comp_of_vertex", I32),
                                      dev_ptr(cof, "comp_of_face", I32), ctypes.byref(n), ctypes.c_void_p(ws.data_ptr()), ws.numel() * 8,
                                      stream_ptr()), "vt_mesh_component_table")
    return ComponentTable(n.value, cov, cof)


def component_stats(vertices, faces, table):
    """ComponentStats(n_faces, n_vertices int32 [C], bbox [C,2,3] in the vertices' dtype, area, volume float64 [C]) per component of
    ``table`` (vt_mesh_component_stats); nothing here waits for the device."""
    what = "mesh.component_stats"
    faces = _faces(what, faces, vertices, table.comp_of_vertex, table.comp_of_face)
    vertices = _vertices(what, vertices)
    V, F, C, dev = vertices.shape[0], faces.shape[0], _count(what, table.n_components, "n_components"), faces.device
    cov, cof = _i32(what, table.comp_of_vertex, V, "comp_of_vertex"), _i32(what, table.comp_of_face, F, "comp_of_face")
    nf = torch.empty(C, dtype=I32, device=dev)
    nv = torch.empty(C, dtype=I32, device=dev)
    bbox = torch.empty((C, 2, 3), dtype=vertices.dtype, device=dev)
    area = torch.empty(C, dtype=F64, device=dev)
    volume = torch.empty(C, dtype=F64, device=dev)
    lib = _lib.load()
    ws = _ws(lib.vt_mesh_component_stats_workspace_bytes(C), dev)
    check(lib.vt_mesh_component_stats(dev_ptr(vertices, "vertices", vertices.dtype), int(vertices.dtype == F64), V, dev_ptr(faces, "faces", I32), F,
                                      dev_ptr(cov, "comp_of_vertex", I32), dev_ptr(cof, "comp_of_face", I32), C, dev_ptr(nf, "n_faces", I32),
                                      dev_ptr(nv, "n_vertices", I32), dev_ptr(bbox, "bbox", bbox.dtype), dev_ptr(area, "area", F64),
                                      dev_ptr(volume, "volume", F64), ctypes.c_void_p(ws.data_ptr()), ws.numel() * 8, stream_ptr()),
          "vt_mesh_component_stats")
    return ComponentStats(nf, nv, bbox, area, volume)


def edge_stats(faces, table):
    """EdgeStats(n_edges, n_boundary, n_nonmanifold, n_misoriented), int32 [C] each, over the undirected edges of every component
    (vt_mesh_edge_stats); nothing here waits for the device."""
    what = "mesh.edge_stats"
    faces = _faces(what, faces, table.comp_of_vertex)
    cov = table.comp_of_vertex
    if cov.dtype != I32 or cov.dim() != 1 or cov.shape[0] < 1:
        raise VtError(f"{what}: comp_of_vertex must be int32 [V] (got {cov.dtype} {tuple(cov.shape)})")
    cov = _c(cov)
    V, F, C, dev = cov.shape[0], faces.shape[0], _count(what, table.n_components, "n_components"), faces.device
    outs = [torch.empty(C, dtype=I32, device=dev) for _ in range(4)]
    lib = _lib.load()
    ws = _ws(lib.vt_mesh_edge_stats_workspace_bytes(F), dev)
    check(lib.vt_mesh_edge_stats(dev_ptr(faces, "faces", I32), F, V, dev_ptr(cov, "comp_of_vertex", I32), C, *[dev_ptr(t, "counts", I32) for t in outs],
                                 ctypes.c_void_p(ws.data_ptr()), ws.numel() * 8, stream_ptr()), "vt_mesh_edge_stats")
    return EdgeStats(*outs)


def filter_components(vertices, faces, table, keep):
    """FilteredMesh(vertices, faces, vertex_map int32 [V]): the components with ``keep`` (uint8 or bool [C]) set -- their faces in the
    original order, re-indexed, and the vertices those reference in the original order (vt_mesh_filter).  The outputs are slices of
    capacity (V, F) buffers, cut after one read of the two counts; keeping nothing gives V = 0 and F = 0."""
    what = "mesh.filter_components"
    faces = _faces(what, faces, vertices, table.comp_of_vertex, table.comp_of_face, keep)
    vertices = _vertices(what, vertices)
    V, F, C, dev = vertices.shape[0], faces.shape[0], _count(what, table.n_components, "n_components"), faces.device
    cov, cof = _i32(what, table.comp_of_vertex, V, "comp_of_vertex"), _i32(what, table.comp_of_face, F, "comp_of_face")
    if keep.dtype not in (U8, torch.bool) or tuple(keep.shape) != (C,):
        raise VtError(f"{what}: keep must be uint8 or bool [{C}] (got {keep.dtype} {tuple(keep.shape)})")
    keep = _c(keep.view(U8) if keep.dtype == torch.bool else keep)
    out_v = torch.empty((V, 3), dtype=vertices.dtype, device=dev)
    out_f = torch.empty((F, 3), dtype=I32, device=dev)
    vmap = torch.empty(V, dtype=I32, device=dev)
    lib = _lib.load()
    ws = _ws(lib.vt_mesh_filter_workspace_bytes(V, F), dev)
    nv, nf = ctypes.c_int(0), ctypes.c_int(0)
    check(lib.vt_mesh_filter(dev_ptr(vertices, "vertices", vertices.dtype), int(vertices.dtype == F64), V, dev_ptr(faces, "faces", I32), F,
                             dev_ptr(cov, "comp_of_vertex", I32), dev_ptr(cof, "comp_of_face", I32), dev_ptr(keep, "keep", U8), C,
                             dev_ptr(out_v, "out_vertices", out_v.dtype), dev_ptr(out_f, "out_faces", I32), dev_ptr(vmap, "vertex_map", I32),
                             ctypes.byref(nv), ctypes.byref(nf), ctypes.c_void_p(ws.data_ptr()), ws.numel() * 8, stream_ptr()), "vt_mesh_filter")
    return FilteredMesh(out_v[:nv.value], out_f[:nf.value], vmap)


# ---- normals (csrc/mesh_normals.hip) ---------------------------------------------------------------------------------------------------
WEIGHTS = ("area", "angle")
MeshNormals = namedtuple("MeshNormals", ["face_normals", "vertex_normals"])


def normals(vertices, faces, weight="area", face=True, vertex=True):
    """MeshNormals(face_normals [F,3], vertex_normals [V,3]) in the vertices' dtype (vt_mesh_normals); ``face`` / ``vertex`` False leaves
    that one None and its work undone.  Face normals are unit, (0,0,0) for a degenerate face.  A vertex normal is the normalised sum over
    the vertex's live faces of the raw cross product (``weight='area'``) or of the unit normal times the corner's angle (``'angle'``);
    (0,0,0) for a vertex that no live face references.  The sums are exact: equal bits from run to run and under any order of the faces.
    One host read (the status word: a face index outside [0, V) raises)."""
    what = "mesh.normals"
    if weight not in WEIGHTS:
        raise VtError(f"{what}: weight must be one of {WEIGHTS} (got {weight!r})")
    if not face and not vertex:
        raise VtError(f"{what}: nothing asked for (face=False, vertex=False)")
    faces = _faces(what, faces, vertices)
    vertices = _vertices(what, vertices)
    V, F, dev = vertices.shape[0], faces.shape[0], faces.device
    fn = torch.empty((F, 3), dtype=vertices.dtype, device=dev) if face else None
    vn = torch.empty((V, 3), dtype=vertices.dtype, device=dev) if vertex else None
    lib = _lib.load()
    ws = _ws(lib.vt_mesh_normals_workspace_bytes(V, F), dev)
    check(lib.vt_mesh_normals(dev_ptr(vertices, "vertices", vertices.dtype), int(vertices.dtype == F64), V, dev_ptr(faces, "faces", I32), F,
                              WEIGHTS.index(weight), dev_ptr(fn, "face_normals", vertices.dtype), dev_ptr(vn, "vertex_normals", vertices.dtype),
                              ctypes.c_void_p(ws.data_ptr()), ws.numel() * 8, stream_ptr()), "vt_mesh_normals")
    return MeshNormals(fn, vn)


# ---- simplification and welding (csrc/mesh_simplify.hip) ---------------------------------------------------------------------------------
# ``cluster`` / ``weld`` make the vertex map, ``cluster_faces`` the faces on it (the one call that waits for the device),
# ``cluster_place`` the vertices.  The calls of one simplification share a ``state`` tensor (int32 [32]: the bounding box as it stays on
# the device, the status bits, K, the face count, the fallbacks); utils/mesh_clean.py strings them together.
Clusters = namedtuple("Clusters", ["cluster_of_vertex", "cluster_rep", "state", "resolution"])
ClusterFaces = namedtuple("ClusterFaces", ["n_clusters", "n_faces", "faces"])
MAX_RESOLUTION = 1 << 20
MAX_CLUSTERS = 1 << 21
PLACEMENTS = ("quadric", "mean", "representative")
STATE_BAD, STATE_K, STATE_NF, STATE_FALLBACKS = 16, 17, 18, 19


def _cluster_call(what, fn_name, vertices, faces, arg):
    faces = _faces(what, faces, vertices)
    vertices = _vertices(what, vertices)
    V, F, dev = vertices.shape[0], faces.shape[0], faces.device
    cov = torch.empty(V, dtype=I32, device=dev)
    rep = torch.empty(V, dtype=I32, device=dev)
    state = torch.empty(32, dtype=I32, device=dev)
    lib = _lib.load()
    ws = _ws(getattr(lib, fn_name + "_workspace_bytes")(V, F), dev)
    check(getattr(lib, fn_name)(dev_ptr(vertices, "vertices", vertices.dtype), int(vertices.dtype == F64), V, dev_ptr(faces, "faces", I32), F, arg,
                                dev_ptr(cov, "cluster_of_vertex", I32), dev_ptr(rep, "cluster_rep", I32), dev_ptr(state, "state", I32),
                                ctypes.c_void_p(ws.data_ptr()), ws.numel() * 8, stream_ptr()), fn_name)
    return cov, rep, state


def cluster(vertices, faces, resolution):
    """Clusters(cluster_of_vertex int32 [V], cluster_rep int32 [V] of which the first K count, state, resolution): the referenced vertices
    grouped by their cell of a grid with ``resolution`` cells along the longest side of their bounding box (vt_mesh_cluster).  Nothing
    here waits for the device: K, and the status bit of a face index outside [0, V) or of a non-finite vertex, are words 17 and 16 of
    ``state``; ``cluster_faces`` reads them."""
    what = "mesh.cluster"
    if isinstance(resolution, bool) or int(resolution) != resolution or not 1 <= int(resolution) <= MAX_RESOLUTION:
        raise VtError(f"{what}: resolution must be an integer in [1, {MAX_RESOLUTION}] (got {resolution!r})")
    cov, rep, state = _cluster_call(what, "vt_mesh_cluster", vertices, faces, int(resolution))
    return Clusters(cov, rep, state, int(resolution))


def weld(vertices, faces, tol=0.0):
    """Clusters of equal vertices (vt_mesh_weld): ``tol`` 0 equal coordinates (-0.0 equals +0.0; a vertex with a NaN merges with
    nothing), ``tol`` > 0 equal rint(x / tol) per axis.  Asynchronous like ``cluster``."""
    what = "mesh.weld"
    tol = float(tol)
    if not 0.0 <= tol < float("inf"):
        raise VtError(f"{what}: tol must be finite and >= 0 (got {tol})")
    cov, rep, state = _cluster_call(what, "vt_mesh_weld", vertices, faces, tol)
    return Clusters(cov, rep, state, 1)


def cluster_faces(faces, clusters, unique=True, count_only=False):
    """ClusterFaces(n_clusters, n_faces, faces int32 [n_faces,3] or None with ``count_only``): the faces on cluster ids without those
    that collapsed and, with ``unique``, without later copies of an unordered triple, in the original order (vt_mesh_cluster_faces).
    One read of ``state``; its status bits raise here."""
    what = "mesh.cluster_faces"
    cov, state = clusters.cluster_of_vertex, clusters.state
    faces = _faces(what, faces, cov, state)
    V, F, dev = cov.shape[0], faces.shape[0], faces.device
    cov = _i32(what, cov, V, "cluster_of_vertex")
    state = _i32(what, state, 32, "state")
    out = None if count_only else torch.empty((F, 3), dtype=I32, device=dev)
    lib = _lib.load()
    ws = _ws(lib.vt_mesh_cluster_faces_workspace_bytes(F), dev)
    nk, nf = ctypes.c_int(0), ctypes.c_int(0)
    check(lib.vt_mesh_cluster_faces(dev_ptr(faces, "faces", I32), F, V, dev_ptr(cov, "cluster_of_vertex", I32), int(bool(unique)),
                                    dev_ptr(out, "out_faces", I32), dev_ptr(state, "state", I32), ctypes.byref(nk), ctypes.byref(nf),
                                    ctypes.c_void_p(ws.data_ptr()), ws.numel() * 8, stream_ptr()), "vt_mesh_cluster_faces")
    return ClusterFaces(nk.value, nf.value, None if count_only else out[:nf.value])


def cluster_place(vertices, faces, clusters, n_clusters, placement="quadric"):
    """vertices [K,3] of the clusters, in the input's dtype (vt_mesh_cluster_place): ``'quadric'`` the minimiser of the summed quadric
    about the cluster's mean, the mean itself where that leaves the cell (counted in word 19 of ``state``); ``'mean'``;
    ``'representative'`` the representative's own coordinates.  Nothing here waits for the device."""
    what = "mesh.cluster_place"
    if placement not in PLACEMENTS:
        raise VtError(f"{what}: placement must be one of {PLACEMENTS} (got {placement!r})")
    cov, rep, state = clusters.cluster_of_vertex, clusters.cluster_rep, clusters.state
    faces = _faces(what, faces, vertices, cov, rep, state)
    vertices = _vertices(what, vertices)
    V, F, dev = vertices.shape[0], faces.shape[0], faces.device
    K = _count(what, n_clusters, "n_clusters")
    if K > V:
        raise VtError(f"{what}: n_clusters must be at most V (got {K} > {V})")
    cov, rep, state = _i32(what, cov, V, "cluster_of_vertex"), _i32(what, rep, V, "cluster_rep"), _i32(what, state, 32, "state")
    out = torch.empty((K, 3), dtype=vertices.dtype, device=dev)
    lib = _lib.load()
    ws = _ws(lib.vt_mesh_cluster_place_workspace_bytes(K), dev)
    check(lib.vt_mesh_cluster_place(dev_ptr(vertices, "vertices", vertices.dtype), int(vertices.dtype == F64), V, dev_ptr(faces, "faces", I32), F,
                                    clusters.resolution, dev_ptr(cov, "cluster_of_vertex", I32), dev_ptr(rep, "cluster_rep", I32), K,
                                    PLACEMENTS.index(placement), dev_ptr(out, "out_vertices", out.dtype), dev_ptr(state, "state", I32),
                                    ctypes.c_void_p(ws.data_ptr()), ws.numel() * 8, stream_ptr()), "vt_mesh_cluster_place")
    return out


# ---- decimation by edge collapse (csrc/mesh_collapse.hip; tests/mesh_collapse_ref.py is the definition) ----------------------------------
Collapsed = namedtuple("Collapsed", ["vertices", "faces", "vertex_map", "rounds", "stalled"])
COLLAPSE_PLACEMENTS = ("optimal", "midpoint")
MAX_COLLAPSE_FACES = (2 ** 31 - 1) // 6


def collapse(vertices, faces, nfaces, placement="optimal", max_rounds=None):
    """Collapsed(vertices, faces, vertex_map int32 [V], rounds, stalled): the mesh decimated to at most ``nfaces`` faces by rounds of
    independent quadric edge collapses (vt_mesh_collapse).  An edge may collapse when neither end touches a boundary or non-manifold
    edge, its ends share exactly two neighbours (and the link is no tetrahedron) and no face around it flips, so a closed manifold stays
    one, with its Euler number, and lands on the largest even count <= ``nfaces``; ``stalled`` tells that a round found nothing left
    to collapse above that.  ``'optimal'`` puts the merged vertex at the minimiser of the summed quadrics (the midpoint where that is
    not finite or not better), ``'midpoint'`` at the midpoint.  ``max_rounds`` bounds the rounds that collapse something (None: no
    bound); ``rounds`` is their number.  ``vertex_map[v]`` is the output vertex that input vertex v went into, -1 for a vertex no face
    references.  Deterministic, bit for bit.  One host read per four rounds and two more; a mesh that has at most ``nfaces`` faces
    comes back as the same tensors with nothing launched (vertex_map None).  ``vertices`` and ``faces`` are slices of capacity
    (V, F) buffers where the result has more than half the input's rows, copies otherwise; ``vertex_map`` is [V] by its meaning."""
    what = "mesh.collapse"
    if placement not in COLLAPSE_PLACEMENTS:
        raise VtError(f"{what}: placement must be one of {COLLAPSE_PLACEMENTS} (got {placement!r})")
    if isinstance(nfaces, bool) or not isinstance(nfaces, numbers.Integral) or nfaces < 1:
        raise VtError(f"{what}: nfaces must be a positive integer (got {nfaces!r})")
    if max_rounds is not None and (isinstance(max_rounds, bool) or not isinstance(max_rounds, numbers.Integral) or not 1 <= max_rounds < 2 ** 31):
        raise VtError(f"{what}: max_rounds must be None or an integer in [1, 2^31) (got {max_rounds!r})")
    given = (vertices, faces)
    faces = _faces(what, faces, vertices)
    vertices = _vertices(what, vertices)
    V, F, dev = vertices.shape[0], faces.shape[0], faces.device
    if F <= nfaces:
        return Collapsed(*given, None, 0, False)
    if F > MAX_COLLAPSE_FACES:
        raise VtError(f"{what}: F = {F} is above {MAX_COLLAPSE_FACES} = (2^31 - 1) / 6")
    out_v = torch.empty((V, 3), dtype=vertices.dtype, device=dev)
    out_f = torch.empty((F, 3), dtype=I32, device=dev)
    vmap = torch.empty(V, dtype=I32, device=dev)
    lib = _lib.load()
    ws = _ws(lib.vt_mesh_collapse_workspace_bytes(V, F), dev)
    nv, nf, rounds, stalled = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    check(lib.vt_mesh_collapse(dev_ptr(vertices, "vertices", vertices.dtype), int(vertices.dtype == F64), V, dev_ptr(faces, "faces", I32), F,
                               int(nfaces), COLLAPSE_PLACEMENTS.index(placement), 2 ** 31 - 1 if max_rounds is None else int(max_rounds),
                               dev_ptr(out_v, "out_vertices", out_v.dtype), dev_ptr(out_f, "out_faces", I32), dev_ptr(vmap, "vertex_map", I32),
                               ctypes.byref(nv), ctypes.byref(nf), ctypes.byref(rounds), ctypes.byref(stalled), ctypes.c_void_p(ws.data_ptr()),
                               ws.numel() * 8, stream_ptr()), "vt_mesh_collapse")
    # the kernel needs capacity (V, F); a result of at most half of that is copied out, so it does not keep the large buffers alive
    vertices, faces = out_v[:nv.value], out_f[:nf.value]
    return Collapsed(vertices.clone() if 2 * nv.value <= V else vertices, faces.clone() if 2 * nf.value <= F else faces, vmap, rounds.value,
                     bool(stalled.value))


# ---- hole filling (csrc/mesh_fill.hip; tests/mesh_fill_ref.py is the definition) ----------------------------------------------------------
# Half-edge h = 3 f + k runs from faces[f, k] to faces[f, (k+1) % 3]; it is a boundary half-edge when no other half-edge uses its
# undirected edge.  A loop is a cycle of "the one boundary half-edge that leaves my head", numbered by its smallest half-edge and
# starting there; boundary half-edges on no cycle (a vertex shared by two holes, a hole beside a flipped face) are irregular.
BoundaryLoops = namedtuple("BoundaryLoops", ["offsets", "vertices", "half_edges", "n_boundary", "n_irregular"])
FillResult = namedtuple("FillResult", ["vertices", "faces", "n_loops", "n_filled", "n_new_faces", "n_new_vertices", "n_irregular"])
FILL_METHODS = ("fan", "centroid")


def _fill_faces(what, faces, *others):
    """``_faces`` that lets F = 0 through."""
    if torch.is_tensor(faces) and faces.is_cuda and faces.dtype == I32 and tuple(faces.shape) == (0, 3) and all(
            torch.is_tensor(t) and t.device == faces.device for t in others):
        return faces
    return _faces(what, faces, *others)


def boundary_loops(faces, n_vertices):
    """BoundaryLoops(offsets int32 [L+1], vertices, half_edges int32 [n_boundary - n_irregular], n_boundary, n_irregular): loop l owns
    [offsets[l], offsets[l+1]); its element p is the p-th half-edge after the loop's smallest one and that half-edge's tail vertex
    (vt_mesh_boundary, vt_mesh_boundary_loops).  Two host reads (n_boundary; L with n_irregular), one for a closed mesh; F = 0 launches
    nothing.  A face index outside [0, V) raises."""
    what = "mesh.boundary_loops"
    faces = _fill_faces(what, faces)
    V, F, dev = _count(what, n_vertices), faces.shape[0], faces.device
    none = lambda n: torch.zeros(n, dtype=I32, device=dev)
    if F == 0:
        return BoundaryLoops(none(1), none(0), none(0), 0, 0)
    lib = _lib.load()
    ws = _ws(lib.vt_mesh_boundary_workspace_bytes(V, F), dev)
    nb = ctypes.c_int(0)
    check(lib.vt_mesh_boundary(dev_ptr(faces, "faces", I32), F, V, ctypes.byref(nb), ctypes.c_void_p(ws.data_ptr()), ws.numel() * 8, stream_ptr()),
          "vt_mesh_boundary")
    NB = nb.value
    if NB == 0:
        return BoundaryLoops(none(1), none(0), none(0), 0, 0)
    off = torch.empty(NB + 1, dtype=I32, device=dev)
    lv = torch.empty(NB, dtype=I32, device=dev)
    lh = torch.empty(NB, dtype=I32, device=dev)
    nl, ni = ctypes.c_int(0), ctypes.c_int(0)
    check(lib.vt_mesh_boundary_loops(dev_ptr(faces, "faces", I32), F, V, NB, dev_ptr(off, "loop_offsets", I32), dev_ptr(lv, "loop_vertices", I32),
                                     dev_ptr(lh, "loop_half_edges", I32), ctypes.byref(nl), ctypes.byref(ni), ctypes.c_void_p(ws.data_ptr()),
                                     ws.numel() * 8, stream_ptr()), "vt_mesh_boundary_loops")
    n = NB - ni.value
    return BoundaryLoops(off[:nl.value + 1], lv[:n], lh[:n], NB, ni.value)


def fill_holes(vertices, faces, method="fan", max_edges=None, loops=None):
    """FillResult(vertices, faces, n_loops, n_filled, n_new_faces, n_new_vertices, n_irregular): every loop of 3 <= n <= ``max_edges``
    edges (None: every loop) capped against the direction of its boundary (vt_mesh_fill_count, vt_mesh_fill_emit).  ``'fan'``: faces
    (v_0, v_{i+1}, v_i), i = 1 .. n-2, no new vertex.  ``'centroid'``: for n >= 4 one new vertex, the loop's mean (an exact sum divided
    by n in float64, rounded to the vertices' dtype) and faces (c, v_{i+1}, v_i), i = 0 .. n-1; a triangle gets the fan's one face.  New
    faces follow the originals by (loop, i), new vertices by loop.  A planar loop is capped exactly (the fan of a concave outline folds
    over itself, with the right signed area); a curved hole gets a crude cap.  ``loops``: ``boundary_loops`` of these faces, when the
    caller has them.  One more host read (the totals); when nothing is filled the input tensors themselves come back."""
    what = "mesh.fill_holes"
    if method not in FILL_METHODS:
        raise VtError(f"{what}: method must be one of {FILL_METHODS} (got {method!r})")
    if max_edges is not None and (isinstance(max_edges, bool) or int(max_edges) != max_edges or int(max_edges) < 3):
        raise VtError(f"{what}: max_edges must be None or an integer >= 3 (got {max_edges!r})")
    faces = _fill_faces(what, faces, vertices)
    vertices = _vertices(what, vertices)
    V, F, dev = vertices.shape[0], faces.shape[0], faces.device
    if loops is None:
        loops = boundary_loops(faces, V)
    L = loops.offsets.shape[0] - 1
    if L == 0:
        return FillResult(vertices, faces, 0, 0, 0, 0, loops.n_irregular)
    off = _i32(what, loops.offsets, L + 1, "loops.offsets")
    lv = _i32(what, loops.vertices, loops.vertices.shape[0], "loops.vertices")
    if off.device != dev or lv.device != dev:
        raise VtError(f"{what}: loops must live on the faces' device")
    lib = _lib.load()
    ws = _ws(lib.vt_mesh_fill_workspace_bytes(L), dev)
    m = FILL_METHODS.index(method)
    nfl, nf, nv = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    check(lib.vt_mesh_fill_count(dev_ptr(off, "loops.offsets", I32), L, m, 0 if max_edges is None else int(max_edges), ctypes.byref(nfl),
                                 ctypes.byref(nf), ctypes.byref(nv), ctypes.c_void_p(ws.data_ptr()), ws.numel() * 8, stream_ptr()), "vt_mesh_fill_count")
    if nf.value == 0:
        return FillResult(vertices, faces, L, 0, 0, 0, loops.n_irregular)
    out_v = torch.empty((V + nv.value, 3), dtype=vertices.dtype, device=dev)
    out_f = torch.empty((F + nf.value, 3), dtype=I32, device=dev)
    check(lib.vt_mesh_fill_emit(dev_ptr(vertices, "vertices", vertices.dtype), int(vertices.dtype == F64), V, dev_ptr(faces, "faces", I32), F,
                                dev_ptr(off, "loops.offsets", I32), dev_ptr(lv, "loops.vertices", I32), L, m, nf.value, nv.value,
                                dev_ptr(out_v, "out_vertices", out_v.dtype), dev_ptr(out_f, "out_faces", I32), ctypes.c_void_p(ws.data_ptr()),
                                ws.numel() * 8, stream_ptr()), "vt_mesh_fill_emit")
    return FillResult(out_v, out_f, L, nfl.value, nf.value, nv.value, loops.n_irregular)


# ---- vertex adjacency and smoothing (csrc/mesh_smooth.hip; tests/mesh_smooth_ref.py is the definition) ------------------------------------
# The undirected edges {a, b}, a != b, each once however many faces share it, as CSR rows: row i owns [offsets[i], offsets[i+1]) of
# ``neighbors``, ascending.  boundary_edge marks the entries whose edge has exactly one face, boundary_vertex the vertices such an edge
# ends at.  The filters carry positions in float64 over all passes, sum every row in ascending neighbour order and round once.
MeshAdjacency = namedtuple("MeshAdjacency", ["offsets", "neighbors", "boundary_edge", "boundary_vertex"])
SMOOTH_METHODS = ("laplacian", "taubin", "humphrey")
SMOOTH_WEIGHTS = ("uniform", "inverse_distance")
SMOOTH_BOUNDARIES = ("pin", "free", "loop")
SMOOTH_FORMS = (None, "launches", "workgroup")
SMOOTH_WORKGROUP_MAX_V = 2048
MAX_ADJACENCY_FACES = (2 ** 31 - 1) // 6


def vertex_adjacency(faces, n_vertices):
    """MeshAdjacency(offsets int32 [V+1], neighbors int32 [nnz], boundary_edge uint8 [nnz], boundary_vertex uint8 [V])
    (vt_mesh_adjacency_count, vt_mesh_adjacency_fill): what ``trimesh.Trimesh.vertex_neighbors`` holds, as rows.  A face with a repeated
    index contributes its proper edges only; an unreferenced vertex has an empty row.  One host read (nnz, to size ``neighbors``); F = 0
    launches nothing.  A face index outside [0, V) raises, and so does F > (2^31 - 1) / 6: nnz <= 6 F has to fit the int32 offsets."""
    what = "mesh.vertex_adjacency"
    faces = _fill_faces(what, faces)
    V, F, dev = _count(what, n_vertices), faces.shape[0], faces.device
    if F > MAX_ADJACENCY_FACES:
        raise VtError(f"{what}: F = {F} is above {MAX_ADJACENCY_FACES} = (2^31 - 1) / 6: the int32 offsets could not hold nnz <= 6 F")
    off = torch.zeros(V + 1, dtype=I32, device=dev) if F == 0 else torch.empty(V + 1, dtype=I32, device=dev)
    empty = lambda: MeshAdjacency(off, torch.zeros(0, dtype=I32, device=dev), torch.zeros(0, dtype=U8, device=dev),
                                  torch.zeros(V, dtype=U8, device=dev))
    if F == 0:
        return empty()
    lib = _lib.load()
    ws = _ws(lib.vt_mesh_adjacency_workspace_bytes(V, F), dev)
    nnz = ctypes.c_int(0)
    check(lib.vt_mesh_adjacency_count(dev_ptr(faces, "faces", I32), F, V, dev_ptr(off, "offsets", I32), ctypes.byref(nnz),
                                      ctypes.c_void_p(ws.data_ptr()), ws.numel() * 8, stream_ptr()), "vt_mesh_adjacency_count")
    if nnz.value == 0:                                                        # (every face has a repeated index)
        return empty()
    nb = torch.empty(nnz.value, dtype=I32, device=dev)
    be = torch.empty(nnz.value, dtype=U8, device=dev)
    bv = torch.empty(V, dtype=U8, device=dev)
    check(lib.vt_mesh_adjacency_fill(F, V, nnz.value, dev_ptr(nb, "neighbors", I32), dev_ptr(be, "boundary_edge", U8),
                                     dev_ptr(bv, "boundary_vertex", U8), ctypes.c_void_p(ws.data_ptr()), ws.numel() * 8, stream_ptr()),
          "vt_mesh_adjacency_fill")
    return MeshAdjacency(off, nb, be, bv)


def _adjacency(what, adjacency, V, dev):
    if not isinstance(adjacency, MeshAdjacency):
        raise VtError(f"{what}: adjacency must be the MeshAdjacency that ops.mesh.vertex_adjacency returns (got {type(adjacency).__name__})")
    if any(not torch.is_tensor(t) or t.device != dev for t in adjacency):
        raise VtError(f"{what}: the adjacency must live on the vertices' device")
    off = _i32(what, adjacency.offsets, V + 1, "adjacency.offsets")
    nnz = adjacency.neighbors.shape[0] if adjacency.neighbors.dim() == 1 else -1
    nb = _i32(what, adjacency.neighbors, nnz, "adjacency.neighbors")
    be, bv = adjacency.boundary_edge, adjacency.boundary_vertex
    if be.dtype != U8 or tuple(be.shape) != (nnz,) or bv.dtype != U8 or tuple(bv.shape) != (V,):
        raise VtError(f"{what}: adjacency.boundary_edge must be uint8 [{nnz}] and adjacency.boundary_vertex uint8 [{V}] "
                      f"(got {be.dtype} {tuple(be.shape)}, {bv.dtype} {tuple(bv.shape)})")
    return off, nb, _c(be), _c(bv), nnz


def smooth_weights(vertices, adjacency, weights="inverse_distance"):
    """w float64 [nnz], one weight per entry of ``adjacency.neighbors`` (vt_mesh_smooth_weights): ``'uniform'`` 1, ``'inverse_distance'``
    1 / |x_j - x_i| of these positions in float64, 0 for a coincident neighbour.  Nothing here waits for the device."""
    what = "mesh.smooth_weights"
    if weights not in SMOOTH_WEIGHTS:
        raise VtError(f"{what}: weights must be one of {SMOOTH_WEIGHTS} (got {weights!r})")
    if not torch.is_tensor(vertices) or not vertices.is_cuda:
        raise VtError(f"{what}: vertices must be a tensor on a HIP device; vtaco_amd has no CPU path")
    vertices = _vertices(what, vertices)
    V, dev = vertices.shape[0], vertices.device
    off, nb, _, _, nnz = _adjacency(what, adjacency, V, dev)
    w = torch.empty(nnz, dtype=F64, device=dev)
    if nnz:
        check(_lib.load().vt_mesh_smooth_weights(dev_ptr(vertices, "vertices", vertices.dtype), int(vertices.dtype == F64), V, dev_ptr(off, "offsets", I32),
                                                 dev_ptr(nb, "neighbors", I32), nnz, SMOOTH_WEIGHTS.index(weights), dev_ptr(w, "w", F64), stream_ptr()),
              "vt_mesh_smooth_weights")
    return w


def _coefficient(what, name, x):
    if isinstance(x, bool) or not isinstance(x, numbers.Real) or x != x or x in (float("inf"), float("-inf")):
        raise VtError(f"{what}: {name} must be a finite number (got {x!r})")
    return float(x)


def smooth_arguments(what, method, iterations, lam, mu, alpha, beta, weights, boundary):
    """The checked (method, iterations, lam, mu, alpha, beta, weights, boundary) of a smoothing call; raises VtError before any launch."""
    if method not in SMOOTH_METHODS:
        raise VtError(f"{what}: method must be one of {SMOOTH_METHODS} (got {method!r})")
    if weights not in SMOOTH_WEIGHTS:
        raise VtError(f"{what}: weights must be one of {SMOOTH_WEIGHTS} (got {weights!r})")
    if boundary not in SMOOTH_BOUNDARIES:
        raise VtError(f"{what}: boundary must be one of {SMOOTH_BOUNDARIES} (got {boundary!r})")
    if isinstance(iterations, bool) or not isinstance(iterations, numbers.Integral) or not 0 <= int(iterations) <= 1 << 20:
        raise VtError(f"{what}: iterations must be an integer in [0, {1 << 20}] (got {iterations!r})")
    lam, mu = _coefficient(what, "lam", lam), _coefficient(what, "mu", mu)
    alpha, beta = _coefficient(what, "alpha", alpha), _coefficient(what, "beta", beta)
    if method in ("laplacian", "taubin") and not 0.0 < lam <= 1.0:
        raise VtError(f"{what}: lam must lie in (0, 1] (got {lam})")
    if method == "taubin" and not mu < -lam:
        raise VtError(f"{what}: taubin needs mu < -lam < 0 (got lam={lam}, mu={mu}); the defaults are 0.5 and -0.53")
    if method == "humphrey" and not (0.0 <= alpha <= 1.0 and 0.0 <= beta <= 1.0):
        raise VtError(f"{what}: humphrey needs alpha and beta in [0, 1] (got alpha={alpha}, beta={beta})")
    return method, int(iterations), lam, mu, alpha, beta, weights, boundary


def smooth(vertices, adjacency, method="taubin", iterations=10, lam=0.5, mu=-0.53, alpha=0.1, beta=0.5, weights="uniform", boundary="pin",
           form=None):
    """New vertices [V,3] in the input's dtype (vt_mesh_smooth_weights, vt_mesh_smooth).  With m_i the weighted mean of vertex i's
    neighbours: ``'laplacian'`` x <- x + lam (m - x), ``iterations`` passes; ``'taubin'`` ``iterations`` pairs of passes, lam then mu
    (mu < -lam < 0: the second pass undoes the first one's shrinkage); ``'humphrey'`` per iteration q <- x, x <- m(q),
    b <- x - (alpha o + (1 - alpha) q) with o the input, x <- x - (beta b + (1 - beta) m(b)).  ``weights='inverse_distance'`` weighs a
    neighbour by 1 / distance in the input positions (computed once; a coincident neighbour weighs 0).  ``boundary='pin'`` keeps the
    vertices on boundary edges where they are, ``'free'`` treats them like the rest, ``'loop'`` averages them over their boundary
    neighbours only, so a planar cut stays in its plane.  Positions are carried in float64 and rounded once; rows are summed in
    ascending neighbour order, so the bits depend on the mesh's edges alone, not on the order or orientation of its faces.  A vertex
    without neighbours keeps its bits; ``iterations=0`` copies the input.  Every pass is enqueued at once; nothing waits for the device.
    ``form``: ``'launches'`` one launch per pass; ``'workgroup'`` every pass in one launch of one workgroup with the positions in LDS (at
    most 2 048 vertices); None that where it fits, launches elsewhere.  The two return equal bits."""
    what = "mesh.smooth"
    method, iterations, lam, mu, alpha, beta, weights, boundary = smooth_arguments(what, method, iterations, lam, mu, alpha, beta, weights, boundary)
    if form not in SMOOTH_FORMS:
        raise VtError(f"{what}: form must be one of {SMOOTH_FORMS} (got {form!r})")
    if not torch.is_tensor(vertices) or not vertices.is_cuda:
        raise VtError(f"{what}: vertices must be a tensor on a HIP device; vtaco_amd has no CPU path")
    vertices = _vertices(what, vertices)
    V, dev = vertices.shape[0], vertices.device
    off, nb, be, bv, nnz = _adjacency(what, adjacency, V, dev)
    out = torch.empty_like(vertices)
    lib = _lib.load()
    moving = iterations > 0 and nnz > 0
    launches = moving and (form == "launches" or (form is None and V > SMOOTH_WORKGROUP_MAX_V))
    w = smooth_weights(vertices, adjacency, weights) if moving and weights != "uniform" else None
    ws = _ws(lib.vt_mesh_smooth_workspace_bytes(V), dev) if launches else None
    check(lib.vt_mesh_smooth(dev_ptr(vertices, "vertices", vertices.dtype), int(vertices.dtype == F64), V, dev_ptr(off, "offsets", I32),
                             dev_ptr(nb, "neighbors", I32) if nnz else None, dev_ptr(be, "boundary_edge", U8) if nnz else None,
                             dev_ptr(bv, "boundary_vertex", U8), nnz, dev_ptr(w, "w", F64), SMOOTH_METHODS.index(method), iterations, lam, mu,
                             alpha, beta, SMOOTH_BOUNDARIES.index(boundary), SMOOTH_FORMS.index(form), dev_ptr(out, "out_vertices", out.dtype),
                             ctypes.c_void_p(ws.data_ptr()) if launches else None, ws.numel() * 8 if launches else 0, stream_ptr()),
          "vt_mesh_smooth")
    return out


# ---- subdivision (csrc/mesh_subdivide.hip; tests/mesh_subdivide_ref.py is the definition) ----------------------------------------------------
# One pipeline: mark a set of edges, give each marked edge one new vertex V + e (e in the order in which a walk over the half-edges first
# meets the edge: the order of the reference's UpSampleLayer), split each face by how many of its edges are marked.
SubdivideInfo = namedtuple("SubdivideInfo", ["edge_verts", "face_parent", "n_marked", "n_irregular"])
SUBDIVIDE_SCHEMES = ("midpoint", "loop")


def _subdivide_count(what, vertices, faces, max_edge, face_mask):
    """The checked arguments and vt_mesh_subdivide_count on them: (vertices, faces, workspace, n_marked, n_out_faces, n_irregular);
    the workspace is None for F = 0, where nothing is launched."""
    if max_edge is not None and face_mask is not None:
        raise VtError(f"{what}: max_edge and face_mask are two marking rules; give one")
    if max_edge is not None:
        if isinstance(max_edge, bool) or not isinstance(max_edge, numbers.Real) or not 0.0 < float(max_edge) < float("inf"):
            raise VtError(f"{what}: max_edge must be a positive finite number (got {max_edge!r})")
    faces = _fill_faces(what, faces, vertices)
    vertices = _vertices(what, vertices)
    V, F, dev = vertices.shape[0], faces.shape[0], faces.device
    mark = 1 if max_edge is not None else 2 if face_mask is not None else 0
    if face_mask is not None:
        if not torch.is_tensor(face_mask) or face_mask.device != dev or face_mask.dtype not in (U8, torch.bool) or tuple(face_mask.shape) != (F,):
            raise VtError(f"{what}: face_mask must be uint8 or bool [{F}] on the faces' device")
        face_mask = _c(face_mask.view(U8) if face_mask.dtype == torch.bool else face_mask)
    if F == 0:
        return vertices, faces, None, 0, 0, 0
    lib = _lib.load()
    ws = _ws(lib.vt_mesh_subdivide_workspace_bytes(V, F), dev)
    nm, nf, ni = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    check(lib.vt_mesh_subdivide_count(dev_ptr(vertices, "vertices", vertices.dtype), int(vertices.dtype == F64), V, dev_ptr(faces, "faces", I32), F,
                                      mark, float(max_edge) if mark == 1 else 0.0, dev_ptr(face_mask, "face_mask", U8) if mark == 2 else None,
                                      ctypes.byref(nm), ctypes.byref(nf), ctypes.byref(ni), ctypes.c_void_p(ws.data_ptr()), ws.numel() * 8,
                                      stream_ptr()), "vt_mesh_subdivide_count")
    return vertices, faces, ws, nm.value, nf.value, ni.value


def subdivide_count(vertices, faces, max_edge=None, face_mask=None):
    """(n_marked, n_out_faces, n_irregular) of ``subdivide`` with these arguments, and nothing emitted (vt_mesh_subdivide_count).  One
    host read."""
    return _subdivide_count("mesh.subdivide_count", vertices, faces, max_edge, face_mask)[3:]


def subdivide(vertices, faces, scheme="midpoint", max_edge=None, face_mask=None):
    """(vertices [V + n_marked, 3] in the input's dtype, faces int32 [F_out, 3], SubdivideInfo(edge_verts int32 [n_marked, 2] = (lo, hi),
    face_parent int32 [F_out], n_marked, n_irregular)) (vt_mesh_subdivide_count, vt_mesh_subdivide_emit).  Every edge is marked unless
    ``max_edge`` (the edges longer than it: squared length in float64) or ``face_mask`` (uint8 or bool [F]: the edges of these faces) is
    given.  A face with 3 marked edges (a, b, c) -> (x,y,z) (a,x,z) (b,y,x) (c,z,y) with x, y, z on ab, bc, ca; 2 and 1 marked edges
    give 3 and 2 children that keep the orientation and conform with every neighbour; 0 the face itself.  ``'midpoint'``: originals bit
    for bit, a new vertex (x_lo + x_hi) * 0.5 in the vertices' type.  ``'loop'`` (every edge only): Loop's rules with Warren's weights
    over ``vertex_adjacency``, in float64 and rounded once; boundary edges and vertices by the curve rule; edges with three faces or a
    flipped neighbour are counted in n_irregular, take the midpoint, and their ends stay.  One host read (the totals; ``'loop'`` one
    more for the adjacency).  F = 0, and a rule that marks nothing, return the input tensors themselves.  A face with an index outside
    [0, V) or with a repeated index raises."""
    what = "mesh.subdivide"
    if scheme not in SUBDIVIDE_SCHEMES:
        raise VtError(f"{what}: scheme must be one of {SUBDIVIDE_SCHEMES} (got {scheme!r})")
    if scheme == "loop" and (max_edge is not None or face_mask is not None):
        raise VtError(f"{what}: scheme 'loop' splits every edge; max_edge and face_mask go with 'midpoint'")
    vertices, faces, ws, E, FO, NI = _subdivide_count(what, vertices, faces, max_edge, face_mask)
    V, F, dev = vertices.shape[0], faces.shape[0], faces.device
    if E == 0:
        return vertices, faces, SubdivideInfo(torch.zeros((0, 2), dtype=I32, device=dev), torch.arange(F, dtype=I32, device=dev), 0, 0)
    adj = vertex_adjacency(faces, V) if scheme == "loop" else None
    nnz = adj.neighbors.shape[0] if adj is not None else 0
    out_v = torch.empty((V + E, 3), dtype=vertices.dtype, device=dev)
    out_f = torch.empty((FO, 3), dtype=I32, device=dev)
    ev = torch.empty((E, 2), dtype=I32, device=dev)
    parent = torch.empty(FO, dtype=I32, device=dev)
    check(_lib.load().vt_mesh_subdivide_emit(dev_ptr(vertices, "vertices", vertices.dtype), int(vertices.dtype == F64), V, dev_ptr(faces, "faces", I32),
                                             F, E, FO, SUBDIVIDE_SCHEMES.index(scheme), dev_ptr(adj.offsets, "offsets", I32) if adj else None,
                                             dev_ptr(adj.neighbors, "neighbors", I32) if nnz else None,
                                             dev_ptr(adj.boundary_edge, "boundary_edge", U8) if nnz else None,
                                             dev_ptr(adj.boundary_vertex, "boundary_vertex", U8) if adj else None, nnz,
                                             dev_ptr(out_v, "out_vertices", out_v.dtype), dev_ptr(out_f, "out_faces", I32),
                                             dev_ptr(ev, "edge_verts", I32), dev_ptr(parent, "face_parent", I32), ctypes.c_void_p(ws.data_ptr()),
                                             ws.numel() * 8, stream_ptr()), "vt_mesh_subdivide_emit")
    return out_v, out_f, SubdivideInfo(ev, parent, E, NI)


def _edge_verts(what, edge_verts, dev):
    if not torch.is_tensor(edge_verts) or edge_verts.device != dev or edge_verts.dtype != I32 or edge_verts.dim() != 2 or edge_verts.shape[1] != 2:
        raise VtError(f"{what}: edge_verts must be int32 [E,2] on the vertices' device, as SubdivideInfo holds them")
    return _c(edge_verts)


def subdivide_midpoints(vertices, edge_verts):
    """[B, V + E, 3] from vertices [B, V, 3] (or [V + E, 3] from [V, 3]): the midpoint scheme's vertices on a connectivity that
    ``subdivide`` made once, for a batch that shares it (vt_mesh_subdivide_midpoints).  Nothing here waits for the device."""
    what = "mesh.subdivide_midpoints"
    if not torch.is_tensor(vertices) or not vertices.is_cuda or vertices.dtype not in (torch.float32, F64) or vertices.dim() not in (2, 3) \
            or vertices.shape[-1] != 3 or vertices.shape[-2] < 1 or vertices.shape[0] < 1:
        raise VtError(f"{what}: vertices must be a float32 or float64 [B,V,3] or [V,3] tensor on a HIP device")
    vertices = _c(vertices)
    edge_verts = _edge_verts(what, edge_verts, vertices.device)
    V, E = vertices.shape[-2], edge_verts.shape[0]
    B = vertices.shape[0] if vertices.dim() == 3 else 1
    out = torch.empty(tuple(vertices.shape[:-2]) + (V + E, 3), dtype=vertices.dtype, device=vertices.device)
    check(_lib.load().vt_mesh_subdivide_midpoints(dev_ptr(vertices, "vertices", vertices.dtype), int(vertices.dtype == F64), B, V,
                                                  dev_ptr(edge_verts, "edge_verts", I32) if E else None, E, dev_ptr(out, "out_vertices", out.dtype),
                                                  stream_ptr()), "vt_mesh_subdivide_midpoints")
    return out


def subdivide_backward(grad_out, edge_verts, n_vertices):
    """grad_vertices [V,3] (or [B,V,3]) from grad_out [V + E, 3] (or [B, V + E, 3]) of the midpoint scheme: g_v[i] = g[i] + 0.5 sum of
    g[V + e] over the edges at i (vt_mesh_subdivide_bwd, once per batch item).  Every sum is exact in fixed point and rounded once:
    equal bits from run to run.  Nothing here waits for the device."""
    what = "mesh.subdivide_backward"
    if not torch.is_tensor(grad_out) or not grad_out.is_cuda or grad_out.dtype not in (torch.float32, F64) or grad_out.dim() not in (2, 3) \
            or grad_out.shape[-1] != 3:
        raise VtError(f"{what}: grad_out must be a float32 or float64 [B,V+E,3] or [V+E,3] tensor on a HIP device")
    grad_out = _c(grad_out)
    edge_verts = _edge_verts(what, edge_verts, grad_out.device)
    V, E = _count(what, n_vertices), edge_verts.shape[0]
    if grad_out.shape[-2] != V + E:
        raise VtError(f"{what}: grad_out must have V + E = {V + E} rows (got {grad_out.shape[-2]})")
    out = torch.empty(tuple(grad_out.shape[:-2]) + (V, 3), dtype=grad_out.dtype, device=grad_out.device)
    lib = _lib.load()
    ws = _ws(lib.vt_mesh_subdivide_bwd_workspace_bytes(V), grad_out.device)
    g2, o2 = grad_out.reshape(-1, V + E, 3), out.reshape(-1, V, 3)
    for b in range(g2.shape[0]):
        check(lib.vt_mesh_subdivide_bwd(dev_ptr(edge_verts, "edge_verts", I32) if E else None, V, E, dev_ptr(g2[b], "grad_out", g2.dtype),
                                        int(g2.dtype == F64), dev_ptr(o2[b], "grad_vertices", o2.dtype), ctypes.c_void_p(ws.data_ptr()),
                                        ws.numel() * 8, stream_ptr()), "vt_mesh_subdivide_bwd")
    return out
