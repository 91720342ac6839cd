"""Which pieces a mesh consists of, which of them are closed, and the mesh without its floaters -- what the reference gets from wrapping
its meshes in ``trimesh.Trimesh`` (``split``, ``area``, ``volume``, ``is_watertight``, ``euler_number``), on the device
(csrc/mesh_topo.hip through ``ops.mesh``).

    components(mesh) -> MeshComponents           every per-component tensor, on the device; ``.report()`` for a host dict
    split(mesh) -> [Mesh, ...]                   one mesh per component, in component order
    keep_largest(mesh, by='faces') -> Mesh       by 'faces', 'area' or 'volume' (|signed volume|); ties go to the lower component
    remove_small(mesh, min_faces=0, min_area_fraction=0.0) -> Mesh
    simplify(mesh, nfaces=None, resolution=None, placement='quadric') -> Mesh        (csrc/mesh_simplify.hip, as the next two)
    simplify_report(...) -> (Mesh, SimplifyReport)
    merge_vertices(mesh, tol=0.0, unique_faces=False) -> Mesh
    decimate(mesh, nfaces, placement='optimal') -> Mesh          manifold-preserving edge collapse (csrc/mesh_collapse.hip, as the next)
    decimate_report(...) -> (Mesh, DecimateReport)
    face_normals(mesh) -> [F,3]                  unit, (0,0,0) for a degenerate face (csrc/mesh_normals.hip, as the next two)
    vertex_normals(mesh, weight='area') -> [V,3] 'area' or 'angle'; (0,0,0) for a vertex no live face references
    with_vertex_normals(mesh, weight='area') -> NormalMesh
    boundary_loops(mesh) -> BoundaryLoops        the boundary half-edges linked into loops (csrc/mesh_fill.hip, as the next two)
    fill_holes(mesh, method='fan', max_edges=None) -> Mesh       every loop capped; the mesh itself when it has none
    fill_report(...) -> (Mesh, FillReport)
    vertex_neighbors(mesh) -> MeshAdjacency      CSR rows of the vertex-vertex adjacency (csrc/mesh_smooth.hip, as the next four)
    vertex_degree(mesh) -> [V], boundary_vertices(mesh) -> bool [V]
    smooth(mesh, method='taubin', iterations=10, ...) -> Mesh    'laplacian', 'taubin' or 'humphrey'; the same faces
    smooth_report(...) -> (Mesh, SmoothReport)
    subdivide(mesh, iterations=1, face_index=None) -> Mesh       1-to-4 midpoint subdivision (csrc/mesh_subdivide.hip, as the next three)
    subdivide_loop(mesh, iterations=1) -> Mesh                   Loop's scheme with Warren's weights
    subdivide_to_size(mesh, max_edge, max_iter=10) -> Mesh       adaptive rounds until no edge is longer than max_edge
    subdivide_report(...) -> (Mesh, SubdivideReport)

A mesh is ``generation.Mesh``, any object with ``.vertices`` / ``.faces``, or a ``(vertices, faces)`` pair of device tensors: vertices
float32 or float64 [V,3], faces int32 [F,3] (int64 faces are converted here).  Components are numbered by their smallest vertex index.
Unreferenced vertices belong to no component and are dropped by every function that returns a mesh.  A mesh without faces has no
components: ``split`` gives [], the other two give the empty mesh.  There is no host path."""
from collections import namedtuple

import torch

from .._lib import VtError

BY = ("faces", "area", "volume")

_FIELDS = ["labels", "comp_of_vertex", "comp_of_face", "n_components", "n_faces", "n_vertices", "bbox", "area", "volume", "n_edges",
           "n_boundary", "n_nonmanifold", "n_misoriented", "euler", "watertight", "oriented", "rounds"]


class MeshComponents(namedtuple("MeshComponents", _FIELDS)):
    """labels, comp_of_vertex [V] and comp_of_face [F] (int32), n_components (int), and per component: n_faces, n_vertices, n_edges,
    n_boundary, n_nonmanifold, n_misoriented, euler (int32 [C]), bbox [C,2,3], area, volume (float64 [C]; the volume is signed, about
    the origin, and means something for closed components only), watertight = no boundary and no non-manifold edge, oriented =
    watertight with every edge run once in each direction (bool [C]).  ``rounds``: the hooking rounds the labels took."""
    __slots__ = ()

    def report(self):
        """A host dict of lists, one entry per component (one device-to-host copy of the integer block, one of the float block)."""
        ints = torch.stack([self.n_faces, self.n_vertices, self.n_edges, self.n_boundary, self.n_nonmanifold, self.n_misoriented,
                            self.euler, self.watertight.int(), self.oriented.int()]).cpu().tolist() if self.n_components else [[]] * 9
        flts = torch.stack([self.area, self.volume]).cpu().tolist() if self.n_components else [[]] * 2
        names = ["n_faces", "n_vertices", "n_edges", "n_boundary", "n_nonmanifold", "n_misoriented", "euler"]
        out = {"n_components": self.n_components, "rounds": self.rounds}
        out.update(dict(zip(names, ints[:7])))
        out["watertight"] = [bool(x) for x in ints[7]]
        out["oriented"] = [bool(x) for x in ints[8]]
        out["area"], out["volume"] = flts
        return out


def _parts(mesh):
    if hasattr(mesh, "vertices") and hasattr(mesh, "faces"):
        v, f = mesh.vertices, mesh.faces
    else:
        v, f = mesh
    if not torch.is_tensor(v) or not torch.is_tensor(f) or not v.is_cuda or not f.is_cuda:
        raise VtError("mesh_clean: vertices and faces must be tensors on a HIP device; vtaco_amd has no CPU path")
    if f.dtype == torch.int64:
        f = f.int()
    return v, f


def _empty(v, f):
    from ..conv_onet.generation import Mesh
    return Mesh(v[:0], f[:0])


def components(mesh):
    """The MeshComponents record of ``mesh``.  Two host reads: the labels' convergence flags (one read per two hooking rounds; a mesh
    whose hooks did not collide takes two rounds) and the component count."""
    from .. import ops
    v, f = _parts(mesh)
    if f.shape[0] == 0:
        raise VtError("mesh_clean.components: a mesh without faces has no components (F = 0)")
    m = ops.mesh
    labels, rounds = m.components(f, v.shape[0], return_rounds=True)
    table = m.component_table(f, labels)
    st = m.component_stats(v, f, table)
    ed = m.edge_stats(f, table)
    euler = st.n_vertices - ed.n_edges + st.n_faces
    watertight = (ed.n_boundary == 0) & (ed.n_nonmanifold == 0)
    oriented = watertight & (ed.n_misoriented == 0)
    return MeshComponents(labels, table.comp_of_vertex, table.comp_of_face, table.n_components, st.n_faces, st.n_vertices, st.bbox, st.area,
                          st.volume, ed.n_edges, ed.n_boundary, ed.n_nonmanifold, ed.n_misoriented, euler, watertight, oriented, rounds)


def _filtered(v, f, comps, keep):
    from .. import ops
    from ..conv_onet.generation import Mesh
    table = ops.mesh.ComponentTable(comps.n_components, comps.comp_of_vertex, comps.comp_of_face)
    out = ops.mesh.filter_components(v, f, table, keep)
    return Mesh(out.vertices, out.faces)


def split(mesh, comps=None):
    """One Mesh per component, in component order (``comps``: a MeshComponents of this mesh, when the caller has one).  One filter
    call per component: each scans all V vertices and F faces, allocates capacity (V, F) outputs and reads its two counts back, so the
    cost is C host reads and C passes over the mesh -- meant for the handful of pieces a generated mesh has, not for thousands (use
    ``comp_of_face`` / ``comp_of_vertex`` of ``components`` to bucket those)."""
    v, f = _parts(mesh)
    if f.shape[0] == 0:
        return []
    comps = components((v, f)) if comps is None else comps
    eye = torch.eye(comps.n_components, dtype=torch.uint8, device=f.device)
    return [_filtered(v, f, comps, eye[c]) for c in range(comps.n_components)]


def largest_mask(comps, by="faces", among=None):
    """bool [C]: the one component that is largest by ``by`` among those ``among`` (bool [C]; all without it) marks; equal sizes go to
    the lower component; nothing set where ``among`` is empty.  Nothing is read back."""
    if by not in BY:
        raise VtError(f"keep_largest: by must be one of {BY} (got {by!r})")
    size = {"faces": comps.n_faces, "area": comps.area, "volume": comps.volume.abs()}[by].double()
    if among is not None:
        size = torch.where(among, size, -1.0)                                # (sizes are >= 0: a component outside never wins)
    # the first index of the maximum: argmax leaves the choice among equals open
    idx = torch.arange(comps.n_components, device=size.device)
    mask = idx == torch.where(size == size.max(), idx, comps.n_components).min()
    return mask if among is None else mask & among


def keep_largest(mesh, by="faces", comps=None):
    """The component with the most faces, the largest area or the largest |signed volume|; equal sizes go to the lower component."""
    if by not in BY:
        raise VtError(f"keep_largest: by must be one of {BY} (got {by!r})")
    v, f = _parts(mesh)
    if f.shape[0] == 0:
        return _empty(v, f)
    comps = components((v, f)) if comps is None else comps
    return _filtered(v, f, comps, largest_mask(comps, by))


def remove_small(mesh, min_faces=0, min_area_fraction=0.0, comps=None):
    """Every component with at least ``min_faces`` faces and at least ``min_area_fraction`` of the mesh's total area."""
    if int(min_faces) != min_faces or min_faces < 0 or not 0.0 <= float(min_area_fraction) <= 1.0:
        raise VtError(f"remove_small: min_faces must be an integer >= 0 and min_area_fraction lie in [0, 1] (got {min_faces}, {min_area_fraction})")
    v, f = _parts(mesh)
    if f.shape[0] == 0:
        return _empty(v, f)
    comps = components((v, f)) if comps is None else comps
    keep = (comps.n_faces >= int(min_faces)) & (comps.area >= float(min_area_fraction) * comps.area.sum())
    return _filtered(v, f, comps, keep)


# ---- simplification and welding (csrc/mesh_simplify.hip; tests/mesh_simplify_ref.py is the definition) --------------------------------
SimplifyReport = namedtuple("SimplifyReport", ["resolution", "probes", "n_clusters", "fallbacks", "cluster_of_vertex"])
SimplifyReport.__doc__ = """resolution: the grid that was used (None: the mesh was returned unchanged); probes: the grids the search for
``nfaces`` counted faces at; n_clusters: K, the vertices of the result; fallbacks: the clusters placed at their mean because the quadric's
minimiser left the cell; cluster_of_vertex int32 [V]: the output vertex of every input vertex (-1: unreferenced)."""


def _positive_int(what, name, x):
    if isinstance(x, bool) or int(x) != x or int(x) < 1:
        raise VtError(f"{what}: {name} must be a positive integer (got {x!r})")
    return int(x)


def _search(count, nfaces, max_resolution):
    """(resolution, probes): gallop from (1, 2) while count(hi) <= nfaces, then bisect on the same predicate; the answer is lo.  count
    is not monotone in the resolution (the lattice aliases): the answer has at most nfaces faces, it is not the finest such grid."""
    lo, hi, probes = 1, 2, 0
    while hi <= max_resolution:
        probes += 1
        if count(hi) > nfaces:
            break
        lo, hi = hi, 2 * hi
    hi = min(hi, max_resolution + 1)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        probes += 1
        if count(mid) <= nfaces:
            lo = mid
        else:
            hi = mid
    return lo, probes


def simplify_report(mesh, nfaces=None, resolution=None, placement="quadric", _count_fallbacks=True):
    """(Mesh, SimplifyReport).  Vertex clustering (Lindstrom 2000): the referenced vertices are grouped by their cell of a grid with
    ``resolution`` cells along the longest side of their bounding box, every occupied cell becomes one vertex, faces that collapse and
    later copies of a face are dropped, the rest keep their order and orientation.  ``placement='quadric'`` puts the vertex where the
    summed squared distances to the planes of the cluster's faces (area-weighted) are smallest, within the cell; ``'mean'`` at the
    mean of the cluster's vertices.  Exactly one of ``nfaces`` / ``resolution``: ``nfaces`` searches the grid (gallop, then bisection;
    one host read per probe; probes run no placement) for a result of at most ``nfaces`` faces and returns the mesh itself, with
    nothing launched, when it has no more than that.  Topology is NOT preserved: handles close, sheets that share a cell merge and
    the result may have non-manifold edges (``components()`` reports them).  Deterministic, bit for bit."""
    from .. import ops
    from ..conv_onet.generation import Mesh
    what = "mesh_clean.simplify"
    if (nfaces is None) == (resolution is None):
        raise VtError(f"{what}: give exactly one of nfaces / resolution (got nfaces={nfaces!r}, resolution={resolution!r})")
    if placement not in ("quadric", "mean"):
        raise VtError(f"{what}: placement must be 'quadric' or 'mean' (got {placement!r})")
    v, f = _parts(mesh)
    m = ops.mesh
    probes = 0
    if nfaces is not None:
        nfaces = _positive_int(what, "nfaces", nfaces)
        if f.shape[0] <= nfaces:
            return (mesh if isinstance(mesh, Mesh) else Mesh(v, f)), SimplifyReport(None, 0, None, 0, None)
        resolution, probes = _search(lambda r: m.cluster_faces(f, m.cluster(v, f, r), count_only=True).n_faces, nfaces, m.MAX_RESOLUTION)
    elif isinstance(resolution, bool) or int(resolution) != resolution or not 1 <= int(resolution) <= m.MAX_RESOLUTION:
        raise VtError(f"{what}: resolution must be an integer in [1, {m.MAX_RESOLUTION}] (got {resolution!r})")
    if f.shape[0] == 0:
        return _empty(v, f), SimplifyReport(int(resolution), 0, 0, 0, None)
    clusters = m.cluster(v, f, int(resolution))
    faces = m.cluster_faces(f, clusters)
    if faces.n_clusters == 0:                                             # (no face with three valid indices is an error before this)
        return _empty(v, f), SimplifyReport(int(resolution), probes, 0, 0, clusters.cluster_of_vertex)
    vertices = m.cluster_place(v, f, clusters, faces.n_clusters, placement)
    fallbacks = int(clusters.state[m.STATE_FALLBACKS]) if placement == "quadric" and _count_fallbacks else 0
    return Mesh(vertices, faces.faces), SimplifyReport(int(resolution), probes, faces.n_clusters, fallbacks, clusters.cluster_of_vertex)


def simplify(mesh, nfaces=None, resolution=None, placement="quadric"):
    """``simplify_report`` without the report, and without its read of the fallback count."""
    return simplify_report(mesh, nfaces=nfaces, resolution=resolution, placement=placement, _count_fallbacks=False)[0]


def merge_vertices(mesh, tol=0.0, unique_faces=False):
    """The mesh with equal vertices merged, as trimesh's ``merge_vertices`` / ``process=True`` leaves it: ``tol`` 0 merges equal
    coordinates (-0.0 equals +0.0; a vertex with a NaN coordinate merges with nothing), ``tol`` > 0 the vertices with equal
    rint(x / tol) on every axis.  Of each group the lowest vertex index survives with its own coordinates, the survivors keep their
    order; faces with two equal corners are dropped, later copies of a face (as an unordered triple) with ``unique_faces``;
    unreferenced vertices are dropped.  One host read."""
    from .. import ops
    from ..conv_onet.generation import Mesh
    v, f = _parts(mesh)
    if f.shape[0] == 0:
        return _empty(v, f)
    m = ops.mesh
    clusters = m.weld(v, f, tol)
    faces = m.cluster_faces(f, clusters, unique=bool(unique_faces))
    if faces.n_clusters == 0:
        return _empty(v, f)
    return Mesh(m.cluster_place(v, f, clusters, faces.n_clusters, "representative"), faces.faces)


# ---- decimation by edge collapse (csrc/mesh_collapse.hip; tests/mesh_collapse_ref.py is the definition) -------------------------------
DecimateReport = namedtuple("DecimateReport", ["rounds", "stalled", "vertex_map"])
DecimateReport.__doc__ = """rounds: the rounds that collapsed at least one edge (0: the mesh was returned unchanged); stalled: a round found
no edge left that may collapse, so the result has more than ``nfaces`` faces; vertex_map int32 [V]: the output vertex every input vertex
went into (-1: unreferenced; None where nothing ran)."""


def decimate_report(mesh, nfaces, placement="optimal"):
    """(Mesh, DecimateReport).  Quadric edge-collapse decimation in rounds of independent collapses (``ops.mesh.collapse``): what the
    reference's ``simplify_nfaces`` means.  Unlike ``simplify`` it keeps the surface what it is -- a closed oriented manifold stays one,
    with its components and Euler number -- and lands on the largest even face count <= ``nfaces``.  Boundary edges and non-manifold
    edges never move, and neither do their ends, so an open mesh keeps its rim vertex for vertex and may stall above ``nfaces``.
    ``placement='optimal'`` puts a merged vertex where the summed squared distances to the planes of both ends' faces are smallest,
    ``'midpoint'`` at the middle of the edge.  A mesh with at most ``nfaces`` faces is returned itself, with nothing launched.  A
    ``NormalMesh`` gets geometric normals afterwards, as after ``simplify``.  Deterministic, bit for bit."""
    from .. import ops
    from ..conv_onet.generation import Mesh, NormalMesh
    what = "mesh_clean.decimate"
    nfaces = _positive_int(what, "nfaces", nfaces)
    if placement not in ops.mesh.COLLAPSE_PLACEMENTS:
        raise VtError(f"{what}: placement must be one of {ops.mesh.COLLAPSE_PLACEMENTS} (got {placement!r})")
    v, f = _parts(mesh)
    if f.shape[0] <= nfaces:
        return (mesh if isinstance(mesh, Mesh) else Mesh(v, f)), DecimateReport(0, False, None)
    out = ops.mesh.collapse(v, f, nfaces, placement=placement)
    result = Mesh(out.vertices, out.faces)
    if isinstance(mesh, NormalMesh) and out.faces.shape[0] > 0:
        result = with_vertex_normals(result, weight="area")
    return result, DecimateReport(out.rounds, out.stalled, out.vertex_map)


def decimate(mesh, nfaces, placement="optimal"):
    """``decimate_report`` without the report."""
    return decimate_report(mesh, nfaces, placement=placement)[0]


# ---- normals (csrc/mesh_normals.hip; tests/mesh_normals_ref.py is the definition) --------------------------------------------------------
def face_normals(mesh):
    """Unit face normals [F,3] in the vertices' dtype, by the faces' winding; (0,0,0) for a degenerate face.  [0,3] without faces."""
    from .. import ops
    v, f = _parts(mesh)
    if f.shape[0] == 0:
        return v.new_zeros((0, 3))
    return ops.mesh.normals(v, f, vertex=False).face_normals


def vertex_normals(mesh, weight="area"):
    """Unit vertex normals [V,3] in the vertices' dtype: the normalised sum of the vertex's faces' raw cross products (``'area'``, what
    trimesh's default amounts to up to its sparse-matrix rounding) or of their unit normals times the corner angle (``'angle'``).
    (0,0,0) for a vertex that no live face references.  Exact sums: the bits do not depend on the order of the faces."""
    from .. import ops
    if weight not in ops.mesh.WEIGHTS:
        raise VtError(f"mesh_clean.vertex_normals: weight must be one of {ops.mesh.WEIGHTS} (got {weight!r})")
    v, f = _parts(mesh)
    if f.shape[0] == 0 or v.shape[0] == 0:
        return torch.zeros_like(v)
    return ops.mesh.normals(v, f, weight=weight, face=False).vertex_normals


def with_vertex_normals(mesh, weight="area"):
    """The mesh as a ``NormalMesh`` that carries its geometric vertex normals (``normals_source='geometry'``)."""
    from ..conv_onet.generation import NormalMesh
    v, f = _parts(mesh)
    return NormalMesh(v, f, vertex_normals=vertex_normals((v, f), weight=weight), normals_source="geometry")


# ---- hole filling (csrc/mesh_fill.hip; tests/mesh_fill_ref.py is the definition) -----------------------------------------------------------
FillReport = namedtuple("FillReport", ["n_loops", "n_filled", "n_new_faces", "n_new_vertices", "n_boundary", "n_irregular", "loops"])
FillReport.__doc__ = """n_loops: the boundary loops of the input; n_filled: those that were capped (3 <= edges <= max_edges); n_new_faces,
n_new_vertices: what the caps added; n_boundary: the input's boundary half-edges; n_irregular: those on no loop (a vertex shared by two
holes, a hole beside a flipped or non-manifold face), which are never filled; loops: the BoundaryLoops record (offsets, vertices,
half_edges on the device)."""


def boundary_loops(mesh):
    """``ops.mesh.BoundaryLoops`` of the mesh: loop l owns ``[offsets[l], offsets[l+1])`` of ``vertices`` / ``half_edges``, starts at
    its smallest half-edge (h = 3 f + k: corner k of face f, to corner (k+1) % 3) and runs with the faces along it; loops are
    numbered by that half-edge.  Two host reads, one for a closed mesh."""
    from .. import ops
    v, f = _parts(mesh)
    if v.shape[0] == 0:
        raise VtError("mesh_clean.boundary_loops: a mesh without vertices (V = 0)")
    return ops.mesh.boundary_loops(f, v.shape[0])


def fill_report(mesh, method="fan", max_edges=None):
    """(Mesh, FillReport).  Every boundary loop of 3 <= n <= ``max_edges`` edges (None: every loop) is capped against the direction of
    its boundary, so the cap continues the surface's orientation.  ``'fan'``: n - 2 faces about the loop's first vertex, no new vertex.
    ``'centroid'``: n faces about one new vertex at the loop's mean (a triangle gets its one face).  New faces follow the originals by
    (loop, position), new vertices by loop; the originals are copied unchanged.  A loop whose vertices lie in one plane -- where
    marching cubes met the side of its box -- is capped exactly by either method (the fan of a concave outline folds over itself, but
    its signed area, and so the mesh's volume and winding number, are right); nested planar loops (a hollow cross-section) get two
    caps of opposite orientation and the result is watertight with the right signed volume.  A curved hole gets a geometrically crude
    cap: closed and oriented, nothing more.  Irregular boundary edges are counted and left open.  A mesh that has no loop to fill
    comes back as the same object.  On a ``NormalMesh`` ``'fan'`` keeps ``vertex_normals`` and ``values`` (no vertex is added) and
    ``'centroid'`` raises.  Three host reads.  Deterministic, bit for bit."""
    from .. import ops
    from ..conv_onet.generation import Mesh, NormalMesh
    what = "mesh_clean.fill_holes"
    if method not in ops.mesh.FILL_METHODS:
        raise VtError(f"{what}: method must be one of {ops.mesh.FILL_METHODS} (got {method!r})")
    if isinstance(mesh, NormalMesh) and method == "centroid":
        raise VtError(f"{what}: method='centroid' adds vertices that have no marching-cubes normal or value, so it is not applied to a "
                      "NormalMesh; use method='fan', which adds none, or fill a plain Mesh and take geometric normals with "
                      "with_vertex_normals()")
    v, f = _parts(mesh)
    same = mesh if isinstance(mesh, Mesh) else Mesh(v, f)
    if f.shape[0] == 0 or v.shape[0] == 0:
        return same, FillReport(0, 0, 0, 0, 0, 0, None)
    loops = ops.mesh.boundary_loops(f, v.shape[0])
    out = ops.mesh.fill_holes(v, f, method=method, max_edges=max_edges, loops=loops)
    report = FillReport(out.n_loops, out.n_filled, out.n_new_faces, out.n_new_vertices, loops.n_boundary, out.n_irregular, loops)
    if out.n_new_faces == 0:
        return same, report
    if isinstance(mesh, NormalMesh):
        return NormalMesh(out.vertices, out.faces, vertex_normals=mesh.vertex_normals, values=mesh.values,
                          normals_source=mesh.normals_source), report
    return Mesh(out.vertices, out.faces), report


def fill_holes(mesh, method="fan", max_edges=None):
    """``fill_report`` without the report."""
    return fill_report(mesh, method=method, max_edges=max_edges)[0]


# ---- vertex adjacency and smoothing (csrc/mesh_smooth.hip; tests/mesh_smooth_ref.py is the definition) -------------------------------------
SmoothReport = namedtuple("SmoothReport", ["area_before", "area_after", "volume_before", "volume_after", "max_displacement",
                                           "rms_displacement", "n_pinned", "adjacency"])
SmoothReport.__doc__ = """area_*, volume_*: the mesh's area and signed volume (``component_stats`` summed over the components; the volume
means something for a closed mesh only) before and after; max_displacement, rms_displacement: over all vertices, in float64; n_pinned:
the boundary vertices that ``boundary='pin'`` held (0 under the other rules); adjacency: the MeshAdjacency that was used."""


def vertex_neighbors(mesh):
    """``ops.mesh.MeshAdjacency`` of the mesh -- what ``trimesh.Trimesh.vertex_neighbors`` holds, as CSR rows on the device: vertex i's
    neighbours are ``neighbors[offsets[i]:offsets[i+1]]``, ascending; ``boundary_edge`` marks the entries across an edge with one face,
    ``boundary_vertex`` the vertices on such an edge.  One host read."""
    from .. import ops
    v, f = _parts(mesh)
    if v.shape[0] == 0:
        raise VtError("mesh_clean.vertex_neighbors: a mesh without vertices (V = 0)")
    return ops.mesh.vertex_adjacency(f, v.shape[0])


def vertex_degree(mesh, adjacency=None):
    """int32 [V]: the number of neighbours of every vertex (0 for an unreferenced one)."""
    adjacency = vertex_neighbors(mesh) if adjacency is None else adjacency
    return adjacency.offsets[1:] - adjacency.offsets[:-1]


def boundary_vertices(mesh, adjacency=None):
    """bool [V]: the vertices that an edge with exactly one face ends at."""
    adjacency = vertex_neighbors(mesh) if adjacency is None else adjacency
    return adjacency.boundary_vertex.bool()


def smooth(mesh, method="taubin", iterations=10, lam=0.5, mu=-0.53, alpha=0.1, beta=0.5, weights="uniform", boundary="pin", adjacency=None):
    """The mesh with the same faces and smoothed vertices: ``'laplacian'``, ``'taubin'`` (the lambda|mu filter, which does not shrink) or
    ``'humphrey'`` (the HC filter of Vollmer et al.), as ``trimesh.smoothing`` offers them; ``ops.mesh.smooth`` has the definitions of
    the arguments.  ``adjacency``: ``vertex_neighbors`` of this mesh, when the caller has it (the call then reads nothing back).  A
    ``NormalMesh`` comes back with its normals recomputed from the new geometry (``normals_source='geometry'``, no ``values``), as from
    ``simplify``.  A mesh without faces, and ``iterations=0``, give a copy of the vertices.  Deterministic, bit for bit."""
    from .. import ops
    from ..conv_onet.generation import Mesh, NormalMesh
    args = ops.mesh.smooth_arguments("mesh_clean.smooth", method, iterations, lam, mu, alpha, beta, weights, boundary)
    v, f = _parts(mesh)
    if v.shape[0] == 0:
        return mesh if isinstance(mesh, Mesh) else Mesh(v, f)
    if adjacency is None:
        adjacency = ops.mesh.vertex_adjacency(f, v.shape[0])
    out = ops.mesh.smooth(v, adjacency, *args)
    if isinstance(mesh, NormalMesh):
        return with_vertex_normals((out, f))
    return Mesh(out, f)


def _area_volume(v, f):
    from .. import ops
    m = ops.mesh
    if f.shape[0] == 0:
        return 0.0, 0.0
    table = m.component_table(f, m.components(f, v.shape[0]))
    st = m.component_stats(v, f, table)
    return float(st.area.sum()), float(st.volume.sum())


def smooth_report(mesh, method="taubin", iterations=10, lam=0.5, mu=-0.53, alpha=0.1, beta=0.5, weights="uniform", boundary="pin",
                  adjacency=None):
    """(Mesh, SmoothReport): ``smooth`` and what it did to the area, the signed volume and the vertices."""
    v, f = _parts(mesh)
    if adjacency is None and v.shape[0]:
        adjacency = vertex_neighbors((v, f))
    out = smooth(mesh, method=method, iterations=iterations, lam=lam, mu=mu, alpha=alpha, beta=beta, weights=weights, boundary=boundary,
                 adjacency=adjacency)
    if v.shape[0] == 0:
        return out, SmoothReport(0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0, None)
    a0, v0 = _area_volume(v, f)
    a1, v1 = _area_volume(out.vertices, f)
    d2 = ((out.vertices.double() - v.double()) ** 2).sum(1)
    n_pinned = int(adjacency.boundary_vertex.sum()) if boundary == "pin" else 0
    return out, SmoothReport(a0, a1, v0, v1, float(d2.max().sqrt()), float(d2.mean().sqrt()), n_pinned, adjacency)


# ---- subdivision (csrc/mesh_subdivide.hip; tests/mesh_subdivide_ref.py is the definition) ---------------------------------------------------
SubdivideReport = namedtuple("SubdivideReport", ["rounds", "n_vertices", "n_faces", "n_marked", "n_irregular", "face_parent"])
SubdivideReport.__doc__ = """rounds: the rounds that split something; n_vertices, n_faces, n_marked, n_irregular: one entry per such round
(the counts after it, the edges it split, the edges among them that are neither interior nor boundary); face_parent int32 [F_out]: the
face of the INPUT mesh every returned face lies in."""


def _positive_count(what, name, x, least=0):
    if isinstance(x, bool) or int(x) != x or int(x) < least:
        raise VtError(f"{what}: {name} must be an integer >= {least} (got {x!r})")
    return int(x)


def subdivide_report(mesh, scheme="midpoint", iterations=1, face_index=None, max_edge=None, max_iter=10):
    """(Mesh, SubdivideReport).  ``max_edge`` None: ``iterations`` rounds of ``scheme`` ('midpoint' or 'loop'), the first over the faces
    ``face_index`` (int tensor or list of face indices, or a bool / uint8 mask [F]; None: every face) and their neighbours' shared
    edges, later rounds over the children of those faces.  ``max_edge``: adaptive midpoint rounds, each splitting the edges longer than
    ``max_edge``, until a round marks nothing; ``VtError`` naming the edges left when ``max_iter`` rounds do not suffice.  One host
    read per round.  Vertices keep their indices, new ones follow; a ``NormalMesh`` comes back with geometric normals
    (``normals_source='geometry'``, no values), as after ``smooth``.  A round that marks nothing returns its input."""
    from .. import ops
    from ..conv_onet.generation import Mesh, NormalMesh
    what = "mesh_clean.subdivide"
    if scheme not in ops.mesh.SUBDIVIDE_SCHEMES:
        raise VtError(f"{what}: scheme must be one of {ops.mesh.SUBDIVIDE_SCHEMES} (got {scheme!r})")
    adaptive = max_edge is not None
    rounds_max = _positive_count(what, "max_iter", max_iter) if adaptive else _positive_count(what, "iterations", iterations)
    if adaptive and (scheme != "midpoint" or face_index is not None):
        raise VtError(f"{what}: max_edge goes with scheme='midpoint' and without face_index")
    if face_index is not None and scheme != "midpoint":
        raise VtError(f"{what}: face_index goes with scheme='midpoint'")
    v, f = _parts(mesh)
    same = mesh if isinstance(mesh, Mesh) else Mesh(v, f)
    F0 = f.shape[0]
    if F0 == 0 or v.shape[0] == 0:
        return same, SubdivideReport(0, [], [], [], [], torch.zeros(0, dtype=torch.int32, device=f.device))
    mask = None
    if face_index is not None:
        idx = torch.as_tensor(face_index, device=f.device)
        if idx.dtype in (torch.bool, torch.uint8) and tuple(idx.shape) == (F0,):
            mask = idx.to(torch.uint8)
        else:
            idx = idx.reshape(-1).long()
            if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= F0):
                raise VtError(f"{what}: face_index outside [0, {F0})")
            mask = torch.zeros(F0, dtype=torch.uint8, device=f.device)
            mask[idx] = 1
    parent = torch.arange(F0, dtype=torch.int32, device=f.device)
    nv, nf, nm, ni = [], [], [], []
    for it in range(rounds_max + (1 if adaptive else 0)):
        if adaptive and it == rounds_max:
            # one more count, nothing emitted: what is left
            left = ops.mesh.subdivide_count(v, f, max_edge=max_edge)[0]
            if left:
                raise VtError(f"mesh_clean.subdivide_to_size: {left} edges are still longer than {max_edge} after {rounds_max} rounds")
            break
        ov, of, info = ops.mesh.subdivide(v, f, scheme=scheme, max_edge=max_edge, face_mask=mask)
        if info.n_marked == 0:
            break
        if mask is not None:
            mask = mask[info.face_parent.long()]                    # the children of the selected faces
        parent = parent[info.face_parent.long()]
        v, f = ov, of
        nv.append(v.shape[0]); nf.append(f.shape[0]); nm.append(info.n_marked); ni.append(info.n_irregular)
    report = SubdivideReport(len(nm), nv, nf, nm, ni, parent)
    if not nm:
        return same, report
    if isinstance(mesh, NormalMesh):
        return with_vertex_normals((v, f)), report
    return Mesh(v, f), report


def subdivide(mesh, iterations=1, face_index=None):
    """1-to-4 midpoint subdivision, ``iterations`` times: every edge gets its midpoint as a new vertex, every face (a, b, c) becomes
    (x,y,z) (a,x,z) (b,y,x) (c,z,y) -- the reference's ``UpSampleLayer``, and ``trimesh.remesh.subdivide`` up to the numbering of the
    new vertices.  ``face_index``: only these faces are split in four; their neighbours are split in two or three so that the mesh stays
    conforming (no T-junction).  ``subdivide_report`` has the rest."""
    return subdivide_report(mesh, "midpoint", iterations=iterations, face_index=face_index)[0]


def subdivide_loop(mesh, iterations=1):
    """Loop subdivision, ``iterations`` times (``trimesh.remesh.subdivide_loop``): the connectivity of ``subdivide``, old and new
    vertices placed by Loop's rules with Warren's weights, boundaries by the curve rule (``ops.mesh.subdivide``)."""
    return subdivide_report(mesh, "loop", iterations=iterations)[0]


def subdivide_to_size(mesh, max_edge, max_iter=10):
    """Adaptive midpoint rounds until no edge is longer than ``max_edge`` (``trimesh.remesh.subdivide_to_size``): each round splits the
    edges that are too long, a face by how many of its edges are.  ``VtError`` naming the remaining count when ``max_iter`` rounds do
    not suffice.  One host read per round."""
    if isinstance(max_edge, bool) or not 0.0 < float(max_edge) < float("inf"):
        raise VtError(f"mesh_clean.subdivide_to_size: max_edge must be a positive finite number (got {max_edge!r})")
    return subdivide_report(mesh, "midpoint", max_edge=float(max_edge), max_iter=max_iter)[0]
