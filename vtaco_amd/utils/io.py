"""Point-cloud and OFF files with the reference's names (src/utils/io.py), without plyfile: the PLY header is a dozen lines of text and
the body one numpy record array.  Host side; tensors are brought to the host first."""
import os

import numpy as np

from .._lib import VtError

_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def _host(x, what, name):
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    x = np.asarray(x)
    if x.ndim != 2 or x.shape[1] != 3:
        raise VtError(f"{what}: {name} must be [N,3] (got {tuple(x.shape)})")
    return np.ascontiguousarray(x.astype(np.float32))


def export_pointcloud(vertices, out_file, as_text=True, normals=None):
    """Write vertices [N,3] (and normals [N,3]) as a PLY vertex element of float32 ``x y z`` (``nx ny nz``): ascii, or
    binary_little_endian with ``as_text=False`` (export_pointcloud, src/utils/io.py:6-14).  ascii values carry 9 significant digits
    and read back to the same float32."""
    what = "export_pointcloud"
    v = _host(vertices, what, "vertices")
    names = ["x", "y", "z"]
    if normals is not None:
        n = _host(normals, what, "normals")
        if len(n) != len(v):
            raise VtError(f"{what}: {len(n)} normals for {len(v)} vertices")
        v = np.ascontiguousarray(np.concatenate([v, n], axis=1))
        names += ["nx", "ny", "nz"]
    head = ["ply", "format ascii 1.0" if as_text else "format binary_little_endian 1.0", f"element vertex {len(v)}"]
    head += [f"property float {c}" for c in names] + ["end_header"]
    with open(out_file, "wb") as fh:
        fh.write(("\n".join(head) + "\n").encode("ascii"))
        if as_text:
            fh.write("".join(" ".join("%.9g" % x for x in row) + "\n" for row in v.tolist()).encode("ascii"))
        else:
            fh.write(v.astype("<f4").tobytes())


def _ply_header(fh, what, in_file):
    """(format, [(element name, count, [(property name, numpy type or None for a list)])]); the file is left at the body's first byte."""
    if fh.readline().strip() != b"ply":
        raise VtError(f"{what}: {in_file} is not a PLY file")
    fmt, elements = None, []
    while True:
        line = fh.readline()
        if not line:
            raise VtError(f"{what}: {in_file} ends inside its header")
        words = line.decode("ascii", "replace").split()
        if not words or words[0] in ("comment", "obj_info"):
            continue
        if words[0] == "format":
            fmt = words[1]
        elif words[0] == "element":
            elements.append((words[1], int(words[2]), []))
        elif words[0] == "property":
            if not elements:
                raise VtError(f"{what}: {in_file} has a property before any element")
            if words[1] == "list":
                elements[-1][2].append((words[-1], None))
            elif words[1] in _PLY_TYPES:
                elements[-1][2].append((words[-1], _PLY_TYPES[words[1]]))
            else:
                raise VtError(f"{what}: {in_file} has a property of unknown type {words[1]!r}")
        elif words[0] == "end_header":
            break
    if fmt not in ("ascii", "binary_little_endian", "binary_big_endian"):
        raise VtError(f"{what}: {in_file} has format {fmt!r}")
    return fmt, elements


def load_pointcloud(in_file, with_normals=False):
    """The vertex element's ``x y z`` of a PLY file as [N,3] (load_pointcloud, src/utils/io.py:17-24), in the type the file stores;
    with ``with_normals`` also ``nx ny nz`` (None when the file has none): ``(vertices, normals)``.  Reads ascii and binary files, with
    any further vertex properties and any elements after the vertices (the faces ``Mesh.export`` writes)."""
    what = "load_pointcloud"
    with open(in_file, "rb") as fh:
        fmt, elements = _ply_header(fh, what, in_file)
        if not elements or elements[0][0] != "vertex":
            raise VtError(f"{what}: the first element of {in_file} is not 'vertex'")
        _, count, props = elements[0]
        names = [p[0] for p in props]
        if any(t is None for _, t in props) or not all(c in names for c in "xyz"):
            raise VtError(f"{what}: the vertex element of {in_file} needs scalar properties x, y, z (got {names})")
        if fmt == "ascii":
            rows = [fh.readline().split() for _ in range(count)]
            if any(len(r) != len(props) for r in rows):
                raise VtError(f"{what}: {in_file} has a vertex line without {len(props)} values")
            cols = {name: np.array([r[i] for r in rows], dtype=t) if count else np.zeros(0, dtype=t) for i, (name, t) in enumerate(props)}
        else:
            order = "<" if fmt == "binary_little_endian" else ">"
            rec = np.dtype([(name, order + t) for name, t in props])
            raw = fh.read(count * rec.itemsize)
            if len(raw) != count * rec.itemsize:
                raise VtError(f"{what}: {in_file} ends inside its vertices")
            data = np.frombuffer(raw, dtype=rec)
            cols = {name: data[name].astype(t) for name, t in props}
    vertices = np.stack([cols["x"], cols["y"], cols["z"]], axis=1)
    if not with_normals:
        return vertices
    normals = np.stack([cols["nx"], cols["ny"], cols["nz"]], axis=1) if all(c in cols for c in ("nx", "ny", "nz")) else None
    return vertices, normals


def read_off(file):
    """(vertices, faces) of a triangle mesh in an OFF file as lists of lists, the faces with their leading 3 (read_off,
    src/utils/io.py:27-110).  The counts may stand on the first line, right behind ``OFF`` (some ModelNet files), or on the second."""
    what = "read_off"
    if not os.path.exists(file):
        raise VtError(f"{what}: file {file} not found")
    with open(file, "r") as fh:
        lines = [line.strip() for line in fh.readlines()]
    if not lines or lines[0][:3] not in ("OFF", "off"):
        raise VtError(f"{what}: invalid OFF file {file}")
    if len(lines[0]) > 3:
        counts, start = lines[0][3:].split(), 1
    else:
        counts, start = lines[1].split() if len(lines) > 1 else [], 2
    if len(counts) != 3:
        raise VtError(f"{what}: {file} has no 'vertices faces edges' line")
    n_vertices, n_faces = int(counts[0]), int(counts[1])
    if n_vertices <= 0 or n_faces <= 0 or len(lines) < start + n_vertices + n_faces:
        raise VtError(f"{what}: {file} announces {n_vertices} vertices and {n_faces} faces and has {len(lines) - start} lines for them")
    vertices = []
    for line in lines[start:start + n_vertices]:
        vertex = [float(word) for word in line.split()]
        if len(vertex) != 3:
            raise VtError(f"{what}: {file} has a vertex line without 3 numbers: {line!r}")
        vertices.append(vertex)
    faces = []
    for line in lines[start + n_vertices:start + n_vertices + n_faces]:
        face = [int(word) for word in line.split()]
        if len(face) != 4 or face[0] != 3:
            raise VtError(f"{what}: only triangle meshes are read ({file}: {line!r})")
        if any(not 0 <= index < n_vertices for index in face[1:]):
            raise VtError(f"{what}: {file} has a face with a vertex outside [0, {n_vertices}): {line!r}")
        faces.append(face)
    return vertices, faces
