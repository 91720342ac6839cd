"""A float64 restatement of the normals and values that scikit-image 0.18.3's Lewiner marching cubes returns next to its vertices and
faces (``measure.marching_cubes(vol, level, gradient_direction='ascent')``), which csrc/mc_normals.hip computes on the device.  numpy
only; the lookup tables are read from oracle/mc_tables.h, the classification is oracle/mc_lewiner.c's, restated.

    mc(vol, level=None) -> dict
        verts [V,3] f64 and faces [F,3] i32 numbered as scikit-image numbers them, array-axis order
        normals [V,3] f64    unit, array-axis order; (0,0,0) where the sum is zero or not finite
        values [V] f32       max over the cells that reference the vertex of (cell max - cell min) of vol - level
        n [V]                the references: how many triangle corners name the vertex
        kappa [V]            the cancellation ratio sum |term| / |sum term| (inf where the sum vanishes)
        centre [V] bool      Lewiner's centre vertex of a cell (the ones that do not lie on a lattice edge)
    bound(n, kappa)          the gate |got - ref| <= (n + 6) 2^-24 kappa per component: f32 accumulation of n terms, then a normalisation
    KAPPA_MAX = 2^12         vertices beyond it are checked for finiteness only

The rule (x, y, z are array axes 2, 1, 0; corner k of a cell has offsets CX, CY, CZ[k]):
  - v = vol - level in double; the gradient at a corner is made of the three one-sided differences inside the cell, low minus high:
    G(k) = (v[x=0] - v[x=1], v[y=0] - v[y=1], v[z=0] - v[z=1]) along the three cell edges that meet in k;
  - the quirk: a corner with y = 1 uses the gradient of the corner mirrored in x, G'(x, 1, z) = G(1 - x, 1, z); G' = G elsewhere;
  - every triangle corner that names the vertex on the cell edge (a, b) adds the two terms w_a G'(a) and w_b G'(b), w = 1 / (eps + |v|)
    with eps the double machine epsilon -- the weights of the vertex position.  The count is per triangle corner, not per cell;
  - a triangle corner that names a cell's centre vertex adds, for each of the eight corners k, w_k (G_z(k), G_y(k), 0) in (x, y, z):
    the plain gradient G, its z component in the x slot and nothing in the z slot.  (Fitted on the 197 single-cell fixtures that have
    a centre vertex, then confirmed on the volumes: scikit-image's centre normals have no axis-0 component.);
  - the normal is the normalised sum; kappa is taken over the individual terms (two per reference on an edge, eight at a centre),
    which is how scikit-image adds them into its float32 array: a reference whose two terms cancel each other counts as cancellation.
    n stays the number of references."""
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
EPS = 2.220446049250313e-16
KAPPA_MAX = 2.0 ** 12

CX = (0, 1, 1, 0, 0, 1, 1, 0)
CY = (0, 0, 1, 1, 0, 0, 1, 1)
CZ = (0, 0, 0, 0, 1, 1, 1, 1)
E0 = (0, 1, 2, 3, 4, 5, 6, 7, 0, 1, 2, 3)
E1 = (1, 2, 3, 0, 5, 6, 7, 4, 4, 5, 6, 7)
CORNER = {(CX[k], CY[k], CZ[k]): k for k in range(8)}
MIRROR = tuple(CORNER[(1 - CX[k], CY[k], CZ[k])] if CY[k] == 1 else k for k in range(8))
# the corner pairs (low, high) of the three differences at corner k
GPAIR = tuple(tuple((CORNER[tuple(0 if d == a else c for d, c in enumerate((CX[k], CY[k], CZ[k])))],
                     CORNER[tuple(1 if d == a else c for d, c in enumerate((CX[k], CY[k], CZ[k])))]) for a in range(3)) for k in range(8))

_T = None


def tables():
    global _T
    if _T is None:
        text = open(os.path.join(os.path.dirname(HERE), "oracle", "mc_tables.h")).read()
        rows = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define MC_(\w+)_ROW (\d+)", text)}
        _T = {}
        for m in re.finditer(r"signed char MC_(\w+)\[\d+\] = \{([^}]*)\}", text):
            a = np.array([int(x) for x in m.group(2).split(",")], dtype=np.int64)
            _T[m.group(1)] = a.reshape(-1, rows[m.group(1)]) if rows[m.group(1)] > 1 else a
    return _T


def default_level(vol):
    return 0.5 * float(np.float32(vol.min()) + np.float32(vol.max()))


# ---- the classification of one cell (oracle/mc_lewiner.c) ----------------------------------------------------------------------------
_FACE = {1: (0, 4, 5, 1), 2: (1, 5, 6, 2), 3: (2, 6, 7, 3), 4: (3, 7, 4, 0), 5: (0, 3, 2, 1), 6: (4, 7, 6, 5)}


def _test_face(v, face):
    A, B, C, D = (v[k] for k in _FACE[abs(face)])
    acbd = A * C - B * D
    if abs(acbd) < EPS:
        return face >= 0
    return face * A * acbd >= 0


_P = (0, 1, 2, 3, 4, 5, 6, 7, 0, 1, 2, 3)
_Q = (1, 2, 3, 0, 5, 6, 7, 4, 4, 5, 6, 7)
_B0 = (3, 0, 1, 2, 7, 4, 5, 6, 3, 0, 1, 2)
_B1 = (2, 3, 0, 1, 6, 7, 4, 5, 7, 4, 5, 6)
_C0 = (7, 4, 5, 6, 3, 0, 1, 2, 2, 3, 0, 1)
_C1 = (6, 7, 4, 5, 2, 3, 0, 1, 6, 7, 4, 5)
_D0 = (4, 5, 6, 7, 0, 1, 2, 3, 1, 2, 3, 0)
_D1 = (5, 6, 7, 4, 1, 2, 3, 0, 5, 6, 7, 4)


def _test_interior(v, case, config, subconfig, s):
    T = tables()
    At = Bt = Ct = Dt = 0.0
    if case in (4, 10):
        a = (v[4] - v[0]) * (v[6] - v[2]) - (v[7] - v[3]) * (v[5] - v[1])
        b = v[2] * (v[4] - v[0]) + v[0] * (v[6] - v[2]) - v[1] * (v[7] - v[3]) - v[3] * (v[5] - v[1])
        t = -b / (2 * a + EPS)
        if t < 0 or t > 1:
            return s > 0
        At = v[0] + (v[4] - v[0]) * t
        Bt = v[3] + (v[7] - v[3]) * t
        Ct = v[2] + (v[6] - v[2]) * t
        Dt = v[1] + (v[5] - v[1]) * t
    elif case in (6, 7, 12, 13):
        edge = {6: lambda: T["TEST6"][config][2], 7: lambda: T["TEST7"][config][4], 12: lambda: T["TEST12"][config][3],
                13: lambda: T["TILING13_5_1"][config][subconfig * 18]}[case]()
        if edge < 0 or edge > 11:
            return s < 0
        t = v[_P[edge]] / (v[_P[edge]] - v[_Q[edge]] + EPS)
        At = 0.0
        Bt = v[_B0[edge]] + (v[_B1[edge]] - v[_B0[edge]]) * t
        Ct = v[_C0[edge]] + (v[_C1[edge]] - v[_C0[edge]]) * t
        Dt = v[_D0[edge]] + (v[_D1[edge]] - v[_D0[edge]]) * t
    test = (At >= 0) + 2 * (Bt >= 0) + 4 * (Ct >= 0) + 8 * (Dt >= 0)
    if test in (0, 1, 2, 3, 4, 6, 8, 9, 12):
        return s > 0
    if test == 5 and At * Ct - Bt * Dt < EPS:
        return s > 0
    if test == 10 and At * Ct - Bt * Dt >= EPS:
        return s > 0
    if test in (7, 11, 13, 14, 15):
        return s < 0
    return False


def cell_triangles(v, index):
    """The edge numbers (12: the centre vertex) of the cell's triangle corners, in emission order."""
    T = tables()
    cs, cf = int(T["CASES"][index][0]), int(T["CASES"][index][1])
    row = lambda name, nt, sub=0, stride=0: [int(x) for x in T[name][cf][sub * stride:sub * stride + 3 * nt]]
    tf = lambda name, k: _test_face(v, int(T[name][cf][k]) if T[name].ndim > 1 else int(T[name][cf]))
    ti = lambda name, k, sc=0: _test_interior(v, cs, cf, sc, int(T[name][cf][k]) if T[name].ndim > 1 else int(T[name][cf]))
    if cs == 0:
        return []
    if cs == 1:
        return row("TILING1", 1)
    if cs == 2:
        return row("TILING2", 2)
    if cs == 3:
        return row("TILING3_2", 4) if tf("TEST3", 0) else row("TILING3_1", 2)
    if cs == 4:
        return row("TILING4_1", 2) if ti("TEST4", 0) else row("TILING4_2", 6)
    if cs == 5:
        return row("TILING5", 3)
    if cs == 6:
        if tf("TEST6", 0):
            return row("TILING6_2", 5)
        return row("TILING6_1_1", 3) if ti("TEST6", 1) else row("TILING6_1_2", 9)
    if cs == 7:
        sub = tf("TEST7", 0) + 2 * tf("TEST7", 1) + 4 * tf("TEST7", 2)
        if sub == 0:
            return row("TILING7_1", 3)
        if sub in (1, 2, 4):
            return row("TILING7_2", 5, {1: 0, 2: 1, 4: 2}[sub], 15)
        if sub in (3, 5, 6):
            return row("TILING7_3", 9, {3: 0, 5: 1, 6: 2}[sub], 27)
        return row("TILING7_4_2", 9) if ti("TEST7", 3) else row("TILING7_4_1", 5)
    if cs == 8:
        return row("TILING8", 2)
    if cs == 9:
        return row("TILING9", 4)
    if cs in (10, 12):
        n = str(cs)
        if tf("TEST" + n, 0):
            return row(f"TILING{n}_1_1_", 4) if tf("TEST" + n, 1) else row(f"TILING{n}_2", 8)
        if tf("TEST" + n, 1):
            return row(f"TILING{n}_2_", 8)
        return row(f"TILING{n}_1_1", 4) if ti("TEST" + n, 2) else row(f"TILING{n}_1_2", 8)
    if cs == 11:
        return row("TILING11", 4)
    if cs == 13:
        sub = sum((1 << k) for k in range(6) if tf("TEST13", k))
        sc = int(T["SUBCONFIG13"][sub])
        if sc == 0:
            return row("TILING13_1", 4)
        if sc <= 6:
            return row("TILING13_2", 6, sc - 1, 18)
        if sc <= 18:
            return row("TILING13_3", 10, sc - 7, 30)
        if sc <= 22:
            return row("TILING13_4", 12, sc - 19, 36)
        if sc <= 26:
            if ti("TEST13", 6, sc - 23):
                return row("TILING13_5_1", 6, sc - 23, 18)
            return row("TILING13_5_2", 10, sc - 23, 30)
        if sc <= 38:
            return row("TILING13_3_", 10, sc - 27, 30)
        if sc <= 44:
            return row("TILING13_2_", 6, sc - 39, 18)
        if sc == 45:
            return row("TILING13_1_", 4)
        return []
    if cs == 14:
        return row("TILING14", 4)
    return []


# ---- per cell: gradients, weights, the term of a reference ----------------------------------------------------------------------------
def cell_gradients(v, quirk=True):
    """G' [8,3] (x, y, z components) of a cell with corner values v[8]."""
    g = np.array([[v[lo] - v[hi] for lo, hi in GPAIR[k]] for k in range(8)])
    return g[list(MIRROR)] if quirk else g


def reference_terms(g, plain, w, vi):
    """The summands (x, y, z components) one triangle corner adds to vertex vi of the cell, in the order they are added."""
    if vi == 12:
        return [np.array([w[k] * plain[k][2], w[k] * plain[k][1], 0.0]) for k in range(8)]
    a, b = E0[vi], E1[vi]
    return [w[a] * g[a], w[b] * g[b]]


def _key(x, y, z, vi):
    """The lattice edge (or cell centre) of vertex vi of cell (x, y, z): (x, y, z, direction)."""
    if vi == 12:
        return (x, y, z, 3)
    a, b = E0[vi], E1[vi]
    d = 0 if CX[a] != CX[b] else (1 if CY[a] != CY[b] else 2)
    return (x + min(CX[a], CX[b]), y + min(CY[a], CY[b]), z + min(CZ[a], CZ[b]), d)


def mc(vol, level=None, quirk=True):
    vol = np.ascontiguousarray(vol, dtype=np.float32)
    if level is None:
        level = default_level(vol)
    n0, n1, n2 = vol.shape
    val = vol.astype(np.float64) - float(level)
    ids, verts, faces, sums, norms, refs, values, centre = {}, [], [], [], [], [], [], []
    for z in range(n0 - 1):
        for y in range(n1 - 1):
            for x in range(n2 - 1):
                v = np.array([val[z + CZ[k], y + CY[k], x + CX[k]] for k in range(8)])
                index = sum(1 << k for k in range(8) if v[k] > 0.0)
                if index == 0 or index == 255:
                    continue
                tri = cell_triangles(v, index)
                if not tri:
                    continue
                g, plain = cell_gradients(v, quirk), cell_gradients(v, False)
                w = 1.0 / (EPS + np.abs(v))
                span = np.float32(v.max() - v.min())
                for vi in tri:
                    key = _key(x, y, z, vi)
                    i = ids.get(key)
                    if i is None:
                        i = ids[key] = len(verts)
                        ks = range(8) if vi == 12 else (E0[vi], E1[vi])
                        ff = sum(w[k] for k in ks)
                        verts.append((z + sum(CZ[k] * w[k] for k in ks) / ff, y + sum(CY[k] * w[k] for k in ks) / ff,
                                      x + sum(CX[k] * w[k] for k in ks) / ff))
                        sums.append(np.zeros(3)); norms.append(0.0); refs.append(0); values.append(np.float32(0)); centre.append(vi == 12)
                    faces.append(i)
                    for t in reference_terms(g, plain, w, vi):
                        sums[i] = sums[i] + t
                        norms[i] += float(np.sqrt((t * t).sum()))
                    refs[i] += 1
                    values[i] = max(values[i], span)
    V = len(verts)
    s = np.array(sums).reshape(V, 3)[:, ::-1]                                # (x, y, z) -> array-axis order
    with np.errstate(all="ignore"):
        length = np.sqrt((s * s).sum(1))
        ok = np.isfinite(length) & (length > 0)
        normals = np.where(ok[:, None], s / np.where(ok, length, 1.0)[:, None], 0.0)
        kappa = np.where(ok, np.array(norms).reshape(V) / np.where(ok, length, 1.0), np.inf)
    return {"verts": np.array(verts).reshape(V, 3), "faces": np.array(faces, dtype=np.int32).reshape(-1, 3), "normals": normals,
            "values": np.array(values, dtype=np.float32).reshape(V), "n": np.array(refs, dtype=np.int64).reshape(V), "kappa": kappa,
            "centre": np.array(centre, dtype=bool).reshape(V), "level": float(level)}


def bound(n, kappa):
    return (np.asarray(n) + 6) * 2.0 ** -24 * np.asarray(kappa)
