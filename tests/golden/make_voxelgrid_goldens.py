#!/usr/bin/env python3
"""Generate tests/golden/g27_voxelgrid.npz.

    python tests/golden/make_voxelgrid_goldens.py

ref.*  from the REAL reference (needs it mounted read-only where make_goldens.py expects it): src/utils/voxels.py and binvox_rw.py are
       loaded through importlib, with stand-ins only for what is not installed (trimesh, skimage.measure.block_reduce, np.bool; the
       fixture records which).  VoxelGrid.to_mesh / contains / down_sample, the three check_voxel_*, binvox_rw.write's bytes, the
       signatures and the ValueError messages, on seeded random volumes at res 4, 6, 9 and on one ray-voxelised torus.
def.*  from tests/voxelize_ref.py (the float64 restatement of voxelize.hip's definitions; the reference never defines its voxelisers):
       packed surface / interior / ray / fill occupancies of the committed cases, one clipped case and one grid-spanning triangle.
No reference code is stored: arrays, byte strings and signature strings only.
"""
import importlib.util
import inspect
import io
import os
import sys
import types

import numpy as np
from scipy import ndimage

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_goldens as mg  # noqa: E402
import voxelize_ref as R  # noqa: E402


class _Trimesh:
    def __init__(self, vertices, faces, process=False):
        self.vertices, self.faces = np.asarray(vertices), np.asarray(faces)


def _block_reduce(image, block_size, func):
    shape = []
    for n, b in zip(image.shape, block_size):
        shape += [n // b, b]
    return func(image.reshape(shape), axis=(1, 3, 5))


def _load_reference():
    stubbed = []
    mg._install_stubs()
    for name, attrs in (("trimesh", dict(Trimesh=_Trimesh)), ("skimage", {}), ("skimage.measure", dict(block_reduce=_block_reduce))):
        try:
            importlib.import_module(name)
        except ImportError:
            m = types.ModuleType(name)
            m.__dict__.update(attrs)
            sys.modules[name] = m
            stubbed.append(name)
    if not hasattr(np, "bool"):
        np.bool = np.bool_
        stubbed.append("np.bool")
    mods = []
    for name in ("voxels", "binvox_rw"):
        spec = importlib.util.spec_from_file_location("ref_" + name, os.path.join(mg.REF, "src", "utils", name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mods.append(mod)
    return mods[0], mods[1], stubbed


class _TextSink:
    """binvox_rw.write writes str pieces (one chr per byte): collect them as latin-1 bytes."""

    def __init__(self):
        self.buf = io.BytesIO()

    def write(self, s):
        self.buf.write(s.encode("latin-1"))


def _probe_points(rng, res, loc, scale):
    """Points inside the grid, and points within one voxel outside each of its six faces (float64 [N,3])."""
    inside = (rng.rand(64, 3) - 0.5) * 0.98
    near = []
    for axis in range(3):
        for sign in (-1, 1):
            p = (rng.rand(12, 3) - 0.5) * 0.98
            p[:, axis] = sign * (0.5 + rng.rand(12) / res)
            near.append(p)
    return np.concatenate([inside] + near) * scale + np.asarray(loc)


def main():
    voxels, binvox_rw, stubbed = _load_reference()
    out = {"ref.stubbed": np.array(stubbed, dtype=str)}
    sig = {"VoxelGrid.__init__": voxels.VoxelGrid.__init__, "VoxelGrid.from_mesh": voxels.VoxelGrid.from_mesh.__func__,
           "VoxelGrid.down_sample": voxels.VoxelGrid.down_sample, "VoxelGrid.to_mesh": voxels.VoxelGrid.to_mesh,
           "VoxelGrid.contains": voxels.VoxelGrid.contains, "voxelize_ray": voxels.voxelize_ray, "voxelize_fill": voxels.voxelize_fill,
           "check_voxel_occupied": voxels.check_voxel_occupied, "check_voxel_unoccupied": voxels.check_voxel_unoccupied,
           "check_voxel_boundary": voxels.check_voxel_boundary}
    for name, fn in sig.items():
        out["ref.sig." + name] = np.array(str(inspect.signature(fn)))

    volumes = {}
    for res, seed in ((4, 40), (6, 60), (9, 90)):
        rng = np.random.RandomState(seed)
        volumes[f"r{res}"] = (rng.rand(res, res, res) < 0.4, rng.randn(3) * 0.2, float(0.7 + rng.rand()))
    v, f = R.CASES["torus16x8"][0]()
    loc, scale = R.default_frame(v)
    volumes["torus"] = (R.ray(v, f, 16, loc, scale), loc, scale)
    for tag, (vol, loc, scale) in volumes.items():
        res = vol.shape[0]
        grid = voxels.VoxelGrid(vol, loc, scale)
        mesh = grid.to_mesh()
        rng = np.random.RandomState(res + 7)
        pts = _probe_points(rng, res, loc, scale)
        out.update({f"ref.{tag}.vol": vol, f"ref.{tag}.loc": np.asarray(loc, dtype=np.float64), f"ref.{tag}.scale": np.float64(scale),
                    f"ref.{tag}.vertices": mesh.vertices.astype(np.float64), f"ref.{tag}.quads": mesh.faces.astype(np.int64),
                    f"ref.{tag}.points": pts, f"ref.{tag}.contains": grid.contains(pts),
                    f"ref.{tag}.points_f32": pts.astype(np.float32), f"ref.{tag}.contains_f32": grid.contains(pts.astype(np.float32))})
        for factor in (2, 3):
            if res % factor == 0:
                out[f"ref.{tag}.down{factor}"] = grid.down_sample(factor).data
        lattice = np.random.RandomState(res + 11).rand(2, res, res, res) < 0.6
        out[f"ref.{tag}.lattice"] = lattice
        out[f"ref.{tag}.occupied"] = voxels.check_voxel_occupied(lattice)
        out[f"ref.{tag}.unoccupied"] = voxels.check_voxel_unoccupied(lattice)
        out[f"ref.{tag}.boundary"] = voxels.check_voxel_boundary(lattice)
        sink = _TextSink()
        binvox_rw.write(binvox_rw.Voxels(vol.astype(np.uint8), [res] * 3, [float(x) for x in loc], float(scale), "xyz"), sink)
        out[f"ref.{tag}.binvox"] = np.frombuffer(sink.buf.getvalue(), dtype=np.uint8)
    # a run of exactly 255 equal voxels followed by another run, and runs longer than 255
    vol = np.zeros((8, 8, 8), dtype=bool)
    vol.reshape(-1)[255:300] = True
    sink = _TextSink()
    binvox_rw.write(binvox_rw.Voxels(np.transpose(vol, (0, 2, 1)).astype(np.uint8), [8] * 3, [0.0, 0.0, 0.0], 1.0, "xyz"), sink)
    out["ref.runs.vol"] = np.transpose(vol, (0, 2, 1))
    out["ref.runs.binvox"] = np.frombuffer(sink.buf.getvalue(), dtype=np.uint8)
    # the two ValueError messages
    try:
        voxels.VoxelGrid(volumes["r4"][0]).down_sample(3)
    except ValueError as e:
        out["ref.msg.down_sample"] = np.array(str(e))
    try:
        voxels.voxelize_fill(types.SimpleNamespace(bounds=np.array([[-0.5, -0.1, -0.1], [0.1, 0.1, 0.1]])), 8)
    except ValueError as e:
        out["ref.msg.fill"] = np.array(str(e))

    # ---- def.*: the restatement ----
    cases = {name: (mk(), res, None) for name, (mk, res) in R.CASES.items()}
    v, f = R.CASES["torus24x12"][0]()
    loc, scale = R.default_frame(v)
    cases["clipped"] = ((v, f), 33, (loc + np.array([0.30, -0.11, 0.07]) * scale, scale * 0.8))
    v, f = R.box()
    cases["box"] = ((v, f), 16, (np.zeros(3), 1.0))
    margins = {}
    for name, ((v, f), res, frame) in cases.items():
        loc, scale = R.default_frame(v) if frame is None else frame
        s, ms = R.surface(v, f, res, loc, scale)
        i, me, mc = R.interior(v, f, res, loc, scale)
        margins[name] = (ms, me, mc)
        out.update({f"def.{name}.verts": v, f"def.{name}.faces": f, f"def.{name}.res": np.int64(res), f"def.{name}.loc": np.asarray(loc, dtype=np.float64),
                    f"def.{name}.scale": np.float64(scale), f"def.{name}.surface": np.packbits(s), f"def.{name}.interior": np.packbits(i),
                    f"def.{name}.ray": np.packbits(s | i), f"def.{name}.fill": np.packbits(ndimage.binary_fill_holes(s)),
                    f"def.{name}.margins": np.array([ms, me, mc])})
        print(f"{name}: res {res}, surface {s.sum()}, interior {i.sum()}, ray {(s | i).sum()}, margins {ms:.2e} {me:.2e} {mc:.2e}")
    v = np.array([[-0.93, -0.71, -0.38], [1.07, -0.52, 0.29], [0.04, 1.13, 0.46]], dtype=np.float32)
    f = np.array([[0, 1, 2]], dtype=np.int64)
    s, ms = R.surface(v, f, 24)
    print(f"spanning triangle: surface {s.sum()}, margin {ms:.2e}")
    out.update({"def.span.verts": v, "def.span.faces": f, "def.span.res": np.int64(24), "def.span.loc": np.zeros(3), "def.span.scale": np.float64(1.0),
                "def.span.surface": np.packbits(s), "def.span.margins": np.array([ms])})
    for name in ("clipped", "span"):
        assert min(margins.get(name, (ms,))) >= 1e-6, name
    mg._save("g27_voxelgrid.npz", **out)


if __name__ == "__main__":
    main()
