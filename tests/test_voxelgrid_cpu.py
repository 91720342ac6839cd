"""CPU: the public face of vtaco_amd.utils.voxels against the reference's (g27_voxelgrid.npz, ``ref.*``: recorded from the real
src/utils/voxels.py and binvox_rw.py) -- signatures, refusals and messages -- and the helpers that are torch ops, on CPU tensors.  The
voxelisers themselves need the device: tests/test_voxelize_gpu.py."""
import inspect
import io
import types

import numpy as np
import pytest
import torch

from conftest import load_golden

TAGS = ("r4", "r6", "r9", "torus")


@pytest.fixture(scope="module")
def z():
    return load_golden("g27_voxelgrid.npz")[0]


def _grid(z, tag):
    from vtaco_amd.utils.voxels import VoxelGrid
    return VoxelGrid(torch.from_numpy(z[f"ref.{tag}.vol"]), z[f"ref.{tag}.loc"], float(z[f"ref.{tag}.scale"]))


def test_signatures_are_the_references(z):
    from vtaco_amd.utils import voxels
    mine = {"VoxelGrid.__init__": voxels.VoxelGrid.__init__, "VoxelGrid.from_mesh": voxels.VoxelGrid.from_mesh.__func__,
            "VoxelGrid.down_sample": voxels.VoxelGrid.down_sample, "VoxelGrid.contains": voxels.VoxelGrid.contains,
            "voxelize_ray": voxels.voxelize_ray, "voxelize_fill": voxels.voxelize_fill, "check_voxel_occupied": voxels.check_voxel_occupied,
            "check_voxel_unoccupied": voxels.check_voxel_unoccupied, "check_voxel_boundary": voxels.check_voxel_boundary}
    for name, fn in mine.items():
        assert str(inspect.signature(fn)) == str(z["ref.sig." + name]), name
    # to_mesh: the reference's (self) plus the one keyword that makes the result exportable
    assert str(z["ref.sig.VoxelGrid.to_mesh"]) == "(self)" and str(inspect.signature(voxels.VoxelGrid.to_mesh)) == "(self, triangles=False)"
    assert str(inspect.signature(voxels.voxelize_surface)) == "(mesh, resolution)"
    assert str(inspect.signature(voxels.voxelize_interior)) == "(mesh, resolution, rule='parity')"
    assert isinstance(voxels.VoxelGrid.resolution, property)


def test_non_cubic_volume_is_refused():
    from vtaco_amd.utils.voxels import VoxelGrid
    for shape in ((4, 4, 5), (4, 4), (2, 4, 4, 4)):
        with pytest.raises(ValueError):
            VoxelGrid(torch.zeros(shape, dtype=torch.bool))
        with pytest.raises(ValueError):
            VoxelGrid(np.zeros(shape, dtype=bool))


def test_value_error_messages_are_the_references(z):
    from vtaco_amd.utils import voxels
    with pytest.raises(ValueError) as e:
        _grid(z, "r4").down_sample(3)
    assert str(e.value) == str(z["ref.msg.down_sample"])
    outside = np.array([[-0.5, -0.1, -0.1], [0.1, 0.1, 0.1], [0.0, 0.1, 0.0]], dtype=np.float32)        # touches the cube's face
    for mesh in ((outside, np.array([[0, 1, 2]])), types.SimpleNamespace(vertices=torch.from_numpy(outside), faces=torch.tensor([[0, 1, 2]]))):
        with pytest.raises(ValueError) as e:
            voxels.voxelize_fill(mesh, 8)
        assert str(e.value) == str(z["ref.msg.fill"])
    with pytest.raises(ValueError):
        voxels._interior(None, None, 8, None, None, rule="bogus")


def test_ops_voxelize_is_a_submodule_and_ops_gained_no_name():
    from vtaco_amd import ops
    assert isinstance(ops.voxelize, types.ModuleType) and ops.voxelize.__name__ == "vtaco_amd.ops.voxelize"
    for name in ("surface", "interior", "fill"):
        assert inspect.isfunction(getattr(ops.voxelize, name)) and not hasattr(ops, name)
    assert not hasattr(ops, "MAX_RES") and "voxelize" in ops.__doc__
    import test_ops_surface_cpu as surface
    assert surface.NEW_PUBLIC == {"decode_lattice_form", "LATTICE_FORMS", "decode_wide_form", "WIDE_KINDS", "fusion_plan"}          # the decoders' and the fuser's form queries; nothing of voxelize
    surface.test_no_other_public_name_appeared()                   # the package's public names are still the recorded ones
    surface.test_every_recorded_name_is_there_unchanged()
    from vtaco_amd import _lib
    for name in ("vt_voxelize_surface", "vt_voxelize_interior", "vt_voxel_fill"):
        assert name in _lib.SIGNATURES


def test_launchers_refuse_before_any_launch():
    from vtaco_amd import ops
    from vtaco_amd._lib import VtError
    v, f = torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32)
    for fn in (ops.voxelize.surface, ops.voxelize.interior):
        with pytest.raises(VtError):
            fn(v, f, 8)                                             # CPU tensors
    with pytest.raises(VtError):
        ops.voxelize.fill(torch.zeros(4, 4, 5, dtype=torch.uint8))


@pytest.mark.parametrize("tag", TAGS)
def test_helpers_on_cpu_tensors_equal_the_reference(z, tag):
    from vtaco_amd.utils import voxels
    g = _grid(z, tag)
    assert g.resolution == z[f"ref.{tag}.vol"].shape[0]
    mesh = g.to_mesh()
    assert mesh.vertices.dtype == torch.float64 and mesh.faces.dtype == torch.int64
    assert np.array_equal(mesh.vertices.numpy(), z[f"ref.{tag}.vertices"])              # 0 abs in float64
    assert np.array_equal(mesh.faces.numpy(), z[f"ref.{tag}.quads"])
    tri = g.to_mesh(triangles=True).faces.numpy()
    q = z[f"ref.{tag}.quads"]
    assert np.array_equal(tri, np.stack([q[:, [0, 1, 2]], q[:, [0, 2, 3]]], axis=1).reshape(-1, 3))
    for key in ("", "_f32"):
        assert np.array_equal(g.contains(z[f"ref.{tag}.points{key}"]).numpy(), z[f"ref.{tag}.contains{key}"])
        assert np.array_equal(g.contains(torch.from_numpy(z[f"ref.{tag}.points{key}"]).reshape(2, -1, 3)).numpy().reshape(-1), z[f"ref.{tag}.contains{key}"])
    for factor in (2, 3):
        if g.resolution % factor == 0:
            d = g.down_sample(factor)
            assert np.array_equal(d.data.numpy(), z[f"ref.{tag}.down{factor}"]) and d.scale == g.scale and np.array_equal(d.loc, g.loc)
    lattice = z[f"ref.{tag}.lattice"]
    for name in ("occupied", "unoccupied", "boundary"):
        fn = getattr(voxels, "check_voxel_" + name)
        assert np.array_equal(fn(torch.from_numpy(lattice)).numpy(), z[f"ref.{tag}.{name}"])
        assert np.array_equal(fn(lattice).numpy(), z[f"ref.{tag}.{name}"])


@pytest.mark.parametrize("tag", TAGS + ("runs",))
def test_binvox_write_bytes_equal_the_references(z, tag, tmp_path):
    from vtaco_amd.data import VoxelsField, binvox
    vol = z[f"ref.{tag}.vol"]
    n = vol.shape[0]
    loc = [float(x) for x in z[f"ref.{tag}.loc"]] if tag != "runs" else [0.0, 0.0, 0.0]
    scale = float(z[f"ref.{tag}.scale"]) if tag != "runs" else 1.0
    buf = io.BytesIO()
    binvox.write(binvox.Voxels(vol, [n] * 3, loc, scale), buf)
    assert buf.getvalue() == z[f"ref.{tag}.binvox"].tobytes()
    if tag != "runs":
        from vtaco_amd.utils.voxels import VoxelGrid
        VoxelGrid(torch.from_numpy(vol), z[f"ref.{tag}.loc"], scale).write_binvox(str(tmp_path / "model.binvox"))
        assert (tmp_path / "model.binvox").read_bytes() == z[f"ref.{tag}.binvox"].tobytes()
    else:
        (tmp_path / "model.binvox").write_bytes(buf.getvalue())
    back = VoxelsField("model.binvox").load(str(tmp_path), 0, 0)
    assert back.dtype == np.float32 and np.array_equal(back, vol.astype(np.float32))
