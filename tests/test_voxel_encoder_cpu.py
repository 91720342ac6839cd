"""CPU: the voxel-input route's host side -- the encoder registry and state_dict keys, the binvox reader and VoxelsField against the
reference-written fixture, the config factories, the per-axis cell tables against the oracle's coordinate arithmetic, and the float64
statement of tests/voxel_encoder_ref.py against the reference's own outputs and gradients (tests/golden/g25_voxel_encoder.npz)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import voxel_encoder_ref as ref
from conftest import GOLDEN, load_golden, sub_sd

FORMS = {"grid": dict(grid_resolution=8, plane_type="grid"),
         "planes": dict(plane_resolution=8, plane_type=["xz", "xy", "yz"]),
         "grid_unet": dict(grid_resolution=8, plane_type="grid", unet3d=True,
                           unet3d_kwargs=dict(num_levels=2, f_maps=8, in_channels=32, out_channels=32)),
         "k1": dict(grid_resolution=8, plane_type="grid", kernel_size=1)}


def _cfg(**data):
    d = {"input_type": "voxels", "voxels_file": "model.binvox", "points_file": None, "points_iou_file": None, "dim": 3, "padding": 0.1}
    d.update(data)
    return {"data": d}


def test_registry_and_state_dict_keys():
    from vtaco_amd.encoder import encoder_dict
    _, sd = load_golden("g25_voxel_encoder.npz")
    for tag, kw in FORMS.items():
        enc = encoder_dict["voxel_simple_local"](dim=3, c_dim=32, padding=0.1, **kw)
        want = sub_sd(sd, tag + ".")
        assert sorted(enc.state_dict()) == sorted(want), tag
        enc.load_state_dict(want, strict=True)
        assert set(k.split(".")[0] for k in want) <= {"conv_in", "unet", "unet3d"}
    # 'grid' takes precedence over planes named next to it (voxels.py:110-118)
    assert encoder_dict["voxel_simple_local"](c_dim=32, grid_resolution=8, plane_type=["xz", "grid"]).planes == ["grid"]


def test_cpu_input_is_refused():
    from vtaco_amd._lib import VtError
    from vtaco_amd.encoder import encoder_dict
    enc = encoder_dict["voxel_simple_local"](c_dim=32, grid_resolution=8, plane_type="grid")
    with pytest.raises(VtError, match="HIP device"):
        enc(torch.zeros(1, 4, 4, 4))


def test_binvox_reader_and_field_reproduce_the_reference_array():
    from vtaco_amd.data import VoxelsField, binvox
    a, _ = load_golden("g25_voxel_encoder.npz")
    with open(os.path.join(GOLDEN, "g25_model.binvox"), "rb") as f:
        vox = binvox.read_as_3d_array(f)
    assert vox.dims == [8, 8, 8] and vox.translate == [0.0, 0.0, 0.0] and vox.scale == 1.0
    assert vox.data.dtype == bool and np.array_equal(vox.data.astype(np.uint8), a["binvox.array"])
    with open(os.path.join(GOLDEN, "g25_model.binvox"), "rb") as f:
        raw = binvox.read_as_3d_array(f, fix_coords=False)
    assert np.array_equal(raw.data.transpose(0, 2, 1), vox.data) and not np.array_equal(raw.data, vox.data)
    field = VoxelsField("g25_model.binvox")
    got = field.load(GOLDEN, 0, 0)
    assert got.dtype == np.float32 and np.array_equal(got, a["binvox.array"].astype(np.float32))
    assert field.check_complete(["g25_model.binvox", "points.npz"]) and not field.check_complete(["points.npz"])
    assert np.array_equal(VoxelsField("g25_model.binvox", transform=lambda v: 1 - v).load(GOLDEN, 0, 0), 1 - got)


def test_binvox_reader_refuses_broken_files(tmp_path):
    from vtaco_amd.data import binvox
    good = open(os.path.join(GOLDEN, "g25_model.binvox"), "rb").read()
    for name, blob in (("magic", b"#notvox 1\n" + good[10:]), ("short", good[:-2]), ("odd", good[:-1])):
        p = tmp_path / name
        p.write_bytes(blob)
        with open(p, "rb") as f, pytest.raises(IOError):
            binvox.read_as_3d_array(f)


def test_config_factories_build_the_voxel_fields():
    from vtaco_amd import config
    from vtaco_amd._lib import VtError
    from vtaco_amd.conv_onet import config as conv_config
    from vtaco_amd.data import VoxelsField
    field = config.get_inputs_field("train", _cfg())
    assert isinstance(field, VoxelsField) and field.file_name == "model.binvox" and field.transform is None
    for mode in ("val", "test", "vis"):
        fields = conv_config.get_data_fields(mode, _cfg(input_type="pointcloud"))
        assert isinstance(fields["voxels"], VoxelsField) and fields["voxels"].file_name == "model.binvox"
    assert "voxels" not in conv_config.get_data_fields("train", _cfg(input_type="pointcloud"))
    assert "voxels" not in conv_config.get_data_fields("val", _cfg(input_type="pointcloud", voxels_file=None))
    with pytest.raises(VtError):                                      # crop mode stays refused
        conv_config.get_data_fields("val", _cfg(input_type="pointcloud_crop"))
    with pytest.raises(NotImplementedError):
        config.get_inputs_field("train", _cfg(input_type="pointcloud_crop"))


@pytest.mark.parametrize("R", [4, 8, 32, 64])
@pytest.mark.parametrize("dims", [(2, 2, 2), (5, 5, 5), (32, 32, 32), (33, 33, 33), (64, 64, 64), (5, 33, 2)])
def test_axis_tables_expand_to_the_oracles_indices(dims, R):
    """a1[i1] + R (a2[i2] + R a3[i3]) (and the plane pairs) over the whole volume equal coordinate2index(normalize_*(p)) on the voxel
    coordinates; the [lo, hi) ranges are the tables' pre-images."""
    from vtaco_amd.ops import voxel_encoder as ve
    for kind, names in (("grid", ("grid",)), ("plane", ref.PLANES)):
        a = [ve.axis_index(d, R, 0.1, kind) for d in dims]
        i1, i2, i3 = torch.meshgrid(*[torch.arange(d) for d in dims], indexing="ij")
        per = [a[0][i1].reshape(-1), a[1][i2].reshape(-1), a[2][i3].reshape(-1)]
        for name in names:
            want, _ = ref.cell_ids(dims, R, 0.1, name)
            if name == "grid":
                got = per[0] + R * (per[1] + R * per[2])
            else:
                u, v = {"xz": (0, 2), "xy": (0, 1), "yz": (1, 2)}[name]
                got = per[u] + R * per[v]
            assert np.array_equal(got.numpy(), want), (kind, name)
        t = ve.Tables(dims, R, 0.1, "cpu", kind)
        assert t.index.dtype == torch.int32 and torch.equal(t.index.long(), torch.cat(a))
        rng = t.ranges.reshape(3, R, 2).long()
        for k in range(3):
            for r in range(R):
                lo, hi = int(rng[k, r, 0]), int(rng[k, r, 1])
                assert torch.equal(torch.nonzero(a[k] == r).reshape(-1), torch.arange(lo, hi))


def test_float64_statement_agrees_with_the_reference_outputs_and_gradients():
    a, sd = load_golden("g25_voxel_encoder.npz")
    x = a["x"]
    for tag in ("grid", "planes", "k1"):
        w, b = sd[f"{tag}.conv_in.weight"].numpy(), sd[f"{tag}.conv_in.bias"].numpy()
        names = ref.PLANES if tag == "planes" else ("grid",)
        out, bound, _ = ref.forward(x, w, b, 8, 0.1, names)
        h32, _, _ = ref.host32(x, w, b, 8, 0.1, names)
        for n in names:
            want = a[f"{tag}.fea.{n}"]
            assert out[n].shape == want.shape
            assert np.abs(out[n] - want).max() <= 1e-5 and np.abs(h32[n] - want).max() <= 1e-5, (tag, n)
            assert np.all(out[n][bound[n] == 0] == 0)
        if tag == "k1":
            continue
        up = {n: a[f"{tag}.up.{n}"] for n in names}
        dw, db, dwb, dbb = ref.backward(x, w, b, 8, 0.1, up)
        _, hw, hb = ref.host32(x, w, b, 8, 0.1, names, up)
        for got, h, want in ((dw, hw, a[f"{tag}.grad.weight"]), (db, hb, a[f"{tag}.grad.bias"])):
            tol = 1e-5 * max(1.0, float(np.abs(want).max()))
            assert got.shape == want.shape and np.abs(got - want).max() <= tol and np.abs(h - want).max() <= tol, tag
        assert np.all(dwb >= np.abs(dw) - 1e-12) and np.all(dbb >= np.abs(db) - 1e-12)


def test_get_dataset_reads_a_voxel_dataset(tmp_path):
    """config.get_dataset with ``input_type: voxels``: the sample's 'inputs' (and, for val, 'voxels') are the volume, batched [B,D,D,D]."""
    import shutil
    from vtaco_amd import config, data
    a, _ = load_golden("g25_voxel_encoder.npz")
    for model in ("m0", "m1"):
        os.makedirs(tmp_path / "cat" / model)
        shutil.copy(os.path.join(GOLDEN, "g25_model.binvox"), tmp_path / "cat" / model / "model.binvox")
    for split in ("train", "val"):
        (tmp_path / "cat" / f"{split}.lst").write_text("m0\nm1\n")
    cfg = _cfg(path=str(tmp_path), classes=["cat"], dataset="Shapes3D", train_split="train", val_split="val", test_split="val")
    cfg["method"] = "vtaco"
    train, val = config.get_dataset("train", cfg), config.get_dataset("val", cfg)
    assert len(train) == len(val) == 2 and set(train[0]) == {"inputs"} and set(val[0]) == {"inputs", "voxels"}
    assert train.test_model_complete("cat", "m0")
    batch = data.collate_remove_none([val[0], val[1]])
    want = torch.from_numpy(a["binvox.array"].astype(np.float32))
    assert batch["inputs"].shape == (2, 8, 8, 8) and batch["inputs"].dtype == torch.float32
    assert torch.equal(batch["inputs"][1], want) and torch.equal(batch["voxels"][0], want)
