"""CPU: the MISE refinement contract (vtaco_amd/csrc/mise.hip) restated in numpy reproduces the reference's MultiGridExtractor
(g22_mise.npz, tests/golden/make_mise_goldens.py) exactly; Generator3D's ``extraction`` setting and its refusals."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

FIELDS = ("sphere", "needle", "noisy")


def g22():
    return np.load(os.path.join(GOLDEN, "g22_mise.npz"))


def side(v, level):
    """Marching cubes' predicate (mc.hip): (double)v - level > 0."""
    return (v.astype(np.float64) - level) > 0


def active_voxels(values, level, rule="mc"):
    s = side(values, level) if rule == "mc" else values < level          # "ref": the reference's occupancy, values < threshold
    corners = [s[a:a + s.shape[0] - 1, b:b + s.shape[1] - 1, c:c + s.shape[2] - 1] for a in (0, 1) for b in (0, 1) for c in (0, 1)]
    return np.logical_or.reduce(corners) & ~np.logical_and.reduce(corners)


def refine(values, known, level):
    """One step of the contract: (fine values, fine known, sorted query ids of the fine lattice)."""
    nc = values.shape[0]
    nf = 2 * nc - 1
    act = active_voxels(values, level)
    idx = np.arange(nf) // 2
    fine = values[np.ix_(idx, idx, idx)].copy()                          # nearest coarse: i // 2 per axis
    fk = np.zeros((nf,) * 3, dtype=bool)
    fk[::2, ::2, ::2] = known                                            # a coarse point's fine copy is known if it was
    vidx = np.arange(nf - 1) // 2
    fine_act = act[np.ix_(vidx, vidx, vidx)]                             # a fine voxel is active when its parent is
    corner = np.zeros((nf,) * 3, dtype=bool)
    for a in (0, 1):
        for b in (0, 1):
            for c in (0, 1):
                corner[a:a + nf - 1, b:b + nf - 1, c:c + nf - 1] |= fine_act
    q = np.flatnonzero((corner & ~fk).ravel()).astype(np.int32)
    return fine, fk, q


def restate(table, r0, steps, level=0.0):
    """The whole extraction with a table lookup as the field: (queries per level, values, known)."""
    n = table.shape[0]
    nc = r0 + 1
    s = (n - 1) // r0
    values = table[::s, ::s, ::s].copy()
    known = np.ones_like(values, dtype=bool)
    queries = [np.arange(nc ** 3, dtype=np.int32)]
    for k in range(1, steps + 1):
        values, known, q = refine(values, known, level)
        nk = values.shape[0]
        s = (n - 1) // (nk - 1)
        x, y, z = np.unravel_index(q, (nk,) * 3)
        values.reshape(-1)[q] = table[x * s, y * s, z * s]
        known.reshape(-1)[q] = True
        queries.append(q)
    return queries, values, known


@pytest.mark.parametrize("name", FIELDS)
def test_contract_reproduces_the_reference_multigrid_extractor(name):
    z = g22()
    r0, steps = (int(v) for v in z[f"{name}.r0_steps"])
    queries, values, known = restate(z[f"{name}.table"], r0, steps)
    assert len(queries) == steps + 1
    for k, q in enumerate(queries):
        assert np.array_equal(q, z[f"{name}.q{k}"]), (name, k)
    assert np.array_equal(known, z[f"{name}.known"].astype(bool))
    assert np.array_equal(values.view(np.uint32), z[f"{name}.values"].view(np.uint32))
    assert sum(map(len, queries)) < 0.5 * values.size                    # the point of the exercise


@pytest.mark.parametrize("name", FIELDS)
def test_marching_cubes_rule_and_reference_rule_agree_without_ties(name):
    z = g22()
    table = z[f"{name}.table"]
    assert not np.any(table == 0.0)
    for vals in (z[f"{name}.values"], table, table[::2, ::2, ::2], table[::4, ::4, ::4]):
        assert np.array_equal(active_voxels(vals, 0.0, "mc"), active_voxels(vals, 0.0, "ref"))
    # ... and they part where a value sits exactly on the level: (double)0 - 0 > 0 is false, 0 < 0 is false as well, so a voxel
    # with corners {0, -1} is active under the reference's rule only
    tie = -np.ones((2, 2, 2), dtype=np.float32)
    tie[0, 0, 0] = 0.0
    assert not active_voxels(tie, 0.0, "mc")[0, 0, 0] and active_voxels(tie, 0.0, "ref")[0, 0, 0]


def test_the_needle_is_missed_by_the_coarse_level():
    """The thin feature: part of it is positive on the finest lattice but never queried (MISE's known limitation)."""
    z = g22()
    table, values, known = z["needle.table"], z["needle.values"], z["needle.known"].astype(bool)
    missed = (table > 0) & (values < 0)
    assert missed.sum() > 0 and not np.any(missed & known)


class _Model(torch.nn.Module):
    def __init__(self, decoder):
        super().__init__()
        self.decoder = decoder


def test_generator_extraction_setting_and_refusals():
    from vtaco_amd._lib import VtError
    from vtaco_amd.conv_onet.generation import Generator3D
    from vtaco_amd.conv_onet.models import decoder_dict
    dec = decoder_dict["simple_local"](dim=3, c_dim=32, hidden_size=32)
    assert Generator3D(_Model(dec)).extraction == "dense"
    gen = Generator3D(_Model(dec), extraction="mise", threshold=0.5, decode_precision="f32")   # (no range guard: no device needed)
    assert gen.extraction == "mise" and gen.mise_level() == 0.0
    assert abs(Generator3D(_Model(dec), extraction="mise", threshold=0.2).mise_level() - np.log(0.25)) < 1e-15
    with pytest.raises(VtError, match="extraction"):
        Generator3D(_Model(dec), extraction="octree")
    att = decoder_dict["attention_local"](dim=3, c_dim=32, hidden_size=32)
    with pytest.raises(VtError, match="attention"):
        Generator3D(_Model(att), extraction="mise")
    Generator3D(_Model(att))                                             # dense keeps it
    with pytest.raises(VtError, match="dense extraction only"):
        gen.generate_mesh_graphed(torch.zeros(1, 8, 3))
    with pytest.raises(VtError, match="dense extraction only"):
        gen.generate_obj_mesh_sharded({"inputs": torch.zeros(1, 8, 3)})
    with pytest.raises(VtError, match="c_img_all"):
        gen.generate_obj_mesh_wnf({"inputs": torch.zeros(1, 8, 3)}, c_img_all=torch.zeros(1, 8, 32))


@pytest.mark.parametrize("value", [None, "dense", "mise"])
def test_get_generator_passes_extraction(value):
    from vtaco_amd.conv_onet import config as cfgmod
    from vtaco_amd.conv_onet.models import decoder_dict
    cfg = {"generation": {"resolution_0": 32, "upsampling_steps": 2}, "test": {"threshold": 0.5},
           "data": {"input_type": "pointcloud", "padding": 0.1}, "model": {}}
    if value is not None:
        cfg["generation"]["extraction"] = value
    gen = cfgmod.get_generator(_Model(decoder_dict["simple_local"](dim=3, c_dim=32, hidden_size=32)), cfg, None)
    assert gen.extraction == (value or "dense") and (gen.resolution0, gen.upsampling_steps) == (32, 2)
