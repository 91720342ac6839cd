"""CPU: the float64 restatement of scikit-image's marching-cubes normals and values (tests/mc_normals_ref.py) against scikit-image
0.18.3's own output (tests/golden/g30_mc_normals.npz, written by tests/golden/make_mc_normals_goldens.py) on the volumes of g7_mc.npz.
Normals: |skimage - restatement| <= (n + 6) 2^-24 kappa per component, centre vertices included; vertices with kappa > 2^12 are
checked for finiteness only and are at most 2 % of a volume's.  Values: within one float32 unit in the last place."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mc_normals_ref as R  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ["sphere16", "torus24", "noise12", "noise20", "noise_rect", "smoothnoise24", "plateau10", "tiny2", "checker8", "noise20@0.25",
         "sphere16@0.25"]
_cache = {}


def fixtures():
    if "z" not in _cache:
        _cache["z"] = (np.load(os.path.join(GOLD, "g7_mc.npz")), np.load(os.path.join(GOLD, "g30_mc_normals.npz")))
    return _cache["z"]


def restated(name):
    """R.mc of a fixture case, computed once per process (the GPU tests share it)."""
    if name not in _cache:
        g7, _ = fixtures()
        _cache[name] = R.mc(g7[name + ".vol"], 0.25 if "@" in name else None)
    return _cache[name]


def check_normals(what, got, ref, unusable=None):
    """The gate of both the CPU and the GPU tests; returns the share of the bound that was used."""
    got = np.asarray(got, dtype=np.float64)
    usable = ref["kappa"] <= R.KAPPA_MAX
    assert (~usable).mean() <= 0.02, (what, float((~usable).mean()))
    if unusable is not None:
        assert not (unusable & usable).any(), what                  # a zero or non-finite scikit-image normal is a cancelled sum
        assert np.isfinite(got[~unusable]).all(), what
    else:
        assert np.isfinite(got).all(), what
    err = np.abs(got[usable] - ref["normals"][usable])
    gate = R.bound(ref["n"][usable], ref["kappa"][usable])[:, None]
    worst = float((err / gate).max()) if err.size else 0.0
    print(f"RATIO {what}: {worst:.3f} of the bound, max |err| {float(err.max()) if err.size else 0:.3e}, {int((~usable).sum())} of {len(usable)} beyond kappa")
    assert worst <= 1.0, (what, worst)
    return worst


@pytest.mark.parametrize("name", CASES)
def test_volume(name):
    g7, g30 = fixtures()
    ref = restated(name)
    assert np.array_equal(ref["faces"], g7[name + ".faces"])
    assert np.abs(ref["verts"] - g7[name + ".verts"]).max() <= 2.0 ** -23 * max(g7[name + ".vol"].shape)
    check_normals(name, g30[name + ".normals"], ref, g30[name + ".unusable"])
    sk = g30[name + ".values"]
    assert sk.dtype == np.float32 and ref["values"].dtype == np.float32
    assert np.all(np.abs(sk.astype(np.float64) - ref["values"].astype(np.float64)) <= np.spacing(np.maximum(sk, ref["values"])))


def test_centre_vertices_are_covered():
    """The centre-vertex rule was fitted, so centre vertices pass the same gate; they exist in the fixtures that test it."""
    counts = {name: int(restated(name)["centre"].sum()) for name in ("noise12", "noise_rect", "checker8")}
    assert all(c >= 10 for c in counts.values()), counts
    for name in ("sphere16", "torus24", "smoothnoise24"):
        assert restated(name)["centre"].mean() <= 0.05


def test_single_cells():
    g7, g30 = fixtures()
    n_cells = g30["cells.normals"].shape[0]
    worst, seen, checked = 0.0, set(), 0
    for i in range(n_cells):
        nv = int(g7["cells.nv"][i])
        if nv == 0:
            continue
        vol = g7["cells.vols"][i]
        ref = R.mc(vol, 0.0)
        assert np.array_equal(ref["faces"], g7["cells.faces"][i][:int(g7["cells.nf"][i])].astype(np.int32)), i
        corner = [float(vol[R.CZ[k], R.CY[k], R.CX[k]]) for k in range(8)]
        seen.add(int(R.tables()["CASES"][sum(1 << k for k in range(8) if corner[k] > 0)][0]))
        sk = g30["cells.normals"][i][:nv].astype(np.float64)
        usable = ref["kappa"] <= R.KAPPA_MAX
        assert not (g30["cells.unusable"][i][:nv] & usable).any(), i
        err = np.abs(sk[usable] - ref["normals"][usable]) / R.bound(ref["n"][usable], ref["kappa"][usable])[:, None]
        worst = max(worst, float(err.max()) if err.size else 0.0)
        assert worst <= 1.0, (i, worst)
        assert np.array_equal(g30["cells.values"][i][:nv], ref["values"]), i
        checked += nv
    print(f"RATIO cells: {worst:.3f} of the bound over {checked} vertices")
    assert seen == set(range(1, 15)) and checked > 10000


def test_quirk_and_reference_count_matter():
    """Without the mirror rule, or counting per cell instead of per triangle corner, the restatement leaves scikit-image's normals."""
    g7, g30 = fixtures()
    ref = R.mc(g7["noise_rect.vol"], quirk=False)
    usable = ref["kappa"] <= R.KAPPA_MAX
    err = np.abs(g30["noise_rect.normals"][usable] - ref["normals"][usable]) / R.bound(ref["n"][usable], ref["kappa"][usable])[:, None]
    assert (err.max(1) > 1.0).mean() > 0.3
