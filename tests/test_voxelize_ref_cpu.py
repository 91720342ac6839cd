"""CPU: tests/voxelize_ref.py, the float64 numpy restatement of voxelize.hip's definitions (DESIGN.md "voxelize.hip"), on the committed
cases -- the counts that pin how the definitions are read, the margins the GPU tests' exact comparisons rest on, and three checks that do
not share code with it: the float64 winding number, scipy's binary_fill_holes and a box whose every tested centre is a tie.

Every committed case keeps its smallest decisive margin (separating-axis slack / |axis|, distance of a tested column centre from the edge
line that decides it, distance of a crossing z - .5 from an integer; grid units) at or above 1e-6, while float64 rounding on the device
can move these quantities by about 1e-15 * res: the GPU comparisons are therefore exact equalities with no excluded voxel.  With the
default frame the longest axis spans exactly 0.05 res .. 0.95 res, so a resolution that is a multiple of 20 puts vertices on grid planes;
the generic cases avoid those."""
import numpy as np
import pytest
from scipy import ndimage

from conftest import load_golden
import voxelize_ref as R

MARGIN = 1e-6
# case -> (faces, res, surface, interior, ray)
COUNTS = {"torus16x8": (256, 16, 610, 400, 756), "torus24x12": (576, 33, 2968, 4232, 5814), "torus12x6": (144, 24, 1354, 1214, 1976),
          "shell": (1152, 44, 8050, 8368, 12402)}
SHELL_FILL = 13998


@pytest.fixture(scope="module")
def computed():
    out = {}
    for name, (make, res) in R.CASES.items():
        v, f = make()
        loc, scale = R.default_frame(v)
        s, ms = R.surface(v, f, res, loc, scale)
        i, me, mc = R.interior(v, f, res, loc, scale)
        out[name] = dict(v=v, f=f, res=res, loc=loc, scale=scale, surface=s, interior=i, margins=(ms, me, mc))
    return out


@pytest.mark.parametrize("name", sorted(COUNTS))
def test_counts_and_margins(computed, name):
    c = computed[name]
    faces, res, n_surface, n_interior, n_ray = COUNTS[name]
    print(name, "margins (surface, edge, crossing):", c["margins"])
    assert c["v"].dtype == np.float32 and len(c["f"]) == faces and c["res"] == res and res % 20 != 0
    assert (int(c["surface"].sum()), int(c["interior"].sum()), int((c["surface"] | c["interior"]).sum())) == (n_surface, n_interior, n_ray)
    assert min(c["margins"]) >= MARGIN, c["margins"]


@pytest.mark.parametrize("name", sorted(COUNTS))
def test_parity_interior_is_the_winding_number(computed, name):
    c = computed[name]
    w = R.winding_number(c["v"], c["f"], R.centres(c["res"], c["loc"], c["scale"])).reshape((c["res"],) * 3)
    assert np.abs(w - np.round(w)).max() < 1e-6                    # a closed mesh: integers away from the surface
    assert int(((w > 0.5) != c["interior"]).sum()) == 0


@pytest.mark.parametrize("name", ["torus16x8", "torus24x12", "torus12x6"])
def test_fill_of_a_solid_surface_is_ray(computed, name):
    c = computed[name]
    assert np.array_equal(ndimage.binary_fill_holes(c["surface"]), c["surface"] | c["interior"])


def test_fill_of_the_shell_also_fills_the_cavity(computed):
    c = computed["shell"]
    filled, ray = ndimage.binary_fill_holes(c["surface"]), c["surface"] | c["interior"]
    assert int(filled.sum()) == SHELL_FILL and int((filled & ~ray).sum()) == SHELL_FILL - COUNTS["shell"][4] == 1596
    assert not (ray & ~filled).any()


def test_tie_rule_on_the_box():
    """Corners at grid 4.5 and 11.5: every column centre on the outline and on the diagonals is an exact tie; (+eps, +eps^2) makes the
    intervals half-open, so 7^3 centres are inside and nothing leaks to the top layer."""
    v, f = R.box()
    assert np.array_equal(R.to_grid(v, (0, 0, 0), 1.0, 16), np.where(v < 0, 4.5, 11.5)) and len(f) == 12
    occ, m_edge, _ = R.interior(v, f, 16)
    assert m_edge == 0.0                                           # the case does contain ties
    assert int(occ.sum()) == 343 and not occ[:, :, -1].any()
    want = np.zeros((16,) * 3, dtype=bool)
    want[4:11, 4:11, 4:11] = True
    assert np.array_equal(occ, want)
    for perm in ([0, 2, 1], [1, 2, 0], [2, 1, 0]):                 # whichever way a triangle is walked
        assert np.array_equal(R.interior(v, f[:, perm], 16)[0], want)


def test_fixture_holds_the_restatement(computed):
    z, _ = load_golden("g27_voxelgrid.npz")
    for name, c in computed.items():
        n = c["res"] ** 3
        assert np.array_equal(z[f"def.{name}.verts"], c["v"]) and np.array_equal(z[f"def.{name}.faces"], c["f"])
        assert np.array_equal(z[f"def.{name}.loc"], c["loc"]) and float(z[f"def.{name}.scale"]) == c["scale"]
        assert np.array_equal(np.unpackbits(z[f"def.{name}.surface"])[:n].astype(bool).reshape(c["surface"].shape), c["surface"])
        assert np.array_equal(np.unpackbits(z[f"def.{name}.interior"])[:n].astype(bool).reshape(c["surface"].shape), c["interior"])
    for name in ("clipped", "span"):
        assert z[f"def.{name}.margins"].min() >= MARGIN
    assert list(z["ref.stubbed"]) == [s for s in z["ref.stubbed"] if s in ("trimesh", "skimage", "skimage.measure", "np.bool")]


def test_pack_bits_layout():
    occ = np.zeros((33,) * 3, dtype=bool)
    occ[1, 2, 0] = occ[1, 2, 31] = occ[1, 2, 32] = True
    bits = R.pack_bits(occ)
    assert bits.shape == (33, 33, 2) and bits[1, 2, 0] == 0x80000001 and bits[1, 2, 1] == 1 and int(bits.astype(np.int64).sum()) == 0x80000002
