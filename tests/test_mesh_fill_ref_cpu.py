"""CPU: the definition in tests/mesh_fill_ref.py against things it shares no code with -- edge counts by numpy's unique, the Euler number,
mesh_topo_ref.topo's boundary count, exact and analytic volumes, invariance under relabelling, and math.fsum for the centroid."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mesh_fill_ref as R  # noqa: E402
import mesh_topo_ref as T  # noqa: E402

NAMES = sorted(R.FIXTURES)


@pytest.mark.parametrize("name", NAMES)
def test_expected_loops(name):
    v, f = R.fixture(name)
    loops = R.boundary_loops(f, v.shape[0])
    _, lengths, n_irregular = R.FIXTURES[name]
    got = np.diff(loops["offsets"]).tolist()
    if lengths is not None:
        assert got == lengths, name
    if n_irregular is not None:
        assert loops["n_irregular"] == n_irregular, name
    assert all(n >= 3 for n in got)
    assert loops["n_boundary"] == loops["n_irregular"] + sum(got)
    # a loop starts at its smallest half-edge and the loops ascend by it
    starts = [int(loops["half_edges"][o]) for o in loops["offsets"][:-1]]
    assert starts == sorted(starts)
    for l, o in enumerate(loops["offsets"][:-1]):
        assert starts[l] == int(loops["half_edges"][o:loops["offsets"][l + 1]].min())


def test_named_expectations():
    lengths = lambda name: sorted(np.diff(R.boundary_loops(R.fixture(name)[1], R.fixture(name)[0].shape[0])["offsets"]).tolist())
    assert lengths("torus_with_holes") == [3, 3, 3, 3, 8]
    assert lengths("torus_with_bowtie") == [3, 3, 8]                     # the two triangles that touch are no loops: 6 irregular edges
    flipped = R.boundary_loops(R.fixture("flipped_next_to_hole")[1], 8)
    assert flipped["n_irregular"] > 0                                     # in / out mismatch at the flipped face's corners
    fan = R.boundary_loops(R.fixture("fan_on_one_edge")[1], 5)
    assert fan["n_boundary"] == 6 and fan["n_loops"] == 0 and fan["n_irregular"] == 6     # the edge used three times is not boundary
    cyl = R.boundary_loops(R.fixture("open_cylinder")[1], 32)
    a, b = (cyl["vertices"][cyl["offsets"][l]:cyl["offsets"][l + 1]] for l in (0, 1))
    assert {int(a[1] - a[0]) % 16, int(b[1] - b[0]) % 16} == {1, 15}                     # opposite sense (ring k is vertices 16 k ..)


@pytest.mark.parametrize("name", [n for n in NAMES if n != "empty"])
def test_boundary_count_is_topo(name):
    v, f = R.fixture(name)
    assert R.boundary_loops(f, v.shape[0])["n_boundary"] == int(T.topo(v, f)["n_boundary"].sum()), name


@pytest.mark.parametrize("method", ["fan", "centroid"])
@pytest.mark.parametrize("name", NAMES)
def test_filled_is_closed_and_oriented(name, method):
    v, f = R.fixture(name)
    ref = R.reference(name, method)
    assert np.array_equal(ref["faces"][:f.shape[0]], f) and ref["vertices"][:v.shape[0]].tobytes() == v.tobytes()
    assert ref["faces"].shape[0] == f.shape[0] + ref["n_new_faces"] and ref["vertices"].shape[0] == v.shape[0] + ref["n_new_vertices"]
    assert ref["n_filled"] == ref["n_loops"]
    if ref["n_irregular"] or name == "fan_on_one_edge":
        return
    assert R.closed_and_oriented(ref["faces"]), name
    # a cap is a disc by either method (fan: n - 2 faces, n - 3 edges; centroid: n faces, n spokes, one vertex): +1 per loop
    assert R.euler_number(ref["faces"]) - R.euler_number(f) == ref["n_filled"], name


def test_max_edges():
    ref = R.reference("torus_with_holes", "fan", 5)
    assert ref["n_loops"] == 5 and ref["n_filled"] == 4 and ref["n_new_faces"] == 4
    assert not R.closed_and_oriented(ref["faces"])
    both = R.reference("torus_with_bowtie", "centroid")
    assert both["n_filled"] == 3 and both["n_new_vertices"] == 1 and both["n_irregular"] == 6


@pytest.mark.parametrize("method", ["fan", "centroid"])
def test_open_cube_volume_is_one(method):
    ref = R.reference("open_cube", method)
    assert R.signed_volume(ref["vertices"], ref["faces"]) == 1.0


@pytest.mark.parametrize("method", ["fan", "centroid"])
@pytest.mark.parametrize("n", R.CONE_SIZES)
def test_cone_volume(n, method):
    ref = R.reference(f"cone{n}", method)
    v, f = ref["vertices"], ref["faces"]
    want = R.cone_volume(R.fixture(f"cone{n}")[0])
    gate = T.sum_gate(f.shape[0], T.term_bounds(v, f)[1].tolist())
    got = R.signed_volume(v, f)
    if method == "centroid" and n >= 4:
        # the centroid is rounded to float32 and leaves the rim's plane by at most half an ulp of its z = 0: nothing; in the plane it
        # may sit anywhere, the cap's signed area does not depend on it
        assert float(v[-1, 2]) == 0.0
    T.log_line(f"RATIO cpu cone{n} {method} volume: {abs(got - want) / gate:.3e} of the gate")
    assert want > 0 and abs(got - want) <= gate, (n, method, got, want, gate)


@pytest.mark.parametrize("name", ["open_cube", "open_cylinder", "torus_with_holes", "torus_with_bowtie", "cone65"])
def test_relabelling_keeps_the_loops(name):
    v, f = R.fixture(name)
    rng = np.random.RandomState(17)
    pi = rng.permutation(v.shape[0]).astype(np.int32)          # old index -> new index
    inv = np.argsort(pi)
    f2 = pi[f][rng.permutation(f.shape[0])]
    f2 = np.stack([np.roll(row, int(s)) for row, s in zip(f2, rng.randint(0, 3, f2.shape[0]))]).astype(np.int32)    # corners rotated too

    def cyclic(loops, back):
        out = set()
        for l in range(loops["n_loops"]):
            ring = [int(back[x]) for x in loops["vertices"][loops["offsets"][l]:loops["offsets"][l + 1]]]
            k = ring.index(min(ring))
            out.add(tuple(ring[k:] + ring[:k]))
        return out

    a, b = R.boundary_loops(f, v.shape[0]), R.boundary_loops(f2, v.shape[0])
    assert cyclic(a, np.arange(v.shape[0])) == cyclic(b, inv)
    assert (a["n_boundary"], a["n_irregular"]) == (b["n_boundary"], b["n_irregular"])


@pytest.mark.parametrize("name", ["open_cube", "cone5", "cone257", "cone1025", "torus_f64", "annulus"])
def test_centroid_against_fsum(name):
    v, f = R.fixture(name)
    loops = R.boundary_loops(f, v.shape[0])
    worst = 0.0
    for l in range(loops["n_loops"]):
        xyz = v[loops["vertices"][loops["offsets"][l]:loops["offsets"][l + 1]]].astype(np.float64)
        n = xyz.shape[0]
        c = R.centroid(xyz)
        for a in range(3):
            want = math.fsum(xyz[:, a].tolist()) / n
            gate = (n + 16) * 2.0 ** -52 * math.fsum(np.abs(xyz[:, a]).tolist()) / n
            err = abs(float(c[a]) - want)
            assert err <= gate, (name, l, a, err, gate)
            worst = max(worst, err / gate if gate > 0 else 0.0)
    T.log_line(f"RATIO cpu {name} centroid: {worst:.3e} of the gate, {loops['n_loops']} loops")


def test_generator_argument_without_a_device():
    import torch
    from vtaco_amd._lib import VtError
    from vtaco_amd.conv_onet import config
    from vtaco_amd.conv_onet.generation import Generator3D, Mesh
    model = torch.nn.Linear(1, 1)
    for bad in ("ear", True, 0, 1.5):
        with pytest.raises(VtError, match="fill_holes"):
            Generator3D(model, device="cpu", fill_holes=bad)
    for bad in (2, 4.0, True, "8"):
        with pytest.raises(VtError, match="fill_holes_max_edges"):
            Generator3D(model, device="cpu", fill_holes="fan", fill_holes_max_edges=bad)
    with pytest.raises(VtError, match=r"'fan'.*with_vertex_normals\(\)"):
        Generator3D(model, device="cpu", fill_holes="centroid", with_normals=True)
    gen = Generator3D(model, device="cpu")
    assert gen.fill_holes is None and gen.fill_holes_max_edges is None
    mesh = Mesh(torch.zeros(3, 3), torch.zeros((1, 3), dtype=torch.int32))
    assert gen._clean(mesh) is mesh                                                  # the default launches nothing
    gen = Generator3D(model, device="cpu", fill_holes="fan", fill_holes_max_edges=np.int64(12), with_normals=True)
    assert (gen.fill_holes, gen.fill_holes_max_edges) == ("fan", 12) and isinstance(gen.fill_holes_max_edges, int)
    with pytest.raises(VtError, match="Mesh.fill_holes"):
        Generator3D(model, device="cpu", fill_holes="fan").generate_obj_mesh_sharded({})
    with pytest.raises(VtError, match="HIP device"):
        mesh.fill_holes()
    with pytest.raises(VtError, match="HIP device"):
        mesh.boundary_loops()
    # the positional order of the constructor is the parent's: the new arguments come last
    import inspect
    names = list(inspect.signature(Generator3D.__init__).parameters)
    assert names[-2:] == ["fill_holes", "fill_holes_max_edges"] and names[-3] == "refine_sampler"
    cfg = {"generation": {"resolution_0": 8, "upsampling_steps": 0, "fill_holes": "fan", "fill_holes_max_edges": 500},
           "test": {"threshold": 0.5}, "data": {"input_type": "pointcloud", "padding": 0.1}, "model": {}}
    gen = config.get_generator(model, cfg, "cpu")
    assert (gen.fill_holes, gen.fill_holes_max_edges) == ("fan", 500)
