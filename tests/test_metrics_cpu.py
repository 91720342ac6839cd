"""CPU: the visualise block's host side -- the reference's metrics (g21) reproduced by the host functions, Mesh.export round
trips, the shuffle rule of Generator3D.reference_metrics, and get_generator's reference_returns pass-through."""
import numpy as np
import pytest
import torch

from conftest import load_golden


def test_g21_reproduced_by_the_host_functions():
    from vtaco_amd import eval as veval
    z, _ = load_golden("g21_metrics.npz")
    assert list(z["cases"]) == ["close", "far", "rect", "mesh"]
    for case in z["cases"]:
        a, b = z[f"{case}.a"], z[f"{case}.b"]
        assert a.dtype == b.dtype == np.float32 and a.shape[0] == 2048
        emd = veval.earth_mover_distance(a, b)
        assert abs(emd - float(z[f"{case}.emd"])) <= 1e-12 * float(z[f"{case}.emd"]), case
        assert abs(float(z[f"{case}.cost"]) / len(a) - emd) <= 1e-12, case
        cd = float(veval.chamfer_distance_naive(torch.from_numpy(a)[None], torch.from_numpy(b)[None])[0])
        assert abs(cd - float(z[f"{case}.cd"])) <= 1e-6 * float(z[f"{case}.cd"]), case
    assert z["rect.b"].shape == (1500, 3)


def test_index_shuffle_draws_the_reference_shuffle():
    """np.random.shuffle of the vertex indices permutes like the reference's in-place shuffle of the [V,3] array and leaves numpy's
    generator in the same state (reference_metrics relies on it to pick the reference's 2048 vertices)."""
    rng = np.random.RandomState(3)
    for V in (1, 5, 2047, 2048, 17163):
        verts = rng.randn(V, 3).astype(np.float32)
        np.random.seed(V)
        order = np.arange(V)
        np.random.shuffle(order)
        after_idx = np.random.randint(1 << 30)
        np.random.seed(V)
        ref = verts.copy()
        np.random.shuffle(ref)
        after_ref = np.random.randint(1 << 30)
        assert np.array_equal(verts[order], ref) and after_idx == after_ref


def read_mesh(path, kind):
    with open(path) as f:
        lines = [ln.split() for ln in f.read().splitlines()]
    if kind == "off":
        assert lines[0] == ["OFF"]
        V, F, _ = map(int, lines[1])
        body = lines[2:]
        return np.array(body[:V], dtype=np.float64).reshape(-1, 3), np.array([r[1:] for r in body[V:V + F]], dtype=np.int64).reshape(-1, 3)
    if kind == "ply":
        end = lines.index(["end_header"])
        head = lines[:end]
        assert head[0] == ["ply"] and head[1] == ["format", "ascii", "1.0"]
        V = int(next(r[2] for r in head if r[:2] == ["element", "vertex"]))
        F = int(next(r[2] for r in head if r[:2] == ["element", "face"]))
        body = lines[end + 1:]
        assert all(r[0] == "3" for r in body[V:V + F])
        return np.array(body[:V], dtype=np.float64).reshape(-1, 3), np.array([r[1:] for r in body[V:V + F]], dtype=np.int64).reshape(-1, 3)
    v = np.array([r[1:] for r in lines if r[0] == "v"], dtype=np.float64).reshape(-1, 3)
    f = np.array([r[1:] for r in lines if r[0] == "f"], dtype=np.int64).reshape(-1, 3) - 1
    return v, f


@pytest.mark.parametrize("kind", ["off", "ply", "obj"])
def test_mesh_export_round_trips(tmp_path, kind):
    from vtaco_amd.conv_onet.generation import Mesh
    rng = np.random.RandomState(4)
    v32 = torch.from_numpy((rng.randn(300, 3) * np.logspace(-8, 3, 300)[:, None]).astype(np.float32))
    v32[:2] = v32[2:4]                                          # duplicate vertices stay duplicates
    faces = torch.from_numpy(rng.randint(0, 300, (500, 3)).astype(np.int32))
    m = Mesh(v32, faces)
    m.export(str(tmp_path / f"m.{kind}"))
    v, f = read_mesh(tmp_path / f"m.{kind}", kind)
    assert v.shape == (300, 3) and f.shape == (500, 3)
    assert np.array_equal(v.astype(np.float32), v32.numpy()) and np.array_equal(f, faces.numpy())
    # float64 vertices (the hand mesh) read back exactly as well; the type can also be named explicitly
    v64 = torch.from_numpy(rng.randn(40, 3))
    Mesh(v64, torch.zeros((0, 3), dtype=torch.int64)).export(str(tmp_path / "h.txt"), file_type=kind)
    v, f = read_mesh(tmp_path / "h.txt", kind)
    assert np.array_equal(v, v64.numpy()) and f.shape == (0, 3)


def test_mesh_stays_the_namedtuple():
    from vtaco_amd._lib import VtError
    from vtaco_amd.conv_onet.generation import Mesh
    v, f = torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32)
    m = Mesh(v, f)
    verts, faces = m
    assert verts is v and faces is f and m.vertices is v and m.faces is f and m._fields == ("vertices", "faces")
    assert m == (v, f) and m == Mesh(v, f) and len(m) == 2 and isinstance(m, tuple)
    assert m._replace(faces=None).faces is None
    with pytest.raises(VtError):
        m.export("mesh.stl")


def _cfg(**generation):
    return {"generation": dict({"resolution_0": 8, "upsampling_steps": 0}, **generation), "test": {"threshold": 0.5},
            "data": {"input_type": "pointcloud", "padding": 0.1}, "model": {}}


def test_get_generator_passes_reference_returns():
    from vtaco_amd.conv_onet import config
    model = torch.nn.Linear(1, 1)
    assert config.get_generator(model, _cfg(), "cpu").reference_returns is False
    assert config.get_generator(model, _cfg(reference_returns=True), "cpu").reference_returns is True
    assert config.get_generator(model, _cfg(reference_returns=True), "cpu", reference_returns=False).reference_returns is False
    assert config.get_generator(model, _cfg(), "cpu", reference_returns=True).reference_returns is True


def test_reference_metrics_host_edge_cases():
    """No points_obj: VtError; an empty mesh: (nan, nan), where the reference fails inside marching cubes."""
    from vtaco_amd._lib import VtError
    from vtaco_amd.conv_onet.generation import Generator3D, Mesh
    gen = Generator3D(torch.nn.Linear(1, 1), device="cpu", reference_returns=True)
    empty = Mesh(torch.zeros((0, 3)), torch.zeros((0, 3), dtype=torch.int32))
    with pytest.raises(VtError, match="points_obj"):
        gen.reference_metrics(empty, {})
    emd, cd = gen.reference_metrics(empty, {"points.points_obj": torch.zeros(1, 2048, 3)})
    assert np.isnan(emd) and np.isnan(cd)
