"""GPU: vt_sample_planes / vt_sample_planes_bwd (ops.planes) against the float64 reference of tests/plane_decode_ref.py under the
project's gate -- |got - ref64| <= 8 max(e32, 2^-24 sum of magnitudes), e32 the error of the same reference run in float32 on the CPU,
strictly (the sampler has no nonlinearity: no entry is excluded) -- and the lattice form against the point form bit for bit."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plane_decode_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GATE = 8.0
SUBSETS = {"xy": ("xy",), "xz+yz": ("xz", "yz"), "all": ("xz", "xy", "yz"), "base+all": ("xz", "xy", "yz")}


def _gate(tag, got, r64, r32, bound):
    ratio, e32 = ref.gate_ratio(got, r64, r32, bound)
    print(f"RATIO {tag}: {ratio:.3f} (e32 {e32:.3e})")
    assert ratio <= GATE, f"{tag}: |got - ref64| is {ratio:.3f} x max(e32, 2^-24 bound), above {GATE}"


def _points(g, B, N, far_every=5):
    """In range |p| <= 0.549, every ``far_every``-th point out of range |p| >= 0.56 on every axis (both signs): the f32 and f64 clamps agree."""
    p = (torch.rand(B, N, 3, generator=g) - 0.5) * (2 * 0.549)
    far = torch.where(torch.rand(B, N, 3, generator=g) < 0.5, -1.0, 1.0) * (0.56 + 0.3 * torch.rand(B, N, 3, generator=g))
    mask = (torch.arange(N) % far_every == far_every - 1).view(1, N, 1)
    return torch.where(mask, far, p)


def _planes(g, keys, B, C, R):
    return {k: torch.randn(B, C, R, R, generator=g) for k in keys}


def _nearest_safe(p, R, keys, g):
    """Redraw until every pixel coordinate is at least 1e-3 from a half-integer (asserted): f32 and f64 round the same way."""
    for _ in range(50):
        bad = torch.zeros(p.shape[:2], dtype=torch.bool)
        for k in keys:
            q = ref.orc.normalize_coordinate(p.double(), 0.1, k)
            f = (q * (R - 1)).clamp(0, R - 1)
            bad |= (((f - f.floor()) - 0.5).abs() < 1e-3).any(-1)
        if not bad.any():
            break
        p = torch.where(bad.unsqueeze(-1), (torch.rand(p.shape, generator=g) - 0.5) * (2 * 0.549), p)
    for k in keys:
        q = ref.orc.normalize_coordinate(p.double(), 0.1, k)
        f = (q * (R - 1)).clamp(0, R - 1)
        assert float((((f - f.floor()) - 0.5).abs()).min()) >= 1e-3
    return p


@pytest.mark.parametrize("mode", ["bilinear", "nearest"])
@pytest.mark.parametrize("R", [2, 5, 33])
@pytest.mark.parametrize("subset", list(SUBSETS))
def test_forward_vs_float64(subset, R, mode):
    from vtaco_amd import ops
    keys = SUBSETS[subset]
    for C in (32, 96):
        for N in (1, 67, 257):
            B = 2
            g = torch.Generator().manual_seed(1000 + R * 7 + C + N)
            planes = _planes(g, keys, B, C, R)
            p = _points(g, B, N)
            if mode == "nearest":
                p = _nearest_safe(p, R, keys, g)
            base = torch.randn(B, N, C, generator=g) if subset.startswith("base") else None
            kw = dict(padding=0.1, mode=mode, base=base)
            r64, r32 = ref.features(planes, p, dtype=torch.float64, **kw), ref.features(planes, p, dtype=torch.float32, **kw)
            bound = ref.features(planes, p, dtype=torch.float64, absolute=True, **kw)
            dev = {k: v.to(DEV) for k, v in planes.items()}
            run = lambda d: ops.planes.sample_planes(d, p.to(DEV), 0.1, base=None if base is None else base.to(DEV), nearest=mode == "nearest")
            got = run(dev)
            assert got.shape == (B, N, C)
            _gate(f"fwd/{subset}/{mode} R{R} C{C} N{N}", got, r64, r32, bound)
            # the sum runs xz, xy, yz whatever order the dict has
            assert torch.equal(got, run({k: dev[k] for k in reversed(list(dev))}))


@pytest.mark.parametrize("nx", [8, 17, 33])
def test_lattice_form_is_the_point_form_bit_for_bit(nx):
    from vtaco_amd import ops
    from vtaco_amd.common import make_3d_grid
    B, C, R, box = 2, 32, 9, 1.1
    g = torch.Generator().manual_seed(50 + nx)
    planes = {k: v.to(DEV) for k, v in _planes(g, ("xz", "xy", "yz"), B, C, R).items()}
    lattice = (box * make_3d_grid((-0.5,) * 3, (0.5,) * 3, (nx,) * 3)).to(DEV)
    for first, count in ((0, nx ** 3), (5, min(1000, nx ** 3 - 5)), (nx * nx + 3, 2 * nx * nx + 7)):
        pts = lattice[first:first + count].unsqueeze(0).expand(B, -1, -1).contiguous()
        for with_base in (False, True):
            base = torch.randn(B, count, C, generator=g).to(DEV) if with_base else None
            want = ops.planes.sample_planes(planes, pts, 0.1, base=None if base is None else base.clone())
            for form in ("table", "points"):
                got = ops.planes.sample_planes(planes, None, 0.1, base=None if base is None else base.clone(),
                                               lattice=(nx, box, first, count), lattice_form=form)
                assert torch.equal(got, want), (nx, first, count, with_base, form)
    one = ops.planes.sample_planes({"xy": planes["xy"]}, None, 0.1, lattice=(nx, box, 3, 77))
    assert torch.equal(one, ops.planes.sample_planes({"xy": planes["xy"]}, lattice[3:80].unsqueeze(0).expand(B, -1, -1).contiguous(), 0.1))


def _clustered(g, B, N, R, n_cluster):
    """``n_cluster`` points inside one bilinear cell of every plane, the rest spread out (some out of range)."""
    p = _points(g, B, N)
    if n_cluster:
        cell = (R - 1) // 2                                          # pixel coordinate in [cell + 0.1, cell + 0.9] on every axis
        f = cell + 0.1 + 0.8 * torch.rand(B, n_cluster, 3, generator=g)
        p[:, :n_cluster] = (f / (R - 1) - 0.5) * float(torch.tensor(1.0 + 0.1 + 10e-6))
    return p


def _check_bwd(tag, keys, B, C, R, N, n_cluster, mode, seed):
    from vtaco_amd import ops
    g = torch.Generator().manual_seed(seed)
    p = _clustered(g, B, N, R, n_cluster)
    if mode == "nearest":
        p = _nearest_safe(p, R, keys, g)
    gf = torch.randn(B, N, C, generator=g)
    nan = lambda: torch.full((B, C, R, R), float("nan"), device=DEV)
    out = {k: nan() for k in ("xz", "xy", "yz")}                     # "written": no pre-zeroing, here NaN
    got = ops.planes.sample_planes_bwd(keys, (B, C, R, R), p.to(DEV), gf.to(DEV), 0.1, nearest=mode == "nearest", out=out)
    assert set(got) == set(keys)
    for k in ("xz", "xy", "yz"):
        if k not in keys:
            assert bool(torch.isnan(out[k]).all()), f"{tag}: the absent plane {k} was touched"
            continue
        assert got[k] is out[k] and bool(torch.isfinite(got[k]).all()), f"{tag}: {k} not fully written"
        kw = dict(padding=0.1, mode=mode)
        r64, r32 = ref.scatter(gf, p, R, k, dtype=torch.float64, **kw), ref.scatter(gf, p, R, k, dtype=torch.float32, **kw)
        _gate(f"{tag} d {k}", got[k], r64, r32, ref.scatter(gf, p, R, k, dtype=torch.float64, absolute=True, **kw))


@pytest.mark.parametrize("R", [2, 5, 33])
@pytest.mark.parametrize("subset", ["xy", "xz+yz", "all"])
def test_backward_clustered_vs_float64(subset, R):
    _check_bwd(f"bwd/{subset} R{R}", SUBSETS[subset], 2, 32, R, 512, 400, "bilinear", 300 + R)


def test_backward_one_point_wide_and_nearest():
    _check_bwd("bwd/N1", ("xz", "xy", "yz"), 2, 32, 5, 1, 0, "bilinear", 400)
    _check_bwd("bwd/C96", ("xz", "yz"), 2, 96, 5, 67, 30, "bilinear", 401)
    _check_bwd("bwd/nearest", ("xz", "xy", "yz"), 2, 32, 5, 512, 400, "nearest", 402)
    _check_bwd("bwd/nearest R33", ("xy",), 2, 32, 33, 257, 100, "nearest", 403)


def test_autograd_function_matches_the_ops():
    """_SamplePlanesFn: the forward is sample_planes', the planes' gradients pass the gate, the base's gradient is the output's."""
    from vtaco_amd import ops
    from vtaco_amd.conv_onet.models.decoder import _SamplePlanesFn
    g = torch.Generator().manual_seed(7)
    B, C, R, N = 2, 32, 5, 67
    planes = {k: v.to(DEV).requires_grad_(True) for k, v in _planes(g, ("yz", "xz"), B, C, R).items()}
    p = _points(g, B, N).to(DEV)
    base = torch.randn(B, N, C, generator=g).to(DEV).requires_grad_(True)
    w = torch.randn(B, N, C, generator=g).to(DEV)
    keys = tuple(planes)
    out = _SamplePlanesFn.apply(p, 0.1, False, base, keys, *[planes[k] for k in keys])
    assert torch.equal(out, ops.planes.sample_planes({k: v.detach() for k, v in planes.items()}, p, 0.1, base=base.detach().clone()))
    (out * w).sum().backward()
    assert torch.equal(base.grad, w)
    # (not bit for bit against a second sample_planes_bwd call: the f32 atomics of neighbouring cells arrive in any order)
    pc, wc = p.cpu(), w.cpu()
    for k in keys:
        r64, r32 = ref.scatter(wc, pc, R, k), ref.scatter(wc, pc, R, k, dtype=torch.float32)
        _gate(f"autograd d {k}", planes[k].grad, r64, r32, ref.scatter(wc, pc, R, k, absolute=True))
