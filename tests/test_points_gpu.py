"""GPU: the five kernels of the PointConv baseline (ops.points: vt_point_sample_fwd / _bwd, vt_fps, vt_ball_query, vt_three_nn)
against the float64 statement of tests/pointconv_ref.py.

Float results go through the project's gate, elementwise |got - ref64| <= 8 max(e32, 2^-24 bound) (decode_train_ref.gate_ratio):
e32 the largest error of the same statement in float32 over the tensor, bound the same sum over magnitudes.  Index results must
equal the float64 reference's exactly; each such test first asserts, on the reference, that the fixture has no near-tie a float32
evaluation could legitimately decide the other way (the margins are in the tests).  Every comparison prints its ratio."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pointconv_ref as R
from decode_train_ref import gate_ratio

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GATE = 8.0
TILE_N = 32                          # cloud points per LDS tile of the sampler (vt_points::TILE_K)
MODES = {"g005": ("gaussian", 0.05), "g02": ("gaussian", 0.2), "inv": ("inverse", None)}


def _ops():
    from vtaco_amd import ops
    return ops.points


def _gate(tag, got, r64, r32, bound):
    ratio, e32 = gate_ratio(got, r64, r32, bound)
    print(f"RATIO {tag}: {ratio:.3f} (e32 {e32:.3e})")
    assert ratio <= GATE, f"{tag}: |got - ref64| is {ratio:.3f} x max(e32, 2^-24 bound), above {GATE}"


@functools.lru_cache(maxsize=None)
def _scene(M, N, C, seed=0):
    """Two different clouds with features, and queries near them: query 0 IS a cloud point (the 10e-6 decides its weight), every
    fifth query starts from the corner point cloud[:, 0] and lies outside the unit cube, the rest sit within 0.17 per axis of a
    cloud point (so the reference's own float32 sum stays far above underflow at gaussian_val 0.05)."""
    g = torch.Generator().manual_seed(7000 + 131 * M + 17 * N + C + seed)
    cloud = torch.rand(2, N, 3, generator=g) - 0.5
    cloud[:, 0] = torch.tensor([0.49, -0.49, 0.48])
    fea = torch.randn(2, N, C, generator=g)
    near = torch.randint(0, N, (2, M), generator=g)
    q = R.index_points(cloud, near) + (torch.rand(2, M, 3, generator=g) - 0.5) * 0.34
    out = torch.arange(M) % 5 == 1
    q[:, out] = cloud[:, :1] + torch.tensor([0.1, -0.1, 0.05]) * (0.5 + 0.5 * torch.rand(2, int(out.sum()), 1, generator=g))
    q[:, 0] = cloud[:, N // 2]
    return cloud, fea, q


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("C", [32, 96, 128])
@pytest.mark.parametrize("N", [1, 3, TILE_N - 1, TILE_N + 1, 65, 513])
@pytest.mark.parametrize("M", [1, 67, 257])
def test_sampler_forward(M, N, C, mode):
    sm, gv = MODES[mode]
    cloud, fea, q = _scene(M, N, C)
    if M > 1:
        assert bool((q.abs() > 0.5).any(dim=-1)[:, 1].all())                                   # a query outside the unit cube
    assert torch.equal(q[:, 0], cloud[:, N // 2])
    _, s32 = R.sample_unshifted(q, cloud, fea, sm, gv, torch.float32)
    assert float(s32.min()) >= 2.0 ** -100, f"the reference's float32 sum underflows ({float(s32.min()):.3e}): not a gated query"
    r64, r32 = R.sample(q, cloud, fea, sm, gv, torch.float64), R.sample(q, cloud, fea, sm, gv, torch.float32)
    bound = R.sample(q, cloud, fea, sm, gv, torch.float64, absolute=True)
    got, shift, total = _ops().point_sample(cloud.to(DEV), fea.to(DEV), pts=q.to(DEV), sample_mode=sm, gaussian_val=gv, want_saved=True)
    assert got.shape == (2, M, C) and shift.shape == total.shape == (2, M)
    _gate(f"sample M={M} N={N} C={C} {mode}", got, r64, r32, bound)
    assert bool((total > 0).all()) and (sm == "gaussian" or bool((shift == 0).all()))


@pytest.mark.parametrize("C", [32, 128])
def test_sampler_far_queries_finite_where_reference_is_nan(C):
    """Queries 0.6 from the nearest cloud point at gaussian_val 0.05: the reference divides 0 by 0; the kernel returns the limit."""
    g = torch.Generator().manual_seed(7100 + C)
    cloud = (torch.rand(2, 65, 3, generator=g) - 0.5) * 0.2
    fea = torch.randn(2, 65, C, generator=g)
    d = torch.randn(2, 67, 3, generator=g)
    q = d / d.norm(dim=-1, keepdim=True) * (0.6 + 0.1 * 3 ** 0.5 + 0.05 * torch.rand(2, 67, 1, generator=g))
    assert float(torch.sqrt(R.d2(cloud[:, None], q[:, :, None])).min()) >= 0.6
    bad, s32 = R.sample_unshifted(q, cloud, fea, "gaussian", 0.05, torch.float32)
    assert float(s32.max()) == 0.0 and bool(torch.isnan(bad).all())
    r64, r32 = (R.sample(q, cloud, fea, "gaussian", 0.05, dt) for dt in (torch.float64, torch.float32))
    got = _ops().point_sample(cloud.to(DEV), fea.to(DEV), pts=q.to(DEV), sample_mode="gaussian", gaussian_val=0.05)
    assert bool(torch.isfinite(got).all())
    _gate(f"sample far C={C}", got, r64, r32, R.sample(q, cloud, fea, "gaussian", 0.05, torch.float64, absolute=True))


@pytest.mark.parametrize("mode", ["g02", "inv"])
@pytest.mark.parametrize("nx", [8, 17])
def test_sampler_lattice_equals_point_form_bit_for_bit(nx, mode):
    """Slabs (0, nx^3), (5, 1000) -- cut at the end of the lattice where nx^3 < 1005 -- and (nx^2 + 3, 2 nx^2 + 7)."""
    from vtaco_amd.common import make_3d_grid
    sm, gv = MODES[mode]
    cloud, fea, _ = _scene(67, 65, 32)
    cloud, fea = cloud.to(DEV), fea.to(DEV)
    box = 1.1
    pts = (box * make_3d_grid((-0.5,) * 3, (0.5,) * 3, (nx,) * 3)).to(DEV)
    for first, count in ((0, nx ** 3), (5, min(1000, nx ** 3 - 5)), (nx * nx + 3, 2 * nx * nx + 7)):
        p = pts[first:first + count].unsqueeze(0).expand(2, -1, -1).contiguous()
        a = _ops().point_sample(cloud, fea, pts=p, sample_mode=sm, gaussian_val=gv, want_saved=True)
        b = _ops().point_sample(cloud, fea, lattice=(nx, box, first, count), sample_mode=sm, gaussian_val=gv, want_saved=True)
        for x, y, what in zip(a, b, ("c", "shift", "sum")):
            assert torch.equal(x, y), f"nx={nx} slab ({first}, {count}) {mode}: {what} differs between the lattice and the point form"
    from vtaco_amd._lib import VtError
    with pytest.raises(VtError):
        _ops().point_sample(cloud, fea, lattice=(nx, box, 1, nx ** 3), sample_mode=sm, gaussian_val=gv)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("M,N,C", [(1100, 70, 32), (1100, 33, 96), (67, 65, 128), (513, 3, 32)])
def test_sampler_backward(M, N, C, mode):
    """grad_fea against float64; M = 1100 is three of the kernel's 512-query chunks (the last one partial), 513 two, 67 one."""
    sm, gv = MODES[mode]
    cloud, _, q = _scene(M, N, C)
    grad_c = torch.randn(2, M, C, generator=torch.Generator().manual_seed(7200 + M + N + C))
    r64, r32 = (R.sample_bwd(q, cloud, grad_c, sm, gv, dt) for dt in (torch.float64, torch.float32))
    bound = R.sample_bwd(q, cloud, grad_c, sm, gv, torch.float64, absolute=True)
    cd, qd, gd = cloud.to(DEV), q.to(DEV), grad_c.to(DEV)
    fea = torch.zeros(2, N, C, device=DEV)
    _, shift, total = _ops().point_sample(cd, fea, pts=qd, sample_mode=sm, gaussian_val=gv, want_saved=True)
    got = _ops().point_sample_bwd(cd, qd, shift, total, gd, sm, gv)
    _gate(f"sample_bwd M={M} N={N} C={C} {mode}", got, r64, r32, bound)
    again = _ops().point_sample_bwd(cd, qd, shift, total, gd, sm, gv)
    assert torch.equal(got, again), "two runs of the backward differ"


# ---- farthest-point sampling -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fps_case(N, npoint):
    """The first seed from 7300 whose float64 run keeps every runner-up 2^-20 (relative) below the maximum: at most 20 tried."""
    start = torch.tensor([0, N - 1])
    for seed in range(7300, 7320):
        cloud = torch.rand(2, N, 3, generator=torch.Generator().manual_seed(seed)) - 0.5
        idx, gap = R.fps(cloud, npoint, start, torch.float64)
        if gap >= 2.0 ** -20:
            return cloud, start, idx, gap
    return None


@pytest.mark.parametrize("N,npoint", [(17, 5), (70, 16), (600, 128), (3000, 512)])
def test_fps_equals_reference(N, npoint):
    case = _fps_case(N, npoint)
    assert case is not None, "no seed in 20 keeps the runner-up 2^-20 below the maximum"
    cloud, start, idx, gap = case
    print(f"fps N={N} npoint={npoint}: smallest relative gap {gap:.3e}")
    got = _ops().fps(cloud.to(DEV), npoint, start)
    assert got.dtype == torch.int64 and torch.equal(got.cpu(), idx)
    assert torch.equal(_ops().fps(cloud.to(DEV), npoint, start.to(DEV)).cpu(), idx)              # start indices already on the device


def test_fps_lowest_index_among_equal_maxima():
    """Points on a lattice of eighths, with exact duplicates: every squared distance is exact in float32 and float64 alike, and
    equal maxima occur at most steps -- the lowest index has to win each of them."""
    g = torch.Generator().manual_seed(7350)
    cloud = torch.randint(0, 5, (2, 64, 3), generator=g).float() / 8
    cloud[:, 40:50] = cloud[:, 3:13]
    start = torch.tensor([7, 63])
    idx, _ = R.fps(cloud, 16, start, torch.float64)
    assert torch.equal(idx, R.fps(cloud, 16, start, torch.float32)[0])
    assert torch.equal(_ops().fps(cloud.to(DEV), 16, start).cpu(), idx)


def test_fps_refuses_short_clouds():
    from vtaco_amd._lib import VtError
    cloud = torch.rand(2, 10, 3, device=DEV)
    with pytest.raises(VtError):
        _ops().fps(cloud, 11, torch.tensor([0, 0]))
    with pytest.raises(VtError):
        _ops().fps(cloud, 4, torch.tensor([0, 10]))
    assert _ops().fps(cloud, 10, torch.tensor([0, 9])).shape == (2, 10)


# ---- ball query --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,S,radius", [(300, 41, 0.2), (10, 3, 0.4), (150, 64, 0.25)])
def test_ball_query_equals_reference(N, S, radius):
    for seed in range(7400, 7420):
        g = torch.Generator().manual_seed(seed)
        cloud = torch.rand(2, N, 3, generator=g) - 0.5
        centres = R.index_points(cloud, torch.stack([torch.randperm(N, generator=g)[:S] for _ in range(2)]))
        sq = R.d2(cloud.double()[:, None], centres.double()[:, :, None])
        if float((sq - radius ** 2).abs().min()) >= 1e-5:
            break
    else:
        pytest.fail("no seed in 20 keeps every pair 1e-5 away from radius^2")
    counts = (sq <= radius ** 2).sum(dim=-1)
    nsample = int(counts.flatten().sort()[0][counts.numel() // 2])                               # the median row has exactly nsample
    assert bool((counts < nsample).any()) and bool((counts == nsample).any()) and bool((counts > nsample).any())
    for ns in (nsample, 2 * N):                                                                  # and more asked for than the cloud holds
        rows, margin = R.ball_query(cloud, centres, radius, ns, torch.float64)
        assert margin >= 1e-5
        got = _ops().ball_query(cloud.to(DEV), centres.to(DEV), radius, ns)
        assert got.dtype == torch.int64 and torch.equal(got.cpu(), rows), f"N={N} S={S} nsample={ns}"


def test_ball_query_empty_row_stays_in_bounds():
    cloud = torch.rand(1, 50, 3) - 0.5
    centres = torch.tensor([[[3.0, 3.0, 3.0], [0.0, 0.0, 0.0]]])
    got = _ops().ball_query(cloud.to(DEV), centres.to(DEV), 0.3, 8).cpu()
    assert bool((got[0, 0] == 0).all()) and torch.equal(got, R.ball_query(cloud, centres, 0.3, 8)[0])


# ---- three nearest neighbours ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 2, 3, 128])
def test_three_nn(S):
    N, D = 200, 16
    for seed in range(7500, 7520):
        g = torch.Generator().manual_seed(seed + S)
        src = torch.rand(2, S, 3, generator=g) - 0.5
        tgt = torch.rand(2, N, 3, generator=g) - 0.5
        tgt[:, :min(S, 10)] = src[:, :min(S, 10)]                                                # targets that are sources
        idx, w64, gap = R.three_nn(tgt, src, torch.float64)
        if gap >= 2.0 ** -20:
            break
    else:
        pytest.fail("no seed in 20 keeps the third and fourth nearest 2^-20 apart")
    f = torch.randn(2, S, D, generator=g)
    gi, gw = _ops().three_nn(tgt.to(DEV), src.to(DEV))
    k = min(3, S)
    assert gi.shape == gw.shape == (2, N, k) and gi.dtype == torch.int64
    assert torch.equal(gi.cpu().sort(dim=-1)[0], idx.sort(dim=-1)[0])
    i32, w32, _ = R.three_nn(tgt, src, torch.float32)
    _gate(f"three_nn S={S}", R.interpolate(f, gi.cpu(), gw.cpu()), R.interpolate(f.double(), idx, w64), R.interpolate(f, i32, w32),
          R.interpolate(f.double(), idx, w64, absolute=True))
    if S == 1:
        assert bool((gi == 0).all()) and bool((gw == 1).all())                                   # the reference's repeat branch
