"""GPU: vt_emd_auction held to the float64 certificate of tests/emd_ref.py where the auction can go wrong -- sizes below a wave, across
the 1024-thread stride and far from square, exact ties (lattice, identical and coincident clouds), both sides of the cache_a
boundary, clouds scaled by powers of two (the scale rule's equivariance), a mixed batch, non-finite input -- and vt_chamfer_nn at
its tile boundaries.

Every auction but the two at the cache_a boundary runs under max_rounds = 4 r + 1000, r the f32 restatement's round count of the
case: a kernel that livelocks stops within milliseconds.  The restatement's square root is correctly rounded and the kernel's is
good to 1 ulp, so the two are never compared bit for bit.  Every case prints one line (N, M, scale, the kernel's rounds / bids /
phases, the restatement's rounds, emd, the optimum or the dual bound, the worst slackness excess / (eps_last + R)) and, with
VTACO_RATIO_LOG naming a file, appends it (profiles/emd_f64_ratios.txt is made so)."""
import functools

import numpy as np
import pytest
import torch

import emd_ref as E
from test_metrics_gpu import check_nn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = torch.from_numpy

SIZES = ((1, 1), (2, 2), (1, 2), (2, 1), (63, 63), (64, 64), (65, 65), (1, 65), (65, 1), (3, 257), (257, 3), (1000, 1025), (1025, 1000))
SCALE_CASES = (("random", 128, 128), ("lattice", 128, 128), ("random", 96, 128))
SCALE_K = (-10, 4, 8, 12)


@functools.lru_cache(maxsize=None)
def restated(name, N, M):
    """The restatement's result for the unscaled case (it is equivariant under powers of two: tests/test_emd_ref_cpu.py)."""
    r = E.auction_f32(*E.case(name, N, M))
    assert isinstance(r, E.Auction), r
    return r


def cap(name, N, M):
    return 4 * restated(name, N, M).rounds + 1000


def solve(a, b, max_rounds=None):
    from vtaco_amd import ops
    return ops.emd_assignment(T(a)[None].to(DEV), T(b)[None].to(DEV), max_rounds=max_rounds)


def certify(tag, a, b, res, k=0, scale=1.0, r_rounds=None):
    """Problem k of ``res`` through the certificate; one line of the record."""
    assign, prices = res.assign[k].cpu().numpy(), res.prices[k].cpu().numpy()
    emd, eps = float(res.emd[k]), float(res.eps[k])
    assert eps == float(E.eps_end_f32(E.crange_f32(a, b)))           # the scale rule: the last epsilon, in input units
    c = E.certificate(a, b, assign, prices, emd, eps)
    rounds = int(res.rounds[k])
    ratio = "-" if r_rounds is None else f"{rounds / r_rounds:.3f}"
    E.record(f"{tag} N {len(a)} M {len(b)} scale {scale:g}",
             f"rounds {rounds} bids {int(res.bids[k])} phases {int(res.phases[k])} restated rounds {'-' if r_rounds is None else r_rounds} "
             f"(ratio {ratio}) emd {emd:.9g} {c.bound} {c.opt:.9g} eps {eps:.3e} slackness excess / (eps + R) {c.excess:.3f}")
    return c


@pytest.mark.parametrize("name", ("random", "lattice"))
@pytest.mark.parametrize("N,M", SIZES)
def test_emd_sizes_at_the_kernel_boundaries(name, N, M):
    a, b = E.case(name, N, M)
    res = solve(a, b, cap(name, N, M))
    assert res.assign.shape == (1, max(N, M)) and res.eps.shape == (1,) and res.eps.dtype == np.float64
    certify(name, a, b, res, r_rounds=restated(name, N, M).rounds)


@pytest.mark.parametrize("name,n", (("identical", 257), ("coincident", 1), ("coincident", 257), ("offset", 257)))
def test_emd_degenerate_clouds(name, n):
    a, b = E.case(name, n)
    res = solve(a, b, cap(name, n, None))
    certify(name, a, b, res, r_rounds=restated(name, n, None).rounds)
    if name in ("identical", "coincident"):
        assert float(res.emd[0]) == 0.0
    if name == "coincident":
        assert int(res.phases[0]) == 1 and int(res.rounds[0]) == n    # cost range 0: one phase; every value ties: one column per round


@pytest.mark.parametrize("n", (3876, 3877))
def test_emd_both_sides_of_the_cache_a_boundary(n):
    """3876 points a side is the last size whose bidders' coordinates live in LDS; 3877 reads them from global memory.  The
    library's default max_rounds; the optimum's stand-in is the dual bound of the returned prices (no scipy at this size)."""
    a, b = E.random(n, n)
    res = solve(a, b)
    c = certify("random", a, b, res)
    assert c.bound == "dual"


@pytest.mark.parametrize("name,N,M", SCALE_CASES)
def test_emd_scale_equivariance_on_the_device(name, N, M):
    a, b = E.case(name, N, M)
    r = restated(name, N, M).rounds
    base = solve(a, b, cap(name, N, M))
    certify(name, a, b, base, r_rounds=r)
    for k in SCALE_K:
        s = np.float32(2.0 ** k)
        res = solve(a * s, b * s, cap(name, N, M))
        assert torch.equal(res.assign, base.assign), k
        assert torch.equal(res.prices, base.prices * float(s)), k
        assert abs(float(res.emd[0]) - float(base.emd[0]) * float(s)) <= 1e-15 * float(base.emd[0]) * float(s), k
        assert (int(res.rounds[0]), int(res.bids[0]), int(res.phases[0])) == (int(base.rounds[0]), int(base.bids[0]), int(base.phases[0])), k
        assert float(res.eps[0]) == float(base.eps[0]) * float(s), k
        certify(name, a * s, b * s, res, scale=float(s), r_rounds=r)


def test_emd_mixed_batch_equals_its_single_problems():
    from vtaco_amd import ops
    n = 257
    names = (("random", n, n), ("lattice", n, n), ("identical", n, None), ("coincident", n, None), ("lattice", n, n))
    scales = (1.0, 1.0, 1.0, 1.0, 1024.0)
    clouds = [tuple(x * np.float32(s) for x in E.case(*c)) for c, s in zip(names, scales)]
    caps = [cap(*c) for c in names]
    ta = T(np.stack([a for a, _ in clouds])).to(DEV)
    tb = T(np.stack([b for _, b in clouds])).to(DEV)
    res = ops.emd_assignment(ta, tb, max_rounds=max(caps))
    again = ops.emd_assignment(ta, tb, max_rounds=max(caps))
    for field in ("assign", "prices"):
        assert torch.equal(getattr(again, field), getattr(res, field)), field
    assert np.array_equal(again.emd, res.emd) and np.array_equal(again.rounds, res.rounds) and np.array_equal(again.eps, res.eps)
    for k, ((a, b), c, s) in enumerate(zip(clouds, names, scales)):
        certify(f"batch[{k}] {c[0]}", a, b, res, k=k, scale=s, r_rounds=restated(*c).rounds)
        single = solve(a, b, caps[k])
        assert torch.equal(single.assign[0], res.assign[k]) and torch.equal(single.prices[0], res.prices[k]), k
        assert single.emd[0] == res.emd[k] and single.rounds[0] == res.rounds[k] and single.eps[0] == res.eps[k], k


@pytest.mark.parametrize("bad,side", ((np.nan, 0), (np.inf, 1)))
def test_emd_non_finite_input_raises_before_the_first_round(bad, side):
    """One NaN (in a) or one inf (in b) in problem 1 of 3: status 2 from the bounding-box pass, no round is run for that problem.  The
    other two problems are identical clouds, done in 9 rounds, so the error names problem 1 alone."""
    from vtaco_amd import ops
    from vtaco_amd._lib import VtError
    a, _ = E.identical(64)
    clouds = [np.stack([a, a, a]), np.stack([a, a, a])]
    clouds[side][1, 37, 2] = bad
    with pytest.raises(VtError, match=r"non-finite.*problems \[1\]"):
        ops.emd_assignment(T(clouds[0]).to(DEV), T(clouds[1]).to(DEV), max_rounds=64)
    x, y = E.random(65, 65)
    certify(f"random after a batch with {bad}", x, y, solve(x, y, cap("random", 65, 65)), r_rounds=restated("random", 65, 65).rounds)


@pytest.mark.parametrize("N", (255, 256, 257))
@pytest.mark.parametrize("M", (1023, 1024, 1025, 2049))
def test_chamfer_nn_at_the_tile_boundaries(N, M):
    """256 queries per workgroup, 1024 targets per LDS tile: one short of, at and one past each, and a third tile of one point."""
    from vtaco_amd import ops
    rng = np.random.RandomState([7, N, M])
    a = (rng.randn(2, N, 3) * 0.2).astype(np.float32)
    b = (rng.randn(2, M, 3) * 0.2).astype(np.float32)
    b[:, ::7] = np.round(b[:, ::7] * 8) / 8                                   # repeated points: ties
    a[:, ::5] = np.round(a[:, ::5] * 8) / 8
    out = [t.cpu().numpy() for t in ops.chamfer_nn(T(a).to(DEV), T(b).to(DEV))]
    for k in range(2):
        check_nn(a[k], b[k], *(o[k] for o in out))
