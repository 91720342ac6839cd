"""CPU: tests/emd_ref.py on its own -- the f32 restatement of vt_emd_auction passes the float64 certificate against scipy on every
case builder, is equivariant under powers of two (the scale rule's contract), keeps the earlier absolute epsilon's livelock on record,
and the certificate rejects a doctored result."""
import numpy as np
import pytest

import emd_ref as E

SCALE_CASES = (("random", 128, 128), ("lattice", 128, 128), ("random", 96, 128))
SCALE_K = (-10, -3, 4, 8, 12)


def run(a, b, **kw):
    r = E.auction_f32(a, b, **kw)
    assert isinstance(r, E.Auction), r
    return r, E.certificate(a, b, r.assign, r.prices, E.emd_f64(a, b, r.assign), r.eps_last, use_scipy=True)


@pytest.mark.parametrize("name", sorted(E.BUILDERS))
def test_restatement_passes_the_certificate_at_128(name):
    a, b = E.case(name, 128, 128)
    r, c = run(a, b)
    assert c.bound == "scipy" and c.excess <= 1.0
    if name in ("identical", "coincident"):
        assert E.emd_f64(a, b, r.assign) == 0.0
    if name == "coincident":
        assert r.phases == 1 and r.rounds == 128 and r.eps_last == float(np.float32(E.EPS_FINAL))


@pytest.mark.parametrize("name", ("random", "lattice"))
@pytest.mark.parametrize("N,M", ((1, 65), (65, 1), (3, 257), (257, 3)))
def test_restatement_passes_the_certificate_at_lopsided_sizes(name, N, M):
    a, b = E.case(name, N, M)
    r, c = run(a, b)
    assert len(r.assign) == max(N, M) and c.bound == "scipy"


def test_last_epsilon_follows_the_binade_of_the_cost_range():
    f = np.float32
    for crange, e in ((1.0, 0), (1.99, 0), (2.0, 1), (0.99, -1), (0.5, -1), (460.0, 8), (2.0 ** -10, -10)):
        assert E.eps_end_f32(f(crange)) == f(E.EPS_FINAL) * f(2.0) ** e
        assert E.eps_end_f32(f(crange), absolute_eps=True) == f(E.EPS_FINAL)
    assert E.eps_end_f32(f(0)) == f(E.EPS_FINAL)


@pytest.mark.parametrize("name,N,M", SCALE_CASES)
def test_scale_equivariance(name, N, M):
    a, b = E.case(name, N, M)
    r0, _ = run(a, b)
    for k in SCALE_K:
        s = np.float32(2.0 ** k)
        r, _ = run(a * s, b * s)
        assert np.array_equal(r.assign, r0.assign), k
        assert np.array_equal(r.prices, r0.prices * s), k
        assert (r.rounds, r.phases) == (r0.rounds, r0.phases), k
        assert r.eps_last == r0.eps_last * float(s), k


def test_the_absolute_epsilon_livelocks_at_scale_and_the_scale_rule_does_not():
    """lattice(128, 128) * 256: prices pass 32, where price + 1e-6 == price in f32, so a tied bid no longer raises the price and two
    persons take one object from each other for ever.  With the epsilon tied to the cost range's binade the scaled problem is the
    unscaled one."""
    a, b = E.lattice(128, 128)
    r0, _ = run(a, b)
    s = np.float32(256)
    assert E.auction_f32(a * s, b * s, max_rounds=30_000, absolute_eps=True) == E.DID_NOT_FINISH
    r, _ = run(a * s, b * s, max_rounds=30_000)
    assert r.rounds <= 4 * r0.rounds
    # at unit scale the two rules are one rule
    old = E.auction_f32(a, b, absolute_eps=True)
    assert E.crange_f32(a, b) >= 1 and E.crange_f32(a, b) < 2
    assert np.array_equal(old.assign, r0.assign) and np.array_equal(old.prices, r0.prices) and old.rounds == r0.rounds


def test_non_finite_input_is_named_before_any_round():
    a, b = E.random(8, 8)
    for bad in (np.nan, np.inf, -np.inf):
        x = a.copy()
        x[3, 1] = bad
        assert E.auction_f32(x, b) == E.NON_FINITE and E.auction_f32(b, x) == E.NON_FINITE
    assert E.auction_f32(a * np.float32(3e38), -b * np.float32(3e38)) == E.NON_FINITE      # finite, the range is not


def test_max_rounds_marks_an_unfinished_auction():
    a, b = E.random(64, 64)
    assert E.auction_f32(a, b, max_rounds=2) == E.DID_NOT_FINISH


def test_certificate_rejects_doctored_results():
    a, b = E.random(128, 128)
    r, c = run(a, b)
    n, tol = 128, r.eps_last + c.R
    cost = E.cost_rows_f64(a, b, 0, n)
    # the swap of two persons' objects that raises the cost most: far more than n (eps_last + R)
    i = np.arange(n)
    own = cost[i, r.assign]
    rise = cost[:, r.assign] + cost[:, r.assign].T - own[:, None] - own[None, :]
    i0, i1 = np.unravel_index(np.argmax(rise), rise.shape)
    assert rise[i0, i1] > n * tol
    swapped = r.assign.copy()
    swapped[[i0, i1]] = swapped[[i1, i0]]
    emd = E.emd_f64(a, b, swapped)                                   # consistent with the doctored assignment: only optimality is off
    with pytest.raises(AssertionError, match="slackness"):
        E.certificate(a, b, swapped, r.prices, emd, r.eps_last)
    with pytest.raises(AssertionError, match="float64 cost"):
        E.certificate(a, b, r.assign, r.prices, E.emd_f64(a, b, r.assign) * (1 + 1e-9), r.eps_last)
    with pytest.raises(AssertionError, match="permutation"):
        E.certificate(a, b, np.where(i == i0, r.assign[i1], r.assign), r.prices, emd, r.eps_last)
    # the dual bound gates too, without scipy
    assert E.certificate(a, b, r.assign, r.prices, E.emd_f64(a, b, r.assign), r.eps_last, use_scipy=False).bound == "dual"
    with pytest.raises(AssertionError):
        E.certificate(a, b, swapped, r.prices, emd, r.eps_last, use_scipy=False)
