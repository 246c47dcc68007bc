"""CPU checks of what tests/test_gpu_american_solver.py stands on: the solver / decision harness compiles for gfx950
with the library's flags, and the references of tests/american_restate.py are right — the exact rational solve against
numpy's least squares, the fp64 replica of am_solve against the exact solve over the accuracy ladder (the source of
the constant C of the ladder's bound), and the exact fused multiply-add against independent forms of it."""
import math
import random
from fractions import Fraction

import numpy as np
import pytest

import american_restate as ar
import american_solve_harness as ash


def test_harness_compiles_with_the_library_flags(tmp_path):
    L = ash.load(ash.compile_harness(tmp_path))
    assert L.as_solve(0, 3, None, -1.0, None, None) == 0
    assert L.as_decide(0, 3, None, None, None, 1, None, None, None, None) == 0


@pytest.mark.parametrize("m", [2, 3, 4])
@pytest.mark.parametrize("lo,hi", [(-0.9, -0.05), (0.02, 2.5), (-0.3, -0.2)])
def test_exact_solve_against_numpy_least_squares(m, lo, hi):
    rng = np.random.default_rng([m, int(abs(lo) * 100)])
    u = rng.uniform(lo, hi, 3000)
    V = ar.ladder_values(u, rng.standard_normal(3000))
    beta, piv = ar.solve_record(ar.record(u, V), m)
    X = np.vander(u, m, increasing=True)
    norm = np.sqrt((X * X).sum(axis=0))
    want = np.linalg.lstsq(X / norm, V, rcond=None)[0] / norm
    fit, ref = X @ np.array([float(b) for b in beta]), X @ want
    # the record's sums carry n 2^-53 of relative rounding, the fit 1 / (smallest pivot) of that
    assert np.abs(fit - ref).max() <= 3000 * ar.EPS / float(min(piv)) * np.abs(ref).max()
    # the exact scaled pivots are those of the Cholesky of the scaled matrix
    A = (X / norm).T @ (X / norm)
    assert np.allclose(np.diag(np.linalg.cholesky(A)) ** 2, [float(p) for p in piv], rtol=1e-6, atol=1e-13)
    assert piv[0] == 1


def test_exact_solve_of_small_systems_by_hand():
    # three points on a line: V = 2 - 3 u exactly, pivots 1 and 1 - (sum u)^2 / (n sum u^2)
    u = np.array([-0.5, -0.25, -0.125, -0.75] * 2)
    beta, piv = ar.solve_record(ar.record(u, 2.0 - 3.0 * u), 2)
    assert beta == [Fraction(2), Fraction(-3)]
    assert piv == [1, 1 - Fraction(float(u.sum())) ** 2 / (8 * Fraction(float((u * u).sum())))]
    assert ar.solve_record(np.zeros(12), 3) == (None, [0])
    one_point = ar.record(np.full(20, -0.25), np.ones(20))
    assert ar.solve_record(one_point, 2) == (None, [1, 0])


@pytest.fixture(scope="module")
def ladder():
    return ar.ladder()


def test_ladder_shape(ladder):
    """what the GPU test needs of the ladder, known from the exact pivots alone"""
    piv = np.array([k["pivot"] for k in ladder])
    assert ar.band_share(ladder) <= 0.02
    assert (piv > ar.BAND[1]).sum() > 1000 and (piv < ar.BAND[0]).sum() > 300 and 4e-15 < piv.min() < 1e-14
    assert piv[piv > ar.BAND[1]].min() < 2.5 * ar.PIVOT_MIN and piv[piv < ar.BAND[0]].max() > 0.4 * ar.PIVOT_MIN
    assert {k["m"] for k in ladder} == {2, 3, 4} and {k["put"] for k in ladder} == {True, False}
    assert min(k["rho"] for k in ladder) == 1.0
    for m in (2, 3, 4):
        assert {k["n"] for k in ladder if k["m"] == m} == {4 * m, 64, 4000, 1_000_000}
    assert all(-1 < k["c"] < 0 if k["put"] else 0 < k["c"] < 3 for k in ladder)


# max of error * pivot / 2^-53 of the replica over the ladder, per m (DESIGN §11's table), to two digits
REPLICA_MAX = {2: 2.43, 3: 2.53, 4: 4.70}


def test_replica_against_the_exact_solve_over_the_ladder(ladder, record_property):
    """am_solve's arithmetic in fp64 without contraction: regressed above the band, not below it, and the measured
    constant of its fitted-value error, error * pivot / 2^-53, is what ar.C_REPLICA states"""
    worst, worst_accepted = {2: 0.0, 3: 0.0, 4: 0.0}, 0.0
    for k in ladder:
        ok, beta = ar.solve_replica(k["rec"], k["m"])
        if k["pivot"] > ar.BAND[1]:
            assert ok, (k["m"], k["c"], k["rho"], k["n"], k["pivot"])
            worst[k["m"]] = max(worst[k["m"]], ar.fit_error(beta, k["beta"], k["u"]) * k["pivot"] / ar.EPS)
        elif k["pivot"] < ar.BAND[0]:
            assert not ok, (k["m"], k["c"], k["rho"], k["n"], k["pivot"])
        if ok:
            worst_accepted = max(worst_accepted, ar.fit_error(beta, k["beta"], k["u"]))
    for m, w in worst.items():
        record_property(f"replica_error_times_pivot_over_eps_m{m}", w)
        assert abs(w - REPLICA_MAX[m]) <= 0.005, (m, w)
    record_property("replica_worst_error_of_an_accepted_record", worst_accepted)
    print(f"replica: max error * pivot / 2^-53 = {worst}, worst accepted error {worst_accepted:.3e}")
    assert 0.9 * ar.C_REPLICA <= max(worst.values()) <= ar.C_REPLICA
    assert ar.C_DEVICE == 4 * ar.C_REPLICA
    assert 1.4e-6 < worst_accepted < 1.6e-6   # 1.5e-6 under the shipped threshold


def test_replica_under_the_first_threshold():
    """DESIGN §11's reason for the threshold: under 1e-12, as first shipped, the replica accepts a record that it fits
    to 1.5e-4 of scale only (m = 4, c = 1.5, 16 points, pivot 2.5e-12), above the 1e-4 at which a boundary moves"""
    first = ar.PIVOT_MIN_FIRST
    cases = ar.ladder(first, near_only=True)
    assert ar.band_share(cases, first) == 0 and len(cases) > 900
    piv = np.array([k["pivot"] for k in cases])
    assert 2 * first < piv[piv > first].min() < 2.5 * first and piv.max() < 100 * first
    worst = (0.0,)
    for k in cases:
        ok, beta = ar.solve_replica(k["rec"], k["m"], first)
        assert ok == (k["pivot"] > first)
        if ok:
            worst = max(worst, (ar.fit_error(beta, k["beta"], k["u"]), k["m"], k["c"], k["n"], k["pivot"]))
    assert 1.5e-4 < worst[0] < 1.56e-4 and worst[1:4] == (4, 1.5, 16) and 2.4e-12 < worst[4] < 2.6e-12, worst


def test_shape_matrix_covers_what_it_claims():
    S = ar.SHAPES
    assert {(m, p) for _, _, m, p, _ in S} == {(m, p) for m in (2, 3, 4) for p in (64, 32)}
    assert {(k, put) for put, k, _, _, _ in S} == {(k, put) for k in (1, 3, 7) for put in (True, False)}
    assert {n % 4 for _, _, _, p, n in S if p == 32} == {0, 1, 2, 3}
    assert any(n % 2 == 1 for _, _, _, p, n in S if p == 64) and all(n % k == 0 for _, k, _, _, n in S)


def test_replica_agrees_with_fit_on_a_well_conditioned_date():
    rng = np.random.default_rng(5)
    S = rng.uniform(25.0, 39.9, 5000)
    V = 0.95 * (40.0 - S) + rng.standard_normal(5000)
    ok_fit, beta_fit = ar.fit(S, V, 40.0, 3)
    ok, beta = ar.solve_replica(ar.record(S / 40.0 - 1.0, V), 3)
    assert ok and ok_fit and np.allclose(beta, beta_fit, rtol=1e-9)
    assert ar.fit(S[:11], V[:11], 40.0, 3) == (False, None) and not ar.solve_replica(ar.record(S[:11], V[:11]), 3)[0]


def fma_int(a, b, c):
    """a third form, for the cross-check: scaled to integers through Fraction's numerators"""
    x = Fraction(a) * Fraction(b) + Fraction(c)
    return x.numerator / x.denominator


def test_fma_emulation():
    rnd = random.Random(11)
    for i in range(60_000):
        a, b, c = (rnd.gauss(0, 1) * 2.0 ** rnd.randint(-40, 40) for _ in range(3))
        if i % 3 == 0:
            c = -a * b            # the product's rounding error is all that is left
        if i % 7 == 0:
            a, b = float(np.float32(a)), float(np.float32(b))   # 24-bit factors: the product is exact in fp64
            assert ar.fma(a, b, c) == a * b + c
        got = ar.fma(a, b, c)
        assert got == ar.fma_fraction(a, b, c) == fma_int(a, b, c)
        if hasattr(math, "fma"):
            assert got == math.fma(a, b, c)
        else:   # an x87 long double holds the product to 64 bits: the fused result is within an fp64 ulp of it
            ld = np.longdouble(a) * np.longdouble(b) + np.longdouble(c)
            assert abs(np.longdouble(got) - ld) <= abs(ld) * 2.0 ** -52 + abs(np.longdouble(a) * b) * 2.0 ** -63
    # one rounding, not two: (1 + e)^2 - 1 keeps its e^2
    e = 2.0 ** -30
    assert ar.fma(1 + e, 1 + e, -1.0) == 2 * e + e * e != (1 + e) * (1 + e) - 1.0
    assert ar.fma(1e308, 10.0, -1e308) == math.inf and ar.fma(-1e308, 10.0, 0.0) == -math.inf
    assert ar.fma(5e-324, 0.5, 0.0) == 0.0 and ar.fma(5e-324, 0.75, 0.0) == 5e-324   # subnormal results round once
    assert ar.fma(2.0 ** -600, 2.0 ** -600, 2.0 ** -1074) == 2.0 ** -1074
    for a, b, c, sign in ((-0.0, 1.0, -0.0, -1), (0.0, 1.0, -0.0, 1), (3.0, -1.0, 3.0, 1), (-0.0, 0.0, 0.0, 1)):
        assert math.copysign(1.0, ar.fma(a, b, c)) == sign
    assert ar.fma(math.inf, 2.0, 1.0) == math.inf and math.isnan(ar.fma(math.inf, 0.0, 1.0))


def test_decision_reference():
    beta = [1.0, 2.0, -4.0]
    # u = -0.25: 1 + 2 (-0.25) - 4 (0.0625) = 0.25 exactly
    assert ar.continuation(beta, -0.25) == 0.25
    assert ar.decide(beta, 0.5, 40.0, True, 30.0) == (True, 5.0, 0.25)
    assert ar.decide(beta, 0.025, 40.0, True, 30.0) == (False, 0.25, 0.25)      # equal is not greater
    assert ar.decide(beta, 0.5, 40.0, True, 40.0) == (False, None, 1.0)         # h = 0 never exercises
    assert ar.decide(beta, 0.5, 40.0, False, 30.0) == (False, None, 0.25)
    assert ar.decide(beta, 0.5, 40.0, False, 50.0)[:2] == (True, 5.0)
