"""The host's phase-table sampler (`PhaseFunctionTable.rows`, `.sample_mu`, `.turn`, pvtrace_amd/material.py) against
the exact reference of the PvtPhaseTables contract (tests/exact_events.py), one turn at a time, on every case: the row
pick and the inverted CDF in exact rationals, the sine, the azimuth and the basis at 60 digits.  The compiled CDF rows
are held to item 1 of the contract in exact rationals as well.  The same cases, rays and draws hold the kernel in
tests/test_gpu_phase_turn_exact.py; here the reference, its margins and the conditions of `check_phase_conditions` are
proven without a GPU.  The host takes cos and sin of fl(2 pi u3) from numpy, so its bound carries TRIG_HOST where the
kernel's carries TRIG_KERNEL.

Measured on these cases (worst |direction - exact| / bound): 0.126; no ray of any case is ambiguous.  The CDF rows are
within 19 U of the exact quotient (the 1801-point rows; 1.5 U on the small tables)."""
from fractions import Fraction as F

import numpy as np
import pytest
from mpmath import mp, mpf

from oracle import oracle as O
from tests import exact_events as X

SEED = X.SEED
# The draws of a ray started inside the block, in the order of its stream: 0 the free path, 1 the component pick, 2 the
# quantum yield, then u1 (only when the table has several rows), u2, u3 (tests/test_gpu_phase_turn_exact.py anchors
# these positions on the same block with an isotropic phase function).
FIRST_PHASE_DRAW = 3


def case_inputs(case):
    """(positions, directions, wavelengths, u1 or None, u2, u3) of a case."""
    pos, dirs, wl = case.rays()
    draws = np.array([O.uniforms(SEED + i, FIRST_PHASE_DRAW + 3) for i in range(case.n)])
    k = FIRST_PHASE_DRAW
    if case.table.n_wavelength > 1:
        return pos, dirs, wl, draws[:, k], draws[:, k + 1], draws[:, k + 2]
    return pos, dirs, wl, None, draws[:, k], draws[:, k + 1]


def test_the_reference_on_turns_worked_by_hand():
    with mp.workdps(X.DIGITS):
        one = X.TABLES["two-point"]()                      # one segment, whatever p: C = (0, 1), mu = 2 u2 - 1
        assert list(one.cdf[0]) == [0.0, 1.0]
        for u2 in (0.0, 0.25, 0.8125, 1.0 - 2.0 ** -53):
            r = X.exact_phase_turn(one, 555.0, (0.0, 0.0, 1.0), 0.0, u2, 0.0)
            assert r.segment == 0 and r.mu == 2 * F(u2) - 1
        # d = +z: s = 1, a = -1 / 2, e1 = (1, 0, 0), e2 = (0, 1, 0): d' = (st cos, st sin, mu)
        r = X.exact_phase_turn(one, 555.0, (0.0, 0.0, 1.0), 0.0, 0.75, 0.25)       # mu = 1 / 2, phi = pi / 2
        st = mp.sqrt(mpf(3) / 4)
        assert r.s_sign == 1.0 and max(abs(a - b) for a, b in zip(r.direction, (0, st, mpf(1) / 2))) < 1e-55
        r = X.exact_phase_turn(one, 555.0, (0.0, 0.0, 1.0), 0.0, 0.75, 0.0)
        assert max(abs(a - b) for a, b in zip(r.direction, (st, 0, mpf(1) / 2))) < 1e-55
        # d = -z: s = -1, a = 1 / 2, e1 = (1, 0, 0), e2 = (0, -1, 0): d' = (st cos, -st sin, -mu)
        r = X.exact_phase_turn(one, 555.0, (0.0, 0.0, -1.0), 0.0, 0.75, 0.25)
        assert r.s_sign == -1.0 and max(abs(a - b) for a, b in zip(r.direction, (0, -st, -mpf(1) / 2))) < 1e-55
        # dz = -0.0: s = -1, a = 1, about d = (1, 0, -0): e1 = (1 - 1, 0, 1) = (0, 0, 1), e2 = (0, -1, 0)
        r = X.exact_phase_turn(one, 555.0, (1.0, 0.0, -0.0), 0.0, 0.75, 0.0)
        assert r.s_sign == -1.0 and max(abs(a - b) for a, b in zip(r.direction, (mpf(1) / 2, 0, st))) < 1e-55
        r = X.exact_phase_turn(one, 555.0, (1.0, 0.0, 0.0), 0.0, 0.75, 0.0)        # dz = +0.0: e1 = (0, 0, -1)
        assert r.s_sign == 1.0 and max(abs(a - b) for a, b in zip(r.direction, (mpf(1) / 2, 0, -st))) < 1e-55
    # the row pick: t = 0.3 at 530 nm between 500 and 600; u1 < t takes the upper row; the ends clamp with t = 0
    two = X.TABLES["two-row"]()
    assert X.pick_row(two.wavelength, 530.0, 0.2999) [:3] == (1, F(3, 10), (0, 1))
    assert X.pick_row(two.wavelength, 530.0, 0.3)[0] == 1          # (the double 0.3 is below 3 / 10 ...
    assert X.pick_row(two.wavelength, 530.0, 0.30000000000000004)[0] == 0          # ... and its neighbour above)
    assert X.pick_row(two.wavelength, 550.0, 0.5) [:3] == (0, F(1, 2), (0, 1))          # u1 = t exactly: not below it
    assert X.pick_row(two.wavelength, 400.0, 0.0) [:3] == (0, F(0), None)
    assert X.pick_row(two.wavelength, 500.0, 0.0) [:3] == (0, F(0), None)
    assert X.pick_row(two.wavelength, 600.0, 0.0) [:3] == (1, F(0), None)
    assert X.pick_row(two.wavelength, 800.0, 0.999) [:3] == (1, F(0), None)
    # the inverted CDF: a knot belongs to the segment it opens; zero-mass segments are never chosen
    zero = X.TABLES["zero-mass"]()
    cdf = zero.cdf[0]
    assert cdf[0] == cdf[1] == 0.0 and cdf[3] == cdf[4] and cdf[6] == cdf[7] == 1.0
    assert X.invert_cdf(zero.mu, cdf, 0.0) == (1, F(float(zero.mu[1])))
    assert X.invert_cdf(zero.mu, cdf, cdf[3]) == (4, F(float(zero.mu[4])))
    assert X.invert_cdf(zero.mu, cdf, 1.0 - 2.0 ** -53)[0] == 5


def test_an_ambiguous_row_pick_accepts_both_rows_each_with_its_own_direction():
    """No ray of any case is ambiguous, so the two-row branch of `exact_phase_turn` and `judge_phase` is run here: at
    530 nm between rows at 500 and 600 nm t = 3 / 10 is no double, so a t formed in doubles is only known to 3 U t, and
    u1 = the double 0.3 lies within that of it.  Either row is accepted with the direction of ITS cdf; the direction of
    a third choice is not.  Four ulps further the pick is definite and only its own row passes."""
    two = X.TABLES["two-row"]()
    d = (0.6, 0.0, -0.8)
    r = X.exact_phase_turn(two, 530.0, d, 0.3, 0.4, 0.7)
    assert r.ambiguous and sorted(r.rows) == [0, 1] and r.row == 1 and 0 < r.t_margin <= 3 * F(1, 2 ** 53) * r.t
    by_row = {row: [float(c) for c in r.rows[row][2]] for row in (0, 1)}
    assert max(abs(a - b) for a, b in zip(by_row[0], by_row[1])) > 1e-3          # (the rows turn the ray differently)
    X.judge_phase("on-t", [r], [by_row[0]], "hand")
    X.judge_phase("on-t", [r], [by_row[1]], "hand")
    with pytest.raises(AssertionError):
        X.judge_phase("on-t", [r], [[0.5 * (a + b) for a, b in zip(by_row[0], by_row[1])]], "hand")
    for u1, row in ((0.2999999999999998, 1), (0.3000000000000002, 0)):   # (3 U t is two ulps of 0.3)
        clear = X.exact_phase_turn(two, 530.0, d, u1, 0.4, 0.7)
        assert not clear.ambiguous and list(clear.rows) == [row]
        X.judge_phase("off-t", [clear], [by_row[row]], "hand")
        with pytest.raises(AssertionError):
            X.judge_phase("off-t", [clear], [by_row[1 - row]], "hand")


@pytest.mark.parametrize("key", sorted(X.TABLES))
def test_the_compiled_cdf_rows_are_the_trapezoid_integral_of_the_contract(key):
    """Item 1: each row is the trapezoid integral of p in mu with a leading 0, divided by its last entry.  The host
    forms each term 0.5 (p_j + p_j+1)(mu_j+1 - mu_j) with three roundings (the half is exact), sums j + 1 of them in
    order (numpy's cumsum along a row), and divides by the total, itself a sum of n - 1 terms: entry j is within
    (3 + j + 3 + (n - 1) + 1) U = (n + j + 6) U of the exact quotient, relatively (all terms are >= 0)."""
    table = X.TABLES[key]()
    assert table.n_wavelength == len(table.cdf)
    worst = X.check_cdf_rows(table, key)
    print(f"{key}: worst |C_j - exact| / (U exact) {worst:.2f}")


@pytest.mark.parametrize("case", X.PHASE_CASES, ids=[c.name for c in X.PHASE_CASES])
def test_the_host_sampler_agrees_with_the_exact_reference_turn_by_turn(case):
    table = case.table
    pos, dirs, wl, u1, u2, u3 = case_inputs(case)
    refs = X.phase_refs(case, dirs, wl, u1, u2, u3, X.TRIG_HOST)
    X.check_phase_conditions(case, refs)
    rows = table.rows(wl, np.zeros(case.n) if u1 is None else u1)
    mu = table.sample_mu(u2, rows)
    out = table.turn(dirs, mu, u3)
    for i, r in enumerate(refs):
        assert int(rows[i]) in r.rows, (case, i, "row", int(rows[i]), r.row, float(r.t))
        if not r.ambiguous:
            j, exact_mu, _, _ = r.rows[r.row]
            assert abs(F(float(mu[i])) - exact_mu) <= F(1, 2 ** 53) * (4 * abs(exact_mu - F(float(table.mu[j]))) + 1), (case, i, "mu")
    X.judge_phase(case, refs, list(out), "host")
