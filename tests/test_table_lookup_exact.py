"""The table lookups against exact rational arithmetic.

Refractive-index tables n(wavelength) and coating reflectivity tables R(wavelength, angle) are evaluated by three
implementations that must agree: the kernel, the CPU referee (oracle/pvt_oracle.c) and the host classes
(`RefractiveIndexTable.at`, `ReflectivityTable.at`).  The GPU parity tests (tests/test_gpu_table_parity.py) hold the
kernel bit for bit to the referee; this file holds the referee and the host to the exact piecewise-linear (bilinear)
value, computed with `fractions.Fraction`, so that a mistake the referee and the kernel shared would not cancel out.

The rule: clamp at both ends; bracket with xs[m] <= x < xs[m + 1]; t = (x - xa) / (xb - xa); a + t (b - a).  For
R, linear in wavelength on the two bracketing angle rows, then linear in angle; the referee and the kernel bracket the
angle of incidence in radians on the axis deg * (pi / 180) that the packer stores, the host in degrees.

Error bound of one step r = fl(a + fl(t^ * fl(b - a))), t^ = fl(fl(x - xa) / fl(xb - xa)), with u = 2^-53 and
M = max(|a|, |b|) (a and b of one sign, as indices (> 0) and reflectivities (>= 0) are, so |b - a| <= M):
  t^ = t (1 + e_t), |e_t| <= (1 + s1 + s2) u, s1 / s2 = 1 when x - xa / xb - xa round (0 when exact, e.g. by Sterbenz
  in a cell narrower than a factor 2, or when xa = 0); fl(b - a) = (b - a)(1 + e_d), |e_d| <= s3 u, s3 = 1 when b - a
  rounds; the product adds u, the final sum u |r|.  So, to first order,
      |r - exact| <= (2 + s1 + s2 + s3) u |t (b - a)| + u |r| <= (3 + s1 + s2 + s3) u M,
which is at most 6 u M and drops to 3 u M in the usual narrow cell.  At t = 0 (a breakpoint, a clamped end) r = a
exactly.  The bilinear value is a convex combination of the two row values, so their errors carry over at most as
their maximum; the angle step adds its own (3 + s1 + s2 + 1) u M (the difference of two computed rows is taken as
rounding): |R - exact| <= (6 + s1w + s2w + s3w + s1a + s2a) u M, M the largest of the four corner values.  The
tests assert the per-query bound (with the flags of that query, a 1e-9 relative slack for the second-order terms) and,
tighter, the worst case measured over these tables: 1.14 u M for n, 1.28 u M for R, asserted as 1.5 u M.
"""
import math
from fractions import Fraction as F

import numpy as np
import pytest

from oracle import oracle as O
from pvtrace_amd import ReflectivityTable, RefractiveIndexTable

U = F(1, 2 ** 53)
RAD_PER_DEG = 3.14159265358979323846 / 180.0   # (the packer's constant, pvt_scene_pack.h)
BIG = np.finfo(np.float64).max


def up(x, k=1):
    for _ in range(k):
        x = float(np.nextafter(x, np.inf))
    return x


def exact_sub(a, b):
    """1 when the double subtraction a - b rounds, else 0."""
    return int(F(a - b) != F(a) - F(b))


def exact_lerp(xs, vs, x):
    """(exact value, t == 0 in the rule, flags s1 + s2 + s3, M) of the piecewise-linear lookup at x."""
    n = len(xs)
    if not x > xs[0]:
        return F(vs[0]), True, 0, abs(vs[0])
    if not x < xs[-1]:
        return F(vs[-1]), True, 0, abs(vs[-1])
    lo = int(np.searchsorted(xs, x, side="right")) - 1
    xa, xb, a, b = xs[lo], xs[lo + 1], vs[lo], vs[lo + 1]
    t = (F(x) - F(xa)) / (F(xb) - F(xa))
    flags = exact_sub(x, xa) + exact_sub(xb, xa) + exact_sub(b, a)
    return F(a) + t * (F(b) - F(a)), x == xa, flags, max(abs(a), abs(b))


def within(got, want, flags, m, steps=1):
    bound = (3 * steps + flags) * U * F(m) * F(1 + 1e-9)
    err = abs(F(got) - want)
    return err <= bound, float(err / (U * F(m))) if m else 0.0


def queries(xs, extra=()):
    """Every breakpoint, one ulp either side of it, mid-cell and a third of the way, far outside both ends and the
    largest finite doubles."""
    q = []
    for x in xs:
        q += [x, up(x), float(np.nextafter(x, -np.inf))]
    for a, b in zip(xs[:-1], xs[1:]):
        q += [a + (b - a) / 2.0, a + (b - a) / 3.0, b - (b - a) / 7.0]
    q += [xs[0] - 1e3, xs[-1] + 1e3, xs[0] * 1e-3 if xs[0] > 0 else xs[0] * 1e3, -BIG, BIG, *extra]
    return [float(v) for v in q if math.isfinite(v)]


# -- refractive-index tables --------------------------------------------------------------------------------------------
rng = np.random.default_rng(11)
_r40 = np.sort(rng.uniform(300.0, 1100.0, 40))
INDEX_TABLES = {
    "one_point": ([555.0], [1.49]),
    "two_points": ([400.0, 800.0], [1.40, 1.70]),
    "non_uniform": ([350.0, 351.5, 420.0, 421.0, 700.0, 1000.0], [1.52, 1.519, 1.51, 1.6, 1.45, 1.45]),
    "ulp_apart": ([500.0, up(500.0), up(500.0, 2), 600.0], [1.3, 1.9, 1.4, 1.5]),
    "wide_cells": ([1.0, 3.0, 1000.0, 1e6], [1.1, 2.3, 1.7, 1.2]),   # xb > 2 xa: x - xa and xb - xa round
    "steep_rising": ([500.0, 500.001], [up(1e-100), float(np.nextafter(1e100, 0.0))]),
    "steep_falling": ([500.0, 501.0], [float(np.nextafter(1e100, 0.0)), up(1e-100)]),
    "flat": ([300.0, 600.0, 900.0], [1.5, 1.5, 1.5]),
    "one_ulp_steps": ([300.0, 600.0, 900.0], [1.5, up(1.5), 1.5]),
    "extreme_axis": ([1e-300, 1e300], [1.2, 2.9]),
    "random_40": (_r40.tolist(), rng.uniform(1.0, 2.5, 40).tolist()),
}


@pytest.mark.parametrize("name", sorted(INDEX_TABLES))
def test_index_table_lookup_is_exact_where_it_must_be_and_bounded_elsewhere(name):
    xs, vs = (np.array(v, dtype=np.float64) for v in INDEX_TABLES[name])
    table = RefractiveIndexTable(xs, vs)
    worst = 0.0
    for x in queries(xs.tolist()):
        want, at_node, flags, m = exact_lerp(xs, vs, x)
        got = O.index_at(xs, vs, x)
        host = table.at(x)
        assert got == host or (math.isnan(got) and math.isnan(host)), (name, x, got, host)   # bit-equal
        if at_node or len(set(vs.tolist())) == 1:
            assert F(got) == want, (name, x, got, float(want))                                  # exact
        ok, ulps = within(got, want, flags, m)
        assert ok, (name, x, got, float(want), ulps, flags)
        worst = max(worst, ulps)
    assert worst <= 1.5   # (measured 1.14 u M; the proven bound is 3-6 u M)


def test_index_lookup_clamps_and_hits_every_breakpoint_exactly():
    xs, vs = np.array([400.0, 500.0, 600.0]), np.array([1.4, 1.45, 1.7])
    for x, want in ((-BIG, 1.4), (0.0, 1.4), (400.0, 1.4), (500.0, 1.45), (600.0, 1.7), (1e9, 1.7), (BIG, 1.7)):
        assert O.index_at(xs, vs, x) == want
    # one ulp either side of a breakpoint lies in the cell on that side (steep enough to show in the last bits)
    vs = np.array([1.0, 1e6, 4e6])
    assert O.index_at(xs, vs, float(np.nextafter(500.0, 0.0))) < 1e6 == O.index_at(xs, vs, 500.0) < O.index_at(xs, vs, up(500.0))


# -- coating reflectivity tables ----------------------------------------------------------------------------------------
_w = np.array([400.0, 430.0, 555.5, 600.0, 820.0])
_a = np.array([0.0, 10.0, 45.0, 89.0, 90.0])
R_TABLES = {
    "full": (_w, _a, np.clip(rng.uniform(-0.2, 1.2, (5, 5)), 0.0, 1.0)),
    "nw1": (np.array([555.0]), np.array([0.0, 30.0, 60.0, 90.0]), np.array([[0.9], [0.6], [0.2], [0.0]])),
    "na1_none": (np.array([400.0, 500.0, 800.0]), None, np.array([0.1, 0.8, 0.3])),
    "na1_45deg": (np.array([400.0, 500.0, 800.0]), np.array([45.0]), np.array([[0.1, 0.8, 0.3]])),
    "one_by_one": (np.array([555.0]), np.array([12.0]), np.array([[0.37]])),
    "wavelength_step": (np.array([300.0, 599.0, 601.0, 1000.0]), None, np.array([1.0, 1.0, 0.0, 0.0])),
    "angle_step": (np.array([300.0, 1000.0]), np.array([0.0, 29.0, 31.0, 90.0]),
                   np.array([[1.0, 1.0], [1.0, 1.0], [0.0, 0.0], [0.0, 0.0]])),
    "wide_angle_cells": (np.array([1.0, 3.0, 900.0]), np.array([0.0, 1.0, 7.0, 90.0]),
                         np.array([[0.0, 1.0, 0.5], [1.0, 0.0, 0.25], [0.3, 0.6, 0.9], [1.0, 1.0, 0.0]])),
    "constant": (np.array([300.0, 550.0, 1000.0]), np.array([0.0, 45.0, 90.0]), np.full((3, 3), 0.3)),
}


def r_axes(name):
    w, a, v = R_TABLES[name]
    table = ReflectivityTable(w, v, angle=a)
    ang = table._angle_axis
    return table, w, ang, np.asarray(table._grid)


def exact_bilinear(w, ang_axis, grid, wl, ang):
    """Exact R on the given axes (degrees for the host, the packer's radians for the referee)."""
    def row(k):
        return exact_lerp(w, grid[k], wl)
    ta_zero = True
    if not ang > ang_axis[0]:
        k0 = k1 = 0
        ta = F(0)
    elif not ang < ang_axis[-1]:
        k0 = k1 = len(ang_axis) - 1
        ta = F(0)
    else:
        k0 = int(np.searchsorted(ang_axis, ang, side="right")) - 1
        k1 = k0 + 1
        ta = (F(ang) - F(ang_axis[k0])) / (F(ang_axis[k1]) - F(ang_axis[k0]))
        ta_zero = ang == ang_axis[k0]
    r0, w_node, wflags0, _ = row(k0)
    r1, _, wflags1, _ = row(k1)
    wflags = max(wflags0, wflags1)
    aflags = 0 if ta_zero else exact_sub(ang, ang_axis[k0]) + exact_sub(ang_axis[k1], ang_axis[k0]) + 1
    lo = int(np.searchsorted(w, wl, side="right")) - 1
    cols = sorted({min(max(lo, 0), len(w) - 1), min(max(lo + 1, 0), len(w) - 1)})
    m = max(abs(grid[k][c]) for k in (k0, k1) for c in cols)
    return r0 + ta * (r1 - r0), w_node and ta_zero, wflags + aflags, m, ta_zero


@pytest.mark.parametrize("name", sorted(R_TABLES))
def test_reflectivity_table_lookup_against_the_exact_bilinear_value(name):
    table, w, ang_deg, grid = r_axes(name)
    ang_rad = ang_deg * RAD_PER_DEG                      # the axis the referee and the kernel bracket on
    deg_queries = queries(ang_deg.tolist(), extra=(0.0, 90.0))
    wl_queries = queries(w.tolist())
    worst = 0.0
    for deg in deg_queries:
        rad = deg * RAD_PER_DEG
        for wl in wl_queries:
            got = O.coat_table_r(w, ang_deg, grid, wl, rad)
            want, at_node, flags, m, ta_zero = exact_bilinear(w, ang_rad, grid, wl, rad)
            if at_node or np.all(grid == grid.flat[0]):
                assert F(got) == want, (name, wl, deg, got, float(want))
            ok, ulps = within(got, want, flags, m, steps=2)
            assert ok, (name, wl, deg, got, float(want), ulps)
            worst = max(worst, ulps)
            # the host brackets the degree axis: bit-equal to the referee wherever the angle step does not
            # interpolate (one angle, a breakpoint, beyond either end), within its own bound elsewhere
            host = table.at(wl, deg)
            hwant, _, hflags, hm, hzero = exact_bilinear(w, ang_deg, grid, wl, deg)
            if hzero and ta_zero:
                assert host == got, (name, wl, deg, host, got)
            ok, _ = within(host, hwant, hflags, hm, steps=2)
            assert ok, (name, wl, deg, host, float(hwant))
    assert worst <= 1.5   # (measured 1.28 u M; the proven bound is 6-12 u M)


def test_the_angle_axis_is_converted_like_the_packer():
    """The referee's angle breakpoints are deg * (pi / 180) rounded once: a query one ulp below the converted 45
    degrees lies in the cell below, the converted value itself on the breakpoint."""
    w, a, v = np.array([500.0]), np.array([0.0, 45.0, 90.0]), np.array([[0.0], [0.5], [1.0]])
    at45 = 45.0 * RAD_PER_DEG
    assert O.coat_table_r(w, a, v, 500.0, at45) == 0.5
    assert O.coat_table_r(w, a, v, 500.0, float(np.nextafter(at45, 0.0))) < 0.5
    assert O.coat_table_r(w, a, v, 500.0, up(at45)) > 0.5
    assert O.coat_table_r(w, a, v, 500.0, math.acos(0.0)) == 1.0          # grazing: pvt_acos(0) is the converted 90
    assert O.coat_table_r(w, a, v, 500.0, 0.0) == 0.0


def test_wavelength_and_angle_are_not_swapped():
    """A table whose rows differ by angle and whose columns differ by wavelength: each axis moves its own way."""
    w, a = np.array([400.0, 800.0]), np.array([0.0, 90.0])
    v = np.array([[0.0, 0.2], [0.6, 1.0]])            # rows: angle 0, 90; columns: 400, 800 nm
    assert O.coat_table_r(w, a, v, 600.0, 0.0) == 0.1
    assert O.coat_table_r(w, a, v, 400.0, 45.0 * RAD_PER_DEG) == 0.3
    assert O.coat_table_r(w, a, v, 800.0, 90.0 * RAD_PER_DEG) == 1.0
