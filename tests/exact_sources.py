"""References of the tabulated sources of device emission -- position grids (PVT_POS_GRID) and direction tables
(PVT_DIR_TABLE), include/pvtrace_hip.h "tabulated sources" -- the case table and the planted faults
(tests/test_tabulated_sources.py, tests/test_gpu_tabulated_sources.py).

Nothing of the product is imported here.  A case is a plain `SourceTables` object with the fields of PvtEmitterTables
and PvtSourceTables, which the device accepts as it stands.  tests/exact_emission.py supplies the stream, the emission
key, the poses and the running error analysis `Bound`; `oracle.oracle.math` the portable sincos2pi.

`kernel_emit` -- the two rules in their OWN float64 operations, one per line, in the contract's order: the light
gi mod n_lights; the wavelength draw of a spectrum light; then the grid's cell draw u_c, the bisection
cdf[m] <= u ? a = m : b = m, the slot (ix ny + iy) nz + iz taken apart, and one draw per bounded axis x, y, z with
lower + ((double)i + u) * h; then the table's u1 (drawn whenever it has several rows, not read: the first row is
used), u2 through the bisection and mu_j + (u2 - C_j) / (C_j+1 - C_j) (mu_j+1 - mu_j), clamped, sqrt((1 - mu)(1 + mu)),
sincos2pi(u3) and the basis of Duff et al. about (0, 0, 1); the pose ((m0 x + m1 y) + m2 z) + m3.  float64 operations
are deterministic: the kernel must equal this for EVERY ray, no tolerance.

`exact_emit` -- the same law on the exact values of the doubles: the cell and the segment picked on
`fractions.Fraction` by a linear scan (the first cell with C_k+1 > u), the cell coordinate and the cosine in rationals,
the root and the circular functions of the exact 2 pi u3 in mpmath at 60 digits.  Every comparison is between stored
doubles, so no ray is ambiguous.

The bounds (U = 2^-53, through `Bound`, the way tests/exact_emission.py derives its own)
 1. coordinate: i + u is one rounding of exact operands (i an integer, u a draw), the product with the double h one,
    the sum with the double lower one: three roundings, through `Bound`.  h is DATA (the contract stores RN((upper -
    lower) / n)), so the exact rule uses the stored double.  An unbounded axis is exactly 0.
 2. cosine: two differences, a quotient, a product and a sum of stored doubles through `Bound`; the clamp projects onto
    an interval that holds the exact value.
 3. its partner sqrt((1 - mu)(1 + mu)): `Bound` through the two sums, the product and the root -- the term
    U / sqrt(1 - mu^2) near |mu| = 1.
 4. direction about (0, 0, 1): s = 1, a = -1/2, b = -0, e1 = (1, -0, -0), e2 = (-0, 1, -0) are exact, the products with
    them and with d = (0, 0, 1) are exact, so x = st cos, y = st sin (one rounding each, sincos2pi < 1 ulp of the exact
    draw's value) and z = mu.
 5. pose: as tests/exact_emission.py, item 6.
The HOST sampler (`emit._sample_light`) forms the same cosine and partner, then cos and sin of phi = RN(RN(2 pi) u3)
with numpy (H_ULP = 4 ulp), and may apply the pose in any order or fused: `host_bounds` gives the order-free first-order
bound sum |m_i| e_i + 4 U (sum |m_i x_i| + |m_3|).

The planted faults (`FAULTS`) are switches of `kernel_emit`.
"""
import math
from fractions import Fraction as F

import mpmath
import numpy as np
from mpmath import mp, mpf

from oracle.oracle import math as portable
from tests.exact_emission import Bound, Tables, emit_key, pose, stream

DIGITS = 60
U = 2.0 ** -53
H_ULP = 4.0
SLACK = 1e-30
TWO_PI_D = 2.0 * 3.14159265358979323846
WL_CONSTANT, WL_SPECTRUM = 0, 1
POS_POINT, POS_RECT, POS_GRID = 0, 1, 4
DIR_Z, DIR_TABLE = 0, 5
ONE = Bound(1.0)
FAULTS = ("cell-bisect-lt", "slot-transposed", "axis-draws-zyx", "h-by-reciprocal", "u1-not-drawn", "row-not-first")
N_RAYS = 4096 + 37


# ------------------------------------------------------------------------------------------------ the tables
def running_cdf(weights):
    """Rule 1, one operation per line: C_0 = 0, the running sum in slot order divided by the total, the last entry 1."""
    flat = [float(v) for v in np.asarray(weights, dtype=np.float64).reshape(-1)]
    sums, acc = [], 0.0
    for w in flat:
        acc = acc + w
        sums.append(acc)
    cdf = [0.0] + [s / acc for s in sums]
    cdf[-1] = 1.0
    return cdf


def table_rows(angle, values, wavelength=None):
    """(wavelengths, mu, CDF rows) of a phase table p(theta) by item 1 of the PvtPhaseTables contract: data for the cases
    (the rules under test take the CDF as it is stored)."""
    ang = np.asarray(angle, dtype=np.float64)
    rows = np.atleast_2d(np.asarray(values, dtype=np.float64))
    mu = np.cos(np.radians(ang))[::-1].copy()
    mu[0], mu[-1] = -1.0, 1.0
    p = rows[:, ::-1]
    cdf = np.cumsum(0.5 * (p[:, :-1] + p[:, 1:]) * np.diff(mu)[None, :], axis=1)
    cdf = np.hstack([np.zeros((rows.shape[0], 1)), cdf / cdf[:, -1:]])
    cdf[:, -1] = 1.0
    wl = np.zeros(1) if wavelength is None else np.asarray(wavelength, dtype=np.float64)
    return wl, mu, cdf


class SourceTables(Tables):
    """`Tables` plus the fields of PvtSourceTables.  A light dict may carry grid=dict(shape, lower, upper, cdf | weights)
    (lower / upper None on an axis without bounds) and table=(wavelengths, mu, cdf rows); equal objects are pooled once."""

    def __init__(self, lights):
        plain = []
        for light in lights:
            light = dict(light)
            if "grid" in light:
                light["pos"] = (POS_GRID, (0.0, 0.0, 0.0))
            if "table" in light:
                light["dir"] = (DIR_TABLE, 0.0)
            plain.append(light)
        super().__init__(plain)
        n = len(lights)
        self.light_grid = np.full(n, -1, dtype=np.int32)
        self.light_table = np.full(n, -1, dtype=np.int32)
        grids, tables = [], []
        for i, light in enumerate(lights):
            for key, pool, index in (("grid", grids, self.light_grid), ("table", tables, self.light_table)):
                if key in light:
                    at = next((k for k, have in enumerate(pool) if have is light[key]), None)
                    if at is None:
                        at = len(pool)
                        pool.append(light[key])
                    index[i] = at
        self.n_grids, self.n_tables = len(grids), len(tables)
        self.grid_shape = np.array([g["shape"] for g in grids], dtype=np.int32).reshape(-1, 3)
        self.grid_bounded = np.array([[lo is not None for lo in g["lower"]] for g in grids], dtype=np.int32).reshape(-1, 3)
        self.grid_lower = np.array([[0.0 if lo is None else lo for lo in g["lower"]] for g in grids], dtype=np.float64).reshape(-1, 3)
        self.grid_upper = np.array([[0.0 if hi is None else hi for hi in g["upper"]] for g in grids], dtype=np.float64).reshape(-1, 3)
        self.grid_h = np.ones((len(grids), 3))
        cdfs = []
        for k, g in enumerate(grids):
            for a in range(3):
                if self.grid_bounded[k, a]:
                    width = float(self.grid_upper[k, a]) - float(self.grid_lower[k, a])
                    self.grid_h[k, a] = width / float(self.grid_shape[k, a])      # one division, as Lattice.h has it
            cdf = g["cdf"] if "cdf" in g else running_cdf(g["weights"])
            assert len(cdf) == int(np.prod(g["shape"])) + 1
            cdfs.append(np.array(cdf, dtype=np.float64))
        self.grid_cdf_start = _starts([c.size for c in cdfs])
        self.grid_cdf = np.concatenate(cdfs) if cdfs else np.zeros(0)
        self.table_nw = np.array([t[2].shape[0] for t in tables], dtype=np.int32)
        self.table_nmu = np.array([t[1].size for t in tables], dtype=np.int32)
        self.table_wl_start = _starts([t[0].size for t in tables])
        self.table_mu_start = _starts([t[1].size for t in tables])
        self.table_cdf_start = _starts([t[2].size for t in tables])
        self.table_wavelength = np.concatenate([t[0] for t in tables]) if tables else np.zeros(0)
        self.table_mu = np.concatenate([t[1] for t in tables]) if tables else np.zeros(0)
        self.table_cdf = np.concatenate([t[2].reshape(-1) for t in tables]) if tables else np.zeros(0)


def _starts(sizes):
    return np.concatenate(([0], np.cumsum(sizes)[:-1])).astype(np.int32) if len(sizes) else np.zeros(0, dtype=np.int32)


_LISTS = {}


def _grid(tab, li):
    """(shape, bounded, lower, h, upper, cdf) of light li's grid as Python numbers; `tab`: any object with the fields."""
    g = int(tab.light_grid[li])
    key = (id(tab), "g", g)
    if key not in _LISTS:
        shape = [int(v) for v in np.asarray(tab.grid_shape).reshape(-1, 3)[g]]
        s = int(tab.grid_cdf_start[g])
        upper = getattr(tab, "grid_upper", None)
        _LISTS[key] = (tab, shape, [int(v) for v in np.asarray(tab.grid_bounded).reshape(-1, 3)[g]],
                       [float(v) for v in np.asarray(tab.grid_lower).reshape(-1, 3)[g]],
                       [float(v) for v in np.asarray(tab.grid_h).reshape(-1, 3)[g]],
                       None if upper is None else [float(v) for v in np.asarray(upper).reshape(-1, 3)[g]],
                       [float(v) for v in np.asarray(tab.grid_cdf)[s:s + shape[0] * shape[1] * shape[2] + 1]])
    return _LISTS[key][1:]


def _table(tab, li):
    """(nw, mu, cdf rows) of light li's table as Python numbers."""
    t = int(tab.light_table[li])
    key = (id(tab), "t", t)
    if key not in _LISTS:
        nw, nm = int(tab.table_nw[t]), int(tab.table_nmu[t])
        m0, c0 = int(tab.table_mu_start[t]), int(tab.table_cdf_start[t])
        mu = [float(v) for v in np.asarray(tab.table_mu)[m0:m0 + nm]]
        rows = [[float(v) for v in np.asarray(tab.table_cdf)[c0 + r * nm:c0 + (r + 1) * nm]] for r in range(nw)]
        _LISTS[key] = (tab, nw, mu, rows)
    return _LISTS[key][1:]


def _spectrum(tab, li):
    s, n = int(tab.wl_spec_start[li]), int(tab.wl_spec_n[li])
    return [float(v) for v in tab.spec_x[s:s + n]], [float(v) for v in tab.spec_cdf[s:s + n]]


def _p(fn, x):
    return float(portable(fn, np.array([x]))[0])


# ------------------------------------------------------------------------------------------------ the kernel's rule
def _interp(xs, ys, x):
    """The spectrum light's wavelength (PVT_WL_SPECTRUM), as tests/exact_emission.py restates it."""
    n = len(xs)
    if n == 1 or x <= xs[0]:
        return ys[0]
    if x >= xs[n - 1]:
        return ys[n - 1]
    lo, hi = 0, n - 1
    while hi - lo > 1:
        mid = (lo + hi) >> 1
        if xs[mid] <= x:
            lo = mid
        else:
            hi = mid
    if xs[hi] == xs[lo]:
        return ys[lo]
    dy = ys[hi] - ys[lo]
    dx = x - xs[lo]
    w = xs[hi] - xs[lo]
    p = dy * dx
    t = p / w
    return ys[lo] + t


def grid_position(grid, u, fault=None):
    """Rules 2 and 3 on the draws u[0], u[1] ... -> ((x, y, z), draws taken, slot)."""
    shape, bounded, lower, h, upper, cdf = grid
    nx, ny, nz = shape
    uc = u[0]
    k = 1
    a, b = 0, nx * ny * nz
    while b - a > 1:
        m = (a + b) >> 1
        if (cdf[m] < uc) if fault == "cell-bisect-lt" else (cdf[m] <= uc):
            a = m
        else:
            b = m
    if fault == "slot-transposed":      # the slot read as (iz ny + iy) nx + ix
        ix = a % nx
        rest = a // nx
        iy = rest % ny
        iz = rest // ny
    else:
        iz = a % nz
        rest = a // nz
        iy = rest % ny
        ix = rest // ny
    index = (ix, iy, iz)
    p = [0.0, 0.0, 0.0]
    for axis in ((2, 1, 0) if fault == "axis-draws-zyx" else (0, 1, 2)):
        if bounded[axis]:
            ua = u[k]
            k += 1
            width = h[axis]
            if fault == "h-by-reciprocal":
                span = upper[axis] - lower[axis]
                inverse = 1.0 / float(shape[axis])
                width = span * inverse
            t = float(index[axis]) + ua
            t = t * width
            p[axis] = lower[axis] + t
    return p, k, a


def table_direction(table, u, fault=None):
    """The table's turn about (0, 0, 1) on the draws u[0] ... -> ((x, y, z), draws taken, segment)."""
    nw, mus, rows = table
    nm = len(mus)
    k = 0
    if nw > 1 and fault != "u1-not-drawn":
        k += 1                                    # u1: drawn, not read -- the first row is used
    cdf = rows[1 if (fault == "row-not-first" and nw > 1) else 0]
    u2 = u[k]
    u3 = u[k + 1]
    k += 2
    a, b = 0, nm - 1
    while b - a > 1:
        m = (a + b) >> 1
        if cdf[m] <= u2:
            a = m
        else:
            b = m
    ca = cdf[a]
    ma = mus[a]
    t1 = u2 - ca
    t2 = cdf[b] - ca
    t3 = t1 / t2
    t4 = mus[b] - ma
    t5 = t3 * t4
    mu = ma + t5
    mu = min(max(mu, -1.0), 1.0)
    w1 = 1.0 - mu
    w2 = 1.0 + mu
    w = w1 * w2
    st = math.sqrt(w)
    sp = _p("sin2pi", u3)
    cp = _p("cos2pi", u3)
    dx, dy, dz = 0.0, 0.0, 1.0
    s = math.copysign(1.0, dz)
    ra = -1.0 / (s + dz)
    rb = dx * dy * ra
    e1 = (1.0 + s * dx * dx * ra, s * rb, -s * dx)
    e2 = (rb, s + dy * dy * ra, -dy)
    out = []
    for c, d in enumerate((dx, dy, dz)):
        along = mu * d
        t6 = cp * e1[c]
        t7 = sp * e2[c]
        across = t6 + t7
        across = st * across
        out.append(along + across)
    return out, k, a


def kernel_emit(tab, emit_seed, gi, fault=None):
    """`emit_one` for global ray gi of an emitter whose lights are points or rectangles along +z (the built-ins the cases
    use), grids and tables -> (pos, dir, wl, draws taken, info)."""
    u = stream(emit_key(emit_seed, gi), 10)
    k = 0
    li = gi % tab.n_lights
    info = {"light": li, "slot": -1, "segment": -1}
    if int(tab.wl_type[li]) == WL_SPECTRUM:
        x, cdf = _spectrum(tab, li)
        wl = _interp(cdf, x, u[k])
        k += 1
    else:
        assert int(tab.wl_type[li]) == WL_CONSTANT
        wl = float(tab.wl_value[li])
    lp = [0.0, 0.0, 0.0]
    pt = int(tab.pos_type[li])
    if pt == POS_RECT:
        pp = [float(v) for v in tab.pos_param[li]]
        for a in range(2):
            twice = 2.0 * pp[a]
            span = twice * u[k]
            k += 1
            lp[a] = -pp[a] + span
    elif pt == POS_GRID:
        lp, taken, info["slot"] = grid_position(_grid(tab, li), u[k:], fault)
        k += taken
    else:
        assert pt == POS_POINT
    ld = [0.0, 0.0, 1.0]
    dt = int(tab.dir_type[li])
    if dt == DIR_TABLE:
        ld, taken, info["segment"] = table_direction(_table(tab, li), u[k:], fault)
        k += taken
    else:
        assert dt == DIR_Z
    m = [[float(v) for v in row] for row in tab.light_to_world[li]]
    pos, direction = [], []
    for r in range(3):
        t0 = m[r][0] * lp[0]
        t1 = m[r][1] * lp[1]
        t2 = m[r][2] * lp[2]
        acc = t0 + t1
        acc = acc + t2
        pos.append(acc + m[r][3])
        t0 = m[r][0] * ld[0]
        t1 = m[r][1] * ld[1]
        t2 = m[r][2] * ld[2]
        acc = t0 + t1
        direction.append(acc + t2)
    info["local_pos"], info["local_dir"] = lp, ld
    return pos, direction, wl, k, info


def kernel_bundle(tab, n, emit_seed, ray_offset=0, fault=None):
    """`kernel_emit` of rays ray_offset .. ray_offset + n - 1 -> (pos (n, 3), dir (n, 3), wl (n), draws (n), infos)."""
    rows = [kernel_emit(tab, emit_seed, ray_offset + i, fault) for i in range(n)]
    return (np.array([r[0] for r in rows]), np.array([r[1] for r in rows]), np.array([r[2] for r in rows]),
            np.array([r[3] for r in rows]), [r[4] for r in rows])


# ------------------------------------------------------------------------------------------------ the exact rule
_FRACTIONS = {}


def _fractions(values):
    key = id(values)
    if key not in _FRACTIONS:
        _FRACTIONS[key] = (values, [F(v) for v in values])
    return _FRACTIONS[key][1]


def _first_above(cq, uq):
    """The first k with C_k+1 > u, by Python's own search on rationals (a non-decreasing list)."""
    import bisect
    return bisect.bisect_right(cq, uq) - 1


def _mp(q):
    return mpf(q.numerator) / mpf(q.denominator) if isinstance(q, F) else mpf(q)


def exact_grid_position(grid, u):
    """Rules 2 and 3 on exact values -> (exact local position as Fractions, `Bound`s of the computed coordinates, draws
    taken, slot)."""
    shape, bounded, lower, h, _, cdf = grid
    cq = _fractions(cdf)
    slot = _first_above(cq, F(u[0]))
    assert cq[slot] <= F(u[0]) < cq[slot + 1]
    iz = slot % shape[2]
    iy = (slot // shape[2]) % shape[1]
    ix = slot // (shape[2] * shape[1])
    k = 1
    lp, bp = [F(0)] * 3, [Bound(0.0) for _ in range(3)]
    for a, i in enumerate((ix, iy, iz)):
        if bounded[a]:
            lp[a] = F(lower[a]) + (i + F(u[k])) * F(h[a])
            b = Bound(lower[a]) + (Bound(float(i)) + Bound(u[k])) * Bound(h[a])
            bp[a] = Bound(float(lp[a]), b.e)
            k += 1
    return lp, bp, k, slot


def _cosine_bound(table, u2, j):
    """Item 2: the cosine's operations on segment j of the first row, through `Bound`."""
    _, mus, rows = table
    cdf = rows[0]
    t = (Bound(u2) - Bound(cdf[j])) / (Bound(cdf[j + 1]) - Bound(cdf[j]))
    return (Bound(mus[j]) + t * (Bound(mus[j + 1]) - Bound(mus[j]))).clamped()


def exact_table_direction(table, u, host=False):
    """The turn about (0, 0, 1) on exact values -> (exact (x, y, z) as mpf, bounds (ex, ey, ez), draws taken, segment).
    host: the bound for the host sampler's circular functions (numpy's cos and sin of RN(RN(2 pi) u3))."""
    nw, mus, rows = table
    k = 1 if nw > 1 else 0
    u2, u3 = u[k], u[k + 1]
    k += 2
    cq, mq = _fractions(rows[0]), _fractions(mus)
    j = _first_above(cq, F(u2))
    assert cq[j] <= F(u2) < cq[j + 1]
    mu_q = mq[j] + (F(u2) - cq[j]) / (cq[j + 1] - cq[j]) * (mq[j + 1] - mq[j])
    assert -1 <= mu_q <= 1
    with mpmath.workdps(DIGITS):
        mu = _mp(mu_q)
        st = mpmath.sqrt((1 - mu) * (1 + mu))
        phi = 2 * mp.pi * _mp(F(u3))
        cp, sp = mpmath.cos(phi), mpmath.sin(phi)
        bmu = _cosine_bound(table, u2, j)
        bmu.x = float(mu)
        bst = ((ONE - bmu) * (ONE + bmu)).sqrt()
        bst.x = float(st)
        if host:
            ang = Bound(TWO_PI_D, abs(float(mpf(TWO_PI_D) - 2 * mp.pi))) * Bound(u3)
            bc, bs = ang.function(float(cp), H_ULP), ang.function(float(sp), H_ULP)
        else:
            bc = Bound(u3).function(float(cp), 1.0, lipschitz=0.0)
            bs = Bound(u3).function(float(sp), 1.0, lipschitz=0.0)
        bx, by = bst * bc, bst * bs
        exact = (st * cp, st * sp, mu)
        slack = [SLACK + 1e-25 * abs(float(v)) for v in exact]
        return exact, (bx.e + slack[0], by.e + slack[1], bmu.e + slack[2]), k, j


def exact_emit(tab, emit_seed, gi, host=False):
    """The law of `kernel_emit` on exact values -> dict(pos, dir: mpf triples, wl, e_pos, e_dir, e_wl, draws, light, slot,
    segment, local_pos, local_dir).  host: the bounds of the host sampler (module docstring)."""
    u = stream(emit_key(emit_seed, gi), 10)
    k = 0
    li = gi % tab.n_lights
    out = {"light": li, "slot": -1, "segment": -1, "e_wl": 0.0}
    with mpmath.workdps(DIGITS):
        if int(tab.wl_type[li]) == WL_SPECTRUM:
            x, cdf = _spectrum(tab, li)
            xq, cq, uq = [F(v) for v in x], [F(v) for v in cdf], F(u[k])
            k += 1
            assert cq[0] < uq < cq[-1]
            lo = _first_above(cq, uq)
            tq = (uq - cq[lo]) / (cq[lo + 1] - cq[lo])
            out["wl"] = xq[lo] + tq * (xq[lo + 1] - xq[lo])
            step = abs(float(tq * (xq[lo + 1] - xq[lo])))
            out["e_wl"] = 0.0 if tq == 0 else (5.0 * U * step + U * abs(float(out["wl"]))) * (1.0 + 1e-9)
        else:
            out["wl"] = F(float(tab.wl_value[li]))
        lp, bp = [F(0)] * 3, [Bound(0.0) for _ in range(3)]
        pt = int(tab.pos_type[li])
        if pt == POS_RECT:
            pp = [float(v) for v in tab.pos_param[li]]
            for a in range(2):
                lp[a] = -F(pp[a]) + 2 * F(pp[a]) * F(u[k])
                b = Bound(-pp[a]) + Bound(2.0 * pp[a]) * Bound(u[k])
                bp[a] = Bound(float(lp[a]), b.e)
                k += 1
        elif pt == POS_GRID:
            lp, bp, taken, out["slot"] = exact_grid_position(_grid(tab, li), u[k:])
            k += taken
        lp = [_mp(v) for v in lp]
        ld, bd = [mpf(0), mpf(0), mpf(1)], [Bound(0.0), Bound(0.0), Bound(1.0)]
        if int(tab.dir_type[li]) == DIR_TABLE:
            ld, ed, taken, out["segment"] = exact_table_direction(_table(tab, li), u[k:], host)
            bd = [Bound(float(v), e) for v, e in zip(ld, ed)]
            k += taken
        m = tab.light_to_world[li]
        pos, direction, e_pos, e_dir = [], [], [], []
        for r in range(3):
            row = [float(v) for v in m[r]]
            pos.append(sum(_mp(F(row[a])) * lp[a] for a in range(3)) + _mp(F(row[3])))
            direction.append(sum(_mp(F(row[a])) * ld[a] for a in range(3)))
            if host:      # any order, fused or not: first order, four roundings of the largest partial sums
                size = sum(abs(row[a] * float(lp[a])) for a in range(3)) + abs(row[3])
                e_pos.append((sum(abs(row[a]) * bp[a].e for a in range(3)) + 4.0 * U * size) * (1.0 + 1e-9) + SLACK)
                size = sum(abs(row[a] * float(ld[a])) for a in range(3))
                e_dir.append((sum(abs(row[a]) * bd[a].e for a in range(3)) + 4.0 * U * size) * (1.0 + 1e-9) + SLACK)
            else:
                b = ((Bound(row[0]) * bp[0] + Bound(row[1]) * bp[1]) + Bound(row[2]) * bp[2]) + Bound(row[3])
                e_pos.append(b.e + SLACK + 1e-25 * abs(b.x))
                b = (Bound(row[0]) * bd[0] + Bound(row[1]) * bd[1]) + Bound(row[2]) * bd[2]
                e_dir.append(b.e + SLACK + 1e-25 * abs(b.x))
        out.update(pos=pos, dir=direction, e_pos=e_pos, e_dir=e_dir, draws=k, local_pos=lp, local_dir=ld,
                   e_local_pos=[b.e + SLACK for b in bp], e_local_dir=[b.e + SLACK for b in bd])
    return out


def worst_ratio(refs, pos, dirs, wl):
    """max |value - exact| / bound over every component of every ray (a zero bound demands equality)."""
    worst = 0.0
    with mpmath.workdps(DIGITS):
        for i, ref in enumerate(refs):
            pairs = [(pos[i][a], ref["pos"][a], ref["e_pos"][a]) for a in range(3)]
            pairs += [(dirs[i][a], ref["dir"][a], ref["e_dir"][a]) for a in range(3)]
            pairs.append((wl[i], _mp(ref["wl"]), ref["e_wl"]))
            for got, want, bound in pairs:
                if not math.isfinite(got):
                    return math.inf
                err = abs(float(_mp(F(float(got))) - want))
                if err > 0.0:
                    worst = max(worst, err / bound if bound > 0.0 else math.inf)
    return worst


# ------------------------------------------------------------------------------------------------ the cases
class Case:
    def __init__(self, name, lights, n=N_RAYS, emit_seed=2026, ray_offset=1000):
        self.name, self.lights, self.n, self.emit_seed, self.ray_offset = name, lights, n, emit_seed, ray_offset
        self._tables = self._kernel = self._exact = None

    def __repr__(self):
        return self.name

    @property
    def tables(self):
        if self._tables is None:
            self._tables = SourceTables(self.lights(self) if callable(self.lights) else self.lights)
        return self._tables

    def kernel(self):
        """`kernel_bundle` of the case, computed once and left unchanged."""
        if self._kernel is None:
            self._kernel = kernel_bundle(self.tables, self.n, self.emit_seed, self.ray_offset)
            for a in self._kernel[:4]:
                a.setflags(write=False)
        return self._kernel

    def exact(self):
        if self._exact is None:
            self._exact = [exact_emit(self.tables, self.emit_seed, self.ray_offset + i) for i in range(self.n)]
        return self._exact


POSE = pose()
POSE2 = pose(parent=(2.3, (-0.2, 0.5, 1.0)), turn=(0.4, (0.1, 0.9, 0.3)), shift=(-4.0, 0.5, 0.125))


def _light(**kw):
    kw.setdefault("pose", POSE)
    return kw


def _tied_3x3(case):
    # zero cells at the first, a middle and the last slot; the knots are cell draws of the case's own rays, so those rays
    # sit ON a knot -- one of them on the tie -- and the `<=` of the bisection decides their cell
    draws = sorted(stream(emit_key(case.emit_seed, case.ray_offset + i), 1)[0] for i in range(0, case.n, case.n // 40))
    k = [draws[5], draws[12], draws[20], draws[28], draws[35]]
    cdf = [0.0, 0.0, k[0], k[1], k[1], k[2], k[3], k[4], 1.0, 1.0]
    return [_light(grid=dict(shape=(3, 3, 1), lower=(-1.5, 0.25, None), upper=(0.75, 2.0, None), cdf=cdf))]


def _image(n=64):
    rng = np.random.default_rng(5)
    img = rng.uniform(0.0, 1.0, (n, n)) ** 2
    img[: n // 2, : n // 4] = 0.0       # a shaded corner
    return img.reshape(n, n, 1)


LED = table_rows(np.linspace(0.0, 180.0, 37), np.where(np.linspace(0.0, 180.0, 37) < 90.0,
                                                       np.cos(np.radians(np.linspace(0.0, 180.0, 37))) ** 3, 0.0))
TWO_ANGLES = table_rows([0.0, 180.0], [1.0, 0.25])
ZERO_MASS = table_rows([0.0, 20.0, 40.0, 60.0, 90.0, 120.0, 180.0], [1.0, 0.8, 0.0, 0.0, 0.5, 0.0, 0.0])
_A3 = np.linspace(0.0, 180.0, 19)
THREE_ROWS = table_rows(_A3, [np.exp(-0.5 * (_A3 / 15.0) ** 2), np.exp(-0.5 * (_A3 / 40.0) ** 2), 1.0 + 0.0 * _A3],
                        wavelength=[450.0, 550.0, 700.0])
# (the z width is one whose third differs from its product with RN(1 / 3): the h-by-reciprocal fault shows there)
GRID_423 = dict(shape=(4, 2, 3), lower=(-1.0, 0.5, 0.05), upper=(1.8, 1.2, 0.6),
                weights=np.random.default_rng(9).uniform(0.0, 1.0, (4, 2, 3)))
GRID_211 = dict(shape=(2, 1, 1), lower=(-0.5, None, None), upper=(2.5, None, None), weights=[0.0, 3.0])
ROUND_ROBIN = [
    _light(wl=(WL_CONSTANT, 632.8), pos=(POS_RECT, (0.5, 1.5, 0.0))),
    _light(wl=(WL_SPECTRUM, ([400.0, 500.0, 650.0], [0.0, 0.3, 1.0])), grid=GRID_423, pose=POSE2),
    _light(grid=dict(shape=(5, 3, 1), lower=(-2.0, -1.0, None), upper=(2.0, 1.0, None),
                     weights=np.random.default_rng(2).integers(0, 4, (5, 3, 1))), table=THREE_ROWS),
]
CASES = [
    Case("G-1x1x1", [_light(grid=dict(shape=(1, 1, 1), lower=(-0.5, -1.5, 0.25), upper=(0.5, 1.5, 0.75), weights=[7.0]))]),
    Case("G-2x1x1-zero-cell", [_light(grid=GRID_211)]),
    Case("G-3x3x1-ties", _tied_3x3),
    Case("G-4x2x3", [_light(grid=GRID_423)]),
    Case("G-64x64-image", [_light(grid=dict(shape=(64, 64, 1), lower=(-2.5, -2.5, None), upper=(2.5, 2.5, None),
                                           weights=_image()))]),
    Case("T-two-angles", [_light(table=TWO_ANGLES)]),
    Case("T-zero-mass", [_light(table=ZERO_MASS)]),
    Case("T-three-rows", [_light(table=THREE_ROWS)]),
    Case("R-three-lights", ROUND_ROBIN),
]
BY_NAME = {c.name: c for c in CASES}
